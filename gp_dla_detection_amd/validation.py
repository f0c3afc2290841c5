"""How well the finder finds absorbers: a processed run scored against a truth table.

    python -m gp_dla_detection_amd.validation --processed processed_qsos.mat --truth mock_truth.mat \\
        [--catalog catalog.mat]

prints one JSON object.  Host code; it restates the scoring methods of the reference's
``QSOLoader`` (CDDF_analysis/qso_loader.py) on the variables a processed file holds:

=================================  ==============================================================
reference                          here
=================================  ==============================================================
``make_ROC`` (:663-717)            :func:`roc`
``make_MAP_comparison`` (:719-745) :func:`map_comparison`
``query_least_num_dlas`` (:838-859) :func:`least_num_dlas`
``make_multi_confusion`` (:878-965) :func:`multi_confusion` (truth counts from a truth table instead
                                   of Parks' catalogue; the same ``p_thresh``, ``min_log_nhi`` and
                                   Ly-beta cuts)
=================================  ==============================================================

plus :func:`completeness_by_log_nhi`, which has no counterpart there.  ``results`` is everywhere the
dict :func:`gp_dla_detection_amd.io.load_processed_qsos` or a ``process_qsos*`` call returns; a truth
table is the CSR triple ``(offsets [nq + 1], z_dlas, log_nhis)`` of :func:`gp_dla_detection_amd.mocks.draw_truth`,
one list per quasar of ``results``.
"""
from __future__ import annotations

import argparse
import json

import numpy as np

from .catalog import occams_model_posteriors
from .parameters import Parameters


def _logsumexp(rows) -> np.ndarray:
    """log Sum_j exp(rows[j]) along axis 0, shifted by the column maximum (what scipy's logsumexp does)."""
    a = np.asarray(rows, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(a, axis=0)
        m = np.where(np.isfinite(m), m, 0.0)
        return np.log(np.sum(np.exp(a - m), axis=0)) + m


def _has_sub_dla(results: dict, sub_dla) -> bool:
    return ("log_posteriors_lls" in results) if sub_dla is None else bool(sub_dla)


def log_odds(results: dict, sub_dla: bool | None = None, occams_razor: float = 10000.0) -> np.ndarray:
    """log [p(any DLA model | y) / p(no DLA | y)] per quasar as make_ROC forms it (:676-694): every
    absorber model's log posterior is lowered by ``log(occams_razor)``, the DLA(1..n) models are summed,
    and -- ``sub_dla`` (default: when the results carry ``log_posteriors_lls``) -- the sub-DLA model is
    folded into "no DLA"."""
    lp_dla = np.asarray(results["log_posteriors_dla"], dtype=np.float64)
    lp_dla = lp_dla.reshape(lp_dla.shape[0], -1).T - np.log(occams_razor)               # :676  [models, nq]
    lp_no = np.asarray(results["log_posteriors_no_dla"], dtype=np.float64).reshape(-1)  # :677
    if _has_sub_dla(results, sub_dla):
        lp_lls = np.asarray(results["log_posteriors_lls"], dtype=np.float64).reshape(-1) - np.log(occams_razor)  # :679
        lp_no = _logsumexp([lp_no, lp_lls])                                             # :682
    return _logsumexp(lp_dla) - lp_no                                                   # :684, :694


def roc(results: dict, real_index, real_index_los=None, sub_dla: bool | None = None,
        occams_razor: float = 10000.0):
    """``QSOLoader.make_ROC`` (:663-717).  ``real_index``: the quasars of ``results`` that truly hold a
    DLA; ``real_index_los``: the sightlines that are scored (default: all).  Sightlines are ranked by
    ascending :func:`log_odds`; point i of the curve thresholds at the i-th smallest with ``>=``
    (:707).  A sightline the sweep skipped (NaN odds) is left out, as the reference's NaN filter
    leaves it out (:687-688).  The reference counts in an O(N^2) loop; here one sort and two cumulative
    sums give the same integers, so the same ratios.  Returns ``(TPR, FPR)`` as arrays."""
    odds_all = log_odds(results, sub_dla, occams_razor)
    los = np.arange(odds_all.size) if real_index_los is None else np.asarray(real_index_los, dtype=np.int64).reshape(-1)
    has = np.isin(los, np.asarray(real_index, dtype=np.int64))                         # :667
    odds = odds_all[los]
    ok = ~np.isnan(odds)
    odds, has = odds[ok], has[ok]
    rank = np.argsort(odds, kind="stable")                                              # :696
    odds, has = odds[rank], has[rank]
    first = np.searchsorted(odds, odds, side="left")       # entries [first[i], N) are >= odds[i]
    cum = np.concatenate([[0], np.cumsum(has)])
    n, npos = odds.size, int(cum[-1])
    tp = npos - cum[first]                                 # true positives at threshold i
    fp = (n - first) - tp
    with np.errstate(invalid="ignore", divide="ignore"):
        return tp / np.float64(npos), fp / np.float64(n - npos)                         # :714-715


def map_model_index(results: dict, occams_razor: float = 10000.0) -> np.ndarray:
    """``dla_map_model_index`` (:143): the column of the Occam-penalised ``model_posteriors`` that wins."""
    mp = occams_model_posteriors(results["model_posteriors"], occams_razor)
    return np.argmax(np.where(np.isnan(mp), -np.inf, mp), axis=1)


def map_comparison(results: dict, real_index, z_dlas, log_nhis, sub_dla: bool | None = None,
                   occams_razor: float = 10000.0):
    """``QSOLoader.make_MAP_comparison`` (:719-745): MAP minus true (z_DLA, log N_HI) of the DLA(1)
    model, over the truly absorbed quasars ``real_index`` (with their true ``z_dlas`` / ``log_nhis``)
    whose most probable model holds at least one DLA (:737).  Returns ``(Delta_z_dlas, Delta_log_nhis)``."""
    real_index = np.asarray(real_index, dtype=np.int64).reshape(-1)
    found = map_model_index(results, occams_razor)[real_index] > int(_has_sub_dla(results, sub_dla))  # :734-737
    idx = real_index[found]
    map_z = np.asarray(results["MAP_z_dlas"], dtype=np.float64)
    map_n = np.asarray(results["MAP_log_nhis"], dtype=np.float64)
    if map_z.ndim == 3:
        map_z, map_n = map_z[:, 0, 0], map_n[:, 0, 0]                                   # :739-740
    return (map_z[idx] - np.asarray(z_dlas, dtype=np.float64).reshape(-1)[found],       # :742
            map_n[idx] - np.asarray(log_nhis, dtype=np.float64).reshape(-1)[found])     # :743


def least_num_dlas(model_posteriors_row, p_thresh: float, sub_dla: bool = True) -> int:
    """``QSOLoader.query_least_num_dlas`` (:838-859): starting from the model with the most DLAs, the
    first whose posterior exceeds ``p_thresh``; each time one does not, the model is removed and the
    rest renormalised (``downward_model``, :832-836).  0 when none does."""
    post = np.asarray(model_posteriors_row, dtype=np.float64)
    tot = post.size - 1 - int(bool(sub_dla))                                            # :847
    for i in range(tot):
        if post[-1] > p_thresh:                                                         # :851-854
            return tot - i
        post = post[:-1] / np.sum(post[:-1])                                            # :836, :856
    return 0


def multi_confusion(results: dict, truth, z_qsos=None, sightlines=None, p_thresh: float = 0.98,
                    lyb: bool = False, min_log_nhi: float = 20.3, sub_dla: bool | None = None,
                    occams_razor: float = 10000.0, params: Parameters | None = None):
    """``QSOLoader.make_multi_confusion`` (:878-965) with a truth table in the place of Parks'
    catalogue.  For every quasar of ``sightlines`` (default: all of ``results``; the reference scores
    those that appear in the catalogue, :912) the found count is :func:`least_num_dlas` of its
    Occam-penalised posteriors, then -- if positive -- the number of MAP absorbers of that model with
    ``z_dla > min_z_dla`` and ``log_nhi > min_log_nhi`` (:945-948); the true count is the number of
    truth entries passing the same two cuts (:872-876; a truth table has no confidence to cut on).
    ``lyb``: ``min_z_dla = (1 + z_qso) lyb / lya - 1`` (:939-942; needs ``z_qsos``), else 0.  A true count
    beyond the matrix is entered in its last column (:959-960).
    Returns ``(confusion_matrix [found, true], counts [n, 3] = (quasar, found, true))``."""
    p = params or Parameters()
    sub = _has_sub_dla(results, sub_dla)
    mp = occams_model_posteriors(results["model_posteriors"], occams_razor)
    map_z = np.asarray(results["MAP_z_dlas"], dtype=np.float64)
    map_n = np.asarray(results["MAP_log_nhis"], dtype=np.float64)
    if map_z.ndim == 1:  # single-DLA results: one model, one slot
        map_z, map_n = map_z[:, None, None], map_n[:, None, None]
    off, tz, tn = (np.asarray(a) for a in truth)
    los = np.arange(mp.shape[0]) if sightlines is None else np.asarray(sightlines, dtype=np.int64).reshape(-1)
    size = mp.shape[1] - int(sub)                                                       # :922
    confusion = np.zeros((size, size))
    counts = np.zeros((los.size, 3), dtype=np.int64)
    for i, q in enumerate(los):
        min_z = (1 + float(np.asarray(z_qsos).reshape(-1)[q])) * p.lyb_wavelength / p.lya_wavelength - 1 if lyb else 0  # :939-942
        n = least_num_dlas(mp[q], p_thresh, sub)                                        # :945
        if n > 0:
            n = int(np.sum((map_z[q, n - 1, :] > min_z) * (map_n[q, n - 1, :] > min_log_nhi)))  # :947-948
        sl = slice(int(off[q]), int(off[q + 1]))
        m = int(np.sum((tz[sl] > min_z) * (tn[sl] > min_log_nhi)))                      # :872-876
        counts[i] = (q, n, m)
        confusion[n, min(m, size - 1)] += 1                                             # :959-961
    return confusion, counts


def completeness_by_log_nhi(results: dict, truth, edges, p_thresh: float = 0.5, max_dz: float | None = None,
                            sub_dla: bool | None = None, occams_razor: float = 10000.0):
    """Fraction of true absorbers that were found, per bin of true log N_HI.  A true absorber counts as
    found when its quasar's Occam-penalised ``p_dla`` (every DLA model, the sub-DLA model folded into
    "no DLA") exceeds ``p_thresh`` and -- ``max_dz`` -- some MAP absorber of the quasar's most
    probable DLA model lies within ``max_dz`` of it in redshift.  Returns ``dict(edges, found, total,
    completeness)``; an empty bin has NaN completeness."""
    sub = _has_sub_dla(results, sub_dla)
    mp = occams_model_posteriors(results["model_posteriors"], occams_razor)
    first = 1 + int(sub)
    p_dla = mp[:, first:].sum(axis=1)
    best = np.argmax(np.where(np.isnan(mp[:, first:]), -np.inf, mp[:, first:]), axis=1)  # most probable DLA(n)
    map_z = np.asarray(results["MAP_z_dlas"], dtype=np.float64)
    if map_z.ndim == 1:
        map_z = map_z[:, None, None]
    off, tz, tn = (np.asarray(a) for a in truth)
    edges = np.asarray(edges, dtype=np.float64)
    found, total = np.zeros(edges.size - 1, dtype=np.int64), np.zeros(edges.size - 1, dtype=np.int64)
    for q in range(mp.shape[0]):
        for j in range(int(off[q]), int(off[q + 1])):
            b = int(np.searchsorted(edges, tn[j], side="right")) - 1
            if b < 0 or b >= total.size:
                continue
            total[b] += 1
            hit = bool(p_dla[q] > p_thresh)
            if hit and max_dz is not None:
                with np.errstate(invalid="ignore"):
                    hit = bool(np.any(np.abs(map_z[q, best[q], :best[q] + 1] - tz[j]) <= max_dz))
            found[b] += int(hit)
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(edges=edges, found=found, total=total, completeness=found / total.astype(np.float64))


def score(results: dict, truth, z_qsos=None, edges=(20.0, 20.3, 20.6, 21.0, 21.5, 22.0, 23.0), p_thresh: float = 0.98,
          min_log_nhi: float = 20.3, occams_razor: float = 10000.0, lyb: bool = False) -> dict:
    """Everything above for one run, as plain Python numbers (what the command prints).  A quasar
    "truly holds a DLA" when its truth list has an entry with log N_HI >= ``min_log_nhi``; the MAP
    comparison takes the strongest entry of each such quasar."""
    off, tz, tn = (np.asarray(a) for a in truth)
    nq = off.size - 1
    strongest = np.full(nq, -1, dtype=np.int64)
    for q in range(nq):
        if off[q + 1] > off[q]:
            j = int(off[q]) + int(np.argmax(tn[off[q]:off[q + 1]]))
            if tn[j] >= min_log_nhi:
                strongest[q] = j
    real = np.flatnonzero(strongest >= 0)
    tpr, fpr = roc(results, real, None, occams_razor=occams_razor)
    dz, dn = map_comparison(results, real, tz[strongest[real]], tn[strongest[real]], occams_razor=occams_razor)
    conf, _ = multi_confusion(results, truth, z_qsos, p_thresh=p_thresh, lyb=lyb, min_log_nhi=min_log_nhi,
                              occams_razor=occams_razor)
    comp = completeness_by_log_nhi(results, truth, edges, occams_razor=occams_razor)
    clean = fpr == 0
    nan = lambda a: [None if np.isnan(x) else float(x) for x in np.asarray(a, dtype=np.float64).reshape(-1)]  # noqa: E731
    return dict(num_quasars=int(nq), num_with_dla=int(real.size), roc_tpr=nan(tpr), roc_fpr=nan(fpr),
                tpr_at_zero_fpr=float(np.max(tpr[clean])) if clean.any() else None,
                map_delta_z_dlas=nan(dz), map_delta_log_nhis=nan(dn), confusion_matrix=conf.tolist(),
                completeness=dict(edges=nan(comp["edges"]), found=comp["found"].tolist(), total=comp["total"].tolist(),
                                  completeness=nan(comp["completeness"])))


def main(argv=None) -> int:
    from . import io, mocks
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--processed", required=True, help="processed_qsos*.mat of the run (chunks recombined)")
    ap.add_argument("--truth", required=True, help="truth file written by gp_dla_detection_amd.mocks")
    ap.add_argument("--catalog", default=None, help="catalog.mat (z_qsos): needed for --lyb")
    ap.add_argument("--lyb", action="store_true", help="confusion matrix: count absorbers redward of the quasar's Ly-beta only")
    ap.add_argument("--p-thresh", type=float, default=0.98)
    ap.add_argument("--min-log-nhi", type=float, default=20.3)
    ap.add_argument("--occams-razor", type=float, default=10000.0)
    a = ap.parse_args(argv)
    results = io.load_processed_qsos(a.processed)
    off, tz, tn = mocks.load_truth(a.truth)
    if "test_ind" in results:  # the truth file covers the catalogue; the run covers its test_ind selection
        sel = np.flatnonzero(np.asarray(results["test_ind"]).reshape(-1).astype(bool))
        if sel.size == np.asarray(results["p_dlas"]).reshape(-1).size and off.size - 1 != sel.size:
            from .api import _take_absorbers
            off, tz, tn = _take_absorbers((off, tz, tn), sel)
    z_qsos = None
    if a.lyb and not a.catalog:
        ap.error("--lyb needs --catalog")
    if a.catalog:
        z = np.asarray(io.load_catalog(a.catalog, ("z_qsos",))["z_qsos"], dtype=np.float64)
        z_qsos = z[sel] if "test_ind" in results and z.size != off.size - 1 else z
    print(json.dumps(score(results, (off, tz, tn), z_qsos, p_thresh=a.p_thresh, min_log_nhi=a.min_log_nhi,
                           occams_razor=a.occams_razor, lyb=a.lyb), sort_keys=True))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
