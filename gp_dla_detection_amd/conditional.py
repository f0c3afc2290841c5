"""Absorbers refined slot by slot, and the search for one more absorber.

The k-DLA likelihood multiplies the model's mean, its low-rank factor and its noise scale by the product of all k
absorption profiles.  With k - 1 absorbers held fixed that product is one vector per quasar; folded into the
prepared rows (:meth:`api.Batch.set_fixed_absorbers`) it turns the single-DLA sweep, and with it the refine pass
of DESIGN.md 4.18, into the k-DLA likelihood as a function of the remaining absorber alone.  Two things are built
on that here:

* *rounds* -- every slot of a quasar's list in turn is refined with the other slots fixed (coordinate ascent on
  the k-DLA likelihood): a refined (z_DLA, log10 N_HI), credible intervals and an effective sample size per slot;
* *discovery* -- with the whole list fixed, is there one more absorber, and where?  The conditional log Bayes
  factor is ``log_likelihoods_conditional - log_likelihoods_fixed``.

These are CONDITIONAL evidences: the evidence of one more absorber given the listed ones at their current values,
not the marginal evidence of the k-DLA model.  Nothing of this exists in the reference.

    python -m gp_dla_detection_amd.conditional PRELOADED CATALOG LEARNED SAMPLES PROCESSED OUT
        [--extra E] [--rounds R] [--levels L] [--points N] [--prior LOG_NHIS] [--batch B]

refines the reported absorbers of a multi-DLA processed file (:func:`api.map_absorbers`), or the MAP absorber of
a single-DLA file where p_dla wins, ``--extra`` looking for more, and writes OUT (:func:`io.save_conditional_results`).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .parameters import MultiParameters, Parameters

#: per (quasar, slot), from the slot's last pass
SLOT_SCALARS = ("log_likelihoods_fixed", "log_likelihoods_conditional", "log_bayes_factor", "mean_z", "std_z", "mean_log_nhi",
                "std_log_nhi", "effective_samples")
SLOT_QUANTILES = ("quantiles_z", "quantiles_log_nhi")
LISTS = ("z_dlas", "log_nhis", "start_z_dlas", "start_log_nhis")
NEVER = _lib.REFINE_NOT_REFINED   # status of a slot no pass has refined


def lists_of(absorbers, num_quasars: int) -> list:
    """A CSR triple ``(offsets, z_dlas, log_nhis)`` (or None: no absorbers) as one list of [z, log_nhi] pairs per quasar."""
    if absorbers is None:
        return [[] for _ in range(num_quasars)]
    off, z, n = absorbers
    off = np.asarray(off, dtype=np.int64).reshape(-1)
    if off.size != num_quasars + 1:
        raise ValueError(f"absorber offsets: {off.size} entries for {num_quasars} quasars")
    z, n = np.asarray(z, dtype=np.float64).reshape(-1), np.asarray(n, dtype=np.float64).reshape(-1)
    return [[[float(z[j]), float(n[j])] for j in range(off[i], off[i + 1])] for i in range(num_quasars)]


def csr_of(lists) -> tuple:
    """The inverse of :func:`lists_of`."""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = [a for x in lists for a in x]
    return off, np.array([a[0] for a in flat], dtype=np.float64), np.array([a[1] for a in flat], dtype=np.float64)


def padded(lists, width: int):
    """(z_dlas, log_nhis) [n, width], NaN behind the end of each list."""
    z, n = np.full((len(lists), width), np.nan), np.full((len(lists), width), np.nan)
    for i, x in enumerate(lists):
        for j, (zj, nj) in enumerate(x):
            z[i, j], n[i, j] = zj, nj
    return z, n


def _run_pass(ctx, spectra, lp_no, lp_dla, idx, fixed, levels, delta, pad, prior, p, t, sep, meanflux, per_batch, slots) -> dict:
    """One pass: the quasars ``idx``, each conditioned on its list ``fixed[i]``, processed and refined batch by batch
    through :func:`api.run_pipeline`.  Returns, per quasar of ``idx``, the refined MAP, the refine status, the
    evidences, the boxes and the refined parameter summaries."""
    from . import api, refine
    n = idx.size
    blocks = api.batch_blocks(n, per_batch)
    num_points = ctx.refine_points[0].size
    ref = refine.empty_results(n, levels, num_points, False)
    first = api.Batch.empty_results(n, ctx.num_samples, False)
    summ = [None] * len(blocks)

    def inputs(i):
        sel = idx[blocks[i][0]:blocks[i][1]]
        return [spectra[j] for j in sel], lp_no[sel], lp_dla[sel]

    def process(i, batch):
        batch.set_fixed_absorbers(csr_of(fixed[blocks[i][0]:blocks[i][1]]), sep, meanflux)
        batch.process()
        batch.refine(None, levels, delta, pad, prior, download=False)

    def download(i, batch):
        batch.download(False, out=first, at=blocks[i][0])
        batch.download_refined(None, levels, False, out=ref, at=blocks[i][0])
        summ[i] = batch.parameter_summaries(refined=True, probabilities=p, thresholds=t)

    api.run_pipeline(ctx, len(blocks), inputs, process, download, slots)
    out = dict(map_z=ref["MAP_z_dlas_refined"], map_n=ref["MAP_log_nhis_refined"], status=ref["status"], boxes=ref["boxes"],
               log_likelihoods_fixed=first["log_likelihoods_no_dla"], log_likelihoods_conditional=ref["log_likelihoods_dla_refined"])
    out["log_bayes_factor"] = out["log_likelihoods_conditional"] - out["log_likelihoods_fixed"]
    for k in ("mean_z", "std_z", "mean_log_nhi", "std_log_nhi"):
        out[k] = np.concatenate([s[k][:, 0, 0] for s in summ]) if n else np.zeros(0)
    for k in SLOT_QUANTILES:
        out[k] = np.concatenate([s[k][:, 0, 0] for s in summ]) if n else np.zeros((0, len(p)))
    out["effective_samples"] = np.concatenate([s["effective_samples"][:, 0] for s in summ]) if n else np.zeros(0)
    return out


def refine_conditional(model: dict, samples: dict, spectra, absorbers, extra: int = 0, rounds: int = 2, levels: int = 2,
                       delta: float = 12.5, pad: float = 2.0, prior=None, points=None, params=None, log_priors=None,
                       min_z_separation: float | None = None, meanflux_rows: bool | None = None, device: int = 0,
                       max_quasars_per_batch: int = 1024, pipeline_slots: int = 3, probabilities=None, history: bool = False) -> dict:
    """Refine the absorber lists of ``spectra`` (a list of per-quasar dicts) slot by slot on the GPU.

    ``absorbers``: the starting lists as the CSR triple :func:`api.map_absorbers` returns (None: empty lists).
    *Discovery*, ``extra`` times: every quasar is conditioned on its current list, processed and refined; the refined
    MAP becomes a new slot unless the row is unusable or the list holds 8 absorbers already.  *Rounds*, ``rounds``
    times: for slot j = 0, 1, ... the quasars that have a slot j are conditioned on their other slots in list order;
    slot j takes the refined MAP (an unusable row keeps its value).  Every pass is one :func:`api.run_pipeline` over
    the quasars concerned, ``max_quasars_per_batch`` at a time.  ``levels``, ``delta``, ``pad``, ``prior``, ``points``:
    as :func:`refine.refine_absorbers`.  ``params``: the context's parameters (default :class:`MultiParameters`, whose
    rows are the multi-DLA driver's; ``meanflux_rows`` / ``min_z_separation`` override what they imply).
    ``log_priors``: ``(log_priors_no_dla, log_priors_dla)`` per quasar (default log 1/2 each; no result here depends
    on them).

    Returns, NaN-padded to the longest final list (at least one column): ``z_dlas``, ``log_nhis``, ``num_absorbers``,
    ``discovered`` (1: the slot was appended by a discovery pass), the starting values ``start_z_dlas`` /
    ``start_log_nhis`` / ``num_start``; per slot from its last pass ``boxes`` [nq, slot, level, 4], ``status`` (the
    refine status; -1: no pass refined the slot), ``log_likelihoods_fixed`` (the pass's ``log_likelihoods_no_dla``:
    the other absorbers alone), ``log_likelihoods_conditional`` (its ``log_likelihoods_dla_refined``),
    ``log_bayes_factor`` (their difference) and the refined summaries ``mean_z``, ``std_z``, ``mean_log_nhi``,
    ``std_log_nhi``, ``quantiles_z``, ``quantiles_log_nhi`` [nq, slot, probability], ``effective_samples``; and
    ``probabilities``.  ``history=True`` adds ``history``: per pass a dict with ``name``, ``quasars``, ``slot`` (-1 for
    a discovery pass), the lists the pass conditioned on (``fixed``: CSR triple), the pass's own results, and the
    lists after it (``z_dlas``, ``log_nhis``, ``num_absorbers``)."""
    from . import api, posteriors as _post, refine
    spectra = list(spectra)
    nq = len(spectra)
    lists = lists_of(absorbers, nq)
    if any(len(x) > _lib.MAX_FIXED_ABSORBERS for x in lists):
        raise ValueError(f"a starting list holds more than {_lib.MAX_FIXED_ABSORBERS} absorbers")
    start = [[list(a) for a in x] for x in lists]
    refine.validate(levels, delta, pad, prior, *(points if points is not None else (None, None)))
    p, t = _post.check_request(_post.DEFAULT_PROBABILITIES if probabilities is None else probabilities, _post.DEFAULT_THRESHOLDS)
    lp_no, lp_dla = (np.full(nq, np.log(0.5)),) * 2 if log_priors is None else \
        (np.ascontiguousarray(x, dtype=np.float64).reshape(-1) for x in log_priors)
    params = params or MultiParameters()
    cap = _lib.MAX_FIXED_ABSORBERS
    width = max(1, min(cap, max([len(x) for x in lists], default=0) + max(0, int(extra))))
    slot = {k: np.full((nq, width), np.nan) for k in SLOT_SCALARS}
    slot.update({k: np.full((nq, width, len(p)), np.nan) for k in SLOT_QUANTILES})
    slot["boxes"] = np.full((nq, width, int(levels), 4), np.nan)
    slot["status"] = np.full((nq, width), NEVER, dtype=np.int32)
    discovered = np.zeros((nq, width), dtype=np.int32)
    hist = []

    def record(name, idx, j, fixed, res):
        if history:
            z, n = padded(lists, width)
            hist.append(dict(name=name, quasars=idx.copy(), slot=j, fixed=csr_of(fixed), z_dlas=z, log_nhis=n,
                             num_absorbers=np.array([len(x) for x in lists], dtype=np.int64), **res))

    def keep(idx, cols, res):
        for k in SLOT_SCALARS + SLOT_QUANTILES + ("boxes", "status"):
            slot[k][idx, cols] = res[k]

    if nq and (extra > 0 or (rounds > 0 and any(lists))):
        ctx = api.Context(device, params)
        try:
            ctx.set_model(model)
            ctx.set_samples(samples)
            ctx.set_refine_points(*(points if points is not None else (None, None)))
            run = lambda idx, fixed: _run_pass(ctx, spectra, lp_no, lp_dla, idx, fixed, int(levels), delta, pad, prior, p, t,  # noqa: E731
                                               min_z_separation, meanflux_rows, max_quasars_per_batch, pipeline_slots)
            for e in range(int(extra)):
                idx = np.arange(nq, dtype=np.int64)
                fixed = [list(lists[i]) for i in idx]
                res = run(idx, fixed)
                took = np.array([res["status"][i] == 0 and len(lists[q]) < cap for i, q in enumerate(idx)], dtype=bool)
                for i in np.flatnonzero(took):
                    lists[idx[i]].append([float(res["map_z"][i]), float(res["map_n"][i])])
                    discovered[idx[i], len(lists[idx[i]]) - 1] = 1
                cols = np.array([len(lists[q]) - 1 for q in idx[took]], dtype=np.int64)
                keep(idx[took], cols, {k: v[took] for k, v in res.items() if k in slot})
                record(f"discover {e}", idx, -1, fixed, res)
            for r in range(int(rounds)):
                for j in range(max((len(x) for x in lists), default=0)):
                    idx = np.array([q for q in range(nq) if len(lists[q]) > j], dtype=np.int64)
                    fixed = [lists[q][:j] + lists[q][j + 1:] for q in idx]
                    res = run(idx, fixed)
                    for i, q in enumerate(idx):
                        if res["status"][i] == 0:
                            lists[q][j] = [float(res["map_z"][i]), float(res["map_n"][i])]
                    keep(idx, np.full(idx.size, j, dtype=np.int64), {k: v for k, v in res.items() if k in slot})
                    record(f"round {r} slot {j}", idx, j, fixed, res)
        finally:
            ctx.close()

    longest = max(1, max((len(x) for x in lists), default=0))
    out = {k: v[:, :longest] for k, v in slot.items()}
    out["discovered"] = discovered[:, :longest]
    out["z_dlas"], out["log_nhis"] = padded(lists, longest)
    out["start_z_dlas"], out["start_log_nhis"] = padded(start, longest)
    out["num_absorbers"] = np.array([len(x) for x in lists], dtype=np.int64)
    out["num_start"] = np.array([len(x) for x in start], dtype=np.int64)
    out["probabilities"] = np.asarray(p, dtype=np.float64)
    if history:
        for h in hist:   # (the lists of every pass at the final width)
            h["z_dlas"], h["log_nhis"] = h["z_dlas"][:, :longest], h["log_nhis"][:, :longest]
        out["history"] = hist
    return out


def refine_multi_absorbers(model: dict, samples: dict, spectra, results_multi: dict, **kw) -> dict:
    """The reported absorbers of a multi-DLA run (:func:`api.map_absorbers` of ``results_multi``, the result of
    :func:`api.process_qsos_multiple_dlas_meanflux` on the same ``spectra``) refined slot by slot:
    :func:`refine_conditional`, which documents the keywords, started from them."""
    from . import api
    return refine_conditional(model, samples, spectra, api.map_absorbers(results_multi), **kw)


def main(argv=None):
    import argparse

    from . import api, io, refine, samples as samples_mod
    ap = argparse.ArgumentParser(description="refine the reported absorbers of a processed file slot by slot (see the module documentation)")
    for name in ("preloaded", "catalog", "learned", "samples", "processed", "out"):
        ap.add_argument(name)
    ap.add_argument("--extra", type=int, default=0, help="discovery passes: look for this many further absorbers")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--levels", type=int, default=refine.DEFAULT_LEVELS)
    ap.add_argument("--points", type=int, default=0, help="refine points (default: the number of DLA samples)")
    ap.add_argument("--prior", default=None, help="file of catalogue log10 N_HI values: fit the column density prior to them")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    processed = io.load_processed_qsos(args.processed)
    multi = np.ndim(processed["log_priors_dla"]) != 1
    catalog = io.load_catalog(args.catalog, names=("z_qsos",))
    test_ind = processed.get("test_ind")
    spectra = io.load_preloaded_qsos(args.preloaded, catalog["z_qsos"], None if test_ind is None else np.asarray(test_ind).reshape(-1).astype(bool))
    model, smp = io.load_learned_model(args.learned), io.load_dla_samples(args.samples)
    prior = samples_mod.fit_nhi_prior(samples_mod.load_log_nhis(args.prior), device=args.device) if args.prior else None
    points = refine.default_points(args.points, args.device) if args.points else None
    lines = dict(num_lines=int(np.asarray(processed["num_lines"]).reshape(-1)[0])) if "num_lines" in processed else {}
    out = refine_conditional(model, smp, spectra, api.map_absorbers(processed), extra=args.extra, rounds=args.rounds, levels=args.levels,
                             prior=prior, points=points, params=(MultiParameters if multi else Parameters)(**lines), device=args.device,
                             max_quasars_per_batch=args.batch)
    io.save_conditional_results(args.out, out, extra=np.float64(args.extra), rounds=np.float64(args.rounds), levels=np.float64(args.levels))
    print(f"{int(out['num_absorbers'].sum())} absorbers of {len(spectra)} quasars ({int(out['discovered'].sum())} discovered) -> {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
