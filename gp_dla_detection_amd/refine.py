"""Refined absorber posteriors: per-quasar zoom boxes of (z_DLA, log10 N_HI) around the
posterior mass of a processed single-DLA batch, re-swept on the GPU on a shared unit-square point set.

The first pass evaluates every quasar on one shared table of samples drawn from the prior; a confident
detection has a posterior much narrower than that table's spacing, so its MAP, its credible intervals and
its evidence rest on a single sample (effective sample size 1).  :meth:`api.Batch.refine` maps the
context's refine points into a box chosen per quasar around the samples within ``delta`` of the maximum,
sweeps them with the same kernels, and repeats from the result (``levels``).  The definitions are in
include/gpdla.h; nothing of this exists in the reference.

    python -m gp_dla_detection_amd.refine PRELOADED CATALOG LEARNED SAMPLES PROCESSED OUT
        [--p-thresh P] [--levels L] [--delta D] [--pad PAD] [--points N] [--prior LOG_NHIS] [--batch B]
        [--posteriors] [--tables]

selects the quasars of a processed single-DLA file by ``p_dlas >= P``, processes and refines them batch by
batch (:func:`api.run_pipeline`) and writes OUT (:func:`io.save_refined_results`).  ``--posteriors`` adds the
model posteriors recomputed from the refined evidence; ``--tables`` adds the last level's
``sample_log_posteriors_refined`` of the selected quasars and the unit points ``refine_u`` / ``refine_v``, which
``python -m gp_dla_detection_amd.cddf --refined OUT`` bins.  Only that table is downloaded, each batch into its
rows of one array, and the file writer streams it: the host holds 8 S' bytes per selected quasar until the file
is written, plus one transposed slab of at most 64 MiB while it is.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

SCALARS = ("log_likelihoods_dla_refined", "log_posteriors_dla_refined", "MAP_z_dlas_refined", "MAP_log_nhis_refined",
           "MAP_inds_refined")
TABLES = ("sample_log_likelihoods_refined", "sample_log_posteriors_refined")
POSTERIORS = ("model_posteriors_refined", "p_no_dlas_refined", "p_dlas_refined", "refined")
POINTS = ("refine_u", "refine_v")   # the unit points the tables were swept on, stored beside them
DEFAULT_LEVELS, DEFAULT_DELTA, DEFAULT_PAD = 2, 12.5, 2.0


def default_points(num: int, device: int = 0):
    """(u, v): ``num`` RR2-scrambled Halton points of bases 2 and 3 from index 1 (index 0 is the origin)."""
    from . import samples
    pts = samples.scrambled_halton(1, int(num), bases=(2, 3), device=device)
    return np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])


def request(levels: int = DEFAULT_LEVELS, delta: float = DEFAULT_DELTA, pad: float = DEFAULT_PAD) -> "_lib.RefineRequest":
    return _lib.RefineRequest(int(levels), float(delta), float(pad))


def validate(levels: int = DEFAULT_LEVELS, delta: float = DEFAULT_DELTA, pad: float = DEFAULT_PAD, prior=None, u=None,
             v=None) -> None:
    """The library's own checks of a request, a prior and a point set (gpdla_refine_validate): raises
    :class:`_lib.GpdlaError` naming the offending field.  Needs no GPU."""
    rq = request(levels, delta, pad)
    ps = C.byref(prior._s if hasattr(prior, "_s") else prior) if prior is not None else None
    n, up, vp = 0, None, None
    if u is not None or v is not None:
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if u.size != v.size:
            raise ValueError(f"{u.size} u for {v.size} v")
        n, up, vp = u.size, _lib.ptr(u), _lib.ptr(v)
    _lib.check(_lib.load().gpdla_refine_validate(C.byref(rq), ps, n, up, vp))


def tables_of(with_samples) -> tuple:
    """The sample tables ``with_samples`` asks for: all of TABLES (True), none (False), or the names given."""
    if isinstance(with_samples, (bool, np.bool_)):
        return TABLES if with_samples else ()
    names = (with_samples,) if isinstance(with_samples, str) else tuple(with_samples)
    if any(k not in TABLES for k in names):
        raise ValueError(f"with_samples names {names}; the tables are {TABLES}")
    return names


def empty_results(n: int, levels: int, num_points: int, with_samples=True) -> dict:
    """Host arrays of gpdla_refined_results for ``n`` quasars.  ``with_samples``: True (both tables), False, or
    the names of the tables wanted."""
    out = {k: np.full(n, np.nan) for k in SCALARS}
    out["boxes"] = np.full((n, int(levels), 4), np.nan)
    out["status"] = np.full(n, _lib.REFINE_NOT_REFINED, dtype=np.int32)
    for k in tables_of(with_samples):
        out[k] = np.full((n, int(num_points)), np.nan)
    return out


def empty_posteriors(n: int) -> dict:
    """Host arrays of gpdla_refined_posteriors for ``n`` quasars."""
    return {"model_posteriors_refined": np.full((n, 2), np.nan), "p_no_dlas_refined": np.full(n, np.nan),
            "p_dlas_refined": np.full(n, np.nan), "refined": np.zeros(n, dtype=np.int32)}


def refine_absorbers(model: dict, samples: dict, spectra, results: dict, p_dla_threshold: float = 0.9, levels: int = DEFAULT_LEVELS,
                     delta: float = DEFAULT_DELTA, pad: float = DEFAULT_PAD, prior=None, points=None, params=None,
                     device: int = 0, max_quasars_per_batch: int = 1024, pipeline_slots: int = 3, with_samples=False,
                     summaries: bool = True, probabilities=None, thresholds=None, posteriors: bool = False) -> dict:
    """The host-arrays convenience: refine the quasars of ``spectra`` (a list of per-quasar dicts) whose
    ``results["p_dlas"]`` (of :func:`api.process_qsos` on the same list) reach ``p_dla_threshold``.  The
    selected quasars are processed again and refined batch by batch through :func:`api.run_pipeline`.
    ``points``: (u, v), default :func:`default_points` with as many points as there are DLA samples.
    Returns ``selection`` (indices into ``spectra``) and, per selected quasar, what :meth:`api.Batch.refine`
    returns, plus (``summaries``) the refined parameter summaries under ``summaries``, (``posteriors``) what
    :meth:`api.Batch.refined_posteriors` returns and (``with_samples``: True, or the names of the tables wanted)
    the unit points ``refine_u`` / ``refine_v``.  Every batch downloads into its rows of ONE set of output arrays:
    the host holds 8 S' bytes per selected quasar and table asked for, and no second copy."""
    from . import api, posteriors as _post
    from .parameters import Parameters
    spectra = list(spectra)
    with np.errstate(invalid="ignore"):
        sel = np.flatnonzero(np.asarray(results["p_dlas"], dtype=np.float64) >= float(p_dla_threshold))
    validate(levels, delta, pad, prior, *(points if points is not None else (None, None)))
    lp_no = np.asarray(results["log_priors_no_dla"], dtype=np.float64)
    lp_dla = np.asarray(results["log_priors_dla"], dtype=np.float64)
    p, t = _post.check_request(_post.DEFAULT_PROBABILITIES if probabilities is None else probabilities,
                               _post.DEFAULT_THRESHOLDS if thresholds is None else thresholds)
    blocks = api.batch_blocks(sel.size, max_quasars_per_batch)
    parts = [None] * len(blocks)
    used_points = points
    num_points = np.asarray(samples["offset_samples"]).size if points is None else np.asarray(points[0]).size
    out = empty_results(sel.size, levels, num_points, with_samples)
    if posteriors:
        out.update(empty_posteriors(sel.size))
    if sel.size:
        ctx = api.Context(device, params or Parameters())
        try:
            ctx.set_model(model)
            ctx.set_samples(samples)
            ctx.set_refine_points(*(points if points is not None else (None, None)))
            used_points = ctx.refine_points

            def inputs(i):
                idx = sel[blocks[i][0]:blocks[i][1]]
                return [spectra[j] for j in idx], lp_no[idx], lp_dla[idx]

            def process(i, batch):
                batch.process()
                batch.refine(None, levels, delta, pad, prior, download=False)

            def download(i, batch):
                batch.download_refined(None, levels, with_samples, out=out, at=blocks[i][0])
                part = {}
                if summaries:
                    part["summaries"] = batch.parameter_summaries(refined=True, probabilities=p, thresholds=t)
                if posteriors:
                    for k, a in batch.refined_posteriors().items():
                        out[k][blocks[i][0]:blocks[i][1]] = a
                parts[i] = part

            api.run_pipeline(ctx, len(blocks), inputs, process, download, pipeline_slots)
        finally:
            ctx.close()
    out["selection"] = sel
    if tables_of(with_samples):
        if used_points is None:   # nothing was selected: the points a context would have made
            used_points = default_points(num_points, device)
        out["refine_u"], out["refine_v"] = (np.array(a, dtype=np.float64).reshape(-1) for a in used_points)
    if summaries and parts:
        out["summaries"] = {k: (np.concatenate([part["summaries"][k] for part in parts]) if k not in ("probabilities", "thresholds", "selection")
                                else parts[0]["summaries"][k]) for k in parts[0]["summaries"]}
        out["summaries"]["selection"] = sel
    return out


def main(argv=None):
    import argparse

    from . import io, samples as samples_mod
    ap = argparse.ArgumentParser(description="refine the absorber posteriors of a processed single-DLA file (see the module documentation)")
    ap.add_argument("preloaded")
    ap.add_argument("catalog")
    ap.add_argument("learned")
    ap.add_argument("samples")
    ap.add_argument("processed")
    ap.add_argument("out")
    ap.add_argument("--p-thresh", type=float, default=0.9)
    ap.add_argument("--levels", type=int, default=DEFAULT_LEVELS)
    ap.add_argument("--delta", type=float, default=DEFAULT_DELTA)
    ap.add_argument("--pad", type=float, default=DEFAULT_PAD)
    ap.add_argument("--points", type=int, default=0, help="refine points (default: the number of DLA samples)")
    ap.add_argument("--prior", default=None, help="file of catalogue log10 N_HI values: fit the column density prior to them")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--posteriors", action="store_true", help="add the model posteriors recomputed from the refined evidence")
    ap.add_argument("--tables", action="store_true",
                    help="add sample_log_posteriors_refined of the selected quasars and the unit points (for cddf --refined)")
    args = ap.parse_args(argv)
    processed = io.load_processed_qsos(args.processed)
    if np.ndim(processed["log_priors_dla"]) != 1:
        raise SystemExit("a multi-DLA file: the refine pass serves single-DLA runs only")
    catalog = io.load_catalog(args.catalog, names=("z_qsos",))
    test_ind = processed.get("test_ind")
    spectra = io.load_preloaded_qsos(args.preloaded, catalog["z_qsos"], None if test_ind is None else np.asarray(test_ind).reshape(-1).astype(bool))
    model, smp = io.load_learned_model(args.learned), io.load_dla_samples(args.samples)
    prior = samples_mod.fit_nhi_prior(samples_mod.load_log_nhis(args.prior), device=args.device) if args.prior else None
    points = default_points(args.points, args.device) if args.points else None
    from .parameters import Parameters
    params = Parameters(num_lines=int(np.asarray(processed["num_lines"]).reshape(-1)[0])) if "num_lines" in processed else Parameters()
    out = refine_absorbers(model, smp, spectra, processed, args.p_thresh, args.levels, args.delta, args.pad, prior, points,
                           params, args.device, args.batch, posteriors=args.posteriors,
                           with_samples=("sample_log_posteriors_refined",) if args.tables else False)   # that table alone
    io.save_refined_results(args.out, out, p_thresh=np.float64(args.p_thresh), levels=np.float64(args.levels),
                            delta=np.float64(args.delta), pad=np.float64(args.pad))
    print(f"refined {out['selection'].size} of {len(spectra)} quasars -> {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
