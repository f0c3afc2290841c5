"""File-to-file model spectra:

    python -m gp_dla_detection_amd.model_spectra --preloaded preloaded_qsos.mat --catalog catalog.mat \\
        --model learned_qso_model.mat --samples dla_samples.mat --processed processed_qsos.mat \\
        --p-dla 0.9 --out model_spectra.mat

For the selected quasars of a processed run -- those with ``p_dla`` at or above a threshold, or an
explicit list of positions within the run -- writes one ``-v7.3`` file with, per pixel of each
quasar's unmasked-range grid: the absorption of the MAP absorbers of its most probable model, the
posterior-weighted mean and variance of the sampled DLA profile, the GP continuum and the model
flux (:func:`gp_dla_detection_amd.api.model_spectra`).  Nothing is swept again: the posterior weights
are the rows of the processed file's sample table, streamed in blocks of selected quasars the way
``cddf.from_processed_file`` reads them.

``--refined [--levels L] [--points N]`` (single-DLA files; the default products, ``--marginal-continuum`` and
``--predictive-flux``): the selected quasars are processed again and refined block by block, and the sampled DLA
profile is averaged over the refined table instead of the first pass's (posterior mass outside a quasar's
last box is ignored).  The file gains ``refine_boxes`` and ``refine_status``.

``--absorption-distribution [--thresholds 0.8,0.5] [--bins 64] [--quantile-levels 0.025,0.16,0.5,0.84,0.975] [--histogram]``
writes the per-pixel distribution of the absorption instead; it combines with ``--multi-models``,
``--components``, ``--model-weights`` and ``--refined`` as ``--predictive-flux`` does.

The module shares its name with :func:`gp_dla_detection_amd.api.model_spectra`, so it is callable:
``gp_dla_detection_amd.model_spectra(model, samples, spectra, results, ...)`` is that function.
"""
from __future__ import annotations

import argparse
import sys
import types

import numpy as np

from . import api, hdf5, io
from .parameters import MultiParameters, Parameters


def sample_row_reader(processed: str, sub_dla: bool = False, span: int = 2048):
    """``rows(idx) -> [len(idx), S]`` over the sample table of a processed file (stored ``[S, nq]``,
    multi-DLA ``[max_dlas, S, nq]``: model DLA(1); ``sub_dla``: ``sample_log_likelihoods_lls``), one
    read per run of selected quasars within ``span`` of its first.  ``idx`` ascending.  Returns
    ``(rows, close)``."""
    f = hdf5.File(processed)
    ds = f["sample_log_likelihoods_lls" if sub_dla else "sample_log_likelihoods_dla"]
    S = ds.shape[-2]

    def rows(idx):
        idx = np.asarray(idx, dtype=np.int64)
        out = np.empty((idx.size, S))
        i = 0
        while i < idx.size:
            lo = int(idx[i])
            j = int(np.searchsorted(idx, lo + span))
            hi = int(idx[j - 1]) + 1
            slab = (ds.read_slab(0, S, axis1=(lo, hi)) if len(ds.shape) == 2
                    else ds.read_slab(0, 1, axis1=(0, S), axis2=(lo, hi))[0])  # [S, hi - lo]
            out[i:j] = slab[:, idx[i:j] - lo].T
            i = j
        return out
    return rows, f.close


def multi_row_reader(processed: str, span: int = 2048):
    """``rows(idx) -> dict`` of ``sample_log_likelihoods_dla [len(idx), max_dlas, S]``, ``base_sample_inds
    [len(idx), max_dlas-1, S]`` and ``sample_log_likelihoods_lls [len(idx), S]`` over the tables of a multi-DLA
    processed file (stored ``[max_dlas, S, nq]``, ``[max_dlas-1, S, nq]`` and ``[S, nq]``), read like
    :func:`sample_row_reader` reads one row: what ``api.model_spectra(multi_models=True)`` streams.  ``idx``
    ascending.  Returns ``(rows, close)``."""
    f = hdf5.File(processed)
    dla, lls = f["sample_log_likelihoods_dla"], f["sample_log_likelihoods_lls"]
    if len(dla.shape) != 3:
        f.close()
        raise ValueError(f"{processed}: not a multi-DLA processed file (sample_log_likelihoods_dla is {len(dla.shape)}-D)")
    md, S = dla.shape[0], dla.shape[1]
    base = f["base_sample_inds"] if md > 1 else None

    def rows(idx):
        idx = np.asarray(idx, dtype=np.int64)
        out = {"sample_log_likelihoods_dla": np.empty((idx.size, md, S)), "sample_log_likelihoods_lls": np.empty((idx.size, S)),
               "base_sample_inds": np.zeros((idx.size, md - 1, S), dtype=np.uint32)}
        i = 0
        while i < idx.size:
            lo = int(idx[i])
            j = int(np.searchsorted(idx, lo + span))
            hi = int(idx[j - 1]) + 1
            take = idx[i:j] - lo
            out["sample_log_likelihoods_dla"][i:j] = dla.read_slab(0, md, axis1=(0, S), axis2=(lo, hi))[:, :, take].transpose(2, 0, 1)
            out["sample_log_likelihoods_lls"][i:j] = lls.read_slab(0, S, axis1=(lo, hi))[:, take].T
            if base is not None:
                out["base_sample_inds"][i:j] = base.read_slab(0, md - 1, axis1=(0, S), axis2=(lo, hi))[:, :, take].transpose(2, 0, 1)
            i = j
        return out
    return rows, f.close


def select(results: dict, p_dla: float | None, indices) -> np.ndarray:
    """Positions within the run: an explicit (sorted, unique) list, or ``p_dlas >= p_dla``."""
    if indices is not None:
        return np.unique(np.asarray(indices, dtype=np.int64))
    p = np.asarray(results["p_dlas"], dtype=np.float64).reshape(-1)
    return np.flatnonzero(p >= (0.0 if p_dla is None else p_dla))


def _open_run(preloaded, catalog, model_file, samples_file, processed, small, p_dla, indices, refined=None):
    """What every run opens of a processed run: the ``small`` variables of the processed file (and ``test_ind``; ``refined``:
    the priors too) with the ``single_`` prefixes dropped and the probabilities and priors flat, the selection, the spectra
    of the selected quasars alone (positions 0 .. len(sel) - 1 of the list map to ``sel``), the model and the samples.
    Returns ``(results, sel, spectra_sel, model, samples)``."""
    small = list(small) + ["test_ind"] + (["log_priors_no_dla", "log_priors_dla"] if refined is not None else [])
    results = {}
    for k, v in io.loadmat73(processed, small).items():
        k = k[len("single_"):] if k.startswith("single_") else k
        results[k] = np.asarray(v, dtype=np.float64).reshape(-1) if k.startswith(("p_", "log_priors_")) else v
    sel = select(results, p_dla, indices)
    z_qsos = np.asarray(io.load_catalog(catalog, ("z_qsos",))["z_qsos"], dtype=np.float64)
    test_ind = np.asarray(results["test_ind"]).reshape(-1).astype(bool) if "test_ind" in results else None
    run_pos = np.flatnonzero(test_ind) if test_ind is not None else np.arange(z_qsos.size)
    spectra_sel = io.load_preloaded_qsos(preloaded, z_qsos, run_pos[sel])
    return results, sel, spectra_sel, io.load_learned_model(model_file), io.load_dla_samples(samples_file)


def run(preloaded: str, catalog: str, model_file: str, samples_file: str, processed: str, out: str,
        p_dla: float | None = None, indices=None, products=("map", "moments", "continuum"), multi: bool | None = None,
        moments_sub_dla: bool = False, device: int = 0, max_quasars_per_batch: int | None = None,
        multi_models: bool = False, refined: dict | None = None) -> dict:
    small = ["model_posteriors", "p_dlas", "MAP_z_dlas", "MAP_log_nhis", "single_MAP_z_dlas", "single_MAP_log_nhis"]
    results, sel, spectra_sel, model, samples = _open_run(preloaded, catalog, model_file, samples_file, processed, small,
                                                          p_dla, indices, refined)
    mp = np.asarray(results["model_posteriors"], dtype=np.float64)
    is_multi = mp.shape[1] > 2 if multi is None else bool(multi)
    for k in ("MAP_z_dlas", "MAP_log_nhis"):
        v = np.asarray(results[k], dtype=np.float64)
        results[k] = v.reshape(-1) if not is_multi else v  # MATLAB [nq x model x slot] is this package's order
    absorbers = api.map_absorbers(results, sub_dla=is_multi)
    absorbers_sel = api._take_absorbers(absorbers, sel)
    if multi_models and not is_multi:
        raise ValueError("--multi-models needs a multi-DLA processed file")
    # (refined: the weights are the refined table's, so the file's sample tables are neither needed nor opened)
    rows, close = sample_row_reader(processed, sub_dla=moments_sub_dla) if refined is None else (None, lambda: None)
    multi_rows, close_multi = multi_row_reader(processed) if multi_models else (None, lambda: None)
    priors = None if refined is None else {k: results[k][sel] for k in ("log_priors_no_dla", "log_priors_dla")}
    try:  # the loaded list holds the selected quasars only: positions 0 .. len(sel) - 1 map to sel
        res = api.model_spectra(model, samples, spectra_sel, priors, params=MultiParameters() if is_multi else Parameters(),
                                absorbers=absorbers_sel, moments_sub_dla=moments_sub_dla, products=products,
                                sample_rows=None if rows is None else (lambda idx: rows(sel[idx])), device=device,
                                max_quasars_per_batch=max_quasars_per_batch, multi_models=multi_models,
                                model_weights=mp[sel] if multi_models else None,
                                multi_rows=(lambda idx: multi_rows(sel[idx])) if multi_models else None, refined=refined)
    finally:
        close()
        close_multi()
    res["selection"] = sel
    res["absorber_offsets"], res["absorber_z_dlas"], res["absorber_log_nhis"] = absorbers_sel
    io.save_model_spectra(out, res, processed_file=str(processed), multi_dla=np.float64(is_multi),
                          **({"refined": np.float64(1)} if refined is not None else {}))
    return res


def _run_mixture(call, preloaded, catalog, model_file, samples_file, processed, p_dla, indices, components, model_weights,
                 multi, device, max_quasars_per_batch, **more):
    """What ``--marginal-continuum`` and ``--predictive-flux`` share: the selection of a processed file, its spectra,
    its sample tables streamed like the moments' rows, and ``call`` (:func:`api.marginal_continuum` or
    :func:`api.predictive_flux`) on them.  Returns ``(result with its selection, is_multi, components)``."""
    results, sel, spectra_sel, model, samples = _open_run(preloaded, catalog, model_file, samples_file, processed,
                                                          ["model_posteriors", "p_dlas", "p_no_dlas", "p_lls"], p_dla, indices,
                                                          more.get("refined"))
    is_multi = np.asarray(results["model_posteriors"]).shape[1] > 2 if multi is None else bool(multi)
    components = tuple(components)
    readers = {} if more.get("refined") is not None else {
        name: sample_row_reader(processed, sub_dla=name == "sub_dla") for name in components if name != "null"}
    res_sel = {k: v[sel] for k, v in results.items() if k.startswith(("p_", "log_priors_"))}
    try:  # the loaded list holds the selected quasars only: positions 0 .. len(sel) - 1 map to sel
        res = call(model, samples, spectra_sel, res_sel, params=MultiParameters() if is_multi else Parameters(),
                   components=components, model_weights="posteriors" if model_weights == "posteriors" else None,
                   sample_rows=lambda idx, name: readers[name][0](sel[idx]), device=device,
                   max_quasars_per_batch=max_quasars_per_batch, **more)
    finally:
        for _, close in readers.values():
            close()
    res["selection"] = sel
    return res, is_multi, components


def _run_mixture_multi(call, preloaded, catalog, model_file, samples_file, processed, p_dla, indices, model_weights, device,
                       max_quasars_per_batch, **more):
    """``--multi-models`` of ``--marginal-continuum`` and ``--predictive-flux``: the selection of a multi-DLA processed file,
    its spectra, its three tables streamed by :func:`multi_row_reader` (as ``--multi-models`` of the moments streams them)
    and ``call(..., multi_models=True)``.  ``model_weights``: ``"posteriors"`` (the file's ``model_posteriors``) or
    ``"equal"`` (equal over all ``2 + max_dlas`` components).  Returns the result with its selection and model_weights."""
    results, sel, spectra_sel, model, samples = _open_run(preloaded, catalog, model_file, samples_file, processed,
                                                          ["model_posteriors", "p_dlas"], p_dla, indices)
    mp = np.asarray(results["model_posteriors"], dtype=np.float64)
    if mp.shape[1] <= 2:
        raise ValueError("--multi-models needs a multi-DLA processed file")
    weights = mp[sel] if model_weights == "posteriors" else np.ones((sel.size, mp.shape[1]))
    multi_rows, close = multi_row_reader(processed)
    try:  # the loaded list holds the selected quasars only: positions 0 .. len(sel) - 1 map to sel
        res = call(model, samples, spectra_sel, None, params=MultiParameters(max_dlas=mp.shape[1] - 2), model_weights=weights,
                   multi_models=True, multi_rows=lambda idx: multi_rows(sel[idx]), device=device,
                   max_quasars_per_batch=max_quasars_per_batch, **more)
    finally:
        close()
    res["selection"] = sel
    res["model_weights"] = weights
    return res


def run_marginal_continuum(preloaded: str, catalog: str, model_file: str, samples_file: str, processed: str, out: str,
                           p_dla: float | None = None, indices=None, components=("dla",), model_weights="posteriors",
                           multi: bool | None = None, device: int = 0, max_quasars_per_batch: int | None = None,
                           multi_models: bool = False, refined: dict | None = None) -> dict:
    """``--marginal-continuum``: :func:`api.marginal_continuum` of the selected quasars of a processed file, its
    sample tables streamed like the moments' rows, written by :func:`io.save_marginal_continuum`.
    ``model_weights``: ``"posteriors"`` (p_no_dlas, p_lls or 0, p_dlas of the file) or ``"equal"``.
    ``multi_models`` (``--multi-models``): the mixture over all models of a multi-DLA file;
    ``components`` is ignored, ``model_weights`` is the file's ``model_posteriors`` or equal over all of them.
    ``refined`` (``--refined``): ``refined=`` of :func:`api.marginal_continuum`; ``"posteriors"`` are then the refined ones."""
    if multi_models and refined is not None:
        raise ValueError("--refined: not with --multi-models (a multi-DLA batch cannot be refined)")
    if multi_models:
        res = _run_mixture_multi(api.marginal_continuum, preloaded, catalog, model_file, samples_file, processed, p_dla, indices,
                                 model_weights, device, max_quasars_per_batch)
        io.save_marginal_continuum(out, res, processed_file=str(processed), multi_dla=np.float64(1), multi_models=np.float64(1))
        return res
    res, is_multi, components = _run_mixture(api.marginal_continuum, preloaded, catalog, model_file, samples_file, processed,
                                             p_dla, indices, components, model_weights, multi, device, max_quasars_per_batch,
                                             **({"refined": refined} if refined is not None else {}))
    io.save_marginal_continuum(out, res, processed_file=str(processed), multi_dla=np.float64(is_multi),
                               components=",".join(components), **({"refined": np.float64(1)} if refined is not None else {}))
    return res


def run_predictive_flux(preloaded: str, catalog: str, model_file: str, samples_file: str, processed: str, out: str,
                        p_dla: float | None = None, indices=None, components=("dla",), model_weights="posteriors",
                        residuals: bool = False, multi: bool | None = None, device: int = 0,
                        max_quasars_per_batch: int | None = None, multi_models: bool = False,
                        refined: dict | None = None) -> dict:
    """``--predictive-flux``: :func:`api.predictive_flux` of the selected quasars of a processed file, its sample
    tables streamed like the moments' rows, written by :func:`io.save_predictive_flux`.  The arguments are those of
    :func:`run_marginal_continuum`; ``residuals``: also the in-sample replicate residuals (``--residuals``)."""
    if multi_models and refined is not None:
        raise ValueError("--refined: not with --multi-models (a multi-DLA batch cannot be refined)")
    if multi_models:
        res = _run_mixture_multi(api.predictive_flux, preloaded, catalog, model_file, samples_file, processed, p_dla, indices,
                                 model_weights, device, max_quasars_per_batch, residuals=residuals)
        io.save_predictive_flux(out, res, processed_file=str(processed), multi_dla=np.float64(1), multi_models=np.float64(1))
        return res
    res, is_multi, components = _run_mixture(api.predictive_flux, preloaded, catalog, model_file, samples_file, processed,
                                             p_dla, indices, components, model_weights, multi, device, max_quasars_per_batch,
                                             residuals=residuals, **({"refined": refined} if refined is not None else {}))
    io.save_predictive_flux(out, res, processed_file=str(processed), multi_dla=np.float64(is_multi),
                            components=",".join(components), **({"refined": np.float64(1)} if refined is not None else {}))
    return res


def run_absorption_distribution(preloaded: str, catalog: str, model_file: str, samples_file: str, processed: str, out: str,
                                p_dla: float | None = None, indices=None, components=("dla",), model_weights="posteriors",
                                thresholds=(0.8,), bins: int = 64, levels=None, histogram: bool = False,
                                multi: bool | None = None, device: int = 0, max_quasars_per_batch: int | None = None,
                                multi_models: bool = False, refined: dict | None = None) -> dict:
    """``--absorption-distribution``: :func:`api.absorption_distribution` of the selected quasars of a processed file, its
    sample tables streamed like the moments' rows, written by :func:`io.save_absorption_distribution`.  ``thresholds``,
    ``bins``, ``levels`` (``--quantile-levels``), ``histogram``: as :meth:`api.Batch.absorption_distribution`; the other
    arguments are those of :func:`run_marginal_continuum`."""
    if multi_models and refined is not None:
        raise ValueError("--refined: not with --multi-models (a multi-DLA batch cannot be refined)")
    dist = dict(thresholds=tuple(thresholds), bins=int(bins), levels=None if not levels else tuple(levels), histogram=bool(histogram))
    request = dict(thresholds=dist["thresholds"], levels=dist["levels"] or (), num_bins=dist["bins"] if (histogram or levels) else 0)
    if multi_models:
        res = _run_mixture_multi(api.absorption_distribution, preloaded, catalog, model_file, samples_file, processed, p_dla,
                                 indices, model_weights, device, max_quasars_per_batch, **dist)
        io.save_absorption_distribution(out, res, processed_file=str(processed), multi_dla=np.float64(1), multi_models=np.float64(1),
                                        **request)
        return res
    res, is_multi, components = _run_mixture(api.absorption_distribution, preloaded, catalog, model_file, samples_file, processed,
                                             p_dla, indices, components, model_weights, multi, device, max_quasars_per_batch,
                                             **dist, **({"refined": refined} if refined is not None else {}))
    io.save_absorption_distribution(out, res, processed_file=str(processed), multi_dla=np.float64(is_multi),
                                    components=",".join(components), **request,
                                    **({"refined": np.float64(1)} if refined is not None else {}))
    return res


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    for name in ("preloaded", "catalog", "model", "samples", "processed", "out"):
        ap.add_argument(f"--{name}", required=True)
    ap.add_argument("--p-dla", type=float, default=None, help="select quasars with p_dla at or above this")
    ap.add_argument("--indices", type=str, default=None, help="comma-separated positions within the run (0-based)")
    ap.add_argument("--products", type=str, default="map,moments,continuum")
    ap.add_argument("--moments-sub-dla", action="store_true", help="weight the sub-DLA sample table")
    ap.add_argument("--multi-models", action="store_true",
                    help="a multi-DLA processed file: also the moments of every model DLA(1..max_dlas) and of the "
                         "sub-DLA model, and the absorption averaged over the models by model_posteriors; with "
                         "--marginal-continuum / --predictive-flux: the mixture over ALL models (DESIGN.md 4.25)")
    ap.add_argument("--marginal-continuum", action="store_true",
                    help="write the marginal continuum instead (DESIGN.md 4.23): its posterior mean and variance over "
                         "the sample tables and the models")
    ap.add_argument("--predictive-flux", action="store_true",
                    help="write the posterior predictive flux instead (DESIGN.md 4.24): per-pixel mean and variance of "
                         "absorption times continuum over the sample tables and the models")
    ap.add_argument("--absorption-distribution", action="store_true",
                    help="write the per-pixel distribution of the absorption instead (DESIGN.md 4.29): the probability of a "
                         "transmission at or below each threshold, the extremes and, with --quantile-levels / --histogram, "
                         "the quantiles and the histogram; combines with --multi-models, --components, --model-weights, --refined")
    ap.add_argument("--thresholds", type=str, default="0.8", help="--absorption-distribution: up to 4 thresholds inside (0, 1)")
    ap.add_argument("--bins", type=int, default=64, help="--absorption-distribution: bins of the histogram, 8 .. 256")
    ap.add_argument("--quantile-levels", type=str, default=None,
                    help="--absorption-distribution: up to 8 quantile levels inside (0, 1), e.g. 0.025,0.16,0.5,0.84,0.975")
    ap.add_argument("--histogram", action="store_true", help="--absorption-distribution: also the histogram itself")
    ap.add_argument("--residuals", action="store_true",
                    help="--predictive-flux: also the in-sample replicate residuals, chi2 and num_kept")
    ap.add_argument("--components", type=str, default="dla",
                    help="--marginal-continuum, --predictive-flux: any of null,sub_dla,dla (ignored with --multi-models: "
                         "every model is a component)")
    ap.add_argument("--model-weights", choices=("posteriors", "equal"), default="posteriors",
                    help="--marginal-continuum, --predictive-flux: mix the components by the file's posteriors, or equally "
                         "(--multi-models: model_posteriors, or equal over all 2 + max_dlas components)")
    ap.add_argument("--refined", action="store_true",
                    help="a single-DLA file: process and refine the selected quasars again and average over the refined "
                         "table (DESIGN.md 4.28); the default products, --marginal-continuum and --predictive-flux")
    ap.add_argument("--levels", type=int, default=None, help="--refined: refine levels (default 2)")
    ap.add_argument("--points", type=int, default=None, help="--refined: number of refine points (default: the DLA samples)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-quasars-per-batch", type=int, default=None)
    a = ap.parse_args(argv)
    idx = None if a.indices is None else [int(x) for x in a.indices.split(",") if x]
    if (a.levels is not None or a.points is not None) and not a.refined:
        ap.error("--levels and --points go with --refined")
    refined = dict(levels=a.levels, points=a.points) if a.refined else None
    if a.absorption_distribution:
        res = run_absorption_distribution(a.preloaded, a.catalog, a.model, a.samples, a.processed, a.out, p_dla=a.p_dla, indices=idx,
                                          components=tuple(x for x in a.components.split(",") if x), model_weights=a.model_weights,
                                          thresholds=tuple(float(x) for x in a.thresholds.split(",") if x), bins=a.bins,
                                          levels=None if a.quantile_levels is None else
                                          tuple(float(x) for x in a.quantile_levels.split(",") if x),
                                          histogram=a.histogram, device=a.device, max_quasars_per_batch=a.max_quasars_per_batch,
                                          multi_models=a.multi_models, refined=refined)
        print(f"wrote {a.out}: {res['selection'].size} quasars, {int(res['offsets'][-1])} grid pixels")
        return 0
    if a.predictive_flux:
        res = run_predictive_flux(a.preloaded, a.catalog, a.model, a.samples, a.processed, a.out, p_dla=a.p_dla, indices=idx,
                                  components=tuple(x for x in a.components.split(",") if x), model_weights=a.model_weights,
                                  residuals=a.residuals, device=a.device, max_quasars_per_batch=a.max_quasars_per_batch,
                                  multi_models=a.multi_models, refined=refined)
        print(f"wrote {a.out}: {res['selection'].size} quasars, {int(res['offsets'][-1])} grid pixels")
        return 0
    if a.marginal_continuum:
        res = run_marginal_continuum(a.preloaded, a.catalog, a.model, a.samples, a.processed, a.out, p_dla=a.p_dla, indices=idx,
                                     components=tuple(x for x in a.components.split(",") if x), model_weights=a.model_weights,
                                     device=a.device, max_quasars_per_batch=a.max_quasars_per_batch, multi_models=a.multi_models,
                                     refined=refined)
        print(f"wrote {a.out}: {res['selection'].size} quasars, {int(res['offsets'][-1])} grid pixels")
        return 0
    res = run(a.preloaded, a.catalog, a.model, a.samples, a.processed, a.out, p_dla=a.p_dla, indices=idx,
              products=tuple(a.products.split(",")), moments_sub_dla=a.moments_sub_dla, device=a.device,
              max_quasars_per_batch=a.max_quasars_per_batch, multi_models=a.multi_models, refined=refined)
    print(f"wrote {a.out}: {res['selection'].size} quasars, {int(res['offsets'][-1])} grid pixels")
    return 0


class _CallableModule(types.ModuleType):
    def __call__(self, *args, **kwargs):
        return api.model_spectra(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule

if __name__ == "__main__":
    raise SystemExit(main())
