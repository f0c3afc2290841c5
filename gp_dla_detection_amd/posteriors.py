"""Credible intervals and moments of the absorber parameters.

A sweep leaves, per quasar and model, a table of S sample log-likelihoods: a weighted sample of the
posterior of (z_DLA, log10 N_HI) of each absorber of the model.  The reference keeps only its largest
entry (the MAP pair).  This module asks k_parameter_summaries for the rest: per (quasar, model, slot)
the posterior mean and standard deviation of both parameters, their covariance, weighted quantiles
(no interpolation: a quantile is one of the slot's sample values), P(log N >= t), and per (quasar,
model) the effective sample size T^2 / sum w^2 -- an ESS near 1 says the Halton samples do not
resolve the posterior and every quantile has collapsed onto one point.

    python -m gp_dla_detection_amd.posteriors PROCESSED SAMPLES OUT [--p-dla X] [--indices ...]
        [--probabilities ...] [--thresholds ...] [--sub-dla] [--device N] [--json FILE --catalog FILE]
        [--maps NZxNN [--levels ...] [--map-range ZLO ZHI NLO NHI] [--no-cells] [--maps-out FILE]]

--maps adds the posterior maps of DESIGN.md section 4.22 (posterior_maps, maps_from_processed_file,
stack_intensity below): per (quasar, model, slot) the posterior mass on a grid of (z_DLA, log N_HI), its
highest-posterior-density regions, and per quasar the absorber intensity averaged over the models.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

DEFAULT_PROBABILITIES = (0.025, 0.16, 0.5, 0.84, 0.975)
DEFAULT_THRESHOLDS = (20.3,)
FIELDS = ("mean_z", "std_z", "mean_log_nhi", "std_log_nhi", "cov", "quantiles_z", "quantiles_log_nhi",
          "exceedance", "effective_samples", "status")
#: a standard deviation below this fraction of the quantity's scale has no correlation coefficient
CORRELATION_FLOOR = 1e-12


def check_request(probabilities, thresholds):
    from . import _lib
    p = [float(x) for x in probabilities]
    t = [float(x) for x in thresholds]
    if len(p) > _lib.POSTERIOR_MAX_PROBABILITIES:
        raise ValueError(f"{len(p)} probabilities; one call takes at most {_lib.POSTERIOR_MAX_PROBABILITIES}")
    if any(not (0.0 < x < 1.0) for x in p) or any(b <= a for a, b in zip(p, p[1:])):
        raise ValueError("probabilities must lie inside (0, 1) and increase strictly")
    if len(t) > _lib.POSTERIOR_MAX_THRESHOLDS:
        raise ValueError(f"{len(t)} thresholds; one call takes at most {_lib.POSTERIOR_MAX_THRESHOLDS}")
    if any(x != x for x in t):
        raise ValueError("NaN threshold")
    return p, t


def _request(md, p, t):
    from . import _lib
    rq = _lib.SummaryRequest()
    rq.num_models, rq.num_probabilities, rq.num_thresholds = int(md), len(p), len(t)
    for i, x in enumerate(p):
        rq.probabilities[i] = x
    for i, x in enumerate(t):
        rq.thresholds[i] = x
    return rq


def _outputs(n, md, Q, nt):
    """Host arrays of gpdla_parameter_summaries and the struct that points at them."""
    from . import _lib
    out = {k: np.full((n, md, md), np.nan) for k in FIELDS[:5]}
    out["quantiles_z"] = np.full((n, md, md, Q), np.nan)
    out["quantiles_log_nhi"] = np.full((n, md, md, Q), np.nan)
    out["exceedance"] = np.full((n, md, md, nt), np.nan)
    out["effective_samples"] = np.full((n, md), np.nan)
    out["status"] = np.zeros((n, md), dtype=np.int32)
    ps = _lib.ParameterSummaries()
    for k in FIELDS[:-1]:
        setattr(ps, k, _lib.ptr(out[k]))
    ps.status = out["status"].ctypes.data_as(_lib._i32p)
    return out, ps


def _run(sll, base, z_min, z_max, offsets, lnhi, p, t, device):
    """gpdla_stats_parameter_summaries on host tables: sll [n, md, S], base [n, md - 1, S] or None."""
    from . import _lib
    lib = _lib.load()
    n, md, S = sll.shape
    out, ps = _outputs(n, md, len(p), len(t))
    rq = _request(md, p, t)
    bp = base.ctypes.data_as(_lib._u32p) if base is not None else None
    _lib.check(lib.gpdla_stats_parameter_summaries(n, S, _lib.ptr(sll), md * S, bp, _lib.ptr(z_min), _lib.ptr(z_max),
                                                   _lib.ptr(offsets), _lib.ptr(lnhi), C.byref(rq), C.byref(ps),
                                                   int(device)))
    return out


def finish(out, z_min, z_max, n_scale, p, t):
    """What the C boundary leaves to Python: the correlation coefficient (NaN where a standard
    deviation is below CORRELATION_FLOOR x the quantity's scale: max(|min_z|, |max_z|) for z, max |log N
    sample| for log N) and the request, for the writers."""
    z_scale = np.maximum(np.abs(z_min), np.abs(z_max))[:, None, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (out["std_z"] >= CORRELATION_FLOOR * z_scale) & (out["std_log_nhi"] >= CORRELATION_FLOOR * n_scale)
        out["correlation"] = np.where(ok, out["cov"] / (out["std_z"] * out["std_log_nhi"]), np.nan)
    out["probabilities"] = np.asarray(p, dtype=np.float64)
    out["thresholds"] = np.asarray(t, dtype=np.float64)
    return out


def _tables(sample_log_likelihoods, base_sample_inds):
    sll = np.asarray(sample_log_likelihoods, dtype=np.float64)
    if sll.ndim == 2:
        sll = sll[:, None, :]
    if sll.ndim != 3 or sll.shape[2] < 1:
        raise ValueError("sample log-likelihoods must be [n, S] or [n, models, S] with S >= 1")
    sll = np.ascontiguousarray(sll)
    n, md, S = sll.shape
    base = None
    if md > 1:
        if base_sample_inds is None:
            raise ValueError(f"{md} models need base_sample_inds [n, {md - 1}, S]")
        base = np.ascontiguousarray(base_sample_inds, dtype=np.uint32)
        if base.ndim == 3 and base.shape[1] > md - 1:
            base = np.ascontiguousarray(base[:, :md - 1])
        if base.shape != (n, md - 1, S):
            raise ValueError(f"base_sample_inds must be [n, {md - 1}, S] = {(n, md - 1, S)}, got {base.shape}")
    return sll, base


def parameter_summaries(sample_log_likelihoods, samples, min_z_dlas, max_z_dlas, base_sample_inds=None,
                        probabilities=DEFAULT_PROBABILITIES, thresholds=DEFAULT_THRESHOLDS, device=0) -> dict:
    """Summaries of host tables.  ``sample_log_likelihoods``: [n, S] (one model) or [n, models, S] as
    process_qsos_multiple_dlas_meanflux returns it, with ``base_sample_inds`` [n, models - 1, S]
    (1-based, 0 = never drawn).  ``samples``: ``offset_samples`` and ``log_nhi_samples`` (for the sub-DLA
    table pass log10 of ``lls_nhi_samples`` as ``log_nhi_samples``).  Returns arrays [n, models, models]
    in (model, slot) order -- NaN where slot > model -- ``quantiles_*`` with a trailing axis of the
    probabilities, ``exceedance`` with one of the thresholds, ``effective_samples`` and ``status``
    [n, models] (bit 1: no usable sample; bit 2: NaN search range), ``correlation``."""
    p, t = check_request(probabilities, thresholds)
    sll, base = _tables(sample_log_likelihoods, base_sample_inds)
    n, md, S = sll.shape
    z_min = np.ascontiguousarray(min_z_dlas, dtype=np.float64).reshape(-1)
    z_max = np.ascontiguousarray(max_z_dlas, dtype=np.float64).reshape(-1)
    off = np.ascontiguousarray(samples["offset_samples"], dtype=np.float64).reshape(-1)
    lnhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64).reshape(-1)
    if z_min.size != n or z_max.size != n:
        raise ValueError("min_z_dlas and max_z_dlas need one entry per row")
    if off.size != S or lnhi.size != S:
        raise ValueError(f"{S} sample columns but {off.size} offsets and {lnhi.size} log N_HI samples")
    return finish(_run(sll, base, z_min, z_max, off, lnhi, p, t, device), z_min, z_max, float(np.max(np.abs(lnhi))), p, t)


def sub_dla_samples(samples: dict) -> dict:
    """The sample dict of the sub-DLA table: its column densities are lls_nhi_samples."""
    return {"offset_samples": samples["offset_samples"],
            "log_nhi_samples": np.log10(np.asarray(samples["lls_nhi_samples"], dtype=np.float64))}


def from_processed_file(processed, samples_file, selection=None, p_dla=None, sub_dla=False, block_size=2048,
                        probabilities=DEFAULT_PROBABILITIES, thresholds=DEFAULT_THRESHOLDS, device=0) -> dict:
    """Summaries of a processed_qsos file, its tables streamed in quasar blocks
    (hdf5.Dataset.read_slab): each read spans at most ``block_size`` quasars, and the host holds at
    most two blocks -- the read and the block handed to the kernel.  ``selection``: quasar indices
    (increasing), or ``p_dla``: the quasars with ``p_dlas >= p_dla``; default all.  ``sub_dla``: the
    sub-DLA table (``sample_log_likelihoods_lls``) with the LLS column densities, one model.  Results
    do not depend on ``block_size``.  Adds ``selection`` to the returned dict."""
    from . import hdf5, io
    if block_size < 1:
        raise ValueError("block_size must be >= 1")
    p, t = check_request(probabilities, thresholds)
    small = io.loadmat73(processed, ["min_z_dlas", "max_z_dlas", "p_dlas"])
    z_min = np.asarray(small["min_z_dlas"], dtype=np.float64).reshape(-1)
    z_max = np.asarray(small["max_z_dlas"], dtype=np.float64).reshape(-1)
    nq = z_min.size
    if selection is not None:
        sel = np.asarray(selection, dtype=np.int64).reshape(-1)
        if sel.size and (np.any(np.diff(sel) <= 0) or sel[0] < 0 or sel[-1] >= nq):
            raise ValueError(f"selection must increase strictly inside [0, {nq})")
    elif p_dla is not None:
        with np.errstate(invalid="ignore"):
            sel = np.flatnonzero(np.asarray(small["p_dlas"], dtype=np.float64).reshape(-1) >= p_dla)
    else:
        sel = np.arange(nq)
    samples = io.load_dla_samples(samples_file) if isinstance(samples_file, str) else samples_file
    if sub_dla:
        samples = sub_dla_samples(samples)
    off = np.ascontiguousarray(samples["offset_samples"], dtype=np.float64).reshape(-1)
    lnhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64).reshape(-1)
    with hdf5.File(processed) as f:
        ds = f["sample_log_likelihoods_lls" if sub_dla else "sample_log_likelihoods_dla"]   # [S, nq] or [md, S, nq]
        md = ds.shape[0] if len(ds.shape) == 3 else 1
        S = ds.shape[-2]
        if off.size != S or lnhi.size != S:
            raise ValueError(f"the sample table has {S} columns, the samples {off.size}")
        db = f["base_sample_inds"] if md > 1 else None                                       # [md - 1, S, nq]
        parts = []
        i = 0
        while i < sel.size:  # one read per run of selected quasars within block_size of its first
            lo = int(sel[i])
            j = int(np.searchsorted(sel, lo + block_size))
            hi = int(sel[j - 1]) + 1
            cols = sel[i:j] - lo
            if len(ds.shape) == 2:
                sll = np.ascontiguousarray(ds.read_slab(0, S, axis1=(lo, hi))[:, cols].T)[:, None, :]
            else:
                sll = np.ascontiguousarray(
                    np.transpose(ds.read_slab(0, md, axis1=(0, S), axis2=(lo, hi))[:, :, cols], (2, 0, 1)))
            base = None
            if db is not None:
                base = np.ascontiguousarray(
                    np.transpose(db.read_slab(0, md - 1, axis1=(0, S), axis2=(lo, hi))[:, :, cols], (2, 0, 1)),
                    dtype=np.uint32)
            zl, zh = np.ascontiguousarray(z_min[sel[i:j]]), np.ascontiguousarray(z_max[sel[i:j]])
            parts.append(_run(np.ascontiguousarray(sll), base, zl, zh, off, lnhi, p, t, device))
            i = j
    if parts:
        out = {k: np.concatenate([q[k] for q in parts]) for k in FIELDS}
    else:
        out, _ = _outputs(0, md, len(p), len(t))
    out = finish(out, z_min[sel], z_max[sel], float(np.max(np.abs(lnhi))), p, t)
    out["selection"] = sel
    return out


# ---------------------------------------------------------------------------------------------
# posterior maps
# ---------------------------------------------------------------------------------------------

DEFAULT_LEVELS = (0.683, 0.95)
MAP_SLOT_FIELDS = ("mass", "hpd_level", "outside", "mode", "hpd_cells", "hpd_threshold")
MAP_ROW_FIELDS = ("intensity", "expected_absorbers", "status", "grid", "edges_z", "edges_log_nhi", "marginal_z",
                  "marginal_log_nhi")


def check_maps_request(shape, levels):
    """(nz, nn) and the credible masses as the library will accept them."""
    from . import _lib
    nz, nn = (int(x) for x in shape)
    if not (1 <= nz <= _lib.MAPS_MAX_SIDE and 1 <= nn <= _lib.MAPS_MAX_SIDE):
        raise ValueError(f"shape = {(nz, nn)}: each axis takes 1 to {_lib.MAPS_MAX_SIDE} cells")
    lv = [float(x) for x in levels]
    if len(lv) > _lib.MAPS_MAX_LEVELS:
        raise ValueError(f"{len(lv)} levels; one call takes at most {_lib.MAPS_MAX_LEVELS}")
    if any(not (0.0 < x < 1.0) for x in lv) or any(b <= a for a, b in zip(lv, lv[1:])):
        raise ValueError("levels must lie inside (0, 1) and increase strictly")
    return (nz, nn), lv


def maps_request(md, shape, levels, mix=False):
    from . import _lib
    rq = _lib.PosteriorMapsRequest()
    rq.num_models, rq.nz, rq.nn, rq.num_levels, rq.mix = int(md), shape[0], shape[1], len(levels), int(bool(mix))
    for i, x in enumerate(levels):
        rq.levels[i] = x
    return rq


def maps_outputs(n, md, shape, L, mix, with_maps):
    """Host arrays of gpdla_posterior_maps and the struct that points at them.  ``with_maps`` False: no
    per-cell array of a slot (mass, hpd_level) is asked for."""
    from . import _lib
    nz, nn = shape
    out = {}
    if with_maps:
        out["mass"] = np.full((n, md, md, nz, nn), np.nan)
        out["hpd_level"] = np.full((n, md, md, nz, nn), np.nan)
    out["outside"] = np.full((n, md, md), np.nan)
    out["mode"] = np.full((n, md, md), -1, dtype=np.int32)
    out["hpd_cells"] = np.full((n, md, md, L), -1, dtype=np.int32)
    out["hpd_threshold"] = np.full((n, md, md, L), np.nan)
    if mix:
        out["intensity"] = np.full((n, nz, nn), np.nan)
        out["expected_absorbers"] = np.full(n, np.nan)
    out["status"] = np.zeros((n, md), dtype=np.int32)
    pm = _lib.PosteriorMaps()
    for k, a in out.items():
        setattr(pm, k, a.ctypes.data_as(_lib._i32p if a.dtype == np.int32 else _lib._dp))
    return out, pm


def grid_edges(grid, shape):
    """The edges the kernel compares against: per row lo + (hi - lo) * (c / n) for c < n, and hi itself."""
    grid = np.asarray(grid, dtype=np.float64).reshape(-1, 4)
    out = []
    for lo, hi, n in ((grid[:, 0], grid[:, 1], shape[0]), (grid[:, 2], grid[:, 3], shape[1])):
        with np.errstate(invalid="ignore", over="ignore"):
            e = lo[:, None] + (hi - lo)[:, None] * (np.arange(n, dtype=np.float64) / np.float64(n))[None, :]
        out.append(np.concatenate([e, hi[:, None]], axis=1))
    return out


def finish_maps(out, grid, shape, levels):
    """What the C boundary leaves to Python: the edges per row, the two marginals (sums of the masses on
    the host, when the maps came along) and the request."""
    out["grid"] = np.asarray(grid, dtype=np.float64).reshape(-1, 4)
    out["edges_z"], out["edges_log_nhi"] = grid_edges(out["grid"], shape)
    if "mass" in out:
        out["marginal_z"] = out["mass"].sum(axis=4)
        out["marginal_log_nhi"] = out["mass"].sum(axis=3)
    out["levels"] = np.asarray(levels, dtype=np.float64)
    out["shape"] = np.asarray(shape, dtype=np.int64)
    return out


def _grid_rows(grid, n):
    """[n, 4] (gz_lo, gz_hi, gn_lo, gn_hi) from one 4-tuple or one row per quasar."""
    g = np.asarray(grid, dtype=np.float64)
    if g.shape == (4,):
        g = np.tile(g, (n, 1))
    if g.shape != (n, 4):
        raise ValueError(f"grid must be (gz_lo, gz_hi, gn_lo, gn_hi) or [n, 4] with n = {n}, got {g.shape}")
    return np.ascontiguousarray(g)


def _grid_columns(g):
    return [np.ascontiguousarray(g[:, i]) for i in range(4)]


def _weights_rows(model_weights, n, md):
    w = np.ascontiguousarray(model_weights, dtype=np.float64)
    if w.shape == (n,) and md == 1:
        w = w.reshape(n, 1)
    if w.shape != (n, md):
        raise ValueError(f"model_weights must be [n, models] = {(n, md)}, got {w.shape}")
    return w


def _run_maps(sll, base, z_min, z_max, offsets, lnhi, grid, weights, shape, levels, with_maps, device):
    """gpdla_stats_posterior_maps on host tables: sll [n, md, S], base [n, md - 1, S] or None, grid [n, 4]."""
    from . import _lib
    lib = _lib.load()
    n, md, S = sll.shape
    out, pm = maps_outputs(n, md, shape, len(levels), weights is not None, with_maps)
    rq = maps_request(md, shape, levels)
    bp = base.ctypes.data_as(_lib._u32p) if base is not None else None
    cols = _grid_columns(grid)
    _lib.check(lib.gpdla_stats_posterior_maps(n, S, _lib.ptr(sll), md * S, bp, _lib.ptr(z_min), _lib.ptr(z_max),
                                              _lib.ptr(offsets), _lib.ptr(lnhi), *[_lib.ptr(c) for c in cols],
                                              _lib.ptr(weights) if weights is not None else None, C.byref(rq), C.byref(pm),
                                              int(device)))
    return out


def posterior_maps(sample_log_likelihoods, samples, min_z_dlas, max_z_dlas, base_sample_inds=None, grid=None,
                   shape=(32, 32), levels=DEFAULT_LEVELS, model_weights=None, with_maps=True, device=0) -> dict:
    """Posterior maps of (z_DLA, log N_HI) of host tables (the arguments of :func:`parameter_summaries`) on a
    ``shape`` = (nz, nn) grid per row.  ``grid``: (gz_lo, gz_hi, gn_lo, gn_hi) for all rows or [n, 4]; None:
    each row's search range and the range of ``log_nhi_samples``.  Returns, in (model, slot) order like the
    summaries, ``mass`` and ``hpd_level`` [n, models, models, nz, nn] (``with_maps``), ``outside``, ``mode``,
    ``hpd_cells`` and ``hpd_threshold`` (trailing axis: ``levels``), ``status`` [n, models] (bit 1: no usable
    sample; 4: bad grid; 8: a level not reached; 16: bad model weights); with ``model_weights`` [n, models]
    the absorber ``intensity`` [n, nz, nn] and ``expected_absorbers`` [n]; and, made here, ``grid``,
    ``edges_z`` [n, nz + 1], ``edges_log_nhi`` [n, nn + 1], ``marginal_z`` and ``marginal_log_nhi``."""
    shape, lv = check_maps_request(shape, levels)
    sll, base = _tables(sample_log_likelihoods, base_sample_inds)
    n, md, S = sll.shape
    z_min = np.ascontiguousarray(min_z_dlas, dtype=np.float64).reshape(-1)
    z_max = np.ascontiguousarray(max_z_dlas, dtype=np.float64).reshape(-1)
    off = np.ascontiguousarray(samples["offset_samples"], dtype=np.float64).reshape(-1)
    lnhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64).reshape(-1)
    if z_min.size != n or z_max.size != n:
        raise ValueError("min_z_dlas and max_z_dlas need one entry per row")
    if off.size != S or lnhi.size != S:
        raise ValueError(f"{S} sample columns but {off.size} offsets and {lnhi.size} log N_HI samples")
    g = default_grid(z_min, z_max, lnhi) if grid is None else _grid_rows(grid, n)
    w = None if model_weights is None else _weights_rows(model_weights, n, md)
    return finish_maps(_run_maps(sll, base, z_min, z_max, off, lnhi, g, w, shape, lv, with_maps, device), g, shape, lv)


def default_grid(z_min, z_max, lnhi):
    """[n, 4]: each row's search range and the range of the log N table."""
    n = len(z_min)
    return np.ascontiguousarray(np.stack([z_min, z_max, np.full(n, float(np.min(lnhi))), np.full(n, float(np.max(lnhi)))], axis=1))


def maps_from_processed_file(processed, samples_file, shape=(32, 32), selection=None, p_dla=None, sub_dla=False,
                             block_size=2048, grid=None, levels=DEFAULT_LEVELS, mix=True, with_maps=True, device=0) -> dict:
    """Posterior maps of a processed_qsos file, its tables streamed in quasar blocks as
    :func:`from_processed_file` streams them (at most two blocks on the host; results do not depend on
    ``block_size``).  ``grid``: one (gz_lo, gz_hi, gn_lo, gn_hi) for every quasar, or None (each quasar's
    search range, the range of the log N table).  ``mix``: the absorber intensity with the file's model
    posteriors of DLA(1 ..) as weights (``p_lls`` for ``sub_dla``, ``p_dlas`` where the file has no
    ``model_posteriors``).  Adds ``selection``."""
    from . import hdf5, io
    if block_size < 1:
        raise ValueError("block_size must be >= 1")
    shape, lv = check_maps_request(shape, levels)
    small = io.loadmat73(processed, ["min_z_dlas", "max_z_dlas", "p_dlas", "p_lls", "model_posteriors"])
    z_min = np.asarray(small["min_z_dlas"], dtype=np.float64).reshape(-1)
    z_max = np.asarray(small["max_z_dlas"], dtype=np.float64).reshape(-1)
    nq = z_min.size
    if selection is not None:
        sel = np.asarray(selection, dtype=np.int64).reshape(-1)
        if sel.size and (np.any(np.diff(sel) <= 0) or sel[0] < 0 or sel[-1] >= nq):
            raise ValueError(f"selection must increase strictly inside [0, {nq})")
    elif p_dla is not None:
        with np.errstate(invalid="ignore"):
            sel = np.flatnonzero(np.asarray(small["p_dlas"], dtype=np.float64).reshape(-1) >= p_dla)
    else:
        sel = np.arange(nq)
    samples = io.load_dla_samples(samples_file) if isinstance(samples_file, str) else samples_file
    if sub_dla:
        samples = sub_dla_samples(samples)
    off = np.ascontiguousarray(samples["offset_samples"], dtype=np.float64).reshape(-1)
    lnhi = np.ascontiguousarray(samples["log_nhi_samples"], dtype=np.float64).reshape(-1)
    g_all = default_grid(z_min, z_max, lnhi) if grid is None else _grid_rows(grid, nq)
    with hdf5.File(processed) as f:
        ds = f["sample_log_likelihoods_lls" if sub_dla else "sample_log_likelihoods_dla"]   # [S, nq] or [md, S, nq]
        md = ds.shape[0] if len(ds.shape) == 3 else 1
        S = ds.shape[-2]
        if off.size != S or lnhi.size != S:
            raise ValueError(f"the sample table has {S} columns, the samples {off.size}")
        w_all = None
        if mix:
            if sub_dla:
                w_all = np.asarray(small["p_lls"], dtype=np.float64).reshape(nq, 1)
            elif "model_posteriors" in small and np.asarray(small["model_posteriors"]).size == nq * (2 + md) and md > 1:
                mp = np.asarray(small["model_posteriors"], dtype=np.float64)
                w_all = (mp if mp.shape[0] == nq else mp.T)[:, 2:2 + md]
            else:
                w_all = np.asarray(small["p_dlas"], dtype=np.float64).reshape(nq, 1)
                if md != 1:
                    raise ValueError("mix needs the file's model_posteriors [quasars x (2 + models)]")
        db = f["base_sample_inds"] if md > 1 else None                                       # [md - 1, S, nq]
        parts = []
        i = 0
        while i < sel.size:  # one read per run of selected quasars within block_size of its first
            lo = int(sel[i])
            j = int(np.searchsorted(sel, lo + block_size))
            hi = int(sel[j - 1]) + 1
            cols = sel[i:j] - lo
            if len(ds.shape) == 2:
                sll = np.ascontiguousarray(ds.read_slab(0, S, axis1=(lo, hi))[:, cols].T)[:, None, :]
            else:
                sll = np.ascontiguousarray(
                    np.transpose(ds.read_slab(0, md, axis1=(0, S), axis2=(lo, hi))[:, :, cols], (2, 0, 1)))
            base = None
            if db is not None:
                base = np.ascontiguousarray(
                    np.transpose(db.read_slab(0, md - 1, axis1=(0, S), axis2=(lo, hi))[:, :, cols], (2, 0, 1)),
                    dtype=np.uint32)
            rows = sel[i:j]
            w = None if w_all is None else np.ascontiguousarray(w_all[rows])
            parts.append(_run_maps(np.ascontiguousarray(sll), base, np.ascontiguousarray(z_min[rows]),
                                   np.ascontiguousarray(z_max[rows]), off, lnhi, np.ascontiguousarray(g_all[rows]), w, shape,
                                   lv, with_maps, device))
            i = j
    if parts:
        out = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
    else:
        out, _ = maps_outputs(0, md, shape, len(lv), w_all is not None, with_maps)
    out = finish_maps(out, g_all[sel], shape, lv)
    out["selection"] = sel
    return out


def stack_intensity(result) -> dict:
    """The absorber intensity summed over the rows of a maps result: a non-parametric f(N, z) that uses every
    model.  Each cell is ``math.fsum`` over the rows in row order; rows of NaN intensity (bad grid or
    weights) are left out and counted.  Raises unless all rows share one grid.  Returns ``intensity``
    [nz, nn], ``expected_absorbers``, ``rows_used``, ``rows_skipped``, ``edges_z``, ``edges_log_nhi``."""
    import math
    if "intensity" not in result:
        raise ValueError("the result holds no intensity (no model weights were given)")
    grid = np.asarray(result["grid"], dtype=np.float64)
    inten = np.asarray(result["intensity"], dtype=np.float64)
    if grid.shape[0] == 0:
        raise ValueError("no rows to stack")
    if not np.array_equal(grid, np.tile(grid[0], (grid.shape[0], 1))):     # (a NaN grid never equals itself)
        raise ValueError("stack_intensity needs one grid shared by all rows")
    use = [r for r in range(inten.shape[0]) if not np.isnan(inten[r]).any()]
    nz, nn = inten.shape[1:]
    stacked = np.array([[math.fsum(inten[r, a, b] for r in use) for b in range(nn)] for a in range(nz)]).reshape(nz, nn)
    ea = np.asarray(result["expected_absorbers"], dtype=np.float64)
    return dict(intensity=stacked, expected_absorbers=math.fsum(ea[r] for r in use), rows_used=len(use),
                rows_skipped=inten.shape[0] - len(use), edges_z=np.asarray(result["edges_z"])[0],
                edges_log_nhi=np.asarray(result["edges_log_nhi"])[0])


def parse_shape(text: str):
    """``NZxNN`` of the command line."""
    parts = text.lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError(f"--maps takes NZxNN, e.g. 32x32; got {text!r}")
    return int(parts[0]), int(parts[1])


def quantile_key(name: str, p: float) -> str:
    """JSON / file key of a quantile: ``log_nhi_q0.025``, ``z_dla_q0.5`` ..."""
    return f"{name}_q{float(p):.6g}"


def threshold_key(t: float) -> str:
    return f"p_log_nhi_ge_{float(t):.6g}"


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gp_dla_detection_amd.posteriors", description=__doc__.split("\n\n")[0])
    ap.add_argument("processed")
    ap.add_argument("samples")
    ap.add_argument("out", help="summaries file (MATLAB v7.3)")
    ap.add_argument("--p-dla", type=float, default=None, help="only quasars with p_dlas >= this")
    ap.add_argument("--indices", type=int, nargs="*", default=None, help="0-based quasar indices, increasing")
    ap.add_argument("--probabilities", type=float, nargs="*", default=list(DEFAULT_PROBABILITIES))
    ap.add_argument("--thresholds", type=float, nargs="*", default=list(DEFAULT_THRESHOLDS))
    ap.add_argument("--sub-dla", action="store_true")
    ap.add_argument("--block-size", type=int, default=2048)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", default=None, help="also write the JSON catalogue with intervals here")
    ap.add_argument("--catalog", default=None, help="catalogue file with ras, decs, ... of the searched quasars (--json)")
    ap.add_argument("--maps", type=parse_shape, default=None, metavar="NZxNN",
                    help="also write posterior maps of (z_DLA, log N_HI) on this grid per quasar (DESIGN.md 4.22)")
    ap.add_argument("--levels", type=float, nargs="*", default=list(DEFAULT_LEVELS), help="credible masses of the HPD regions (--maps)")
    ap.add_argument("--map-range", type=float, nargs=4, default=None, metavar=("ZLO", "ZHI", "NLO", "NHI"),
                    help="one grid for every quasar (--maps; default: each search range, the log N range of the samples)")
    ap.add_argument("--no-cells", action="store_true", help="--maps: leave the per-cell arrays of the slots out")
    ap.add_argument("--maps-out", default=None, help="maps file (default: OUT with _maps before its extension)")
    return ap


def main(argv=None):
    import os

    from . import catalog, io
    a = build_parser().parse_args(argv)
    out = from_processed_file(a.processed, a.samples, selection=a.indices, p_dla=a.p_dla, sub_dla=a.sub_dla,
                              block_size=a.block_size, probabilities=a.probabilities, thresholds=a.thresholds,
                              device=a.device)
    io.save_parameter_summaries(a.out, out, processed_file=a.processed, sub_dla=float(a.sub_dla))
    print(f"{out['selection'].size} quasars x {out['status'].shape[1]} models -> {a.out}")
    if a.maps is not None:
        maps = maps_from_processed_file(a.processed, a.samples, shape=a.maps, selection=a.indices, p_dla=a.p_dla,
                                        sub_dla=a.sub_dla, block_size=a.block_size, grid=a.map_range, levels=a.levels,
                                        with_maps=not a.no_cells, device=a.device)
        stem, ext = os.path.splitext(a.out)
        maps_out = a.maps_out or f"{stem}_maps{ext}"
        io.save_posterior_maps(maps_out, maps, processed_file=a.processed, sub_dla=float(a.sub_dla))
        print(f"{maps['selection'].size} quasars, {a.maps[0]} x {a.maps[1]} cells -> {maps_out}")
    if a.json:
        if a.sub_dla:
            raise SystemExit("--json lists the DLAs of the most probable model: run without --sub-dla")
        if not a.catalog:
            raise SystemExit("--json needs --catalog")
        results = io.load_processed_qsos(a.processed)
        info = io.load_catalog(a.catalog, names=("ras", "decs", "plates", "mjds", "fiber_ids", "thing_ids", "z_qsos", "snrs"))
        if "test_ind" in results and len(info["z_qsos"]) != len(results["min_z_dlas"]):
            ti = np.asarray(results["test_ind"]).reshape(-1).astype(bool)
            info = {k: np.asarray(v).reshape(-1)[ti] for k, v in info.items()}
        recs = catalog.generate_json_catalogue_with_intervals(results, info, out, outfile=a.json)
        print(f"{len(recs)} records -> {a.json}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
