"""GPU checks of the posterior maps against the NumPy restatement
(tests/posterior_maps_restatement.py).

Set A (md = 4; grids 16 x 16 and 64 x 64) walks the sample counts that straddle the thread stride and the
1024-sample tile of k_posterior_maps; set B (S = 257, 1025; md = 1, 2, 4) the cell counts below, on and above
the 256 threads and the full 4096.  Every case holds the 13 rows of maps_case on their default grids, four
of them again on a grid over half the z range, on one that leaves the posterior peak out and on a reversed
/ NaN one, and the rows whose samples sit bitwise on edges.

Cell membership (mass > 0), the HPD outputs derived from the GPU's own masses, the mix of the GPU's own
masses and the status bits are exact.  mass and outside: tol = 10 x the restatement's float64-versus-
np.longdouble disagreement on the same inputs, floored at 1e-13 absolute.  Every figure is printed before
it is asserted."""
import ctypes as C

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, conditional, posteriors, synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import posterior_maps_restatement as M
import posterior_restatement as R
import refine_cases as RC

MAPS_API = (posteriors.posterior_maps, posteriors.stack_intensity, _lib.PosteriorMapsRequest)   # the feature under test

pytestmark = pytest.mark.gpu

S_SET_A = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 10004)
SHAPES_A = ((16, 16), (64, 64))
SHAPES_B = ((1, 1), (1, 64), (64, 1), (3, 5), (15, 17), (16, 16), (64, 64))
EXTRA = (0, 1, 2, 8)      # peaked, broad, flat, base_zeros: the rows that come again on the other grids
SLOT_KEYS = ("mass", "hpd_level", "outside", "mode", "hpd_cells", "hpd_threshold")
ALL_KEYS = SLOT_KEYS + ("intensity", "expected_absorbers", "status")
SUMMARY_KEYS = tuple(k for k in ALL_KEYS if k not in ("mass", "hpd_level"))
_INPUTS = {}


def _inputs(S, md):
    """The stacked table of one case: (sll, base, off, lnhi, z_min, z_max, grids, weights), once per (S, md)."""
    if (S, md) not in _INPUTS:
        sll, base, off, lnhi, z_min, z_max = M.maps_case(S, md)
        v = M.grid_variants(z_min, z_max, lnhi)
        nopeak = M.peak_excluding_grids(sll, base, off, lnhi, z_min, z_max)
        rows = np.concatenate([np.arange(sll.shape[0])] + [np.array(EXTRA)] * 3)
        grids = np.concatenate([v["full"], v["half"][list(EXTRA)], nopeak[list(EXTRA)], v["bad"][list(EXTRA)]])
        sll, z_min, z_max = sll[rows], z_min[rows], z_max[rows]
        base = None if base is None else base[rows]
        status = M.maps(sll, off, lnhi, z_min, z_max, grids, (1, 1), base)["status"]
        _INPUTS[(S, md)] = (np.ascontiguousarray(sll), None if base is None else np.ascontiguousarray(base), off, lnhi,
                            z_min, z_max, grids, M.weight_cases(status))
    return _INPUTS[(S, md)]


def _gpu(inp, shape, levels=M.LEVELS, weights=True, rows=slice(None), **kw):
    sll, base, off, lnhi, z_min, z_max, grids, w = inp
    return posteriors.posterior_maps(sll[rows], dict(offset_samples=off, log_nhi_samples=lnhi), z_min[rows], z_max[rows],
                                     None if base is None else base[rows], grid=grids[rows], shape=shape, levels=levels,
                                     model_weights=w[rows] if weights else None, **kw)


def _same(a, b, keys=ALL_KEYS, rows_a=slice(None), rows_b=slice(None)):
    for k in keys:
        np.testing.assert_array_equal(a[k][rows_a], b[k][rows_b], err_msg=k)   # NaN pattern included


def _check(got, inp, shape, label, levels=M.LEVELS, n_lo=None, n_hi=None):
    """Everything the issue asks of one call, against the restatement of the same inputs."""
    sll, base, off, lnhi, z_min, z_max, grids, w = inp
    f64 = M.maps(sll, off, lnhi, z_min, z_max, grids, shape, base, levels, model_weights=w, n_lo=n_lo, n_hi=n_hi)
    ext = M.maps(sll, off, lnhi, z_min, z_max, grids, shape, base, (), n_lo=n_lo, n_hi=n_hi, extended=True)
    tol, dis = M.mass_tolerance(f64, ext)
    np.testing.assert_array_equal(got["status"], f64["status"])
    np.testing.assert_array_equal(np.isnan(got["mass"]), np.isnan(f64["mass"]))
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(got["mass"] > 0, f64["mass"] > 0)      # cell membership: exact
        worst = max(np.nanmax(np.abs(got["mass"] - ext["mass"]), initial=0.0), np.nanmax(np.abs(got["outside"] - ext["outside"]), initial=0.0))
        total = got["mass"].sum(axis=(3, 4)) + got["outside"]
        closure = np.nanmax(np.abs(total - 1.0), initial=0.0)
    print(f"{label}: restatement f64 vs extended {dis:.2e}, tolerance {tol:.2e}, GPU worst {worst:.2e}, |sum + outside - 1| {closure:.2e}")
    np.testing.assert_array_equal(np.isnan(got["outside"]), np.isnan(f64["outside"]))
    assert worst <= tol and closure <= 1e-13
    # the HPD outputs and the mix: the contract applied to the GPU's own masses, bit for bit
    h = M.hpd_of(got["mass"], got["status"], levels)
    for k in ("hpd_level", "mode", "hpd_cells", "hpd_threshold"):
        np.testing.assert_array_equal(got[k], h[k], err_msg=k)
    np.testing.assert_array_equal((got["status"] & M.SHORT) != 0, h["short"])
    mx = M.mix_of(got["mass"], got["status"], w)
    np.testing.assert_array_equal(got["intensity"], mx["intensity"])
    np.testing.assert_array_equal(got["expected_absorbers"], mx["expected_absorbers"])
    np.testing.assert_array_equal((got["status"] & M.BAD_WEIGHTS) != 0, np.broadcast_to((mx["row_status"] != 0)[:, None], got["status"].shape))
    return f64


@pytest.mark.parametrize("shape", SHAPES_A, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("S", S_SET_A)
def test_set_a_sample_counts(S, shape):
    inp = _inputs(S, 4)
    got = _gpu(inp, shape)
    f64 = _check(got, inp, shape, f"S {S} md 4 grid {shape}")
    n0 = 13
    assert ((f64["status"][n0 + 8:] & M.BAD_GRID) != 0).all()
    if S >= 255:                                                            # (a handful of samples need not span a grid)
        assert ((f64["status"][:n0 + 8] & M.BAD_GRID) != 0).sum() == 2 * 4   # nan_max_z and zero_width alone
        with np.errstate(invalid="ignore"):
            assert (got["outside"][n0:n0 + 4] > 0.1).sum() >= 4              # the half grids leave mass outside
        assert got["status"][n0 + 4, 0] & M.SHORT                           # the peak of the peaked row is left out


@pytest.mark.parametrize("shape", SHAPES_B, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("md", (1, 2, 4))
@pytest.mark.parametrize("S", (257, 1025))
def test_set_b_cell_counts(S, md, shape):
    inp = _inputs(S, md)
    _check(_gpu(inp, shape), inp, shape, f"S {S} md {md} grid {shape}")


def test_samples_on_edges():
    sll, base, off, lnhi, z_min, z_max, grids, on_edge = M.edge_case()
    assert on_edge.sum() >= 50
    n, md = sll.shape[:2]
    w = np.full((n, md), 0.5)
    inp = (sll, base, off, lnhi, z_min, z_max, grids, w)
    got = _gpu(inp, (8, 5))
    f64 = _check(got, inp, (8, 5), "edge samples, 8 x 5")
    # slot 1 of model 1 reads the samples themselves: every cell that holds only on-edge samples is where the
    # restatement's searchsorted put it (membership above), and the flat row ties three cells or more
    flat = got["mass"][2, 0, 0].reshape(-1)
    assert np.unique(flat[flat > 0], return_counts=True)[1].max() >= 3
    np.testing.assert_array_equal(got["mode"], f64["mode"])
    np.testing.assert_array_equal(got["hpd_cells"][2], f64["hpd_cells"][2])


def test_mass_above_a_threshold_equals_the_summaries_exceedance():
    """An independent kernel: on a grid whose log N axis starts at 20.3 and ends above every sample, over the
    search range, the mass inside is k_parameter_summaries' P(log N >= 20.3)."""
    checked = 0
    for S, md in ((257, 2), (1025, 4)):
        sll, base, off, lnhi, z_min, z_max = M.maps_case(S, md)
        n = sll.shape[0]
        grids = np.stack([z_min, z_max, np.full(n, 20.3), np.full(n, 23.5)], axis=1)
        assert lnhi.max() < 23.5
        smp = dict(offset_samples=off, log_nhi_samples=lnhi)
        got = posteriors.posterior_maps(sll, smp, z_min, z_max, base, grid=grids, shape=(5, 7), levels=())
        summ = posteriors.parameter_summaries(sll, smp, z_min, z_max, base, probabilities=(), thresholds=(20.3,))
        for r in range(n):
            for m in range(md):
                if got["status"][r, m] or summ["status"][r, m]:
                    continue
                for j in range(m + 1):
                    _, z, _ = R.slot_table(sll, off, lnhi, z_min, z_max, base, r, m + 1, j)
                    if not np.all((z >= z_min[r]) & (z <= z_max[r])):
                        continue
                    inside = got["mass"][r, m, j].sum()
                    assert abs(inside - summ["exceedance"][r, m, j, 0]) <= 1e-13, (S, md, r, m, j)
                    assert abs(inside + got["outside"][r, m, j] - 1.0) <= 1e-13
                    checked += 1
    print(f"{checked} (row, model, slot) sums compared with the exceedance")
    assert checked >= 100


@pytest.mark.parametrize("S,md,shape", [(257, 2, (15, 17)), (1025, 4, (64, 64))])
def test_rows_do_not_depend_on_selection_order_blocking_or_run(S, md, shape):
    inp = _inputs(S, md)
    n = inp[0].shape[0]
    whole = _gpu(inp, shape)
    _same(_gpu(inp, shape), whole)
    rev = slice(None, None, -1)
    _same(_gpu(inp, shape, rows=rev), whole, rows_a=rev)
    pick = np.array([7, 3, 20, 3])
    _same(_gpu(inp, shape, rows=pick), whole, rows_b=pick)
    for r in (0, 4, 12, n - 1):
        _same(_gpu(inp, shape, rows=slice(r, r + 1)), whole, rows_b=slice(r, r + 1))
    _same(_gpu(inp, shape, with_maps=False), whole, SUMMARY_KEYS)
    assert "mass" not in _gpu(inp, shape, with_maps=False)
    # a strided table (rows of a wider array) is packed by the library
    sll, base, off, lnhi, z_min, z_max, grids, w = inp
    wide = np.full((n, md * S + 3), 7.0)
    wide[:, :md * S] = sll.reshape(n, -1)
    out, pm = posteriors.maps_outputs(n, md, shape, len(M.LEVELS), True, True)
    rq = posteriors.maps_request(md, shape, list(M.LEVELS))
    cols = posteriors._grid_columns(grids)
    _lib.check(_lib.load().gpdla_stats_posterior_maps(
        n, S, _lib.ptr(wide), wide.shape[1], base.ctypes.data_as(_lib._u32p), _lib.ptr(z_min), _lib.ptr(z_max), _lib.ptr(off),
        _lib.ptr(lnhi), *[_lib.ptr(c) for c in cols], _lib.ptr(w), C.byref(rq), C.byref(pm), 0))
    _same(out, whole)


def test_the_seam_between_two_launches():
    lib = _lib.load()
    shape, md, S = (64, 64), 4, 64
    per = lib.gpdla_posterior_maps_rows_per_launch(md, *shape)
    n = per + 11
    sll, base, off, lnhi, z_min, z_max = R.make_case(S, md)
    rows = np.random.default_rng(9).permutation(np.arange(n) % 12)
    smp = dict(offset_samples=off, log_nhi_samples=lnhi)
    grids = M.default_grids(z_min, z_max, lnhi)[rows]
    w = np.random.default_rng(10).random((n, md))
    big = posteriors.posterior_maps(sll[rows], smp, z_min[rows], z_max[rows], base[rows], grid=grids, shape=shape,
                                    levels=M.LEVELS, model_weights=w)
    launches = lib.gpdla_debug_last_maps_launches()
    print(f"{n} rows, {per} per launch: {launches} launches")
    assert launches >= 2
    for r in range(per - 2, per + 2):
        one = posteriors.posterior_maps(sll[rows[r:r + 1]], smp, z_min[rows[r:r + 1]], z_max[rows[r:r + 1]], base[rows[r:r + 1]],
                                        grid=grids[r:r + 1], shape=shape, levels=M.LEVELS, model_weights=w[r:r + 1])
        assert lib.gpdla_debug_last_maps_launches() == 1
        _same(one, big, rows_b=slice(r, r + 1))


# ---- resident forms ----

def test_resident_single_dla_batch_equals_the_host_form():
    model, samples = synthetic.make_model(20), synthetic.make_samples(300)
    spectra = [synthetic.make_spectrum(70 + i, n, model, mask_fraction=0.05 if i else 0.0) for i, n in enumerate([250, 301, 280])]
    ctx = gp.Context(0, Parameters())
    ctx.set_model(model)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra, np.full(3, np.log(0.9)), np.full(3, np.log(0.1)))
    try:
        batch.process()
        res = batch.download()
        resident = batch.posterior_maps(shape=(16, 12))
        picked = batch.posterior_maps(selection=[2, 0], shape=(16, 12))
        lean = batch.posterior_maps(shape=(16, 12), with_maps=False)
        # the library's own defaults (NULL grid arrays, NULL weights with mix set)
        own, pm = posteriors.maps_outputs(3, 1, (16, 12), len(posteriors.DEFAULT_LEVELS), True, True)
        rq = posteriors.maps_request(1, (16, 12), list(posteriors.DEFAULT_LEVELS), mix=True)
        _lib.check(ctx.lib.gpdla_batch_posterior_maps(ctx._h, batch._h, 0, 0, None, 3, None, None, None, None, None, C.byref(rq),
                                                      C.byref(pm)))
    finally:
        batch.close()
        ctx.close()
    lnhi = np.asarray(samples["log_nhi_samples"])
    np.testing.assert_array_equal(resident["grid"], posteriors.default_grid(res["min_z_dlas"], res["max_z_dlas"], lnhi))
    host = posteriors.posterior_maps(res["sample_log_likelihoods_dla"], samples, res["min_z_dlas"], res["max_z_dlas"],
                                     grid=resident["grid"], shape=(16, 12), model_weights=res["p_dlas"])
    _same(resident, host, ALL_KEYS + ("edges_z", "edges_log_nhi", "marginal_z", "marginal_log_nhi"))
    _same(picked, host, rows_b=[2, 0])
    _same(lean, host, SUMMARY_KEYS)
    _same(own, host)
    assert (host["status"] == 0).all() and np.all(np.abs(host["expected_absorbers"] - res["p_dlas"] * (1 - host["outside"][:, 0, 0])) < 1e-12)


def test_resident_multi_dla_batch_equals_the_host_form():
    p = MultiParameters(max_dlas=3)
    model, samples = synthetic.make_model(20), synthetic.make_samples(200)
    spectra = [synthetic.make_spectrum(80 + i, n, model, mask_fraction=0.04) for i, n in enumerate([260, 301])]
    ctx = gp.Context(0, p)
    ctx.set_model(model)
    ctx.set_samples(samples)
    lp_dla = np.log(np.full((2, 3), 0.1) ** np.arange(1, 4))
    batch = ctx.upload(spectra, np.full(2, np.log(0.85)), lp_dla, np.full(2, np.log(0.05)))
    try:
        batch.process_multi()
        res = batch.download_multi()
        resident = batch.posterior_maps(multi=True, shape=(9, 64))
        swapped = batch.posterior_maps(selection=[1, 0], multi=True, shape=(9, 64))
        sub = batch.posterior_maps(multi=True, sub_dla=True, shape=(9, 64))
    finally:
        batch.close()
        ctx.close()
    weights = np.asarray(res["model_posteriors"])[:, 2:5]        # DLA(1 .. 3): the default weights
    host = posteriors.posterior_maps(res["sample_log_likelihoods_dla"], samples, res["min_z_dlas"], res["max_z_dlas"],
                                     res["base_sample_inds"], grid=resident["grid"], shape=(9, 64), model_weights=weights)
    _same(resident, host)
    _same(swapped, host, rows_b=[1, 0])
    assert host["status"].shape == (2, 3) and (host["status"] & ~M.SHORT == 0).all()
    assert np.isnan(host["mass"][:, 0, 1:]).all() and not np.isnan(host["mass"][:, 2]).any()
    sub_smp = posteriors.sub_dla_samples(samples)
    sub_host = posteriors.posterior_maps(res["sample_log_likelihoods_lls"], sub_smp, res["min_z_dlas"], res["max_z_dlas"],
                                         grid=sub["grid"], shape=(9, 64), model_weights=res["p_lls"])
    _same(sub, sub_host)
    lls = sub_smp["log_nhi_samples"]
    assert np.allclose(sub["grid"][:, 2], lls.min(), rtol=1e-15) and np.allclose(sub["grid"][:, 3], lls.max(), rtol=1e-15)


def _refined_batch(**params):
    k, nl = RC.CONFIGS[0]
    model, samples, spectra, truth = RC.make_batch(k, nl)
    ctx = gp.Context(0, Parameters(num_lines=nl, **params))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(128))
    n = len(spectra)
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1))), samples


def _host_refined(full, levels, shape, weights, grid=None):
    u, v = RC.halton_points(128)
    box = np.ascontiguousarray(full["boxes"][:, -1])
    return box, _refined_host_call(full["sample_log_posteriors_refined"], u, v, box, box if grid is None else grid, shape, levels, weights)


def _refined_host_call(lam, u, v, box, grid, shape, levels, weights):
    """The host entry has no affine reading of log N: the restatement's (n_lo, n_hi) form is what the refined
    entry computes, so the host form is fed log N = n_lo + (n_hi - n_lo) v row by row."""
    parts = []
    for i in range(lam.shape[0]):
        with np.errstate(invalid="ignore"):
            ln = box[i, 2] + (box[i, 3] - box[i, 2]) * v
        if not np.all(np.isfinite(ln)):       # an unusable row: its box is NaN, and so is every output
            ln = v
        parts.append(posteriors.posterior_maps(lam[i:i + 1], dict(offset_samples=u, log_nhi_samples=ln), box[i:i + 1, 0], box[i:i + 1, 1],
                                               grid=grid[i:i + 1], shape=shape, levels=levels, model_weights=weights[i:i + 1]))
    return {k: np.concatenate([p[k] for p in parts]) for k in ALL_KEYS}


def test_refined_and_conditioned_batches():
    shape, levels = (32, 32), (0.5, 0.95)
    ctx, batch, samples = _refined_batch()
    try:
        batch.process()
        res = batch.download()
        first = batch.posterior_maps(shape=shape, levels=levels)
        full = batch.refine(levels=RC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        ref = batch.posterior_maps(refined=True, shape=shape, levels=levels)
        picked = batch.posterior_maps(refined=True, shape=shape, levels=levels, selection=[3, 0])
        # a conditioned batch is served as it is
        i = RC.KINDS.index("strong")
        lists = [[] for _ in RC.KINDS]
        lists[i] = [(float(full["MAP_z_dlas_refined"][i]), float(full["MAP_log_nhis_refined"][i]))]
        batch.set_fixed_absorbers(conditional.csr_of(lists))
        batch.process()
        cres = batch.download()
        cond = batch.posterior_maps(shape=shape, levels=levels)
        cfull = batch.refine(levels=RC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        cref = batch.posterior_maps(refined=True, shape=shape, levels=levels)
    finally:
        batch.close()
        ctx.close()
    box, host = _host_refined(full, levels, shape, res["p_dlas"][:, None])
    np.testing.assert_array_equal(ref["grid"], box)             # the default grid: the quasar's last box
    _same(ref, host)
    _same(picked, host, rows_b=[3, 0])
    usable = full["status"] == 0
    assert usable.sum() >= 5 and (ref["status"][~usable, 0] & (M.UNUSABLE | M.BAD_GRID) != 0).all()
    # the 0.95 region holds the refined MAP's cell
    for q in np.flatnonzero(usable):
        cz = M.cells_of(full["MAP_z_dlas_refined"][q:q + 1], box[q, 0], box[q, 1], shape[0])[0]
        cn = M.cells_of(full["MAP_log_nhis_refined"][q:q + 1], box[q, 2], box[q, 3], shape[1])[0]
        assert cz >= 0 and cn >= 0
        if ref["status"][q, 0] & M.SHORT:
            continue
        lv = ref["hpd_level"][q, 0, 0]
        with np.errstate(invalid="ignore"):
            reached = lv[lv >= 0.95]                              # C at the rank that closes the region, and beyond
        assert reached.size and lv[cz, cn] <= reached.min(), RC.KINDS[q]
    # purpose: a strong row's first-pass 0.95 region is one cell, the refined one is more
    for kind in RC.PEAKED:
        q = RC.KINDS.index(kind)
        print(f"{kind}: first-pass 0.95 region {first['hpd_cells'][q, 0, 0, 1]} cells, refined {ref['hpd_cells'][q, 0, 0, 1]} cells")
        assert first["hpd_cells"][q, 0, 0, 1] == 1 and ref["hpd_cells"][q, 0, 0, 1] > 1
    # the conditioned batch: the same entries on its own tables
    chost = posteriors.posterior_maps(cres["sample_log_likelihoods_dla"], samples, cres["min_z_dlas"], cres["max_z_dlas"],
                                      grid=cond["grid"], shape=shape, levels=levels, model_weights=cres["p_dlas"])
    _same(cond, chost)
    cbox, chost_ref = _host_refined(cfull, levels, shape, cres["p_dlas"][:, None])
    _same(cref, chost_ref)
    assert not np.array_equal(cref["mass"][i], ref["mass"][i])   # (it is another posterior: one more absorber)


def test_refusals_of_the_resident_entries():
    ctx, batch, _ = _refined_batch(contraction_precision=1)      # the fp32 study class
    try:
        batch.process()
        with pytest.raises(_lib.GpdlaError, match="fp64 only") as e:
            batch.posterior_maps(refined=True, grid=(2.0, 3.0, 20.0, 23.0))
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        batch.close()
        ctx.close()
    ctx, batch, _ = _refined_batch()
    try:
        with pytest.raises(_lib.GpdlaError, match="not been processed"):
            batch.posterior_maps()
        batch.process()
        with pytest.raises(_lib.GpdlaError, match="not been refined"):
            batch.posterior_maps(refined=True)
        with pytest.raises(_lib.GpdlaError, match="multi = 0"):
            batch.posterior_maps(multi=True, num_models=1)
        with pytest.raises(ValueError, match="selection"):
            batch.posterior_maps(selection=[len(RC.KINDS)])
        with pytest.raises(_lib.GpdlaError, match="all four or none"):
            rq = posteriors.maps_request(1, (4, 4), [0.5])
            out, pm = posteriors.maps_outputs(1, 1, (4, 4), 1, False, False)
            _lib.check(ctx.lib.gpdla_batch_posterior_maps(ctx._h, batch._h, 0, 0, None, 1, _lib.ptr(np.ones(1)), None, None, None, None,
                                                          C.byref(rq), C.byref(pm)))
    finally:
        batch.close()
        ctx.close()
    model, samples, spectra, _ = RC.make_batch(8, 3)
    ctx = gp.Context(0, MultiParameters(max_dlas=2))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(16))
    batch = ctx.upload(spectra[:2], np.full(2, np.log(0.8)), np.log(np.full((2, 2), 0.1)), np.full(2, np.log(0.05)))
    try:
        batch.process_multi()
        rq = posteriors.maps_request(1, (4, 4), [0.5])
        out, pm = posteriors.maps_outputs(2, 1, (4, 4), 1, False, False)
        rc = ctx.lib.gpdla_batch_refined_posterior_maps(ctx._h, batch._h, None, 2, None, None, None, None, None, C.byref(rq), C.byref(pm))
        assert rc == _lib.ERR_UNSUPPORTED and b"single-DLA" in ctx.lib.gpdla_last_error()
        with pytest.raises(ValueError, match="refined=True"):
            batch.posterior_maps(refined=True, multi=True)
    finally:
        batch.close()
        ctx.close()


def test_purpose_expected_absorbers_of_a_two_absorber_sightline():
    """A multi-DLA batch of sightlines that hold more than one absorber: on a grid over log N >= 20.3 the expected number of
    absorbers is Sum_m P(m) m restricted to the same cut, computed from the downloaded tables by the
    restatement, to 0.05."""
    p = MultiParameters(max_dlas=3)
    model, samples = synthetic.make_model(20), synthetic.make_samples(200)
    spectra = []
    for i, n in enumerate([300, 320]):
        sp = synthetic.make_spectrum(91 + 2 * i, n, model, p)    # odd index: an absorber of its own; two more are put in
        wl = sp["wavelengths"]
        rest = wl / (1 + sp["z_qso"])
        inside = wl[(rest >= p.min_lambda) & (rest <= p.max_lambda)]
        zmin, zmax = p.min_z_dla(inside, sp["z_qso"]), p.max_z_dla(inside, sp["z_qso"])
        for f, ln in ((0.3, 21.0), (0.7, 20.8)):
            sp["flux"] = sp["flux"] * synthetic._injected_absorption(wl, zmin + f * (zmax - zmin), 10.0 ** ln, p.num_lines)
        spectra.append(sp)
    ctx = gp.Context(0, p)
    ctx.set_model(model)
    ctx.set_samples(samples)
    lp_dla = np.log(np.full((2, 3), 0.1) ** np.arange(1, 4))
    batch = ctx.upload(spectra, np.full(2, np.log(0.85)), lp_dla, np.full(2, np.log(0.05)))
    try:
        batch.process_multi()
        res = batch.download_multi()
        n = 2
        grid = np.stack([res["min_z_dlas"], res["max_z_dlas"], np.full(n, 20.3), np.full(n, 23.5)], axis=1)
        got = batch.posterior_maps(multi=True, grid=grid, shape=(32, 16))
    finally:
        batch.close()
        ctx.close()
    post = np.asarray(res["model_posteriors"])[:, 2:5]
    ref = M.maps(res["sample_log_likelihoods_dla"], samples["offset_samples"], samples["log_nhi_samples"], res["min_z_dlas"],
                 res["max_z_dlas"], grid, (1, 1), res["base_sample_inds"])
    # Sum_m P(m) x (the expected number of model m's absorbers above the cut) = Sum_m P(m) Sum_j (1 - outside)
    want = np.array([sum(post[r, m] * sum(1.0 - ref["outside"][r, m, j] for j in range(m + 1)) for m in range(3)) for r in range(n)])
    print(f"P(m) {post}, expected absorbers {got['expected_absorbers']}, Sum_m P(m) m above the cut {want}")
    assert np.all(np.abs(got["expected_absorbers"] - want) <= 0.05)
    assert np.all((got["expected_absorbers"] >= 0.0) & (got["expected_absorbers"] <= 3.0 + 1e-12))


def test_command_line_on_a_processed_multi_dla_file(tmp_path):
    """python -m gp_dla_detection_amd.posteriors --maps, in process, on a processed multi-DLA file (the
    committed consumer chunks, combined) with a block size that splits the run: equal to the in-memory path."""
    import glob
    import os

    from gp_dla_detection_amd import io
    cons = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consumer")
    processed = str(tmp_path / "processed.mat")
    io.combine_processed_chunks(sorted(glob.glob(os.path.join(cons, "processed_qsos_multi_meanfluxsynth_[0-9]*.mat"))), processed)
    inputs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=40, num_samples=24, empty_quasar=None)
    out = str(tmp_path / "summaries.mat")
    assert posteriors.main([processed, inputs["paths"]["samples"], out, "--block-size", "7", "--maps", "12x9", "--levels", "0.5",
                            "0.9"]) == 0
    res = io.load_processed_qsos(processed)
    smp = io.load_dla_samples(inputs["paths"]["samples"])
    md = res["sample_log_likelihoods_dla"].shape[1]
    want = posteriors.posterior_maps(res["sample_log_likelihoods_dla"], smp, res["min_z_dlas"], res["max_z_dlas"],
                                     res["base_sample_inds"], shape=(12, 9), levels=(0.5, 0.9),
                                     model_weights=np.asarray(res["model_posteriors"])[:, 2:2 + md])
    back = io.load_posterior_maps(str(tmp_path / "summaries_maps.mat"))
    _same(back, want, ALL_KEYS + ("grid", "edges_z", "edges_log_nhi", "marginal_z", "marginal_log_nhi", "levels", "shape"))
    np.testing.assert_array_equal(back["selection"], np.arange(len(res["min_z_dlas"])))
    one = posteriors.maps_from_processed_file(processed, smp, shape=(12, 9), levels=(0.5, 0.9), block_size=1000)
    _same(one, want)
    st = posteriors.stack_intensity(posteriors.maps_from_processed_file(processed, smp, shape=(12, 9), grid=(2.0, 5.0, 20.0, 23.0),
                                                                        with_maps=False))
    assert st["rows_used"] > 0 and st["intensity"].shape == (12, 9) and np.isfinite(st["expected_absorbers"])
