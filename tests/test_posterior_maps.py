"""CPU checks of the posterior maps: the NumPy restatement (tests/posterior_maps_restatement.py)
against Python loops with math.fsum and a linear search over the edges, on tiny tables -- cells, mode, ranks
and hpd_cells exact, masses and levels to 1e-13 -- and what needs no GPU: the argument checks of the three
entries, stack_intensity, the io round trip and the command line's parser."""
import ctypes as C

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, io, posteriors

import posterior_maps_restatement as M
import posterior_restatement as R

MAPS_API = (posteriors.posterior_maps, posteriors.stack_intensity, _lib.PosteriorMapsRequest)   # the feature under test


def _cases():
    """(name, sll, base, offsets, lnhi, z_min, z_max, grids, shape) of the tiny tables."""
    out = []
    for S, md, shape in ((24, 1, (3, 5)), (40, 2, (4, 4)), (33, 3, (1, 7))):
        sll, base, off, lnhi, z_min, z_max = M.maps_case(S, md)
        for name, g in M.grid_variants(z_min, z_max, lnhi).items():
            out.append((f"S{S}md{md}{name}", sll, base, off, lnhi, z_min, z_max, g, shape))
        out.append((f"S{S}md{md}nopeak", sll, base, off, lnhi, z_min, z_max,
                    M.peak_excluding_grids(sll, base, off, lnhi, z_min, z_max), shape))
    sll, base, off, lnhi, z_min, z_max, grids, _ = M.edge_case()
    out.append(("edges", sll, base, off, lnhi, z_min, z_max, grids, (8, 5)))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_against_python_loops(case):
    _, sll, base, off, lnhi, z_min, z_max, grids, shape = case
    got = M.maps(sll, off, lnhi, z_min, z_max, grids, shape, base, M.LEVELS)
    n, md, S = sll.shape
    nz, nn = shape
    compared = 0
    for r in range(n):
        ok = M.grid_ok(grids[r])
        for m in range(1, md + 1):
            tab = R.slot_table(sll, off, lnhi, z_min, z_max, base, r, m, 0)
            assert bool(got["status"][r, m - 1] & M.UNUSABLE) == (tab is None)
            assert bool(got["status"][r, m - 1] & M.BAD_GRID) == (not ok)
            if tab is None or not ok:
                assert np.isnan(got["mass"][r, m - 1]).all() and np.isnan(got["outside"][r, m - 1]).all()
                assert (got["mode"][r, m - 1] == -1).all() and (got["hpd_cells"][r, m - 1] == -1).all()
                continue
            short = False
            for j in range(m):
                w, z, ln = R.slot_table(sll, off, lnhi, z_min, z_max, base, r, m, j)
                mass, outside, level, mode, ranks, hc, cell = M.brute_slot(w, z, ln, grids[r], nz, nn, M.LEVELS)
                # cells: exact
                cz, cn = M.cells_of(z, grids[r, 0], grids[r, 1], nz), M.cells_of(ln, grids[r, 2], grids[r, 3], nn)
                np.testing.assert_array_equal(np.where((cz < 0) | (cn < 0), -1, cz * nn + cn), cell)
                at = (r, m - 1, j)
                gm = got["mass"][at].reshape(-1)
                np.testing.assert_array_equal(gm > 0, mass > 0)
                assert np.max(np.abs(gm - mass)) <= 1e-13 and abs(got["outside"][at] - outside) <= 1e-13
                assert abs(gm.sum() + got["outside"][at] - 1.0) <= 1e-13
                # mode, ranks and hpd_cells: exact (the restatement's order of its own masses is the loops' order of theirs
                # unless two masses that differ by rounding swap; the cases hold none)
                assert got["mode"][at] == mode
                gl = got["hpd_level"][at].reshape(-1)
                np.testing.assert_array_equal(np.isnan(gl), np.isnan(level))
                mine = sorted(np.flatnonzero(gm > 0), key=lambda c: (gl[c], c))
                assert [int(c) for c in mine] == ranks
                assert np.nanmax(np.abs(gl - level), initial=0.0) <= 1e-13
                assert list(got["hpd_cells"][at]) == hc
                for q, k in enumerate(hc):
                    assert np.isnan(got["hpd_threshold"][at + (q,)]) if k == 0 else got["hpd_threshold"][at + (q,)] == gm[ranks[k - 1]]
                short |= any((not ranks) or level[ranks[-1]] < p for p in M.LEVELS)
                compared += 1
            assert bool(got["status"][r, m - 1] & M.SHORT) == short
    assert compared > 0 or case[0].endswith("bad")      # (on the reversed / NaN grids nothing is left to compare)


def test_samples_on_edges_open_their_cell_and_the_value_below_closes_the_one_before():
    sll, base, off, lnhi, z_min, z_max, grids, on_edge = M.edge_case()
    nz, nn = 8, 5
    z = 2.0 + 1.0 * off
    ez, en = M.edges(2.0, 3.0, nz), M.edges(20.0, 23.0, nn)
    cz, cn = M.cells_of(z, 2.0, 3.0, nz), M.cells_of(lnhi, 20.0, 23.0, nn)
    n_on = int(on_edge.sum())
    assert n_on >= 50
    seen_hi = 0
    for i in np.flatnonzero(on_edge):
        below = i + n_on                                  # the same sample one double below the edge
        if z[i] in ez:
            c = int(np.flatnonzero(ez == z[i])[0])
            assert cz[i] == min(c, nz - 1)                # opens its cell; hi itself falls in the last
            assert cz[below] == c - 1                     # closes the cell before (-1: below the grid)
            seen_hi += c == nz
        else:
            k = int(np.flatnonzero(en == lnhi[i])[0])
            assert lnhi[i] in en and cn[i] == min(k, nn - 1)
            assert cn[below] == k - 1
            seen_hi += k == nn
    assert seen_hi >= 2
    # a flat row: exact ties, so the region goes by index
    got = M.maps(sll, off, lnhi, z_min, z_max, grids, (nz, nn), base, M.LEVELS)
    flat = got["mass"][2, 0, 0].reshape(-1)
    values, counts = np.unique(flat[flat > 0], return_counts=True)
    assert counts.max() >= 3, "the flat row must hold a tie of three or more cells"
    level = got["hpd_level"][2, 0, 0].reshape(-1)
    tied = np.flatnonzero(flat == values[np.argmax(counts)])
    assert np.all(np.diff(level[tied]) > 0)               # among equal masses the smaller index ranks first


def test_the_case_set_is_not_vacuous():
    sll, base, off, lnhi, z_min, z_max = M.maps_case(40, 2)
    g = M.grid_variants(z_min, z_max, lnhi)
    half = M.maps(sll, off, lnhi, z_min, z_max, g["half"], (4, 4), base, M.LEVELS)
    assert np.nansum(half["outside"] > 0.1) >= 5
    bad = M.maps(sll, off, lnhi, z_min, z_max, g["bad"], (4, 4), base, M.LEVELS)
    assert ((bad["status"] & M.BAD_GRID) != 0).all() and np.isnan(bad["mass"]).all()
    nopeak = M.maps(sll, off, lnhi, z_min, z_max, M.peak_excluding_grids(sll, base, off, lnhi, z_min, z_max), (4, 4), base, M.LEVELS)
    k = R.ROW_KINDS.index("peaked")
    assert nopeak["status"][k, 0] & M.SHORT and nopeak["outside"][k, 0, 0] > 0.99
    full = M.maps(sll, off, lnhi, z_min, z_max, g["full"], (4, 4), base, M.LEVELS)
    w = M.weight_cases(full["status"])
    mixed = M.maps(sll, off, lnhi, z_min, z_max, g["full"], (4, 4), base, M.LEVELS, model_weights=w)
    bit16 = (mixed["status"] & M.BAD_WEIGHTS) != 0
    assert bit16[0].all() and bit16[1].all() and bit16[-1].all() and bit16.all(axis=1).sum() == 3
    k = R.ROW_KINDS.index("all_nan")                      # zero weights on its unusable models: legal, an empty sum
    assert not bit16[k].any() and mixed["expected_absorbers"][k] == 0.0
    ok = ~bit16.any(axis=1) & ((mixed["status"] & M.BAD_GRID) == 0).all(axis=1)
    assert ok.sum() >= 6 and np.isfinite(mixed["expected_absorbers"][ok]).all()
    assert np.isnan(mixed["intensity"][~ok]).all()


# ---- the three entries refuse a bad request before they touch the device ----

def _host_call(lib, rq, n=2, S=5, md=1, grid=True, weights=False, intensity=False, base=None, off=None):
    sll = np.zeros((n, md, S))
    z = np.ones(n)
    off = np.linspace(0.0, 0.9, S) if off is None else off
    lnhi = np.linspace(20.0, 22.0, S)
    g = [_lib.ptr(np.ones(n)) for _ in range(4)] if grid else [None] * 4
    out, pm = posteriors.maps_outputs(n, md, (max(1, min(rq.nz, 64)), max(1, min(rq.nn, 64))), 0, intensity, False)
    bp = base.ctypes.data_as(_lib._u32p) if base is not None else None
    w = _lib.ptr(np.ones((n, md))) if weights else None
    return lib.gpdla_stats_posterior_maps(n, S, _lib.ptr(sll), md * S, bp, _lib.ptr(z), _lib.ptr(z), _lib.ptr(off), _lib.ptr(lnhi),
                                          *g, w, C.byref(rq), C.byref(pm), 0)


def test_argument_validation_needs_no_gpu():
    _lib.build()
    lib = _lib.load()
    err = lambda: lib.gpdla_last_error().decode()   # noqa: E731
    good = posteriors.maps_request(1, (4, 4), [0.5, 0.9])
    bad_requests = []
    for field, value in (("num_models", 0), ("num_models", 5), ("nz", 0), ("nz", 65), ("nn", 0), ("nn", 65), ("num_levels", 9),
                         ("num_levels", -1)):
        rq = posteriors.maps_request(1, (4, 4), [0.5, 0.9])
        setattr(rq, field, value)
        bad_requests.append((rq, field))
    for lv, word in (([0.0], "levels[0]"), ([0.5, 1.0], "levels[1]"), ([0.5, 0.5], "increase"), ([float("nan")], "levels[0]")):
        bad_requests.append((posteriors.maps_request(1, (4, 4), lv), word))
    out, pm = posteriors.maps_outputs(1, 1, (4, 4), 2, False, False)
    sel = np.zeros(1, dtype=np.int64)
    for rq, word in bad_requests:
        calls = (lambda: _host_call(lib, rq),
                 lambda: lib.gpdla_batch_posterior_maps(None, None, 0, 0, sel.ctypes.data_as(_lib._i64p), 1, None, None, None, None,
                                                        None, C.byref(rq), C.byref(pm)),
                 lambda: lib.gpdla_batch_refined_posterior_maps(None, None, sel.ctypes.data_as(_lib._i64p), 1, None, None, None, None,
                                                                None, C.byref(rq), C.byref(pm)))
        for call in calls:
            assert call() == _lib.ERR_INVALID_ARGUMENT and word in err(), (word, err())
    # a good request on no batch is refused too
    assert lib.gpdla_batch_posterior_maps(None, None, 0, 0, None, 0, None, None, None, None, None, C.byref(good), C.byref(pm)) \
        == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_batch_refined_posterior_maps(None, None, None, 0, None, None, None, None, None, C.byref(good), C.byref(pm)) \
        == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_stats_posterior_maps(1, 5, None, 5, None, None, None, None, None, None, None, None, None, None, None, None, 0) \
        == _lib.ERR_INVALID_ARGUMENT and "request" in err()
    # the host entry: sample-table size, index range, finiteness, grid arrays, weights
    assert _host_call(lib, good, S=0) == _lib.ERR_INVALID_ARGUMENT and "num_samples" in err()
    assert _host_call(lib, good, grid=False) == _lib.ERR_INVALID_ARGUMENT and "grid_z_lo" in err()
    assert _host_call(lib, good, intensity=True) == _lib.ERR_INVALID_ARGUMENT and "model_weights" in err()
    two = posteriors.maps_request(2, (4, 4), [0.5])
    assert _host_call(lib, two, md=2) == _lib.ERR_INVALID_ARGUMENT and "base_sample_inds" in err()
    base = np.full((2, 1, 5), 6, dtype=np.uint32)
    assert _host_call(lib, two, md=2, base=base) == _lib.ERR_INVALID_ARGUMENT and "exceeds num_samples" in err()
    off = np.linspace(0.0, 0.9, 5)
    off[3] = np.inf
    assert _host_call(lib, good, off=off) == _lib.ERR_INVALID_ARGUMENT and "offset_samples[3]" in err()
    assert lib.gpdla_posterior_maps_rows_per_launch(4, 64, 64) == (256 << 20) // (16 * 4096 * 8) == 512
    assert lib.gpdla_posterior_maps_rows_per_launch(1, 1, 1) == (256 << 20) // 8
    assert lib.gpdla_posterior_maps_rows_per_launch(5, 64, 64) == 0 and lib.gpdla_posterior_maps_rows_per_launch(1, 65, 1) == 0
    # Python refuses the same before the library is asked
    for shape, lv in (((0, 4), [0.5]), ((4, 65), [0.5]), ((4, 4), [0.9, 0.5]), ((4, 4), [1.0]), ((4, 4), [0.1] * 9)):
        with pytest.raises(ValueError):
            posteriors.check_maps_request(shape, lv)


def _fake_result(n=5, md=2, shape=(3, 4), seed=0):
    rng = np.random.default_rng(seed)
    out, _ = posteriors.maps_outputs(n, md, shape, 2, True, True)
    for k, a in out.items():
        a[...] = rng.integers(0, 9, a.shape) if a.dtype == np.int32 else rng.random(a.shape)
    out["mass"][:, 0, 1:] = np.nan
    out = posteriors.finish_maps(out, np.tile([2.0, 3.0, 20.0, 23.0], (n, 1)), shape, [0.5, 0.9])
    out["selection"] = np.arange(n) * 2
    return out


def test_stack_intensity():
    import math
    res = _fake_result()
    res["intensity"][:, 0, 0] = [1e16, 1.0, -1e16, 1.0, 0.5]      # fsum: exact where a running sum is not
    res["intensity"][3] = np.nan                                   # a row of bad weights is left out
    res["expected_absorbers"][3] = np.nan
    st = posteriors.stack_intensity(res)
    assert st["rows_used"] == 4 and st["rows_skipped"] == 1
    assert st["intensity"][0, 0] == 1.5
    use = [0, 1, 2, 4]
    assert st["intensity"][2, 3] == math.fsum(res["intensity"][r, 2, 3] for r in use)
    assert st["expected_absorbers"] == math.fsum(res["expected_absorbers"][r] for r in use)
    np.testing.assert_array_equal(st["edges_z"], res["edges_z"][0])
    np.testing.assert_array_equal(st["edges_log_nhi"], M.edges(20.0, 23.0, 4))
    res["grid"][2, 1] = 3.5
    with pytest.raises(ValueError, match="one grid"):
        posteriors.stack_intensity(res)
    del res["intensity"]
    with pytest.raises(ValueError, match="no intensity"):
        posteriors.stack_intensity(res)


def test_edges_are_the_restatements():
    grid = np.array([[2.0, 3.0, 20.0, 23.0], [2.1, 2.7, 19.5, 22.9]])
    ez, en = posteriors.grid_edges(grid, (7, 64))
    for r in range(2):
        np.testing.assert_array_equal(ez[r], M.edges(grid[r, 0], grid[r, 1], 7))
        np.testing.assert_array_equal(en[r], M.edges(grid[r, 2], grid[r, 3], 64))


@pytest.mark.parametrize("with_maps", [True, False])
def test_io_round_trip(tmp_path, with_maps):
    res = _fake_result()
    if not with_maps:
        for k in ("mass", "hpd_level", "marginal_z", "marginal_log_nhi"):
            del res[k]
    path = str(tmp_path / "maps.mat")
    io.save_posterior_maps(path, res, processed_file="p.mat", sub_dla=0.0)
    back = io.load_posterior_maps(path)
    for k, v in res.items():
        np.testing.assert_array_equal(back[k], v, err_msg=k)
        assert back[k].dtype == np.asarray(v).dtype, k
    assert back["processed_file"] == "p.mat"
    # one model: MATLAB drops the trailing singleton axes; the reader restores this package's shapes
    one = _fake_result(md=1, shape=(1, 1))
    io.save_posterior_maps(path, one)
    back = io.load_posterior_maps(path)
    for k, v in one.items():
        np.testing.assert_array_equal(back[k], v, err_msg=k)


def test_command_line_parsing():
    ap = posteriors.build_parser()
    a = ap.parse_args(["p.mat", "s.mat", "out.mat"])
    assert a.maps is None and not a.no_cells and a.map_range is None        # without --maps: as before
    a = ap.parse_args(["p.mat", "s.mat", "out.mat", "--maps", "32x16", "--levels", "0.5", "0.9", "--map-range", "2", "4", "20", "23",
                       "--no-cells", "--block-size", "7"])
    assert a.maps == (32, 16) and a.levels == [0.5, 0.9] and a.map_range == [2.0, 4.0, 20.0, 23.0] and a.no_cells
    assert a.block_size == 7 and a.maps_out is None
    for bad in ("32", "32x", "ax4", "4x4x4"):
        with pytest.raises(SystemExit):
            ap.parse_args(["p.mat", "s.mat", "out.mat", "--maps", bad])
