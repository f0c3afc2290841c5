"""The model-spectra kernels at their own tile, chunk and launch-split edges
(tests/model_spectra_edge_cases.py) against the NumPy-and-oracle restatement
(tests/model_spectra_restatement.py): k_spectra_map's 250-pixel tile with absorbers on its seams,
k_spectra_weights / k_spectra_moments / k_spectra_combine at grids of 1 .. 257 pixels and 1 .. 513 samples with
the whole weight on either side of a wave or chunk seam, the launch split of the moments pass, and
k_spectra_continuum's 128-pixel tile and thread-to-entry map at the ranks where [vech(B) | v] straddles a slot.
Tolerances are those of tests/test_gpu_model_spectra.py; every figure is printed before it is asserted, and
no comparison passes on empty or NaN arrays: what is expected to be a number is asserted finite on both
sides, what is expected to be NaN is asserted NaN with the status beside it."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import model_spectra_edge_cases as E
import model_spectra_restatement as R
from test_gpu_model_spectra import TOL_MAP, TOL_MOMENTS, _dev, _multi, _single

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------
# P1
# ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def map_case(oracle):
    model, spectra = E.map_batch()
    grids = [R.grid(oracle, model, sp) for sp in spectra]
    return model, spectra, grids, E.map_lists(), E.resolve_absorbers(E.map_lists(), grids)


@pytest.mark.parametrize("num_lines", E.MAP_LINES)
def test_map_absorption_at_the_tile_edges(oracle, map_case, num_lines):
    """n_u at, one short of and one past 244, 250, 256 and 500 (and 1, 2, 6, 7: n_pad = 7 .. 13), 0 / 1 / 4 / 8
    absorbers, absorbers centred on the pixels either side of a tile seam and on the last pixel, masked and
    unmasked quasars alternating, a fully masked quasar last.  (At 31 lines the absorber on the last pixel of the
    249-pixel grid has its Ly-31 core next to a padding pixel at the blue end, where one ulp of the padding wavelength
    is 1.5e-11 of the line's profile: 6.3e-13 was measured there, 1e-15 everywhere else.  DESIGN.md 4.12, "Edges".)"""
    model, spectra, grids, lists, absorbers = map_case
    off, zs, lns = absorbers
    ctx, batch = _single(model, synthetic.make_samples(16), spectra, Parameters(num_lines=num_lines))
    try:
        res = batch.model_spectra(absorbers=absorbers, products=("map",))
        counts = batch.unmasked_counts()
    finally:
        batch.close()
        ctx.close()
    n_u = list(E.MAP_NU) + [grids[-1]["n_u"]]
    np.testing.assert_array_equal(counts, n_u)
    np.testing.assert_array_equal(np.diff(res["offsets"]), n_u)
    assert res["offsets"][0] == 0 and res["map_absorption"].size == sum(n_u)
    got = gp.split_cells(res["map_absorption"], res["offsets"])
    assert res["status"].tolist() == [0] * len(E.MAP_NU) + [1]
    assert got[-1].size == n_u[-1] > 0 and np.isnan(got[-1]).all()            # the fully masked quasar: a NaN row, status 1
    worst, seams = 0.0, 0
    for i, g in enumerate(grids[:-1]):
        want = R.map_absorption(oracle, g["pad"], zs[off[i]:off[i + 1]], lns[off[i]:off[i + 1]], num_lines)
        assert want.size == got[i].size == g["n_u"] and np.isfinite(want).all() and np.isfinite(got[i]).all()
        d = _dev(got[i], want)
        print(f"lines {num_lines} n_u {g['n_u']}: {len(lists[i])} absorbers, |delta| {d:.2e}")
        worst = max(worst, d)
        if not lists[i]:
            assert (got[i] == 1.0).all()
        for item, pixels in E.seam_pixels(lists[i], g["n_u"]):
            assert pixels and (want[pixels] < 0.5).all() and (got[i][pixels] < 0.5).all(), (g["n_u"], item)   # the trough is there
            seams += 1
    print(f"P1 edges, worst |delta| at {num_lines} lines: {worst:.3e} ({seams} absorbers on a seam)")
    assert seams == 10
    assert worst < TOL_MAP


# ------------------------------------------------------------------------------------------------
# P2
# ------------------------------------------------------------------------------------------------

_MOMENT_GRIDS = {}


def _moment_batch(oracle, nus):
    if nus not in _MOMENT_GRIDS:
        model, spectra = E.moments_batch(nus)
        _MOMENT_GRIDS[nus] = (model, spectra, [R.grid(oracle, model, sp) for sp in spectra])
    return _MOMENT_GRIDS[nus]


def _check_entries(oracle, grids, samples, entries, rows, res, nhi_key, num_lines, label):
    """Every entry of a call against the restatement.  Returns the worst deviation of the entries that expect numbers."""
    mean, var = gp.split_cells(res["mean_absorption"], res["offsets"]), gp.split_cells(res["var_absorption"], res["offsets"])
    np.testing.assert_array_equal(np.diff(res["offsets"]), [grids[q]["n_u"] for q, _ in entries])
    order = E.z_order(samples)
    worst, numbers, nans = 0.0, 0, 0
    for j, (q, kind) in enumerate(entries):
        g = grids[q]
        assert res["status"][j] == 0 and mean[j].size == var[j].size == g["n_u"] > 0
        want_mean, want_var = E.want_moments(oracle, g, samples, rows[j], nhi_key, num_lines)
        if E.expects_nan(kind, rows[j]):
            assert kind in E.NAN_ROWS, (label, j, q, kind)          # (the sweep's own row always has weight)
            assert np.isnan(want_mean).all() and np.isnan(mean[j]).all() and np.isnan(var[j]).all(), (label, j, q, kind)
            nans += 1
            continue
        assert np.isfinite(want_mean).all() and np.isfinite(want_var).all(), (label, j, q, kind)
        assert np.isfinite(mean[j]).all() and np.isfinite(var[j]).all(), (label, j, q, kind)
        assert (var[j] >= 0.0).all(), (label, j, q, kind)
        dm, dv = _dev(mean[j], want_mean), _dev(var[j], want_var)
        worst = max(worst, dm, dv)
        numbers += 1
        note = ""
        if kind[0] == "hot":            # the whole weight on one sample: its own profile, no spread
            i = order[kind[1]]
            z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"][i]
            own = _dev(mean[j], oracle.voigt(g["pad"], z, samples[nhi_key][i], num_lines))
            worst = max(worst, own)
            note = f", |mean - own profile| {own:.2e}, max var {var[j].max():.1e}"
            assert (var[j] < E.ONE_HOT_VAR).all(), (label, j, q, kind, float(var[j].max()))
        print(f"{label} entry {j}: n_u {g['n_u']} {kind}: |delta mean| {dm:.2e}, |delta var| {dv:.2e}{note}")
    assert nans == E.MOM_REPEATS * len(E.NAN_ROWS) and numbers == len(entries) - nans
    return worst


def _moments_at(oracle, S, nus, num_lines, resident):
    model, spectra, grids = _moment_batch(oracle, nus)
    samples = synthetic.make_samples(S)
    entries = E.moment_entries(S, len(nus))
    sel = np.array([q for q, _ in entries], dtype=np.int64)
    ctx, batch = _single(model, samples, spectra, Parameters(num_lines=num_lines))
    try:
        np.testing.assert_array_equal(batch.unmasked_counts(), nus)
        batch.process()
        sweep = np.array(batch.download()["sample_log_likelihoods_dla"])
        rows = np.stack([E.moment_row(kind, S, samples, sweep[q]) for q, kind in entries])
        res = batch.model_spectra(selection=sel, weights=rows, products=("moments",))
        res_lls = batch.model_spectra(selection=sel, weights=rows, sub_dla=True, products=("moments",))
        if resident:
            own = batch.model_spectra(weights="resident", products=("moments",))
            host = batch.model_spectra(weights=sweep, products=("moments",))
    finally:
        batch.close()
        ctx.close()
    assert sweep.shape == (len(nus), S) and np.isfinite(sweep).any(axis=1).all()
    worst = _check_entries(oracle, grids, samples, entries, rows, res, "nhi_samples", num_lines, f"S={S} dla")
    worst_lls = _check_entries(oracle, grids, samples, entries, rows, res_lls, "lls_nhi_samples", num_lines, f"S={S} lls")
    assert not np.array_equal(_bits(res["mean_absorption"]), _bits(res_lls["mean_absorption"]))      # other column densities
    if resident:
        for name in ("mean_absorption", "var_absorption"):
            assert np.isfinite(own[name]).all() and own[name].size == sum(nus)
            assert np.array_equal(_bits(own[name]), _bits(host[name])), name
    return worst, worst_lls


@pytest.mark.parametrize("S", E.MOM_S)
def test_moments_at_the_tile_wave_and_chunk_edges(oracle, S):
    """Grids of 1, 2, 15 .. 17, 31 .. 33, 250 and 257 pixels, S on either side of a wave (64) and a chunk (256), rows
    from a host table: flat, the sweep's own, every second entry NaN, the whole weight on the sample at z-order
    position 0 / 62 / 63 / 64 / 254 / 255 / 256 / S - 1, and the rows without weight (all NaN, all -inf, one +inf:
    NaN moments); then the same with the sub-DLA column densities.  At S = 65 and 257 the resident table gives
    the bits of the same table passed from the host."""
    worst, worst_lls = _moments_at(oracle, S, E.MOM_NU, 3, S in E.RESIDENT_S)
    print(f"P2 edges, worst |delta| at S = {S}: dla {worst:.3e}, lls {worst_lls:.3e}")
    assert worst < TOL_MOMENTS and worst_lls < TOL_MOMENTS


def test_moments_at_the_tile_edges_31_lines(oracle):
    worst, worst_lls = _moments_at(oracle, E.MOM_S_31, E.MOM_NU_31, 31, False)
    print(f"P2 edges, worst |delta| at 31 lines, S = {E.MOM_S_31}: dla {worst:.3e}, lls {worst_lls:.3e}")
    assert worst < TOL_MOMENTS and worst_lls < TOL_MOMENTS


def test_moments_launch_split(oracle):
    """gpdla_batch_model_spectra takes the selection in groups whose partial sums fit 256 MiB and hands
    k_spectra_moments / k_spectra_combine the group's first entry s0: w, sel, flag and out_off are indexed by
    s0 + sl, the partial sums by sl.  8 quasars of 1500 in-range (1504 stored) pixels at S = 10^4, the shape
    DESIGN.md 4.12 records as "groups of 278": chunks = ceil(10^4 / 256) = 40, stride = 16 ceil(1504 / 16) =
    1504, nsub = 2^28 // (40 x 2 x 1504 x 8) = 278.  600 entries (the 8 quasars repeated in a shuffled order)
    make launches of 278, 278 and 44; fewer than 2 x 278 + 1 would not give a second seam.  Every entry within
    2 of a seam and every 16th equal, bit for bit, the same (quasar, row) computed alone; the NaN pattern of
    EVERY entry is that of its own row (an all-NaN row every 41st entry: an entry never shares its flag with
    the one 278 before it); one entry behind each seam is compared with the restatement."""
    model, spectra = E.split_batch()
    S = E.SPLIT_S
    samples = synthetic.make_samples(S)
    sel = E.split_selection()
    nsel = sel.size
    stored = max(np.asarray(sp["wavelengths"]).size for sp in spectra)
    nsub = E.launch_group(S, stored)
    print(f"launch split: {nsel} entries, groups of {nsub}: launches of {[min(nsub, nsel - s0) for s0 in range(0, nsel, nsub)]}")
    assert nsel > 2 * nsub and nsel % nsub != 0
    checked = E.split_checked_entries(nsel, nsub)
    nan_row = E.split_nan_entries(nsel)
    alone = {}
    ctx, batch = _single(model, samples, spectra)
    try:
        batch.process()
        sweep = np.array(batch.download()["sample_log_likelihoods_dla"])
        rows = E.split_rows(sel, sweep, samples)
        res = batch.model_spectra(selection=sel, weights=rows, products=("moments",))
        for j in checked:
            alone[j] = batch.model_spectra(selection=sel[j:j + 1], weights=rows[j:j + 1], products=("moments",))
    finally:
        batch.close()
        ctx.close()
    assert np.isfinite(sweep).any(axis=1).all()
    np.testing.assert_array_equal(np.diff(res["offsets"]), np.full(nsel, E.SPLIT_NU))
    assert (res["status"] == 0).all()
    mean = res["mean_absorption"].reshape(nsel, E.SPLIT_NU)
    var = res["var_absorption"].reshape(nsel, E.SPLIT_NU)
    # every entry: NaN exactly where its own row has no weight, numbers elsewhere
    np.testing.assert_array_equal(np.isnan(mean).all(axis=1), nan_row)
    np.testing.assert_array_equal(np.isnan(var).all(axis=1), nan_row)
    assert np.isfinite(mean[~nan_row]).all() and np.isfinite(var[~nan_row]).all() and (var[~nan_row] >= 0).all()
    assert (mean[~nan_row].min(axis=1) < 1.0 - 1e-4).all()          # weight was there: no row of ones
    # neighbours differ, so an entry that took its neighbour's weights or partial sums shows
    assert all(not np.array_equal(_bits(mean[j]), _bits(mean[j + 1])) for j in range(nsel - 1))
    differing = 0
    for j in checked:
        one = alone[j]
        assert one["offsets"].tolist() == [0, E.SPLIT_NU] and one["status"][0] == 0
        for name, table in (("mean_absorption", mean), ("var_absorption", var)):
            assert nan_row[j] or np.isfinite(one[name]).all()
            same = np.array_equal(_bits(one[name]), _bits(table[j]))
            differing += not same
            if not same:
                print(f"entry {j} (group {j // nsub}, quasar {sel[j]}) differs from the same row alone: {name} by {_dev(one[name], table[j]):.2e}")
    print(f"launch split: {len(checked)} entries against the same (quasar, row) alone, {differing} arrays differ")
    assert differing == 0
    # against the restatement: a sweep row behind the first seam and a one-hot or flat row in the last group
    first = next(j for j in range(nsub + 1, 2 * nsub) if j % 5 == 0 and not nan_row[j])
    last = next(j for j in range(2 * nsub + 1, nsel) if j % 5 != 0 and not nan_row[j] and sel[j] != sel[first])
    worst = 0.0
    for j in (first, last):
        g = R.grid(oracle, model, spectra[sel[j]])
        want_mean, want_var = R.moments(oracle, g, samples["offset_samples"], samples["nhi_samples"], rows[j], 3)
        assert np.isfinite(want_mean).all() and np.isfinite(want_var).all()
        dm, dv = _dev(mean[j], want_mean), _dev(var[j], want_var)
        print(f"entry {j} (group {j // nsub}, quasar {sel[j]}): |delta mean| {dm:.2e}, |delta var| {dv:.2e}")
        worst = max(worst, dm, dv)
    print(f"P2 launch split, worst |delta| of two entries behind the seams: {worst:.3e}")
    assert worst < TOL_MOMENTS


# ------------------------------------------------------------------------------------------------
# P3
# ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def continuum_tolerance(oracle):
    disagreement = E.continuum_disagreement(oracle)
    tol = R.continuum_tolerance(disagreement)
    print(f"dense-vs-Woodbury disagreement on the edge cases {disagreement:.2e} -> tolerance {tol:.2e}")
    return tol


@pytest.mark.parametrize("k", E.CONT_RANKS)
def test_continuum_at_the_tile_edges_and_entry_slots(oracle, continuum_tolerance, k):
    """Ranks 1, 2, 21 (230 + 21 entries: slot 0 only), 22 (v straddles slots 0 and 1), 23 (vech(B) straddles) and
    40 (every slot full); grids of 2 (fewer kept pixels than k), 127 .. 129 and 256, 257 pixels, masked at 5 %
    from 127 up; the null model and two absorbers; with the mean-flux model too at k = 22 and 40.  Against the
    dense form of the restatement."""
    c = E.continuum_wanted(oracle, k)
    worst = 0.0
    for (meanflux, with_absorbers), v in c["variants"].items():
        p = MultiParameters() if meanflux else Parameters()
        ctx, batch = (_multi if meanflux else _single)(c["model"], synthetic.make_samples(16), c["spectra"], p)
        try:
            res = batch.model_spectra(absorbers=v["absorbers"], meanflux=meanflux, products=("map", "continuum"))
        finally:
            batch.close()
            ctx.close()
        assert res["status"].tolist() == [0] * len(E.CONT_NU)
        np.testing.assert_array_equal(np.diff(res["offsets"]), E.CONT_NU)
        cont, flux = gp.split_cells(res["continuum"], res["offsets"]), gp.split_cells(res["model_flux"], res["offsets"])
        for i, (g, (want_cont, want_flux)) in enumerate(zip(c["grids"], v["dense"])):
            assert np.isfinite(want_cont).all() and np.isfinite(want_flux).all() and want_cont.size == g["n_u"]
            assert np.isfinite(cont[i]).all() and np.isfinite(flux[i]).all()          # masked pixels inside the grid too
            assert g["n_u"] < 127 or (~g["kept"]).any()
            dc, df = _dev(cont[i], want_cont), _dev(flux[i], want_flux)
            print(f"k {k} meanflux {int(meanflux)} absorbers {2 * int(with_absorbers)} n_u {g['n_u']} ({int(g['kept'].sum())} kept): "
                  f"|delta continuum| {dc:.2e}, |delta model flux| {df:.2e}")
            worst = max(worst, dc, df)
    print(f"P3 edges, worst |delta| at k = {k}: {worst:.3e} (tolerance {continuum_tolerance:.2e})")
    assert worst < continuum_tolerance
