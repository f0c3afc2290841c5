"""GPU checks of what carries the refine pass into P(DLA) and the CDDF statistics:

 - k_bin_posteriors_boxed: the row normaliser against the math.fsum restatement, 4 x spacing(|shift|) per row
   (one rounding each of the sum, the log and the add; the sum itself is compensated); the partials against
   tests/refined_stats_restatement.py fed the GPU's own shift, at the acceptance of tests/test_gpu_cddf.py
   (NaN and zero patterns, counts and kept bins exact, values at rtol 1e-13), at S' around the 1024-sample
   tile, 1 and 64 bins, 1 and 4 requests, 1 and 3 rows with a row stride above S';
 - bit-identity across blockings and runs, and against the existing gpdla_stats_bin_posteriors where the box
   is the prior's full range;
 - k_refined_posteriors against the restatement (rtol 16 x 2^-52: exp, add and divide, each within an ulp,
   on both sides), its fallback rows, its refusals;
 - refine_absorbers(with_samples, posteriors) -> DLAStatistics(refined=...), and the two command lines.
Every figure is printed before it is asserted."""
import ctypes as C
import json

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, catalog, cddf, io, refine, synthetic
from gp_dla_detection_amd.parameters import Parameters

import cddf_restatement as R
import refine_cases as RC
import refined_stats_restatement as RS

pytestmark = pytest.mark.gpu

EDGES_Z = tuple(np.linspace(2.0, 5.0, 19))
SHAPES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)   # kStatsTile = 1024; a wave is 64 lanes
RTOL = 1e-13


def requests():
    """Four requests: 64 and 1 bins, strict and histogram, with and without the N_HI moment."""
    return [cddf.BinRequest("z", tuple(np.linspace(2.0, 5.0, 65)), 2.0, 5.0, 20.3, 23.0, lowzcut=True),
            cddf.BinRequest("lnhi", (20.0, 23.0), 2.0, 5.0, 20.0, 23.0),
            cddf.BinRequest("z", EDGES_Z, 2.0, 5.0, 20.3, 23.0, histogram=True, moment=True),
            cddf.BinRequest("lnhi", tuple(np.linspace(19.5, 23.5, 65)), 1.0, 6.0, 19.0, 24.0, histogram=True)]


def make_rows(rng, n, S):
    """Refined rows as the refine pass leaves them: log posteriors of a few hundred in size, peaked, in boxes
    that are small against the prior's range.  Returns (lam, p_dla, boxes, upper_z, u, v)."""
    u, v = rng.uniform(0, 1, S), rng.uniform(0, 1, S)
    z_lo = rng.uniform(2.05, 3.2, n)
    n_lo = rng.uniform(20.05, 21.2, n)
    boxes = np.stack([z_lo, z_lo + rng.uniform(0.01, 0.9, n), n_lo, n_lo + rng.uniform(0.05, 1.6, n)], axis=1)
    lam = np.empty((n, S))
    for s in range(n):
        lam[s] = np.log(np.maximum(rng.dirichlet(np.full(S, 0.2)), 1e-300)) + rng.normal(-900, 250)
    return lam, rng.uniform(0.06, 1.0, n), boxes, boxes[:, 1] + rng.uniform(-0.3, 0.3, n), u, v


def unusable_rows(lam, p_dla, boxes, upper_z, u, v, reqs):
    """The input conditions, from the restatement alone: rows with a p within 1e-9 relative of a request's
    p_thresh_sample or p_switch, or a z within one spacing of a window bound.  (z and log N are formed by the
    same individually rounded operations on both sides; p carries the two exps.)"""
    shift = RS.row_shifts(lam)
    bad = np.zeros(lam.shape[0], dtype=bool)
    for s in range(lam.shape[0]):
        with np.errstate(invalid="ignore"):
            p = R.sample_probabilities(lam[s], shift[s], p_dla[s])
        z, _ = RS.mapped_samples(boxes[s], u, v)
        for rq in reqs:
            for t in (rq.p_thresh_sample, rq.p_switch):
                bad[s] |= bool(np.any(np.abs(p - t) <= 1e-9 * t))
            for bound in (rq.z_lo, rq.z_hi, min(upper_z[s], rq.z_hi)):
                bad[s] |= bool(np.any(np.abs(z - bound) <= np.spacing(abs(bound))))
    return bad


def keep_usable(rows, reqs):
    lam, p_dla, boxes, upper_z, u, v = rows
    bad = unusable_rows(lam, p_dla, boxes, upper_z, u, v, reqs)
    assert bad.sum() <= 0.02 * bad.size, f"{bad.sum()} of {bad.size} generated rows are too close to a threshold"
    ok = ~bad
    return lam[ok], p_dla[ok], boxes[ok], upper_z[ok], u, v


def assert_shift(got, lam, tag):
    want = RS.row_shifts(lam)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=tag)
    ok = ~np.isnan(want)
    if ok.any():
        ulps = np.abs(got[ok] - want[ok]) / np.spacing(np.abs(want[ok]))
        print(f"{tag}: shift against math.fsum, worst {ulps.max():.2f} spacings over {ok.sum()} rows (bound 4)")
        assert (ulps <= 4).all(), tag


def assert_partials_equal(got, want, reqs, tag, rtol=RTOL):
    worst_moment = 0.0
    for g, w, rq in zip(got, want, reqs):
        for k in ("pois", "mean", "var"):
            np.testing.assert_array_equal(np.isnan(g[k]), np.isnan(w[k]), err_msg=f"{tag} {k}")
            np.testing.assert_array_equal(g[k] == 0, w[k] == 0, err_msg=f"{tag} {k}")
            if rq.moment and k != "pois":
                with np.errstate(invalid="ignore", divide="ignore"):
                    dev = np.abs(g[k] - w[k]) / np.abs(w[k])
                if np.isfinite(dev).any():
                    worst_moment = max(worst_moment, float(np.nanmax(np.where(np.isfinite(dev), dev, 0.0))))
            np.testing.assert_allclose(g[k], w[k], rtol=rtol, atol=0, equal_nan=True, err_msg=f"{tag} {k}")
        np.testing.assert_array_equal(g["count"], w["count"], err_msg=tag)
        np.testing.assert_array_equal(g["kept_bin"], w["kept_bin"], err_msg=tag)
        np.testing.assert_allclose(g["kept_p"], w["kept_p"], rtol=rtol, atol=0, err_msg=tag)
    if any(rq.moment for rq in reqs):
        print(f"{tag}: moment sums (device exp10 against NumPy's 10**), worst relative deviation {worst_moment:.2e} (bound {rtol:g})")
    return worst_moment


def assert_same(a, b, tag=""):
    for x, y in zip(a, b):
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=f"{tag} {k}")   # NaN pattern included


def take(parts, rows):
    return [{k: p[k][rows] for k in p} for p in parts]


# ---------------------------------------------------------------------------------------------
# k_bin_posteriors_boxed
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", SHAPES)
def test_shapes_around_the_tile(S):
    rng = np.random.default_rng(100 + S)
    reqs = requests()
    rows = make_rows(rng, 3, S)
    if S > 2:
        rows[0][1, S // 2] = np.nan
    lam, p_dla, boxes, upper_z, u, v = keep_usable(rows, reqs)
    wide = np.full((lam.shape[0], S + 5), np.inf)            # a row stride above S'
    wide[:, :S] = lam
    got, shift = cddf.bin_posteriors_boxed(wide[:, :S], p_dla, boxes, upper_z, u, v, reqs)
    assert_shift(shift, lam, f"S' {S} n 3 R 4")
    assert_partials_equal(got, RS.bin_posteriors_boxed(lam, shift, p_dla, boxes, upper_z, u, v, reqs), reqs, f"S' {S} n 3 R 4")
    # one row, one request of one bin
    one, sh1 = cddf.bin_posteriors_boxed(lam[:1], p_dla[:1], boxes[:1], upper_z[:1], u, v, reqs[1:2])
    np.testing.assert_array_equal(sh1, shift[:1])
    assert_same(one, take(got[1:2], slice(0, 1)), f"S' {S} n 1 R 1")
    # ... and one request of 64 bins with the moment request beside it
    two, _ = cddf.bin_posteriors_boxed(lam, p_dla, boxes, upper_z, u, v, [reqs[2], reqs[0]])
    assert_same(two, [got[2], got[0]], f"S' {S} R 2")
    assert S < 64 or any(np.any(g[k] != 0) for g in got for k in ("pois", "mean"))


def content_rows():
    """Sixty rows at S' = 300, the first twelve with the contents the kernel treats apart."""
    rng = np.random.default_rng(41)
    S = 300
    lam, p_dla, boxes, upper_z, u, v = make_rows(rng, 60, S)
    lam[1, ::9] = np.nan                                        # NaN entries (a NaN weight in the moment request)
    lam[2] = np.nan                                             # an all-NaN row
    lam[3] = -np.inf                                            # no finite entry
    lam[4, 17] = np.inf                                         # +inf
    lam[5] = -np.inf                                            # one-hot
    lam[5, 123] = -731.25
    p_dla[5] = 0.625
    boxes[6, 1] = boxes[6, 0]                                   # zero width in z
    boxes[7, 3] = boxes[7, 2] = 21.0625                         # ... and in log N
    lam[7, :3] = lam[7].max() + 4.0
    p_dla[7] = 0.97                                             # three kept pairs
    boxes[8] = (2.5, 2.5, 20.5, 20.5)                           # a point
    boxes[9] = (2.2, 4.4, 20.0, 23.0)                           # the whole window and beyond
    lam[10, :] = -800.0                                         # a flat row: every p = p_dla / S'
    boxes[11] = (1.5, 1.9, 20.5, 21.5)                          # wholly outside the z window
    return lam, p_dla, boxes, upper_z, u, v


def test_row_contents():
    reqs = requests()
    rows = content_rows()
    assert not unusable_rows(*rows, reqs)[:12].any()            # the special rows stay
    lam, p_dla, boxes, upper_z, u, v = keep_usable(rows, reqs)
    got, shift = cddf.bin_posteriors_boxed(lam, p_dla, boxes, upper_z, u, v, reqs)
    assert_shift(shift, lam, "row contents")
    assert np.isnan(shift[[2, 3, 4]]).all() and shift[5] == -731.25 and np.isfinite(shift[[0, 1, 6, 7, 8, 9, 10, 11]]).all()
    want = RS.bin_posteriors_boxed(lam, shift, p_dla, boxes, upper_z, u, v, reqs)
    assert_partials_equal(got, want, reqs, "row contents")
    # the contents took effect
    for s in (2, 3, 4):                                         # NaN shift: every p NaN, nothing kept, histogram bins poisoned
        assert got[0]["count"][s] == 0 and not got[0]["pois"][s].any() and np.isnan(got[3]["mean"][s]).any()
    assert np.isnan(got[2]["mean"][1]).any() and not np.isnan(got[0]["pois"][1]).any()
    assert got[1]["count"][5] == 1 and got[1]["kept_p"][5, 0] == 0.625          # exp(0) p_dla
    assert got[1]["count"][7] == 3 and got[1]["count"][6] + np.count_nonzero(got[1]["pois"][6]) >= 1
    assert not any(np.any(g[k][11] != 0) for g in got[:3] for k in ("pois", "mean", "var")) and got[0]["count"][11] == 0


def test_kept_capacity_overflow_names_the_row():
    rng = np.random.default_rng(2)
    lam, p_dla, boxes, upper_z, u, v = make_rows(rng, 5, 200)
    boxes[3] = (2.1, 4.9, 21.2, 21.2)
    upper_z[3] = 4.8
    lam[3] = -1e4
    lam[3, :10] = -700.0                                        # ten samples of p = 0.1 each, all in the window
    p_dla[3] = 1.0
    u[:10] = np.linspace(0.05, 0.35, 10)
    req = cddf.BinRequest("lnhi", tuple(np.linspace(20.0, 23.0, 7)), 2.0, 5.0, 20.0, 23.0, p_switch=0.05)
    with pytest.raises(cddf.KeptCapacityError, match="spectrum 3 keeps 10"):
        cddf.bin_posteriors_boxed(lam, p_dla, boxes, upper_z, u, v, [req])
    # the library returns GPDLA_ERR_UNSUPPORTED with the outputs written and the row named
    reqs, outs, keep, res = cddf._bin_structs([req], 5)
    shift = np.full(5, np.nan)
    rc = _lib.load().gpdla_stats_bin_posteriors_boxed(5, 200, _lib.ptr(lam), 200, _lib.ptr(p_dla), _lib.ptr(boxes), _lib.ptr(upper_z),
                                                      _lib.ptr(u), _lib.ptr(v), 1, reqs, outs, _lib.ptr(shift), 0)
    assert rc == _lib.ERR_UNSUPPORTED and "spectrum 3" in _lib.load().gpdla_last_error().decode()
    assert res[0]["count"].tolist()[3] == 10 and (res[0]["kept_bin"][3] == 2).all() and np.isfinite(shift).all()
    want = RS.bin_posteriors_boxed(lam, shift, p_dla, boxes, upper_z, u, v, [req])
    assert_partials_equal(res, want, [req], "overflow")


def test_bit_identity_across_blockings_and_runs():
    reqs = requests()
    lam, p_dla, boxes, upper_z, u, v = content_rows()
    n = 12
    lam, p_dla, boxes, upper_z = lam[:n], p_dla[:n], boxes[:n], upper_z[:n]
    full, shift = cddf.bin_posteriors_boxed(lam, p_dla, boxes, upper_z, u, v, reqs)
    again, shift2 = cddf.bin_posteriors_boxed(lam, p_dla, boxes, upper_z, u, v, reqs)
    assert_same(full, again, "second run")
    np.testing.assert_array_equal(shift, shift2)
    r = slice(None, None, -1)
    rev, shift_r = cddf.bin_posteriors_boxed(lam[r], p_dla[r], boxes[r], upper_z[r], u, v, reqs)
    assert_same(take(rev, r), full, "reversed")
    np.testing.assert_array_equal(shift_r[r], shift)
    for step in (1, 2):
        for a in range(0, n, step):
            b = slice(a, a + step)
            part, sh = cddf.bin_posteriors_boxed(lam[b], p_dla[b], boxes[b], upper_z[b], u, v, reqs)
            assert_same(part, take(full, b), f"rows {a}..{a + step}")
            np.testing.assert_array_equal(sh, shift[b])


def test_full_range_boxes_equal_the_existing_kernel():
    """Boxes equal to the prior's range, v on a grid that makes n_lo + (n_hi - n_lo) v exact: the samples are
    those of a first pass, and gpdla_stats_bin_posteriors fed the boxed entry's shift is the yardstick."""
    rng = np.random.default_rng(77)
    n, S = 9, 1500
    lam, p_dla, boxes, upper_z, u, _ = make_rows(rng, n, S)
    v = rng.integers(0, 1024, S) / 1024.0
    boxes[:, 0] = rng.uniform(1.8, 2.6, n)
    boxes[:, 1] = boxes[:, 0] + rng.uniform(0.8, 2.8, n)
    boxes[:, 2], boxes[:, 3] = 20.0, 24.0
    upper_z = boxes[:, 1] - 0.1
    lnhi = 20.0 + 4.0 * v
    assert np.all(lnhi * 256 == np.round(lnhi * 256))                                 # on the grid: the map is exact
    lam[2, ::11] = np.nan
    reqs = requests()
    got, shift = cddf.bin_posteriors_boxed(lam, p_dla, boxes, upper_z, u, v, reqs)
    old = cddf.bin_posteriors(lam, shift, p_dla, boxes[:, 0], boxes[:, 1], upper_z, u, lnhi, reqs)
    for i, rq in enumerate(reqs):
        if rq.moment:
            assert_partials_equal(got[i:i + 1], old[i:i + 1], [rq], "full range, moment request")
        else:
            assert_same(got[i:i + 1], old[i:i + 1], f"full range, request {i}")
    assert np.any(got[0]["pois"] > 0) and np.any(got[3]["mean"] > 0)


# ---------------------------------------------------------------------------------------------
# k_refined_posteriors
# ---------------------------------------------------------------------------------------------

SR, LEVELS = 128, 2
# the refine's selection, by kind of quasar (tests/refine_cases.py): broad, edge and masked_run are left out;
# status1 and status3 are unusable
REFINED_KINDS = ("strong_masked", "status1", "strong", "none", "status3")
REFINE_SELECTION = [RC.KINDS.index(k) for k in REFINED_KINDS]


def _context():
    model, samples, spectra, _ = RC.make_batch(8, 3)
    ctx = gp.Context(0, Parameters(num_lines=3))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(SR))
    n = len(spectra)
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))


def test_refined_posteriors_against_the_restatement():
    ctx, batch = _context()
    try:
        batch.process()
        first = batch.download()
        with pytest.raises(_lib.GpdlaError, match="not been refined") as e:          # refused before any refine
            batch.refined_posteriors()
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
        batch.refine(REFINE_SELECTION, levels=LEVELS, delta=RC.DELTA, pad=RC.PAD, download=False)
        ref = batch.download_refined(None, with_samples=False)                      # all eight: status -1 outside the selection
        got = batch.refined_posteriors()
        sub = batch.refined_posteriors([5, 0, 0, 3])
        with pytest.raises(_lib.GpdlaError, match="selection"):
            batch.refined_posteriors([8])
        after = batch.download()
    finally:
        batch.close()
        ctx.close()
    want_status = [(1 if k.startswith("status") else 0) if k in REFINED_KINDS else _lib.REFINE_NOT_REFINED for k in RC.KINDS]
    assert ref["status"].tolist() == want_status
    mp, p_no, p_dla, refined = RS.refined_posteriors(first["log_posteriors_no_dla"], ref["log_posteriors_dla_refined"], ref["status"],
                                                     first["model_posteriors"], first["p_no_dlas"], first["p_dlas"])
    np.testing.assert_array_equal(got["refined"], refined)
    assert refined.tolist() == [int(st == 0) for st in want_status] and refined.sum() == 3
    on = refined == 1
    rtol = 16 * 2.0 ** -52
    for name, want in (("model_posteriors_refined", mp), ("p_no_dlas_refined", p_no), ("p_dlas_refined", p_dla)):
        with np.errstate(invalid="ignore", divide="ignore"):
            dev = np.abs(got[name][on] - want[on]) / np.abs(want[on])
        print(f"{name}: refined rows against the restatement, worst relative deviation {np.nanmax(np.nan_to_num(dev)):.2e} (bound {rtol:.2e}); "
              f"values {got[name][on].reshape(-1)}")
        np.testing.assert_allclose(got[name][on], want[on], rtol=rtol, atol=0)
    for name, key in (("model_posteriors_refined", "model_posteriors"), ("p_no_dlas_refined", "p_no_dlas"), ("p_dlas_refined", "p_dlas")):
        np.testing.assert_array_equal(got[name][~on], first[key][~on], err_msg=name)   # the first pass's columns, NaN included
    for name in got:
        np.testing.assert_array_equal(sub[name], got[name][[5, 0, 0, 3]], err_msg=name)
    for key in first:
        np.testing.assert_array_equal(after[key], first[key], err_msg=key)          # process() results are untouched
    print(f"P(DLA) first pass {first['p_dlas']} -> refined {got['p_dlas_refined']}")


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------

def test_refine_then_statistics():
    model, samples, spectra, _ = RC.make_batch(8, 3)
    results = gp.process_qsos(model, samples, spectra, prior_catalog=synthetic.make_prior_catalog())
    points = RC.halton_points(SR)
    ref = refine.refine_absorbers(model, samples, spectra, results, 0.5, levels=RC.LEVELS, delta=RC.DELTA, pad=RC.PAD,
                                  points=points, with_samples=True, posteriors=True)
    peaked = [RC.KINDS.index(k) for k in RC.PEAKED]
    assert set(peaked) <= set(ref["selection"].tolist())
    np.testing.assert_array_equal(ref["refine_u"], points[0])
    np.testing.assert_array_equal(ref["refined"], (ref["status"] == 0).astype(np.int32))
    snrs = np.ones(len(spectra))
    kw = dict(sub_dla=False, p_thresh_spec=1e-3)
    plain = cddf.DLAStatistics(results, samples, snrs, **kw)
    st = cddf.DLAStatistics(results, samples, snrs, refined=ref, block_size=2, **kw)
    reqs = [st._line_request(2, 5), st._cddf_request(2., 5., 30, 20., 23.), cddf.omega_dla_request(2, 5)]
    got, old = st.partials(reqs), plain.partials(reqs)
    # without `refined`: what one direct call of the existing pass gives
    sel = plain.selected
    direct = cddf.bin_posteriors(results["sample_log_likelihoods_dla"][sel], plain._shift, plain.p_dla[sel], results["min_z_dlas"][sel],
                                 results["max_z_dlas"][sel], plain._upper_z, samples["offset_samples"], samples["log_nhi_samples"], reqs)
    assert_same(old, direct, "plain statistics")
    rows = np.flatnonzero(ref["status"] == 0)
    quasars = ref["selection"][rows]
    mp = catalog.occams_model_posteriors(ref["model_posteriors_refined"][rows])
    np.testing.assert_array_equal(st.p_dla[quasars], mp[:, 1])
    boxed = np.isin(st.selected, quasars)
    assert boxed.any() and set(peaked) <= set(st.selected[boxed].tolist())
    r = rows[np.searchsorted(quasars, st.selected[boxed])]                          # (the selection is ascending)
    want, _ = cddf.bin_posteriors_boxed(ref["sample_log_posteriors_refined"][r], st.p_dla[st.selected[boxed]], ref["boxes"][r, -1],
                                        st._upper_z[boxed], ref["refine_u"], ref["refine_v"], reqs)
    assert_same(take(got, boxed), want, "refined quasars")
    both = np.intersect1d(st.selected[~boxed], plain.selected)
    assert both.size == np.count_nonzero(~boxed)
    assert_same(take(got, np.flatnonzero(np.isin(st.selected, both))), take(old, np.flatnonzero(np.isin(plain.selected, both))),
                "unrefined quasars")
    # purpose: how many of the 30 log N_HI bins over 20 .. 23 receive more than 1 % of a row's weight
    hist = cddf.BinRequest("lnhi", tuple(np.linspace(20.0, 23.0, 31)), 0.0, 10.0, 19.0, 24.0, histogram=True)
    (a,), (b,) = plain.partials([hist]), st.partials([hist])
    for q in peaked:
        wa, wb = a["mean"][np.flatnonzero(plain.selected == q)[0]], b["mean"][np.flatnonzero(st.selected == q)[0]]
        na, nb = int(np.sum(wa > 0.01 * wa.sum())), int(np.sum(wb > 0.01 * wb.sum()))
        print(f"{RC.KINDS[q]}: log N_HI bins with more than 1 % of the row's weight: first pass {na}, refined {nb}")
        assert nb > 1
    # the statistics themselves run on the merged partials
    out = st.statistics(2, 5)
    assert set(out) == {"line_density", "column_density_function", "omega_dla"}


def test_command_lines_equal_the_in_memory_path(tmp_path):
    files = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=12, num_samples=64, empty_quasar=3)
    paths, test_ind = files["paths"], files["test_ind"]
    spectra = [s for s, t in zip(files["spectra"], test_ind) if t]
    results = gp.process_qsos(files["model"], files["samples"], spectra, prior_catalog=files["prior"])
    processed, out = str(tmp_path / "processed.mat"), str(tmp_path / "refined.mat")
    io.save_processed_qsos(processed, results, test_ind=test_ind)
    args = [paths["preloaded"], paths["catalog"], paths["learned"], paths["samples"], processed, out, "--p-thresh", "0.3",
            "--levels", "2", "--points", "50", "--batch", "4"]
    assert refine.main(args + ["--tables", "--posteriors"]) == 0
    want = refine.refine_absorbers(files["model"], files["samples"], spectra, results, 0.3, levels=2,
                                   points=refine.default_points(50), with_samples=True, posteriors=True)
    back = io.load_refined_results(out)
    assert want["selection"].size >= 2 and "sample_log_likelihoods_refined" not in back   # --tables: the posterior table alone
    for key in refine.SCALARS + refine.POSTERIORS + refine.POINTS + ("boxes", "status", "selection", "sample_log_posteriors_refined"):
        np.testing.assert_array_equal(back[key], want[key], err_msg=key)
    # one table by name is that table of the two, and the other is not downloaded
    only = refine.refine_absorbers(files["model"], files["samples"], spectra, results, 0.3, levels=2,
                                   points=refine.default_points(50), with_samples=("sample_log_posteriors_refined",),
                                   posteriors=True, max_quasars_per_batch=3)
    assert "sample_log_likelihoods_refined" not in only
    for key in refine.SCALARS + refine.POSTERIORS + refine.POINTS + ("boxes", "status", "selection", "sample_log_posteriors_refined"):
        np.testing.assert_array_equal(only[key], want[key], err_msg=key)                  # and in batches of 3
    # without the switches the file holds what it held before
    assert refine.main(args) == 0
    assert not any(k in io.load_refined_results(out) for k in refine.POSTERIORS + refine.POINTS + refine.TABLES)
    with pytest.raises(ValueError, match="--tables"):
        cddf.main([processed, paths["samples"], "--refined", out])
    # cddf --refined against DLAStatistics(refined=dict) on the in-memory results
    assert refine.main(args + ["--tables", "--posteriors"]) == 0
    j = str(tmp_path / "cddf.json")
    cddf.main([processed, paths["samples"], "--z-min", "2", "--z-max", "5", "--lnhi-nbins", "6", "--block-size", "3", "--refined", out,
               "--json", j])
    st = cddf.DLAStatistics(results, files["samples"], np.full(len(spectra), np.inf), sub_dla=False, refined=want)
    mem = {k: cddf._jsonable(v) for k, v in st.statistics(2., 5., 6).items()}
    assert json.load(open(j)) == json.loads(json.dumps(mem))
    plain = cddf.DLAStatistics(results, files["samples"], np.full(len(spectra), np.inf), sub_dla=False)
    assert np.isin(want["selection"][want["status"] == 0], st.selected).all()
    print(f"selected spectra: {plain.selected.size} without, {st.selected.size} with the refined results; "
          f"{np.count_nonzero(want['status'] == 0)} refined")
