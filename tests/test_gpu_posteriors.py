"""GPU checks of the parameter summaries against the NumPy restatement
(tests/posterior_restatement.py).  The sample counts are those at which the tiling and the bucket
logic of k_parameter_summaries can go wrong (B = ceil(S / 256) = 1, 2, 4, 5, 40, 65; a staging tile of
1024 samples less one, exactly, plus one); each case holds one row of every kind of R.ROW_KINDS.

Quantile acceptance (exact, no per-case exclusions): with F and F- from the restatement's
extended-precision sums the GPU's v* is bitwise one of the slot's values of positive weight, F-(v*) / T
< p + eps and F(v*) / T >= p - eps, eps = 1e-11; where only one value is acceptable -- more than 98 % of
the compared cases, asserted on the CPU in tests/test_posteriors.py -- that is the restatement's float64
value too, so the GPU equals it bitwise.  Moments, exceedance and ESS: tol x scale, tol = 10 x the
restatement's float64-versus-extended disagreement on the same inputs, floored at 1e-13, capped at 1e-9.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import cddf, posteriors, synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import posterior_restatement as R

pytestmark = pytest.mark.gpu

def _gpu(inputs, **kw):
    sll, base, off, lnhi, z_min, z_max = inputs
    return posteriors.parameter_summaries(sll, dict(offset_samples=off, log_nhi_samples=lnhi), z_min, z_max, base,
                                          probabilities=R.PROBABILITIES, thresholds=R.THRESHOLDS, **kw)


def _same(a, b, keys=posteriors.FIELDS):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)   # NaN pattern included


@pytest.mark.parametrize("md", R.MD_VALUES)
@pytest.mark.parametrize("S", R.S_VALUES)
def test_against_the_restatement(S, md):
    ref = R.case_reference(S, md)
    got = _gpu(ref["inputs"])
    f64 = ref["f64"]
    np.testing.assert_array_equal(got["status"], f64["status"])
    kinds = R.ROW_KINDS
    assert (got["status"][kinds.index("all_nan")] == 1).all() and (got["status"][kinds.index("nan_max_z")] == 2).all()
    # quantiles
    for k in ("quantiles_z", "quantiles_log_nhi"):
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(f64[k]), err_msg=k)
    unique = bitwise = 0
    for (r, m, j, qy, q), vals in ref["accept"].items():
        k = "quantiles_log_nhi" if qy else "quantiles_z"
        v = got[k][r, m, j, q]
        assert v in vals, f"S {S} md {md} row {kinds[r]} model {m + 1} slot {j + 1} {k} p {R.PROBABILITIES[q]}: " \
                          f"{v!r} not in {vals!r} (restatement {f64[k][r, m, j, q]!r})"
        if vals.size == 1:
            unique += 1
            assert v == f64[k][r, m, j, q]
        bitwise += v == f64[k][r, m, j, q]
    print(f"S {S} md {md}: {len(ref['accept'])} quantiles compared, {unique} with one acceptable value, "
          f"{bitwise} bitwise equal to the restatement")
    # moments, exceedance, ESS
    for k, (atol, dis, tol) in R.tolerances(ref).items():
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref["ext"][k]), err_msg=k)
        with np.errstate(invalid="ignore"):
            dev = np.abs(got[k] - ref["ext"][k]) / (atol / tol if np.ndim(atol) == got[k].ndim or np.ndim(atol) == 0
                                                    else (atol / tol)[..., None])
        worst = float(np.nanmax(dev)) if np.isfinite(dev).any() else 0.0
        print(f"S {S} md {md} {k}: restatement f64 vs extended {dis:.2e}, tolerance {tol:.2e}, GPU worst {worst:.2e} (scale units)")
        assert worst <= tol, k
    assert abs(got["effective_samples"][kinds.index("peaked"), 0] - 1.0) < 1e-6
    # the correlation Python derives: NaN where a std vanishes (one point; zero-width range)
    assert np.isnan(got["correlation"][kinds.index("one_finite")]).all()
    assert np.isnan(got["correlation"][kinds.index("zero_width")]).all()


@pytest.mark.parametrize("S,md", [(257, 2), (R.TILE + 1, 4)])
def test_rows_do_not_depend_on_selection_order_or_blocking(S, md):
    sll, base, off, lnhi, z_min, z_max = R.case_reference(S, md)["inputs"]
    whole = _gpu((sll, base, off, lnhi, z_min, z_max))
    again = _gpu((sll, base, off, lnhi, z_min, z_max))
    _same(whole, again)
    rev = slice(None, None, -1)
    back = _gpu((sll[rev], None if base is None else base[rev], off, lnhi, z_min[rev], z_max[rev]))
    for k in posteriors.FIELDS:
        np.testing.assert_array_equal(back[k][rev], whole[k], err_msg=k)
    for r in (0, 2, 6, 8, 11):
        one = _gpu((sll[r:r + 1], None if base is None else base[r:r + 1], off, lnhi, z_min[r:r + 1], z_max[r:r + 1]))
        for k in posteriors.FIELDS:
            np.testing.assert_array_equal(one[k][0], whole[k][r], err_msg=f"{k} row {r}")
    # fewer models of the same table: the leading models and slots
    if md > 2:
        two = posteriors.parameter_summaries(sll[:, :2], dict(offset_samples=off, log_nhi_samples=lnhi), z_min, z_max,
                                             base, probabilities=R.PROBABILITIES, thresholds=R.THRESHOLDS)
        for k in posteriors.FIELDS[:8]:
            np.testing.assert_array_equal(two[k], whole[k][:, :2, :2], err_msg=k)
    # a strided table (rows of a wider array) is packed by the library
    wide = np.full((sll.shape[0], md * S + 3), 7.0)
    wide[:, :md * S] = sll.reshape(sll.shape[0], -1)
    from gp_dla_detection_amd import _lib
    import ctypes as C
    out, ps = posteriors._outputs(sll.shape[0], md, len(R.PROBABILITIES), len(R.THRESHOLDS))
    rq = posteriors._request(md, list(R.PROBABILITIES), list(R.THRESHOLDS))
    _lib.check(_lib.load().gpdla_stats_parameter_summaries(
        sll.shape[0], S, _lib.ptr(wide), wide.shape[1], base.ctypes.data_as(_lib._u32p), _lib.ptr(z_min), _lib.ptr(z_max),
        _lib.ptr(off), _lib.ptr(lnhi), C.byref(rq), C.byref(ps), 0))
    _same(out, whole)


def _map_inside(summ, res, sll, base, samples_lnhi):
    """[p = 0.025, p = 0.975] of each slot contains the slot's MAP value whenever the MAP sample's weight
    share exceeds 5 %.  Returns the number of slots checked."""
    sll = sll if sll.ndim == 3 else sll[:, None, :]
    probs = list(summ["probabilities"])
    lo, hi = probs.index(0.025), probs.index(0.975)
    map_z = np.asarray(res["MAP_z_dlas"]).reshape(sll.shape[0], -1, sll.shape[1] if sll.shape[1] > 1 else 1)
    map_n = np.asarray(res["MAP_log_nhis"]).reshape(map_z.shape)
    checked = 0
    for r in range(sll.shape[0]):
        for m in range(1, sll.shape[1] + 1):
            if summ["status"][r, m - 1]:
                continue
            w, ok = R.model_weights(sll[r, m - 1], None if m == 1 else base[r, :m - 1], sll.shape[2])
            assert ok
            if 1.0 / w.sum() <= 0.05:
                continue
            for j in range(m):
                at = (r, m - 1, j)
                assert summ["quantiles_z"][at + (lo,)] <= map_z[at] <= summ["quantiles_z"][at + (hi,)], at
                assert summ["quantiles_log_nhi"][at + (lo,)] <= map_n[at] <= summ["quantiles_log_nhi"][at + (hi,)], at
                checked += 1
    return checked


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
        resident = batch.parameter_summaries()
        picked = batch.parameter_summaries(selection=[2, 0])
    finally:
        batch.close()
        ctx.close()
    host = posteriors.parameter_summaries(res["sample_log_likelihoods_dla"], samples, res["min_z_dlas"], res["max_z_dlas"])
    _same(resident, host, posteriors.FIELDS + ("correlation",))
    for k in posteriors.FIELDS:
        np.testing.assert_array_equal(picked[k], host[k][[2, 0]], err_msg=k)
    assert (host["status"] == 0).all()
    checked = _map_inside(host, res, res["sample_log_likelihoods_dla"], None, samples["log_nhi_samples"])
    print(f"single-DLA batch: ESS {host['effective_samples'].ravel()}, {checked} MAP slots inside [2.5 %, 97.5 %]")
    # the threshold sums against cddf's p for the same window: one bin [t, 25] of log N, no other cut
    sll = res["sample_log_likelihoods_dla"]
    t = 20.3
    ext = R.summaries(sll, samples["offset_samples"], samples["log_nhi_samples"], res["min_z_dlas"], res["max_z_dlas"],
                      thresholds=(t,), extended=True)["exceedance"][:, 0, 0, 0]
    f64 = R.summaries(sll, samples["offset_samples"], samples["log_nhi_samples"], res["min_z_dlas"], res["max_z_dlas"],
                      thresholds=(t,))["exceedance"][:, 0, 0, 0]
    tol = min(max(10 * float(np.max(np.abs(f64 - ext))), 1e-13), 1e-9)
    # cddf's p = exp(sll - shift) p_dla with shift = the row's maximum (exact) and p_dla = 1 / T: the weights w / T
    shift = np.nanmax(sll, axis=1)
    T = np.array([R.model_weights(row, None, row.size)[0].astype(np.longdouble).sum() for row in sll])
    req = cddf.BinRequest("lnhi", (t, 25.0), -1e9, 1e9, -1e9, 1e9, histogram=True)
    p = cddf.bin_posteriors(sll, shift, (1 / T).astype(np.float64), res["min_z_dlas"], res["max_z_dlas"], res["max_z_dlas"],
                            samples["offset_samples"], samples["log_nhi_samples"], [req])[0]["mean"][:, 0]
    dev = np.abs(host["exceedance"][:, 0, 0, 0] - p)
    print(f"P(log N >= {t}): summaries {host['exceedance'][:, 0, 0, 0]}, cddf {p}, |delta| {dev.max():.2e}, tolerance {tol:.2e}")
    assert np.all(np.abs(host["exceedance"][:, 0, 0, 0] - ext) <= tol) and dev.max() <= tol


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
        resident = batch.parameter_summaries(multi=True)
        swapped = batch.parameter_summaries(selection=[1, 0], multi=True)
        sub = batch.parameter_summaries(multi=True, sub_dla=True)
    finally:
        batch.close()
        ctx.close()
    host = posteriors.parameter_summaries(res["sample_log_likelihoods_dla"], samples, res["min_z_dlas"], res["max_z_dlas"],
                                          res["base_sample_inds"])
    _same(resident, host, posteriors.FIELDS + ("correlation",))
    for k in posteriors.FIELDS:
        np.testing.assert_array_equal(swapped[k], host[k][[1, 0]], err_msg=k)
    assert host["status"].shape == (2, 3) and (host["status"] == 0).all()
    assert np.isnan(host["mean_z"][:, 0, 1:]).all() and not np.isnan(host["mean_z"][:, 2, :]).any()
    sub_host = posteriors.parameter_summaries(res["sample_log_likelihoods_lls"], posteriors.sub_dla_samples(samples),
                                              res["min_z_dlas"], res["max_z_dlas"])
    _same(sub, sub_host)
    checked = _map_inside(host, res, res["sample_log_likelihoods_dla"], res["base_sample_inds"], samples["log_nhi_samples"])
    print(f"multi-DLA batch: ESS {host['effective_samples']}, {checked} MAP slots inside [2.5 %, 97.5 %]")


def test_command_line_on_a_processed_multi_dla_file(tmp_path):
    """python -m gp_dla_detection_amd.posteriors, in process: a processed multi-DLA file (the committed
    consumer chunks, combined) -> a summaries file and a JSON catalogue with intervals, equal to the
    in-memory path on the same tables for a block size that splits the run."""
    import glob
    import json
    import os

    from gp_dla_detection_amd import io
    cons = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consumer")
    processed = str(tmp_path / "processed.mat")
    io.combine_processed_chunks(sorted(glob.glob(os.path.join(cons, "processed_qsos_multi_meanfluxsynth_[0-9]*.mat"))), processed)
    inputs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=40, num_samples=24, empty_quasar=None)
    out, js = str(tmp_path / "summaries.mat"), str(tmp_path / "with_intervals.json")
    assert posteriors.main([processed, inputs["paths"]["samples"], out, "--block-size", "7", "--json", js,
                            "--catalog", inputs["paths"]["catalog"]]) == 0
    res = io.load_processed_qsos(processed)
    want = posteriors.parameter_summaries(res["sample_log_likelihoods_dla"], io.load_dla_samples(inputs["paths"]["samples"]),
                                          res["min_z_dlas"], res["max_z_dlas"], res["base_sample_inds"])
    back = io.load_parameter_summaries(out)
    _same(back, want, posteriors.FIELDS + ("correlation",))
    recs = json.load(open(js))
    ref = json.load(open(os.path.join(cons, "expected_predictions_multi_DLAs.json")))
    assert len(recs) == len(ref) and sum(len(r["dlas"]) for r in recs) > 0
    for r in recs:
        for d in r["dlas"]:
            assert d["log_nhi_q0.025"] <= d["log_nhi_q0.5"] <= d["log_nhi_q0.975"] and d["z_dla_std"] >= 0
