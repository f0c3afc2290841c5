"""GPU checks of the absorption distribution against tests/absorption_distribution_restatement.py.
Every comparison is ``lo - EPS <= gpu <= hi + EPS`` on the restatement's bounds, NaN patterns equal; each figure is printed
before it is asserted.  The inputs are host tables, the ones tests/test_absorption_distribution.py shows the bounds to be
tight on."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import absorption_distribution_restatement as D
import production_shapes as ps
import absorption_distribution_groups_worker as worker
import refine_cases as RC

pytestmark = pytest.mark.gpu


def _single(model, samples, spectra, params=None, refine_points=None):
    ctx = gp.Context(0, params or Parameters())
    ctx.set_model(model)
    ctx.set_samples(samples)
    if refine_points is not None:
        ctx.set_refine_points(*refine_points)
    n = len(spectra)
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))


def _multi(model, samples, spectra, params):
    ctx = gp.Context(0, params)
    ctx.set_model(model)
    ctx.set_samples(samples)
    n = len(spectra)
    lp_dla = np.log(np.full((n, params.max_dlas), 0.1) ** np.arange(1, params.max_dlas + 1))
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.85)), lp_dla, np.full(n, np.log(0.05)))


def _bytes_equal(a: dict, b: dict, label=""):
    assert a.keys() == b.keys()
    for name in a:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{label}: {name} differs"


def _masked_out(sp):
    out = dict(sp)
    ps.mask_pixels(out, np.arange(np.asarray(sp["wavelengths"]).size))
    return out


@pytest.mark.parametrize("S", D.SAMPLE_COUNTS)
def test_sample_and_pixel_edges_against_the_restatement(oracle, S):
    cases = [c for c in D.shape_cases() if c[0] == S]
    model, samples, spectra, table = D.case_inputs(S, [c[1] for c in cases], seed=100 + S)
    ctx, batch = _single(model, samples, spectra)
    bad = []
    try:
        for s, ((_, n_u, request), sp, row) in enumerate(zip(cases, spectra, table)):
            got = batch.absorption_distribution(selection=[s], weights=row[None, :], **request)
            assert got["status"][0] == 0 and got["offsets"][1] == n_u
            assert set(got) == {"offsets", "status", "prob_below", "absorption_min", "absorption_max"} | \
                ({"quantiles"} if request.get("levels") else set()) | ({"histogram"} if request.get("histogram") else set())
            want = D.restate_single(oracle, model, samples, sp, row, request)
            bad += D.failures(got, want, slice(0, n_u), f"S={S} n_u={n_u} {sorted(request)}")
    finally:
        batch.close()
        ctx.close()
    assert not bad, bad


def test_production_shape_quasar_all_outputs(oracle):
    """The tile-boundary run of tests/production_shapes.py (968 grid pixels), S = 300, every output at once; the whole
    selection in one call, so that blocks of several quasars share a launch."""
    model, samples, spectra, table = D.production_case()
    request = D.REQUEST_ALL
    ctx, batch = _single(model, samples, spectra)
    try:
        got = batch.absorption_distribution(weights=table, **request)
        plain = batch.absorption_distribution(weights=table, thresholds=D.THRESHOLDS4)
    finally:
        batch.close()
        ctx.close()
    # the kernel without bins and the one with them own different pixel ranges: the same sums in the same order
    _bytes_equal({k: got[k] for k in plain}, plain, "with and without bins")
    bad = []
    for s, want in enumerate(D.production_restated(oracle)):
        bad += D.failures(got, want, slice(got["offsets"][s], got["offsets"][s + 1]), f"quasar {s}")
    assert not bad, bad
    assert np.abs(got["histogram"].sum(axis=0) - 1.0).max() < 1e-12


def test_special_rows(oracle):
    model = synthetic.make_model(20)
    S = 300
    samples = synthetic.make_samples(S)
    base = [synthetic.make_spectrum(5400 + i, 40, model) for i in range(5)]
    spectra = [base[0], _masked_out(base[1]), base[2], base[3], base[4]]
    spectra[4] = dict(spectra[4])
    nv = np.array(spectra[4]["noise_variance"], dtype=np.float64)
    nv[3] = -1.0                                   # a kept pixel of unusable noise variance: status 3
    spectra[4]["noise_variance"] = nv
    rng = np.random.default_rng(6)
    table = np.stack([D.table_row(samples, rng) for _ in spectra])
    table[2, :] = np.nan                           # an all-NaN row
    table[3, :] = np.nan
    table[3, 123] = -7.0                           # a single finite entry
    request = dict(thresholds=(0.8, 0.3), bins=50, levels=(0.16, 0.5, 0.84), histogram=True)
    ctx, batch = _single(model, samples, spectra)
    try:
        got = batch.absorption_distribution(weights=table, **request)
        null = batch.absorption_distribution(weights=None, components=("null",), **request)
    finally:
        batch.close()
        ctx.close()
    off = got["offsets"]
    print("status", got["status"])
    np.testing.assert_array_equal(got["status"], [0, 1, 0, 0, 3])
    for s in (1, 2, 4):
        for name in ("prob_below", "absorption_min", "absorption_max", "histogram", "quantiles"):
            assert np.isnan(got[name][..., off[s]:off[s + 1]]).all(), (s, name)
    for s in (0, 3):
        for name in ("prob_below", "absorption_min", "absorption_max", "histogram", "quantiles"):
            assert np.isfinite(got[name][..., off[s]:off[s + 1]]).all(), (s, name)
    # one live sample: the distribution is one atom
    sl = slice(off[3], off[4])
    g = D.grid(oracle, model, spectra[3])
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"][123]
    a = np.clip(oracle.voigt(g["pad"], z, samples["nhi_samples"][123], 3), 0, 1)
    assert np.isin(got["prob_below"][:, sl], (0.0, 1.0)).all()
    assert np.array_equal(got["absorption_min"][sl], got["absorption_max"][sl])
    assert np.abs(got["absorption_min"][sl] - a).max() <= D.DELTA
    assert np.abs(got["quantiles"][:, sl] - a).max() <= D.DELTA
    want = D.restate_single(oracle, model, samples, spectra[0], table[0], request)
    assert not D.failures(got, want, slice(off[0], off[1]), "quasar 0")
    # the null-only mixture, no weights source: exact values (NaN rows where the quasar has no usable pixel)
    live = np.concatenate([np.full(off[s + 1] - off[s], null["status"][s] == 0) for s in range(5)])
    np.testing.assert_array_equal(null["status"], [0, 1, 0, 0, 3])
    assert (null["prob_below"][:, live] == 0).all()
    assert (null["histogram"][:-1][:, live] == 0).all() and (null["histogram"][-1, live] == 1).all()
    for name in ("absorption_min", "absorption_max", "quantiles"):
        assert (null[name][..., live] == 1).all(), name
        assert np.isnan(null[name][..., ~live]).all(), name


def test_three_component_mixture_and_a_component_of_weight_zero(oracle):
    model, samples, spectra, dla, lls, pw = D.mixture_case()
    request = D.REQUEST_MIX
    ctx, batch = _single(model, samples, spectra)
    try:
        got = batch.absorption_distribution(weights={"dla": dla, "sub_dla": lls}, components=("null", "sub_dla", "dla"),
                                            model_weights=pw, **request)
        # a component nobody weighs is not evaluated: its table may hold anything
        pw0 = np.array([[0.4, 0.0, 0.6], [0.0, 0.0, 1.0]])
        zero = batch.absorption_distribution(weights={"dla": dla, "sub_dla": np.full_like(lls, np.nan)},
                                             components=("null", "sub_dla", "dla"), model_weights=pw0, **request)
        same = batch.absorption_distribution(weights={"dla": dla}, components=("null", "dla"), model_weights=pw0, **request)
    finally:
        batch.close()
        ctx.close()
    assert all(np.isfinite(zero[k]).all() for k in ("prob_below", "histogram", "quantiles", "absorption_min"))
    _bytes_equal(zero, same, "a zero-weight component")
    bad = []
    for s, want in enumerate(D.mixture_restated(oracle)):
        bad += D.failures(got, want, slice(got["offsets"][s], got["offsets"][s + 1]), f"mixture quasar {s}")
    assert not bad, bad
    assert (got["absorption_max"] == 1.0).all()           # the null atom


def test_refined_source(oracle):
    """Two levels, S' = 300: the DLA component on the refine points mapped through each quasar's last box, weighted by its
    resident refined row; a quasar outside the refine selection gets NaN rows and the NOT_REFINED bit."""
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(300)
    spectra = [synthetic.make_spectrum(5600 + i, 65, model) for i in range(3)]
    u, v = RC.halton_points(300)
    request = dict(thresholds=(0.8, 0.5), bins=64, levels=(0.16, 0.5, 0.84), histogram=True)
    ctx, batch = _single(model, samples, spectra, refine_points=(u, v))
    try:
        batch.process()
        ref = batch.refine(selection=[0, 2], levels=2)
        got = batch.absorption_distribution(weights="refined", **request)
    finally:
        batch.close()
        ctx.close()
    off = got["offsets"]
    assert got["status"][1] == _lib.SPECTRA_NOT_REFINED and np.isnan(got["prob_below"][:, off[1]:off[2]]).all()
    assert np.isnan(got["quantiles"][:, off[1]:off[2]]).all()
    bad = []
    for j, s in enumerate((0, 2)):
        assert ref["status"][j] == 0 and got["status"][s] == 0
        g = D.grid(oracle, model, spectra[s])
        z_lo, z_hi, n_lo, n_hi = ref["boxes"][j, -1]
        z, N = z_lo + (z_hi - z_lo) * u, 10.0 ** (n_lo + (n_hi - n_lo) * v)
        A = np.stack([oracle.voigt(g["pad"], z[i], N[i], 3) for i in range(u.size)])
        w = D.weights(ref["sample_log_posteriors_refined"][j])
        want = D.distribution([(1.0, w, A)], 0.0, g["n_u"], request["thresholds"], request["bins"], request["levels"])
        bad += D.failures(got, want, slice(off[s], off[s + 1]), f"refined quasar {s}")
    assert not bad, bad


def test_all_models_of_a_multi_dla_run(oracle):
    """max_dlas = 3, S = 300, processed by process_multi; quasar 1 also from host tables whose base rows make DLA(2) and
    DLA(3) carry weight."""
    params, model, samples, spectra, t2, pw = D.multi_case()
    request = D.REQUEST_MIX
    ctx, batch = _multi(model, samples, spectra, params)
    try:
        batch.process_multi()
        out = batch.download_multi()
        resident = batch.absorption_distribution_multi(**request)
        tables = {k: np.array(out[k]) for k in ("sample_log_likelihoods_dla", "base_sample_inds", "sample_log_likelihoods_lls")}
        host = batch.absorption_distribution_multi(tables=tables, model_weights=out["model_posteriors"], **request)
        # host tables of our own: peaked rows for every model, base rows that draw (almost) everywhere
        own = batch.absorption_distribution_multi(tables=t2, model_weights=pw, **request)
        flat = dict(t2, sample_log_likelihoods_dla=t2["sample_log_likelihoods_dla"].copy())
        flat["sample_log_likelihoods_dla"][0, 1, :] = np.nan    # DLA(2) of quasar 0 has no weights
        flagged = batch.absorption_distribution_multi(tables=flat, model_weights=pw, **request)
    finally:
        batch.close()
        ctx.close()
    _bytes_equal(resident, host, "resident and host tables")
    assert flagged["model_flags"][0] == 2 and flagged["model_flags"][1] == 0 and flagged["status"][0] == 0
    assert np.isnan(flagged["prob_below"][:, :flagged["offsets"][1]]).all()
    _bytes_equal({k: v[..., own["offsets"][1]:] for k, v in own.items() if k in ("prob_below", "histogram", "quantiles")},
                 {k: v[..., own["offsets"][1]:] for k, v in flagged.items() if k in ("prob_below", "histogram", "quantiles")}, "quasar 1")
    assert (own["model_flags"] == 0).all()
    bad = []
    for s, want in enumerate(D.multi_restated(oracle)):
        bad += D.failures(own, want, slice(own["offsets"][s], own["offsets"][s + 1]), f"multi quasar {s}")
    assert not bad, bad


def test_bit_identity():
    """Two runs; a permuted selection; the resident and the host form of the same table."""
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(300)
    spectra = [synthetic.make_spectrum(5800 + i, n, model, mask_fraction=0.05) for i, n in enumerate((65, 17, 300, 64))]
    request = dict(thresholds=D.THRESHOLDS4, bins=64, levels=D.LEVELS8, histogram=True)
    ctx, batch = _single(model, samples, spectra)
    try:
        batch.process()
        rows = np.array(batch.download()["sample_log_likelihoods_dla"])
        a = batch.absorption_distribution(**request)
        b = batch.absorption_distribution(**request)
        host = batch.absorption_distribution(weights=rows, **request)
        perm = np.array([2, 0, 3, 1])
        c = batch.absorption_distribution(selection=perm, **request)
        one = [batch.absorption_distribution(selection=[q], **request) for q in range(4)]
    finally:
        batch.close()
        ctx.close()
    _bytes_equal(a, b, "two runs")
    _bytes_equal(a, host, "resident and host table")
    assert np.isfinite(a["prob_below"]).all() and (a["prob_below"] >= 0).all() and (a["prob_below"] <= 1).all()
    assert (np.diff(a["quantiles"], axis=0) >= 0).all()
    for j, q in enumerate(perm):
        for name in ("prob_below", "absorption_min", "absorption_max", "histogram", "quantiles"):
            x = a[name][..., a["offsets"][q]:a["offsets"][q + 1]]
            y = c[name][..., c["offsets"][j]:c["offsets"][j + 1]]
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (name, q)
            assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(one[q][name]).view(np.uint8)), (name, q)


def test_production_scale(oracle):
    """64 quasars x 1500 pixels x 10^4 samples (the production sample count: 157 groups of 64 samples a block walks):
    thresholds and a 64-bin histogram; invariants everywhere, three quasars against the restatement -- each on a window of
    80 pixels that straddles multiples of 64, the seams of the kernel's pixel ranges (D.SCALE_WINDOWS: pixels 0 .. 80 across
    64; 696 .. 776 across 704 and 768; the last 80 across 1472): the restatement of all 1500 pixels of one quasar takes nine
    seconds, and a pixel's comparison does not depend on its neighbours'."""
    case = D.scale_case()
    model, samples, spectra, table = case
    request = D.REQUEST_MIX
    ctx, batch = _single(model, samples, spectra)
    try:
        got = batch.absorption_distribution(weights=table, **request)
        plain = batch.absorption_distribution(weights=table, thresholds=request["thresholds"])
    finally:
        batch.close()
        ctx.close()
    assert (got["status"] == 0).all() and got["offsets"][-1] == 64 * 1500
    assert (got["prob_below"] >= 0).all() and (got["prob_below"] <= 1).all()
    worst = np.abs(got["histogram"].sum(axis=0) - 1.0).max()
    print(f"histogram sums: worst |sum - 1| {worst:.3e}")
    assert worst < 1e-9
    assert (np.diff(got["quantiles"], axis=0) >= 0).all()
    assert (got["prob_below"][0] >= got["prob_below"][1]).all()
    _bytes_equal({k: got[k] for k in plain}, plain, "with and without bins")   # (the 64-pixel ranges of the kernel without bins)
    bad = []
    for (s, first), want in zip(D.SCALE_WINDOWS, D.scale_restated(oracle, case)):
        lo = got["offsets"][s] + first
        bad += D.failures(got, want, slice(lo, lo + 80), f"scale quasar {s} pixels {first}..{first + 80}")
    assert not bad, bad


def test_driver_equals_the_batch_path(tmp_path):
    """api.absorption_distribution block by block (two quasars a block) returns the bytes of one Batch call, single and
    multi_models; an empty selection returns the same keys with no extent; the saver takes what the driver returns."""
    from gp_dla_detection_amd import api, io
    model = synthetic.make_model(20)
    S = 300
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(6000 + i, n, model) for i, n in enumerate((65, 17, 33, 64, 40))]
    rng = np.random.default_rng(5)
    table = np.stack([D.table_row(samples, rng) for _ in spectra])
    pw = np.tile([0.3, 0.0, 0.7], (5, 1))
    request = dict(thresholds=(0.8, 0.5), bins=64, levels=(0.16, 0.5, 0.84), histogram=True)
    sel = np.array([4, 0, 2, 3])
    ctx, batch = _single(model, samples, spectra)
    try:
        want = batch.absorption_distribution(selection=sel, weights=table[sel], components=("null", "dla"), model_weights=pw[sel],
                                             **request)
    finally:
        batch.close()
        ctx.close()
    results = {"sample_log_likelihoods_dla": table}
    got = api.absorption_distribution(model, samples, spectra, results, selection=sel, components=("null", "dla"),
                                      model_weights=pw, max_quasars_per_batch=2, **request)
    np.testing.assert_array_equal(got.pop("selection"), sel)
    _bytes_equal(got, want, "driver")
    mask = gp.forest_mask(got, threshold_index=1, probability=0.5)
    assert mask.shape == got["absorption_min"].shape and mask.dtype == bool
    empty = api.absorption_distribution(model, samples, spectra, results, selection=[], components=("null", "dla"),
                                        model_weights=pw, **request)
    assert set(empty) == set(want) | {"selection"}
    assert empty["prob_below"].shape == (2, 0) and empty["quantiles"].shape == (3, 0) and empty["histogram"].shape == (64, 0)
    path = str(tmp_path / "dist.mat")
    io.save_absorption_distribution(path, dict(got, selection=sel), thresholds=request["thresholds"], levels=request["levels"],
                                    num_bins=64)
    back = io.loadmat73(path)
    np.testing.assert_array_equal(np.asarray(back["histogram"][1]), want["histogram"][:, want["offsets"][1]:want["offsets"][2]].T)

    # multi_models
    params = MultiParameters(max_dlas=3)
    t2 = dict(sample_log_likelihoods_dla=np.stack([[D.table_row(samples, rng) for _ in range(3)] for _ in spectra]),
              sample_log_likelihoods_lls=np.stack([D.table_row(samples, rng) for _ in spectra]),
              base_sample_inds=rng.integers(1, S + 1, size=(5, 2, S)).astype(np.uint32))
    pw5 = np.tile([0.1, 0.1, 0.3, 0.3, 0.2], (5, 1))
    ctx, batch = _multi(model, samples, spectra, params)
    try:
        want = batch.absorption_distribution_multi(selection=sel, tables={k: v[sel] for k, v in t2.items()}, model_weights=pw5[sel],
                                                   **request)
    finally:
        batch.close()
        ctx.close()
    got = api.absorption_distribution(model, samples, spectra, dict(t2, model_posteriors=pw5), params=params, selection=sel,
                                      multi_models=True, max_quasars_per_batch=3, **request)
    got.pop("selection")
    _bytes_equal(got, want, "driver, multi_models")


def test_bit_identity_across_launch_groups(tmp_path):
    """One launch group against many: the calls of tests/absorption_distribution_groups_worker.py in this process with the
    product library, and in a clean child process that loads libgpdla_legacy.so with its debug-only budget
    GPDLA_MC_SCRATCH_BYTES shrunk to two quasars' weight rows of the single-DLA entry (three groups of the five quasars;
    the multi entry, with four sampled components, then takes one quasar a group)."""
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    want = worker.run_case()
    out = tmp_path / "groups.npz"
    env = {"GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH, "GPDLA_MC_SCRATCH_BYTES": str(worker.BUDGET)}
    pr = mp.get_context("forkserver").Process(target=worker.run_child, args=(env, str(out)))
    pr.start()
    pr.join(300)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
        raise AssertionError("the child process did not finish")
    assert pr.exitcode == 0
    got = np.load(out)
    assert set(got.files) == set(want)
    for name in want:
        x, y = np.ascontiguousarray(got[name]), np.ascontiguousarray(np.asarray(want[name]))
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    for prefix in ("", "host_", "multi_"):
        assert want[prefix + "status"].tolist() == [0] * 5
        for name in worker.ARRAYS:
            assert np.isfinite(want[prefix + name]).all(), prefix + name
    assert (want["multi_model_flags"] == 0).all()
    np.testing.assert_array_equal(np.diff(want["host_offsets"]), [worker.NUS[q] for q in worker.HOST_SELECTION])
    for name in ("prob_below", "absorption_min", "absorption_max"):
        assert np.array_equal(want["plain_" + name], want["host_" + name]), name


@pytest.mark.parametrize("multi", [False, True])
def test_command_line_run_equals_the_in_memory_call(tmp_path, multi):
    """python -m gp_dla_detection_amd.model_spectra --absorption-distribution on the -v7.3 files of a run, in batches of 3:
    the file holds what api.absorption_distribution returns for the same quasars in memory; a single-DLA run mixes
    (null, dla) by the posteriors, a multi-DLA run goes through --multi-models."""
    from gp_dla_detection_amd import io, model_spectra as cli
    fs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=12, num_samples=96)
    run_pos = np.flatnonzero(fs["test_ind"])
    spectra = [fs["spectra"][i] for i in run_pos]
    z = fs["catalog"]["z_qsos"][run_pos]
    processed = str(tmp_path / "processed.mat")
    if multi:
        p = MultiParameters(max_dlas=3)
        lp = gp.dla_existence_prior_multi(fs["prior"]["z_qsos"], fs["prior"]["dla_ind"], z, fs["Z_lls"], fs["Z_dla"], p)
        results = gp.process_qsos_multiple_dlas_meanflux(fs["model"], fs["samples"], spectra, lp, params=p)
        io.save_processed_qsos_multi(processed, results, test_ind=fs["test_ind"])
        more, kw = ["--multi-models"], dict(multi_models=True)
    else:
        p = Parameters()
        results = gp.process_qsos(fs["model"], fs["samples"], spectra, prior_catalog=fs["prior"])
        io.save_processed_qsos(processed, results, test_ind=fs["test_ind"])
        more, kw = ["--components", "null,dla"], dict(components=("null", "dla"), model_weights="posteriors")
    idx = [int(run_pos.size - 1), 0, 3, 5]
    out = str(tmp_path / "absorption_distribution.mat")
    rc = cli.main(["--preloaded", fs["paths"]["preloaded"], "--catalog", fs["paths"]["catalog"], "--model", fs["paths"]["learned"],
                   "--samples", fs["paths"]["samples"], "--processed", processed, "--out", out, "--indices", ",".join(map(str, idx)),
                   "--absorption-distribution", "--thresholds", "0.8,0.5", "--bins", "50", "--quantile-levels", "0.16,0.5,0.84",
                   "--histogram", "--max-quasars-per-batch", "3"] + more)
    assert rc == 0
    sel = np.array(sorted(idx))
    want = gp.absorption_distribution(fs["model"], fs["samples"], spectra, results, params=p, selection=sel, thresholds=(0.8, 0.5),
                                      bins=50, levels=(0.16, 0.5, 0.84), histogram=True, **kw)
    back = io.loadmat73(out)
    off = want["offsets"]
    np.testing.assert_array_equal(np.asarray(back["quasar_ind"]).reshape(-1) - 1, sel)
    np.testing.assert_array_equal(np.asarray(back["num_pixels"]).reshape(-1), np.diff(off))
    np.testing.assert_array_equal(np.asarray(back["status"]).reshape(-1), want["status"])
    np.testing.assert_array_equal(np.asarray(back["thresholds"]).reshape(-1), [0.8, 0.5])
    np.testing.assert_array_equal(np.asarray(back["levels"]).reshape(-1), [0.16, 0.5, 0.84])
    assert float(np.asarray(back["num_bins"]).reshape(-1)[0]) == 50
    if multi:
        np.testing.assert_array_equal(np.asarray(back["model_flags"]).reshape(-1), want["model_flags"])
    for name, planes in (("prob_below", 2), ("quantiles", 3), ("histogram", 50)):
        assert want[name].shape == (planes, off[-1])
        for i in range(sel.size):
            ref = want[name][:, off[i]:off[i + 1]].T
            got = np.asarray(back[name][i], dtype=np.float64)
            assert got.size == ref.size, name
            if ref.size:
                assert got.shape == ref.shape, (name, got.shape, ref.shape)
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(ref).view(np.uint8)), (name, i)
    for name in ("absorption_min", "absorption_max"):
        for i in range(sel.size):
            got = np.asarray(back[name][i], dtype=np.float64).reshape(-1)
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want[name][off[i]:off[i + 1]]).view(np.uint8)), (name, i)
    usable = want["status"] == 0
    assert usable.any() and np.isfinite(want["prob_below"][:, :off[np.flatnonzero(usable)[0] + 1]]).all()
