"""GPU checks of the posterior predictive flux (csrc/predictive_flux_kernels.hpp) against the NumPy-and-oracle
restatement tests/predictive_flux_restatement.py in its DENSE form.  Tolerances are not fixed in advance: per product
family (the mean; the variances) ``R.continuum_tolerance`` of the restatement's own dense-vs-Woodbury disagreement on the
same cases.  Every figure is printed before it is asserted; NaN and status patterns must match exactly."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import marginal_continuum_cases as MC
import model_spectra_edge_cases as E
import model_spectra_restatement as R
import predictive_flux_cases as PC
import predictive_flux_groups_worker as worker
import predictive_flux_restatement as PR

pytestmark = pytest.mark.gpu

ALL = PR.PRODUCTS


def _batch(model, samples, spectra, params):
    ctx = gp.Context(0, params)
    ctx.set_model(model)
    ctx.set_samples(samples)
    n = len(spectra)
    if isinstance(params, MultiParameters):
        lp_dla = np.log(np.full((n, params.max_dlas), 0.1) ** np.arange(1, params.max_dlas + 1))
        return ctx, ctx.upload(spectra, np.full(n, np.log(0.85)), lp_dla, np.full(n, np.log(0.05)))
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))


def _sweep_tables(batch, multi):
    if multi:
        batch.process_multi()
        out = batch.download_multi()
        return {"dla": np.array(out["sample_log_likelihoods_dla"][:, 0, :]), "sub_dla": np.array(out["sample_log_likelihoods_lls"])}
    batch.process()
    return {"dla": np.array(batch.download()["sample_log_likelihoods_dla"])}


def _compare(label, got, want, products=ALL):
    """Worst deviation per product of the GPU's per-quasar dicts from the dense restatement, against the tolerance of the
    restatement's own disagreement; statuses exact."""
    dis = PC.disagreement(want)
    tol = PR.tolerances(dis)
    worst = {n: max(PR.deviation(g[n], w[n]) for g, w in zip(got, want["dense"])) for n in products}
    for n in products:
        print(f"{label} {n}: dense-vs-Woodbury {dis[n]:.2e} -> tolerance {tol[n]:.2e}; GPU worst |delta| {worst[n]:.3e}")
    assert [g["status"] for g in got] == [w["status"] for w in want["dense"]]
    for n in products:
        assert worst[n] < tol[n], (label, n, worst[n], tol[n])


def _consistent(res):
    ok = np.isfinite(res["flux_mean"])
    assert (res["flux_var"][ok] == res["flux_var_within"][ok] + res["flux_var_between"][ok]).all()
    assert (res["flux_var_between"][ok] >= 0).all() and (res["flux_var_within"][ok] >= 0).all()


# ------------------------------------------------------------------------------------------------
# every product against the dense restatement
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s["name"] for s in PC.SETUPS])
def test_all_products_against_the_dense_restatement(oracle, name):
    """The five per-pixel arrays, weights from the batch's own (resident) table after the sweep."""
    st = PC.setup(name)
    model, samples, spectra = PC.build(st)
    comp = st["table"]
    ctx, batch = _batch(model, samples, spectra, PC.params(st))
    try:
        if comp == "sub_dla" and not st["multi"]:     # a single-DLA batch has no resident sub-DLA table: the host form
            tables = {"sub_dla": _sweep_tables(batch, False)["dla"] * 0.5 - 3.0}
            res = batch.predictive_flux(weights=tables["sub_dla"], components=(comp,))
        else:
            tables = _sweep_tables(batch, st["multi"])
            res = batch.predictive_flux(weights="resident", components=(comp,))
    finally:
        batch.close()
        ctx.close()
    pw = [0.0, 1.0, 0.0] if comp == "sub_dla" else [0.0, 0.0, 1.0]
    want = PC.wanted(oracle, name, model, samples, spectra, tables, pw, st["multi"], st["lines"])
    np.testing.assert_array_equal(np.diff(res["offsets"]), [w["flux_mean"].size for w in want["dense"]])
    _compare(name, PC.split(res), want)
    _consistent(res)


# ------------------------------------------------------------------------------------------------
# weight rows
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PC.ROW_SETUPS, ids=lambda c: f"k{c['k']}_S{c['S']}")
def test_weight_rows(oracle, case):
    """A host table over a repeated selection: the sweep's row, a flat row, every second entry NaN, one-hot rows at the
    edges of the sample chunks in z order, rows with 1 and the packing width +- 1 live samples, and the three rows without
    weights.  A one-hot row is the model flux of that sample's absorber (Batch.model_spectra: absorption x continuum) with no
    between-variance at all."""
    k, S = case["k"], case["S"]
    st = dict(k=k, S=S, nus=case["nus"], lines=3, multi=False)
    model, samples, spectra = PC.build(st)
    kinds = PC.row_kinds(S)
    sel = np.array([i % len(spectra) for i in range(len(kinds))], dtype=np.int64)
    order = E.z_order(samples)
    ctx, batch = _batch(model, samples, spectra, Parameters())
    try:
        sweep = _sweep_tables(batch, False)["dla"]
        out = batch.download()
        rows = np.array([PC.make_row(kind, S, samples, sweep[q]) for q, kind in zip(sel, kinds)])
        res = batch.predictive_flux(selection=sel, weights=rows)
        hot = [(j, kind[1]) for j, kind in enumerate(kinds) if isinstance(kind, tuple) and kind[0] == "hot"]
        i_hot = np.array([order[pos] for _, pos in hot])
        q_hot = sel[[j for j, _ in hot]]
        z_hot = out["min_z_dlas"][q_hot] + (out["max_z_dlas"][q_hot] - out["min_z_dlas"][q_hot]) * samples["offset_samples"][i_hot]
        cond = batch.model_spectra(selection=q_hot, absorbers=(np.arange(len(hot) + 1), z_hot, samples["log_nhi_samples"][i_hot]),
                                   products=("continuum",))
    finally:
        batch.close()
        ctx.close()
    got = PC.split(res)
    for j, kind in enumerate(kinds):
        if isinstance(kind, tuple) and kind[0] == "live":
            assert (R.weights(rows[j]) > 0).sum() == kind[1]
    want = PC.wanted(oracle, ("rows", k, S), model, samples, [spectra[q] for q in sel], {"dla": rows}, [0, 0, 1], False, 3)
    _compare(f"rows k={k} S={S}", got, want)
    _consistent(res)
    tol = PR.tolerances(PC.disagreement(want))["flux_mean"]
    for j, kind in enumerate(kinds):
        if kind in E.NAN_ROWS:
            assert got[j]["status"] == 0 and all(np.isnan(got[j][n]).all() for n in ALL), kind
    cells = gp.split_cells(cond["model_flux"], cond["offsets"])
    for (j, pos), cell in zip(hot, cells):
        d = PR.deviation(got[j]["flux_mean"], cell)
        print(f"one-hot at z position {pos}: |flux_mean - model_spectra model_flux| {d:.2e} (tolerance {tol:.2e})")
        assert d < tol
        assert (got[j]["flux_var_between"] == 0).all() and (got[j]["flux_var"] == got[j]["flux_var_within"]).all()


def test_zero_weight_samples_are_skipped(oracle):
    """All but three samples at l = -1e6 (weight exactly 0); one of the skipped samples has a NaN column density, so its
    profile is NaN and its B_i would not be positive definite if it were touched.  The result is the three-sample restatement:
    finite, status 0."""
    k, S = 20, PC.SKIP_S
    model = synthetic.make_model(k)
    samples = dict(synthetic.make_samples(S))
    order = E.z_order(samples)
    samples["nhi_samples"] = np.array(samples["nhi_samples"])
    samples["nhi_samples"][order[PC.SKIP_POISON]] = np.nan
    spectra = [synthetic.make_spectrum(6300, 65, model, mask_fraction=0.05), synthetic.make_spectrum(6302, 33, model)]
    rows = np.tile(PC.skip_row(samples), (2, 1))
    ctx, batch = _batch(model, samples, spectra, Parameters())
    try:
        res = batch.predictive_flux(weights=rows)
        poisoned = np.array(rows)
        poisoned[:, order[PC.SKIP_POISON]] = -3.0          # the same sample WITH weight: status 4, NaN rows
        bad = batch.predictive_flux(weights=poisoned)
    finally:
        batch.close()
        ctx.close()
    want = PC.wanted(oracle, "skip", model, samples, spectra, {"dla": rows}, [0, 0, 1], False, 3)
    assert res["status"].tolist() == [0, 0] and all(np.isfinite(res[n]).all() for n in PR.PRODUCTS_MEAN + PR.PRODUCTS_VAR[:3])
    _compare("skip", PC.split(res), want)
    assert bad["status"].tolist() == [4, 4] and all(np.isnan(bad[n]).all() for n in ALL)


# ------------------------------------------------------------------------------------------------
# mixing
# ------------------------------------------------------------------------------------------------

def test_mixing(oracle):
    k, S = 20, 65
    st = dict(k=k, S=S, nus=(5, 33, 65), lines=3, multi=False)
    model, samples, spectra = PC.build(st)
    n = len(spectra)
    rng = np.random.default_rng(11)
    ctx, batch = _batch(model, samples, spectra, Parameters())
    try:
        dla = _sweep_tables(batch, False)["dla"]
        tables = {"dla": dla, "sub_dla": dla * 0.7 + rng.normal(0, 1.0, dla.shape)}
        null = batch.predictive_flux(components=("null",), weights=None)
        mc_null = batch.marginal_continuum(components=("null",), weights=None)
        default = batch.predictive_flux(weights="resident")
        dla_only = batch.predictive_flux(weights=tables, components=("null", "sub_dla", "dla"), model_weights=np.tile([0.0, 0.0, 1.0], (n, 1)))
        pw = np.array([[0.2, 0.3, 0.5], [1.0, 2.0, 1.0], [0.6, 0.0, 0.4]])
        three = batch.predictive_flux(weights=tables, components=("null", "sub_dla", "dla"), model_weights=pw)
        nan_lls = dict(tables, sub_dla=np.full(dla.shape, np.nan))
        ignored = batch.predictive_flux(weights=nan_lls, components=("null", "sub_dla", "dla"), model_weights=np.tile([0.5, 0.0, 0.5], (n, 1)))
        flagged = batch.predictive_flux(weights=nan_lls, components=("null", "sub_dla", "dla"), model_weights=np.tile([0.5, 1e-300, 0.5], (n, 1)))
        with_res = batch.predictive_flux(weights=tables, components=("null", "sub_dla", "dla"), model_weights=pw, residuals=True)
        y, kept = batch.grid_flux()
    finally:
        batch.close()
        ctx.close()
    # (1, 0, 0): a = 1, so the flux is the null continuum of the marginal continuum, the same c_0 and Sigma_0 from the same
    # functions (csrc/continuum_solve.hpp): bit for bit
    d_mean = PR.deviation(null["flux_mean"], mc_null["continuum_mean"])
    d_var = PR.deviation(null["flux_var"], mc_null["continuum_var"])
    print(f"(1, 0, 0) against the null continuum of marginal_continuum: |delta mean| {d_mean:.2e}, |delta var| {d_var:.2e}")
    np.testing.assert_array_equal(null["flux_mean"], mc_null["continuum_mean"])
    np.testing.assert_array_equal(null["flux_var"], mc_null["continuum_var"])
    assert (null["flux_var_between"] == 0).all()
    assert (null["flux_var"] > 0).all() and null["status"].tolist() == [0] * n
    for name in ALL:
        np.testing.assert_array_equal(default[name], dla_only[name], err_msg=name)
    want = PC.wanted(oracle, "mixing", model, samples, spectra, tables, pw, False, 3)
    _compare("three-way", PC.split(three), want)
    _consistent(three)
    assert all(np.isfinite(ignored[n_]).all() for n_ in ALL[:4]) and ignored["status"].tolist() == [0] * n
    assert all(np.isnan(flagged[n_]).all() for n_ in ALL) and flagged["status"].tolist() == [0] * n
    # residuals: formed from the arrays above, NaN exactly on the masked pixels
    for name in ALL:
        np.testing.assert_array_equal(with_res[name], three[name], err_msg=name)
    assert not kept.all() and np.array_equal(np.isnan(three["noise_var"]), ~kept)
    assert np.array_equal(np.isnan(with_res["residual"]), ~kept)
    np.testing.assert_array_equal(with_res["residual"][kept], ((y - three["flux_mean"]) / np.sqrt(three["flux_var"] + three["noise_var"]))[kept])
    assert with_res["num_kept"].tolist() == [int(kept[a:b].sum()) for a, b in zip(three["offsets"][:-1], three["offsets"][1:])]
    np.testing.assert_allclose(with_res["chi2"], [np.nansum(with_res["residual"][a:b] ** 2) for a, b in zip(three["offsets"][:-1], three["offsets"][1:])], rtol=1e-14)


def test_nan_rows_of_unusable_quasars():
    """Prepare status 1 (no kept pixel): NaN rows with that status, whatever the mixture."""
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(16)
    good = synthetic.make_spectrum(6400, 40, model)
    ctx, batch = _batch(model, samples, [good, E.masked_out(good)], Parameters())
    try:
        batch.process()
        res = batch.predictive_flux(weights="resident", components=("null", "dla"))
    finally:
        batch.close()
        ctx.close()
    got = PC.split(res)
    assert res["status"].tolist() == [0, 1]
    assert all(np.isfinite(got[0][n]).all() for n in ALL) and all(np.isnan(got[1][n]).all() for n in ALL)
    assert got[1]["flux_mean"].size == got[0]["flux_mean"].size


def test_conditioned_batch_is_refused():
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(16)
    spectra = [synthetic.make_spectrum(6410, 40, model)]
    ctx, batch = _batch(model, samples, spectra, Parameters())
    try:
        batch.process()
        out = batch.download()
        z = out["min_z_dlas"] + 0.5 * (out["max_z_dlas"] - out["min_z_dlas"])
        batch.set_fixed_absorbers((np.array([0, 1]), z, np.array([20.5])))
        with pytest.raises(gp._lib.GpdlaError) as err:
            batch.predictive_flux(components=("null",), weights=None)
        assert err.value.code == gp._lib.ERR_UNSUPPORTED and "conditioned" in str(err.value)
        batch.set_fixed_absorbers(None)
        batch.process()
        assert np.isfinite(batch.predictive_flux(weights="resident")["flux_mean"]).all()
    finally:
        batch.close()
        ctx.close()


# ------------------------------------------------------------------------------------------------
# multi-DLA batch
# ------------------------------------------------------------------------------------------------

def test_multi_dla_batch_resident_tables(oracle):
    """The resident DLA(1) and sub-DLA tables of a multi-DLA batch, mean-flux rows by default, mixed with the null model."""
    k, S = 20, 65
    st = dict(k=k, S=S, nus=(5, 33, 65), lines=3, multi=True)
    model, samples, spectra = PC.build(st)
    p = MultiParameters(max_dlas=2)
    pw = np.array([[0.1, 0.3, 0.6], [0.0, 0.5, 0.5], [0.3, 0.7, 0.0]])
    ctx, batch = _batch(model, samples, spectra, p)
    try:
        tables = _sweep_tables(batch, True)
        res = batch.predictive_flux(weights="resident", components=("null", "sub_dla", "dla"), model_weights=pw)
        host = batch.predictive_flux(weights=tables, components=("null", "sub_dla", "dla"), model_weights=pw)
    finally:
        batch.close()
        ctx.close()
    for name in ALL:
        np.testing.assert_array_equal(res[name], host[name], err_msg=name)
    want = PC.wanted(oracle, "multi", model, samples, spectra, tables, pw, True, 3)
    _compare("multi-DLA", PC.split(res), want)
    _consistent(res)


# ------------------------------------------------------------------------------------------------
# bit identity
# ------------------------------------------------------------------------------------------------

def test_bit_identity_selection_order_and_weights_source():
    st = dict(k=20, S=130, nus=(5, 33, 65, 129, 31), lines=3, multi=False)
    model, samples, spectra = PC.build(st)
    ctx, batch = _batch(model, samples, spectra, Parameters())
    try:
        rows = _sweep_tables(batch, False)["dla"]
        a = batch.predictive_flux(weights="resident", components=("null", "dla"))
        b = batch.predictive_flux(weights=rows, components=("null", "dla"))
        perm = np.random.default_rng(3).permutation(len(spectra))
        c = batch.predictive_flux(selection=perm, weights="resident", components=("null", "dla"))
        one = batch.predictive_flux(selection=[3], weights="resident", components=("null", "dla"))
    finally:
        batch.close()
        ctx.close()
    assert np.isfinite(a["flux_var"]).all()
    for name in ALL:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    sa, sc, so = PC.split(a), PC.split(c), PC.split(one)
    for j, q in enumerate(perm):
        for name in ALL:
            np.testing.assert_array_equal(sc[j][name], sa[q][name], err_msg=name)
    for name in ALL:
        np.testing.assert_array_equal(so[0][name], sa[3][name], err_msg=name)


def test_bit_identity_across_launch_groups(tmp_path):
    """One call of the product library against the same call in a clean child process that loads libgpdla_legacy.so with
    its debug-only budget GPDLA_MC_SCRATCH_BYTES shrunk to two quasars' scratch rows: three launch groups."""
    from gp_dla_detection_amd import _lib
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    want = worker.run_case()
    k, S = worker.K, worker.S
    budget = 2 * S * (k * (k + 1) // 2 + k) * 8
    out = tmp_path / "groups.npz"
    env = {"GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH, "GPDLA_MC_SCRATCH_BYTES": str(budget)}
    pr = mp.get_context("forkserver").Process(target=worker.run_child, args=(env, str(out)))
    pr.start()
    pr.join(300)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
        raise AssertionError("the child process did not finish")
    assert pr.exitcode == 0
    got = np.load(out)
    for name in ALL + ("status", "offsets"):
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    assert np.isfinite(want["flux_var"]).all()
    # host tables (null, sub-DLA and DLA under an unsorted selection): staged one launch group at a time
    for name in ALL + ("status", "offsets"):
        np.testing.assert_array_equal(got["host_" + name], want["host_" + name], err_msg="host_" + name)
    assert np.isfinite(want["host_flux_var"]).all() and want["host_status"].tolist() == [0] * 5
    np.testing.assert_array_equal(np.diff(want["host_offsets"]), [worker.NUS[q] for q in worker.HOST_SELECTION])


@pytest.mark.parametrize("k, which", [(20, "one_left_out"), (20, "all_five"), (40, "all_five")])
def test_module_level_results_do_not_depend_on_the_batching(k, which):
    """gp.predictive_flux over five quasars of unequal length in blocks of two (one upload, then reloads; the selection of all
    five ends on a short block) against the same call with all of them in one batch: every returned array, bit for bit.
    k = 40 once: another instantiation of k_mc_contract."""
    model, samples, spectra, p, log_priors = MC.batching_case(k)
    results = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, log_priors, params=p)
    kw = dict(params=p, selection=MC.BATCHING_SELECTIONS[which], components=("null", "sub_dla", "dla"), model_weights="posteriors",
              residuals=True)
    blocks = gp.predictive_flux(model, samples, spectra, results, max_quasars_per_batch=2, **kw)
    whole = gp.predictive_flux(model, samples, spectra, results, max_quasars_per_batch=5, **kw)
    assert set(ALL) <= set(whole) and whole["status"].tolist() == [0] * len(kw["selection"]) and np.isfinite(whole["flux_var"]).all()
    np.testing.assert_array_equal(np.diff(whole["offsets"]), [MC.BATCHING_NUS[q] for q in kw["selection"]])
    MC.assert_same_results(blocks, whole)


# ------------------------------------------------------------------------------------------------
# file to file
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("multi", [False, True])
def test_command_line_run_equals_the_in_memory_call(tmp_path, multi):
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
        components = ("null", "sub_dla", "dla")
    else:
        p = Parameters()
        results = gp.process_qsos(fs["model"], fs["samples"], spectra, prior_catalog=fs["prior"])
        io.save_processed_qsos(processed, results, test_ind=fs["test_ind"])
        components = ("null", "dla")
    idx = [int(run_pos.size - 1), 0, 3, 5]
    out = str(tmp_path / "predictive_flux.mat")
    rc = cli.main(["--preloaded", fs["paths"]["preloaded"], "--catalog", fs["paths"]["catalog"], "--model", fs["paths"]["learned"],
                   "--samples", fs["paths"]["samples"], "--processed", processed, "--out", out, "--indices", ",".join(map(str, idx)),
                   "--predictive-flux", "--residuals", "--components", ",".join(components), "--max-quasars-per-batch", "3"])
    assert rc == 0
    sel = np.array(sorted(idx))
    want = gp.predictive_flux(fs["model"], fs["samples"], spectra, results, params=p, selection=sel, components=components,
                              model_weights="posteriors", residuals=True)
    back = io.load_predictive_flux(out)
    np.testing.assert_array_equal(back["selection"], sel)
    np.testing.assert_array_equal(back["offsets"], want["offsets"])
    np.testing.assert_array_equal(back["status"], want["status"])
    for name in io.PREDICTIVE_FLUX_CELLS:
        for got, ref in zip(back[name], gp.split_cells(want[name], want["offsets"])):
            np.testing.assert_array_equal(got, ref, err_msg=name)
    np.testing.assert_array_equal(back["chi2"], want["chi2"])
    np.testing.assert_array_equal(back["num_kept"], want["num_kept"])
    usable = want["status"] == 0
    assert usable.any() and np.isfinite(want["flux_var"][:want["offsets"][np.flatnonzero(usable)[0] + 1]]).all()
