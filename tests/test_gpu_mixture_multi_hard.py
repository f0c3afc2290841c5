"""The marginal continuum, the predictive flux and the absorption moments over ALL models of a multi-DLA run against 50-digit
arithmetic where the arithmetic is hard (tests/mixture_multi_hard_cases.py; tests/golden/exact_mixture_multi_hard.npz): four
classes of hard_conditioning_cases.py (cond(B) of the null model 3e6 .. 6e6, saturated troughs) in a context of max_dlas = 4,
with base indices and weight rows placed by hand so that every model's product profiles carry weight.  Per (class, row,
mixture) and product, the rule of tests/test_gpu_continuum_hard.py:

    e_gpu = max |GPU - exact| / max(1, max |exact|)          (and per pixel, relatively, for continuum_var, flux_var
                                                               and flux_var_within)
    e_gpu <= max(10 x e_restatement, 1e-12),  e_restatement = the Woodbury-form restatement's error over the product's
                                                               family on the SAME inputs, from the fixture alone

on the rows ``top8_flat``, ``adjacent_pair`` and ``flat`` under every mixture, and for the absorption moments of
Batch.model_spectra_multi the same with the floor TOL_MOMENTS.  Every figure is printed before it is asserted.

The ``near_one_hot`` row (weights 1 and 1e-6, on the mixture of four-fold products alone) is printed, not asserted; the exact
statements hold on it too.  Its one-pass between-variances (9e-7 .. 4e-3 in size) are off by 1e-5 .. 2e-2 relatively, on the GPU as in both restatements.
And with one live sample e_restatement is one draw of one inversion, not the largest of many: on ``correlated``, 31 lines,
``coef_cov_within`` measured 1.32e-10 on the MI355X against a restatement at 1.04e-11, a ratio of 12.6.  The cause is the
inputs, not the arithmetic: the device forms its own Voigt profiles, held to 2e-13 of the oracle's each, and four stored
profiles moved by that much move this sample's Sigma by 1.2e-10 (median of 200 draws; largest 4.7e-10) on the CPU, while a
Cholesky inverse of the restatement's own B is 1.2e-11 from exact (test_mixture_multi_hard.py,
``test_profile_parity_outweighs_the_restatement_on_one_sample``).  One context and one upload per class and no sweep: every table is a host table.  Kernels:
k_mc_contract_multi<4,4,32> (k = 20), k_mc_contract_multi<1,14,64> (k = 40), k_pf_pixels_multi, k_spectra_weights_multi,
k_spectra_moments_multi, and the solve and finish kernels they share with the three-component entries."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd.parameters import MultiParameters

import continuum_hard_cases as CH
import hard_conditioning_cases as H
import mixture_multi_cases as XC
import mixture_multi_hard_cases as XH
from test_gpu_model_spectra import TOL_MOMENTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden):
    return XH.load_fixture(golden)


def run_gpu(case, e):
    """([(marginal continuum dict, predictive flux dict)] per (row, mixture number) of XH.COMBOS, {row: model_spectra_multi
    result}) from one batch of a max_dlas = 4 context"""
    cls, sp = case["cls"], case["spectrum"]
    meanflux = XH.meanflux_of(cls)
    ctx = gp.Context(0, MultiParameters(max_dlas=XH.MD, num_lines=cls[3]))
    try:
        ctx.set_model(case["model"])
        ctx.set_samples(case["samples"])
        lp_dla = np.log(np.full((1, XH.MD), 0.1 / XH.MD))
        batch = ctx.upload([sp], np.array([np.log(0.85)]), lp_dla, np.array([np.log(0.05)]))
        try:
            out, spectra = [], {}
            for row, m in XH.COMBOS:
                kw = dict(tables=XH.host_tables(XH.stored_rows(e, row), e["base_sample_inds"]), model_weights=np.array([XH.MIXTURES[m]]),
                          meanflux=meanflux)
                out.append((XC.split_mc(batch.marginal_continuum_multi(**kw))[0], XC.split_pf(batch.predictive_flux_multi(**kw))[0]))
            for row in XH.MOMENT_ROWS if cls in XH.MOMENT_CLASSES else ():
                spectra[row] = batch.model_spectra_multi(tables=XH.host_tables(XH.stored_rows(e, row), e["base_sample_inds"]),
                                                         model_weights=np.array([XH.MIXTURES[0]]), meanflux=meanflux)
        finally:
            batch.close()
    finally:
        ctx.close()
    return out, spectra


@pytest.mark.parametrize("cls", XH.CLASSES, ids=H.class_name)
def test_class_against_exact_arithmetic(cls, fixture):
    assert TOL_MOMENTS == XH.TOL_MOMENTS
    name = H.class_name(cls)
    e = fixture[name]
    case = H.build_case(cls)
    bsi = e["base_sample_inds"]
    full = XH.with_products(XH.stored_inputs(e), bsi)
    results, spectra = run_gpu(case, e)
    forms = {form: XH.restatement_samples(full, form) for form in ("woodbury", "dense")}
    bad = []
    for (row, m), (mc, pf) in zip(XH.COMBOS, results):
        pw = XH.MIXTURES[m]
        exact = XH.stored_exact(e, row, m)
        eff = XH.effective_rows(XH.stored_rows(e, row), bsi)
        rest = XH.restatement_products(full, forms["woodbury"], eff, pw)
        got = {**mc, **pf}
        label = f"{name} {row} {pw}"
        figs = CH.figures(got, exact, rest)
        for n, e_rest, e_gpu, tol in figs:
            print(f"{label} {n}: e_restatement {e_rest:.3e}, e_gpu {e_gpu:.3e}, ratio {CH.ratio(e_gpu, e_rest):.2f}, tolerance {tol:.3e}")
        if row == "near_one_hot":      # reported, not asserted (the module docstring says why); the exact statements below hold
            dense = XH.restatement_products(full, forms["dense"], eff, pw)
            for n in ("continuum_var_between", "flux_var_between"):
                ok = exact[n] > 0
                rel = [float((np.abs(v[n][ok] - exact[n][ok]) / exact[n][ok]).max()) for v in (got, rest, dense)]
                print(f"{label} {n}: worst relative error GPU {rel[0]:.2e}, Woodbury form {rel[1]:.2e}, dense form {rel[2]:.2e} "
                      f"(largest exact value {exact[n].max():.2e})")
        # exact statements
        assert mc["status"] == 0 and pf["status"] == 0 and mc["model_flags"] == 0 and pf["model_flags"] == 0, label
        assert np.array_equal(np.isnan(pf["noise_var"]), ~e["kept"]), label
        assert (mc["continuum_var"] >= mc["continuum_var_between"]).all() and (mc["continuum_var_between"] >= 0).all(), label
        assert (pf["flux_var"] == pf["flux_var_within"] + pf["flux_var_between"]).all() and (pf["flux_var_between"] >= 0).all(), label
        assert all(np.isfinite(got[n]).all() for n in exact if n != "noise_var") and np.isfinite(pf["noise_var"][e["kept"]]).all(), label
        if row != "near_one_hot":
            bad += CH.failures(label, figs)
    # k_spectra_weights_multi and k_spectra_moments_multi: the same gather, a weighted sum per pixel and no matrix
    for row, res in spectra.items():
        label = f"{name} {row} {XH.MIXTURES[0]}"
        assert res["status"].tolist() == [0] and res["model_flags"].tolist() == [0] and np.diff(res["offsets"]).tolist() == [H.N_PIX], label
        eff = XH.effective_rows(XH.stored_rows(e, row), bsi)
        figs = XH.moment_figures(res, XH.stored_moments(e, row), XH.restatement_moments(full, eff, XH.MIXTURES[0]))
        for n, e_rest, e_gpu, tol in figs:
            print(f"{label} {n}: e_restatement {e_rest:.3e}, e_gpu {e_gpu:.3e}, ratio {CH.ratio(e_gpu, e_rest):.2f}, tolerance {tol:.3e}")
        assert all(np.isfinite(res[n]).all() and (res[n] >= 0).all() for n in XH.MOMENTS), label
        bad += XH.moment_failures(label, figs)
    assert not bad, bad
