"""The marginal continuum, the posterior predictive flux and the per-absorber continuum of model spectra against 50-digit
arithmetic where the arithmetic is hard (tests/continuum_hard_cases.py; tests/golden/exact_continuum_hard.npz and
exact_continuum_hard_k33_k40.npz): the classes of hard_conditioning_cases.py (cond(B) up to 1e7, saturated absorbers,
fewer kept pixels than the rank), with weight rows placed by hand so that the between-sample sums carry weight.  There
the two fp64 restatements disagree by more than ``R.continuum_tolerance`` allows, so the rule is, per (class, row,
mixture) and product:

    e_gpu = max |GPU - exact| / max(1, max |exact|)          (and per pixel, relatively, for continuum_var, flux_var
                                                               and flux_var_within)
    e_gpu <= max(10 x e_restatement, 1e-12),  e_restatement = the Woodbury-form restatement's error over the product's
                                                               family on the SAME inputs, from the fixture alone

Every figure is printed before it is asserted.  One context and one upload per class and no sweep: the weights are host
tables.  Kernels: k_mc_contract<4,4,32> (k = 20), k_mc_contract<1,14,64> (k = 33, 40), k_mc_solve, k_mc_finish,
k_pf_solve, k_pf_live, k_pf_pixels, k_pf_finish, k_spectra_continuum."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp

import continuum_hard_cases as CH
import hard_conditioning_cases as H
import marginal_continuum_cases as MC
import predictive_flux_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden):
    return CH.load_fixture(golden)


def run_gpu(case, e, combos):
    """[(marginal continuum dict, predictive flux dict)] per (row, mixture number) of ``combos`` and the three
    per-absorber continua [3, n_u], from one batch"""
    cls, sp, p = case["cls"], case["spectrum"], case["params"]
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(case["model"])
        ctx.set_samples(case["samples"])
        if case["bsi"] is None:
            batch = ctx.upload([sp], np.array([np.log(0.9)]), np.array([np.log(0.1)]))
        else:
            lp_dla = np.log(np.full((1, H.MAX_DLAS), 0.1 / H.MAX_DLAS))
            batch = ctx.upload([sp], np.array([np.log(0.85)]), lp_dla, np.array([np.log(0.05)]))
        try:
            out = []
            for row, m in combos:
                pw, sc = CH.mixtures_of(cls)[m]
                kw = dict(weights={t: v[None] for t, v in CH.stored_rows(e, cls, row).items()}, components=CH.components_of(pw),
                          model_weights=np.array([pw]))
                mc = batch.marginal_continuum(sample_coefficients=sc, **kw)
                pf = batch.predictive_flux(**kw)
                out.append((MC.split(mc, cls[2])[0], PC.split(pf)[0]))
            three = e["spectra_samples"]
            spectra = batch.model_spectra(selection=[0, 0, 0], products=("continuum",),
                                          absorbers=(np.arange(4), e["z_dlas"][three], case["samples"]["log_nhi_samples"][three]))
        finally:
            batch.close()
    finally:
        ctx.close()
    assert spectra["status"].tolist() == [0, 0, 0]
    return out, np.stack(gp.split_cells(spectra["continuum"], spectra["offsets"]))


@pytest.mark.parametrize("cls", H.CLASSES, ids=H.class_name)
def test_class_against_exact_arithmetic(cls, fixture):
    name = H.class_name(cls)
    e = fixture[name]
    case = H.build_case(cls)
    inp = CH.stored_inputs(e, cls)
    combos = [(row, m) for row in CH.ROWS for m in range(len(CH.mixtures_of(cls)))]
    results, continua = run_gpu(case, e, combos)
    forms = {form: CH.restatement_samples(inp, CH.tables_of(cls), form) for form in ("woodbury", "dense")}
    bad = []
    for (row, m), (mc, pf) in zip(combos, results):
        pw, sc = CH.mixtures_of(cls)[m]
        exact = CH.stored_exact(e, cls, row, m)
        rest = CH.restatement_products(inp, forms["woodbury"], CH.stored_rows(e, cls, row), pw, sc)
        got = {**mc, **pf}
        label = f"{name} {row} {pw}"
        figs = CH.figures(got, exact, rest)
        for n, e_rest, e_gpu, tol in figs:
            print(f"{label} {n}: e_restatement {e_rest:.3e}, e_gpu {e_gpu:.3e}, ratio {CH.ratio(e_gpu, e_rest):.2f}, tolerance {tol:.3e}")
        if row == "near_one_hot":      # reported, not asserted: the one-pass form loses it, and so do the restatements
            dense = CH.restatement_products(inp, forms["dense"], CH.stored_rows(e, cls, row), pw, sc)
            for n in ("continuum_var_between", "flux_var_between"):
                ok = exact[n] > 0
                rel = [float((np.abs(v[n][ok] - exact[n][ok]) / exact[n][ok]).max()) for v in (got, rest, dense)]
                print(f"{label} {n}: worst relative error GPU {rel[0]:.2e}, Woodbury form {rel[1]:.2e}, dense form {rel[2]:.2e} "
                      f"(largest exact value {exact[n].max():.2e})")
        # exact statements
        assert mc["status"] == 0 and pf["status"] == 0, label
        assert np.array_equal(np.isnan(pf["noise_var"]), ~e["kept"]), label
        assert (mc["continuum_var"] >= mc["continuum_var_between"]).all() and (mc["continuum_var_between"] >= 0).all(), label
        assert (pf["flux_var"] == pf["flux_var_within"] + pf["flux_var_between"]).all() and (pf["flux_var_between"] >= 0).all(), label
        bad += CH.failures(label, figs)
    # k_spectra_continuum: mu + M c_i of three samples of top8_flat, one absorber each
    exact = e["exact_spectra_continuum"]
    three = e["spectra_samples"]
    rest = np.stack([forms["woodbury"]["dla"][int(i)][2] for i in three])
    e_rest, e_gpu = CH.error(rest, exact), CH.error(continua, exact)
    tol = CH.tolerance(e_rest)
    print(f"{name} samples {three.tolist()} model_spectra continuum: e_restatement {e_rest:.3e}, e_gpu {e_gpu:.3e}, "
          f"ratio {CH.ratio(e_gpu, e_rest):.2f}, tolerance {tol:.3e}")
    if not e_gpu <= tol:
        bad.append(f"{name} model_spectra continuum: error {e_gpu:.3e} > {tol:.3e}")
    assert not bad, bad
