"""GPU checks of the marginal continuum and the predictive flux over all models of a multi-DLA run (DESIGN.md 4.25;
csrc/marginal_continuum_kernels.hpp, csrc/predictive_flux_kernels.hpp, csrc/host_mixture_multi.hpp) against the NumPy-and-oracle restatements
tests/marginal_continuum_multi_restatement.py and tests/predictive_flux_multi_restatement.py in their DENSE form, at the
shapes of tests/mixture_multi_cases.py.  Tolerances against the restatement are not fixed in advance: per product family
``R.continuum_tolerance`` of the restatement's own dense-vs-Woodbury disagreement on the same case (10 x, floored at 1e-12,
capped at 1e-8; tests/test_mixture_multi.py holds every setup below 1e-9).  Every figure is printed before it is asserted;
NaN, status and flag patterns must match exactly."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, synthetic
from gp_dla_detection_amd.parameters import MultiParameters

import marginal_continuum_multi_restatement as MMR
import marginal_continuum_restatement as MR
import mixture_multi_cases as XC
import mixture_multi_groups_worker as worker
import model_spectra_edge_cases as E
import model_spectra_multi_cases as MSC
import model_spectra_multi_restatement as RM
import model_spectra_restatement as R
import predictive_flux_multi_restatement as PMR
from test_gpu_model_spectra import _multi, _single

pytestmark = pytest.mark.gpu

MC_ALL = MMR.ARRAYS + MMR.ROWS
PF_ALL = PMR.PRODUCTS
UNDEFINED = _lib.SPECTRA_AVERAGE_UNDEFINED
TOL_ONE_HOT_CONTINUUM, TOL_ONE_HOT_FLUX = 1e-12, 1e-11


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a: dict, b: dict, names, label=""):
    for name in names:
        assert np.array_equal(_bits(a[name]), _bits(b[name])), (label, name)
    for name in ("offsets", "status", "model_flags"):
        if name in a and name in b:
            np.testing.assert_array_equal(a[name], b[name], err_msg=f"{label} {name}")


def _compare(label, mc, pf, want):
    """Worst deviation per product of the GPU's per-quasar dicts from the dense restatement against the tolerance of the
    restatement's own disagreement; statuses and flags exact.  Returns the figures."""
    dis = {**MMR.disagreement(want["mc"]["dense"], want["mc"]["woodbury"]), **PMR.disagreement(want["pf"]["dense"], want["pf"]["woodbury"])}
    tol = {**MMR.tolerances(dis), **PMR.tolerances(dis)}
    worst = {n: max(MR.deviation(g[n], w[n]) for g, w in zip(mc, want["mc"]["dense"])) for n in MMR.PRODUCTS_COEF + MMR.PRODUCTS_COV}
    worst.update({n: max(MR.deviation(g[n], w[n]) for g, w in zip(pf, want["pf"]["dense"])) for n in PMR.PRODUCTS})
    for n in worst:
        print(f"{label} {n}: dense-vs-Woodbury {dis[n]:.2e} -> tolerance {tol[n]:.2e}; GPU worst |delta| {worst[n]:.3e}")
    for got, kind in ((mc, "mc"), (pf, "pf")):
        assert [g["status"] for g in got] == [w["status"] for w in want[kind]["dense"]], (label, kind)
        assert [g["model_flags"] for g in got] == [w["model_flags"] for w in want[kind]["dense"]], (label, kind)
    for n in worst:
        assert worst[n] < tol[n], (label, n, worst[n], tol[n])
    return dis, worst


# ------------------------------------------------------------------------------------------------
# 1. every product of both entries against the dense restatement
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s["name"] for s in XC.SETUPS])
def test_all_products_against_the_dense_restatement(oracle, name):
    """A multi-DLA batch swept by process_multi with the setup's base indices where a quasar keeps the sweep's rows; the call
    takes the downloaded tables with each quasar's row kind as host tables, weight on every component."""
    st = XC.setup(name)
    model, samples, spectra = XC.build(st)
    p = XC.params(st)
    P = XC.model_weights(st)
    ctx, batch = _multi(model, samples, spectra, p)
    try:
        if "sweep" in st["kinds"]:
            batch.process_multi(XC.base_in(st, samples))
            down = batch.download_multi()
            np.testing.assert_array_equal(down["base_sample_inds"], XC.base_in(st, samples))
            sweep = (np.array(down["sample_log_likelihoods_dla"]), np.array(down["sample_log_likelihoods_lls"]))
        else:
            sweep = XC.synthetic_sweep(st)
        tables = XC.host_tables(st, samples, *sweep)
        mc = batch.marginal_continuum_multi(tables=tables, model_weights=P, meanflux=st["meanflux"])
        pf = batch.predictive_flux_multi(tables=tables, model_weights=P, meanflux=st["meanflux"])
    finally:
        batch.close()
        ctx.close()
    want = XC.wanted(oracle, ("gpu", name), model, samples, spectra, tables, P, st["meanflux"], st["lines"], p=p)
    np.testing.assert_array_equal(np.diff(mc["offsets"]), [w["continuum_mean"].size for w in want["mc"]["dense"]])
    np.testing.assert_array_equal(mc["offsets"], pf["offsets"])
    got_mc, got_pf = XC.split_mc(mc), XC.split_pf(pf)
    _compare(name, got_mc, got_pf, want)
    for q, kind in enumerate(st["kinds"]):
        finite = all(np.isfinite(got_mc[q][n]).all() for n in MC_ALL) and all(np.isfinite(got_pf[q][n]).all() for n in PF_ALL[:4])
        print(f"{name} quasar {q} ({kind}): {'finite' if finite else 'NaN rows'}, flags {got_mc[q]['model_flags']:#x}")
        if kind == "none":
            assert got_mc[q]["model_flags"] == got_pf[q]["model_flags"] == XC.all_flags(st["md"])
            assert all(np.isnan(got_mc[q][n]).all() for n in MC_ALL) and all(np.isnan(got_pf[q][n]).all() for n in PF_ALL)
        elif kind != "sweep":       # (a sweep may leave a model of a short spectrum without a usable sample: flagged on both sides)
            assert finite and got_mc[q]["model_flags"] == 0
    ok = mc["status"] == 0
    assert (mc["continuum_var"][np.isfinite(mc["continuum_var"])] >= 0).all() and ok.all()
    assert (pf["flux_var_between"][np.isfinite(pf["flux_var_between"])] >= 0).all()


# ------------------------------------------------------------------------------------------------
# 2. the gather and the slot order: a one-hot row on model n at sample i is the library's own conditional continuum
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [20, 40])
def test_one_hot_row_is_model_spectra_of_the_slot_absorbers(oracle, k):
    """One entry per model n = 1 .. 4 and z-order position 15 / 16 / 63 / 64 of the own sample: the whole model weight on
    DLA(n), the whole sample weight on sample i.  ``continuum`` and ``model_flux`` of Batch.model_spectra with the n slot
    absorbers of sample i as its absorber list; no between-variance at all."""
    S, md, nus = 65, 4, (33, 65)
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(7000 + 2 * i, n, model, mask_fraction=0.05 * i) for i, n in enumerate(nus)]
    grids = [R.grid(oracle, model, sp) for sp in spectra]
    order = E.z_order(samples)
    entries = [(n, pos) for n in range(1, md + 1) for pos in (15, 16, 63, 64)]
    sel = np.array([e % 2 for e in range(len(entries))], dtype=np.int64)
    dla, lls = np.empty((len(entries), md, S)), np.zeros((len(entries), S))
    base = np.stack([MSC.base_rows("random", S, md, samples, seed=30 + e) for e in range(len(entries))])
    P = np.zeros((len(entries), 2 + md))
    off, zs, lns = [0], [], []
    for e, (n, pos) in enumerate(entries):
        i = int(order[pos])
        dla[e] = E.moment_row(("hot", pos), S, samples, None)
        P[e, 1 + n] = 1.0
        g = grids[sel[e]]
        s = RM.slots(base[e], n, i)
        assert len(s) == n
        zs += list(g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"][s])
        lns += list(samples["log_nhi_samples"][s])
        off.append(len(zs))
    tables = dict(sample_log_likelihoods_dla=dla, base_sample_inds=base, sample_log_likelihoods_lls=lls)
    ctx, batch = _single(model, samples, spectra)
    try:
        mc = batch.marginal_continuum_multi(selection=sel, tables=tables, model_weights=P, meanflux=False)
        pf = batch.predictive_flux_multi(selection=sel, tables=tables, model_weights=P, meanflux=False)
        own = batch.model_spectra(selection=sel, absorbers=(np.array(off), np.array(zs), np.array(lns)), products=("continuum",),
                                  meanflux=False)
    finally:
        batch.close()
        ctx.close()
    np.testing.assert_array_equal(mc["offsets"], own["offsets"])
    assert (mc["status"] == 0).all() and (pf["status"] == 0).all() and (mc["model_flags"] == 0).all()
    o = mc["offsets"]
    worst_c = worst_f = 0.0
    for e, (n, pos) in enumerate(entries):
        sl = slice(o[e], o[e + 1])
        assert np.isfinite(own["continuum"][sl]).all() and np.isfinite(own["model_flux"][sl]).all()
        d_c, d_f = MR.deviation(mc["continuum_mean"][sl], own["continuum"][sl]), MR.deviation(pf["flux_mean"][sl], own["model_flux"][sl])
        deepest = float((own["model_flux"][sl] / own["continuum"][sl]).min())
        print(f"k {k} model {n} z position {pos}: |continuum_mean - continuum| {d_c:.2e}, |flux_mean - model_flux| {d_f:.2e}, "
              f"deepest absorption {deepest:.3f}")
        worst_c, worst_f = max(worst_c, d_c), max(worst_f, d_f)
        assert (mc["coef_cov_between"][e] == 0).all() and (mc["continuum_var_between"][sl] == 0).all()
        assert (pf["flux_var_between"][sl] == 0).all()
    print(f"k {k}: worst |delta| {worst_c:.3e} (continuum, bound {TOL_ONE_HOT_CONTINUUM:.0e}), {worst_f:.3e} (flux, bound {TOL_ONE_HOT_FLUX:.0e})")
    assert worst_c < TOL_ONE_HOT_CONTINUUM and worst_f < TOL_ONE_HOT_FLUX


# ------------------------------------------------------------------------------------------------
# 3., 6., 8. a swept batch: the seam with the existing entries, resident = host, the mixtures, the residuals
# ------------------------------------------------------------------------------------------------

def test_resident_tables_the_seam_with_the_three_component_entries_and_the_mixtures(oracle):
    """A multi-DLA batch of 3 quasars (60 and 257 pixels and a fully masked one), S = 65, max_dlas = 3, swept with supplied
    base_sample_inds.  Resident = host on the downloaded tables, default weights = the explicit model_posteriors; weights that
    reach only (null, sub-DLA, DLA(1)) give the arrays of Batch.marginal_continuum / Batch.predictive_flux bit for bit; a
    three-way and a five-way mixture against the restatement; residuals=True against NumPy on the returned arrays."""
    S, md = 65, 3
    model = synthetic.make_model(20)
    spectra = [synthetic.make_spectrum(6400, 60, model), synthetic.make_spectrum(6402, 257, model, mask_fraction=0.05),
               E.masked_out(synthetic.make_spectrum(6404, 100, model))]
    samples = synthetic.make_samples(S)
    p = MultiParameters(max_dlas=md)
    base_in = np.stack([MSC.base_rows(("random", "cyclic", "one")[q], S, md, samples, seed=q) for q in range(3)])
    seam = np.array([[0.2, 0.3, 0.5, 0, 0], [0.0, 1.5, 0.5, 0, 0], [0.3, 0.3, 0.4, 0, 0]])
    mix = np.array([[0.3, 0.2, 0.0, 0.5, 0.0], [0.1, 0.2, 0.3, 0.25, 0.15], [0.2, 0.2, 0.2, 0.2, 0.2]])
    ctx, batch = _multi(model, samples, spectra, p)
    try:
        batch.process_multi(base_in)
        down = batch.download_multi()
        tables = dict(sample_log_likelihoods_dla=np.array(down["sample_log_likelihoods_dla"]), base_sample_inds=np.array(down["base_sample_inds"]),
                      sample_log_likelihoods_lls=np.array(down["sample_log_likelihoods_lls"]))
        post = np.array(down["model_posteriors"])
        res = {"mc": batch.marginal_continuum_multi(), "pf": batch.predictive_flux_multi(residuals=True)}
        explicit = {"mc": batch.marginal_continuum_multi(model_weights=post), "pf": batch.predictive_flux_multi(model_weights=post)}
        host = {"mc": batch.marginal_continuum_multi(tables=tables, model_weights=post), "pf": batch.predictive_flux_multi(tables=tables, model_weights=post)}
        new3 = {"mc": batch.marginal_continuum_multi(model_weights=seam), "pf": batch.predictive_flux_multi(model_weights=seam)}
        old3 = {"mc": batch.marginal_continuum(components=("null", "sub_dla", "dla"), model_weights=seam[:, :3]),
                "pf": batch.predictive_flux(components=("null", "sub_dla", "dla"), model_weights=seam[:, :3])}
        mixed = {"mc": batch.marginal_continuum_multi(model_weights=mix), "pf": batch.predictive_flux_multi(model_weights=mix)}
        y, kept = batch.grid_flux()
    finally:
        batch.close()
        ctx.close()
    np.testing.assert_array_equal(tables["base_sample_inds"], base_in)
    print(f"model_posteriors {post.tolist()}; status {res['mc']['status'].tolist()}, flags {res['mc']['model_flags'].tolist()}")
    for kind, names in (("mc", MC_ALL), ("pf", PF_ALL)):
        _same(res[kind], explicit[kind], names, f"default weights {kind}")
        _same(res[kind], host[kind], names, f"resident = host {kind}")
        _same(new3[kind], old3[kind], names, f"seam {kind}")
        assert res[kind]["status"][2] == 1 and np.diff(res[kind]["offsets"]).tolist() == [60, 257, 100]
        assert all(np.isnan(res[kind][n][res[kind]["offsets"][2]:]).all() for n in names if res[kind][n].ndim == 1 and n not in MMR.ROWS)
        assert new3[kind]["status"].tolist() == [0, 0, 1] and all(np.isfinite(new3[kind][n][:317]).all() for n in names if n not in MMR.ROWS + ("noise_var",))
    assert np.isnan(res["mc"]["coef_mean"][2]).all() and np.isfinite(new3["mc"]["coef_mean"][:2]).all()
    # the mixtures (row 0: null, sub-DLA and DLA(2); row 1: all five) against the restatement
    want = XC.wanted(oracle, "resident mixtures", model, samples, spectra, tables, mix, True, 3, p=p)
    _compare("three- and five-way mixtures", XC.split_mc(mixed["mc"]), XC.split_pf(mixed["pf"]), want)
    assert mixed["mc"]["status"].tolist() == [0, 0, 1]
    assert np.isfinite(mixed["mc"]["continuum_mean"][:317]).all() or mixed["mc"]["model_flags"][:2].any()
    # the residuals, from the returned arrays
    pf = res["pf"]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(kept, (y - pf["flux_mean"]) / np.sqrt(pf["flux_var"] + pf["noise_var"]), np.nan)
    assert np.array_equal(_bits(pf["residual"]), _bits(r)) and pf["num_kept"].tolist() == [int(kept[:60].sum()), int(kept[60:317].sum()), 0]
    for q in range(2):
        sl = slice(pf["offsets"][q], pf["offsets"][q + 1])
        if pf["status"][q] == 0 and not pf["model_flags"][q]:
            assert pf["chi2"][q] == float(np.sum(r[sl][kept[sl]] ** 2)) and np.isfinite(pf["chi2"][q])
            print(f"quasar {q}: chi2 {pf['chi2'][q]:.1f} over {pf['num_kept'][q]} kept pixels")


# ------------------------------------------------------------------------------------------------
# 4. base index 0
# ------------------------------------------------------------------------------------------------

def test_base_index_zero(oracle):
    """A finite log-likelihood on a sample whose slot index is 0 gives the bits of the same call with that entry NaN.  A model
    whose every live sample consumes a 0 is flagged: with P_n > 0 NaN rows and status 0, with P_n = 0 it is skipped.  A NaN
    column density on a sample of weight 0 that no live sample gathers changes nothing."""
    S, md, nus = 65, 4, (17, 33)
    model, spectra = MSC.batch(nus)
    samples = dict(synthetic.make_samples(S))
    rng = np.random.default_rng(11)
    dla = -1000.0 + 6.0 * rng.standard_normal((2, md, S))
    lls = -1000.0 + 6.0 * rng.standard_normal((2, S))
    base = np.stack([MSC.base_rows("random", S, md, samples, seed=s) for s in range(2)])
    zeros = [3, 20, 64]
    base[0, 1, zeros] = 0                      # entry 0: slot 3 of three samples was never drawn (models 3 and 4)
    dla[0, 2:, zeros] = -985.0                 # ... and their log-likelihoods would carry much of the weight
    live = np.arange(S) % 3 == 0
    dla[1, 2, ~live] = np.nan
    base[1, 1, live] = 0                       # entry 1: every live sample of model 3 consumes a 0
    masked = dla.copy()
    masked[0, 2:, zeros] = np.nan
    # the poisoned sample: weight 0 everywhere, gathered by no sample
    poison = 40
    dla[:, :, poison] = masked[:, :, poison] = lls[:, poison] = np.nan
    base[base == poison + 1] = poison + 2
    P = np.tile([0.1, 0.1, 0.2, 0.2, 0.2, 0.2], (2, 1))
    P0 = P.copy()
    P0[1, 4] = 0.0
    t = lambda d: dict(sample_log_likelihoods_dla=d, base_sample_inds=base, sample_log_likelihoods_lls=lls)   # noqa: E731
    out = {}
    for label in ("clean", "poisoned"):
        smp = dict(samples)
        if label == "poisoned":
            for key in ("nhi_samples", "lls_nhi_samples"):
                smp[key] = np.array(samples[key])
                smp[key][poison] = np.nan
        ctx, batch = _single(model, smp, spectra)
        try:
            out[label] = {(kind, which): getattr(batch, f"{kind}_multi")(tables=t(d), model_weights=w, meanflux=False)
                          for kind in ("marginal_continuum", "predictive_flux")
                          for which, d, w in (("finite", dla, P), ("nan", masked, P), ("skipped", dla, P0))}
        finally:
            batch.close()
            ctx.close()
    n0 = 17
    for kind, names in (("marginal_continuum", MC_ALL), ("predictive_flux", PF_ALL)):
        a, b, c = (out["clean"][(kind, which)] for which in ("finite", "nan", "skipped"))
        _same(a, b, names, f"{kind}: finite entry on a zero slot")
        assert a["model_flags"].tolist() == [0, 1 << 2] and a["status"].tolist() == [0, 0]
        per_pixel = [n for n in names if n not in MMR.ROWS]
        assert all(np.isfinite(a[n][:n0]).all() and np.isnan(a[n][n0:]).all() for n in per_pixel), kind
        assert c["model_flags"].tolist() == [0, 0] and c["status"].tolist() == [0, 0]
        assert all(np.isfinite(c[n]).all() for n in per_pixel), kind
        for which in ("finite", "nan", "skipped"):
            _same(out["clean"][(kind, which)], out["poisoned"][(kind, which)], names, f"{kind}: NaN column density at weight 0 ({which})")
    # the zeros matter: the restatement with the zeros drawn differs, and the GPU follows the one with them
    g = R.grid(oracle, model, spectra[0])
    tab = XC.quasar_tables(t(dla), 0)
    full = dict(tab, base_sample_inds=np.where(tab["base_sample_inds"] == 0, 1, tab["base_sample_inds"]))
    want = MMR.marginal_continuum_multi(oracle, model, g, samples, tab, P[0], False, 3)
    wood = MMR.marginal_continuum_multi(oracle, model, g, samples, tab, P[0], False, 3, "woodbury")
    other = MMR.marginal_continuum_multi(oracle, model, g, samples, full, P[0], False, 3)
    tol = R.continuum_tolerance(MR.deviation(want["continuum_mean"], wood["continuum_mean"]))
    got = out["clean"][("marginal_continuum", "finite")]["continuum_mean"][:n0]
    d, apart = MR.deviation(got, want["continuum_mean"]), MR.deviation(want["continuum_mean"], other["continuum_mean"])
    print(f"index 0: |delta| {d:.2e} (tolerance {tol:.1e}); the restatement moves by {apart:.2e} when the zeros are drawn")
    assert d < tol and apart > 1e3 * tol


# ------------------------------------------------------------------------------------------------
# 5. NaN weight rows, unusable quasars, refusals
# ------------------------------------------------------------------------------------------------

def test_nan_weight_row_unusable_quasar_and_refusals():
    S, md = 17, 2
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(S)
    good = synthetic.make_spectrum(6400, 40, model)
    spectra = [good, E.masked_out(good), synthetic.make_spectrum(6402, 33, model)]
    rng = np.random.default_rng(3)
    tables = dict(sample_log_likelihoods_dla=-50.0 + 3.0 * rng.standard_normal((3, md, S)),
                  base_sample_inds=np.stack([MSC.base_rows("random", S, md, samples, seed=q) for q in range(3)]),
                  sample_log_likelihoods_lls=-50.0 + 3.0 * rng.standard_normal((3, S)))
    P = np.array([[0.2, np.nan, 0.3, 0.5], [0.25, 0.25, 0.25, 0.25], [0.25, 0.25, 0.25, 0.25]])
    ctx, batch = _single(model, samples, spectra)
    try:
        mc = batch.marginal_continuum_multi(tables=tables, model_weights=P, meanflux=False)
        pf = batch.predictive_flux_multi(tables=tables, model_weights=P, meanflux=False)
        with pytest.raises(_lib.GpdlaError):        # a single-DLA batch has no resident multi-DLA tables
            batch.marginal_continuum_multi()
        with pytest.raises(_lib.GpdlaError):
            batch.predictive_flux_multi(model_weights=P)
        bad = P.copy()
        bad[2, 1] = -0.5
        with pytest.raises(_lib.GpdlaError):
            batch.predictive_flux_multi(tables=tables, model_weights=bad, meanflux=False)
        batch.set_fixed_absorbers((np.array([0, 1, 1, 1]), np.array([2.4]), np.array([20.5])))
        for call in (batch.marginal_continuum_multi, batch.predictive_flux_multi):
            with pytest.raises(_lib.GpdlaError) as err:
                call(tables=tables, model_weights=P, meanflux=False)
            assert "conditioned" in str(err.value)
    finally:
        batch.close()
        ctx.close()
    for res, names in ((mc, MMR.ARRAYS), (pf, PF_ALL)):
        o = res["offsets"]
        assert res["status"].tolist() == [UNDEFINED, 1, 0] and res["model_flags"].tolist() == [0, 0, 0]
        assert all(np.isnan(res[n][:o[2]]).all() for n in names) and all(np.isfinite(res[n][o[2]:]).all() for n in names)
        assert np.diff(o).tolist() == [40, 40, 33]
    assert np.isnan(mc["coef_mean"][:2]).all() and np.isfinite(mc["coef_mean"][2]).all()
    # an unprocessed multi-DLA batch has no resident tables either
    ctx, batch = _multi(model, samples, spectra, MultiParameters(max_dlas=md))
    try:
        with pytest.raises(_lib.GpdlaError) as err:
            batch.marginal_continuum_multi()
        assert "not been processed" in str(err.value)
    finally:
        batch.close()
        ctx.close()


# ------------------------------------------------------------------------------------------------
# 7. bit identity
# ------------------------------------------------------------------------------------------------

def test_bit_identity_under_a_reversed_selection():
    want = worker.run_case()
    n = len(worker.NUS)
    rev = np.arange(n)[::-1].copy()
    got, one = worker.run_case(rev), worker.run_case([3])
    assert (want["mc_status"] == 0).all() and np.isfinite(want["pf_flux_var"]).all() and np.isfinite(want["mc_continuum_var"]).all()
    fo, ro = want["mc_offsets"], got["mc_offsets"]
    np.testing.assert_array_equal(np.diff(ro), np.diff(fo)[rev])
    for j, q in enumerate(rev):
        for name in MMR.ARRAYS:
            assert np.array_equal(_bits(got[f"mc_{name}"][ro[j]:ro[j + 1]]), _bits(want[f"mc_{name}"][fo[q]:fo[q + 1]])), name
        for name in MMR.ROWS:
            assert np.array_equal(_bits(got[f"mc_{name}"][j]), _bits(want[f"mc_{name}"][q])), name
        for name in PF_ALL:
            assert np.array_equal(_bits(got[f"pf_{name}"][ro[j]:ro[j + 1]]), _bits(want[f"pf_{name}"][fo[q]:fo[q + 1]])), name
    for name in PF_ALL:
        assert np.array_equal(_bits(one[f"pf_{name}"]), _bits(want[f"pf_{name}"][fo[3]:fo[4]])), name
    for name in MMR.ARRAYS:
        assert np.array_equal(_bits(one[f"mc_{name}"]), _bits(want[f"mc_{name}"][fo[3]:fo[4]])), name


def test_bit_identity_across_launch_groups(tmp_path):
    """One call of each entry with the product library against the same calls in a clean child process that loads
    libgpdla_legacy.so with its debug-only budget GPDLA_MC_SCRATCH_BYTES shrunk to two quasars' scratch rows: three launch
    groups, the host tables staged group by group."""
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
    assert set(got.files) == set(want)
    for name in want:
        x, y = np.asarray(got[name]), np.asarray(want[name])
        assert x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), name
    assert np.isfinite(want["mc_continuum_var"]).all() and np.isfinite(want["pf_flux_var"]).all()


# ------------------------------------------------------------------------------------------------
# 9. file to file
# ------------------------------------------------------------------------------------------------

def test_command_line_multi_models_equals_the_in_memory_call(tmp_path):
    """python -m gp_dla_detection_amd.model_spectra --marginal-continuum --multi-models and --predictive-flux --multi-models
    --residuals on the -v7.3 files of a multi-DLA run, in batches of 3: the files hold what the in-memory calls return."""
    from gp_dla_detection_amd import io, model_spectra as cli
    fs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=12, num_samples=96)
    run_pos = np.flatnonzero(fs["test_ind"])
    spectra = [fs["spectra"][i] for i in run_pos]
    z = fs["catalog"]["z_qsos"][run_pos]
    processed = str(tmp_path / "processed.mat")
    p = MultiParameters(max_dlas=3)
    lp = gp.dla_existence_prior_multi(fs["prior"]["z_qsos"], fs["prior"]["dla_ind"], z, fs["Z_lls"], fs["Z_dla"], p)
    results = gp.process_qsos_multiple_dlas_meanflux(fs["model"], fs["samples"], spectra, lp, params=p)
    io.save_processed_qsos_multi(processed, results, test_ind=fs["test_ind"])
    sel = np.arange(0, len(spectra), 2)
    common = ["--preloaded", fs["paths"]["preloaded"], "--catalog", fs["paths"]["catalog"], "--model", fs["paths"]["learned"],
              "--samples", fs["paths"]["samples"], "--processed", processed, "--indices", ",".join(map(str, sel)),
              "--multi-models", "--max-quasars-per-batch", "3", "--components", "null"]     # (--components is ignored)
    out_mc, out_pf = str(tmp_path / "mc.mat"), str(tmp_path / "pf.mat")
    assert cli.main(common + ["--out", out_mc, "--marginal-continuum"]) == 0
    assert cli.main(common + ["--out", out_pf, "--predictive-flux", "--residuals"]) == 0
    kw = dict(params=p, selection=sel, multi_models=True)
    want_mc = gp.marginal_continuum(fs["model"], fs["samples"], spectra, results, **kw)
    want_pf = gp.predictive_flux(fs["model"], fs["samples"], spectra, results, residuals=True, **kw)
    back_mc, back_pf = io.load_model_spectra(out_mc), io.load_predictive_flux(out_pf)
    for back, want, cells in ((back_mc, want_mc, io.MARGINAL_CONTINUUM_CELLS), (back_pf, want_pf, io.PREDICTIVE_FLUX_CELLS)):
        np.testing.assert_array_equal(back["selection"], sel)
        np.testing.assert_array_equal(back["offsets"], want["offsets"])
        np.testing.assert_array_equal(back["status"], want["status"])
        np.testing.assert_array_equal(np.asarray(back["model_flags"]).reshape(-1), want["model_flags"])
        np.testing.assert_array_equal(np.asarray(back["model_weights"]).reshape(sel.size, 5), results["model_posteriors"][sel])
        for name in cells:
            for got, ref in zip(back[name], gp.split_cells(want[name], want["offsets"])):
                np.testing.assert_array_equal(got, ref, err_msg=name)
    for name in ("coef_mean", "coef_cov_within", "coef_cov_between"):
        np.testing.assert_array_equal(np.asarray(back_mc[name]).reshape(want_mc[name].shape), want_mc[name], err_msg=name)
    np.testing.assert_array_equal(back_pf["chi2"], want_pf["chi2"])
    np.testing.assert_array_equal(back_pf["num_kept"], want_pf["num_kept"])
    usable = np.flatnonzero((want_mc["status"] == 0) & (want_mc["model_flags"] == 0))
    print(f"{usable.size} of {sel.size} selected quasars usable; status {want_mc['status'].tolist()}, flags {want_mc['model_flags'].tolist()}")
    assert usable.size and all(np.isfinite(want_mc["continuum_var"][want_mc["offsets"][s]:want_mc["offsets"][s + 1]]).all() for s in usable)
    assert all(np.isfinite(want_pf["flux_mean"][want_pf["offsets"][s]:want_pf["offsets"][s + 1]]).all() for s in usable)
    # equal weights over all 2 + max_dlas components, and the refusal of a single-DLA file
    assert cli.main(common + ["--out", out_mc, "--marginal-continuum", "--model-weights", "equal"]) == 0
    eq = gp.marginal_continuum(fs["model"], fs["samples"], spectra, results, model_weights=np.ones((len(spectra), 5)), **kw)
    back = io.load_model_spectra(out_mc)
    for got, ref in zip(back["continuum_mean"], gp.split_cells(eq["continuum_mean"], eq["offsets"])):
        np.testing.assert_array_equal(got, ref)
    single = str(tmp_path / "single.mat")
    res1 = gp.process_qsos(fs["model"], fs["samples"], spectra, prior_catalog=fs["prior"])
    io.save_processed_qsos(single, res1, test_ind=fs["test_ind"])
    args1 = [single if a == processed else a for a in common]
    with pytest.raises(ValueError):
        cli.main(args1 + ["--out", out_mc, "--marginal-continuum"])
