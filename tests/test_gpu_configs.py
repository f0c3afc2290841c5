"""BASELINE.json configs 4 and 5 at their FULL sizes on the GPU, through the C-ABI.

Config 4: the multi-DLA driver (multi_dlas/process_qsos_multiple_dlas_meanflux.m) with n = 1500
pixels, S = 10 000 samples, max_dlas = 4.  The oracle cannot sweep 4 x 10^4 stacked-profile
likelihoods per quasar in test time, so parity is established (i) by the oracle on random
(sample, model) entries -- it is handed exactly the index chains those entries consume -- and (ii)
by size-independent properties recomputed on the host from the returned tables: NaN-aware
log-mean-exp evidences with their Occam terms (:400-409), the separation mask (:386-392), MAP =
argmax bookkeeping (:439-445), the posteriors (:482-495), and invariance under the HBM sub-batch
split of the profile table.

Config 5: the fp32-contraction study variant at k = 40 against the ORACLE (not against the repo's
own fp64 path), with the tolerance it actually meets written down, and its effect on the model
posteriors over 1000 quasars.
"""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters

pytestmark = pytest.mark.gpu
TOL = 1e-8
Z_LLS, Z_DLA = 0.31, 0.69


def multi_priors(spectra, p):
    cat = synthetic.make_prior_catalog()
    z = np.array([s["z_qso"] for s in spectra])
    return gp.dla_existence_prior_multi(cat["z_qsos"], cat["dla_ind"], z, Z_LLS, Z_DLA, p)


def nan_lme(col):
    """max + log(nanmean(exp(col - max))), multi :400-408."""
    mx = np.nanmax(col)
    return mx + np.log(np.nanmean(np.exp(col - mx)))


@pytest.fixture(scope="module")
def config4():
    p = MultiParameters()  # max_dlas = 4
    model = synthetic.make_model(20)
    S = 10000
    samples = synthetic.make_samples(S)
    spectra = synthetic.make_spectra(3, 1500, model, mask_fraction=0.02, first_index=700)
    lp = multi_priors(spectra, p)
    out = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p)
    return p, model, samples, spectra, lp, out


def test_config4_full_size_properties(config4):
    """The size-independent properties of the module docstring, at the workload's shape and NumPy's precision
    (the evidences and posteriors against 50-digit values: tests/test_gpu_multi_epilogue.py)."""
    p, model, samples, spectra, lp, out = config4
    S, md = 10000, p.max_dlas
    log_S = np.log(S)
    sll, base = out["sample_log_likelihoods_dla"], out["base_sample_inds"]
    assert sll.shape == (3, md, S) and base.shape == (3, md - 1, S)
    assert base.min() >= 1 and base.max() <= S and (out["status"] == 0).all()
    off, lognhi = samples["offset_samples"], samples["log_nhi_samples"]
    for q in range(3):
        z = out["min_z_dlas"][q] + (out["max_z_dlas"][q] - out["min_z_dlas"][q]) * off   # :309-311
        for nd in range(1, md + 1):
            col = sll[q, nd - 1]
            # separation mask (:386-392): any(diff(sort(z of the nd absorbers)) < min_z_separation)
            zs = np.stack([z] + [z[base[q, j].astype(np.int64) - 1] for j in range(nd - 1)], axis=0)
            close = (np.diff(np.sort(zs, axis=0), axis=0) < p.min_z_separation).any(axis=0) \
                if nd > 1 else np.zeros(S, bool)
            np.testing.assert_array_equal(np.isnan(col), close)
            assert (~close).sum() > S // 4
            # evidence with the Occam terms (:400-409)
            assert abs(out["log_likelihoods_dla"][q, nd - 1] - (nan_lme(col) - log_S * (nd - 1))) < 1e-9
            # MAP bookkeeping (:439-445): first nanmax, then its chain of base indices
            arg = int(np.nanargmax(col))
            chain = [arg] + [int(base[q, j, arg]) - 1 for j in range(nd - 1)]
            np.testing.assert_array_equal(out["MAP_inds"][q, nd - 1, :nd], np.array(chain) + 1.0)
            np.testing.assert_array_equal(out["MAP_z_dlas"][q, nd - 1, :nd], z[chain])
            np.testing.assert_array_equal(out["MAP_log_nhis"][q, nd - 1, :nd], lognhi[chain])
            assert np.isnan(out["MAP_inds"][q, nd - 1, nd:]).all()
            # the weighted resampling only draws indices that carry weight in the previous model
            if nd < md:
                assert np.isfinite(col[base[q, nd - 1].astype(np.int64) - 1]).all()
        assert abs(out["log_likelihoods_lls"][q] - nan_lme(out["sample_log_likelihoods_lls"][q])) < 1e-9
        # posteriors (:300-301, :411-413, :428-430, :482-495)
        lpost = np.concatenate([[lp[0][q] + out["log_likelihoods_no_dla"][q]],
                                [lp[1][q] + out["log_likelihoods_lls"][q]],
                                lp[2][q] + out["log_likelihoods_dla"][q]])
        np.testing.assert_allclose(np.concatenate([[out["log_posteriors_no_dla"][q]],
                                                   [out["log_posteriors_lls"][q]],
                                                   out["log_posteriors_dla"][q]]), lpost, rtol=0, atol=1e-12)
        mp = np.exp(lpost - np.nanmax(lpost))
        mp /= mp.sum()
        np.testing.assert_allclose(out["model_posteriors"][q], mp, rtol=0, atol=1e-12)
        assert abs(out["p_dlas"][q] - (1 - mp[0] - mp[1])) < 1e-12


def test_config4_oracle_on_random_entries(config4, oracle):
    """48 samples (16 per quasar) x all 4 models + the sub-DLA model against the oracle: a reduced
    sample list holds each picked sample followed by the chain base_sample_inds gives it, and the
    oracle runs the whole driver on that list.  Its Occam term is -log(S') for the reduced list,
    which is put back to -log(S)."""
    p, model, samples, spectra, lp, out = config4
    S, md = 10000, p.max_dlas
    rng = np.random.default_rng(4)
    checked = 0
    for q, sp in enumerate(spectra):
        base = out["base_sample_inds"][q].astype(np.int64) - 1      # [md-1, S], 0-based
        picks = rng.choice(S, 16, replace=False)
        chains = np.stack([picks] + [base[j, picks] for j in range(md - 1)], axis=1)  # [16, md]
        flat = chains.reshape(-1)                                    # reduced sample r = 4 t + j
        Sr = flat.size
        red_base = np.ones((md - 1, Sr), dtype=np.uint32)            # others: any valid index
        for t in range(picks.size):
            red_base[:, 4 * t] = 4 * t + 1 + np.arange(1, md)        # 1-based positions of the chain
        ref = oracle.process_spectrum_multi(
            model, samples["offset_samples"][flat], samples["nhi_samples"][flat],
            samples["log_nhi_samples"][flat], samples["lls_nhi_samples"][flat], red_base,
            sp["wavelengths"], sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"],
            max_dlas=md, num_forest_lines=p.num_forest_lines, min_z_separation=p.min_z_separation,
            prev_tau_0=p.prev_tau_0, prev_beta=p.prev_beta)
        shift = np.log(Sr) - np.log(S)
        assert abs(out["log_likelihoods_no_dla"][q] - ref["log_likelihood_no_dla"]) < TOL
        assert abs(out["min_z_dlas"][q] - ref["min_z_dla"]) < 1e-14
        for t, i in enumerate(picks):
            want = ref["sample_log_likelihoods_dla"][4 * t] + shift    # [md]
            got = out["sample_log_likelihoods_dla"][q, :, i]
            np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
            assert np.nanmax(np.abs(got - want)) < TOL, (q, i, got, want)
            lls = ref["sample_log_likelihoods_lls"][4 * t] + shift
            assert abs(out["sample_log_likelihoods_lls"][q, i] - lls) < TOL
            checked += md + 1
    assert checked == 48 * 5


def test_config4_sub_batch_split_is_invisible(config4):
    """The profile table (243 MB per quasar at this size) is swept in sub-batches that fit an HBM
    budget (default 16 GiB = 67 quasars).  With the budget set to ONE quasar's worth the three
    quasars go through three sub-batches; every output must equal the single-sub-batch run bit
    for bit (same Philox keys: the generator is keyed by the global quasar index)."""
    p, model, samples, spectra, lp, out = config4
    one_quasar = 2 * 10000 * 1520 * 8
    p1 = MultiParameters(multi_profile_bytes=one_quasar)
    split = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p1)
    for key in ("sample_log_likelihoods_dla", "sample_log_likelihoods_lls", "base_sample_inds",
                "log_likelihoods_dla", "log_likelihoods_lls", "model_posteriors", "MAP_inds"):
        np.testing.assert_array_equal(split[key], out[key], err_msg=key)
    # and host-side batching (two resident batches, first_quasar_index advanced) likewise
    two = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p,
                                                 max_quasars_per_batch=2)
    for key in ("sample_log_likelihoods_dla", "base_sample_inds", "model_posteriors"):
        np.testing.assert_array_equal(two[key], out[key], err_msg=key)


def test_config4_resident_batch_and_summary_row(config4):
    """The resident form (gpdla_batch_process_multi): results stay in HBM, the 78-column summary
    row is what a multi-GPU run gathers, and it carries every non-per-sample saved variable."""
    from gp_dla_detection_amd.distributed import summary_to_fields_multi
    p, model, samples, spectra, lp, out = config4
    ctx = gp.Context(0, p)
    ctx.set_model(model)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra, lp[0], lp[2], lp[1])
    batch.process_multi()
    ctx.synchronize()
    t = batch.summary_tensor()
    assert tuple(t.shape) == (3, 78) and t.is_cuda
    f = summary_to_fields_multi(t, p.max_dlas)
    for key in ("min_z_dlas", "max_z_dlas", "log_likelihoods_no_dla", "log_likelihoods_lls",
                "log_likelihoods_dla", "log_posteriors_no_dla", "log_posteriors_lls", "log_posteriors_dla",
                "model_posteriors", "p_no_dlas", "p_lls", "p_dlas", "MAP_z_dlas", "MAP_log_nhis", "MAP_inds"):
        np.testing.assert_array_equal(f[key], out[key], err_msg=key)
    np.testing.assert_array_equal(f["log_priors_dla"], np.asarray(lp[2]))
    assert np.isnan(f["all_exceptions"]).all()
    sd, sl = batch.samples_multi_tensors()
    np.testing.assert_array_equal(sd.cpu().numpy(), out["sample_log_likelihoods_dla"])
    np.testing.assert_array_equal(sl.cpu().numpy(), out["sample_log_likelihoods_lls"])
    batch.close()
    ctx.close()


def test_undrawn_base_indices_do_not_fault(oracle):
    """Replaying a reference file: rows of base_sample_inds the reference never drew are zero
    (multi :116, :460-464).  A zero must not be followed (it would read before the table): the
    samples that would consume it come out NaN, everything else is untouched; an index above S is
    rejected outright."""
    from gp_dla_detection_amd import _lib
    p = MultiParameters(max_dlas=3)
    model = synthetic.make_model(20)
    S = 96
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(75 + i, 240, model) for i in range(2)]
    lp = multi_priors(spectra, p)
    drawn = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p)
    bsi = drawn["base_sample_inds"].copy()
    bsi[0, 1, :] = 0          # quasar 0: the row for model 3 was never drawn
    bsi[1, 0, ::2] = 0        # quasar 1: half of the row for model 2
    out = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p,
                                                 base_sample_inds=bsi)
    np.testing.assert_array_equal(out["sample_log_likelihoods_dla"][:, 0], drawn["sample_log_likelihoods_dla"][:, 0])
    np.testing.assert_array_equal(out["sample_log_likelihoods_dla"][0, 1], drawn["sample_log_likelihoods_dla"][0, 1])
    assert np.isnan(out["sample_log_likelihoods_dla"][0, 2]).all()
    assert np.isnan(out["log_likelihoods_dla"][0, 2])
    # MATLAB's nanmax of an all-NaN column returns index 1 (:439); its chain is followed as far
    # as it was drawn, the undrawn slot stays NaN
    np.testing.assert_array_equal(out["MAP_inds"][0, 2], [1.0, float(bsi[0, 0, 0]), np.nan])
    assert np.isnan(out["sample_log_likelihoods_dla"][1, 1, ::2]).all()
    np.testing.assert_array_equal(out["sample_log_likelihoods_dla"][1, 1, 1::2],
                                  drawn["sample_log_likelihoods_dla"][1, 1, 1::2])
    assert np.isnan(out["sample_log_likelihoods_dla"][1, 2, ::2]).all()   # model 3 consumes row 0 too
    bad = drawn["base_sample_inds"].copy()
    bad[1, 1, 7] = S + 1
    with pytest.raises(_lib.GpdlaError) as e:
        gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p, base_sample_inds=bad)
    assert e.value.code == -1


def test_resampling_follows_the_weights():
    """k_multi_resample stands in for randsample(S, S, true, W) (multi :467-472): at S = 10^4 the
    drawn indices must be distributed as W = exp(ll - max) / sum.  Chi-square over ~40 bins of
    (nearly) equal probability mass along the sample axis (S draws; bins expecting <= 5 draws are
    left out; 99.99 % quantile), for the first resampling step of 4 quasars; plus independence of
    the stream across quasars.  (Every single draw is restated exactly, at small shapes, in
    tests/test_gpu_multi_epilogue.py.)"""
    from scipy.stats import chi2
    p = MultiParameters(max_dlas=2)
    model = synthetic.make_model(20)
    S = 10000
    samples = synthetic.make_samples(S)
    spectra = synthetic.make_spectra(4, 600, model, first_index=720)
    out = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, multi_priors(spectra, p), params=p)
    for q in range(4):
        col = out["sample_log_likelihoods_dla"][q, 0]
        w = np.exp(col - np.nanmax(col))
        w[np.isnan(w)] = 0.0
        w /= w.sum()
        draws = out["base_sample_inds"][q, 0].astype(np.int64) - 1
        cum = np.concatenate([[0.0], np.cumsum(w)])                 # cum[i] = sum w[:i]
        edges = np.searchsorted(cum, np.arange(1, 40) / 40.0)       # ~40 bins of equal probability mass
        bins = np.searchsorted(edges, draws, side="right")          # bin b: edges[b-1] <= draw < edges[b]
        observed = np.bincount(bins, minlength=40).astype(np.float64)
        expected = S * np.diff(np.concatenate([[0.0], cum[edges], [1.0]]))
        assert observed[expected == 0].sum() == 0                   # nothing drawn where W = 0
        ok = expected > 5
        stat = ((observed - expected)[ok] ** 2 / expected[ok]).sum()
        assert stat < chi2.ppf(0.9999, int(ok.sum())), (q, stat, int(ok.sum()))
    assert (out["base_sample_inds"][0, 0] != out["base_sample_inds"][1, 0]).mean() > 0.5


# ------------------------------------------------------------------------------ config 5

def test_config5_fp32_contraction_vs_oracle(oracle):
    """BASELINE config 5: k = 40, contraction [W|U].[P|M] on the fp32 matrix cores (fp32
    accumulation over the n = 1500 pixels), everything else -- Voigt profile, weights, quadratic
    form, log-determinant, Cholesky -- in fp64.  Checked against the ORACLE on 2 quasars x 64
    random samples + the null model.

    Tolerance this variant actually meets (and why it is a study variant, not a parity path):
    the fp32 accumulation of B = I + sum w m m' and v = sum u m carries ~n * 2^-24 relative error
    into log det B and v'B^-1 v, and the quadratic form cancels ~10^4 against ~10^4; the measured
    error is a few tenths of a nat on single log-likelihoods of magnitude 10^3 - 10^4.  The bound
    asserted here is 2.0 nats absolute (4e-4 relative)."""
    model = synthetic.make_model(40)
    S = 10000
    samples = synthetic.make_samples(S)
    spectra = synthetic.make_spectra(2, 1500, model, first_index=740)
    lp = (np.full(2, np.log(0.9)), np.full(2, np.log(0.1)))
    got = gp.process_qsos(model, samples, spectra, log_priors=lp, params=gp.Parameters(contraction_precision=1))
    f64 = gp.process_qsos(model, samples, spectra, log_priors=lp)
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(S, 64, replace=False))
    worst32 = worst64 = 0.0
    for i, sp in enumerate(spectra):
        ref = oracle.process_spectrum(model, samples["offset_samples"][pick], samples["nhi_samples"][pick],
                                      sp["wavelengths"], sp["flux"], sp["noise_variance"],
                                      sp["pixel_mask"], sp["z_qso"])
        want = ref["sample_log_likelihoods_dla"]
        worst32 = max(worst32, np.abs(got["sample_log_likelihoods_dla"][i, pick] - want).max(),
                      abs(got["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]))
        worst64 = max(worst64, np.abs(f64["sample_log_likelihoods_dla"][i, pick] - want).max(),
                      abs(f64["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]))
    print(f"config 5: max |delta| vs oracle: fp32 contraction {worst32:.3e}, fp64 {worst64:.3e}")
    assert worst64 < TOL          # the parity-grade path at the same shape
    assert worst32 < 2.0          # the study variant: see the docstring
    assert worst32 > 1e-6         # and it IS the fp32 path that ran
    assert np.isfinite(got["sample_log_likelihoods_dla"]).all()


def test_config5_effect_on_model_posteriors_over_1000_quasars():
    """What the fp32 contraction does to the quantity the catalogue is built from: p_DLA and
    model_posteriors over 1000 quasars (k = 40, n = 1500, S = 10^4), fp32-contraction vs the fp64
    path (which the tests above pin to the oracle at 1e-8).  With the synthetic catalogue's priors
    every posterior is saturated (evidence ratios of e^100s), which would hide any error, so the
    comparison is ALSO made with adversarial priors that put every quasar within e^+-3 of even
    odds under the fp64 evidences -- the worst case for a perturbed evidence:
    delta p <= p (1 - p) * delta(log odds) <= 0.25 * (|d log ev DLA| + |d log ev null|)."""
    model = synthetic.make_model(40)
    samples = synthetic.make_samples(10000)
    base = synthetic.make_spectra(100, 1500, model, first_index=760)
    rng = np.random.default_rng(6)
    spectra = []
    for r in range(10):  # 1000 distinct quasars: 100 templates x 10 independent noise draws
        for sp in base:
            s = dict(sp)
            s["flux"] = sp["flux"] + np.sqrt(sp["noise_variance"]) * 0.5 * rng.standard_normal(sp["flux"].size)
            spectra.append(s)
    cat = synthetic.make_prior_catalog()
    z = np.array([s["z_qso"] for s in spectra])
    lp = gp.dla_existence_prior(cat["z_qsos"], cat["dla_ind"], z)
    f32 = gp.Parameters(contraction_precision=1)
    a = gp.process_qsos(model, samples, spectra, log_priors=lp)
    b = gp.process_qsos(model, samples, spectra, log_priors=lp, params=f32)
    d_ev = np.abs(b["log_likelihoods_dla"] - a["log_likelihoods_dla"])
    d_no = np.abs(b["log_likelihoods_no_dla"] - a["log_likelihoods_no_dla"])
    assert np.isfinite(b["p_dlas"]).all()
    assert np.abs(b["p_dlas"] - a["p_dlas"]).max() < 1e-6  # saturated either way
    # adversarial priors: prior log-odds = -(evidence log-ratio) + U(-3, 3)
    x = -(a["log_likelihoods_dla"] - a["log_likelihoods_no_dla"]) + rng.uniform(-3, 3, len(spectra))
    adv = (-np.logaddexp(0.0, x), -np.logaddexp(0.0, -x))        # (log p(no DLA), log p(DLA))
    a2 = gp.process_qsos(model, samples, spectra, log_priors=adv)
    b2 = gp.process_qsos(model, samples, spectra, log_priors=adv, params=f32)
    assert (np.abs(a2["p_dlas"] - 0.5) < 0.46).all()              # every quasar really is undecided
    d_p = np.abs(b2["p_dlas"] - a2["p_dlas"])
    d_mp = np.abs(b2["model_posteriors"] - a2["model_posteriors"]).max()
    flips = (a2["p_dlas"] > 0.5) != (b2["p_dlas"] > 0.5)
    print(f"config 5 over {len(spectra)} quasars: max |d log evidence| DLA {d_ev.max():.3e} / null "
          f"{d_no.max():.3e}; adversarial priors: max |d p_DLA| {d_p.max():.3e} (mean {d_p.mean():.3e}), "
          f"max |d model_posteriors| {d_mp:.3e}, flips at 0.5: {int(flips.sum())}")
    assert d_ev.max() < 0.1 and d_no.max() < 0.1
    assert d_p.max() <= 0.25 * (d_ev.max() + d_no.max()) + 1e-12
    assert d_p.max() < 0.02 and d_mp < 0.02
    assert (np.abs(a2["p_dlas"][flips] - 0.5) < 0.01).all()       # only razor-edge cases can flip
