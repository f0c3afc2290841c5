"""The multi-DLA epilogue -- k_multi_evidence, k_multi_resample, k_multi_posteriors (csrc/multi_kernels.hpp,
DESIGN.md 4.7) -- against its exact restatement (tests/multi_epilogue_restatement.py), alone: every case runs the
driver once, downloads the GPU's OWN sample_log_likelihoods_dla / _lls and base_sample_inds, and the restatement is
fed those tables bit for bit, so the sweeps' 1e-8 parity with the oracle does not enter.

What a case asserts (``check_epilogue``):

* resampling, every draw of every model step: base_sample_inds[q, nd-1, j] - 1 is in ``acceptable(col_nd, u_j)``
  with u_j restated from (rng_seed, first_quasar_index + q, nd, j); where that set has one member -- all but at
  most 1 in 10^5 draws, counted -- this is equality; rows behind an early exit stay 0;
* separation mask: the NaN pattern of model nd >= 2 is ``separation_mask``, no absorber pair being within 4 ulp of
  min_z_separation (so that a fused multiply-add in z could not flip a sample);
* evidences: |gpu - evidence_exact| <= 2 spacing(|max|) + (ceil(S/256) + 16) 2^-52 (``evidence_bound``);
* MAP_inds / MAP_z_dlas / MAP_log_nhis: ``map_chain`` exactly, slots beyond nd NaN;
* posteriors: log posteriors are fl(prior + evidence) exactly; model_posteriors, p_no_dlas, p_lls within 8 ulp of
  ``posteriors_exact``, p_dlas within 8 ulp of 1.

Sample counts: 1 (if the driver takes it), 63, 255, 256, 257, 513, 1025 -- fewer samples than threads, threads wholly
past the end (257: chunk 2, threads 129 .. 255 idle), chunks of 1, 2, 3 and 5 -- and 19200, the limit of the
resampling's LDS, with 19201 refused.  Each with three 61 .. 96 pixel quasars from ``synthetic``: one clean, one
behind a strong injected absorber (a few live samples, most weights exactly 0), one with masked pixels.

Measured on the MI355X (recorded here, used by no assertion): 33 669 draws over the cases, none with more than one
acceptable index and none outside its set; worst evidence error / bound 0.44 (the ties case at S = 514; 0.17 at
S = 19200); posteriors within 2.3 ulp, p_dlas within 1.1 ulp of 1 -- after k_multi_posteriors was changed to carry
the rounding error of ``log posterior - max`` into the exponential; without that, float64 arithmetic in the
kernel's order puts a posterior of e^-190 off by 94 ulp (see test_posteriors_at_their_edges).  The whole file takes 3.3 s, its slowest case (S = 1, the first to touch the
GPU) 1.8 s, S = 19200 0.6 s.
"""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, synthetic
from gp_dla_detection_amd.parameters import MultiParameters

import multi_epilogue_restatement as R

pytestmark = pytest.mark.gpu
Z_LLS, Z_DLA = 0.31, 0.69
SEED = 0x5EED0D1A00C0FFEE            # a non-default rng_seed, both halves non-zero
DEFAULT_SEED = MultiParameters().rng_seed
_cache = {}


def model():
    if "model" not in _cache:
        _cache["model"] = synthetic.make_model(20)
    return _cache["model"]


def samples_of(S):
    if ("samples", S) not in _cache:
        _cache["samples", S] = synthetic.make_samples(S)
    return _cache["samples", S]


def quasars():
    """Clean (96 pixels, no absorber, the noise variance taken 100 times larger: a broad posterior in which nearly
    every sample carries weight), strong absorber (72 pixels, log N_HI = 21.3 injected at 0.3 of its search
    range and the noise variance taken 20 times smaller, which leaves a handful of samples with weight and nine in
    ten with none at all), masked (61 pixels, a tenth of them masked, synthetic's own absorber)."""
    if "quasars" not in _cache:
        p = MultiParameters()
        clean = synthetic.make_spectrum(9100, 96, model())
        clean = dict(clean, noise_variance=100.0 * clean["noise_variance"])
        strong = synthetic.make_spectrum(9102, 72, model())
        wl, zq = strong["wavelengths"], strong["z_qso"]
        z = 0.7 * p.min_z_dla(wl, zq) + 0.3 * p.max_z_dla(wl, zq)
        strong = dict(strong, flux=strong["flux"] * synthetic._injected_absorption(wl, z, 10.0 ** 21.3, p.num_lines),
                      noise_variance=0.05 * strong["noise_variance"])
        masked = synthetic.make_spectrum(9105, 61, model(), mask_fraction=0.1)
        assert clean["true_z_dla"] is None and masked["true_z_dla"] is not None and masked["pixel_mask"].sum() > 0
        _cache["quasars"] = [clean, strong, masked]
    return _cache["quasars"]


def priors(spectra, p):
    cat = synthetic.make_prior_catalog()
    z = np.array([s["z_qso"] for s in spectra])
    return gp.dla_existence_prior_multi(cat["z_qsos"], cat["dla_ind"], z, Z_LLS, Z_DLA, p)


def check_epilogue(out, samples, p, lp, supplied=False, label=""):
    """Every assertion of the module docstring on one driver output; returns the counts it prints."""
    sll, sll_lls, base = out["sample_log_likelihoods_dla"], out["sample_log_likelihoods_lls"], out["base_sample_inds"]
    nq, md, S = sll.shape
    assert base.shape == (nq, md - 1, S) and (out["status"] == 0).all()
    off, lognhi = samples["offset_samples"], samples["log_nhi_samples"]
    stats = dict(draws=0, ambiguous=0, undecided=0, evidence=0.0, posterior=0.0, p_dla=0.0, live=[], zero=[], exits=0)

    def evidence(got, col, nd):
        mx, _, want = R.evidence_exact(col, nd)
        if np.isnan(mx):
            assert np.isnan(got)
            return
        err = float(abs(R.mp.mpf(float(got)) - want)) / R.evidence_bound(mx, S) if np.isfinite(got) else np.inf
        stats["evidence"] = max(stats["evidence"], err)
        assert err <= 1.0, (label, nd, got, float(want), err)

    for q in range(nq):
        z = out["min_z_dlas"][q] + (out["max_z_dlas"][q] - out["min_z_dlas"][q]) * off       # multi :309-311
        alive = True
        for nd in range(1, md + 1):
            col = sll[q, nd - 1]
            if not alive:        # behind the early exit (multi :460-464): nothing evaluated, nothing drawn
                assert np.isnan(col).all() and np.isnan(out["log_likelihoods_dla"][q, nd - 1])
                for key in ("MAP_inds", "MAP_z_dlas", "MAP_log_nhis"):
                    assert np.isnan(out[key][q, nd - 1]).all()
                if nd < md and not supplied:
                    assert (base[q, nd - 1] == 0).all()
                continue
            if nd > 1:
                assert R.closest_to_separation(z, base[q], nd, p.min_z_separation) >= 4.0
                np.testing.assert_array_equal(np.isnan(col), R.separation_mask(z, base[q], nd, p.min_z_separation))
            evidence(out["log_likelihoods_dla"][q, nd - 1], col, nd)
            chain = R.map_chain(col, base[q], nd)
            np.testing.assert_array_equal(out["MAP_inds"][q, nd - 1, :nd], chain)
            idx = np.where(np.isnan(chain), 0, chain - 1).astype(np.int64)
            np.testing.assert_array_equal(out["MAP_z_dlas"][q, nd - 1, :nd], np.where(np.isnan(chain), np.nan, z[idx]))
            np.testing.assert_array_equal(out["MAP_log_nhis"][q, nd - 1, :nd], np.where(np.isnan(chain), np.nan, lognhi[idx]))
            for key in ("MAP_inds", "MAP_z_dlas", "MAP_log_nhis"):
                assert np.isnan(out[key][q, nd - 1, nd:]).all()
            if np.isnan(out["log_likelihoods_dla"][q, nd - 1]):
                alive = False
                stats["exits"] += 1
            if nd < md and not supplied:
                if not alive:
                    assert (base[q, nd - 1] == 0).all()
                    continue
                m = R.uniforms(p.rng_seed, p.first_quasar_index + q, nd, S)
                ex = R.weights_exact(col)
                drawn = base[q, nd - 1].astype(np.int64) - 1
                unique, other = R.acceptable_all(col, m, ex)
                wrong = np.flatnonzero((unique >= 0) & (drawn != unique))
                assert wrong.size == 0, (label, q, nd, wrong[:8], drawn[wrong[:8]], unique[wrong[:8]])
                for j, allowed in other.items():
                    assert int(drawn[j]) in allowed, (label, q, nd, j, int(drawn[j]), allowed)
                stats["draws"] += S
                stats["ambiguous"] += sum(1 for s in other.values() if len(s) > 1)
                stats["undecided"] += len(other)
                if nd == 1:      # weights that can matter in a double sum / that are exactly 0 in a double
                    d = col - ex["max"]
                    stats["live"].append(int((d > -36.0).sum()))
                    stats["zero"].append(int((d < -745.2).sum()))
        evidence(out["log_likelihoods_lls"][q], sll_lls[q], 1)
        # posteriors (multi :300-301, :411-413, :428-430, :482-495)
        prior = np.concatenate([[lp[0][q]], [lp[1][q]], np.asarray(lp[2]).reshape(nq, md)[q]])
        ll = np.concatenate([[out["log_likelihoods_no_dla"][q]], [out["log_likelihoods_lls"][q]], out["log_likelihoods_dla"][q]])
        lpost, post, p_dla = R.posteriors_exact(prior, ll)
        got_lpost = np.concatenate([[out["log_posteriors_no_dla"][q]], [out["log_posteriors_lls"][q]], out["log_posteriors_dla"][q]])
        np.testing.assert_array_equal(got_lpost, lpost)
        if np.isnan(lpost).any():        # MATLAB's sum() does not skip NaN (:491)
            for key in ("model_posteriors", "p_no_dlas", "p_lls", "p_dlas"):
                assert np.isnan(out[key][q]).all(), key
            continue
        for got, want in list(zip(out["model_posteriors"][q], post)) + [(out["p_no_dlas"][q], post[0]), (out["p_lls"][q], post[1])]:
            stats["posterior"] = max(stats["posterior"], R.ulps(got, want))
        err = float(abs(R.mp.mpf(float(out["p_dlas"][q])) - p_dla)) / 2.0 ** -52
        stats["p_dla"] = max(stats["p_dla"], err)
        assert stats["posterior"] <= 8.0 and err <= 8.0, (label, q, stats["posterior"], err, out["model_posteriors"][q])
    # all but at most 1 in 10^5 draws are decided: equality was asserted for them
    assert stats["ambiguous"] * 10 ** 5 <= stats["draws"]
    print(f"{label}: {stats['draws']} draws, {stats['ambiguous']} with more than one acceptable index "
          f"({stats['undecided']} not decided by the double-precision bracket), model 1: weights above 2^-52 {stats['live']}, "
          f"exactly 0 {stats['zero']}, "
          f"early exits {stats['exits']}; worst evidence error / bound {stats['evidence']:.3f}; posteriors within "
          f"{stats['posterior']:.2f} ulp, p_dlas within {stats['p_dla']:.2f} ulp of 1")
    return stats


#            S,    rng_seed,     first_quasar_index
CASES = [(1, DEFAULT_SEED, 0), (63, DEFAULT_SEED, 2 ** 32 + 5), (255, SEED, 7), (256, DEFAULT_SEED, 2 ** 32 + 5),
         (257, DEFAULT_SEED, 0), (513, SEED, 2 ** 32 + 5), (1025, SEED, 0)]


@pytest.mark.parametrize("S,seed,first", CASES, ids=[f"S{c[0]}" for c in CASES])
def test_epilogue_restated_exactly(S, seed, first):
    """max_dlas = 3, the three quasars of ``quasars()``; the keys cover a quasar index above 2^32 and a seed with a
    non-zero high half, separately and together.  (S = 1: one sample, so model 2 pairs it with itself, every
    sample of model 2 is masked and the quasar leaves at the early exit -- the smallest S is run as it is.)"""
    p = MultiParameters(max_dlas=3, rng_seed=seed, first_quasar_index=first)
    spectra, samples = quasars(), samples_of(S)
    lp = priors(spectra, p)
    out = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, lp, params=p)
    stats = check_epilogue(out, samples, p, lp, label=f"S = {S}")
    if S >= 255:
        assert stats["draws"] == 3 * 2 * S                       # nobody left early: every step was drawn
        assert stats["zero"][1] > (3 * S) // 4 and stats["live"][1] <= S // 16         # the peaked column
        assert stats["live"][0] > S // 2 and stats["zero"][0] == 0                     # and the broad one


def test_early_exit_leaves_the_later_rows_zero():
    """A min_z_separation wider than the search range masks all of model 2: its evidence is NaN, row 1 of
    base_sample_inds (drawn after model 2) stays 0, model 3 is never evaluated and every posterior is NaN --
    while row 0, drawn from model 1, is restated draw by draw."""
    p = MultiParameters(max_dlas=3, min_z_separation=10.0, first_quasar_index=2 ** 32 + 5)
    spectra, samples = quasars(), samples_of(63)
    lp = priors(spectra, p)
    out = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, lp, params=p)
    stats = check_epilogue(out, samples, p, lp, label="early exit")
    assert stats["exits"] == 3 and stats["draws"] == 3 * 63
    assert (out["base_sample_inds"][:, 0] >= 1).all() and (out["base_sample_inds"][:, 1] == 0).all()


def test_sample_count_at_the_limit_of_the_resampling():
    """S = 19200: 150 KiB of dynamic LDS, chunks of 75; max_dlas = 2 and one 48-pixel quasar (a profile table of
    2 x 19200 x 64 doubles)."""
    S = 19200
    p = MultiParameters(max_dlas=2, rng_seed=SEED, first_quasar_index=2 ** 32 + 5)
    spectra, samples = [synthetic.make_spectrum(9110, 48, model())], samples_of(S)
    lp = priors(spectra, p)
    out = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, lp, params=p)
    stats = check_epilogue(out, samples, p, lp, label="S = 19200")
    assert stats["draws"] == S


def test_one_sample_more_is_refused_and_the_context_lives():
    """S = 19201 returns GPDLA_ERR_UNSUPPORTED naming the limit; the context then takes S = 63 and gives what a
    fresh one gives."""
    p = MultiParameters(max_dlas=2)
    spectra = [synthetic.make_spectrum(9110, 48, model())]
    lp = priors(spectra, p)
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(model())
        ctx.set_samples(samples_of(19201))
        batch = ctx.upload(spectra, lp[0], lp[2], lp[1])
        with pytest.raises(_lib.GpdlaError) as e:
            batch.process_multi()
        assert e.value.code == -5 and "19200" in str(e.value)        # GPDLA_ERR_UNSUPPORTED
        batch.close()
        ctx.synchronize()
        ctx.set_samples(samples_of(63))
        batch = ctx.upload(spectra, lp[0], lp[2], lp[1])
        batch.process_multi()
        got = batch.download_multi()
        batch.close()
    finally:
        ctx.close()
    want = gp.process_qsos_multiple_dlas_meanflux(model(), samples_of(63), spectra, lp, params=p)
    for key in ("sample_log_likelihoods_dla", "sample_log_likelihoods_lls", "base_sample_inds", "log_likelihoods_dla",
                "log_likelihoods_lls", "model_posteriors", "MAP_inds", "p_dlas"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    check_epilogue(got, samples_of(63), p, lp, label="after the refusal")


@pytest.mark.parametrize("S", [512, 514])
def test_ties_take_the_first_index(S):
    """The sample list is the same S/2 samples twice and the supplied base_sample_inds has two equal halves, so every
    model's column holds exact pairs (asserted on the GPU's own columns: if the halves differed in a bit, the
    sweep would not be position-independent and this would not be a tie -- that is reported, not assumed).  The
    MAP index is the first of its pair in every model, through lanes, waves and the four-wave merge of
    nan_evidence (S = 512: the partner is 256 further, the same thread's next sample; S = 514: 257 further, the
    next thread, for lane 63 the next wave); the evidence is that of the half list, to the bound."""
    h = S // 2
    half = samples_of(h)
    samples = {k: np.concatenate([v, v]) for k, v in half.items()}
    p = MultiParameters(max_dlas=3)
    spectra = quasars()
    lp = priors(spectra, p)
    rng = np.random.default_rng(S)
    hb = rng.integers(1, S + 1, size=(3, 2, h), dtype=np.uint32)
    base = np.concatenate([hb, hb], axis=2)
    out = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, lp, params=p, base_sample_inds=base)
    np.testing.assert_array_equal(out["base_sample_inds"], base)
    sll = out["sample_log_likelihoods_dla"]
    assert np.array_equal(sll[:, :, :h], sll[:, :, h:], equal_nan=True), "the sweep is not position-independent"
    np.testing.assert_array_equal(out["sample_log_likelihoods_lls"][:, :h], out["sample_log_likelihoods_lls"][:, h:])
    check_epilogue(out, samples, p, lp, supplied=True, label=f"ties, S = {S}")
    for q in range(3):
        for nd in range(1, 4):
            col = sll[q, nd - 1]
            first = int(out["MAP_inds"][q, nd - 1, 0]) - 1
            assert first < h and col[first] == col[first + h] == np.nanmax(col)
            mx, arg, want = R.evidence_exact(col[:h], nd)
            assert arg == first
            with R.mp.workdps(R.DPS):
                want = want + (nd - 1) * (R.mp.log(h) - R.mp.log(S))
                err = float(abs(R.mp.mpf(float(out["log_likelihoods_dla"][q, nd - 1])) - want))
            assert err <= R.evidence_bound(mx, S), (q, nd, err)


def test_posteriors_at_their_edges():
    """Supplied indices and priors, S = 96: quasar 0 with log priors that push the sub-DLA model and model 3 more
    than 745 below the rest, so that their posteriors are exactly 0 while the others are held to 8 ulp; quasar 1
    whose row for model 3 is all zero (never drawn), so that model 3's evidence is NaN and the NaN propagates into
    every posterior as the reference's sum() does; quasar 2 whose row for model 2 is all zero: ``alive`` stops
    model 3 as well; quasars 3 and 4 (the spectra of 0 and 2 again) with priors that put posteriors at
    e^-150 .. e^-600 -- small, normal numbers, whose 8 ulp need the rounding error of ``log posterior - max``
    carried into the exponential (k_multi_posteriors; without it they are off by up to 2^-53 times that
    difference, 30 .. 130 ulp: the regression case of that fix)."""
    S = 96
    p = MultiParameters(max_dlas=3)
    spectra, samples = quasars(), samples_of(S)
    spectra = spectra + [spectra[0], spectra[2]]
    lp = [np.array(x, dtype=np.float64) for x in priors(spectra, p)]
    lp[1][0] -= 2000.0
    lp[2][0, 2] -= 2500.0
    lp[1][3] -= 150.0
    lp[2][3] -= [300.0, 450.0, 560.0]
    lp[0][4] -= 333.0
    lp[2][4] -= [0.0, 222.0, 0.0]
    base = np.random.default_rng(96).integers(1, S + 1, size=(5, 2, S), dtype=np.uint32)
    base[1, 1] = 0
    base[2, 0] = 0
    out = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, tuple(lp), params=p, base_sample_inds=base)
    stats = check_epilogue(out, samples, p, lp, supplied=True, label="posterior edges")
    assert stats["exits"] == 2
    mp0 = out["model_posteriors"][0]
    assert mp0[1] == 0.0 and mp0[4] == 0.0 and out["p_lls"][0] == 0.0 and (mp0[[0, 2, 3]] > 0).all()
    assert abs(mp0.sum() - 1) < 1e-15
    assert np.isfinite(out["log_likelihoods_dla"][1, :2]).all() and np.isnan(out["log_likelihoods_dla"][1, 2])
    assert np.isfinite(out["log_likelihoods_dla"][2, 0]) and np.isnan(out["log_likelihoods_dla"][2, 1:]).all()
    assert np.isnan(out["sample_log_likelihoods_dla"][2, 2]).all()          # never swept
    assert np.isnan(out["model_posteriors"][1:3]).all() and np.isnan(out["p_dlas"][1:3]).all()
    small = np.sort(out["model_posteriors"][3:].reshape(-1))[:6]
    assert (small > 1e-300).all() and (small < 1e-60).all()
    assert np.isfinite(out["log_posteriors_no_dla"]).all() and np.isfinite(out["log_posteriors_lls"]).all()


def test_bit_identity_at_257_samples():
    """One call, one quasar per resident batch, and a profile table of one quasar's worth: every array identical
    (the larger shapes have this test in test_gpu_configs.py)."""
    S = 257
    p = MultiParameters(max_dlas=3, rng_seed=SEED, first_quasar_index=2 ** 32 + 5)
    spectra, samples = quasars(), samples_of(S)
    lp = priors(spectra, p)
    one = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, lp, params=p)
    per_quasar = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, lp, params=p, max_quasars_per_batch=1)
    stride = ((4 * ((max(s["wavelengths"].size for s in spectra) + 3) // 4) + 4 + 15) // 16) * 16
    p1 = MultiParameters(max_dlas=3, rng_seed=SEED, first_quasar_index=2 ** 32 + 5, multi_profile_bytes=2 * S * stride * 8)
    split = gp.process_qsos_multiple_dlas_meanflux(model(), samples, spectra, lp, params=p1)
    assert set(one) == set(per_quasar) == set(split)
    for key in one:
        np.testing.assert_array_equal(per_quasar[key], one[key], err_msg=f"{key}: one quasar per batch")
        np.testing.assert_array_equal(split[key], one[key], err_msg=f"{key}: one quasar per profile sub-batch")
