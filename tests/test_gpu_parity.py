"""Parity of the HIP path (through the C-ABI) against the CPU oracle and the golden fixtures.

Tolerance (BASELINE.json north_star): fp64, |delta| <= 1e-8 absolute on every log-likelihood /
log-evidence; absorption profiles <= 2e-13 absolute (the reference's own scipy-vs-mpmath spread).
Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.fixture(scope="module")
def model20():
    return synthetic.make_model(20)


def flat_priors(n):
    return np.full(n, np.log(0.9)), np.full(n, np.log(0.1))


# ---------------------------------------------------------------- voigt (voigt.c:253-304)

def test_voigt_golden_profiles(golden):
    g = golden("voigt_profiles.npz")
    for c in range(int(g["num_cases"])):
        z, N, nl = g[f"args_{c}"]
        prof = gp.voigt(g[f"lambdas_{c}"], z, N, int(nl))
        assert prof.shape == (g[f"lambdas_{c}"].size - 6,)
        assert np.abs(prof - g[f"profile_{c}"]).max() < 2e-13, c


def test_voigt_matches_oracle_on_irregular_grids(oracle):
    rng = np.random.default_rng(11)
    for trial in range(6):
        n = int(rng.integers(7, 900))
        lam = np.sort(rng.uniform(3600.0, 9000.0, n))  # not log-uniform, arbitrary length
        z = float(rng.uniform(2.0, 5.0))
        N = 10.0 ** float(rng.uniform(17.0, 23.0))
        nl = int(rng.choice([1, 2, 3, 7, 31]))
        got = gp.voigt(lam, z, N, nl)
        want = oracle.voigt(lam, z, N, nl)
        assert np.abs(got - want).max() < 2e-13, (trial, n, nl)


def test_voigt_default_num_lines_is_31(oracle):
    lam = 10.0 ** (3.6 + 1e-4 * np.arange(300))
    np.testing.assert_allclose(gp.voigt(lam, 2.4, 1e21), oracle.voigt(lam, 2.4, 1e21, 31),
                               rtol=0, atol=2e-13)


def test_voigt_bad_arguments():
    with pytest.raises(_lib.GpdlaError):
        gp.voigt(np.linspace(4000, 4001, 6), 2.0, 1e20, 3)
    with pytest.raises(_lib.GpdlaError):
        gp.voigt(np.linspace(4000, 4100, 60), 2.0, 1e20, 0)
    with pytest.raises(_lib.GpdlaError):
        gp.voigt(np.linspace(4000, 4100, 60), 2.0, 1e20, 32)


# ------------------------------------------------ log_mvnpdf_low_rank (log_mvnpdf_low_rank.m)

def test_log_mvnpdf_golden(golden):
    g = golden("log_mvnpdf_low_rank.npz")
    for c in range(int(g["num_cases"])):
        lp = gp.log_mvnpdf_low_rank(g[f"y_{c}"], g[f"mu_{c}"], g[f"M_{c}"], g[f"d_{c}"])
        assert abs(lp - float(g[f"log_p_{c}"])) < TOL, c


def test_log_mvnpdf_against_exact_arithmetic(golden):
    """HIP log_mvnpdf_low_rank within 1e-9 of the 50-digit value at the same fp64 inputs
    (tests/golden/make_exact.py): five random cases up to (n, k) = (1500, 40), and the null
    model + 32 absorbed samples of the config-1 quasar."""
    from test_oracle_lowrank import exact_case_inputs
    g, e = golden("log_mvnpdf_low_rank.npz"), golden("exact_log_mvnpdf.npz")
    for c in range(int(e["num_cases"])):
        lp = gp.log_mvnpdf_low_rank(g[f"y_{c}"], g[f"mu_{c}"], g[f"M_{c}"], g[f"d_{c}"])
        assert abs(lp - float(e[f"log_p_exact_{c}"])) < 1e-9, c
    worst = 0.0
    for tag, y, mu, M, d, exact in exact_case_inputs(golden):
        worst = max(worst, abs(gp.log_mvnpdf_low_rank(y, mu, M, d) - exact))
    assert worst < 1e-9, worst


def test_sweep_against_exact_arithmetic(golden, model20):
    """The fused sweep kernel (its own Voigt tiers, weights, MFMA contraction, Cholesky) against
    the 50-digit log-likelihoods of the same 32 samples + the null model.  The exact values were
    formed from the oracle's absorption vectors; the kernel's own profile differs from those by
    <= 2e-13, which moves a log-likelihood by up to a few 1e-10, hence 1e-8 here (the tolerance
    of BASELINE.json) rather than the 1e-9 of the pure low-rank check above."""
    g, e = golden("spectrum_config1.npz"), golden("exact_log_mvnpdf.npz")
    samples = synthetic.make_samples(1000)
    sp = dict(wavelengths=g["wavelengths"], flux=g["flux"], noise_variance=g["noise_variance"],
              pixel_mask=g["pixel_mask"], z_qso=float(g["z_qso"]))
    out = run_gpu(model20, samples, [sp])
    assert abs(out["log_likelihoods_no_dla"][0] - float(e["null_log_p_exact"])) < 1e-9
    d = np.abs(out["sample_log_likelihoods_dla"][0][e["sample_indices"]] - e["sample_log_p_exact"])
    print(f"sweep vs 50-digit exact: max |delta| = {d.max():.3e}")
    assert d.max() < TOL, d.max()


def test_log_mvnpdf_ranks_beyond_the_sweep_limit(oracle):
    """The MATLAB function takes any k; the stand-alone surface accepts k <= 256 (only the batch
    sweep is limited to GPDLA_MAX_K = 40)."""
    rng = np.random.default_rng(21)
    for n, k in ((300, 64), (500, 129), (260, 256)):
        M = rng.standard_normal((n, k)) * 0.2
        mu = rng.standard_normal(n)
        d = 10.0 ** rng.uniform(-2, 0, n)
        y = mu + M @ rng.standard_normal(k) + np.sqrt(d) * rng.standard_normal(n)
        want, rc = oracle.log_mvnpdf_low_rank(y, mu, M, d)
        assert rc == 0
        assert abs(gp.log_mvnpdf_low_rank(y, mu, M, d) - want) < 1e-9 * max(1.0, abs(want)), (n, k)
    with pytest.raises(_lib.GpdlaError) as e:
        gp.log_mvnpdf_low_rank(np.zeros(4), np.zeros(4), np.zeros((4, 257)), np.ones(4))
    assert e.value.code == -5


def test_log_mvnpdf_not_positive_definite():
    n, k = 6, 2
    with pytest.raises(_lib.GpdlaError) as e:
        gp.log_mvnpdf_low_rank(np.zeros(n), np.zeros(n), np.ones((n, k)), np.full(n, -0.5))
    assert e.value.code == -4


# ---------------------------------------------------------- process_qsos (process_qsos.m)

def run_gpu(model, samples, spectra):
    lp = flat_priors(len(spectra))
    return gp.process_qsos(model, samples, spectra, log_priors=lp)


def run_oracle(oracle, model, samples, sp):
    return oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"],
                                   sp["wavelengths"], sp["flux"], sp["noise_variance"],
                                   sp["pixel_mask"], sp["z_qso"], num_threads=0)


def test_config1_golden_spectrum(golden, model20):
    """BASELINE config 1: n = 800, k = 20, S = 1000, 5 % masked (NaN flux / inf variance there)."""
    g = golden("spectrum_config1.npz")
    samples = synthetic.make_samples(1000)
    sp = dict(wavelengths=g["wavelengths"], flux=g["flux"], noise_variance=g["noise_variance"],
              pixel_mask=g["pixel_mask"], z_qso=float(g["z_qso"]))
    out = run_gpu(model20, samples, [sp])
    assert out["status"][0] == 0
    assert abs(out["min_z_dlas"][0] - float(g["min_z_dla"])) < 1e-14
    assert abs(out["max_z_dlas"][0] - float(g["max_z_dla"])) < 1e-14
    assert abs(out["log_likelihoods_no_dla"][0] - float(g["log_likelihood_no_dla"])) < TOL
    d = np.abs(out["sample_log_likelihoods_dla"][0] - g["sample_log_likelihoods_dla"])
    assert d.max() < TOL, (d.max(), int(d.argmax()))
    assert abs(out["log_likelihoods_dla"][0] - float(g["log_likelihood_dla"])) < TOL


def test_ragged_batch_vs_oracle(oracle, model20):
    """Several quasars of different lengths, with and without masks, one launch."""
    samples = synthetic.make_samples(200)
    sizes = [203, 400, 777, 1001, 64, 1250]
    spectra = [synthetic.make_spectrum(10 + i, n, model20, mask_fraction=0.05 if i % 2 else 0.0)
               for i, n in enumerate(sizes)]
    out = run_gpu(model20, samples, spectra)
    lp_no, lp_dla = flat_priors(len(spectra))
    for i, sp in enumerate(spectra):
        ref = run_oracle(oracle, model20, samples, sp)
        assert out["status"][i] == 0
        assert abs(out["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]) < TOL, i
        d = np.abs(out["sample_log_likelihoods_dla"][i] - ref["sample_log_likelihoods_dla"])
        assert d.max() < TOL, (i, d.max())
        assert abs(out["log_likelihoods_dla"][i] - ref["log_likelihood_dla"]) < TOL, i
        # process_qsos.m:153-154, 212-213, 224-233
        post = np.array([lp_no[i] + ref["log_likelihood_no_dla"], lp_dla[i] + ref["log_likelihood_dla"]])
        assert abs(out["log_posteriors_no_dla"][i] - post[0]) < TOL
        assert abs(out["log_posteriors_dla"][i] - post[1]) < TOL
        mp = np.exp(post - post.max())
        mp /= mp.sum()
        np.testing.assert_allclose(out["model_posteriors"][i], mp, rtol=0, atol=1e-9)
        assert abs(out["p_no_dlas"][i] - mp[0]) < 1e-9 and abs(out["p_dlas"][i] - (1 - mp[0])) < 1e-9


def test_empty_and_fully_masked_spectra_stay_nan(oracle, model20):
    samples = synthetic.make_samples(48)
    good = synthetic.make_spectrum(30, 300, model20)
    red = dict(wavelengths=np.linspace(9000, 9100, 50), flux=np.ones(50),
               noise_variance=np.ones(50), pixel_mask=np.zeros(50, np.uint8), z_qso=2.5)
    masked = synthetic.make_spectrum(31, 250, model20)
    masked["pixel_mask"] = np.ones_like(masked["pixel_mask"])
    out = run_gpu(model20, samples, [red, good, masked])
    assert list(out["status"]) == [1, 0, 1]
    for i in (0, 2):  # the reference leaves its NaN pre-fill in place (process_qsos.m:74-82)
        assert np.isnan(out["sample_log_likelihoods_dla"][i]).all()
        assert np.isnan(out["log_likelihoods_no_dla"][i]) and np.isnan(out["log_likelihoods_dla"][i])
        assert np.isnan(out["model_posteriors"][i]).all()
    ref = run_oracle(oracle, model20, samples, good)
    assert np.abs(out["sample_log_likelihoods_dla"][1] - ref["sample_log_likelihoods_dla"]).max() < TOL


def test_unsorted_wavelengths(oracle, model20):
    """The reference never assumes ascending wavelengths; neither may the selection scan."""
    samples = synthetic.make_samples(32)
    sp = synthetic.make_spectrum(40, 300, model20, mask_fraction=0.05)
    order = np.random.default_rng(1).permutation(sp["wavelengths"].size)
    for key in ("wavelengths", "flux", "noise_variance", "pixel_mask"):
        sp[key] = sp[key][order]
    ref = run_oracle(oracle, model20, samples, sp)
    out = run_gpu(model20, samples, [sp])
    assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL


def test_num_lines_31_and_1(oracle, model20):
    samples = synthetic.make_samples(40)
    sp = synthetic.make_spectrum(41, 350, model20)
    for nl in (1, 31):
        p = gp.Parameters(num_lines=nl)
        out = gp.process_qsos(model20, samples, [sp], log_priors=flat_priors(1), params=p)
        from oracle.oracle import OracleParams
        ref = oracle.process_spectrum(model20, samples["offset_samples"], samples["nhi_samples"],
                                      sp["wavelengths"], sp["flux"], sp["noise_variance"],
                                      sp["pixel_mask"], sp["z_qso"], params=OracleParams(num_lines=nl))
        assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL, nl


def test_rank_40_model(oracle):
    """BASELINE config 5's shape (k = 40) in fp64: the tile-split sweep."""
    model = synthetic.make_model(40)
    samples = synthetic.make_samples(50)
    sp = synthetic.make_spectrum(50, 420, model, mask_fraction=0.05)
    out = run_gpu(model, samples, [sp])
    ref = run_oracle(oracle, model, samples, sp)
    assert abs(out["log_likelihoods_no_dla"][0] - ref["log_likelihood_no_dla"]) < TOL
    assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL


@pytest.mark.parametrize("k", [21, 24, 25, 27, 33, 39])
def test_ranks_between_the_tile_classes(oracle, k):
    """20 < k < 40 runs on the k <= 40 kernel with zero-padded tiles: 21 is the first rank past the
    one-wave class, 27 and 33 leave different numbers of the 52 + 4 tiles (partly) empty.  The
    epilogue deals rows 0..8 / 9..24 / 25..40 to three register slots (factor_rows16): at k = 24 the
    last row (v) is the last of the second slot, at k = 25 the first of the third."""
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(40)
    sp = synthetic.make_spectrum(52 + k, 333, model, mask_fraction=0.03)
    out = run_gpu(model, samples, [sp])
    ref = run_oracle(oracle, model, samples, sp)
    assert abs(out["log_likelihoods_no_dla"][0] - ref["log_likelihood_no_dla"]) < TOL
    assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL


@pytest.mark.parametrize("k", [16, 17, 19])
def test_ranks_around_the_off_mfma_columns(oracle, k):
    """k <= 20 keeps vech columns 208, 209 and projection columns 16..19 on the VALU: k = 16 uses
    none of them, 17 and 19 some of the projection columns only, 20 (everywhere else) all six."""
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(48)
    sp = synthetic.make_spectrum(90 + k, 287, model, mask_fraction=0.03)
    out = run_gpu(model, samples, [sp])
    ref = run_oracle(oracle, model, samples, sp)
    assert abs(out["log_likelihoods_no_dla"][0] - ref["log_likelihood_no_dla"]) < TOL
    assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL


def test_small_rank_model(oracle):
    model = synthetic.make_model(5)
    samples = synthetic.make_samples(20)
    sp = synthetic.make_spectrum(51, 210, model)
    out = run_gpu(model, samples, [sp])
    ref = run_oracle(oracle, model, samples, sp)
    assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL


# -------------------------------------------------- BASELINE config 2 sizes, by properties

def test_full_size_properties(oracle, model20):
    """n = 1500, S = 10000 (BASELINE config 2's per-quasar shape) on 3 quasars: the oracle checks a
    random subset of samples; size-independent properties cover the rest."""
    S = 10000
    samples = synthetic.make_samples(S)
    spectra = synthetic.make_spectra(3, 1500, model20, first_index=100)
    out = run_gpu(model20, samples, spectra)
    sll = out["sample_log_likelihoods_dla"]
    assert sll.shape == (3, S) and np.isfinite(sll).all()
    # (a) evidence is the log-mean-exp of the sample table (process_qsos.m:203-210)
    mx = sll.max(axis=1)
    ev = mx + np.log(np.mean(np.exp(sll - mx[:, None]), axis=1))
    np.testing.assert_allclose(out["log_likelihoods_dla"], ev, rtol=0, atol=TOL)
    # (b) oracle on a random subset of the samples (the oracle takes any sample list)
    rng = np.random.default_rng(0)
    pick = np.sort(rng.choice(S, 48, replace=False))
    sub = dict(offset_samples=samples["offset_samples"][pick], nhi_samples=samples["nhi_samples"][pick])
    for i, sp in enumerate(spectra):
        ref = run_oracle(oracle, model20, sub, sp)
        assert abs(out["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]) < TOL
        d = np.abs(sll[i, pick] - ref["sample_log_likelihoods_dla"])
        assert d.max() < TOL, (i, d.max())
    # (c) the result of a sample does not depend on which other samples share its launch:
    #     permute the sample list and compare entry by entry (bit-exact)
    perm = rng.permutation(S)
    shuffled = {k: v[perm] for k, v in samples.items()}
    out2 = run_gpu(model20, shuffled, spectra[:1])
    np.testing.assert_array_equal(out2["sample_log_likelihoods_dla"][0], sll[0, perm])
    # (d) a quasar with an injected DLA prefers the DLA model and recovers its redshift
    for i, sp in enumerate(spectra):
        if sp["true_z_dla"] is not None and sp["true_log_nhi"] > 20.5:
            zs = out["min_z_dlas"][i] + (out["max_z_dlas"][i] - out["min_z_dlas"][i]) * samples["offset_samples"]
            assert abs(zs[sll[i].argmax()] - sp["true_z_dla"]) < 5e-3
            assert out["log_likelihoods_dla"][i] > out["log_likelihoods_no_dla"][i]


def test_resident_batch_is_idempotent(model20):
    """Processing the same resident batch twice gives bit-identical tables (no stale state)."""
    samples = synthetic.make_samples(500)
    spectra = synthetic.make_spectra(4, 600, model20, first_index=200)
    ctx = gp.Context(0)
    ctx.set_model(model20)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra, *flat_priors(4))
    batch.process()
    a = batch.download()
    batch.process()
    b = batch.download()
    for key in ("sample_log_likelihoods_dla", "log_likelihoods_dla", "model_posteriors"):
        np.testing.assert_array_equal(a[key], b[key])
    t = batch.summary_tensor()
    assert tuple(t.shape) == (4, 15) and t.is_cuda
    np.testing.assert_array_equal(t.cpu().numpy()[:, 5], a["log_likelihoods_dla"])
    np.testing.assert_array_equal(t.cpu().numpy()[:, 12], a["MAP_inds"])
    batch.close()
    ctx.close()


def test_map_columns_of_the_evidence_kernel(model20):
    """generate_ascii_catalog.m:73-80 on the GPU: [~, map_ind] = nanmax(sample_log_likelihoods_dla(i, :)),
    map_z_dla from the quasar's own search range, log_nhi_samples(map_ind) -- found by k_evidence
    while it walks the table, compared with the host recomputation (catalog.map_estimates)."""
    from gp_dla_detection_amd import catalog
    samples = synthetic.make_samples(3000)
    spectra = synthetic.make_spectra(5, 420, model20, mask_fraction=0.03, first_index=480)
    red = dict(wavelengths=np.linspace(9000, 9100, 50), flux=np.ones(50),
               noise_variance=np.ones(50), pixel_mask=np.zeros(50, np.uint8), z_qso=2.5)
    spectra.insert(2, red)  # an empty quasar: its MAP columns stay NaN
    out = run_gpu(model20, samples, spectra)
    z, lognhi, ind = catalog.map_estimates_host(out, samples)
    ok = out["status"] == 0
    np.testing.assert_array_equal(out["MAP_inds"][ok], ind[ok] + 1.0)   # 1-based like MATLAB
    np.testing.assert_array_equal(out["MAP_z_dlas"][ok], z[ok])
    np.testing.assert_array_equal(out["MAP_log_nhis"][ok], lognhi[ok])
    assert np.isnan(out["MAP_inds"][2]) and np.isnan(out["MAP_z_dlas"][2])
    # without log_nhi_samples the column is log10(nhi_samples(map_ind))
    bare = {k: samples[k] for k in ("offset_samples", "nhi_samples")}
    out2 = run_gpu(model20, bare, spectra[:1])
    assert abs(out2["MAP_log_nhis"][0] - lognhi[0]) < 1e-12
    # ties: the FIRST index wins (MATLAB's max): duplicate the sample list
    dup = {k: np.concatenate([v, v]) for k, v in samples.items()}
    out3 = run_gpu(model20, dup, spectra[:1])
    assert out3["MAP_inds"][0] == out["MAP_inds"][0]


def test_fp32_contraction_study_variant_vs_oracle(oracle, model20):
    """BASELINE config 5: contraction on the fp32 matrix cores, the rest in fp64.  Not parity-grade:
    its distance from the ORACLE is bounded at k = 20 here (the k = 40 form: test_gpu_configs.py)."""
    samples = synthetic.make_samples(96)
    sp = synthetic.make_spectrum(300, 500, model20)
    got = gp.process_qsos(model20, samples, [sp], log_priors=flat_priors(1),
                          params=gp.Parameters(contraction_precision=1))
    ref = run_oracle(oracle, model20, samples, sp)
    d = np.abs(got["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"])
    assert np.isfinite(got["sample_log_likelihoods_dla"]).all()
    assert d.max() < 0.5, d.max()   # fp32 accumulation over n pixels: ~1e-2 nat on values of 10^3
    assert got["min_z_dlas"][0] == ref["min_z_dla"]


def test_tiny_and_odd_shapes(oracle, model20):
    """Edge shapes: fewer pixels than one K-step, pixel counts not divisible by 4, and sample
    counts around the 16-slot wave / 128-slot block boundaries (1, 15, 16, 17, 127, 128, 129)."""
    for n in (1, 3, 5, 9):
        samples = synthetic.make_samples(7)
        sp = synthetic.make_spectrum(400 + n, n, model20, edge_pixels=1)
        out = run_gpu(model20, samples, [sp])
        ref = run_oracle(oracle, model20, samples, sp)
        assert out["status"][0] == 0
        assert abs(out["log_likelihoods_no_dla"][0] - ref["log_likelihood_no_dla"]) < TOL, n
        assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL, n
    sp = synthetic.make_spectrum(450, 222, model20, mask_fraction=0.05)
    for S in (1, 15, 16, 17, 127, 128, 129):
        samples = synthetic.make_samples(S)
        out = run_gpu(model20, samples, [sp])
        ref = run_oracle(oracle, model20, samples, sp)
        assert out["sample_log_likelihoods_dla"].shape == (1, S)
        assert np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]).max() < TOL, S
        assert abs(out["log_likelihoods_dla"][0] - ref["log_likelihood_dla"]) < TOL, S


def test_bad_pixels_in_kept_data_propagate_like_the_reference(oracle, model20):
    """A NaN flux in an UNMASKED pixel poisons that quasar only (NaN log-likelihoods, as MATLAB
    arithmetic would give), not its neighbours in the batch."""
    samples = synthetic.make_samples(24)
    a = synthetic.make_spectrum(460, 210, model20)
    b = synthetic.make_spectrum(461, 230, model20)
    a["flux"] = a["flux"].copy()
    a["flux"][100] = np.nan
    out = run_gpu(model20, samples, [a, b])
    assert np.isnan(out["sample_log_likelihoods_dla"][0]).all() and np.isnan(out["log_likelihoods_no_dla"][0])
    ref = run_oracle(oracle, model20, samples, b)
    assert np.abs(out["sample_log_likelihoods_dla"][1] - ref["sample_log_likelihoods_dla"]).max() < TOL


def test_chunked_driver_matches_single_batch(model20):
    """process_qsos sweeps a long quasar list in bounded batches through the upload / sweep /
    download pipeline (api.run_pipeline); results are identical whatever the batching and the
    number of batch slots -- ragged sizes, so re-filled slots both reuse and grow their buffers."""
    samples = synthetic.make_samples(64)
    spectra = [synthetic.make_spectrum(470 + i, n, model20, mask_fraction=0.03)
               for i, n in enumerate([260, 120, 410, 90, 333, 505, 64, 280, 199, 620, 75])]
    lp = flat_priors(len(spectra))
    one = gp.process_qsos(model20, samples, spectra, log_priors=lp, max_quasars_per_batch=len(spectra))
    for per_batch, slots in ((3, 3), (2, 2), (1, 1), (4, 2), (5, 3)):
        many = gp.process_qsos(model20, samples, spectra, log_priors=lp, max_quasars_per_batch=per_batch,
                               pipeline_slots=slots)
        for key in one:
            np.testing.assert_array_equal(one[key], many[key], err_msg=f"{key} {per_batch} {slots}")
    default = gp.process_qsos(model20, samples, spectra, log_priors=lp)
    np.testing.assert_array_equal(one["sample_log_likelihoods_dla"], default["sample_log_likelihoods_dla"])


def test_one_shot_pipeline_many_small_blocks(model20):
    """The library's three host stages over 150 one-quasar blocks and over blocks of 7 through 2 slots
    (every hand-off between the upload thread, the caller's thread and the download thread, a few
    hundred times): bit-equal to one batch, nothing lost or duplicated; and a block that fails in the
    middle (a model with more columns than the uploaded priors allow cannot be provoked here, so: an
    out-of-range replayed index of the multi-DLA driver) stops all three stages with the library's
    message."""
    samples = synthetic.make_samples(16)
    rng = np.random.default_rng(11)
    spectra = [synthetic.make_spectrum(1200 + i, int(rng.integers(20, 90)), model20, mask_fraction=0.02) for i in range(150)]
    lp = flat_priors(len(spectra))
    one = gp.process_qsos(model20, samples, spectra, log_priors=lp, max_quasars_per_batch=len(spectra))
    for per_batch, slots in ((1, 3), (7, 2), (1, 1)):
        many = gp.process_qsos(model20, samples, spectra, log_priors=lp, max_quasars_per_batch=per_batch, pipeline_slots=slots)
        for key in one:
            np.testing.assert_array_equal(one[key], many[key], err_msg=f"{key} {per_batch} {slots}")
    from gp_dla_detection_amd.parameters import MultiParameters
    p = MultiParameters(max_dlas=2)
    msamples = synthetic.make_samples(16)
    few = spectra[:12]
    z = np.array([s["z_qso"] for s in few])
    cat = synthetic.make_prior_catalog()
    mlp = gp.dla_existence_prior_multi(cat["z_qsos"], cat["dla_ind"], z, 0.3, 0.7, p)
    base = np.ones((12, 1, 16), dtype=np.uint32)
    base[7, 0, 3] = 99  # > S: rejected when block 7 is launched, after blocks 0..6 went through
    with pytest.raises(Exception) as err:
        gp.process_qsos_multiple_dlas_meanflux(model20, msamples, few, mlp, params=p, base_sample_inds=base,
                                               max_quasars_per_batch=1, pipeline_slots=3)
    assert "exceeds num_dla_samples" in str(err.value)


def test_cell_and_csr_entries_agree(model20):
    """gpdla_process_cells (one array per quasar, flattened block by block inside the library) and
    gpdla_process_batch (CSR arrays) are the same loop: bit-equal results, whatever the batching;
    non-contiguous / non-float64 cells and boolean masks are accepted."""
    samples = synthetic.make_samples(48)
    spectra = [synthetic.make_spectrum(900 + i, n, model20, mask_fraction=0.04)
               for i, n in enumerate([130, 77, 412, 50, 256, 9, 333])]
    spectra[3] = dict(wavelengths=np.zeros(0), flux=np.zeros(0), noise_variance=np.zeros(0),
                      pixel_mask=np.zeros(0, dtype=bool), z_qso=2.5)             # an empty cell stays NaN
    spectra[1] = dict(spectra[1], flux=np.asarray(spectra[1]["flux"], dtype=np.float32).astype(np.float64)[::1],
                      pixel_mask=np.asarray(spectra[1]["pixel_mask"]).astype(bool))
    spectra[4] = dict(spectra[4], wavelengths=np.repeat(spectra[4]["wavelengths"], 2)[::2])  # a strided view
    lp = flat_priors(len(spectra))
    from gp_dla_detection_amd import api
    csr = api.spectra_to_csr(spectra)
    want = gp.process_qsos(model20, samples, csr, log_priors=lp)
    for per_batch, slots in ((None, 3), (2, 2), (3, 1)):
        got = gp.process_qsos(model20, samples, spectra, log_priors=lp, max_quasars_per_batch=per_batch, pipeline_slots=slots)
        for key in want:
            np.testing.assert_array_equal(want[key], got[key], err_msg=f"{key} {per_batch} {slots}")
    assert np.isnan(want["log_likelihoods_dla"][3]) and want["status"][3] == 1


def test_record_pool_groups_do_not_change_results(model20):
    """A batch whose K-step records exceed Parameters.record_pool_bytes is swept group by group
    through one pool (records built, swept, next group): identical results for every record class
    -- slim (k <= 20, 3 lines), pre-expanded (5 lines; fp32 study), and the k <= 40 tile split."""
    samples = synthetic.make_samples(48)
    for k, extra in ((20, {}), (20, dict(num_lines=5)), (20, dict(contraction_precision=1)), (33, {})):
        model = model20 if k == 20 else synthetic.make_model(k)
        spectra = [synthetic.make_spectrum(700 + i, n, model, mask_fraction=0.02)
                   for i, n in enumerate([300, 90, 410, 150, 222, 505, 64])]
        lp = flat_priors(len(spectra))
        one = gp.process_qsos(model, samples, spectra, log_priors=lp, params=gp.Parameters(**extra),
                              max_quasars_per_batch=len(spectra))
        # 505 pixels = 128 K-step records; a pool of 150 records holds one or two quasars at a time
        per_step = 896 if (k == 20 and not extra) else (7680 if k == 20 else 29696)
        many = gp.process_qsos(model, samples, spectra, log_priors=lp, max_quasars_per_batch=len(spectra),
                               params=gp.Parameters(record_pool_bytes=150 * per_step, **extra))
        for key in one:
            np.testing.assert_array_equal(one[key], many[key], err_msg=f"{key} k={k} {extra}")


def test_batch_reload_and_destroy_order(model20):
    """gpdla_batch_reload re-fills a batch in place; a batch may outlive its context (it is
    orphaned, not left with a dangling pointer); using it then is an error, destroying it is not."""
    samples = synthetic.make_samples(48)
    a = synthetic.make_spectra(3, 300, model20, first_index=610)
    b = synthetic.make_spectra(5, 180, model20, first_index=620)
    ctx = gp.Context(0)
    ctx.set_model(model20)
    ctx.set_samples(samples)
    batch = ctx.upload(a, *flat_priors(3))
    batch.process()
    ra = batch.download()
    batch.reload(b, *flat_priors(5))      # more quasars, fewer pixels
    batch.process()
    rb = batch.download()
    batch.reload(a, *flat_priors(3))
    batch.process()
    ra2 = batch.download()
    for key in ra:
        np.testing.assert_array_equal(ra[key], ra2[key], err_msg=key)
    fresh = gp.process_qsos(model20, samples, b, log_priors=flat_priors(5))
    np.testing.assert_array_equal(rb["sample_log_likelihoods_dla"], fresh["sample_log_likelihoods_dla"])
    ctx.close()                           # context first ...
    with pytest.raises(Exception):
        batch.process()
    batch.close()                         # ... batch afterwards: only frees its memory


def test_noise_variance_guards(model20, oracle):
    """A kept pixel of infinite noise variance (a zero inverse variance the mask missed): the
    reference sums log(inf) into the log-determinant (log_mvnpdf_low_rank.m:30), so every
    log-likelihood of that quasar is -inf and the evidences follow (process_qsos.m:203-213) -- the
    oracle does exactly that.  A kept pixel with variance <= 0 or NaN has no defined result in the
    reference; here the quasar is skipped with status 3."""
    samples = synthetic.make_samples(40)
    sp = synthetic.make_spectra(3, 240, model20, first_index=640)
    sp[0]["noise_variance"] = sp[0]["noise_variance"].copy()
    sp[0]["noise_variance"][57] = np.inf
    sp[2]["noise_variance"] = sp[2]["noise_variance"].copy()
    sp[2]["noise_variance"][100] = -1e-3
    out = gp.process_qsos(model20, samples, sp, log_priors=flat_priors(3))
    assert out["status"].tolist() == [0, 0, 3]
    ref = oracle.process_spectrum(model20, samples["offset_samples"], samples["nhi_samples"], sp[0]["wavelengths"],
                                  sp[0]["flux"], sp[0]["noise_variance"], sp[0]["pixel_mask"], sp[0]["z_qso"])
    assert np.all(np.isneginf(ref["sample_log_likelihoods_dla"])) and np.isneginf(ref["log_likelihood_no_dla"])
    assert np.all(np.isneginf(out["sample_log_likelihoods_dla"][0])) and np.isneginf(out["log_likelihoods_no_dla"][0])
    assert np.isnan(out["log_likelihoods_dla"][0]) and np.isnan(ref["log_likelihood_dla"])
    assert out["MAP_inds"][0] == 1
    ok = oracle.process_spectrum(model20, samples["offset_samples"], samples["nhi_samples"], sp[1]["wavelengths"],
                                 sp[1]["flux"], sp[1]["noise_variance"], sp[1]["pixel_mask"], sp[1]["z_qso"])
    assert np.abs(out["sample_log_likelihoods_dla"][1] - ok["sample_log_likelihoods_dla"]).max() < TOL
    assert np.all(np.isnan(out["sample_log_likelihoods_dla"][2])) and np.isnan(out["p_dlas"][2])


HUGE_NV = (1e40, 1e100, 1e160, 1e200, 1e290, 1e300, 1e307)


def huge_variance_batch(model, n=400, first_index=5000):
    """One quasar per (variance, pattern): kept pixels of huge but finite noise variance, alone, in a
    pair 4 apart (the same lane of consecutive K-steps) and in a run of 12, in the middle of the
    Lyman-alpha forest (the middle of the z_DLA range), so that many samples put damping-wing
    absorption on the pixel three K-steps ahead.  Then one quasar with NaN flux on such a pixel."""
    spectra = []
    patterns = ([0], [0, 4], list(range(12)))
    for i, (nv, pat) in enumerate((nv, pat) for nv in HUGE_NV for pat in patterns):
        sp = synthetic.make_spectrum(first_index + i, n, model)
        sp["noise_variance"] = sp["noise_variance"].copy()
        sp["noise_variance"][n // 2 + 2 + np.array(pat)] = nv  # (+2: the pixels before the modelled range)
        spectra.append(sp)
    bad = synthetic.make_spectrum(first_index + len(spectra), n, model)
    bad["noise_variance"] = bad["noise_variance"].copy()
    bad["flux"] = bad["flux"].copy()
    bad["noise_variance"][n // 2 + 2: n // 2 + 6] = 1e300
    bad["flux"][n // 2 + 3] = np.nan
    return spectra, bad


@pytest.mark.parametrize("k,num_lines", [(20, 3), (20, 1), (33, 3)])
def test_huge_finite_noise_variances(oracle, k, num_lines):
    """Kept pixels with noise variances up to 1e307: every log-likelihood matches the oracle at 1e-8
    (k = 20, 3 lines: k_sweep_slim<3>, whose shared wing-tier reciprocal and two-step log-determinant
    product would overflow on them in the K-loop; 1 line: k_sweep_slim<0>; k = 33:
    k_sweep_split_slim).  k_prepare sweeps such a pixel as a neutral row and adds -log(nu)/2 to the
    quasar's result; with NaN flux on it the quasar stays NaN, as the reference gives."""
    from oracle.oracle import OracleParams
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(200)
    spectra, bad = huge_variance_batch(model)
    out = gp.process_qsos(model, samples, spectra + [bad], log_priors=flat_priors(len(spectra) + 1),
                          params=gp.Parameters(num_lines=num_lines))
    assert (out["status"][:-1] == 0).all()
    dev = []
    for i, sp in enumerate(spectra):
        ref = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"],
                                      sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"],
                                      params=OracleParams(num_lines=num_lines))
        assert np.isfinite(ref["sample_log_likelihoods_dla"]).all()
        d = max(float(np.abs(out["sample_log_likelihoods_dla"][i] - ref["sample_log_likelihoods_dla"]).max()),
                abs(out["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]),
                abs(out["log_likelihoods_dla"][i] - ref["log_likelihood_dla"]))
        dev.append(d if d == d else np.inf)
    bad = [f"nu = {HUGE_NV[i // 3]:.0e} on {(1, 2, 12)[i % 3]} pixel(s): {d:.2e}"
           for i, d in enumerate(dev) if not d < TOL]
    assert not bad, "; ".join(bad)  # (every failing case)
    assert np.isnan(out["sample_log_likelihoods_dla"][-1]).all() and np.isnan(out["log_likelihoods_no_dla"][-1])
    print(f"huge noise variances (k = {k}, {num_lines} lines): worst |delta| = {max(dev):.2e}")


def test_huge_finite_noise_variances_multi(oracle):
    """The multi-DLA mean-flux driver (max_dlas = 2: k_sweep_multi_slim) on the same batch."""
    from gp_dla_detection_amd.parameters import MultiParameters
    from test_gpu_multi import compare, oracle_multi, priors
    p = MultiParameters(max_dlas=2)
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(200)
    spectra, bad = huge_variance_batch(model)
    batch = spectra + [bad]
    out = gp.process_qsos_multiple_dlas_meanflux(model, samples, batch, priors(batch, p), params=p)
    assert (out["status"][:-1] == 0).all()
    for i, sp in enumerate(spectra):
        compare(out, i, oracle_multi(oracle, model, samples, sp, out["base_sample_inds"][i], p), p)
    assert np.isnan(out["sample_log_likelihoods_dla"][-1]).all() and np.isnan(out["log_likelihoods_no_dla"][-1])


def test_randomised_shapes_vs_oracle(oracle):
    """Seeded fuzz over the sweep's shape space: rank 1..40 (all three kernel classes), 30..700
    pixels, 1..90 samples, 0..20 % masked, 1 / 3 / 5 lines -- every log-likelihood against the
    oracle at 1e-8."""
    from oracle.oracle import OracleParams
    rng = np.random.default_rng(7)
    worst = 0.0
    for trial in range(24):
        k = int(rng.integers(1, 41))
        n = int(rng.integers(30, 700))
        S = int(rng.integers(1, 90))
        nl = int(rng.choice([3, 3, 1, 5]))
        model = synthetic.make_model(k)
        samples = synthetic.make_samples(S)
        sp = synthetic.make_spectrum(2000 + trial, n, model, mask_fraction=float(rng.uniform(0, 0.2)))
        out = gp.process_qsos(model, samples, [sp], log_priors=flat_priors(1), params=gp.Parameters(num_lines=nl))
        ref = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"],
                                      sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"],
                                      params=OracleParams(num_lines=nl))
        d = max(float(np.nanmax(np.abs(out["sample_log_likelihoods_dla"][0] - ref["sample_log_likelihoods_dla"]))),
                abs(out["log_likelihoods_no_dla"][0] - ref["log_likelihood_no_dla"]),
                abs(out["log_likelihoods_dla"][0] - ref["log_likelihood_dla"]))
        assert d < TOL, (trial, k, n, S, nl, d)
        worst = max(worst, d)
    print(f"fuzz: worst |delta| over 24 random shapes = {worst:.2e}")
