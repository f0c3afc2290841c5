"""Learning the model from spectra on the GPU (csrc/learn_kernels.hpp, training.learn_qso_model),
held to the numpy restatement of tests/learn_restatement.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_restatement as R  # noqa: E402

import gp_dla_detection_amd as gp  # noqa: E402
from gp_dla_detection_amd import io, synthetic  # noqa: E402
from gp_dla_detection_amd.api import spectra_to_csr  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters, Parameters  # noqa: E402
from gp_dla_detection_amd.training import TrainingSet, learn_qso_model, rest_grid_size  # noqa: E402

pytestmark = pytest.mark.gpu

SUBSPACE_MIN_COSINE = 0.95  # calibrated in tests/test_learn.py


def mixed_spectra(nq, seed=0, meanflux=False):
    """DR12Q-mix quasars with the awkward cases mixed in: a one-pixel spectrum, a fully masked
    quasar, noise above the cut, z near 2.15 and near 5; even entries unmasked (complete rows)."""
    model = synthetic.make_model(20)
    z = synthetic.sample_dr12q_redshifts(nq + 8, seed=4321 + seed)[:nq]
    out = []
    for i in range(nq):
        zi = 2.1501 if i % 7 == 3 else (4.98 if i % 7 == 5 else float(z[i]))
        s = synthetic.make_boss_spectrum(2 * i + 10000 * seed, zi, model, mask_fraction=0.0 if i % 2 == 0 else 0.05)
        out.append(s)
    if nq > 1:
        out[1] = dict(out[1], wavelengths=out[1]["wavelengths"][:1], flux=out[1]["flux"][:1],
                      noise_variance=out[1]["noise_variance"][:1], pixel_mask=out[1]["pixel_mask"][:1])
    if nq > 2:
        s = out[2]
        out[2] = dict(s, pixel_mask=np.ones_like(s["pixel_mask"]), flux=np.full_like(s["flux"], np.nan))
    cut = 9.0 if meanflux else 1.0
    s = out[-1]
    nv = s["noise_variance"].copy()
    nv[100:140] = 3.0 * cut
    out[-1] = dict(s, noise_variance=nv)
    return out


def restated(csr, p, meanflux):
    return R.rest_grid(csr, rest_grid_size(p), p.min_lambda, p.dlambda, p.lya_wavelength, p.max_noise_variance,
                       31 if meanflux else 0, 0.0023, 3.65)


def assert_close_nan(a, b, rtol):
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN patterns differ"
    assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), "+-inf differ"
    fin = np.isfinite(b)
    err = np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300)
    assert err.max(initial=0.0) <= rtol, err.max()


@pytest.mark.parametrize("meanflux", [False, True])
@pytest.mark.parametrize("nq", [1, 17, 400])
def test_rest_grid_and_stats_match_the_restatement(nq, meanflux):
    p = MultiParameters() if meanflux else Parameters()
    csr = spectra_to_csr(mixed_spectra(nq, meanflux=meanflux))
    F, L, N = restated(csr, p, meanflux)
    t = TrainingSet.from_spectra(csr, p, meanflux)
    try:
        f, l, n = t.download()
        tol = 1e-12 if meanflux else 1e-13
        assert_close_nan(f, F, tol)
        assert_close_nan(l, L, 1e-13)
        assert_close_nan(n, N, tol)
        mu, std, count = t.column_stats()
        rmu, centered, rstd, rcount = R.column_stats(F)
        assert np.array_equal(count, rcount)
        assert_close_nan(mu, rmu, 1e-12)
        assert_close_nan(std, rstd, 1e-12)
        fc, _, _ = t.download()
        # centred values cancel: held to the flux scale, not to themselves
        assert np.array_equal(np.isnan(fc), np.isnan(centered))
        fin = np.isfinite(centered)
        if fin.any():
            assert np.abs(fc[fin] - centered[fin]).max() <= 1e-12 * np.abs(F[fin]).max()
    finally:
        t.close()


@pytest.fixture(scope="module")
def big_set():
    return spectra_to_csr(mixed_spectra(4997, seed=1))


@pytest.mark.parametrize("G", [16, 17, 1217])
@pytest.mark.parametrize("nq", [17, 4997])
def test_covariance_matches_the_restatement(nq, G, big_set):
    p = Parameters(min_lambda=1100.0, max_lambda=1100.0 + 0.25 * (G - 1)) if G < 1217 else Parameters()
    if nq == 4997:
        csr = big_set
    else:
        csr = spectra_to_csr(mixed_spectra(nq, seed=2))
    F, _, _ = restated(csr, p, False)
    _, centered, _, _ = R.column_stats(F)
    t = TrainingSet.from_spectra(csr, p)
    try:
        t.column_stats()
        for complete in (False, True):
            rcov, rN, rrows = R.pca_covariance(centered, complete)
            cov, N, rows = t.pca_covariance(complete, with_count=True)
            assert rows == rrows
            assert np.array_equal(cov, cov.T, equal_nan=True)
            assert np.array_equal(N, rN)
            assert np.array_equal(np.isnan(cov), np.isnan(rcov))
            assert np.array_equal(np.isposinf(cov), np.isposinf(rcov)) and np.array_equal(np.isneginf(cov), np.isneginf(rcov))
            fin = np.isfinite(rcov)
            if fin.any():  # (one complete row of 17 at G = 1217: 0 / 0 everywhere)
                assert np.abs(cov[fin] - rcov[fin]).max() <= 1e-11 * np.abs(rcov[fin]).max()
    finally:
        t.close()


def test_two_handles_are_bit_identical(big_set):
    outs = []
    for _ in range(2):
        t = TrainingSet.from_spectra(big_set)
        try:
            raw = t.download()
            stats = t.column_stats()
            cov = t.pca_covariance(False)[0], t.pca_covariance(True)[0]
            outs.append((raw, stats, cov))
        finally:
            t.close()
    (r0, s0, c0), (r1, s1, c1) = outs
    for a, b in zip(r0 + s0 + c0, r1 + s1 + c1):
        assert np.array_equal(a, b, equal_nan=True)


def e2e_training_spectra(meanflux, num=300):
    if not meanflux:  # the subspace threshold is calibrated on 1000 quasars
        spectra, gen = R.dla_free_training_set(1000, first_index=20000)
        return spectra, gen
    # 'rows','complete' needs quasars that cover the whole rest range unmasked: z > 2.95, no mask
    gen = synthetic.make_model(20)
    z = np.linspace(3.0, 4.2, num)
    return [synthetic.make_boss_spectrum(20000 + 2 * i, float(z[i]), gen, mask_fraction=0.0) for i in range(num)], gen


@pytest.mark.parametrize("meanflux", [False, True])
def test_learn_qso_model_end_to_end(meanflux, tmp_path):
    p = MultiParameters() if meanflux else Parameters()
    spectra, gen = e2e_training_spectra(meanflux)
    csr = spectra_to_csr(spectra)
    model = learn_qso_model(csr, p, meanflux=meanflux, max_iter=3, max_fun_evals=20)
    # initial_x: the restatement's assembly on the GPU's own covariance, bit for bit
    t = TrainingSet.from_spectra(csr, p, meanflux)
    try:
        _, std, _ = t.column_stats()
        cov, _, _ = t.pca_covariance(meanflux)
    finally:
        t.close()
    M0, latent = R.pca_init(cov, 20)
    assert np.array_equal(model["initial_x"], R.initial_x(M0, std))
    F, _, _ = restated(csr, p, meanflux)
    _, centered, _, _ = R.column_stats(F)
    _, rlatent = R.pca_init(R.pca_covariance(centered, meanflux)[0], 20)
    np.testing.assert_allclose(model["latent"][:20], rlatent[:20], rtol=1e-10)
    res = model["fit"]
    assert res.nit >= 1 and res.fun < res.trace_fval[0]
    if not meanflux:
        cos = R.principal_cosines(model["initial_M"][:, :3], gen["M"][:, :3])
        assert cos.min() > SUBSPACE_MIN_COSINE, cos
    path = str(tmp_path / "learned_qso_model_e2e.mat")
    io.save_learned_model(path, model, training_release="synthetic", train_ind=np.ones(len(spectra), bool))
    loaded = io.load_learned_model(path)
    mem = {k: model[k] for k in loaded}
    for k in loaded:
        assert np.array_equal(loaded[k], mem[k]), k
    held = [synthetic.make_boss_spectrum(2 * i + 1, z, gen) for i, z in enumerate((2.4, 3.1, 3.6))]
    samples = synthetic.make_samples(512)
    if meanflux:
        from gp_dla_detection_amd import api
        cat = synthetic.make_prior_catalog()
        zq = np.array([s["z_qso"] for s in held])
        lp = api.dla_existence_prior_multi(cat["z_qsos"], cat["dla_ind"], zq, 0.31, 0.69, p)
        run = lambda m: gp.process_qsos_multiple_dlas_meanflux(m, samples, held, lp, params=p)
        key = "log_likelihoods_dla"
    else:
        cat = synthetic.make_prior_catalog()
        run = lambda m: gp.process_qsos(m, samples, held, prior_catalog=cat)
        key = "log_likelihoods_dla"
    a, b = run(loaded), run(mem)
    assert np.all(np.isfinite(a[key])) and np.all(np.isfinite(a["log_likelihoods_no_dla"]))
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
