"""CPU checks of learning the model from spectra: the numpy restatement (tests/learn_restatement.py)
on hand-made cases, the new C entry points' argument checks (no GPU needed), the learned-model
writer, and a science check of the restatement's PCA starting point."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_restatement as R  # noqa: E402

from gp_dla_detection_amd import _lib, io, synthetic  # noqa: E402
from gp_dla_detection_amd.training import learn_config  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters, Parameters  # noqa: E402

#: principal cosines of initial_M[:, :3] against the generator's M[:, :3] from 1000 DLA-free quasars:
#: the restatement gives >= 0.984 (its smallest); skipping the centring gives 0.09
SUBSPACE_MIN_COSINE = 0.95


def test_interp1_edges_and_nan_neighbours():
    x = np.array([1.0, 2.0, 4.0])
    v = np.array([10.0, 20.0, np.nan])
    out = R.interp1(x, v, np.array([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 4.5]))
    assert np.isnan(out[0]) and np.isnan(out[-1])          # outside [x_1, x_n]
    assert out[1] == 10.0 and out[2] == 15.0
    assert np.isnan(out[3])   # the bracket of 2.0 is [2, 4] (last x_j <= xq): 20 + 0 * (NaN - 20)
    assert np.isnan(out[4]) and np.isnan(out[5])            # a NaN neighbour
    assert np.all(np.isnan(R.interp1([1.0], [5.0], [1.0])))  # fewer than two pixels
    # the last point uses the clipped bracket n - 2
    assert R.interp1([0.0, 1.0, 2.0], [0.0, 1.0, 4.0], [2.0])[0] == 4.0


def test_noise_mask_removes_all_three():
    wl = 1100.0 * 3.0 + np.arange(8) * 2.0
    csr = dict(offsets=np.array([0, 8]), wavelengths=wl, flux=np.ones(8),
               noise_variance=np.array([0.5, 0.5, 2.0, 2.0, 0.5, 0.5, 0.5, 0.5]),
               pixel_mask=np.zeros(8, np.uint8), z_qsos=np.array([2.0]))
    F, L, N = R.rest_grid(csr, 8, min_lambda=1100.0, dlambda=0.5, max_noise_variance=1.0)
    v = R.interp1(wl / 3.0, csr["noise_variance"], 1100.0 + 0.5 * np.arange(8))
    noisy = v > 1.0
    assert noisy.any() and (np.isfinite(v) & ~noisy).any()
    assert np.array_equal(np.isnan(N[0]), ~(v <= 1.0))
    assert np.array_equal(np.isnan(F), np.isnan(N)) and np.array_equal(np.isnan(L), np.isnan(N))
    # masked pixels: flux and noise NaN, lya_1pzs kept
    csr["pixel_mask"] = np.array([0, 0, 0, 0, 0, 1, 0, 0], np.uint8)
    csr["noise_variance"] = np.full(8, 0.5)
    F, L, N = R.rest_grid(csr, 8, min_lambda=1100.0, dlambda=0.5)
    assert np.isnan(F[0, 6:8]).all() and np.isfinite(F[0, :6]).all() and np.isfinite(L[0, :8]).all()


def test_pairwise_covariance_by_hand():
    X = np.array([[1.0, 2.0, np.nan],
                  [-1.0, np.nan, 1.0],
                  [0.5, -2.0, 2.0],
                  [np.nan, 1.0, -1.0]])
    cov, N, rows = R.pca_covariance(X)
    # (a, b) = sum over quasars finite in both of x_qa x_qb / (N_ab - 1)
    assert N[0, 0] == 3 and N[0, 1] == 2 and N[0, 2] == 2 and N[1, 2] == 2 and rows == 4
    assert cov[0, 0] == (1 + 1 + 0.25) / 2
    assert cov[0, 1] == (2.0 - 1.0) / 1
    assert cov[0, 2] == (-1.0 + 1.0) / 1
    assert cov[1, 2] == (-4.0 - 1.0) / 1
    assert cov[1, 1] == (4 + 4 + 1) / 2 and cov[2, 2] == (1 + 4 + 1) / 2
    assert np.array_equal(cov, cov.T)


def test_complete_rows_centre_by_their_own_mean():
    X = np.array([[1.0, 2.0], [3.0, 6.0], [np.nan, 100.0], [5.0, 4.0]])
    cov, _, rows = R.pca_covariance(X, complete_rows=True)
    assert rows == 3
    Xc = X[[0, 1, 3]] - X[[0, 1, 3]].mean(axis=0)
    np.testing.assert_array_equal(cov, Xc.T @ Xc / 2)
    assert cov[0, 0] == 4.0 and cov[1, 1] == 4.0 and cov[0, 1] == 2.0


def test_sign_convention_largest_element_positive():
    cov = np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, 0.0], [0.0, 0.0, 0.5]])
    M, latent = R.pca_init(cov, 2)
    np.testing.assert_allclose(latent, [3.0, 1.0, 0.5], rtol=1e-14)
    for c in range(2):
        col = M[:, c]
        assert col[np.abs(col).argmax()] > 0
    np.testing.assert_allclose(np.abs(M[:, 0]), np.sqrt(3.0) * np.array([1, 1, 0]) / np.sqrt(2), atol=1e-14)


def _csr_args(nq=3, n=5):
    wl = np.tile(4000.0 + np.arange(n, dtype=np.float64), nq)
    keep = dict(offsets=np.arange(0, nq * n + 1, n, dtype=np.int64), wavelengths=wl, flux=np.ones(nq * n),
                noise=np.ones(nq * n), mask=np.zeros(nq * n, np.uint8), z=np.full(nq, 2.5))
    sp = _lib.Spectra()
    sp.num_quasars = nq
    sp.offsets = keep["offsets"].ctypes.data_as(_lib._i64p)
    sp.wavelengths = keep["wavelengths"].ctypes.data_as(_lib._dp)
    sp.flux = keep["flux"].ctypes.data_as(_lib._dp)
    sp.noise_variance = keep["noise"].ctypes.data_as(_lib._dp)
    sp.pixel_mask = keep["mask"].ctypes.data_as(_lib._u8p)
    sp.z_qsos = keep["z"].ctypes.data_as(_lib._dp)
    return sp, learn_config(Parameters()), keep


def test_create_from_spectra_validates_before_it_touches_the_gpu():
    lib = _lib.load()
    out = C.c_void_p()
    call = lambda sp, cfg: lib.gpdla_training_create_from_spectra(0, C.byref(sp), C.byref(cfg), C.byref(out))
    sp, cfg, keep = _csr_args()
    keep["offsets"][2] = keep["offsets"][1] - 1
    assert call(sp, cfg) == _lib.ERR_INVALID_ARGUMENT
    assert b"non-decreasing" in lib.gpdla_last_error() and b"quasar 1" in lib.gpdla_last_error()
    sp, cfg, keep = _csr_args()
    keep["wavelengths"][7] = keep["wavelengths"][6]
    assert call(sp, cfg) == _lib.ERR_INVALID_ARGUMENT
    assert b"strictly increasing" in lib.gpdla_last_error() and b"quasar 1" in lib.gpdla_last_error()
    sp, cfg, keep = _csr_args()
    cfg.num_rest_pixels = 0
    assert call(sp, cfg) == _lib.ERR_INVALID_ARGUMENT and b"rest grid is empty" in lib.gpdla_last_error()
    sp, cfg, keep = _csr_args()
    cfg.num_forest_lines = 32
    assert call(sp, cfg) == _lib.ERR_INVALID_ARGUMENT and b"num_forest_lines" in lib.gpdla_last_error()
    sp, cfg, keep = _csr_args()
    cfg.dlambda = 0.0
    assert call(sp, cfg) == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_training_create_from_spectra(0, None, C.byref(cfg), C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    # the other new entries refuse a null handle
    assert lib.gpdla_training_column_stats(None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_training_pca_covariance(None, 0, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_training_download(None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_parameters_of_learning():
    p, m = Parameters(), MultiParameters()
    assert (p.max_noise_variance, p.initial_c_0, p.initial_tau_0, p.initial_beta) == (1.0, 0.1, 0.0023, 3.65)
    assert m.max_noise_variance == 9.0
    cfg = learn_config(m, meanflux=True)
    assert cfg.num_rest_pixels == 1217 and cfg.num_forest_lines == 31 and cfg.max_noise_variance == 9.0
    assert learn_config(m, meanflux=False).num_forest_lines == 0


def test_save_learned_model_round_trip(tmp_path):
    model = synthetic.make_model(5)
    model.update(initial_M=model["M"] * 0.5, initial_log_omega=model["log_omega"] - 1, initial_log_c_0=-2.0,
                 initial_tau_0=0.0023, initial_beta=3.65, log_likelihood=-123.5, max_noise_variance=1.0)
    ind = np.arange(30) % 4 == 1
    path = str(tmp_path / "learned_qso_model_test.mat")
    io.save_learned_model(path, model, training_release="dr9", train_ind=ind)
    back = io.load_learned_model(path)
    for k in ("rest_wavelengths", "mu", "M", "log_omega"):
        assert np.array_equal(back[k], model[k]), k
    for k in ("log_c_0", "log_tau_0", "log_beta"):
        assert back[k] == model[k]
    raw = io.loadmat73(path, list(io.LEARNED_MODEL_VARIABLES))
    assert raw["mu"].shape == (1, 1217) and raw["rest_wavelengths"].shape == (1, 1217)
    assert raw["log_omega"].shape == (1, 1217) and raw["initial_log_omega"].shape == (1, 1217)
    assert raw["M"].shape == (1217, 5) and raw["initial_M"].shape == (1217, 5)
    assert raw["train_ind"].dtype == bool and raw["train_ind"].shape == (30, 1)
    assert np.array_equal(raw["train_ind"][:, 0], ind)
    assert raw["training_release"] == "dr9"
    assert float(np.ravel(raw["log_likelihood"])[0]) == -123.5
    with pytest.raises(TypeError):
        io.save_learned_model(path, model, train_ind=np.flatnonzero(ind))


def test_restatement_recovers_the_generating_subspace():
    from gp_dla_detection_amd.api import spectra_to_csr
    spectra, model = R.dla_free_training_set(1000)
    F, _, _ = R.rest_grid(spectra_to_csr(spectra), 1217)
    _, centered, std, count = R.column_stats(F)
    assert count.min() >= 2 and np.all(np.isfinite(std))
    cov, _, _ = R.pca_covariance(centered)
    M, latent = R.pca_init(cov, 20)
    assert np.all(latent[:20] > 0)
    cos = R.principal_cosines(M[:, :3], model["M"][:, :3])
    assert cos.min() > SUBSPACE_MIN_COSINE, cos
