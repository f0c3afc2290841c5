"""A numpy restatement of learning the GP model's starting point (learn_qso_model.m:37-96 and
multi_dlas/learn_qso_model_meanflux.m:43-157), written from the contract in DESIGN.md section 4
("Learning the model from spectra"), independently of csrc/learn_kernels.hpp.  It is the yardstick
the GPU is held to by tests/test_gpu_learn.py; tests/test_learn.py checks it on hand-made cases."""
import numpy as np

from gp_dla_detection_amd._lyman_data import LINES

LYA_OSCILLATOR_STRENGTH = 0.416400  # set_parameters_multi.m:144


def interp1(x, v, xq):
    """interp1(x, v, xq) (linear) as the contract states it: the bracket of xq is the last j with
    x_j <= xq, clipped to n - 2; v_j + t (v_{j+1} - v_j); NaN outside [x_1, x_n] and for n < 2."""
    x, v, xq = (np.asarray(a, dtype=np.float64) for a in (x, v, xq))
    out = np.full(xq.shape, np.nan)
    n = x.size
    if n < 2:
        return out
    j = np.clip(np.searchsorted(x, xq, side="right") - 1, 0, n - 2)
    t = (xq - x[j]) / (x[j + 1] - x[j])
    val = v[j] + t * (v[j + 1] - v[j])
    inside = (xq >= x[0]) & (xq <= x[-1])
    out[inside] = val[inside]
    return out


def rest_grid(csr, G, min_lambda=911.75, dlambda=0.25, lya_wavelength=1215.6701, max_noise_variance=1.0,
              num_forest_lines=0, prev_tau_0=0.0023, prev_beta=3.65):
    """(rest_fluxes, lya_1pzs, rest_noise_variances), [num_quasars, G] each: learn_qso_model.m:37-67;
    with num_forest_lines > 1 the flux and noise of learn_qso_model_meanflux.m:98-129 (line table in
    Angstrom)."""
    off = np.asarray(csr["offsets"])
    nq = off.size - 1
    xq = min_lambda + np.arange(G) * dlambda
    F, L, N = (np.full((nq, G), np.nan) for _ in range(3))
    wl_a = [row[0] * 1e8 for row in LINES]
    tau0 = [prev_tau_0 * row[1] / LYA_OSCILLATOR_STRENGTH * (row[0] * 1e8) / lya_wavelength for row in LINES]
    for i in range(nq):
        s = slice(off[i], off[i + 1])
        wl = np.asarray(csr["wavelengths"][s], dtype=np.float64)
        mk = np.asarray(csr["pixel_mask"][s]) != 0
        fl = np.where(mk, np.nan, csr["flux"][s])
        nv = np.where(mk, np.nan, csr["noise_variance"][s])
        z = float(csr["z_qsos"][i])
        rest = wl / (1 + z)
        lya = interp1(rest, 1 + (wl - lya_wavelength) / lya_wavelength, xq)
        f = interp1(rest, fl, xq)
        v = interp1(rest, nv, xq)
        ind = v > max_noise_variance
        lya[ind] = f[ind] = v[ind] = np.nan
        if num_forest_lines > 1:
            total = np.zeros(G)
            for j in range(num_forest_lines):
                zj = interp1(rest, 1 + (wl - wl_a[j]) / wl_a[j], xq)
                if j > 0:
                    zj = zj * (zj <= 1 + z)
                zj[ind] = np.nan
                tj = tau0[j] * zj ** prev_beta
                total = total + np.where(np.isnan(tj), 0.0, tj)
            absorption = np.exp(-total)
            f = f / absorption
            v = v / (absorption * absorption)
        F[i], L[i], N[i] = f, lya, v
    return F, L, N


def column_stats(rest_fluxes):
    """(mu, centered, std, count): nanmean (:70), the centring (:71), nanstd with n - 1 (:87)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            mu = np.nanmean(rest_fluxes, axis=0)
            centered = rest_fluxes - mu
            std = np.nanstd(centered, axis=0, ddof=1)
    count = np.isfinite(rest_fluxes).sum(axis=0)
    std[count == 1] = 0.0  # MATLAB's std of one value
    return mu, centered, std, count


def pca_covariance(centered, complete_rows=False):
    """(cov, count, rows_used) of pca(centered, 'rows', 'pairwise' | 'complete').  Pairwise: the
    non-centred second moment over the quasars finite in both pixels over (N_ab - 1) (pca's own
    re-centring by the column nanmean, O(1e-16) after the centring, omitted).  Complete: the rows
    without NaN, centred by their own column mean, X'X / (n_c - 1)."""
    if complete_rows:
        rows = np.all(np.isfinite(centered), axis=1)
        X = centered[rows]
        X = X - X.mean(axis=0)
        n = float(rows.sum())
        return X.T @ X / (n - 1.0), np.full((centered.shape[1],) * 2, n), int(rows.sum())
    fin = np.isfinite(centered)
    X = np.where(fin, centered, 0.0)
    Mk = fin.astype(np.float64)
    P, N = X.T @ X, Mk.T @ Mk
    with np.errstate(invalid="ignore", divide="ignore"):
        return P / (N - 1.0), N, int(np.any(fin, axis=1).sum())


def pca_init(cov, k):
    """(initial_M, latent): eigenvalues descending, each coefficient column flipped so that its
    element of largest magnitude is positive, initial_M = coeff(:, 1:k) .* sqrt(latent(1:k))'."""
    w, V = np.linalg.eigh(cov)
    latent = w[::-1]
    coeff = V[:, ::-1][:, :k]
    big = np.abs(coeff).argmax(axis=0)
    coeff = coeff * np.where(coeff[big, np.arange(k)] < 0.0, -1.0, 1.0)[None, :]
    return coeff * np.sqrt(latent[:k])[None, :], latent


def initial_x(initial_M, std, initial_c_0=0.1, initial_tau_0=0.0023, initial_beta=3.65):
    """learn_qso_model.m:87-96."""
    return np.concatenate([np.asarray(initial_M).ravel(order="F"), np.log(std),
                           [np.log(initial_c_0), np.log(initial_tau_0), np.log(initial_beta)]])


def principal_cosines(A, B):
    """Cosines of the principal angles between the column spaces of A and B (descending)."""
    qa, _ = np.linalg.qr(A)
    qb, _ = np.linalg.qr(B)
    return np.linalg.svd(qa.T @ qb, compute_uv=False)


def dla_free_training_set(num, k=20, first_index=0):
    """``num`` DLA-free synthetic quasars (the even indices of make_boss_spectrum, which inject no
    DLA) with the DR12Q redshift mix, and the generator's model."""
    from gp_dla_detection_amd import synthetic
    model = synthetic.make_model(k)
    idx = first_index + 2 * np.arange(num)
    z = synthetic.sample_dr12q_redshifts(int(idx[-1]) + 1)
    return [synthetic.make_boss_spectrum(int(i), float(z[i]), model) for i in idx], model
