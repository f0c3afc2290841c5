"""NumPy-and-oracle restatement of the marginal continuum (plain module: tests/test_marginal_continuum.py
and tests/test_gpu_marginal_continuum.py import it; no package compute code is used).

Written from the definitions in include/gpdla.h.  Per sample i with broadened profile a_i (``oracle.voigt``) on the
kept pixels, in TWO forms:

* dense     K_i = A_i (M M' + Omega) A_i + N formed explicitly; c_i = (A_i M)' K_i^-1 (y - a_i mu),
            Sigma_i = I - (A_i M)' K_i^-1 A_i M -- no Woodbury identity;
* woodbury  B_i = I + M' diag(a_i^2 / d_i) M; c_i = B_i^-1 M' (a_i (y - a_i mu) / d_i), Sigma_i = B_i^-1.

Then the reduction over the samples of a table (weights of ``model_spectra_restatement.weights``; a sample of weight
exactly 0 is never touched), the mixture over (null, sub-DLA table, DLA table), and the three per-pixel arrays on the
whole grid with a masked pixel's mu and M interpolated like a kept one's.
"""
from __future__ import annotations

import numpy as np

from model_spectra_restatement import grid, interp_rows, meanflux_rows, weights  # noqa: F401  (grid: re-exported)

COMPONENTS = ("null", "sub_dla", "dla")
NHI_KEY = {"sub_dla": "lls_nhi_samples", "dla": "nhi_samples"}


def sample_dense(y, mu, M, omega2, nu, a):
    """(c_i, Sigma_i) with K_i formed and solved."""
    AM = a[:, None] * M
    K = AM @ AM.T + np.diag(a * a * omega2 + nu)
    sol = np.linalg.solve(K, np.column_stack([y - a * mu, AM]))
    return AM.T @ sol[:, 0], np.eye(M.shape[1]) - AM.T @ sol[:, 1:]


def sample_woodbury(y, mu, M, omega2, nu, a):
    d = a * a * omega2 + nu
    B = np.eye(M.shape[1]) + M.T @ ((a * a / d)[:, None] * M)
    Binv = np.linalg.inv(B)
    return Binv @ (M.T @ (a * (y - a * mu) / d)), Binv


def prepared_rows(oracle, model, g, meanflux: bool):
    """(y, mu, M, omega2, nu) of the kept pixels."""
    mu, M, omega2 = meanflux_rows(oracle, model, g) if meanflux else (g["mu"], g["M"], g["omega2"])
    return g["y"], mu, M, omega2, g["nu"]


def has_weights(ll) -> bool:
    """A row of sample log-likelihoods with an entry above -inf and none at +inf."""
    ll = np.asarray(ll, dtype=np.float64)
    return bool((ll[~np.isnan(ll)] > -np.inf).any() and not np.isposinf(ll).any())


def sampled_component(oracle, rows, g, offset_samples, nhi, ll, num_lines: int, form: str = "dense") -> dict:
    """cbar, W, S2 = Sum w c c' and the per-sample c_i [S, k] (NaN rows at weight 0) of one table."""
    k = rows[2].shape[1]
    w = weights(ll)
    solve = sample_dense if form == "dense" else sample_woodbury
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.asarray(offset_samples)
    cbar, W, S2 = np.zeros(k), np.zeros((k, k)), np.zeros((k, k))
    ci = np.full((w.size, k), np.nan)
    for i in np.flatnonzero(w > 0):
        a = oracle.voigt(g["pad"], z[i], nhi[i], num_lines)[g["kept"]]
        c, Sig = solve(*rows, a)
        ci[i] = c
        cbar += w[i] * c
        W += w[i] * Sig
        S2 += w[i] * np.outer(c, c)
    return dict(cbar=cbar, W=W, S2=S2, sample_coefficients=ci)


def null_component(rows, form: str = "dense") -> dict:
    c, Sig = (sample_dense if form == "dense" else sample_woodbury)(*rows, np.ones(rows[0].size))
    return dict(cbar=c, W=Sig, S2=np.outer(c, c))


def mix(parts, p):
    """c, W, V from [(component dict or None)] and the normalised weights p; a weight of 0 skips the component."""
    k = next(x for x in parts if x is not None)["cbar"].size
    c, W, S2 = np.zeros(k), np.zeros((k, k)), np.zeros((k, k))
    for part, pm in zip(parts, p):
        if pm > 0:
            c += pm * part["cbar"]
            W += pm * part["W"]
            S2 += pm * part["S2"]
    return c, W, S2 - np.outer(c, c)


def on_grid(oracle, model, g, meanflux: bool, c, W, V):
    """continuum_mean, continuum_var, continuum_var_between on all n_u pixels."""
    mu_all, M_all = interp_rows(model, g["wl"], g["z_qso"])
    if meanflux:
        f = oracle.mean_flux_suppression(g["wl"], g["z_qso"], 0.0023, 3.65, 31, 1215.6701)
        mu_all, M_all = mu_all * f, M_all * f[:, None]
    return (mu_all + M_all @ c, np.einsum("pi,ij,pj->p", M_all, W + V, M_all), np.einsum("pi,ij,pj->p", M_all, V, M_all))


def vech(A) -> np.ndarray:
    """The packed lower triangle, row by row."""
    return A[np.tril_indices(A.shape[0])]


def marginal_continuum(oracle, model, g, samples, tables: dict, p, meanflux: bool, num_lines: int = 3, form: str = "dense") -> dict:
    """Everything gpdla_batch_marginal_continuum returns for one quasar.  ``tables``: {"dla": row, "sub_dla": row} of
    sample log-likelihoods (those of weight 0 may be missing); ``p``: (null, sub-DLA, DLA) weights, not yet normalised."""
    k = np.asarray(model["M"]).shape[1]
    nb, n_u = k * (k + 1) // 2, g["n_u"]
    S = np.asarray(samples["offset_samples"]).size
    p = np.asarray(p, dtype=np.float64)
    p = p / p.sum()
    nan = dict(continuum_mean=np.full(n_u, np.nan), continuum_var=np.full(n_u, np.nan), continuum_var_between=np.full(n_u, np.nan),
               coef_mean=np.full(k, np.nan), coef_cov_within=np.full(nb, np.nan), coef_cov_between=np.full(nb, np.nan),
               sample_coefficients=np.full((S, k), np.nan))
    if "pad" not in g:
        return dict(nan, status=1)
    rows = prepared_rows(oracle, model, g, meanflux)
    parts, ci = [null_component(rows, form) if p[0] > 0 else None], nan["sample_coefficients"]
    none = False
    for name, pm in zip(COMPONENTS[1:], p[1:]):
        if pm > 0 and not has_weights(tables[name]):
            none = True
        if pm > 0 and not none:
            parts.append(sampled_component(oracle, rows, g, samples["offset_samples"], samples[NHI_KEY[name]], tables[name],
                                           num_lines, form))
            ci = parts[-1]["sample_coefficients"]
        else:
            parts.append(None)
    if none:
        return dict(nan, status=0)
    c, W, V = mix(parts, p)
    mean, var, btw = on_grid(oracle, model, g, meanflux, c, W, V)
    return dict(continuum_mean=mean, continuum_var=var, continuum_var_between=btw, coef_mean=c, coef_cov_within=vech(W),
                coef_cov_between=vech(V), sample_coefficients=ci, status=0)


def brute_force_mixture(parts_samples, p):
    """The law of total variance the long way: the mixture over (model, sample) PAIRS with weights p_m w_i.
    ``parts_samples``: per component a list of (w_i, c_i, Sigma_i) (the null component: one pair of weight 1).
    Returns (mean, total covariance) of c."""
    pairs = [(pm * w, c, Sig) for comp, pm in zip(parts_samples, p) if pm > 0 for (w, c, Sig) in comp if w > 0]
    mean = sum(wt * c for wt, c, _ in pairs)
    cov = sum(wt * (Sig + np.outer(c - mean, c - mean)) for wt, c, Sig in pairs)
    return mean, cov


PRODUCTS_COEF = ("sample_coefficients", "coef_mean", "continuum_mean")          # R.continuum_tolerance of their own disagreement
PRODUCTS_COV = ("coef_cov_within", "coef_cov_between", "continuum_var", "continuum_var_between")


def deviation(a, b) -> float:
    """max |a - b| with matching NaN patterns (inf otherwise)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return float("inf")
    d = np.abs(a - b)[~np.isnan(a)]
    return float(d.max()) if d.size else 0.0
