"""NumPy-and-oracle restatement of the posterior predictive flux (plain module: tests/test_predictive_flux.py
and tests/test_gpu_predictive_flux.py import it; no package compute code is used).

Written from the definitions in include/gpdla.h.  Per sample i of weight > 0, with the broadened profile a_i
(``oracle.voigt``) on the whole grid, (c_i, Sigma_i) from the kept pixels in TWO forms -- dense (K_i formed and solved,
``marginal_continuum_restatement.sample_dense``) and Woodbury -- and then on EVERY pixel p of the grid, with mu_p and m_p
interpolated (and suppressed) like a kept pixel's:

    t_ip = mu_p + m_p' c_i,   s_ip = m_p' Sigma_i m_p,   f_ip = a_ip t_ip
    F1 = Sum w f,  F2 = Sum w f^2,  FW = Sum w a^2 s,  FD = Sum w (a^2 omega2 + nu)  (kept pixels; NaN on masked ones)

the null component with a = 1 and one sample of weight 1, and the mixture over (null, sub-DLA table, DLA table).
``brute_force_mixture`` states the law of total variance the long way, over (model, sample) pairs.
"""
from __future__ import annotations

import numpy as np

import marginal_continuum_restatement as MR
import model_spectra_restatement as R
from marginal_continuum_restatement import COMPONENTS, NHI_KEY, deviation, has_weights  # noqa: F401  (re-exported)

PRODUCTS_MEAN = ("flux_mean",)
PRODUCTS_VAR = ("flux_var", "flux_var_within", "flux_var_between", "noise_var")
PRODUCTS = PRODUCTS_MEAN + PRODUCTS_VAR


def grid_rows(oracle, model, g, meanflux: bool):
    """(mu_p, m_p) on all n_u pixels, and (omega2_p, nu_p) there with NaN on masked pixels."""
    mu_all, M_all = R.interp_rows(model, g["wl"], g["z_qso"])
    if meanflux:
        f = oracle.mean_flux_suppression(g["wl"], g["z_qso"], 0.0023, 3.65, 31, 1215.6701)
        mu_all, M_all = mu_all * f, M_all * f[:, None]
    rows = MR.prepared_rows(oracle, model, g, meanflux)
    omega2, nu = np.full(g["n_u"], np.nan), np.full(g["n_u"], np.nan)
    omega2[g["kept"]], nu[g["kept"]] = rows[3], rows[4]
    return mu_all, M_all, omega2, nu, rows


def per_sample(rows, mu_all, M_all, a_full, kept, form: str):
    """(t, s, f) on the whole grid for one profile."""
    solve = MR.sample_dense if form == "dense" else MR.sample_woodbury
    c, Sig = solve(*rows, a_full[kept])
    t = mu_all + M_all @ c
    s = np.einsum("pi,ij,pj->p", M_all, Sig, M_all)
    return t, s, a_full * t


def component(oracle, model, g, samples, name: str, ll, meanflux: bool, num_lines: int, form: str) -> dict:
    """F1, F2, FW, FD of one component and its (w_i, a_i, t_i, s_i) list; ``name`` "null": a = 1, weight 1."""
    mu_all, M_all, omega2, nu, rows = grid_rows(oracle, model, g, meanflux)
    n_u = g["n_u"]
    if name == "null":
        w, profiles = np.ones(1), [np.ones(n_u)]
    else:
        wt = R.weights(ll)
        z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.asarray(samples["offset_samples"])
        live = np.flatnonzero(wt > 0)       # a sample of weight exactly 0 is never touched
        w = wt[live]
        profiles = [oracle.voigt(g["pad"], z[i], samples[NHI_KEY[name]][i], num_lines) for i in live]
    F1, F2, FW, FD = np.zeros(n_u), np.zeros(n_u), np.zeros(n_u), np.zeros(n_u)
    pairs = []
    for wi, a in zip(w, profiles):
        t, s, f = per_sample(rows, mu_all, M_all, a, g["kept"], form)
        F1 += wi * f
        F2 += wi * f * f
        FW += wi * a * a * s
        FD += wi * (a * a * omega2 + nu)
        pairs.append((wi, a, t, s))
    return dict(F1=F1, F2=F2, FW=FW, FD=FD, pairs=pairs)


def mix(parts, p) -> dict:
    """The five arrays from [(component dict or None)] and the normalised weights p; a weight of 0 skips the component."""
    n_u = next(x for x in parts if x is not None)["F1"].size
    m1, m2, wi, nd = np.zeros(n_u), np.zeros(n_u), np.zeros(n_u), np.zeros(n_u)
    for part, pm in zip(parts, p):
        if pm > 0:
            m1 += pm * part["F1"]
            m2 += pm * part["F2"]
            wi += pm * part["FW"]
            nd += pm * part["FD"]
    btw = np.maximum(m2 - m1 * m1, 0.0)
    return dict(flux_mean=m1, flux_var_within=wi, flux_var_between=btw, flux_var=wi + btw, noise_var=nd)


def components(oracle, model, g, samples, tables: dict, p, meanflux: bool, num_lines: int = 3, form: str = "dense"):
    """(parts, none): the component dicts of positive weight (None otherwise), and whether a table of positive weight has
    no weights."""
    parts, none = [], False
    for name, pm in zip(COMPONENTS, p):
        if name != "null" and pm > 0 and not has_weights(tables[name]):
            none = True
        if pm > 0 and not none:
            parts.append(component(oracle, model, g, samples, name, None if name == "null" else tables[name], meanflux, num_lines, form))
        else:
            parts.append(None)
    return parts, none


def predictive_flux(oracle, model, g, samples, tables: dict, p, meanflux: bool, num_lines: int = 3, form: str = "dense") -> dict:
    """Everything gpdla_batch_predictive_flux returns for one quasar.  ``tables``: {"dla": row, "sub_dla": row} of sample
    log-likelihoods (those of weight 0 may be missing); ``p``: (null, sub-DLA, DLA) weights, not yet normalised."""
    n_u = g["n_u"]
    p = np.asarray(p, dtype=np.float64)
    p = p / p.sum()
    nan = {name: np.full(n_u, np.nan) for name in PRODUCTS}
    if "pad" not in g:
        return dict(nan, status=1)
    parts, none = components(oracle, model, g, samples, tables, p, meanflux, num_lines, form)
    if none:
        return dict(nan, status=0)
    return dict(mix(parts, p), status=0)


def brute_force_mixture(parts, p):
    """The law of total variance the long way: the mixture over (model, sample) PAIRS with weights p_m w_i, each pair a
    flux of mean a t and variance a^2 s.  Returns (mean, total variance) per pixel."""
    pairs = [(pm * w, a * t, a * a * s) for part, pm in zip(parts, p) if pm > 0 for (w, a, t, s) in part["pairs"] if w > 0]
    mean = sum(wt * f for wt, f, _ in pairs)
    var = sum(wt * (v + (f - mean) ** 2) for wt, f, v in pairs)
    return mean, var


def tolerances(dis: dict) -> dict:
    """R.continuum_tolerance per product family (the mean; the variances): 10 x the dense-vs-Woodbury disagreement of that
    family, floored at 1e-12, capped at 1e-8."""
    mean = R.continuum_tolerance(max(dis[n] for n in PRODUCTS_MEAN))
    var = R.continuum_tolerance(max(dis[n] for n in PRODUCTS_VAR))
    return {**{n: mean for n in PRODUCTS_MEAN}, **{n: var for n in PRODUCTS_VAR}}
