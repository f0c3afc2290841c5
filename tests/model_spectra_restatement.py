"""NumPy-and-oracle restatement of the model-spectra products (plain module: tests/test_model_spectra.py
and tests/test_gpu_model_spectra.py import it; no package compute code is used -- only the package's
Lyman-series DATA table and parameter defaults).

Everything is written from the definitions:

* the unmasked-range grid and its padded wavelengths (process_qsos.m:104-108, :168-176), the padding
  taken from the oracle's own dump so that both sides evaluate profiles at the same numbers;
* P1  ``map_absorption``: product of ``oracle.voigt`` profiles (voigt.c:253-304);
* P2  ``moments``: w_i = exp(l_i - nanmax l) / Sum, NaN -> 0; mean = Sum w a, var = Sum w (a - mean)^2;
* the prepared rows of the kept pixels -- the oracle's dump for the single-DLA model, and the
  mean-flux model's rows by multi :245-293 (``oracle.mean_flux_suppression`` for :267-285);
* P3  ``continuum``: the posterior mean of the low-rank coefficients in TWO forms -- dense, K = A (M M'
  + Omega) A + N formed explicitly and solved, and Woodbury, B = I + M' diag(a^2/d) M -- then mu + M c
  on the whole grid with a masked pixel's mu and M interpolated like a kept one's;
* P4  ``model_mean``: qso_loader.py:1685-1711 with ``oracle.voigt(raw=True)`` and the total scale
  factor of :1777-1822.
"""
from __future__ import annotations

import numpy as np

from gp_dla_detection_amd._lyman import LINES
from gp_dla_detection_amd.parameters import Parameters

WL = np.array([row[0] for row in LINES]) * 1e8      # all_transition_wavelengths, Angstrom
OSC = np.array([row[1] for row in LINES])           # all_oscillator_strengths


def grid(oracle, model, sp, p: Parameters | None = None) -> dict:
    """The unmasked-range grid of one quasar and the oracle's prepared quantities on its kept pixels."""
    from oracle.oracle import OracleParams
    p = p or Parameters()
    wl = np.asarray(sp["wavelengths"], dtype=np.float64)
    rest = wl / (1 + sp["z_qso"])
    inside = (rest >= p.min_lambda) & (rest <= p.max_lambda)
    kept_in = (np.asarray(sp["pixel_mask"])[inside] == 0)
    g = dict(inside=inside, kept=kept_in, n_u=int(inside.sum()), wl=wl[inside], z_qso=float(sp["z_qso"]))
    if not kept_in.any():
        return g
    r = oracle.process_spectrum(model, np.array([0.5]), np.array([1e20]), wl, sp["flux"], sp["noise_variance"],
                                sp["pixel_mask"], sp["z_qso"], params=OracleParams(num_lines=1), dump=True)
    assert r["rc"] == 0 and r["n_unmasked"] == g["n_u"] and r["n_kept"] == kept_in.sum()
    g.update(pad=r["padded_wavelengths"], min_z=r["min_z_dla"], max_z=r["max_z_dla"], mu=r["this_mu"],
             M=r["this_M"], omega2=r["this_omega2"], y=np.asarray(sp["flux"], dtype=np.float64)[inside][kept_in],
             nu=np.asarray(sp["noise_variance"], dtype=np.float64)[inside][kept_in])
    assert np.array_equal(g["pad"][3:-3], g["wl"])
    return g


def map_absorption(oracle, pad, z_dlas, log_nhis, num_lines: int) -> np.ndarray:
    a = np.ones(pad.size - 6)
    for z, ln in zip(z_dlas, log_nhis):
        a = a * oracle.voigt(pad, z, 10.0 ** ln, num_lines)
    return a


def weights(ll) -> np.ndarray:
    ll = np.asarray(ll, dtype=np.float64)
    if np.isnan(ll).all():
        return np.full(ll.size, np.nan)
    w = np.exp(ll - np.nanmax(ll))
    w[np.isnan(w)] = 0.0
    return w / w.sum()


def moments(oracle, g, offset_samples, nhi_samples, ll, num_lines: int):
    """(mean, var) over ALL samples of the broadened profile, weighted by the posterior of row ``ll``."""
    w = weights(ll)
    n_u = g["n_u"]
    if np.isnan(w).all() or "pad" not in g:
        return np.full(n_u, np.nan), np.full(n_u, np.nan)
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.asarray(offset_samples)
    A = np.empty((w.size, n_u))
    for i in range(w.size):
        A[i] = oracle.voigt(g["pad"], z[i], nhi_samples[i], num_lines)
    mean = w @ A
    return mean, w @ (A - mean) ** 2


def interp_rows(model, wl, z_qso):
    """mu and M of the model at observed wavelengths (griddedInterpolant 'linear', process_qsos.m:66-71)."""
    rest = wl / (1 + z_qso)
    grid_ = np.asarray(model["rest_wavelengths"])
    mu = np.interp(rest, grid_, model["mu"])
    M = np.stack([np.interp(rest, grid_, np.asarray(model["M"])[:, c]) for c in range(np.asarray(model["M"]).shape[1])], axis=1)
    return mu, M


def meanflux_rows(oracle, model, g, prev_tau_0=0.0023, prev_beta=3.65, num_forest_lines=31, lya_wavelength=1215.6701):
    """The kept-pixel rows (mu, M, omega2) of the mean-flux model, multi :236-293, from the single-DLA
    dump: omega2 there is exp(2 log omega) x (1 - exp(-tau_0 (1+z)^beta) + c_0)^2 (process_qsos.m:142-146),
    so the interpolated exp(2 log omega) is re-made here from the model."""
    wl = g["wl"][g["kept"]]
    z_qso = g["z_qso"]
    rest = wl / (1 + z_qso)
    log_omega = np.interp(rest, model["rest_wavelengths"], model["log_omega"])
    omega2 = np.exp(2 * log_omega)
    tau_0, beta, c_0 = np.exp(model["log_tau_0"]), np.exp(model["log_beta"]), np.exp(model["log_c_0"])
    lya_zs = (wl - lya_wavelength) / lya_wavelength
    depth = tau_0 * (1 + lya_zs) ** beta
    for l in range(1, num_forest_lines):
        one_pz = WL[0] * (1 + lya_zs) / WL[l]
        one_pz = one_pz * (one_pz <= (1 + z_qso))
        depth = depth + tau_0 * WL[l] * OSC[l] / (WL[0] * OSC[0]) * one_pz ** beta
    omega2 = omega2 * (1 - np.exp(-depth) + c_0) ** 2
    mf = oracle.mean_flux_suppression(wl, z_qso, prev_tau_0, prev_beta, num_forest_lines, lya_wavelength)
    return g["mu"] * mf, g["M"] * mf[:, None], omega2 * mf ** 2


def coefficients_dense(y, mu, M, omega2, nu, a):
    """E[c | y] for y = a (mu + M c + omega eps) + noise, c ~ N(0, I): with K = A (M M' + Omega) A + N formed
    explicitly, c = (A M)' K^-1 (y - a mu)."""
    AM = a[:, None] * M
    K = AM @ AM.T + np.diag(a * a * omega2 + nu)
    return AM.T @ np.linalg.solve(K, y - a * mu)


def coefficients_woodbury(y, mu, M, omega2, nu, a):
    d = a * a * omega2 + nu
    r = y - a * mu
    B = np.eye(M.shape[1]) + M.T @ ((a * a / d)[:, None] * M)
    return np.linalg.solve(B, M.T @ (a * r / d))


def continuum(oracle, model, g, a_full, meanflux: bool, form: str = "dense", **mf):
    """(continuum, model_flux) on the whole grid; ``a_full``: absorption on the grid (ones: null model)."""
    mu, M, omega2 = meanflux_rows(oracle, model, g, **mf) if meanflux else (g["mu"], g["M"], g["omega2"])
    a = a_full[g["kept"]]
    solve = coefficients_dense if form == "dense" else coefficients_woodbury
    c = solve(g["y"], mu, M, omega2, g["nu"], a)
    mu_all, M_all = interp_rows(model, g["wl"], g["z_qso"])
    if meanflux:
        f = oracle.mean_flux_suppression(g["wl"], g["z_qso"], mf.get("prev_tau_0", 0.0023), mf.get("prev_beta", 3.65),
                                         mf.get("num_forest_lines", 31), mf.get("lya_wavelength", 1215.6701))
        mu_all, M_all = mu_all * f, M_all * f[:, None]
    cont = mu_all + M_all @ c
    return cont, a_full * cont


def total_scale_factor(tau, beta, z_qso, rest_wavelengths, num_lines=31):
    """qso_loader.py:1777-1822."""
    total = np.zeros(rest_wavelengths.size)
    for i in range(num_lines):
        one_pz = rest_wavelengths * (1 + z_qso) / WL[i]
        if i != 0:
            one_pz = one_pz * (one_pz <= (1 + z_qso))
        total = total + (tau * OSC[i] / OSC[0] * WL[i] / 1215.6701) * one_pz ** beta   # tau_lyseries, :29-30
    return np.exp(-total)


def model_mean(oracle, rest_wavelengths, mu, z_qso, z_dlas, log_nhis, suppressed, num_voigt_lines, num_forest_lines,
               tau=0.0023, beta=3.65):
    """qso_loader.py:1685-1711: this_mu."""
    this_mu = np.asarray(mu, dtype=np.float64)
    if suppressed:
        this_mu = this_mu * total_scale_factor(tau, beta, z_qso, rest_wavelengths, num_forest_lines)
    for z, ln in zip(z_dlas, log_nhis):
        this_mu = this_mu * oracle.voigt(rest_wavelengths * (1 + z_qso), z, 10.0 ** ln, num_voigt_lines, raw=True)
    return this_mu


# ------------------------------------------------------------------------------------------------
# the continuum cases the CPU test and the GPU test share
# ------------------------------------------------------------------------------------------------

def continuum_cases(oracle, ranks=(20, 40)) -> list:
    """Quasars x (mean-flux model or not) x (null model or absorbers) for the continuum comparison: for
    each rank the tile-boundary quasar of tests/production_shapes.py (a masked run across stored pixels
    250 .. 262) in all four variants, and the confined (36 .. 40 kept of ~1249), both-ends-masked and a
    ``synthetic.make_spectrum`` quasar in one variant each."""
    import production_shapes as ps
    from gp_dla_detection_amd import synthetic
    cases = []
    for k in ranks:
        model = synthetic.make_model(k)
        strat = ps.stratified_quasars(k)
        picks = [("tile_boundary_run", mf, ab) for mf in (False, True) for ab in (False, True)]
        picks += [("confined_40px", True, True), ("both_ends_masked_runs", False, True), ("synthetic", True, False)]
        for name, meanflux, with_abs in picks:
            sp = (synthetic.make_spectrum(4100 + k, 700, model, mask_fraction=0.05) if name == "synthetic"
                  else strat[ps.by_stratum(strat, name)])
            g = grid(oracle, model, sp)
            lo, hi = g["min_z"], g["max_z"]
            z = [lo + 0.35 * (hi - lo), lo + 0.8 * (hi - lo)] if with_abs else []
            ln = [20.6, 21.4] if with_abs else []
            a = map_absorption(oracle, g["pad"], z, ln, 3)
            cases.append(dict(name=f"k={k} {name} meanflux={int(meanflux)} absorbers={len(z)}", k=k, model=model,
                              spectrum=sp, grid=g, meanflux=meanflux, z_dlas=np.array(z), log_nhis=np.array(ln),
                              absorption=a))
    return cases


def continuum_tolerance(disagreement: float) -> float:
    """10 x the dense-vs-Woodbury disagreement of the restatement, floored at 1e-12, never looser than 1e-8."""
    return float(min(max(10.0 * disagreement, 1e-12), 1e-8))
