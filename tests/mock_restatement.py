"""NumPy-and-oracle restatement of the mock-spectra draw (plain module: tests/test_mocks.py and
tests/test_gpu_mocks.py import it; no package compute code is used -- only parameter defaults).

Written from the definitions in include/gpdla.h ("Mock spectra"):

* Philox4x32-10 on NumPy integers (Salmon et al. 2011), counter (lo32(index), hi32(index), stream, 1),
  key (seed ^ qid, (seed >> 32) ^ (qid >> 32) ^ 0x5851F42D);
* the two 53-bit uniforms and the Box-Muller normal;
* the prepared rows of the kept pixels from the ORACLE (``process_spectrum(dump=True)``; mean-flux model:
  ``model_spectra_restatement.meanflux_rows``), the broadened absorption from ``oracle.voigt``;
* flux = a (mu + M z) + sqrt(a^2 omega2 + nu) eps.

And the two whitened statistics that say whether a set of spectra is a draw from the likelihood's model.
"""
from __future__ import annotations

import numpy as np

import model_spectra_restatement as msr
from gp_dla_detection_amd.parameters import Parameters

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over NumPy uint64 arrays holding 32-bit values; returns four such arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32)
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def key(seed: int, qid: int):
    seed, qid = int(seed) & (2 ** 64 - 1), int(qid) & (2 ** 64 - 1)
    return (seed ^ qid) & 0xFFFFFFFF, ((seed >> 32) ^ (qid >> 32) ^ 0x5851F42D) & 0xFFFFFFFF


def mantissas(out):
    """(m1, m2): 53-bit integers from the four output words."""
    m = lambda a, b: (a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)  # noqa: E731
    return m(out[0], out[1]), m(out[2], out[3])


def normal_from_mantissas(m1, m2):
    u1, u2 = (np.asarray(m1, dtype=np.float64) + 1.0) * 2.0 ** -53, np.asarray(m2, dtype=np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)


def normals(seed: int, qid: int, stream: int, indices) -> np.ndarray:
    idx = np.asarray(indices, dtype=np.uint64)
    k0, k1 = key(seed, qid)
    return normal_from_mantissas(*mantissas(philox4x32_10(idx & M32, idx >> np.uint64(32), stream, 1, k0, k1)))


def rows(oracle, model, sp, meanflux: bool, p: Parameters | None = None):
    """(grid dict, mu, M, omega2) of the kept pixels: what the sweep sees."""
    g = msr.grid(oracle, model, sp, p)
    if "pad" not in g:
        return g, None, None, None
    mu, M, om = msr.meanflux_rows(oracle, model, g) if meanflux else (g["mu"], g["M"], g["omega2"])
    return g, mu, M, om


def draw(oracle, model, sp, qid: int, seed: int, z_dlas=(), log_nhis=(), meanflux: bool = False, num_lines: int = 3,
         p: Parameters | None = None) -> dict:
    """One quasar.  ``flux`` in the stored layout; ``absorption, continuum, sigma`` on the unmasked-range
    grid (NaN continuum / sigma at its masked pixels); ``latents``; plus the kept-pixel rows used."""
    g, mu, M, om = rows(oracle, model, sp, meanflux, p)
    flux = np.array(sp["flux"], dtype=np.float64)
    n_u = g["n_u"]
    if mu is None:
        return dict(flux=flux, grid=g, status=1, absorption=np.full(n_u, np.nan), continuum=np.full(n_u, np.nan),
                    sigma=np.full(n_u, np.nan), latents=np.full(np.asarray(model["M"]).shape[1], np.nan))
    k = M.shape[1]
    z = normals(seed, qid, 0, np.arange(k))
    a_full = msr.map_absorption(oracle, g["pad"], z_dlas, log_nhis, num_lines)
    a = a_full[g["kept"]]
    stored = np.flatnonzero(g["inside"])            # stored position of every grid pixel
    eps = normals(seed, qid, 1, stored[g["kept"]])
    cont = mu + M @ z
    sigma = np.sqrt(a * a * om + g["nu"])
    f = a * cont + sigma * eps
    flux[stored] = _scatter(f, g["kept"])
    return dict(flux=flux, grid=g, status=0, absorption=a_full, continuum=_scatter(cont, g["kept"]), sigma=_scatter(sigma, g["kept"]), latents=z,
                mu=mu, M=M, omega2=om, a=a, nu=g["nu"], y=f)


def _scatter(v, kept):
    out = np.full(kept.size, np.nan)
    out[kept] = v
    return out


def whitened_statistics(y, a, mu, M, omega2, nu):
    """(Q1, Q2, n, k) of one quasar's kept pixels under N(a mu, A (M M' + Omega) A + N):
    Q1 = r' K^-1 r (chi^2 with n degrees of freedom), through the Woodbury identity; and
    Q2 = g' [(B - I) B]^-1 g with g = (A M)' D^-1 r, B = I + (A M)' D^-1 (A M): g ~ N(0, (B - I) B), so Q2 is
    chi^2 with k degrees of freedom -- and collapses towards 0 when the low-rank term is missing from
    the draw (then g ~ N(0, B - I))."""
    r = y - a * mu
    d = a * a * omega2 + nu
    AM = a[:, None] * M
    k = M.shape[1]
    C = AM.T @ (AM / d[:, None])          # B - I
    B = np.eye(k) + C
    g = AM.T @ (r / d)
    q1 = r @ (r / d) - g @ np.linalg.solve(B, g)
    q2 = g @ np.linalg.solve(C @ B, g)
    return float(q1), float(q2), int(r.size), int(k)


def chi2_bound(dof: int) -> float:
    """5 sigma of a chi^2 with ``dof`` degrees of freedom in the normal approximation."""
    return 5.0 * np.sqrt(2.0 * dof)


# ------------------------------------------------------------------------------------------------
# the inputs the CPU tests and the GPU tests share
# ------------------------------------------------------------------------------------------------

MOCK_SEED = 0x5EED0D1A2026     # seed of the draws (chosen as tests/test_gpu_mocks.py's docstring tells)
TRUTH_SEED = 20261017
PRIOR_P_DLA = 0.1


def recovery_case(oracle, num: int = 24, k: int = 20, num_samples: int = 2048) -> dict:
    """24 BOSS-grid templates with the DR12Q length mix; quasar i has no absorber (i % 3 == 0), one with
    log N_HI uniform in [20.3, 22] (i % 3 == 1) or in [21, 22] (i % 3 == 2), z uniform in its search range."""
    from gp_dla_detection_amd import synthetic
    model, samples = synthetic.make_model(k), synthetic.make_samples(num_samples)
    zq = synthetic.sample_dr12q_redshifts(num)
    templates = [synthetic.make_boss_spectrum(i, float(zq[i]), model, mask_fraction=0.05) for i in range(num)]
    rng = np.random.default_rng(TRUTH_SEED)
    off, zs, ns = np.zeros(num + 1, dtype=np.int64), [], []
    for i, t in enumerate(templates):
        g = msr.grid(oracle, model, t)
        u, v = rng.uniform(), rng.uniform()
        if i % 3:
            zs.append(g["min_z"] + (g["max_z"] - g["min_z"]) * u)
            ns.append((20.3 if i % 3 == 1 else 21.0) + ((22.0 - 20.3) if i % 3 == 1 else 1.0) * v)
        off[i + 1] = len(zs)
    return dict(model=model, samples=samples, templates=templates, truth=(off, np.array(zs), np.array(ns)))


def meanflux_case(oracle, num: int = 6, k: int = 20, num_samples: int = 512) -> dict:
    """Templates for the mean-flux model (MultiParameters): quasar i has i % 4 absorbers (0 .. 3), at
    least 0.05 apart in redshift, log N_HI in [20.3, 21.8]."""
    from gp_dla_detection_amd import synthetic
    model, samples = synthetic.make_model(k), synthetic.make_samples(num_samples)
    zq = synthetic.sample_dr12q_redshifts(40)[20:20 + num]
    templates = [synthetic.make_boss_spectrum(500 + i, float(zq[i]), model, mask_fraction=0.05) for i in range(num)]
    rng = np.random.default_rng(TRUTH_SEED + 1)
    off, zs, ns = np.zeros(num + 1, dtype=np.int64), [], []
    for i, t in enumerate(templates):
        g = msr.grid(oracle, model, t)
        n = i % 4
        frac = np.sort(rng.uniform(0.05, 0.95, size=8))[::2][:n]       # spread over the search range
        for f in frac:
            zs.append(g["min_z"] + (g["max_z"] - g["min_z"]) * f)
            ns.append(rng.uniform(20.3, 21.8))
        off[i + 1] = len(zs)
    return dict(model=model, samples=samples, templates=templates, truth=(off, np.array(zs), np.array(ns)))


def absorbers_of(truth, i):
    off, z, n = truth
    return z[off[i]:off[i + 1]], n[off[i]:off[i + 1]]


def log_odds_oracle(oracle, model, samples, sp, flux, p_dla: float = PRIOR_P_DLA):
    """(log odds DLA : no DLA, oracle result) of one quasar with ``flux`` in place of the template's."""
    r = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"], flux,
                                sp["noise_variance"], sp["pixel_mask"], sp["z_qso"])
    assert r["rc"] == 0
    return (r["log_likelihood_dla"] + np.log(p_dla)) - (r["log_likelihood_no_dla"] + np.log(1 - p_dla)), r
