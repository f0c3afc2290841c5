"""Spectra on which the arithmetic of the learning front end is hard (plain module, like training_hard_cases.py and
continuum_hard_cases.py: the fixture generator tests/golden/make_exact_learn_hard.py, test_learn_hard.py,
test_gpu_learn_hard.py and, for ``evaluate`` / ``against_restatement``, test_gpu_learn_edges.py import it, nothing else does).

The front end is csrc/learn_kernels.hpp behind gpdla_training_create_from_spectra, gpdla_training_column_stats and
gpdla_training_pca_covariance: interp1 onto the rest grid, the noise mask, the mean-flux model's
optical depth and division, nanmean, the centring, nanstd (n - 1), the pairwise second moment and the complete-rows
covariance.  tests/test_gpu_learn.py holds it to the numpy restatement (tests/learn_restatement.py) on one family of
BOSS-like spectra under hand-set bounds.  Here the yardstick is a 50-digit evaluation of the very float64 inputs
(tests/golden/exact_learn_hard*.npz), the measure is ``deviation`` per block, and the bound is ``tolerance``: 10 x what
the restatement attains on the same block, floored at the bound test_gpu_learn.py holds the kernels to (FLOORS).

The CSR spectra are built directly, pixel by pixel.  Two constructions:

    base        jittered, evenly spread rest pixels (12 .. 54 of them) over part or all of the grid, flux 1 + 0.3 sin + noise,
                noise variances 10^U(-2, -0.5), a few masked pixels: the recipe of test_gpu_learn.mixed_spectra, small
    midpoint    G + 1 pixels, pixel j at rest min_lambda + (j - 1/2 + U(-0.3, 0.3)) dlambda, so that grid point g is
                bracketed by the pixels g and g + 1 whatever the rounding of lambda / (1 + z): a rest pixel whose two
                pixels carry the same value v interpolates to v exactly (v + t (v - v)), in every quasar

    class (stratum)        legs         what is hard
    control                both         nothing: the base recipe with its awkward quasars (one pixel, all masked, a noisy stretch)
    offset_flux_1e6        both         midpoint, shared; flux = 1e6 (1 + 1e-9 N(0, 1)), a few pixels masked: nanmean, the centring,
    offset_flux_1e-6       both           the one-pass std and the second moment under cancellation; the same at the 1e-6 scale
    constant_columns       both         midpoint, shared, 65 quasars; rest pixels where every quasar carries the same value
                                          (0.1 (g + 1): the sum rounds) and rest pixels scattered +-2 ulp about 1 + g / 64, with 2,
                                          3, 64 and 65 finite quasars (nested sets, so N_ab >= 2; two complete rows): std >= 0 and
                                          finite, 0 on the constant ones, log(std) finite on the scattered ones.  The mean-flux leg
                                          has prev_tau_0 = 0 (``parameters`` says why)
    dynamic_range          both         per-quasar flux scales 1e-6 .. 1e6 in one column: the order of the sequential sums, values
                                          relative to themselves at every scale
    tight_pixels           both         base, plus pixel pairs 1e-9, 1e-7 and 1e-5 apart (relative) that straddle a grid point,
                                          flux -5 | +5 on the pair: x1 - x0 keeps 7, 9 and 11 digits of the rest wavelengths
    sparse_pairs           both         midpoint, 9 quasars; 16-pixel tiles finite in quasars {0, 1}, {1, 2} and (pixel 32) {3, 4}:
                                          whole tile pairs with N_ab = 2, 1 (P / 0 = +-inf) and 0 (0 / -1 = -0); rest pixels with 1
                                          and 0 finite quasars; no complete row
    noise_cut              both         midpoint; every third rest pixel has its noise 0 .. 3 ulp below, on, or 1 .. 3 ulp above
                                          max_noise_variance (exactly: both pixels of its bracket carry it).  Equal is not noisy.
    high_z                 mean-flux    base at 915 .. 923 A (the lines to the levels 9 .. 16 lie inside the grid, so their indicators
    high_z_tau100          mean-flux      switch), z_qso in {4.98, 6.5}; the second at 1020 .. 1028 A with 100 x prev_tau_0: e^-tau
                                          spans 1 .. 1e-109 and noise / (e^-tau)^2 stays finite (up to 1e217).  The complete rows are
                                          the z = 6.5 ones: next to them in a column a z = 4.98 flux is 1e-60 of the mean and is
                                          rounded away by the centring, in any float64 evaluation
    indicator_edge_beta    mean-flux    midpoint, 70 quasars, G = 49; min_lambda set so that grid point 24 is the Ly-beta (Ly-gamma)
    indicator_edge_gamma   mean-flux      wavelength to an ulp: there the line's interpolated 1 + z_j sits within a few ulp of
                                          1 + z_qso, on either side

``excluded`` (indicator_edge, and wherever else it happens): the exact evaluation cannot settle a tie that float64 rounding
decides.  The yardstick takes the indicators as float64 forms them (the as-written comparison, as
make_exact_training_hard.py does for spectrum_loss_lyseries.m:32) and records the pixels where the 50-digit comparison
of some line says otherwise.  Those pixels are left out of the rest flux and rest noise blocks, and the rest pixels
(columns) that hold one are left out of the statistics and covariance blocks; EXCLUDED_CAP bounds their share of the
class's finite pixels.  On every other pixel a GPU indicator that differs from the restatement's moves the flux by
percents, far outside the bound.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_restatement as R  # noqa: E402
from training_hard_cases import save_npz  # noqa: E402,F401  (the generator writes with it)

from gp_dla_detection_amd._lyman_data import LINES  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters, Parameters  # noqa: E402

TOL_FACTOR = 10.0              # the project's convention (hard_conditioning_cases.TOL_FACTOR)
ORACLE_CAP = 1e-6              # a condition on the choice of inputs: the restatement stays this close to exact in every block
EXCLUDED_CAP = 0.02            # share of a class's finite pixels whose line indicator float64 rounding decides
DPS = 50                       # digits of the yardstick
FIXTURES = ("exact_learn_hard.npz", "exact_learn_hard_meanflux.npz")     # the single-DLA legs, the mean-flux legs

BLOCKS = ("rest_flux", "lya_1pzs", "rest_noise", "mu", "centered", "std", "cov_pairwise", "cov_complete")
#: the bounds of tests/test_gpu_learn.py: rest grid 1e-13 (mean-flux 1e-12), statistics 1e-12, covariance 1e-11 of max |cov|
FLOORS = {False: dict(rest_flux=1e-13, lya_1pzs=1e-13, rest_noise=1e-13, mu=1e-12, centered=1e-12, std=1e-12,
                      cov_pairwise=1e-11, cov_complete=1e-11),
          True: dict(rest_flux=1e-12, lya_1pzs=1e-13, rest_noise=1e-12, mu=1e-12, centered=1e-12, std=1e-12,
                     cov_pairwise=1e-11, cov_complete=1e-11)}

BOTH = ("control", "offset_flux_1e6", "offset_flux_1e-6", "constant_columns", "dynamic_range", "tight_pixels", "sparse_pairs",
        "noise_cut")
MEANFLUX_ONLY = ("high_z", "high_z_tau100", "indicator_edge_beta", "indicator_edge_gamma")
CLASSES = tuple((s, mf) for s in BOTH for mf in (False, True)) + tuple((s, True) for s in MEANFLUX_ONLY)
HARD_CLASSES = tuple(c for c in CLASSES if c[0] != "control")
assert len(CLASSES) == 20

BASE_SEED = 4100
NQ, G_SMALL, G_WIDE = 24, 33, 49
CONST_COLUMNS = {3: 2, 7: 3, 16: 64, 20: 65}       # rest pixel -> finite quasars (the first that many)
ULP_COLUMNS = {23: 2, 26: 3, 29: 64, 32: 65}          # (three apart: the rest pixel between two of them mixes an ordinary pixel in)
CUT_COLUMNS = tuple(range(1, G_SMALL, 3))
EDGE_POINT = 24                                      # the grid point of indicator_edge that sits on the line
TIGHT = (1e-9, 1e-7, 1e-5)


def class_name(cls) -> str:
    return f"{cls[0]}-{'meanflux' if cls[1] else 'single'}"


def fixture_of(cls) -> str:
    return FIXTURES[1] if cls[1] else FIXTURES[0]


def line_wavelengths():
    """the library's Lyman lines in Angstrom, as the restatement and the host form them"""
    return np.array([row[0] * 1e8 for row in LINES])


def parameters(cls):
    """the grid and the cuts of a class"""
    stratum, meanflux = cls
    G = G_WIDE if stratum.startswith("indicator_edge") else G_SMALL
    if not meanflux:
        lo = 1100.0
    elif stratum == "high_z":
        lo = 915.0
    elif stratum.startswith("indicator_edge"):
        lo = float(line_wavelengths()[1 if stratum.endswith("beta") else 2] - EDGE_POINT * 0.25)
    else:
        lo = 1020.0
    kw = dict(min_lambda=lo, max_lambda=lo + 0.25 * (G - 1))
    if meanflux:
        # constant_columns: prev_tau_0 = 0, e^-tau = 1 -- a quotient by any other e^-tau rounds by half an ulp, a quarter of the
        # scatter of the ulp columns, and no float64 evaluation has their std to better than 20 % (measured on the restatement)
        tau_0 = {"high_z_tau100": 0.23, "constant_columns": 0.0}.get(stratum, 0.0023)
        return MultiParameters(prev_tau_0=tau_0, **kw)
    return Parameters(**kw)


# ---------------------------------------------------------------- the spectra

def _pack(quasars, z):
    n = [q[0].size for q in quasars]
    cat = lambda i, dt: np.concatenate([np.asarray(q[i], dtype=dt) for q in quasars]) if sum(n) else np.zeros(0, dt)  # noqa: E731
    return dict(offsets=np.concatenate([[0], np.cumsum(n)]).astype(np.int64), wavelengths=cat(0, np.float64),
                flux=cat(1, np.float64), noise_variance=cat(2, np.float64), pixel_mask=cat(3, np.uint8),
                z_qsos=np.asarray(z, dtype=np.float64))


def _base_quasar(rng, z, p, G, full, mask_fraction):
    lo, hi = p.min_lambda, p.min_lambda + (G - 1) * p.dlambda
    a = lo - 1.0 if full else lo + rng.uniform(-2.0, 3.0)
    b = hi + 1.0 if full else hi - rng.uniform(-2.0, 3.0)
    n = int(rng.integers(12, 55))             # (tight_pixels adds up to 6: 60 at the most)
    rest = a + (b - a) / (n - 1) * (np.arange(n) + rng.uniform(-0.3, 0.3, n))
    nv = 10 ** rng.uniform(-2.0, -0.5, n)
    flux = 1 + 0.3 * np.sin(rest / 3 + rng.uniform(0, 6)) + np.sqrt(nv) * rng.standard_normal(n)
    return [rest * (1 + z), flux, nv, (rng.uniform(size=n) < mask_fraction).astype(np.uint8)]


def _base(rng, p, G, nq, redshifts=None):
    z = rng.uniform(2.2, 4.5, nq) if redshifts is None else np.asarray(redshifts, dtype=np.float64)
    return [_base_quasar(rng, z[i], p, G, i % 2 == 0, 0.0 if i % 2 == 0 else 0.05) for i in range(nq)], z


def _midpoint(rng, p, G, nq, shared=False):
    """nq quasars of G + 1 pixels that bracket every grid point, flux smooth + noise.  ``shared``: one redshift and one
    set of pixel positions for all of them, so that the mean-flux model divides a rest pixel by the same e^-tau in every
    quasar and a constant column stays constant"""
    z = np.full(nq, 3.0) if shared else rng.uniform(2.2, 4.5, nq)
    out = []
    jitter = rng.uniform(-0.3, 0.3, G + 1)
    for i in range(nq):
        rest = p.min_lambda + (np.arange(G + 1) - 0.5 + (jitter if shared else rng.uniform(-0.3, 0.3, G + 1))) * p.dlambda
        fl = 1 + 0.3 * np.sin(rest / 3 + rng.uniform(0, 6)) + 0.1 * rng.standard_normal(G + 1)
        out.append([rest * (1 + z[i]), fl, 10 ** rng.uniform(-2.0, -0.5, G + 1), np.zeros(G + 1, np.uint8)])
    return out, z


def _steps(value, k):
    """value moved by k ulp"""
    v = np.float64(value)
    for _ in range(abs(int(k))):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return v


def problem(cls):
    """(csr, parameters) of a class"""
    stratum, meanflux = cls
    p = parameters(cls)
    G = G_WIDE if stratum.startswith("indicator_edge") else G_SMALL
    rng = np.random.default_rng(BASE_SEED + CLASSES.index(cls))
    cut = p.max_noise_variance
    if stratum == "control":
        z = rng.uniform(2.2, 4.5, NQ)
        z[3::7], z[5::7] = 2.1501, 4.98
        qs, z = _base(rng, p, G, NQ, z)
        qs[1] = [a[:1] for a in qs[1]]
        qs[2][1], qs[2][3] = np.full_like(qs[2][1], np.nan), np.ones_like(qs[2][3])
        qs[-1][2][5:9] = 3.0 * cut
    elif stratum.startswith("offset_flux"):
        scale = float(stratum.split("_")[-1])
        qs, z = _midpoint(rng, p, G, NQ, shared=True)
        for i, q in enumerate(qs):
            q[1] = scale * (1 + 1e-9 * rng.standard_normal(q[1].size))
            q[3] = (rng.uniform(size=q[1].size) < (0.0 if i % 2 == 0 else 0.05)).astype(np.uint8)
    elif stratum == "constant_columns":
        qs, z = _midpoint(rng, p, G, 65, shared=True)
        for i, q in enumerate(qs):
            for g, count in {**CONST_COLUMNS, **ULP_COLUMNS}.items():
                if g in CONST_COLUMNS:
                    v = np.float64(0.1 * (g + 1))
                else:
                    v = _steps(1.0 + g / 64.0, rng.integers(-2, 3))
                q[1][g:g + 2] = v
                if i >= count:
                    q[3][g:g + 2] = 1
    elif stratum == "dynamic_range":
        qs, z = _base(rng, p, G, NQ)
        for i, q in enumerate(qs):
            q[1] = q[1] * 10.0 ** (6 - i % 13)
    elif stratum == "tight_pixels":
        qs, z = _base(rng, p, G, NQ)
        for i, q in enumerate(qs):
            opz, rest = 1 + z[i], q[0] / (1 + z[i])
            points = p.min_lambda + p.dlambda * rng.choice(np.arange(2, G - 2), 3, replace=False)
            points = points[(points > rest[0] + 0.1) & (points < rest[-1] - 0.1)]
            keep = np.all(np.abs(rest[:, None] - points[None, :]) > 0.05, axis=1)
            wl, fl, nv, mk = (a[keep] for a in q)
            for xq, eps in zip(points, TIGHT):
                a, b = rng.uniform(0.2, 0.8, 2)
                sign = 1.0 if rng.uniform() < 0.5 else -1.0
                wl = np.concatenate([wl, [xq * opz * (1 - a * eps), xq * opz * (1 + b * eps)]])
                fl = np.concatenate([fl, [-5.0 * sign, 5.0 * sign]])
                nv = np.concatenate([nv, [0.01, 0.3]])
                mk = np.concatenate([mk, [0, 0]]).astype(np.uint8)
            order = np.argsort(wl)
            qs[i] = [wl[order], fl[order], nv[order], mk[order]]
    elif stratum == "sparse_pairs":
        qs, z = _midpoint(rng, p, G, 9)
        want = np.zeros((9, G), bool)             # the rest pixels a quasar keeps
        want[0, 0:16] = want[1, 0:16] = True
        want[1, 16:32] = want[2, 16:32] = True
        want[3, 32] = want[4, 32] = True
        want[1, 5:7] = False                      # rest pixels 5, 6: quasar 0 alone
        want[1, 20:22] = want[2, 20:22] = False   # rest pixels 20, 21: nobody
        for i, q in enumerate(qs):                # (quasars 5 and 6: all masked; 7: one pixel; 8: none; no complete row)
            ok = np.concatenate([[False], want[i]]) | np.concatenate([want[i], [False]])
            q[3] = (~ok).astype(np.uint8)
            q[2][:] = 0.05
        qs[7] = [a[:1] for a in qs[7]]
        qs[8] = [a[:0] for a in qs[8]]
    elif stratum == "noise_cut":
        qs, z = _midpoint(rng, p, G, NQ)
        for q in qs:
            for g in CUT_COLUMNS:
                q[2][g:g + 2] = _steps(cut, rng.integers(-3, 4))
    elif stratum in ("high_z", "high_z_tau100"):
        qs, z = _base(rng, p, G, NQ, np.where(np.arange(NQ) % 2 == 0, 6.5, 4.98))    # (the complete rows: 6.5)
    elif stratum.startswith("indicator_edge"):
        qs, z = _midpoint(rng, p, G, 70)
    else:
        raise ValueError(stratum)
    return _pack(qs, z), p


def digest(cls, csr, p) -> str:
    """SHA-256 of the bytes of a class's inputs: the CSR arrays, the grid, the cuts and the line table"""
    h = hashlib.sha256()
    for key, dt in (("offsets", np.int64), ("wavelengths", np.float64), ("flux", np.float64), ("noise_variance", np.float64),
                    ("pixel_mask", np.uint8), ("z_qsos", np.float64)):
        h.update(np.ascontiguousarray(csr[key], dtype=dt).tobytes())
    scal = [p.min_lambda, p.max_lambda, p.dlambda, p.lya_wavelength, p.max_noise_variance]
    if cls[1]:
        scal += [p.prev_tau_0, p.prev_beta, float(p.num_forest_lines)] + list(line_wavelengths()) + [row[1] for row in LINES]
    h.update(np.array(scal, dtype=np.float64).tobytes())
    return h.hexdigest()


def check_digest(cls, entry, csr, p):
    got, stored = digest(cls, csr, p), str(entry["sha256"])
    assert got == stored, (f"{class_name(cls)}: the inputs learn_hard_cases.problem forms today (sha256 {got[:16]}...) are not the "
                           f"ones the exact values were computed on ({stored[:16]}...): the recipe or numpy's generators drifted; "
                           "run tests/golden/make_exact_learn_hard.py again")


# ---------------------------------------------------------------- the restatement and its worse variants

def grid_size(p) -> int:
    return int(round((p.max_lambda - p.min_lambda) / p.dlambda)) + 1


def rest_grid(cls, csr, p, interp1=None):
    """R.rest_grid of a class (``interp1``: another interpolation in its place, for the sensitivity legs)"""
    args = (csr, grid_size(p), p.min_lambda, p.dlambda, p.lya_wavelength, p.max_noise_variance) + (
        (p.num_forest_lines, p.prev_tau_0, p.prev_beta) if cls[1] else (0, 0.0023, 3.65))
    if interp1 is None:
        return R.rest_grid(*args)
    keep, R.interp1 = R.interp1, interp1
    try:
        return R.rest_grid(*args)
    finally:
        R.interp1 = keep


def statistics(F, L, N, column_stats=R.column_stats):
    """every block (and the exact-match arrays count, N_pairwise, rows_complete) from the three rest-grid matrices"""
    mu, centered, std, count = column_stats(F)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            cov_p, N_p, _ = R.pca_covariance(centered, False)
            cov_c, _, rows = R.pca_covariance(centered, True)
    return dict(rest_flux=F, lya_1pzs=L, rest_noise=N, mu=mu, centered=centered, std=std, count=count, cov_pairwise=cov_p,
                N_pairwise=N_p, cov_complete=cov_c, rows_complete=rows)


def restated(cls, csr, p):
    return statistics(*rest_grid(cls, csr, p))


# ---------------------------------------------------------------- the measure and the bound

def _relative(a, b, keep):
    sel = keep & np.isfinite(b)
    if not sel.any():
        return 0.0
    with np.errstate(all="ignore"):
        e = np.abs(a[sel] - b[sel]) / np.maximum(np.abs(b[sel]), 1e-300)
    return float(np.where(np.isnan(e), np.inf, e).max())


def _absolute(a, b, keep, scale):
    sel = keep & np.isfinite(b)
    if not sel.any():
        return 0.0
    with np.errstate(all="ignore"):
        e = np.abs(a[sel] - b[sel])
    return float(np.where(np.isnan(e), np.inf, e).max() / scale)


def deviation(got: dict, exact: dict) -> dict:
    """Per block, ``got`` against the fixture entry, scaled as tests/test_gpu_learn.py scales it: the rest grid, mu and
    std relative to themselves; the centred flux relative to the flux scale (max |rest flux|); the covariances relative to
    max |cov|.  Over the finite entries of the exact value that are not excluded (a non-finite ``got`` there is inf)."""
    excl = np.asarray(exact["excluded"], bool)
    pix = ~excl
    col = ~excl.any(axis=0)
    pair = col[:, None] & col[None, :]
    F = exact["rest_flux"]
    flux_scale = np.abs(F[np.isfinite(F)]).max(initial=0.0) or 1.0
    out = dict(rest_flux=_relative(got["rest_flux"], F, pix),
               lya_1pzs=_relative(got["lya_1pzs"], exact["lya_1pzs"], np.ones_like(pix)),
               rest_noise=_relative(got["rest_noise"], exact["rest_noise"], pix),
               mu=_relative(got["mu"], exact["mu"], col), std=_relative(got["std"], exact["std"], col),
               centered=_absolute(got["centered"], exact["centered"], pix & col[None, :], flux_scale))
    for key in ("cov_pairwise", "cov_complete"):
        c = exact[key]
        fin = np.isfinite(c) & pair
        out[key] = _absolute(got[key], c, pair, np.abs(c[fin]).max(initial=0.0) or 1.0)
    return out


def patterns(got: dict, exact: dict) -> list:
    """What has to be equal exactly: NaN placement, +-inf placement with sign, the counts.  Returns the differences."""
    excl = np.asarray(exact["excluded"], bool)
    col = ~excl.any(axis=0)
    bad = []
    for key in BLOCKS:
        a, b = np.asarray(got[key]), np.asarray(exact[key])
        keep = np.ones(b.shape, bool)
        if key in ("rest_flux", "rest_noise", "centered"):
            keep = ~excl & (col[None, :] if key == "centered" else True)
        elif key in ("mu", "std"):
            keep = col
        elif key.startswith("cov"):
            keep = col[:, None] & col[None, :]
        if a.shape != b.shape:
            bad.append(f"{key}: shape {a.shape} against {b.shape}")
            continue
        for what, fa, fb in (("NaN", np.isnan(a), np.isnan(b)), ("+inf", np.isposinf(a), np.isposinf(b)),
                             ("-inf", np.isneginf(a), np.isneginf(b))):
            n = int(((fa != fb) & keep).sum())
            if n:
                bad.append(f"{key}: {what} placement differs in {n} entries")
    for key in ("count", "N_pairwise", "rows_complete"):
        if not np.array_equal(np.asarray(got[key], dtype=np.float64), np.asarray(exact[key], dtype=np.float64)):
            bad.append(f"{key} differs")
    return bad


def tolerance(e_restatement: float, floor: float) -> float:
    return max(TOL_FACTOR * e_restatement, floor)


def failures(cls, e_got: dict, e_rest: dict) -> list:
    """the blocks of ``e_got`` above max(10 x the restatement's, the floor of the block)"""
    floors = FLOORS[cls[1]]
    return [f"{class_name(cls)} {b}: {e_got[b]:.3e} > {tolerance(e_rest[b], floors[b]):.3e} = max(10 x {e_rest[b]:.3e}, {floors[b]:.0e})"
            for b in BLOCKS if not e_got[b] <= tolerance(e_rest[b], floors[b])]


def report(cls, e_got: dict, e_rest: dict) -> str:
    floors = FLOORS[cls[1]]
    ratio = lambda b: e_got[b] / tolerance(e_rest[b], floors[b])  # noqa: E731
    worst = max(BLOCKS, key=ratio)
    return (f"{class_name(cls)}: worst block {worst} ({e_got[worst]:.1e} against a bound of "
            f"{tolerance(e_rest[worst], floors[worst]):.1e});  e_restatement / e_gpu  "
            + "  ".join(f"{b} {e_rest[b]:.1e} {e_got[b]:.1e}" for b in BLOCKS))


# ---------------------------------------------------------------- the fixture

KEYS = BLOCKS + ("count", "N_pairwise", "rows_complete", "excluded", "sha256")


def load_fixture(golden) -> dict:
    """{class name: {key: array}} of both files"""
    out = {}
    for fname in FIXTURES:
        z = golden(fname)
        for full in z.files:
            name, key = full.split("/", 1)
            out.setdefault(name, {})[key] = z[full]
    return out


# ---------------------------------------------------------------- the GPU's blocks, and the existing bounds

def evaluate(csr, p, meanflux: bool) -> dict:
    """every block (and count, N_pairwise, N_complete, rows_complete) from csrc/learn_kernels.hpp, on one handle"""
    from gp_dla_detection_amd.training import TrainingSet
    t = TrainingSet.from_spectra(csr, p, meanflux)
    try:
        F, L, N = t.download()
        mu, std, count = t.column_stats()
        centered, _, _ = t.download()
        cov_p, N_p, _ = t.pca_covariance(False, with_count=True)
        cov_c, N_c, rows = t.pca_covariance(True, with_count=True)
    finally:
        t.close()
    return dict(rest_flux=F, lya_1pzs=L, rest_noise=N, mu=mu, centered=centered, std=std, count=count, cov_pairwise=cov_p,
                N_pairwise=N_p, cov_complete=cov_c, N_complete=N_c, rows_complete=rows)


def against_restatement(got: dict, ref: dict, meanflux: bool) -> list:
    """``got`` held to the restatement's blocks ``ref`` as tests/test_gpu_learn.py holds it (FLOORS), with exact counts
    and exact NaN / +-inf placement.  Returns what differs."""
    ref = dict(ref, excluded=np.zeros(ref["rest_flux"].shape, bool))
    bad = patterns(got, ref)
    e = deviation(got, ref)
    bad += [f"{b}: {e[b]:.3e} > {FLOORS[meanflux][b]:.0e}" for b in BLOCKS if not e[b] <= FLOORS[meanflux][b]]
    if "N_complete" in got and not np.array_equal(got["N_complete"], np.full_like(got["N_complete"], float(ref["rows_complete"]))):
        bad.append("N_complete is not the number of complete rows everywhere")
    for key in ("cov_pairwise", "cov_complete"):
        if not np.array_equal(got[key], got[key].T, equal_nan=True):
            bad.append(f"{key} is not symmetric")
    return bad
