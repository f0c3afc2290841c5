"""Training sets on which the arithmetic of the training objective is hard (plain module, like hard_conditioning_cases.py
and continuum_hard_cases.py: the fixture generator tests/golden/make_exact_training_hard.py, test_training_hard.py and
test_gpu_training_hard.py import it, nothing else does).

Every other statement about the objective (objective.m:12-75 over spectrum_loss.m:14-76) rests on
``test_training.training_problem``: independent columns of amplitude 0.3 x 0.8^j, noise variances 10^U(-3,-1), log omega
in (-3,-2) and the three scalars at the prior means, where B_q = I + M' D^-1 M has a condition number of ~1e3 and the
as-written fp64 oracle is the yardstick.  ``problem`` generalises that recipe (STRATA): model amplitude, column mixing
and collinearity, a log omega shift, the noise range, which noise the flux is drawn at, a flux factor and shifts of the
three scalars.  The yardstick here is a 50-digit evaluation of the very fp64 inputs (tests/golden/exact_training_hard.npz),
the measure is ``test_training.objective_deviation`` per block, and the bound is ``tolerance``: 10 x what the oracle
attains on the same block, floored at the 1e-9 that ``assert_objective_close`` holds the HIP path to.

    strata      STRATA; every class carries the data edges of ``test_training.with_edge_cases`` at small indices (EDGES)
    classes     (stratum, nq, G, k, lines): CLASSES -- the smallest shapes that are ragged in the 16-quasar, 16-pixel and
                4-step tilings and reach both kernels of each rank class; lines = 0 is objective.m, 6 the Lyman-series
                objective on the library's table, 31 on the caller's
    restatement ``gpu_algebra``: the forms the HIP kernels use (Woodbury pieces; B^-1 or, as before these tests, T = B^-1 + z z'
                contracted for diag K^-1), in fp64 numpy

In ``opaque_forest`` e^-tau is exactly 0 in fp64 (1e-2600 at 50 digits): the data's share of the log tau0 and log beta
entries is nothing, and the prior terms of objective.m:59-71 ARE those two entries.  (log beta is moved off the prior mean
by 0.05 in this stratum alone: at the mean its prior term is the rounding residual of exp(log 3.65), 1e-14, of which no
fp64 evaluation has a digit.)  In ``thin_forest`` tau is 1e-13 and the two entries are the data's, 1e-8 and smaller; the
prior on log tau0 is a thousandth of its entry.  Both strata are there for f, M, log omega and log c0.  No stratum lets
(1+z)^beta overflow: spectrum_loss.m:69 is inf x 0 = NaN there in the reference as well.

``omega_large`` and ``opaque_forest`` are the two hard strata on which noise variances rounded to float32 are not seen:
omega2 sf^2 (sf >= c0 with omega2 ~ 20; sf = 1 + c0) is 30 .. 1e6 times the noise, 1000 times at the median, and what
the rounding moves stays under the floor of 1e-9 (0.01 and 0.9 of it, measured on the oracle).  There the sensitivity leg
of test_training_hard.py rounds log omega instead (NOISE_BLIND_STRATA).
"""
from __future__ import annotations

import hashlib
import zipfile

import numpy as np

from gp_dla_detection_amd import _lyman_data

TOL_FACTOR = 10.0              # the project's convention (hard_conditioning_cases.TOL_FACTOR)
TOL_FLOOR = 1e-9               # assert_objective_close's rtol
ORACLE_CAP = 1e-6              # a condition on the choice of inputs: the oracle stays this close to exact in every block
FD_STEP = 1e-15                # central differences of the exact value
FD_RTOL = 1e-20
DPS = 50                       # digits of the yardstick
GUARD = 20                     # guard digits the generator works with on top of them (its docstring says why)
FD_ATOL = 1e-40                # x |f|: what the difference quotient cannot resolve
FIXTURES = ("exact_training_hard.npz", "exact_training_hard_k33_k40.npz")
LYA = 1215.6701

# the data edges (test_training.with_edge_cases, at indices every class has)
ALL_NAN_QUASAR, ONE_PIXEL_QUASAR, ONE_PIXEL, GROUP_QUASAR, GROUP, MISSING_PIXEL, QUIET_PIXEL = 3, 5, 20, 7, 2, 50, 70
MISSING = 0.1

LN = np.log
# stratum -> amp (x 0.8^j), mix, collinear, log omega shift, shift of the noise exponent U(-3,-1), the noise the flux is drawn at
# ("own": the stratum's, "shipped": 10^U(-3,-1)), flux factor, shifts of (log c0, log tau0, log beta), quiet pixel, few pixels
_BASE = dict(amp=0.3, mix=0.0, collinear=False, omega_shift=0.0, noise_shift=0.0, flux_noise="own", factor=1.0,
             scalars=(0.0, 0.0, 0.0), quiet=False, few=False)
_HIGH = dict(_BASE, amp=1.0, noise_shift=-3.0)
_CORR = dict(_HIGH, amp=5.0, mix=0.5, collinear=True, flux_noise="shipped", factor=0.6)
STRATA = {
    "control": _BASE,
    "high_snr": _HIGH,
    "high_snr_misfit": dict(_HIGH, flux_noise="shipped"),
    "correlated": _CORR,
    "bad_continuum": dict(_CORR, factor=1.2),
    "quiet_pixel": dict(_BASE, amp=1.0, noise_shift=-1.0, quiet=True),
    "omega_tiny": dict(_HIGH, omega_shift=-12.0),
    "omega_large": dict(_HIGH, omega_shift=4.0),
    "opaque_forest": dict(_HIGH, scalars=(0.0, float(LN(1e5)), 0.05)),
    "thin_forest": dict(_HIGH, scalars=(0.0, -float(LN(1e12)), 0.0)),
    "few_pixels": dict(_CORR, few=True),
}
HARD_STRATA = tuple(s for s in STRATA if s != "control")
FOREST_STRATA = ("opaque_forest", "thin_forest")
NOISE_BLIND_STRATA = ("omega_large", "opaque_forest")
BINV_LOWERS_LOG_OMEGA = ("high_snr", "quiet_pixel", "omega_tiny")

SHAPE20, SHAPE40, SHAPE33 = (37, 203, 20), (24, 131, 40), (21, 131, 33)
CLASSES = (
    tuple((s,) + SHAPE20 + (0,) for s in STRATA)                                          # k_train_factor<20>, k_train_core
    + tuple((s,) + SHAPE40 + (0,) for s in ("correlated", "bad_continuum", "high_snr", "few_pixels"))  # factor16<40>, core_wide
    + tuple((s,) + SHAPE33 + (0,) for s in ("correlated", "omega_tiny"))
    + (("correlated",) + SHAPE20 + (6,), ("high_snr",) + SHAPE33 + (31,))                 # the LY = true kernels
)
assert len(CLASSES) == 19

# class -> (flux factor, seed) where they are not the stratum's factor and BASE_SEED + the class's place in CLASSES.
# The oracle has to stay within ORACLE_CAP of the exact value in every block of every class (test_training_hard.py);
# a class that did not at its first draw got another seed or a softer flux factor, judged by the oracle alone:
#   class                          first draw: worst block of the oracle      choice
#   (none: every class met the cap at its first draw; worst 7.5e-07, few_pixels-37x203x20-l0 M[:, 1])
BASE_SEED = 700
TUNING: dict = {}


def class_name(cls) -> str:
    stratum, nq, G, k, lines = cls
    return f"{stratum}-{nq}x{G}x{k}-l{lines}"


def fixture_of(cls) -> str:
    return FIXTURES[0] if cls[3] <= 20 else FIXTURES[1]


def series_tables():
    """(wavelengths [Angstrom], oscillator strengths) of the library's Lyman lines (set_parameters_multi.m:77-108)"""
    return (np.array([line[0] * 1e8 for line in _lyman_data.LINES]), np.array([line[1] for line in _lyman_data.LINES]))


def problem(cls):
    """(x, F, L1, NV) of a class.  With the ``control`` settings the draws are ``training_problem``'s, bit for bit."""
    stratum, nq, G, k, lines = cls
    s = STRATA[stratum]
    factor, seed = TUNING.get(cls, (s["factor"], BASE_SEED + CLASSES.index(cls)))
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((G, k)) * s["amp"] * 0.8 ** np.arange(k)
    lo = rng.uniform(-3, -2, G)
    z = rng.standard_normal((nq, k))
    L1 = 1 + rng.uniform(1.5, 3.0, (nq, G))
    E = rng.uniform(-3, -1, (nq, G))
    draw = rng.standard_normal((nq, G))
    missing = rng.uniform(size=(nq, G)) < MISSING
    if s["mix"]:
        Z = np.random.default_rng(5).standard_normal((k, k))
        M = M @ (np.eye(k) + s["mix"] * Z / np.sqrt(k))
    if s["collinear"]:
        M[:, 1] = M[:, 0] * (1 + 1e-3) + 1e-3 * M[:, 1]
    NV = 10 ** (E + s["noise_shift"]) if s["noise_shift"] else 10 ** E
    if s["quiet"]:
        NV[:, QUIET_PIXEL] = 1e-10
    F = z @ M.T + np.sqrt(NV if s["flux_noise"] == "own" else 10 ** E) * draw
    if factor != 1.0:
        F = F * factor
    F[missing] = np.nan
    if s["few"]:        # every other quasar keeps fewer valid pixels than k
        few = np.random.default_rng(seed + 1000)
        for q in range(1, nq, 2):
            keep = few.choice(G, size=int(few.integers(k // 2, k)), replace=False)
            row = np.full(G, np.nan)
            row[keep] = F[q, keep]
            F[q] = row
    F[ALL_NAN_QUASAR] = np.nan
    keep = F[ONE_PIXEL_QUASAR, ONE_PIXEL]
    F[ONE_PIXEL_QUASAR] = np.nan
    F[ONE_PIXEL_QUASAR, ONE_PIXEL] = 0.0 if np.isnan(keep) else keep
    F[GROUP_QUASAR, 16 * GROUP:16 * GROUP + 16] = np.nan
    F[:, MISSING_PIXEL] = np.nan
    if lines:           # test_training.lyseries_problem's wavelength grid: the last column is 1 + z_qso
        rest = np.linspace(911.75, LYA, G)
        L1 = (1 + np.random.default_rng(seed).uniform(2.1, 4.5, nq))[:, None] * rest[None, :] / LYA
    lo = lo + s["omega_shift"] if s["omega_shift"] else lo
    scal = np.array([LN(0.1), LN(0.0023), LN(3.65)]) + np.array(s["scalars"])
    x = np.concatenate([M.ravel(order="F"), lo, scal])
    return x, F, L1, NV


def digest(cls, x, F, L1, NV) -> str:
    """SHA-256 of the bytes of a class's inputs (and of the line tables a Lyman-series class uses)"""
    h = hashlib.sha256()
    for a in (x, F, L1, NV) + (tuple(t[:cls[4]] for t in series_tables()) if cls[4] else ()):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def run_oracle(oracle, cls, x, F, L1, NV):
    if cls[4]:
        return oracle.objective_lyseries(x, F, L1, NV, cls[4], *series_tables())
    return oracle.objective(x, F, L1, NV)


def split(x, G, k):
    return x[:G * k].reshape((G, k), order="F"), x[G * k:G * (k + 1)], x[G * (k + 1):]


def optical_depth(cls, tau_0, beta, l1_row):
    """spectrum_loss.m:22 / spectrum_loss_lyseries.m:22-39 on one quasar's full row, in fp64"""
    od = tau_0 * l1_row ** beta
    if cls[4]:
        wl, fs = series_tables()
        for i in range(1, cls[4]):
            lyman = wl[0] * l1_row / wl[i]
            lyman = lyman * (lyman <= l1_row[-1])
            od = od + tau_0 * wl[i] * fs[i] / (wl[0] * fs[0]) * lyman ** beta
    return od


def cond_B(cls, x, F, L1, NV, q: int = 0) -> float:
    G, k = cls[2], cls[3]
    M, lo, (lc, lt, lb) = split(x, G, k)
    ok = ~np.isnan(F[q])
    sf = 1 - np.exp(-optical_depth(cls, np.exp(lt), np.exp(lb), L1[q])) + np.exp(lc)
    d = (NV[q] + np.exp(2 * lo) * sf ** 2)[ok]
    return float(np.linalg.cond(np.eye(k) + M[ok].T @ (M[ok] / d[:, None])))


def prior_terms(x):
    """objective.m:59-71: what is added to the log tau0 and log beta entries"""
    t0, b0 = np.exp(x[-2]), np.exp(x[-1])
    return t0 * (t0 - 0.0023) / 0.0007 ** 2, b0 * (b0 - 3.65) / 0.21 ** 2


def gpu_algebra(cls, x, F, L1, NV, contract: str = "Binv"):
    """(f, g) by the forms of csrc/training_mfma_kernels.hpp, in fp64 numpy: K^-1 M = D^-1 M B^-1, y'K^-1 y = Sum y^2 w - y'y
    with y = L^-1 t, z = L^-T y, dM = w m'T - u z' with T = B^-1 + z z', and (K^-1)_pp = w - w^2 X with X = m'B^-1 m
    (train_core_tile).  ``contract`` = "T": what the core did before these tests, X = m'T m and (K^-1)_pp = w - w^2 X +
    w^2 Y^2 with Y = m'z -- the form that cancels."""
    G, k = cls[2], cls[3]
    M, lo, (lc, lt, lb) = split(x, G, k)
    om, c_0, tau_0, beta = np.exp(2 * lo), np.exp(lc), np.exp(lt), np.exp(lb)
    f, dM, dlo, dsc = 0.0, np.zeros((G, k)), np.zeros(G), np.zeros(3)
    for q in range(F.shape[0]):
        ok = ~np.isnan(F[q])
        if not ok.any():
            continue
        y, m, lz = F[q, ok], M[ok], np.log(L1[q, ok])
        od = optical_depth(cls, tau_0, beta, L1[q])[ok]
        ab = np.exp(-od)
        sf = 1 - ab + c_0
        an = om[ok] * sf * sf
        d = NV[q, ok] + an
        w = 1 / d
        u = w * y
        B = np.eye(k) + m.T @ (m * w[:, None])
        t = m.T @ u
        L = np.linalg.cholesky(B)
        Linv = np.linalg.solve(L, np.eye(k))                  # (both factor kernels: L^-1 by substitution, B^-1 = L^-T L^-1,
        Binv = Linv.T @ Linv                                  #  t'z = v'v with v = L^-1 t)
        v = Linv @ t
        zq = Linv.T @ v
        T = Binv + np.outer(zq, zq)
        f += 0.5 * (np.sum(y * y * w) - v @ v + np.sum(np.log(d)) + 2 * np.sum(np.log(np.diag(L))) + y.size * 1.83787706640934534)
        dM[ok] += (m @ T) * w[:, None] - np.outer(u, zq)
        Y = m @ zq
        if contract == "T":
            diag = w - w * w * np.einsum("pi,ij,pj->p", m, T, m) + w * w * Y * Y
        else:
            diag = w - w * w * np.einsum("pi,ij,pj->p", m, Binv, m)
        core = (u - w * Y) ** 2 - diag
        dlo[ok] -= an * core
        da = om[ok] * sf * od * ab
        dsc -= np.array([np.sum(core * c_0 * om[ok] * sf), np.sum(core * da), np.sum(core * da * lz * beta)])
    dsc[1:] += prior_terms(x)
    return f, np.concatenate([dM.ravel(order="F"), dlo, dsc])


# ---------------------------------------------------------------- the bound

def tolerance(e_oracle: float) -> float:
    return max(TOL_FACTOR * e_oracle, TOL_FLOOR)


def failures(name: str, e_got: dict, e_oracle: dict) -> list:
    """the blocks of ``e_got`` (objective_deviation against exact) above max(10 x the oracle's, 1e-9)"""
    return [f"{name} {b}: {e_got[b]:.3e} > {tolerance(e_oracle[b]):.3e} = max(10 x {e_oracle[b]:.3e}, 1e-9)"
            for b in e_got if not e_got[b] <= tolerance(e_oracle[b])]


def ratio(e, e_ref):
    return e / e_ref if e_ref > 0 else float("inf")


def summary(e: dict, k: int) -> dict:
    """f, the worst M column (and which), log omega and the three scalars of a per-block dict"""
    worst = max(range(k), key=lambda c: e[f"M[:, {c}]"])
    return {"f": e["f"], "M": e[f"M[:, {worst}]"], "M_col": worst, "log_omega": e["log_omega"], "log_c0": e["log_c0"],
            "log_tau0": e["log_tau0"], "log_beta": e["log_beta"]}


# ---------------------------------------------------------------- the fixture

FD_M, FD_OMEGA = 8, 4


def fd_indices(cls):
    """The entries of x whose exact derivative is checked by central differences: FD_M random entries of M, FD_OMEGA of
    log omega (pixels somebody observes) and the scalars -- without log beta in a Lyman-series class, whose
    as-written entry (spectrum_loss_lyseries.m:90) is not a derivative."""
    _, nq, G, k, lines = cls
    rng = np.random.default_rng(9000 + CLASSES.index(cls))
    pixels = np.setdiff1d(np.arange(G), [MISSING_PIXEL])
    idx = [int(rng.choice(pixels)) + G * int(rng.integers(k)) for _ in range(FD_M)]
    idx += [G * k + int(p) for p in rng.choice(pixels, FD_OMEGA, replace=False)]
    idx += [G * (k + 1) + i for i in range(2 if lines else 3)]
    return np.array(idx, dtype=np.int64)


def save_npz(path, arrays: dict):
    """np.savez_compressed with fixed member dates, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def load_fixture(golden) -> dict:
    """{class name: {key: array}} of both files"""
    out = {}
    for fname in FIXTURES:
        z = golden(fname)
        for full in z.files:
            name, key = full.split("/", 1)
            out.setdefault(name, {})[key] = z[full]
    return out


def check_digest(cls, entry, inputs):
    got, stored = digest(cls, *inputs), str(entry["sha256"])
    assert got == stored, (f"{class_name(cls)}: the inputs training_hard_cases.problem forms today (sha256 {got[:16]}...) are not "
                           f"the ones the exact values were computed on ({stored[:16]}...): the recipe or numpy's generators "
                           "drifted; run tests/golden/make_exact_training_hard.py again")
