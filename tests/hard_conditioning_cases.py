"""Inputs on which the arithmetic of the sweeps is hard (plain module, like production_shapes.py: the fixture
generator tests/golden/make_exact_hard.py, test_hard_conditioning.py and test_gpu_hard_conditioning.py import it,
nothing else does).

Every other parity statement of the project rests on ``synthetic.make_model`` (orthogonal, small columns) and on
noise variances of 10^U(-3,-1): there the capacitance matrix B = I + M' D^-1 M of log_mvnpdf_low_rank.m:22-26 is
nearly diagonal (cond ~ 1e2), |log-likelihood| is a few thousand and an fp64 evaluation is ~1e-12 from the true
value.  Here: S/N of 100 .. 1000 per pixel, a model whose columns are mixed, five times larger and (two of them)
nearly collinear, and fluxes the model does not fit -- cond(B) up to 1e7, |log-likelihood| up to 1e7, where a
faithful fp64 evaluation of the reference's own formulae is already 1e-9 .. 1e-6 from the true value.  The yardstick
there is the 50-digit value (tests/golden/make_exact.py::exact_log_mvnpdf) and the bound is set by what the
as-written fp64 oracle attains on the same inputs, not by a fixed 1e-8.

    strata      one quasar each (the same sightline: 131 in-range pixels = 33 K-steps, one run of five masked
                pixels; model, noise and flux as the table in STRATA says)
    classes     (stratum, driver, k, Voigt lines): which kernel sweeps it (CLASSES)
    low-rank    hand-made (y, mu, M, d) for the stand-alone function at k = 20, 40, 41, 64 and cond(B) ~ 1e4, 1e8, 1e12

Hot loops: process_qsos.m:185-199, process_qsos_multiple_dlas_meanflux.m:340-381, log_mvnpdf_low_rank.m:11-32.
"""
from __future__ import annotations

import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd._lyman import LINES
from gp_dla_detection_amd.parameters import MultiParameters, Parameters
from production_shapes import in_range, mask_pixels

N_PIX = 131                    # in-range pixels: 33 K-steps, past the 32-step ring wrap and the chunk edges
S = 65                         # null slot in the ordinary place, a partly filled last wave
EDGE = 2                       # synthetic.make_spectrum: pixels in front of the modelled range
INDEX = 8812                   # the sightline (even: no DLA injected into the flux)
MASK_RUN = (EDGE + 40, EDGE + 45)
FEW_KEPT = 24
NOISE_SEED, FLUX_SEED, BSI_SEED = 611, 612, 977
TOL_FLOOR = 1e-9               # the bound the two older exact fixtures hold the HIP path to
TOL_FACTOR = 10.0              # the project's convention (R.continuum_tolerance, posterior_restatement.tolerances)
ORACLE_CAP = 1e-6              # a condition on the choice of inputs: the oracle itself stays this close to exact
LINE_A = [LINES[j][0] * 1e8 for j in range(3)]   # Angstrom

# stratum -> (model: None = as shipped, else (amp, mix, omega_shift); hard noise; flux; flux factor)
#   flux "model":   what make_spectrum drew from the stratum's model at the SHIPPED noise level, 10^U(-3,-1)
#   flux "fitted":  drawn from the stratum's model AT the stratum's own noise
STRATA = {
    "control": (None, False, "model", 1.0),
    "high_snr": ((1.0, 0.0, -3.0), True, "fitted", 1.0),
    "high_snr_misfit": ((1.0, 0.0, -3.0), True, "model", 1.0),
    "correlated": ((5.0, 0.5, -3.0), True, "model", 0.6),
    "bad_continuum": ((5.0, 0.5, -3.0), True, "model", 1.2),     # x 2
    "saturated": ((5.0, 0.5, -3.0), True, "model", 0.6),
    "few_pixels": ((5.0, 0.5, -3.0), True, "model", 1.0),
}
HARD_STRATA = tuple(s for s in STRATA if s != "control")
ON_CORRELATED_MODEL = ("correlated", "bad_continuum", "saturated", "few_pixels")

# (stratum, driver, k, Voigt lines): the kernel is chosen by (driver, k, lines)
CLASSES = (
    ("control", "single", 20, 3),           # k_sweep_slim<3>
    ("high_snr", "single", 20, 3),
    ("high_snr_misfit", "single", 20, 3),
    ("correlated", "single", 20, 3),
    ("bad_continuum", "single", 20, 3),
    ("saturated", "single", 20, 3),
    ("correlated", "single", 20, 31),       # k_sweep_slim<0>
    ("correlated", "single", 40, 3),        # k_sweep_split_slim
    ("bad_continuum", "single", 40, 3),
    ("correlated", "single", 33, 3),
    ("few_pixels", "single", 40, 3),
    ("correlated", "multi", 20, 3),         # k_profiles, k_sweep_multi_slim<1>, <2>, the sub-DLA sweep
    ("saturated", "multi", 20, 3),
)
MAX_DLAS = 2

# (stratum, k) -> (flux factor, seed of the noise variances) where they are not the stratum's factor and NOISE_SEED.
# The oracle has to stay within ORACLE_CAP of the exact value on all 66 values of a class (test_hard_conditioning.py).
# With every sample of the box evaluated -- log N_HI up to 23 laid over an unabsorbed flux of S/N 1000 -- its worst
# error is 1e-6 .. 1.5e-5 at the factors 1 and 2 first tried, set by max |ll| ~ 1e7 and by which pixels are the quiet
# ones; the flux factor was softened to 0.6 (bad continuum: twice that) and the noise draw chosen, per class, among
# the seeds 611 .. 638 so that the oracle (never the GPU, which was unmeasured then) meets the cap.
TUNING = {
    ("correlated", 20): (0.6, 614),
    ("bad_continuum", 20): (1.2, 618),
    ("saturated", 20): (0.6, 613),
    ("correlated", 33): (0.6, 617),
    ("correlated", 40): (0.7, 629),
    ("bad_continuum", 40): (0.8, 613),   # x 2 is out of reach at k = 40: 2e-6 .. 2.7e-5 at factors 1.2 .. 1.6, 36 draws
}


def class_name(cls) -> str:
    stratum, driver, k, lines = cls
    return f"{stratum}-{driver}-k{k}-l{lines}"


def hard_model(k: int, amp: float, mix: float, omega_shift: float) -> dict:
    """``make_model(k)`` with M <- amp M A, A = I + mix Z / sqrt(k) (Z standard normal), column 1 then made
    collinear with column 0 to 1e-3, and log omega shifted."""
    model = dict(synthetic.make_model(k))
    Z = np.random.default_rng(5).standard_normal((k, k))
    M = amp * (np.asarray(model["M"]) @ (np.eye(k) + mix * Z / np.sqrt(k)))
    M[:, 1] = M[:, 0] * (1 + 1e-3) + 1e-3 * M[:, 1]
    model["M"] = np.asfortranarray(M)
    model["log_omega"] = np.asarray(model["log_omega"]) + omega_shift
    return model


def stratum_model(stratum: str, k: int) -> dict:
    spec = STRATA[stratum][0]
    return synthetic.make_model(k) if spec is None else hard_model(k, *spec)


def quasar(stratum: str, k: int, factor: float | None = None, noise_seed: int = NOISE_SEED) -> dict:
    _, hard_noise, flux_kind, stratum_factor = STRATA[stratum]
    factor = stratum_factor if factor is None else factor
    model = stratum_model(stratum, k)
    sp = synthetic.make_spectrum(INDEX, N_PIX, model)
    sp = {key: (np.array(v) if isinstance(v, np.ndarray) else v) for key, v in sp.items()}
    wl = sp["wavelengths"]
    if hard_noise:
        sp["noise_variance"] = 10.0 ** np.random.default_rng(noise_seed).uniform(-6.0, -4.0, size=wl.size)
    if flux_kind == "fitted":      # as make_spectrum draws it, at this noise
        rest = wl / (1 + sp["z_qso"])
        grid = model["rest_wavelengths"]
        mu = np.interp(rest, grid, model["mu"])
        Mi = np.stack([np.interp(rest, grid, model["M"][:, c]) for c in range(k)], 1)
        omega2 = np.exp(2 * np.interp(rest, grid, model["log_omega"]))
        rng = np.random.default_rng(FLUX_SEED)
        sp["flux"] = (mu + Mi @ rng.standard_normal(k)
                      + np.sqrt(omega2 * 0.04 + sp["noise_variance"]) * rng.standard_normal(wl.size))
    sp["flux"] = sp["flux"] * factor
    inside = np.flatnonzero(in_range(sp))
    assert inside.size == N_PIX
    if stratum == "few_pixels":
        keep = inside[6 + 5 * np.arange(FEW_KEPT)]
        mask_pixels(sp, np.setdiff1d(inside, keep))
    else:
        mask_pixels(sp, np.arange(*MASK_RUN))
    sp["stratum"] = stratum
    return sp


def search_range(sp, p: Parameters | None = None):
    p = p or Parameters()
    kept = sp["wavelengths"][in_range(sp) & (sp["pixel_mask"] == 0)]
    return p.min_z_dla(kept, sp["z_qso"]), p.max_z_dla(kept, sp["z_qso"])   # process_qsos.m:159-160


DEEP = ((0, 26.3), (1, 26.2), (0, 25.0), (2, 25.0))   # (line, log N_HI)
NUM_PLACED = 8 + len(DEEP)


def placed_saturated(sp):
    """(z offset, log N_HI) of the placed samples.  Eight as physical as the sample box allows: the core of each of
    the three lines on the pixel in the middle of what it can reach, at log N_HI = 23 and 22.5, and the Lyman-alpha
    core a quarter and three quarters of the way, at 23.  On these 2.3 A (rest) pixels their broadened absorption
    bottoms out near 1e-31 (three raw pixels under 1e-260, spread by the seven-tap instrument profile), so four more
    (DEEP) carry column densities far beyond the box: at log N_HI = 26.3 the trough is wider than half the spectrum,
    exactly 0 inside and denormal on its rim -- the rows a kernel multiplies by 0 and by 1e-310."""
    lo, hi = search_range(sp)
    wl = sp["wavelengths"][in_range(sp)]
    mid, off, lognhi = [], [], []
    for j, line in enumerate(LINE_A):
        z0 = wl / line - 1
        ok = np.flatnonzero((z0 > lo + 0.02 * (hi - lo)) & (z0 < hi - 0.02 * (hi - lo)))
        assert ok.size, j
        mid.append((z0[ok[ok.size // 2]] - lo) / (hi - lo))
        for n in (23.0, 22.5):
            off.append(mid[j])
            lognhi.append(n)
        if j == 0:
            quarters = [(z0[ok[ok.size // 4]] - lo) / (hi - lo), (z0[ok[3 * ok.size // 4]] - lo) / (hi - lo)]
    off = np.array(off + quarters + [mid[j] for j, _ in DEEP])
    lognhi = np.array(lognhi + [23.0, 23.0] + [n for _, n in DEEP])
    assert off.size == NUM_PLACED and ((off >= 0) & (off < 1)).all()
    return off, lognhi


def sample_table(stratum: str, sp) -> dict:
    s = {key: np.array(v) for key, v in synthetic.make_samples(S).items()}
    if stratum == "saturated":      # placed samples overwrite the leading entries
        off, lognhi = placed_saturated(sp)
        s["offset_samples"][:off.size] = off
        s["log_nhi_samples"][:off.size] = lognhi
        s["nhi_samples"][:off.size] = 10.0 ** lognhi
    return s


def base_sample_inds(stratum: str) -> np.ndarray:
    """[MAX_DLAS - 1, S], 1-based: the second absorber of every sample, supplied by the caller; in ``saturated``
    each placed sample is paired with another placed one"""
    bsi = np.random.default_rng(BSI_SEED).integers(1, S + 1, size=(MAX_DLAS - 1, S)).astype(np.uint32)
    if stratum == "saturated":
        bsi[0, :NUM_PLACED] = (np.arange(NUM_PLACED) + 5) % NUM_PLACED + 1
    return bsi


def params_of(cls):
    _, driver, _, lines = cls
    return MultiParameters(max_dlas=MAX_DLAS, num_lines=lines) if driver == "multi" else Parameters(num_lines=lines)


def build_case(cls) -> dict:
    stratum, driver, k, lines = cls
    sp = quasar(stratum, k, *TUNING.get((stratum, k), ()))
    return dict(cls=cls, name=class_name(cls), model=stratum_model(stratum, k), spectrum=sp,
                samples=sample_table(stratum, sp), params=params_of(cls),
                bsi=base_sample_inds(stratum) if driver == "multi" else None)


def run_oracle(oracle, case, noise_variance=None, dump=True) -> dict:
    """The oracle on a case: the driver's result plus, flattened, the values the comparison uses --
    ``null``, ``dla`` [S] and, multi-DLA, ``lls`` [S] and ``dla2`` [S] (NaN where the pair is closer than
    min_z_separation), as the drivers report them (the multi-DLA ones carry - log S, multi :359-361)."""
    from oracle.oracle import OracleParams
    sp, sm, p = case["spectrum"], case["samples"], case["params"]
    nv = sp["noise_variance"] if noise_variance is None else noise_variance
    if case["bsi"] is None:
        r = oracle.process_spectrum(case["model"], sm["offset_samples"], sm["nhi_samples"], sp["wavelengths"],
                                    sp["flux"], nv, sp["pixel_mask"], sp["z_qso"],
                                    params=OracleParams(num_lines=p.num_lines), num_threads=0, dump=dump)
        assert r["rc"] == 0
        r.update(null=r["log_likelihood_no_dla"], dla=r["sample_log_likelihoods_dla"])
    else:
        r = oracle.process_spectrum_multi(
            case["model"], sm["offset_samples"], sm["nhi_samples"], sm["log_nhi_samples"], sm["lls_nhi_samples"],
            case["bsi"], sp["wavelengths"], sp["flux"], nv, sp["pixel_mask"], sp["z_qso"],
            params=OracleParams(num_lines=p.num_lines), max_dlas=p.max_dlas, num_forest_lines=p.num_forest_lines,
            min_z_separation=p.min_z_separation, prev_tau_0=p.prev_tau_0, prev_beta=p.prev_beta, dump=dump)
        assert r["rc"] == 0
        r.update(null=r["log_likelihood_no_dla"], dla=r["sample_log_likelihoods_dla"][:, 0],
                 lls=r["sample_log_likelihoods_lls"], dla2=r["sample_log_likelihoods_dla"][:, 1])
    return r


TABLES = ("dla", "lls", "dla2")


def absorption_tables(oracle, case, run) -> dict:
    """What the drivers multiply the model rows by, on the in-range pixels (masked or not), per table:
    process_qsos.m:187-188; multi :343-351 (the product of the two absorbers' profiles), :365-368"""
    sm, lines = case["samples"], case["params"].num_lines
    pad, z = run["padded_wavelengths"], run["sample_z_dlas"]
    out = {"dla": np.stack([oracle.voigt(pad, float(z[i]), float(sm["nhi_samples"][i]), lines) for i in range(S)])}
    if case["bsi"] is not None:
        out["lls"] = np.stack([oracle.voigt(pad, float(z[i]), float(sm["lls_nhi_samples"][i]), lines) for i in range(S)])
        out["dla2"] = np.stack([out["dla"][i] * out["dla"][int(case["bsi"][0, i]) - 1] for i in range(S)])
    return out


def lowrank_inputs(case, run, absorption=None):
    """(y, mu, M, d) process_qsos.m:149-151 (``absorption`` None) / :190-198 hands to log_mvnpdf_low_rank"""
    sp = case["spectrum"]
    inside = in_range(sp)
    mask = sp["pixel_mask"].astype(bool)
    y, nv = sp["flux"][inside & ~mask], sp["noise_variance"][inside & ~mask]
    mu, M, om2 = run["this_mu"], run["this_M"], run["this_omega2"]
    if absorption is None:
        return y, mu, M, om2 + nv
    a = absorption[~mask[inside]]
    return y, mu * a, M * a[:, None], om2 * a ** 2 + nv


def shift_of(case) -> float:
    """what the driver subtracts from a sample's log-likelihood: log S in the multi-DLA driver (multi :359-361)"""
    return float(np.log(S)) if case["bsi"] is not None else 0.0


def cond_B(y, mu, M, d) -> float:
    B = np.eye(M.shape[1]) + M.T @ (M / d[:, None])
    return float(np.linalg.cond(B))


# ---------------------------------------------------------------- the stand-alone low-rank function

LOWRANK_N = 128
LOWRANK_KS = (20, 40, 41, 64)
LOWRANK_CONDS = (1e4, 1e8, 1e12)
LOWRANK_SEED = 20270


def lowrank_case(k: int, cond: float):
    """(y, mu, M, d), n = 128: M standard normal with column 1 collinear with column 0 to 1e-6, d in U(0.5, 1.5)
    scaled down so that the largest eigenvalue of M' D^-1 M (about 2.6 n over the scale) is about ``cond`` -- the
    smallest of B is 1 to within the collinear pair's 1e-12 share -- and y one noise sigma plus a thousandth of a
    draw of the model off the mean.  (With a whole draw of the model in y the oracle itself is 2 .. 17 from the exact
    value at cond 1e12: y' D^-1 y ~ 1e13 cancels against the Woodbury term.  Without it the oracle's error there is
    1e-4, the unit eigenvalue of B under a largest one of 1e12: 1e12 x 2^-53.)  M, mu and the draws depend on k alone."""
    rng = np.random.default_rng(LOWRANK_SEED + k)
    n = LOWRANK_N
    M = rng.standard_normal((n, k))
    M[:, 1] = M[:, 0] * (1 + 1e-6) + 1e-6 * M[:, 1]
    mu = 1.0 + 0.1 * rng.standard_normal(n)
    d = rng.uniform(0.5, 1.5, size=n) * (2.6 * n / cond)
    y = mu + 1e-3 * (M @ rng.standard_normal(k)) + np.sqrt(d) * rng.standard_normal(n)
    return y, mu, np.asfortranarray(M), d


def lowrank_name(k: int, cond: float) -> str:
    return f"lowrank-k{k}-c{cond:.0e}"


def lowrank_cases():
    return [(k, c) + lowrank_case(k, c) for k in LOWRANK_KS for c in LOWRANK_CONDS]


# ---------------------------------------------------------------- the comparison the GPU tests use

def tolerance(e_oracle: float) -> float:
    return max(TOL_FACTOR * e_oracle, TOL_FLOOR)


def worst_error(values: dict, exact: dict) -> float:
    """max |value - exact| over the null model and every table of ``exact``; inf where a value is not finite
    although the exact one is, or finite although the exact one is NaN"""
    worst = abs(float(values["null"]) - float(exact["null"]))
    worst = worst if np.isfinite(worst) else np.inf
    for t in TABLES:
        if t not in exact:
            continue
        v, e = np.asarray(values[t], dtype=np.float64), np.asarray(exact[t], dtype=np.float64)
        if v.shape != e.shape or not np.array_equal(np.isfinite(v), np.isfinite(e)):
            return float("inf")
        ok = np.isfinite(e)
        if ok.any():
            worst = max(worst, float(np.abs(v[ok] - e[ok]).max()))
    return worst


def class_failures(name: str, got: dict, exact: dict, oracle_values: dict, extra_bound: float | None = None):
    """Compare ``got`` (null, dla[, lls, dla2]) with the exact values at 10 x the oracle's own worst error on the
    class (floored at 1e-9; ``extra_bound``: a fixed bound that must hold as well).  Returns (failures, e_got,
    e_oracle, tolerance)."""
    e_oracle = worst_error(oracle_values, exact)
    e_got = worst_error(got, exact)
    tol = tolerance(e_oracle)
    failures = []
    if not e_got <= tol:
        failures.append(f"{name}: |value - exact| = {e_got:.3e} > {tol:.3e} = max(10 x {e_oracle:.3e}, 1e-9)")
    if extra_bound is not None and not e_got <= extra_bound:
        failures.append(f"{name}: |value - exact| = {e_got:.3e} > {extra_bound:.1e}")
    return failures, e_got, e_oracle, tol


def closest_top_two(exact_table) -> float:
    """the gap between the two largest finite exact values of a table (a MAP index is decided by it)"""
    v = np.sort(np.asarray(exact_table)[np.isfinite(exact_table)])
    return float(v[-1] - v[-2])


# ---------------------------------------------------------------- the fixture and the GPU side

FIXTURE = "exact_hard_conditioning.npz"


def load_fixture(golden) -> dict:
    """{class name: {key: array}} of tests/golden/exact_hard_conditioning.npz; an array stored once and referred
    to by a later class ("<key>@" holds the first holder's name) is resolved here"""
    z = golden(FIXTURE)
    out = {}
    for full in z.files:
        name, key = full.split("/", 1)
        out.setdefault(name, {})[key.rstrip("@")] = z[str(z[full])] if key.endswith("@") else z[full]
    return out


def stored_values(entry: dict, prefix: str) -> dict:
    """the ``exact_`` or ``oracle_`` values of a fixture entry under the names the comparison uses"""
    return {t: entry[prefix + t] for t in ("null",) + TABLES if prefix + t in entry}


def run_gpu(case) -> dict:
    """The case through Context / Batch.process (single DLA) or Batch.process_multi with the caller's base sample
    indices: the downloaded results plus ``null``, ``dla`` [, ``lls``, ``dla2``] as :func:`run_oracle` names them"""
    import gp_dla_detection_amd as gp
    sp, p = case["spectrum"], case["params"]
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(case["model"])
        ctx.set_samples(case["samples"])
        if case["bsi"] is None:
            batch = ctx.upload([sp], np.array([np.log(0.9)]), np.array([np.log(0.1)]))
        else:
            lp_dla = np.log(np.full((1, MAX_DLAS), 0.1 / MAX_DLAS))
            batch = ctx.upload([sp], np.array([np.log(0.85)]), lp_dla, np.array([np.log(0.05)]))
        try:
            if case["bsi"] is None:
                batch.process()
                out = batch.download()
                out.update(null=out["log_likelihoods_no_dla"][0], dla=out["sample_log_likelihoods_dla"][0])
            else:
                batch.process_multi(case["bsi"][None])
                out = batch.download_multi()
                out.update(null=out["log_likelihoods_no_dla"][0], dla=out["sample_log_likelihoods_dla"][0, 0],
                           lls=out["sample_log_likelihoods_lls"][0], dla2=out["sample_log_likelihoods_dla"][0, 1])
        finally:
            batch.close()
    finally:
        ctx.close()
    return out


def run_gpu_child(classes, env, out_path):
    """In a clean child (record_class_worker.py explains why): ``env`` set before the library is loaded, then
    :func:`run_gpu` for every class, every array saved under <class name>/<key>"""
    import os
    os.environ.update(env)
    arrays = {}
    for cls in classes:
        out = run_gpu(build_case(cls))
        arrays.update({f"{class_name(cls)}/{key}": np.asarray(v) for key, v in out.items() if isinstance(v, np.ndarray)})
    np.savez(out_path, **arrays)
