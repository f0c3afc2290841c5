"""The refine pass and the batch conditioned on fixed absorbers (4.20) where the arithmetic is hard
(plain module, like hard_conditioning_cases.py, whose strata, classes and comparison it reuses: the fixture generator
tests/golden/make_exact_refine_hard.py, test_refine_hard.py and test_gpu_refine_hard.py import it, nothing else does).

Both families reach the sweep cores through front ends of their own -- the boxed prologue, which forms
N' = exp10(n_lo + (n_hi - n_lo) v) and z' = z_lo + (z_hi - z_lo) u on the device, and k_condition_rows, which
multiplies the prepared rows by the fixed absorbers' absorption -- and both were only ever measured on the shipped,
well-conditioned model.  Here they run on the strata of hard_conditioning_cases.py (S/N 100 .. 1000, cond(B) ~ 5e6,
|log-likelihood| ~ 1e5 .. 1e7), and the yardstick is the 50-digit value at the fp64 inputs the contract defines.

    refine        six classes of H.CLASSES (REFINE_CLASSES), S' = 65 plain Halton points (66 slots: the partly filled
                  last group H.S was chosen for), 3 levels, delta 12.5, pad 2, uniform prior.  Level 1's box comes from
                  the EXACT first-pass table of exact_hard_conditioning.npz rounded to fp64, every later box from the
                  exact lambda of the level before: the fixture's boxes are those of exact arithmetic.
    conditioned   four classes (COND_CLASSES), two fixed lists each (``one``, ``three``: fixed_lists).

Box determinism is a condition on the inputs, not a tolerance.  The box arithmetic is a handful of fp64 operations
and bit-reproducible (test_gpu_refine.py::test_boxes_equal_the_restatement), so a box of the GPU's can differ from
the fixture's only through the membership of A = {l >= max l - delta}, and the outside sums only through the side of
a box edge a sample falls on.  Required at every level (asserted by the generator, re-asserted by test_refine_hard.py
from the stored values): no source value within MARGIN of its cut, no source sample within EDGE_REL (relative) of a
box edge.  MARGIN is a thousand times the oracle cap, EDGE_REL ten million ulps.

Hot loops: process_qsos.m:185-199, process_qsos_multiple_dlas_meanflux.m:340-392, log_mvnpdf_low_rank.m:11-32.
"""
from __future__ import annotations

import numpy as np

import conditional_restatement as CR
import hard_conditioning_cases as H
from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters

SR = 65                        # refine points: 66 slots with the null model's
LEVELS, DELTA, PAD = 3, 12.5, 2.0
MARGIN = 1e-3                  # no exact l (lambda) this close to max - delta
EDGE_REL = 1e-9                # no source sample this close (relative to the edge) to a box edge
MIN_FINITE = 40                # conditioned tables: samples outside the separation, of 65
SEPARATION = MultiParameters().min_z_separation

# (stratum, driver, k, Voigt lines) of H.CLASSES -> the boxed kernel that sweeps it
REFINE_CLASSES = (
    ("high_snr", "single", 20, 3),          # k_sweep_slim_boxed<3>
    ("correlated", "single", 20, 3),
    ("saturated", "single", 20, 3),
    ("correlated", "single", 20, 31),       # k_sweep_slim_boxed<0>
    ("correlated", "single", 40, 3),        # k_sweep_split_slim<3, 0, BoxedSweepArgs>
    ("few_pixels", "single", 40, 3),
)
# the conditioned batch is a single-DLA batch; the ``multi`` class is the multi-DLA driver's rows (meanflux_rows = 1)
COND_CLASSES = (
    ("correlated", "single", 20, 3),
    ("saturated", "single", 20, 3),
    ("correlated", "single", 40, 3),
    ("correlated", "multi", 20, 3),
)
LISTS = ("one", "three")
assert set(REFINE_CLASSES) <= set(H.CLASSES) and set(COND_CLASSES) <= set(H.CLASSES)

# class -> (first Halton index, delta) where they are not (1, DELTA).  A class whose exact tables miss MARGIN or whose
# oracle misses H.ORACLE_CAP at some level is moved to another first Halton index (1 .. 28), then to delta 25; the
# oracle and the exact values alone decide, never a GPU result.  With 31 lines the oracle is 1.146e-6 from the exact
# value at the twelfth Halton point of level 1's box (u = 3/16, v = 4/9), whichever slot holds it: first indices
# 1 .. 12 all carry that point, 13 is the first without it (6.2e-7).
TUNING = {
    ("correlated", "single", 20, 31): (13, DELTA),
}

# fixed absorbers as (fraction of the search range, log10 N_HI), in list order.  The search range is 80 separations
# wide and the first-pass offsets are Halton points of base 2 (spacing 1/64 = 1.25 separations), so every fixed
# redshift has one or two samples inside its separation; the fractions are 13 separations and more apart, clear of
# the masked run (fractions 0.275 .. 0.305 in Lyman alpha).  ``three`` holds one absorber of log N_HI = 23, whose
# Lyman alpha trough bottoms out at 1e-28 on kept pixels.  Laid over an unabsorbed flux of S/N 1000 it takes
# |log-likelihood| to 3e6 .. 6e6, and where it lies decides whether the oracle (never the GPU, unmeasured then) meets
# H.ORACLE_CAP on all four classes: of the 27 fractions tried between 0.05 and 0.96 (worst oracle error 5e-7 .. 8e-6)
# 0.05, 0.11 and 0.14 do; 0.11 has the deepest trough of the three.
FIXED = {
    "one": ((0.40, 21.0),),
    "three": ((0.45, 20.5), (0.11, 23.0), (0.85, 21.3)),
}


def refine_name(cls) -> str:
    return "refine-" + H.class_name(cls)


def cond_name(cls, which: str) -> str:
    return f"cond-{which}-" + H.class_name(cls)


def tuning(cls):
    return TUNING.get(cls, (1, DELTA))


def points(first: int = 1):
    """(u, v): SR plain Halton points of bases 2 and 3 from index ``first`` (refine_cases.halton_points starts at 1)"""
    n = first - 1 + SR
    return synthetic.halton(n, 2)[first - 1:].copy(), synthetic.halton(n, 3)[first - 1:].copy()


def n_range(lnhi):
    return float(np.min(lnhi)), float(np.max(lnhi))


def first_pass_coordinates(entry):
    """(z, n) of the first pass's samples as the contract forms them, from an entry of exact_hard_conditioning.npz"""
    min_z, max_z = float(entry["min_z_dla"]), float(entry["max_z_dla"])
    return min_z + (max_z - min_z) * np.asarray(entry["offset_samples"], dtype=np.float64), np.asarray(entry["log_nhi_samples"], dtype=np.float64)


def box_margins(src, src_z, src_n, parent, box, delta):
    """(distance of the nearest finite source value to the cut max - delta, smallest relative distance of a source
    sample to an edge of ``box``): the two conditions under which a table within MARGIN of ``src`` gives the same box
    and the same outside set.  An edge clamped to the parent's is not looked at: it IS the parent's edge, bit for bit,
    no source sample lies beyond it, and "outside" is strict -- the sample that defines N_lo or N_hi sits exactly
    on it."""
    src = np.asarray(src, dtype=np.float64)
    fin = np.isfinite(src)
    cut = np.max(src[fin]) - delta
    cut_margin = float(np.min(np.abs(src[fin] - cut)))
    edge = np.inf
    for j, c in enumerate((src_z, src_z, src_n, src_n)):
        if box[j] != parent[j]:
            edge = min(edge, float(np.min(np.abs(c - box[j]) / max(abs(box[j]), 1.0))))
        else:
            assert (c <= box[j]).all() if j % 2 else (c >= box[j]).all()
    return cut_margin, edge


def refined_coordinates(box, u, v):
    """z' = z_lo + (z_hi - z_lo) u, n' = n_lo + (n_hi - n_lo) v, one rounding each, as the contract writes them"""
    return box[0] + (box[1] - box[0]) * u, box[2] + (box[3] - box[2]) * v


def refined_absorption(oracle, run, z, n, lines):
    """[S', in-range pixels]: oracle.voigt at (z', 10^n') -- the host's power, where the device takes exp10"""
    return np.stack([oracle.voigt(run["padded_wavelengths"], float(zi), 10.0 ** float(ni), lines) for zi, ni in zip(z, n)])


def oracle_values(oracle, inputs):
    out = []
    for args in inputs:
        lp, rc = oracle.log_mvnpdf_low_rank(*args)
        assert rc == 0
        out.append(lp)
    return np.array(out)


# ---------------------------------------------------------------- fixed absorbers

def fixed_lists(run) -> dict:
    """{"one": [(z, log N)], "three": [...]} for a quasar whose search range is the oracle run's"""
    lo, hi = float(run["min_z_dla"]), float(run["max_z_dla"])
    out = {which: [(lo + f * (hi - lo), ln) for f, ln in spec] for which, spec in FIXED.items()}
    for lst in out.values():
        zs = [z for z, _ in lst]
        assert all(abs(a - b) >= 3 * SEPARATION for i, a in enumerate(zs) for b in zs[:i])
    return out


def meanflux_rows(cls) -> bool:
    return cls[1] == "multi"


def fixed_absorption(run, fixed, lines):
    """A on the in-range grid: the product in list order (N = 10^log N taken by the host, as the library takes it)"""
    return CR.absorption(run["padded_wavelengths"], [(float(z), float(ln)) for z, ln in fixed], lines)


def conditioned_inputs(case, run, A, a=None):
    """(y, mu, M, d) of the conditioned null model (``a`` None) or of a sample whose absorption on the in-range grid is
    ``a``, each product rounded in the contract's order: the rows are conditioned first (mu A, M A, omega2 (A A)),
    the sweep multiplies the conditioned rows by the sample's profile"""
    y, mu, M, d = H.lowrank_inputs(case, run)
    sp = case["spectrum"]
    inside = H.in_range(sp)
    kept = ~sp["pixel_mask"].astype(bool)[inside]
    nv = sp["noise_variance"][inside][kept]
    A = A[kept]
    mu, M, om2 = run["this_mu"] * A, run["this_M"] * A[:, None], run["this_omega2"] * (A * A)
    if a is None:
        return y, mu, M, om2 + nv
    a = a[kept]
    return y, mu * a, M * a[:, None], om2 * a ** 2 + nv


# ---------------------------------------------------------------- the comparison

def table_error(values, exact) -> float:
    """max |value - exact| over a table; inf where the two are not finite, -inf and NaN in the same places"""
    v, e = np.asarray(values, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    same = (v.shape == e.shape and np.array_equal(np.isfinite(v), np.isfinite(e)) and np.array_equal(np.isneginf(v), np.isneginf(e))
            and np.array_equal(np.isnan(v), np.isnan(e)))
    if not same:
        return float("inf")
    ok = np.isfinite(e)
    return float(np.abs(v[ok] - e[ok]).max()) if ok.any() else 0.0


def failures(name, e_got, e_oracle):
    """the rule of hard_conditioning_cases.py: e_got <= max(10 x e_oracle, 1e-9).  Returns (failures, tolerance)."""
    tol = H.tolerance(e_oracle)
    if e_got <= tol:
        return [], tol
    return [f"{name}: |value - exact| = {e_got:.3e} > {tol:.3e} = max(10 x {e_oracle:.3e}, 1e-9)"], tol


def ratio(e_got, e_oracle):
    return e_got / e_oracle if e_oracle > 0 else float("inf")


# ---------------------------------------------------------------- the fixture and the GPU side

FIXTURE = "exact_refine_hard.npz"


def load_fixture(golden) -> dict:
    """{entry name: {key: array}} of tests/golden/exact_refine_hard.npz"""
    z = golden(FIXTURE)
    out = {}
    for full in z.files:
        name, key = full.split("/", 1)
        out.setdefault(name, {})[key] = z[full]
    return out


def evidence_bound(first_entry, entry, levels: int = LEVELS) -> float:
    """max(10 E, 1e-9), E the oracle's worst error over the first-pass table and the levels up to ``levels``:
    log-sum-exp is 1-Lipschitz in the sup norm, so the tables' error bounds the evidence's; what remains is one
    rounding of M + log(tot), below the floor up to |M| ~ 4e6"""
    E = table_error(first_entry["oracle_dla"], first_entry["exact_dla"])
    for lev in range(levels):
        E = max(E, table_error(entry["oracle_ell"][lev], entry["exact_ell"][lev]))
    return H.tolerance(E)


def run_gpu_refine(case, u, v, delta) -> dict:
    """process(), then refine at 1 .. LEVELS levels (a level's tables are resident only after the call with that many
    levels) on one context and one upload: ``first`` (the first pass's download) and ``levels`` (a list)"""
    import gp_dla_detection_amd as gp
    sp = case["spectrum"]
    ctx = gp.Context(0, case["params"])
    try:
        ctx.set_model(case["model"])
        ctx.set_samples(case["samples"])
        ctx.set_refine_points(u, v)
        batch = ctx.upload([sp], np.array([np.log(0.9)]), np.array([np.log(0.1)]))
        try:
            batch.process()
            first = batch.download()
            levels = [batch.refine(levels=lev + 1, delta=delta, pad=PAD) for lev in range(LEVELS)]
        finally:
            batch.close()
    finally:
        ctx.close()
    return dict(first=first, levels=levels)


def run_gpu_conditioned(case, lists: dict) -> dict:
    """{list name: download} of the case as a single-DLA batch conditioned on each list in turn, on one context and
    one upload; the ``multi`` class with the multi-DLA driver's rows, under its MultiParameters"""
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd import conditional
    sp = case["spectrum"]
    ctx = gp.Context(0, case["params"])
    out = {}
    try:
        ctx.set_model(case["model"])
        ctx.set_samples(case["samples"])
        batch = ctx.upload([sp], np.array([np.log(0.9)]), np.array([np.log(0.1)]))
        try:
            for which, fixed in lists.items():
                batch.set_fixed_absorbers(conditional.csr_of([[list(map(float, a)) for a in fixed]]), SEPARATION,
                                          meanflux_rows(case["cls"]))
                batch.process()
                out[which] = batch.download()
        finally:
            batch.close()
    finally:
        ctx.close()
    return out
