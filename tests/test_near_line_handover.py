"""The three-line optical-depth sum of a voted K-step (near_lines3 in csrc/voigt_tiers.hpp), restated in Python
floats in the kernel's operation order and compared with 50-digit sums of sqrt(pi) lead_j Re w(x_j + i y_j)
(voigt.c:282-289).  No GPU.

 - new: per line, s_j = x_j^2 + y_j^2 on the FMA velocity; where s_j < 900 the term is
   (sqrt(pi) lead_j) * near_poly(|x_j|) on the reference's two-rounding velocity (voigt.c:287; the library's own
   tables through gpdla_debug_near_poly), elsewhere the wing tier's (lead_j y_j) * rho_j T(rho_j) as wing_sum3 forms
   it (one reciprocal of s_a s_b s_c, peeled; the priming's spelling of the leading Horner step); summed as the
   wing tier sums: fma(c2, t2, fma(c1, t1, c0 t0)).
 - parent (total_near<3>, which it replaces): per line on the two-rounding velocity, |x| < 30 ? the same polynomial
   term : (lead_j y_j) * wing_core(x^2, y_j^2); summed ((f0 + f1) + f2).
Both are evaluated for each line at detunings 29 .. 33 on either side of the line (the other two lines where one
absorber redshift puts them, thousands of Doppler widths off), and at points where a second line is made near as
well (its multiplier chosen for that: the function takes any three multipliers).  The reciprocals are exact
quotients rounded once in both (the kernels' fast_rcp adds 2.2e-15 to either).  The bound is not a fixed number:
both forms are rounding-level in different orders, so the new one must stay within twice the parent's worst relative
error on the same points.  Both figures are printed before the assertion."""
import ctypes as C
import os
import re
from fractions import Fraction

import mpmath as mp
import numpy as np
import pytest

from gp_dla_detection_amd import _lib
from gp_dla_detection_amd._lyman import C_CGS, LINES, SIGMA_CGS

SQRT_PI = 1.7724538509055159
INV_S = 1.0 / (np.sqrt(2.0) * SIGMA_CGS)                       # host_common.hpp: LineTable::inv_sqrt2_sigma
LEAD = [LINES[j][3] for j in range(3)]
Y = [LINES[j][4] / np.sqrt(2.0) / SIGMA_CGS for j in range(3)]
Y2 = [y * y for y in Y]
CWING = [l * y for l, y in zip(LEAD, Y)]
Z_DLA = 2.7


def fma(a, b, c):
    """a b + c with ONE rounding, as v_fma_f64 gives it"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def rew_exact(x, y):
    """Re w(x + i y) by the Voigt function's continued fraction (Laplace): for |x| >= 30 (as tests/test_wing_exp_series.py,
    which checks it against exp(-z^2) erfc(-i z) to 1e-40 there)"""
    z = mp.mpc(x, y)
    f = mp.mpf(0)
    for n in range(60, 0, -1):
        f = (mp.mpf(n) / 2) / (z - f)
    return (mp.mpc(0, 1) / mp.sqrt(mp.pi) / (z - f)).real


@pytest.fixture(autouse=True)
def fifty_digits():
    with mp.workdps(50):
        yield


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def wing():
    with open(os.path.join(_lib.CSRC, "voigt_tiers.hpp")) as f:
        found = dict(re.findall(r"\b(kE\d) = (0x1\.[0-9a-f]+p[+-]\d+)", f.read()))
    return {name: float.fromhex(v) for name, v in found.items()}


def rcp(v):
    return float(1 / Fraction(v))


def near_poly(lib, line, ax):
    v = C.c_double()
    assert lib.gpdla_debug_near_poly(line, float(ax), C.byref(v), None) == 0
    return v.value


def multipliers(z):
    return [float(C_CGS) / (LINES[j][0] * (1 + z)) / 1e8 for j in range(3)]       # voigt.c:278-279


def two_rounding_x(lam, m):
    return (lam * m - float(C_CGS)) * INV_S                                        # voigt.c:287 (-ffp-contract=off)


def new_sum(lib, c, lam, mm):
    ms = [m * INV_S for m in mm]
    cs = float(C_CGS) * INV_S
    x = [fma(lam, ms[j], -cs) for j in range(3)]
    s = [fma(x[j], x[j], Y2[j]) for j in range(3)]
    rinv = rcp((s[0] * s[1]) * s[2])                                               # wing_sum3
    r = [rinv * (s[1] * s[2]), rinv * (s[0] * s[2]), rinv * (s[0] * s[1])]
    coef, term = [], []
    for j in range(3):
        t = r[j] * c["kE4"] + c["kE3"]
        t = fma(t, r[j], c["kE2"] - 2.0 * Y2[j])
        t = fma(t, r[j], c["kE1"])
        t = fma(t, r[j], 1.0)
        if s[j] < 900.0:
            ax = min(abs(two_rounding_x(lam, mm[j])), float.fromhex("0x1.fffffffffffffp+4"))
            coef.append(SQRT_PI * LEAD[j])
            term.append(near_poly(lib, j, ax))
        else:
            coef.append(CWING[j])
            term.append(r[j] * t)
    return fma(coef[2], term[2], fma(coef[1], term[1], coef[0] * term[0]))


def wing_core(c, x2, y2):
    rho = rcp(x2 + y2)
    t = fma(c["kE4"], rho, c["kE3"])
    t = fma(t, rho, c["kE2"])
    t = fma(t, rho, c["kE1"])
    t = fma(t, rho, 1.0)
    t = fma(-2.0 * y2 * rho, rho, t)
    return rho * t


def parent_sum(lib, c, lam, mm):
    total = 0.0
    for j in range(3):
        ax = abs(two_rounding_x(lam, mm[j]))
        total += SQRT_PI * LEAD[j] * near_poly(lib, j, ax) if ax < 30.0 else CWING[j] * wing_core(c, ax * ax, Y2[j])
    return total


def exact_sum(lam, mm):
    total = mp.mpf(0)
    for j in range(3):
        x = abs((mp.mpf(lam) * mp.mpf(mm[j]) - mp.mpf(float(C_CGS))) * mp.mpf(INV_S))
        if x >= 30:
            rew = rew_exact(x, mp.mpf(Y[j]))
        else:
            z = mp.mpc(x, mp.mpf(Y[j]))
            rew = (mp.exp(-z * z) * mp.erfc(-1j * z)).real
        total += mp.sqrt(mp.pi) * mp.mpf(LEAD[j]) * rew
    return total


def points():
    """(wavelength, three multipliers, label)"""
    mm = multipliers(Z_DLA)
    out = []
    grid = [29.0 + 0.0173 * i for i in range(232)]                                 # 29 .. 33, off the round numbers
    for j in range(3):
        for sign in (1.0, -1.0):
            for x in grid:
                lam = float(C_CGS) * (1 + sign * x / (float(C_CGS) * INV_S)) / mm[j]
                out.append((lam, mm, f"line {j} at x = {sign * x:+.4f}"))
    # a second (and a third) line near as well: their multipliers put them where asked, at this wavelength
    for xa, xb, xc in ((8.0, 29.5, None), (30.5, 3.0, None), (29.99, 30.01, None), (0.0, 12.0, 29.0), (31.0, 31.5, 30.2)):
        lam = float(C_CGS) * (1 + xa / (float(C_CGS) * INV_S)) / mm[0]
        m2 = list(mm)
        for j, xj in ((1, xb), (2, xc)):
            if xj is not None:
                m2[j] = float(C_CGS) * (1 + xj / (float(C_CGS) * INV_S)) / lam
        out.append((lam, m2, f"lines at x = {xa}, {xb}, {xc}"))
    return out


def worst_of(lib, wing, pts):
    worst_new, worst_parent = (0.0, None), (0.0, None)
    for lam, mm, label in pts:
        want = exact_sum(lam, mm)
        e_new = float(abs(mp.mpf(new_sum(lib, wing, lam, mm)) / want - 1))
        e_par = float(abs(mp.mpf(parent_sum(lib, wing, lam, mm)) / want - 1))
        if e_new > worst_new[0]:
            worst_new = (e_new, label)
        if e_par > worst_parent[0]:
            worst_parent = (e_par, label)
    return worst_new, worst_parent


@pytest.mark.parametrize("group", ["one line, x = 29 .. 33", "two or three lines near"])
def test_new_combination_against_the_parents(lib, wing, group):
    """Each group of points by itself: the error at a line's steep core (the velocity's own rounding times
    2 x) would otherwise hide the hand-over region."""
    pts = [p for p in points() if p[2].startswith("lines at") == (group != "one line, x = 29 .. 33")]
    worst_new, worst_parent = worst_of(lib, wing, pts)
    print(f"{group}, {len(pts)} points: worst relative error of the sum: new {worst_new[0]:.3e} ({worst_new[1]}), "
          f"parent {worst_parent[0]:.3e} ({worst_parent[1]})")
    assert worst_new[0] <= 2.0 * worst_parent[0]
