"""The two short series of the sweeps' profile arithmetic, as shipped: the coefficients are read out of
csrc/voigt_tiers.hpp and both series are evaluated the way the kernels evaluate them (fp64, one rounding per
FMA, the kernels' Horner order), then compared with 50-digit mpmath values.

 - the wing tier (wing_core / wing_sum3 / wing_sum3_rcp4 and the halves in csrc/sweep_slim_kernel.hpp):
   rho [1 + rho (kE1 + rho (t2_j + rho (kE3 + rho kE4)))] with t2_j = kE2 - 2 y_j^2, against
   Re w(x + i y_j) sqrt(pi) / y_j over |x| in [30, 1e5] at the three lines' y_j (voigt.c:282-289);
   bound 6e-15 relative.  Measured 4.9e-15, at Lyman-alpha and |x| = 31.4: the degree-4 fit's 1.25e-15 (an
   extremum of its error lies there) on top of what the wing formula itself neglects, terms in y^2 rho^3, 4.6e-15
   at |x| = 30 for Lyman-alpha's y and 3.5e-15 there (the degree-6 form has them too), and the roundings.
 - the exp polynomial (exp_table_end_scaled, and exp_series_scaled in csrc/sweep_slim_kernel.hpp):
   1 + d (c1 + d (c2 + d (c3 + d (c4 + d c5)))), c_k = (ln2/64)^k / k! as the header forms them, against
   exp(d ln2 / 64) over |d| <= 1/2; bound 4e-15 relative (the polynomial stayed at degree 5, whose truncation is
   3.6e-17: what is left is rounding).
Every figure is printed before it is asserted."""
import os
import re
from fractions import Fraction

import mpmath as mp
import pytest

from gp_dla_detection_amd import _lib
from gp_dla_detection_amd._lyman import LINES, SIGMA_CGS


@pytest.fixture(autouse=True)
def fifty_digits():
    """mpmath's precision is global and other test modules set their own: 50 digits here, restored afterwards"""
    with mp.workdps(50):
        yield


def fma(a, b, c):
    """a b + c with ONE rounding, as v_fma_f64 gives it"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def source(name):
    with open(os.path.join(_lib.CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def wing():
    found = dict(re.findall(r"\b(kE\d) = (0x1\.[0-9a-f]+p[+-]\d+)", source("voigt_tiers.hpp")))
    print("shipped wing coefficients:", found)
    assert sorted(found) == ["kE1", "kE2", "kE3", "kE4"], "the wing series is of degree 4"
    return {name: float.fromhex(v) for name, v in found.items()}


@pytest.fixture(scope="module")
def exp_poly():
    """c1..c5 of exp_table_end_scaled, formed as its constexpr line forms them"""
    text = source("voigt_tiers.hpp")
    body = text[text.index("double exp_table_end_scaled("):]
    body = body[:body.index("\n}\n")]
    L = float(re.search(r"constexpr double L = ([0-9.e+-]+);", body).group(1))
    line = re.search(r"constexpr double (c1 = L, c2 = [^;]+);", body).group(1)
    print("shipped exp coefficients: L =", L, ";", line)
    assert line == "c1 = L, c2 = L * L / 2, c3 = L * L * L / 6, c4 = L * L * L * L / 24, c5 = L * L * L * L * L / 120"
    c = [L, L * L / 2, L * L * L / 6, L * L * L * L / 24, L * L * L * L * L / 120]
    # Horner order of the five steps: c5, c4 | c3 | c2 | c1 | 1.0
    steps = re.findall(r'asm\("v_fma_f64[^;]+?"[sv]"\((c\dv?)\)\);', body)
    print("Horner steps:", steps)
    assert steps == ["c4v", "c3", "c2", "c1"] and '"s"(c5), "v"(e.r), "v"(c4v)' in body and "fma(p, e.r, 1.0)" in body
    return L, c


def test_both_spellings_are_in_step():
    """The two-halves spelling of the slim sweep takes the shared wing constants and spells the same exp series."""
    slim = source("sweep_slim_kernel.hpp")
    assert not re.search(r"\bkE\d = ", slim)
    for name in ("kE1", "kE3", "wing_lead"):   # (kE4 is wing_lead's, kE2 rides in LineTable::t2)
        assert re.search(rf"\b{name}\b", slim), name
    assert "kE5" not in slim and "kE5" not in source("voigt_tiers.hpp")
    one = source("voigt_tiers.hpp")
    one = one[one.index("double exp_table_end_scaled("):]
    two = slim[slim.index("double exp_series_scaled("):]
    pick = lambda s: re.findall(r"constexpr double (?:L|c1) = [^;]+;|asm\(\"v_fma_f64[^;]+;", s[:s.index("\n}\n")])
    assert pick(one) == pick(two) and len(pick(one)) == 6


def wing_as_the_kernels(x, y, c, fused_lead):
    """``fused_lead``: the leading Horner step as one FMA (wing_core; wing_lead in wing_sum3_rcp4 and
    wing3_back_rcp4) or as a multiply and an add, two roundings (wing_sum3: `r * kE4 + kE3` under -ffp-contract=off)"""
    y2 = y * y
    s = fma(x, x, y2)
    rho = float(1 / Fraction(s))                     # (the kernels' fast_rcp adds its own 2.2e-15: not the series')
    t2 = c["kE2"] - 2.0 * y2                         # host_common.hpp: LineTable::t2
    t = fma(rho, c["kE4"], c["kE3"]) if fused_lead else rho * c["kE4"] + c["kE3"]
    t = fma(t, rho, t2)
    t = fma(t, rho, c["kE1"])
    t = fma(t, rho, 1.0)
    return rho * t


def rew_exact(x, y):
    """Re w(x + i y) by the Voigt function's continued fraction (Laplace): converges for y > 0, fast for |z| >= 30"""
    z = mp.mpc(x, y)
    f = mp.mpf(0)
    for n in range(60, 0, -1):                        # w(z) = (i / sqrt(pi)) / (z - (1/2) / (z - (2/2) / (z - ...
        f = (mp.mpf(n) / 2) / (z - f)
    return (mp.mpc(0, 1) / mp.sqrt(mp.pi) / (z - f)).real


def test_the_continued_fraction_is_the_faddeeva_function():
    for x, y in ((30.0, 6.67e-4), (45.5, 1.2e-4), (300.0, 5e-5)):
        z = mp.mpc(x, y)
        want = (mp.exp(-z * z) * mp.erfc(-1j * z)).real
        rel = abs(rew_exact(x, y) / want - 1)
        print(f"x = {x}, y = {y}: continued fraction vs exp(-z^2) erfc(-i z): {mp.nstr(rel, 3)}")
        assert rel < mp.mpf("1e-40")


def test_wing_series_degree_4(wing):
    ys = [LINES[j][4] / 2 ** 0.5 / SIGMA_CGS for j in range(3)]
    xs = [30.0 + 0.0371 * i for i in range(120)] + [30.0 * (1e5 / 30.0) ** (i / 199.0) for i in range(200)]
    worst = (0.0, None)
    for j, y in enumerate(ys):
        for x in xs:
            want = rew_exact(x, y) * mp.sqrt(mp.pi) / mp.mpf(y)
            for fused_lead in (True, False):
                rel = float(abs(mp.mpf(wing_as_the_kernels(x, y, wing, fused_lead)) / want - 1))
                if rel > worst[0]:
                    worst = (rel, (j, x))
    print(f"wing tier, degree 4: worst relative error {worst[0]:.3e} at (line, |x|) = {worst[1]}")
    assert worst[0] <= 6e-15


def test_exp_polynomial(exp_poly):
    L, c = exp_poly
    assert abs(mp.mpf(L) / (mp.log(2) / 64) - 1) < mp.mpf("3e-16")
    worst = (0.0, None)
    for i in range(2001):
        d = (i - 1000) / 2000.0
        p = fma(c[4], d, c[3])
        for ck in (c[2], c[1], c[0], 1.0):
            p = fma(p, d, ck)
        rel = float(abs(mp.mpf(p) / mp.exp(mp.log(2) / 64 * mp.mpf(d)) - 1))
        if rel > worst[0]:
            worst = (rel, d)
    print(f"exp polynomial, degree 5: worst relative error {worst[0]:.3e} at delta = {worst[1]}")
    assert worst[0] <= 4e-15
