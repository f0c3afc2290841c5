// voigt_tiers.hpp -- the optical-depth sum of voigt.c:282-290 in two tiers, and the exp of :291 through a table.  The
// wing tier (|x| >= 30 Doppler widths from every line) is a degree-4 series, branch-free; the accurate tier is the
// piecewise polynomial of near_tables.hpp, taken under a wave-uniform vote.
#pragma once
#include "faddeeva.hpp"
#include "near_tables.hpp"
#include "sweep_primitives.hpp"

namespace gpdla {

// Re w(x+iy) sqrt(pi)/y for |x| >= 30 given x2 = x^2 (see faddeeva.hpp rew_wing), with the fast
// reciprocal.  Returns the value with the y/sqrt(pi) factor left out.
// The wing series T(rho) = Sum_{m<=6} (2m+1)!!/2^m rho^m as 1 + rho (kE1 + kE2 rho + kE3 rho^2 + kE4 rho^3) on the
// interval the wing tier uses, 0 <= rho <= 1/900 (|x| >= 30): the degree-4 minimax polynomial with the constant
// term pinned at 1.0 (an inline constant).  Derivation, in 50-digit mpmath: Remez exchange on the error
// 1 + rho q(rho) - T(rho), q cubic, five alternation points in (0, 1/900] (the error vanishes at 0 by construction),
// its extrema located on a 4001-point grid, iterated until the points stop moving; the coefficients then rounded to
// fp64.  Maximum relative error 1.25e-15 (the degree-5 economisation this replaces: 1.9e-18), below the 2.2e-15 of
// fast_rcp that every rho carries anyway.  Two FMAs per line and evaluation less than the plain series;
// tests/test_wing_exp_series.py reads these constants.
constexpr double kE1 = 0x1.7fffffffd940ep+0, kE2 = 0x1.e0000294b4cbcp+1, kE3 = 0x1.a3f92a26b3728p+3,
                 kE4 = 0x1.df9f0e43cd754p+5;
// The leading Horner step kE4 rho + kE3 of the K-step's three lines as ONE three-address v_fma_f64 each (kE4 a scalar
// operand, kE3 in a vector register the lines share).  Spelled `rho * kE4 + kE3` it is a multiply and an add under
// the build's -ffp-contract=off, and as fma() the compiler picks v_fmac_f64 and copies the constant in front of
// each: 139.59 against 140.38 ms per launch for the multiply and add (profiles/ab_fp64_ops.txt, session 4).
__device__ __forceinline__ double wing_lead(double rho, double e3v) {
  double t;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(t) : "v"(rho), "s"(kE4), "v"(e3v));
  return t;
}

__device__ __forceinline__ double wing_core(double x2, double y2) {
  const double rho = fast_rcp(x2 + y2);
  double t = fma(kE4, rho, kE3);
  t = fma(t, rho, kE2);
  t = fma(t, rho, kE1);
  t = fma(t, rho, 1.0);
  t = fma(-2.0 * y2 * rho, rho, t);
  return rho * t;
}

// Accurate tier of the raw profile: Re w(|x| + i y_j) for |x| < 32 from line j's piecewise
// polynomial (near_tables.hpp; same index arithmetic and Horner order as near_poly_host).
__device__ __forceinline__ double near_poly(const double *line_tab, double ax) {
  const bool core = ax < 8.0;
  const double u = core ? ax * 8.0 : (ax - 8.0) * 2.0;
  const int i = (int)u;
  const double t = (u - (double)i) - 0.5;
  const double *c = line_tab + (size_t)((core ? 0 : kNearCore) + i) * kNearCoef;
  double cf[kNearCoef];
#pragma unroll
  for (int k = 0; k < kNearCoef; ++k) cf[k] = c[k];  // 12 independent loads, then the Horner chain
  double p = cf[kNearCoef - 1];
#pragma unroll
  for (int k = kNearCoef - 2; k >= 0; --k) p = fma(p, t, cf[k]);
  return p;
}

__device__ __forceinline__ uint32_t hi_word(double v) { return (uint32_t)__double2hiint(v); }

// What the three-line wing tier leaves for the accurate tier of a voted line (near_lines3): per line
// s = x^2 + y^2 on the FMA velocity (line j is near where hi_word(s[j]) < hi_word(900.0), the vote's own
// test) and q = rho T(rho), the line's wing-tier term with cwing[j] left out.
struct WingLines3 {
  double s[3], q[3];
};

// Wing-tier optical-depth sum for the three-line case (Ly-alpha, beta, gamma): FMA-form
// velocities, ONE reciprocal for the three lines (1/(sa sb sc), then peeled), degree-4 series.
// Returns Sum_j lead_j y_j [Re w_j sqrt(pi)/y_j]; *near: some line within 30 Doppler widths.
__device__ __forceinline__ double wing_sum3(double lamP, double msa, double msb, double msc, double cs,
                                            bool *near, WingLines3 *lines = nullptr) {
  const double xa = fma(lamP, msa, -cs), xb = fma(lamP, msb, -cs), xc = fma(lamP, msc, -cs);
  // x^2 + y^2 in one FMA; "near" is then tested on it (a threshold shift of y^2 <= 3e-7 in x^2,
  // immaterial: both tiers are accurate on either side of |x| = 30)
  const double sa = fma(xa, xa, g_lines.y2[0]), sb = fma(xb, xb, g_lines.y2[1]), sc = fma(xc, xc, g_lines.y2[2]);
  // some s < 900: on the high words, as unsigned integers -- positive doubles order like their bit
  // patterns and 900.0 has a zero low word, so s < 900.0 <=> hi(s) < hi(900.0); one three-way
  // integer minimum and one compare instead of two fp64 minima and a compare.
  static_assert(__builtin_bit_cast(unsigned long long, 900.0) == 0x408C200000000000ull, "bits of 900.0");
  *near = min(min(hi_word(sa), hi_word(sb)), hi_word(sc)) < 0x408C2000u;
  const double pab = sa * sb, pbc = sb * sc, pac = sa * sc;
  const double rinv = fast_rcp(pab * sc);
  const double ra = rinv * pbc, rb = rinv * pac, rc = rinv * pab;
  // T(rho) - 2 y^2 rho^2 by Horner; the -2 y_j^2 correction rides in the rho^2 coefficient (t2[j]).
  // The leading step as a multiply and an add (-ffp-contract=off): this form serves the primings and the kernels
  // off the headline; the K-step's own spelling, wing_sum3_rcp4, has it as one v_fma_f64 (wing_lead).
  double ta = ra * kE4 + kE3, tb = rb * kE4 + kE3, tc = rc * kE4 + kE3;
  ta = fma(ta, ra, g_lines.t2[0]); tb = fma(tb, rb, g_lines.t2[1]); tc = fma(tc, rc, g_lines.t2[2]);
  ta = fma(ta, ra, kE1); tb = fma(tb, rb, kE1); tc = fma(tc, rc, kE1);
  ta = fma(ta, ra, 1.0); tb = fma(tb, rb, 1.0); tc = fma(tc, rc, 1.0);
  const double qa = ra * ta, qb = rb * tb, qc = rc * tc;
  if (lines) *lines = WingLines3{{sa, sb, sc}, {qa, qb, qc}};
  return fma(g_lines.cwing[2], qc, fma(g_lines.cwing[1], qb, g_lines.cwing[0] * qa));
}

// wing_sum3 with the K-step's OTHER reciprocal riding along: 1/d of the weights (process_qsos.m:192-198
// folded into log_mvnpdf_low_rank.m:13-15; d is finite and positive, k_prepare sees to that) comes out
// of the same v_rcp_f64 as the three lines' 1/s_j -- prefix products, one reciprocal of s_a s_b s_c d,
// peeled: 9 multiplies and one fast_rcp instead of 7 multiplies and two (v_rcp_f64 issues in 17 cycles,
// a multiply in 5.4: tools/valu_rate_probe.hip).  s_j in [2e-7, 2e9] and d in [1e-280, 1e100 + omega2 a^2]
// (k_prepare sweeps a pixel of larger noise variance as a neutral row, kNeutralNoiseVariance): the
// product and its reciprocal stay normal.  Each quotient carries two or three more roundings than fast_rcp's 2.2e-15.
// (sweep_slim_kernel.hpp spells the same operations as two halves, wing3_front + wing3_back_rcp4: the record classes
// are bit-identical only while both stay in step -- change them together.)
__device__ __forceinline__ double wing_sum3_rcp4(double lamP, double msa, double msb, double msc, double cs,
                                                 bool *near, double d, double *inv_d, WingLines3 *lines) {
  const double xa = fma(lamP, msa, -cs), xb = fma(lamP, msb, -cs), xc = fma(lamP, msc, -cs);
  const double sa = fma(xa, xa, g_lines.y2[0]), sb = fma(xb, xb, g_lines.y2[1]), sc = fma(xc, xc, g_lines.y2[2]);
  *near = min(min(hi_word(sa), hi_word(sb)), hi_word(sc)) < 0x408C2000u;
  const double pab = sa * sb, pabc = pab * sc;
  const double rinv = fast_rcp(pabc * d);
  *inv_d = rinv * pabc;
  const double r3 = rinv * d;            // 1 / (sa sb sc)
  const double rc = r3 * pab, r2 = r3 * sc;  // 1 / sc, 1 / (sa sb)
  const double ra = r2 * sb, rb = r2 * sa;
  const double e3v = kE3;
  double ta = wing_lead(ra, e3v), tb = wing_lead(rb, e3v), tc = wing_lead(rc, e3v);
  ta = fma(ta, ra, g_lines.t2[0]); tb = fma(tb, rb, g_lines.t2[1]); tc = fma(tc, rc, g_lines.t2[2]);
  ta = fma(ta, ra, kE1); tb = fma(tb, rb, kE1); tc = fma(tc, rc, kE1);
  ta = fma(ta, ra, 1.0); tb = fma(tb, rb, 1.0); tc = fma(tc, rc, 1.0);
  const double qa = ra * ta, qb = rb * tb, qc = rc * tc;
  *lines = WingLines3{{sa, sb, sc}, {qa, qb, qc}};
  return fma(g_lines.cwing[2], qc, fma(g_lines.cwing[1], qb, g_lines.cwing[0] * qa));
}

constexpr int kRing2 = 33;   // doubled raw-profile ring: 32 slots + 1 pad per sample
constexpr int kExpTab = 64;  // entries of the 2^(j/64) table behind exp_table()

// exp(x) for x <= 0 through a 64-entry table: x = (64 n + j) ln2/64 + r, |r| <= ln2/128,
// exp(x) = 2^n * 2^(j/64) * P5(r).  Relative error < 2e-16 (r^6/720 < 3.6e-17).
// In two halves so that a caller can request the table entry early (exp_table_begin), put other
// LDS traffic behind it, and finish later (exp_table_end) without waiting for that traffic.
struct ExpState {
  double r, tabv;
  int ni;
};
__device__ __forceinline__ ExpState exp_table_begin(double x, const double *tab) {
  // no clamp: for x << -745 the integer conversion saturates, ni >> 6 is hugely negative and
  // ldexp returns 0; the reduced argument stays tiny (nf is exact to 0.5 up to |x| ~ 1e13)
  ExpState e;
  const double nf = rint(x * 92.33248261689366);            // 64 / ln2
  // saturating conversion, spelled as the instruction: (int)nf is undefined out of range
  asm("v_cvt_i32_f64 %0, %1" : "=v"(e.ni) : "v"(nf));
  e.tabv = tab[e.ni & (kExpTab - 1)];
  e.r = fma(-nf, 0.010830424667801708, x);                    // ln2/64 high part (low 24 bits zero)
  e.r = fma(-nf, 2.8447437476627285e-11, e.r);                // ln2/64 low part
  return e;
}
__device__ __forceinline__ double exp_table_end(const ExpState &e) {
  // The first two steps are spelled as three-address v_fma_f64: the compiler picks the two-address
  // v_fmac_f64 and then has to copy the (register-resident) constant in front of each, 3 moves
  // per value; 0.5 and 1.0 below are inline constants and need none.
  double p, c4 = 0.041666666666666664, c3 = 0.16666666666666666;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "s"(0.008333333333333333), "v"(e.r), "v"(c4));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(e.r), "v"(c3));
  p = fma(p, e.r, 0.5);
  p = fma(p, e.r, 1.0);
  p = fma(p, e.r, 1.0);
  return ldexp(e.tabv * p, e.ni >> 6);
}
// The same with the argument pre-scaled by the caller: t = x * 64/ln2 (fold the factor into whatever
// x is multiplied by anyway).  delta = t - rint(t) is exact, and the series runs in delta with the
// powers of ln2/64 folded into its coefficients: one multiply and one FMA fewer than the form
// above (which forms x * 64/ln2 and then reduces x in two parts).  Same table, same error: the
// rounding of t is the rounding x itself would have had.
constexpr double kExpScale = 92.33248261689366;  // 64 / ln2
__device__ __forceinline__ ExpState exp_table_begin_scaled(double t, const double *tab) {
  ExpState e;
  const double nf = rint(t);
  asm("v_cvt_i32_f64 %0, %1" : "=v"(e.ni) : "v"(nf));  // saturating (see exp_table_begin)
  e.tabv = tab[e.ni & (kExpTab - 1)];
  e.r = t - nf;
  return e;
}
// (sweep_slim_kernel.hpp has this function as two halves, exp_series_scaled + exp_finish_scaled: change them together.)
__device__ __forceinline__ double exp_table_end_scaled(const ExpState &e) {
  // (ln2/64)^k / k!
  constexpr double L = 0.010830424696249145;
  constexpr double c1 = L, c2 = L * L / 2, c3 = L * L * L / 6, c4 = L * L * L * L / 24, c5 = L * L * L * L * L / 120;
  double p;
  const double c4v = c4;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "s"(c5), "v"(e.r), "v"(c4v));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(e.r), "s"(c3));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(e.r), "s"(c2));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(e.r), "s"(c1));
  p = fma(p, e.r, 1.0);
  return ldexp(e.tabv * p, e.ni >> 6);
}
__device__ __forceinline__ double exp_table(double x, const double *tab) {
  return exp_table_end(exp_table_begin(x, tab));
}
__device__ __forceinline__ double exp_table_scaled(double t, const double *tab) {  // t = x * kExpScale
  return exp_table_end_scaled(exp_table_begin_scaled(t, tab));
}

// Optical-depth sum sqrt(pi) Sum_j lead_j Re w_j where some line is within 30 Doppler widths
// (voigt.c:282-289, reference two-rounding velocity): per line either the piecewise polynomial or
// the wing formula, a few dozen instructions inline -- no call, no divergent trapezoid sums.
template <int LINES>
__device__ __forceinline__ double total_near(double lamP, double m0, double m1, double m2,
                                             const double *mult_lds, int L) {
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double *tab = g_lines.near_poly;
  double total = 0.0;  // sqrt(pi) Sum_j lead_j Re w_j, the convention of the wing tier
  if (LINES > 0) {
    const double mm[3] = {m0, m1, m2};
#pragma unroll
    for (int j = 0; j < (LINES > 0 ? LINES : 1); ++j) {
      const double ax = fabs((lamP * mm[j < 3 ? j : 0] - c_light) * inv_s);  // voigt.c:287
      const double f = ax < 30.0
                           ? 1.7724538509055159 * g_lines.leading[j] * near_poly(tab + j * kNearLineDoubles, ax)
                           : g_lines.cwing[j] * wing_core(ax * ax, g_lines.y2[j]);
      total += f;
    }
  } else {
    for (int j = 0; j < L; ++j) {
      const double ax = fabs((lamP * mult_lds[j] - c_light) * inv_s);
      const double f = ax < 30.0
                           ? 1.7724538509055159 * g_lines.leading[j] * near_poly(tab + j * kNearLineDoubles, ax)
                           : g_lines.cwing[j] * wing_core(ax * ax, g_lines.y2[j]);
      total += f;
    }
  }
  return total;
}

// The three-line sum where the wave voted (some lane within 30 Doppler widths of some line): the wing tier's own
// sum with the accurate tier in the terms that need it and nowhere else.  Line by line, under a wave-uniform
// vote of the wing tier's own per-line test: the lanes within reach of line j replace its term by
// sqrt(pi) lead_j Re w_j from the piecewise polynomial, on the reference's two-rounding velocity (voigt.c:287);
// every other lane, and every line nobody voted for, keeps the wing-tier term it has just computed.  Any
// number of lines may be voted.  The terms are then summed as the wing tier sums them.  (total_near<3>, which
// this replaces in the three-line kernels, recomputed all three lines in every lane of a voting wave: the
// lines are thousands of Doppler widths apart, so two of the three, and the far lanes of the third, were
// thrown away.)  The two-rounding |x| of a near lane can exceed the FMA form's by an ulp of the velocity;
// it is held below 32, the end of the table, so the gather stays inside line j's coefficients whatever s says.
__device__ __forceinline__ double near_lines3(double lamP, double m0, double m1, double m2, const WingLines3 &w) {
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double mm[3] = {m0, m1, m2};
  double coef[3], term[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    coef[j] = g_lines.cwing[j];
    term[j] = w.q[j];
    const bool near_j = hi_word(w.s[j]) < 0x408C2000u;
    if (__any(near_j)) {
      if (near_j) {
        const double ax = fmin(fabs((lamP * mm[j] - c_light) * inv_s), 0x1.fffffffffffffp+4);  // voigt.c:287
        coef[j] = 1.7724538509055159 * g_lines.leading[j];
        term[j] = near_poly(g_lines.near_poly + j * kNearLineDoubles, ax);
      }
    }
  }
  return fma(coef[2], term[2], fma(coef[1], term[1], coef[0] * term[0]));
}

// Wing tier for a line count known at run time only: sqrt(pi) Sum_{j<L} lead_j Re w_j by the wing
// formula, from rho = lambda / (1 + z_DLA), kLineUnroll lines at a time -- their scalar loads are
// issued together and their dependent chains (reciprocal, Newton step, degree-4 Horner) interleave;
// line by line, a wave waited for three scalar loads and one ~20-deep chain per line (measured at 31
// lines on 200 x 1500 pixels x 10^4 samples: 115 ms one at a time).  *near: some line j < L is
// within 30 Doppler widths of this lane's pixel (the caller then takes total_near_at).
constexpr int kLineUnroll = 4;
__device__ __forceinline__ double wing_sum_runtime(double rho, double cs, int L, bool *near_out) {
  double total = 0.0;
  bool near = false;
  int j0 = 0;
  for (; j0 + kLineUnroll <= L; j0 += kLineUnroll) {  // whole groups
    double f[kLineUnroll];
#pragma unroll
    for (int u = 0; u < kLineUnroll; ++u) {
      const double x = fma(rho, g_lines.wing[j0 + u].kms, -cs);
      const double x2 = x * x;
      near |= x2 < 900.0;
      f[u] = wing_core(x2, g_lines.wing[j0 + u].y2);
    }
#pragma unroll
    for (int u = 0; u < kLineUnroll; ++u) total = fma(g_lines.wing[j0 + u].cwing, f[u], total);
  }
  for (; j0 < L; ++j0) {  // the last L mod kLineUnroll lines, one at a time (padding the group to
    // four cost 5 ms of 40 at five lines and of 31 at one)
    const double x = fma(rho, g_lines.wing[j0].kms, -cs);
    const double x2 = x * x;
    near |= x2 < 900.0;
    total = fma(g_lines.wing[j0].cwing, wing_core(x2, g_lines.wing[j0].y2), total);
  }
  *near_out = near;
  return total;
}

// The same sum with the reference's multiplier c / (wavelength_j (1 + z)) / 1e8 (voigt.c:278-279) formed
// here, line by line: for kernels that keep no table of it (k_sweep_slim<0>); two divisions per line,
// on the rare pixels within 30 Doppler widths of a line only.
__device__ __forceinline__ double total_near_at(double lamP, double one_plus_z, int L) {
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double *tab = g_lines.near_poly;
  double total = 0.0;
  for (int j = 0; j < L; ++j) {
    const double mult = c_light / (g_lines.wavelength_cm[j] * one_plus_z) / 1e8;
    const double ax = fabs((lamP * mult - c_light) * inv_s);  // voigt.c:287
    const double f = ax < 30.0
                         ? 1.7724538509055159 * g_lines.leading[j] * near_poly(tab + j * kNearLineDoubles, ax)
                         : g_lines.cwing[j] * wing_core(ax * ax, g_lines.y2[j]);
    total += f;
  }
  return total;
}

}  // namespace gpdla
