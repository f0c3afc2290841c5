// sampled_profile.hpp -- "the broadened Voigt profile of sample i at padded pixel P", the stage that k_profiles
// (multi_kernels.hpp), k_spectra_moments(_multi) (spectra_moments_body.hpp), k_mc_contract(_multi) (mc_contract_body.hpp)
// and k_pf_pixels(_multi) (pf_pixels_body.hpp) share, as functions.  A kernel keeps the sample's
// multipliers (voigt.c:278-279: mult[j], ms[j] = mult[j] / (sqrt2 sigma), cs, inv_opz) and the seven taps in registers
// of its own and hands them in: with them formed in here the compiled kernels change (tools/isa_diff.py), with them
// handed in every kernel compiles to the instructions it had with the text written out.
#pragma once
#include "voigt_tiers.hpp"

namespace gpdla {

// voigt.c:282-290: sqrt(pi) Sum_j lead_j Re w_j of the sample at z_dla, at the padded wavelength lamP, in two tiers.
// The wing tier: wing_sum3 at the production's three lines (L == 3), wing_sum_runtime at a run-time count.  Where any
// lane of the wave is within 30 Doppler widths of a line the WHOLE wave takes the accurate tier instead (wave-uniformly:
// which tier a sample gets depends on the samples of its wave alone): per line the piecewise polynomial of
// near_tables.hpp on the reference's two-rounding velocity (:287), or the wing formula beyond 30 widths; total_near_at
// at a run-time count.  Every caller multiplies the sum by its own pre-scaled -N / (sqrt2pi sigma sqrt(pi)) 64 / ln2 and
// takes exp_table_scaled of it (:291).
__device__ __forceinline__ double sampled_line_sum(double lamP, const double (&mult)[3], const double (&ms)[3], double cs,
                                                   double inv_opz, double z_dla, int L) {
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  double total;
  bool near = false;
  if (L == 3) total = wing_sum3(lamP, ms[0], ms[1], ms[2], cs, &near);
  else total = wing_sum_runtime(lamP * inv_opz, cs, L, &near);
  if (__any(near)) {  // accurate tier, wave-uniformly
    if (L == 3) {
      total = 0.0;
      for (int j = 0; j < 3; ++j) {
        const double ax = fabs((lamP * mult[j] - c_light) * inv_s);
        total += ax < 30.0 ? 1.7724538509055159 * g_lines.leading[j] *
                                 near_poly(g_lines.near_poly + j * kNearLineDoubles, ax)
                           : g_lines.cwing[j] * wing_core(ax * ax, g_lines.y2[j]);
      }
    } else {
      total = total_near_at(lamP, 1 + z_dla, L);
    }
  }
  return total;
}

// voigt.c:297-299: the instrument broadening of seven consecutive raw values, taps in ascending order.
__device__ __forceinline__ double tap_fold(double a0, double a1, double a2, double a3, double a4, double a5, double a6,
                                           double t0, double t1, double t2, double t3, double t4, double t5, double t6) {
  double acc = a0 * t0;
  acc = fma(a1, t1, acc);
  acc = fma(a2, t2, acc);
  acc = fma(a3, t3, acc);
  acc = fma(a4, t4, acc);
  acc = fma(a5, t5, acc);
  acc = fma(a6, t6, acc);
  return acc;
}

}  // namespace gpdla
