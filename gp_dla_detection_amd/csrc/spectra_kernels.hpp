// spectra_kernels.hpp -- device side of the "model spectra" subsystem: what the
// fitted model looks like on a spectrum, per pixel of the quasar's unmasked-range grid (the n_u
// stored pixels with rest wavelength in [min_lambda, max_lambda], masked or not -- the grid
// k_prepare lays out and the Voigt stage of every sweep walks).
//
//   k_spectra_map        process_qsos.m:187-190 (multi :342-351)  product of the instrument-broadened
//                                                 Voigt profiles of a list of absorbers        (P1)
//   k_spectra_weights    posterior weights of the S samples of a quasar from a row of sample
//                        log-likelihoods: w_i = exp(l_i - max l) / Sum                           (P2)
//   k_spectra_moments    Sum_i w_i (1 - a_i(p)) and Sum_i w_i (1 - a_i(p))^2 over 256 samples of a
//                        quasar, a_i the broadened profile of sample i -- the hot kernel         (P2)
//   k_spectra_combine    the chunks of k_spectra_moments in chunk order -> mean, variance        (P2)
//   k_spectra_continuum  GP posterior mean of the low-rank continuum under a chosen absorption  (P3)
//   k_spectra_model_mean qso_loader.py:1685-1711: mu x mean-flux suppression x raw profiles on the
//                        model's rest grid                                                       (P4)
//
// Every sum runs in a fixed order and nothing is accumulated with atomics: outputs are bit-identical
// from run to run and depend on their own quasar only.
#pragma once
#include "continuum_solve.hpp"
#include "sampled_profile.hpp"
#include "sweep_primitives.hpp"  // kRefineBoxStride

namespace gpdla {

constexpr int kSpectraMaxAbsorbers = 8;

// voigt.c:278-291 at one wavelength, with the arithmetic of k_voigt_raw (gpdla_voigt's tiers).
__device__ __forceinline__ double spectra_raw_at(double lambda, double z, double N, int num_lines) {
  double total = 0.0;
  for (int j = 0; j < num_lines; ++j) {
    const double mult = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z)) / 1e8;  // voigt.c:279
    const double velocity = lambda * mult - g_lines.c;                           // voigt.c:287
    const double v = rew_full(velocity * g_lines.inv_sqrt2_sigma, g_lines.y[j]) * g_lines.inv_sqrt2pi_sigma;
    total += -g_lines.leading[j] * v;                                            // voigt.c:288
  }
  return exp(N * total);                                                         // voigt.c:291
}

// ------------------------------------------------------------------------------------------
// k_spectra_map: one block per selected quasar.  A tile of 250 output pixels needs 256 raw values;
// each thread evaluates one, the block broadens (voigt.c:297-299, taps in ascending order like
// k_voigt_broaden) and multiplies the absorbers in list order.  A quasar without a kept pixel has
// no padded grid (k_prepare writes the six padding wavelengths only then): its row is NaN.
// ------------------------------------------------------------------------------------------
struct SpectraMapArgs {
  const QuasarMeta *meta;
  const double *lam_pad;
  const int64_t *sel;       // [nsel] quasar of the batch
  const int64_t *abs_off;   // [nsel + 1] into abs_z / abs_n, or nullptr: no absorbers anywhere
  const double *abs_z, *abs_n;
  const int64_t *out_off;   // [nsel + 1]
  int32_t num_lines;
  double *out;
};

constexpr int kMapTile = 250;

__global__ __launch_bounds__(256) void k_spectra_map(SpectraMapArgs a) {
  __shared__ double s_raw[256];
  const int s = blockIdx.x, tid = threadIdx.x;
  const QuasarMeta m = a.meta[a.sel[s]];
  const double *lam = a.lam_pad + m.lam_off;
  double *out = a.out + a.out_off[s];
  const int64_t j0 = a.abs_off ? a.abs_off[s] : 0, j1 = a.abs_off ? a.abs_off[s + 1] : 0;
  const int n_pad = m.n_u + 6;
  for (int t0 = 0; t0 < m.n_u; t0 += kMapTile) {
    double prod = 1.0;
    for (int64_t j = j0; j < j1; ++j) {
      const int P = t0 + tid;
      if (P < n_pad) s_raw[tid] = spectra_raw_at(lam[P], a.abs_z[j], a.abs_n[j], a.num_lines);
      __syncthreads();
      if (tid < kMapTile && P < m.n_u) {
        double acc = 0.0;
        for (int kk = 0; kk < 7; ++kk) acc += s_raw[tid + kk] * g_lines.taps[kk];
        prod = (j == j0) ? acc : prod * acc;
      }
      __syncthreads();
    }
    if (tid < kMapTile && t0 + tid < m.n_u) out[t0 + tid] = m.n_kept > 0 ? prod : NAN;
  }
}

// ------------------------------------------------------------------------------------------
// k_spectra_weights: one block per selected quasar.  Row s of sample log-likelihoods starts at
// table + row_start[s].  w_i = exp(l_i - max l) / Sum_j exp(l_j - max l); a NaN l_i weighs 0.
// flag[s] = 1 when no entry is above -inf (an all-NaN row, or a quasar whose log-likelihoods are all
// -inf): its outputs are NaN.
// ------------------------------------------------------------------------------------------
struct SpectraWeightsArgs {
  const double *table;
  const int64_t *row_start;  // [nsel]
  int64_t S;
  double *w;                 // [nsel][S]
  int32_t *flag;             // [nsel]
};

__global__ __launch_bounds__(256) void k_spectra_weights(SpectraWeightsArgs a) {
  __shared__ double s_red[4];
  const int s = blockIdx.x, tid = threadIdx.x;
  const double *row = a.table + a.row_start[s];
  double *w = a.w + (int64_t)s * a.S;
  double mx = -INFINITY;
  for (int64_t i = tid; i < a.S; i += 256) mx = fmax(mx, row[i]);  // (fmax returns the other operand for a NaN)
  mx = block_reduce_minmax(mx, false, s_red);
  const bool none = !(mx > -INFINITY) || mx == INFINITY;
  double sum = 0.0;
  for (int64_t i = tid; i < a.S; i += 256) {
    const double l = row[i];
    const double e = (l == l) ? exp(l - mx) : 0.0;
    w[i] = e;
    sum += e;
  }
  sum = block_reduce_sum(sum, s_red);
  for (int64_t i = tid; i < a.S; i += 256) w[i] = none ? 0.0 : w[i] / sum;
  if (tid == 0) a.flag[s] = none ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// k_spectra_moments: the Voigt stage of k_profiles -- one LANE per sample, 64 neighbours in z_DLA
// per wave walking the padded pixels in lockstep, seven raw values in registers for the instrument
// broadening, the accurate tier taken by whole waves -- with the store of the profile replaced by
// its reduction.  A block is four waves = 256 consecutive samples (in z_DLA order) of one quasar.
// Per tile of 16 pixels a wave transposes its 64 x 16 broadened values through LDS; lane (g, t) =
// (lane >> 4, lane & 15) then adds rows 4 e + g, e = 0 .. 15, of pixel t in that order, the four g
// are combined as (g0 + g1) + (g2 + g3), the four waves in wave order, and the block writes its
// two partial sums per pixel.  What is summed is the absorbed fraction b = 1 - a, not a: where the
// profiles are ~1 the moments then keep their relative accuracy.  No per-sample profile reaches HBM.
// part[((sl * chunks + chunk) * 2 + moment) * stride + p]
// ------------------------------------------------------------------------------------------
struct SpectraMomentsArgs {
  const QuasarMeta *meta;
  const double *lam_pad;
  const double *offset_samples, *nhi;  // nhi: nhi_samples, or lls_nhi_samples for the sub-DLA model
  const int32_t *perm;
  const int64_t *sel;   // [nsel]; this launch takes sel[s0 .. s0 + nsub)
  const double *w;      // [nsel][S]
  int64_t S;
  int32_t num_lines;
  int64_t s0;
  int32_t chunks;       // ceil(S / 256): blocks per quasar
  int64_t stride;       // >= n_u of every selected quasar
  double *part;
};

constexpr int kMomWaves = 4;

// The body is spectra_moments_body.hpp, which k_spectra_moments_multi (spectra_multi_kernels.hpp) includes as well.
__global__ __launch_bounds__(kMomWaves * 64) void k_spectra_moments(SpectraMomentsArgs a) {
#define GPDLA_SPECTRA_MOMENTS_MULTI 0
#include "spectra_moments_body.hpp"
#undef GPDLA_SPECTRA_MOMENTS_MULTI
}

// ------------------------------------------------------------------------------------------
// k_spectra_moments_boxed: k_spectra_moments over the refine points of a refined batch.  The samples
// are the context's S' unit points (m.offset_samples = u, m.nhi = v, m.perm the order of u, m.S = S', m.w the weights of the
// resident lambda rows) mapped through the quasar's last box: z' = z_lo + (z_hi - z_lo) u with the range read from the
// refine's copy of the metadata, N' = exp10(n_lo + (n_hi - n_lo) v) -- the boxed sweep's own two expressions.  Everything
// after the prologue is k_spectra_moments; a quasar whose refine status is not 0 has no box and is not evaluated.
// ------------------------------------------------------------------------------------------
struct SpectraMomentsBoxedArgs {
  SpectraMomentsArgs m;
  const QuasarMeta *rmeta;  // [nq] the refine's copy: min_z_dla, max_z_dla are the last box's z_lo, z_hi
  const double *box;        // quasar q's LAST box at box + q * kRefineBoxStride: (z_lo, z_hi, n_lo, n_hi)
  const int32_t *rstatus;   // [nq] refine status: 0 = the quasar has a box and a lambda row
};

__global__ __launch_bounds__(kMomWaves * 64) void k_spectra_moments_boxed(SpectraMomentsBoxedArgs bx) {
  const SpectraMomentsArgs &a = bx.m;
#define GPDLA_SPECTRA_MOMENTS_MULTI 0
#define GPDLA_SPECTRA_MOMENTS_BOXED
#include "spectra_moments_body.hpp"
#undef GPDLA_SPECTRA_MOMENTS_BOXED
#undef GPDLA_SPECTRA_MOMENTS_MULTI
}

// ------------------------------------------------------------------------------------------
// k_spectra_combine: one block per selected quasar of a launch of k_spectra_moments; the chunks in
// chunk order.  mean = 1 - Sum w b, var = Sum w b^2 - (Sum w b)^2 (never negative).
// ------------------------------------------------------------------------------------------
struct SpectraCombineArgs {
  const QuasarMeta *meta;
  const int64_t *sel;
  const int32_t *flag;
  const int64_t *out_off;
  const double *part;
  int64_t s0;
  int32_t chunks;
  int64_t stride;
  double *mean, *var;
};

__global__ __launch_bounds__(256) void k_spectra_combine(SpectraCombineArgs a) {
  const int64_t sl = blockIdx.x, s = a.s0 + sl;
  const QuasarMeta m = a.meta[a.sel[s]];
  const bool none = m.status != 0 || a.flag[s] != 0;
  const double *part = a.part + (sl * a.chunks * 2) * a.stride;
  double *mean = a.mean + a.out_off[s], *var = a.var + a.out_off[s];
  for (int p = threadIdx.x; p < m.n_u; p += 256) {
    double m1 = 0.0, m2 = 0.0;
    if (!none)
      for (int c = 0; c < a.chunks; ++c) {
        m1 += part[(2 * c) * a.stride + p];
        m2 += part[(2 * c + 1) * a.stride + p];
      }
    mean[p] = none ? NAN : 1.0 - m1;
    var[p] = none ? NAN : fmax(m2 - m1 * m1, 0.0);
  }
}

// ------------------------------------------------------------------------------------------
// k_spectra_continuum: one block per selected quasar.  With the prepared rows of k_prepare (y, mu, M,
// omega2, nu; a masked pixel is the neutral row y = mu = omega2 = 0, nu = 1, M = 0 and drops out of
// every sum) and a = the absorption on the grid (nullptr: ones, the null model):
//   d = a^2 omega2 + nu,  r = y - a mu,  B = I + M' diag(a^2 / d) M,  c = B^-1 M' (a r / d)
// which is the posterior mean of the coefficients of the low-rank part of the covariance
// (log_mvnpdf_low_rank.m's B and its right-hand side, solved instead of folded into the
// likelihood): continuum_null_solve (continuum_solve.hpp), which k_mc_finish and k_pf_finish call with a = 1.
// continuum = mu + M c is evaluated at ALL n_u pixels -- a masked pixel's mu and M row
// are interpolated here as k_prepare interpolates a kept one -- and model_flux = a continuum.  The
// pixel-diagonal omega term has no posterior mean away from the pixel that measured it and is left
// out.  B not positive definite: NaN rows and status 4.
// The shapes the edge tests are built around (tests/model_spectra_edge_cases.py): the solve stages the pixel weights
// kContTile at a time, and thread tid of the 256 accumulates the entries of [vech(B) | v] that the solve enumerates as
//   const int e = tid + 256 * t;
// ------------------------------------------------------------------------------------------
struct SpectraContinuumArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *Mi;
  const double *lam_pad;
  const double *z_qsos;
  const int64_t *sel;
  const int64_t *out_off;
  const double *absorption;  // on the output layout, or nullptr
  ContinuumModelArgs g;
  double *continuum, *model_flux;  // either may be nullptr
  int32_t *status;                 // [nsel]
};

constexpr int kContTile = 128;  // pixels staged at a time by continuum_null_solve, here and in the two finish kernels

__global__ __launch_bounds__(256) void k_spectra_continuum(SpectraContinuumArgs a) {
  constexpr int kNb = GPDLA_MAX_K * (GPDLA_MAX_K + 1) / 2;
  __shared__ double s_B[kNb + GPDLA_MAX_K];  // packed lower triangle of B / L, then v (then c)
  __shared__ double s_wt[kContTile], s_ut[kContTile];
  __shared__ double s_piv;
  __shared__ int s_pd;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int64_t q = a.sel[s];
  const QuasarMeta m = a.meta[q];
  const ModelDev &model = a.g.model;
  const int k = model.k, G = model.G;
  const PixelRow *pix = a.pix + m.pix_off;
  const double *Mi = a.Mi + m.pix_off * k;
  const double *absn = a.absorption ? a.absorption + a.out_off[s] : nullptr;
  double *cont = a.continuum ? a.continuum + a.out_off[s] : nullptr;
  double *flux = a.model_flux ? a.model_flux + a.out_off[s] : nullptr;
  if (m.status != 0) {  // no kept pixel, or a kept pixel of unusable noise variance: nothing to condition on
    for (int p = tid; p < m.n_u; p += 256) {
      if (cont) cont[p] = NAN;
      if (flux) flux[p] = NAN;
    }
    if (tid == 0) a.status[s] = m.status;
    return;
  }
  if (tid == 0) s_pd = 1;
  continuum_null_solve<kContTile>(pix, Mi, m.n_u, k, absn, s_B, s_wt, s_ut, &s_piv, &s_pd, tid);
  if (tid == 0) a.status[s] = s_pd ? 0 : 4;
  __syncthreads();
  const bool pd = s_pd != 0;
  const double *v = s_B + k * (k + 1) / 2;  // c
  // mu + M c on the whole grid, a thread per pixel: the interpolation of k_prepare (process_qsos.m:138-139, multi :287-288)
  const double *lam = a.lam_pad + m.lam_off + 3;
  const double z_qso = a.z_qsos[q];
  for (int p = tid; p < m.n_u; p += 256) {
    const double wl = lam[p];
    int lo;
    const double t = model_bracket(model, wl / (1 + z_qso), &lo);
    const double mf = a.g.mean_flux(wl, z_qso);
    double val = model.mu[lo] + (model.mu[lo + 1] - model.mu[lo]) * t;
    if (a.g.meanflux) val = val * mf;
    for (int c = 0; c < k; ++c) {
      const double m0 = model.M[lo + (int64_t)c * G], m1 = model.M[lo + 1 + (int64_t)c * G];
      val = fma((m0 + (m1 - m0) * t) * mf, v[c], val);
    }
    if (!pd) val = NAN;
    if (cont) cont[p] = val;
    if (flux) flux[p] = (absn ? absn[p] : 1.0) * val;
  }
}

// ------------------------------------------------------------------------------------------
// k_spectra_model_mean: qso_loader.py:1685-1711 as data.  Item it, grid point g:
//   mu[g] x (suppressed: total_scale_factor at rest[g] (1 + z_qso), :1777-1822)
//         x Prod_j raw profile of absorber j at rest[g] (1 + z_qso) (Voigt_absorption: no broadening),
// multiplied in that order.
// ------------------------------------------------------------------------------------------
struct SpectraModelMeanArgs {
  const double *rest, *mu;
  int32_t G;
  int64_t num_items;
  const double *z_qsos;
  const int64_t *abs_off;  // [num_items + 1]
  const double *abs_z, *abs_n;
  int32_t num_voigt_lines, num_forest_lines, suppressed;
  double lya_wavelength, prev_tau_0, prev_beta;
  double *out;  // [num_items][G]
};

__global__ __launch_bounds__(256) void k_spectra_model_mean(SpectraModelMeanArgs a) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= a.num_items * a.G) return;
  const int64_t it = e / a.G;
  const int g = (int)(e - it * a.G);
  const double z_qso = a.z_qsos[it];
  const double wl = a.rest[g] * (1 + z_qso);
  double val = a.mu[g];
  if (a.suppressed)
    val = val * spectra_mean_flux(wl, z_qso, a.lya_wavelength, a.prev_tau_0, a.prev_beta, a.num_forest_lines);
  for (int64_t j = a.abs_off[it]; j < a.abs_off[it + 1]; ++j)
    val = val * spectra_raw_at(wl, a.abs_z[j], a.abs_n[j], a.num_voigt_lines);
  a.out[e] = val;
}

}  // namespace gpdla
