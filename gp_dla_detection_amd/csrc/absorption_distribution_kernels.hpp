// absorption_distribution_kernels.hpp -- device side of the "absorption distribution" subsystem: per
// pixel of a quasar's unmasked-range grid, the DISTRIBUTION of the clamped broadened absorption abar = min(max(a, 0), 1)
// over the sample tables and the models -- where the moments of 4.12 / 4.21 keep two sums, this keeps the mass at or below
// up to four thresholds, the minimum and the maximum over the support, and a histogram of up to 256 bins, from which the
// quantiles are read.
//
//   k_absorption_init     the accumulators of the call: 0 for the masses, +inf / -inf for minimum / maximum
//   k_absorption_dist     per (selected quasar, range of pixels) and ONE sampled component: ALL samples of the component,
//                         the Voigt stage of k_spectra_moments (sampled_profile.hpp) with the store of the profile replaced
//                         by the reduction below; three stages under one body: the sample's own profile, the refine points
//                         of the quasar's last box (4.28), the gathered product of model DLA(n) (4.21)
//   k_absorption_combine  per selected quasar: the null atom, the cumulative sums and the quantiles, the NaN rows, the status
//
// A block owns PIXELS, not samples: nothing partial leaves the CU.  Wave w of the block takes the 64-sample groups w, w + nw,
// .. in z_DLA order (the groups k_spectra_moments gives its waves, so a sample gets the tier it gets there); a group all of
// whose 64 weights are exactly 0 is skipped before its Voigt work.  Per tile of 16 pixels the wave transposes its 64 x 16
// profiles through LDS as the moments body does; lane (g, t) = (lane >> 4, lane & 15) then walks rows 4 e + g, e = 0 .. 15, of
// pixel t:
//   thresholds  up to four sums in registers, (g0 + g1) + (g2 + g3) by __shfl_xor, added into the wave's accumulator of the
//               pixel in group order;
//   min / max   fmin / fmax by the same shuffles; a sample of weight 0 does not enter;
//   histogram   the wave's own [16][B + 1] histogram in LDS, plain read-modify-write: the four g run one after the other with a
//               wave barrier between them, so the 16 lanes of a pass touch 16 different pixels' histograms and the additions
//               into a bin run in the order (group, g, e).
// At the end the waves are added in wave order, multiplied by the component's model weight p_m and ADDED to the call's
// accumulators in HBM by the one thread that owns the (pixel, plane) -- the components' launches are stream-ordered, so the
// mixture runs in component order.  No floating-point atomic anywhere; a block depends on its own (quasar, range) only, so
// outputs are bit-identical for any selection order, any launch grouping and either form of a table.
// The histogram variant is chosen at LAUNCH (template parameter): a request without bins runs the variant without them, whose
// block owns four tiles and carries the six raw halo values from tile to tile like the moments body.
#pragma once
#include "marginal_continuum_kernels.hpp"  // MixtureArgs' conventions: mixture_row_undefined, kMixMaxSampled
#include "sampled_profile.hpp"
#include "spectra_multi_kernels.hpp"       // kSpectraAverageUndefined
#include "sweep_primitives.hpp"            // kRefineBoxStride

namespace gpdla {

constexpr int kDistMaxThresholds = 4;
constexpr int kDistMaxLevels = 8;
constexpr int kDistMinBins = 8, kDistMaxBins = 256;
constexpr int kDistAcc = kDistMaxThresholds + 2;  // per pixel: the threshold sums, the minimum, the maximum
constexpr int kDistTilesPlain = 4;                // tiles of kProfTile pixels a block owns without bins (with bins: 1)
constexpr int kDistMaxWaves = 4;
constexpr int kDistOwn = 0, kDistBoxed = 1, kDistProduct = 2;  // the three Voigt stages

// doubles of LDS of a block of nw waves (the layout of absorption_dist_body)
__host__ __device__ constexpr size_t absorption_dist_lds_doubles(int nw, bool hist, int bins) {
  return (size_t)kExpTab + (size_t)nw * 64 * (kProfTile + 1) + (size_t)nw * 64 +
         (size_t)nw * (hist ? 1 : kDistTilesPlain) * kDistAcc * kProfTile + (hist ? (size_t)nw * kProfTile * (bins + 1) : 0);
}

struct AbsorptionInitArgs {
  int64_t total;
  int32_t num_thresholds, num_bins;  // planes of prob and hist (0: none)
  double *prob, *amin, *amax, *hist;
};

__global__ __launch_bounds__(256) void k_absorption_init(AbsorptionInitArgs a) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.total; e += step) {
    a.amin[e] = INFINITY;
    a.amax[e] = -INFINITY;
    for (int j = 0; j < a.num_thresholds; ++j) a.prob[j * a.total + e] = 0.0;
    for (int b = 0; b < a.num_bins; ++b) a.hist[b * a.total + e] = 0.0;
  }
}

// Every pointer indexed by entry is the launch group's: entry sl of the group is sel[sl], out_off[sl], w[sl], pm[sl], flag[sl].
struct AbsorptionDistArgs {
  const QuasarMeta *meta;
  const double *lam_pad;
  const double *offset_samples, *nhi;  // boxed: the unit points u, v
  const int32_t *perm;
  const int64_t *sel;
  const int64_t *out_off;
  const double *w;      // [n][S] of this component
  const double *pm;     // [n] model weight of this component: 0 = not evaluated
  const int32_t *flag;  // [n] != 0: the component's row has no weights (k_absorption_combine writes NaN)
  int64_t S;
  int32_t num_lines;
  int32_t ranges;       // blocks per quasar
  int32_t num_bins;
  double thresholds[kDistMaxThresholds];  // past the request's count: -1, which no abar reaches
  int32_t num_thresholds;
  int64_t total;        // the plane stride of prob and hist
  double *prob, *amin, *amax, *hist;
  // kDistBoxed
  const QuasarMeta *rmeta;
  const double *box;
  const int32_t *rstatus;
  // kDistProduct: model DLA(nslots)
  const uint32_t *base;
  const int64_t *base_start;
  int32_t nslots;
};

__device__ __forceinline__ void dist_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int STAGE, bool HIST>
__device__ __forceinline__ void absorption_dist_body(const AbsorptionDistArgs &a) {
  extern __shared__ double s_dist[];
  constexpr int NT = HIST ? 1 : kDistTilesPlain;
  constexpr int kStride = kProfTile + 1;
  const int nw = blockDim.x >> 6;
  const int B = a.num_bins, hstride = B + 1;
  double *s_exp = s_dist;                                   // [kExpTab]
  double *s_out = s_exp + kExpTab;                          // [nw][64][kProfTile + 1]
  double *s_w = s_out + nw * 64 * kStride;                  // [nw][64]
  double *s_acc = s_w + nw * 64;                            // [nw][NT][kDistAcc][kProfTile]
  double *s_hist = s_acc + nw * NT * kDistAcc * kProfTile;  // [nw][kProfTile][B + 1]

  const int64_t sl = blockIdx.x / a.ranges;
  const int range = (int)(blockIdx.x - sl * a.ranges);
  const int64_t q = a.sel[sl];
  const QuasarMeta m = a.meta[q];
  const int P0 = range * NT * kProfTile;
  // (the whole block: no sample redshifts, a component the quasar does not weigh or that has no weights, past the grid)
  if (m.status != 0 || !(a.pm[sl] > 0.0) || a.flag[sl] != 0 || P0 >= m.n_u) return;
  if constexpr (STAGE == kDistBoxed)
    if (a.rstatus[q] != 0) return;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int e = tid; e < kExpTab; e += blockDim.x) s_exp[e] = exp2((double)e * (1.0 / kExpTab));
  for (int e = tid; e < nw * NT * kDistAcc * kProfTile; e += blockDim.x) {
    const int j = (e / kProfTile) % kDistAcc;
    s_acc[e] = j < kDistMaxThresholds ? 0.0 : (j == kDistMaxThresholds ? (double)INFINITY : -(double)INFINITY);
  }
  if constexpr (HIST)
    for (int e = tid; e < nw * kProfTile * hstride; e += blockDim.x) s_hist[e] = 0.0;
  __syncthreads();

  double *so = s_out + wave * 64 * kStride, *sw = s_w + wave * 64;
  double *sacc = s_acc + wave * NT * kDistAcc * kProfTile;
  double *sh = s_hist + wave * kProfTile * hstride;
  const int L = a.num_lines;
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double cs = c_light * inv_s;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;
  const double t0 = g_lines.taps[0], t1 = g_lines.taps[1], t2 = g_lines.taps[2], t3 = g_lines.taps[3],
               t4 = g_lines.taps[4], t5 = g_lines.taps[5], t6 = g_lines.taps[6];
  const double th0 = a.thresholds[0], th1 = a.thresholds[1], th2 = a.thresholds[2], th3 = a.thresholds[3];
  const int g = lane >> 4, tt = lane & 15;  // lane (g, t) walks rows 4 e + g of pixel t
  const double *wrow = a.w + sl * a.S;
  const int64_t ngroups = (a.S + 63) / 64;

  // one profile: the multipliers of the sample at (z, nscale), voigt.c:278-279, and its raw value at a padded pixel
  struct Sample {
    double mult[3], ms[3], inv_opz, z_dla, nscale;
  };
  auto sample_at = [&](double z_dla, double nscale) {
    Sample sm;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      sm.mult[j] = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z_dla)) / 1e8;
      sm.ms[j] = sm.mult[j] * inv_s;
    }
    sm.inv_opz = 1.0 / (1 + z_dla);
    sm.z_dla = z_dla;
    sm.nscale = nscale;
    return sm;
  };
  auto raw = [&](const Sample &sm, int P) -> double {
    const double lamP = lam[min(P, n_pad - 1)];  // wave-uniform address
    return exp_table_scaled(sm.nscale * sampled_line_sum(lamP, sm.mult, sm.ms, cs, sm.inv_opz, sm.z_dla, L), s_exp);
  };
  const double nfac = g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;

  for (int64_t gi = wave; gi < ngroups; gi += nw) {
    const int64_t pos = gi * 64 + lane;
    const bool live = pos < a.S;
    const int64_t i = a.perm[live ? pos : a.S - 1];
    const double wgt = live ? wrow[i] : 0.0;
    if (!__any(wgt > 0.0)) continue;  // wave-uniform: the group adds nothing to any sum and enters no minimum or maximum
    sw[lane] = wgt;
    Sample sm;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6;
    if constexpr (STAGE == kDistOwn) {
      sm = sample_at(m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[i], -a.nhi[i] * nfac);
    } else if constexpr (STAGE == kDistBoxed) {
      const QuasarMeta rm = a.rmeta[q];
      const double *box = a.box + q * kRefineBoxStride;
      sm = sample_at(rm.min_z_dla + (rm.max_z_dla - rm.min_z_dla) * a.offset_samples[i],
                     -exp10(box[2] + (box[3] - box[2]) * a.nhi[i]) * nfac);
    }
    if constexpr (STAGE != kDistProduct) {
      a0 = raw(sm, P0), a1 = raw(sm, P0 + 1), a2 = raw(sm, P0 + 2), a3 = raw(sm, P0 + 3), a4 = raw(sm, P0 + 4), a5 = raw(sm, P0 + 5);
    }
#pragma unroll 1
    for (int tile = 0; tile < NT; ++tile) {
      const int p0 = P0 + tile * kProfTile;
      if (p0 >= m.n_u) break;
      if constexpr (STAGE == kDistProduct) {
        const uint32_t *base = a.base + a.base_start[sl] + i;
        for (int j = 1; j <= a.nslots; ++j) {
          int64_t sj = i;                                 // slot 1: the sample itself
          if (j > 1) {
            const uint32_t b1 = base[(int64_t)(j - 2) * a.S];
            sj = b1 ? (int64_t)b1 - 1 : 0;                // (never drawn: the weight is 0)
          }
          sm = sample_at(m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[sj], -a.nhi[sj] * nfac);
          a0 = raw(sm, p0), a1 = raw(sm, p0 + 1), a2 = raw(sm, p0 + 2), a3 = raw(sm, p0 + 3), a4 = raw(sm, p0 + 4), a5 = raw(sm, p0 + 5);
#pragma unroll
          for (int u = 0; u < kProfTile; ++u) {
            a6 = raw(sm, p0 + u + 6);
            const double acc = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
            so[lane * kStride + u] = (j == 1) ? acc : so[lane * kStride + u] * acc;  // multi :342-351, in slot order
            a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < kProfTile; ++u) {
          a6 = raw(sm, p0 + u + 6);
          so[lane * kStride + u] = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
          a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
        }
      }
      dist_wave_sync();
      double f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0, mn = INFINITY, mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const double wv = sw[4 * e + g];
        const double x = fmin(fmax(so[(4 * e + g) * kStride + tt], 0.0), 1.0);
        f0 += x <= th0 ? wv : 0.0;
        f1 += x <= th1 ? wv : 0.0;
        f2 += x <= th2 ? wv : 0.0;
        f3 += x <= th3 ? wv : 0.0;
        if (wv > 0.0) {
          mn = fmin(mn, x);
          mx = fmax(mx, x);
        }
      }
      f0 += __shfl_xor(f0, 16); f1 += __shfl_xor(f1, 16); f2 += __shfl_xor(f2, 16); f3 += __shfl_xor(f3, 16);
      mn = fmin(mn, __shfl_xor(mn, 16)); mx = fmax(mx, __shfl_xor(mx, 16));
      f0 += __shfl_xor(f0, 32); f1 += __shfl_xor(f1, 32); f2 += __shfl_xor(f2, 32); f3 += __shfl_xor(f3, 32);
      mn = fmin(mn, __shfl_xor(mn, 32)); mx = fmax(mx, __shfl_xor(mx, 32));
      if (lane < kProfTile) {  // (the one lane that ever touches these entries)
        double *acc = sacc + tile * kDistAcc * kProfTile + lane;
        acc[0 * kProfTile] += f0;
        acc[1 * kProfTile] += f1;
        acc[2 * kProfTile] += f2;
        acc[3 * kProfTile] += f3;
        acc[4 * kProfTile] = fmin(acc[4 * kProfTile], mn);
        acc[5 * kProfTile] = fmax(acc[5 * kProfTile], mx);
      }
      if constexpr (HIST) {
        const double Bd = (double)B;
        for (int gg = 0; gg < 4; ++gg) {
          if (g == gg) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const double wv = sw[4 * e + g];
              if (wv > 0.0) {
                const double x = fmin(fmax(so[(4 * e + g) * kStride + tt], 0.0), 1.0);
                const int bin = min(B - 1, (int)(x * Bd));
                sh[tt * hstride + bin] += wv;
              }
            }
          }
          dist_wave_sync();
        }
      } else {
        dist_wave_sync();  // (the reads of so and sw before the next tile's, or group's, writes)
      }
    }
  }
  __syncthreads();

  // the waves in wave order, times the model weight, into the call's accumulators
  const double pm = a.pm[sl];
  const int64_t o = a.out_off[sl];
  for (int e = tid; e < NT * kProfTile; e += blockDim.x) {
    const int p = P0 + e;
    if (p >= m.n_u) continue;
    const int tile = e / kProfTile, t = e - tile * kProfTile;
    const double *acc = s_acc + tile * kDistAcc * kProfTile + t;
    const int wstride = NT * kDistAcc * kProfTile;
    for (int j = 0; j < a.num_thresholds; ++j) {
      double sum = acc[j * kProfTile];
      for (int wv = 1; wv < nw; ++wv) sum += acc[wv * wstride + j * kProfTile];
      a.prob[j * a.total + o + p] += pm * sum;
    }
    double mn = acc[4 * kProfTile], mx = acc[5 * kProfTile];
    for (int wv = 1; wv < nw; ++wv) {
      mn = fmin(mn, acc[wv * wstride + 4 * kProfTile]);
      mx = fmax(mx, acc[wv * wstride + 5 * kProfTile]);
    }
    a.amin[o + p] = fmin(a.amin[o + p], mn);
    a.amax[o + p] = fmax(a.amax[o + p], mx);
  }
  if constexpr (HIST) {
    for (int e = tid; e < B * kProfTile; e += blockDim.x) {
      const int b = e / kProfTile, t = e - b * kProfTile;
      if (P0 + t >= m.n_u) continue;
      double sum = s_hist[t * hstride + b];
      for (int wv = 1; wv < nw; ++wv) sum += s_hist[(wv * kProfTile + t) * hstride + b];
      a.hist[b * a.total + o + P0 + t] += pm * sum;
    }
  }
}

template <int STAGE, bool HIST>
__global__ __launch_bounds__(kDistMaxWaves * 64) void k_absorption_dist(AbsorptionDistArgs a) {
  absorption_dist_body<STAGE, HIST>(a);
}

// ------------------------------------------------------------------------------------------
// k_absorption_combine: one block per selected quasar of the CALL (after its last launch group), a thread per pixel.
//   The null atom of weight p_0 > 0: abar = 1 -- bin B - 1, the maximum, never below a threshold.
//   C_b = H_0 + .. + H_b in ascending b; for level l the first b with C_b >= l (none: B - 1):
//   q = (b + clamp((l - C_{b-1}) / H_b, 0, 1)) / B, clamped to [minimum, maximum].
// status: the quasar's prepare status (1, 3: NaN rows); kSpectraAverageUndefined for a row of model weights with a NaN
// (NaN rows); a component of weight > 0 whose weight row has no weights: NaN rows, status 0.
// pw [nsel][1 + sampled], flag [sampled][nsel].
// ------------------------------------------------------------------------------------------
struct AbsorptionCombineArgs {
  const QuasarMeta *meta;
  const int64_t *sel;
  const int64_t *out_off;
  const double *pw;
  const int32_t *flag;
  int64_t flag_stride;
  int32_t sampled;
  int32_t num_thresholds, num_bins, num_levels;  // num_bins 0: no histogram (and no quantiles)
  double levels[kDistMaxLevels];
  int64_t total;
  double *prob, *amin, *amax, *hist, *quant;     // quant may be nullptr
  int32_t *status;
};

__global__ __launch_bounds__(256) void k_absorption_combine(AbsorptionCombineArgs a) {
  const int64_t s = blockIdx.x;
  const QuasarMeta m = a.meta[a.sel[s]];
  const int64_t o = a.out_off[s];
  const double *P = a.pw + s * (int64_t)(1 + a.sampled);
  const bool undefined = m.status == 0 && mixture_row_undefined(P, a.sampled);
  bool none = m.status != 0 || undefined;
  if (!none)
    for (int comp = 0; comp < a.sampled; ++comp)
      if (P[1 + comp] > 0.0 && a.flag[comp * a.flag_stride + s] != 0) none = true;
  if (threadIdx.x == 0) a.status[s] = m.status != 0 ? m.status : undefined ? kSpectraAverageUndefined : 0;
  const double p0 = none ? 0.0 : P[0];
  const int B = a.num_bins;
  for (int p = threadIdx.x; p < m.n_u; p += 256) {
    const int64_t e = o + p;
    if (none) {
      for (int j = 0; j < a.num_thresholds; ++j) a.prob[j * a.total + e] = NAN;
      a.amin[e] = a.amax[e] = NAN;
      for (int b = 0; b < B; ++b) a.hist[b * a.total + e] = NAN;
      if (a.quant)
        for (int j = 0; j < a.num_levels; ++j) a.quant[j * a.total + e] = NAN;
      continue;
    }
    // (normalised weights add up to 1 within rounding: a reported probability does not exceed 1)
    for (int j = 0; j < a.num_thresholds; ++j) a.prob[j * a.total + e] = fmin(a.prob[j * a.total + e], 1.0);
    double mn = a.amin[e], mx = a.amax[e];
    if (p0 > 0.0) {
      mn = fmin(mn, 1.0);
      mx = 1.0;
      a.amin[e] = mn;
      a.amax[e] = mx;
      if (B > 0) a.hist[(int64_t)(B - 1) * a.total + e] += p0;
    }
    if (!a.quant || B == 0) continue;
    double qv[kDistMaxLevels];
    bool found[kDistMaxLevels];
#pragma unroll
    for (int j = 0; j < kDistMaxLevels; ++j) {
      qv[j] = 0.0;
      found[j] = false;
    }
    double Cprev = 0.0, C = 0.0, H = 0.0;
    for (int b = 0; b < B; ++b) {
      Cprev = C;
      H = a.hist[b * a.total + e];
      C = Cprev + H;
#pragma unroll
      for (int j = 0; j < kDistMaxLevels; ++j)
        if (j < a.num_levels && !found[j] && (C >= a.levels[j] || b == B - 1)) {
          found[j] = true;
          const double frac = fmin(fmax((a.levels[j] - Cprev) / H, 0.0), 1.0);
          qv[j] = ((double)b + frac) / (double)B;
        }
    }
#pragma unroll
    for (int j = 0; j < kDistMaxLevels; ++j)
      if (j < a.num_levels) a.quant[j * a.total + e] = fmin(fmax(qv[j], mn), mx);
  }
}

}  // namespace gpdla
