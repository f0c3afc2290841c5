// spectra_multi_kernels.hpp -- device side of the model spectra of a multi-DLA run: the
// per-pixel absorption averaged over the samples of every model DLA(n), n >= 2, and over the models.
//
//   k_spectra_weights_multi  the posterior weights of the S samples of model DLA(n) of a quasar: the rule of
//                            k_spectra_weights on row n - 1 of sample_log_likelihoods_dla, with a sample that
//                            consumes a base index of 0 ("never drawn") read as a NaN log-likelihood
//   k_spectra_moments_multi  Sum_i w_i b_i(p) and Sum_i w_i b_i(p)^2, b = 1 - A_{n,i}, A_{n,i} = Prod_j c_{s_j(i)}
//                            the product of the n instrument-broadened profiles of sample i's slots
//                            (multi :342-351), over 256 samples of one (quasar, model) -- the hot kernel
//   k_spectra_model_average  1 - Sum_m P_m Sum w b and the variance of the mixture over the models, from the
//                            partial sums of every model
//
// Model DLA(1) and the sub-DLA model are k_spectra_moments' (spectra_kernels.hpp); every model's chunks are
// combined by k_spectra_combine.  Sums run in a fixed order, nothing is accumulated with atomics and an
// entry is reduced on its own: outputs are bit-identical from run to run and for any grouping.
#pragma once
#include "spectra_kernels.hpp"

namespace gpdla {

// ------------------------------------------------------------------------------------------
// k_spectra_weights_multi: one block per (entry, model) of models n_lo .. n_hi (n_lo >= 2).  Entry s reads
// row table + row_start[s] + (n - 1) S and the base rows base + base_start[s] + (j - 2) S, j = 2 .. n (1-based
// indices, 0 = never drawn).  w[(n cap + s) S + i] and flag[n flag_stride + s] as k_spectra_weights writes them.
// ------------------------------------------------------------------------------------------
struct SpectraWeightsMultiArgs {
  const double *table;
  const int64_t *row_start;   // [n]
  const uint32_t *base;
  const int64_t *base_start;  // [n]
  int64_t S, cap, flag_stride;
  int32_t n_lo, n_hi;
  double *w;                  // [1 + max_dlas][cap][S]: row 0 the sub-DLA model, row n model DLA(n)
  int32_t *flag;              // [1 + max_dlas][flag_stride]
};

__global__ __launch_bounds__(256) void k_spectra_weights_multi(SpectraWeightsMultiArgs a) {
  __shared__ double s_red[4];
  const int nm = a.n_hi - a.n_lo + 1;
  const int64_t s = blockIdx.x / nm;
  const int n = a.n_lo + (int)(blockIdx.x - s * nm), tid = threadIdx.x;
  const double *row = a.table + a.row_start[s] + (int64_t)(n - 1) * a.S;
  const uint32_t *base = a.base + a.base_start[s];
  double *w = a.w + ((int64_t)n * a.cap + s) * a.S;
  auto value = [&](int64_t i) -> double {  // the log-likelihood, NaN where a slot was never drawn
    bool drawn = true;
    for (int j = 2; j <= n; ++j) drawn = drawn && base[(int64_t)(j - 2) * a.S + i] != 0;
    return drawn ? row[i] : NAN;
  };
  double mx = -INFINITY;
  for (int64_t i = tid; i < a.S; i += 256) mx = fmax(mx, value(i));  // (fmax returns the other operand for a NaN)
  mx = block_reduce_minmax(mx, false, s_red);
  const bool none = !(mx > -INFINITY) || mx == INFINITY;
  double sum = 0.0;
  for (int64_t i = tid; i < a.S; i += 256) {
    const double l = value(i);
    const double e = (l == l) ? exp(l - mx) : 0.0;
    w[i] = e;
    sum += e;
  }
  sum = block_reduce_sum(sum, s_red);
  for (int64_t i = tid; i < a.S; i += 256) w[i] = none ? 0.0 : w[i] / sum;
  if (tid == 0) a.flag[(int64_t)n * a.flag_stride + s] = none ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// k_spectra_moments_multi: the decomposition of k_spectra_moments -- one LANE per sample, a wave of 64
// neighbours in z_DLA, a block of four waves = 256 samples of one (entry, model), 16-pixel tiles transposed
// through LDS, rows 4 e + g, then (g0 + g1) + (g2 + g3), the waves in wave order -- with the profile of a
// sample replaced by the product over its slots.  The slots are looped INSIDE the tile: slot j's line sums
// are evaluated at the tile's 22 padded pixels (the six carried raw values are recomputed: 22 / 16 of the
// line sums, nothing kept per slot in registers or LDS), broadened with the taps in ascending order and
// multiplied into the lane's own s_out row in slot order -- a lane owns its row until the transpose, so
// this needs no barrier.  Each slot takes the accurate tier under its own __any(near): the own samples of
// a wave are neighbours in z_DLA, the gathered ones are wherever the resampling put them.
// A sample of weight 0 (a NaN log-likelihood, a slot never drawn) is evaluated like any other and drops
// out of the sums; its missing slot reads sample 0.
// part[(((n cap + sl) chunks + chunk) 2 + moment) stride + p]
// ------------------------------------------------------------------------------------------
struct SpectraMomentsMultiArgs {
  const QuasarMeta *meta;
  const double *lam_pad;
  const double *offset_samples, *nhi;
  const int32_t *perm;
  const int64_t *sel;         // [n] quasars of the batch
  const uint32_t *base;
  const int64_t *base_start;  // [n]
  const double *w;            // [1 + max_dlas][cap][S]
  const int32_t *flag;        // [1 + max_dlas][flag_stride]
  int64_t S, cap, flag_stride;
  int32_t num_lines, n_lo, n_hi;
  int32_t chunks;
  int64_t stride;
  double *part;
};

__global__ __launch_bounds__(kMomWaves * 64) void k_spectra_moments_multi(SpectraMomentsMultiArgs a) {
  __shared__ double s_exp[kExpTab];
  __shared__ double s_out[kMomWaves][64][kProfTile + 1];
  __shared__ double s_w[kMomWaves][64];
  __shared__ double s_part[2][kMomWaves][2][kProfTile];

  for (int e = threadIdx.x; e < kExpTab; e += kMomWaves * 64) s_exp[e] = exp2((double)e * (1.0 / kExpTab));
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nm = a.n_hi - a.n_lo + 1;
  const int64_t item = blockIdx.x / a.chunks;     // (entry, model)
  const int chunk = (int)(blockIdx.x - item * a.chunks);
  const int64_t sl = item / nm;
  const int n = a.n_lo + (int)(item - sl * nm);
  const QuasarMeta m = a.meta[a.sel[sl]];
  // (the whole block: no sample redshifts, or no weight -- k_spectra_combine writes NaN without reading)
  if (m.status != 0 || a.flag[(int64_t)n * a.flag_stride + sl] != 0) return;
  const int L = a.num_lines;
  const int64_t pos = (int64_t)chunk * (kMomWaves * 64) + wave * 64 + lane;
  const bool live = pos < a.S;
  const int64_t i = a.perm[live ? pos : a.S - 1];
  s_w[wave][lane] = live ? a.w[((int64_t)n * a.cap + sl) * a.S + i] : 0.0;
  __syncthreads();
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double cs = c_light * inv_s;
  const uint32_t *base = a.base + a.base_start[sl] + i;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;
  const double t0 = g_lines.taps[0], t1 = g_lines.taps[1], t2 = g_lines.taps[2], t3 = g_lines.taps[3],
               t4 = g_lines.taps[4], t5 = g_lines.taps[5], t6 = g_lines.taps[6];

  // lane (g, t) adds up rows 4 e + g of pixel t; their 16 weights stay in s_w (read again every tile: next to
  // n x 22 line sums the 16 LDS reads are nothing, and 32 registers are not held across the slot loop)
  const int g = lane >> 4, tt = lane & 15;

  double *part = a.part + ((((int64_t)n * a.cap + sl) * a.chunks + chunk) * 2) * a.stride;
  int buf = 0;
  for (int p0 = 0; p0 < m.n_u; p0 += kProfTile, buf ^= 1) {
    for (int j = 1; j <= n; ++j) {
      int64_t sj = i;                                 // slot 1: the sample itself
      if (j > 1) {
        const uint32_t b1 = base[(int64_t)(j - 2) * a.S];
        sj = b1 ? (int64_t)b1 - 1 : 0;                // (never drawn: the weight is 0)
      }
      const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[sj];
      double mult[3], ms[3];
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        mult[l] = g_lines.c / (g_lines.wavelength_cm[l] * (1 + z_dla)) / 1e8;  // voigt.c:278-279
        ms[l] = mult[l] * inv_s;
      }
      const double inv_opz = 1.0 / (1 + z_dla);
      const double nscale = -a.nhi[sj] * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;

      auto raw = [&](int P) -> double {  // voigt.c:282-291 for slot j's sample at padded pixel P (as k_spectra_moments)
        const double lamP = lam[min(P, n_pad - 1)];  // wave-uniform address
        double total;
        bool near = false;
        if (L == 3) total = wing_sum3(lamP, ms[0], ms[1], ms[2], cs, &near);
        else total = wing_sum_runtime(lamP * inv_opz, cs, L, &near);
        if (__any(near)) {  // accurate tier, wave-uniformly
          if (L == 3) {
            total = 0.0;
            for (int l = 0; l < 3; ++l) {
              const double ax = fabs((lamP * mult[l] - c_light) * inv_s);
              total += ax < 30.0 ? 1.7724538509055159 * g_lines.leading[l] *
                                       near_poly(g_lines.near_poly + l * kNearLineDoubles, ax)
                                 : g_lines.cwing[l] * wing_core(ax * ax, g_lines.y2[l]);
            }
          } else {
            total = total_near_at(lamP, 1 + z_dla, L);
          }
        }
        return exp_table_scaled(nscale * total, s_exp);
      };

      double a0 = raw(p0), a1 = raw(p0 + 1), a2 = raw(p0 + 2), a3 = raw(p0 + 3), a4 = raw(p0 + 4), a5 = raw(p0 + 5), a6;
#pragma unroll
      for (int u = 0; u < kProfTile; ++u) {
        a6 = raw(p0 + u + 6);
        double acc = a0 * t0;  // voigt.c:297-299, taps in ascending order
        acc = fma(a1, t1, acc);
        acc = fma(a2, t2, acc);
        acc = fma(a3, t3, acc);
        acc = fma(a4, t4, acc);
        acc = fma(a5, t5, acc);
        acc = fma(a6, t6, acc);
        s_out[wave][lane][u] = (j == 1) ? acc : s_out[wave][lane][u] * acc;  // multi :342-351, in slot order
        a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const double b = 1.0 - s_out[wave][4 * e + g][tt];
      const double t = s_w[wave][4 * e + g] * b;
      m1 += t;
      m2 = fma(t, b, m2);
    }
    m1 += __shfl_xor(m1, 16);
    m2 += __shfl_xor(m2, 16);
    m1 += __shfl_xor(m1, 32);
    m2 += __shfl_xor(m2, 32);
    if (lane < kProfTile) {
      s_part[buf][wave][0][lane] = m1;
      s_part[buf][wave][1][lane] = m2;
    }
    // one barrier a tile, as in k_spectra_moments: s_part is double-buffered, and the barrier orders this
    // wave's reads of s_out before its writes of the next tile
    __syncthreads();
    if (threadIdx.x < 2 * kProfTile) {
      const int mom = threadIdx.x >> 4, t = threadIdx.x & 15;
      double sum = s_part[buf][0][mom][t];
#pragma unroll
      for (int w = 1; w < kMomWaves; ++w) sum += s_part[buf][w][mom][t];
      if (p0 + t < m.n_u) part[mom * a.stride + p0 + t] = sum;
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_spectra_model_average: one block per entry.  With P = (P_null, P_lls, P_1 .. P_md) the entry's model
// weights and mb_m(p) = Sum w b, m2_m(p) = Sum w b^2 of model m (its chunks in chunk order, as
// k_spectra_combine adds them):
//   Eb = P_lls mb_lls + Sum_n P_n mb_n,  Eb2 = P_lls m2_lls + Sum_n P_n m2_n   (sub-DLA, DLA(1), .., DLA(md))
//   expected = 1 - Eb,  variance = max(Eb2 - Eb^2, 0)
// The null model absorbs nothing.  A model of weight 0 is skipped, flagged or not; a NaN weight, or a weight
// on a flagged model, leaves the entry's two rows NaN and sets kSpectraAverageUndefined in its status.
// ------------------------------------------------------------------------------------------
constexpr int32_t kSpectraAverageUndefined = 8;  // GPDLA_SPECTRA_AVERAGE_UNDEFINED

struct SpectraModelAverageArgs {
  const QuasarMeta *meta;
  const int64_t *sel;         // [n]
  const int64_t *out_off;     // [n + 1]
  const int32_t *flag;        // [1 + max_dlas][flag_stride]
  const double *weights;      // [n][2 + max_dlas]
  const double *part;
  int64_t cap, flag_stride;
  int32_t md, chunks;
  int64_t stride;
  double *expected, *expected_var;
  int32_t *status;            // [n]
};

__global__ __launch_bounds__(256) void k_spectra_model_average(SpectraModelAverageArgs a) {
  const int64_t sl = blockIdx.x;
  const QuasarMeta m = a.meta[a.sel[sl]];
  const double *P = a.weights + sl * (2 + a.md);
  bool undefined = P[0] != P[0];
  for (int r = 0; r <= a.md; ++r) {
    const double pr = P[1 + r];
    undefined = undefined || pr != pr || (pr != 0.0 && a.flag[(int64_t)r * a.flag_stride + sl] != 0);
  }
  const bool none = m.status != 0 || undefined;
  double *ex = a.expected + a.out_off[sl], *ev = a.expected_var + a.out_off[sl];
  for (int p = threadIdx.x; p < m.n_u; p += 256) {
    double eb = 0.0, eb2 = 0.0;
    if (!none)
      for (int r = 0; r <= a.md; ++r) {
        const double pr = P[1 + r];
        if (pr == 0.0) continue;
        const double *part = a.part + (((int64_t)r * a.cap + sl) * a.chunks * 2) * a.stride;
        double m1 = 0.0, m2 = 0.0;
        for (int c = 0; c < a.chunks; ++c) {
          m1 += part[(2 * c) * a.stride + p];
          m2 += part[(2 * c + 1) * a.stride + p];
        }
        eb += pr * m1;
        eb2 += pr * m2;
      }
    ex[p] = none ? NAN : 1.0 - eb;
    ev[p] = none ? NAN : fmax(eb2 - eb * eb, 0.0);
  }
  if (threadIdx.x == 0) a.status[sl] = m.status | (m.status == 0 && undefined ? kSpectraAverageUndefined : 0);
}

}  // namespace gpdla
