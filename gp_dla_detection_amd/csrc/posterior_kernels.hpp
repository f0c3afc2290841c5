// posterior_kernels.hpp -- credible intervals and moments of the absorber parameters (DESIGN.md
// section 4.17).  A row of S sample log-likelihoods is a weighted sample of the posterior of
// (z_DLA, log10 N_HI) of each absorber ("slot") of a model; the host side is host_posterior.hpp.
//
//   k_parameter_summaries   one block of 256 threads per (row, model).  Per model: max l, T = sum w,
//                           sum w^2 (w = exp(l - max l)).  Per slot of the model: the weighted mean,
//                           variance and covariance of z and log N (two passes about the computed
//                           mean), the threshold sums P(log N >= t), and the weighted quantiles of z
//                           and of log N without interpolation.
//
// Quantiles go by RANK, not by value: the host ranks offset_samples and log_nhi_samples once per call
// (stable, ties by index); z is monotone in the offset, so one permutation serves every row.  The key
// of sample i for (slot, quantity) is the rank of the slot's base sample.  Level 1: thread t owns the
// rank bucket [t B, (t + 1) B), B = ceil(S / 256); (w, key) tiles are staged in LDS, every thread
// reads the same sample (broadcast) and adds it when the key is in its bucket; the 256 bucket sums
// added in bucket order give F at the bucket edges and each target p T picks its bucket.  Level 2:
// wave v serves probabilities v and v + 4; its lanes own the single ranks of the chosen bucket (64 a
// round), the samples are walked once more, and the first rank whose running sum reaches p T names
// the value.
//
// No atomics.  Every sum runs in an order fixed by (S, thread index) alone: a thread's samples in
// sample order, the lanes of a wave in a butterfly, the four waves as (w0 + w1) + (w2 + w3).  Every
// output is a function of its own row only and bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stats_kernels.hpp"

#pragma clang fp contract(off)

namespace gpdla {

constexpr int kPostMaxModels = 4;         // what the multi-DLA driver accepts
constexpr int kPostMaxProbabilities = 8;  // two per wave
constexpr int kPostMaxThresholds = 4;
constexpr int kPostTile = 1024;           // samples staged in LDS per step (16 KiB)

struct PosteriorArgs {
  int64_t S;
  int32_t md;                       // models per row
  int32_t Q, nt;                    // probabilities, thresholds
  double prob[kPostMaxProbabilities];
  double thresh[kPostMaxThresholds];
  const double *sll;                // model m of row r: sll + row_start[r] + (m - 1) S
  const int64_t *row_start;         // [n]
  const uint32_t *base;             // slot j >= 2 of row r: base + base_start[r] + (j - 2) S; 1-based, 0 = never drawn
  const int64_t *base_start;        // [n] (null when md == 1)
  const double *z_min, *z_max;      // [n]
  const double *offsets, *lnhi;     // [S]
  const int32_t *rank_off, *rank_n; // [S] stable rank of sample i
  const int32_t *inv_off, *inv_n;   // [S] sample of rank r
  // outputs, NaN-prefilled by the host: [n][md][md] (model, slot) per field
  double *mean_z, *std_z, *mean_n, *std_n, *cov;
  double *quant_z, *quant_n;        // [n][md][md][Q]
  double *exceed;                   // [n][md][md][nt]
  double *ess;                      // [n][md]
  int32_t *status;                  // [n][md]  1: no usable sample, 2: NaN search range
  // optional affine reading of lnhi per row (the refined tables of DESIGN.md 4.18, whose lnhi holds unit
  // coordinates): log N = n_lo[r] + (n_hi[r] - n_lo[r]) lnhi[i], in the moments, against the thresholds and in
  // the quantiles.  Null: lnhi is log N itself.
  const double *n_lo, *n_hi;        // [n] or null
};

__device__ inline double post_log_n(bool mapped, double lo, double width, double v) { return mapped ? lo + width * v : v; }

// (post_block_sum and post_block_max, the block reductions of every sum and maximum here, are in stats_kernels.hpp)

// l_i of model m as the summaries see it: NaN when a slot of the model was never drawn for sample i
// (stored index 0; an index above S is refused by the host and read here as "never drawn" too)
__device__ inline double post_ll(const double *row, const uint32_t *brow, int m, int64_t S, int64_t i) {
  double l = row[i];
  for (int j = 0; j + 1 < m; ++j) {
    const uint32_t b = brow[(int64_t)j * S + i];
    if (b == 0u || (int64_t)b > S) l = __builtin_nan("");
  }
  return l;
}

__device__ inline double post_weight(double l, double mx) { return (l == l) ? exp(l - mx) : 0.0; }

// base sample (0-based) of sample i in slot j (0-based); 0 where the stored index is unusable (the
// sample then has weight 0)
__device__ inline int64_t post_base(const uint32_t *brow, int j, int64_t S, int64_t i) {
  if (j == 0) return i;
  const uint32_t b = brow[(int64_t)(j - 1) * S + i];
  return (b == 0u || (int64_t)b > S) ? 0 : (int64_t)b - 1;
}

// One tile of (weight, key of z, key of log N) of slot j into LDS
__device__ inline void post_stage(const PosteriorArgs &a, const double *row, const uint32_t *brow, int m, int j, double mx,
                                  bool rev, int64_t t0, int nt, double *sw, int32_t *skz, int32_t *skn) {
  for (int q = threadIdx.x; q < nt; q += 256) {
    const int64_t i = t0 + q;
    const int64_t b = post_base(brow, j, a.S, i);
    sw[q] = post_weight(post_ll(row, brow, m, a.S, i), mx);
    const int32_t kz = a.rank_off[b];
    skz[q] = rev ? (int32_t)(a.S - 1) - kz : kz;
    skn[q] = a.rank_n[b];
  }
}

__global__ __launch_bounds__(256) void k_parameter_summaries(PosteriorArgs a) {
  __shared__ double sw[kPostTile];
  __shared__ int32_t skz[kPostTile], skn[kPostTile];
  __shared__ double bsum[2][256];                         // level 1: bucket sums of z and of log N
  __shared__ double red[4];
  __shared__ int32_t pick_bucket[2][kPostMaxProbabilities];
  __shared__ double pick_start[2][kPostMaxProbabilities]; // F below the picked bucket

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t r = blockIdx.x / a.md;
  const int m = (int)(blockIdx.x - r * a.md) + 1;         // this block's model: m absorbers
  const int64_t S = a.S;
  const double *row = a.sll + a.row_start[r] + (int64_t)(m - 1) * S;
  const uint32_t *brow = a.base ? a.base + a.base_start[r] : nullptr;
  const double zmin = a.z_min[r], zmax = a.z_max[r];
  const double dz = zmax - zmin;
  const bool z_ok = zmin == zmin && zmax == zmax;
  const bool rev = dz < 0.0;                              // z falls with the offset: ranks run backwards
  const bool mapped = a.n_lo != nullptr;
  const double nlo = mapped ? a.n_lo[r] : 0.0, nw = mapped ? a.n_hi[r] - a.n_lo[r] : 1.0;
  const int64_t om = r * a.md + (m - 1);                  // [n][md]
  const double nan = __builtin_nan("");

  // ---- the model: max l, T, sum w^2 ----
  double mx = -__builtin_inf();
  for (int64_t i = tid; i < S; i += 256) {
    const double l = post_ll(row, brow, m, S, i);
    if (l == l) mx = fmax(mx, l);
  }
  mx = post_block_max(mx, red);
  int32_t st = z_ok ? 0 : 2;
  if (!(mx > -__builtin_inf() && mx < __builtin_inf())) {  // no finite entry, or +inf: unusable
    if (tid == 0) a.status[om] = st | 1;                   // (every output of the model stays NaN)
    return;
  }
  CompSum cT, cT2;
  for (int64_t i = tid; i < S; i += 256) {
    const double w = post_weight(post_ll(row, brow, m, S, i), mx);
    cT.add(w);
    cT2.add(w * w);
  }
  const double T = post_block_sum(cT.value(), red);
  const double T2 = post_block_sum(cT2.value(), red);
  if (tid == 0) {
    a.ess[om] = T * T / T2;
    a.status[om] = st;
  }

  const int32_t B = (int32_t)((S + 255) / 256);           // ranks per bucket (the host keeps S below 2^30)
  const int32_t lo = tid * B;

  for (int j = 0; j < m; ++j) {
    const int64_t o = om * a.md + j;                      // [n][md][md]

    // ---- moments and threshold sums: pass 1 about 0, pass 2 about the mean ----
    CompSum sz, sn, se[kPostMaxThresholds];
    for (int64_t i = tid; i < S; i += 256) {
      const double w = post_weight(post_ll(row, brow, m, S, i), mx);
      const int64_t b = post_base(brow, j, S, i);
      const double z = zmin + dz * a.offsets[b], ln = post_log_n(mapped, nlo, nw, a.lnhi[b]);
      if (w > 0.0) {                                      // a sample of weight 0 does not exist
        if (z_ok) sz.add(w * z);
        sn.add(w * ln);
#pragma unroll
        for (int t = 0; t < kPostMaxThresholds; ++t)
          if (t < a.nt && ln >= a.thresh[t]) se[t].add(w);
      }
    }
    const double mz = z_ok ? post_block_sum(sz.value(), red) / T : nan;
    const double mn = post_block_sum(sn.value(), red) / T;
#pragma unroll
    for (int t = 0; t < kPostMaxThresholds; ++t) {
      if (t < a.nt) {
        const double e = post_block_sum(se[t].value(), red) / T;
        if (tid == 0) a.exceed[o * a.nt + t] = e;
      }
    }
    CompSum vz, vn, vc;
    for (int64_t i = tid; i < S; i += 256) {
      const double w = post_weight(post_ll(row, brow, m, S, i), mx);
      const int64_t b = post_base(brow, j, S, i);
      const double z = zmin + dz * a.offsets[b], ln = post_log_n(mapped, nlo, nw, a.lnhi[b]);
      if (w > 0.0) {
        const double dn = ln - mn;
        vn.add(w * (dn * dn));
        if (z_ok) {
          const double dzz = z - mz;
          vz.add(w * (dzz * dzz));
          vc.add(w * (dzz * dn));
        }
      }
    }
    const double var_n = post_block_sum(vn.value(), red) / T;
    const double var_z = z_ok ? post_block_sum(vz.value(), red) / T : nan;
    const double cov = z_ok ? post_block_sum(vc.value(), red) / T : nan;
    if (tid == 0) {
      a.mean_z[o] = mz;
      a.std_z[o] = z_ok ? sqrt(var_z) : nan;
      a.mean_n[o] = mn;
      a.std_n[o] = sqrt(var_n);
      a.cov[o] = cov;
    }
    if (a.Q == 0) continue;

    // ---- quantiles, level 1: the bucket sums of both quantities in one walk ----
    double accz = 0.0, accn = 0.0;
    for (int64_t t0 = 0; t0 < S; t0 += kPostTile) {
      const int nt = (int)((S - t0 < kPostTile) ? (S - t0) : kPostTile);
      __syncthreads();
      post_stage(a, row, brow, m, j, mx, rev, t0, nt, sw, skz, skn);
      __syncthreads();
      for (int q = 0; q < nt; ++q) {                      // every lane reads the same sample: LDS broadcasts
        const double w = sw[q];
        const uint32_t uz = (uint32_t)(skz[q] - lo), un = (uint32_t)(skn[q] - lo);
        accz += (uz < (uint32_t)B) ? w : 0.0;
        accn += (un < (uint32_t)B) ? w : 0.0;
      }
    }
    bsum[0][tid] = accz;
    bsum[1][tid] = accn;
    __syncthreads();
    if (lane == 0 && wave < 2) {                          // one thread per quantity adds the buckets in order
      const int qy = wave;
      int next = 0, last_pos = 0;
      double run = 0.0;
      for (int t = 0; t < 256; ++t) {
        const double before = run, s = bsum[qy][t];
        run = before + s;
        if (s > 0.0) last_pos = t;
        while (next < a.Q && run >= a.prob[next] * T) {   // probabilities increase: so do the targets
          pick_bucket[qy][next] = t;
          pick_start[qy][next] = before;
          ++next;
        }
      }
      for (; next < a.Q; ++next) {                        // the total fell short of p T by rounding:
        pick_bucket[qy][next] = last_pos;                 // the last bucket that holds weight
        pick_start[qy][next] = -1.0;                      // (level 2 then finds no crossing either)
      }
    }
    __syncthreads();

    // ---- level 2: wave v serves probabilities v and v + 4 ----
    for (int qy = z_ok ? 0 : 1; qy < 2; ++qy) {
      const int32_t *keys = qy ? skn : skz;
      const int q0 = wave, q1 = wave + 4;
      const bool have0 = q0 < a.Q, have1 = q1 < a.Q;
      const int32_t r0 = have0 ? pick_bucket[qy][q0] * B : 0;
      const int32_t r1 = have1 ? pick_bucket[qy][q1] * B : 0;
      const double tg0 = have0 ? a.prob[q0] * T : 0.0, tg1 = have1 ? a.prob[q1] * T : 0.0;
      double run0 = have0 ? pick_start[qy][q0] : 0.0, run1 = have1 ? pick_start[qy][q1] : 0.0;
      const bool short0 = run0 < 0.0, short1 = run1 < 0.0; // fallback: take the last rank with weight
      bool done0 = !have0, done1 = !have1;
      int64_t ans0 = -1, ans1 = -1;                        // rank of the answer; wave-uniform
      for (int32_t c0 = 0; c0 < B; c0 += 64) {             // 64 ranks of the bucket per round
        if (__syncthreads_and(done0 && done1)) break;      // (the staging below needs the whole block)
        const int32_t my0 = r0 + c0 + lane, my1 = r1 + c0 + lane;
        double acc0 = 0.0, acc1 = 0.0;
        for (int64_t t0 = 0; t0 < S; t0 += kPostTile) {
          const int nt = (int)((S - t0 < kPostTile) ? (S - t0) : kPostTile);
          if (S > kPostTile) {                             // (a single tile is still staged from level 1)
            __syncthreads();
            post_stage(a, row, brow, m, j, mx, rev, t0, nt, sw, skz, skn);
            __syncthreads();
          }
          for (int q = 0; q < nt; ++q) {
            const double w = sw[q];
            const int32_t k = keys[q];
            acc0 += (k == my0) ? w : 0.0;
            acc1 += (k == my1) ? w : 0.0;
          }
        }
        // running sums in rank order; the first lane that reaches the target names the value
        for (int l = 0; l < 64; ++l) {
          const double x0 = __shfl(acc0, l), x1 = __shfl(acc1, l);
          const bool pos0 = x0 > 0.0, pos1 = x1 > 0.0;
          if (!done0 && pos0) {
            run0 = short0 ? run0 : run0 + x0;
            if (short0 || run0 < tg0) ans0 = r0 + c0 + l;   // the last rank with weight so far
            else { ans0 = r0 + c0 + l; done0 = true; }
          }
          if (!done1 && pos1) {
            run1 = short1 ? run1 : run1 + x1;
            if (short1 || run1 < tg1) ans1 = r1 + c0 + l;
            else { ans1 = r1 + c0 + l; done1 = true; }
          }
        }
      }
      if (lane == 0) {
        double *out = qy ? a.quant_n : a.quant_z;
        for (int k = 0; k < 2; ++k) {
          const int q = k ? q1 : q0;
          const int64_t ans = k ? ans1 : ans0;
          if (q >= a.Q || ans < 0) continue;
          double v;
          if (qy) {
            v = post_log_n(mapped, nlo, nw, a.lnhi[a.inv_n[ans]]);
          } else {
            const int64_t rk = rev ? (S - 1) - ans : ans;
            v = zmin + dz * a.offsets[a.inv_off[rk]];
          }
          out[o * a.Q + q] = v;
        }
      }
    }
  }
}

}  // namespace gpdla
