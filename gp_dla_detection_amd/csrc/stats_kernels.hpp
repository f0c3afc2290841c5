// stats_kernels.hpp -- the two GPU passes behind the CDDF statistics (CDDF_analysis/calc_cddf.py,
// class DLACatalogue).  The host side is gp_dla_detection_amd/cddf.py.
//
//   k_bin_posteriors        one block per selected spectrum: reads its S sample log-likelihoods
//                           once, forms p = exp(sll - shift) * p_dla and z = z_min + (z_max - z_min)
//                           * offset, and evaluates up to four bin requests on them: per bin the
//                           Poisson sum of the small probabilities and the directly kept (bin, p)
//                           pairs (strict rule, :994-1034), or the moment sums of np.histogram's
//                           bins (:1101-1125)
//   k_poisson_binomial_cf   one thread per (segment, n): fsum_j log|1 + p_j (w^n - 1)| and
//                           fsum_j arg(...), w = e^{-2 pi i/(N+1)} (:1293-1295, :1307-1317)
//
// No atomics: each spectrum's sums run in sample order inside one lane (the lane owns one bin),
// each n's sums in segment order inside one thread, so every output depends on its own row only
// and is bit-identical run to run and across any blocking of the spectra.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace gpdla {

constexpr int kStatsMaxBins = 64;      // one bin per lane of a wave
constexpr int kStatsMaxRequests = 4;   // one wave per request
constexpr int kStatsKept = 8;          // directly kept pairs per (spectrum, request)
constexpr int kStatsTile = 1024;       // samples staged in LDS per step (32 KiB)
constexpr int kStatsCfTile = 2048;     // probabilities staged per step of k_poisson_binomial_cf

// s + c carries a sum to about one rounding of the exact value (TwoSum, Knuth); with
// -ffp-contract=off and no reassociation the compiler keeps the error term.
struct CompSum {
  double s = 0.0, c = 0.0;
  __device__ inline void add(double x) {
    const double t = s + x;
    const double bp = t - s;
    c += (s - (t - bp)) + (x - bp);
    s = t;
  }
  __device__ inline double value() const { return s + c; }
};

struct StatsRequest {
  int32_t quantity;      // 0: z, 1: log10 N_HI
  int32_t nb;            // bins, 1 .. kStatsMaxBins
  int32_t histogram;     // 0: strict edges, 1: np.histogram's [a, b) with the last bin closed
  int32_t moment;        // histogram: weight 10^lnhi
  int32_t lowzcut;       // strict: z < min(upper_z, z_hi)
  double z_lo, z_hi, lnhi_lo, lnhi_hi, p_thresh, p_switch;
};

struct StatsBinArgs {
  int64_t n, S, ld;                       // spectra, samples, row stride of sll (elements)
  const double *sll;                      // [n][ld]
  const double *shift, *p_dla, *z_min, *z_max, *upper_z;  // [n]
  const double *offsets, *lnhi, *w10;     // [S]; w10 = 10^lnhi (host pow)
  const double *edges;                    // [R][kStatsMaxBins + 1]
  int32_t R;
  StatsRequest req[kStatsMaxRequests];
  double *pois, *mean, *var;              // [R][n][kStatsMaxBins]
  int32_t *count;                         // [R][n]
  int32_t *kept_bin;                      // [R][n][kStatsKept]
  double *kept_p;                         // [R][n][kStatsKept]
};

__global__ __launch_bounds__(256) void k_bin_posteriors(StatsBinArgs a) {
  __shared__ double sp[kStatsTile], sz[kStatsTile], sl[kStatsTile], sw[kStatsTile];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const double shift = a.shift[s], pd = a.p_dla[s], zmin = a.z_min[s], dz = a.z_max[s] - a.z_min[s];
  const double *row = a.sll + s * a.ld;

  const bool active = wave < a.R;
  StatsRequest rq = a.req[active ? wave : 0];
  const bool mine = active && lane < rq.nb;
  const double e_lo = mine ? a.edges[wave * (kStatsMaxBins + 1) + lane] : 0.0;
  const double e_hi = mine ? a.edges[wave * (kStatsMaxBins + 1) + lane + 1] : 0.0;
  const bool last = lane == rq.nb - 1;
  const double z_up = rq.lowzcut ? fmin(a.upper_z[s], rq.z_hi) : rq.z_hi;
  CompSum acc0, acc1;        // strict: Poisson sum; histogram: w p and w^2 (1 - p) p
  bool poison = false;       // histogram: a NaN weight at or below this bin (np.histogram's cumsum)
  int kept = 0;              // wave-uniform

  for (int64_t t0 = 0; t0 < a.S; t0 += kStatsTile) {
    const int nt = (int)((a.S - t0 < kStatsTile) ? (a.S - t0) : kStatsTile);
    __syncthreads();
    for (int j = tid; j < nt; j += 256) {
      const int64_t g = t0 + j;
      sp[j] = exp(row[g] - shift) * pd;
      sz[j] = zmin + dz * a.offsets[g];
      sl[j] = a.lnhi[g];
      sw[j] = a.w10[g];
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < nt; ++j) {     // every lane reads the same sample: LDS broadcasts
      const double p = sp[j], z = sz[j], l = sl[j];
      const double q = rq.quantity ? l : z;
      if (!rq.histogram) {
        if (!(l > rq.lnhi_lo && l < rq.lnhi_hi && z < z_up && z > rq.z_lo && p > rq.p_thresh)) continue;
        const bool inb = mine && q > e_lo && q < e_hi;
        if (p < rq.p_switch) {
          if (inb) acc0.add(p);
        } else if (__ballot(inb)) {
          if (inb && kept < kStatsKept) {
            const int64_t o = ((int64_t)wave * a.n + s) * kStatsKept + kept;
            a.kept_bin[o] = lane;
            a.kept_p[o] = p;
          }
          ++kept;
        }
      } else {
        if (!(l > rq.lnhi_lo && l < rq.lnhi_hi && z < rq.z_hi && z > rq.z_lo)) continue;
        const double w = rq.moment ? sw[j] : 1.0;
        const double wm = w * p, wv = w * w * (1 - p) * p;
        const bool below = last ? q <= e_hi : q < e_hi;
        if (mine && q >= e_lo && below) {
          acc0.add(wm);
          acc1.add(wv);
        }
        if (mine && below && wm != wm) poison = true;
      }
    }
  }
  if (!active) return;
  const int64_t o = (int64_t)wave * a.n + s;
  if (mine) {
    const double nan = __builtin_nan("");
    if (rq.histogram) {
      a.mean[o * kStatsMaxBins + lane] = poison ? nan : acc0.value();
      a.var[o * kStatsMaxBins + lane] = poison ? nan : acc1.value();
    } else {
      a.pois[o * kStatsMaxBins + lane] = acc0.value();
    }
  }
  if (lane == 0) a.count[o] = kept;
}

struct StatsCfArgs {
  const int64_t *seg_off;   // [nseg + 1] into p
  const int64_t *out_off;   // [nseg + 1] into logsum / argsum: (N + 1) / 2 + 1 values per segment
  const int64_t *blk_seg;   // [blocks] segment of each block
  const int64_t *blk_n0;    // [blocks] first n of each block
  const double *p;
  double *logsum, *argsum;
};

__global__ __launch_bounds__(256) void k_poisson_binomial_cf(StatsCfArgs a) {
  __shared__ double sp[kStatsCfTile];
  const int64_t seg = a.blk_seg[blockIdx.x];
  const int64_t n = a.blk_n0[blockIdx.x] + threadIdx.x;
  const int64_t p0 = a.seg_off[seg], N = a.seg_off[seg + 1] - p0;
  const int64_t M = (N + 1) / 2 + 1;
  const bool act = n < M;
  // nco = exp(-2 pi i n / (N + 1)) - 1 as cmath forms it: t = (-2 pi n) / (N + 1)
  const double t = (-2.0 * 3.141592653589793 * (double)n) / (double)(N + 1);
  double sn, cs;
  sincos(t, &sn, &cs);
  const double re_c = cs - 1.0, im_c = sn;
  CompSum ls, as;
  for (int64_t t0 = 0; t0 < N; t0 += kStatsCfTile) {
    const int nt = (int)((N - t0 < kStatsCfTile) ? (N - t0) : kStatsCfTile);
    __syncthreads();
    for (int j = threadIdx.x; j < nt; j += 256) sp[j] = a.p[p0 + t0 + j];
    __syncthreads();
    if (!act) continue;
    for (int j = 0; j < nt; ++j) {
      const double pj = sp[j];
      const double re = 1.0 + pj * re_c, im = pj * im_c;   // 1 + p * nco
      ls.add(log(hypot(re, im)));
      as.add(atan2(im, re));
    }
  }
  if (act) {
    a.logsum[a.out_off[seg] + n] = ls.value();
    a.argsum[a.out_off[seg] + n] = as.value();
  }
}

}  // namespace gpdla
