// stats_kernels.hpp -- the two GPU passes behind the CDDF statistics (CDDF_analysis/calc_cddf.py,
// class DLACatalogue).  The host side is gp_dla_detection_amd/cddf.py.
//
//   k_bin_posteriors        one block per selected spectrum: reads its S sample log-likelihoods
//                           once, forms p = exp(sll - shift) * p_dla and z = z_min + (z_max - z_min)
//                           * offset, and evaluates up to four bin requests on them: per bin the
//                           Poisson sum of the small probabilities and the directly kept (bin, p)
//                           pairs (strict rule, :994-1034), or the moment sums of np.histogram's
//                           bins (:1101-1125)
//   k_bin_posteriors_boxed  the same for the rows of a refine pass: the samples are unit points mapped
//                           into each row's own box, and the row's normaliser is formed first, by all
//                           four waves (stats_bin_body.hpp holds both kernels)
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

// Sum over the block, the same bits in every thread: butterfly inside each wave, then the four wave
// totals as (w0 + w1) + (w2 + w3).
__device__ inline double post_block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ inline double post_block_max(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

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

// The rows of a refine pass: every row has its own box of the last level, the
// samples are the shared unit points mapped into it, and the row's normaliser is formed by the kernel.
// The field names the walk uses are StatsBinArgs' (offsets = u, lnhi = v).
struct StatsBoxedArgs {
  int64_t n, S, ld;                       // rows, refine points, row stride of lam (elements)
  const double *lam;                      // [n][ld] lambda of the last level
  const double *p_dla, *upper_z;          // [n]
  const double *boxes;                    // [n][4] (z_lo, z_hi, n_lo, n_hi) of the last level
  const double *offsets, *lnhi;           // [S] the unit points u and v
  const double *edges;                    // [R][kStatsMaxBins + 1]
  int32_t R;
  StatsRequest req[kStatsMaxRequests];
  double *shift;                          // [n] out: m + log Sum_j exp(lambda_j - m)
  double *pois, *mean, *var;              // [R][n][kStatsMaxBins]
  int32_t *count;                         // [R][n]
  int32_t *kept_bin;                      // [R][n][kStatsKept]
  double *kept_p;                         // [R][n][kStatsKept]
};

// The kernel lives in stats_bin_body.hpp, a header WITHOUT an include guard that is included twice.
#define GPDLA_STATS_BIN_KERNEL k_bin_posteriors
#define GPDLA_STATS_BIN_ARGS StatsBinArgs
#include "stats_bin_body.hpp"
#undef GPDLA_STATS_BIN_KERNEL
#undef GPDLA_STATS_BIN_ARGS
#define GPDLA_STATS_BIN_KERNEL k_bin_posteriors_boxed
#define GPDLA_STATS_BIN_ARGS StatsBoxedArgs
#define GPDLA_STATS_BIN_BOXED
#include "stats_bin_body.hpp"
#undef GPDLA_STATS_BIN_BOXED
#undef GPDLA_STATS_BIN_KERNEL
#undef GPDLA_STATS_BIN_ARGS

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

// ---------------------------------------------------------------------------------------------
// Sightline S/N, path-length matrix and the stratified bootstrap.
//
//   k_sightline_snr    one block per sightline of a ragged CSR set: the pixels redward of
//                      1215.67 (1 + max_z_dla), sqrt(noise_variance) / |floored flux| of each,
//                      their median as NumPy takes it, snr = 1 / median (find_snr as executed,
//                      calc_cddf.py:1167-1185).  The selected values are compacted into LDS in
//                      pixel order and the two middle ones found by rank (ties broken by
//                      position), in tiles when more qualify than one tile holds.
//   k_path_lengths     one thread per (sightline, bin): Gauss-Legendre (8 nodes on panels no wider
//                      than 0.25 in z) of (1+z)^2 / sqrt(Om (1+z)^3 + 1 - Om) over the overlap of
//                      the sightline's search range with the bin (cddf.path_length's rules)
//   k_bootstrap_sums   one block per replicate: column sums of V[N][C] over the rows the replicate
//                      draws (Philox4x32-10, counter (lo32(j), hi32(j), r, 2)); a lane owns columns,
//                      a wave a fixed stride of positions, the four waves combine in a fixed tree
//
// No atomics anywhere; every output is bit-identical run to run, and a replicate's sums do not
// depend on which launch computed it.
// ---------------------------------------------------------------------------------------------

constexpr int kSnrTile = 2048;          // selected values held in LDS per step (16 KiB a buffer)
constexpr int kPathOrder = 8;           // Gauss-Legendre nodes per panel
constexpr double kPathPanel = 0.25;     // widest panel in z
constexpr int kBootMaxColumns = 256;    // columns of V: 64 lanes x kBootTiles
constexpr int kBootTiles = kBootMaxColumns / 64;

struct SnrArgs {
  const int64_t *offsets;                 // [n + 1]
  const double *wavelengths, *flux, *noise_variance;
  const double *max_z;                    // [n]
  const double *normalizers;              // [n] or null
  double *snr;                            // [n]
};

// sqrt(nv) / |flux with the floor of find_snr|, each operation rounded once
__device__ inline double snr_value(double f, double nv, bool has_norm, double nm) {
  if (has_norm) {
    if (f / nm < 0.1) f = nm * 0.1;
  } else if (f < 0.1) {
    f = 0.1;
  }
  return sqrt(nv) / fabs(f);
}

// Compacts, in pixel order, the selected values whose compaction index lies in [start, start +
// kSnrTile) into buf; returns the number of selected pixels and whether any value is NaN.
__device__ inline int snr_stage(const SnrArgs &a, int64_t p0, int np, double thresh, bool has_norm, double nm,
                                int start, double *buf, int *wave_tot, bool *any_nan) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int base = 0;
  bool nan_here = false;
  for (int t0 = 0; t0 < np; t0 += 256) {
    const int j = t0 + tid;
    bool sel = false;
    double v = 0.0;
    if (j < np && a.wavelengths[p0 + j] > thresh) {
      sel = true;
      v = snr_value(a.flux[p0 + j], a.noise_variance[p0 + j], has_norm, nm);
      nan_here |= v != v;
    }
    const unsigned long long m = __ballot(sel);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    const int total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    const int pos = off + before - start;
    if (sel && pos >= 0 && pos < kSnrTile) buf[pos] = v;
    base += total;
    __syncthreads();
  }
  *any_nan = __syncthreads_or(nan_here) != 0;
  return base;
}

__global__ __launch_bounds__(256) void k_sightline_snr(SnrArgs a) {
  __shared__ double cand[kSnrTile], other[kSnrTile];
  __shared__ double mid[2];
  __shared__ int wave_tot[4];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t p0 = a.offsets[s];
  const int np = (int)(a.offsets[s + 1] - p0);
  const bool has_norm = a.normalizers != nullptr;
  const double nm = has_norm ? a.normalizers[s] : 1.0;
  const double thresh = 1215.67 * (1.0 + a.max_z[s]);   // NaN max_z: no pixel passes
  const double nan = __builtin_nan("");
  bool any_nan;
  const int m = snr_stage(a, p0, np, thresh, has_norm, nm, 0, cand, wave_tot, &any_nan);
  if (m == 0 || any_nan) {   // block-uniform; NaN is settled before any ordering
    if (tid == 0) a.snr[s] = nan;
    return;
  }
  const int k_lo = (m - 1) / 2, k_hi = m / 2;
  constexpr int kPer = kSnrTile / 256;
  for (int c0 = 0; c0 < m; c0 += kSnrTile) {
    if (c0 > 0) snr_stage(a, p0, np, thresh, has_norm, nm, c0, cand, wave_tot, &any_nan);
    const int nc = (m - c0 < kSnrTile) ? (m - c0) : kSnrTile;
    int rank[kPer];
    double mine[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      rank[q] = 0;
      mine[q] = (tid + 256 * q < nc) ? cand[tid + 256 * q] : 0.0;
    }
    for (int b0 = 0; b0 < m; b0 += kSnrTile) {
      const double *src = cand;
      if (m > kSnrTile) {   // more than one tile: the values compared against are staged apart
        snr_stage(a, p0, np, thresh, has_norm, nm, b0, other, wave_tot, &any_nan);
        src = other;
      }
      const int nb = (m - b0 < kSnrTile) ? (m - b0) : kSnrTile;
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        const int i = tid + 256 * q;
        if (i >= nc) continue;
        const double x = mine[q];
        const int gi = c0 + i;
        int r = 0;
        for (int j = 0; j < nb; ++j) {
          const double y = src[j];
          r += (y < x || (y == x && b0 + j < gi)) ? 1 : 0;
        }
        rank[q] += r;
      }
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      if (tid + 256 * q >= nc) continue;
      if (rank[q] == k_lo) mid[0] = mine[q];
      if (rank[q] == k_hi) mid[1] = mine[q];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double med = (k_lo == k_hi) ? mid[0] : (mid[0] + mid[1]) / 2.0;   // np.median: mean of the middle two
    a.snr[s] = 1.0 / med;
  }
}

struct PathArgs {
  int64_t n;
  int32_t nb, lowzcut;
  const double *z_min, *z_max;   // [n]
  const double *edges;           // [nb + 1]
  double proximity_zone, omega_m;
  double *dX;                    // [n][nb]
};

__device__ __constant__ const double kGaussX[kPathOrder / 2] = {0.1834346424956498, 0.525532409916329,
                                                                0.7966664774136267, 0.9602898564975363};
__device__ __constant__ const double kGaussW[kPathOrder / 2] = {0.362683783378362, 0.31370664587788727,
                                                                0.22238103445337448, 0.10122853629037626};

__device__ inline double dX_dz(double z, double om) {
  const double x = 1.0 + z;
  return x * x / sqrt(om * (x * x * x) + (1.0 - om));
}

__global__ __launch_bounds__(256) void k_path_lengths(PathArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n * a.nb) return;
  const int64_t i = t / a.nb;
  const int b = (int)(t - i * a.nb);
  const double lo = a.z_min[i];
  double hi = a.z_max[i];
  if (a.lowzcut) hi = fmax(fmin(hi, hi - a.proximity_zone), lo);
  const double e_lo = a.edges[b], e_hi = a.edges[b + 1];
  double out = 0.0;
  if (lo < e_hi && hi > e_lo) {   // `inside`; NaN ends fail it
    const double za = fmax(e_lo, lo), zb = fmin(e_hi, hi);
    const double width = zb - za;
    int panels = (int)ceil(width / kPathPanel);
    if (panels < 1) panels = 1;
    const double half = width / (2.0 * panels);
    CompSum acc;
    for (int p = 0; p < panels; ++p) {
      const double mid = za + (2.0 * p + 1.0) * half;
      for (int k = 0; k < kPathOrder / 2; ++k) {
        const double d = half * kGaussX[k];
        acc.add(kGaussW[k] * (dX_dz(mid - d, a.omega_m) + dX_dz(mid + d, a.omega_m)));
      }
    }
    out = half * acc.value();
  }
  a.dX[t] = out;
}

struct BootArgs {
  int64_t n;                      // rows of V, sorted by stratum
  int32_t C;                      // columns, <= kBootMaxColumns
  const double *V;                // [n][C]
  const int32_t *first, *size;    // [n] first row and size of the stratum of position j
  uint32_t key0, key1;
  int64_t r0;                     // replicate index of block 0
  double *out;                    // [gridDim.x][C]
};

__global__ __launch_bounds__(256) void k_bootstrap_sums(BootArgs a) {
  __shared__ double ss[4][kBootMaxColumns], sc[4][kBootMaxColumns];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t r = (uint32_t)(a.r0 + blockIdx.x);
  CompSum acc[kBootTiles];
  for (int64_t base = (int64_t)wave * 64; base < a.n; base += 256) {
    const int64_t j = base + lane;
    int row = 0;
    if (j < a.n) {   // this lane draws position j; the wave then reads the 64 drawn rows one by one
      uint32_t w[4];
      philox4x32_10((uint32_t)j, (uint32_t)((uint64_t)j >> 32), r, 2u, a.key0, a.key1, w);
      row = a.first[j] + (int)(((uint64_t)w[0] * (uint64_t)(uint32_t)a.size[j]) >> 32);
    }
    const int cnt = (a.n - base < 64) ? (int)(a.n - base) : 64;
#pragma unroll 4
    for (int q = 0; q < cnt; ++q) {
      const double *v = a.V + (int64_t)__shfl(row, q) * a.C;   // adjacent lanes, adjacent columns
#pragma unroll
      for (int t = 0; t < kBootTiles; ++t)
        if (lane + 64 * t < a.C) acc[t].add(v[lane + 64 * t]);
    }
  }
#pragma unroll
  for (int t = 0; t < kBootTiles; ++t) {
    ss[wave][lane + 64 * t] = acc[t].s;
    sc[wave][lane + 64 * t] = acc[t].c;
  }
  __syncthreads();
  for (int c = tid; c < a.C; c += 256) {   // (w0 + w1) + (w2 + w3)
    CompSum lo, hi;
    lo.s = ss[0][c]; lo.c = sc[0][c];
    lo.add(ss[1][c]); lo.c += sc[1][c];
    hi.s = ss[2][c]; hi.c = sc[2][c];
    hi.add(ss[3][c]); hi.c += sc[3][c];
    lo.add(hi.s); lo.c += hi.c;
    a.out[(int64_t)blockIdx.x * a.C + c] = lo.value();
  }
}

}  // namespace gpdla
