// sample_kernels.hpp -- the DLA parameter samples and the LLS normalisers (generate_dla_samples.m,
// multi_dlas/generate_dla_samples_multi.m, multi_dlas/set_lls_parameters.m).
// The host side is host_samples.hpp and gp_dla_detection_amd/samples.py.
//
//   k_rank_select      one thread per catalogue value: its rank among all N (ties broken by position),
//                      the catalogue streamed through LDS; the threads of rank k_lo / k_hi write the
//                      two middle order statistics (the two medians of the bandwidth rule)
//   k_abs_deviation    |v - median|, the median taken from those two as NumPy / MATLAB take it
//   k_kde_partial      grid points x catalogue values: a block holds 256 grid points and one CHUNK of
//                      kKdeChunk values, streamed through LDS in tiles; each thread's compensated sum
//                      of exp(-z^2 / 2) runs in catalogue order
//   k_kde_finish       one thread per grid point: compensated sum of its chunk partials in chunk
//                      order, over N h sqrt(2 pi)
//   k_prior_panels     one thread per panel of the cumulative table: 8-node Gauss-Legendre of the
//                      prior density over the panel
//   k_prior_prefix     the running (compensated) sum of the panels, in panel order, by one thread
//   k_prior_eval       one thread per point: density and F(x) = table entry + Gauss-Legendre on the
//                      partial panel
//   k_halton           one thread per index: the RR2-scrambled radical inverses
//   k_draw_samples     one thread per sample: its quasi-random coordinates (or the caller's), the
//                      inverse CDF by table search + safeguarded Newton, 10^x
//
// The chunk and panel sizes are constants, not launch parameters, and nothing is accumulated with
// atomics: every output is bit-identical run to run and does not depend on the launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stats_kernels.hpp"   // CompSum, kGaussX / kGaussW

#pragma clang fp contract(off)

namespace gpdla {

constexpr int kKdeChunk = 4096;          // catalogue values per partial sum
constexpr int kKdeTile = 1024;           // values staged in LDS per step (8 KiB)
constexpr int kPriorPanels = 512;        // equal panels per smooth segment of [lower, kPriorUpper]
constexpr int kPriorMaxSegments = 4;     // lower | uniform_min | flat-below break | uniform_max | upper
constexpr double kPriorUpper = 25.0;     // upper limit of every integral of the three scripts
constexpr int kHaltonMaxDims = 8;
constexpr int kHaltonMaxBase = 64;
constexpr double kInverseTol = 1e-13;    // |F(x) - u| at which the inverse CDF stops
constexpr int kInverseMaxIter = 128;

// ---------------------------------------------------------------------------------------------
// medians by rank
// ---------------------------------------------------------------------------------------------
struct SelectArgs {
  const double *v;     // [N], finite
  int64_t N, k_lo, k_hi;
  double *out;         // [2]: the order statistics k_lo and k_hi
};

__global__ __launch_bounds__(256) void k_rank_select(SelectArgs a) {
  __shared__ double tile[kKdeTile];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const double x = (i < a.N) ? a.v[i] : 0.0;
  int64_t rank = 0;
  for (int64_t t0 = 0; t0 < a.N; t0 += kKdeTile) {
    const int nt = (a.N - t0 < kKdeTile) ? (int)(a.N - t0) : kKdeTile;
    for (int j = tid; j < nt; j += 256) tile[j] = a.v[t0 + j];
    __syncthreads();
    int r = 0;
    for (int j = 0; j < nt; ++j) {
      const double y = tile[j];
      r += (y < x || (y == x && t0 + j < i)) ? 1 : 0;
    }
    rank += r;
    __syncthreads();
  }
  if (i < a.N) {   // the ranks are a permutation of 0 .. N-1: one writer each
    if (rank == a.k_lo) a.out[0] = x;
    if (rank == a.k_hi) a.out[1] = x;
  }
}

__global__ __launch_bounds__(256) void k_abs_deviation(const double *v, int64_t N, const double *mid, double *dev) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const double med = (mid[0] + mid[1]) / 2.0;   // odd N: both are the middle value
  dev[i] = fabs(v[i] - med);
}

// ---------------------------------------------------------------------------------------------
// kernel density estimate on a grid (normal kernel, no boundary correction)
// ---------------------------------------------------------------------------------------------
struct KdeArgs {
  const double *values;   // [N]
  const double *points;   // [G]
  int64_t N, G, gblocks;  // gblocks = ceil(G / 256); the launch has gblocks * ceil(N / kKdeChunk) blocks
  double h;
  double *partial;        // [chunks][G]
  double *density;        // [G]
};

__global__ __launch_bounds__(256) void k_kde_partial(KdeArgs a) {
  __shared__ double tile[kKdeTile];
  const int tid = threadIdx.x;
  const int64_t chunk = (int64_t)blockIdx.x / a.gblocks;
  const int64_t g = ((int64_t)blockIdx.x - chunk * a.gblocks) * 256 + tid;
  const double x = (g < a.G) ? a.points[g] : 0.0;
  const int64_t j0 = chunk * kKdeChunk;
  const int64_t j1 = (a.N - j0 < kKdeChunk) ? a.N : j0 + kKdeChunk;
  CompSum acc;
  for (int64_t t0 = j0; t0 < j1; t0 += kKdeTile) {
    const int nt = (j1 - t0 < kKdeTile) ? (int)(j1 - t0) : kKdeTile;
    for (int j = tid; j < nt; j += 256) tile[j] = a.values[t0 + j];
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
      const double z = (x - tile[j]) / a.h;
      acc.add(exp(-0.5 * (z * z)));
    }
    __syncthreads();
  }
  if (g < a.G) a.partial[chunk * a.G + g] = acc.value();
}

__global__ __launch_bounds__(256) void k_kde_finish(KdeArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.G) return;
  const int64_t chunks = (a.N + kKdeChunk - 1) / kKdeChunk;
  CompSum acc;
  for (int64_t c = 0; c < chunks; ++c) acc.add(a.partial[c * a.G + g]);
  a.density[g] = acc.value() / (((double)a.N * a.h) * 2.5066282746310002);   // sqrt(2 pi)
}

// ---------------------------------------------------------------------------------------------
// the column density prior and its cumulative table
// ---------------------------------------------------------------------------------------------
struct PriorDev {
  double c0, c1, c2;      // log g(t) = c0 + c1 s + c2 s^2, s = t - centre
  double centre;
  double alpha;           // weight of g / Z
  double umin, umax;      // the uniform component
  double lower;           // F(lower) = 0
  double flat_below;      // NaN: none; else g(t) = g(flat_below) for t < flat_below
  double Z;               // integral of g over [lower, kPriorUpper]
};

struct PriorTable {
  int32_t nseg;
  double edge[kPriorMaxSegments + 1];   // lower = edge[0] < ... < edge[nseg] = kPriorUpper
  double *cum;                          // [nseg * kPriorPanels + 1], cum[0] = 0
};

__device__ inline double prior_g(const PriorDev &p, double t) {
  if (t < p.flat_below) t = p.flat_below;   // (a NaN break point compares false)
  const double s = t - p.centre;
  return exp(p.c0 + s * (p.c1 + s * p.c2));
}

// the density where the uniform component is known to be on (inside a panel it does not change)
__device__ inline double prior_p(const PriorDev &p, double t, bool in_uniform) {
  const double fit = p.alpha * (prior_g(p, t) / p.Z);
  return in_uniform ? fit + (1.0 - p.alpha) * (1.0 / (p.umax - p.umin)) : fit;
}

__device__ inline double prior_pdf(const PriorDev &p, double t) { return prior_p(p, t, t >= p.umin && t <= p.umax); }

__device__ inline double panel_edge(const PriorTable &T, int s, int j) {
  return (j >= kPriorPanels) ? T.edge[s + 1] : T.edge[s] + (T.edge[s + 1] - T.edge[s]) * ((double)j / kPriorPanels);
}

__device__ inline bool panel_in_uniform(const PriorDev &p, const PriorTable &T, int s) {
  const double mid = 0.5 * (T.edge[s] + T.edge[s + 1]);   // break points are segment edges
  return mid >= p.umin && mid <= p.umax;
}

// 8-node Gauss-Legendre of the density over [a, b], inside one panel
__device__ inline double prior_gl(const PriorDev &p, double a, double b, bool in_uniform) {
  const double half = 0.5 * (b - a), mid = a + half;
  CompSum acc;
  for (int k = 0; k < kPathOrder / 2; ++k) {
    const double d = half * kGaussX[k];
    acc.add(kGaussW[k] * (prior_p(p, mid - d, in_uniform) + prior_p(p, mid + d, in_uniform)));
  }
  return half * acc.value();
}

__global__ __launch_bounds__(256) void k_prior_panels(PriorDev p, PriorTable T, double *panel) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T.nseg * kPriorPanels) return;
  const int s = t / kPriorPanels, j = t - s * kPriorPanels;
  panel[t] = prior_gl(p, panel_edge(T, s, j), panel_edge(T, s, j + 1), panel_in_uniform(p, T, s));
}

__global__ void k_prior_prefix(const double *panel, PriorTable T) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  CompSum acc;
  T.cum[0] = 0.0;
  for (int t = 0; t < T.nseg * kPriorPanels; ++t) {
    acc.add(panel[t]);
    T.cum[t + 1] = acc.value();
  }
}

// F(x): the table up to x's panel, Gauss-Legendre on the rest
__device__ inline double prior_cdf(const PriorDev &p, const PriorTable &T, double x) {
  if (!(x > T.edge[0])) return 0.0;
  if (x >= T.edge[T.nseg]) return T.cum[T.nseg * kPriorPanels];
  int s = 0;
  while (s + 1 < T.nseg && x >= T.edge[s + 1]) ++s;
  int j = (int)((x - T.edge[s]) / (T.edge[s + 1] - T.edge[s]) * kPriorPanels);
  j = j < 0 ? 0 : (j > kPriorPanels - 1 ? kPriorPanels - 1 : j);
  while (j > 0 && x < panel_edge(T, s, j)) --j;
  while (j < kPriorPanels - 1 && x >= panel_edge(T, s, j + 1)) ++j;
  return T.cum[s * kPriorPanels + j] + prior_gl(p, panel_edge(T, s, j), x, panel_in_uniform(p, T, s));
}

__global__ __launch_bounds__(256) void k_prior_eval(PriorDev p, PriorTable T, int64_t n, const double *x, double *pdf,
                                                    double *cdf) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (pdf) pdf[i] = prior_pdf(p, x[i]);
  if (cdf) cdf[i] = prior_cdf(p, T, x[i]);
}

// F^{-1}(u): the panel by bisection of the table, then Newton on F inside it, kept inside a bracket
// that every evaluation narrows (a step that leaves the bracket becomes its midpoint)
__device__ inline double prior_inverse(const PriorDev &p, const PriorTable &T, double u) {
  const int P = T.nseg * kPriorPanels;
  if (!(u > 0.0)) return T.edge[0];
  if (u >= T.cum[P]) return T.edge[T.nseg];
  int lo = 0, hi = P;   // cum[lo] <= u < cum[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (T.cum[mid] <= u) lo = mid; else hi = mid;
  }
  const int s = lo / kPriorPanels, j = lo - s * kPriorPanels;
  const double a = panel_edge(T, s, j), b = panel_edge(T, s, j + 1);
  const bool in_uniform = panel_in_uniform(p, T, s);
  const double target = u - T.cum[lo], mass = T.cum[lo + 1] - T.cum[lo];
  double xl = a, xh = b;
  double x = a + (b - a) * (target / mass), last = a;
  for (int it = 0; it < kInverseMaxIter; ++it) {
    if (!(x > xl && x < xh)) x = xl + 0.5 * (xh - xl);
    if (!(x > xl && x < xh)) return x;   // the bracket is one ulp wide
    last = x;
    const double r = prior_gl(p, a, x, in_uniform) - target;
    if (fabs(r) <= kInverseTol) return x;
    if (r > 0.0) xh = x; else xl = x;
    x = x - r / prior_p(p, x, in_uniform);
  }
  return last;
}

// ---------------------------------------------------------------------------------------------
// RR2-scrambled Halton points
// ---------------------------------------------------------------------------------------------
struct HaltonArgs {
  int32_t ndim;
  int32_t base[kHaltonMaxDims];
  uint8_t perm[kHaltonMaxDims][kHaltonMaxBase];   // perm[d][digit]: the reverse-radix permutation of base[d]
};

// sum_j perm(d_j) b^-(j+1) over the base-b digits d_j of `index` (< 2^32): an exact integer numerator
// over b^J (both below 2^53 for b <= 2^21) and one division, so the result is the correctly rounded
// value of the rational
__device__ inline double scrambled_radical_inverse(uint64_t index, int b, const uint8_t *perm) {
  uint64_t num = 0, den = 1;
  const uint64_t ub = (uint64_t)b;
  while (index > 0) {
    const uint64_t q = index / ub;
    num = num * ub + perm[index - q * ub];
    den *= ub;
    index = q;
  }
  return (double)num / (double)den;
}

__global__ __launch_bounds__(256) void k_halton(HaltonArgs h, int64_t first, int64_t num, double *out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= num) return;
  for (int d = 0; d < h.ndim; ++d)
    out[i * h.ndim + d] = scrambled_radical_inverse((uint64_t)(first + i), h.base[d], h.perm[d]);
}

struct DrawArgs {
  PriorDev p;
  PriorTable T;
  HaltonArgs h;            // bases 2, 3, 5
  int64_t first, num;
  const double *sequence;  // [num][seq_dims] uniforms used instead of the Halton points, or null
  int32_t seq_dims;
  int32_t want_lls;
  double lls_lo, lls_hi;
  double *offset, *log_nhi, *nhi;               // [num]
  double *lls_offset, *lls_log_nhi, *lls_nhi;   // [num] when want_lls
};

__global__ __launch_bounds__(256) void k_draw_samples(DrawArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.num) return;
  double u[3];
  for (int d = 0; d < 3; ++d) {
    if (a.sequence)
      u[d] = (d < a.seq_dims) ? a.sequence[i * a.seq_dims + d] : 0.0;
    else
      u[d] = scrambled_radical_inverse((uint64_t)(a.first + i), a.h.base[d], a.h.perm[d]);
  }
  a.offset[i] = u[0];
  const double x = prior_inverse(a.p, a.T, u[1]);
  a.log_nhi[i] = x;
  a.nhi[i] = pow(10.0, x);
  if (a.want_lls) {
    const double l = a.lls_lo + (a.lls_hi - a.lls_lo) * u[2];
    a.lls_offset[i] = u[2];
    a.lls_log_nhi[i] = l;
    a.lls_nhi[i] = pow(10.0, l);
  }
}

}  // namespace gpdla
