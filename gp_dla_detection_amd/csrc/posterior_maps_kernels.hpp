// posterior_maps_kernels.hpp -- posterior maps of (z_DLA, log10 N_HI) on a per-row grid, their highest
// posterior density (HPD) regions, and the absorber intensity mixed over the models (DESIGN.md section
// 4.22; the contract is the comment in include/gpdla.h).  The host side is host_posterior_maps.hpp.
//
//   k_posterior_maps       one block of 256 threads per (row, model, slot).  max l and T as
//                          k_parameter_summaries takes them.  (w, flat cell) tiles of 1024 samples are staged
//                          in LDS; every thread reads the same sample (broadcast) and the thread that owns
//                          the cell (cell mod 256) adds the weight into the LDS map, so a cell's sum runs in
//                          sample order.  Divide by T; bitonic sort of (mass, index) in LDS, mass descending
//                          and ties by index ascending; one lane accumulates C over the positive cells in
//                          rank order and answers the credible masses; the block scatters C to the cells.
//   k_posterior_maps_mix   one block per row: intensity = sum over the models of weight x (sum of the
//                          model's slot maps), cell by cell from the maps k_posterior_maps left in device
//                          memory, and its sum in flat-index order by one lane.
//
// No atomics, LDS atomics included.  Every sum runs in an order fixed by the contract: a cell's samples in
// sample order, C in rank order, the mix in (model, slot) order, the row's intensity in cell order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "posterior_kernels.hpp"
#include "stats_kernels.hpp"

#pragma clang fp contract(off)

namespace gpdla {

constexpr int kMapMaxSide = 64;                           // cells per axis
constexpr int kMapMaxCells = kMapMaxSide * kMapMaxSide;   // 4096: the LDS map is 32 KiB
constexpr int kMapMaxLevels = 8;
constexpr int32_t kMapUnusable = 1, kMapBadGrid = 4, kMapShort = 8, kMapBadWeights = 16;  // status bits

struct PosteriorMapsArgs {
  int64_t S;
  int32_t md;                       // models per row
  int32_t nz, nn;                   // cells per axis, 1 .. kMapMaxSide each
  int32_t L;                        // credible masses
  double level[kMapMaxLevels];
  const double *sll;                // model m of row r: sll + row_start[r] + (m - 1) S
  const int64_t *row_start;         // [n]
  const uint32_t *base;             // as PosteriorArgs::base
  const int64_t *base_start;        // [n] (null when md == 1)
  const double *z_min, *z_max;      // [n]
  const double *offsets, *lnhi;     // [S]
  const double *n_lo, *n_hi;        // [n] or null: the affine reading of lnhi (PosteriorArgs::n_lo)
  const double *grid;               // [n][4] as (gz_lo, gz_hi, gn_lo, gn_hi)
  // outputs per (row, model, slot), [n][md][md] with slot > model left as the host prefilled it
  double *mass;                     // [n][md][md][nz nn]; never null: k_posterior_maps_mix reads it
  double *hpd_level;                // [n][md][md][nz nn] or null
  double *outside;                  // [n][md][md]
  int32_t *mode;                    // [n][md][md]
  int32_t *hpd_cells;               // [n][md][md][L]
  double *hpd_threshold;            // [n][md][md][L]
  int32_t *slot_status;             // [n][md][md]
};

struct PosteriorMixArgs {
  int32_t md, cells;
  const double *mass;               // [n][md][md][cells]
  const int32_t *slot_status;       // [n][md][md]
  const double *weights;            // [n][md]
  double *intensity;                // [n][cells]
  double *expected;                 // [n]
  int32_t *row_status;              // [n]
};

// edge c < n of an axis; edge n is hi itself
__device__ inline double map_edge(double lo, double width, int c, int n) { return lo + width * ((double)c / (double)n); }

// The cell of v on [lo, hi] cut into n: the largest c with edge(c) <= v, v == hi in the last; -1 outside or
// NaN.  The arithmetic guess is settled against the edges.
__device__ inline int map_cell(double v, double lo, double hi, double width, int n) {
  if (!(v >= lo && v <= hi)) return -1;
  if (v == hi) return n - 1;
  const double g = (v - lo) / width * (double)n;
  int c = g < (double)(n - 1) ? (int)g : n - 1;
  while (c > 0 && map_edge(lo, width, c, n) > v) --c;
  while (c < n - 1 && map_edge(lo, width, c + 1, n) <= v) ++c;
  return c;
}

__device__ inline bool map_grid_ok(const double *g) {
  const double wz = g[1] - g[0], wn = g[3] - g[2];
  const double inf = __builtin_inf();
  bool ok = true;
  for (int i = 0; i < 4; ++i) ok = ok && g[i] > -inf && g[i] < inf;
  return ok && g[1] > g[0] && g[3] > g[2] && wz < inf && wn < inf;
}

// a ranks before b: the larger mass, ties by the smaller index
__device__ inline bool map_before(double ma, int ia, double mb, int ib) { return ma > mb || (ma == mb && ia < ib); }

__global__ __launch_bounds__(256) void k_posterior_maps(PosteriorMapsArgs a) {
  __shared__ double smap[kMapMaxCells];     // the map; after the sort the masses in rank order, then C
  __shared__ uint16_t sidx[kMapMaxCells];   // the cell of each rank
  __shared__ double sw[kPostTile];
  __shared__ int32_t scell[kPostTile];
  __shared__ double red[4];
  __shared__ int32_t s_npos;

  const int tid = threadIdx.x;
  const int md = a.md, cells = a.nz * a.nn;
  const int64_t blk = blockIdx.x;
  const int64_t r = blk / (md * md);
  const int mj = (int)(blk - r * (md * md));
  const int m = mj / md + 1, j = mj - (m - 1) * md;       // this block's model (m absorbers) and slot (0-based)
  if (j >= m) return;                                      // (the host prefilled the slot's outputs)
  const int64_t o = blk;                                   // [n][md][md]
  const int64_t S = a.S;
  const double *row = a.sll + a.row_start[r] + (int64_t)(m - 1) * S;
  const uint32_t *brow = a.base ? a.base + a.base_start[r] : nullptr;
  const double *g = a.grid + 4 * r;
  const bool grid_ok = map_grid_ok(g);
  int32_t st = grid_ok ? 0 : kMapBadGrid;

  // ---- the model: max l and T, as k_parameter_summaries takes them ----
  double mx = -__builtin_inf();
  for (int64_t i = tid; i < S; i += 256) {
    const double l = post_ll(row, brow, m, S, i);
    if (l == l) mx = fmax(mx, l);
  }
  mx = post_block_max(mx, red);
  if (!(mx > -__builtin_inf() && mx < __builtin_inf())) st |= kMapUnusable;
  if (st) {                                                // every output of the slot stays NaN / -1
    if (tid == 0) a.slot_status[o] = st;
    return;
  }
  CompSum cT;
  for (int64_t i = tid; i < S; i += 256) cT.add(post_weight(post_ll(row, brow, m, S, i), mx));
  const double T = post_block_sum(cT.value(), red);

  const double zmin = a.z_min[r], dz = a.z_max[r] - zmin;
  const bool mapped = a.n_lo != nullptr;
  const double nlo = mapped ? a.n_lo[r] : 0.0, nw = mapped ? a.n_hi[r] - a.n_lo[r] : 1.0;
  const double gz_lo = g[0], gz_hi = g[1], gn_lo = g[2], gn_hi = g[3];
  const double wz = gz_hi - gz_lo, wn = gn_hi - gn_lo;

  // ---- the map: a cell's weights in sample order, by the thread that owns the cell ----
  for (int c = tid; c < cells; c += 256) smap[c] = 0.0;
  double out_acc = 0.0;                                    // the same sum in every thread
  for (int64_t t0 = 0; t0 < S; t0 += kPostTile) {
    const int nt = (int)((S - t0 < kPostTile) ? (S - t0) : kPostTile);
    __syncthreads();
    for (int q = tid; q < nt; q += 256) {
      const int64_t i = t0 + q;
      const int64_t b = post_base(brow, j, S, i);
      sw[q] = post_weight(post_ll(row, brow, m, S, i), mx);
      const double z = zmin + dz * a.offsets[b], ln = post_log_n(mapped, nlo, nw, a.lnhi[b]);
      const int cz = map_cell(z, gz_lo, gz_hi, wz, a.nz), cn = map_cell(ln, gn_lo, gn_hi, wn, a.nn);
      scell[q] = (cz < 0 || cn < 0) ? -1 : cz * a.nn + cn;
    }
    __syncthreads();
    for (int q = 0; q < nt; ++q) {                         // every lane reads the same sample: LDS broadcasts
      const double w = sw[q];
      const int32_t c = scell[q];
      if (w > 0.0) {                                       // a sample of weight 0 does not exist
        if (c < 0) out_acc += w;
        else if ((c & 255) == tid) smap[c] += w;
      }
    }
  }
  __syncthreads();

  // ---- masses; the sort's padding ranks behind every cell ----
  int P = 1;
  while (P < cells) P <<= 1;
  double *gm = a.mass + o * cells;
  for (int c = tid; c < P; c += 256) {
    if (c < cells) {
      const double ms = smap[c] / T;
      smap[c] = ms;
      gm[c] = ms;
    } else {
      smap[c] = -1.0;
    }
    sidx[c] = (uint16_t)c;
  }
  if (tid == 0) a.outside[o] = out_acc / T;
  __syncthreads();

  // ---- bitonic sort of (mass, index): mass descending, ties by index ascending ----
  for (int k = 2; k <= P; k <<= 1) {
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int t = tid; t < (P >> 1); t += 256) {
        const int lo = ((t & ~(s - 1)) << 1) | (t & (s - 1)), hi = lo | s;
        const bool up = (lo & k) == 0;                     // this run sorts towards the front
        const double m0 = smap[lo], m1 = smap[hi];
        const int i0 = sidx[lo], i1 = sidx[hi];
        const bool swap = up ? map_before(m1, i1, m0, i0) : map_before(m0, i0, m1, i1);
        if (swap) {
          smap[lo] = m1;
          smap[hi] = m0;
          sidx[lo] = (uint16_t)i1;
          sidx[hi] = (uint16_t)i0;
        }
      }
      __syncthreads();
    }
  }

  // ---- C in rank order by one lane; the credible masses ----
  if (tid == 0) {
    int next = 0, npos = 0;
    double C = 0.0, last = __builtin_nan("");
    for (int k = 0; k < cells; ++k) {
      const double ms = smap[k];
      if (!(ms > 0.0)) break;
      C = C + ms;
      smap[k] = C;
      last = ms;
      npos = k + 1;
      while (next < a.L && C >= a.level[next]) {           // the masses increase: so do their ranks
        a.hpd_cells[o * a.L + next] = npos;
        a.hpd_threshold[o * a.L + next] = ms;
        ++next;
      }
    }
    if (next < a.L) st |= kMapShort;                       // too much mass outside: every positive cell
    for (; next < a.L; ++next) {
      a.hpd_cells[o * a.L + next] = npos;
      a.hpd_threshold[o * a.L + next] = last;
    }
    a.mode[o] = npos ? (int32_t)sidx[0] : -1;
    a.slot_status[o] = st;
    s_npos = npos;
  }
  __syncthreads();
  if (a.hpd_level) {
    double *gl = a.hpd_level + o * cells;
    const int npos = s_npos;
    for (int k = tid; k < cells; k += 256) gl[sidx[k]] = k < npos ? smap[k] : __builtin_nan("");
  }
}

__global__ __launch_bounds__(256) void k_posterior_maps_mix(PosteriorMixArgs a) {
  __shared__ double sint[kMapMaxCells];
  const int tid = threadIdx.x, md = a.md, cells = a.cells;
  const int64_t r = blockIdx.x;
  const int32_t *ss = a.slot_status + r * md * md;
  const double *w = a.weights + r * md;
  const double nan = __builtin_nan("");
  // the grid is the row's: a bad one shows in every slot; the weights are judged on a good grid only
  const bool grid_bad = (ss[0] & kMapBadGrid) != 0;
  bool bad = false;
  for (int m = 0; m < md; ++m) {
    const double wm = w[m];
    if (!(wm >= 0.0)) bad = true;                                          // NaN or negative
    else if (wm > 0.0 && (ss[m * md] & kMapUnusable)) bad = true;          // weight on an unusable model
  }
  if (grid_bad || bad) {
    for (int c = tid; c < cells; c += 256) a.intensity[r * cells + c] = nan;
    if (tid == 0) {
      a.expected[r] = nan;
      a.row_status[r] = (bad && !grid_bad) ? kMapBadWeights : 0;
    }
    return;
  }
  const double *mass = a.mass + r * md * md * cells;
  for (int c = tid; c < cells; c += 256) {
    double acc = 0.0;
    for (int m = 0; m < md; ++m) {
      const double wm = w[m];
      if (wm == 0.0) continue;                                             // skipped, usable or not
      double s = 0.0;
      for (int j = 0; j <= m; ++j) s += mass[(int64_t)(m * md + j) * cells + c];
      acc += wm * s;
    }
    sint[c] = acc;
    a.intensity[r * cells + c] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;
    for (int c = 0; c < cells; ++c) e += sint[c];
    a.expected[r] = e;
    a.row_status[r] = 0;
  }
}

}  // namespace gpdla
