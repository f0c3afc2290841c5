// condition_kernels.hpp -- a single-DLA batch conditioned on fixed absorbers (the
// contract is in include/gpdla.h, the host side in host_condition.hpp, the NumPy restatement in
// tests/conditional_restatement.py).
//
// The k-DLA likelihood (multi :342-351) multiplies mu, M and omega by the product of all k profiles.  With
// k - 1 absorbers held fixed their product A is a vector per quasar; folded once into the prepared rows
// (mu A, M A, omega2 A^2) it turns the shipped single-DLA sweeps into the k-DLA likelihood as a function of
// the remaining absorber alone.
//
//   k_condition_rows   one block of 256 threads per quasar, behind k_prepare.  A_u = the product, in list
//                      order, of the instrument-broadened profiles of the quasar's fixed absorbers on its
//                      unmasked-range grid, with the arithmetic and the tiling of k_spectra_map (250 pixels
//                      per 256 raw values, seven taps ascending).  Then, each rounded once: mu <- mu A,
//                      omega2 <- omega2 (A A), Mi[u][c] <- Mi[u][c] A.  y and nu are not touched; a neutral
//                      row (mu = omega2 = 0, zero M row) stays neutral because A is finite.  A quasar without
//                      fixed absorbers, or of status != 0, is not touched.
//   k_condition_mask   one block per quasar (of a list, or of the batch), behind a sweep.  The separation
//                      rule of multi :386-392 for one free absorber among fixed ones: an entry whose own z
//                      lies strictly closer than min_z_separation to a fixed z becomes -inf.  z is computed
//                      as the sweep that made the table computed it: lo + (hi - lo) u with (lo, hi) the
//                      quasar's search range (first pass) or its box (a boxed level).
//
// No atomics, no reductions: every output is a function of its own quasar only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spectra_kernels.hpp"

namespace gpdla {

constexpr int kMaxFixedAbsorbers = 8;

struct ConditionRowsArgs {
  const QuasarMeta *meta;   // [nq] as k_prepare left it
  const double *lam_pad;
  const int64_t *fx_off;    // [nq + 1] into fx_z / fx_n
  const double *fx_z, *fx_n;  // redshifts and column densities (not logarithms)
  int32_t num_lines, k;
  PixelRow *pix;
  double *Mi;
};

__global__ __launch_bounds__(256) void k_condition_rows(ConditionRowsArgs a) {
  __shared__ double s_raw[256];
  __shared__ double s_A[kMapTile];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int64_t j0 = a.fx_off[q], j1 = a.fx_off[q + 1];
  if (j1 <= j0) return;  // (block-uniform) no fixed absorber: the rows stay bit for bit what k_prepare wrote
  const QuasarMeta m = a.meta[q];
  if (m.status != 0) return;
  const double *lam = a.lam_pad + m.lam_off;
  PixelRow *pix = a.pix + m.pix_off;
  double *Mi = a.Mi + m.pix_off * a.k;
  const int n_pad = m.n_u + 6;
  for (int t0 = 0; t0 < m.n_u; t0 += kMapTile) {
    double prod = 1.0;
    for (int64_t j = j0; j < j1; ++j) {  // k_spectra_map's loop
      const int P = t0 + tid;
      if (P < n_pad) s_raw[tid] = spectra_raw_at(lam[P], a.fx_z[j], a.fx_n[j], a.num_lines);
      __syncthreads();
      if (tid < kMapTile && P < m.n_u) {
        double acc = 0.0;
        for (int kk = 0; kk < 7; ++kk) acc += s_raw[tid + kk] * g_lines.taps[kk];
        prod = (j == j0) ? acc : prod * acc;
      }
      __syncthreads();
    }
    const int np = min(kMapTile, m.n_u - t0);
    if (tid < np) {
      s_A[tid] = prod;
      PixelRow row = pix[t0 + tid];
      row.mu = row.mu * prod;
      row.omega2 = row.omega2 * (prod * prod);
      pix[t0 + tid] = row;
    }
    __syncthreads();
    double *Mt = Mi + (int64_t)t0 * a.k;
    for (int e = tid; e < np * a.k; e += 256) Mt[e] = Mt[e] * s_A[e / a.k];
    __syncthreads();  // (s_A and s_raw are rewritten by the next tile)
  }
}

struct ConditionMaskArgs {
  const int32_t *rows;      // [gridDim.x] quasars of the batch, or nullptr: quasar blockIdx.x
  const QuasarMeta *meta;   // the batch's
  const int32_t *status;    // [nq] refine status (a row that is not 0 was not swept), or nullptr
  const double *box;        // nullptr: z over the quasar's search range; else quasar q's (z_lo, z_hi) at box + q * kRefineBoxStride
  const double *su;         // [S] offset_samples, or the unit points' u
  int64_t S;
  const int64_t *fx_off;
  const double *fx_z;
  double sep;
  double *table;            // [nq][S]
};

__global__ __launch_bounds__(256) void k_condition_mask(ConditionMaskArgs a) {
  const int64_t q = a.rows ? a.rows[blockIdx.x] : blockIdx.x;
  const int64_t j0 = a.fx_off[q], j1 = a.fx_off[q + 1];
  if (j1 <= j0) return;
  if (a.meta[q].status != 0 || (a.status && a.status[q] != 0)) return;
  const double lo = a.box ? a.box[q * kRefineBoxStride + 0] : a.meta[q].min_z_dla;
  const double hi = a.box ? a.box[q * kRefineBoxStride + 1] : a.meta[q].max_z_dla;
  double fz[kMaxFixedAbsorbers];
  const int F = (int)min((int64_t)kMaxFixedAbsorbers, j1 - j0);
#pragma unroll
  for (int f = 0; f < kMaxFixedAbsorbers; ++f) fz[f] = f < F ? a.fx_z[j0 + f] : __builtin_inf();
  double *row = a.table + q * a.S;
  for (int64_t i = threadIdx.x; i < a.S; i += 256) {
    const double z = lo + (hi - lo) * a.su[i];
    bool close = false;
#pragma unroll
    for (int f = 0; f < kMaxFixedAbsorbers; ++f) close = close || (fmax(z, fz[f]) - fmin(z, fz[f]) < a.sep);
    if (close) row[i] = -__builtin_inf();
  }
}

}  // namespace gpdla
