// continuum_solve.hpp -- the device pieces the three continuum kernels share: k_spectra_continuum,
// k_mc_finish (4.23) and k_pf_finish (4.24) solve the same low-rank system and evaluate the same model rows, and
// k_mc_solve / k_pf_solve invert the same packed factor.  Each piece is stated once here, so a guard on a pivot or a
// change of the tile reaches every kernel, and the kernels agree to the last bit because they run the same code.
//
//   packed_unpack          (i, j) of an entry of a packed lower triangle
//   ContinuumModelArgs     the model and the mean-flux suppression, as one kernel argument
//   model_bracket          a rest wavelength in the model's grid: cell and fraction
//   model_tile_rows        m_p and mu_p of a tile of pixels into LDS (block-wide)
//   continuum_null_solve   [vech(B) | v] of a quasar under one absorption row, + I, packed Cholesky, c (block-wide)
//   packed_inverse_column  column cx of X = L^-1
//   packed_gram_entry      entry (ia, ib) of X'X = (L L')^-1
//
// __device__ __forceinline__ only: a kernel keeps its own __shared__ arrays and passes pointers.
#pragma once
#include "batch_types.hpp"

namespace gpdla {

// (i, j), i >= j, of entry e of a packed lower triangle stored row by row
__device__ __forceinline__ void packed_unpack(int e, int *pi, int *pj) {
  int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  while (i * (i + 1) / 2 > e) --i;
  *pi = i;
  *pj = e - i * (i + 1) / 2;
}

// multi :267-285 at one observed wavelength (the arithmetic of k_prepare): exp(-Sum_l tau_l (1 + z_l)^beta)
__device__ __forceinline__ double spectra_mean_flux(double wl, double z_qso, double lya_wavelength, double prev_tau_0,
                                                    double prev_beta, int num_forest_lines) {
  const double f_1 = g_lines.osc[0];
  double total = 0.0;
  for (int l = 0; l < num_forest_lines; ++l) {
    const double wl_l = g_lines.wavelength_cm[l] * 1e8;
    const double z_l = (wl - wl_l) / wl_l;                                       // multi :184-186
    const double tau_l = prev_tau_0 * g_lines.osc[l] / f_1 * wl_l / lya_wavelength;
    const double od = tau_l * pow(1 + z_l, prev_beta);                           // multi :275-276
    if (l > 0 && z_l > z_qso) continue;                                          // multi :279-282
    total += od;
  }
  return exp(-total);                                                            // multi :285
}

// What it takes to evaluate mu_p and m_p at a pixel: the model's grid and, under meanflux, the suppression of
// the multi-DLA driver (1 otherwise).
struct ContinuumModelArgs {
  ModelDev model;
  double lya_wavelength, prev_tau_0, prev_beta;
  int32_t meanflux, num_forest_lines;

  __device__ __forceinline__ double mean_flux(double wl, double z_qso) const {
    return meanflux ? spectra_mean_flux(wl, z_qso, lya_wavelength, prev_tau_0, prev_beta, num_forest_lines) : 1.0;
  }
};

// The cell [rest[lo], rest[lo + 1]] of the model's grid that brackets `rest` (the end cells beyond the grid) and the
// fraction t along it: the interpolation of k_prepare (griddedInterpolant 'linear', process_qsos.m:66-71).
__device__ __forceinline__ double model_bracket(const ModelDev &model, double rest, int *plo) {
  const int G = model.G;
  int lo = 0, hi = G - 1;
  if (rest >= model.rest[G - 1]) lo = G - 2;
  else if (rest > model.rest[0]) {
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (model.rest[mid] <= rest) lo = mid; else hi = mid;
    }
  }
  *plo = lo;
  return (rest - model.rest[lo]) / (model.rest[lo + 1] - model.rest[lo]);
}

// m_p (suppressed under meanflux) and mu_p of the pixels p0 .. p0 + np of a quasar's grid (lam: its n_u wavelengths),
// interpolated as k_prepare interpolates a kept pixel (process_qsos.m:138-139, multi :287-288): rows[pl * stride + cm],
// mu[pl]; mf[pl] is the suppression.  Pixels past n_u repeat the last one.  All 256 threads; one barrier inside,
// after which mf is complete; rows and mu are the caller's to publish.
__device__ __forceinline__ void model_tile_rows(const ContinuumModelArgs &g, const double *lam, double z_qso, int n_u, int p0,
                                                int np, double *rows, int stride, double *mu, double *mf, int tid) {
  const int k = g.model.k, G = g.model.G;
  for (int pl = tid; pl < np; pl += 256) {
    const int p = min(p0 + pl, n_u - 1);
    mf[pl] = g.mean_flux(lam[p], z_qso);
  }
  __syncthreads();
  for (int e = tid; e < np * (k + 1); e += 256) {
    const int pl = e / (k + 1), cm = e - pl * (k + 1);
    const int p = min(p0 + pl, n_u - 1);
    int lo;
    const double t = model_bracket(g.model, lam[p] / (1 + z_qso), &lo);
    if (cm == k) {
      double val = g.model.mu[lo] + (g.model.mu[lo + 1] - g.model.mu[lo]) * t;
      if (g.meanflux) val = val * mf[pl];
      mu[pl] = val;
    } else {
      const double m0 = g.model.M[lo + (int64_t)cm * G], m1 = g.model.M[lo + 1 + (int64_t)cm * G];
      rows[pl * stride + cm] = (m0 + (m1 - m0) * t) * mf[pl];
    }
  }
}

// The coefficients of the low-rank continuum under one absorption row.  With the prepared rows of k_prepare (pix: y, mu,
// omega2, nu; Mi: the M rows; a masked pixel is the neutral row and drops out of every sum) and a = absn on the grid
// (nullptr: ones, the null model):
//   d = a^2 omega2 + nu,  r = y - a mu,  B = I + M' diag(a^2 / d) M,  v = M' (a r / d),  L L' = B,  c = L'^-1 L^-1 v
// All 256 threads, barriers included.  Entry e = tid + 256 t of [vech(B) | v] is accumulated by thread tid over tiles of
// TILE pixels in pixel order (the tile only stages the weights: the sums do not depend on it); the Cholesky runs column by column (as k_lowrank_single), the two substitutions on
// thread 0.  On return s_B holds the packed L and, from s_B + k (k + 1) / 2, c; *s_pd is CLEARED when a pivot is not
// positive (the caller sets it to 1 beforehand, and writes the status).  L is published to the block; c is thread 0's
// until the caller's next barrier.  s_B: k (k + 1) / 2 + k doubles, s_wt and s_ut: TILE <= 256 each.
template <int TILE>
__device__ __forceinline__ void continuum_null_solve(const PixelRow *pix, const double *Mi, int n_u, int k, const double *absn,
                                                     double *s_B, double *s_wt, double *s_ut, double *s_piv, int *s_pd,
                                                     int tid) {
  constexpr int kNb = GPDLA_MAX_K * (GPDLA_MAX_K + 1) / 2;
  const int nb = k * (k + 1) / 2;
  // the entries of [vech(B) | v] this thread accumulates (at most 4 for k = 40), as (i, j); j < 0: v_i
  constexpr int kMine = (kNb + GPDLA_MAX_K + 255) / 256;
  int ei[kMine], ej[kMine];
  double acc[kMine];
#pragma unroll
  for (int t = 0; t < kMine; ++t) {
    const int e = tid + 256 * t;
    acc[t] = 0.0;
    ei[t] = ej[t] = -1;
    if (e < nb) packed_unpack(e, &ei[t], &ej[t]);
    else if (e < nb + k) ei[t] = e - nb;
  }
  for (int p0 = 0; p0 < n_u; p0 += TILE) {
    if (tid < TILE) {
      const int p = p0 + tid;
      double wt = 0.0, ut = 0.0;
      if (p < n_u) {
        const PixelRow row = pix[p];
        const double ab = absn ? absn[p] : 1.0;
        const double d = ab * ab * row.omega2 + row.nu;
        const double r = row.y - ab * row.mu;
        wt = ab * ab / d;
        ut = ab * r / d;
      }
      s_wt[tid] = wt;
      s_ut[tid] = ut;
    }
    __syncthreads();
    const int np = min(TILE, n_u - p0);
#pragma unroll
    for (int t = 0; t < kMine; ++t) {
      if (ei[t] < 0) continue;
      const double *Mp = Mi + (int64_t)p0 * k;
      double sum = acc[t];
      if (ej[t] >= 0)
        for (int p = 0; p < np; ++p) sum = fma(Mp[p * k + ei[t]] * s_wt[p], Mp[p * k + ej[t]], sum);
      else
        for (int p = 0; p < np; ++p) sum = fma(Mp[p * k + ei[t]], s_ut[p], sum);
      acc[t] = sum;
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < kMine; ++t)
    if (ei[t] >= 0) s_B[tid + 256 * t] = acc[t] + ((ej[t] == ei[t]) ? 1.0 : 0.0);
  __syncthreads();
  double *v = s_B + nb;
  for (int j = 0; j < k; ++j) {
    const int rj = j * (j + 1) / 2;
    __syncthreads();
    if (tid == 0) {
      double sum = s_B[rj + j];
      for (int mm = 0; mm < j; ++mm) sum = fma(-s_B[rj + mm], s_B[rj + mm], sum);
      if (!(sum > 0.0)) *s_pd = 0;
      const double ljj = sqrt(sum);
      s_B[rj + j] = ljj;
      *s_piv = ljj;
    }
    __syncthreads();
    const double ljj = *s_piv;
    for (int i = j + 1 + tid; i < k; i += 256) {
      const int ri = i * (i + 1) / 2;
      double sum = s_B[ri + j];
      for (int mm = 0; mm < j; ++mm) sum = fma(-s_B[ri + mm], s_B[rj + mm], sum);
      s_B[ri + j] = sum / ljj;
    }
  }
  __syncthreads();
  if (tid == 0) {  // c = L'^-1 L^-1 v
    for (int i = 0; i < k; ++i) {
      const int ri = i * (i + 1) / 2;
      double zi = v[i];
      for (int mm = 0; mm < i; ++mm) zi = fma(-s_B[ri + mm], v[mm], zi);
      v[i] = zi / s_B[ri + i];
    }
    for (int i = k - 1; i >= 0; --i) {
      double ci = v[i];
      for (int mm = i + 1; mm < k; ++mm) ci = fma(-s_B[mm * (mm + 1) / 2 + i], v[mm], ci);
      v[i] = ci / s_B[i * (i + 1) / 2 + i];
    }
  }
}

// Column cx of X = L^-1, L and X packed lower triangles (one thread per column; a column reads only itself)
__device__ __forceinline__ void packed_inverse_column(const double *L, double *X, int k, int cx) {
  X[cx * (cx + 1) / 2 + cx] = 1.0 / L[cx * (cx + 1) / 2 + cx];
  for (int ii = cx + 1; ii < k; ++ii) {
    const int ri = ii * (ii + 1) / 2;
    double sum = 0.0;
    for (int mm = cx; mm < ii; ++mm) sum = fma(L[ri + mm], X[mm * (mm + 1) / 2 + cx], sum);
    X[ri + cx] = -sum / L[ri + ii];
  }
}

// Entry (ia, ib), ia >= ib, of X'X = (L L')^-1: Sum_{m >= ia} X[m][ia] X[m][ib]
__device__ __forceinline__ double packed_gram_entry(const double *X, int k, int ia, int ib) {
  double sig = 0.0;
  for (int mm = ia; mm < k; ++mm) {
    const int rm = mm * (mm + 1) / 2;
    sig = fma(X[rm + ia], X[rm + ib], sig);
  }
  return sig;
}

}  // namespace gpdla
