// mock_kernels.hpp -- device side of the mock spectra: one draw per quasar from the
// distribution whose likelihood the sweeps evaluate (process_qsos.m:190-198),
//     flux ~ N(a mu, A (M M' + diag omega2) A + diag nu)
// on the kept pixels of the unmasked-range grid.  mu, M, omega2 are read from the pools k_prepare
// has just filled -- the rows the sweep sees, single-DLA or mean-flux -- and a from the output of
// k_spectra_map; nothing of either is computed a second time here.
//
//   k_mock_draw   z ~ N(0, I_k) per quasar, eps ~ N(0, 1) per stored pixel (Philox4x32-10),
//                 continuum = mu + M z, sigma = sqrt(a^2 omega2 + nu), flux = a continuum + sigma eps
//
// No atomics, one writer per output element, the k-term dot product in column order: outputs are
// bit-identical from run to run and depend on (seed, global quasar index, stored position) only.
#pragma once
#include "spectra_kernels.hpp"

namespace gpdla {

// One standard normal from one Philox call (gpdla.h: counter (index, stream, 1), Box-Muller on two
// 53-bit uniforms, u1 in (0, 1] so the logarithm is finite: |n| <= sqrt(106 ln 2) = 8.58).
__device__ __forceinline__ double mock_normal(uint64_t index, uint32_t stream, uint32_t k0, uint32_t k1) {
  uint32_t r[4];
  philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), stream, 1u, k0, k1, r);
  const double m1 = (double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6);
  const double m2 = (double)(r[2] >> 5) * 67108864.0 + (double)(r[3] >> 6);
  const double u1 = (m1 + 1.0) * (1.0 / 9007199254740992.0), u2 = m2 * (1.0 / 9007199254740992.0);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// ------------------------------------------------------------------------------------------
// k_mock_draw: one 256-thread block per quasar, z in LDS, one stored pixel per thread and step.  The
// stored pixels are walked in tiles of 256 with the order-preserving count of k_prepare, so that
// pixel i of the upload layout finds its row u of the grid.  flux is updated IN PLACE (the host
// hands either the batch's resident array or a copy of it): a stored pixel outside the modelled
// range and every pixel of a quasar of status != 0 are simply not written.
// ------------------------------------------------------------------------------------------
struct MockDrawArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *Mi;
  const int64_t *offsets;         // [nq + 1] upload layout
  const double *wavelengths, *noise_variance;
  const uint8_t *pixel_mask;
  const double *z_qsos;
  double min_lambda, max_lambda;
  int32_t k;
  uint64_t seed;
  int64_t first_quasar_index;
  const int64_t *grid_off;        // [nq + 1]
  const double *absorption;       // grid layout, or nullptr: ones
  double *flux;                   // upload layout, in place
  double *continuum, *sigma;      // grid layout; either may be nullptr
  double *latents;                // [nq][k] or nullptr
};

__global__ __launch_bounds__(256) void k_mock_draw(MockDrawArgs a) {
  __shared__ double s_z[GPDLA_MAX_K];
  __shared__ int s_cnt[4];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const QuasarMeta m = a.meta[q];
  const int k = a.k;
  double *cont = a.continuum ? a.continuum + a.grid_off[q] : nullptr;
  double *sig = a.sigma ? a.sigma + a.grid_off[q] : nullptr;
  if (m.status != 0) {  // nothing to draw from: no kept pixel, or a kept pixel of unusable noise variance
    for (int u = tid; u < m.n_u; u += 256) {
      if (cont) cont[u] = NAN;
      if (sig) sig[u] = NAN;
    }
    if (a.latents && tid < k) a.latents[(int64_t)q * k + tid] = NAN;
    return;
  }
  const uint64_t qid = (uint64_t)(a.first_quasar_index + q);
  const uint32_t k0 = (uint32_t)(a.seed ^ qid), k1 = (uint32_t)((a.seed >> 32) ^ (qid >> 32) ^ 0x5851F42Du);
  if (tid < k) {
    const double z = mock_normal((uint64_t)tid, 0u, k0, k1);
    s_z[tid] = z;
    if (a.latents) a.latents[(int64_t)q * k + tid] = z;
  }
  const int64_t base = a.offsets[q];
  const int npix = (int)(a.offsets[q + 1] - base);
  const double z_qso = a.z_qsos[q];
  const PixelRow *pix = a.pix + m.pix_off;
  const double *Mi = a.Mi + m.pix_off * k;
  const double *absn = a.absorption ? a.absorption + a.grid_off[q] : nullptr;
  int done = 0;  // grid pixels before this tile (block-uniform)
  for (int tile = 0; tile < npix; tile += 256) {
    const int i = tile + tid;
    bool in_range = false;
    if (i < npix) {
      const double rest = a.wavelengths[base + i] / (1 + z_qso);       // process_qsos.m:102
      in_range = (rest >= a.min_lambda) && (rest <= a.max_lambda);     // :104-105
    }
    const unsigned long long bal = __ballot(in_range);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();  // (the previous tile's s_cnt has been read; first tile: s_z is written)
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int wbase = done, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) wbase += s_cnt[w];
      total += s_cnt[w];
    }
    done += total;
    const int u = wbase + pre;
    if (in_range && u < m.n_u) {  // (u < n_u always: the same count k_prepare made; kept as the bound of every access below)
      double c = NAN, s = NAN, f = NAN;
      if (a.pixel_mask[base + i] == 0) {                               // :110
        const PixelRow row = pix[u];
        const double *Mp = Mi + (int64_t)u * k;
        c = row.mu;
        for (int j = 0; j < k; ++j) c += Mp[j] * s_z[j];
        const double ab = absn ? absn[u] : 1.0;
        s = sqrt(ab * ab * row.omega2 + a.noise_variance[base + i]);
        f = ab * c + s * mock_normal((uint64_t)i, 1u, k0, k1);
      }
      a.flux[base + i] = f;
      if (cont) cont[u] = c;
      if (sig) sig[u] = s;
    }
  }
}

}  // namespace gpdla
