// preload_kernels.hpp -- spectra as the SDSS spec files hold them -> the normalised, truncated spectra of
// preloaded_qsos.mat (read_spec.m:27-38, preload_qsos.m:26-67).
//
//   k_preload          one block per spectrum of a raw CSR set (float32 flux, loglam, ivar; int32
//                      and_mask).  Per pixel, after widening to fp64: lambda = 10^loglam, noise variance
//                      = 1 / ivar, mask = (ivar == 0) | bit 23 of and_mask (MATLAB's bitget(., 24)),
//                      rest = lambda / (1 + z).  The normaliser is the median of the non-NaN flux of
//                      the unmasked pixels inside the normalisation window, found by rank in LDS tiles
//                      (the scheme of k_sightline_snr, copied: ties broken by position, any count).
//                      No such pixel: flag bit 2; fewer than min_num_pixels unmasked pixels in the
//                      modelling range: flag bit 3; either way the quasar keeps no pixel and normaliser
//                      0, as does one whose input flag is already set.  Otherwise the pixels inside
//                      the loading range, masked or not, and the nearest unmasked pixel outside it on
//                      either side are compacted in pixel order (ballots and a scan) into a staging
//                      area at the spectrum's INPUT offset, flux / median and variance / median^2.
//   k_preload_offsets  one block: the exclusive scan of the kept counts.
//   k_preload_pack     one block per spectrum: staging -> the packed CSR output.
//
// No atomics anywhere; the output is bit-identical run to run and does not depend on how a set is
// split into calls.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpdla {

constexpr int kPreloadTile = 2048;   // window values held in LDS per step (16 KiB a buffer)

struct PreloadArgs {
  const int64_t *offsets;            // [n + 1]
  const float *flux, *loglam, *ivar; // raw columns
  const int32_t *and_mask;
  const double *z;                   // [n]
  uint8_t *flags;                    // [n] in/out
  double load_lo, load_hi, norm_lo, norm_hi, model_lo, model_hi;
  int64_t min_num_pixels;
  int32_t *count;                    // [n] kept pixels
  double *w, *f, *nv;                // staging, indexed like the input
  uint8_t *m;
  double *normalizers;               // [n]
};

struct PreloadPixel {
  double lam, rest;
  bool mask;
};

__device__ inline PreloadPixel preload_pixel(const PreloadArgs &a, int64_t p, double zp1) {
  PreloadPixel x;
  x.lam = pow(10.0, (double)a.loglam[p]);
  x.rest = x.lam / zp1;
  x.mask = a.ivar[p] == 0.0f || (((uint32_t)a.and_mask[p] >> 23) & 1u);
  return x;
}

// op 0: sum, 1: min, 2: max over the block's 256 threads (every thread gets the result)
__device__ inline int preload_reduce(int v, int op, int *scratch) {
  for (int d = 32; d > 0; d >>= 1) {
    const int o = __shfl_xor(v, d, 64);
    v = op == 0 ? v + o : (op == 1 ? (o < v ? o : v) : (o > v ? o : v));
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();   // scratch may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) scratch[wave] = v;
  __syncthreads();
  int r = scratch[0];
  for (int k = 1; k < 4; ++k) {
    const int o = scratch[k];
    r = op == 0 ? r + o : (op == 1 ? (o < r ? o : r) : (o > r ? o : r));
  }
  return r;
}

// Compacts, in pixel order, the window values (unmasked, inside the normalisation window, flux not
// NaN) whose compaction index lies in [start, start + kPreloadTile) into buf; returns their number.
__device__ inline int preload_stage(const PreloadArgs &a, int64_t p0, int np, double zp1, int start, double *buf,
                                    int *wave_tot) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  int base = 0;
  for (int t0 = 0; t0 < np; t0 += 256) {
    const int j = t0 + tid;
    bool sel = false;
    double v = 0.0;
    if (j < np) {
      const PreloadPixel x = preload_pixel(a, p0 + j, zp1);
      v = (double)a.flux[p0 + j];
      sel = x.rest >= a.norm_lo && x.rest <= a.norm_hi && !x.mask && v == v;
    }
    const unsigned long long m = __ballot(sel);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    const int total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    const int pos = off + before - start;
    if (sel && pos >= 0 && pos < kPreloadTile) buf[pos] = v;
    base += total;
    __syncthreads();
  }
  return base;
}

__global__ __launch_bounds__(256) void k_preload(PreloadArgs a) {
  __shared__ double cand[kPreloadTile], other[kPreloadTile];
  __shared__ double mid[2];
  __shared__ int wave_tot[4];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t p0 = a.offsets[s];
  const int np = (int)(a.offsets[s + 1] - p0);
  const uint8_t flag_in = a.flags[s];
  if (flag_in > 0) {   // not loaded at all (preload_qsos.m:19-21); block-uniform
    if (tid == 0) {
      a.count[s] = 0;
      a.normalizers[s] = 0.0;
    }
    return;
  }
  const double zp1 = 1.0 + a.z[s];

  // --- the normaliser: nanmedian of the window's flux ---
  const int m = preload_stage(a, p0, np, zp1, 0, cand, wave_tot);
  if (m == 0) {   // bit 2: cannot normalise
    if (tid == 0) {
      a.flags[s] = flag_in | 4;
      a.count[s] = 0;
      a.normalizers[s] = 0.0;
    }
    return;
  }
  const int k_lo = (m - 1) / 2, k_hi = m / 2;
  constexpr int kPer = kPreloadTile / 256;
  for (int c0 = 0; c0 < m; c0 += kPreloadTile) {
    if (c0 > 0) preload_stage(a, p0, np, zp1, c0, cand, wave_tot);
    const int nc = (m - c0 < kPreloadTile) ? (m - c0) : kPreloadTile;
    int rank[kPer];
    double mine[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      rank[q] = 0;
      mine[q] = (tid + 256 * q < nc) ? cand[tid + 256 * q] : 0.0;
    }
    for (int b0 = 0; b0 < m; b0 += kPreloadTile) {
      const double *src = cand;
      if (m > kPreloadTile) {   // more than one tile: the values compared against are staged apart
        preload_stage(a, p0, np, zp1, b0, other, wave_tot);
        src = other;
      }
      const int nb = (m - b0 < kPreloadTile) ? (m - b0) : kPreloadTile;
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
  const double med = (k_lo == k_hi) ? mid[0] : (mid[0] + mid[1]) / 2.0;

  // --- one pass: unmasked pixels in the modelling range; first and last pixel of the loading range ---
  int good = 0, first = np, last = -1;
  for (int j = tid; j < np; j += 256) {
    const PreloadPixel x = preload_pixel(a, p0 + j, zp1);
    good += (x.rest >= a.model_lo && x.rest <= a.model_hi && !x.mask) ? 1 : 0;
    if (x.rest >= a.load_lo && x.rest <= a.load_hi) {
      first = j < first ? j : first;
      last = j > last ? j : last;
    }
  }
  good = preload_reduce(good, 0, wave_tot);
  if ((int64_t)good < a.min_num_pixels) {   // bit 3: not enough pixels
    if (tid == 0) {
      a.flags[s] = flag_in | 8;
      a.count[s] = 0;
      a.normalizers[s] = 0.0;
    }
    return;
  }
  first = preload_reduce(first, 1, wave_tot);
  last = preload_reduce(last, 2, wave_tot);

  // --- the nearest unmasked pixel outside the loading range on either side (none: -1 / np) ---
  int below = -1, above = np;
  if (last >= 0) {
    for (int j = tid; j < np; j += 256) {
      if (j >= first && j <= last) continue;
      const PreloadPixel x = preload_pixel(a, p0 + j, zp1);
      if (x.mask) continue;   // (outside [first, last] no pixel is inside the loading range)
      if (j < first) below = j > below ? j : below;
      if (j > last) above = j < above ? j : above;
    }
    below = preload_reduce(below, 2, wave_tot);
    above = preload_reduce(above, 1, wave_tot);
  }

  // --- compaction in pixel order ---
  const double med2 = med * med;
  int base = 0;
  for (int t0 = 0; t0 < np; t0 += 256) {
    const int j = t0 + tid;
    bool keep = false;
    PreloadPixel x{};
    if (j < np && last >= 0) {
      x = preload_pixel(a, p0 + j, zp1);
      keep = (x.rest >= a.load_lo && x.rest <= a.load_hi) || j == below || j == above;
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();   // wave_tot may still be read (a reduction, or the previous step)
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    base += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    if (keep) {
      const int64_t o = p0 + off + before;   // off + before <= j: inside this spectrum's input range
      a.w[o] = x.lam;
      a.f[o] = (double)a.flux[p0 + j] / med;
      a.nv[o] = (1.0 / (double)a.ivar[p0 + j]) / med2;
      a.m[o] = x.mask ? 1 : 0;
    }
  }
  if (tid == 0) {
    a.count[s] = base;
    a.normalizers[s] = med;
  }
}

// out_offsets[0 .. n]: the exclusive scan of count[0 .. n).  One block of 256 threads; thread t owns
// the slice [t * per, (t + 1) * per).
__global__ __launch_bounds__(256) void k_preload_offsets(int64_t n, const int32_t *count, int64_t *out_offsets) {
  __shared__ int64_t part[256];
  const int tid = threadIdx.x;
  const int64_t per = (n + 255) / 256;
  const int64_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int64_t sum = 0;
  for (int64_t i = lo; i < hi; ++i) sum += count[i];
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < 256; ++t) {
      const int64_t c = part[t];
      part[t] = run;
      run += c;
    }
    out_offsets[n] = run;
  }
  __syncthreads();
  int64_t run = part[tid];
  for (int64_t i = lo; i < hi; ++i) {
    out_offsets[i] = run;
    run += count[i];
  }
}

struct PreloadPackArgs {
  const int64_t *offsets, *out_offsets;
  const int32_t *count;
  const double *w, *f, *nv;
  const uint8_t *m;
  double *out_w, *out_f, *out_nv;
  uint8_t *out_m;
};

__global__ __launch_bounds__(256) void k_preload_pack(PreloadPackArgs a) {
  const int64_t s = blockIdx.x;
  const int64_t src = a.offsets[s], dst = a.out_offsets[s];
  const int n = a.count[s];
  for (int j = threadIdx.x; j < n; j += 256) {
    a.out_w[dst + j] = a.w[src + j];
    a.out_f[dst + j] = a.f[src + j];
    a.out_nv[dst + j] = a.nv[src + j];
    a.out_m[dst + j] = a.m[src + j];
  }
}

}  // namespace gpdla
