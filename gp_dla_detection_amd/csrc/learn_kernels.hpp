// learn_kernels.hpp -- the data-parallel half of learning the quasar GP model: the reference's
// learn_qso_model.m:27-84 (single-DLA model) and multi_dlas/learn_qso_model_meanflux.m:27-138
// (mean-flux model), up to the PCA covariance.  The eigen-decomposition and the L-BFGS driver run
// on the host (gp_dla_detection_amd/training.py); the objective they minimise reads the buffers
// these kernels write, in place.
//
//   k_learn_rest_grid     one block per quasar: interp1 of flux, noise and 1 + z onto the rest grid
//                         (learn_qso_model.m:37-60), the noise mask (:64-67) and, for the mean-flux
//                         model, the 31-line optical depth and the division by exp(-tau)
//                         (learn_qso_model_meanflux.m:61-126), written straight into the training
//                         handle's quasar-major, 16-padded rows
//   k_learn_colsum        partial column sums (sum, sum of squares, count of finite entries) over a
//                         contiguous range of quasars; k_learn_colfinish adds the partials in split
//                         order: nanmean (:70), nanstd (:87), the complete-row mean of pca 'complete'
//   k_learn_center        centred = rest_fluxes - mu, in place (:71)
//   k_learn_rowflag       per quasar: 1 if every rest pixel of its flux is finite (pca 'rows','complete')
//   k_learn_gram          P = X'X and N = M'M on v_mfma_f64_16x16x4_f64 over lower-triangular 16 x 16
//                         tile pairs, split along the quasars into partial sums; k_learn_gram_finish
//                         adds them in split order and writes cov = P / (N - 1), exactly symmetric
//
// No atomics anywhere: every sum has a fixed order, so results are bit-identical run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpdla {

typedef double learn_d4 __attribute__((ext_vector_type(4)));  // one f64 16x16x4 accumulator per lane

constexpr int kLearnMaxLines = 31;   // set_parameters_multi.m:75
constexpr int kLearnStage = 4096;    // rest wavelengths of one spectrum staged in LDS (32 KiB)

// ------------------------------------------------------------------------------------------
// k_learn_rest_grid.  Interpolation as interp1(x, v, xq, 'linear') is taken here: the bracket of xq
// is the last j with x_j <= xq, clipped to n - 2, and the value is v_j + t (v_{j+1} - v_j) with
// t = (xq - x_j) / (x_{j+1} - x_j); outside [x_1, x_n] (and for spectra of fewer than two pixels) the
// result is NaN, and a NaN neighbour makes it NaN.  The query grid min_lambda + p dlambda is exact
// for the reference's grid (multiples of 0.25).
//
// Line wavelengths: set_parameters_multi.m:77 holds all_transition_wavelengths in cm, and
// learn_qso_model_meanflux.m:67 and :113 combine them with Angstrom quantities.  Read literally,
// every line's 1 + z would be ~3e8 and every flux would be divided by exp(-huge) = 0; as the sweep
// does for the same mixed-unit code of the multi-DLA driver (prepare_kernels.hpp, wavelength_cm *
// 1e8), the host passes the table in Angstrom (line_wl) and tau0_j = prev_tau_0 f_j / f_lya *
// lambda_j / lambda_lya computed from it (line_tau0).
// ------------------------------------------------------------------------------------------
struct LearnGridArgs {
  int64_t nq, G, ld;
  const int64_t *offsets;            // [nq + 1]
  const double *wl, *flux, *noise;   // observed wavelengths (Angstrom), flux, noise variance
  const uint8_t *mask;               // nonzero = masked
  const double *z;                   // [nq]
  double min_lambda, dlambda, lya_wavelength, max_noise_variance, prev_beta;
  int32_t nfl;                       // > 1: the mean-flux model (lines 0 .. nfl-1)
  double line_wl[kLearnMaxLines], line_tau0[kLearnMaxLines];
  double *out_flux, *out_lya, *out_noise, *out_loglya;  // [nq][ld]
};

__global__ __launch_bounds__(256) void k_learn_rest_grid(LearnGridArgs a) {
  __shared__ double sx[kLearnStage];
  const int64_t q = blockIdx.x;
  const int64_t o0 = a.offsets[q], n = a.offsets[q + 1] - o0;
  const double opz = 1.0 + a.z[q];
  const double *wl = a.wl + o0, *fl = a.flux + o0, *nv = a.noise + o0;
  const uint8_t *mk = a.mask + o0;
  const bool staged = n <= kLearnStage;
  if (staged)  // emitted_wavelengths (set_parameters.m:14-15): observed / (1 + z)
    for (int64_t j = threadIdx.x; j < n; j += blockDim.x) sx[j] = wl[j] / opz;
  __syncthreads();
  auto X = [&](int64_t j) { return staged ? sx[j] : wl[j] / opz; };
  const double nan = __builtin_nan("");
  double *of = a.out_flux + q * a.ld, *ol = a.out_lya + q * a.ld, *on = a.out_noise + q * a.ld,
         *og = a.out_loglya + q * a.ld;
  for (int64_t p = threadIdx.x; p < a.ld; p += blockDim.x) {
    if (p >= a.G) {  // the row padding of gpdla_training_create
      of[p] = nan;
      ol[p] = 1.0;
      on[p] = 1.0;
      og[p] = 0.0;
      continue;
    }
    const double xq = a.min_lambda + (double)p * a.dlambda;
    double f = nan, l = nan, v = nan;
    double tau = 0.0;
    if (n >= 2 && xq >= X(0) && xq <= X(n - 1)) {
      int64_t lo = 0, hi = n - 1;  // X(lo) <= xq throughout: find the last such j
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (X(mid) <= xq) lo = mid;
        else hi = mid - 1;
      }
      const int64_t j = lo < n - 2 ? lo : n - 2;
      const double x0 = X(j), x1 = X(j + 1);
      const double t = (xq - x0) / (x1 - x0);
      auto lerp = [&](double v0, double v1) { return v0 + t * (v1 - v0); };
      // learn_qso_model.m:47-48: masked pixels are NaN in flux and noise (not in lya_1pzs)
      f = lerp(mk[j] ? nan : fl[j], mk[j + 1] ? nan : fl[j + 1]);
      v = lerp(mk[j] ? nan : nv[j], mk[j + 1] ? nan : nv[j + 1]);
      const double lw = a.lya_wavelength;
      l = lerp(1.0 + (wl[j] - lw) / lw, 1.0 + (wl[j + 1] - lw) / lw);
      const bool noisy = v > a.max_noise_variance;  // :64-67 (NaN noise is not > max)
      if (noisy) f = l = v = nan;
      if (a.nfl > 1 && !noisy) {
        // learn_qso_model_meanflux.m:61-76 (each line's 1 + z interpolated, lines past the first
        // times the indicator 1 + z_line <= 1 + z_qso) and :98-126 (nansum of tau0_j (1 + z_j)^beta)
        for (int jl = 0; jl < a.nfl; ++jl) {
          const double lj = a.line_wl[jl];
          double zj = lerp(1.0 + (wl[j] - lj) / lj, 1.0 + (wl[j + 1] - lj) / lj);
          if (jl > 0) zj = zj * (zj <= opz ? 1.0 : 0.0);
          const double tj = a.line_tau0[jl] * pow(zj, a.prev_beta);
          if (tj == tj) tau += tj;
        }
      }
    }
    if (a.nfl > 1) {  // :128-129: flux / exp(-tau), noise / exp(-tau)^2
      const double absorption = exp(-tau);
      f = f / absorption;
      v = v / (absorption * absorption);
    }
    of[p] = f;
    ol[p] = l;
    on[p] = v;
    og[p] = log(l);
  }
}

// ------------------------------------------------------------------------------------------
// Column statistics.  Threads run along the pixels of a row (coalesced); split s of the grid's y
// dimension sums the quasars [nq s / S, nq (s + 1) / S) in order.  With w != NULL only quasars with
// w[q] != 0 count (the complete rows).
// ------------------------------------------------------------------------------------------
struct LearnColArgs {
  const double *x;      // [nq][ld]
  const double *w;      // [nq] or NULL
  int64_t nq, ld;
  int32_t nsplit;
  double *part;         // [nsplit][3][ld]: sum, sum of squares, count
};

__global__ __launch_bounds__(256) void k_learn_colsum(LearnColArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.ld) return;
  const int s = blockIdx.y;
  const int64_t q0 = a.nq * s / a.nsplit, q1 = a.nq * (s + 1) / a.nsplit;
  double s1 = 0.0, s2 = 0.0, c = 0.0;
  for (int64_t q = q0; q < q1; ++q) {
    const double v = a.x[q * a.ld + p];
    if (v == v && (!a.w || a.w[q] != 0.0)) {
      s1 += v;
      s2 += v * v;
      c += 1.0;
    }
  }
  double *o = a.part + (int64_t)s * 3 * a.ld + p;
  o[0] = s1;
  o[a.ld] = s2;
  o[2 * a.ld] = c;
}

// mode 0: mean[p] = sum / count (NaN without entries); mode 1: std[p] with n - 1 (nanstd, :87; 0 for
// one entry, NaN for none); mode 2: the mean, 0 without entries (the offset of k_learn_gram, which
// multiplies (x - offset) by a weight of 0 there: a NaN offset would turn the empty sum 0 into NaN).
// count[p] = the number of entries.  Pixels in [G, ld) get mean 0.
struct LearnColFinishArgs {
  const double *part;
  int64_t G, ld;
  int32_t nsplit, mode;
  double *out, *count;
};

__global__ __launch_bounds__(256) void k_learn_colfinish(LearnColFinishArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.ld) return;
  double s1 = 0.0, s2 = 0.0, c = 0.0;
  for (int s = 0; s < a.nsplit; ++s) {
    const double *o = a.part + (int64_t)s * 3 * a.ld + p;
    s1 += o[0];
    s2 += o[a.ld];
    c += o[2 * a.ld];
  }
  double r;
  if (p >= a.G) r = 0.0;
  else if (a.mode != 1) r = c > 0.0 ? s1 / c : (a.mode == 2 ? 0.0 : __builtin_nan(""));
  else r = c > 1.0 ? sqrt((s2 - s1 * (s1 / c)) / (c - 1.0)) : (c == 1.0 ? 0.0 : __builtin_nan(""));
  a.out[p] = r;
  if (a.count) a.count[p] = c;
}

__global__ __launch_bounds__(256) void k_learn_center(double *x, const double *mu, int64_t nq, int64_t G, int64_t ld) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * ld) return;
  const int64_t p = i % ld;
  if (p < G) x[i] = x[i] - mu[p];
}

// flags[q] = 1 if every rest pixel of quasar q's flux is finite, else 0; any[q] = 1 if some is
__global__ __launch_bounds__(256) void k_learn_rowflag(const double *x, int64_t G, int64_t ld, double *flags, double *any) {
  const int64_t q = blockIdx.x;
  int missing = 0, present = 0;
  for (int64_t p = threadIdx.x; p < G; p += blockDim.x) {
    const double v = x[q * ld + p];
    if (v == v) present = 1;
    else missing = 1;
  }
  missing = __syncthreads_or(missing);
  present = __syncthreads_or(present);
  if (threadIdx.x == 0) {
    flags[q] = missing ? 0.0 : 1.0;
    any[q] = present ? 1.0 : 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// k_learn_gram.  One wave = one lower-triangular tile pair (ta >= tb) of 16 x 16 pixels and one split
// of the quasars.  A step takes 4 quasars: lane l holds quasar 4 s + (l >> 4) at pixel 16 t + (l & 15)
// of each tile, which is at once the A operand (X' rows) of tile ta and the B operand (X columns) of
// tile tb of v_mfma_f64_16x16x4_f64.  X = (x - offset_p) w_q with NaN -> 0, M = finite(x) w_q:
// pairwise: offset 0, w 1; complete: offset = the complete-row mean, w = the complete-row flag.
// Padding pixels (NaN) and quasars past nq contribute 0, so G and nq need not be multiples of 16 / 4.
// ------------------------------------------------------------------------------------------
struct LearnGramArgs {
  const double *x;        // [nq][ld]
  const double *offset;   // [ld] or NULL
  const double *w;        // [nq] or NULL
  int64_t nq, ld, npairs;
  int32_t nsplit;
  double *partP, *partN;  // [npairs][nsplit][16][16]
};

__device__ __forceinline__ void learn_pair_tiles(int64_t pair, int64_t *ta, int64_t *tb) {
  int64_t a = (int64_t)((sqrt(8.0 * (double)pair + 1.0) - 1.0) * 0.5);
  while (a * (a + 1) / 2 > pair) --a;
  while ((a + 1) * (a + 2) / 2 <= pair) ++a;
  *ta = a;
  *tb = pair - a * (a + 1) / 2;
}

__global__ __launch_bounds__(256) void k_learn_gram(LearnGramArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= a.npairs * a.nsplit) return;  // whole waves
  const int64_t pair = item / a.nsplit;
  const int h = (int)(item % a.nsplit);
  int64_t ta, tb;
  learn_pair_tiles(pair, &ta, &tb);
  const int c = lane & 15, r = lane >> 4;
  const int64_t pa = 16 * ta + c, pb = 16 * tb + c;
  const double oa = a.offset ? a.offset[pa] : 0.0, ob = a.offset ? a.offset[pb] : 0.0;
  const int64_t steps = (a.nq + 3) / 4;
  const int64_t s0 = steps * h / a.nsplit, s1 = steps * (h + 1) / a.nsplit;
  learn_d4 accP = {0.0, 0.0, 0.0, 0.0}, accN = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t q = 4 * s + r;
    double xa = 0.0, xb = 0.0, ma = 0.0, mb = 0.0;
    if (q < a.nq) {
      const double wq = a.w ? a.w[q] : 1.0;
      const double va = a.x[q * a.ld + pa], vb = a.x[q * a.ld + pb];
      if (va == va) {
        xa = (va - oa) * wq;
        ma = wq;
      }
      if (vb == vb) {
        xb = (vb - ob) * wq;
        mb = wq;
      }
    }
    accP = __builtin_amdgcn_mfma_f64_16x16x4f64(xa, xb, accP, 0, 0, 0);
    accN = __builtin_amdgcn_mfma_f64_16x16x4f64(ma, mb, accN, 0, 0, 0);
  }
  // result register rr: row (lane >> 4) + 4 rr of tile ta, column lane & 15 of tile tb
  double *oP = a.partP + item * 256, *oN = a.partN + item * 256;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    oP[(r + 4 * rr) * 16 + c] = accP[rr];
    oN[(r + 4 * rr) * 16 + c] = accN[rr];
  }
}

// One thread per element of a tile pair: the partials added in split order, cov = P / (N - 1) written
// to (a, b) and (b, a) from the one value (a >= b), so the matrix is exactly symmetric.
struct LearnGramFinishArgs {
  const double *partP, *partN;
  int64_t G, npairs;
  int32_t nsplit;
  double *cov, *count;  // [G][G]; count may be NULL
};

__global__ __launch_bounds__(256) void k_learn_gram_finish(LearnGramFinishArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.npairs * 256) return;
  const int64_t pair = i >> 8;
  const int e = (int)(i & 255);
  int64_t ta, tb;
  learn_pair_tiles(pair, &ta, &tb);
  const int64_t ra = 16 * ta + (e >> 4), cb = 16 * tb + (e & 15);
  if (ra >= a.G || cb >= a.G || cb > ra) return;
  double P = 0.0, N = 0.0;
  for (int h = 0; h < a.nsplit; ++h) {
    const int64_t o = (pair * a.nsplit + h) * 256 + e;
    P += a.partP[o];
    N += a.partN[o];
  }
  const double v = P / (N - 1.0);
  a.cov[ra * a.G + cb] = v;
  a.cov[cb * a.G + ra] = v;
  if (a.count) {
    a.count[ra * a.G + cb] = N;
    a.count[cb * a.G + ra] = N;
  }
}

}  // namespace gpdla
