// batch_types.hpp -- the types and constants every subsystem shares: the MFMA operand maps (Mat<T>), the Lyman-series
// table in constant memory (g_lines), what k_prepare leaves per quasar and per pixel (QuasarMeta, PixelRow), the model
// and the configuration as kernel arguments, the layout of a K-step record, and the block-wide reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

namespace gpdla {

typedef double d4 __attribute__((ext_vector_type(4)));

typedef float f4 __attribute__((ext_vector_type(4)));

// Precision of the [W | U] * [P | M] contraction.  double: v_mfma_f64_16x16x4_f64 (the shipped,
// parity-grade path).  float: v_mfma_f32_16x16x4_f32 on the XDL matrix cores -- BASELINE config 5's
// "fp32 mixed-precision variant with fp64 log-det accumulation": weights, quadratic form and log
// determinant stay fp64, only B and v are accumulated in fp32 (a speed/accuracy study, not parity).
// Both instructions take A[row l&15][k l>>4], B[k l>>4][col l&15]; the result maps differ:
// f64: row = (l>>4) + 4 reg;  f32: row = 4 (l>>4) + reg  (col = l&15 in both).
template <typename T> struct Mat;
template <> struct Mat<double> {
  using acc_t = d4;
  static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int sample_of(int jj, int r) { return jj + 4 * r; }
  static __device__ __forceinline__ int jj_of(int sample) { return sample & 3; }
  static __device__ __forceinline__ int reg_of(int sample) { return sample >> 2; }
};
template <> struct Mat<float> {
  using acc_t = f4;
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int sample_of(int jj, int r) { return 4 * jj + r; }
  static __device__ __forceinline__ int jj_of(int sample) { return sample >> 2; }
  static __device__ __forceinline__ int reg_of(int sample) { return sample & 3; }
};

constexpr int kMaxLines = 31;
constexpr int kSamplesPerWave = 16;   // rows of the 16x16x4 MFMA
constexpr double kLog2Pi = 1.83787706640934534;  // log_mvnpdf_low_rank.m:7

// Lyman-series constants in device constant memory (filled once per process from
// include/gpdla_lyman_series.h).
struct LineTable {
  double wavelength_cm[kMaxLines];  // voigt.c:31
  double leading[kMaxLines];        // voigt.c:151
  double osc[kMaxLines];            // oscillator strengths, voigt.c:66 (multi-DLA mean-flux model)
  double y[kMaxLines];              // gamma_j / (sqrt2 sigma): damping parameter of w(z)
  double y2[kMaxLines];             // y_j^2
  double cwing[kMaxLines];          // leading_j * y_j            (wing formula prefactor)
  double t2[kMaxLines];             // kE2 - 2 y_j^2: rho^2 coefficient of T(rho) - 2 y^2 rho^2 (wing formula)
  double taps[7];                   // voigt.c:242-251
  double c;                         // voigt.c:22
  double inv_sqrt2_sigma;           // 1/(sqrt2 sigma)
  double inv_sqrt2pi_sigma;         // 1/(sqrt(2 pi) sigma)
  const double *near_poly;          // [31][kNearIntervals][kNearCoef], near_tables.hpp (device memory)
  // wing tier of a run-time line count, one 32-byte entry per line (one scalar load each):
  // x_j = lambda / (1 + z) kms_j - c / (sqrt2 sigma) with kms_j = c / (wavelength_j 1e8) / (sqrt2 sigma).
  struct WingLine {
    double kms, y2, cwing, pad;
  } wing[kMaxLines];
};
__constant__ LineTable g_lines;

// Per-quasar metadata produced by k_prepare.
struct QuasarMeta {
  int32_t n_u;       // pixels in the modelled rest range (process_qsos.m:104-108)
  int32_t n_kept;    // of those, not masked (:110)
  int32_t steps;     // ceil(n_u / 4): K-steps of the contraction
  int32_t status;    // 0 ok, 1 empty, 3 a kept pixel with noise variance <= 0 or NaN (skipped)
  double min_z_dla;  // :159
  double max_z_dla;  // :160
  int64_t pix_off;   // first row of this quasar in the pixel pools (multiple of 4)
  int64_t lam_off;   // first entry in the padded-wavelength pool
  int64_t rec_off;   // first K-step record in the record pool (records of a group of quasars share the
                     // pool: PrepareArgs::rec_off; without groups it is pix_off / 4)
  // What the kept pixels of noise variance above kNeutralNoiseVariance contribute, added to each
  // result: the sweeps see such a pixel as a neutral row.  -inf when one has variance +inf (a zero
  // inverse variance the mask missed): log_mvnpdf_low_rank.m:30 then sums log(inf) into the
  // log-determinant and every log-likelihood of the quasar is -inf.  Otherwise the sum of their
  // -log(nu)/2 (0 when there are none).  So the K-loop never sees a d above 1e100 + omega2 a^2: its
  // fast reciprocals would return NaN for an infinite d (where exact division gives 0) and overflow
  // or flush to 0 on products with a d above ~1e280, and its two-step log-determinant product would
  // overflow for two such d in one lane.
  double ll_bias;
};

// A kept pixel of finite noise variance nu above this (and finite flux) is swept as a neutral row
// (r = 0, d = 1, zero M row) and its -log(nu)/2 goes into QuasarMeta::ll_bias.  What the neutral row
// drops from log_mvnpdf_low_rank.m -- r^2/d, log(d / nu) = log(1 + omega2 a^2 / nu), and the row's
// M a M a' / d in B = I + M' D^-1 M -- is below 1e-39 in absolute value while |y|, |mu|, |M| and
// omega2 stay below 1e30 (absorption a <= 1), against the pixel's own log(nu)/2 > 115.
constexpr double kNeutralNoiseVariance = 1e100;

struct PixelRow {  // one row of the per-pixel pool, on the unmasked-range grid
  double y, mu, omega2, nu;
};

struct Config {
  double min_lambda, max_lambda, lya_wavelength, lyman_limit, pixel_spacing, max_z_cut, min_z_cut;
  int32_t num_lines;
};

struct ModelDev {
  int32_t G, k;
  const double *rest, *mu, *M, *log_omega;
  double c_0, tau_0, beta;
};

constexpr int kSummaryCols = 15;  // doubles of a summary row (k_evidence; GPDLA_SUMMARY_COLS in gpdla.h)

// The layout of a K-step record (k_build_records in prepare_kernels.hpp describes what the fields hold).
// Tile classes.  k <= 40: ntiles = 52 w-tiles + 4 u-tiles.  k <= 20 ("compact", ntiles == 14): 13
// FULL w-tiles (vech columns 0..207) + 1 full u-tile (m columns 0..15) on the matrix cores; the
// remaining 2 vech columns (208, 209) and 4 m columns (16..19) would each occupy a tile that is
// 7/8 resp. 3/4 empty -- 128 of the 1024 MFMA cycles of a K-step -- and are accumulated with 6
// FMAs per lane and K-step instead (kXW / kXU, operands in the record's extras).
constexpr int kCompactTiles = 14, kXW = 2, kXU = 4, kXWColumn = 208, kXUColumn = 16;
__host__ __device__ constexpr bool tiles_compact(int ntiles) { return ntiles == kCompactTiles; }
// doubles of per-step extras behind the tiles of a record
// (compact: 4 x 11 used of 64, which also makes a record a whole number of 512-byte tiles)
// (other classes: 20 used of 128, which makes a record a whole number of KiB for the chunk copy)
__host__ __device__ constexpr int record_extras(int ntiles) { return tiles_compact(ntiles) ? 64 : 128; }
// offsets into the extras of pixel jj's PixelRow and of its padded wavelength; compact class: of
// its m columns 16..19 and vech columns 208, 209 relative to the PixelRow
__host__ __device__ constexpr int extras_row(int ntiles, int jj) { return tiles_compact(ntiles) ? 16 * jj : 4 * jj; }
__host__ __device__ constexpr int extras_lam(int ntiles, int jj) { return tiles_compact(ntiles) ? 16 * jj + 10 : 16 + jj; }
__host__ __device__ constexpr int extras_lam_stride(int ntiles) { return extras_lam(ntiles, 1) - extras_lam(ntiles, 0); }
constexpr int kExtrasXU = 4, kExtrasXW = 8;
// tiles' worth of columns a sample's [vech(B) | v] occupies in the epilogue's LDS rows
__host__ __device__ constexpr int logical_tiles(int ntiles) { return tiles_compact(ntiles) ? 16 : ntiles; }
// doubles per record: tiles (64 elements each, as double or float) + the extras
__host__ __device__ constexpr int record_doubles(int ntiles, int f32_tiles) {
  return ntiles * (f32_tiles ? 32 : 64) + record_extras(ntiles);
}

// Block-wide reductions.
__device__ __forceinline__ double block_reduce_sum(double v, double *sh) {  // (fixed order: deterministic)
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += sh[w];
  return r;
}

__device__ __forceinline__ double block_reduce_minmax(double v, bool is_min, double *sh) {
  for (int o = 32; o > 0; o >>= 1) {
    double other = __shfl_xor(v, o);
    v = is_min ? fmin(v, other) : fmax(v, other);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = is_min ? fmin(r, sh[w]) : fmax(r, sh[w]);
  return r;
}

}  // namespace gpdla
