// spectra_multi_kernels.hpp -- device side of the model spectra of a multi-DLA run: the
// per-pixel absorption averaged over the samples of every model DLA(n), n >= 2, and over the models.
//
//   k_spectra_weights_multi  the posterior weights of the S samples of model DLA(n) of a quasar: the rule of
//                            k_spectra_weights on row n - 1 of sample_log_likelihoods_dla, with a sample that
//                            consumes a base index of 0 ("never drawn") read as a NaN log-likelihood
//   k_spectra_moments_multi  Sum_i w_i b_i(p) and Sum_i w_i b_i(p)^2, b = 1 - A_{n,i}, A_{n,i} = Prod_j c_{s_j(i)}
//                            the product of the n instrument-broadened profiles of sample i's slots
//                            (multi :342-351), over 256 samples of one (quasar, model) -- the hot kernel
//   k_spectra_model_average  1 - Sum_m P_m Sum w b and the variance of the mixture over the models, from the
//                            partial sums of every model
//
// Model DLA(1) and the sub-DLA model are k_spectra_moments' (spectra_kernels.hpp); every model's chunks are
// combined by k_spectra_combine.  The two moments kernels include one body (spectra_moments_body.hpp,
// DESIGN.md 4.26); the two weights kernels are written out twice, because the softmax as one function over a value(i)
// functor reorders k_spectra_weights' instructions (same section).  Sums run in a fixed order, nothing is accumulated with atomics and an
// entry is reduced on its own: outputs are bit-identical from run to run and for any grouping.
#pragma once
#include "spectra_kernels.hpp"

namespace gpdla {

// ------------------------------------------------------------------------------------------
// k_spectra_weights_multi: one block per (entry, model) of models n_lo .. n_hi (n_lo >= 2).  Entry s reads
// row table + row_start[s] + (n - 1) S and the base rows base + base_start[s] + (j - 2) S, j = 2 .. n (1-based
// indices, 0 = never drawn).  w[(n cap + s) S + i] and flag[n flag_stride + s] as k_spectra_weights writes them.
// ------------------------------------------------------------------------------------------
struct SpectraWeightsMultiArgs {
  const double *table;
  const int64_t *row_start;   // [n]
  const uint32_t *base;
  const int64_t *base_start;  // [n]
  int64_t S, cap, flag_stride;
  int32_t n_lo, n_hi;
  double *w;                  // [1 + max_dlas][cap][S]: row 0 the sub-DLA model, row n model DLA(n)
  int32_t *flag;              // [1 + max_dlas][flag_stride]
};

__global__ __launch_bounds__(256) void k_spectra_weights_multi(SpectraWeightsMultiArgs a) {
  __shared__ double s_red[4];
  const int nm = a.n_hi - a.n_lo + 1;
  const int64_t s = blockIdx.x / nm;
  const int n = a.n_lo + (int)(blockIdx.x - s * nm), tid = threadIdx.x;
  const double *row = a.table + a.row_start[s] + (int64_t)(n - 1) * a.S;
  const uint32_t *base = a.base + a.base_start[s];
  double *w = a.w + ((int64_t)n * a.cap + s) * a.S;
  auto value = [&](int64_t i) -> double {  // the log-likelihood, NaN where a slot was never drawn
    bool drawn = true;
    for (int j = 2; j <= n; ++j) drawn = drawn && base[(int64_t)(j - 2) * a.S + i] != 0;
    return drawn ? row[i] : NAN;
  };
  double mx = -INFINITY;
  for (int64_t i = tid; i < a.S; i += 256) mx = fmax(mx, value(i));  // (fmax returns the other operand for a NaN)
  mx = block_reduce_minmax(mx, false, s_red);
  const bool none = !(mx > -INFINITY) || mx == INFINITY;
  double sum = 0.0;
  for (int64_t i = tid; i < a.S; i += 256) {
    const double l = value(i);
    const double e = (l == l) ? exp(l - mx) : 0.0;
    w[i] = e;
    sum += e;
  }
  sum = block_reduce_sum(sum, s_red);
  for (int64_t i = tid; i < a.S; i += 256) w[i] = none ? 0.0 : w[i] / sum;
  if (tid == 0) a.flag[(int64_t)n * a.flag_stride + s] = none ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// k_spectra_moments_multi: the decomposition of k_spectra_moments -- one LANE per sample, a wave of 64
// neighbours in z_DLA, a block of four waves = 256 samples of one (entry, model), 16-pixel tiles transposed
// through LDS, rows 4 e + g, then (g0 + g1) + (g2 + g3), the waves in wave order -- with the profile of a
// sample replaced by the product over its slots.  The slots are looped INSIDE the tile: slot j's line sums
// are evaluated at the tile's 22 padded pixels (the six carried raw values are recomputed: 22 / 16 of the
// line sums, nothing kept per slot in registers or LDS), broadened with the taps in ascending order and
// multiplied into the lane's own s_out row in slot order -- a lane owns its row until the transpose, so
// this needs no barrier.  Each slot takes the accurate tier under its own vote of the wave: the own samples of
// a wave are neighbours in z_DLA, the gathered ones are wherever the resampling put them.
// A sample of weight 0 (a NaN log-likelihood, a slot never drawn) is evaluated like any other and drops
// out of the sums; its missing slot reads sample 0.
// part[(((n cap + sl) chunks + chunk) 2 + moment) stride + p]
// ------------------------------------------------------------------------------------------
struct SpectraMomentsMultiArgs {
  const QuasarMeta *meta;
  const double *lam_pad;
  const double *offset_samples, *nhi;
  const int32_t *perm;
  const int64_t *sel;         // [n] quasars of the batch
  const uint32_t *base;
  const int64_t *base_start;  // [n]
  const double *w;            // [1 + max_dlas][cap][S]
  const int32_t *flag;        // [1 + max_dlas][flag_stride]
  int64_t S, cap, flag_stride;
  int32_t num_lines, n_lo, n_hi;
  int32_t chunks;
  int64_t stride;
  double *part;
};

// The body is spectra_moments_body.hpp, the one k_spectra_moments (spectra_kernels.hpp) includes.
__global__ __launch_bounds__(kMomWaves * 64) void k_spectra_moments_multi(SpectraMomentsMultiArgs a) {
#define GPDLA_SPECTRA_MOMENTS_MULTI 1
#include "spectra_moments_body.hpp"
#undef GPDLA_SPECTRA_MOMENTS_MULTI
}

// ------------------------------------------------------------------------------------------
// k_spectra_model_average: one block per entry.  With P = (P_null, P_lls, P_1 .. P_md) the entry's model
// weights and mb_m(p) = Sum w b, m2_m(p) = Sum w b^2 of model m (its chunks in chunk order, as
// k_spectra_combine adds them):
//   Eb = P_lls mb_lls + Sum_n P_n mb_n,  Eb2 = P_lls m2_lls + Sum_n P_n m2_n   (sub-DLA, DLA(1), .., DLA(md))
//   expected = 1 - Eb,  variance = max(Eb2 - Eb^2, 0)
// The null model absorbs nothing.  A model of weight 0 is skipped, flagged or not; a NaN weight, or a weight
// on a flagged model, leaves the entry's two rows NaN and sets kSpectraAverageUndefined in its status.
// ------------------------------------------------------------------------------------------
constexpr int32_t kSpectraAverageUndefined = 8;  // GPDLA_SPECTRA_AVERAGE_UNDEFINED

struct SpectraModelAverageArgs {
  const QuasarMeta *meta;
  const int64_t *sel;         // [n]
  const int64_t *out_off;     // [n + 1]
  const int32_t *flag;        // [1 + max_dlas][flag_stride]
  const double *weights;      // [n][2 + max_dlas]
  const double *part;
  int64_t cap, flag_stride;
  int32_t md, chunks;
  int64_t stride;
  double *expected, *expected_var;
  int32_t *status;            // [n]
};

__global__ __launch_bounds__(256) void k_spectra_model_average(SpectraModelAverageArgs a) {
  const int64_t sl = blockIdx.x;
  const QuasarMeta m = a.meta[a.sel[sl]];
  const double *P = a.weights + sl * (2 + a.md);
  bool undefined = P[0] != P[0];
  for (int r = 0; r <= a.md; ++r) {
    const double pr = P[1 + r];
    undefined = undefined || pr != pr || (pr != 0.0 && a.flag[(int64_t)r * a.flag_stride + sl] != 0);
  }
  const bool none = m.status != 0 || undefined;
  double *ex = a.expected + a.out_off[sl], *ev = a.expected_var + a.out_off[sl];
  for (int p = threadIdx.x; p < m.n_u; p += 256) {
    double eb = 0.0, eb2 = 0.0;
    if (!none)
      for (int r = 0; r <= a.md; ++r) {
        const double pr = P[1 + r];
        if (pr == 0.0) continue;
        const double *part = a.part + (((int64_t)r * a.cap + sl) * a.chunks * 2) * a.stride;
        double m1 = 0.0, m2 = 0.0;
        for (int c = 0; c < a.chunks; ++c) {
          m1 += part[(2 * c) * a.stride + p];
          m2 += part[(2 * c + 1) * a.stride + p];
        }
        eb += pr * m1;
        eb2 += pr * m2;
      }
    ex[p] = none ? NAN : 1.0 - eb;
    ev[p] = none ? NAN : fmax(eb2 - eb * eb, 0.0);
  }
  if (threadIdx.x == 0) a.status[sl] = m.status | (m.status == 0 && undefined ? kSpectraAverageUndefined : 0);
}

}  // namespace gpdla
