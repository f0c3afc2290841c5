// refine_kernels.hpp -- per-quasar zoom boxes around the posterior mass of (z_DLA, log10 N_HI), re-swept
// on a shared unit-square point set (the contract is in include/gpdla.h, the
// host side in host_refine.hpp, the NumPy restatement in tests/refine_restatement.py).
//
//   k_refine_boxes    one block of 256 threads per selected quasar.  From a source table (the first
//                     pass's l_i with the global offset / log N tables, or the previous level's lambda_j
//                     with the unit points mapped through the previous box): pass 1 the NaN-aware
//                     maximum, pass 2 the extrema of z and log N over A = {l >= max - delta}, passes 3 and 4
//                     the maximum m of the samples strictly outside the new box and their sum of
//                     exp(l - m).  Writes the box, a copy of the quasar's QuasarMeta whose search range is
//                     the box (the batch's own meta is not touched), and the evidence term (m, scaled sum)
//                     of what lies outside.
//   the boxed sweep   k_sweep_slim_boxed<LINES> / k_sweep_split_slim<LINES, 0, BoxedSweepArgs>: the shipped
//                     kernels with one prologue line changed (N = exp10(n_lo + (n_hi - n_lo) v)).
//   k_refine_finish   one block per quasar: lambda_j = l'_j + log p_N(n'_j), its maximum, first argmax
//                     and sum; at the last level the refined evidence and MAP.
//   k_refined_posteriors   one thread per selected quasar: the model posteriors of the first pass's
//                     log_posteriors_no_dla against the refined log_posteriors_dla, by the five operations of
//                     k_evidence's tail; a quasar that was not refined, or is unusable,
//                     gets the first pass's own four numbers.
//
// No atomics.  Minima and maxima are exact in any order; every sum runs in an order fixed by (S, thread
// index) alone (a thread's samples in sample order into a CompSum, then post_block_sum).  Every output is
// a function of its own quasar only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "posterior_kernels.hpp"
#include "sample_kernels.hpp"
#include "sweep_primitives.hpp"  // kRefineMaxLevels, kRefineBoxStride

#pragma clang fp contract(off)

namespace gpdla {

constexpr int kRefineTerms = kRefineMaxLevels + 1;       // evidence terms per quasar: (max, scaled sum) each
constexpr int kRefineScalars = 5;                        // log Z_ref, log posterior, MAP z, MAP log N, MAP index

struct RefineBoxArgs {
  const int32_t *rows;        // [gridDim.x] quasars of the batch
  int32_t level;              // the level whose box is made, 0-based
  int64_t S;                  // samples of the source table
  double sqrt_S;              // sqrt((double)S), rounded by the host
  const double *src;          // [nq][S]: l of the first pass (level 0), lambda of level - 1
  const double *su, *sv;      // [S]: offset_samples and the log N table (level 0), the unit points
  const QuasarMeta *meta;     // the batch's
  double N_lo, N_hi, delta, pad;
  double *box;                // [nq][kRefineBoxStride]
  QuasarMeta *rmeta;          // [nq]
  double *terms;              // [nq][kRefineTerms][2]
  int32_t *status;            // [nq]
};

__device__ inline double refine_block_min(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
}

__global__ __launch_bounds__(256) void k_refine_boxes(RefineBoxArgs a) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int64_t q = a.rows[blockIdx.x];
  const int64_t S = a.S;
  // (only the three fields that are used: a per-thread copy of the whole struct is an array in private memory,
  // which the compiler moves to LDS -- 44 B x 256 threads)
  const int32_t meta_status = a.meta[q].status;
  const double min_z = a.meta[q].min_z_dla, max_z = a.meta[q].max_z_dla;
  const double *row = a.src + q * S;
  double *box = a.box + q * kRefineBoxStride;
  const double inf = __builtin_inf();
  // the parent: the prior's range at level 0, the previous box above
  const double pz_lo = a.level ? box[4 * (a.level - 1) + 0] : min_z;
  const double pz_hi = a.level ? box[4 * (a.level - 1) + 1] : max_z;
  const double pn_lo = a.level ? box[4 * (a.level - 1) + 2] : a.N_lo;
  const double pn_hi = a.level ? box[4 * (a.level - 1) + 3] : a.N_hi;
  const double pdz = pz_hi - pz_lo, pdn = pn_hi - pn_lo;

  double mx = -inf;
  for (int64_t i = tid; i < S; i += 256) {
    const double l = row[i];
    if (l == l) mx = fmax(mx, l);
  }
  mx = post_block_max(mx, red);
  const bool range_ok = min_z <= max_z;   // (false for a NaN end as well)
  const int32_t before = a.level ? a.status[q] : 0;
  if (before != 0 || meta_status != 0 || !range_ok || !(mx > -inf && mx < inf)) {
    if (tid == 0) {
      a.rmeta[q] = a.meta[q];
      a.rmeta[q].status = 1;   // the boxed sweep skips the row
      a.status[q] = before | 1;
    }
    return;
  }

  const double cut = mx - a.delta;
  double z0 = inf, z1 = -inf, n0 = inf, n1 = -inf;
  for (int64_t i = tid; i < S; i += 256) {
    if (row[i] >= cut) {   // NaN never qualifies
      const double z = pz_lo + pdz * a.su[i], n = a.level ? pn_lo + pdn * a.sv[i] : a.sv[i];
      z0 = fmin(z0, z);
      z1 = fmax(z1, z);
      n0 = fmin(n0, n);
      n1 = fmax(n1, n);
    }
  }
  z0 = refine_block_min(z0, red);
  z1 = post_block_max(z1, red);
  n0 = refine_block_min(n0, red);
  n1 = post_block_max(n1, red);
  const double padz = a.pad * pdz / a.sqrt_S, padn = a.pad * pdn / a.sqrt_S;
  const double z_lo = fmax(pz_lo, z0 - padz), z_hi = fmin(pz_hi, z1 + padz);
  const double n_lo = fmax(pn_lo, n0 - padn), n_hi = fmin(pn_hi, n1 + padn);

  // the term's own maximum: the samples outside the box, not the level's.  On a narrow posterior the level's
  // maximum lies inside the box and thousands above everything outside: exp(l - mx) is 0 for every sample the
  // term sums, and a term that is 0 next to its own shift takes Z_ref with it (k_refine_finish).
  double omx = -inf;
  for (int64_t i = tid; i < S; i += 256) {
    const double l = row[i];
    const double z = pz_lo + pdz * a.su[i], n = a.level ? pn_lo + pdn * a.sv[i] : a.sv[i];
    if (l == l && (z < z_lo || z > z_hi || n < n_lo || n > n_hi)) omx = fmax(omx, l);
  }
  omx = post_block_max(omx, red);
  CompSum out;
  if (omx > -inf)   // (else nothing outside, or -inf only: the term is (-inf, 0))
    for (int64_t i = tid; i < S; i += 256) {
      const double l = row[i];
      const double z = pz_lo + pdz * a.su[i], n = a.level ? pn_lo + pdn * a.sv[i] : a.sv[i];
      if (l == l && (z < z_lo || z > z_hi || n < n_lo || n > n_hi)) out.add(exp(l - omx));
    }
  const double sum = post_block_sum(out.value(), red);
  if (tid == 0) {
    box[4 * a.level + 0] = z_lo;
    box[4 * a.level + 1] = z_hi;
    box[4 * a.level + 2] = n_lo;
    box[4 * a.level + 3] = n_hi;
    a.rmeta[q] = a.meta[q];
    a.rmeta[q].min_z_dla = z_lo;
    a.rmeta[q].max_z_dla = z_hi;
    // what the source level holds outside the new box: exp(mx) * scaled is its share of Z_ref
    double scaled = sum / (double)S;
    if (a.level) {
      const double prior_dz = max_z - min_z;
      const double V = prior_dz == 0.0 ? 1.0 : pdz / prior_dz;
      scaled = (V * pdn) * scaled;
    }
    double *t = a.terms + (q * kRefineTerms + a.level) * 2;
    t[0] = omx;
    t[1] = scaled;
    a.status[q] = 0;
  }
}

struct RefineFinishArgs {
  const int32_t *rows;
  int32_t level, last;        // 0-based level just swept; last != 0: finish Z_ref and the MAP
  int64_t S;                  // refine points
  const double *u, *v;        // [S]
  const QuasarMeta *meta;     // the batch's
  const double *box;          // [nq][kRefineBoxStride]
  double *ell, *lam;          // [nq][S]
  int32_t has_prior;
  PriorDev prior;
  double log_uniform;         // log p_N without a prior: -log(N_hi - N_lo), rounded by the host
  double *terms;              // [nq][kRefineTerms][2]
  const double *lp_dla;       // [nq] the batch's log_priors_dla
  double *scal;               // [nq][kRefineScalars]
  int32_t *status;            // [nq]
};

__global__ __launch_bounds__(256) void k_refine_finish(RefineFinishArgs a) {
  __shared__ double red[4];
  __shared__ long long red_arg[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = a.rows[blockIdx.x];
  const int64_t S = a.S;
  double *ell = a.ell + q * S, *lam = a.lam + q * S;
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  if (a.status[q] != 0) {   // not swept: nothing of the row is a result
    for (int64_t j = tid; j < S; j += 256) ell[j] = lam[j] = nan;
    return;
  }
  const double *box = a.box + q * kRefineBoxStride + 4 * a.level;
  const double z_lo = box[0], z_hi = box[1], n_lo = box[2], n_hi = box[3];
  const double dn = n_hi - n_lo;

  double mx = -inf;
  long long arg = S;
  for (int64_t j = tid; j < S; j += 256) {
    const double n = n_lo + dn * a.v[j];
    const double lp = a.has_prior ? log(prior_pdf(a.prior, n)) : a.log_uniform;
    const double l = ell[j] + lp;
    lam[j] = l;
    if (l > mx || (l == mx && j < arg)) {   // NaN compares false; the first j of the largest lambda
      mx = l;
      arg = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(mx, o);
    const long long oa = __shfl_xor(arg, o);
    if (om > mx || (om == mx && oa < arg)) {
      mx = om;
      arg = oa;
    }
  }
  if (lane == 0) {
    red[wave] = mx;
    red_arg[wave] = arg;
  }
  __syncthreads();
  mx = red[0];
  arg = red_arg[0];
  for (int w = 1; w < 4; ++w)
    if (red[w] > mx || (red[w] == mx && red_arg[w] < arg)) {
      mx = red[w];
      arg = red_arg[w];
    }
  __syncthreads();   // (red is reused by the sum)
  if (!(mx > -inf && mx < inf)) {   // no finite lambda, or +inf: the row ends here
    __syncthreads();                // (every thread's lam[] writes are behind the barrier above)
    for (int64_t j = tid; j < S; j += 256) ell[j] = lam[j] = nan;
    if (tid == 0) a.status[q] = 1;
    return;
  }
  if (!a.last) return;

  CompSum acc;
  for (int64_t j = tid; j < S; j += 256) {
    const double l = lam[j];   // this thread's own writes
    if (l == l) acc.add(exp(l - mx));
  }
  const double sum = post_block_sum(acc.value(), red);
  if (tid == 0) {
    const double prior_dz = a.meta[q].max_z_dla - a.meta[q].min_z_dla;
    const double V = prior_dz == 0.0 ? 1.0 : (z_hi - z_lo) / prior_dz;
    double *t = a.terms + q * kRefineTerms * 2;
    t[2 * (a.level + 1) + 0] = mx;
    t[2 * (a.level + 1) + 1] = (V * dn) * (sum / (double)S);
    // Z_ref = Sum_l exp(m_l) s_l over those of the a.level + 2 terms that are not 0, with the one shift M = the
    // largest m_l among them (a term of s_l = 0 -- nothing outside its box, or a box of no volume -- has no say
    // in the shift: exp(m_l - M) may overflow next to its 0)
    double M = -inf;
    for (int l = 0; l <= a.level + 1; ++l)
      if (t[2 * l + 1] > 0.0) M = fmax(M, t[2 * l]);
    double tot = 0.0;
    for (int l = 0; l <= a.level + 1; ++l)
      if (t[2 * l + 1] > 0.0) tot = tot + exp(t[2 * l] - M) * t[2 * l + 1];
    const double log_z = M + log(tot);   // (no term at all: -inf + -inf)
    double *out = a.scal + q * kRefineScalars;
    out[0] = log_z;
    out[1] = a.lp_dla[q] + log_z;
    out[2] = z_lo + (z_hi - z_lo) * a.u[arg];
    out[3] = n_lo + dn * a.v[arg];
    out[4] = (double)(arg + 1);
  }
}

struct RefinedPosteriorArgs {
  int64_t n;                  // selected quasars
  const int64_t *sel;         // [n] quasars of the batch
  const double *summary;      // [nq][kSummaryCols] of the first pass
  const double *scal;         // [nq][kRefineScalars]
  const int32_t *status;      // [nq] refine status
  double *post;               // [n][4]: model posteriors (no DLA, DLA), p_no_dla, p_dla
  int32_t *refined;           // [n]
};

__global__ __launch_bounds__(256) void k_refined_posteriors(RefinedPosteriorArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int64_t q = a.sel[i];
  const double *sm = a.summary + q * kSummaryCols;
  double *out = a.post + 4 * i;
  if (a.status[q] != 0) {   // not refined or unusable: the first pass's columns, so that the table is complete
    for (int c = 0; c < 4; ++c) out[c] = sm[8 + c];
    a.refined[i] = 0;
    return;
  }
  // k_evidence's tail (process_qsos.m:224-233) with the refined log posterior of the DLA model
  const double lp_no = sm[6], lp_dla = a.scal[q * kRefineScalars + 1];
  const double mxp = fmax(lp_no, lp_dla);
  double p0 = exp(lp_no - mxp), p1 = exp(lp_dla - mxp);
  const double tot = p0 + p1;
  p0 /= tot;
  p1 /= tot;
  out[0] = p0;
  out[1] = p1;
  out[2] = p0;
  out[3] = 1 - p0;
  a.refined[i] = 1;
}

}  // namespace gpdla
