// multi_kernels.hpp -- device side of the multi-DLA driver
// (multi_dlas/process_qsos_multiple_dlas_meanflux.m, "multi :N" below).
//
// In the multi-DLA models sample i of model nd multiplies nd Voigt profiles: its own and those of
// the samples base_sample_inds(1:nd-1, i) (multi :342-351).  Every profile is a function of one
// sample index alone, so the 2 S distinct profiles of a quasar (S DLA + S sub-DLA column densities,
// multi :365-368) are computed ONCE (k_profiles) into HBM -- 288 GB holds them for hundreds of
// quasars at a time -- and the sweeps of the 1 + max_dlas models gather and multiply them
// (k_sweep_multi_slim, k_sweep_split_slim), feeding the same MFMA contraction and Cholesky epilogue as the
// single-DLA sweep.
//
//   k_profiles        voigt.c:278-299 for every (quasar, DLA|LLS, sample)
//   SweepMultiArgs    multi :340-381   (the parfor body: sweep_multi_slim_kernel.hpp, sweep_split_slim_kernel.hpp;
//                                      on pre-expanded records, superseded_kernels.hpp)
//   k_multi_evidence  multi :386-445   separation mask, nanmax/nanmean evidence, Occam terms, MAP
//   k_multi_resample  multi :467-472   weighted resampling (documented counter-based RNG; the
//                                      reference uses MATLAB's rng('default') + randsample)
//   k_multi_posteriors multi :482-495
#pragma once
#include <type_traits>

#include "sampled_profile.hpp"

namespace gpdla {

// ------------------------------------------------------------------------------------------
// k_profiles: one LANE per sample, BOTH of its profiles (kind 0: the DLA column density, kind 1:
// the sub-DLA one, multi :365-368).  The two share z_DLA and therefore the whole line sum
// Sum_j c_j H(x_j) of voigt.c:282-290 -- only the column density that scales it inside the
// exponential differs (:291) -- so a padded pixel costs one wing / accurate-tier evaluation and two
// exponentials (round 2: one wave per (kind, 64 samples), the line sum taken twice).
// A wave holds 64 samples that are neighbours in z_DLA (perm order) and walks the padded pixels in
// lockstep -- the padded wavelength is a wave-uniform load, the accurate Voigt tier is taken by
// whole waves -- and keeps the seven raw values per kind that the instrument broadening needs
// (voigt.c:297-299) in registers: no cross-lane traffic and no idle lanes (the round-1 form, one
// wave per profile with lanes along the pixels, paid 12 ds_bpermute per value and idled 6 of 64
// lanes).  Outputs are transposed through LDS, 16 pixels at a time, so that every store
// instruction writes whole 128-byte pieces of profile rows.
// prof[((ql * 2 + kind) * S + i) * stride + p], p < stride (>= 4 * steps; entries >= n_u are 1).
// ------------------------------------------------------------------------------------------
struct ProfilesArgs {
  const QuasarMeta *meta;
  const double *lam_pad;
  const double *offset_samples, *nhi_samples, *lls_nhi_samples;
  const int32_t *perm;   // [S] sample indices in ascending offset (= z_DLA) order
  int64_t S;
  int32_t num_lines;
  int64_t q0;        // first quasar of this sub-batch
  int32_t nq_sub;
  int64_t stride;
  double *prof;
};

constexpr int kProfTile = 16;   // pixels per transposed store
constexpr int kProfWaves = 4;   // waves per block (4 x 2 x 64 x 17 doubles of LDS: two blocks per CU)

__global__ __launch_bounds__(kProfWaves * 64) void k_profiles(ProfilesArgs a) {
  __shared__ double s_exp[kExpTab];  // 2^(j/64), the table behind exp_table()
  __shared__ double s_out[kProfWaves][2][64][kProfTile + 1];

  for (int e = threadIdx.x; e < kExpTab; e += kProfWaves * 64) s_exp[e] = exp2((double)e * (1.0 / kExpTab));
  __syncthreads();  // (before any wave may leave)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t wpq = (a.S + 63) / 64;  // waves per quasar
  const int64_t w_global = (int64_t)blockIdx.x * kProfWaves + wave;
  const int64_t ql = w_global / wpq;
  if (ql >= a.nq_sub) return;
  const int64_t pos0 = (w_global - ql * wpq) * 64;
  const QuasarMeta m = a.meta[a.q0 + ql];
  if (m.status != 0) return;
  const int L = a.num_lines;
  const bool live = pos0 + lane < a.S;
  const int64_t i = a.perm[live ? pos0 + lane : a.S - 1];
  const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[i];  // multi :309
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  double mult[3], ms[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    mult[j] = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z_dla)) / 1e8;  // voigt.c:278-279
    ms[j] = mult[j] * inv_s;
  }
  const double cs = c_light * inv_s;
  const double inv_opz = 1.0 / (1 + z_dla);  // (run-time line counts: wing_sum_runtime)
  // (pre-scaled exp, voigt_tiers.hpp)
  const double nscale_a = -a.nhi_samples[i] * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
  const double nscale_b = -a.lls_nhi_samples[i] * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;
  double *rows_a = a.prof + ((ql * 2 + 0) * a.S) * a.stride;  // + i * stride + p
  double *rows_b = a.prof + ((ql * 2 + 1) * a.S) * a.stride;
  const double t0 = g_lines.taps[0], t1 = g_lines.taps[1], t2 = g_lines.taps[2], t3 = g_lines.taps[3],
               t4 = g_lines.taps[4], t5 = g_lines.taps[5], t6 = g_lines.taps[6];

  auto line_sum = [&](int P) -> double {  // voigt.c:282-290 for this lane's z_DLA at padded pixel P
    const double lamP = lam[min(P, n_pad - 1)];  // wave-uniform address
    return sampled_line_sum(lamP, mult, ms, cs, inv_opz, z_dla, L);
  };
  // the two raw profiles at padded pixel P (voigt.c:291)
#define GPDLA_PROF_RAW(P, ra, rb)                          \
  {                                                        \
    const double total_ = line_sum(P);                     \
    ra = exp_table_scaled(nscale_a * total_, s_exp);       \
    rb = exp_table_scaled(nscale_b * total_, s_exp);       \
  }

  // windows of raw values P .. P+6 for output pixel P (the profile of pixel p uses padded p .. p+6)
  double a0, a1, a2, a3, a4, a5, a6, b0, b1, b2, b3, b4, b5, b6;
  GPDLA_PROF_RAW(0, a0, b0);
  GPDLA_PROF_RAW(1, a1, b1);
  GPDLA_PROF_RAW(2, a2, b2);
  GPDLA_PROF_RAW(3, a3, b3);
  GPDLA_PROF_RAW(4, a4, b4);
  GPDLA_PROF_RAW(5, a5, b5);
  const int64_t nrows = min((int64_t)64, a.S - pos0);
  // the 16 profile rows this lane stores into (store instruction e writes rows 4e .. 4e+3): their
  // offsets once, not a perm look-up and a 64-bit multiply per store
  int64_t roff[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int rl = 4 * e + (lane >> 4);
    roff[e] = rl < nrows ? (int64_t)a.perm[pos0 + rl] * a.stride + (lane & 15) : -1;
  }
  for (int p0 = 0; p0 < m.n_u; p0 += kProfTile) {
#pragma unroll
    for (int tt = 0; tt < kProfTile; ++tt) {
      GPDLA_PROF_RAW(p0 + tt + 6, a6, b6);
      s_out[wave][0][lane][tt] = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
      s_out[wave][1][lane][tt] = tap_fold(b0, b1, b2, b3, b4, b5, b6, t0, t1, t2, t3, t4, t5, t6);
      a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
      b0 = b1; b1 = b2; b2 = b3; b3 = b4; b4 = b5; b5 = b6;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // transposed store: instruction e writes pixels p0 .. p0+15 of rows 4e .. 4e+3
    const int tt = lane & 15;
    const bool in_row = p0 + tt < m.n_u;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int rl = 4 * e + (lane >> 4);
      if (roff[e] >= 0 && in_row) {
        // (non-temporal: the table is 15 GB per sub-batch and is next read by another kernel)
        __builtin_nontemporal_store(s_out[wave][0][rl][tt], &rows_a[roff[e] + p0]);
        __builtin_nontemporal_store(s_out[wave][1][rl][tt], &rows_b[roff[e] + p0]);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
#undef GPDLA_PROF_RAW
  // padding behind the pixels: 1 (no absorption)
  for (int64_t rl = 0; rl < nrows; ++rl) {
    const int64_t ir = a.perm[pos0 + rl];
    for (int64_t p = m.n_u + lane; p < a.stride; p += 64) {
      rows_a[ir * a.stride + p] = 1.0;
      rows_b[ir * a.stride + p] = 1.0;
    }
  }
}

struct SweepMultiArgs {
  const QuasarMeta *meta;
  const double *records;
  const double *prof;
  const PixelRow *pix;         // per-pixel pool (k_sweep_multi_split reads rows directly)
  const uint32_t *base_inds;   // [nq][max_dlas-1][S], 1-based (multi :116, :476)
  const int32_t *alive;        // [nq] 0 once an evidence came out NaN (multi :460-464)
  int64_t S, q0, stride;
  int32_t nq_sub, blocks_per_quasar, k, mode, max_dlas;
  double log_S;
  double *sample_ll_dla;       // [nq][max_dlas][S]
  double *sample_ll_lls;       // [nq][S]
  double *ll_no_dla;           // [nq]
};

// ------------------------------------------------------------------------------------------
// Block-wide helpers (256 threads).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double *sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// ------------------------------------------------------------------------------------------
// k_multi_evidence: one block per quasar, for model `nd` (and the LLS model when nd == 1).
// ------------------------------------------------------------------------------------------
struct MultiEvidenceArgs {
  const QuasarMeta *meta;
  const double *offset_samples, *log_nhi_samples;
  const uint32_t *base_inds;
  int32_t *alive;
  int64_t S;
  int32_t nd, max_dlas;
  double min_z_separation, log_S;
  double *sample_ll_dla, *sample_ll_lls;
  double *ll_dla;     // [nq][max_dlas]
  double *ll_lls;     // [nq]
  double *map_z, *map_lognhi, *map_ind;   // [nq][max_dlas][max_dlas]
};

__device__ inline void nan_evidence(const double *ll, int64_t S, double *sh, double *out_max,
                                    double *out_lme, int64_t *out_arg) {
  // nanmax with the FIRST index attaining it, then max + log(nanmean(exp(ll - max)))  (multi :400-408)
  const int tid = threadIdx.x;
  double mx = -INFINITY;
  int64_t arg = S;
  for (int64_t i = tid; i < S; i += 256) {
    const double v = ll[i];
    if (!isnan(v) && (v > mx || (v == mx && i < arg))) {
      mx = v;
      arg = i;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(mx, o);
    const long long oa = __shfl_xor((long long)arg, o);
    if (om > mx || (om == mx && oa < arg)) {
      mx = om;
      arg = oa;
    }
  }
  __shared__ double s_m[4];
  __shared__ long long s_a[4];
  const int wave = tid >> 6, lane = tid & 63;
  __syncthreads();
  if (lane == 0) {
    s_m[wave] = mx;
    s_a[wave] = arg;
  }
  __syncthreads();
  mx = s_m[0];
  arg = s_a[0];
  for (int w = 1; w < 4; ++w)
    if (s_m[w] > mx || (s_m[w] == mx && s_a[w] < arg)) {
      mx = s_m[w];
      arg = s_a[w];
    }
  const bool any = arg < S;
  double sum = 0.0, cnt = 0.0;
  for (int64_t i = tid; i < S; i += 256) {
    const double v = ll[i];
    if (!isnan(v)) {
      sum += exp(v - mx);
      cnt += 1.0;
    }
  }
  sum = block_sum(sum, sh);
  cnt = block_sum(cnt, sh);
  *out_max = any ? mx : NAN;
  *out_lme = any ? mx + log(sum / cnt) : NAN;
  *out_arg = any ? arg : 0;  // MATLAB's nanmax of an all-NaN column returns index 1
}

__global__ __launch_bounds__(256) void k_multi_evidence(MultiEvidenceArgs a) {
  const int q = blockIdx.x, tid = threadIdx.x;
  __shared__ double sh[4];
  const QuasarMeta m = a.meta[q];
  if (m.status != 0 || a.alive[q] == 0) return;
  const int nd = a.nd, md = a.max_dlas;
  double *col = a.sample_ll_dla + ((int64_t)q * md + (nd - 1)) * a.S;
  const uint32_t *base = a.base_inds + (int64_t)q * (md - 1) * a.S;
  const double zr = m.max_z_dla - m.min_z_dla;
  if (nd > 1) {  // multi :386-392: any two absorbers of the sample closer than min_z_separation
    for (int64_t i = tid; i < a.S; i += 256) {
      double zs[4];
      zs[0] = m.min_z_dla + zr * a.offset_samples[i];
      bool close = false;
      for (int j = 1; j < nd; ++j) {
        const int64_t bj = (int64_t)base[(int64_t)(j - 1) * a.S + i] - 1;
        const bool ok = bj >= 0 && bj < a.S;  // undrawn / out-of-range index: the sample is NaN
        close |= !ok;
        zs[j] = m.min_z_dla + zr * a.offset_samples[ok ? bj : i];
      }
      for (int x = 0; x < nd; ++x)
        for (int y = x + 1; y < nd; ++y) close |= fabs(zs[x] - zs[y]) < a.min_z_separation;
      if (close) col[i] = NAN;
    }
    __syncthreads();
  }
  double mx, lme;
  int64_t arg;
  nan_evidence(col, a.S, sh, &mx, &lme, &arg);
  if (tid == 0) {
    const double ev = lme - a.log_S * (nd - 1);  // multi :407-409
    a.ll_dla[(int64_t)q * md + (nd - 1)] = ev;
    // MAP bookkeeping, multi :439-445 ([model][slot], 1-based indices)
    for (int j = 0; j < nd; ++j) {
      const int64_t idx = j == 0 ? arg : (int64_t)base[(int64_t)(j - 1) * a.S + arg] - 1;
      const int64_t at = ((int64_t)q * md + (nd - 1)) * md + j;
      if (idx < 0 || idx >= a.S) continue;  // undrawn index (all-NaN column): slot stays NaN
      a.map_ind[at] = (double)(idx + 1);
      a.map_z[at] = m.min_z_dla + zr * a.offset_samples[idx];
      a.map_lognhi[at] = a.log_nhi_samples[idx];
    }
    if (isnan(ev)) a.alive[q] = 0;  // multi :460-464
  }
  if (nd == 1) {  // multi :416-430
    double mx2, lme2;
    int64_t arg2;
    nan_evidence(a.sample_ll_lls + (int64_t)q * a.S, a.S, sh, &mx2, &lme2, &arg2);
    if (tid == 0) a.ll_lls[q] = lme2;
  }
}

// ------------------------------------------------------------------------------------------
// k_multi_resample: base_sample_inds(nd, :) ~ randsample(S, S, true, W), W = exp(ll - max) with
// NaN -> 0 (multi :467-472).  MATLAB's generator cannot be reproduced; this one is Philox4x32-10
// keyed by (seed, global quasar index) with counter (draw j, model nd), inverse-CDF sampling on the
// prefix sums of W taken in sample order.
// ------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t *out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct MultiResampleArgs {
  const QuasarMeta *meta;
  const int32_t *alive;
  const double *sample_ll_dla;
  int64_t S, first_quasar_index;
  uint64_t seed;
  int32_t nd, max_dlas;
  uint32_t *base_inds;
};

__global__ __launch_bounds__(256) void k_multi_resample(MultiResampleArgs a) {
  extern __shared__ double cdf[];  // [S]
  __shared__ double sh[4];
  __shared__ double s_part[256];
  const int q = blockIdx.x, tid = threadIdx.x;
  const QuasarMeta m = a.meta[q];
  if (m.status != 0 || a.alive[q] == 0) return;
  const double *col = a.sample_ll_dla + ((int64_t)q * a.max_dlas + (a.nd - 1)) * a.S;
  double mx = -INFINITY;
  for (int64_t i = tid; i < a.S; i += 256) {
    const double v = col[i];
    if (!isnan(v)) mx = fmax(mx, v);
  }
  mx = block_reduce_minmax(mx, false, sh);
  // chunked inclusive scan: thread t owns [t*chunk, (t+1)*chunk)
  const int64_t chunk = (a.S + 255) / 256;
  const int64_t lo = (int64_t)tid * chunk, hi = lo + chunk < a.S ? lo + chunk : a.S;
  double run = 0.0;
  for (int64_t i = lo; i < hi; ++i) {
    const double v = col[i];
    run += isnan(v) ? 0.0 : exp(v - mx);
    cdf[i] = run;
  }
  s_part[tid] = run;
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int t = 0; t < 256; ++t) {
      const double v = s_part[t];
      s_part[t] = acc;
      acc += v;
    }
  }
  __syncthreads();
  const double off = s_part[tid];
  for (int64_t i = lo; i < hi; ++i) cdf[i] += off;
  __syncthreads();
  const double total = cdf[a.S - 1];
  const uint64_t qid = (uint64_t)(a.first_quasar_index + q);
  uint32_t *out = a.base_inds + ((int64_t)q * (a.max_dlas - 1) + (a.nd - 1)) * a.S;
  for (int64_t j = tid; j < a.S; j += 256) {
    uint32_t r[4];
    philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), (uint32_t)a.nd, 0u,
                  (uint32_t)(a.seed ^ qid), (uint32_t)((a.seed >> 32) ^ (qid >> 32) ^ 0x5851F42Du), r);
    const double u = ((double)(r[0] >> 5) * 67108864.0 + (double)(r[1] >> 6)) * (1.0 / 9007199254740992.0);
    const double target = u * total;
    int64_t lo2 = 0, hi2 = a.S - 1;  // first index with cdf > target
    while (lo2 < hi2) {
      const int64_t mid = (lo2 + hi2) >> 1;
      if (cdf[mid] > target) hi2 = mid; else lo2 = mid + 1;
    }
    out[j] = (uint32_t)(lo2 + 1);
  }
}

// ------------------------------------------------------------------------------------------
// k_multi_posteriors: multi :300-301, :411-413, :428-430, :482-495.  One thread per quasar.
// post: [nq][2 + max_dlas] = (no DLA, LLS, 1..max_dlas DLAs).
// ------------------------------------------------------------------------------------------
struct MultiPostArgs {
  const QuasarMeta *meta;
  int64_t nq;
  int32_t max_dlas;
  const double *lp_no, *lp_lls, *lp_dla;   // log priors: [nq], [nq], [nq][max_dlas]
  const double *ll_no, *ll_lls, *ll_dla;
  double *lpost_no, *lpost_lls, *lpost_dla, *post, *p_no, *p_lls, *p_dla;
  const double *map_z, *map_lognhi, *map_ind;   // [nq][max_dlas][max_dlas]
  double *summary;   // [nq][14 + 4 md + 3 md^2], layout: GPDLA_SUMMARY_COLS_MULTI in gpdla.h
};

__global__ void k_multi_posteriors(MultiPostArgs a) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.nq) return;
  const int md = a.max_dlas, nm = 2 + md;
  double lp[2 + 8];
  lp[0] = a.lp_no[q] + a.ll_no[q];
  lp[1] = a.lp_lls[q] + a.ll_lls[q];
  for (int j = 0; j < md; ++j) lp[2 + j] = a.lp_dla[q * md + j] + a.ll_dla[q * md + j];
  a.lpost_no[q] = lp[0];
  a.lpost_lls[q] = lp[1];
  for (int j = 0; j < md; ++j) a.lpost_dla[q * md + j] = lp[2 + j];
  double mx = -INFINITY;  // MATLAB max skips NaN (:482-483)
  bool any = false;
  for (int j = 0; j < nm; ++j)
    if (!isnan(lp[j])) {
      mx = fmax(mx, lp[j]);
      any = true;
    }
  if (!any) mx = NAN;
  double e[2 + 8], sum = 0.0;
  for (int j = 0; j < nm; ++j) {
    // :485-488.  lp[j] - mx rounds by up to |lp[j] - mx| 2^-53, which exp() turns into a relative error of that
    // size -- 64 ulp on a posterior of 1e-80.  The rounding error of the difference is recovered exactly (two-sum;
    // the build has no fast-math and no contraction) and applied to first order: exp(d + r) = exp(d) (1 + r).
    const double d = lp[j] - mx, bv = d - lp[j];
    const double r = (lp[j] - (d - bv)) - (mx + bv);
    const double ed = exp(d);
    e[j] = r == r ? ed + ed * r : ed;  // (r is NaN where d is infinite or NaN: keep exp(d))
    sum += e[j];             // NaN entries propagate, as sum() does (:491)
  }
  for (int j = 0; j < nm; ++j) a.post[q * nm + j] = e[j] * (1.0 / sum);
  a.p_no[q] = a.post[q * nm];
  a.p_lls[q] = a.post[q * nm + 1];
  a.p_dla[q] = 1 - a.p_no[q] - a.p_lls[q];  // :493-495
  // the row a multi-GPU run gathers: every saved variable of multi :498-510 that is not per-sample
  const QuasarMeta m = a.meta[q];
  double *o = a.summary + q * (14 + 4 * md + 3 * md * md);
  *o++ = m.min_z_dla;
  *o++ = m.max_z_dla;
  *o++ = a.lp_no[q];
  *o++ = a.lp_lls[q];
  for (int j = 0; j < md; ++j) *o++ = a.lp_dla[q * md + j];
  *o++ = a.ll_no[q];
  *o++ = a.ll_lls[q];
  for (int j = 0; j < md; ++j) *o++ = a.ll_dla[q * md + j];
  *o++ = lp[0];
  *o++ = lp[1];
  for (int j = 0; j < md; ++j) *o++ = lp[2 + j];
  for (int j = 0; j < nm; ++j) *o++ = a.post[q * nm + j];
  *o++ = a.p_no[q];
  *o++ = a.p_lls[q];
  *o++ = a.p_dla[q];
  for (int j = 0; j < md * md; ++j) *o++ = a.map_z[q * md * md + j];
  for (int j = 0; j < md * md; ++j) *o++ = a.map_lognhi[q * md * md + j];
  for (int j = 0; j < md * md; ++j) *o++ = a.map_ind[q * md * md + j];
  *o++ = m.status == 1 ? 1.0 : NAN;  // all_exceptions, multi :139, :232
}

}  // namespace gpdla
