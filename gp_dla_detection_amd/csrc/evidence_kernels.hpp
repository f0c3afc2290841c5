// evidence_kernels.hpp -- k_evidence (process_qsos.m:203-213, 224-233: log-mean-exp, posteriors) and the stand-alone
// kernels behind gpdla_voigt and gpdla_log_mvnpdf_low_rank.
#pragma once
#include "batch_types.hpp"
#include "faddeeva.hpp"

namespace gpdla {

// ------------------------------------------------------------------------------------------
// k_evidence: one block per quasar.  process_qsos.m:203-213 and :224-233.
// summary row: see GPDLA_SUMMARY_COLS in gpdla.h.
// ------------------------------------------------------------------------------------------
struct EvidenceArgs {
  const QuasarMeta *meta;
  const double *sample_ll;   // [nq][S]
  const double *ll_no_dla;   // [nq]
  const double *log_prior_no_dla, *log_prior_dla;
  const double *offset_samples, *nhi_samples, *log_nhi_samples;  // log_nhi_samples may be null
  int64_t S;
  double *summary;           // [nq][kSummaryCols]
};

__global__ __launch_bounds__(256) void k_evidence(EvidenceArgs a) {
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double sh[4];
  __shared__ long long sh_arg[4];
  const QuasarMeta m = a.meta[q];
  double *out = a.summary + (int64_t)q * kSummaryCols;
  if (m.status != 0) {
    if (tid < kSummaryCols) out[tid] = NAN;
    if (tid == 2) out[2] = a.log_prior_no_dla[q];
    if (tid == 3) out[3] = a.log_prior_dla[q];
    return;
  }
  const double *ll = a.sample_ll + (int64_t)q * a.S;
  double mx = -INFINITY;
  long long arg = a.S;  // first index attaining the nanmax (generate_ascii_catalog.m:73)
  for (int64_t i = tid; i < a.S; i += 256) {
    const double v = ll[i];
    if (v > mx || (v == mx && i < arg)) {  // NaN compares false: skipped like MATLAB's max (:203)
      mx = v;
      arg = i;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double om = __shfl_xor(mx, o);
    const long long oa = __shfl_xor(arg, o);
    if (om > mx || (om == mx && oa < arg)) {
      mx = om;
      arg = oa;
    }
  }
  if (lane == 0) {
    sh[wave] = mx;
    sh_arg[wave] = arg;
  }
  __syncthreads();
  mx = sh[0];
  arg = sh_arg[0];
  for (int w = 1; w < 4; ++w)
    if (sh[w] > mx || (sh[w] == mx && sh_arg[w] < arg)) {
      mx = sh[w];
      arg = sh_arg[w];
    }
  if (arg >= a.S) arg = 0;  // all NaN (or all -inf): MATLAB's nanmax returns index 1
  double sum = 0.0;
  for (int64_t i = tid; i < a.S; i += 256) sum += exp(ll[i] - mx);  // :205-207 (NaN propagates)
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  __syncthreads();
  if (lane == 0) sh[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    sum = sh[0] + sh[1] + sh[2] + sh[3];
    const double ll_dla = mx + log(sum / (double)a.S);                   // :209-210
    const double ll_no = a.ll_no_dla[q];
    const double lp_no = a.log_prior_no_dla[q] + ll_no;                  // :153-154
    const double lp_dla = a.log_prior_dla[q] + ll_dla;                   // :212-213
    const double mxp = fmax(lp_no, lp_dla);                              // :224-225
    double p0 = exp(lp_no - mxp), p1 = exp(lp_dla - mxp);                // :227-228
    const double tot = p0 + p1;
    p0 /= tot;                                                           // :230
    p1 /= tot;
    out[0] = m.min_z_dla;
    out[1] = m.max_z_dla;
    out[2] = a.log_prior_no_dla[q];
    out[3] = a.log_prior_dla[q];
    out[4] = ll_no;
    out[5] = ll_dla;
    out[6] = lp_no;
    out[7] = lp_dla;
    out[8] = p0;
    out[9] = p1;
    out[10] = p0;        // p_no_dlas, :232
    out[11] = 1 - p0;    // p_dlas,    :233
    // generate_ascii_catalog.m:73-80
    out[12] = (double)(arg + 1);
    out[13] = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[arg];
    out[14] = a.log_nhi_samples ? a.log_nhi_samples[arg] : log10(a.nhi_samples[arg]);
  }
}

// ------------------------------------------------------------------------------------------
// Stand-alone surfaces.
// ------------------------------------------------------------------------------------------

// voigt.c:278-292, one thread per padded pixel.
__global__ void k_voigt_raw(const double *lambdas, int64_t n, double z, double N, int num_lines,
                            double *raw) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double total = 0.0;
  for (int j = 0; j < num_lines; ++j) {
    const double mult = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z)) / 1e8;  // voigt.c:279
    const double velocity = lambdas[i] * mult - g_lines.c;                       // voigt.c:287
    const double v = rew_full(velocity * g_lines.inv_sqrt2_sigma, g_lines.y[j]) * g_lines.inv_sqrt2pi_sigma;
    total += -g_lines.leading[j] * v;                                            // voigt.c:288
  }
  raw[i] = exp(N * total);                                                       // voigt.c:291
}

// voigt.c:297-299, one thread per output pixel.
__global__ void k_voigt_broaden(const double *raw, int64_t n_out, double *profile) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  double acc = 0.0;
  for (int kk = 0; kk < 7; ++kk) acc += raw[i + kk] * g_lines.taps[kk];
  profile[i] = acc;
}

// log_mvnpdf_low_rank.m:5-34 for one (y, mu, M, d): a single 256-thread block.
// ws: k(k+1)/2 + k + 2 doubles of workspace.  status: 0 ok, 1 not PD.
__global__ __launch_bounds__(256) void k_lowrank_single(const double *y, const double *mu,
                                                        const double *M, const double *d, int64_t n,
                                                        int k, double *ws, double *log_p,
                                                        int *status) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double sh[4];
  const int nb = k * (k + 1) / 2;
  // B (lower triangle) and v = M' D^-1 (y - mu): one output entry per thread, strided
  for (int e = tid; e < nb + k; e += 256) {
    double acc = 0.0;
    if (e < nb) {
      int i = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while ((i + 1) * (i + 2) / 2 <= e) ++i;
      while (i * (i + 1) / 2 > e) --i;
      const int j = e - i * (i + 1) / 2;
      for (int64_t p = 0; p < n; ++p) acc = fma(M[p + i * n] / d[p], M[p + j * n], acc);
      if (i == j) acc += 1.0;
    } else {
      const int i = e - nb;
      for (int64_t p = 0; p < n; ++p) acc = fma(M[p + i * n], (y[p] - mu[p]) / d[p], acc);
    }
    ws[e] = acc;
  }
  double qs = 0.0, ld = 0.0;
  for (int64_t p = tid; p < n; p += 256) {
    const double r = y[p] - mu[p];
    qs = fma(r, r / d[p], qs);
    ld += log(d[p]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    qs += __shfl_xor(qs, o);
    ld += __shfl_xor(ld, o);
  }
  if (lane == 0) sh[wave] = qs;
  __syncthreads();
  qs = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  if (lane == 0) sh[wave] = ld;
  __syncthreads();
  ld = sh[0] + sh[1] + sh[2] + sh[3];
  __threadfence_block();
  __syncthreads();
  // Cholesky of the packed lower triangle, column by column: the pivot by thread 0, the column
  // below it by all threads (left-looking), then z = L^-1 v (log_mvnpdf_low_rank.m:24-28)
  __shared__ double s_piv;
  __shared__ int s_pd;
  if (tid == 0) s_pd = 1;
  double *v = ws + nb;
  for (int j = 0; j < k; ++j) {
    const int rj = j * (j + 1) / 2;
    __syncthreads();
    if (tid == 0) {
      double sum = ws[rj + j];
      for (int mm = 0; mm < j; ++mm) sum = fma(-ws[rj + mm], ws[rj + mm], sum);
      if (!(sum > 0.0)) s_pd = 0;
      const double ljj = sqrt(sum);
      ws[rj + j] = ljj;
      s_piv = ljj;
    }
    __syncthreads();
    const double ljj = s_piv;
    for (int i = j + 1 + tid; i < k; i += 256) {
      const int ri = i * (i + 1) / 2;
      double sum = ws[ri + j];
      for (int mm = 0; mm < j; ++mm) sum = fma(-ws[ri + mm], ws[rj + mm], sum);
      ws[ri + j] = sum / ljj;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double log_diag = 0.0, zz = 0.0;
    for (int i = 0; i < k; ++i) {
      const int ri = i * (i + 1) / 2;
      log_diag += log(ws[ri + i]);
      double zi = v[i];
      for (int mm = 0; mm < i; ++mm) zi = fma(-ws[ri + mm], v[mm], zi);
      zi /= ws[ri + i];
      v[i] = zi;
      zz = fma(zi, zi, zz);
    }
    const bool pd = s_pd != 0;
    *log_p = pd ? -0.5 * ((qs - zz) + ld + 2 * log_diag + (double)n * kLog2Pi) : NAN;
    *status = pd ? 0 : 1;
  }
}

}  // namespace gpdla
