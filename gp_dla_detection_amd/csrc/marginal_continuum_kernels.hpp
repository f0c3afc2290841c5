// marginal_continuum_kernels.hpp -- device side of the "marginal continuum" subsystem:
// the GP posterior mean and variance of the low-rank continuum, averaged over the sample table(s) and
// over the models instead of conditioned on one absorber list (k_spectra_continuum).  The
// components of the mixture are the null model and a run-time number of sampled ones: the sub-DLA table and
// DLA(1), .., DLA(max_dlas); the single-DLA entries run it with two (the sub-DLA table, the DLA table).
//
//   k_mc_contract   per (quasar of the launch group, chunk of samples in z_DLA order): the Voigt stage of
//                   k_spectra_moments fused with the contraction of the two per-sample weight vectors
//                   a^2/d and a (y - a mu)/d onto [vech(m_p m_p') | m_p] on v_mfma_f64_16x16x4_f64;
//                   writes [vech(M' diag(a^2/d) M) | M'(a r/d)] per sample to a scratch table
//   k_mc_contract_multi  k_mc_contract for one model DLA(n), n >= 2: sample i absorbs with the product of the n
//                   broadened profiles of its slots (the gather of 4.21), formed by a slot loop INSIDE the tile.  The
//                   two are one text, mc_contract_body.hpp, included under the two names with a switch for the
//                   Voigt stage; the line sum and the tap fold are those of sampled_profile.hpp
//   k_mc_solve      per (quasar, 64 samples): B_i = I + ..., packed Cholesky, L^-1, c_i, Sigma_i =
//                   L^-T L^-1 of every sample of weight > 0, one sample per wave; the block's weighted
//                   partial sums of c_i, Sigma_i and c_i c_i', a not-positive-definite flag, the optional c_i row
//   k_mc_finish     per quasar: the chunk partials in chunk order, the null component (a = 1: the
//                   solve k_spectra_continuum calls, continuum_null_solve of continuum_solve.hpp), the
//                   mixture over (null, sampled components in their order), the coefficient outputs and the
//                   three per-pixel arrays on the unmasked-range grid
//
// Every kernel is handed the pointers of its launch group (the s0 of k_mc_contract is 0): entry sl of the group is
// sel[sl], w[sl], pm[sl], ...
// Every sum runs in a fixed order and nothing is accumulated with atomics: within a wave the samples in
// index order, the four waves in wave order, the chunks in chunk order, the components in component order.
// A block depends on its own (quasar, chunk) only, so outputs are bit-identical
// for any selection order, any launch grouping and either source of the weights.
#pragma once
#include "spectra_multi_kernels.hpp"

namespace gpdla {

constexpr int kMcNb = GPDLA_MAX_K * (GPDLA_MAX_K + 1) / 2;
constexpr int kMcSolveChunk = 64;  // samples (z_DLA positions) per block of k_mc_solve
constexpr int kMixMaxSampled = 1 + GPDLA_POSTERIOR_MAX_MODELS;  // sampled components at most: sub-DLA table, DLA(1) .. DLA(max)

typedef double mc_d4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// k_mc_contract<RT, CPW, PT>: 256 threads, NS = 16 RT samples of one quasar (consecutive in the
// context's z_DLA order), PT pixels a tile.
//   Voigt stage (the arithmetic of k_spectra_moments): thread t takes sample t % NS and the sub-run
//   of PT / (256 / NS) pixels t / NS of the tile; seven raw values in registers, the accurate tier by
//   whole waves (sampled_line_sum).  RT = 4: a lane is a sample and a wave is a quarter of the tile.
//   The two weights of (sample, pixel) go to LDS as the A operands, [pixel][sample].
//   Contraction: D[sample][column] += Sum_p A[sample][p] F[p][column].  The columns are nbt = ceil(nb / 16)
//   tiles of vech(m_p m_p') (weight a^2/d) followed by ceil(k / 16) tiles of m_p (weight a r/d); wave w owns
//   column tiles w, w + 4, ... (CPW of them at most) for all RT row tiles.  The B operand is formed in
//   registers from the tile's Mi rows in LDS, F = M[p][i] M[p][j]; the rows carry a 1 in column k (the
//   m_p tiles: j = k) and a 0 in column k + 1 (padding columns).  Pixels past n_u weigh 0; a masked
//   pixel's Mi row is 0 (k_prepare).
// scratch[((sl * S + pos) * (nb + k)) + column], pos = the sample's position in z_DLA order.
// A block whose samples all weigh exactly 0 (or lie past S) returns at once: k_mc_solve never reads
// their rows.
// ------------------------------------------------------------------------------------------
struct McContractArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *Mi;
  const double *lam_pad;
  const double *offset_samples, *nhi;  // nhi: nhi_samples, or lls_nhi_samples for the sub-DLA table
  const int32_t *perm;
  const int64_t *sel;   // [nsel]; this launch takes sel[s0 .. s0 + nsub)
  const double *w;      // [nsel][S] of this component
  const double *pm;     // [nsel] model weight of this component: 0 = not evaluated
  int64_t S;
  int32_t num_lines, k;
  int64_t s0;
  int32_t chunks;       // ceil(S / NS): blocks per quasar
  double *scratch;
};

// ------------------------------------------------------------------------------------------
// k_mc_contract_multi<RT, CPW, PT>: the decomposition, the contraction and the scratch layout of k_mc_contract.
//   Voigt stage: for slot j = 1 .. nslots (block-uniform: a launch is one model) the lane reads the index of its
//   gathered sample (slot 1: the sample itself; slot j: base[(j - 2) S + i] - 1), forms that sample's multipliers,
//   evaluates the raw values of its sub-run plus the 6 of halo, broadens with the taps in ascending order and
//   multiplies the result into the running product, which lives in the lane's OWN s_wt entries (no barrier between
//   slots, no register per slot).  Each slot takes the accurate tier under its own vote of the wave.  After the last slot
//   the product is turned into (a^2/d, a r/d) in place.
//   A sample that consumes a base index of 0 has weight 0 (k_spectra_weights_multi); its lane gathers ITS OWN
//   sample for that slot, so no index is formed from the 0, and its row is written and never read.
// ------------------------------------------------------------------------------------------
struct McContractMultiArgs {
  McContractArgs c;           // c.w, c.pm: of this model; c.nhi: nhi_samples
  const uint32_t *base;       // base rows of entry s start at base + base_start[s]: [max_dlas - 1][S], 1-based, 0 = never drawn
  const int64_t *base_start;  // [nsel]
  int32_t nslots;             // n of DLA(n), >= 2
};

// The body of both kernels is mc_contract_body.hpp, a header WITHOUT an include guard that is included twice.
template <int RT, int CPW, int PT>
__global__ __launch_bounds__(256) void k_mc_contract(McContractArgs a) {
#define GPDLA_MC_CONTRACT_MULTI 0
#include "mc_contract_body.hpp"
#undef GPDLA_MC_CONTRACT_MULTI
}

template <int RT, int CPW, int PT>
__global__ __launch_bounds__(256) void k_mc_contract_multi(McContractMultiArgs am) {
  const McContractArgs &a = am.c;
#define GPDLA_MC_CONTRACT_MULTI 1
#include "mc_contract_body.hpp"
#undef GPDLA_MC_CONTRACT_MULTI
}

// ------------------------------------------------------------------------------------------
// k_mc_contract_boxed<RT, CPW, PT>: k_mc_contract over the refine points of a refined batch, as
// k_spectra_moments_boxed is k_spectra_moments: c.offset_samples = u, c.nhi = v, c.perm the order of u, c.S = S', c.w the
// weights of the resident lambda rows; z' from the refine's copy of the metadata, N' = exp10(n_lo + (n_hi - n_lo) v) from the
// quasar's last box.  The decomposition, the contraction and the scratch layout are k_mc_contract's, on S' samples.
// ------------------------------------------------------------------------------------------
struct McContractBoxedArgs {
  McContractArgs c;
  const QuasarMeta *rmeta;  // [nq]
  const double *box;        // quasar q's LAST box at box + q * kRefineBoxStride
  const int32_t *rstatus;   // [nq] refine status
};

template <int RT, int CPW, int PT>
__global__ __launch_bounds__(256) void k_mc_contract_boxed(McContractBoxedArgs bx) {
  const McContractArgs &a = bx.c;
#define GPDLA_MC_CONTRACT_MULTI 0
#define GPDLA_MC_CONTRACT_BOXED
#include "mc_contract_body.hpp"
#undef GPDLA_MC_CONTRACT_BOXED
#undef GPDLA_MC_CONTRACT_MULTI
}

// ------------------------------------------------------------------------------------------
// k_mc_solve: 256 threads, the 64 consecutive z_DLA positions `chunk` of one selected quasar.  Wave 0 lists
// the positions of weight > 0 in index order; the four waves take them round robin, a sample per
// wave: L L' = B_i = I + scratch row (column by column, as continuum_null_solve), X = L^-1 (lane c solves
// column c), z = X v, c_i = X' z, Sigma_i = X' X.  A sample of weight exactly 0 is never factorised.
// part[(sl * chunks + chunk) * (k + 2 nb)]: Sum w c_i [k] | Sum w Sigma_i [nb] | Sum w c_i c_i' [nb];
// notpd[sl * chunks + chunk] != 0: a pivot of a sample of weight > 0 was not positive.
// ------------------------------------------------------------------------------------------
struct McSolveArgs {
  const QuasarMeta *meta;
  const int32_t *perm;
  const int64_t *sel;
  const double *w;      // [n][S]
  const double *pm;     // [n]
  int64_t S;
  int32_t k;
  int32_t chunks;       // ceil(S / kMcSolveChunk)
  const double *scratch;
  double *part;
  int32_t *notpd;
  double *sample_coef;  // [n][S][k] in sample order, or nullptr
};

// KEEP (the predictive flux): the sample's scratch row, consumed by then, is overwritten in place
// with [vech(Sigma_i) | c_i], and no partial sums are written (a.part is not read).
template <bool KEEP>
__device__ __forceinline__ void mc_solve_body(const McSolveArgs &a, double *keep) {
  constexpr int kMine = (kMcNb + 63) / 64;
  __shared__ double s_L[4][kMcNb + GPDLA_MAX_K];  // packed L, then v (then c_i)
  __shared__ double s_X[4][kMcNb + GPDLA_MAX_K];  // packed L^-1, then z
  __shared__ int s_live[kMcSolveChunk];
  __shared__ int s_nlive, s_bad;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t sl = blockIdx.x / a.chunks;
  const int chunk = blockIdx.x - sl * a.chunks;
  const QuasarMeta m = a.meta[a.sel[sl]];
  const int k = a.k, nb = k * (k + 1) / 2, ncol = nb + k, plen = k + 2 * nb;
  double *part = KEEP ? nullptr : a.part + (sl * a.chunks + chunk) * (int64_t)plen;
  const bool off = m.status != 0 || a.pm[sl] == 0.0;
  if (wave == 0) {
    const int64_t pos = (int64_t)chunk * kMcSolveChunk + lane;
    const int64_t i = a.perm[pos < a.S ? pos : a.S - 1];
    const bool live = !off && pos < a.S && a.w[sl * a.S + i] > 0.0;
    const unsigned long long mask = __ballot(live);
    if (live) s_live[__popcll(mask & ((1ull << lane) - 1ull))] = (int)(pos - (int64_t)chunk * kMcSolveChunk);
    if (lane == 0) {
      s_nlive = __popcll(mask);
      s_bad = 0;
    }
    if (a.sample_coef && pos < a.S && !live)
      for (int cidx = 0; cidx < k; ++cidx) a.sample_coef[(sl * a.S + i) * k + cidx] = NAN;
  }
  __syncthreads();
  const int nl = s_nlive;
  if (nl == 0) {
    if constexpr (!KEEP)
      for (int e = tid; e < plen; e += 256) part[e] = 0.0;
    if (tid == 0) a.notpd[sl * a.chunks + chunk] = 0;
    return;
  }
  // the packed entries this lane adds up: e = lane + 64 t as (ea, eb), ea >= eb
  int ea[kMine], eb[kMine];
  double accW[kMine], accV[kMine], accC = 0.0;
#pragma unroll
  for (int t = 0; t < kMine; ++t) {
    const int e = lane + 64 * t;
    ea[t] = eb[t] = -1;
    accW[t] = accV[t] = 0.0;
    if (e < nb) packed_unpack(e, &ea[t], &eb[t]);
  }
  double *Lw = s_L[wave], *Xw = s_X[wave];
  double *v = Lw + nb, *z = Xw + nb;
  bool bad = false;
  for (int it = 0; it * 4 < nl; ++it) {
    const int idx = it * 4 + wave;
    const bool has = idx < nl;
    const int64_t pos = (int64_t)chunk * kMcSolveChunk + (has ? s_live[idx] : s_live[0]);
    const int64_t i = a.perm[pos];
    const double wi = a.w[sl * a.S + i];
    const double *row = a.scratch + (sl * a.S + pos) * (int64_t)ncol;
    double *krow = KEEP ? keep + (sl * a.S + pos) * (int64_t)ncol : nullptr;
    if (has) {
#pragma unroll
      for (int t = 0; t < kMine; ++t)
        if (ea[t] >= 0) Lw[lane + 64 * t] = row[lane + 64 * t] + (ea[t] == eb[t] ? 1.0 : 0.0);
      if (lane < k) v[lane] = row[nb + lane];
    }
    for (int j = 0; j < k; ++j) {  // Cholesky of the packed lower triangle, column by column
      __syncthreads();
      if (has) {
        const int rj = j * (j + 1) / 2;
        double sum = Lw[rj + j];
        for (int mm = 0; mm < j; ++mm) sum = fma(-Lw[rj + mm], Lw[rj + mm], sum);
        if (!(sum > 0.0)) bad = true;
        const double ljj = sqrt(sum);
        for (int ii = j + 1 + lane; ii < k; ii += 64) {
          const int ri = ii * (ii + 1) / 2;
          double t = Lw[ri + j];
          for (int mm = 0; mm < j; ++mm) t = fma(-Lw[ri + mm], Lw[rj + mm], t);
          Lw[ri + j] = t / ljj;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) Lw[rj + j] = ljj;
      }
    }
    __syncthreads();
    if (has && lane < k) packed_inverse_column(Lw, Xw, k, lane);  // X = L^-1, a lane per column
    __syncthreads();
    if (has && lane < k) {  // z = X v
      const int ri = lane * (lane + 1) / 2;
      double sum = 0.0;
      for (int mm = 0; mm <= lane; ++mm) sum = fma(Xw[ri + mm], v[mm], sum);
      z[lane] = sum;
    }
    __syncthreads();
    if (has && lane < k) {  // c_i = X' z, over v
      double sum = 0.0;
      for (int ii = lane; ii < k; ++ii) sum = fma(Xw[ii * (ii + 1) / 2 + lane], z[ii], sum);
      v[lane] = sum;
      accC += wi * sum;
      if (a.sample_coef) a.sample_coef[(sl * a.S + i) * k + lane] = sum;
      if constexpr (KEEP) krow[nb + lane] = sum;
    }
    __syncthreads();
    if (has) {
#pragma unroll
      for (int t = 0; t < kMine; ++t) {
        if (ea[t] < 0) continue;
        const double sig = packed_gram_entry(Xw, k, ea[t], eb[t]);  // Sigma_i[ea][eb]
        accW[t] += wi * sig;
        accV[t] += wi * (v[ea[t]] * v[eb[t]]);
        if constexpr (KEEP) krow[lane + 64 * t] = sig;
      }
    }
    __syncthreads();
  }
  if (bad) s_bad = 1;
  if constexpr (KEEP) {
    __syncthreads();
    if (tid == 0) a.notpd[sl * a.chunks + chunk] = s_bad;
    return;
  }
  // the four waves in wave order
#pragma unroll
  for (int t = 0; t < kMine; ++t)
    if (ea[t] >= 0) {
      Lw[lane + 64 * t] = accW[t];
      Xw[lane + 64 * t] = accV[t];
    }
  if (lane < k) v[lane] = accC;
  __syncthreads();
  for (int e = tid; e < plen; e += 256) {
    double sum;
    if (e < k) {
      sum = s_L[0][nb + e];
      for (int wv = 1; wv < 4; ++wv) sum += s_L[wv][nb + e];
    } else if (e < k + nb) {
      sum = s_L[0][e - k];
      for (int wv = 1; wv < 4; ++wv) sum += s_L[wv][e - k];
    } else {
      sum = s_X[0][e - k - nb];
      for (int wv = 1; wv < 4; ++wv) sum += s_X[wv][e - k - nb];
    }
    part[e] = sum;
  }
  if (tid == 0) a.notpd[sl * a.chunks + chunk] = s_bad;
}

__global__ __launch_bounds__(256) void k_mc_solve(McSolveArgs a) { mc_solve_body<false>(a, nullptr); }

// ------------------------------------------------------------------------------------------
// What the two finish kernels share: entry s of a launch group mixes the null component and `sampled` sampled
// components (the single-DLA entries: the sub-DLA table, the DLA table; the multi entries: the sub-DLA table, DLA(1), ..,
// DLA(max_dlas)).  pw[s][1 + sampled] are the normalised model weights; a row with a NaN entry is UNDEFINED (NaN rows,
// kSpectraAverageUndefined; the single-DLA entries refuse such a row).  flag[comp * flag_stride + s] != 0: the
// component's weight row has no weights.  notpd[comp * notpd_stride + s * chunks + ch].
// ------------------------------------------------------------------------------------------
struct MixtureArgs {
  const double *pw;
  const int32_t *flag;
  const int32_t *notpd;
  int64_t flag_stride, notpd_stride;
  int32_t sampled, chunks;
};

__device__ __forceinline__ bool mixture_row_undefined(const double *P, int sampled) {
  bool undefined = false;
  for (int mm = 0; mm <= sampled; ++mm) undefined = undefined || P[mm] != P[mm];
  return undefined;
}

// ------------------------------------------------------------------------------------------
// k_mc_finish: one block per quasar of a launch group; all pointers are the group's: entry s is block s.
//   sampled component m of weight p_m > 0: cbar_m, W_m, S_m = Sum w c c' from
//   the chunk partials in chunk order; the null component of weight p_0 > 0: c_0 from continuum_null_solve with
//   a = 1 (the function k_spectra_continuum calls), Sigma_0 = B_0^-1 through L^-1, S_0 = c_0 c_0';
//   c = Sum p_m cbar_m, W = Sum p_m W_m, V = Sum p_m S_m - c c' in component order.
//   continuum_mean = mu + m_p' c, continuum_var = m_p' (W + V) m_p, continuum_var_between = m_p' V m_p at all n_u
//   pixels, m_p interpolated (and suppressed) by model_tile_rows, in the arithmetic of k_spectra_continuum.  The
//   pixel-diagonal omega term is left out as there.
// status: the quasar's prepare status (1, 3: NaN rows); 4 = some B not positive definite (NaN rows);
// a component of weight > 0 whose weight row has no weights: NaN rows, status 0.
// part[comp * part_stride + (s * chunks + ch) * (k + 2 nb)].
// ------------------------------------------------------------------------------------------
struct McFinishArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *Mi;
  const double *lam_pad;
  const double *z_qsos;
  const int64_t *sel;
  const int64_t *out_off;
  ContinuumModelArgs g;
  MixtureArgs mix;
  const double *part;
  int64_t part_stride;
  double *mean, *var, *var_between;              // flat, out_off
  double *coef_mean, *cov_within, *cov_between;  // [n][k], [n][nb], [n][nb]
  int32_t *status;                               // [n]
};

constexpr int kMcPixTile = 64;

__global__ __launch_bounds__(256) void k_mc_finish(McFinishArgs a) {
  __shared__ double s_B[kMcNb + GPDLA_MAX_K];  // null component: packed B / L, then v (then c_0)
  __shared__ double s_X[kMcNb];                // null component: L^-1
  __shared__ double s_c[GPDLA_MAX_K], s_W[kMcNb], s_V[kMcNb];
  __shared__ double s_wt[kContTile], s_ut[kContTile];
  __shared__ double s_m[kMcPixTile][GPDLA_MAX_K + 1], s_mu[kMcPixTile], s_mf[kMcPixTile];
  __shared__ double s_piv;
  __shared__ int s_pd, s_none;
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t q = a.sel[s];
  const QuasarMeta m = a.meta[q];
  const int k = a.g.model.k, nb = k * (k + 1) / 2, plen = k + 2 * nb;
  const double *P = a.mix.pw + s * (int64_t)(1 + a.mix.sampled);
  double *o_mean = a.mean + a.out_off[s], *o_var = a.var + a.out_off[s], *o_btw = a.var_between + a.out_off[s];
  double *o_c = a.coef_mean + s * k, *o_W = a.cov_within + s * nb, *o_V = a.cov_between + s * nb;
  const bool undefined = m.status == 0 && mixture_row_undefined(P, a.mix.sampled);
  if (m.status != 0 || undefined) {
    for (int p = tid; p < m.n_u; p += 256) o_mean[p] = o_var[p] = o_btw[p] = NAN;
    for (int e = tid; e < nb; e += 256) o_W[e] = o_V[e] = NAN;
    for (int e = tid; e < k; e += 256) o_c[e] = NAN;
    if (tid == 0) a.status[s] = undefined ? kSpectraAverageUndefined : m.status;
    return;
  }
  const double p0 = P[0];
  for (int e = tid; e < nb; e += 256) s_W[e] = s_V[e] = 0.0;
  for (int e = tid; e < k; e += 256) s_c[e] = 0.0;
  if (tid == 0) {
    s_pd = 1;
    s_none = 0;
  }
  __syncthreads();

  if (p0 > 0.0) {  // the null component: a = 1
    continuum_null_solve<kContTile>(a.pix + m.pix_off, a.Mi + m.pix_off * k, m.n_u, k, nullptr, s_B, s_wt, s_ut, &s_piv, &s_pd, tid);
    const double *v = s_B + nb;  // c_0
    if (tid >= 64 && tid < 64 + k) packed_inverse_column(s_B, s_X, k, tid - 64);  // (another wave than the substitution's)
    __syncthreads();
    for (int e = tid; e < nb; e += 256) {
      int ia, ib;
      packed_unpack(e, &ia, &ib);
      s_W[e] += p0 * packed_gram_entry(s_X, k, ia, ib);  // Sigma_0 = B_0^-1
      s_V[e] += p0 * (v[ia] * v[ib]);
    }
    for (int e = tid; e < k; e += 256) s_c[e] += p0 * v[e];
    __syncthreads();
  }

  for (int comp = 0; comp < a.mix.sampled; ++comp) {  // the sampled components in their order
    const double pm = P[1 + comp];
    if (!(pm > 0.0)) continue;
    if (a.mix.flag[comp * a.mix.flag_stride + s] != 0) {
      if (tid == 0) s_none = 1;
      continue;
    }
    const int64_t first = s * a.mix.chunks;
    const int nch = a.mix.chunks;
    const double *part = a.part + comp * a.part_stride;
    for (int e = tid; e < plen; e += 256) {
      double sum = 0.0;
      for (int ch = 0; ch < nch; ++ch) sum += part[(first + ch) * plen + e];
      if (e < k) s_c[e] += pm * sum;
      else if (e < k + nb) s_W[e - k] += pm * sum;
      else s_V[e - k - nb] += pm * sum;
    }
    for (int ch = tid; ch < nch; ch += 256)
      if (a.mix.notpd[comp * a.mix.notpd_stride + first + ch] != 0) s_pd = 0;
  }
  __syncthreads();
  for (int e = tid; e < nb; e += 256) {
    int ia, ib;
    packed_unpack(e, &ia, &ib);
    s_V[e] = s_V[e] - s_c[ia] * s_c[ib];
  }
  __syncthreads();
  const bool ok = s_pd != 0 && s_none == 0;
  for (int e = tid; e < nb; e += 256) {
    o_W[e] = ok ? s_W[e] : NAN;
    o_V[e] = ok ? s_V[e] : NAN;
  }
  for (int e = tid; e < k; e += 256) o_c[e] = ok ? s_c[e] : NAN;
  if (tid == 0) a.status[s] = s_pd ? 0 : 4;

  // the three per-pixel arrays, a tile of model rows at a time
  const double *lam = a.lam_pad + m.lam_off + 3;
  const double z_qso = a.z_qsos[q];
  for (int pt0 = 0; pt0 < m.n_u; pt0 += kMcPixTile) {
    __syncthreads();
    model_tile_rows(a.g, lam, z_qso, m.n_u, pt0, kMcPixTile, &s_m[0][0], GPDLA_MAX_K + 1, s_mu, s_mf, tid);
    __syncthreads();
    if (tid < kMcPixTile && pt0 + tid < m.n_u) {
      const int p = pt0 + tid;
      const double *mp = s_m[tid];
      double val = s_mu[tid];
      for (int cm = 0; cm < k; ++cm) val = fma(mp[cm], s_c[cm], val);
      double qt = 0.0, qb = 0.0;  // m' (W + V) m and m' V m over the packed triangles, row by row
      for (int ia = 0; ia < k; ++ia) {
        const int ra = ia * (ia + 1) / 2;
        double rt = 0.0, rb = 0.0;
        for (int ib = 0; ib < ia; ++ib) {
          rt = fma(s_W[ra + ib] + s_V[ra + ib], mp[ib], rt);
          rb = fma(s_V[ra + ib], mp[ib], rb);
        }
        rt = 2.0 * rt + (s_W[ra + ia] + s_V[ra + ia]) * mp[ia];
        rb = 2.0 * rb + s_V[ra + ia] * mp[ia];
        qt = fma(rt, mp[ia], qt);
        qb = fma(rb, mp[ia], qb);
      }
      o_mean[p] = ok ? val : NAN;
      o_var[p] = ok ? fmax(qt, 0.0) : NAN;
      o_btw[p] = ok ? fmax(qb, 0.0) : NAN;
    }
  }
}

}  // namespace gpdla
