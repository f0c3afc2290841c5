// predictive_flux_kernels.hpp -- device side of the "posterior predictive flux" subsystem:
// per pixel, the mean and variance of the model flux a_i (mu + M c_i), absorption times continuum, over the
// sample table(s) and the models.  It needs the per-pixel cross term of a_i and c_i, which none of the
// products of 4.12, 4.21 and 4.23 carries.
//
//   k_mc_contract(_multi)  (marginal_continuum_kernels.hpp) fills the scratch rows [vech(B_i - I) | v_i]
//   k_pf_solve      the solve of k_mc_solve (one device body, mc_solve_body<KEEP = true>): every sample of
//                   weight > 0 overwrites its scratch row in place with [vech(Sigma_i) | c_i]; a
//                   not-positive-definite flag per block; no partial sums
//   k_pf_live       per selected quasar: the z_DLA positions of weight > 0, compacted in position order (ballots)
//   k_pf_pixels     per (selected quasar, tile of kPfPixTile pixels): walks that live list, kPfSamples at
//                   a time, in list order: the Voigt stage of k_mc_contract gives a_ip, v_mfma_f64_16x16x4_f64 contracts the
//                   scratch rows onto [vech(m_p m_p'), off-diagonal entries doubled | m_p] to give
//                   s_ip = m_p' Sigma_i m_p and m_p' c_i, and the epilogue adds up the four weighted sums
//                   F1 = Sum w f, F2 = Sum w f^2, FW = Sum w a^2 s, FD = Sum w (a^2 omega2 + nu), f = a (mu + m' c)
//   k_pf_pixels_multi  k_pf_pixels for one model DLA(n), n >= 2: a_ip is the product over the sample's n slots,
//                   kept slot by slot in the lane's a_ip entries of LDS (as k_mc_contract_multi); the two are one
//                   text, pf_pixels_body.hpp, included under the two names
//   k_pf_finish     per selected quasar: the null component (a = 1; c_0, Sigma_0 from the solve k_mc_finish
//                   calls, continuum_solve.hpp), the mixture over (null, the sampled components in their order:
//                   MixtureArgs), the NaN and status rules and the five per-pixel arrays
//
// Every kernel is handed the pointers of its launch group (the s0 of k_pf_pixels is 0): entry sl of the group is
// sel[sl], w[sl], out_off[sl], ...
// Nothing is accumulated with atomics and every sum runs in a fixed order: a lane adds its samples in the
// order (list chunk, row tile, result register), the four lanes that share a pixel are added in lane order.  A block
// depends on its own (quasar, pixel tile) only, so outputs are bit-identical for any selection order, any launch
// grouping and either source of the weights.
#pragma once
#include "marginal_continuum_kernels.hpp"

namespace gpdla {

constexpr int kPfRowTiles = 4;                 // RT: 16-sample row tiles of the MFMA a wave carries
constexpr int kPfSamples = 16 * kPfRowTiles;   // entries of the live list a block takes at a time (the packing width)
constexpr int kPfPixTile = 64;                 // pixels per block: one 16-pixel column tile per wave
constexpr int kPfSlab = 16;                   // K-columns a wave requests at a time: 4 K-steps of the MFMA
constexpr int kPfCols = kMcNb + GPDLA_MAX_K + 2 * kPfSlab;  // K-columns: vech padded to a slab, then the k entries likewise

__global__ __launch_bounds__(256) void k_pf_solve(McSolveArgs a, double *keep) { mc_solve_body<true>(a, keep); }

// ------------------------------------------------------------------------------------------
// k_pf_live: one block per selected quasar of a launch group and ONE sampled component.  list[sl * S + j]: the z_DLA
// position of the j-th sample of weight > 0, in position order (a ballot per 256 positions, the counts of the waves
// added in wave order: deterministic); count[sl]: how many there are (0 for a quasar that is not evaluated).
// ------------------------------------------------------------------------------------------
struct PfLiveArgs {
  const QuasarMeta *meta;
  const int32_t *perm;
  const int64_t *sel;
  const double *w;   // [n][S]
  const double *pm;  // [n]
  int64_t S;
  int32_t *list;     // [n][S]
  int32_t *count;    // [n]
};

__global__ __launch_bounds__(256) void k_pf_live(PfLiveArgs a) {
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t sl = blockIdx.x;
  const QuasarMeta m = a.meta[a.sel[sl]];
  const bool off = m.status != 0 || a.pm[sl] == 0.0;
  int done = 0;  // live positions before this stretch (block-uniform)
  for (int64_t t0 = 0; t0 < a.S; t0 += 256) {
    const int64_t pos = t0 + tid;
    const bool live = !off && pos < a.S && a.w[sl * a.S + a.perm[pos < a.S ? pos : a.S - 1]] > 0.0;
    const unsigned long long bal = __ballot(live);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();  // (the previous stretch's s_cnt has been read)
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int wbase = done, total = 0;
    for (int wv = 0; wv < 4; ++wv) {
      if (wv < wave) wbase += s_cnt[wv];
      total += s_cnt[wv];
    }
    done += total;
    if (live) a.list[sl * a.S + wbase + pre] = (int32_t)pos;
  }
  if (tid == 0) a.count[sl] = done;
}

// ------------------------------------------------------------------------------------------
// k_pf_pixels: 256 threads, the pixels p0 = tile * kPfPixTile .. of one selected quasar and ONE sampled component.
//   Tile set-up: mu_p and m_p of the tile from the model (model_tile_rows; not from d_Mi, whose masked rows are 0),
//   the rows with a 1 in column k and a 0 in column k + 1; the K-column table s_ij: column e < nb of the vech part
//   is (i, j, doubled = i != j), padded to a multiple of kPfSlab with (k + 1, k + 1); then column iv < k of the c part
//   is (iv, k), padded likewise.  No slab of 4 K-steps straddles the vech | c boundary or runs past the row.
//   Per chunk of kPfSamples entries of the live list (k_pf_live), in list order; past the end of the list a lane
//   repeats the list's first sample and adds nothing:
//   Voigt stage (the arithmetic of k_mc_contract): thread t takes sample t % 64 and the sub-run of 16 pixels t / 64;
//   a lane is a sample and a wave a quarter of the tile; the accurate tier by whole waves (sampled_line_sum); the
//   same taps in the same order.  a_ip goes to LDS as [pixel][sample].
//   Contraction: D[sample][pixel] += A[sample][col] F[col][pixel]; A is the sample's scratch row, read from
//   global memory (the four waves read the same rows: they meet in L1/L2), F = row[i] row[j] (x 2) formed in
//   registers from the tile's rows in LDS.  Wave w owns the 16 pixels w of the tile for all RT row tiles; the vech
//   columns accumulate s_ip, the c columns m_p' c_i, in separate accumulators.
//   Epilogue in the accumulator layout (register rr of row tile rt: sample rt * 16 + (lane >> 4) + 4 rr, pixel
//   lane & 15): f = a (mu + t) and the four sums; a sample of weight 0 is not added (its a, and its row, may be NaN).
// sums[(out_off[s] + p) * 4 + (F1, F2, FW, FD)] of this component.
// ------------------------------------------------------------------------------------------
struct PfPixelsArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *lam_pad;
  const double *z_qsos;
  const double *offset_samples, *nhi;  // nhi: nhi_samples, or lls_nhi_samples for the sub-DLA table
  const int32_t *perm;
  const int64_t *sel;      // [nsel]; this launch takes sel[s0 .. s0 + nsub)
  const int64_t *out_off;  // [nsel + 1]
  const double *w;         // [nsel][S] of this component
  const double *pm;        // [nsel] model weight of this component: 0 = not evaluated
  ContinuumModelArgs g;
  int64_t S;
  int32_t num_lines;
  int64_t s0;
  int32_t tiles;           // blocks per quasar: ceil(longest grid of the launch / kPfPixTile)
  const double *scratch;   // [nsub][S][nb + k]: vech(Sigma_i) | c_i  (k_pf_solve)
  const int32_t *list;     // [nsub][S], count [nsub]: k_pf_live
  const int32_t *count;
  double *sums;            // [total][4]
};

// ------------------------------------------------------------------------------------------
// k_pf_pixels_multi: k_pf_pixels for one model DLA(n), n >= 2 -- the tile set-up, the live list (of this model),
// the contraction and the epilogue as there; in the Voigt stage a lane is a live sample and the product over its
// slots is kept in its a_ip entries of s_a, slot by slot, as k_mc_contract_multi keeps it in s_wt.
// ------------------------------------------------------------------------------------------
struct PfPixelsMultiArgs {
  PfPixelsArgs p;             // p.w, p.pm, p.list, p.count: of this model; p.nhi: nhi_samples
  const uint32_t *base;
  const int64_t *base_start;  // [nsel]
  int32_t nslots;
};

// The body of both kernels is pf_pixels_body.hpp, a header WITHOUT an include guard that is included twice.
__global__ __launch_bounds__(256) void k_pf_pixels(PfPixelsArgs a) {
#define GPDLA_PF_PIXELS_MULTI 0
#include "pf_pixels_body.hpp"
#undef GPDLA_PF_PIXELS_MULTI
}

__global__ __launch_bounds__(256) void k_pf_pixels_multi(PfPixelsMultiArgs am) {
  const PfPixelsArgs &a = am.p;
#define GPDLA_PF_PIXELS_MULTI 1
#include "pf_pixels_body.hpp"
#undef GPDLA_PF_PIXELS_MULTI
}

// ------------------------------------------------------------------------------------------
// k_pf_pixels_boxed: k_pf_pixels over the refine points of a refined batch, as k_mc_contract_boxed is
// k_mc_contract: p.offset_samples = u, p.nhi = v, p.perm the order of u, p.S = S'; the live list, the scratch rows and the
// weights are those of the S' refined samples.
// ------------------------------------------------------------------------------------------
struct PfPixelsBoxedArgs {
  PfPixelsArgs p;
  const QuasarMeta *rmeta;  // [nq]
  const double *box;        // quasar q's LAST box at box + q * kRefineBoxStride
  const int32_t *rstatus;   // [nq] refine status
};

__global__ __launch_bounds__(256) void k_pf_pixels_boxed(PfPixelsBoxedArgs bx) {
  const PfPixelsArgs &a = bx.p;
#define GPDLA_PF_PIXELS_MULTI 0
#define GPDLA_PF_PIXELS_BOXED
#include "pf_pixels_body.hpp"
#undef GPDLA_PF_PIXELS_BOXED
#undef GPDLA_PF_PIXELS_MULTI
}

// ------------------------------------------------------------------------------------------
// k_pf_finish: one block per selected quasar of a launch group.
//   The null component of weight p_0 > 0: c_0 from continuum_null_solve with a = 1 (the function k_mc_finish and
//   k_spectra_continuum call), Sigma_0 = B_0^-1 through L^-1; per pixel (model_tile_rows) t_0 = mu + m' c_0,
//   s_0 = m' Sigma_0 m, and F1 = t_0, F2 = t_0^2, FW = s_0, FD = omega2 + nu.
//   The mixture in component order (MixtureArgs): flux_mean = Sum p_m F1_m, flux_var_within = Sum p_m FW_m,
//   flux_var_between = max(Sum p_m F2_m - flux_mean^2, 0) (not fused), flux_var = within + between,
//   noise_var = Sum p_m FD_m on kept pixels, NaN on masked ones.
// status: the quasar's prepare status (1, 3: NaN rows); 4 = some B not positive definite (NaN rows);
// a component of weight > 0 whose weight row has no weights: NaN rows, status 0.
// sel, out_off, mix and status are those of the launch group; sums[comp * sums_stride + (out_off[s] + p) * 4 + .] and
// the five outputs are indexed by the selection's own offsets.
// ------------------------------------------------------------------------------------------
struct PfFinishArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *Mi;
  const double *lam_pad;
  const double *z_qsos;
  const int64_t *offsets;      // [nq + 1] upload layout
  const double *wavelengths;   // upload layout
  const uint8_t *pixel_mask;   // upload layout
  double min_lambda, max_lambda;
  const int64_t *sel;
  const int64_t *out_off;
  ContinuumModelArgs g;
  MixtureArgs mix;
  const double *sums;
  int64_t sums_stride;
  double *mean, *var, *var_within, *var_between, *noise_var;  // flat, out_off
  int32_t *status;                                            // [n]
};

__global__ __launch_bounds__(256) void k_pf_finish(PfFinishArgs a) {
  __shared__ double s_B[kMcNb + GPDLA_MAX_K];  // null component: packed B / L, then v (then c_0)
  __shared__ double s_X[kMcNb];                // null component: L^-1
  __shared__ double s_W[kMcNb];                // Sigma_0
  __shared__ double s_wt[kContTile], s_ut[kContTile];
  __shared__ double s_m[kMcPixTile][GPDLA_MAX_K + 1], s_mu[kMcPixTile], s_mf[kMcPixTile];
  __shared__ double s_piv;
  __shared__ int s_pd, s_none, s_cnt[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t s = blockIdx.x;
  const int64_t q = a.sel[s];
  const QuasarMeta m = a.meta[q];
  const int k = a.g.model.k, nb = k * (k + 1) / 2;
  const int64_t o = a.out_off[s];
  const double *P = a.mix.pw + s * (int64_t)(1 + a.mix.sampled);
  const bool undefined = m.status == 0 && mixture_row_undefined(P, a.mix.sampled);
  if (m.status != 0 || undefined) {
    for (int p = tid; p < m.n_u; p += 256)
      a.mean[o + p] = a.var[o + p] = a.var_within[o + p] = a.var_between[o + p] = a.noise_var[o + p] = NAN;
    if (tid == 0) a.status[s] = undefined ? kSpectraAverageUndefined : m.status;
    return;
  }
  const double p0 = P[0];
  if (tid == 0) {
    s_pd = 1;
    s_none = 0;
  }
  __syncthreads();
  const PixelRow *pix = a.pix + m.pix_off;
  const double *v = s_B + nb;  // c_0

  if (p0 > 0.0) {  // the null component: a = 1
    continuum_null_solve<kContTile>(pix, a.Mi + m.pix_off * k, m.n_u, k, nullptr, s_B, s_wt, s_ut, &s_piv, &s_pd, tid);
    if (tid >= 64 && tid < 64 + k) packed_inverse_column(s_B, s_X, k, tid - 64);  // (another wave than the substitution's)
    __syncthreads();
    for (int e = tid; e < nb; e += 256) {
      int ia, ib;
      packed_unpack(e, &ia, &ib);
      s_W[e] = packed_gram_entry(s_X, k, ia, ib);
    }
    __syncthreads();
  }

  double pmv[kMixMaxSampled];
#pragma unroll
  for (int comp = 0; comp < kMixMaxSampled; ++comp) {  // the sampled components in their order
    pmv[comp] = 0.0;
    if (comp >= a.mix.sampled) continue;
    const double pm = P[1 + comp];
    if (!(pm > 0.0)) continue;
    if (a.mix.flag[comp * a.mix.flag_stride + s] != 0) {
      if (tid == 0) s_none = 1;
      continue;
    }
    pmv[comp] = pm;
    for (int ch = tid; ch < a.mix.chunks; ch += 256)
      if (a.mix.notpd[comp * a.mix.notpd_stride + s * a.mix.chunks + ch] != 0) s_pd = 0;
  }
  __syncthreads();
  const bool ok = s_pd != 0 && s_none == 0;
  if (tid == 0) a.status[s] = s_pd ? 0 : 4;

  const double *lam = a.lam_pad + m.lam_off + 3;
  const double z_qso = a.z_qsos[q];
  for (int pt0 = 0; pt0 < m.n_u; pt0 += kMcPixTile) {
    __syncthreads();
    if (p0 > 0.0) model_tile_rows(a.g, lam, z_qso, m.n_u, pt0, kMcPixTile, &s_m[0][0], GPDLA_MAX_K + 1, s_mu, s_mf, tid);
    __syncthreads();
    if (tid < kMcPixTile && pt0 + tid < m.n_u) {
      const int p = pt0 + tid;
      double m1 = 0.0, m2 = 0.0, wi = 0.0, nd = 0.0;
      if (p0 > 0.0) {
        const double *mp = s_m[tid];
        double t = s_mu[tid];
        for (int cm = 0; cm < k; ++cm) t = fma(mp[cm], v[cm], t);
        double qs = 0.0;  // m' Sigma_0 m over the packed triangle, row by row
        for (int ia = 0; ia < k; ++ia) {
          const int ra = ia * (ia + 1) / 2;
          double rt = 0.0;
          for (int ib = 0; ib < ia; ++ib) rt = fma(s_W[ra + ib], mp[ib], rt);
          rt = 2.0 * rt + s_W[ra + ia] * mp[ia];
          qs = fma(rt, mp[ia], qs);
        }
        const PixelRow row = pix[p];
        m1 += p0 * t;
        m2 += p0 * (t * t);
        wi += p0 * qs;
        nd += p0 * (row.omega2 + row.nu);
      }
#pragma unroll
      for (int comp = 0; comp < kMixMaxSampled; ++comp) {
        if (!(pmv[comp] > 0.0)) continue;
        const double *F = a.sums + comp * a.sums_stride + (o + p) * 4;
        m1 += pmv[comp] * F[0];
        m2 += pmv[comp] * F[1];
        wi += pmv[comp] * F[2];
        nd += pmv[comp] * F[3];
      }
      const double sq = m1 * m1;
      const double btw = fmax(m2 - sq, 0.0);
      a.mean[o + p] = ok ? m1 : NAN;
      a.var_within[o + p] = ok ? wi : NAN;
      a.var_between[o + p] = ok ? btw : NAN;
      a.var[o + p] = ok ? wi + btw : NAN;
      a.noise_var[o + p] = ok ? nd : NAN;
    }
  }
  // a masked pixel has no omega2 and nu: the grid position of every stored pixel, counted as k_prepare counts
  __syncthreads();
  const int64_t base = a.offsets[q];
  const int npix = (int)(a.offsets[q + 1] - base);
  int done = 0;
  for (int t0 = 0; t0 < npix; t0 += 256) {
    const int i = t0 + tid;
    bool in_range = false;
    if (i < npix) {
      const double rest = a.wavelengths[base + i] / (1 + z_qso);       // process_qsos.m:102
      in_range = (rest >= a.min_lambda) && (rest <= a.max_lambda);     // :104-105
    }
    const unsigned long long bal = __ballot(in_range);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int wbase = done, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) wbase += s_cnt[w];
      total += s_cnt[w];
    }
    done += total;
    const int u = wbase + pre;
    if (in_range && u < m.n_u && a.pixel_mask[base + i] != 0) a.noise_var[o + u] = NAN;
  }
}

}  // namespace gpdla
