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
//                   kept slot by slot in the lane's a_ip entries of LDS (as k_mc_contract_multi); a body of its own
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
//   a lane is a sample and a wave a quarter of the tile; the accurate tier by whole waves under __any(near); the
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

__global__ __launch_bounds__(256) void k_pf_pixels(PfPixelsArgs a) {
  constexpr int RT = kPfRowTiles, NS = kPfSamples, PT = kPfPixTile, PPS = PT / (256 / NS), KS = GPDLA_MAX_K + 2;
  static_assert(NS == 64 && PT == 64 && PPS * (256 / NS) == PT, "a lane is a sample, a wave a 16-pixel column tile");
  __shared__ double s_exp[kExpTab];
  __shared__ double s_a[PT * NS];  // a_ip as [pixel][sample]; at the end the lane partials
  __shared__ double s_M[PT * KS];
  __shared__ double s_mu[PT], s_mf[PT], s_w[NS];
  __shared__ int s_ij[kPfCols];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t sl = blockIdx.x / a.tiles;
  const int tile = blockIdx.x - sl * a.tiles;
  const int64_t s = a.s0 + sl;
  const int64_t q = a.sel[s];
  const QuasarMeta m = a.meta[q];
  const int p0 = tile * PT;
  if (m.status != 0 || a.pm[s] == 0.0 || p0 >= m.n_u) return;  // (the whole block)

  const int k = a.g.model.k, nb = k * (k + 1) / 2, ncol = nb + k;
  const int nbp = (nb + kPfSlab - 1) & ~(kPfSlab - 1), kp = (k + kPfSlab - 1) & ~(kPfSlab - 1);
  const int L = a.num_lines;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;

  for (int e = tid; e < kExpTab; e += 256) s_exp[e] = exp2((double)e * (1.0 / kExpTab));
  for (int e = tid; e < nbp + kp; e += 256) {  // (i, j) in 6 bits each, the doubling bit, the scratch column + 1 (0: a zero column)
    int fi = k + 1, fj = k + 1, dbl = 0, ac = -1;
    if (e < nb) {
      packed_unpack(e, &fi, &fj);
      dbl = fi != fj;
      ac = e;
    } else if (e >= nbp && e - nbp < k) {
      fi = e - nbp;
      fj = k;
      ac = nb + fi;
    }
    s_ij[e] = fi | (fj << 6) | (dbl << 12) | ((ac + 1) << 13);
  }
  for (int e = tid; e < PT * 2; e += 256) s_M[(e >> 1) * KS + k + (e & 1)] = (e & 1) ? 0.0 : 1.0;
  model_tile_rows(a.g, lam + 3, a.z_qsos[q], m.n_u, p0, PT, s_M, KS, s_mu, s_mf, tid);
  __syncthreads();

  const int r = lane >> 4, c = lane & 15;
  const int smp = tid % NS, sub = tid / NS;
  const int myp = p0 + wave * 16 + c;  // this lane's pixel in the accumulator layout
  const bool pin = myp < m.n_u;
  PixelRow prow = {0.0, 0.0, 0.0, 0.0};
  if (pin) prow = a.pix[m.pix_off + myp];
  const double mu_p = s_mu[wave * 16 + c];
  const double *Mrow = s_M + (wave * 16 + c) * KS;
  const double *rows = a.scratch + (sl * a.S) * (int64_t)ncol;
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double cs = c_light * inv_s;
  const double t0 = g_lines.taps[0], t1 = g_lines.taps[1], t2 = g_lines.taps[2], t3 = g_lines.taps[3],
               t4 = g_lines.taps[4], t5 = g_lines.taps[5], t6 = g_lines.taps[6];
  double F1 = 0.0, F2 = 0.0, FW = 0.0, FD = 0.0;

  const int nlive = a.count[sl];
  const int32_t *list = a.list + sl * a.S;
  const int nchunks = (nlive + NS - 1) / NS;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const int idx = chunk * NS + smp;
    const bool live = idx < nlive;
    const int64_t i = a.perm[list[live ? idx : 0]];
    const double wgt = live ? a.w[s * a.S + i] : 0.0;
    __syncthreads();  // (the previous chunk's epilogue has read s_a and s_w)

    const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[i];
    double mult[3], ms[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      mult[j] = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z_dla)) / 1e8;  // voigt.c:278-279
      ms[j] = mult[j] * inv_s;
    }
    const double inv_opz = 1.0 / (1 + z_dla);
    const double nscale = -a.nhi[i] * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
    auto raw = [&](int P) -> double {  // voigt.c:282-291 for this thread's sample at padded pixel P (as k_mc_contract)
      const double lamP = lam[min(P, n_pad - 1)];
      double total;
      bool near = false;
      if (L == 3) total = wing_sum3(lamP, ms[0], ms[1], ms[2], cs, &near);
      else total = wing_sum_runtime(lamP * inv_opz, cs, L, &near);
      if (__any(near)) {  // accurate tier, wave-uniformly
        if (L == 3) {
          total = 0.0;
          for (int j = 0; j < 3; ++j) {
            const double ax = fabs((lamP * mult[j] - c_light) * inv_s);
            total += ax < 30.0 ? 1.7724538509055159 * g_lines.leading[j] *
                                     near_poly(g_lines.near_poly + j * kNearLineDoubles, ax)
                               : g_lines.cwing[j] * wing_core(ax * ax, g_lines.y2[j]);
          }
        } else {
          total = total_near_at(lamP, 1 + z_dla, L);
        }
      }
      return exp_table_scaled(nscale * total, s_exp);
    };
    const int pp = p0 + sub * PPS;
    double a0 = raw(pp), a1 = raw(pp + 1), a2 = raw(pp + 2), a3 = raw(pp + 3), a4 = raw(pp + 4), a5 = raw(pp + 5), a6;
#pragma unroll 4
    for (int u = 0; u < PPS; ++u) {
      a6 = raw(pp + u + 6);
      double ab = a0 * t0;  // voigt.c:297-299, taps in ascending order
      ab = fma(a1, t1, ab);
      ab = fma(a2, t2, ab);
      ab = fma(a3, t3, ab);
      ab = fma(a4, t4, ab);
      ab = fma(a5, t5, ab);
      ab = fma(a6, t6, ab);
      a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
      s_a[(sub * PPS + u) * NS + smp] = ab;
    }
    if (sub == 0) s_w[smp] = wgt > 0.0 ? wgt : 0.0;
    __syncthreads();

    // contraction: (nbp + kp) / 16 slabs of 4 K-steps.  Within a slab, K-step u takes column 4 r + u of lane group r
    // (A and F alike), so a lane requests four consecutive entries of its sample's row, and the requests of the
    // next slab are issued before the MFMAs of this one: the row is read from global memory at full latency.
    const double *arow[RT];
    mc_d4 accS[RT], accT[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int po = chunk * NS + rt * 16 + c;
      arow[rt] = rows + (int64_t)list[po < nlive ? po : 0] * ncol;
      accS[rt] = mc_d4{0.0, 0.0, 0.0, 0.0};
      accT[rt] = mc_d4{0.0, 0.0, 0.0, 0.0};
    }
    struct Slab {
      double av[4][RT], fv[4];
    };
    auto request = [&](int col0, Slab &sb) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ent = s_ij[col0 + 4 * r + u];
        double f = Mrow[ent & 63] * Mrow[(ent >> 6) & 63];
        if (ent & 4096) f = 2.0 * f;
        sb.fv[u] = f;
        const int ac = (ent >> 13) - 1;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) sb.av[u][rt] = ac >= 0 ? arow[rt][ac] : 0.0;
      }
    };
    const int nslab_s = nbp / kPfSlab, nslab = (nbp + kp) / kPfSlab;
    Slab cur, nxt;
    request(0, cur);
    for (int sb = 0; sb < nslab; ++sb) {
      if (sb + 1 < nslab) request((sb + 1) * kPfSlab, nxt);
      if (sb < nslab_s) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) accS[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.av[u][rt], cur.fv[u], accS[rt], 0, 0, 0);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) accT[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.av[u][rt], cur.fv[u], accT[rt], 0, 0, 0);
      }
      cur = nxt;
    }
    // epilogue
    const double *ap = s_a + (wave * 16 + c) * NS;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int sm = rt * 16 + r + 4 * rr;
        const double wv = s_w[sm];
        if (wv > 0.0) {
          const double ab = ap[sm];
          const double f = ab * (mu_p + accT[rt][rr]);
          const double a2 = ab * ab;
          F1 += wv * f;
          F2 += wv * (f * f);
          FW += wv * (a2 * accS[rt][rr]);
          FD += wv * (a2 * prow.omega2 + prow.nu);
        }
      }
  }
  // the four lanes of a pixel in lane order
  __syncthreads();
  double *red = s_a + ((wave * 4 + r) * 16 + c) * 4;
  red[0] = F1;
  red[1] = F2;
  red[2] = FW;
  red[3] = FD;
  __syncthreads();
  if (r == 0 && pin) {
    double *out = a.sums + (a.out_off[s] + myp) * 4;
    for (int j = 0; j < 4; ++j) {
      double sum = s_a[((wave * 4 + 0) * 16 + c) * 4 + j];
      for (int rr = 1; rr < 4; ++rr) sum += s_a[((wave * 4 + rr) * 16 + c) * 4 + j];
      out[j] = sum;
    }
  }
}

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

__global__ __launch_bounds__(256) void k_pf_pixels_multi(PfPixelsMultiArgs am) {
  const PfPixelsArgs &a = am.p;
  constexpr int RT = kPfRowTiles, NS = kPfSamples, PT = kPfPixTile, PPS = PT / (256 / NS), KS = GPDLA_MAX_K + 2;
  static_assert(NS == 64 && PT == 64 && PPS * (256 / NS) == PT, "a lane is a sample, a wave a 16-pixel column tile");
  __shared__ double s_exp[kExpTab];
  __shared__ double s_a[PT * NS];  // a_ip as [pixel][sample]; at the end the lane partials
  __shared__ double s_M[PT * KS];
  __shared__ double s_mu[PT], s_mf[PT], s_w[NS];
  __shared__ int s_ij[kPfCols];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t sl = blockIdx.x / a.tiles;
  const int tile = blockIdx.x - sl * a.tiles;
  const int64_t s = a.s0 + sl;
  const int64_t q = a.sel[s];
  const QuasarMeta m = a.meta[q];
  const int p0 = tile * PT;
  if (m.status != 0 || a.pm[s] == 0.0 || p0 >= m.n_u) return;  // (the whole block)

  const int k = a.g.model.k, nb = k * (k + 1) / 2, ncol = nb + k;
  const int nbp = (nb + kPfSlab - 1) & ~(kPfSlab - 1), kp = (k + kPfSlab - 1) & ~(kPfSlab - 1);
  const int L = a.num_lines, nslots = am.nslots;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;

  for (int e = tid; e < kExpTab; e += 256) s_exp[e] = exp2((double)e * (1.0 / kExpTab));
  for (int e = tid; e < nbp + kp; e += 256) {  // (i, j) in 6 bits each, the doubling bit, the scratch column + 1 (0: a zero column)
    int fi = k + 1, fj = k + 1, dbl = 0, ac = -1;
    if (e < nb) {
      packed_unpack(e, &fi, &fj);
      dbl = fi != fj;
      ac = e;
    } else if (e >= nbp && e - nbp < k) {
      fi = e - nbp;
      fj = k;
      ac = nb + fi;
    }
    s_ij[e] = fi | (fj << 6) | (dbl << 12) | ((ac + 1) << 13);
  }
  for (int e = tid; e < PT * 2; e += 256) s_M[(e >> 1) * KS + k + (e & 1)] = (e & 1) ? 0.0 : 1.0;
  model_tile_rows(a.g, lam + 3, a.z_qsos[q], m.n_u, p0, PT, s_M, KS, s_mu, s_mf, tid);
  __syncthreads();

  const int r = lane >> 4, c = lane & 15;
  const int smp = tid % NS, sub = tid / NS;
  const int myp = p0 + wave * 16 + c;  // this lane's pixel in the accumulator layout
  const bool pin = myp < m.n_u;
  PixelRow prow = {0.0, 0.0, 0.0, 0.0};
  if (pin) prow = a.pix[m.pix_off + myp];
  const double mu_p = s_mu[wave * 16 + c];
  const double *Mrow = s_M + (wave * 16 + c) * KS;
  const double *rows = a.scratch + (sl * a.S) * (int64_t)ncol;
  const uint32_t *base_q = am.base + am.base_start[s];
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double cs = c_light * inv_s;
  const double t0 = g_lines.taps[0], t1 = g_lines.taps[1], t2 = g_lines.taps[2], t3 = g_lines.taps[3],
               t4 = g_lines.taps[4], t5 = g_lines.taps[5], t6 = g_lines.taps[6];
  double F1 = 0.0, F2 = 0.0, FW = 0.0, FD = 0.0;

  const int nlive = a.count[sl];
  const int32_t *list = a.list + sl * a.S;
  const int nchunks = (nlive + NS - 1) / NS;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const int idx = chunk * NS + smp;
    const bool live = idx < nlive;
    const int64_t i = a.perm[list[live ? idx : 0]];
    const double wgt = live ? a.w[s * a.S + i] : 0.0;
    __syncthreads();  // (the previous chunk's epilogue has read s_a and s_w)

    const int pp = p0 + sub * PPS;
    for (int j = 1; j <= nslots; ++j) {
      int64_t sj = i;  // slot 1: the sample itself
      if (j > 1) {
        const uint32_t b1 = base_q[(int64_t)(j - 2) * a.S + i];
        sj = b1 ? (int64_t)b1 - 1 : i;  // (never drawn: not on the live list; a lane past its end repeats a live sample)
      }
      const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[sj];
      double mult[3], ms[3];
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        mult[l] = g_lines.c / (g_lines.wavelength_cm[l] * (1 + z_dla)) / 1e8;  // voigt.c:278-279
        ms[l] = mult[l] * inv_s;
      }
      const double inv_opz = 1.0 / (1 + z_dla);
      const double nscale = -a.nhi[sj] * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
      auto raw = [&](int P) -> double {  // voigt.c:282-291 for slot j's sample at padded pixel P (as k_pf_pixels)
        const double lamP = lam[min(P, n_pad - 1)];
        double total;
        bool near = false;
        if (L == 3) total = wing_sum3(lamP, ms[0], ms[1], ms[2], cs, &near);
        else total = wing_sum_runtime(lamP * inv_opz, cs, L, &near);
        if (__any(near)) {  // accurate tier, wave-uniformly
          if (L == 3) {
            total = 0.0;
            for (int l = 0; l < 3; ++l) {
              const double ax = fabs((lamP * mult[l] - c_light) * inv_s);
              total += ax < 30.0 ? 1.7724538509055159 * g_lines.leading[l] *
                                       near_poly(g_lines.near_poly + l * kNearLineDoubles, ax)
                                 : g_lines.cwing[l] * wing_core(ax * ax, g_lines.y2[l]);
            }
          } else {
            total = total_near_at(lamP, 1 + z_dla, L);
          }
        }
        return exp_table_scaled(nscale * total, s_exp);
      };
      double a0 = raw(pp), a1 = raw(pp + 1), a2 = raw(pp + 2), a3 = raw(pp + 3), a4 = raw(pp + 4), a5 = raw(pp + 5), a6;
#pragma unroll 4
      for (int u = 0; u < PPS; ++u) {
        a6 = raw(pp + u + 6);
        double ab = a0 * t0;  // voigt.c:297-299, taps in ascending order
        ab = fma(a1, t1, ab);
        ab = fma(a2, t2, ab);
        ab = fma(a3, t3, ab);
        ab = fma(a4, t4, ab);
        ab = fma(a5, t5, ab);
        ab = fma(a6, t6, ab);
        a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
        double *slot = s_a + (sub * PPS + u) * NS + smp;
        *slot = (j == 1) ? ab : *slot * ab;  // multi :342-351, in slot order
      }
    }
    if (sub == 0) s_w[smp] = wgt > 0.0 ? wgt : 0.0;
    __syncthreads();

    // contraction: (nbp + kp) / 16 slabs of 4 K-steps, as k_pf_pixels
    const double *arow[RT];
    mc_d4 accS[RT], accT[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int po = chunk * NS + rt * 16 + c;
      arow[rt] = rows + (int64_t)list[po < nlive ? po : 0] * ncol;
      accS[rt] = mc_d4{0.0, 0.0, 0.0, 0.0};
      accT[rt] = mc_d4{0.0, 0.0, 0.0, 0.0};
    }
    struct Slab {
      double av[4][RT], fv[4];
    };
    auto request = [&](int col0, Slab &sb) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ent = s_ij[col0 + 4 * r + u];
        double f = Mrow[ent & 63] * Mrow[(ent >> 6) & 63];
        if (ent & 4096) f = 2.0 * f;
        sb.fv[u] = f;
        const int ac = (ent >> 13) - 1;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) sb.av[u][rt] = ac >= 0 ? arow[rt][ac] : 0.0;
      }
    };
    const int nslab_s = nbp / kPfSlab, nslab = (nbp + kp) / kPfSlab;
    Slab cur, nxt;
    request(0, cur);
    for (int sb = 0; sb < nslab; ++sb) {
      if (sb + 1 < nslab) request((sb + 1) * kPfSlab, nxt);
      if (sb < nslab_s) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) accS[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.av[u][rt], cur.fv[u], accS[rt], 0, 0, 0);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) accT[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur.av[u][rt], cur.fv[u], accT[rt], 0, 0, 0);
      }
      cur = nxt;
    }
    // epilogue
    const double *ap = s_a + (wave * 16 + c) * NS;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int sm = rt * 16 + r + 4 * rr;
        const double wv = s_w[sm];
        if (wv > 0.0) {
          const double ab = ap[sm];
          const double f = ab * (mu_p + accT[rt][rr]);
          const double a2 = ab * ab;
          F1 += wv * f;
          F2 += wv * (f * f);
          FW += wv * (a2 * accS[rt][rr]);
          FD += wv * (a2 * prow.omega2 + prow.nu);
        }
      }
  }
  // the four lanes of a pixel in lane order
  __syncthreads();
  double *red = s_a + ((wave * 4 + r) * 16 + c) * 4;
  red[0] = F1;
  red[1] = F2;
  red[2] = FW;
  red[3] = FD;
  __syncthreads();
  if (r == 0 && pin) {
    double *out = a.sums + (a.out_off[s] + myp) * 4;
    for (int j = 0; j < 4; ++j) {
      double sum = s_a[((wave * 4 + 0) * 16 + c) * 4 + j];
      for (int rr = 1; rr < 4; ++rr) sum += s_a[((wave * 4 + rr) * 16 + c) * 4 + j];
      out[j] = sum;
    }
  }
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
