// mixture_multi_kernels.hpp -- device side of the marginal continuum and the posterior predictive flux over ALL
// models of a multi-DLA run: the mixtures of 4.23 and 4.24 with the components
// (null, sub-DLA table, DLA(1), .., DLA(max_dlas)), where sample i of model DLA(n) absorbs with the product of the n
// broadened profiles of its slots (the gather of 4.21, spectra_multi_kernels.hpp).
//
//   k_mc_contract_multi  k_mc_contract with the slot loop INSIDE the tile: the scratch rows [vech(B_i - I) | v_i] of
//                        one model DLA(n), n >= 2.  k_mc_solve, k_pf_solve and k_pf_live run on them as they are.
//   k_pf_pixels_multi    k_pf_pixels with the same slot loop in its Voigt stage
//   k_mc_finish_multi    k_mc_finish over a run-time number of sampled components
//   k_pf_finish_multi    k_pf_finish likewise
//
// The sub-DLA table and model DLA(1) go through k_mc_contract and k_pf_pixels themselves: the kernels here have
// bodies of their own, so that the single-DLA entries keep the code they were measured with.  The weights of
// models n >= 2 are k_spectra_weights_multi's.  Nothing is accumulated with atomics and every sum runs in a fixed
// order: samples in list / index order, waves in wave order, chunks in chunk order, components in component order.
#pragma once
#include "predictive_flux_kernels.hpp"
#include "spectra_multi_kernels.hpp"

namespace gpdla {

constexpr int kMixMaxSampled = 1 + GPDLA_POSTERIOR_MAX_MODELS;  // sub-DLA table, DLA(1) .. DLA(max)

// ------------------------------------------------------------------------------------------
// k_mc_contract_multi<RT, CPW, PT>: the decomposition, the contraction and the scratch layout of k_mc_contract.
//   Voigt stage: for slot j = 1 .. nslots (block-uniform: a launch is one model) the lane reads the index of its
//   gathered sample (slot 1: the sample itself; slot j: base[(j - 2) S + i] - 1), forms that sample's multipliers,
//   evaluates the raw values of its sub-run plus the 6 of halo, broadens with the taps in ascending order and
//   multiplies the result into the running product, which lives in the lane's OWN s_wt entries (no barrier between
//   slots, no register per slot).  Each slot takes the accurate tier under its own __any(near).  After the last slot
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

template <int RT, int CPW, int PT>
__global__ __launch_bounds__(256) void k_mc_contract_multi(McContractMultiArgs am) {
  const McContractArgs &a = am.c;
  constexpr int NS = 16 * RT, NSUB = 256 / NS, PPS = PT / NSUB, KS = GPDLA_MAX_K + 2;
  static_assert(PPS >= 1 && PPS * NSUB == PT && PT % 4 == 0, "tile shape");
  __shared__ double s_exp[kExpTab];
  __shared__ double s_wt[PT * NS], s_ut[PT * NS];
  __shared__ double s_M[PT * KS];
  __shared__ int s_any;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t sl = blockIdx.x / a.chunks;
  const int chunk = blockIdx.x - sl * a.chunks;
  const int64_t s = a.s0 + sl;
  const QuasarMeta m = a.meta[a.sel[s]];
  if (m.status != 0 || a.pm[s] == 0.0) return;  // (the whole block)
  const int smp = tid % NS, sub = tid / NS;
  const int64_t pos = (int64_t)chunk * NS + smp;
  const bool live = pos < a.S;
  const int64_t i = a.perm[pos < a.S ? pos : a.S - 1];
  const double wgt = live ? a.w[s * a.S + i] : 0.0;
  if (tid == 0) s_any = 0;
  for (int e = tid; e < kExpTab; e += 256) s_exp[e] = exp2((double)e * (1.0 / kExpTab));
  __syncthreads();
  if (wgt > 0.0) s_any = 1;
  __syncthreads();
  if (!s_any) return;

  const int k = a.k, nb = k * (k + 1) / 2, ncol = nb + k;
  const int nbt = (nb + 15) / 16, nct = nbt + (k + 15) / 16;
  const int L = a.num_lines, nslots = am.nslots;
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double cs = c_light * inv_s;
  const uint32_t *base = am.base + am.base_start[s] + i;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;
  const double t0 = g_lines.taps[0], t1 = g_lines.taps[1], t2 = g_lines.taps[2], t3 = g_lines.taps[3],
               t4 = g_lines.taps[4], t5 = g_lines.taps[5], t6 = g_lines.taps[6];

  // this lane's B-operand columns: (fi, fj) index the LDS copy of an Mi row, F = row[fi] * row[fj]
  const int r = lane >> 4, c = lane & 15;
  int fi[CPW], fj[CPW], ocol[CPW];
  bool isv[CPW], valid[CPW];
  mc_d4 acc[CPW][RT];
#pragma unroll
  for (int cc = 0; cc < CPW; ++cc) {
    const int ct = wave + 4 * cc;
    fi[cc] = fj[cc] = k + 1;
    ocol[cc] = -1;
    valid[cc] = ct < nct;
    isv[cc] = ct >= nbt;
    if (ct < nbt) {
      const int e = ct * 16 + c;
      if (e < nb) {
        packed_unpack(e, &fi[cc], &fj[cc]);
        ocol[cc] = e;
      }
    } else if (ct < nct) {
      const int iv = (ct - nbt) * 16 + c;
      if (iv < k) {
        fi[cc] = iv;
        fj[cc] = k;
        ocol[cc] = nb + iv;
      }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[cc][rt] = mc_d4{0.0, 0.0, 0.0, 0.0};
  }

  const PixelRow *pix = a.pix + m.pix_off;
  const double *Mi = a.Mi + m.pix_off * k;
  for (int p0 = 0; p0 < m.n_u; p0 += PT) {
    // the Mi rows of the tile, with the 1 and the 0
    for (int e = tid; e < PT * (k + 2); e += 256) {
      const int pl = e / (k + 2), cm = e - pl * (k + 2);
      const int p = p0 + pl;
      double val = cm == k ? 1.0 : 0.0;
      if (cm < k && p < m.n_u) val = Mi[(int64_t)p * k + cm];
      s_M[pl * KS + cm] = val;
    }
    // Voigt stage: the product over the slots, in slot order, in this lane's s_wt entries
    const int pp = p0 + sub * PPS;
    for (int j = 1; j <= nslots; ++j) {
      int64_t sj = i;  // slot 1: the sample itself
      if (j > 1) {
        const uint32_t b1 = base[(int64_t)(j - 2) * a.S];
        sj = b1 ? (int64_t)b1 - 1 : i;  // (never drawn: the weight is 0)
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
      auto raw = [&](int P) -> double {  // voigt.c:282-291 for slot j's sample at padded pixel P (as k_mc_contract)
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
#pragma unroll
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
        double *slot = s_wt + (sub * PPS + u) * NS + smp;
        *slot = (j == 1) ? ab : *slot * ab;  // multi :342-351, in slot order
      }
    }
    // the two weights, in place
#pragma unroll
    for (int u = 0; u < PPS; ++u) {
      const int p = pp + u;
      const double ab = s_wt[(sub * PPS + u) * NS + smp];
      double wt = 0.0, ut = 0.0;
      if (p < m.n_u) {
        const PixelRow row = pix[p];
        const double d = ab * ab * row.omega2 + row.nu;
        const double rr = row.y - ab * row.mu;
        wt = ab * ab / d;
        ut = ab * rr / d;
      }
      s_wt[(sub * PPS + u) * NS + smp] = wt;
      s_ut[(sub * PPS + u) * NS + smp] = ut;
    }
    __syncthreads();
    // contraction: PT / 4 K-steps of 4 pixels
    for (int st = 0; st < PT / 4; ++st) {
      const int pl = 4 * st + r;
      double aw[RT], au[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        aw[rt] = s_wt[pl * NS + rt * 16 + c];
        au[rt] = s_ut[pl * NS + rt * 16 + c];
      }
      const double *Mrow = s_M + pl * KS;
#pragma unroll
      for (int cc = 0; cc < CPW; ++cc) {
        if (!valid[cc]) continue;  // (wave-uniform)
        const double f = Mrow[fi[cc]] * Mrow[fj[cc]];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
          acc[cc][rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(isv[cc] ? au[rt] : aw[rt], f, acc[cc][rt], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // result register rr of row tile rt: sample rt * 16 + (lane >> 4) + 4 rr, column tile's column lane & 15
  double *out = a.scratch + (sl * a.S) * (int64_t)ncol;
#pragma unroll
  for (int cc = 0; cc < CPW; ++cc) {
    if (!valid[cc] || ocol[cc] < 0) continue;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int64_t po = (int64_t)chunk * NS + rt * 16 + r + 4 * rr;
        if (po < a.S) out[po * ncol + ocol[cc]] = acc[cc][rt][rr];
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

// What the two finish kernels share: entry s of a launch group mixes the null component and `sampled` sampled
// components (0: the sub-DLA table, n: DLA(n)).  pw[s][1 + sampled] are the normalised model weights; a row with a NaN
// entry is UNDEFINED (NaN rows, kSpectraAverageUndefined).  flag[comp * flag_stride + s] != 0: the component's
// weight row has no weights.  notpd[comp * notpd_stride + sl * chunks + ch].
struct MixtureMultiArgs {
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
// k_mc_finish_multi: k_mc_finish over the components (null, sub-DLA, DLA(1), .., DLA(max_dlas)), in that order.  All
// pointers are those of the launch group: entry sl of the group is block sl.
// part[comp * part_stride + (sl * chunks + ch) * (k + 2 nb)].
// ------------------------------------------------------------------------------------------
struct McFinishMultiArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *Mi;
  const double *lam_pad;
  const double *z_qsos;
  const int64_t *sel;
  const int64_t *out_off;
  ContinuumModelArgs g;
  MixtureMultiArgs mix;
  const double *part;
  int64_t part_stride;
  double *mean, *var, *var_between;              // flat, out_off
  double *coef_mean, *cov_within, *cov_between;  // [n][k], [n][nb], [n][nb]
  int32_t *status;                               // [n]
};

__global__ __launch_bounds__(256) void k_mc_finish_multi(McFinishMultiArgs a) {
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

  for (int comp = 0; comp < a.mix.sampled; ++comp) {  // the sub-DLA table, then DLA(1), .., DLA(max_dlas)
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

// ------------------------------------------------------------------------------------------
// k_pf_finish_multi: k_pf_finish over the components (null, sub-DLA, DLA(1), .., DLA(max_dlas)), in that order.
// sel, out_off, mix and status are those of the launch group; sums[comp * sums_stride + (out_off[s] + p) * 4 + .] and
// the five outputs are indexed by the selection's own offsets.
// ------------------------------------------------------------------------------------------
struct PfFinishMultiArgs {
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
  MixtureMultiArgs mix;
  const double *sums;
  int64_t sums_stride;
  double *mean, *var, *var_within, *var_between, *noise_var;  // flat, out_off
  int32_t *status;                                            // [n]
};

__global__ __launch_bounds__(256) void k_pf_finish_multi(PfFinishMultiArgs a) {
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
  for (int comp = 0; comp < kMixMaxSampled; ++comp) {  // the sub-DLA table, then DLA(1), .., DLA(max_dlas)
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
