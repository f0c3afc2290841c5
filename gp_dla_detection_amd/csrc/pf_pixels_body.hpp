// pf_pixels_body.hpp -- the body of k_pf_pixels and of k_pf_pixels_multi.  predictive_flux_kernels.hpp includes this file
// between the braces of either kernel (no include guard), as marginal_continuum_kernels.hpp includes
// mc_contract_body.hpp: `a` is the kernel's PfPixelsArgs, and GPDLA_PF_PIXELS_MULTI is 0 (a_ip is the sample's own
// profile) or 1 (model DLA(n), n >= 2: a_ip is the product over the sample's n slots, which `am`, the kernel's
// PfPixelsMultiArgs, lists).  Under the switch stand the head of the slot loop and what is done with a broadened value; the
// tile set-up, the live list, the sample's multipliers, the contraction, the epilogue and the reduction stand once
// (DESIGN.md 4.26).
// With GPDLA_PF_PIXELS_BOXED defined (and the switch at 0) the file is k_pf_pixels_boxed over the refine points
// (DESIGN.md 4.28): `bx` is its PfPixelsBoxedArgs and `a` its PfPixelsArgs, whose offset_samples, nhi, perm and S are the
// unit points u, v, their order and S'.  Two lines of the sample's multipliers differ: z' takes the range of the refine's
// copy of the quasar's metadata and N' = exp10(n_lo + (n_hi - n_lo) v) the quasar's last box, both in the boxed sweep's
// own expressions (sweep_slim_body.hpp); a quasar without a box returns at once.
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
#ifdef GPDLA_PF_PIXELS_BOXED
  if (bx.rstatus[q] != 0) return;  // (not refined, or unusable: no box; the host gives it pm = 0 as well)
  const QuasarMeta rm = bx.rmeta[q];
  const double *box = bx.box + q * kRefineBoxStride;
#endif

  const int k = a.g.model.k, nb = k * (k + 1) / 2, ncol = nb + k;
  const int nbp = (nb + kPfSlab - 1) & ~(kPfSlab - 1), kp = (k + kPfSlab - 1) & ~(kPfSlab - 1);
#if GPDLA_PF_PIXELS_MULTI
  const int L = a.num_lines, nslots = am.nslots;
#else
  const int L = a.num_lines;
#endif
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
#if GPDLA_PF_PIXELS_MULTI
  const uint32_t *base_q = am.base + am.base_start[s];
#endif
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

    // Voigt stage: a_ip of this lane's sample at its sub-run of the tile
#if GPDLA_PF_PIXELS_MULTI
    const int pp = p0 + sub * PPS;
    for (int j = 1; j <= nslots; ++j) {  // the product over the slots, in slot order, in this lane's s_a entries
      int64_t sj = i;  // slot 1: the sample itself
      if (j > 1) {
        const uint32_t b1 = base_q[(int64_t)(j - 2) * a.S + i];
        sj = b1 ? (int64_t)b1 - 1 : i;  // (never drawn: not on the live list; a lane past its end repeats a live sample)
      }
#else
      const int64_t sj = i;  // (no scope of its own: the slot loop's closing brace stands under the switch too)
#endif
#ifdef GPDLA_PF_PIXELS_BOXED
      const double z_dla = rm.min_z_dla + (rm.max_z_dla - rm.min_z_dla) * a.offset_samples[sj];
#else
      const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[sj];
#endif
      double mult[3], ms[3];
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        mult[l] = g_lines.c / (g_lines.wavelength_cm[l] * (1 + z_dla)) / 1e8;  // voigt.c:278-279
        ms[l] = mult[l] * inv_s;
      }
      const double inv_opz = 1.0 / (1 + z_dla);
#ifdef GPDLA_PF_PIXELS_BOXED
      const double nscale = -exp10(box[2] + (box[3] - box[2]) * a.nhi[sj]) * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
#else
      const double nscale = -a.nhi[sj] * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
#endif
      auto raw = [&](int P) -> double {  // sample sj at padded pixel P
        const double lamP = lam[min(P, n_pad - 1)];
        return exp_table_scaled(nscale * sampled_line_sum(lamP, mult, ms, cs, inv_opz, z_dla, L), s_exp);
      };
#if !GPDLA_PF_PIXELS_MULTI
      const int pp = p0 + sub * PPS;  // (where it stood in the written-out kernel: the place decides the prologue's order)
#endif
      double a0 = raw(pp), a1 = raw(pp + 1), a2 = raw(pp + 2), a3 = raw(pp + 3), a4 = raw(pp + 4), a5 = raw(pp + 5), a6;
#pragma unroll 4
      for (int u = 0; u < PPS; ++u) {
        a6 = raw(pp + u + 6);
        const double ab = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
        a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
#if GPDLA_PF_PIXELS_MULTI
        double *slot = s_a + (sub * PPS + u) * NS + smp;
        *slot = (j == 1) ? ab : *slot * ab;  // multi :342-351, in slot order
#else
        s_a[(sub * PPS + u) * NS + smp] = ab;
#endif
      }
#if GPDLA_PF_PIXELS_MULTI
    }
#endif
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
