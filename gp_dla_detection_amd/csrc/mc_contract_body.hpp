// mc_contract_body.hpp -- the body of k_mc_contract and of k_mc_contract_multi.  marginal_continuum_kernels.hpp includes
// this file between the braces of either kernel template (no include guard; sweep_slim_kernel.hpp includes
// sweep_slim_body.hpp twice in the same way): `a` is the kernel's McContractArgs, RT, CPW and PT are its template
// parameters, and GPDLA_MC_CONTRACT_MULTI is 0 (a sample absorbs with its own profile) or 1 (model DLA(n), n >= 2: the
// product of the profiles of the sample's n slots, which `am`, the kernel's McContractMultiArgs, lists).  Under the switch
// stand where the per-sample multipliers are formed (once, or per slot) and one of the two Voigt stages; the prologue, the
// column set-up, the Mi tile, the weights, the contraction and the result store stand once.  By inclusion and not as a
// templated device function: that form moved the register allocation of both kernels and ran slower (DESIGN.md
// 4.25 (c)); this one compiles to the instructions of two written-out kernels (4.26).
// With GPDLA_MC_CONTRACT_BOXED defined (and the switch at 0) the file is k_mc_contract_boxed over the refine points
// (DESIGN.md 4.28): `bx` is its McContractBoxedArgs and `a` its McContractArgs, whose offset_samples, nhi, perm and S are
// the unit points u, v, their order and S'.  Two prologue lines differ: z' takes the range of the refine's copy of the
// quasar's metadata and N' = exp10(n_lo + (n_hi - n_lo) v) the quasar's last box, both in the boxed sweep's own
// expressions (sweep_slim_body.hpp); a quasar without a box returns at once.
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
#ifdef GPDLA_MC_CONTRACT_BOXED
  if (bx.rstatus[a.sel[s]] != 0) return;  // (not refined, or unusable: no box; the host gives it pm = 0 as well)
#endif
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
#if GPDLA_MC_CONTRACT_MULTI
  const int L = a.num_lines, nslots = am.nslots;
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double cs = c_light * inv_s;
  const uint32_t *base = am.base + am.base_start[s] + i;
#else
  const int L = a.num_lines;
#ifdef GPDLA_MC_CONTRACT_BOXED
  const QuasarMeta rm = bx.rmeta[a.sel[s]];
  const double z_dla = rm.min_z_dla + (rm.max_z_dla - rm.min_z_dla) * a.offset_samples[i];
#else
  const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[i];
#endif
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  double mult[3], ms[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    mult[j] = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z_dla)) / 1e8;  // voigt.c:278-279
    ms[j] = mult[j] * inv_s;
  }
  const double cs = c_light * inv_s;
  const double inv_opz = 1.0 / (1 + z_dla);
#ifdef GPDLA_MC_CONTRACT_BOXED
  const double *box = bx.box + a.sel[s] * kRefineBoxStride;
  const double nscale = -exp10(box[2] + (box[3] - box[2]) * a.nhi[i]) * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
#else
  const double nscale = -a.nhi[i] * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
#endif
#endif
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
    const int pp = p0 + sub * PPS;
#if GPDLA_MC_CONTRACT_MULTI
    // Voigt stage: the product over the slots, in slot order, in this lane's s_wt entries
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
      auto raw = [&](int P) -> double {  // slot j's sample at padded pixel P
        const double lamP = lam[min(P, n_pad - 1)];
        return exp_table_scaled(nscale * sampled_line_sum(lamP, mult, ms, cs, inv_opz, z_dla, L), s_exp);
      };
      double a0 = raw(pp), a1 = raw(pp + 1), a2 = raw(pp + 2), a3 = raw(pp + 3), a4 = raw(pp + 4), a5 = raw(pp + 5), a6;
#pragma unroll
      for (int u = 0; u < PPS; ++u) {
        a6 = raw(pp + u + 6);
        const double ab = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
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
#else
    // Voigt stage, straight into the two weights
    auto raw = [&](int P) -> double {  // this thread's sample at padded pixel P
      const double lamP = lam[min(P, n_pad - 1)];
      return exp_table_scaled(nscale * sampled_line_sum(lamP, mult, ms, cs, inv_opz, z_dla, L), s_exp);
    };
    double a0 = raw(pp), a1 = raw(pp + 1), a2 = raw(pp + 2), a3 = raw(pp + 3), a4 = raw(pp + 4), a5 = raw(pp + 5), a6;
#pragma unroll
    for (int u = 0; u < PPS; ++u) {
      a6 = raw(pp + u + 6);
      const double ab = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
      a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
      const int p = pp + u;
#endif
      // (either loop goes on:) a^2/d and a r/d of this thread's sample at pixel p
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
