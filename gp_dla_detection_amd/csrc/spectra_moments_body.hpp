// spectra_moments_body.hpp -- the body of k_spectra_moments (spectra_kernels.hpp) and of k_spectra_moments_multi
// (spectra_multi_kernels.hpp), which include this file between the braces of the kernel (no include guard) with
// GPDLA_SPECTRA_MOMENTS_MULTI set to 0 or 1; `a` is the kernel's argument struct.  Under the switch stand what the two
// argument structs index differently (the block's entry and model, the weight row, the partial sums), where the sample's
// multipliers are formed and one of the two Voigt stages:
//   0  the sample's own profile: the multipliers once, the seven raw values carried from tile to tile, the 16 weights of
//      the rows a lane adds up in registers
//   1  model DLA(n), n >= 2: the product over the n slots in the lane's own s_out row, slot by slot INSIDE the tile; the
//      multipliers per slot, the six carried raw values recomputed per tile, the weights read from s_w every tile
// The shared memory, the decomposition, the transpose, the reduction and the stores stand once.
// With GPDLA_SPECTRA_MOMENTS_BOXED defined (and the switch at 0) the file is k_spectra_moments_boxed over the refine
// points: `bx` is its SpectraMomentsBoxedArgs and `a` its SpectraMomentsArgs, whose offset_samples, nhi,
// perm and S are the unit points u, v, their order and S'.  Two prologue lines differ: z' takes the range of the refine's
// copy of the quasar's metadata and N' = exp10(n_lo + (n_hi - n_lo) v) the quasar's last box, both in the boxed sweep's
// own expressions (sweep_slim_body.hpp); a quasar without a box returns at once.
  __shared__ double s_exp[kExpTab];
  __shared__ double s_out[kMomWaves][64][kProfTile + 1];
  __shared__ double s_w[kMomWaves][64];
  __shared__ double s_part[2][kMomWaves][2][kProfTile];

  for (int e = threadIdx.x; e < kExpTab; e += kMomWaves * 64) s_exp[e] = exp2((double)e * (1.0 / kExpTab));
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#if GPDLA_SPECTRA_MOMENTS_MULTI
  const int nm = a.n_hi - a.n_lo + 1;
  const int64_t item = blockIdx.x / a.chunks;     // (entry, model)
  const int chunk = (int)(blockIdx.x - item * a.chunks);
  const int64_t sl = item / nm;
  const int n = a.n_lo + (int)(item - sl * nm);
  const QuasarMeta m = a.meta[a.sel[sl]];
  // (the whole block: no sample redshifts, or no weight -- k_spectra_combine writes NaN without reading)
  if (m.status != 0 || a.flag[(int64_t)n * a.flag_stride + sl] != 0) return;
#else
  const int64_t sl = blockIdx.x / a.chunks;       // selected quasar of this launch
  const int chunk = blockIdx.x - sl * a.chunks;
  const int64_t s = a.s0 + sl;
  const QuasarMeta m = a.meta[a.sel[s]];
  if (m.status != 0) return;  // (the whole block: no sample redshifts; k_spectra_combine writes NaN)
#ifdef GPDLA_SPECTRA_MOMENTS_BOXED
  if (bx.rstatus[a.sel[s]] != 0) return;  // (not refined, or unusable: no box; its lambda row is NaN and so are its rows)
#endif
#endif
  const int L = a.num_lines;
  const int64_t pos = (int64_t)chunk * (kMomWaves * 64) + wave * 64 + lane;
  const bool live = pos < a.S;
  const int64_t i = a.perm[live ? pos : a.S - 1];
#if GPDLA_SPECTRA_MOMENTS_MULTI
  s_w[wave][lane] = live ? a.w[((int64_t)n * a.cap + sl) * a.S + i] : 0.0;
#else
  s_w[wave][lane] = live ? a.w[s * a.S + i] : 0.0;
#endif
  __syncthreads();
#if GPDLA_SPECTRA_MOMENTS_MULTI
  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  const double cs = c_light * inv_s;
  const uint32_t *base = a.base + a.base_start[sl] + i;
#else
#ifdef GPDLA_SPECTRA_MOMENTS_BOXED
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
#ifdef GPDLA_SPECTRA_MOMENTS_BOXED
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

  // lane (g, t) adds up rows 4 e + g of pixel t
  const int g = lane >> 4, tt = lane & 15;
#if GPDLA_SPECTRA_MOMENTS_MULTI
  // (their 16 weights stay in s_w, read again every tile: next to n x 22 line sums the 16 LDS reads are nothing, and 32
  // registers are not held across the slot loop)
  double *part = a.part + ((((int64_t)n * a.cap + sl) * a.chunks + chunk) * 2) * a.stride;
#else
  auto raw = [&](int P) -> double {  // this lane's sample at padded pixel P
    const double lamP = lam[min(P, n_pad - 1)];  // wave-uniform address
    return exp_table_scaled(nscale * sampled_line_sum(lamP, mult, ms, cs, inv_opz, z_dla, L), s_exp);
  };
  double wr[16];  // the 16 weights of those rows
#pragma unroll
  for (int e = 0; e < 16; ++e) wr[e] = s_w[wave][4 * e + g];

  double a0 = raw(0), a1 = raw(1), a2 = raw(2), a3 = raw(3), a4 = raw(4), a5 = raw(5), a6;
  double *part = a.part + ((sl * a.chunks + chunk) * 2) * a.stride;
#endif
  int buf = 0;
  for (int p0 = 0; p0 < m.n_u; p0 += kProfTile, buf ^= 1) {
#if GPDLA_SPECTRA_MOMENTS_MULTI
    for (int j = 1; j <= n; ++j) {
      int64_t sj = i;                                 // slot 1: the sample itself
      if (j > 1) {
        const uint32_t b1 = base[(int64_t)(j - 2) * a.S];
        sj = b1 ? (int64_t)b1 - 1 : 0;                // (never drawn: the weight is 0)
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
        const double lamP = lam[min(P, n_pad - 1)];  // wave-uniform address
        return exp_table_scaled(nscale * sampled_line_sum(lamP, mult, ms, cs, inv_opz, z_dla, L), s_exp);
      };
      double a0 = raw(p0), a1 = raw(p0 + 1), a2 = raw(p0 + 2), a3 = raw(p0 + 3), a4 = raw(p0 + 4), a5 = raw(p0 + 5), a6;
#pragma unroll
      for (int u = 0; u < kProfTile; ++u) {
        a6 = raw(p0 + u + 6);
        const double acc = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
        s_out[wave][lane][u] = (j == 1) ? acc : s_out[wave][lane][u] * acc;  // multi :342-351, in slot order
        a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
      }
    }
#else
#pragma unroll
    for (int u = 0; u < kProfTile; ++u) {
      a6 = raw(p0 + u + 6);
      s_out[wave][lane][u] = tap_fold(a0, a1, a2, a3, a4, a5, a6, t0, t1, t2, t3, t4, t5, t6);
      a0 = a1; a1 = a2; a2 = a3; a3 = a4; a4 = a5; a5 = a6;
    }
#endif
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const double b = 1.0 - s_out[wave][4 * e + g][tt];
#if GPDLA_SPECTRA_MOMENTS_MULTI
      const double t = s_w[wave][4 * e + g] * b;
#else
      const double t = wr[e] * b;
#endif
      m1 += t;
      m2 = fma(t, b, m2);
    }
    m1 += __shfl_xor(m1, 16);
    m2 += __shfl_xor(m2, 16);
    m1 += __shfl_xor(m1, 32);
    m2 += __shfl_xor(m2, 32);
    if (lane < kProfTile) {
      s_part[buf][wave][0][lane] = m1;
      s_part[buf][wave][1][lane] = m2;
    }
    // one barrier a tile: s_part is double-buffered (wave 0 reads buffer `buf` of tile t while the
    // other waves can at most be writing buffer `buf ^ 1` of tile t + 1), and it also orders this
    // wave's reads of s_out before its writes of the next tile
    __syncthreads();
    if (threadIdx.x < 2 * kProfTile) {
      const int mom = threadIdx.x >> 4, t = threadIdx.x & 15;
      double sum = s_part[buf][0][mom][t];
#pragma unroll
      for (int w = 1; w < kMomWaves; ++w) sum += s_part[buf][w][mom][t];
      if (p0 + t < m.n_u) part[mom * a.stride + p0 + t] = sum;
    }
  }
