// sweep_slim_body.hpp -- the kernel of sweep_slim_kernel.hpp, which includes this file TWICE inside
// namespace gpdla (no include guard): as k_sweep_slim over SweepArgs, and as k_sweep_slim_boxed over
// BoxedSweepArgs for the refine pass.  GPDLA_SWEEP_SLIM_KERNEL names the kernel and
// GPDLA_SWEEP_SLIM_ARGS its argument struct.  The boxed form differs in one prologue line: nhi_samples
// holds unit coordinates v that are mapped into the quasar's own box of log10 N_HI (offset_samples, perm
// and meta are then the refine points' and the box's).  Two kernel templates of different names rather
// than one with a flag: k_sweep_slim<3> keeps its name, its arguments and its code.
//
// LINES: 3 (set_parameters.m:63, the production value: the three-line wing tier wing_sum3), or 0: the
// line count is a.num_lines, read at run time (voigt.c:16, 266 default to all 31).  The block's 80 KiB of
// LDS are spoken for, so the run-time form keeps no per-sample table of line multipliers: the wing tier
// takes x_j = (lambda / (1 + z_DLA)) kms_j - c / (sqrt2 sigma) with kms_j from constant memory (scalar
// loads; wing_sum_runtime), and the rare near tier forms the reference's own multiplier (voigt.c:278-279) on the spot.
template <int LINES>
__global__ __launch_bounds__(kSlimWaves * 64, 2) void GPDLA_SWEEP_SLIM_KERNEL(GPDLA_SWEEP_SLIM_ARGS a) {
  static_assert(LINES == 3 || LINES == 0, "three lines at compile time, or a run-time count");
  extern __shared__ double smem[];
  constexpr int WAVES = kSlimWaves, CH = kSlimSweepCH;
  const int64_t xj = blockIdx.x >> 3;
  const int64_t pos = 8 * (xj / a.blocks_per_quasar) + (blockIdx.x & 7);
  const int bq = (int)(xj % a.blocks_per_quasar);
  if (pos >= a.nq) return;
  const int64_t q = a.order[pos];  // quasars dealt to the XCDs in order of decreasing length (k_sweep)
  const QuasarMeta m = a.meta[q];
  if (m.status != 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int s = lane & 15, jj = lane >> 4;

  double *ring = smem;                                   // [4][16][33]; pad slot 32 of row j: 2^(j/64)
  double *blocks = ring + kSlimSweepRingD;               // [2 parities]{[4 steps][13 tiles][64], [4 steps][112]}
  double *land = blocks + 2 * kSlimSweepBlock + wave * kSlimLand;  // this wave's landing zone: [4][32] rows twice, [4][4] m16..19
  const double *exp_pad = ring + 32;

  const int64_t slot0 = (int64_t)bq * (WAVES * kSamplesPerWave) + wave * kSamplesPerWave;
  const int64_t slot = slot0 + s;
  const bool is_sample = slot < a.S;
  const bool is_null = !is_sample;  // slot == S is the null model; slots beyond it are idle copies
  // the null-model and idle slots evaluate the LAST sample in z order (a wave that holds them next to real samples
  // holds that one too, or one of equal z), never input sample 0: the accurate Voigt tier is taken by a whole wave
  // when any lane asks for it, so which tier a sample gets must depend on the samples of its wave alone
  const int32_t sample = a.perm[is_sample ? slot : a.S - 1];
  const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[sample];  // process_qsos.m:162-164
  double nhi = a.nhi_samples[sample];
  // (LINES makes the condition dependent: the branch is not instantiated for SweepArgs)
  if constexpr (std::is_same_v<GPDLA_SWEEP_SLIM_ARGS, BoxedSweepArgs> && LINES >= 0) {
    const double *box = sweep_box(a, q);
    nhi = exp10(box[2] + (box[3] - box[2]) * nhi);
  }
  [[maybe_unused]] double mult_r[3];
  [[maybe_unused]] const double opz = 1 + z_dla, inv_opz = 1.0 / opz;
  [[maybe_unused]] const int L = LINES > 0 ? LINES : a.num_lines;
  if constexpr (LINES == 3) {
#pragma unroll
    for (int j = 0; j < 3; ++j) mult_r[j] = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z_dla)) / 1e8;  // voigt.c:278-279
  }
  if (tid < kExpTab) ring[tid * kRing2 + 32] = exp2((double)tid * (1.0 / kExpTab));
  double *my_ring = ring + (size_t)(wave * kSamplesPerWave + s) * kRing2 + jj;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;
  const double nscale64 = -nhi * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
  const double *rec_base = a.records + m.rec_off * (int64_t)kSlimRec;
  const int nchunks = (m.steps + CH - 1) / CH;

  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  // The block's copy of chunk c's raw records (3584 B): wave w brings record w, 896 B, with its lanes 0..55 -- one
  // copy instruction per wave and chunk, and nothing lands behind the parity's raw buffer (the other parity's tiles
  // or the landing zones follow it at once)
  // The source of all three copies is this wave's record of the chunk: a block-uniform address in scalar registers
  // that advances by one chunk per chunk (scalar adds), under lane offsets formed once, here (glds16_at).
  double *const raw_mine = blocks + kSlimSweepTileBuf + wave_s * kSlimRec;
  const double *const my_rec0 = uniform_pointer(rec_base + (size_t)wave_s * kSlimRec);
  constexpr size_t kChunkDoubles = (size_t)CH * kSlimRec;
  uint32_t off_raw = 16u * (uint32_t)lane;
  auto issue_chunk = [&](int parity, const double *my_rec) {  // my_rec: this wave's record of a chunk of that parity
    if (lane < kSlimRec / 2) glds16_at(my_rec, off_raw, raw_mine + parity * kSlimSweepBlock);
  };
  // This wave's private copy of K-step `wave` of a chunk: its 4 M rows, each laid down twice
  // (lane 16 jj + p fetches doubles 2 (p & 7), 2 (p & 7) + 1 of pixel jj's row), and m[16..19] of
  // the 4 pixels (lanes 0..7).
  uint32_t off_rows = 8u * (uint32_t)(4 * kSlimExtras + 16 * jj + 2 * (s & 7));
  uint32_t off_x = 8u * (uint32_t)(kSlimExtras * (lane >> 1) + 4 + 2 * (lane & 1));
  asm volatile("" : "+v"(off_raw), "+v"(off_rows), "+v"(off_x));  // kept in registers, not re-derived per chunk
  auto issue_private = [&](const double *my_rec) {
    glds16_at(my_rec, off_rows, land);
    if (lane < 8) glds16_at(my_rec, off_x, land + 4 * 32);
  };
  // Expansion of this wave's K-step of the chunk that goes to tile buffer P, tiles [t0, t1): the
  // operands are requested by expand_load (early in a K-step) and multiplied and stored by
  // expand_store (late, long after they landed)
  const double *row = land + 32 * jj + s;                  // m[c] at +0, m[(c + n) & 15] at +n
  const double *bc = land + 4 * 32 + 4 * jj;               // m[16 + r] at +r
  // tile 8: lanes c < 8 multiply m[c] m[c + 8]; lanes c >= 8 the pairs (16 + a, 16 + b)
  const double *a8 = s < 8 ? row : bc + (slim_pair_i(8, s) - 16);
  const double *b8 = s < 8 ? row + 8 : bc + (slim_pair_j(8, s) - 16);
  struct Operands {
    double mc, o[5], p8;
  };
  auto expand_load = [&](int t0, int t1, Operands &x) {
    x.mc = row[0];
#pragma unroll
    for (int t = t0; t < t1; ++t) {
      if (t == 8) {
        x.o[t - t0] = a8[0];
        x.p8 = b8[0];
      } else {
        x.o[t - t0] = t == 0 ? x.mc : t < 8 ? row[t] : bc[t - 9];
      }
    }
  };
  auto expand_store = [&](double *dst, int t0, int t1, const Operands &x) {
#pragma unroll
    for (int t = t0; t < t1; ++t) dst[t * 64] = (t == 8 ? x.p8 : x.mc) * x.o[t - t0];
  };
  // an address the compiler must keep in a register instead of re-deriving it in every K-step
  auto pinned = [](const double *p) {
    uint32_t v = lds_address(p);
    asm volatile("" : "+v"(v));
    return (double *)(__attribute__((address_space(3))) double *)(uintptr_t)v;
  };
  // per-lane LDS bases, in registers from here on (a chunk then forms its four parity addresses with one add
  // each): this wave's expansion target in parity 1 -- a chunk expands into the OTHER parity -- and, of parity
  // 0, the tile fragments, this lane's pixel block of a raw record, the u tile of a raw record
  double *const xd1 = pinned(blocks + kSlimSweepBlock + (size_t)wave_s * kSlimStepTiles + lane);
  double *const xd0 = xd1 - kSlimSweepBlock;  // (the priming's target: chunk 0 is parity 0)
  const double *const tb0 = pinned(blocks + lane);
  const double *const mb0 = pinned(blocks + kSlimSweepTileBuf + kSlimExtras * jj);
  const double *const ub0 = pinned(blocks + kSlimSweepTileBuf + 4 * kSlimExtras + lane);

  issue_private(my_rec0);
  issue_chunk(0, my_rec0);

  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  [[maybe_unused]] double ms_r[3];
  if constexpr (LINES == 3) {
#pragma unroll
    for (int j = 0; j < 3; ++j) ms_r[j] = mult_r[j] * inv_s;
  }
  const double cs = c_light * inv_s;
  // sqrt(pi) Sum_j lead_j Re w_j at one padded pixel: voigt.c:282-289
  auto optical_sum = [&](double lamP) -> double {
    if constexpr (LINES == 3) {
      bool near;
      WingLines3 wl;
      double total = wing_sum3(lamP, ms_r[0], ms_r[1], ms_r[2], cs, &near, &wl);
      if (__builtin_expect(__any(near), 0)) total = near_lines3(lamP, mult_r[0], mult_r[1], mult_r[2], wl);
      return total;
    } else {
      bool near;
      double total = wing_sum_runtime(lamP * inv_opz, cs, L, &near);
      if (__builtin_expect(__any(near), 0)) total = total_near_at(lamP, opz, L);
      return total;
    }
  };

  __syncthreads();  // the exp table visible
  // prime the ring with padded pixels 0..11 (the raw profile runs three K-steps ahead)
  for (int c3 = 0; c3 < 3; ++c3) {
    const double lam0 = lam[min(4 * c3 + jj, n_pad - 1)];
    const double tot = optical_sum(lam0);
    const ExpState es0 = exp_ring_begin_scaled(nscale64 * tot, exp_pad);
    const double v = exp_table_end_scaled(es0);
    my_ring[4 * c3] = v;
    my_ring[4 * c3 + 16] = v;
  }

  d4 acc[14];
#pragma unroll
  for (int c = 0; c < 14; ++c) acc[c] = d4{0, 0, 0, 0};
  double quad_sum = 0.0, dprod = 1.0;
  double xw[kXW] = {0.0, 0.0}, xu[kXU] = {0.0, 0.0, 0.0, 0.0};
  int dexp = 0;
  const double tap0 = g_lines.taps[0], tap1 = g_lines.taps[1], tap2 = g_lines.taps[2], tap3 = g_lines.taps[3];

  glds_wait();  // this wave's rows of chunk 0 (and its share of the raw chunk) landed
  {
    const double mc = row[0];
    for (int t = 0; t < kSlimTilesW; ++t)
      xd0[t * 64] = (t == 8 ? b8[0] : mc) * (t == 8 ? a8[0] : t == 0 ? mc : t < 8 ? row[t] : bc[t - 9]);
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the landing zone has been read ...
  if (nchunks > 1) issue_private(my_rec0 + kChunkDoubles);   // ... and may be refilled
  glds_wait();
  __syncthreads();

  // One chunk of 4 K-steps per iteration, from parity c & 1.  While it runs, this wave expands its
  // K-step of chunk c + 1 into the other parity: five tiles in K-step 0, four in each of K-steps 1
  // and 2 (operands requested before the MFMA burst, multiplied and stored behind its 11th MFMA;
  // unconditionally: after the last chunk the products of stale rows land in a buffer nobody reads),
  // and in K-step 3 refills its landing zone for chunk c + 2 -- every read of it has been consumed
  // by a multiply by then, and the 1-KiB copy lands during that K-step's burst, before the chunk's
  // closing barrier.  Measured on the 8-wave block with 8-step chunks this kernel had before, on one
  // box (tools/ab.sh, ms per launch): two tiles per K-step over seven K-steps 149.6; three over five
  // 150.1; products stored before the burst 152.0; without the explicit lgkmcnt(0) at the top of a
  // K-step 153.1; pre-expanded records (k_sweep) 149.5.
  //
  // LDS latency.  Inside a chunk the ring taps and the pixel row of K-step tt + 1 are requested in K-step tt's MFMA
  // burst, after its 11th MFMA (most B fragments are dead by then and three MFMAs, >= 190 cycles, still cover the
  // round trip), carried in n0..n6 / n01, n23 as lam_next is, and consumed behind the lgkmcnt(0) at the top of the
  // next K-step.  The reads stand behind this step's ring write: lanes jj = 2, 3 of step tt + 1 read what step tt
  // writes.  A read for a step that does not exist (rn + 1 == m.steps) fetches valid LDS and is dropped.  The taps
  // are requested across the chunk edge in the same way (the ring is wave-private; chunk 0's behind the priming),
  // which a chunk of 4 steps pays for: 142.3 against 143.1 ms per launch (profiles/ab_half_blocks.txt).  K-step 0
  // of a chunk has its row in the other parity's raw buffer, complete only behind the chunk barrier: it requests
  // wavelength and row itself and runs the part of the wing tier that needs the wavelength alone in front of
  // their first use.  The exp table entry is covered by the series and the weights.  Measurements and the variants
  // that lost: LABBOOK, "Taps and row under the MFMA burst".
  // taps of the next K-step, carried across the chunk barrier too (the ring is this wave's own)
  double n0 = my_ring[0], n1 = my_ring[1], n2 = my_ring[2], n3 = my_ring[3], n4 = my_ring[4], n5 = my_ring[5], n6 = my_ring[6];
  const double *next_rec = my_rec0 + kChunkDoubles;  // this wave's record of chunk c + 1
  // The wavelength and the pixel row of the next K-step live across the chunk loop although K-step 0 reads neither:
  // declared inside a chunk they were set to zero once per chunk, and once more on the path of a K-step that does not run.
  double lam_next = 0.0;
  double2 n01 = {0.0, 0.0}, n23 = {0.0, 0.0};                                    // its pixel row
  // kE3, which the leading Horner step of the wing series takes from a vector register (wing_lead): held in one from
  // here on.  Left to itself the compiler moves it there from a scalar pair in every K-step, behind the v_rcp_f64.
  double e3v = kE3;
  asm volatile("" : "+v"(e3v));
  // One chunk, of the parity given.  A callable, and the parity an argument, on purpose: the same K-step written
  // straight into the loop below has the same vector instructions, but the compiler then interleaves the exp series
  // with the weights less well (137.6 against 136.6 ms per launch; LABBOOK, "Bookkeeping instructions of the K-step").
  auto chunk = [&](const int c, const int parity) __attribute__((always_inline)) {
    // vmcnt(0): nothing of ours is in flight (see k_sweep).  lgkmcnt(0): no LDS request is open behind the chunk
    // barrier either, but the compiler cannot know that no scalar load of the prologue is (they return out of order),
    // and would make K-step 0's first use of LDS data wait for ALL of that step's requests
    __builtin_amdgcn_s_waitcnt(0x0070);
    if (c + 1 < nchunks) issue_chunk(1 - parity, next_rec);
    const int par = parity * kSlimSweepBlock;
    const double *tbuf = pinned(tb0 + par);
    const double *mine0 = pinned(mb0 + par);
    const double *ubuf = pinned(ub0 + par);
    double *xdst = pinned(xd1 - par);
#pragma unroll
    for (int tt = 0; tt < CH; ++tt) {
      const int rn = c * CH + tt;
      constexpr int kXS = 3;  // K-steps that carry expansion work
      constexpr int kT0[3] = {0, 5, 9}, kT1[3] = {5, 9, 13};
      if (tt == kXS && c + 2 < nchunks) issue_private(next_rec + kChunkDoubles);
      if (rn < m.steps) {
        const double *tl = tbuf + (size_t)tt * kSlimStepTiles;
        const double *mine = mine0 + (size_t)tt * kSlimRec;
        const int slot_p = (4 * tt) & 15;
        const int slot_w = (slot_p + 12) & 15;
        if (tt > 0) __builtin_amdgcn_s_waitcnt(0xC07F);  // what the last burst requested (lam_next, taps, row) is here
        const double lamP = tt == 0 ? mine[10] : lam_next;
        double g0 = n0, g1 = n1, g2 = n2, g3 = n3, g4 = n4, g5 = n5, g6 = n6;
        double2 p01 = n01, p23 = n23;
        if (tt == 0) {
          p01 = *reinterpret_cast<const double2 *>(mine);
          p23 = *reinterpret_cast<const double2 *>(mine + 2);
        }
        const double py = p01.x, pmu = p01.y, pom = p23.x, pnu = p23.y;
        __builtin_amdgcn_sched_barrier(0);
        [[maybe_unused]] WingFront wf;
        [[maybe_unused]] bool near = false;
        if constexpr (LINES == 3) {
          if (tt == 0) {  // needs the wavelength (requested first) only: runs while taps and row arrive
            wf = wing3_front(lamP, ms_r[0], ms_r[1], ms_r[2], cs, &near);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        // (2) instrument broadening for pixel 4 rn + jj: voigt.c:297-299 (symmetric taps).  In front of (1)
        // since round 5: the three-line wing tier takes this pixel's d along and returns 1/d from the same
        // v_rcp_f64 as its own three quotients (wing_sum3_rcp4): 151.06 -> 150.21 ms on one box
        // (profiles/r05_ab_rcp4.txt), and the two spilled registers are gone.  On the symmetric pairs: three adds,
        // one multiply and three FMAs instead of eight operations (as k_sweep: change them together).
        double absorb = g3 * tap3;
        absorb = fma(g0 + g6, tap0, absorb);
        absorb = fma(g1 + g5, tap1, absorb);
        absorb = fma(g2 + g4, tap2, absorb);
        if (is_null) absorb = 1.0;
        const double a2 = absorb * absorb;
        const double d = fma(pom, a2, pnu);
        double inv_d;
        // (1) raw profile three K-steps ahead: voigt.c:282-292
        double total;
        if constexpr (LINES == 3) {
          if (tt > 0) wf = wing3_front(lamP, ms_r[0], ms_r[1], ms_r[2], cs, &near);
          WingLines3 wl;
          total = wing3_back_rcp4(wf, d, e3v, &inv_d, &wl);
          if (__builtin_expect(__any(near), 0)) total = near_lines3(lamP, mult_r[0], mult_r[1], mult_r[2], wl);
        } else {
          total = optical_sum(lamP);
          inv_d = fast_rcp(d);
        }
        const ExpState es = exp_ring_begin_scaled(nscale64 * total, exp_pad);
        __builtin_amdgcn_sched_barrier(0);
        double bop[14];
#pragma unroll
        for (int cc = 0; cc < kSlimTilesW; ++cc) bop[cc] = tl[cc * 64];
        bop[13] = ubuf[(size_t)tt * kSlimRec];  // m[0..15] of the 4 pixels in lane order: the u tile
        __builtin_amdgcn_sched_barrier(0);
        const double pser = exp_series_scaled(es);
        // (3) weights: process_qsos.m:192-198 folded into log_mvnpdf_low_rank.m:11-15.  Between the exp series and
        // its multiply by the table entry, which was requested just before the B fragments.
        const double r = fma(-absorb, pmu, py);
        const double w = a2 * inv_d;
        const double ri = r * inv_d;
        const double u = absorb * ri;
        quad_sum = fma(r, ri, quad_sum);
        dprod *= d;
        if (tt & 1) {
          dexp += __builtin_amdgcn_frexp_exp(dprod);
          dprod = __builtin_amdgcn_frexp_mant(dprod);
        }
        __builtin_amdgcn_sched_barrier(0);
        const double raw = exp_finish_scaled(es, pser);
        my_ring[slot_w] = raw;
        my_ring[slot_w + 16] = raw;
        Operands x;
        if (tt < kXS) expand_load(kT0[tt < kXS ? tt : 0], kT1[tt < kXS ? tt : 0], x);
        if (tt + 1 < CH) lam_next = mine[kSlimRec + 10];
        __builtin_amdgcn_sched_barrier(0);
        // (4) rank-4 update of [B | v] on the matrix cores, in two parts with the next K-step's requests between them
        constexpr int kSplit = 11;
        // vech columns 208, 209 and m columns 16..19 of this lane's pixel
        const double2 xp = *reinterpret_cast<const double2 *>(mine + 8);
        const double2 u01 = *reinterpret_cast<const double2 *>(mine + 4);
        const double2 u23 = *reinterpret_cast<const double2 *>(mine + 6);
#pragma unroll
        for (int cc = 0; cc < kSplit; ++cc)
          acc[cc] = __builtin_amdgcn_mfma_f64_16x16x4f64(cc < kSlimTilesW ? w : u, bop[cc], acc[cc], 0, 0, 0);
        if (tt < kXS) expand_store(xdst, kT0[tt < kXS ? tt : 0], kT1[tt < kXS ? tt : 0], x);
        if (tt + 1 < CH) {
          __builtin_amdgcn_sched_barrier(0);
          const double *g = my_ring + ((4 * (tt + 1)) & 15);
          n0 = g[0], n1 = g[1], n2 = g[2], n3 = g[3], n4 = g[4], n5 = g[5], n6 = g[6];
          n01 = *reinterpret_cast<const double2 *>(mine + kSlimRec);
          n23 = *reinterpret_cast<const double2 *>(mine + kSlimRec + 2);
          __builtin_amdgcn_sched_barrier(0);
        } else {  // K-step 0 of the next chunk finds its taps in registers (ring slots 0..9: 4 CH is a multiple of 16)
          __builtin_amdgcn_sched_barrier(0);
          const double *g = my_ring;
          n0 = g[0], n1 = g[1], n2 = g[2], n3 = g[3], n4 = g[4], n5 = g[5], n6 = g[6];
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int cc = kSplit; cc < 14; ++cc)
          acc[cc] = __builtin_amdgcn_mfma_f64_16x16x4f64(cc < kSlimTilesW ? w : u, bop[cc], acc[cc], 0, 0, 0);
        // the 6 FMAs of the off-matrix columns
        xw[0] = fma(w, xp.x, xw[0]);
        xw[1] = fma(w, xp.y, xw[1]);
        xu[0] = fma(u, u01.x, xu[0]);
        xu[1] = fma(u, u01.y, xu[1]);
        xu[2] = fma(u, u23.x, xu[2]);
        xu[3] = fma(u, u23.y, xu[3]);
      }
    }
    glds_wait();      // the prefetched raw chunk and this wave's next rows have landed ...
    __syncthreads();  // ... everyone's tiles of the next chunk are written; this chunk's buffers are free
    next_rec += kChunkDoubles;
  };
  for (int c = 0; c < nchunks; ++c) chunk(c, c & 1);

  double logd_sum = log(dprod) + (double)dexp * 0.6931471805599453;
  quad_sum += __shfl_xor(quad_sum, 16);
  quad_sum += __shfl_xor(quad_sum, 32);
  logd_sum += __shfl_xor(logd_sum, 16);
  logd_sum += __shfl_xor(logd_sum, 32);
#pragma unroll
  for (int x = 0; x < kXW; ++x) {
    xw[x] += __shfl_xor(xw[x], 16);
    xw[x] += __shfl_xor(xw[x], 32);
  }
#pragma unroll
  for (int x = 0; x < kXU; ++x) {
    xu[x] += __shfl_xor(xu[x], 16);
    xu[x] += __shfl_xor(xu[x], 32);
  }

  using ES = EpilogueShape<13, 1>;
  double *Eg = smem + (size_t)wave * ES::SPP * ES::stride(16);
#pragma unroll
  for (int p = 0; p < ES::PASSES; ++p) {
    int sigma;
    bool writer;
    const double ll = slim_factor_pass(acc, xw, xu, p, Eg, lane, a.k, quad_sum, logd_sum, m.n_kept, &sigma, &writer);
    const int64_t slot_s = slot0 + sigma;
    const int32_t sample_s = __shfl(sample, sigma + 16 * jj);
    if (writer) {
      if (slot_s < a.S) a.sample_ll[(int64_t)q * a.S + sample_s] = ll + m.ll_bias;
      else if (slot_s == a.S) a.ll_no_dla[q] = ll + m.ll_bias;
    }
  }
}
