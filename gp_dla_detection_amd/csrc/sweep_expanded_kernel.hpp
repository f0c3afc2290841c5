// sweep_expanded_kernel.hpp -- k_sweep, the sweep on pre-expanded records: fused Voigt profile -> scaled low-rank
// Gaussian log-pdf, one sample per MFMA row (process_qsos.m:149-151 and 185-199 + voigt.c:278-299 +
// log_mvnpdf_low_rank.m).  The fp64 product sweeps are k_sweep_slim and k_sweep_split_slim; this kernel serves the
// fp32-contraction study (k_sweep<float, ...>) and, as k_sweep<double, ...>, the bit-identity tests of the legacy library.
#pragma once
#include "epilogue_factor.hpp"
#include "voigt_tiers.hpp"

namespace gpdla {

// ------------------------------------------------------------------------------------------
// k_sweep.
//
// Grid: 8 * ceil(nq/8) * blocks_per_quasar blocks of 512 threads = 8 waves (two per SIMD, so one
// wave's Voigt VALU work overlaps the other's MFMAs), flattened in x.  Workgroups are dealt
// round-robin over the 8 XCDs, so block i works on quasar 8*(i/8/bpq) + i%8: every XCD streams ONE
// quasar's records at a time and keeps them in its own 4 MB L2.
//
// A wave owns 16 sample slots (MFMA rows); lane l = 16*jj + s works on sample slot s and, at
// K-step t, on pixel 4t + jj.  Slot S (one past the last sample) is the null model (a = 1):
// process_qsos.m:149-151.  Samples are visited in ascending z_DLA order (perm), so the lanes of a
// wave sit within a few pixels of each other relative to every line centre and the accurate
// tier of the Voigt function is taken by whole waves, one line at a time.
//
// TS ("tile split"): number of waves that share one group of 16 samples and split the B tiles
// between them (1 for k <= 20; 4 for k <= 40, where 55 tiles of accumulators do not fit one wave).
//
// LDS (one dynamic array): exp table | two chunk buffers of kChunkSteps records (global_load_lds
// double buffering) | raw-profile rings | per-sample line multipliers.  After the loop everything
// behind the exp table is reused by the Cholesky epilogue.
//
// Template parameters: NTW B tiles per wave, TS tile split, kChunkSteps records per LDS chunk
// (4, or 2 with two chunks unrolled: ring slots are then compile-time; 1: run-time slots),
// TW tiles that take the weight w (the rest take u; TS*NTW tiles in all, zero-padded), LINES
// number of Lyman lines when known at compile time (0: read num_lines at run time).
template <typename T, int WAVES, int NTW, int TS, int kChunkSteps, int TW, int LINES>
__global__ __launch_bounds__(WAVES * 64) void k_sweep(SweepArgs a) {
  extern __shared__ double smem[];
  static_assert(kChunkSteps == 8 || kChunkSteps == 4 || kChunkSteps == 2 || kChunkSteps == 1, "chunks of 8, 4, 2 or 1 K-steps");
  // chunks unrolled per loop iteration so that 4 K-steps (one turn of the 16-slot ring) are
  // straight-line code with compile-time ring slots and stage-buffer addresses
  constexpr int UN = kChunkSteps == 2 ? 2 : 1;
  constexpr int GROUPS = WAVES / TS;  // sample groups per block
  constexpr int NT = NTW * TS;
  constexpr int TD = 64 * (int)sizeof(T) / 8;  // doubles occupied by one 64-element tile
  constexpr int RD = NT * TD + record_extras(NT);
  constexpr bool kCompact = tiles_compact(NT);  // 13 + 1 tiles on the matrix cores, 2 + 4 columns on the VALU
  using acc_t = typename Mat<T>::acc_t;
  const int64_t xj = blockIdx.x >> 3;
  const int64_t pos = 8 * (xj / a.blocks_per_quasar) + (blockIdx.x & 7);
  const int bq = (int)(xj % a.blocks_per_quasar);
  if (pos >= a.nq) return;
  // quasars are dealt in order of decreasing length (a.order, built at upload), so the eight
  // quasars in flight -- one per XCD -- are of nearly equal length and the XCDs stay in step
  const int64_t q = a.order[pos];
  const QuasarMeta m = a.meta[q];
  if (m.status != 0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int group = wave / TS, role = wave % TS;
  const int s = lane & 15, jj = lane >> 4;
  const int L = LINES > 0 ? LINES : a.num_lines;

  // LDS addressing costs VALU instructions (which cost MFMA time, fact 1 of DESIGN.md section 4)
  // whenever a constant does not fit the instruction's offset field: 8 bits x 8 B for
  // ds_read2_b64, 8 bits x 512 B for ds_read2st64_b64, 16 bits for ds_read_b64 / ds_read_b128.  So:
  // the ring, read with ds_read2_b64, sits at address 0 (a lane's 37 slots fit the 2040 B reach);
  // the exp table and the records' extras are read with b64 / b128; records are a multiple of
  // 512 B and the stage buffers 512-B aligned, so the tile reads fold (buffer, step, tile) into
  // the st64 offsets.
  double *ring = smem;                                             // [WAVES][16][33]
  double *exp_tab = ring + WAVES * kSamplesPerWave * kRing2;       // [64]
  double *stage = exp_tab + kExpTab;                               // [2][kChunkSteps][RD]
  double *mult_s = stage + (size_t)2 * kChunkSteps * RD;           // [GROUPS*16][L]

  const int64_t slot0 = (int64_t)bq * (GROUPS * kSamplesPerWave) + group * kSamplesPerWave;
  const int64_t slot = slot0 + s;
  const bool is_sample = slot < a.S;
  const bool is_null = !is_sample;  // slot == S is the null model; slots beyond it are idle copies
  // (null-model and idle slots: the last sample in z order, see k_sweep_slim)
  const int32_t sample = a.perm[is_sample ? slot : a.S - 1];
  // process_qsos.m:162-164
  const double z_dla = m.min_z_dla + (m.max_z_dla - m.min_z_dla) * a.offset_samples[sample];
  const double nhi = a.nhi_samples[sample];
  double *my_mult = mult_s + (size_t)(group * kSamplesPerWave + s) * L;
  double mult_r[LINES > 0 ? LINES : 1];
  if (LINES > 0) {
#pragma unroll
    for (int j = 0; j < LINES; ++j)  // voigt.c:278-279
      mult_r[j] = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z_dla)) / 1e8;
  } else if (role == 0 && jj == 0) {
    for (int j = 0; j < L; ++j) my_mult[j] = g_lines.c / (g_lines.wavelength_cm[j] * (1 + z_dla)) / 1e8;
  }
  if (tid < kExpTab) exp_tab[tid] = exp2((double)tid * (1.0 / kExpTab));
  // this lane's ring row, already offset by its pixel phase jj (slots are then compile-time)
  double *my_ring = ring + (size_t)(wave * kSamplesPerWave + s) * kRing2 + jj;
  const double *lam = a.lam_pad + m.lam_off;
  const int n_pad = m.n_u + 6;
  // exp(N * total / (sqrt(2 pi) sigma)) with total = -Sum lead_j Re w_j (voigt.c:288-291)
  // (times 64/ln2: the exp below takes its argument pre-scaled, exp_table_begin_scaled)
  const double nscale64 = -nhi * g_lines.inv_sqrt2pi_sigma * kInvSqrtPi * kExpScale;
  const double *rec_base = a.records + m.rec_off * (int64_t)RD;
  const int nchunks = (m.steps + kChunkSteps - 1) / kChunkSteps;

  // asynchronous global -> LDS copy of one chunk of records (see glds_chunk)
  static_assert((kChunkSteps * RD) % 128 == 0, "a chunk is a whole number of KiB");
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t stage_lds = __builtin_amdgcn_readfirstlane(lds_address(stage));
  auto issue_chunk = [&](int c) {
    glds_chunk<kChunkSteps * RD / 128, WAVES>(rec_base + (size_t)c * kChunkSteps * RD,
                                              stage_lds + (uint32_t)(c & 1) * (uint32_t)(kChunkSteps * RD * 8), wave_s, lane);
  };
  issue_chunk(0);

  const double c_light = g_lines.c, inv_s = g_lines.inv_sqrt2_sigma;
  // wing tier in FMA form: x = lam * (mult_j / (sqrt2 sigma)) - c / (sqrt2 sigma).  It differs
  // from the reference's two-rounding velocity (voigt.c:287, kept in the accurate tier) by
  // <= 3e-12 in x, i.e. <= 2e-13 relative in the optical depth where |x| >= 30.
  double ms_r[LINES > 0 ? LINES : 1];
#pragma unroll
  for (int j = 0; j < (LINES > 0 ? LINES : 0); ++j) ms_r[j] = mult_r[j] * inv_s;
  const double cs = c_light * inv_s;
#define GPDLA_TOTAL_ACCURATE(lamP)                                                        \
  total_near<LINES>((lamP), mult_r[0], mult_r[LINES > 1 ? 1 : 0], mult_r[LINES > 2 ? 2 : 0], \
                    my_mult, L)
#define GPDLA_RAW_ACCURATE(lamP) exp_table_scaled(nscale64 * GPDLA_TOTAL_ACCURATE(lamP), exp_tab)

  __syncthreads();  // multipliers and the exp table visible
  // prime the ring with padded pixels 0..11 (the raw profile runs three K-steps ahead)
  for (int c3 = 0; c3 < 3; ++c3) {
    const double lam0 = lam[min(4 * c3 + jj, n_pad - 1)];
    double v;
    if (LINES == 3) {
      bool near0;
      WingLines3 wl;
      double total = wing_sum3(lam0, ms_r[0], ms_r[LINES > 1 ? 1 : 0], ms_r[LINES > 2 ? 2 : 0], cs, &near0, &wl);
      if (__any(near0)) total = near_lines3(lam0, mult_r[0], mult_r[LINES > 1 ? 1 : 0], mult_r[LINES > 2 ? 2 : 0], wl);
      v = exp_table_scaled(nscale64 * total, exp_tab);
    } else {
      v = GPDLA_RAW_ACCURATE(lam0);
    }
    my_ring[4 * c3] = v;
    my_ring[4 * c3 + 16] = v;
  }

  acc_t acc[NTW];
#pragma unroll
  for (int c = 0; c < NTW; ++c) acc[c] = acc_t{0, 0, 0, 0};
  double quad_sum = 0.0, dprod = 1.0;
  double xw[kXW] = {0.0, 0.0}, xu[kXU] = {0.0, 0.0, 0.0, 0.0};  // compact class: columns kept off the MFMA
  int dexp = 0;
  const int tile0 = role * NTW;
  const double tap0 = g_lines.taps[0], tap1 = g_lines.taps[1], tap2 = g_lines.taps[2],
               tap3 = g_lines.taps[3];

  glds_wait();  // chunk 0 landed
  __syncthreads();

  // The fp64 MFMA does not overlap with VALU work on its SIMD (tools/fp64_mix_probe.hip), so the
  // loop is written for the fewest instructions, not for interleaving: per K-step one raw-profile
  // value three steps ahead (wing tier branch-free; accurate tier under a wave-uniform vote), the
  // 7-tap broadening from the doubled ring (no wrap-around: slots are compile-time), the weights,
  // then 16 MFMAs.  Two waves per SIMD hide LDS and dependent-issue latency.
  // Per K-step: all LDS operands (7 ring taps, pixel row, 16 B fragments) are requested first and
  // land while the raw-profile VALU chain runs; the only read that chain itself needs, the padded
  // wavelength, is fetched one step early (within a chunk), before the previous MFMA burst.
  for (int c0 = 0; c0 < nchunks; c0 += UN) {
#pragma unroll
  for (int hc = 0; hc < UN; ++hc) {
    const int c = c0 + hc;
    if (UN > 1 && c >= nchunks) break;  // block-uniform
    // Nothing of ours is in flight here (drained before the barrier), so this wait is free; it is
    // for the compiler, whose scratch reloads of the loop preheader would otherwise be waited for
    // inside the K-steps -- behind the prefetch issued on the next line.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (c + 1 < nchunks) issue_chunk(c + 1);  // lands in the other buffer while we compute
    const double *buf = stage + (size_t)(UN > 1 ? hc : (c & 1)) * kChunkSteps * RD;  // UN = 2: c0 is even
    double lam_next = 0.0;
#pragma unroll
    for (int tt = 0; tt < kChunkSteps; ++tt) {
      const int rn = c * kChunkSteps + tt;
      if (rn < m.steps) {
        const double *rec = buf + (size_t)tt * RD;
        const double *extra = rec + NT * TD;
        // ring slot of pixel 4 rn (+ jj, folded into my_ring); compile-time when chunks are 4 long
        const int slot_p = kChunkSteps >= 4 ? (4 * tt) & 15 : (kChunkSteps == 2 ? 4 * (2 * hc + tt) : ((4 * rn) & 15));
        const int slot_w = (slot_p + 12) & 15;
        // lam_next was requested before the previous MFMA burst and has long landed: saying so
        // (s_waitcnt lgkmcnt(0), free) lets the raw chain start under the 15 reads issued next
        // instead of behind all of them.
        if (tt > 0) __builtin_amdgcn_s_waitcnt(0xC07F);
        const double *mine = extra + extras_row(NT, 1) * jj;  // this lane's pixel
        const double lamP = tt == 0 ? extra[extras_lam_stride(NT) * jj + extras_lam(NT, 0)] : lam_next;
        // operands of the broadening / weights / MFMAs of this step
        const double *g = my_ring + slot_p;
        const double g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3], g4 = g[4], g5 = g[5], g6 = g[6];
        const double2 p01 = *reinterpret_cast<const double2 *>(mine);  // ds_read_b128
        const double2 p23 = *reinterpret_cast<const double2 *>(mine + 2);
        const double py = p01.x, pmu = p01.y, pom = p23.x, pnu = p23.y;
        __builtin_amdgcn_sched_barrier(0);  // keep the reads up here (the scheduler sinks them)
        // (2) instrument broadening for pixel 4 rn + jj: voigt.c:297-299 (symmetric taps) -- in front of
        // (1) since round 5: the three-line wing tier takes d along (wing_sum3_rcp4).  On the symmetric pairs:
        // three adds, one multiply and three FMAs (k_sweep_slim spells the same operations: change them together).
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
        bool near;
        [[maybe_unused]] WingLines3 wl;
        if (LINES == 3) {
          total = wing_sum3_rcp4(lamP, ms_r[0], ms_r[LINES > 1 ? 1 : 0], ms_r[LINES > 2 ? 2 : 0], cs, &near, d, &inv_d, &wl);
        } else {
          inv_d = fast_rcp(d);
          total = 0.0;
          near = false;
          for (int j = 0; j < L; ++j) {
            const double x = fma(lamP, my_mult[j] * inv_s, -cs);
            const double x2 = x * x;
            near |= x2 < 900.0;
            total = fma(g_lines.cwing[j], wing_core(x2, g_lines.y2[j]), total);
          }
        }
        if (__builtin_expect(__any(near), 0)) {
          if (LINES == 3) total = near_lines3(lamP, mult_r[0], mult_r[LINES > 1 ? 1 : 0], mult_r[LINES > 2 ? 2 : 0], wl);
          else total = GPDLA_TOTAL_ACCURATE(lamP);
        }
        // B fragments of this step: requested only now, so that they are not live across the
        // accurate-tier branch above (it would spill to make room); they land during the rest of
        // the step, which is ONE basic block from here on: the exp chain of the raw profile and the
        // broadening / weight chain of this step's pixel are independent, and the scheduler
        // interleaves them, so a wave running alone on its SIMD does not sit out their latencies.
        // (the exp table entry is requested ahead of them: LDS returns in order, and the exp chain
        // then waits for one read instead of nine)
        const ExpState es = exp_table_begin_scaled(nscale64 * total, exp_tab);
        __builtin_amdgcn_sched_barrier(0);
        const T *bt = reinterpret_cast<const T *>(rec) + (size_t)tile0 * 64 + lane;
        T bop[NTW];
#pragma unroll
        for (int cc = 0; cc < NTW; ++cc) bop[cc] = bt[(size_t)cc * 64];
        __builtin_amdgcn_sched_barrier(0);
        double raw = exp_table_end_scaled(es);
        my_ring[slot_w] = raw;
        my_ring[slot_w + 16] = raw;
        // (3) weights: process_qsos.m:192-198 folded into log_mvnpdf_low_rank.m:11-15
        const double r = fma(-absorb, pmu, py);
        const double w = a2 * inv_d;
        const double ri = r * inv_d;
        const double u = absorb * ri;
        quad_sum = fma(r, ri, quad_sum);
        // Sum log d as the log of a running product, renormalised every second step (the
        // mantissa times two factors stays in range for any d in [1e-150, 1e150])
        dprod *= d;
        if (kChunkSteps == 1 || (tt & 1)) {
          dexp += __builtin_amdgcn_frexp_exp(dprod);
          dprod = __builtin_amdgcn_frexp_mant(dprod);
        }
        // next step's wavelength, in flight during the MFMA burst
        if (tt + 1 < kChunkSteps) {
          lam_next = extra[RD + extras_lam_stride(NT) * jj + extras_lam(NT, 0)];
          __builtin_amdgcn_sched_barrier(0);
        }
        // (4) rank-4 update of [B | v] on the matrix cores
        // With a tile split only the last role's last NT - TW tiles take u; one wave-uniform
        // select per step instead of one per tile.
        constexpr int kTail = TS == 1 ? 0 : NT - TW;
        static_assert(TS == 1 || kTail <= NTW, "u-tiles must sit in the last role's tiles");
        const T a_tail = (T)(role == TS - 1 ? u : w);
#pragma unroll
        for (int cc = 0; cc < NTW; ++cc) {
          const T aop = TS == 1 ? (T)(cc < TW ? w : u) : (cc < NTW - kTail ? (T)w : a_tail);
          acc[cc] = Mat<T>::mfma(aop, bop[cc], acc[cc]);
        }
        if (kCompact) {  // vech columns 208, 209 and m columns 16..19 of this lane's pixel: 6 FMAs
          static_assert(kXW == 2 && kXU == 4, "three 16-byte reads");
          const double2 xp = *reinterpret_cast<const double2 *>(mine + kExtrasXW);
          const double2 u01 = *reinterpret_cast<const double2 *>(mine + kExtrasXU);
          const double2 u23 = *reinterpret_cast<const double2 *>(mine + kExtrasXU + 2);
          xw[0] = fma(w, xp.x, xw[0]);
          xw[1] = fma(w, xp.y, xw[1]);
          xu[0] = fma(u, u01.x, xu[0]);
          xu[1] = fma(u, u01.y, xu[1]);
          xu[2] = fma(u, u23.x, xu[2]);
          xu[3] = fma(u, u23.y, xu[3]);
        }
      }
    }
    glds_wait();  // the prefetched chunk has landed (this wave's part) ...
    __syncthreads();  // ... and everyone's; all reads of the buffer refilled next are done
  }
  }
#undef GPDLA_RAW_ACCURATE
#undef GPDLA_TOTAL_ACCURATE
  // per-sample scalar sums: combine the four pixel phases jj of each sample
  double logd_sum = log(dprod) + (double)dexp * 0.6931471805599453;
  quad_sum += __shfl_xor(quad_sum, 16);
  quad_sum += __shfl_xor(quad_sum, 32);
  logd_sum += __shfl_xor(logd_sum, 16);
  logd_sum += __shfl_xor(logd_sum, 32);
  if (kCompact) {
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
  }

  // ---- epilogue: factor_pass over the MFMA result registers ------------------------------------
  using ES = EpilogueShape<TW, TS>;
  double *Eg = smem + kExpTab + (size_t)group * ES::SPP * ES::stride(logical_tiles(NT));  // [SPP samples][stride] of this group
#pragma unroll
  for (int p = 0; p < ES::PASSES; ++p) {
    int sigma;
    bool writer;
    const double ll = factor_pass<T, NTW, TS, TW>(acc, xw, xu, p, Eg, lane, role, tile0, a.k, quad_sum,
                                                  logd_sum, m.n_kept, &sigma, &writer);
    const int64_t slot_s = slot0 + sigma;
    const int32_t sample_s = __shfl(sample, sigma + 16 * jj);
    if (writer) {
      if (slot_s < a.S) a.sample_ll[(int64_t)q * a.S + sample_s] = ll + m.ll_bias;
      else if (slot_s == a.S) a.ll_no_dla[q] = ll + m.ll_bias;
    }
  }
}

}  // namespace gpdla
