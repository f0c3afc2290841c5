// sweep_slim_kernel.hpp -- the fp64 sweep for k <= 20, three Lyman lines (the production case), on
// SLIM step records: the B-operand tiles vech(m m') are formed inside the sweep.
//
// k_sweep (sweep_expanded_kernel.hpp) streams, per K-step of 4 pixels, a pre-expanded record of 14 MFMA
// B-operand tiles: 7680 B of HBM per step, 2.9 MB per quasar, 2.9 GB per 1000 quasars -- 18 times
// the algorithmic traffic, 59 GB for one DR12Q shard.  Only 4 x (20 + 5) of those 960 doubles are
// information: the 4 interpolated M rows, the 4 pixel rows and the wavelengths.  Here a step record
// is those alone (896 B, 0.34 MB per quasar) and the 13 vech tiles are produced on the fly:
//
//   * Column map.  The MFMA does not care which (i, j) a tile column holds, only the epilogue does,
//     so the 210 = 208 + 2 entries of the lower triangle are dealt to (tile, column) such that a
//     lane can form its 13 products from ONE address register and immediate offsets: with c = its
//     column (0..15) and the row of M stored twice in a row in LDS,
//        tile n = 0..7 :  m[c] * m[(c + n) mod 16]       the n-th circulant diagonal of the 16 x 16 block
//        tile 8        :  m[c] * m[c + 8]  (c < 8);  for c >= 8 eight of the ten pairs (16+a, 16+b)
//        tile 9 + r    :  m[c] * m[16 + r]               r = 0..3
//     and the last two pairs, (19, 18) and (19, 19), stay on the VALU as in k_sweep (vech columns
//     208, 209).  Per tile: one ds_read_b64 (immediate offset 8 n), one v_mul_f64, one ds_write_b64.
//   * Who does it.  Wave w of the block expands K-step w of the NEXT chunk (4 steps per chunk, 4
//     waves) into the tile buffer the block will read after the next barrier, spread over K-steps
//     0..2 of the current chunk: 13 multiplies per wave and chunk, 3.3 per K-step, against 93 VALU
//     instructions a K-step already has.  Its 4 M rows arrive by a private 1-KiB LDS-DMA whose
//     per-lane source addresses lay each 16-double row down twice (that is what makes (c + n) mod 16
//     an immediate offset); nobody else reads that landing zone, so it needs no barrier.
//   * The rest of a record (pixel rows, m columns 16..19, the two VALU columns, wavelengths, and m
//     columns 0..15 in lane order, which IS the u tile) is copied whole by the block's chunk DMA,
//     double-buffered as before.  One barrier per chunk, as before.
//
// Block shape.  k_sweep_slim and k_sweep_slim_boxed run 4 waves (64 sample slots) on 4-step chunks in
// exactly HALF of a CU's LDS, so that two blocks share a CU: the two waves of a SIMD then belong to
// different blocks, meet no common barrier and do not enter prologue and epilogue together (the
// fp64 MFMA and the VALU do not overlap within a SIMD; what one wave leaves idle only an independent
// wave can fill).  __launch_bounds__(256, 2) keeps a wave at 256 registers for that.  The multi-DLA
// kernel (sweep_multi_slim_kernel.hpp) keeps the 8-wave block and 8-step chunks of kSlimCH below.
//
// LDS of a block (80 KiB):
//        0  ring: 4 waves x 16 samples x 33 doubles                                       16 896 B
//           (the 64-entry exp table lives in the pad slot, 32, of its 64 rows)
//   16 896  parity 0: 4 K-steps x 13 tiles of 512 B (26 624 B) | 4 raw records (3584 B)    30 208 B
//   47 104  parity 1: the same                                                            30 208 B
//   77 312  4 landing zones of 1152 B                                                      4 608 B
//   81 920
// Every per-parity address is (per-lane constant) + parity x 30 208 B: four adds per chunk, none per
// K-step.  The raw chunk is copied record by record, wave w record w with 56 lanes: 3584 B is no
// whole number of KiB and nothing may land behind a parity's raw buffer.
// Results are bit-identical to k_sweep's: the same products, the same MFMA sequence per column.
#pragma once
#include <type_traits>

#include "epilogue_factor.hpp"
#include "prepare_kernels.hpp"  // BuildRecordsArgs
#include "voigt_tiers.hpp"

namespace gpdla {

constexpr int kSlimExtras = 12;                      // doubles per pixel: y mu omega2 nu | m16..19 | p208 p209 | lam | pad
constexpr int kSlimRec = 4 * kSlimExtras + 64;       // 112 doubles = 896 B per K-step: extras, then m[0..15] of 4 pixels
constexpr int kSlimCH = 8;                           // K-steps per chunk = waves per block (k_sweep_multi_slim)
constexpr int kSlimTilesW = 13;
constexpr int kSlimStepTiles = kSlimTilesW * 64;     // doubles of expanded tiles per K-step
constexpr int kSlimTileBuf = kSlimCH * kSlimStepTiles;               // 6656
constexpr int kSlimRawBuf = kSlimCH * kSlimRec;                      // 896
constexpr int kSlimLand = 4 * 32 + 4 * 4;                            // per wave: 4 doubled rows + 4 x m16..19
constexpr int kSlimBlock = kSlimTileBuf + kSlimRawBuf;               // one parity: tiles, then raw records (7552 doubles)
static_assert((kSlimBlock * 8) % 512 == 0, "both parities reachable with ds_read2st64 offsets");
static_assert((kSlimCH * kSlimRec) % 128 == 0, "a raw chunk is a whole number of KiB");
// k_sweep_slim / k_sweep_slim_boxed: 4 waves, 4-step chunks, half a CU's LDS (see "Block shape" above)
constexpr int kSlimWaves = 4;
constexpr int kSlimSweepCH = 4;                                                  // K-steps per chunk = waves per block
constexpr int kSlimSweepRingD = kSlimWaves * kSamplesPerWave * kRing2;           // 2112
constexpr int kSlimSweepTileBuf = kSlimSweepCH * kSlimStepTiles;                 // 3328
constexpr int kSlimSweepBlock = kSlimSweepTileBuf + kSlimSweepCH * kSlimRec;     // one parity: 3776 doubles
constexpr int kSlimLdsDoubles = kSlimSweepRingD + 2 * kSlimSweepBlock + kSlimWaves * kSlimLand;
static_assert(kSlimSweepCH == kSlimWaves, "wave w expands, and copies, K-step w of the next chunk");
static_assert((kSlimSweepBlock * 8) % 512 == 0, "both parities reachable with ds_read2st64 offsets");
static_assert(kSlimLdsDoubles * 8 == 80 * 1024, "two blocks of the slim sweep fill the LDS of a CU exactly");
static_assert(kSlimWaves * kSamplesPerWave == kExpTab, "the exp table has one ring row's pad slot per entry");
static_assert((kSlimSweepCH * 4) % 16 == 0, "the ring slots of a K-step depend on its place in the chunk alone");
static_assert(kSlimRec % 2 == 0 && kSlimRec / 2 <= 64, "one wave copies one record, 16 bytes per lane");
static_assert(kSlimWaves * EpilogueShape<13, 1>::SPP * EpilogueShape<13, 1>::stride(16) <= kSlimLdsDoubles,
              "the epilogue's rows fit the block's LDS");

// (i, j), i >= j, of column `col` of tile `tile` (see the column map above)
__host__ __device__ constexpr int slim_pair_i(int tile, int col) {
  if (tile < 8) {
    const int b = (col + tile) & 15;
    return col > b ? col : b;
  }
  if (tile == 8) {
    if (col < 8) return col + 8;
    const int l = col - 8;  // (16,16) (17,16) (17,17) (18,16) (18,17) (18,18) (19,16) (19,17)
    return l < 1 ? 16 : l < 3 ? 17 : l < 6 ? 18 : 19;
  }
  return 16 + (tile - 9);
}
__host__ __device__ constexpr int slim_pair_j(int tile, int col) {
  if (tile < 8) {
    const int b = (col + tile) & 15;
    return col > b ? b : col;
  }
  if (tile == 8) {
    if (col < 8) return col;
    const int l = col - 8;
    return 16 + (l < 1 ? 0 : l < 3 ? l - 1 : l < 6 ? l - 3 : l - 6);
  }
  return col;
}
// position in the packed lower triangle (row-wise, idx(i, j) = i (i + 1) / 2 + j) the epilogue reads
__host__ __device__ constexpr int slim_pos(int tile, int col) {
  return slim_pair_i(tile, col) * (slim_pair_i(tile, col) + 1) / 2 + slim_pair_j(tile, col);
}

// ------------------------------------------------------------------------------------------
// k_build_slim_records: record(q, t) = [4 pixels x 12 extras | 4 pixels x m[0..15]], record `steps`
// neutral, as k_build_records' trailing one.  A pure gather: 112 doubles per K-step.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_build_slim_records(BuildRecordsArgs a) {
  const int q = a.order[blockIdx.x / a.blocks_per_quasar];
  const int bq = blockIdx.x % a.blocks_per_quasar;
  const QuasarMeta m = a.meta[q];
  const int k = a.k;
  const int n_pad = m.n_u + 6;
  double *out = a.records + m.rec_off * (int64_t)kSlimRec;
  const int64_t total = (int64_t)(m.steps + 1) * kSlimRec;
  for (int64_t e = (int64_t)bq * 256 + threadIdx.x; e < total; e += (int64_t)a.blocks_per_quasar * 256) {
    const int step = (int)(e / kSlimRec), r = (int)(e - (int64_t)step * kSlimRec);
    double v = 0.0;
    if (r < 4 * kSlimExtras) {
      const int jj = r / kSlimExtras, f = r - jj * kSlimExtras;
      const int64_t row = m.pix_off + 4 * (int64_t)step + jj;
      if (f < 4) {
        const PixelRow px = a.pix[row];
        v = f == 0 ? px.y : f == 1 ? px.mu : f == 2 ? px.omega2 : px.nu;
      } else if (f < 8) {
        if (kXUColumn + (f - 4) < k) v = a.Mi[row * k + kXUColumn + (f - 4)];
      } else if (f < 10) {  // vech columns 208, 209 = (19, 18), (19, 19)
        if (k == 20) v = a.Mi[row * k + 19] * a.Mi[row * k + 18 + (f - 8)];
      } else if (f == 10) {
        int P = 4 * (step + 3) + jj;
        if (P > n_pad - 1) P = n_pad - 1;
        v = a.lam_pad[m.lam_off + P];
      }
    } else {
      const int l = r - 4 * kSlimExtras, jj = l >> 4, col = l & 15;
      if (col < k) v = a.Mi[(m.pix_off + 4 * (int64_t)step + jj) * k + col];
    }
    out[e] = v;
  }
}

// exp tables in the ring's pad slots: entry j of the 2^(j/64) table sits in slot 32 of ring row j
__device__ __forceinline__ ExpState exp_ring_begin_scaled(double t, const double *ring_pad) {
  ExpState e;
  const double nf = rint(t);
  asm("v_cvt_i32_f64 %0, %1" : "=v"(e.ni) : "v"(nf));  // saturating (see exp_table_begin)
  e.tabv = ring_pad[(e.ni & (kExpTab - 1)) * kRing2];
  e.r = t - nf;
  return e;
}

// exp_table_end_scaled in two pieces, so that arithmetic which does not need the table entry can stand
// between its request and its first use: the series in the reduced argument (no LDS data) ...
__device__ __forceinline__ double exp_series_scaled(const ExpState &e) {
  constexpr double L = 0.010830424696249145;  // (ln2/64)^k / k!, as in exp_table_end_scaled
  constexpr double c1 = L, c2 = L * L / 2, c3 = L * L * L / 6, c4 = L * L * L * L / 24, c5 = L * L * L * L * L / 120;
  double p;
  const double c4v = c4;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "s"(c5), "v"(e.r), "v"(c4v));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(e.r), "s"(c3));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(e.r), "s"(c2));
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(p) : "v"(p), "v"(e.r), "s"(c1));
  return fma(p, e.r, 1.0);
}
// ... and the table entry times the series, scaled
__device__ __forceinline__ double exp_finish_scaled(const ExpState &e, double p) { return ldexp(e.tabv * p, e.ni >> 6); }

// wing_sum3_rcp4 in two pieces (the same operations on the same operands): the part that needs the
// wavelength alone -- velocities, s_j, the near vote, the prefix products -- and the part that takes d (e3v: kE3 in
// a vector register, which the caller holds there across its loop).
struct WingFront {
  double sa, sb, sc, pab, pabc;
};
__device__ __forceinline__ WingFront wing3_front(double lamP, double msa, double msb, double msc, double cs, bool *near) {
  WingFront f;
  const double xa = fma(lamP, msa, -cs), xb = fma(lamP, msb, -cs), xc = fma(lamP, msc, -cs);
  f.sa = fma(xa, xa, g_lines.y2[0]), f.sb = fma(xb, xb, g_lines.y2[1]), f.sc = fma(xc, xc, g_lines.y2[2]);
  *near = min(min(hi_word(f.sa), hi_word(f.sb)), hi_word(f.sc)) < 0x408C2000u;
  f.pab = f.sa * f.sb, f.pabc = f.pab * f.sc;
  return f;
}
__device__ __forceinline__ double wing3_back_rcp4(const WingFront &f, double d, double e3v, double *inv_d, WingLines3 *lines) {
  const double rinv = fast_rcp(f.pabc * d);
  *inv_d = rinv * f.pabc;
  const double r3 = rinv * d;
  const double rc = r3 * f.pab, r2 = r3 * f.sc;
  const double ra = r2 * f.sb, rb = r2 * f.sa;
  double ta = wing_lead(ra, e3v), tb = wing_lead(rb, e3v), tc = wing_lead(rc, e3v);
  ta = fma(ta, ra, g_lines.t2[0]); tb = fma(tb, rb, g_lines.t2[1]); tc = fma(tc, rc, g_lines.t2[2]);
  ta = fma(ta, ra, kE1); tb = fma(tb, rb, kE1); tc = fma(tc, rc, kE1);
  ta = fma(ta, ra, 1.0); tb = fma(tb, rb, 1.0); tc = fma(tc, rc, 1.0);
  const double qa = ra * ta, qb = rb * tb, qc = rc * tc;
  *lines = WingLines3{{f.sa, f.sb, f.sc}, {qa, qb, qc}};  // for near_lines3, where the wave votes
  return fma(g_lines.cwing[2], qc, fma(g_lines.cwing[1], qb, g_lines.cwing[0] * qa));
}

// Epilogue pass of the slim sweep: factor_pass of epilogue_factor.hpp with the spill scattered
// through the column map (tile, column) -> packed-triangle position.
__device__ __forceinline__ double slim_factor_pass(const d4 (&acc)[14], const double (&xw)[kXW],
                                                   const double (&xu)[kXU], int p, double *Eg, int lane, int k,
                                                   double quad_sum, double logd_sum, int n_kept,
                                                   int *sigma_out, bool *writer) {
  using ES = EpilogueShape<13, 1>;
  constexpr int voff = (13 + 1) * 16;
  constexpr int ncols = ES::stride(16);
  const int s = lane & 15, jj = lane >> 4;
  const int half = s >> 3;
  const int sigma = Mat<double>::sample_of(jj, ES::RPP * p + half);
  const double q_s = __shfl(quad_sum, sigma + 16 * jj);
  const double ld_s = __shfl(logd_sum, sigma + 16 * jj);
  double *e = Eg + (size_t)(jj * ES::RPP) * ncols;
#pragma unroll
  for (int cc = 0; cc < 14; ++cc) {
    const int at = cc < kSlimTilesW ? slim_pos(cc, s) : voff + s;  // the u tile: v[0..15]
#pragma unroll
    for (int h = 0; h < ES::RPP; ++h) e[h * ncols + at] = acc[cc][ES::RPP * p + h];
  }
  {
    const int r = Mat<double>::reg_of(s);
    if (jj == 0 && r / ES::RPP == p) {
      double *es = Eg + (size_t)(Mat<double>::jj_of(s) * ES::RPP + r % ES::RPP) * ncols;
#pragma unroll
      for (int x = 0; x < kXW; ++x) es[kXWColumn + x] = xw[x];
#pragma unroll
      for (int x = 0; x < kXU; ++x) es[voff + kXUColumn + x] = xu[x];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  *sigma_out = sigma;
  *writer = (s & (ES::LPS - 1)) == 0;
  return factor_rows<ES::ROWS, ES::LPS, 20>(e + half * ncols, s & (ES::LPS - 1), k, voff, q_s, ld_s, n_kept);
}

// The kernel itself lives in sweep_slim_body.hpp, a header WITHOUT an include guard that is included twice:
// once as k_sweep_slim over SweepArgs and once as k_sweep_slim_boxed over BoxedSweepArgs (the refine pass,
// DESIGN.md 4.18).  Two templates of different names, not one with a flag or one device body behind two
// wrappers: either of those changed the name or the register allocation of the shipped k_sweep_slim<3>.
#define GPDLA_SWEEP_SLIM_KERNEL k_sweep_slim
#define GPDLA_SWEEP_SLIM_ARGS SweepArgs
#include "sweep_slim_body.hpp"
#undef GPDLA_SWEEP_SLIM_KERNEL
#undef GPDLA_SWEEP_SLIM_ARGS
#define GPDLA_SWEEP_SLIM_KERNEL k_sweep_slim_boxed
#define GPDLA_SWEEP_SLIM_ARGS BoxedSweepArgs
#include "sweep_slim_body.hpp"
#undef GPDLA_SWEEP_SLIM_KERNEL
#undef GPDLA_SWEEP_SLIM_ARGS

}  // namespace gpdla
