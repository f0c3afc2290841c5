// sweep_primitives.hpp -- what the sweep kernels are written in: their argument structs, the fast reciprocal, exp and
// reciprocal square root, and the asynchronous global -> LDS copies.
//
// Algebra of the sweep.  For one quasar and one sample with absorption a (n pixels):
//   r = y - a mu,  d = omega2 a^2 + nu,  w = a^2/d,  u = a r/d
//   B = I + Sum_p w_p m_p m_p',  v = Sum_p u_p m_p,
//   log N = -1/2 [ Sum r^2/d - v' B^-1 v + Sum log d + 2 Sum log L_jj + n log 2pi ],  B = L L'.
// This is log_mvnpdf_low_rank.m:11-32 with the k x n matrix C of :26 eliminated.  Over the S
// samples of a quasar, B and v are ONE dense contraction  [W | U] (S x n) * [P | M] (n x (k(k+1)/2
// + k))  with P_p = vech(m_p m_p') depending on the quasar only: that runs on the fp64 matrix
// cores (v_mfma_f64_16x16x4_f64), while the Voigt profile that produces W and U runs on the VALU
// and never touches HBM.
#pragma once
#include "batch_types.hpp"

namespace gpdla {

constexpr int kSweepWaves = 8;  // waves per block of the fp64 sweeps

struct SweepArgs {
  const QuasarMeta *meta;
  const double *records;
  const double *lam_pad;
  const double *offset_samples;   // [S]
  const double *nhi_samples;      // [S]
  const int32_t *perm;            // [S] sample indices in ascending offset (= z_DLA) order
  const int32_t *order;           // [nq] quasar indices in order of decreasing pixel count
  const PixelRow *pix;            // per-pixel pool (k_sweep_split reads rows directly)
  int64_t S;
  int64_t nq;
  int32_t blocks_per_quasar;
  int32_t k, tiles_w, ntiles, num_lines;
  double *sample_ll;              // [nq][S]   process_qsos.m:196
  double *ll_no_dla;              // [nq]      process_qsos.m:149
};

// The boxed sweeps of the refine pass (refine_kernels.hpp): SweepArgs plus the box of
// (z_DLA, log10 N_HI) of the level being swept, quasar q's at box + q * kRefineBoxStride as
// (z_lo, z_hi, n_lo, n_hi).  The unboxed sweeps take plain SweepArgs: their kernel arguments do not change.
constexpr int kRefineMaxLevels = 4;
constexpr int kRefineBoxStride = 4 * kRefineMaxLevels;   // doubles per quasar: [level][4]
struct BoxedSweepArgs : SweepArgs {
  const double *box;
};
// quasar q's box (the first overload is only ever named in a discarded branch of an unboxed sweep)
__device__ __forceinline__ const double *sweep_box(const SweepArgs &, int64_t) { return nullptr; }
__device__ __forceinline__ const double *sweep_box(const BoxedSweepArgs &a, int64_t q) { return a.box + q * kRefineBoxStride; }

// 1/a to 2.2e-15 relative: v_rcp_f64 seed (measured 4.6e-8, tools/rcp_accuracy_probe.hip) + ONE
// Newton step.  a must be finite and normal, and so must 1/a (NaN for a = inf, 0 once 1/a is
// subnormal): k_prepare keeps non-positive and NaN noise variances out of the sweeps (status 3) and
// those above 1e100 out of the K-loop (QuasarMeta::ll_bias).  A second step would make it correctly rounded at
// two more fp64 instructions per use -- two uses per K-step of the sweep, 4 % of its VALU work.
// What 2e-15 costs: the optical depth moves by 2e-15 relative (absorption by <= 8e-16 absolute),
// Sum r^2/d by <= 2e-15 |Sum r^2/d| ~ 1e-11..1e-10, log det B by <= k 2e-15: two orders below the
// 1e-8 parity tolerance (GPU tests observe <= 3e-10 against the oracle and the 50-digit values).
__device__ __forceinline__ double fast_rcp(double a) {
  const double r = __builtin_amdgcn_rcp(a);
  const double e = fma(-a, r, 1.0);
  return fma(r, e, r);
}

// exp(x) for x <= 0 (optical depths): x = n ln2 + r, |r| <= ln2/2, degree-12 Taylor, ldexp.
__device__ __forceinline__ double exp_nonpos(double x) {
  x = fmax(x, -800.0);  // exp(-800) = 0 in fp64; keeps n in int range
  const double n = rint(x * 1.4426950408889634);
  double r = fma(-n, 0.6931471803691238, x);      // ln2 high part (trailing bits zero)
  r = fma(-n, 1.9082149292705877e-10, r);         // ln2 low part
  double p = 2.08767569878681e-09;                // 1/12!
  p = fma(p, r, 2.505210838544172e-08);           // 1/11!
  p = fma(p, r, 2.755731922398589e-07);
  p = fma(p, r, 2.755731922398589e-06);
  p = fma(p, r, 2.48015873015873e-05);
  p = fma(p, r, 0.0001984126984126984);
  p = fma(p, r, 0.001388888888888889);
  p = fma(p, r, 0.008333333333333333);
  p = fma(p, r, 0.041666666666666664);
  p = fma(p, r, 0.16666666666666666);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)n);
}

// 1/sqrt(x): v_rsq_f64 + two Newton steps (the pivots of the epilogue factorisations, epilogue_factor.hpp)
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);  // ~2^-26
  const double h = 0.5 * x;
  double err = fma(-h * y, y, 0.5);
  y = fma(y, err, y);
  err = fma(-h * y, y, 0.5);
  return fma(y, err, y);
}

// Asynchronous global -> LDS copy, 16 bytes per lane (lane l lands at lds_wave_base + 16 l).
// Issued as inline assembly on purpose: with __builtin_amdgcn_global_load_lds the compiler cannot
// tell which LDS bytes the DMA writes and puts s_waitcnt vmcnt(0) in front of EVERY later LDS read,
// i.e. the first K-step of a chunk waits for the prefetch of the next one (measured: 20 % of the
// sweep).  The kernels order these copies themselves: glds_wait() + __syncthreads() before a stage
// buffer is read, and a barrier after its last read before it is refilled.
__device__ __forceinline__ void glds16(const double *gsrc, double *lds_wave_base) {
  const uint32_t lds = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)lds_wave_base);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off"
               :
               : "v"(gsrc), "s"(lds)
               : "memory", "m0");
}
// The same copy with the source as a wave-uniform 64-bit base in scalar registers plus a 32-bit byte offset per
// lane (the instruction's SADDR form).  For a source that advances by a constant from copy to copy under a lane
// offset that never changes: the advance is then scalar arithmetic and the lane offset is formed once, where
// glds16 has the caller re-form a 64-bit address per lane (two vector adds) for every copy.
__device__ __forceinline__ const double *uniform_pointer(const double *p) {  // p is wave-uniform: say so
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const double *)(uintptr_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ void glds16_at(const double *sbase, uint32_t lane_bytes, double *lds_wave_base) {
  const uint32_t lds = __builtin_amdgcn_readfirstlane(
      (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void *)lds_wave_base);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               :
               : "v"(lane_bytes), "s"(sbase), "s"(lds)
               : "memory", "m0");
}
// s_waitcnt vmcnt(0) only (gfx9 encoding: expcnt and lgkmcnt fields at their maxima).  The builtin,
// not inline assembly: the compiler's own wait-count bookkeeping sees it and keeps its
// conservative vmcnt waits out of the loops that follow.
__device__ __forceinline__ void glds_wait() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
  asm volatile("" ::: "memory");
}

// A whole chunk, KIB KiB-blocks long, copied global -> LDS by the WAVES waves of a block.  One
// global_load_lds_dwordx4 moves 1 KiB (lane l: 16 bytes at +16 l on both sides), and the
// instruction's immediate offset moves BOTH addresses (tools/glds_offset_probe.hip), so four
// instructions share one M0 and one address register; each wave takes a contiguous span of PER
// blocks.  Per chunk and wave that is two or three vector instructions where a loop over
// (unit < units ? glds16 : skip) costs eight per block -- and non-arithmetic VALU instructions are
// MFMA time in these kernels.  The copy always moves the whole chunk: a chunk that runs past a
// quasar's last record reads the next quasar's records or the pool's padding (host_sweep.hpp allocates
// kRecordPoolPad records behind the pool), which no K-step consumes.
constexpr int kRecordPoolPad = 8;
__device__ __forceinline__ void glds_quad(const double *gsrc, uint32_t lds, int count) {
  if (count >= 4)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off\n\t"
                 "global_load_lds_dwordx4 %0, off offset:1024\n\tglobal_load_lds_dwordx4 %0, off offset:2048\n\t"
                 "global_load_lds_dwordx4 %0, off offset:3072"
                 :
                 : "v"(gsrc), "s"(lds)
                 : "memory", "m0");
  else if (count == 3)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off\n\t"
                 "global_load_lds_dwordx4 %0, off offset:1024\n\tglobal_load_lds_dwordx4 %0, off offset:2048"
                 :
                 : "v"(gsrc), "s"(lds)
                 : "memory", "m0");
  else if (count == 2)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off\n\t"
                 "global_load_lds_dwordx4 %0, off offset:1024"
                 :
                 : "v"(gsrc), "s"(lds)
                 : "memory", "m0");
  else if (count == 1)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gsrc), "s"(lds) : "memory", "m0");
}
// src: the chunk's first double in global memory; lds: byte address of its LDS buffer; wave: this
// wave's index within the block -- all three wave-uniform (scalar registers).
template <int KIB, int WAVES>
__device__ __forceinline__ void glds_chunk(const double *src, uint32_t lds, int wave, int lane) {
  constexpr int PER = (KIB + WAVES - 1) / WAVES;
  const int first = wave * PER;
  const int count = min(PER, KIB - first);  // <= 0 for waves behind the last block
  const double *p = src + (size_t)first * 128 + 2 * lane;
  const uint32_t l = lds + (uint32_t)first * 1024u;
#pragma unroll
  for (int g = 0; g < (PER + 3) / 4; ++g)
    if (count > 4 * g) glds_quad(p + g * 512, l + (uint32_t)g * 4096u, count - 4 * g);
}
// LDS byte address of a pointer into the dynamic shared array
__device__ __forceinline__ uint32_t lds_address(const void *p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}

}  // namespace gpdla
