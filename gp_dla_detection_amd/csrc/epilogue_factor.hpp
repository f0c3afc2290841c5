// epilogue_factor.hpp -- the per-sample Cholesky factorisations that end every sweep: from a sample's [vech(B) | v]
// to its log-likelihood (log_mvnpdf_low_rank.m:22-32).  factor_lds works next to LDS, factor_rows keeps a lane's rows
// in registers (k <= 20), factor_rows16 keeps a whole sample in the registers of one DPP row (20 < k <= 40);
// factor_pass is one pass of the epilogue of the kernels that hold a sample group per wave.
#pragma once
#include "sweep_primitives.hpp"

namespace gpdla {

// Epilogue shared by the sweep kernels: one round (MFMA result register r) of the per-sample
// factorisation.  The 16 lanes of row jj hold, in register r of every tile, the 16*NT columns of
// sample jj + 4r: they spill them to LDS (e = [16*NT] doubles for this row: packed lower triangle
// of B, then v at voff) and factor the augmented (k+1) x (k+1) matrix [[I + B, v], [v', .]] column
// by column (left-looking).  Row k of the augmented matrix is v, so its factor row is z = L^-1 v.
//
// Lane s of the 16 owns rows s, s+16 (, s+32) for the whole factorisation and keeps their running
// diagonals  dd_i = A_ii - Sum_{m<j} l_im^2  in registers.  Column j then needs no dot product for
// its pivot: the owner of row j broadcasts dd_j, every lane takes ONE reciprocal square root
// (v_rsq_f64 + two Newton steps: no sqrt, no division, :24 is only ever used through 1/L_jj and
// log L_jj = log(d_j)/2), and the row dot products -- which do not depend on the pivot -- run
// alongside.  -dd of row k ends as z'z.

// The factorisation proper, on one sample's columns already in LDS, by LPS lanes (s = 0..LPS-1);
// ROWS = ceil((k+1)/LPS) rows per lane at most.  Returns log N(y; a mu, ...) of that sample
// (log_mvnpdf_low_rank.m:30-32) in every lane of the group.  q_s = Sum r^2/d, ld_s = Sum log d.
template <int ROWS, int LPS>
__device__ __forceinline__ double factor_lds(double *e, int s, int k, int voff, double q_s, double ld_s,
                                          int n_kept) {
  // Columns are taken in panels of PW: the part of their dot products that involves earlier
  // panels (the bulk) is formed for the whole panel at once, so each own-row entry read from LDS
  // feeds PW multiply-adds instead of one; only the few in-panel terms follow the column-by-column
  // dependency chain.  The summation order per entry is unchanged (columns ascending).
  constexpr int PW = ROWS <= 3 ? 8 : 4;
  int ro[ROWS];
  double dd[ROWS];
#pragma unroll
  for (int a = 0; a < ROWS; ++a) {
    const int i = s + LPS * a;
    ro[a] = i < k ? i * (i + 1) / 2 : voff;        // rows beyond k alias v and are never written
    dd[a] = i < k ? e[ro[a] + i] + 1.0 : 0.0;      // log_mvnpdf_low_rank.m:22-23
  }
  double lprod = 1.0;
  int lexp = 0;
  bool pd = true;
  for (int j0 = 0; j0 < k; j0 += PW) {
    double t[ROWS][PW];
    int rp[PW];  // pivot rows of the panel (clamped in the last, partial panel: those columns are unused)
#pragma unroll
    for (int c = 0; c < PW; ++c) {
      const int j = min(j0 + c, k - 1);
      rp[c] = j * (j + 1) / 2;
#pragma unroll
      for (int a = 0; a < ROWS; ++a) t[a][c] = e[ro[a] + j0 + c];
    }
#pragma unroll 2
    for (int mm = 0; mm < j0; ++mm) {
      double own[ROWS], piv[PW];
#pragma unroll
      for (int a = 0; a < ROWS; ++a) own[a] = e[ro[a] + mm];
#pragma unroll
      for (int c = 0; c < PW; ++c) piv[c] = e[rp[c] + mm];
#pragma unroll
      for (int a = 0; a < ROWS; ++a)
#pragma unroll
        for (int c = 0; c < PW; ++c) t[a][c] = fma(-own[a], piv[c], t[a][c]);
    }
#pragma unroll
    for (int c = 0; c < PW; ++c) {
      const int j = j0 + c;
      if (j < k) {  // block-uniform
#pragma unroll
        for (int cp = 0; cp < c; ++cp) {  // in-panel terms: own entries are still in registers
          const double pv = e[rp[c] + j0 + cp];
#pragma unroll
          for (int a = 0; a < ROWS; ++a) t[a][c] = fma(-t[a][cp], pv, t[a][c]);
        }
        double dsel = dd[0];
#pragma unroll
        for (int a = 1; a < ROWS; ++a)
          if (j >= LPS * a) dsel = dd[a];
        const double dj = __shfl(dsel, j & (LPS - 1), LPS);  // pivot, from the lane that owns row j
        pd = pd && (dj > 0.0);                         // chol would throw here (:24)
        const double inv = rsqrt_nr(dj);
        lprod *= dj;                                   // 2 Sum log L_jj = log Prod d_j (:30)
        lexp += __builtin_amdgcn_frexp_exp(lprod);
        lprod = __builtin_amdgcn_frexp_mant(lprod);
#pragma unroll
        for (int a = 0; a < ROWS; ++a) {
          const int i = s + LPS * a;
          t[a][c] *= inv;
          if (i > j && i <= k) {
            e[ro[a] + j] = t[a][c];
            dd[a] = fma(-t[a][c], t[a][c], dd[a]);
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  double zsel = dd[0];
#pragma unroll
  for (int a = 1; a < ROWS; ++a)
    if (k >= LPS * a) zsel = dd[a];
  const double zz = -__shfl(zsel, k & (LPS - 1), LPS);  // z'z with z = L^-1 v
  const double log_det = ld_s + log(lprod) + (double)lexp * 0.6931471805599453;  // :30
  const double ll = -0.5 * ((q_s - zz) + log_det + (double)n_kept * kLog2Pi);    // :32
  return pd ? ll : NAN;
}

// The same factorisation with each lane's own rows held in registers (k <= KMAX known at compile
// time, column loop fully unrolled).  The LDS version reads, for every column, the lane's three
// rows AND the pivot row -- 4 streams, 300 KB per wave and pass, which made the epilogue LDS
// bandwidth-bound; here only the pivot row (a broadcast within the sample's lanes) comes from LDS,
// at compile-time offsets.  Same operation order, so results are bit-identical to factor_lds.
template <int ROWS, int LPS, int KMAX>
__device__ __forceinline__ double factor_rows(double *e, int s, int k, int voff, double q_s, double ld_s,
                                           int n_kept) {
  int ro[ROWS];
  double dd[ROWS];
  double rc[ROWS][KMAX];  // rc[a][m] = entry (row s + LPS a, column m): A before column m, L after
#pragma unroll
  for (int a = 0; a < ROWS; ++a) {
    const int i = s + LPS * a;
    ro[a] = i < k ? i * (i + 1) / 2 : voff;        // rows beyond k alias v and are never written
    dd[a] = i < k ? e[ro[a] + i] + 1.0 : 0.0;      // log_mvnpdf_low_rank.m:22-23
#pragma unroll
    for (int m = 0; m < KMAX; ++m) rc[a][m] = e[ro[a] + m];  // (columns >= the row index: unused)
  }
  double lprod = 1.0;
  int lexp = 0;
  bool pd = true;
#pragma unroll
  for (int j = 0; j < KMAX; ++j) {
    if (j < k) {  // block-uniform
      const int rj = j * (j + 1) / 2;
      double dsel = dd[0];
#pragma unroll
      for (int a = 1; a < ROWS; ++a)
        if (j >= LPS * a) dsel = dd[a];
      const double dj = __shfl(dsel, j & (LPS - 1), LPS);  // pivot, from the lane that owns row j
      double t[ROWS];
#pragma unroll
      for (int a = 0; a < ROWS; ++a) t[a] = rc[a][j];
#pragma unroll
      for (int mm = 0; mm < j; ++mm) {
        const double c = e[rj + mm];
#pragma unroll
        for (int a = 0; a < ROWS; ++a) t[a] = fma(-rc[a][mm], c, t[a]);
      }
      pd = pd && (dj > 0.0);                         // chol would throw here (:24)
      const double inv = rsqrt_nr(dj);
      lprod *= dj;                                   // 2 Sum log L_jj = log Prod d_j (:30)
      lexp += __builtin_amdgcn_frexp_exp(lprod);
      lprod = __builtin_amdgcn_frexp_mant(lprod);
#pragma unroll
      for (int a = 0; a < ROWS; ++a) {
        const int i = s + LPS * a;
        t[a] *= inv;
        rc[a][j] = t[a];
        if (i > j && i <= k) {
          e[ro[a] + j] = t[a];                       // row i becomes a pivot row later
          dd[a] = fma(-t[a], t[a], dd[a]);
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
  }
  double zsel = dd[0];
#pragma unroll
  for (int a = 1; a < ROWS; ++a)
    if (k >= LPS * a) zsel = dd[a];
  const double zz = -__shfl(zsel, k & (LPS - 1), LPS);  // z'z with z = L^-1 v
  const double log_det = ld_s + log(lprod) + (double)lexp * 0.6931471805599453;  // :30
  const double ll = -0.5 * ((q_s - zz) + log_det + (double)n_kept * kLog2Pi);    // :32
  return pd ? ll : NAN;
}

// t += (-p[lane n of this lane's 16-lane row]) * r in one instruction: the DPP form of the fp64
// multiply-add broadcasts its first source across a row of 16 lanes (row_newbcast, the only DPP
// control the 64-bit ALU knows).  Bit for bit fma(-p_n, r, t) and the same issue cost as the plain
// instruction (tools/dpp_f64_probe.hip).  p must not have been written by a VALU instruction in
// the two instructions before (DPP hazard; nothing pads inline assembly): here p always comes
// straight from an LDS read, and tools/check_dpp_hazard.py checks the ISA of a build.
template <int N, bool PAD = false>
__device__ __forceinline__ void fmac_bcast(double &t, double p, double r) {
  if constexpr (PAD)  // p may have been written by the instruction before: two wait states by hand
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(t) : "v"(p), "v"(r), "n"(N));
  else
    asm("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(t) : "v"(p), "v"(r), "n"(N));
}

// p[lane N of this lane's 16-lane row] (same hazard rule)
template <int N, bool PAD = false>
__device__ __forceinline__ double mov_bcast(double p) {
  double d;
  if constexpr (PAD)
    asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(p), "n"(N));
  else
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(p), "n"(N));
  return d;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a constant
// expression in the body (the DPP lane above is an instruction field)
template <int... I, typename F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, I...>, F &&f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_seq(std::make_integer_sequence<int, N>{}, static_cast<F &&>(f));
}

// The factorisation of the 20 < k <= 40 classes with NOTHING in LDS: one sample on the 16 lanes of
// one DPP row, all its k + 1 rows in registers.  Lane l owns rows l (l < RA = KMAX - 31 = 9), RA + l
// and RA + 16 + l -- three slots whose rows need 8, 24 and 40 columns: 72 entries per lane.  Every
// row a column step needs from another lane -- the pivot row's entries, the pivot itself -- lives
// in a register of the SAME 16-lane row, so the DPP broadcast takes it straight from its owner's
// register (fmac_bcast / mov_bcast with the owner's lane as a compile-time field): no LDS traffic,
// no masked stores, no panels, and a slot's multiply-adds stop once its rows are finished
// (1084 per column sweep at k = 40 for FOUR samples per wave; factor_lds<2, 32>: 1640 for two).  A
// block's 32 samples therefore factor in ONE round, four per wave; LDS only transposes the
// accumulators into rows (load_rows16 reads what the spill laid down, 16 samples at a time).
// Entry by entry the operations and their order are those of factor_lds: bit-identical results.
template <int KMAX> struct Rows16 {
  static constexpr int RA = KMAX + 1 - 32;
  static constexpr int NA = RA - 1, NB = RA + 15, NC = KMAX;  // columns the rows of a slot need
  static_assert(RA >= 2 && RA <= 16, "three slots of at most 16 rows");
  double a[NA], b[NB], c[NC];  // entry (row, column m): A before column m, L after
  double da, db, dc;           // running diagonals dd_i = A_ii + 1 - Sum_{m<j} l_im^2 (row k: -z'z)
};

// e: the sample's spilled columns (packed lower triangle of B, then v at voff), l = 0..15
template <int KMAX>
__device__ __forceinline__ void load_rows16(Rows16<KMAX> &R, const double *e, int l, int k, int voff) {
  using RR = Rows16<KMAX>;
  const int ia = l, ib = RR::RA + l, ic = RR::RA + 16 + l;
  // rows beyond k do not exist and row k is v: both read v's storage (the former compute a copy of
  // z nobody looks at)
  const bool fa = l < RR::RA && ia < k, fb = ib < k, fc = ic < k;
  const int roa = fa ? ia * (ia + 1) / 2 : voff, rob = fb ? ib * (ib + 1) / 2 : voff, roc = fc ? ic * (ic + 1) / 2 : voff;
  R.da = fa ? e[roa + ia] + 1.0 : 0.0;  // log_mvnpdf_low_rank.m:22-23
  R.db = fb ? e[rob + ib] + 1.0 : 0.0;
  R.dc = fc ? e[roc + ic] + 1.0 : 0.0;
#pragma unroll
  for (int m = 0; m < RR::NA; ++m) R.a[m] = e[roa + m];
#pragma unroll
  for (int m = 0; m < RR::NB; ++m) R.b[m] = e[rob + m];
#pragma unroll
  for (int m = 0; m < RR::NC; ++m) R.c[m] = e[roc + m];  // (columns >= the row index: unused)
}

// Returns log N(y; a mu, ...) of the sample (log_mvnpdf_low_rank.m:30-32) in each of its 16 lanes.
template <int KMAX>
__device__ __forceinline__ double factor_rows16(Rows16<KMAX> &R, int k, double q_s, double ld_s, int n_kept) {
  using RR = Rows16<KMAX>;
  double lprod = 1.0;
  int lexp = 0;
  bool pd = true;
  static_for<KMAX>([&](auto J_) __attribute__((always_inline)) {
    constexpr int j = decltype(J_)::value;
    if (j < k) {  // block-uniform
      constexpr int slot = j < RR::RA ? 0 : j < RR::RA + 16 ? 1 : 2;         // where row j lives ...
      constexpr int ol = j - (slot == 0 ? 0 : slot == 1 ? RR::RA : RR::RA + 16);  // ... and in which lane
      constexpr bool act_a = j < RR::NA, act_b = j < RR::NB;  // some row of the slot is still below row j
      static_for<j>([&](auto M_) __attribute__((always_inline)) {
        constexpr int mm = decltype(M_)::value;
        constexpr bool fresh = mm == j - 1;  // the pivot row's newest entry was scaled one column step ago
        double piv;
        if constexpr (slot == 0) piv = R.a[mm];
        else if constexpr (slot == 1) piv = R.b[mm];
        else piv = R.c[mm];
        if constexpr (act_a) fmac_bcast<ol, fresh>(R.a[j], piv, R.a[mm]);
        if constexpr (act_b) fmac_bcast<ol, fresh>(R.b[j], piv, R.b[mm]);
        fmac_bcast<ol, fresh>(R.c[j], piv, R.c[mm]);
      });
      double dsel;
      if constexpr (slot == 0) dsel = R.da;
      else if constexpr (slot == 1) dsel = R.db;
      else dsel = R.dc;
      const double dj = mov_bcast<ol, true>(dsel);     // pivot
      pd = pd && (dj > 0.0);                           // chol would throw here (:24)
      const double inv = rsqrt_nr(dj);
      lprod *= dj;                                     // 2 Sum log L_jj = log Prod d_j (:30)
      if constexpr ((j & 3) == 3) {  // (scaling by powers of two is exact: every fourth column gives the same bits)
        lexp += __builtin_amdgcn_frexp_exp(lprod);
        lprod = __builtin_amdgcn_frexp_mant(lprod);
      }
      if constexpr (act_a) {
        R.a[j] *= inv;
        R.da = fma(-R.a[j], R.a[j], R.da);             // (a finished row's dd is dead)
      }
      if constexpr (act_b) {
        R.b[j] *= inv;
        R.db = fma(-R.b[j], R.b[j], R.db);
      }
      R.c[j] *= inv;
      R.dc = fma(-R.c[j], R.c[j], R.dc);
    }
  });
  lexp += __builtin_amdgcn_frexp_exp(lprod);  // (k need not be a multiple of four)
  lprod = __builtin_amdgcn_frexp_mant(lprod);
  // row k: -dd ends as z'z with z = L^-1 v
  const double zz = -(k >= RR::RA + 16 ? __shfl(R.dc, k - RR::RA - 16, 16) : __shfl(R.db, k - RR::RA, 16));
  const double log_det = ld_s + log(lprod) + (double)lexp * 0.6931471805599453;  // :30
  const double ll = -0.5 * ((q_s - zz) + log_det + (double)n_kept * kLog2Pi);    // :32
  return pd ? ll : NAN;
}

// Samples factored per pass by one wave (and LDS rows of 16*NT doubles it needs for them): 8 lanes
// per sample, i.e. 8 samples = two MFMA result registers per pass, with three rows per lane for
// k <= 20 (TW = 14) and six for k <= 40 (TW = 52).  The factorisation is a latency chain of k
// column steps per pass, so fewer, fatter passes win.
template <int TW, int TS> struct EpilogueShape {
  // (k <= 40 without a tile split -- the fp32 study kernel, one wave per sample group -- keeps 16
  // lanes per sample: 8 samples x 56 tiles per wave would not fit the LDS)
  static constexpr int LPS = (TW > 30 && TS == 1) ? 16 : 8;  // lanes per sample
  static constexpr int RPP = 16 / LPS;               // MFMA result registers per pass
  static constexpr int PASSES = 4 / RPP;
  static constexpr int SPP = 4 * RPP;                // samples per pass
  static constexpr int ROWS = TW > 30 ? 48 / LPS : 3;  // ceil(41/LPS); ceil(21/8)
  // LDS doubles per sample: its 16*NT columns + 4.  Without the pad every sample's copy of a row
  // starts on the same bank (16*NT*8 bytes is a multiple of the 256-byte bank cycle) and the SPP
  // samples a wave factors at once conflict SPP-way on every read; +32 bytes staggers them.
  static constexpr int stride(int nt) { return nt * 16 + 4; }
};

// One epilogue pass: spill the result registers RPP*p .. of every tile (the 16 lanes of row jj
// hold, in register r, the 16*NT columns of sample sample_of(jj, r)) to LDS and factor them.
// Returns the sample's log-likelihood; *sigma_out = its index among the wave's 16, *writer = this
// lane is the one that stores it.
// xw / xu: the compact class's columns accumulated off the matrix cores (sample s = lane & 15 of
// the wave, already summed over the four pixel phases); ignored otherwise.
template <typename T, int NTW, int TS, int TW, typename ACC>
__device__ __forceinline__ double factor_pass(const ACC (&acc)[NTW], const double (&xw)[kXW],
                                              const double (&xu)[kXU], int p, double *Eg, int lane,
                                              int role, int tile0, int k, double quad_sum,
                                              double logd_sum, int n_kept, int *sigma_out,
                                              bool *writer) {
  using ES = EpilogueShape<TW, TS>;
  constexpr bool compact = tiles_compact(NTW * TS);
  constexpr int voff = (TW + (compact ? 1 : 0)) * 16;  // v behind the vech columns (210 <= 224 when compact)
  constexpr int ncols = ES::stride(logical_tiles(NTW * TS));
  const int s = lane & 15, jj = lane >> 4;
  const int half = ES::RPP == 2 ? (s >> 3) : 0;
  const int sigma = Mat<T>::sample_of(jj, ES::RPP * p + half);
  // the sample's scalar sums live in the lanes whose s equals sigma
  const double q_s = __shfl(quad_sum, sigma + 16 * jj);
  const double ld_s = __shfl(logd_sum, sigma + 16 * jj);
  double *e = Eg + (size_t)(jj * ES::RPP) * ncols;
  if (TS > 1) __syncthreads();
#pragma unroll
  for (int cc = 0; cc < NTW; ++cc) {
    const int tile = tile0 + cc;
    const int col0 = tile < TW ? tile * 16 : voff + (tile - TW) * 16;  // w-tiles, then u-tiles at voff
#pragma unroll
    for (int h = 0; h < ES::RPP; ++h) e[h * ncols + col0 + s] = (double)acc[cc][ES::RPP * p + h];
  }
  if (compact) {
    // lane (s, jj = 0) holds sample s of the wave; it is factored in pass reg/RPP from the LDS row
    // of lane group jj_of(s), half reg % RPP
    const int r = Mat<T>::reg_of(s);
    if (jj == 0 && r / ES::RPP == p) {
      double *es = Eg + (size_t)(Mat<T>::jj_of(s) * ES::RPP + r % ES::RPP) * ncols;
#pragma unroll
      for (int x = 0; x < kXW; ++x) es[kXWColumn + x] = xw[x];
#pragma unroll
      for (int x = 0; x < kXU; ++x) es[voff + kXUColumn + x] = xu[x];
    }
  }
  if (TS > 1) __syncthreads();
  else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  *sigma_out = sigma;
  *writer = role == 0 && (s & (ES::LPS - 1)) == 0;
  if (role != 0) return NAN;
  if (TW <= 14)  // k <= 20: own rows in registers
    return factor_rows<ES::ROWS, ES::LPS, 20>(e + half * ncols, s & (ES::LPS - 1), k, voff, q_s, ld_s, n_kept);
  if constexpr (TW > 30 && ES::LPS == 16) {
    // k <= 40 without a tile split (the fp32 study kernel): a sample is on the 16 lanes of one DPP
    // row already -- all its rows in registers, nothing read from LDS after the spill (factor_rows16)
    Rows16<40> R;
    load_rows16<40>(R, e, s, k, voff);
    return factor_rows16<40>(R, k, q_s, ld_s, n_kept);
  }
  return factor_lds<ES::ROWS, ES::LPS>(e + half * ncols, s & (ES::LPS - 1), k, voff, q_s, ld_s, n_kept);
}

}  // namespace gpdla
