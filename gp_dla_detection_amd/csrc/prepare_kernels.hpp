// prepare_kernels.hpp -- what runs once per batch before any sweep (reference lines they replace; paths relative to
// the reference tree):
//   k_prepare   process_qsos.m:102-119, 138-146, 159-176   per-quasar pixel selection, GP
//                                                          interpolation, noise scaling, padding
//   k_build_records (no reference counterpart)              packs vech(m m') | m per pixel into MFMA
//                                                          B-operand tiles + the per-pixel vectors
#pragma once
#include "batch_types.hpp"

namespace gpdla {

// ------------------------------------------------------------------------------------------
// k_prepare: one 256-thread block per quasar.
// ------------------------------------------------------------------------------------------
struct PrepareArgs {
  int64_t nq;
  const int64_t *offsets;
  const double *wavelengths, *flux, *noise_variance;
  const uint8_t *pixel_mask;
  const double *z_qsos;
  ModelDev model;
  Config cfg;
  QuasarMeta *meta;        // [nq]  pix_off / lam_off pre-filled by the host
  PixelRow *pix;           // pool
  double *Mi;              // pool [row][k] interpolated (and zeroed for masked rows) M
  double *lam_pad;         // pool
  const int64_t *rec_off;  // [nq] record-pool offsets planned by the host (host_sweep.hpp plan_records)
  // multi-DLA driver only (process_qsos_multiple_dlas_meanflux.m:245-293): Lyman-series noise
  // scaling and mean-flux suppression of mu, M, omega2
  int32_t multi;
  int32_t num_forest_lines;
  double prev_tau_0, prev_beta;
};

__global__ __launch_bounds__(256) void k_prepare(PrepareArgs a) {
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ int s_cnt[4];
  __shared__ int s_base;
  __shared__ double s_red[4];
  const int64_t base = a.offsets[q];
  const int npix = (int)(a.offsets[q + 1] - base);
  const double z_qso = a.z_qsos[q];
  QuasarMeta m = a.meta[q];
  PixelRow *pix = a.pix + m.pix_off;
  double *Mi = a.Mi + m.pix_off * a.model.k;
  double *lam = a.lam_pad + m.lam_off;
  const int k = a.model.k, G = a.model.G;
  if (tid == 0) s_base = 0;
  __syncthreads();
  double kept_min = INFINITY, kept_max = -INFINITY, un_min = INFINITY, un_max = -INFINITY;
  int kept_count = 0;
  int nv_flags = 0;  // 1: a kept pixel with noise variance +inf; 2: one with variance <= 0 or NaN
  double huge_nv_ll = 0.0;  // -log(nu)/2 of the kept pixels of finite variance above kNeutralNoiseVariance
  for (int tile = 0; tile < npix; tile += 256) {
    const int i = tile + tid;
    double wl = 0.0, rest = 0.0;
    bool in_range = false;
    if (i < npix) {
      wl = a.wavelengths[base + i];
      rest = wl / (1 + z_qso);                                             // process_qsos.m:102
      in_range = (rest >= a.cfg.min_lambda) && (rest <= a.cfg.max_lambda); // :104-105
    }
    const unsigned long long bal = __ballot(in_range);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int wbase = s_base, total = 0;
    for (int w = 0; w < 4; ++w) {
      if (w < wave) wbase += s_cnt[w];
      total += s_cnt[w];
    }
    if (in_range) {
      const int u = wbase + pre;  // order-preserving index on the unmasked grid (:108)
      lam[3 + u] = wl;
      un_min = fmin(un_min, wl);
      un_max = fmax(un_max, wl);
      const bool keep = a.pixel_mask[base + i] == 0;                       // :110, :181
      PixelRow row = {0.0, 0.0, 0.0, 1.0};  // masked: contributes r = 0, d = 1, zero B-operand row
      double mf = 1.0;                       // mean-flux factor applied to mu and M (multi only)
      // bracket rest in the model grid (griddedInterpolant 'linear', :66-71)
      int lo = 0, hi = G - 1;
      if (rest >= a.model.rest[G - 1]) lo = G - 2;
      else if (rest > a.model.rest[0]) {
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (a.model.rest[mid] <= rest) lo = mid; else hi = mid;
        }
      }
      const double t = (rest - a.model.rest[lo]) / (a.model.rest[lo + 1] - a.model.rest[lo]);
      if (keep) {
        kept_count++;
        kept_min = fmin(kept_min, wl);
        kept_max = fmax(kept_max, wl);
        row.y = a.flux[base + i];
        row.nu = a.noise_variance[base + i];
        if (!(row.nu > 0.0)) nv_flags |= 2;  // the reference's result is undefined (log of d <= 0, 0/0)
        else if (row.nu == INFINITY) nv_flags |= 1;
        row.mu = a.model.mu[lo] + (a.model.mu[lo + 1] - a.model.mu[lo]) * t;          // :138
        const double lo_om = a.model.log_omega[lo] +
                             (a.model.log_omega[lo + 1] - a.model.log_omega[lo]) * t;  // :141
        const double omega2 = exp(2 * lo_om);                                          // :142
        const double lya_z = (wl - a.cfg.lya_wavelength) / a.cfg.lya_wavelength;       // :117-119
        if (!a.multi) {
          const double sc = 1 - exp(-a.model.tau_0 * pow(1 + lya_z, a.model.beta)) + a.model.c_0; // :144
          row.omega2 = omega2 * (sc * sc);                                             // :146
        } else {
          // multi :245-263: effective optical depth of the whole Lyman series in the noise model
          const double wl_1 = g_lines.wavelength_cm[0] * 1e8, f_1 = g_lines.osc[0];
          double depth = a.model.tau_0 * pow(1 + lya_z, a.model.beta);
          for (int l = 1; l < a.num_forest_lines; ++l) {
            const double wl_l = g_lines.wavelength_cm[l] * 1e8;
            double one_pz = wl_1 * (1 + lya_z) / wl_l;                                 // multi :248-249
            one_pz = one_pz * ((one_pz <= (1 + z_qso)) ? 1.0 : 0.0);                   // multi :252-253
            const double tau = a.model.tau_0 * wl_l * g_lines.osc[l] / (wl_1 * f_1);   // multi :255-256
            depth = depth + tau * pow(one_pz, a.model.beta);                           // multi :258
          }
          const double sc = 1 - exp(-depth) + a.model.c_0;                             // multi :261
          double om = omega2 * (sc * sc);                                              // multi :263
          // multi :267-285: mean-flux suppression exp(-Sum tau_l (1+z_l)^beta) with Kim's priors
          double total = 0.0;
          for (int l = 0; l < a.num_forest_lines; ++l) {
            const double wl_l = g_lines.wavelength_cm[l] * 1e8;
            const double z_l = (wl - wl_l) / wl_l;                                     // multi :184-186
            const double tau_l = a.prev_tau_0 * g_lines.osc[l] / f_1 * wl_l / a.cfg.lya_wavelength;
            const double od = tau_l * pow(1 + z_l, a.prev_beta);                       // multi :275-276
            if (l > 0 && z_l > z_qso) continue;                                        // multi :279-282
            total += od;
          }
          mf = exp(-total);                                                            // multi :285
          row.mu = row.mu * mf;                                                        // multi :287
          row.omega2 = om * (mf * mf);                                                 // multi :293
        }
      }
      // a kept pixel of huge or infinite variance weighs (next to) nothing but log d is large or
      // inf: it is swept as a neutral row and its effect re-enters through ll_bias (unless its flux
      // is NaN, which the reference propagates into every result: then the row is left as it is)
      const bool huge_nv = keep && row.nu > kNeutralNoiseVariance && row.y == row.y;
      if (huge_nv) {
        if (row.nu != INFINITY) huge_nv_ll -= 0.5 * log(row.nu);
        row = PixelRow{0.0, 0.0, 0.0, 1.0};
      }
      pix[u] = row;
      for (int c = 0; c < k; ++c) {                                                    // :139
        const double m0 = a.model.M[lo + (int64_t)c * G], m1 = a.model.M[lo + 1 + (int64_t)c * G];
        Mi[(int64_t)u * k + c] = (keep && !huge_nv) ? (m0 + (m1 - m0) * t) * mf : 0.0;  // multi :288
      }
    }
    __syncthreads();
    if (tid == 0) s_base += total;
    __syncthreads();
  }
  const int n_u = s_base;
  // block reductions
  int kc = kept_count;
  for (int o = 32; o > 0; o >>= 1) kc += __shfl_xor(kc, o);
  __syncthreads();
  if (lane == 0) s_cnt[wave] = kc;
  __syncthreads();
  const int n_kept = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  kept_min = block_reduce_minmax(kept_min, true, s_red);
  kept_max = block_reduce_minmax(kept_max, false, s_red);
  un_min = block_reduce_minmax(un_min, true, s_red);
  un_max = block_reduce_minmax(un_max, false, s_red);
  huge_nv_ll = block_reduce_sum(huge_nv_ll, s_red);
  nv_flags = __syncthreads_or(nv_flags & 1) | (__syncthreads_or(nv_flags & 2) ? 2 : 0);
  const int steps = (n_u + 3) >> 2;
  // pad rows up to 4*(steps+1): neutral pixels (the last 4 feed the neutral trailing record)
  for (int u = n_u + tid; u < 4 * steps + 4; u += 256) {
    pix[u] = PixelRow{0.0, 0.0, 0.0, 1.0};
    for (int c = 0; c < k; ++c) Mi[(int64_t)u * k + c] = 0.0;
  }
  if (tid == 0) {
    m.n_u = n_u;
    m.n_kept = n_kept;
    m.steps = steps;
    m.status = (n_kept > 0) ? ((nv_flags & 2) ? 3 : 0) : 1;
    m.rec_off = a.rec_off[q];
    m.ll_bias = (nv_flags & 1) ? -INFINITY : huge_nv_ll;
    if (n_kept > 0) {
      // set_parameters.m:65-73 on the kept-pixel wavelengths (process_qsos.m:159-160)
      m.max_z_dla = (kept_max / a.cfg.lya_wavelength - 1) - a.cfg.max_z_cut;
      const double za = kept_min / a.cfg.lya_wavelength - 1;
      const double zb = a.cfg.lyman_limit * (1 + z_qso) / a.cfg.lya_wavelength - 1 + a.cfg.min_z_cut;
      m.min_z_dla = fmax(za, zb);
      // process_qsos.m:168-176: logspace(a, b, 3) = 10.^[a, a + (b-a)/2, b]
      const double lo = log10(un_min), hi = log10(un_max), ps = a.cfg.pixel_spacing;
      const double a0 = lo - 3 * ps, b0 = lo - ps, a1 = hi + ps, b1 = hi + 3 * ps;
      lam[0] = pow(10.0, a0);
      lam[1] = pow(10.0, a0 + 1.0 * (b0 - a0) / 2.0);
      lam[2] = pow(10.0, b0);
      lam[3 + n_u] = pow(10.0, a1);
      lam[4 + n_u] = pow(10.0, a1 + 1.0 * (b1 - a1) / 2.0);
      lam[5 + n_u] = pow(10.0, b1);
    } else {
      m.min_z_dla = m.max_z_dla = NAN;
    }
    a.meta[q] = m;
  }
}

// ------------------------------------------------------------------------------------------
// k_build_records: everything one K-step of the sweep reads, packed contiguously so that a
// chunk of steps is ONE linear global->LDS DMA (global_load_lds_dwordx4).
//
// record(q, t) = RD doubles, RD = ntiles*64 + 32:
//   [0, ntiles*64)   B-operand tiles.  Tile c, lane l = 16*jj + col holds, for pixel 4t + jj,
//                    column 16c + col of [vech(m m') | m]  (row-wise lower triangle:
//                    idx(i, j) = i(i+1)/2 + j, j <= i).  The first tiles_w = ceil(k(k+1)/2 / 16)
//                    tiles take the weight w, the following ceil(k/16) tiles take u.
//   [+0, +16)        PixelRow (y, mu, omega2, nu) of pixels 4t .. 4t+3
//   [+16, +20)       padded wavelengths 4(t+3) .. 4(t+3)+3 (the raw profile runs three steps ahead)
// Record `steps` (one past the last K-step) is neutral: zero tiles, (y, mu, omega2, nu) = (0,0,0,1).
//   [+20, +32)       unused (keeps records 16-byte granular and 256-byte aligned)
// compact class (record_extras == 64) instead: one 16-double block per pixel jj at +16 jj, so that
// a lane of the sweep reaches all of its operands from ONE address (see k_sweep on LDS offsets):
//   +0 .. +3   PixelRow (y, mu, omega2, nu) of pixel 4t + jj
//   +4 .. +7   m columns 16 .. 19 of that pixel
//   +8, +9     vech columns 208, 209 of that pixel
//   +10        padded wavelength 4(t+3) + jj
//   +11 .. +15 unused
// ------------------------------------------------------------------------------------------
struct BuildRecordsArgs {
  const QuasarMeta *meta;
  const PixelRow *pix;
  const double *Mi;
  const double *lam_pad;
  double *records;        // pool, record index = pix_off/4 + step
  int32_t k, tiles_w, ntiles;
  int32_t blocks_per_quasar;
  int32_t f32_tiles;      // 1: tiles stored as float (the fp32-contraction study), 0: double
  const int32_t *order;   // the records of quasars order[0 .. grid / blocks_per_quasar) are built
};

__global__ __launch_bounds__(256) void k_build_records(BuildRecordsArgs a) {
  // One block builds whole records (steps bq, bq + blocks_per_quasar, ...): the four M rows of a
  // step are staged in LDS, the (i, j) of every vech column comes from a table built once per
  // block, and every thread writes 16 bytes at a time -- the kernel is a pure HBM write stream.
  constexpr int SB = 8;  // steps staged per pair of barriers
  __shared__ double s_rows[SB * 4][GPDLA_MAX_K];
  __shared__ uint8_t s_vi[52 * 16], s_vj[52 * 16];
  const int q = a.order[blockIdx.x / a.blocks_per_quasar];
  const int bq = blockIdx.x % a.blocks_per_quasar;
  const QuasarMeta m = a.meta[q];
  const int tid = threadIdx.x;
  const int RD = record_doubles(a.ntiles, a.f32_tiles);
  const int xtra = record_extras(a.ntiles);
  const int ncol_w = a.k * (a.k + 1) / 2;
  const int n_pad = m.n_u + 6;
  const int k = a.k;
  for (int c = tid; c < a.tiles_w * 16; c += 256) {
    int i = 0, j = 0;
    if (c < ncol_w) {
      i = (int)((sqrt(8.0 * c + 1.0) - 1.0) * 0.5);
      while ((i + 1) * (i + 2) / 2 <= c) ++i;
      while (i * (i + 1) / 2 > c) --i;
      j = c - i * (i + 1) / 2;
    }
    s_vi[c] = (uint8_t)i;
    s_vj[c] = (uint8_t)j;
  }
  double *out = a.records + m.rec_off * (int64_t)RD;
  const int nrec = m.steps + 1;  // record `steps` is the neutral trailing one
  for (int step0 = bq * SB; step0 < nrec; step0 += a.blocks_per_quasar * SB) {
    const int nst = min(SB, nrec - step0);
    __syncthreads();  // previous rows consumed (and, first time, the table complete)
    for (int e = tid; e < nst * 4 * k; e += 256)  // rows 4 step0 .. of Mi are contiguous
      s_rows[e / k][e % k] = a.Mi[(m.pix_off + 4 * (int64_t)step0) * k + e];
    __syncthreads();
    const int per = a.ntiles * 32;  // 16-byte units of tiles per record
    for (int u = tid; u < nst * per; u += 256) {
      const int ls = u / per, rem = 2 * (u - ls * per);  // two neighbouring columns of one pixel
      const int tile = rem >> 6, l = rem & 63;
      const int jj = l >> 4, col = l & 15;
      const double *row = s_rows[ls * 4 + jj];
      double v0 = 0.0, v1 = 0.0;
      if (tile < a.tiles_w) {
        const int c = tile * 16 + col;
        if (c < ncol_w) v0 = row[s_vi[c]] * row[s_vj[c]];
        if (c + 1 < ncol_w) v1 = row[s_vi[c + 1]] * row[s_vj[c + 1]];
      } else {
        const int c = (tile - a.tiles_w) * 16 + col;
        if (c < k) v0 = row[c];
        if (c + 1 < k) v1 = row[c + 1];
      }
      double *rec = out + (int64_t)(step0 + ls) * RD;
      if (a.f32_tiles) *reinterpret_cast<float2 *>(reinterpret_cast<float *>(rec) + rem) = make_float2((float)v0, (float)v1);
      else *reinterpret_cast<double2 *>(rec + rem) = make_double2(v0, v1);
    }
    for (int e = tid; e < nst * xtra; e += 256) {
      const int ls = e / xtra, r2 = e - ls * xtra;
      const int step = step0 + ls;
      double v = 0.0;
      // (pixel, field): field 0..3 PixelRow, 4 wavelength, 5..8 m columns 16.., 9, 10 vech 208, 209
      int jj = -1, f = 0;
      if (tiles_compact(a.ntiles)) {  // compact class: per-pixel blocks
        const int o = r2 & 15;
        jj = r2 >> 4;
        f = o < 4 ? o : o < 4 + kXU ? 5 + (o - 4) : o < 4 + kXU + kXW ? 9 + (o - 4 - kXU) : o == 10 ? 4 : -1;
        static_assert(kExtrasXU == 4 && kExtrasXW == 4 + kXU && 4 + kXU + kXW == 10, "block layout");
      } else if (r2 < 16) {
        jj = r2 >> 2;
        f = r2 & 3;
      } else if (r2 < 20) {
        jj = r2 - 16;
        f = 4;
      }
      if (jj >= 0 && f >= 0) {
        if (f < 4) {
          const PixelRow px = a.pix[m.pix_off + 4 * (int64_t)step + jj];
          v = f == 0 ? px.y : f == 1 ? px.mu : f == 2 ? px.omega2 : px.nu;
        } else if (f == 4) {
          int P = 4 * (step + 3) + jj;
          if (P > n_pad - 1) P = n_pad - 1;
          v = a.lam_pad[m.lam_off + P];
        } else {  // compact class: the columns kept off the matrix cores
          const double *row = s_rows[ls * 4 + jj];
          if (f >= 9) {  // vech index 208 + x = (19, 18 + x)
            const int x = f - 9;
            if (kXWColumn + x < ncol_w) v = row[19] * row[18 + x];
          } else if (kXUColumn + (f - 5) < k) {
            v = row[kXUColumn + (f - 5)];
          }
        }
      }
      out[(int64_t)step * RD + RD - xtra + r2] = v;
    }
  }
}

}  // namespace gpdla
