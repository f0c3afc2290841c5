// stats_bin_body.hpp -- the kernel of the per-spectrum pass of stats_kernels.hpp, which includes this file
// TWICE inside namespace gpdla (no include guard), the way sweep_slim_kernel.hpp includes sweep_slim_body.hpp:
// as k_bin_posteriors over StatsBinArgs, and, with GPDLA_STATS_BIN_BOXED defined, as k_bin_posteriors_boxed
// over StatsBoxedArgs for the rows of a refine pass.  GPDLA_STATS_BIN_KERNEL names the kernel
// and GPDLA_STATS_BIN_ARGS its argument struct.  Two kernels from one text rather than one device body behind
// two wrappers: that form changed the instruction stream of the shipped k_bin_posteriors.
//
// The boxed form differs in two places.  Before the walk, all four waves form the row's normaliser (pass 1):
// the NaN-skipping maximum m of lambda and Sum_j exp(lambda_j - m), a thread's samples in sample order into a
// CompSum, the partials through post_block_sum; shift = m + log(Sum), NaN for a row without a finite entry or
// with +inf, which makes every p of the row NaN.  In the staging, the sample tables are the unit points: z =
// z_lo + (z_hi - z_lo) u_j through the row's own box (a.offsets = u, zmin / dz from the box), l = n_lo + (n_hi
// - n_lo) v_j (a.lnhi = v) and w = exp10(l).
__global__ __launch_bounds__(256) void GPDLA_STATS_BIN_KERNEL(GPDLA_STATS_BIN_ARGS a) {
  __shared__ double sp[kStatsTile], sz[kStatsTile], sl[kStatsTile], sw[kStatsTile];
  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#ifdef GPDLA_STATS_BIN_BOXED
  __shared__ double red[4];
  const double *row = a.lam + s * a.ld;
  const double inf = __builtin_inf();
  // pass 1, all four waves: the row's normaliser
  double mx = -inf;
  for (int64_t i = tid; i < a.S; i += 256) {
    const double l = row[i];
    if (l == l) mx = fmax(mx, l);
  }
  mx = post_block_max(mx, red);
  double shift = __builtin_nan("");
  if (mx > -inf && mx < inf) {   // block-uniform: post_block_max returns the same bits in every thread
    CompSum norm;
    for (int64_t i = tid; i < a.S; i += 256) {
      const double l = row[i];
      if (l == l) norm.add(exp(l - mx));
    }
    shift = mx + log(post_block_sum(norm.value(), red));
  }
  if (tid == 0) a.shift[s] = shift;
  const double pd = a.p_dla[s];
  const double zmin = a.boxes[4 * s + 0], dz = a.boxes[4 * s + 1] - zmin;
  const double nmin = a.boxes[4 * s + 2], dn = a.boxes[4 * s + 3] - nmin;
#else
  const double shift = a.shift[s], pd = a.p_dla[s], zmin = a.z_min[s], dz = a.z_max[s] - a.z_min[s];
  const double *row = a.sll + s * a.ld;
#endif

  const bool active = wave < a.R;
  StatsRequest rq = a.req[active ? wave : 0];
  const bool mine = active && lane < rq.nb;
  const double e_lo = mine ? a.edges[wave * (kStatsMaxBins + 1) + lane] : 0.0;
  const double e_hi = mine ? a.edges[wave * (kStatsMaxBins + 1) + lane + 1] : 0.0;
  const bool last = lane == rq.nb - 1;
  const double z_up = rq.lowzcut ? fmin(a.upper_z[s], rq.z_hi) : rq.z_hi;
  CompSum acc0, acc1;        // strict: Poisson sum; histogram: w p and w^2 (1 - p) p
  bool poison = false;       // histogram: a NaN weight at or below this bin (np.histogram's cumsum)
  int kept = 0;              // wave-uniform

  for (int64_t t0 = 0; t0 < a.S; t0 += kStatsTile) {
    const int nt = (int)((a.S - t0 < kStatsTile) ? (a.S - t0) : kStatsTile);
    __syncthreads();
    for (int j = tid; j < nt; j += 256) {
      const int64_t g = t0 + j;
      sp[j] = exp(row[g] - shift) * pd;
      sz[j] = zmin + dz * a.offsets[g];
#ifdef GPDLA_STATS_BIN_BOXED
      const double n = nmin + dn * a.lnhi[g];
      sl[j] = n;
      sw[j] = exp10(n);   // the boxed sweep's own N' (sweep_slim_body.hpp)
#else
      sl[j] = a.lnhi[g];
      sw[j] = a.w10[g];
#endif
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < nt; ++j) {     // every lane reads the same sample: LDS broadcasts
      const double p = sp[j], z = sz[j], l = sl[j];
      const double q = rq.quantity ? l : z;
      if (!rq.histogram) {
        if (!(l > rq.lnhi_lo && l < rq.lnhi_hi && z < z_up && z > rq.z_lo && p > rq.p_thresh)) continue;
        const bool inb = mine && q > e_lo && q < e_hi;
        if (p < rq.p_switch) {
          if (inb) acc0.add(p);
        } else if (__ballot(inb)) {
          if (inb && kept < kStatsKept) {
            const int64_t o = ((int64_t)wave * a.n + s) * kStatsKept + kept;
            a.kept_bin[o] = lane;
            a.kept_p[o] = p;
          }
          ++kept;
        }
      } else {
        if (!(l > rq.lnhi_lo && l < rq.lnhi_hi && z < rq.z_hi && z > rq.z_lo)) continue;
        const double w = rq.moment ? sw[j] : 1.0;
        const double wm = w * p, wv = w * w * (1 - p) * p;
        const bool below = last ? q <= e_hi : q < e_hi;
        if (mine && q >= e_lo && below) {
          acc0.add(wm);
          acc1.add(wv);
        }
        if (mine && below && wm != wm) poison = true;
      }
    }
  }
  if (!active) return;
  const int64_t o = (int64_t)wave * a.n + s;
  if (mine) {
    const double nan = __builtin_nan("");
    if (rq.histogram) {
      a.mean[o * kStatsMaxBins + lane] = poison ? nan : acc0.value();
      a.var[o * kStatsMaxBins + lane] = poison ? nan : acc1.value();
    } else {
      a.pois[o * kStatsMaxBins + lane] = acc0.value();
    }
  }
  if (lane == 0) a.count[o] = kept;
}
