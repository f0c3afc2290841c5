// host_stats.hpp -- the CDDF statistics (stats_kernels.hpp)
#pragma once

static_assert(GPDLA_STATS_MAX_BINS == gpdla::kStatsMaxBins && GPDLA_STATS_MAX_REQUESTS == gpdla::kStatsMaxRequests &&
                  GPDLA_STATS_KEPT_CAPACITY == gpdla::kStatsKept,
              "gpdla.h and stats_kernels.hpp disagree");

extern "C" {

int gpdla_stats_bin_posteriors(int64_t num_spectra, int64_t num_samples, const double *sample_log_likelihoods,
                               int64_t row_stride, const double *shift, const double *p_dla,
                               const double *z_min, const double *z_max, const double *upper_z,
                               const double *offset_samples, const double *log_nhi_samples,
                               int num_requests, const gpdla_bin_request *requests,
                               gpdla_bin_output *outputs, int device_id) try {
  using namespace gpdla;
  if (num_spectra < 0 || num_samples < 1 || row_stride < num_samples)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "need num_spectra >= 0, S >= 1 and row_stride >= S");
  if (num_requests < 1 || num_requests > kStatsMaxRequests || !requests || !outputs)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "%d bin requests; one pass takes 1 to %d", num_requests, kStatsMaxRequests);
  if (!offset_samples || !log_nhi_samples) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null samples");
  if (num_spectra > 0 && (!sample_log_likelihoods || !shift || !p_dla || !z_min || !z_max || !upper_z))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null per-spectrum input");
  if (num_spectra > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 spectra in one block");
  StatsBinArgs a{};
  std::vector<double> edges((size_t)num_requests * (kStatsMaxBins + 1), 0.0);
  for (int r = 0; r < num_requests; ++r) {
    const gpdla_bin_request &q = requests[r];
    const gpdla_bin_output &o = outputs[r];
    if (q.num_bins < 1 || q.num_bins > kStatsMaxBins)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "request %d: %d bins; a request takes 1 to %d", r, q.num_bins, kStatsMaxBins);
    if (!q.edges) return fail(GPDLA_ERR_INVALID_ARGUMENT, "request %d: null edges", r);
    if (q.quantity != 0 && q.quantity != 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "request %d: quantity must be 0 or 1", r);
    for (int b = 0; b <= q.num_bins; ++b) {
      if (!std::isfinite(q.edges[b]) || (b > 0 && !(q.edges[b] > q.edges[b - 1])))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "request %d: edges must be finite and strictly increasing", r);
      edges[(size_t)r * (kStatsMaxBins + 1) + b] = q.edges[b];
    }
    for (double v : {q.z_lo, q.z_hi, q.lnhi_lo, q.lnhi_hi, q.p_thresh_sample, q.p_switch})
      if (std::isnan(v)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "request %d: NaN window or threshold", r);
    if (num_spectra > 0 && (q.histogram ? (!o.mean || !o.var) : (!o.pois || !o.kept_count || !o.kept_bin || !o.kept_p)))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "request %d: null output", r);
    a.req[r] = StatsRequest{q.quantity, q.num_bins, q.histogram != 0, q.moment != 0, q.lowzcut != 0,
                            q.z_lo, q.z_hi, q.lnhi_lo, q.lnhi_hi, q.p_thresh_sample, q.p_switch};
  }
  if (num_spectra == 0) return GPDLA_OK;
  int rc = select_device(device_id);
  if (rc) return rc;
  const int64_t n = num_spectra, S = num_samples, R = num_requests;
  std::vector<double> w10(S);
  for (int64_t j = 0; j < S; ++j) w10[j] = std::pow(10.0, log_nhi_samples[j]);  // numpy's 10**lnhi: libm pow
  std::vector<double> rows;
  const double *src = sample_log_likelihoods;
  const int64_t ld = S;
  if (row_stride != S) {  // pack the rows: the device copy is [n][S]
    rows.resize((size_t)n * S);
    for (int64_t s = 0; s < n; ++s) std::memcpy(rows.data() + s * S, src + s * row_stride, S * sizeof(double));
    src = rows.data();
  }
  DeviceTemps tmp;
  double *d_sll, *d_vec, *d_smp, *d_edges, *d_sums, *d_kp;
  int32_t *d_cnt, *d_kb;
  if ((rc = tmp.alloc(&d_sll, (size_t)n * S)) || (rc = tmp.alloc(&d_vec, (size_t)5 * n)) ||
      (rc = tmp.alloc(&d_smp, (size_t)3 * S)) || (rc = tmp.alloc(&d_edges, edges.size())) ||
      (rc = tmp.alloc(&d_sums, (size_t)3 * R * n * kStatsMaxBins)) || (rc = tmp.alloc(&d_kp, (size_t)R * n * kStatsKept)) ||
      (rc = tmp.alloc(&d_cnt, (size_t)R * n)) || (rc = tmp.alloc(&d_kb, (size_t)R * n * kStatsKept)))
    return rc;
  HIP_TRY(hipMemcpy(d_sll, src, (size_t)n * S * sizeof(double), hipMemcpyHostToDevice));
  const double *vecs[5] = {shift, p_dla, z_min, z_max, upper_z};
  for (int i = 0; i < 5; ++i) HIP_TRY(hipMemcpy(d_vec + i * n, vecs[i], n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_smp, offset_samples, S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_smp + S, log_nhi_samples, S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_smp + 2 * S, w10.data(), S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_edges, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d_sums, 0, (size_t)3 * R * n * kStatsMaxBins * sizeof(double)));
  a.n = n;
  a.S = S;
  a.ld = ld;
  a.sll = d_sll;
  a.shift = d_vec;
  a.p_dla = d_vec + n;
  a.z_min = d_vec + 2 * n;
  a.z_max = d_vec + 3 * n;
  a.upper_z = d_vec + 4 * n;
  a.offsets = d_smp;
  a.lnhi = d_smp + S;
  a.w10 = d_smp + 2 * S;
  a.edges = d_edges;
  a.R = (int32_t)R;
  a.pois = d_sums;
  a.mean = d_sums + R * n * kStatsMaxBins;
  a.var = d_sums + 2 * R * n * kStatsMaxBins;
  a.count = d_cnt;
  a.kept_bin = d_kb;
  a.kept_p = d_kp;
  hipLaunchKernelGGL(k_bin_posteriors, dim3((unsigned)n), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  std::vector<double> sums((size_t)3 * R * n * kStatsMaxBins), kp((size_t)R * n * kStatsKept);
  std::vector<int32_t> cnt((size_t)R * n), kb((size_t)R * n * kStatsKept);
  HIP_TRY(hipMemcpy(sums.data(), d_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(kp.data(), d_kp, kp.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cnt.data(), d_cnt, cnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(kb.data(), d_kb, kb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t over = -1;
  int over_r = 0;
  for (int64_t r = 0; r < R; ++r) {
    const gpdla_bin_output &o = outputs[r];
    const int nb = requests[r].num_bins;
    for (int64_t s = 0; s < n; ++s) {
      const size_t base = ((size_t)r * n + s) * kStatsMaxBins;
      for (int b = 0; b < nb; ++b) {
        if (o.pois) o.pois[s * nb + b] = sums[base + b];
        if (o.mean) o.mean[s * nb + b] = sums[(size_t)R * n * kStatsMaxBins + base + b];
        if (o.var) o.var[s * nb + b] = sums[(size_t)2 * R * n * kStatsMaxBins + base + b];
      }
      const int c = requests[r].histogram ? 0 : cnt[r * n + s];
      if (c > kStatsKept && over < 0) {
        over = s;
        over_r = (int)r;
      }
      if (o.kept_count) o.kept_count[s] = c;
      for (int i = 0; i < kStatsKept; ++i) {
        const bool used = i < c;
        if (o.kept_bin) o.kept_bin[s * kStatsKept + i] = used ? kb[((size_t)r * n + s) * kStatsKept + i] : -1;
        if (o.kept_p) o.kept_p[s * kStatsKept + i] = used ? kp[((size_t)r * n + s) * kStatsKept + i] : 0.0;
      }
    }
  }
  if (over >= 0)
    return fail(GPDLA_ERR_UNSUPPORTED, "spectrum %lld of the block keeps %d samples directly in request %d (capacity %d)",
                (long long)over, cnt[over_r * n + over], over_r, kStatsKept);
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_stats_poisson_binomial_cf(int64_t num_segments, const int64_t *offsets, const double *p,
                                    double *logsum, double *argsum, int device_id) try {
  using namespace gpdla;
  if (num_segments < 0 || (num_segments > 0 && (!offsets || !logsum || !argsum)))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument or negative segment count");
  if (num_segments == 0) return GPDLA_OK;
  if (offsets[0] != 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  std::vector<int64_t> out_off(num_segments + 1, 0), blk_seg, blk_n0;
  for (int64_t g = 0; g < num_segments; ++g) {
    const int64_t N = offsets[g + 1] - offsets[g];
    if (N < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (segment %lld)", (long long)g);
    const int64_t M = (N + 1) / 2 + 1;
    out_off[g + 1] = out_off[g] + M;
    for (int64_t n0 = 0; n0 < M; n0 += 256) {
      blk_seg.push_back(g);
      blk_n0.push_back(n0);
    }
  }
  const int64_t total = offsets[num_segments];
  if (total > 0 && !p) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null probabilities");
  // p may exceed 1 by a few ulps (a dominant sample of a strong absorber: p_dla and the normalisation
  // each round); the reference accepts any value, and the sums are well defined for p near 1.
  for (int64_t j = 0; j < total; ++j)
    if (!(p[j] >= 0.0 && std::isfinite(p[j])))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "probability %lld is negative or not finite", (long long)j);
  if (blk_seg.size() > 2147483647ULL) return fail(GPDLA_ERR_UNSUPPORTED, "too many segments for one launch");
  int rc = select_device(device_id);
  if (rc) return rc;
  DeviceTemps tmp;
  int64_t *d_seg, *d_out, *d_bs, *d_bn;
  double *d_p, *d_ls, *d_as;
  const int64_t nb = (int64_t)blk_seg.size(), M = out_off[num_segments];
  if ((rc = tmp.alloc(&d_seg, (size_t)num_segments + 1)) || (rc = tmp.alloc(&d_out, (size_t)num_segments + 1)) ||
      (rc = tmp.alloc(&d_bs, (size_t)nb)) || (rc = tmp.alloc(&d_bn, (size_t)nb)) || (rc = tmp.alloc(&d_p, (size_t)total)) ||
      (rc = tmp.alloc(&d_ls, (size_t)M)) || (rc = tmp.alloc(&d_as, (size_t)M)))
    return rc;
  HIP_TRY(hipMemcpy(d_seg, offsets, (num_segments + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_out, out_off.data(), out_off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_bs, blk_seg.data(), nb * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_bn, blk_n0.data(), nb * sizeof(int64_t), hipMemcpyHostToDevice));
  if (total > 0) HIP_TRY(hipMemcpy(d_p, p, total * sizeof(double), hipMemcpyHostToDevice));
  StatsCfArgs a{d_seg, d_out, d_bs, d_bn, d_p, d_ls, d_as};
  hipLaunchKernelGGL(k_poisson_binomial_cf, dim3((unsigned)nb), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(logsum, d_ls, M * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(argsum, d_as, M * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
