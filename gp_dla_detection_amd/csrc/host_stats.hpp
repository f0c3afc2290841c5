// host_stats.hpp -- the CDDF statistics (stats_kernels.hpp), the sightline S/N table,
// the path-length matrix and the stratified bootstrap
#pragma once

static_assert(GPDLA_STATS_MAX_BINS == gpdla::kStatsMaxBins && GPDLA_STATS_MAX_REQUESTS == gpdla::kStatsMaxRequests &&
                  GPDLA_STATS_KEPT_CAPACITY == gpdla::kStatsKept,
              "gpdla.h and stats_kernels.hpp disagree");
static_assert(GPDLA_BOOTSTRAP_MAX_COLUMNS == gpdla::kBootMaxColumns, "gpdla.h and stats_kernels.hpp disagree");

namespace {

// Measuring aid (tools/bench_refined_stats.py): once gpdla_debug_time_bin_kernels(1) has been called on a thread,
// its launches of k_bin_posteriors / k_bin_posteriors_boxed are bracketed by device events and
// gpdla_debug_last_bin_ms returns the last duration.  Off by default: a call then launches as it always did.
thread_local bool t_bin_timing = false;
thread_local double t_bin_ms = -1.0;

template <typename Args>
int launch_bin_kernel(void (*kernel)(Args), int64_t n, const Args &a) {
  EventPair ev;
  if (t_bin_timing) {
    int rc = ev.create();
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ev.e0, 0));
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  if (t_bin_timing) {
    HIP_TRY(hipEventRecord(ev.e1, 0));
    HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = -1.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    t_bin_ms = (double)ms;
  }
  return GPDLA_OK;
}

// The bin requests of a per-spectrum pass, checked and turned into the kernels' form: req[r] and the edges
// table [R][kStatsMaxBins + 1].  need_outputs: the outputs each request writes must not be null.
int stats_bin_requests(int num_requests, const gpdla_bin_request *requests, const gpdla_bin_output *outputs, bool need_outputs,
                       gpdla::StatsRequest *req, std::vector<double> &edges) {
  using namespace gpdla;
  edges.assign((size_t)num_requests * (kStatsMaxBins + 1), 0.0);
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
    if (need_outputs && (q.histogram ? (!o.mean || !o.var) : (!o.pois || !o.kept_count || !o.kept_bin || !o.kept_p)))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "request %d: null output", r);
    req[r] = StatsRequest{q.quantity, q.num_bins, q.histogram != 0, q.moment != 0, q.lowzcut != 0,
                          q.z_lo, q.z_hi, q.lnhi_lo, q.lnhi_hi, q.p_thresh_sample, q.p_switch};
  }
  return GPDLA_OK;
}

// The output tables of a per-spectrum pass on the device: sums = pois, mean, var ([R][n][kStatsMaxBins] each,
// zeroed), the kept pairs and their counts.
struct StatsBinTables {
  double *sums, *kp;
  int32_t *cnt, *kb;
  int alloc(DeviceTemps &tmp, int64_t R, int64_t n) {
    using namespace gpdla;
    int rc;
    if ((rc = tmp.alloc(&sums, (size_t)3 * R * n * kStatsMaxBins)) || (rc = tmp.alloc(&kp, (size_t)R * n * kStatsKept)) ||
        (rc = tmp.alloc(&cnt, (size_t)R * n)) || (rc = tmp.alloc(&kb, (size_t)R * n * kStatsKept)))
      return rc;
    HIP_TRY(hipMemset(sums, 0, (size_t)3 * R * n * kStatsMaxBins * sizeof(double)));
    return GPDLA_OK;
  }
  template <typename Args>
  void bind(Args &a, int64_t R, int64_t n) const {
    a.pois = sums;
    a.mean = sums + R * n * gpdla::kStatsMaxBins;
    a.var = sums + 2 * R * n * gpdla::kStatsMaxBins;
    a.count = cnt;
    a.kept_bin = kb;
    a.kept_p = kp;
  }
  // into the caller's arrays; a row above the kept capacity makes the call GPDLA_ERR_UNSUPPORTED, outputs written
  int unpack(int64_t R, int64_t n, const gpdla_bin_request *requests, gpdla_bin_output *outputs) const;
};

int StatsBinTables::unpack(int64_t R, int64_t n, const gpdla_bin_request *requests, gpdla_bin_output *outputs) const {
  using namespace gpdla;
  std::vector<double> hs((size_t)3 * R * n * kStatsMaxBins), hkp((size_t)R * n * kStatsKept);
  std::vector<int32_t> hcnt((size_t)R * n), hkb((size_t)R * n * kStatsKept);
  HIP_TRY(hipMemcpy(hs.data(), sums, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hkp.data(), kp, hkp.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hcnt.data(), cnt, hcnt.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hkb.data(), kb, hkb.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t over = -1;
  int over_r = 0;
  for (int64_t r = 0; r < R; ++r) {
    const gpdla_bin_output &o = outputs[r];
    const int nb = requests[r].num_bins;
    for (int64_t s = 0; s < n; ++s) {
      const size_t base = ((size_t)r * n + s) * kStatsMaxBins;
      for (int b = 0; b < nb; ++b) {
        if (o.pois) o.pois[s * nb + b] = hs[base + b];
        if (o.mean) o.mean[s * nb + b] = hs[(size_t)R * n * kStatsMaxBins + base + b];
        if (o.var) o.var[s * nb + b] = hs[(size_t)2 * R * n * kStatsMaxBins + base + b];
      }
      const int c = requests[r].histogram ? 0 : hcnt[r * n + s];
      if (c > kStatsKept && over < 0) {
        over = s;
        over_r = (int)r;
      }
      if (o.kept_count) o.kept_count[s] = c;
      for (int i = 0; i < kStatsKept; ++i) {
        const bool used = i < c;
        if (o.kept_bin) o.kept_bin[s * kStatsKept + i] = used ? hkb[((size_t)r * n + s) * kStatsKept + i] : -1;
        if (o.kept_p) o.kept_p[s * kStatsKept + i] = used ? hkp[((size_t)r * n + s) * kStatsKept + i] : 0.0;
      }
    }
  }
  if (over >= 0)
    return fail(GPDLA_ERR_UNSUPPORTED, "spectrum %lld of the block keeps %d samples directly in request %d (capacity %d)",
                (long long)over, hcnt[over_r * n + over], over_r, kStatsKept);
  return GPDLA_OK;
}

// the rows of a host table [n][S] at stride row_stride as one packed block (`rows` holds it when a copy is needed)
const double *stats_packed_rows(const double *src, int64_t n, int64_t S, int64_t row_stride, std::vector<double> &rows) {
  if (row_stride == S) return src;
  rows.resize((size_t)n * S);
  for (int64_t s = 0; s < n; ++s) std::memcpy(rows.data() + s * S, src + s * row_stride, S * sizeof(double));
  return rows.data();
}

}  // namespace

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
  std::vector<double> edges;
  int rc = stats_bin_requests(num_requests, requests, outputs, num_spectra > 0, a.req, edges);
  if (rc) return rc;
  if (num_spectra == 0) return GPDLA_OK;
  if ((rc = select_device(device_id))) return rc;
  const int64_t n = num_spectra, S = num_samples, R = num_requests;
  std::vector<double> w10(S);
  for (int64_t j = 0; j < S; ++j) w10[j] = std::pow(10.0, log_nhi_samples[j]);  // numpy's 10**lnhi: libm pow
  std::vector<double> rows;
  const double *src = stats_packed_rows(sample_log_likelihoods, n, S, row_stride, rows);  // the device copy is [n][S]
  const int64_t ld = S;
  DeviceTemps tmp;
  double *d_sll, *d_vec, *d_smp, *d_edges;
  StatsBinTables tab;
  if ((rc = tmp.alloc(&d_sll, (size_t)n * S)) || (rc = tmp.alloc(&d_vec, (size_t)5 * n)) ||
      (rc = tmp.alloc(&d_smp, (size_t)3 * S)) || (rc = tmp.alloc(&d_edges, edges.size())) || (rc = tab.alloc(tmp, R, n)))
    return rc;
  HIP_TRY(hipMemcpy(d_sll, src, (size_t)n * S * sizeof(double), hipMemcpyHostToDevice));
  const double *vecs[5] = {shift, p_dla, z_min, z_max, upper_z};
  for (int i = 0; i < 5; ++i) HIP_TRY(hipMemcpy(d_vec + i * n, vecs[i], n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_smp, offset_samples, S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_smp + S, log_nhi_samples, S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_smp + 2 * S, w10.data(), S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_edges, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice));
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
  tab.bind(a, R, n);
  if ((rc = launch_bin_kernel(k_bin_posteriors, n, a))) return rc;
  return tab.unpack(R, n, requests, outputs);
} GPDLA_NO_THROW

int gpdla_stats_bin_posteriors_boxed(int64_t num_rows, int64_t num_points, const double *sample_log_posteriors,
                                     int64_t row_stride, const double *p_dla, const double *boxes, const double *upper_z,
                                     const double *u, const double *v, int num_requests, const gpdla_bin_request *requests,
                                     gpdla_bin_output *outputs, double *shift, int device_id) try {
  using namespace gpdla;
  if (num_rows < 0 || num_points < 1 || row_stride < num_points)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "need num_rows >= 0, S' >= 1 and row_stride >= S'");
  if (num_requests < 1 || num_requests > kStatsMaxRequests || !requests || !outputs)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "%d bin requests; one pass takes 1 to %d", num_requests, kStatsMaxRequests);
  if (!u || !v) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null unit points");
  if (num_rows > 0 && (!sample_log_posteriors || !p_dla || !boxes || !upper_z || !shift))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null per-row input or null shift");
  if (num_rows > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 rows in one block");
  for (int64_t j = 0; j < num_points; ++j) {
    if (!(u[j] >= 0.0 && u[j] < 1.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "u[%lld] = %g is not inside [0, 1)", (long long)j, u[j]);
    if (!(v[j] >= 0.0 && v[j] < 1.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "v[%lld] = %g is not inside [0, 1)", (long long)j, v[j]);
  }
  StatsBoxedArgs a{};
  std::vector<double> edges;
  int rc = stats_bin_requests(num_requests, requests, outputs, num_rows > 0, a.req, edges);
  if (rc) return rc;
  if (num_rows == 0) return GPDLA_OK;
  if ((rc = select_device(device_id))) return rc;
  const int64_t n = num_rows, S = num_points, R = num_requests;
  std::vector<double> rows;
  const double *src = stats_packed_rows(sample_log_posteriors, n, S, row_stride, rows);  // the device copy is [n][S]
  DeviceTemps tmp;
  double *d_lam, *d_vec, *d_box, *d_uv, *d_edges, *d_shift;
  StatsBinTables tab;
  if ((rc = tmp.alloc(&d_lam, (size_t)n * S)) || (rc = tmp.alloc(&d_vec, (size_t)2 * n)) || (rc = tmp.alloc(&d_box, (size_t)4 * n)) ||
      (rc = tmp.alloc(&d_uv, (size_t)2 * S)) || (rc = tmp.alloc(&d_edges, edges.size())) || (rc = tmp.alloc(&d_shift, (size_t)n)) ||
      (rc = tab.alloc(tmp, R, n)))
    return rc;
  HIP_TRY(hipMemcpy(d_lam, src, (size_t)n * S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_vec, p_dla, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_vec + n, upper_z, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_box, boxes, 4 * n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_uv, u, S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_uv + S, v, S * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_edges, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice));
  a.n = n;
  a.S = S;
  a.ld = S;
  a.lam = d_lam;
  a.p_dla = d_vec;
  a.upper_z = d_vec + n;
  a.boxes = d_box;
  a.offsets = d_uv;
  a.lnhi = d_uv + S;
  a.edges = d_edges;
  a.R = (int32_t)R;
  a.shift = d_shift;
  tab.bind(a, R, n);
  if ((rc = launch_bin_kernel(k_bin_posteriors_boxed, n, a))) return rc;
  HIP_TRY(hipMemcpy(shift, d_shift, n * sizeof(double), hipMemcpyDeviceToHost));
  return tab.unpack(R, n, requests, outputs);
} GPDLA_NO_THROW

void gpdla_debug_time_bin_kernels(int on) { t_bin_timing = on != 0; }

double gpdla_debug_last_bin_ms(void) { return t_bin_ms; }

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

int gpdla_stats_sightline_snrs(int64_t num_sightlines, const int64_t *offsets, const double *wavelengths,
                               const double *flux, const double *noise_variance, const double *max_z_dlas,
                               const double *normalizers, double *snrs, int device_id) try {
  using namespace gpdla;
  if (num_sightlines < 0 || (num_sightlines > 0 && (!offsets || !max_z_dlas || !snrs)))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument or negative sightline count");
  if (num_sightlines == 0) return GPDLA_OK;
  if (num_sightlines > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 sightlines in one call");
  const int64_t n = num_sightlines;
  if (offsets[0] != 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  for (int64_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (sightline %lld)", (long long)i);
    if (offsets[i + 1] - offsets[i] > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "sightline %lld has more than 2^31 - 1 pixels", (long long)i);
  }
  const int64_t total = offsets[n];
  if (total > 0 && (!wavelengths || !flux || !noise_variance)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null pixel arrays");
  int rc = select_device(device_id);
  if (rc) return rc;
  DeviceTemps tmp;
  int64_t *d_off;
  double *d_pix, *d_z, *d_nm = nullptr, *d_out;
  if ((rc = tmp.alloc(&d_off, (size_t)n + 1)) || (rc = tmp.alloc(&d_pix, (size_t)3 * total)) || (rc = tmp.alloc(&d_z, (size_t)n)) ||
      (rc = tmp.alloc(&d_out, (size_t)n)) || (normalizers && (rc = tmp.alloc(&d_nm, (size_t)n))))
    return rc;
  HIP_TRY(hipMemcpy(d_off, offsets, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (total > 0) {
    HIP_TRY(hipMemcpy(d_pix, wavelengths, total * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_pix + total, flux, total * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_pix + 2 * total, noise_variance, total * sizeof(double), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(d_z, max_z_dlas, n * sizeof(double), hipMemcpyHostToDevice));
  if (normalizers) HIP_TRY(hipMemcpy(d_nm, normalizers, n * sizeof(double), hipMemcpyHostToDevice));
  SnrArgs a{d_off, d_pix, d_pix + total, d_pix + 2 * total, d_z, d_nm, d_out};
  hipLaunchKernelGGL(k_sightline_snr, dim3((unsigned)n), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(snrs, d_out, n * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_stats_path_lengths(int64_t num_sightlines, const double *min_z_dlas, const double *max_z_dlas,
                             int num_bins, const double *edges, int lowzcut, double proximity_zone, double omega_m,
                             double *dX, int device_id) try {
  using namespace gpdla;
  if (num_sightlines < 0 || (num_sightlines > 0 && (!min_z_dlas || !max_z_dlas || !dX)))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument or negative sightline count");
  if (num_bins < 1 || num_bins > kStatsMaxBins || !edges)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "%d bins; a request takes 1 to %d", num_bins, kStatsMaxBins);
  for (int b = 0; b <= num_bins; ++b)
    if (!std::isfinite(edges[b]) || (b > 0 && !(edges[b] > edges[b - 1])))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "edges must be finite and strictly increasing");
  if (!(edges[0] > -1.0) || edges[num_bins] - edges[0] > 1000.0)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "edges must lie above z = -1 and span at most 1000");
  if (!std::isfinite(proximity_zone) || !(omega_m > 0.0 && omega_m <= 1.0))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "need a finite proximity zone and 0 < omega_m <= 1");
  for (int64_t i = 0; i < num_sightlines; ++i) {
    const double lo = min_z_dlas[i];
    double hi = max_z_dlas[i];
    if (lowzcut) hi = std::fmax(std::fmin(hi, hi - proximity_zone), lo);
    if (hi - lo < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the search range of sightline %lld ends below its start", (long long)i);
  }
  if (num_sightlines == 0) return GPDLA_OK;
  const int64_t n = num_sightlines, cells = n * num_bins;
  if ((cells + 255) / 256 > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "too many sightlines for one launch");
  int rc = select_device(device_id);
  if (rc) return rc;
  DeviceTemps tmp;
  double *d_z, *d_e, *d_out;
  if ((rc = tmp.alloc(&d_z, (size_t)2 * n)) || (rc = tmp.alloc(&d_e, (size_t)num_bins + 1)) || (rc = tmp.alloc(&d_out, (size_t)cells)))
    return rc;
  HIP_TRY(hipMemcpy(d_z, min_z_dlas, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_z + n, max_z_dlas, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_e, edges, (num_bins + 1) * sizeof(double), hipMemcpyHostToDevice));
  PathArgs a{n, num_bins, lowzcut != 0, d_z, d_z + n, d_e, proximity_zone, omega_m, d_out};
  hipLaunchKernelGGL(k_path_lengths, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(dX, d_out, cells * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_stats_bootstrap_sums(int64_t num_rows, int num_columns, const double *V, const int32_t *stratum,
                               uint64_t seed, int64_t first_replicate, int64_t num_replicates, double *sums,
                               int device_id) try {
  using namespace gpdla;
  if (num_rows < 1 || !V || !stratum || !sums) return fail(GPDLA_ERR_INVALID_ARGUMENT, "need num_rows >= 1 and non-null arrays");
  if (num_columns < 1 || num_columns > kBootMaxColumns)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "%d columns; the matrix takes 1 to %d", num_columns, kBootMaxColumns);
  if (num_replicates < 1 || first_replicate < 0 || first_replicate + num_replicates > 4294967296LL)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "need num_replicates >= 1 and replicate indices in [0, 2^32)");
  if (num_rows > 2147483647LL || num_replicates > 2147483647LL)
    return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 rows or replicates in one call");
  const int64_t n = num_rows;
  std::vector<int32_t> first(n), size(n);
  if (stratum[0] < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "stratum labels must be >= 0");
  for (int64_t i = 0, start = 0; i < n; ++i) {   // rows come sorted by stratum
    if (i > 0 && stratum[i] < stratum[i - 1]) return fail(GPDLA_ERR_INVALID_ARGUMENT, "rows must be sorted by stratum (row %lld)", (long long)i);
    if (i > 0 && stratum[i] != stratum[i - 1]) start = i;
    first[i] = (int32_t)start;
  }
  for (int64_t i = n - 1, end = n; i >= 0; --i) {
    size[i] = (int32_t)(end - first[i]);
    if (first[i] == i) end = i;
  }
  int rc = select_device(device_id);
  if (rc) return rc;
  DeviceTemps tmp;
  double *d_V, *d_out;
  int32_t *d_fs;
  const size_t cells = (size_t)n * num_columns, outs = (size_t)num_replicates * num_columns;
  if ((rc = tmp.alloc(&d_V, cells)) || (rc = tmp.alloc(&d_fs, (size_t)2 * n)) || (rc = tmp.alloc(&d_out, outs))) return rc;
  HIP_TRY(hipMemcpy(d_V, V, cells * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_fs, first.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_fs + n, size.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  BootArgs a{n, num_columns, d_V, d_fs, d_fs + n, (uint32_t)seed, (uint32_t)(seed >> 32), first_replicate, d_out};
  hipLaunchKernelGGL(k_bootstrap_sums, dim3((unsigned)num_replicates), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(sums, d_out, outs * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
