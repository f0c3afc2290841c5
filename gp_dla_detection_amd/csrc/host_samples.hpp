// host_samples.hpp -- DLA parameter samples and LLS normalisers (sample_kernels.hpp):
// the KDE of the catalogue's log N_HI, the quadratic through its logarithm, the cumulative table of
// the mixture prior, the scrambled Halton points and the inverse-CDF draw
#pragma once

static_assert(GPDLA_HALTON_MAX_DIMS == gpdla::kHaltonMaxDims && GPDLA_HALTON_MAX_BASE == gpdla::kHaltonMaxBase &&
                  GPDLA_SAMPLES_UPPER == gpdla::kPriorUpper,
              "gpdla.h and sample_kernels.hpp disagree");

namespace {

int check_finite(const double *v, int64_t n, const char *what) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return fail(GPDLA_ERR_INVALID_ARGUMENT, "%s %lld is not finite", what, (long long)i);
  return GPDLA_OK;
}

int check_catalogue(int64_t n, const double *values, double bandwidth) {
  if (n < 2 || !values) return fail(GPDLA_ERR_INVALID_ARGUMENT, "need at least 2 catalogue values (got %lld)", (long long)n);
  if (n > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 catalogue values");
  if (!(bandwidth >= 0.0) || !std::isfinite(bandwidth))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "bandwidth must be finite and >= 0 (0: the normal-reference rule)");
  return check_finite(values, n, "catalogue value");
}

int check_prior(const gpdla_nhi_prior *p) {
  if (!p) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null prior");
  for (double v : {p->coeff[0], p->coeff[1], p->coeff[2], p->centre, p->alpha, p->uniform_min, p->uniform_max, p->lower, p->Z})
    if (!std::isfinite(v)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the prior holds a value that is not finite");
  if (std::isinf(p->flat_below)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "flat_below must be finite or NaN");
  if (!(p->alpha >= 0.0 && p->alpha <= 1.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "alpha %g is outside [0, 1]", p->alpha);
  if (!(p->uniform_min < p->uniform_max))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "uniform range [%g, %g] is not ordered", p->uniform_min, p->uniform_max);
  if (!(p->lower < GPDLA_SAMPLES_UPPER))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "lower limit %g is not below the upper limit %g", p->lower, GPDLA_SAMPLES_UPPER);
  if (!(p->Z > 0.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "Z must be positive");
  return GPDLA_OK;
}

// h = sig (4 / (3 N))^(1/5), sig = median(|v - median(v)|) / 0.6745, the medians on the device
int rule_bandwidth(DeviceTemps &tmp, const double *d_values, int64_t n, double *h) {
  using namespace gpdla;
  int rc;
  double *d_mid, *d_dev;
  if ((rc = tmp.alloc(&d_mid, 4)) || (rc = tmp.alloc(&d_dev, (size_t)n))) return rc;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_rank_select, dim3(blocks), dim3(256), 0, 0, SelectArgs{d_values, n, (n - 1) / 2, n / 2, d_mid});
  hipLaunchKernelGGL(k_abs_deviation, dim3(blocks), dim3(256), 0, 0, d_values, n, d_mid, d_dev);
  hipLaunchKernelGGL(k_rank_select, dim3(blocks), dim3(256), 0, 0, SelectArgs{d_dev, n, (n - 1) / 2, n / 2, d_mid + 2});
  HIP_TRY(hipGetLastError());
  double mid[4];
  HIP_TRY(hipMemcpy(mid, d_mid, sizeof(mid), hipMemcpyDeviceToHost));
  const double sig = ((mid[2] + mid[3]) / 2.0) / 0.6745;
  if (!(sig > 0.0))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the median absolute deviation of the catalogue is 0: pass a bandwidth");
  *h = sig * std::pow(4.0 / (3.0 * (double)n), 1.0 / 5.0);
  return GPDLA_OK;
}

// density of d_values on d_points into d_density (device); h == 0: the rule
int kde_on_device(DeviceTemps &tmp, const double *d_values, int64_t n, const double *d_points, int64_t G, double *h,
                  double *d_density) {
  using namespace gpdla;
  int rc;
  if (*h == 0.0 && (rc = rule_bandwidth(tmp, d_values, n, h))) return rc;
  if (G == 0) return GPDLA_OK;
  const int64_t gblocks = (G + 255) / 256, chunks = (n + kKdeChunk - 1) / kKdeChunk;
  if (gblocks * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "too many grid points x catalogue values for one launch");
  double *d_partial;
  if ((rc = tmp.alloc(&d_partial, (size_t)(chunks * G)))) return rc;
  KdeArgs a{d_values, d_points, n, G, gblocks, *h, d_partial, d_density};
  hipLaunchKernelGGL(k_kde_partial, dim3((unsigned)(gblocks * chunks)), dim3(256), 0, 0, a);
  hipLaunchKernelGGL(k_kde_finish, dim3((unsigned)gblocks), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

gpdla::PriorDev prior_dev(const gpdla_nhi_prior &p) {
  return gpdla::PriorDev{p.coeff[0], p.coeff[1], p.coeff[2], p.centre, p.alpha, p.uniform_min, p.uniform_max,
                         p.lower, p.flat_below, p.Z};
}

// The cumulative table of `dev` on [lower, upper], split at the break points inside; *total
// (optional) receives its last entry.
int build_prior_table(DeviceTemps &tmp, const gpdla::PriorDev &dev, gpdla::PriorTable *T, double *total) {
  using namespace gpdla;
  std::vector<double> edges{dev.lower};
  std::vector<double> breaks{dev.umin, dev.umax};
  if (!std::isnan(dev.flat_below)) breaks.push_back(dev.flat_below);
  std::sort(breaks.begin(), breaks.end());
  for (double b : breaks)
    if (b > edges.back() && b < kPriorUpper) edges.push_back(b);
  edges.push_back(kPriorUpper);
  T->nseg = (int32_t)edges.size() - 1;   // 1 .. kPriorMaxSegments
  for (size_t i = 0; i < edges.size(); ++i) T->edge[i] = edges[i];
  const int P = T->nseg * kPriorPanels;
  int rc;
  double *d_panel;
  if ((rc = tmp.alloc(&d_panel, (size_t)P)) || (rc = tmp.alloc(&T->cum, (size_t)P + 1))) return rc;
  hipLaunchKernelGGL(k_prior_panels, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, 0, dev, *T, d_panel);
  hipLaunchKernelGGL(k_prior_prefix, dim3(1), dim3(64), 0, 0, d_panel, *T);
  HIP_TRY(hipGetLastError());
  if (total) HIP_TRY(hipMemcpy(total, T->cum + P, sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
}

// the reverse-radix permutation of base b: the m-bit reversals of 0, 1, ... in order, m = ceil(log2 b),
// those >= b dropped
void rr2_permutation(int b, uint8_t *perm) {
  int m = 0;
  while ((1 << m) < b) ++m;
  int count = 0;
  for (int v = 0; v < (1 << m); ++v) {
    int r = 0;
    for (int bit = 0; bit < m; ++bit)
      if (v & (1 << bit)) r |= 1 << (m - 1 - bit);
    if (r < b) perm[count++] = (uint8_t)r;
  }
}

int halton_args(int num_bases, const int32_t *bases, gpdla::HaltonArgs *h) {
  using namespace gpdla;
  if (num_bases < 1 || num_bases > kHaltonMaxDims || !bases)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "%d bases; a call takes 1 to %d", num_bases, kHaltonMaxDims);
  std::memset(h, 0, sizeof(*h));
  h->ndim = num_bases;
  for (int d = 0; d < num_bases; ++d) {
    if (bases[d] < 2 || bases[d] > kHaltonMaxBase)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "base %d is outside 2 .. %d", bases[d], kHaltonMaxBase);
    h->base[d] = bases[d];
    rr2_permutation(bases[d], h->perm[d]);
  }
  return GPDLA_OK;
}

int check_index_range(int64_t first_index, int64_t num) {
  if (first_index < 0 || num < 0 || first_index > 4294967296LL || num > 4294967296LL || first_index + num > 4294967296LL)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "need first_index >= 0, num >= 0 and first_index + num <= 2^32");
  return GPDLA_OK;
}

// least-squares quadratic through (t_i, y_i) about `centre`, by polynomials orthogonal on the points
void fit_quadratic(const std::vector<double> &t, const std::vector<double> &y, double centre, double c[3]) {
  const size_t n = t.size();
  long double m1 = 0, a = 0;
  for (size_t i = 0; i < n; ++i) {
    const long double s = (long double)t[i] - centre;
    m1 += s;
    a += s * s;
  }
  m1 /= n;
  a /= n;
  long double n11 = 0, b = 0;
  for (size_t i = 0; i < n; ++i) {
    const long double s = (long double)t[i] - centre, q1 = s - m1;
    n11 += q1 * q1;
    b += s * s * q1;
  }
  b /= n11;
  long double n22 = 0, a0 = 0, a1 = 0, a2 = 0;
  for (size_t i = 0; i < n; ++i) {
    const long double s = (long double)t[i] - centre, q1 = s - m1, q2 = s * s - b * q1 - a;
    n22 += q2 * q2;
    a0 += y[i];
    a1 += y[i] * q1;
    a2 += y[i] * q2;
  }
  a0 /= n;
  a1 /= n11;
  a2 /= n22;
  c[2] = (double)a2;
  c[1] = (double)(a1 - a2 * b);
  c[0] = (double)(a0 - a1 * m1 + a2 * (b * m1 - a));
}

}  // namespace

extern "C" {

int gpdla_samples_kde(int64_t num_values, const double *values, int64_t num_points, const double *points,
                      double bandwidth, double *density, double *bandwidth_used, int device_id) try {
  int rc = check_catalogue(num_values, values, bandwidth);
  if (rc) return rc;
  if (num_points < 0 || (num_points > 0 && (!points || !density)))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null grid or negative number of grid points");
  if ((rc = check_finite(points, num_points, "grid point"))) return rc;
  if ((rc = select_device(device_id))) return rc;
  DeviceTemps tmp;
  double *d_values, *d_points, *d_density;
  if ((rc = tmp.alloc(&d_values, (size_t)num_values)) || (rc = tmp.alloc(&d_points, (size_t)num_points)) ||
      (rc = tmp.alloc(&d_density, (size_t)num_points)))
    return rc;
  HIP_TRY(hipMemcpy(d_values, values, num_values * sizeof(double), hipMemcpyHostToDevice));
  if (num_points > 0) HIP_TRY(hipMemcpy(d_points, points, num_points * sizeof(double), hipMemcpyHostToDevice));
  double h = bandwidth;
  if ((rc = kde_on_device(tmp, d_values, num_values, d_points, num_points, &h, d_density))) return rc;
  if (num_points > 0) HIP_TRY(hipMemcpy(density, d_density, num_points * sizeof(double), hipMemcpyDeviceToHost));
  if (bandwidth_used) *bandwidth_used = h;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_samples_fit_prior(int64_t num_values, const double *values, double fit_min, double fit_max, double alpha,
                            double uniform_min, double uniform_max, double lower, double flat_below,
                            double bandwidth, gpdla_nhi_prior *prior, int device_id) try {
  int rc = check_catalogue(num_values, values, bandwidth);
  if (rc) return rc;
  if (!std::isfinite(fit_min) || !std::isfinite(fit_max) || !(fit_min < fit_max))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "fit range [%g, %g] is not ordered", fit_min, fit_max);
  gpdla_nhi_prior p{};
  p.centre = (fit_min + fit_max) / 2.0;
  p.alpha = alpha;
  p.uniform_min = uniform_min;
  p.uniform_max = uniform_max;
  p.lower = lower;
  p.flat_below = flat_below;
  p.Z = 1.0;
  if ((rc = check_prior(&p))) return rc;
  if ((rc = select_device(device_id))) return rc;
  constexpr int G = GPDLA_SAMPLES_FIT_POINTS;
  std::vector<double> x(G), kde(G), logk(G);
  const double step = (fit_max - fit_min) / (G - 1);   // linspace
  for (int i = 0; i < G; ++i) x[i] = (double)i * step + fit_min;
  x[G - 1] = fit_max;
  DeviceTemps tmp;
  double *d_values, *d_points, *d_density;
  if ((rc = tmp.alloc(&d_values, (size_t)num_values)) || (rc = tmp.alloc(&d_points, (size_t)G)) || (rc = tmp.alloc(&d_density, (size_t)G)))
    return rc;
  HIP_TRY(hipMemcpy(d_values, values, num_values * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_points, x.data(), G * sizeof(double), hipMemcpyHostToDevice));
  double h = bandwidth;
  if ((rc = kde_on_device(tmp, d_values, num_values, d_points, G, &h, d_density))) return rc;
  HIP_TRY(hipMemcpy(kde.data(), d_density, G * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < G; ++i) {
    if (!(kde[i] > 0.0) || !std::isfinite(kde[i]))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "the density estimate is %g at %g: its logarithm cannot be fitted", kde[i], x[i]);
    logk[i] = std::log(kde[i]);
  }
  fit_quadratic(x, logk, p.centre, p.coeff);
  // Z: the table of g alone (alpha = 1 and Z = 1 leave p = g)
  gpdla::PriorDev g = prior_dev(p);
  g.alpha = 1.0;
  gpdla::PriorTable T{};
  double Z = 0.0;
  if ((rc = build_prior_table(tmp, g, &T, &Z))) return rc;
  if (!(Z > 0.0) || !std::isfinite(Z)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the fitted density integrates to %g", Z);
  p.Z = Z;
  *prior = p;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_samples_prior_eval(const gpdla_nhi_prior *prior, int64_t num_points, const double *x, double *pdf,
                             double *cdf, int device_id) try {
  int rc = check_prior(prior);
  if (rc) return rc;
  if (num_points < 0 || (num_points > 0 && !x)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null points or negative count");
  if ((rc = check_finite(x, num_points, "point"))) return rc;
  if (num_points == 0 || (!pdf && !cdf)) return GPDLA_OK;
  if ((num_points + 255) / 256 > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "too many points for one launch");
  if ((rc = select_device(device_id))) return rc;
  DeviceTemps tmp;
  const gpdla::PriorDev dev = prior_dev(*prior);
  gpdla::PriorTable T{};
  if ((rc = build_prior_table(tmp, dev, &T, nullptr))) return rc;
  double *d_x, *d_pdf = nullptr, *d_cdf = nullptr;
  if ((rc = tmp.alloc(&d_x, (size_t)num_points)) || (pdf && (rc = tmp.alloc(&d_pdf, (size_t)num_points))) ||
      (cdf && (rc = tmp.alloc(&d_cdf, (size_t)num_points))))
    return rc;
  HIP_TRY(hipMemcpy(d_x, x, num_points * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(gpdla::k_prior_eval, dim3((unsigned)((num_points + 255) / 256)), dim3(256), 0, 0, dev, T, num_points,
                     (const double *)d_x, d_pdf, d_cdf);
  HIP_TRY(hipGetLastError());
  if (pdf) HIP_TRY(hipMemcpy(pdf, d_pdf, num_points * sizeof(double), hipMemcpyDeviceToHost));
  if (cdf) HIP_TRY(hipMemcpy(cdf, d_cdf, num_points * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_samples_halton(int64_t first_index, int64_t num, int num_bases, const int32_t *bases, double *out,
                         int device_id) try {
  int rc = check_index_range(first_index, num);
  if (rc) return rc;
  gpdla::HaltonArgs h;
  if ((rc = halton_args(num_bases, bases, &h))) return rc;
  if (num > 0 && !out) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null output");
  if (num == 0) return GPDLA_OK;
  if ((rc = select_device(device_id))) return rc;
  DeviceTemps tmp;
  double *d_out;
  if ((rc = tmp.alloc(&d_out, (size_t)num * num_bases))) return rc;
  hipLaunchKernelGGL(gpdla::k_halton, dim3((unsigned)((num + 255) / 256)), dim3(256), 0, 0, h, first_index, num, d_out);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out, (size_t)num * num_bases * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_samples_draw(const gpdla_nhi_prior *prior, int64_t first_index, int64_t num, const double *sequence,
                       int sequence_dims, double lls_lower, double lls_upper, gpdla_sample_draw *out,
                       int device_id) try {
  int rc = check_prior(prior);
  if (rc) return rc;
  if ((rc = check_index_range(first_index, num))) return rc;
  if (!out || (num > 0 && (!out->offset || !out->log_nhi || !out->nhi))) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null output");
  const int lls_given = (out->lls_offset != nullptr) + (out->lls_log_nhi != nullptr) + (out->lls_nhi != nullptr);
  if (lls_given != 0 && lls_given != 3) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the three LLS outputs come together or not at all");
  const bool want_lls = lls_given == 3;
  if (want_lls && (!std::isfinite(lls_lower) || !std::isfinite(lls_upper) || !(lls_lower < lls_upper)))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "LLS range [%g, %g] is not ordered", lls_lower, lls_upper);
  if (sequence) {
    if (sequence_dims != 2 && sequence_dims != 3) return fail(GPDLA_ERR_INVALID_ARGUMENT, "a sequence has 2 or 3 columns (got %d)", sequence_dims);
    if (want_lls && sequence_dims != 3) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the LLS outputs need a third column of the sequence");
    for (int64_t i = 0; i < num * sequence_dims; ++i)
      if (!(sequence[i] >= 0.0 && sequence[i] <= 1.0))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "sequence value %lld is outside [0, 1]", (long long)i);
  }
  if (num == 0) return GPDLA_OK;
  if ((rc = select_device(device_id))) return rc;
  DeviceTemps tmp;
  gpdla::DrawArgs a{};
  a.p = prior_dev(*prior);
  if ((rc = build_prior_table(tmp, a.p, &a.T, nullptr))) return rc;
  const int32_t bases[3] = {2, 3, 5};
  if ((rc = halton_args(3, bases, &a.h))) return rc;
  a.first = first_index;
  a.num = num;
  a.seq_dims = sequence ? sequence_dims : 0;
  a.want_lls = want_lls;
  a.lls_lo = lls_lower;
  a.lls_hi = lls_upper;
  double *d_seq = nullptr, *d_out;
  const int ncol = want_lls ? 6 : 3;
  if ((sequence && (rc = tmp.alloc(&d_seq, (size_t)num * sequence_dims))) || (rc = tmp.alloc(&d_out, (size_t)num * ncol))) return rc;
  if (sequence) HIP_TRY(hipMemcpy(d_seq, sequence, (size_t)num * sequence_dims * sizeof(double), hipMemcpyHostToDevice));
  a.sequence = d_seq;
  a.offset = d_out;
  a.log_nhi = d_out + num;
  a.nhi = d_out + 2 * num;
  if (want_lls) {
    a.lls_offset = d_out + 3 * num;
    a.lls_log_nhi = d_out + 4 * num;
    a.lls_nhi = d_out + 5 * num;
  }
  hipLaunchKernelGGL(gpdla::k_draw_samples, dim3((unsigned)((num + 255) / 256)), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  double *dst[6] = {out->offset, out->log_nhi, out->nhi, out->lls_offset, out->lls_log_nhi, out->lls_nhi};
  for (int c = 0; c < ncol; ++c) HIP_TRY(hipMemcpy(dst[c], d_out + (size_t)c * num, num * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
