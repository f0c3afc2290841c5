// host_learn.hpp -- learning the quasar model from spectra (learn_kernels.hpp): the training set on
// the rest-frame grid, its column statistics and the PCA covariance.
#pragma once

namespace {

int64_t learn_splits(int64_t work, int64_t per_split, int64_t max_splits) {
  return std::max<int64_t>(1, std::min<int64_t>(max_splits, (work + per_split - 1) / per_split));
}

// mean (mode 0; mode 2: 0 where nobody counts) or std (mode 1) of the columns of x over the quasars with w != 0 (w NULL: all)
int learn_column_pass(const gpdla_training *t, const double *x, const double *w, int mode, double *part,
                      int32_t nsplit, double *out, double *count) {
  LearnColArgs a;
  a.x = x;
  a.w = w;
  a.nq = t->nq;
  a.ld = t->ld;
  a.nsplit = nsplit;
  a.part = part;
  const unsigned blocks = (unsigned)((t->ld + 255) / 256);
  hipLaunchKernelGGL(k_learn_colsum, dim3(blocks, (unsigned)nsplit), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  LearnColFinishArgs f;
  f.part = part;
  f.G = t->G;
  f.ld = t->ld;
  f.nsplit = nsplit;
  f.mode = mode;
  f.out = out;
  f.count = count;
  hipLaunchKernelGGL(k_learn_colfinish, dim3(blocks), dim3(256), 0, 0, f);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// nanmean, centring in place, nanstd: once per handle (caller selected the device)
int learn_column_stats(gpdla_training *t) {
  if (t->centered) return GPDLA_OK;
  const int32_t nsplit = (int32_t)learn_splits(t->nq, 64, 64);
  DeviceTemps tmp;
  double *part = nullptr;
  int rc;
  if ((rc = tmp.alloc(&part, (size_t)nsplit * 3 * t->ld))) return rc;
  if (!t->d_mu && (rc = dev_alloc(&t->d_mu, (size_t)t->ld))) return rc;
  if (!t->d_std && (rc = dev_alloc(&t->d_std, (size_t)t->ld))) return rc;
  if (!t->d_cnt && (rc = dev_alloc(&t->d_cnt, (size_t)t->ld))) return rc;
  if ((rc = learn_column_pass(t, t->d_flux, nullptr, 0, part, nsplit, t->d_mu, t->d_cnt))) return rc;
  const int64_t n = t->nq * t->ld;
  hipLaunchKernelGGL(k_learn_center, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, t->d_flux, t->d_mu, t->nq,
                     t->G, t->ld);
  HIP_TRY(hipGetLastError());
  if ((rc = learn_column_pass(t, t->d_flux, nullptr, 1, part, nsplit, t->d_std, nullptr))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  t->centered = true;
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_training_create_from_spectra(int device_id, const gpdla_spectra *sp, const gpdla_learn_config *cfg,
                                       gpdla_training **out) try {
  if (!out || !sp || !cfg) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (sp->num_quasars < 1 || !sp->offsets || !sp->wavelengths || !sp->flux || !sp->noise_variance ||
      !sp->pixel_mask || !sp->z_qsos)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/empty spectra field");
  const int64_t nq = sp->num_quasars, G = cfg->num_rest_pixels;
  if (G < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_rest_pixels = %lld: the rest grid is empty", (long long)G);
  if (!(cfg->dlambda > 0.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "dlambda must be positive");
  if (cfg->num_forest_lines < 0 || cfg->num_forest_lines > kLearnMaxLines)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_forest_lines = %d outside [0, %d]", cfg->num_forest_lines, kLearnMaxLines);
  if (sp->offsets[0] < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets[0] must not be negative");
  for (int64_t q = 0; q < nq; ++q) {
    if (sp->offsets[q + 1] < sp->offsets[q])
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (quasar %lld)", (long long)q);
    for (int64_t j = sp->offsets[q] + 1; j < sp->offsets[q + 1]; ++j)
      if (!(sp->wavelengths[j] > sp->wavelengths[j - 1]))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "wavelengths of quasar %lld must be strictly increasing (pixel %lld)",
                    (long long)q, (long long)(j - sp->offsets[q]));
  }
  int rc = select_device(device_id);
  if (rc) return rc;
  const int64_t base = sp->offsets[0], total = sp->offsets[nq] - base;
  std::vector<int64_t> offs(nq + 1);
  for (int64_t q = 0; q <= nq; ++q) offs[q] = sp->offsets[q] - base;
  DeviceTemps tmp;
  int64_t *d_off = nullptr;
  double *d_wl = nullptr, *d_fl = nullptr, *d_nv = nullptr, *d_z = nullptr;
  uint8_t *d_mk = nullptr;
  if ((rc = tmp.alloc(&d_off, (size_t)nq + 1)) || (rc = tmp.alloc(&d_wl, (size_t)total)) ||
      (rc = tmp.alloc(&d_fl, (size_t)total)) || (rc = tmp.alloc(&d_nv, (size_t)total)) ||
      (rc = tmp.alloc(&d_mk, (size_t)total)) || (rc = tmp.alloc(&d_z, (size_t)nq)))
    return rc;
  HIP_TRY(hipMemcpy(d_off, offs.data(), (nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_z, sp->z_qsos, nq * sizeof(double), hipMemcpyHostToDevice));
  if (total > 0) {
    HIP_TRY(hipMemcpy(d_wl, sp->wavelengths + base, total * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_fl, sp->flux + base, total * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_nv, sp->noise_variance + base, total * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_mk, sp->pixel_mask + base, total * sizeof(uint8_t), hipMemcpyHostToDevice));
  }
  gpdla_training *t = nullptr;
  if ((rc = training_alloc(device_id, nq, G, &t))) return rc;
  t->from_spectra = true;
  LearnGridArgs a{};
  a.nq = nq;
  a.G = G;
  a.ld = t->ld;
  a.offsets = d_off;
  a.wl = d_wl;
  a.flux = d_fl;
  a.noise = d_nv;
  a.mask = d_mk;
  a.z = d_z;
  a.min_lambda = cfg->min_lambda;
  a.dlambda = cfg->dlambda;
  a.lya_wavelength = cfg->lya_wavelength;
  a.max_noise_variance = cfg->max_noise_variance;
  a.prev_beta = cfg->prev_beta;
  a.nfl = cfg->num_forest_lines > 1 ? cfg->num_forest_lines : 0;
  // the table of set_parameters_multi.m:76-144 in Angstrom (learn_kernels.hpp: the unit decision), and
  // tau0_j = prev_tau_0 f_j / f_lya lambda_j / lambda_lya (learn_qso_model_meanflux.m:111-113, in that order)
#define GPDLA_LEARN_WL(i, wl_cm, f, rate, lead, width) wl_cm * 1e8,
#define GPDLA_LEARN_FS(i, wl_cm, f, rate, lead, width) f,
  static const double wl_a[] = {GPDLA_LYMAN_SERIES(GPDLA_LEARN_WL)};
  static const double fs[] = {GPDLA_LYMAN_SERIES(GPDLA_LEARN_FS)};
#undef GPDLA_LEARN_WL
#undef GPDLA_LEARN_FS
  static_assert(sizeof wl_a / sizeof wl_a[0] == kLearnMaxLines, "31 Lyman lines");
  const double lya_oscillator_strength = 0.416400;  // set_parameters_multi.m:144
  for (int l = 0; l < kLearnMaxLines; ++l) {
    a.line_wl[l] = wl_a[l];
    a.line_tau0[l] = cfg->prev_tau_0 * fs[l] / lya_oscillator_strength * wl_a[l] / cfg->lya_wavelength;
  }
  a.out_flux = t->d_flux;
  a.out_lya = t->d_lya;
  a.out_noise = t->d_noise;
  a.out_loglya = t->d_loglya;
  hipLaunchKernelGGL(k_learn_rest_grid, dim3((unsigned)nq), dim3(256), 0, 0, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    gpdla_training_destroy(t);
    return fail(GPDLA_ERR_HIP, "k_learn_rest_grid failed: %s", hipGetErrorString(e));
  }
  *out = t;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_training_column_stats(gpdla_training *t, double *mu, double *std, int64_t *count) try {
  if (!t) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null training set");
  if (!t->from_spectra)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "column statistics need a training set made by gpdla_training_create_from_spectra");
  HIP_TRY(hipSetDevice(t->device_id));
  int rc = learn_column_stats(t);
  if (rc) return rc;
  if (mu) HIP_TRY(hipMemcpy(mu, t->d_mu, t->G * sizeof(double), hipMemcpyDeviceToHost));
  if (std) HIP_TRY(hipMemcpy(std, t->d_std, t->G * sizeof(double), hipMemcpyDeviceToHost));
  if (count) {
    std::vector<double> c(t->G);
    HIP_TRY(hipMemcpy(c.data(), t->d_cnt, t->G * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t p = 0; p < t->G; ++p) count[p] = (int64_t)c[p];
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_training_pca_covariance(gpdla_training *t, int complete_rows, double *cov, double *count,
                                  int64_t *rows_used) try {
  if (!t || !cov) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (!t->from_spectra)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the PCA covariance needs a training set made by gpdla_training_create_from_spectra");
  HIP_TRY(hipSetDevice(t->device_id));
  int rc = learn_column_stats(t);
  if (rc) return rc;
  const int64_t G = t->G, ld = t->ld, nq = t->nq, PG = ld / 16, npairs = PG * (PG + 1) / 2;
  const int32_t nsplit = (int32_t)learn_splits((nq + 3) / 4, 256, 8);
  DeviceTemps tmp;
  double *d_flags = nullptr, *d_any = nullptr, *d_cmean = nullptr, *d_cpart = nullptr, *d_pP = nullptr,
         *d_pN = nullptr, *d_cov = nullptr, *d_cnt = nullptr;
  if ((rc = tmp.alloc(&d_flags, (size_t)nq)) || (rc = tmp.alloc(&d_any, (size_t)nq)) ||
      (rc = tmp.alloc(&d_pP, (size_t)npairs * nsplit * 256)) || (rc = tmp.alloc(&d_pN, (size_t)npairs * nsplit * 256)) ||
      (rc = tmp.alloc(&d_cov, (size_t)G * G)) || (count && (rc = tmp.alloc(&d_cnt, (size_t)G * G))))
    return rc;
  hipLaunchKernelGGL(k_learn_rowflag, dim3((unsigned)nq), dim3(256), 0, 0, (const double *)t->d_flux, G, ld, d_flags, d_any);
  HIP_TRY(hipGetLastError());
  if (complete_rows) {  // the complete rows' own column mean (pca 'rows','complete' centres what it keeps)
    const int32_t cs = (int32_t)learn_splits(nq, 64, 64);
    if ((rc = tmp.alloc(&d_cmean, (size_t)ld)) || (rc = tmp.alloc(&d_cpart, (size_t)cs * 3 * ld))) return rc;
    // (mode 2: without a complete row the covariance is the empty sum over n_c - 1 = -1, not NaN)
    if ((rc = learn_column_pass(t, t->d_flux, d_flags, 2, d_cpart, cs, d_cmean, nullptr))) return rc;
  }
  LearnGramArgs g;
  g.x = t->d_flux;
  g.offset = complete_rows ? d_cmean : nullptr;
  g.w = complete_rows ? d_flags : nullptr;
  g.nq = nq;
  g.ld = ld;
  g.npairs = npairs;
  g.nsplit = nsplit;
  g.partP = d_pP;
  g.partN = d_pN;
  hipLaunchKernelGGL(k_learn_gram, dim3((unsigned)((npairs * nsplit + 3) / 4)), dim3(256), 0, 0, g);
  HIP_TRY(hipGetLastError());
  LearnGramFinishArgs f;
  f.partP = d_pP;
  f.partN = d_pN;
  f.G = G;
  f.npairs = npairs;
  f.nsplit = nsplit;
  f.cov = d_cov;
  f.count = d_cnt;
  hipLaunchKernelGGL(k_learn_gram_finish, dim3((unsigned)((npairs * 256 + 255) / 256)), dim3(256), 0, 0, f);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(cov, d_cov, (size_t)G * G * sizeof(double), hipMemcpyDeviceToHost));
  if (count) HIP_TRY(hipMemcpy(count, d_cnt, (size_t)G * G * sizeof(double), hipMemcpyDeviceToHost));
  if (rows_used) {
    std::vector<double> fl(nq);
    HIP_TRY(hipMemcpy(fl.data(), complete_rows ? d_flags : d_any, nq * sizeof(double), hipMemcpyDeviceToHost));
    int64_t n = 0;
    for (double v : fl) n += v != 0.0;
    *rows_used = n;
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_training_download(gpdla_training *t, double *flux, double *lya, double *noise) try {
  if (!t) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null training set");
  HIP_TRY(hipSetDevice(t->device_id));
  const int64_t nq = t->nq, G = t->G, ld = t->ld;
  std::vector<double> row((size_t)nq * ld);
  for (auto [src, dst] : {std::make_pair((const double *)t->d_flux, flux), std::make_pair((const double *)t->d_lya, lya),
                          std::make_pair((const double *)t->d_noise, noise)}) {
    if (!dst) continue;
    HIP_TRY(hipMemcpy(row.data(), src, row.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < nq; ++q)  // quasar-major [nq][ld] -> column-major [nq x G]
      for (int64_t p = 0; p < G; ++p) dst[q + p * nq] = row[(size_t)q * ld + p];
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
