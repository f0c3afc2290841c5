// host_preload.hpp -- raw spec-file columns -> the spectra of preloaded_qsos.mat (preload_kernels.hpp;
// DESIGN.md 4.16)
#pragma once

extern "C" {

int gpdla_preload_spectra(int64_t num_quasars, const int64_t *offsets, const float *flux, const float *loglam,
                          const float *ivar, const int32_t *and_mask, const double *z_qsos, uint8_t *filter_flags,
                          const gpdla_preload_config *config, int64_t *out_offsets, double *wavelengths,
                          double *out_flux, double *noise_variance, uint8_t *pixel_mask, double *normalizers,
                          int device_id) try {
  using namespace gpdla;
  if (num_quasars < 0 || !config || !out_offsets)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument or negative quasar count");
  const gpdla_preload_config &c = *config;
  for (double v : {c.loading_min_lambda, c.loading_max_lambda, c.normalization_min_lambda, c.normalization_max_lambda,
                   c.min_lambda, c.max_lambda})
    if (std::isnan(v)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "NaN wavelength threshold");
  if (!(c.loading_min_lambda <= c.min_lambda && c.min_lambda <= c.max_lambda && c.max_lambda <= c.loading_max_lambda))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the loading range [%g, %g] must contain the modelling range [%g, %g]",
                c.loading_min_lambda, c.loading_max_lambda, c.min_lambda, c.max_lambda);
  if (c.min_num_pixels < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative min_num_pixels");
  out_offsets[0] = 0;
  if (num_quasars == 0) return GPDLA_OK;
  if (!offsets || !z_qsos || !filter_flags || !normalizers) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null per-quasar argument");
  if (num_quasars > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 quasars in one call");
  const int64_t n = num_quasars;
  if (offsets[0] != 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets[0] must be 0");
  for (int64_t i = 0; i < n; ++i) {
    if (offsets[i + 1] < offsets[i]) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (quasar %lld)", (long long)i);
    if (offsets[i + 1] - offsets[i] > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "quasar %lld has more than 2^31 - 1 pixels", (long long)i);
  }
  const int64_t total = offsets[n];
  if (total > 0 && (!flux || !loglam || !ivar || !and_mask || !wavelengths || !out_flux || !noise_variance || !pixel_mask))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null pixel arrays");
  int rc = select_device(device_id);
  if (rc) return rc;
  DeviceTemps tmp;
  int64_t *d_off, *d_out_off;
  float *d_raw;
  int32_t *d_and, *d_count;
  double *d_z, *d_norm, *d_stage, *d_out;
  uint8_t *d_flags, *d_stage_m, *d_out_m;
  if ((rc = tmp.alloc(&d_off, (size_t)n + 1)) || (rc = tmp.alloc(&d_out_off, (size_t)n + 1)) ||
      (rc = tmp.alloc(&d_raw, (size_t)3 * total)) || (rc = tmp.alloc(&d_and, (size_t)total)) ||
      (rc = tmp.alloc(&d_count, (size_t)n)) || (rc = tmp.alloc(&d_z, (size_t)n)) || (rc = tmp.alloc(&d_norm, (size_t)n)) ||
      (rc = tmp.alloc(&d_stage, (size_t)3 * total)) || (rc = tmp.alloc(&d_out, (size_t)3 * total)) ||
      (rc = tmp.alloc(&d_flags, (size_t)n)) || (rc = tmp.alloc(&d_stage_m, (size_t)total)) ||
      (rc = tmp.alloc(&d_out_m, (size_t)total)))
    return rc;
  HIP_TRY(hipMemcpy(d_off, offsets, (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (total > 0) {
    HIP_TRY(hipMemcpy(d_raw, flux, total * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_raw + total, loglam, total * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_raw + 2 * total, ivar, total * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_and, and_mask, total * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(d_z, z_qsos, n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_flags, filter_flags, n * sizeof(uint8_t), hipMemcpyHostToDevice));
  PreloadArgs a{d_off, d_raw, d_raw + total, d_raw + 2 * total, d_and, d_z, d_flags,
                c.loading_min_lambda, c.loading_max_lambda, c.normalization_min_lambda, c.normalization_max_lambda,
                c.min_lambda, c.max_lambda, c.min_num_pixels,
                d_count, d_stage, d_stage + total, d_stage + 2 * total, d_stage_m, d_norm};
  hipLaunchKernelGGL(k_preload, dim3((unsigned)n), dim3(256), 0, 0, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_preload_offsets, dim3(1), dim3(256), 0, 0, n, (const int32_t *)d_count, d_out_off);
  HIP_TRY(hipGetLastError());
  PreloadPackArgs p{d_off, d_out_off, d_count, d_stage, d_stage + total, d_stage + 2 * total, d_stage_m,
                    d_out, d_out + total, d_out + 2 * total, d_out_m};
  hipLaunchKernelGGL(k_preload_pack, dim3((unsigned)n), dim3(256), 0, 0, p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out_offsets, d_out_off, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(filter_flags, d_flags, n * sizeof(uint8_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(normalizers, d_norm, n * sizeof(double), hipMemcpyDeviceToHost));
  const int64_t kept = out_offsets[n];
  if (kept < 0 || kept > total) return fail(GPDLA_ERR_HOST, "kept pixel count %lld outside [0, %lld]", (long long)kept, (long long)total);
  if (kept > 0) {
    HIP_TRY(hipMemcpy(wavelengths, d_out, kept * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_flux, d_out + total, kept * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(noise_variance, d_out + 2 * total, kept * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pixel_mask, d_out_m, kept * sizeof(uint8_t), hipMemcpyDeviceToHost));
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
