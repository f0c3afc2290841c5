// host_condition.hpp -- a single-DLA batch conditioned on fixed absorbers (the contract is in
// include/gpdla.h): the checks of the lists, gpdla_batch_set_fixed_absorbers / _clear_, the launches of
// k_condition_rows and k_condition_mask (condition_kernels.hpp) that gpdla_batch_process and
// gpdla_batch_refine make on such a batch, and the test hook that returns the conditioned rows.
#pragma once

static_assert(GPDLA_MAX_FIXED_ABSORBERS == gpdla::kMaxFixedAbsorbers, "gpdla.h and condition_kernels.hpp disagree");
static_assert(GPDLA_MAX_FIXED_ABSORBERS == gpdla::kSpectraMaxAbsorbers, "the conditioned rows are checked against k_spectra_map's lists");

namespace {

int validate_fixed_absorbers(int64_t nq, const int64_t *offsets, const double *z, const double *log_nhi, double sep) {
  if (nq < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_quasars = %lld must be positive", (long long)nq);
  if (!offsets) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null offsets");
  if (!(sep >= 0.0) || !std::isfinite(sep))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "min_z_separation = %g must be finite and >= 0", sep);
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t n = offsets[q + 1] - offsets[q];
    if (n < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (quasar %lld)", (long long)q);
    if (n > GPDLA_MAX_FIXED_ABSORBERS)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets: quasar %lld lists %lld fixed absorbers, at most %d", (long long)q, (long long)n,
                  GPDLA_MAX_FIXED_ABSORBERS);
  }
  if (offsets[nq] > offsets[0] && (!z || !log_nhi)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null z_dlas / log_nhis");
  for (int64_t q = 0; q < nq; ++q) {
    for (int64_t j = offsets[q]; j < offsets[q + 1]; ++j) {
      if (!std::isfinite(z[j]))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "z_dlas[%lld] = %g of quasar %lld is not finite", (long long)j, z[j], (long long)q);
      if (!std::isfinite(log_nhi[j]))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "log_nhis[%lld] = %g of quasar %lld is not finite", (long long)j, log_nhi[j], (long long)q);
    }
    for (int64_t j = offsets[q]; j < offsets[q + 1]; ++j)
      for (int64_t i = offsets[q]; i < j; ++i)
        if (std::fmax(z[i], z[j]) - std::fmin(z[i], z[j]) < sep)
          return fail(GPDLA_ERR_INVALID_ARGUMENT, "z_dlas[%lld] = %.17g and z_dlas[%lld] = %.17g of quasar %lld are closer than min_z_separation = %g",
                      (long long)i, z[i], (long long)j, z[j], (long long)q, sep);
  }
  return GPDLA_OK;
}

// what a conditioned batch needs of its batch and context: the classes the refine pass serves
int check_conditionable(const gpdla_context *c, const gpdla_batch *b) {
  if (b->md) return fail(GPDLA_ERR_UNSUPPORTED, "fixed absorbers condition single-DLA batches only (uploaded without log_priors_lls)");
  if (c->cfg.contraction_precision == 1) return fail(GPDLA_ERR_UNSUPPORTED, "fixed absorbers are fp64 only (contraction_precision = 1)");
  if (b->k > 40) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d: fixed absorbers serve k <= 40", b->k);
  return GPDLA_OK;
}

int launch_condition_rows(gpdla_context *c, gpdla_batch *b) {
  ConditionRowsArgs a{};
  a.meta = b->d_meta;
  a.lam_pad = b->d_lam;
  a.fx_off = b->fx->d_off;
  a.fx_z = b->fx->d_z;
  a.fx_n = b->fx->d_n;
  a.num_lines = c->cfg.num_lines;
  a.k = b->k;
  a.pix = b->d_pix;
  a.Mi = b->d_Mi;
  hipLaunchKernelGGL(k_condition_rows, dim3((unsigned)b->nq), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

int launch_condition_mask(gpdla_context *c, gpdla_batch *b, const int32_t *rows, int64_t count, const int32_t *status,
                          const double *box, const double *su, int64_t S, double *table) {
  if (count < 1) return GPDLA_OK;
  ConditionMaskArgs a{};
  a.rows = rows;
  a.meta = b->d_meta;
  a.status = status;
  a.box = box;
  a.su = su;
  a.S = S;
  a.fx_off = b->fx->d_off;
  a.fx_z = b->fx->d_z;
  a.sep = b->fx->sep;
  a.table = table;
  hipLaunchKernelGGL(k_condition_mask, dim3((unsigned)count), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// set / clear: the results on the device belong to the previous state of the batch
void condition_changed(gpdla_batch *b) {
  b->processed = false;
  if (b->rf) b->rf->levels = 0;
}

}  // namespace

extern "C" {

int gpdla_fixed_absorbers_validate(int64_t nq, const int64_t *offsets, const double *z_dlas, const double *log_nhis,
                                   double min_z_separation) try {
  return validate_fixed_absorbers(nq, offsets, z_dlas, log_nhis, min_z_separation);
} GPDLA_NO_THROW

int gpdla_batch_set_fixed_absorbers(gpdla_context *c, gpdla_batch *b, const int64_t *offsets, const double *z_dlas,
                                    const double *log_nhis, double min_z_separation, int32_t meanflux_rows) try {
  int rc = check_batch_pair(c, b);
  if (rc || (rc = check_conditionable(c, b))) return rc;
  if (meanflux_rows != 0 && meanflux_rows != 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "meanflux_rows = %d must be 0 or 1", (int)meanflux_rows);
  if ((rc = validate_fixed_absorbers(b->nq, offsets, z_dlas, log_nhis, min_z_separation))) return rc;
  HIP_TRY(hipSetDevice(c->device_id));
  const size_t nq = (size_t)b->nq;
  const int64_t a0 = offsets[0], na = offsets[nq] - a0;
  std::vector<int64_t> off(nq + 1);
  for (size_t q = 0; q <= nq; ++q) off[q] = offsets[q] - a0;
  std::vector<double> nhi((size_t)na);
  for (int64_t j = 0; j < na; ++j) nhi[(size_t)j] = std::pow(10.0, log_nhis[a0 + j]);
  if (!b->fx) b->fx = new FixedAbsorbers();
  FixedAbsorbers *fx = b->fx;
  // kernels of the batch's previous process / refine call may still read the lists
  HIP_TRY(hipEventSynchronize(b->ev_done));
  fx->on = false;
  condition_changed(b);
  if ((rc = reserve(&fx->d_off, &fx->cap_off, nq + 1)) || (rc = reserve(&fx->d_z, &fx->cap_z, nq * GPDLA_MAX_FIXED_ABSORBERS)) ||
      (rc = reserve(&fx->d_n, &fx->cap_n, nq * GPDLA_MAX_FIXED_ABSORBERS)))
    return rc;
  {
    // on the upload stream, beside a sweep of another batch in flight; drained before the host vectors go
    hipStream_t st = c->up_stream;
    StreamDrain drain{st};
    HIP_TRY(hipMemcpyAsync(fx->d_off, off.data(), (nq + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (na > 0) {
      HIP_TRY(hipMemcpyAsync(fx->d_z, z_dlas + a0, (size_t)na * sizeof(double), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(fx->d_n, nhi.data(), (size_t)na * sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
  }
  fx->meanflux = meanflux_rows;
  fx->sep = min_z_separation;
  fx->on = true;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_clear_fixed_absorbers(gpdla_context *c, gpdla_batch *b) try {
  int rc = check_batch_pair(c, b);
  if (rc) return rc;
  if (is_conditioned(b)) {
    b->fx->on = false;
    condition_changed(b);
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_debug_conditioned_rows(gpdla_context *c, gpdla_batch *b, int32_t meanflux_rows, int64_t quasar, double *rows_out,
                                 double *M_out, int64_t capacity_rows, int64_t *num_rows_out) try {
  int rc = check_batch_pair(c, b, rows_out && num_rows_out);
  if (rc || (rc = check_conditionable(c, b)) || (rc = check_unchanged(c, b, true))) return rc;
  if (quasar < 0 || quasar >= b->nq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "quasar %lld outside the batch", (long long)quasar);
  if (capacity_rows < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity_rows");
  HIP_TRY(hipSetDevice(c->device_id));
  // the record plan of gpdla_batch_process (k_prepare copies its offsets into the metadata): a processed batch keeps its plan
  const RecordClass cls = legacy_record_class(b->k, b->k <= 20 ? kRecSlim20 : kRecSlim40);
  if ((rc = plan_records(c, b, record_class_doubles(cls, b->ntiles, false), false))) return rc;
  hipStream_t st = c->stream;
  HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
  const bool conditioned = is_conditioned(b);
  if ((rc = launch_prepare(c, b, conditioned ? b->fx->meanflux != 0 : meanflux_rows != 0))) return rc;
  if (conditioned && (rc = launch_condition_rows(c, b))) return rc;
  HIP_TRY(hipEventRecord(b->ev_done, st));
  QuasarMeta m;
  HIP_TRY(hipMemcpyAsync(&m, b->d_meta + quasar, sizeof(m), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t n = std::min<int64_t>(m.n_u, capacity_rows);
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(rows_out, b->d_pix + m.pix_off, (size_t)n * sizeof(PixelRow), hipMemcpyDeviceToHost, st));
    if (M_out)
      HIP_TRY(hipMemcpyAsync(M_out, b->d_Mi + m.pix_off * b->k, (size_t)n * b->k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  *num_rows_out = n;
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
