// host_spectra.hpp -- model spectra: the per-pixel absorption of listed absorbers,
// the posterior moments of the sampled profile, the GP continuum on a resident batch, and the
// reference's `this_mu` on the model grid.  Kernels: spectra_kernels.hpp.
#pragma once

namespace {

// bytes of partial sums k_spectra_moments may have in flight: the selected quasars are taken in
// groups that fit (results do not depend on the grouping: every quasar is reduced on its own)
constexpr size_t kSpectraPartialBytes = (size_t)256 << 20;

int validate_absorbers(int64_t n, const int64_t *off, const double *z, const double *nhi) {
  if (!off) return GPDLA_OK;
  if (off[0] < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "absorber_offsets[0] = %lld is negative", (long long)off[0]);
  for (int64_t s = 0; s < n; ++s) {
    const int64_t na = off[s + 1] - off[s];
    if (na < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "absorber_offsets must be non-decreasing (entry %lld)", (long long)s);
    if (na > GPDLA_SPECTRA_MAX_ABSORBERS)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "%lld absorbers for entry %lld: at most %d", (long long)na, (long long)s,
                  GPDLA_SPECTRA_MAX_ABSORBERS);
  }
  if (off[n] > off[0] && (!z || !nhi)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "absorbers listed but absorber_z / absorber_nhi is null");
  return GPDLA_OK;
}

int validate_model_spectra(const gpdla_model_spectra_request *rq, int64_t nq, int64_t S, bool has_lls) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  int rc = check_selection(nq, rq->selection, rq->num_selected);
  if (rc) return rc;
  const int known = GPDLA_SPECTRA_MAP | GPDLA_SPECTRA_MOMENTS | GPDLA_SPECTRA_CONTINUUM;
  if (!rq->products || (rq->products & ~known))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "products = %d: a non-empty set of GPDLA_SPECTRA_MAP | _MOMENTS | _CONTINUUM", rq->products);
  if ((rc = validate_absorbers(rq->num_selected, rq->absorber_offsets, rq->absorber_z, rq->absorber_nhi))) return rc;
  if (rq->products & GPDLA_SPECTRA_MOMENTS) {
    if (rq->weights_source != GPDLA_SPECTRA_WEIGHTS_RESIDENT && rq->weights_source != GPDLA_SPECTRA_WEIGHTS_HOST &&
        rq->weights_source != GPDLA_SPECTRA_WEIGHTS_REFINED)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "mean / var absorption need a weights source (resident, host or refined table)");
    if (rq->weights_source == GPDLA_SPECTRA_WEIGHTS_REFINED && rq->sub_dla)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "the refined table is the DLA table: sub_dla has no refined source");
    if (rq->weights_source == GPDLA_SPECTRA_WEIGHTS_HOST && !rq->sample_log_likelihoods)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "weights source is the host table but sample_log_likelihoods is null");
    if (rq->sub_dla && !has_lls)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "sub_dla needs lls_nhi_samples in the context's samples");
    if (S < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "no samples");
  }
  if (rq->capacity < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_model_spectra_validate(const gpdla_model_spectra_request *rq, int64_t num_quasars, int64_t num_samples,
                                 int has_lls_nhi_samples) try {
  return validate_model_spectra(rq, num_quasars, num_samples, has_lls_nhi_samples != 0);
} GPDLA_NO_THROW

int gpdla_batch_unmasked_counts(gpdla_context *c, gpdla_batch *b, int64_t *n_u) try {
  int rc = check_batch_pair(c, b, n_u != nullptr);
  if (rc || (rc = check_unconditioned(b, "unmasked counts")) || (rc = check_unchanged(c, b, true))) return rc;
  HIP_TRY(hipSetDevice(c->device_id));
  std::vector<QuasarMeta> meta;
  if ((rc = spectra_prepare(c, b, b->md != 0, meta))) return rc;
  for (int64_t q = 0; q < b->nq; ++q) n_u[q] = meta[(size_t)q].n_u;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_model_spectra(gpdla_context *c, gpdla_batch *b, const gpdla_model_spectra_request *rq,
                              gpdla_model_spectra *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  if (rc || (rc = check_unconditioned(b, "model spectra")) || (rc = validate_model_spectra(rq, b->nq, b->S, c->d_lls_nhi != nullptr)) || (rc = check_unchanged(c, b, true))) return rc;
  const bool want_map = (rq->products & GPDLA_SPECTRA_MAP) && out->map_absorption;
  const bool want_mom = (rq->products & GPDLA_SPECTRA_MOMENTS) && (out->mean_absorption || out->var_absorption);
  const bool want_cont = (rq->products & GPDLA_SPECTRA_CONTINUUM) && (out->continuum || out->model_flux);
  if (want_mom && rq->weights_source != GPDLA_SPECTRA_WEIGHTS_HOST && (rc = check_processed(b, "resident weights: "))) return rc;
  const bool use_refined = want_mom && rq->weights_source == GPDLA_SPECTRA_WEIGHTS_REFINED;
  RefinedTable refined;
  if (use_refined && (rc = refined_table(c, b, &refined))) return rc;
  const int64_t nsel = rq->num_selected;
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  GridSelection gs;
  std::vector<int64_t> rows;
  std::vector<int32_t> status((size_t)nsel);
  AbsorberLists lists;
  Staging sg(st);
  if ((rc = gs.open(c, b, rq->meanflux != 0, rq->selection, nsel, rq->capacity, out->offsets, sg)) || nsel == 0) return rc;
  const std::vector<int64_t> &sel = gs.sel;
  const int64_t *d_sel = gs.d_sel, *d_off = gs.d_off;
  if ((rc = lists.upload(sg, nsel, rq->absorber_offsets, rq->absorber_z, rq->absorber_nhi))) return rc;
  const size_t tot = (size_t)gs.total;

  // P1 (also the absorption the continuum conditions on)
  double *d_map = nullptr;
  if (want_map || (want_cont && lists.have_abs)) {
    if ((rc = sg.tmp.alloc(&d_map, tot))) return rc;
    if ((rc = launch_spectra_map(c, b, nsel, d_sel, d_off, lists, d_map, st))) return rc;
    if (want_map && (rc = sg.fetch(out->map_absorption, d_map, tot))) return rc;
  }

  // P2
  if (want_mom) {
    const int64_t S = use_refined ? refined.Sr : b->S;  // (refined: the S' refine points)
    double *d_w = nullptr, *d_mean = nullptr, *d_var = nullptr, *d_part = nullptr;
    int32_t *d_flag = nullptr;
    if ((rc = sg.tmp.alloc(&d_w, (size_t)nsel * S)) || (rc = sg.tmp.alloc(&d_flag, (size_t)nsel)) ||
        (rc = sg.tmp.alloc(&d_mean, tot)) || (rc = sg.tmp.alloc(&d_var, tot)))
      return rc;
    if (use_refined) {  // the rows of the resident lambda table, S' apart (a quasar that was not refined has a NaN row)
      int64_t *d_rows = nullptr;
      rows.resize((size_t)nsel);
      for (int64_t s = 0; s < nsel; ++s) rows[(size_t)s] = sel[(size_t)s] * S;
      if ((rc = sg.put(&d_rows, rows.data(), (size_t)nsel)) || (rc = launch_sample_weights(refined.lam, d_rows, S, nsel, d_w, d_flag, st)))
        return rc;
    } else if ((rc = launch_sample_weights(sg, b, gs, rq->weights_source == GPDLA_SPECTRA_WEIGHTS_HOST ? rq->sample_log_likelihoods : nullptr,
                                           rq->sub_dla != 0, rows, d_w, d_flag))) {
      return rc;
    }

    const int chunks = (int)((S + kMomWaves * 64 - 1) / (kMomWaves * 64));
    const int64_t stride = ((std::max<int64_t>(b->max_pix, 1) + 15) / 16) * 16;  // n_u <= stored pixels
    const size_t per_q = (size_t)chunks * 2 * (size_t)stride;
    const int64_t nsub = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(kSpectraPartialBytes / (per_q * sizeof(double)))));
    if ((int64_t)nsub * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
    if ((rc = sg.tmp.alloc(&d_part, (size_t)nsub * per_q))) return rc;
    // (gpdla_context_set_timing: the moments kernels of this call are what gpdla_context_last_sweep_ms reports)
    if ((rc = begin_timing(c, st))) return rc;
    for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
      const int64_t n = std::min(nsub, nsel - s0);
      SpectraMomentsArgs pa;
      pa.meta = b->d_meta;
      pa.lam_pad = b->d_lam;
      pa.offset_samples = use_refined ? c->d_ru : c->d_offset;
      pa.nhi = use_refined ? c->d_rv : rq->sub_dla ? c->d_lls_nhi : c->d_nhi;
      pa.perm = use_refined ? c->d_rperm : c->d_perm;
      pa.sel = d_sel;
      pa.w = d_w;
      pa.S = S;
      pa.num_lines = c->cfg.num_lines;
      pa.s0 = s0;
      pa.chunks = chunks;
      pa.stride = stride;
      pa.part = d_part;
      if (use_refined) {
        SpectraMomentsBoxedArgs ba;
        ba.m = pa;
        ba.rmeta = refined.rmeta;
        ba.box = refined.box;
        ba.rstatus = refined.d_status;
        hipLaunchKernelGGL(k_spectra_moments_boxed, dim3((unsigned)(n * chunks)), dim3(kMomWaves * 64), 0, st, ba);
      } else {
        hipLaunchKernelGGL(k_spectra_moments, dim3((unsigned)(n * chunks)), dim3(kMomWaves * 64), 0, st, pa);
      }
      HIP_TRY(hipGetLastError());
      SpectraCombineArgs ca;
      ca.meta = b->d_meta;
      ca.sel = d_sel;
      ca.flag = d_flag;
      ca.out_off = d_off;
      ca.part = d_part;
      ca.s0 = s0;
      ca.chunks = chunks;
      ca.stride = stride;
      ca.mean = d_mean;
      ca.var = d_var;
      hipLaunchKernelGGL(k_spectra_combine, dim3((unsigned)n), dim3(256), 0, st, ca);
      HIP_TRY(hipGetLastError());
    }
    if ((rc = end_timing(c, st))) return rc;
    if ((rc = sg.fetch(out->mean_absorption, d_mean, tot)) || (rc = sg.fetch(out->var_absorption, d_var, tot))) return rc;
  }

  // P3
  for (int64_t s = 0; s < nsel; ++s) status[(size_t)s] = gs.meta[(size_t)sel[(size_t)s]].status;
  // refined moments of a quasar without a refined row: NaN rows (its lambda row is NaN) and the status bit
  std::vector<uint8_t> not_refined((size_t)nsel, 0);
  if (use_refined)
    for (int64_t s = 0; s < nsel; ++s)
      not_refined[(size_t)s] = status[(size_t)s] == 0 && refined.status[(size_t)sel[(size_t)s]] != 0;
  if (want_cont) {
    double *d_cont = nullptr, *d_flux = nullptr;
    int32_t *d_status = nullptr;
    if ((rc = sg.tmp.alloc(&d_cont, tot)) || (rc = sg.tmp.alloc(&d_flux, tot)) || (rc = sg.tmp.alloc(&d_status, (size_t)nsel))) return rc;
    SpectraContinuumArgs ka;
    ka.meta = b->d_meta;
    ka.pix = b->d_pix;
    ka.Mi = b->d_Mi;
    ka.lam_pad = b->d_lam;
    ka.z_qsos = b->d_z;
    ka.sel = d_sel;
    ka.out_off = d_off;
    ka.absorption = lists.have_abs ? d_map : nullptr;
    ka.g = continuum_model_args(c, rq->meanflux != 0);
    ka.continuum = d_cont;
    ka.model_flux = d_flux;
    ka.status = d_status;
    hipLaunchKernelGGL(k_spectra_continuum, dim3((unsigned)nsel), dim3(256), 0, st, ka);
    HIP_TRY(hipGetLastError());
    if ((rc = sg.fetch(out->continuum, d_cont, tot)) || (rc = sg.fetch(out->model_flux, d_flux, tot)) ||
        (rc = sg.fetch(status.data(), d_status, (size_t)nsel)))
      return rc;
  }
  HIP_TRY(hipStreamSynchronize(st));
  for (int64_t s = 0; s < nsel; ++s)
    if (not_refined[(size_t)s]) status[(size_t)s] |= GPDLA_SPECTRA_NOT_REFINED;
  if (out->status) std::memcpy(out->status, status.data(), (size_t)nsel * sizeof(int32_t));
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_debug_profiles_ms(gpdla_context *c, gpdla_batch *b, double *ms_out) try {
  int rc = check_batch_pair(c, b, ms_out != nullptr);
  if (rc) return rc;
  if (!b->md) return fail(GPDLA_ERR_INVALID_ARGUMENT, "not a multi-DLA batch (upload it with log_priors_lls)");
  if (b->S != c->S || b->k != c->model.k || !c->d_lls_nhi)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "model/samples changed after the batch was uploaded, or no lls_nhi_samples");
  HIP_TRY(hipSetDevice(c->device_id));
  std::lock_guard<std::mutex> multi_lock(c->multi_mu);
  hipStream_t st = c->stream;
  if ((rc = multi_alloc(b))) return rc;
  if ((rc = launch_prepare(c, b, true))) return rc;
  EventPair ev;
  if ((rc = ev.create())) return rc;
  HIP_TRY(hipEventRecord(ev.e0, st));
  const int64_t nq_sub = b->mb->prof_quasars;
  for (int64_t q0 = 0; q0 < b->nq; q0 += nq_sub) {
    ProfilesArgs pa;
    pa.meta = b->d_meta;
    pa.lam_pad = b->d_lam;
    pa.offset_samples = c->d_offset;
    pa.nhi_samples = c->d_nhi;
    pa.lls_nhi_samples = c->d_lls_nhi;
    pa.perm = c->d_perm;
    pa.S = b->S;
    pa.num_lines = c->cfg.num_lines;
    pa.q0 = q0;
    pa.nq_sub = (int32_t)std::min(nq_sub, b->nq - q0);
    pa.stride = b->mb->prof_stride;
    pa.prof = c->d_prof;
    const int64_t waves = (int64_t)pa.nq_sub * ((b->S + 63) / 64);
    hipLaunchKernelGGL(k_profiles, dim3((unsigned)((waves + kProfWaves - 1) / kProfWaves)), dim3(kProfWaves * 64), 0, st, pa);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(ev.e1, st));
  HIP_TRY(hipEventSynchronize(ev.e1));
  float ms = -1.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  *ms_out = (double)ms;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_model_mean(const gpdla_model *model, int64_t num_items, const double *z_qsos, const int64_t *absorber_offsets,
                     const double *absorber_z, const double *absorber_nhi, int num_voigt_lines, int num_forest_lines,
                     int suppressed, double prev_tau_0, double prev_beta, double *out, int device_id) try {
  if (!model || !model->rest_wavelengths || !model->mu || !z_qsos || !out) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null pointer");
  if (model->num_rest_pixels < 1 || num_items < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "empty model grid or negative item count");
  if (num_voigt_lines < 1 || num_voigt_lines > kMaxLines)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_voigt_lines %d outside [1, 31]", num_voigt_lines);
  if (suppressed && (num_forest_lines < 1 || num_forest_lines > kMaxLines))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_forest_lines %d outside [1, 31]", num_forest_lines);
  int rc = validate_absorbers(num_items, absorber_offsets, absorber_z, absorber_nhi);
  if (rc) return rc;
  if (num_items == 0) return GPDLA_OK;
  if ((rc = select_device(device_id))) return rc;
  if ((rc = ensure_line_table(device_id))) return rc;
  const size_t G = (size_t)model->num_rest_pixels, n = (size_t)num_items;
  AbsorberLists lists;
  Staging sg(nullptr);  // the default stream, which the blocking copy of the result waits for
  double *d_rest = nullptr, *d_mu = nullptr, *d_z = nullptr, *d_out = nullptr;
  if ((rc = sg.put(&d_rest, model->rest_wavelengths, G)) || (rc = sg.put(&d_mu, model->mu, G)) || (rc = sg.put(&d_z, z_qsos, n)) ||
      (rc = lists.upload(sg, num_items, absorber_offsets, absorber_z, absorber_nhi, true)) || (rc = sg.tmp.alloc(&d_out, n * G)))
    return rc;
  SpectraModelMeanArgs ma;
  ma.rest = d_rest;
  ma.mu = d_mu;
  ma.G = (int32_t)G;
  ma.num_items = num_items;
  ma.z_qsos = d_z;
  ma.abs_off = lists.d_off;
  ma.abs_z = lists.d_z;
  ma.abs_n = lists.d_nhi;
  ma.num_voigt_lines = num_voigt_lines;
  ma.num_forest_lines = num_forest_lines;
  ma.suppressed = suppressed ? 1 : 0;
  ma.lya_wavelength = 1215.6701;  // set_parameters.m:5
  ma.prev_tau_0 = prev_tau_0;
  ma.prev_beta = prev_beta;
  ma.out = d_out;
  hipLaunchKernelGGL(k_spectra_model_mean, dim3((unsigned)((n * G + 255) / 256)), dim3(256), 0, 0, ma);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out, d_out, n * G * sizeof(double), hipMemcpyDeviceToHost));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
