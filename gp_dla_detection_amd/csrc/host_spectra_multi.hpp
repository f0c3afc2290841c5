// host_spectra_multi.hpp -- model spectra of a multi-DLA run: the posterior moments of the
// sampled absorption of every model DLA(1 .. max_dlas) and of the sub-DLA model, and their average over the
// models.  Kernels: spectra_multi_kernels.hpp (models of two or more absorbers, the model average) and
// spectra_kernels.hpp (DLA(1), the sub-DLA model and every combine).
#pragma once

namespace {

int validate_model_spectra_multi(const gpdla_model_spectra_multi_request *rq, int64_t nq, int64_t S, bool has_lls,
                                 int batch_max_dlas, bool batch_processed) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  int rc = check_selection(nq, rq->selection, rq->num_selected);
  if (rc) return rc;
  const int known = GPDLA_SPECTRA_MULTI_MODELS | GPDLA_SPECTRA_MULTI_AVERAGE;
  if (!rq->products || (rq->products & ~known))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "products = %d: a non-empty set of GPDLA_SPECTRA_MULTI_MODELS | _AVERAGE", rq->products);
  const int md = rq->max_dlas;
  if (md < 1 || md > GPDLA_POSTERIOR_MAX_MODELS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "max_dlas = %d outside [1, %d]", md, GPDLA_POSTERIOR_MAX_MODELS);
  if (rq->first_model < 1 || rq->last_model > md || rq->first_model > rq->last_model)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "models %d .. %d outside 1 .. max_dlas = %d", rq->first_model, rq->last_model, md);
  if (S < 1 || S > (1LL << 30)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "need 1 <= num_samples <= 2^30");
  if (!has_lls) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the sub-DLA model needs lls_nhi_samples in the context's samples");
  if (rq->tables_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT) {
    if (!batch_max_dlas) return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: not a multi-DLA batch (upload it with log_priors_lls)");
    if (batch_max_dlas != md)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: the batch holds max_dlas = %d, the request says %d", batch_max_dlas, md);
    if (!batch_processed) return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: the batch has not been processed (gpdla_batch_process_multi)");
  } else if (rq->tables_source == GPDLA_SPECTRA_WEIGHTS_HOST) {
    if (!rq->sample_log_likelihoods_dla || !rq->sample_log_likelihoods_lls || (md > 1 && !rq->base_sample_inds))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables: sample_log_likelihoods_dla, sample_log_likelihoods_lls%s must be given",
                  md > 1 ? " and base_sample_inds" : "");
    if ((rq->products & GPDLA_SPECTRA_MULTI_AVERAGE) && !rq->model_weights)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "the model average of host tables needs model_weights");
    const size_t nbase = (size_t)rq->num_selected * (size_t)(md - 1) * (size_t)S;
    for (size_t e = 0; e < nbase; ++e)
      if ((int64_t)rq->base_sample_inds[e] > S)
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "base_sample_inds entry %zu = %u exceeds num_samples = %lld", e,
                    rq->base_sample_inds[e], (long long)S);
  } else {
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "tables_source = %d: GPDLA_SPECTRA_WEIGHTS_RESIDENT or _HOST", rq->tables_source);
  }
  if (rq->capacity < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_model_spectra_multi_validate(const gpdla_model_spectra_multi_request *rq, int64_t num_quasars, int64_t num_samples,
                                       int has_lls_nhi_samples, int batch_max_dlas, int batch_processed) try {
  return validate_model_spectra_multi(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, batch_max_dlas, batch_processed != 0);
} GPDLA_NO_THROW

int gpdla_batch_model_spectra_multi(gpdla_context *c, gpdla_batch *b, const gpdla_model_spectra_multi_request *rq,
                                    gpdla_model_spectra_multi *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  if (rc || (rc = check_unconditioned(b, "model spectra")) ||
      (rc = validate_model_spectra_multi(rq, b->nq, b->S, c->d_lls_nhi != nullptr, b->md, b->md && b->mb && b->mb->processed)) ||
      (rc = check_unchanged(c, b, true)))
    return rc;
  const bool resident = rq->tables_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT;
  const bool want_avg = (rq->products & GPDLA_SPECTRA_MULTI_AVERAGE) != 0;
  const bool want_models = (rq->products & GPDLA_SPECTRA_MULTI_MODELS) != 0;
  const bool out_lls = want_models && (out->mean_absorption_lls || out->var_absorption_lls);
  const int md = rq->max_dlas;
  // the models whose moments are formed: the average needs every one
  const bool do_lls = want_avg || out_lls;
  const int n_first = want_avg ? 1 : rq->first_model, n_last = want_avg ? md : rq->last_model;
  const int64_t nsel = rq->num_selected, S = b->S;
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  // the host buffers of the asynchronous copies first, then the Staging (its rule)
  GridSelection gs;
  std::vector<double> weights;
  std::vector<int64_t> rows_dla((size_t)nsel), rows_lls((size_t)nsel), rows_base((size_t)nsel);
  std::vector<int32_t> status((size_t)nsel), flags;
  Staging sg(st);
  if ((rc = gs.open(c, b, rq->meanflux != 0, rq->selection, nsel, rq->capacity, out->offsets, sg)) || nsel == 0) return rc;
  const std::vector<int64_t> &sel = gs.sel;
  int64_t *d_sel = gs.d_sel, *d_off = gs.d_off;
  const size_t tot = (size_t)gs.total, ncols = (size_t)(2 + md);

  // groups of entries whose partial sums (every model's) fit kSpectraPartialBytes
  const int chunks = (int)((S + kMomWaves * 64 - 1) / (kMomWaves * 64));
  const int64_t stride = ((std::max<int64_t>(b->max_pix, 1) + 15) / 16) * 16;  // n_u <= stored pixels
  const size_t per_q = (size_t)chunks * 2 * (size_t)stride, nrows = (size_t)(1 + md);
  const int64_t cap = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(kSpectraPartialBytes / (per_q * nrows * sizeof(double)))));
  if (cap * md * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");

  // the model weights of the entries
  if (want_avg) {
    weights.resize((size_t)nsel * ncols);
    if (rq->model_weights) {
      std::memcpy(weights.data(), rq->model_weights, weights.size() * sizeof(double));
    } else {  // (validated: a processed multi-DLA batch) its model_posteriors, gathered by entry
      std::vector<double> post((size_t)b->nq * ncols);
      HIP_TRY(hipMemcpyAsync(post.data(), b->mb->post, post.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (int64_t s = 0; s < nsel; ++s)
        std::memcpy(weights.data() + (size_t)s * ncols, post.data() + (size_t)sel[(size_t)s] * ncols, ncols * sizeof(double));
    }
  }

  // where an entry's rows start: in the resident tables, or in the group's staged slice of the host tables
  for (int64_t s = 0; s < nsel; ++s) {
    const int64_t r = resident ? sel[(size_t)s] : s % cap;
    rows_dla[(size_t)s] = r * md * S;
    rows_lls[(size_t)s] = r * S;
    rows_base[(size_t)s] = r * (md - 1) * S;
  }
  flags.assign(nrows * (size_t)nsel, 0);
  for (int64_t s = 0; s < nsel; ++s) status[(size_t)s] = gs.meta[(size_t)sel[(size_t)s]].status;

  int64_t *d_rows_dla = nullptr, *d_rows_lls = nullptr, *d_rows_base = nullptr;
  double *d_weights = nullptr, *d_w = nullptr, *d_part = nullptr, *d_planes = nullptr, *d_lls = nullptr, *d_avg = nullptr;
  double *d_tab_dla = nullptr, *d_tab_lls = nullptr;
  uint32_t *d_tab_base = nullptr;
  int32_t *d_flag = nullptr, *d_status = nullptr;
  if ((rc = sg.put(&d_rows_dla, rows_dla.data(), (size_t)nsel)) || (rc = sg.put(&d_rows_lls, rows_lls.data(), (size_t)nsel)) ||
      (rc = sg.put(&d_rows_base, rows_base.data(), (size_t)nsel)) ||
      (rc = sg.tmp.alloc(&d_w, nrows * (size_t)cap * S)) || (rc = sg.tmp.alloc(&d_flag, nrows * (size_t)nsel)) ||
      (rc = sg.tmp.alloc(&d_part, nrows * (size_t)cap * per_q)) || (rc = sg.tmp.alloc(&d_planes, 2 * (size_t)md * tot)) ||
      (rc = sg.tmp.alloc(&d_lls, 2 * tot)) || (rc = sg.tmp.alloc(&d_avg, 2 * tot)) || (rc = sg.tmp.alloc(&d_status, (size_t)nsel)))
    return rc;
  if (want_avg && (rc = sg.put(&d_weights, weights.data(), weights.size()))) return rc;
  if (!resident && ((rc = sg.tmp.alloc(&d_tab_dla, (size_t)cap * md * S)) || (rc = sg.tmp.alloc(&d_tab_lls, (size_t)cap * S)) ||
                    (rc = sg.tmp.alloc(&d_tab_base, (size_t)cap * (md > 1 ? md - 1 : 1) * S))))
    return rc;
  HIP_TRY(hipMemsetAsync(d_flag, 0, nrows * (size_t)nsel * sizeof(int32_t), st));
  HIP_TRY(hipMemsetAsync(d_planes, 0xFF, 2 * (size_t)md * tot * sizeof(double), st));  // NaN: a model that was not asked for
  const double *tab_dla = resident ? b->mb->sll_dla : d_tab_dla, *tab_lls = resident ? b->mb->sll_lls : d_tab_lls;
  const uint32_t *tab_base = resident ? b->mb->base : d_tab_base;
  double *d_mean_models = d_planes, *d_var_models = d_planes + (size_t)md * tot;

  // the existing single-profile path for one row of the group: weights, moments, combine
  auto single_profile = [&](int row, int64_t g0, int64_t n, const double *table, const int64_t *d_rows, const double *nhi) -> int {
    double *w = d_w + (size_t)row * cap * S;
    int rc = launch_sample_weights(table, d_rows + g0, S, n, w, d_flag + (size_t)row * nsel + g0, st);
    if (rc) return rc;
    SpectraMomentsArgs pa;
    pa.meta = b->d_meta;
    pa.lam_pad = b->d_lam;
    pa.offset_samples = c->d_offset;
    pa.nhi = nhi;
    pa.perm = c->d_perm;
    pa.sel = d_sel + g0;
    pa.w = w;
    pa.S = S;
    pa.num_lines = c->cfg.num_lines;
    pa.s0 = 0;
    pa.chunks = chunks;
    pa.stride = stride;
    pa.part = d_part + (size_t)row * cap * per_q;
    hipLaunchKernelGGL(k_spectra_moments, dim3((unsigned)(n * chunks)), dim3(kMomWaves * 64), 0, st, pa);
    HIP_TRY(hipGetLastError());
    return GPDLA_OK;
  };
  auto combine = [&](int row, int64_t g0, int64_t n, double *mean, double *var) -> int {
    SpectraCombineArgs ca;
    ca.meta = b->d_meta;
    ca.sel = d_sel + g0;
    ca.flag = d_flag + (size_t)row * nsel + g0;
    ca.out_off = d_off + g0;
    ca.part = d_part + (size_t)row * cap * per_q;
    ca.s0 = 0;
    ca.chunks = chunks;
    ca.stride = stride;
    ca.mean = mean;
    ca.var = var;
    hipLaunchKernelGGL(k_spectra_combine, dim3((unsigned)n), dim3(256), 0, st, ca);
    HIP_TRY(hipGetLastError());
    return GPDLA_OK;
  };

  // (gpdla_context_set_timing: the launches of this loop are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t g0 = 0; g0 < nsel; g0 += cap) {
    const int64_t n = std::min(cap, nsel - g0);
    if (!resident) {  // the group's slice of the caller's tables
      HIP_TRY(hipMemcpyAsync(d_tab_dla, rq->sample_log_likelihoods_dla + (size_t)g0 * md * S, (size_t)n * md * S * sizeof(double),
                             hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_tab_lls, rq->sample_log_likelihoods_lls + (size_t)g0 * S, (size_t)n * S * sizeof(double),
                             hipMemcpyHostToDevice, st));
      if (md > 1)
        HIP_TRY(hipMemcpyAsync(d_tab_base, rq->base_sample_inds + (size_t)g0 * (md - 1) * S,
                               (size_t)n * (md - 1) * S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    }
    if (do_lls) {
      if ((rc = single_profile(0, g0, n, tab_lls, d_rows_lls, c->d_lls_nhi))) return rc;
      if ((rc = combine(0, g0, n, d_lls, d_lls + tot))) return rc;
    }
    if (n_first == 1) {  // DLA(1): row 0 of the quasar's [max_dlas][S] table, one profile a sample
      if ((rc = single_profile(1, g0, n, tab_dla, d_rows_dla, c->d_nhi))) return rc;
      if ((rc = combine(1, g0, n, d_mean_models, d_var_models))) return rc;
    }
    const int n_lo = std::max(n_first, 2);
    if (n_last >= n_lo) {
      const int nm = n_last - n_lo + 1;
      SpectraWeightsMultiArgs wa;
      wa.table = tab_dla;
      wa.row_start = d_rows_dla + g0;
      wa.base = tab_base;
      wa.base_start = d_rows_base + g0;
      wa.S = S;
      wa.cap = cap;
      wa.n_lo = n_lo;
      wa.n_hi = n_last;
      wa.w = d_w;
      wa.flag = d_flag + g0;
      wa.flag_stride = nsel;
      hipLaunchKernelGGL(k_spectra_weights_multi, dim3((unsigned)(n * nm)), dim3(256), 0, st, wa);
      HIP_TRY(hipGetLastError());
      SpectraMomentsMultiArgs pa;
      pa.meta = b->d_meta;
      pa.lam_pad = b->d_lam;
      pa.offset_samples = c->d_offset;
      pa.nhi = c->d_nhi;
      pa.perm = c->d_perm;
      pa.sel = d_sel + g0;
      pa.base = tab_base;
      pa.base_start = d_rows_base + g0;
      pa.w = d_w;
      pa.flag = d_flag + g0;
      pa.flag_stride = nsel;
      pa.S = S;
      pa.cap = cap;
      pa.num_lines = c->cfg.num_lines;
      pa.n_lo = n_lo;
      pa.n_hi = n_last;
      pa.chunks = chunks;
      pa.stride = stride;
      pa.part = d_part;
      hipLaunchKernelGGL(k_spectra_moments_multi, dim3((unsigned)(n * nm * chunks)), dim3(kMomWaves * 64), 0, st, pa);
      HIP_TRY(hipGetLastError());
      for (int nn = n_lo; nn <= n_last; ++nn)
        if ((rc = combine(nn, g0, n, d_mean_models + (size_t)(nn - 1) * tot, d_var_models + (size_t)(nn - 1) * tot))) return rc;
    }
    if (want_avg) {
      SpectraModelAverageArgs aa;
      aa.meta = b->d_meta;
      aa.sel = d_sel + g0;
      aa.out_off = d_off + g0;
      aa.flag = d_flag + g0;
      aa.flag_stride = nsel;
      aa.weights = d_weights + (size_t)g0 * ncols;
      aa.part = d_part;
      aa.cap = cap;
      aa.md = md;
      aa.chunks = chunks;
      aa.stride = stride;
      aa.expected = d_avg;
      aa.expected_var = d_avg + tot;
      aa.status = d_status + g0;
      hipLaunchKernelGGL(k_spectra_model_average, dim3((unsigned)n), dim3(256), 0, st, aa);
      HIP_TRY(hipGetLastError());
    }
  }
  if ((rc = end_timing(c, st))) return rc;

  if (want_models) {
    for (int nn = 1; nn <= md; ++nn) {  // plane nn - 1 of the caller's [max_dlas][capacity] arrays; NaN outside first .. last
      const double *mean = d_mean_models + (size_t)(nn - 1) * tot, *var = d_var_models + (size_t)(nn - 1) * tot;
      if (nn < rq->first_model || nn > rq->last_model) {
        // (with the average every model was formed: hand out only what was asked for)
        for (double *plane : {out->mean_absorption_models, out->var_absorption_models})
          if (plane) std::fill(plane + (size_t)(nn - 1) * (size_t)rq->capacity, plane + (size_t)(nn - 1) * (size_t)rq->capacity + tot, (double)NAN);
        continue;
      }
      if ((rc = sg.fetch(out->mean_absorption_models ? out->mean_absorption_models + (size_t)(nn - 1) * (size_t)rq->capacity : nullptr, mean, tot)) ||
          (rc = sg.fetch(out->var_absorption_models ? out->var_absorption_models + (size_t)(nn - 1) * (size_t)rq->capacity : nullptr, var, tot)))
        return rc;
    }
    if (out_lls && ((rc = sg.fetch(out->mean_absorption_lls, d_lls, tot)) || (rc = sg.fetch(out->var_absorption_lls, d_lls + tot, tot))))
      return rc;
  }
  if (want_avg) {
    if ((rc = sg.fetch(out->expected_absorption, d_avg, tot)) || (rc = sg.fetch(out->expected_var_absorption, d_avg + tot, tot)) ||
        (rc = sg.fetch(status.data(), d_status, (size_t)nsel)))
      return rc;
  }
  if ((rc = sg.fetch(flags.data(), d_flag, nrows * (size_t)nsel))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (out->status) std::memcpy(out->status, status.data(), (size_t)nsel * sizeof(int32_t));
  if (out->model_flags)
    for (int64_t s = 0; s < nsel; ++s) {
      uint32_t word = flags[(size_t)s] ? GPDLA_SPECTRA_MULTI_FLAG_LLS : 0u;
      for (int nn = 1; nn <= md; ++nn)
        if (flags[(size_t)nn * (size_t)nsel + (size_t)s]) word |= 1u << (nn - 1);
      out->model_flags[s] = word;
    }
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
