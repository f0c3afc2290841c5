// host_predictive_flux.hpp -- the posterior predictive flux: per-pixel mean and variance of
// absorption times continuum over the sample tables and the models, on a resident batch.
// Kernels: predictive_flux_kernels.hpp (and k_mc_contract of marginal_continuum_kernels.hpp).
#pragma once

namespace {

// the request as the marginal continuum's, whose checks are the ones to make (validate_marginal_continuum)
gpdla_marginal_continuum_request pf_as_mc_request(const gpdla_predictive_flux_request *rq) {
  gpdla_marginal_continuum_request mq;
  mq.num_selected = rq->num_selected;
  mq.selection = rq->selection;
  mq.weights_source = rq->weights_source;
  mq.sample_log_likelihoods_dla = rq->sample_log_likelihoods_dla;
  mq.sample_log_likelihoods_lls = rq->sample_log_likelihoods_lls;
  mq.model_weights = rq->model_weights;
  mq.meanflux = rq->meanflux;
  mq.sample_coefficients = 0;
  mq.capacity = rq->capacity;
  return mq;
}

int validate_predictive_flux(const gpdla_predictive_flux_request *rq, int64_t nq, int64_t S, bool has_lls, int *tables_out) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  const gpdla_marginal_continuum_request mq = pf_as_mc_request(rq);
  return validate_marginal_continuum(&mq, nq, S, has_lls, tables_out);
}

}  // namespace

extern "C" {

int gpdla_predictive_flux_validate(const gpdla_predictive_flux_request *rq, int64_t num_quasars, int64_t num_samples,
                                   int has_lls_nhi_samples) try {
  return validate_predictive_flux(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, nullptr);
} GPDLA_NO_THROW

int gpdla_batch_predictive_flux(gpdla_context *c, gpdla_batch *b, const gpdla_predictive_flux_request *rq,
                                gpdla_predictive_flux *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  int tables = 0;
  if (rc || (rc = check_unconditioned(b, "predictive flux")) ||
      (rc = validate_predictive_flux(rq, b->nq, b->S, c->d_lls_nhi != nullptr, &tables)) || (rc = check_unchanged(c, b, true)))
    return rc;
  if (tables && rq->weights_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT && (rc = check_processed(b, "resident weights: "))) return rc;
  const int64_t nsel = rq->num_selected, S = b->S;
  const int k = c->model.k, nb = k * (k + 1) / 2, ncol = nb + k;
  if (k > GPDLA_MAX_K) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d > %d", k, GPDLA_MAX_K);
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  std::vector<QuasarMeta> meta;
  if ((rc = spectra_prepare(c, b, rq->meanflux != 0, meta))) return rc;

  std::vector<int64_t> sel((size_t)nsel), off((size_t)nsel + 1, 0);
  for (int64_t s = 0; s < nsel; ++s) {
    sel[(size_t)s] = rq->selection ? rq->selection[s] : s;
    off[(size_t)s + 1] = off[(size_t)s] + meta[(size_t)sel[(size_t)s]].n_u;
  }
  const int64_t total = off[(size_t)nsel];
  std::memcpy(out->offsets, off.data(), ((size_t)nsel + 1) * sizeof(int64_t));
  if (total > rq->capacity)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the selection has %lld grid pixels, capacity is %lld (offsets are written)",
                (long long)total, (long long)rq->capacity);
  if (nsel == 0) return GPDLA_OK;

  // model weights, each row normalised by its sum; per component as a column for the sample kernels
  std::vector<double> pw((size_t)nsel * 3), pcol[2];
  for (int64_t s = 0; s < nsel; ++s) {
    double p[3] = {0.0, 0.0, 1.0};
    if (rq->model_weights) std::memcpy(p, rq->model_weights + 3 * s, sizeof p);
    const double sum = p[0] + p[1] + p[2];
    for (int mm = 0; mm < 3; ++mm) pw[(size_t)s * 3 + mm] = p[mm] / sum;
  }
  std::vector<int64_t> rows[2];
  std::vector<int32_t> status((size_t)nsel);
  Staging sg(st);
  int64_t *d_sel = nullptr, *d_off = nullptr;
  double *d_pw = nullptr;
  if ((rc = sg.put(&d_sel, sel.data(), (size_t)nsel)) || (rc = sg.put(&d_off, off.data(), (size_t)nsel + 1)) ||
      (rc = sg.put(&d_pw, pw.data(), (size_t)nsel * 3)))
    return rc;
  const size_t tot = (size_t)std::max<int64_t>(total, 1);

  // the posterior weights of each table the mixture reaches (k_spectra_weights, as the marginal continuum)
  double *d_w[2] = {nullptr, nullptr}, *d_pm[2] = {nullptr, nullptr}, *d_sums[2] = {nullptr, nullptr};
  int32_t *d_flag[2] = {nullptr, nullptr};
  for (int comp = 0; comp < 2; ++comp) {
    if (!(tables & (1 << comp))) continue;
    const bool lls = comp == 0;
    const double *table;
    rows[comp].resize((size_t)nsel);
    pcol[comp].resize((size_t)nsel);
    for (int64_t s = 0; s < nsel; ++s) pcol[comp][(size_t)s] = pw[(size_t)s * 3 + 1 + comp];
    if (rq->weights_source == GPDLA_SPECTRA_WEIGHTS_HOST) {
      double *d_table = nullptr;
      if ((rc = sg.put(&d_table, lls ? rq->sample_log_likelihoods_lls : rq->sample_log_likelihoods_dla, (size_t)nsel * S))) return rc;
      table = d_table;
      for (int64_t s = 0; s < nsel; ++s) rows[comp][(size_t)s] = s * S;
    } else {
      const SampleTable t = resident_samples(b, lls);
      table = t.table;
      for (int64_t s = 0; s < nsel; ++s) rows[comp][(size_t)s] = sel[(size_t)s] * t.width;
    }
    int64_t *d_rows = nullptr;
    if ((rc = sg.put(&d_rows, rows[comp].data(), (size_t)nsel)) || (rc = sg.put(&d_pm[comp], pcol[comp].data(), (size_t)nsel)) ||
        (rc = sg.tmp.alloc(&d_w[comp], (size_t)nsel * S)) || (rc = sg.tmp.alloc(&d_flag[comp], (size_t)nsel)) ||
        (rc = sg.tmp.alloc(&d_sums[comp], tot * 4)))
      return rc;
    SpectraWeightsArgs wa;
    wa.table = table;
    wa.row_start = d_rows;
    wa.S = S;
    wa.w = d_w[comp];
    wa.flag = d_flag[comp];
    hipLaunchKernelGGL(k_spectra_weights, dim3((unsigned)nsel), dim3(256), 0, st, wa);
    HIP_TRY(hipGetLastError());
  }

  double *d_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // mean, var, within, between, noise
  int32_t *d_status = nullptr;
  for (int j = 0; j < 5; ++j)
    if ((rc = sg.tmp.alloc(&d_out[j], tot))) return rc;
  if ((rc = sg.tmp.alloc(&d_status, (size_t)nsel))) return rc;

  // launch groups: the scratch rows of a group's quasars fit the budget of the marginal continuum
  const int chunks = (int)((S + kMcSolveChunk - 1) / kMcSolveChunk);
  int64_t nsub = nsel;
  double *d_scratch = nullptr;
  int32_t *d_notpd[2] = {nullptr, nullptr}, *d_list = nullptr, *d_count = nullptr;
  if (tables) {
    const size_t per_q = (size_t)S * ncol * sizeof(double);
    nsub = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(mc_scratch_bytes() / per_q)));
    if (nsub * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
    if ((rc = sg.tmp.alloc(&d_scratch, (size_t)nsub * S * ncol)) || (rc = sg.tmp.alloc(&d_list, (size_t)nsub * S)) ||
        (rc = sg.tmp.alloc(&d_count, (size_t)nsub)))
      return rc;
    for (int comp = 0; comp < 2; ++comp)
      if ((tables & (1 << comp)) && (rc = sg.tmp.alloc(&d_notpd[comp], (size_t)nsub * chunks))) return rc;
  }
  PfModelArgs g;
  g.model = c->model;
  g.lya_wavelength = c->cfg.lya_wavelength;
  g.prev_tau_0 = c->cfg.prev_tau_0;
  g.prev_beta = c->cfg.prev_beta;
  g.meanflux = rq->meanflux ? 1 : 0;
  g.num_forest_lines = c->cfg.num_forest_lines;
  // (gpdla_context_set_timing: the kernels of this call are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    int64_t longest = 1;
    for (int64_t s = s0; s < s0 + n; ++s) longest = std::max<int64_t>(longest, meta[(size_t)sel[(size_t)s]].n_u);
    const int64_t tiles = (longest + kPfPixTile - 1) / kPfPixTile;
    if (n * tiles > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
    for (int comp = 0; comp < 2; ++comp) {
      if (!(tables & (1 << comp))) continue;
      McContractArgs ca;
      ca.meta = b->d_meta;
      ca.pix = b->d_pix;
      ca.Mi = b->d_Mi;
      ca.lam_pad = b->d_lam;
      ca.offset_samples = c->d_offset;
      ca.nhi = comp == 0 ? c->d_lls_nhi : c->d_nhi;
      ca.perm = c->d_perm;
      ca.sel = d_sel;
      ca.w = d_w[comp];
      ca.pm = d_pm[comp];
      ca.S = S;
      ca.num_lines = c->cfg.num_lines;
      ca.k = k;
      ca.s0 = s0;
      ca.chunks = 0;
      ca.scratch = d_scratch;
      if ((rc = k <= 20 ? launch_mc_contract<4, 4, 32>(ca, n, S, st) : launch_mc_contract<1, 14, 64>(ca, n, S, st))) return rc;
      McSolveArgs sa;
      sa.meta = b->d_meta;
      sa.perm = c->d_perm;
      sa.sel = d_sel;
      sa.w = d_w[comp];
      sa.pm = d_pm[comp];
      sa.S = S;
      sa.k = k;
      sa.s0 = s0;
      sa.chunks = chunks;
      sa.scratch = d_scratch;
      sa.part = nullptr;
      sa.notpd = d_notpd[comp];
      sa.sample_coef = nullptr;
      hipLaunchKernelGGL(k_pf_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, sa, d_scratch);
      HIP_TRY(hipGetLastError());
      PfLiveArgs la;
      la.meta = b->d_meta;
      la.perm = c->d_perm;
      la.sel = d_sel;
      la.w = d_w[comp];
      la.pm = d_pm[comp];
      la.S = S;
      la.s0 = s0;
      la.list = d_list;
      la.count = d_count;
      hipLaunchKernelGGL(k_pf_live, dim3((unsigned)n), dim3(256), 0, st, la);
      HIP_TRY(hipGetLastError());
      PfPixelsArgs pa;
      pa.meta = b->d_meta;
      pa.pix = b->d_pix;
      pa.lam_pad = b->d_lam;
      pa.z_qsos = b->d_z;
      pa.offset_samples = c->d_offset;
      pa.nhi = ca.nhi;
      pa.perm = c->d_perm;
      pa.sel = d_sel;
      pa.out_off = d_off;
      pa.w = d_w[comp];
      pa.pm = d_pm[comp];
      pa.g = g;
      pa.S = S;
      pa.num_lines = c->cfg.num_lines;
      pa.s0 = s0;
      pa.tiles = (int32_t)tiles;
      pa.scratch = d_scratch;
      pa.list = d_list;
      pa.count = d_count;
      pa.sums = d_sums[comp];
      hipLaunchKernelGGL(k_pf_pixels, dim3((unsigned)(n * tiles)), dim3(256), 0, st, pa);
      HIP_TRY(hipGetLastError());
    }
    PfFinishArgs fa;
    fa.meta = b->d_meta;
    fa.pix = b->d_pix;
    fa.Mi = b->d_Mi;
    fa.lam_pad = b->d_lam;
    fa.z_qsos = b->d_z;
    fa.offsets = b->d_offsets;
    fa.wavelengths = b->d_wl;
    fa.pixel_mask = b->d_mask;
    fa.min_lambda = c->cfg.min_lambda;
    fa.max_lambda = c->cfg.max_lambda;
    fa.sel = d_sel;
    fa.out_off = d_off;
    fa.g = g;
    fa.pw = d_pw;
    for (int comp = 0; comp < 2; ++comp) {
      fa.flag[comp] = d_flag[comp];
      fa.sums[comp] = d_sums[comp];
      fa.notpd[comp] = d_notpd[comp];
    }
    fa.s0 = s0;
    fa.chunks = chunks;
    fa.mean = d_out[0];
    fa.var = d_out[1];
    fa.var_within = d_out[2];
    fa.var_between = d_out[3];
    fa.noise_var = d_out[4];
    fa.status = d_status;
    hipLaunchKernelGGL(k_pf_finish, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out->flux_mean, d_out[0], (size_t)total)) || (rc = sg.fetch(out->flux_var, d_out[1], (size_t)total)) ||
      (rc = sg.fetch(out->flux_var_within, d_out[2], (size_t)total)) || (rc = sg.fetch(out->flux_var_between, d_out[3], (size_t)total)) ||
      (rc = sg.fetch(out->noise_var, d_out[4], (size_t)total)) || (rc = sg.fetch(status.data(), d_status, (size_t)nsel)))
    return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (out->status) std::memcpy(out->status, status.data(), (size_t)nsel * sizeof(int32_t));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
