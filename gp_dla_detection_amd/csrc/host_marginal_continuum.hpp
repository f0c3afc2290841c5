// host_marginal_continuum.hpp -- the marginal continuum: the GP posterior mean and
// variance of the low-rank continuum over the sample tables and the models, on a resident batch.
// Kernels: marginal_continuum_kernels.hpp.
#pragma once

namespace {

// bytes of per-sample [vech(B) | v] rows k_mc_contract may have in flight: the selected quasars are taken
// in groups that fit (results do not depend on the grouping: every quasar is reduced on its own)
constexpr size_t kMcScratchBytes = (size_t)512 << 20;

size_t mc_scratch_bytes() {
#ifdef GPDLA_WITH_LEGACY
  // debug-only (libgpdla_legacy.so): a small budget forces several launch groups at test size
  if (const char *e = std::getenv("GPDLA_MC_SCRATCH_BYTES")) {
    const long long v = std::atoll(e);
    if (v > 0) return (size_t)v;
  }
#endif
  return kMcScratchBytes;
}

// which tables the model weights reach: bit 0 the sub-DLA table, bit 1 the DLA table
int validate_marginal_continuum(const gpdla_marginal_continuum_request *rq, int64_t nq, int64_t S, bool has_lls, int *tables_out) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  int rc = check_selection(nq, rq->selection, rq->num_selected);
  if (rc) return rc;
  int tables = 0;
  if (!rq->model_weights) {
    tables = rq->num_selected > 0 ? 2 : 0;
  } else {
    for (int64_t s = 0; s < rq->num_selected; ++s) {
      const double *p = rq->model_weights + 3 * s;
      double sum = 0.0;
      for (int mm = 0; mm < 3; ++mm) {
        if (!(p[mm] >= 0.0) || !std::isfinite(p[mm]))
          return fail(GPDLA_ERR_INVALID_ARGUMENT, "model_weights[%lld][%d] = %g: weights are finite and not negative", (long long)s, mm, p[mm]);
        sum += p[mm];
      }
      if (!(sum > 0.0) || !std::isfinite(sum))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "model_weights row %lld sums to %g: a row needs a positive finite sum", (long long)s, sum);
      if (p[1] > 0.0) tables |= 1;
      if (p[2] > 0.0) tables |= 2;
    }
  }
  if (tables) {
    if (rq->weights_source != GPDLA_SPECTRA_WEIGHTS_RESIDENT && rq->weights_source != GPDLA_SPECTRA_WEIGHTS_HOST)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "a sampled component needs a weights source (resident table or host table)");
    if (rq->weights_source == GPDLA_SPECTRA_WEIGHTS_HOST) {
      if ((tables & 2) && !rq->sample_log_likelihoods_dla)
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "weights source is the host table but sample_log_likelihoods_dla is null");
      if ((tables & 1) && !rq->sample_log_likelihoods_lls)
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "weights source is the host table but sample_log_likelihoods_lls is null");
    }
    if ((tables & 1) && !has_lls) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the sub-DLA component needs lls_nhi_samples in the context's samples");
    if (S < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "no samples");
  }
  if (rq->sample_coefficients && tables != 1 && tables != 2)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "sample_coefficients are those of ONE sampled component: the model weights reach %s",
                tables == 3 ? "both tables" : "none");
  if (rq->capacity < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");
  if (tables_out) *tables_out = tables;
  return GPDLA_OK;
}

template <int RT, int CPW, int PT>
int launch_mc_contract(const McContractArgs &ca, int64_t n, int64_t S, hipStream_t st) {
  McContractArgs args = ca;
  args.chunks = (int32_t)((S + 16 * RT - 1) / (16 * RT));
  if (n * args.chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
  hipLaunchKernelGGL((k_mc_contract<RT, CPW, PT>), dim3((unsigned)(n * args.chunks)), dim3(256), 0, st, args);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_marginal_continuum_validate(const gpdla_marginal_continuum_request *rq, int64_t num_quasars, int64_t num_samples,
                                      int has_lls_nhi_samples) try {
  return validate_marginal_continuum(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, nullptr);
} GPDLA_NO_THROW

int gpdla_batch_marginal_continuum(gpdla_context *c, gpdla_batch *b, const gpdla_marginal_continuum_request *rq,
                                   gpdla_marginal_continuum *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  int tables = 0;
  if (rc || (rc = check_unconditioned(b, "marginal continuum")) ||
      (rc = validate_marginal_continuum(rq, b->nq, b->S, c->d_lls_nhi != nullptr, &tables)) || (rc = check_unchanged(c, b, true)))
    return rc;
  if (tables && rq->weights_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT && (rc = check_processed(b, "resident weights: "))) return rc;
  const int64_t nsel = rq->num_selected, S = b->S;
  const int k = c->model.k, nb = k * (k + 1) / 2, ncol = nb + k, plen = k + 2 * nb;
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

  // the posterior weights of each table the mixture reaches (k_spectra_weights, as model spectra)
  double *d_w[2] = {nullptr, nullptr}, *d_pm[2] = {nullptr, nullptr};
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
        (rc = sg.tmp.alloc(&d_w[comp], (size_t)nsel * S)) || (rc = sg.tmp.alloc(&d_flag[comp], (size_t)nsel)))
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

  double *d_mean = nullptr, *d_var = nullptr, *d_btw = nullptr, *d_c = nullptr, *d_W = nullptr, *d_V = nullptr, *d_sc = nullptr;
  int32_t *d_status = nullptr;
  if ((rc = sg.tmp.alloc(&d_mean, tot)) || (rc = sg.tmp.alloc(&d_var, tot)) || (rc = sg.tmp.alloc(&d_btw, tot)) ||
      (rc = sg.tmp.alloc(&d_c, (size_t)nsel * k)) || (rc = sg.tmp.alloc(&d_W, (size_t)nsel * nb)) ||
      (rc = sg.tmp.alloc(&d_V, (size_t)nsel * nb)) || (rc = sg.tmp.alloc(&d_status, (size_t)nsel)))
    return rc;
  const bool want_sc = rq->sample_coefficients && out->sample_coefficients;
  if (want_sc && (rc = sg.tmp.alloc(&d_sc, (size_t)nsel * S * k))) return rc;

  // launch groups: the scratch rows of a group's quasars fit the budget
  const int chunks = (int)((S + kMcSolveChunk - 1) / kMcSolveChunk);
  int64_t nsub = nsel;
  double *d_scratch = nullptr, *d_part[2] = {nullptr, nullptr};
  int32_t *d_notpd[2] = {nullptr, nullptr};
  if (tables) {
    const size_t per_q = (size_t)S * ncol * sizeof(double);
    nsub = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(mc_scratch_bytes() / per_q)));
    if (nsub * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
    if ((rc = sg.tmp.alloc(&d_scratch, (size_t)nsub * S * ncol))) return rc;
    for (int comp = 0; comp < 2; ++comp)
      if ((tables & (1 << comp)) &&
          ((rc = sg.tmp.alloc(&d_part[comp], (size_t)nsub * chunks * plen)) || (rc = sg.tmp.alloc(&d_notpd[comp], (size_t)nsub * chunks))))
        return rc;
  }
  // (gpdla_context_set_timing: the three kernels of this call are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
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
      // k <= 20: 16 column tiles, 64 samples a block; k <= 40: 55 column tiles, 16 samples a block
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
      sa.part = d_part[comp];
      sa.notpd = d_notpd[comp];
      sa.sample_coef = want_sc ? d_sc : nullptr;
      hipLaunchKernelGGL(k_mc_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, sa);
      HIP_TRY(hipGetLastError());
    }
    McFinishArgs fa;
    fa.meta = b->d_meta;
    fa.pix = b->d_pix;
    fa.Mi = b->d_Mi;
    fa.lam_pad = b->d_lam;
    fa.z_qsos = b->d_z;
    fa.sel = d_sel;
    fa.out_off = d_off;
    fa.model = c->model;
    fa.lya_wavelength = c->cfg.lya_wavelength;
    fa.prev_tau_0 = c->cfg.prev_tau_0;
    fa.prev_beta = c->cfg.prev_beta;
    fa.meanflux = rq->meanflux ? 1 : 0;
    fa.num_forest_lines = c->cfg.num_forest_lines;
    fa.pw = d_pw;
    for (int comp = 0; comp < 2; ++comp) {
      fa.flag[comp] = d_flag[comp];
      fa.part[comp] = d_part[comp];
      fa.notpd[comp] = d_notpd[comp];
    }
    fa.s0 = s0;
    fa.chunks = chunks;
    fa.mean = d_mean;
    fa.var = d_var;
    fa.var_between = d_btw;
    fa.coef_mean = d_c;
    fa.cov_within = d_W;
    fa.cov_between = d_V;
    fa.status = d_status;
    hipLaunchKernelGGL(k_mc_finish, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out->continuum_mean, d_mean, (size_t)total)) || (rc = sg.fetch(out->continuum_var, d_var, (size_t)total)) ||
      (rc = sg.fetch(out->continuum_var_between, d_btw, (size_t)total)) || (rc = sg.fetch(out->coef_mean, d_c, (size_t)nsel * k)) ||
      (rc = sg.fetch(out->coef_cov_within, d_W, (size_t)nsel * nb)) || (rc = sg.fetch(out->coef_cov_between, d_V, (size_t)nsel * nb)) ||
      (rc = sg.fetch(status.data(), d_status, (size_t)nsel)))
    return rc;
  if (want_sc && (rc = sg.fetch(out->sample_coefficients, d_sc, (size_t)nsel * S * k))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (out->status) std::memcpy(out->status, status.data(), (size_t)nsel * sizeof(int32_t));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
