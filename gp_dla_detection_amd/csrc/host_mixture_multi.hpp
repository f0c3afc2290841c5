// host_mixture_multi.hpp -- the marginal continuum and the posterior predictive flux over all models of a multi-DLA
// run: the mixtures of host_marginal_continuum.hpp and host_predictive_flux.hpp over the components
// (null, sub-DLA table, DLA(1), .., DLA(max_dlas)), from the resident tables of a processed multi-DLA batch or from
// host tables.  Kernels: mixture_multi_kernels.hpp for models of two or more absorbers and the two finishes; the
// sub-DLA table and DLA(1) run k_mc_contract and k_pf_pixels, every component k_mc_solve / k_pf_solve / k_pf_live.
#pragma once

namespace {

// What gpdla_marginal_continuum_multi_request and gpdla_predictive_flux_multi_request share (the same fields)
struct MixtureMultiRequest {
  int64_t num_selected;
  const int64_t *selection;
  int32_t max_dlas, tables_source;
  const double *sample_log_likelihoods_dla;
  const uint32_t *base_sample_inds;
  const double *sample_log_likelihoods_lls, *model_weights;
  int32_t meanflux;
  int64_t capacity;
  template <typename Request>
  explicit MixtureMultiRequest(const Request &q)
      : num_selected(q.num_selected), selection(q.selection), max_dlas(q.max_dlas), tables_source(q.tables_source),
        sample_log_likelihoods_dla(q.sample_log_likelihoods_dla), base_sample_inds(q.base_sample_inds),
        sample_log_likelihoods_lls(q.sample_log_likelihoods_lls), model_weights(q.model_weights), meanflux(q.meanflux),
        capacity(q.capacity) {}
};

// reach_out: the sampled components some row weighs, bit 0 the sub-DLA table, bit n model DLA(n); without
// model_weights (the resident model_posteriors, known only on the device) every one
int validate_mixture_multi(const MixtureMultiRequest &rq, int64_t nq, int64_t S, bool has_lls, int batch_max_dlas,
                           bool batch_processed, unsigned *reach_out) {
  int rc = check_selection(nq, rq.selection, rq.num_selected);
  if (rc) return rc;
  const int md = rq.max_dlas;
  if (md < 1 || md > GPDLA_POSTERIOR_MAX_MODELS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "max_dlas = %d outside [1, %d]", md, GPDLA_POSTERIOR_MAX_MODELS);
  if (S < 1 || S > (1LL << 30)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "need 1 <= num_samples <= 2^30");
  const int ncols = 2 + md;
  unsigned reach = 0;
  if (!rq.model_weights) {
    reach = rq.num_selected > 0 ? (2u << md) - 1u : 0u;
  } else {
    for (int64_t s = 0; s < rq.num_selected; ++s) {
      const double *p = rq.model_weights + (size_t)ncols * (size_t)s;
      bool undefined = false;
      for (int mm = 0; mm < ncols; ++mm) undefined = undefined || p[mm] != p[mm];
      if (undefined) continue;  // (NaN rows and GPDLA_SPECTRA_AVERAGE_UNDEFINED for that quasar, not a refusal)
      double sum = 0.0;
      for (int mm = 0; mm < ncols; ++mm) {
        if (!(p[mm] >= 0.0) || !std::isfinite(p[mm]))
          return fail(GPDLA_ERR_INVALID_ARGUMENT, "model_weights[%lld][%d] = %g: weights are not negative and not infinite", (long long)s, mm, p[mm]);
        sum += p[mm];
      }
      if (!(sum > 0.0) || !std::isfinite(sum))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "model_weights row %lld sums to %g: a row needs a positive finite sum", (long long)s, sum);
      for (int comp = 0; comp <= md; ++comp)
        if (p[1 + comp] > 0.0) reach |= 1u << comp;
    }
  }
  if (rq.tables_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT) {
    if (!batch_max_dlas) return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: not a multi-DLA batch (upload it with log_priors_lls)");
    if (batch_max_dlas != md)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: the batch holds max_dlas = %d, the request says %d", batch_max_dlas, md);
    if (!batch_processed) return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: the batch has not been processed (gpdla_batch_process_multi)");
  } else if (rq.tables_source == GPDLA_SPECTRA_WEIGHTS_HOST) {
    if (!rq.model_weights) return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables need model_weights (the resident model_posteriors go with the resident tables)");
    if ((reach & ~1u) && !rq.sample_log_likelihoods_dla)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables: sample_log_likelihoods_dla is null");
    if ((reach & 1u) && !rq.sample_log_likelihoods_lls)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables: sample_log_likelihoods_lls is null");
    if ((reach >> 2) && !rq.base_sample_inds) return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables: base_sample_inds is null");
    if (rq.base_sample_inds) {
      const size_t nbase = (size_t)rq.num_selected * (size_t)(md - 1) * (size_t)S;
      for (size_t e = 0; e < nbase; ++e)
        if ((int64_t)rq.base_sample_inds[e] > S)
          return fail(GPDLA_ERR_INVALID_ARGUMENT, "base_sample_inds entry %zu = %u exceeds num_samples = %lld", e,
                      rq.base_sample_inds[e], (long long)S);
    }
  } else {
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "tables_source = %d: GPDLA_SPECTRA_WEIGHTS_RESIDENT or _HOST", rq.tables_source);
  }
  if ((reach & 1u) && !has_lls) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the sub-DLA component needs lls_nhi_samples in the context's samples");
  if (rq.capacity < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");
  *reach_out = reach;
  return GPDLA_OK;
}

template <typename Request>
int validate_mixture_multi_request(const Request *rq, int64_t nq, int64_t S, bool has_lls, int batch_max_dlas,
                                   bool batch_processed, unsigned *reach_out) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  return validate_mixture_multi(MixtureMultiRequest(*rq), nq, S, has_lls, batch_max_dlas, batch_processed, reach_out);
}

template <int RT, int CPW, int PT>
int launch_mc_contract_multi(const McContractMultiArgs &ca, int64_t n, int64_t S, hipStream_t st) {
  McContractMultiArgs args = ca;
  args.c.chunks = (int32_t)((S + 16 * RT - 1) / (16 * RT));
  if (n * args.c.chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
  hipLaunchKernelGGL((k_mc_contract_multi<RT, CPW, PT>), dim3((unsigned)(n * args.c.chunks)), dim3(256), 0, st, args);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// MixturePlan (host_grid.hpp) for 1 + max_dlas sampled components: comp 0 is the sub-DLA table, comp n model DLA(n).
// The entry loops
//   for (s0 = 0; s0 < nsel; s0 += nsub) { n = min(nsub, nsel - s0); begin_group(s0, n);
//                                         per reached comp: contract(comp, s0, n), own kernels; finish }
// Everything a kernel of a group indexes by entry is handed to it from the group's first entry on (the kernels' s0 is
// 0), so the weights and the staged slice of host tables are the group's own, as in host_spectra_multi.hpp.  The
// scratch table is ONE group-sized buffer, reused component after component.  Host buffers first, the Staging last.
struct MixtureMultiPlan {
  gpdla_context *c;
  gpdla_batch *b;
  unsigned reach;
  hipStream_t st = nullptr;
  int md = 0, ncomp = 0;              // ncomp = 1 + md sampled components
  bool resident = true;
  int64_t nsel = 0, S = 0, nsub = 0;  // nsub: quasars a launch group
  int k = 0, nb = 0, ncol = 0;
  int chunks = 0;                     // kMcSolveChunk samples each
  size_t tot = 1;
  const MixtureMultiRequest rq;
  GridSelection gs;
  std::vector<double> pw, pcol, post;  // [nsel][2 + md] normalised; [ncomp][nsel] columns, 0 for an undefined row
  std::vector<int64_t> rows_dla, rows_lls, rows_base;
  std::vector<int32_t> status, flags;
  Staging sg;
  double *d_pw = nullptr, *d_pcol = nullptr, *d_w = nullptr, *d_scratch = nullptr, *d_tab_dla = nullptr, *d_tab_lls = nullptr;
  uint32_t *d_tab_base = nullptr;
  int64_t *d_rows_dla = nullptr, *d_rows_lls = nullptr, *d_rows_base = nullptr;
  int32_t *d_flag = nullptr, *d_notpd = nullptr;
  const double *tab_dla = nullptr, *tab_lls = nullptr;
  const uint32_t *tab_base = nullptr;

  MixtureMultiPlan(gpdla_context *ctx, gpdla_batch *batch, const MixtureMultiRequest &request, unsigned reached)
      : c(ctx), b(batch), reach(reached), rq(request), sg(ctx->stream) {}
  bool reaches(int comp) const { return (reach >> comp) & 1u; }
  double *w(int comp) const { return d_w + (size_t)comp * nsub * S; }
  const double *pm(int comp, int64_t s0) const { return d_pcol + (size_t)comp * nsel + s0; }
  int32_t *notpd(int comp) const { return d_notpd + (size_t)comp * nsub * chunks; }

  // nsel == 0: GPDLA_OK with the offsets written and nothing else done (the entry returns)
  int open(int64_t *offsets_out) {
    int rc = check_unchanged(c, b, true);
    if (rc) return rc;
    md = rq.max_dlas, ncomp = 1 + md;
    resident = rq.tables_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT;
    nsel = rq.num_selected, S = b->S;
    k = c->model.k, nb = k * (k + 1) / 2, ncol = nb + k;
    if (k > GPDLA_MAX_K) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d > %d", k, GPDLA_MAX_K);
    HIP_TRY(hipSetDevice(c->device_id));
    st = c->stream;
    if ((rc = gs.open(c, b, rq.meanflux != 0, rq.selection, nsel, rq.capacity, offsets_out, sg)) || nsel == 0) return rc;
    tot = (size_t)std::max<int64_t>(gs.total, 1);
    const size_t ncols = (size_t)(2 + md);

    // model weights: the caller's rows or (validated: a processed multi-DLA batch) the resident model_posteriors
    // gathered by entry; each row normalised by its sum, added in component order; a row with a NaN stays NaN
    pw.resize((size_t)nsel * ncols);
    if (rq.model_weights) {
      std::memcpy(pw.data(), rq.model_weights, pw.size() * sizeof(double));
    } else {
      post.resize((size_t)b->nq * ncols);
      HIP_TRY(hipMemcpyAsync(post.data(), b->mb->post, post.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (int64_t s = 0; s < nsel; ++s)
        std::memcpy(pw.data() + (size_t)s * ncols, post.data() + (size_t)gs.sel[(size_t)s] * ncols, ncols * sizeof(double));
    }
    pcol.assign((size_t)ncomp * nsel, 0.0);
    reach = 0;
    for (int64_t s = 0; s < nsel; ++s) {
      double *p = pw.data() + (size_t)s * ncols;
      double sum = 0.0;
      for (size_t mm = 0; mm < ncols; ++mm) sum += p[mm];
      // (the resident posteriors are not the caller's to get refused: a row that is no distribution is undefined)
      const bool good = sum > 0.0 && std::isfinite(sum);
      for (size_t mm = 0; mm < ncols; ++mm) p[mm] = good ? p[mm] / sum : (double)NAN;
      if (!good) continue;
      for (int comp = 0; comp < ncomp; ++comp) {
        pcol[(size_t)comp * nsel + s] = p[1 + comp];
        if (p[1 + comp] > 0.0) reach |= 1u << comp;
      }
    }
    if ((reach & 1u) && !c->d_lls_nhi) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the sub-DLA component needs lls_nhi_samples in the context's samples");
    status.resize((size_t)nsel);
    flags.assign((size_t)ncomp * nsel, 0);
    if ((rc = sg.put(&d_pw, pw.data(), pw.size())) || (rc = sg.put(&d_pcol, pcol.data(), pcol.size()))) return rc;

    // launch groups: the scratch rows of a group's quasars fit the budget
    chunks = (int)((S + kMcSolveChunk - 1) / kMcSolveChunk);
    nsub = nsel;
    if (reach) {
      const size_t per_q = (size_t)S * ncol * sizeof(double);
      nsub = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(mc_scratch_bytes() / per_q)));
      if (nsub * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
      if ((rc = sg.tmp.alloc(&d_scratch, (size_t)nsub * S * ncol)) || (rc = sg.tmp.alloc(&d_notpd, (size_t)ncomp * nsub * chunks)) ||
          (rc = sg.tmp.alloc(&d_w, (size_t)ncomp * nsub * S)))
        return rc;
    }
    if ((rc = sg.tmp.alloc(&d_flag, (size_t)ncomp * nsel))) return rc;
    HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)ncomp * nsel * sizeof(int32_t), st));

    // where an entry's rows start: in the resident tables, or in the group's staged slice of the host tables
    rows_dla.resize((size_t)nsel), rows_lls.resize((size_t)nsel), rows_base.resize((size_t)nsel);
    for (int64_t s = 0; s < nsel; ++s) {
      const int64_t r = resident ? gs.sel[(size_t)s] : s % nsub;
      rows_dla[(size_t)s] = r * md * S;
      rows_lls[(size_t)s] = r * S;
      rows_base[(size_t)s] = r * (md - 1) * S;
    }
    if ((rc = sg.put(&d_rows_dla, rows_dla.data(), (size_t)nsel)) || (rc = sg.put(&d_rows_lls, rows_lls.data(), (size_t)nsel)) ||
        (rc = sg.put(&d_rows_base, rows_base.data(), (size_t)nsel)))
      return rc;
    if (!resident && reach &&
        ((rc = sg.tmp.alloc(&d_tab_dla, (size_t)nsub * md * S)) || (rc = sg.tmp.alloc(&d_tab_lls, (size_t)nsub * S)) ||
         (rc = sg.tmp.alloc(&d_tab_base, (size_t)nsub * (md > 1 ? md - 1 : 1) * S))))
      return rc;
    tab_dla = resident ? b->mb->sll_dla : d_tab_dla;
    tab_lls = resident ? b->mb->sll_lls : d_tab_lls;
    tab_base = resident ? b->mb->base : d_tab_base;
    return GPDLA_OK;
  }

  // the group's slice of the caller's tables, then the posterior weights of every reached component of its quasars
  int begin_group(int64_t s0, int64_t n) {
    if (!reach) return GPDLA_OK;
    int rc;
    if (!resident) {
      if (reach & ~1u)
        HIP_TRY(hipMemcpyAsync(d_tab_dla, rq.sample_log_likelihoods_dla + (size_t)s0 * md * S, (size_t)n * md * S * sizeof(double),
                               hipMemcpyHostToDevice, st));
      if (reach & 1u)
        HIP_TRY(hipMemcpyAsync(d_tab_lls, rq.sample_log_likelihoods_lls + (size_t)s0 * S, (size_t)n * S * sizeof(double),
                               hipMemcpyHostToDevice, st));
      if (reach >> 2)
        HIP_TRY(hipMemcpyAsync(d_tab_base, rq.base_sample_inds + (size_t)s0 * (md - 1) * S, (size_t)n * (md - 1) * S * sizeof(uint32_t),
                               hipMemcpyHostToDevice, st));
    }
    if (reaches(0) && (rc = launch_sample_weights(tab_lls, d_rows_lls + s0, S, n, w(0), d_flag + s0, st))) return rc;
    // DLA(1): row 0 of the quasar's [max_dlas][S] table
    if (reaches(1) && (rc = launch_sample_weights(tab_dla, d_rows_dla + s0, S, n, w(1), d_flag + nsel + s0, st))) return rc;
    int n_lo = 0, n_hi = 0;
    for (int nn = 2; nn <= md; ++nn)
      if (reaches(nn)) {
        if (!n_lo) n_lo = nn;
        n_hi = nn;
      }
    if (n_lo) {
      SpectraWeightsMultiArgs wa;
      wa.table = tab_dla;
      wa.row_start = d_rows_dla + s0;
      wa.base = tab_base;
      wa.base_start = d_rows_base + s0;
      wa.S = S;
      wa.cap = nsub;
      wa.flag_stride = nsel;
      wa.n_lo = n_lo;
      wa.n_hi = n_hi;
      wa.w = d_w;
      wa.flag = d_flag + s0;
      hipLaunchKernelGGL(k_spectra_weights_multi, dim3((unsigned)(n * (n_hi - n_lo + 1))), dim3(256), 0, st, wa);
      HIP_TRY(hipGetLastError());
    }
    return GPDLA_OK;
  }

  // the scratch rows of component comp for quasars [s0, s0 + n) of the selection
  int contract(int comp, int64_t s0, int64_t n) const {
    McContractMultiArgs ma;
    McContractArgs &ca = ma.c;
    ca.meta = b->d_meta;
    ca.pix = b->d_pix;
    ca.Mi = b->d_Mi;
    ca.lam_pad = b->d_lam;
    ca.offset_samples = c->d_offset;
    ca.nhi = nhi(comp);
    ca.perm = c->d_perm;
    ca.sel = gs.d_sel + s0;
    ca.w = w(comp);
    ca.pm = pm(comp, s0);
    ca.S = S;
    ca.num_lines = c->cfg.num_lines;
    ca.k = k;
    ca.s0 = 0;
    ca.chunks = 0;
    ca.scratch = d_scratch;
    // k <= 20: 16 column tiles, 64 samples a block; k <= 40: 55 column tiles, 16 samples a block
    if (comp < 2) return k <= 20 ? launch_mc_contract<4, 4, 32>(ca, n, S, st) : launch_mc_contract<1, 14, 64>(ca, n, S, st);
    ma.base = tab_base;
    ma.base_start = d_rows_base + s0;
    ma.nslots = comp;
    return k <= 20 ? launch_mc_contract_multi<4, 4, 32>(ma, n, S, st) : launch_mc_contract_multi<1, 14, 64>(ma, n, S, st);
  }
  const double *nhi(int comp) const { return comp == 0 ? c->d_lls_nhi : c->d_nhi; }

  McSolveArgs solve_args(int comp, int64_t s0) const {
    McSolveArgs sa;
    sa.meta = b->d_meta;
    sa.perm = c->d_perm;
    sa.sel = gs.d_sel + s0;
    sa.w = w(comp);
    sa.pm = pm(comp, s0);
    sa.S = S;
    sa.k = k;
    sa.s0 = 0;
    sa.chunks = chunks;
    sa.scratch = d_scratch;
    sa.part = nullptr;
    sa.notpd = notpd(comp);
    sa.sample_coef = nullptr;
    return sa;
  }

  MixtureMultiArgs mixture_args(int64_t s0) const {
    MixtureMultiArgs mx;
    mx.pw = d_pw + (size_t)s0 * (2 + md);
    mx.flag = d_flag + s0;
    mx.notpd = d_notpd;
    mx.flag_stride = nsel;
    mx.notpd_stride = nsub * chunks;
    mx.sampled = ncomp;
    mx.chunks = chunks;
    return mx;
  }

  // after the last group: the status of every entry and which of ITS components of positive weight had no weights
  int close(int32_t *d_status, int32_t *status_out, uint32_t *flags_out) {
    int rc;
    if ((rc = sg.fetch(status.data(), d_status, (size_t)nsel)) || (rc = sg.fetch(flags.data(), d_flag, flags.size()))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    if (status_out) std::memcpy(status_out, status.data(), (size_t)nsel * sizeof(int32_t));
    if (flags_out)
      for (int64_t s = 0; s < nsel; ++s) {
        uint32_t word = 0;
        for (int comp = 0; comp < ncomp; ++comp)
          if (flags[(size_t)comp * nsel + s] && pcol[(size_t)comp * nsel + s] > 0.0)
            word |= comp == 0 ? GPDLA_SPECTRA_MULTI_FLAG_LLS : 1u << (comp - 1);
        flags_out[s] = word;
      }
    return GPDLA_OK;
  }
};

bool batch_multi_processed(const gpdla_batch *b) { return b->md && b->mb && b->mb->processed; }

}  // namespace

extern "C" {

int gpdla_marginal_continuum_multi_validate(const gpdla_marginal_continuum_multi_request *rq, int64_t num_quasars, int64_t num_samples,
                                            int has_lls_nhi_samples, int batch_max_dlas, int batch_processed) try {
  unsigned reach = 0;
  return validate_mixture_multi_request(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, batch_max_dlas, batch_processed != 0, &reach);
} GPDLA_NO_THROW

int gpdla_predictive_flux_multi_validate(const gpdla_predictive_flux_multi_request *rq, int64_t num_quasars, int64_t num_samples,
                                         int has_lls_nhi_samples, int batch_max_dlas, int batch_processed) try {
  unsigned reach = 0;
  return validate_mixture_multi_request(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, batch_max_dlas, batch_processed != 0, &reach);
} GPDLA_NO_THROW

int gpdla_batch_marginal_continuum_multi(gpdla_context *c, gpdla_batch *b, const gpdla_marginal_continuum_multi_request *rq,
                                         gpdla_marginal_continuum_multi *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  unsigned reach = 0;
  if (rc || (rc = check_unconditioned(b, "marginal continuum")) ||
      (rc = validate_mixture_multi_request(rq, b->nq, b->S, c->d_lls_nhi != nullptr, b->md, batch_multi_processed(b), &reach)))
    return rc;
  MixtureMultiPlan plan(c, b, MixtureMultiRequest(*rq), reach);
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  Staging &sg = plan.sg;
  hipStream_t st = plan.st;
  const int64_t nsel = plan.nsel, nsub = plan.nsub, total = plan.gs.total;
  const int k = plan.k, nb = plan.nb, plen = k + 2 * nb, chunks = plan.chunks;
  const size_t tot = plan.tot, part_stride = (size_t)nsub * chunks * plen;

  double *d_mean = nullptr, *d_var = nullptr, *d_btw = nullptr, *d_c = nullptr, *d_W = nullptr, *d_V = nullptr, *d_part = nullptr;
  int32_t *d_status = nullptr;
  if ((rc = sg.tmp.alloc(&d_mean, tot)) || (rc = sg.tmp.alloc(&d_var, tot)) || (rc = sg.tmp.alloc(&d_btw, tot)) ||
      (rc = sg.tmp.alloc(&d_c, (size_t)nsel * k)) || (rc = sg.tmp.alloc(&d_W, (size_t)nsel * nb)) ||
      (rc = sg.tmp.alloc(&d_V, (size_t)nsel * nb)) || (rc = sg.tmp.alloc(&d_status, (size_t)nsel)) ||
      (rc = sg.tmp.alloc(&d_part, (size_t)plan.ncomp * part_stride)))
    return rc;
  // (gpdla_context_set_timing: the kernels of this loop are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    if ((rc = plan.begin_group(s0, n))) return rc;
    for (int comp = 0; comp < plan.ncomp; ++comp) {
      if (!plan.reaches(comp)) continue;
      if ((rc = plan.contract(comp, s0, n))) return rc;
      McSolveArgs sa = plan.solve_args(comp, s0);
      sa.part = d_part + (size_t)comp * part_stride;
      hipLaunchKernelGGL(k_mc_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, sa);
      HIP_TRY(hipGetLastError());
    }
    McFinishMultiArgs fa;
    fa.meta = b->d_meta;
    fa.pix = b->d_pix;
    fa.Mi = b->d_Mi;
    fa.lam_pad = b->d_lam;
    fa.z_qsos = b->d_z;
    fa.sel = plan.gs.d_sel + s0;
    fa.out_off = plan.gs.d_off + s0;
    fa.g = continuum_model_args(c, rq->meanflux != 0);
    fa.mix = plan.mixture_args(s0);
    fa.part = d_part;
    fa.part_stride = (int64_t)part_stride;
    fa.mean = d_mean;
    fa.var = d_var;
    fa.var_between = d_btw;
    fa.coef_mean = d_c + (size_t)s0 * k;
    fa.cov_within = d_W + (size_t)s0 * nb;
    fa.cov_between = d_V + (size_t)s0 * nb;
    fa.status = d_status + s0;
    hipLaunchKernelGGL(k_mc_finish_multi, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out->continuum_mean, d_mean, (size_t)total)) || (rc = sg.fetch(out->continuum_var, d_var, (size_t)total)) ||
      (rc = sg.fetch(out->continuum_var_between, d_btw, (size_t)total)) || (rc = sg.fetch(out->coef_mean, d_c, (size_t)nsel * k)) ||
      (rc = sg.fetch(out->coef_cov_within, d_W, (size_t)nsel * nb)) || (rc = sg.fetch(out->coef_cov_between, d_V, (size_t)nsel * nb)))
    return rc;
  return plan.close(d_status, out->status, out->model_flags);
} GPDLA_NO_THROW

int gpdla_batch_predictive_flux_multi(gpdla_context *c, gpdla_batch *b, const gpdla_predictive_flux_multi_request *rq,
                                      gpdla_predictive_flux_multi *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  unsigned reach = 0;
  if (rc || (rc = check_unconditioned(b, "predictive flux")) ||
      (rc = validate_mixture_multi_request(rq, b->nq, b->S, c->d_lls_nhi != nullptr, b->md, batch_multi_processed(b), &reach)))
    return rc;
  MixtureMultiPlan plan(c, b, MixtureMultiRequest(*rq), reach);
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  Staging &sg = plan.sg;
  hipStream_t st = plan.st;
  const int64_t nsel = plan.nsel, S = plan.S, nsub = plan.nsub, total = plan.gs.total;
  const int chunks = plan.chunks;
  const size_t tot = plan.tot;
  const int64_t *d_sel = plan.gs.d_sel, *d_off = plan.gs.d_off;

  double *d_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // mean, var, within, between, noise
  double *d_sums = nullptr;
  int32_t *d_status = nullptr, *d_list = nullptr, *d_count = nullptr;
  for (int j = 0; j < 5; ++j)
    if ((rc = sg.tmp.alloc(&d_out[j], tot))) return rc;
  if ((rc = sg.tmp.alloc(&d_status, (size_t)nsel)) || (rc = sg.tmp.alloc(&d_sums, (size_t)plan.ncomp * tot * 4)) ||
      (rc = sg.tmp.alloc(&d_list, (size_t)nsub * S)) || (rc = sg.tmp.alloc(&d_count, (size_t)nsub)))
    return rc;
  const ContinuumModelArgs g = continuum_model_args(c, rq->meanflux != 0);
  // (gpdla_context_set_timing: the kernels of this loop are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    int64_t longest = 1;
    for (int64_t s = s0; s < s0 + n; ++s) longest = std::max<int64_t>(longest, plan.gs.meta[(size_t)plan.gs.sel[(size_t)s]].n_u);
    const int64_t tiles = (longest + kPfPixTile - 1) / kPfPixTile;
    if (n * tiles > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
    if ((rc = plan.begin_group(s0, n))) return rc;
    for (int comp = 0; comp < plan.ncomp; ++comp) {
      if (!plan.reaches(comp)) continue;
      if ((rc = plan.contract(comp, s0, n))) return rc;
      const McSolveArgs sa = plan.solve_args(comp, s0);
      hipLaunchKernelGGL(k_pf_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, sa, plan.d_scratch);
      HIP_TRY(hipGetLastError());
      PfLiveArgs la;
      la.meta = b->d_meta;
      la.perm = c->d_perm;
      la.sel = d_sel + s0;
      la.w = plan.w(comp);
      la.pm = plan.pm(comp, s0);
      la.S = S;
      la.s0 = 0;
      la.list = d_list;
      la.count = d_count;
      hipLaunchKernelGGL(k_pf_live, dim3((unsigned)n), dim3(256), 0, st, la);
      HIP_TRY(hipGetLastError());
      PfPixelsMultiArgs ma;
      PfPixelsArgs &pa = ma.p;
      pa.meta = b->d_meta;
      pa.pix = b->d_pix;
      pa.lam_pad = b->d_lam;
      pa.z_qsos = b->d_z;
      pa.offset_samples = c->d_offset;
      pa.nhi = plan.nhi(comp);
      pa.perm = c->d_perm;
      pa.sel = d_sel + s0;
      pa.out_off = d_off + s0;
      pa.w = plan.w(comp);
      pa.pm = plan.pm(comp, s0);
      pa.g = g;
      pa.S = S;
      pa.num_lines = c->cfg.num_lines;
      pa.s0 = 0;
      pa.tiles = (int32_t)tiles;
      pa.scratch = plan.d_scratch;
      pa.list = d_list;
      pa.count = d_count;
      pa.sums = d_sums + (size_t)comp * tot * 4;
      if (comp < 2) {
        hipLaunchKernelGGL(k_pf_pixels, dim3((unsigned)(n * tiles)), dim3(256), 0, st, pa);
      } else {
        ma.base = plan.tab_base;
        ma.base_start = plan.d_rows_base + s0;
        ma.nslots = comp;
        hipLaunchKernelGGL(k_pf_pixels_multi, dim3((unsigned)(n * tiles)), dim3(256), 0, st, ma);
      }
      HIP_TRY(hipGetLastError());
    }
    PfFinishMultiArgs fa;
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
    fa.sel = d_sel + s0;
    fa.out_off = d_off + s0;
    fa.g = g;
    fa.mix = plan.mixture_args(s0);
    fa.sums = d_sums;
    fa.sums_stride = (int64_t)(tot * 4);
    fa.mean = d_out[0];
    fa.var = d_out[1];
    fa.var_within = d_out[2];
    fa.var_between = d_out[3];
    fa.noise_var = d_out[4];
    fa.status = d_status + s0;
    hipLaunchKernelGGL(k_pf_finish_multi, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out->flux_mean, d_out[0], (size_t)total)) || (rc = sg.fetch(out->flux_var, d_out[1], (size_t)total)) ||
      (rc = sg.fetch(out->flux_var_within, d_out[2], (size_t)total)) || (rc = sg.fetch(out->flux_var_between, d_out[3], (size_t)total)) ||
      (rc = sg.fetch(out->noise_var, d_out[4], (size_t)total)))
    return rc;
  return plan.close(d_status, out->status, out->model_flags);
} GPDLA_NO_THROW

}  // extern "C"
