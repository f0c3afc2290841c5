// host_grid.hpp -- the front end of the entries that write per-pixel arrays on the unmasked-range grids of
// selected quasars of a resident batch (model spectra, multi-model spectra, the marginal continuum, the
// posterior predictive flux): the selection and its output offsets, the posterior weights of a sample table,
// and what the two mixtures over the sample tables and the models share up to their launch groups.
#pragma once

namespace {

// k_prepare for the batch (its metadata and rows are a pure function of the spectra, the model and
// the configuration: running it again changes nothing a later process call relies on), then the
// metadata on the host
int spectra_prepare(gpdla_context *c, gpdla_batch *b, bool meanflux, std::vector<QuasarMeta> &meta) {
  hipStream_t st = c->stream;
  HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
  // (no record plan is needed: k_prepare copies the planned record offsets into the metadata, and
  // the next process call plans and prepares again before it reads them)
  int rc = launch_prepare(c, b, meanflux);
  if (rc) return rc;
  meta.resize((size_t)b->nq);
  HIP_TRY(hipMemcpyAsync(meta.data(), b->d_meta, (size_t)b->nq * sizeof(QuasarMeta), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return GPDLA_OK;
}

// What the continuum kernels need to evaluate mu_p and m_p at a pixel (continuum_solve.hpp)
ContinuumModelArgs continuum_model_args(const gpdla_context *c, bool meanflux) {
  ContinuumModelArgs g;
  g.model = c->model;
  g.lya_wavelength = c->cfg.lya_wavelength;
  g.prev_tau_0 = c->cfg.prev_tau_0;
  g.prev_beta = c->cfg.prev_beta;
  g.meanflux = meanflux ? 1 : 0;
  g.num_forest_lines = c->cfg.num_forest_lines;
  return g;
}

// The selected quasars of a batch and where each one's pixels start in the flat per-pixel outputs (CSR over
// the unmasked-range grids, n_u pixels each).  Host buffers of asynchronous copies, so it is declared before
// the Staging it uploads through.
struct GridSelection {
  std::vector<QuasarMeta> meta;   // of every quasar of the batch, after k_prepare
  std::vector<int64_t> sel, off;  // [nsel], [nsel + 1]
  int64_t total = 0;              // off[nsel]: the grid pixels of the selection
  int64_t *d_sel = nullptr, *d_off = nullptr;

  // selection == nullptr: the first nsel quasars.  offsets_out is written before the capacity is tested, so
  // that a refused caller learns the size it needs.
  int open(gpdla_context *c, gpdla_batch *b, bool meanflux, const int64_t *selection, int64_t nsel, int64_t capacity,
           int64_t *offsets_out, Staging &sg) {
    int rc = spectra_prepare(c, b, meanflux, meta);
    if (rc) return rc;
    sel.resize((size_t)nsel);
    off.assign((size_t)nsel + 1, 0);
    for (int64_t s = 0; s < nsel; ++s) {
      sel[(size_t)s] = selection ? selection[s] : s;
      off[(size_t)s + 1] = off[(size_t)s] + meta[(size_t)sel[(size_t)s]].n_u;
    }
    total = off[(size_t)nsel];
    std::memcpy(offsets_out, off.data(), ((size_t)nsel + 1) * sizeof(int64_t));
    if (total > capacity)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "the selection has %lld grid pixels, capacity is %lld (offsets are written)",
                  (long long)total, (long long)capacity);
    if ((rc = sg.put(&d_sel, sel.data(), (size_t)nsel))) return rc;
    return sg.put(&d_off, off.data(), (size_t)nsel + 1);
  }
};

// k_spectra_weights: the posterior weights of n entries whose rows of `table` start at d_rows[0 .. n)
int launch_sample_weights(const double *table, const int64_t *d_rows, int64_t S, int64_t n, double *d_w, int32_t *d_flag,
                          hipStream_t st) {
  SpectraWeightsArgs wa;
  wa.table = table;
  wa.row_start = d_rows;
  wa.S = S;
  wa.w = d_w;
  wa.flag = d_flag;
  hipLaunchKernelGGL(k_spectra_weights, dim3((unsigned)n), dim3(256), 0, st, wa);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// ... of the whole selection under one sample table: the caller's host table [nsel][S], staged (entry s's row
// starts at s * S), or -- host_table == nullptr -- the batch's resident one (at sel[s] * width).  `rows` is
// the source of an asynchronous copy: the caller declares it before `sg`.
int launch_sample_weights(Staging &sg, const gpdla_batch *b, const GridSelection &gs, const double *host_table, bool sub_dla,
                          std::vector<int64_t> &rows, double *d_w, int32_t *d_flag) {
  const int64_t nsel = (int64_t)gs.sel.size(), S = b->S;
  const double *table;
  int rc;
  rows.resize((size_t)nsel);
  if (host_table) {
    double *d_table = nullptr;
    if ((rc = sg.put(&d_table, host_table, (size_t)nsel * S))) return rc;
    table = d_table;
    for (int64_t s = 0; s < nsel; ++s) rows[(size_t)s] = s * S;
  } else {
    const SampleTable t = resident_samples(b, sub_dla);
    table = t.table;
    for (int64_t s = 0; s < nsel; ++s) rows[(size_t)s] = gs.sel[(size_t)s] * t.width;
  }
  int64_t *d_rows = nullptr;
  if ((rc = sg.put(&d_rows, rows.data(), (size_t)nsel))) return rc;
  return launch_sample_weights(table, d_rows, S, nsel, d_w, d_flag, sg.st);
}

// bytes of per-sample [vech(B) | v] rows k_mc_contract may have in flight: the selected quasars are taken in
// groups that fit (results do not depend on the grouping: every quasar is reduced on its own)
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

template <int RT, int CPW, int PT>
int launch_mc_contract(const McContractArgs &ca, int64_t n, int64_t S, hipStream_t st) {
  McContractArgs args = ca;
  args.chunks = (int32_t)((S + 16 * RT - 1) / (16 * RT));
  if (n * args.chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
  hipLaunchKernelGGL((k_mc_contract<RT, CPW, PT>), dim3((unsigned)(n * args.chunks)), dim3(256), 0, st, args);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// What gpdla_marginal_continuum_request and gpdla_predictive_flux_request share (the fields have the same names)
struct MixtureRequest {
  int64_t num_selected;
  const int64_t *selection;
  int32_t weights_source;
  const double *sample_log_likelihoods_dla, *sample_log_likelihoods_lls, *model_weights;
  int32_t meanflux;
  int64_t capacity;
  template <typename Request>
  explicit MixtureRequest(const Request &q)
      : num_selected(q.num_selected), selection(q.selection), weights_source(q.weights_source),
        sample_log_likelihoods_dla(q.sample_log_likelihoods_dla), sample_log_likelihoods_lls(q.sample_log_likelihoods_lls),
        model_weights(q.model_weights), meanflux(q.meanflux), capacity(q.capacity) {}
};

// tables_out: which tables the model weights reach, bit 0 the sub-DLA table, bit 1 the DLA table
int validate_mixture(const MixtureRequest &rq, int64_t nq, int64_t S, bool has_lls, int *tables_out) {
  int rc = check_selection(nq, rq.selection, rq.num_selected);
  if (rc) return rc;
  int tables = 0;
  if (!rq.model_weights) {
    tables = rq.num_selected > 0 ? 2 : 0;
  } else {
    for (int64_t s = 0; s < rq.num_selected; ++s) {
      const double *p = rq.model_weights + 3 * s;
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
    if (rq.weights_source != GPDLA_SPECTRA_WEIGHTS_RESIDENT && rq.weights_source != GPDLA_SPECTRA_WEIGHTS_HOST)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "a sampled component needs a weights source (resident table or host table)");
    if (rq.weights_source == GPDLA_SPECTRA_WEIGHTS_HOST) {
      if ((tables & 2) && !rq.sample_log_likelihoods_dla)
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "weights source is the host table but sample_log_likelihoods_dla is null");
      if ((tables & 1) && !rq.sample_log_likelihoods_lls)
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "weights source is the host table but sample_log_likelihoods_lls is null");
    }
    if ((tables & 1) && !has_lls) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the sub-DLA component needs lls_nhi_samples in the context's samples");
    if (S < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "no samples");
  }
  if (rq.capacity < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");
  *tables_out = tables;
  return GPDLA_OK;
}

// A mixture over the sample tables and the models, from the request its entry has validated down to the launch
// groups: the refusals that need the batch, the selection, the normalised model weights, the posterior weights
// of each table the mixture reaches, and the scratch rows of k_mc_contract.  The entry then loops
//   for (s0 = 0; s0 < nsel; s0 += nsub) { n = min(nsub, nsel - s0); per reached table: contract(comp, s0, n), own kernels }
// comp 0 is the sub-DLA table, comp 1 the DLA table.  Host buffers first, the Staging last (its rule).
struct MixturePlan {
  gpdla_context *c;
  gpdla_batch *b;
  const int tables;
  hipStream_t st = nullptr;
  int64_t nsel = 0, S = 0, nsub = 0;  // nsub: quasars a launch group
  int k = 0, nb = 0, ncol = 0;        // nb: packed triangle of B; ncol: a scratch row, [vech(B) | v]
  int chunks = 0;                     // kMcSolveChunk samples each
  size_t tot = 1;                     // max(gs.total, 1)
  GridSelection gs;
  std::vector<double> pw, pcol[2];    // [nsel][3] rows normalised by their sums; a reached component's column
  std::vector<int64_t> rows[2];
  std::vector<int32_t> status;        // [nsel]: where the entry fetches its status
  Staging sg;
  double *d_pw = nullptr, *d_w[2] = {nullptr, nullptr}, *d_pm[2] = {nullptr, nullptr}, *d_scratch = nullptr;
  int32_t *d_flag[2] = {nullptr, nullptr}, *d_notpd[2] = {nullptr, nullptr};

  MixturePlan(gpdla_context *ctx, gpdla_batch *batch, int reached) : c(ctx), b(batch), tables(reached), sg(ctx->stream) {}
  bool reaches(int comp) const { return (tables & (1 << comp)) != 0; }

  // nsel == 0: GPDLA_OK with the offsets written and nothing else done (the entry returns)
  int open(const MixtureRequest &rq, int64_t *offsets_out) {
    int rc = check_unchanged(c, b, true);
    if (rc) return rc;
    if (tables && rq.weights_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT && (rc = check_processed(b, "resident weights: "))) return rc;
    nsel = rq.num_selected, S = b->S;
    k = c->model.k, nb = k * (k + 1) / 2, ncol = nb + k;
    if (k > GPDLA_MAX_K) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d > %d", k, GPDLA_MAX_K);
    HIP_TRY(hipSetDevice(c->device_id));
    st = c->stream;
    if ((rc = gs.open(c, b, rq.meanflux != 0, rq.selection, nsel, rq.capacity, offsets_out, sg)) || nsel == 0) return rc;
    tot = (size_t)std::max<int64_t>(gs.total, 1);

    // model weights, each row normalised by its sum; per component as a column for the sample kernels
    pw.resize((size_t)nsel * 3);
    for (int64_t s = 0; s < nsel; ++s) {
      double p[3] = {0.0, 0.0, 1.0};
      if (rq.model_weights) std::memcpy(p, rq.model_weights + 3 * s, sizeof p);
      const double sum = p[0] + p[1] + p[2];
      for (int mm = 0; mm < 3; ++mm) pw[(size_t)s * 3 + mm] = p[mm] / sum;
    }
    status.resize((size_t)nsel);
    if ((rc = sg.put(&d_pw, pw.data(), (size_t)nsel * 3))) return rc;

    // the posterior weights of each table the mixture reaches (k_spectra_weights, as model spectra)
    const bool host = rq.weights_source == GPDLA_SPECTRA_WEIGHTS_HOST;
    for (int comp = 0; comp < 2; ++comp) {
      if (!reaches(comp)) continue;
      pcol[comp].resize((size_t)nsel);
      for (int64_t s = 0; s < nsel; ++s) pcol[comp][(size_t)s] = pw[(size_t)s * 3 + 1 + comp];
      const double *host_table = !host ? nullptr : comp == 0 ? rq.sample_log_likelihoods_lls : rq.sample_log_likelihoods_dla;
      if ((rc = sg.put(&d_pm[comp], pcol[comp].data(), (size_t)nsel)) || (rc = sg.tmp.alloc(&d_w[comp], (size_t)nsel * S)) ||
          (rc = sg.tmp.alloc(&d_flag[comp], (size_t)nsel)) ||
          (rc = launch_sample_weights(sg, b, gs, host_table, comp == 0, rows[comp], d_w[comp], d_flag[comp])))
        return rc;
    }

    // launch groups: the scratch rows of a group's quasars fit the budget
    chunks = (int)((S + kMcSolveChunk - 1) / kMcSolveChunk);
    nsub = nsel;
    if (tables) {
      const size_t per_q = (size_t)S * ncol * sizeof(double);
      nsub = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(mc_scratch_bytes() / per_q)));
      if (nsub * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
      if ((rc = sg.tmp.alloc(&d_scratch, (size_t)nsub * S * ncol))) return rc;
      for (int comp = 0; comp < 2; ++comp)
        if (reaches(comp) && (rc = sg.tmp.alloc(&d_notpd[comp], (size_t)nsub * chunks))) return rc;
    }
    return GPDLA_OK;
  }

  // k_mc_contract: the scratch rows of table comp for quasars [s0, s0 + n) of the selection
  int contract(int comp, int64_t s0, int64_t n) const {
    McContractArgs ca;
    ca.meta = b->d_meta;
    ca.pix = b->d_pix;
    ca.Mi = b->d_Mi;
    ca.lam_pad = b->d_lam;
    ca.offset_samples = c->d_offset;
    ca.nhi = nhi(comp);
    ca.perm = c->d_perm;
    ca.sel = gs.d_sel;
    ca.w = d_w[comp];
    ca.pm = d_pm[comp];
    ca.S = S;
    ca.num_lines = c->cfg.num_lines;
    ca.k = k;
    ca.s0 = s0;
    ca.chunks = 0;
    ca.scratch = d_scratch;
    // k <= 20: 16 column tiles, 64 samples a block; k <= 40: 55 column tiles, 16 samples a block
    return k <= 20 ? launch_mc_contract<4, 4, 32>(ca, n, S, st) : launch_mc_contract<1, 14, 64>(ca, n, S, st);
  }
  const double *nhi(int comp) const { return comp == 0 ? c->d_lls_nhi : c->d_nhi; }
};

}  // namespace
