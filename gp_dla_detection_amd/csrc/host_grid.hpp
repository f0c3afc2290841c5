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

// The refined source of the DLA component (GPDLA_SPECTRA_WEIGHTS_REFINED): the resident tables of the batch's
// last gpdla_batch_refine -- S' unit points, the lambda rows [nq][S'], the refine's copy of the metadata, every quasar's last
// box -- and the refine status of every quasar, read once per call.  refined_table (host_refine.hpp) makes the checks of
// the refined summaries and fills it.
struct RefinedTable {
  int64_t Sr = 0;
  const double *lam = nullptr;        // [nq][Sr]
  const QuasarMeta *rmeta = nullptr;  // [nq]
  const double *box = nullptr;        // quasar q's last box at box + q * kRefineBoxStride
  const int32_t *d_status = nullptr;  // [nq]
  std::vector<int32_t> status;        // [nq] on the host
};
int refined_table(gpdla_context *c, gpdla_batch *b, RefinedTable *out);

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

// ma.nslots < 2: k_mc_contract on ma.c; else k_mc_contract_multi for the model DLA(ma.nslots)
template <int RT, int CPW, int PT>
int launch_mc_contract(const McContractMultiArgs &ma, int64_t n, int64_t S, hipStream_t st) {
  McContractMultiArgs args = ma;
  args.c.chunks = (int32_t)((S + 16 * RT - 1) / (16 * RT));
  if (n * args.c.chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
  const dim3 grid((unsigned)(n * args.c.chunks));
  if (args.nslots >= 2) hipLaunchKernelGGL((k_mc_contract_multi<RT, CPW, PT>), grid, dim3(256), 0, st, args);
  else hipLaunchKernelGGL((k_mc_contract<RT, CPW, PT>), grid, dim3(256), 0, st, args.c);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// k_mc_contract_boxed on the refine points (ba.c.S of them)
template <int RT, int CPW, int PT>
int launch_mc_contract_boxed(const McContractBoxedArgs &ba, int64_t n, hipStream_t st) {
  McContractBoxedArgs args = ba;
  args.c.chunks = (int32_t)((args.c.S + 16 * RT - 1) / (16 * RT));
  if (n * args.c.chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
  hipLaunchKernelGGL((k_mc_contract_boxed<RT, CPW, PT>), dim3((unsigned)(n * args.c.chunks)), dim3(256), 0, st, args);
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
    if (rq.weights_source != GPDLA_SPECTRA_WEIGHTS_RESIDENT && rq.weights_source != GPDLA_SPECTRA_WEIGHTS_HOST &&
        rq.weights_source != GPDLA_SPECTRA_WEIGHTS_REFINED)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "a sampled component needs a weights source (resident, host or refined table)");
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

// What a MixturePlan is built from, once its entry has validated the request.  The mixture has the null component
// and 1 + md sampled ones: comp 0 is the sub-DLA table, comp n model DLA(n), whose sample i absorbs with the product
// of n profiles gathered through the base rows (n >= 2).  The single-DLA entries have md = 1 and no base rows.
struct MixtureSpec {
  int64_t num_selected;
  const int64_t *selection;
  int md;
  bool resident;                    // the tables are the batch's, on the device; else the caller's, [num_selected] quasars
  const double *lls, *dla;          // quasar r's rows start at lls + r * lls_stride ([S]) and dla + r * dla_stride ([md][S])
  int64_t lls_stride, dla_stride;
  const uint32_t *base;             // [.][md - 1][S]
  const double *model_weights;      // host [num_selected][2 + md]; nullptr: `posteriors`, the device's [nq][2 + md]
  const double *posteriors;         // gathered by entry, or (nullptr as well) the row (0, .., 0, 1)
  bool meanflux;
  int64_t capacity;
  const RefinedTable *refined;      // md = 1: DLA(1) runs on the refined table with its own S' samples; nullptr: on `dla`
  bool no_scratch;                  // the product runs no k_mc_contract: no scratch rows, no chunk flags; a group is sized by its weights
};

// of a single-DLA entry; `tables` as validate_mixture gave them (no table is looked up for a mixture that reaches none)
MixtureSpec mixture_spec(const gpdla_batch *b, const MixtureRequest &rq, int tables, const RefinedTable *refined = nullptr) {
  MixtureSpec sp = {};
  sp.refined = refined;
  sp.num_selected = rq.num_selected;
  sp.selection = rq.selection;
  sp.md = 1;
  sp.resident = rq.weights_source != GPDLA_SPECTRA_WEIGHTS_HOST;
  if (sp.resident && tables) {
    const SampleTable lls = resident_samples(b, true), dla = resident_samples(b, false);
    sp.lls = lls.table, sp.lls_stride = lls.width;
    sp.dla = dla.table, sp.dla_stride = dla.width;
  } else {
    sp.lls = rq.sample_log_likelihoods_lls, sp.dla = rq.sample_log_likelihoods_dla;
    sp.lls_stride = sp.dla_stride = b->S;
  }
  sp.model_weights = rq.model_weights;
  sp.meanflux = rq.meanflux != 0;
  sp.capacity = rq.capacity;
  return sp;
}

// A mixture over the sample tables and the models, from the validated request down to the launch groups: the
// selection, the normalised model weights, the scratch rows of k_mc_contract and, group by group, the staged slice of
// host tables and the posterior weights of every component the mixture reaches.  The two products loop
//   for (s0 = 0; s0 < nsel; s0 += nsub) { n = min(nsub, nsel - s0); begin_group(s0, n);
//                                         per reached comp: contract(comp, s0, n), own kernels; finish }
// Everything a kernel of a group indexes by entry is handed to it from the group's first entry on, so the weights and
// the staged slice are the group's own, as in host_spectra_multi.hpp.  The scratch table is ONE group-sized buffer,
// reused component after component.  Host buffers first, the Staging last (its rule).
// A component has a sample count of its own, samples(comp): S, or the S' refine points of DLA(1) on a refined table
// (sp.refined).  What is sized per group -- the scratch rows, the weights, the chunk flags -- is sized by the larger of the
// counts, Smax; a component's rows of weights and of scratch are packed at its own count.  chunks counts the
// kMcSolveChunk-blocks of Smax: the solve kernels run that many blocks for every component (a block past a component's
// last sample writes zero partials and a clear flag), so the finish kernels read one chunk count.
struct MixturePlan {
  gpdla_context *c;
  gpdla_batch *b;
  const MixtureSpec sp;
  hipStream_t st = nullptr;
  int md = 0, ncomp = 0;              // ncomp = 1 + md sampled components
  unsigned reach = 0;                 // bit comp: some row weighs the component
  int64_t nsel = 0, S = 0, Smax = 0, nsub = 0;  // nsub: quasars a launch group
  int k = 0, nb = 0, ncol = 0;        // nb: packed triangle of B; ncol: a scratch row, [vech(B) | v]
  int chunks = 0;                     // kMcSolveChunk samples each
  size_t tot = 1;                     // max(gs.total, 1)
  ContinuumModelArgs g;
  GridSelection gs;
  std::vector<double> pw, pcol, post;  // [nsel][2 + md] normalised; [ncomp][nsel] columns, 0 for an undefined row
  std::vector<int64_t> rows_dla, rows_lls, rows_base;
  std::vector<int32_t> status, flags;
  std::vector<uint8_t> not_refined;    // [nsel] refined source: the DLA component weighs, the quasar has no refined row
  Staging sg;
  double *d_pw = nullptr, *d_pcol = nullptr, *d_w = nullptr, *d_scratch = nullptr, *d_tab_dla = nullptr, *d_tab_lls = nullptr;
  uint32_t *d_tab_base = nullptr;
  int64_t *d_rows_dla = nullptr, *d_rows_lls = nullptr, *d_rows_base = nullptr;
  int32_t *d_flag = nullptr, *d_notpd = nullptr;
  const double *tab_dla = nullptr, *tab_lls = nullptr;
  const uint32_t *tab_base = nullptr;

  MixturePlan(gpdla_context *ctx, gpdla_batch *batch, const MixtureSpec &spec) : c(ctx), b(batch), sp(spec), sg(ctx->stream) {}
  bool reaches(int comp) const { return (reach >> comp) & 1u; }
  bool boxed(int comp) const { return comp == 1 && sp.refined; }
  int64_t samples(int comp) const { return boxed(comp) ? sp.refined->Sr : S; }
  const int32_t *perm(int comp) const { return boxed(comp) ? c->d_rperm : c->d_perm; }
  double *w(int comp) const { return d_w + (size_t)comp * nsub * Smax; }               // [ncomp][nsub][samples(comp)], Smax apart
  const double *pm(int comp, int64_t s0) const { return d_pcol + (size_t)comp * nsel + s0; }
  int32_t *notpd(int comp) const { return d_notpd + (size_t)comp * nsub * chunks; }  // [ncomp][nsub][chunks]
  const double *nhi(int comp) const { return comp == 0 ? c->d_lls_nhi : c->d_nhi; }

  // nsel == 0: GPDLA_OK with the offsets written and nothing else done (the entry returns)
  int open(int64_t *offsets_out) {
    int rc;
    md = sp.md, ncomp = 1 + md;
    nsel = sp.num_selected, S = b->S;
    Smax = std::max(S, samples(1));
    k = c->model.k, nb = k * (k + 1) / 2, ncol = nb + k;
    if (k > GPDLA_MAX_K) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d > %d", k, GPDLA_MAX_K);
    HIP_TRY(hipSetDevice(c->device_id));
    st = c->stream;
    g = continuum_model_args(c, sp.meanflux);
    if ((rc = gs.open(c, b, sp.meanflux, sp.selection, nsel, sp.capacity, offsets_out, sg)) || nsel == 0) return rc;
    tot = (size_t)std::max<int64_t>(gs.total, 1);
    const size_t ncols = (size_t)(2 + md);

    // model weights: the caller's rows, the resident model_posteriors gathered by entry, or the last component alone;
    // each row normalised by its sum, added in component order; a row with a NaN stays NaN
    pw.assign((size_t)nsel * ncols, 0.0);
    if (sp.model_weights) {
      std::memcpy(pw.data(), sp.model_weights, pw.size() * sizeof(double));
    } else if (sp.posteriors) {
      post.resize((size_t)b->nq * ncols);
      HIP_TRY(hipMemcpyAsync(post.data(), sp.posteriors, post.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (int64_t s = 0; s < nsel; ++s)
        std::memcpy(pw.data() + (size_t)s * ncols, post.data() + (size_t)gs.sel[(size_t)s] * ncols, ncols * sizeof(double));
    } else {
      for (int64_t s = 0; s < nsel; ++s) pw[(size_t)s * ncols + ncols - 1] = 1.0;
    }
    pcol.assign((size_t)ncomp * nsel, 0.0);
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
    // refined source: a quasar without a refined row is not evaluated (its lambda row is NaN: the finish kernels write NaN rows)
    not_refined.assign((size_t)nsel, 0);
    if (sp.refined)
      for (int64_t s = 0; s < nsel; ++s)
        if (pcol[(size_t)nsel + s] > 0.0 && sp.refined->status[(size_t)gs.sel[(size_t)s]] != 0) {
          pcol[(size_t)nsel + s] = 0.0;
          not_refined[(size_t)s] = 1;
        }
    if ((reach & 1u) && !c->d_lls_nhi) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the sub-DLA component needs lls_nhi_samples in the context's samples");
    status.resize((size_t)nsel);
    flags.assign((size_t)ncomp * nsel, 0);
    if ((rc = sg.put(&d_pw, pw.data(), pw.size())) || (rc = sg.put(&d_pcol, pcol.data(), pcol.size()))) return rc;

    // launch groups: the scratch rows of a group's quasars fit the budget
    chunks = (int)((Smax + kMcSolveChunk - 1) / kMcSolveChunk);
    nsub = nsel;
    if (reach) {
      const size_t per_q = (size_t)Smax * (sp.no_scratch ? ncomp : ncol) * sizeof(double);
      nsub = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(mc_scratch_bytes() / per_q)));
      if (nsub * chunks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
      if (!sp.no_scratch &&
          ((rc = sg.tmp.alloc(&d_scratch, (size_t)nsub * Smax * ncol)) || (rc = sg.tmp.alloc(&d_notpd, (size_t)ncomp * nsub * chunks))))
        return rc;
      if ((rc = sg.tmp.alloc(&d_w, (size_t)ncomp * nsub * Smax))) return rc;
    }
    if ((rc = sg.tmp.alloc(&d_flag, (size_t)ncomp * nsel))) return rc;
    HIP_TRY(hipMemsetAsync(d_flag, 0, (size_t)ncomp * nsel * sizeof(int32_t), st));

    // where an entry's rows start: in the resident tables, or in the group's staged slice of the host tables
    // (bit 0: the sub-DLA table; any higher bit: the DLA table; from bit 2 on: the base rows, which models n >= 2 alone read)
    const bool need_lls = reach & 1u, need_dla = reach & ~1u, need_base = reach >> 2;
    rows_dla.resize((size_t)nsel), rows_lls.resize((size_t)nsel), rows_base.resize(need_base ? (size_t)nsel : 0);
    for (int64_t s = 0; s < nsel; ++s) {
      const int64_t r = sp.resident ? gs.sel[(size_t)s] : s % nsub;
      rows_dla[(size_t)s] = r * (sp.refined ? sp.refined->Sr : sp.dla_stride);
      rows_lls[(size_t)s] = r * sp.lls_stride;
      if (need_base) rows_base[(size_t)s] = r * (md - 1) * S;
    }
    if ((rc = sg.put(&d_rows_dla, rows_dla.data(), (size_t)nsel)) || (rc = sg.put(&d_rows_lls, rows_lls.data(), (size_t)nsel)) ||
        (need_base && (rc = sg.put(&d_rows_base, rows_base.data(), (size_t)nsel))))
      return rc;
    if (!sp.resident && ((need_dla && (rc = sg.tmp.alloc(&d_tab_dla, (size_t)nsub * sp.dla_stride))) ||
                         (need_lls && (rc = sg.tmp.alloc(&d_tab_lls, (size_t)nsub * sp.lls_stride))) ||
                         (need_base && (rc = sg.tmp.alloc(&d_tab_base, (size_t)nsub * (md - 1) * S)))))
      return rc;
    tab_dla = sp.refined ? sp.refined->lam : sp.resident ? sp.dla : d_tab_dla;
    tab_lls = sp.resident ? sp.lls : d_tab_lls;
    tab_base = sp.resident ? sp.base : d_tab_base;
    return GPDLA_OK;
  }

  // the group's slice of the caller's tables, then the posterior weights of every reached component of its quasars
  int begin_group(int64_t s0, int64_t n) {
    if (!reach) return GPDLA_OK;
    int rc;
    if (!sp.resident) {
      if (reach & ~1u)
        HIP_TRY(hipMemcpyAsync(d_tab_dla, sp.dla + (size_t)s0 * sp.dla_stride, (size_t)n * sp.dla_stride * sizeof(double),
                               hipMemcpyHostToDevice, st));
      if (reach & 1u)
        HIP_TRY(hipMemcpyAsync(d_tab_lls, sp.lls + (size_t)s0 * sp.lls_stride, (size_t)n * sp.lls_stride * sizeof(double),
                               hipMemcpyHostToDevice, st));
      if (reach >> 2)
        HIP_TRY(hipMemcpyAsync(d_tab_base, sp.base + (size_t)s0 * (md - 1) * S, (size_t)n * (md - 1) * S * sizeof(uint32_t),
                               hipMemcpyHostToDevice, st));
    }
    if (reaches(0) && (rc = launch_sample_weights(tab_lls, d_rows_lls + s0, S, n, w(0), d_flag + s0, st))) return rc;
    // DLA(1): row 0 of the quasar's [md][S] table, or its row of the refined table
    if (reaches(1) && (rc = launch_sample_weights(tab_dla, d_rows_dla + s0, samples(1), n, w(1), d_flag + nsel + s0, st))) return rc;
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

  // k_mc_contract(_multi): the scratch rows of component comp for quasars [s0, s0 + n) of the selection
  int contract(int comp, int64_t s0, int64_t n) const {
    McContractMultiArgs ma;
    McContractArgs &ca = ma.c;
    ca.meta = b->d_meta;
    ca.pix = b->d_pix;
    ca.Mi = b->d_Mi;
    ca.lam_pad = b->d_lam;
    ca.offset_samples = boxed(comp) ? c->d_ru : c->d_offset;
    ca.nhi = boxed(comp) ? c->d_rv : nhi(comp);
    ca.perm = perm(comp);
    ca.sel = gs.d_sel + s0;
    ca.w = w(comp);
    ca.pm = pm(comp, s0);
    ca.S = samples(comp);
    ca.num_lines = c->cfg.num_lines;
    ca.k = k;
    ca.s0 = 0;
    ca.chunks = 0;
    ca.scratch = d_scratch;
    ma.base = tab_base;
    ma.base_start = d_rows_base + s0;
    ma.nslots = comp;  // (0, 1: one profile a sample, k_mc_contract itself)
    // k <= 20: 16 column tiles, 64 samples a block; k <= 40: 55 column tiles, 16 samples a block
    if (boxed(comp)) {
      McContractBoxedArgs ba;
      ba.c = ca;
      ba.rmeta = sp.refined->rmeta;
      ba.box = sp.refined->box;
      ba.rstatus = sp.refined->d_status;
      return k <= 20 ? launch_mc_contract_boxed<4, 4, 32>(ba, n, st) : launch_mc_contract_boxed<1, 14, 64>(ba, n, st);
    }
    return k <= 20 ? launch_mc_contract<4, 4, 32>(ma, n, S, st) : launch_mc_contract<1, 14, 64>(ma, n, S, st);
  }

  McSolveArgs solve_args(int comp, int64_t s0) const {
    McSolveArgs sa;
    sa.meta = b->d_meta;
    sa.perm = perm(comp);
    sa.sel = gs.d_sel + s0;
    sa.w = w(comp);
    sa.pm = pm(comp, s0);
    sa.S = samples(comp);
    sa.k = k;
    sa.chunks = chunks;
    sa.scratch = d_scratch;
    sa.part = nullptr;
    sa.notpd = notpd(comp);
    sa.sample_coef = nullptr;
    return sa;
  }

  PfLiveArgs live_args(int comp, int64_t s0, int32_t *d_list, int32_t *d_count) const {
    PfLiveArgs la;
    la.meta = b->d_meta;
    la.perm = perm(comp);
    la.sel = gs.d_sel + s0;
    la.w = w(comp);
    la.pm = pm(comp, s0);
    la.S = samples(comp);
    la.list = d_list;
    la.count = d_count;
    return la;
  }

  // (.p alone for k_pf_pixels: comp < 2; boxed(comp): pixels_boxed_args)
  PfPixelsMultiArgs pixels_args(int comp, int64_t s0, int64_t tiles, const int32_t *d_list, const int32_t *d_count, double *d_sums) const {
    PfPixelsMultiArgs ma;
    PfPixelsArgs &pa = ma.p;
    pa.meta = b->d_meta;
    pa.pix = b->d_pix;
    pa.lam_pad = b->d_lam;
    pa.z_qsos = b->d_z;
    pa.offset_samples = boxed(comp) ? c->d_ru : c->d_offset;
    pa.nhi = boxed(comp) ? c->d_rv : nhi(comp);
    pa.perm = perm(comp);
    pa.sel = gs.d_sel + s0;
    pa.out_off = gs.d_off + s0;
    pa.w = w(comp);
    pa.pm = pm(comp, s0);
    pa.g = g;
    pa.S = samples(comp);
    pa.num_lines = c->cfg.num_lines;
    pa.s0 = 0;
    pa.tiles = (int32_t)tiles;
    pa.scratch = d_scratch;
    pa.list = d_list;
    pa.count = d_count;
    pa.sums = d_sums;
    ma.base = tab_base;
    ma.base_start = d_rows_base + s0;
    ma.nslots = comp;
    return ma;
  }

  PfPixelsBoxedArgs pixels_boxed_args(const PfPixelsArgs &pa) const {
    PfPixelsBoxedArgs ba;
    ba.p = pa;
    ba.rmeta = sp.refined->rmeta;
    ba.box = sp.refined->box;
    ba.rstatus = sp.refined->d_status;
    return ba;
  }

  MixtureArgs mixture_args(int64_t s0) const {
    MixtureArgs mx;
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
    // (a prepare status, or an undefined row, keeps its own value: those rows are NaN for that reason)
    for (int64_t s = 0; s < nsel; ++s)
      if (not_refined[(size_t)s] && status[(size_t)s] == 0) status[(size_t)s] = GPDLA_SPECTRA_NOT_REFINED;
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

}  // namespace
