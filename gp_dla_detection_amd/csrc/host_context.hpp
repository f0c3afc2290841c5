// host_context.hpp -- contexts and batches: the two handles of include/gpdla.h, the model and the
// samples in HBM, upload and reload of a batch of spectra into its arena.
#pragma once

struct gpdla_context {
  int device_id = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // Copy streams: uploads and downloads run beside a sweep in flight on `stream`, so a host
  // pipeline can upload batch i+1 and download batch i-1 while batch i is swept (one thread each:
  // the entry points of ONE context may be called concurrently as long as each batch is touched
  // by one thread at a time).
  hipStream_t up_stream = nullptr, down_stream = nullptr;
  std::mutex mu;  // guards `batches`
  // model
  bool has_model = false;
  ModelDev model{};
  double *d_rest = nullptr, *d_mu = nullptr, *d_M = nullptr, *d_log_omega = nullptr;
  // samples
  bool has_samples = false;
  int64_t S = 0;
  double *d_offset = nullptr, *d_nhi = nullptr, *d_log_nhi = nullptr, *d_lls_nhi = nullptr;
  int32_t *d_perm = nullptr;
  // the refine pass (host_refine.hpp): the range of the log N table, the table itself where the samples
  // came without one (log10 of nhi_samples, taken by the host), and the unit-square point set with the
  // order of u (the boxed sweep's perm) and the stable ranks of u and v (the refined summaries)
  double log_nhi_lo = NAN, log_nhi_hi = NAN;
  double *d_log_nhi_derived = nullptr;
  int64_t Sr = 0;
  double *d_ru = nullptr, *d_rv = nullptr;
  int32_t *d_rperm = nullptr;
  std::vector<double> h_ru, h_rv;
  int64_t refine_points_gen = 0;  // counts gpdla_context_set_refine_points calls: a refined batch remembers its set
  gpdla_config cfg{};
  // timing
  bool timing = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool have_timing = false;
  // batches uploaded through this context and not yet destroyed.  A batch points back at its
  // context; destroying the context first orphans them (ctx = nullptr) instead of leaving that
  // pointer dangling, so gpdla_batch_destroy is safe in either order.
  std::vector<gpdla_batch *> batches;
  // The multi-DLA profile table (k_profiles -> k_sweep_multi, up to cfg.multi_profile_bytes, 16 GiB
  // by default) is scratch of one process call: it belongs to the context, is allocated once and
  // grows only.  multi_mu keeps two threads' gpdla_batch_process_multi calls on this context from
  // interleaving their launches (the launches of one call are ordered on `stream`).
  double *d_prof = nullptr;
  size_t prof_capacity = 0;  // doubles
  std::mutex multi_mu;
};

struct gpdla_batch {
  gpdla_context *ctx = nullptr;
  int device_id = 0;
  hipEvent_t ev_done = nullptr;  // recorded on the compute stream behind the last kernel of a process call
  // capacities (elements) of the device arrays below: gpdla_batch_reload re-fills a batch in
  // place and reallocates only what has grown, so a pipeline's batch slots do no hipMalloc/hipFree
  // (hipFree waits for the whole device) in the steady state
  // Every array below except the record pool is carved out of ONE device allocation (arena): a
  // batch slot costs two hipMalloc / hipFree in its life, not eighteen (a hipFree waits for the
  // whole device; on the PCIe-inclusive path the frees of three slots were 1.5 % of a 2048-quasar run)
  void *arena = nullptr;
  struct {
    size_t arena = 0, records = 0;  // bytes; elements
  } cap;
  // Record plan (plan_records): the K-step records of the batch's quasars live in ONE pool of at most
  // cfg.record_pool_bytes; quasars are taken in dealing order (h_order: decreasing length) and cut
  // into groups whose records fit, each group built and swept in turn.
  std::vector<int32_t> h_order;                            // host copy of d_order
  std::vector<int64_t> h_recs;                             // records a quasar occupies (K-steps + 1), by quasar
  std::vector<int64_t> h_rec_off;                          // planned pool offset (in records), by quasar
  std::vector<std::pair<int64_t, int64_t>> groups;         // [g0, g1) ranges of h_order
  int64_t *d_rec_off = nullptr;
  int64_t plan_per_step = 0, plan_budget = -1, plan_pool_records = 0;  // what the current plan was made for
  int64_t nq = 0, S = 0, total_pix = 0;
  int64_t *d_offsets = nullptr;
  double *d_wl = nullptr, *d_flux = nullptr, *d_nv = nullptr, *d_z = nullptr;
  uint8_t *d_mask = nullptr;
  double *d_lp_no = nullptr, *d_lp_dla = nullptr;
  QuasarMeta *d_meta = nullptr;
  int32_t *d_order = nullptr;  // quasar indices by decreasing pixel count (dealing order of k_sweep)
  PixelRow *d_pix = nullptr;
  double *d_Mi = nullptr, *d_lam = nullptr, *d_records = nullptr;
  double *d_sample_ll = nullptr, *d_ll_no = nullptr, *d_summary = nullptr;
  int64_t pool_rows = 0, max_pix = 0;
  int32_t k = 0, tiles_w = 0, ntiles = 0;
  // multi-DLA batch (uploaded with log_priors_lls): result tables, allocated by the first
  // gpdla_batch_process_multi and kept for the life of the batch
  int32_t md = 0;  // max_dlas the priors were uploaded for; 0 = single-DLA batch
  bool processed = false;  // single-DLA batch: gpdla_batch_process has run on the current spectra
  struct MultiBuffers *mb = nullptr;
  struct RefineBuffers *rf = nullptr;  // the refine pass's tables, allocated by the first gpdla_batch_refine
  struct FixedAbsorbers *fx = nullptr;  // gpdla_batch_set_fixed_absorbers (host_condition.hpp); kept across reloads
};

// The fixed absorbers a single-DLA batch is conditioned on: CSR lists per quasar in HBM,
// allocated by the first gpdla_batch_set_fixed_absorbers and grown only.  `on` is what makes the batch a
// conditioned one; a reload or gpdla_batch_clear_fixed_absorbers turns it off and keeps the arrays.
struct FixedAbsorbers {
  bool on = false;
  int32_t meanflux = 0;     // rows prepared as the multi-DLA driver prepares them
  double sep = 0.0;         // min_z_separation of the call
  int64_t *d_off = nullptr; // [nq + 1]
  double *d_z = nullptr, *d_n = nullptr;  // redshifts, column densities
  size_t cap_off = 0, cap_z = 0, cap_n = 0;
  ~FixedAbsorbers() {
    if (d_off) (void)hipFree(d_off);
    if (d_z) (void)hipFree(d_z);
    if (d_n) (void)hipFree(d_n);
  }
};

// What gpdla_batch_refine keeps per batch (host_refine.hpp): tables indexed by the batch's quasar, kept
// across reloads while they suffice.
struct RefineBuffers {
  void *arena = nullptr;
  size_t cap_bytes = 0;
  int64_t nq = 0, Sr = 0;              // what the arena is laid out for
  double *box = nullptr;               // [nq][kRefineBoxStride]
  QuasarMeta *rmeta = nullptr;         // [nq]
  double *ell = nullptr, *lam = nullptr;  // [nq][Sr] the last level's l' and lambda
  double *ll_scratch = nullptr;        // [nq] the boxed sweep's null-model row
  double *terms = nullptr;             // [nq][kRefineTerms][2]
  double *scal = nullptr;              // [nq][kRefineScalars]
  int32_t *status = nullptr;           // [nq]
  int32_t *rows = nullptr;             // [nq] the selected quasars in dealing order
  std::vector<int32_t> h_rows;         // source of the asynchronous copy into `rows`
  hipEvent_t ev_rows = nullptr;        // behind that copy: h_rows may be rewritten once it has run
  int32_t levels = 0;                  // of the last call; 0: none since the last (re)load
  int64_t points_gen = 0;              // gpdla_context::refine_points_gen of the last call
  ~RefineBuffers() {
    if (ev_rows) (void)hipEventDestroy(ev_rows);
    if (arena) (void)hipFree(arena);
  }
};

struct MultiBuffers {
  double *sll_dla = nullptr, *sll_lls = nullptr, *ll_no = nullptr, *ll_dla = nullptr, *ll_lls = nullptr;
  double *map_z = nullptr, *map_n = nullptr, *map_i = nullptr;
  double *lp_lls = nullptr, *lp_dla = nullptr;
  double *post = nullptr, *scal = nullptr;  // scal: lpost_no, lpost_lls, p_no, p_lls, p_dla [5][nq]; lpost_dla after
  double *summary = nullptr;                // [nq][GPDLA_SUMMARY_COLS_MULTI(md)]
  uint32_t *base = nullptr;
  int32_t *alive = nullptr;
  // what the result tables / the prior arrays were allocated for: a re-filled batch slot keeps them
  // while it does not grow (the tables are indexed per quasar, so spare rows behind nq are unused)
  int64_t cap_nq = 0, cap_S = 0, lp_cap_nq = 0;
  int cap_md = 0, lp_cap_md = 0;
  int64_t prof_quasars = 0, prof_stride = 0;  // sub-batching of the context's profile table for this batch
  bool processed = false;
  void free_tables() {
    for (void **p : {(void **)&sll_dla, (void **)&sll_lls, (void **)&ll_no, (void **)&ll_dla, (void **)&ll_lls,
                     (void **)&map_z, (void **)&map_n, (void **)&map_i, (void **)&post, (void **)&scal,
                     (void **)&summary, (void **)&base, (void **)&alive}) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
    }
    cap_nq = cap_S = 0;
    cap_md = 0;
  }
  ~MultiBuffers() {
    free_tables();
    if (lp_lls) (void)hipFree(lp_lls);
    if (lp_dla) (void)hipFree(lp_dla);
  }
};

namespace {

// The timed region of gpdla_context_last_sweep_ms (gpdla_context_set_timing): around the kernels of the
// context's most recent sweep, moments or mock-draw call on `st`.
int begin_timing(gpdla_context *c, hipStream_t st) {
  if (c->timing) HIP_TRY(hipEventRecord(c->ev0, st));
  return GPDLA_OK;
}

int end_timing(gpdla_context *c, hipStream_t st) {
  if (!c->timing) return GPDLA_OK;
  HIP_TRY(hipEventRecord(c->ev1, st));
  c->have_timing = true;
  return GPDLA_OK;
}

}  // namespace

extern "C" {

void gpdla_default_config(gpdla_config *cfg) {
  if (!cfg) return;
  const double kms = 1000.0 / 299792458.0;  // set_parameters.m:8, :11
  cfg->min_lambda = 911.75;                 // :33
  cfg->max_lambda = 1215.75;                // :34
  cfg->lya_wavelength = 1215.6701;          // :5
  cfg->lyman_limit = 911.7633;              // :7
  cfg->pixel_spacing = 1e-4;                // :60
  cfg->max_z_cut = 3000 * kms;              // :65
  cfg->min_z_cut = 3000 * kms;              // :69
  cfg->width = 3;                           // :59
  cfg->num_lines = 3;                       // :63
  cfg->max_dlas = 4;                        // process_qsos_multiple_dlas_meanflux.m:32
  cfg->num_forest_lines = 31;               // set_parameters_multi.m:75
  cfg->min_z_separation = 3000 * kms;       // multi :33
  cfg->prev_tau_0 = 0.0023;                 // multi :36
  cfg->prev_beta = 3.65;                    // multi :37
  cfg->rng_seed = 0x9E3779B97F4A7C15ull;
  cfg->first_quasar_index = 0;
  cfg->contraction_precision = 0;
  cfg->multi_profile_bytes = 0;
  cfg->record_pool_bytes = 0;
  cfg->pipeline_slots = 0;
  cfg->max_quasars_per_batch = 0;
}

/* ------------------------------ context ------------------------------ */

int gpdla_context_create(int device_id, gpdla_context **out) try {
  if (!out) return fail(GPDLA_ERR_INVALID_ARGUMENT, "ctx out pointer is null");
  *out = nullptr;
  int rc = select_device(device_id);
  if (rc) return rc;
  rc = ensure_line_table(device_id);
  if (rc) return rc;
  gpdla_context *c = new gpdla_context();
  c->device_id = device_id;
  hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    gpdla_context_destroy(c);
    return fail(GPDLA_ERR_HIP, "hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
  }
  c->stream = c->own_stream;
  gpdla_default_config(&c->cfg);
  *out = c;
  return GPDLA_OK;
} GPDLA_NO_THROW

void gpdla_context_destroy(gpdla_context *c) {
  if (!c) return;
  (void)hipSetDevice(c->device_id);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->up_stream) (void)hipStreamSynchronize(c->up_stream);
  if (c->down_stream) (void)hipStreamSynchronize(c->down_stream);
  {
    std::lock_guard<std::mutex> lock(c->mu);
    for (gpdla_batch *b : c->batches) b->ctx = nullptr;  // orphaned: they only free their memory now
    c->batches.clear();
  }
  dev_free(c->d_rest);
  dev_free(c->d_mu);
  dev_free(c->d_M);
  dev_free(c->d_log_omega);
  dev_free(c->d_offset);
  dev_free(c->d_nhi);
  dev_free(c->d_log_nhi);
  dev_free(c->d_lls_nhi);
  dev_free(c->d_perm);
  dev_free(c->d_log_nhi_derived);
  dev_free(c->d_ru);
  dev_free(c->d_rv);
  dev_free(c->d_rperm);
  dev_free(c->d_prof);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
  if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
  delete c;
}

int gpdla_context_set_stream(gpdla_context *c, void *hip_stream) try {
  if (!c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null context");
  hipStream_t next = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->own_stream;
  if (next != c->stream && c->d_prof) {
    // work queued on the old stream may still use the context's profile table, which the next
    // multi-DLA call (on the new stream) overwrites
    HIP_TRY(hipSetDevice(c->device_id));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  c->stream = next;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_context_set_config(gpdla_context *c, const gpdla_config *cfg) try {
  if (!c || !cfg) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null context/config");
  if (cfg->width != 3)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "width must be 3 (voigt.c:229 hard-codes the 7-tap profile)");
  if (cfg->num_lines < 1 || cfg->num_lines > kMaxLines)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_lines %d outside [1, 31]", cfg->num_lines);
  if (cfg->contraction_precision != 0 && cfg->contraction_precision != 1)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "contraction_precision must be 0 (fp64) or 1 (fp32 study)");
  c->cfg = *cfg;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_context_set_first_quasar_index(gpdla_context *c, int64_t first_quasar_index) try {
  if (!c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null context");
  c->cfg.first_quasar_index = first_quasar_index;  // (no upload path reads this field)
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_context_synchronize(gpdla_context *c) try {
  if (!c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null context");
  HIP_TRY(hipSetDevice(c->device_id));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->up_stream));
  HIP_TRY(hipStreamSynchronize(c->down_stream));
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_context_set_model(gpdla_context *c, const gpdla_model *m) try {
  if (!c || !m || !m->rest_wavelengths || !m->mu || !m->M || !m->log_omega)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null model field");
  if (m->num_rest_pixels < 2 || m->k < 1)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "model needs >= 2 grid points and k >= 1");
  if (m->k > GPDLA_MAX_K) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d > %d", m->k, GPDLA_MAX_K);
  HIP_TRY(hipSetDevice(c->device_id));
  HIP_TRY(hipStreamSynchronize(c->stream));
  dev_free(c->d_rest);
  dev_free(c->d_mu);
  dev_free(c->d_M);
  dev_free(c->d_log_omega);
  const size_t G = (size_t)m->num_rest_pixels;
  int rc;
  if ((rc = upload(&c->d_rest, m->rest_wavelengths, G, c->stream))) return rc;
  if ((rc = upload(&c->d_mu, m->mu, G, c->stream))) return rc;
  if ((rc = upload(&c->d_M, m->M, G * m->k, c->stream))) return rc;
  if ((rc = upload(&c->d_log_omega, m->log_omega, G, c->stream))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->model.G = m->num_rest_pixels;
  c->model.k = m->k;
  c->model.rest = c->d_rest;
  c->model.mu = c->d_mu;
  c->model.M = c->d_M;
  c->model.log_omega = c->d_log_omega;
  c->model.c_0 = std::exp(m->log_c_0);      // process_qsos.m:84-86
  c->model.tau_0 = std::exp(m->log_tau_0);
  c->model.beta = std::exp(m->log_beta);
  c->has_model = true;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_context_set_samples(gpdla_context *c, const gpdla_samples *s) try {
  if (!c || !s || !s->offset_samples || !s->nhi_samples || s->num_dla_samples < 1)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/empty samples");
  HIP_TRY(hipSetDevice(c->device_id));
  HIP_TRY(hipStreamSynchronize(c->stream));
  dev_free(c->d_offset);
  dev_free(c->d_nhi);
  dev_free(c->d_log_nhi);
  dev_free(c->d_lls_nhi);
  dev_free(c->d_perm);
  dev_free(c->d_log_nhi_derived);
  c->d_log_nhi = c->d_lls_nhi = c->d_log_nhi_derived = nullptr;
  const size_t S = (size_t)s->num_dla_samples;
  // visit samples in ascending z_DLA order: z = min + (max - min) * offset is monotone in offset
  // for every quasar, so one permutation serves the whole run
  std::vector<int32_t> perm(S);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) {
    return s->offset_samples[a] < s->offset_samples[b];
  });
  int rc;
  if ((rc = upload(&c->d_offset, s->offset_samples, S, c->stream))) return rc;
  if ((rc = upload(&c->d_nhi, s->nhi_samples, S, c->stream))) return rc;
  if (s->log_nhi_samples && (rc = upload(&c->d_log_nhi, s->log_nhi_samples, S, c->stream))) return rc;
  if (s->lls_nhi_samples && (rc = upload(&c->d_lls_nhi, s->lls_nhi_samples, S, c->stream))) return rc;
  if ((rc = upload(&c->d_perm, perm.data(), S, c->stream))) return rc;
  // (for the refine pass) the range of log N; without a log table, log10 of nhi_samples as the table
  std::vector<double> derived;
  const double *ln = s->log_nhi_samples;
  if (!ln) {
    derived.resize(S);
    for (size_t i = 0; i < S; ++i) derived[i] = std::log10(s->nhi_samples[i]);
    ln = derived.data();
    if ((rc = upload(&c->d_log_nhi_derived, ln, S, c->stream))) return rc;
  }
  c->log_nhi_lo = c->log_nhi_hi = ln[0];
  for (size_t i = 1; i < S; ++i) {
    c->log_nhi_lo = ln[i] < c->log_nhi_lo ? ln[i] : c->log_nhi_lo;
    c->log_nhi_hi = ln[i] > c->log_nhi_hi ? ln[i] : c->log_nhi_hi;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->S = (int64_t)S;
  c->has_samples = true;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_context_set_timing(gpdla_context *c, int enabled) try {
  if (!c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null context");
  HIP_TRY(hipSetDevice(c->device_id));
  if (enabled && !c->ev0) {
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
  }
  c->timing = enabled != 0;
  c->have_timing = false;
  return GPDLA_OK;
} GPDLA_NO_THROW

double gpdla_context_last_sweep_ms(gpdla_context *c) {
  if (!c || !c->have_timing) return -1.0;
  (void)hipSetDevice(c->device_id);
  if (hipEventSynchronize(c->ev1) != hipSuccess) return -1.0;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) return -1.0;
  return (double)ms;
}

/* ------------------------------ batch ------------------------------ */

void gpdla_batch_destroy(gpdla_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->device_id);
  if (b->ctx) {
    (void)hipStreamSynchronize(b->ctx->stream);
    (void)hipStreamSynchronize(b->ctx->up_stream);
    (void)hipStreamSynchronize(b->ctx->down_stream);
    std::lock_guard<std::mutex> lock(b->ctx->mu);
    auto &v = b->ctx->batches;
    v.erase(std::remove(v.begin(), v.end(), b), v.end());
  } else {
    (void)hipDeviceSynchronize();  // the context (and its streams) went first
  }
  if (b->ev_done) (void)hipEventDestroy(b->ev_done);
  dev_free(b->arena);
  dev_free(b->d_records);
  delete b->mb;
  delete b->rf;
  delete b->fx;
  delete b;
}

}  // extern "C"

namespace {

int validate_spectra(gpdla_context *c, const gpdla_spectra *sp, int *md_out) {
  if (!c->has_model || !c->has_samples)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "set the model and the samples before uploading spectra");
  if (sp->num_quasars < 1 || !sp->offsets || !sp->wavelengths || !sp->flux || !sp->noise_variance ||
      !sp->pixel_mask || !sp->z_qsos || !sp->log_priors_no_dla || !sp->log_priors_dla)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/empty spectra field");
  const int md = sp->log_priors_lls ? c->cfg.max_dlas : 0;
  if (sp->log_priors_lls && (md < 1 || md > 4))
    return fail(GPDLA_ERR_UNSUPPORTED, "max_dlas = %d outside [1, 4]", md);
  for (int64_t q = 0; q < sp->num_quasars; ++q)
    if (sp->offsets[q + 1] < sp->offsets[q])
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (quasar %lld)", (long long)q);
  *md_out = md;
  return GPDLA_OK;
}

// The device arrays of a batch in its arena: this order, each 256-byte aligned.  Returns the bytes
// they take; with a base address it also points the batch's arrays into the arena.
size_t batch_layout(gpdla_batch *b, char *base, size_t npx, size_t nqs, size_t rows, size_t lam, int md) {
  size_t at = 0;
  auto take = [&](auto *&p, size_t count) {
    using T = std::remove_reference_t<decltype(*p)>;
    if (base) p = reinterpret_cast<T *>(base + at);
    at += (std::max<size_t>(count * sizeof(T), 8) + 255) & ~(size_t)255;
  };
  take(b->d_offsets, nqs + 1);
  take(b->d_wl, npx);
  take(b->d_flux, npx);
  take(b->d_nv, npx);
  take(b->d_mask, npx);
  take(b->d_z, nqs);
  take(b->d_lp_no, nqs);
  take(b->d_lp_dla, md ? 1 : nqs);  // (a multi-DLA batch keeps its priors and results in MultiBuffers)
  take(b->d_meta, nqs);
  take(b->d_order, nqs);
  take(b->d_rec_off, nqs);
  take(b->d_pix, rows);
  take(b->d_Mi, rows * b->k);
  take(b->d_lam, lam);
  take(b->d_sample_ll, md ? 1 : nqs * b->S);
  take(b->d_ll_no, md ? 1 : nqs);
  take(b->d_summary, md ? 1 : nqs * GPDLA_SUMMARY_COLS);
  return at;
}

// Fill batch b (new or being reloaded) from host spectra: H2D on the context's upload stream, which
// is drained before returning (the caller's buffers and the host vectors here are consumed).
int batch_fill(gpdla_context *c, gpdla_batch *b, const gpdla_spectra *sp, int md) {
  const int64_t nq = sp->num_quasars;
  b->nq = nq;
  b->S = c->S;
  b->k = c->model.k;
  // k <= 20: 13 w-tiles + 1 u-tile (+ 2 + 4 columns on the VALU); k <= 40: 52 + 4 tiles
  b->tiles_w = b->k <= 20 ? 13 : 52;
  b->ntiles = b->k <= 20 ? kCompactTiles : 56;
  const int64_t base = sp->offsets[0];
  b->total_pix = sp->offsets[nq] - base;
  b->max_pix = 0;
  std::vector<int64_t> off(nq + 1);
  std::vector<QuasarMeta> meta(nq);
  int64_t rows = 0, lam = 0;
  for (int64_t q = 0; q <= nq; ++q) off[q] = sp->offsets[q] - base;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t npix = off[q + 1] - off[q];
    std::memset(&meta[q], 0, sizeof(QuasarMeta));
    meta[q].status = 1;
    meta[q].pix_off = rows;
    meta[q].lam_off = lam;
    rows += 4 * ((npix + 3) / 4) + 4;
    lam += ((npix + 6 + 1) / 2) * 2 + 2;
    b->max_pix = std::max(b->max_pix, npix);
  }
  b->pool_rows = rows;
  b->h_recs.resize((size_t)nq);
  for (int64_t q = 0; q < nq; ++q) b->h_recs[q] = (off[q + 1] - off[q] + 3) / 4 + 1;
  b->plan_budget = -1;  // the record plan is remade by the next process call
  b->processed = false;
  if (b->rf) b->rf->levels = 0;  // (the tables are kept; their contents belong to the previous spectra)
  if (b->fx) b->fx->on = false;  // fixed absorbers belong to the previous spectra as well
  if (b->md != md) {  // (reload with a different kind of batch)
    delete b->mb;
    b->mb = nullptr;
  }
  b->md = md;
  hipStream_t st = c->up_stream;
  StreamDrain drain{st};  // on every exit: nothing still reads off / meta / order / the caller's arrays
  int rc = GPDLA_OK;
  auto chk = [&](int r) { if (r && !rc) rc = r; };
  std::vector<int32_t> order((size_t)nq);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
    return off[x + 1] - off[x] > off[y + 1] - off[y];
  });
  b->h_order = order;
  // lay the arrays out in the arena, growing it when this fill needs more
  const size_t npx = (size_t)b->total_pix, nqs = (size_t)nq;
  const size_t need = batch_layout(b, nullptr, npx, nqs, (size_t)rows, (size_t)lam, md);
  if (!b->arena || b->cap.arena < need) {
    dev_free(b->arena);
    b->arena = nullptr;
    b->cap.arena = 0;
    void *p = nullptr;
    const double t_malloc = wall_ms();
    if (hipMalloc(&p, need) != hipSuccess) return fail(GPDLA_ERR_HIP, "hipMalloc of %zu bytes for a batch failed", need);
    if (kOneShotTiming)
      std::fprintf(stderr, "[batch] arena of %.1f MB: hipMalloc %.2f ms\n", (double)need / 1e6, wall_ms() - t_malloc);
    b->arena = p;
    b->cap.arena = need;
  }
  batch_layout(b, static_cast<char *>(b->arena), npx, nqs, (size_t)rows, (size_t)lam, md);
  auto put = [&](void *dst, const void *src, size_t bytes) -> int {
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
    return GPDLA_OK;
  };
  chk(put(b->d_offsets, off.data(), (nqs + 1) * 8));
  chk(put(b->d_wl, sp->wavelengths + base, npx * 8));
  chk(put(b->d_flux, sp->flux + base, npx * 8));
  chk(put(b->d_nv, sp->noise_variance + base, npx * 8));
  chk(put(b->d_mask, sp->pixel_mask + base, npx));
  chk(put(b->d_z, sp->z_qsos, nqs * 8));
  chk(put(b->d_lp_no, sp->log_priors_no_dla, nqs * 8));
  if (!md) {
    chk(put(b->d_lp_dla, sp->log_priors_dla, nqs * 8));
  } else {  // multi-DLA batch: [nq][max_dlas] DLA priors + the sub-DLA prior (multi :204-210)
    if (!b->mb) b->mb = new MultiBuffers();
    MultiBuffers &mb = *b->mb;
    mb.processed = false;  // (the result tables are kept: gpdla_batch_process_multi regrows them if needed)
    if (mb.lp_cap_nq < nq || mb.lp_cap_md != md) {
      dev_free(mb.lp_dla);
      dev_free(mb.lp_lls);
      mb.lp_dla = mb.lp_lls = nullptr;
      mb.lp_cap_nq = 0;
      chk(dev_alloc(&mb.lp_dla, nqs * md));
      chk(dev_alloc(&mb.lp_lls, nqs));
      if (!rc) {
        mb.lp_cap_nq = nq;
        mb.lp_cap_md = md;
      }
    }
    if (!rc) {
      chk(put(mb.lp_dla, sp->log_priors_dla, nqs * md * 8));
      chk(put(mb.lp_lls, sp->log_priors_lls, nqs * 8));
    }
  }
  chk(put(b->d_meta, meta.data(), nqs * sizeof(QuasarMeta)));
  chk(put(b->d_order, order.data(), nqs * 4));
  if (rc) return rc;
  if (hipStreamSynchronize(st) != hipSuccess) return fail(GPDLA_ERR_HIP, "upload synchronize failed");
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_batch_upload(gpdla_context *c, const gpdla_spectra *sp, gpdla_batch **out) try {
  if (!c || !sp || !out) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  int md = 0;
  int rc = validate_spectra(c, sp, &md);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device_id));
  gpdla_batch *b = new gpdla_batch();
  b->ctx = c;
  b->device_id = c->device_id;
  {
    std::lock_guard<std::mutex> lock(c->mu);
    c->batches.push_back(b);
  }
  if (hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming) != hipSuccess) {
    gpdla_batch_destroy(b);
    return fail(GPDLA_ERR_HIP, "hipEventCreateWithFlags failed");
  }
  if ((rc = batch_fill(c, b, sp, md))) {
    gpdla_batch_destroy(b);
    return rc;
  }
  *out = b;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_reload(gpdla_context *c, gpdla_batch *b, const gpdla_spectra *sp) try {
  if (!c || !b || !sp || b->ctx != c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched context or batch");
  int md = 0;
  int rc = validate_spectra(c, sp, &md);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device_id));
  // the batch's previous sweep (if any) must have finished reading what is overwritten here; its
  // download is the caller's to have completed (gpdla.h)
  HIP_TRY(hipEventSynchronize(b->ev_done));
  HIP_TRY(hipStreamSynchronize(c->down_stream));
  return batch_fill(c, b, sp, md);  // on failure the batch stays valid to destroy, not to process
} GPDLA_NO_THROW

}  // extern "C"
