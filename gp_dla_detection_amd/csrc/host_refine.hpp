// host_refine.hpp -- the refine pass of a processed single-DLA batch (the contract is in
// include/gpdla.h): the argument checks, the refine points of a context, gpdla_batch_refine over
// k_refine_boxes, the boxed sweeps and k_refine_finish (refine_kernels.hpp), the download of its results,
// the summaries of the refined tables through k_parameter_summaries, and the model posteriors of the
// refined evidence (k_refined_posteriors).
#pragma once

static_assert(GPDLA_REFINE_MAX_LEVELS == gpdla::kRefineMaxLevels, "gpdla.h and sweep_primitives.hpp disagree");

namespace {

// device time of the calling thread's most recent gpdla_batch_refine with the context's timing on
// (gpdla_debug_last_refine_ms; tools/bench_refine.py)
thread_local double t_refine_ms = -1.0;

int validate_refine_request(const gpdla_refine_request *rq, const gpdla_nhi_prior *prior) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null refine request");
  if (rq->levels < 1 || rq->levels > GPDLA_REFINE_MAX_LEVELS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "levels = %d outside [1, %d]", rq->levels, GPDLA_REFINE_MAX_LEVELS);
  if (!(rq->delta > 0.0) || !std::isfinite(rq->delta)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "delta = %g must be finite and > 0", rq->delta);
  if (!(rq->pad >= 0.0) || !std::isfinite(rq->pad)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "pad = %g must be finite and >= 0", rq->pad);
  return prior ? check_prior(prior) : GPDLA_OK;
}

int validate_refine_points(int64_t n, const double *u, const double *v) {
  if (n < 1 || n > (1LL << 30)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_points = %lld outside [1, 2^30]", (long long)n);
  if (!u || !v) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null u / v");
  for (int64_t j = 0; j < n; ++j) {
    if (!(u[j] >= 0.0 && u[j] < 1.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "u[%lld] = %g is not inside [0, 1)", (long long)j, u[j]);
    if (!(v[j] >= 0.0 && v[j] < 1.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "v[%lld] = %g is not inside [0, 1)", (long long)j, v[j]);
  }
  return GPDLA_OK;
}

// The tables of RefineBuffers in one allocation, each 256-byte aligned (batch_layout's scheme)
size_t refine_layout(RefineBuffers *rf, char *base, size_t nq, size_t Sr) {
  size_t at = 0;
  auto take = [&](auto *&p, size_t count) {
    using T = std::remove_reference_t<decltype(*p)>;
    if (base) p = reinterpret_cast<T *>(base + at);
    at += (std::max<size_t>(count * sizeof(T), 8) + 255) & ~(size_t)255;
  };
  take(rf->box, nq * kRefineBoxStride);
  take(rf->rmeta, nq);
  take(rf->ell, nq * Sr);
  take(rf->lam, nq * Sr);
  take(rf->ll_scratch, nq);
  take(rf->terms, nq * kRefineTerms * 2);
  take(rf->scal, nq * kRefineScalars);
  take(rf->status, nq);
  take(rf->rows, nq);
  return at;
}

int refine_reserve(gpdla_batch *b, int64_t Sr) {
  if (!b->rf) b->rf = new RefineBuffers();
  RefineBuffers *rf = b->rf;
  if (!rf->ev_rows) HIP_TRY(hipEventCreateWithFlags(&rf->ev_rows, hipEventDisableTiming));
  const size_t need = refine_layout(rf, nullptr, (size_t)b->nq, (size_t)Sr);
  if (!rf->arena || rf->cap_bytes < need) {
    dev_free(rf->arena);
    rf->arena = nullptr;
    rf->cap_bytes = 0;
    void *p = nullptr;
    if (hipMalloc(&p, need) != hipSuccess) return fail(GPDLA_ERR_HIP, "hipMalloc of %zu bytes for the refine tables failed", need);
    rf->arena = p;
    rf->cap_bytes = need;
  }
  refine_layout(rf, static_cast<char *>(rf->arena), (size_t)b->nq, (size_t)Sr);
  rf->nq = b->nq;
  rf->Sr = Sr;
  return GPDLA_OK;
}

// The boxed sweep of `count` quasars (rows) at one level; the launch shapes of launch_sweep
int launch_boxed_sweep(gpdla_context *c, gpdla_batch *, RecordClass cls, int64_t count, const BoxedSweepArgs &args) {
  const bool three = args.num_lines == 3;
  if (cls == kRecSlim20)
    return launch_sweep_kernel(c, three ? &k_sweep_slim_boxed<3> : &k_sweep_slim_boxed<0>, kSlimWaves * 64,
                               (size_t)kSlimLdsDoubles * sizeof(double), kSlimWaves * kSamplesPerWave, count, args);
  const size_t lds = std::max(sweep_split_slim_lds_doubles(false), kExpTab + kSplitEpilogueDoubles) * sizeof(double);
  if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "split sweep needs %zu B of LDS", lds);
  return launch_sweep_kernel(c, three ? &k_sweep_split_slim<3, 0, BoxedSweepArgs> : &k_sweep_split_slim<0, 0, BoxedSweepArgs>, 512, lds,
                             2 * kSamplesPerWave, count, args);
}

// what the refined entry points ask of a batch
int check_refinable(gpdla_context *c, gpdla_batch *b) {
  int rc = check_batch_pair(c, b);
  if (rc) return rc;
  if (b->md) return fail(GPDLA_ERR_UNSUPPORTED, "the refine pass serves single-DLA batches only");
  if (c->cfg.contraction_precision == 1) return fail(GPDLA_ERR_UNSUPPORTED, "the refine pass is fp64 only (contraction_precision = 1)");
  if (b->k > 40) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d: the refine pass serves k <= 40", b->k);
  return GPDLA_OK;
}

// The refined source of the per-pixel products (host_grid.hpp): the checks of the refined summaries
// -- the batch has been refined, on the context's present refine points -- then the resident tables, every quasar's
// LAST box and the refine status of every quasar, downloaded once.
int refined_table(gpdla_context *c, gpdla_batch *b, RefinedTable *out) {
  int rc = check_refinable(c, b);
  if (rc) return rc;
  RefineBuffers *rf = b->rf;
  if (!rf || rf->levels < 1 || rf->nq != b->nq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the batch has not been refined");
  if (rf->Sr != c->Sr || rf->points_gen != c->refine_points_gen)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the refine points changed after the batch was refined");
  HIP_TRY(hipSetDevice(c->device_id));
  out->Sr = rf->Sr;
  out->lam = rf->lam;
  out->rmeta = rf->rmeta;
  out->box = rf->box + 4 * (rf->levels - 1);
  out->d_status = rf->status;
  out->status.resize((size_t)b->nq);
  hipStream_t st = c->stream;
  StreamDrain drain{st};
  HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
  HIP_TRY(hipMemcpyAsync(out->status.data(), rf->status, (size_t)b->nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_refine_validate(const gpdla_refine_request *request, const gpdla_nhi_prior *prior, int64_t num_points,
                          const double *u, const double *v) try {
  int rc = validate_refine_request(request, prior);
  if (rc) return rc;
  return (num_points || u || v) ? validate_refine_points(num_points, u, v) : GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_context_set_refine_points(gpdla_context *c, int64_t num_points, const double *u, const double *v) try {
  if (!c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null context");
  int rc = validate_refine_points(num_points, u, v);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device_id));
  HIP_TRY(hipStreamSynchronize(c->stream));
  dev_free(c->d_ru);
  dev_free(c->d_rv);
  dev_free(c->d_rperm);
  c->d_ru = c->d_rv = nullptr;
  c->d_rperm = nullptr;
  c->Sr = 0;
  const size_t n = (size_t)num_points;
  std::vector<int32_t> perm(n);  // ascending u: z' is monotone in u for every box
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int32_t x, int32_t y) { return u[x] < u[y]; });
  if ((rc = upload(&c->d_ru, u, n, c->stream)) || (rc = upload(&c->d_rv, v, n, c->stream)) ||
      (rc = upload(&c->d_rperm, perm.data(), n, c->stream)))
    return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->h_ru.assign(u, u + n);
  c->h_rv.assign(v, v + n);
  c->Sr = num_points;
  ++c->refine_points_gen;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_refine(gpdla_context *c, gpdla_batch *b, const int64_t *selection, int64_t num_selected,
                       const gpdla_refine_request *request, const gpdla_nhi_prior *prior) try {
  int rc = check_refinable(c, b);
  if (rc) return rc;
  if ((rc = validate_refine_request(request, prior))) return rc;
  if ((rc = check_selection(b->nq, selection, num_selected))) return rc;
  if ((rc = check_processed(b)) || (rc = check_unchanged(c, b, true))) return rc;
  if (c->Sr < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "no refine points: call gpdla_context_set_refine_points");
  if (!(c->log_nhi_lo < c->log_nhi_hi) || !std::isfinite(c->log_nhi_lo) || !std::isfinite(c->log_nhi_hi))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the log N table spans [%g, %g]: the refine pass needs a finite range of positive width",
                c->log_nhi_lo, c->log_nhi_hi);
  const RecordClass cls = legacy_record_class(b->k, b->k <= 20 ? kRecSlim20 : kRecSlim40);
  if (cls == kRecExpanded) return fail(GPDLA_ERR_UNSUPPORTED, "the refine pass sweeps slim records only");
  // the record plan the first pass made (offsets in the batch's meta, groups): it must still hold
  const int64_t per_step = record_class_doubles(cls, b->ntiles, false);
  const int64_t budget_bytes = c->cfg.record_pool_bytes > 0 ? c->cfg.record_pool_bytes : (int64_t)16 << 30;
  if (b->plan_per_step != per_step || b->plan_budget != std::max<int64_t>(1, budget_bytes / (per_step * 8)))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "record_pool_bytes changed since the batch was processed: process it again");
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  const int64_t nq = b->nq, Sr = c->Sr;
  const int L = request->levels;
  if ((rc = refine_reserve(b, Sr))) return rc;
  RefineBuffers *rf = b->rf;

  // the selected quasars, once each, in dealing order, group by group
  std::vector<uint8_t> chosen((size_t)nq, 0);
  for (int64_t s = 0; s < num_selected; ++s) chosen[(size_t)(selection ? selection[s] : s)] = 1;
  HIP_TRY(hipEventSynchronize(rf->ev_rows));  // the previous call's copy out of h_rows has run
  rf->h_rows.clear();
  std::vector<std::pair<int64_t, int64_t>> spans;  // [r0, r1) of h_rows per record group
  for (const auto &g : b->groups) {
    const int64_t r0 = (int64_t)rf->h_rows.size();
    for (int64_t i = g.first; i < g.second; ++i)
      if (chosen[(size_t)b->h_order[(size_t)i]]) rf->h_rows.push_back(b->h_order[(size_t)i]);
    spans.emplace_back(r0, (int64_t)rf->h_rows.size());
  }
  HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
  if (!rf->h_rows.empty())
    HIP_TRY(hipMemcpyAsync(rf->rows, rf->h_rows.data(), rf->h_rows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipEventRecord(rf->ev_rows, st));
  // NaN everywhere; status: not refined (the kernels overwrite the selected rows)
  HIP_TRY(hipMemsetAsync(rf->box, 0xFF, (size_t)nq * kRefineBoxStride * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(rf->ell, 0xFF, (size_t)nq * Sr * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(rf->lam, 0xFF, (size_t)nq * Sr * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(rf->scal, 0xFF, (size_t)nq * kRefineScalars * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(rf->terms, 0, (size_t)nq * kRefineTerms * 2 * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(rf->status, 0xFF, (size_t)nq * sizeof(int32_t), st));  // -1: GPDLA_REFINE_NOT_REFINED
  rf->levels = L;
  rf->points_gen = c->refine_points_gen;

  RefineBoxArgs ba{};
  ba.meta = b->d_meta;
  ba.N_lo = c->log_nhi_lo;
  ba.N_hi = c->log_nhi_hi;
  ba.delta = request->delta;
  ba.pad = request->pad;
  ba.box = rf->box;
  ba.rmeta = rf->rmeta;
  ba.terms = rf->terms;
  ba.status = rf->status;

  BoxedSweepArgs sa{};
  sa.meta = rf->rmeta;
  sa.records = b->d_records;
  sa.lam_pad = b->d_lam;
  sa.offset_samples = c->d_ru;
  sa.nhi_samples = c->d_rv;
  sa.perm = c->d_rperm;
  sa.pix = b->d_pix;
  sa.S = Sr;
  sa.k = b->k;
  sa.tiles_w = b->tiles_w;
  sa.ntiles = b->ntiles;
  sa.num_lines = c->cfg.num_lines;
  sa.sample_ll = rf->ell;
  sa.ll_no_dla = rf->ll_scratch;
  sa.blocks_per_quasar = 0;  // set by launch_sweep_kernel

  RefineFinishArgs fa{};
  fa.S = Sr;
  fa.u = c->d_ru;
  fa.v = c->d_rv;
  fa.meta = b->d_meta;
  fa.box = rf->box;
  fa.ell = rf->ell;
  fa.lam = rf->lam;
  fa.has_prior = prior ? 1 : 0;
  if (prior) fa.prior = prior_dev(*prior);
  fa.log_uniform = -std::log(c->log_nhi_hi - c->log_nhi_lo);
  fa.terms = rf->terms;
  fa.lp_dla = b->d_lp_dla;
  fa.scal = rf->scal;
  fa.status = rf->status;

  // (the timed region spans every group and level, as gpdla_context_last_sweep_ms does for the first pass)
  EventPair ev;
  if (c->timing) {
    if ((rc = ev.create())) return rc;
    HIP_TRY(hipEventRecord(ev.e0, st));
  }
  for (size_t g = 0; g < b->groups.size(); ++g) {
    const int64_t r0 = spans[g].first, count = spans[g].second - spans[g].first;
    if (count == 0) continue;
    if ((rc = launch_build_records(c, b, b->groups[g].first, b->groups[g].second, false, cls))) return rc;
    for (int l = 0; l < L; ++l) {
      ba.rows = rf->rows + r0;
      ba.level = l;
      ba.S = l ? Sr : b->S;
      ba.sqrt_S = std::sqrt((double)ba.S);
      ba.src = l ? rf->lam : b->d_sample_ll;
      ba.su = l ? c->d_ru : c->d_offset;
      ba.sv = l ? c->d_rv : (c->d_log_nhi ? c->d_log_nhi : c->d_log_nhi_derived);
      hipLaunchKernelGGL(k_refine_boxes, dim3((unsigned)count), dim3(256), 0, st, ba);
      HIP_TRY(hipGetLastError());
      sa.order = rf->rows + r0;
      sa.nq = count;
      sa.box = rf->box + 4 * l;
      if ((rc = launch_boxed_sweep(c, b, cls, count, sa))) return rc;
      if (is_conditioned(b) &&
          (rc = launch_condition_mask(c, b, rf->rows + r0, count, rf->status, rf->box + 4 * l, c->d_ru, Sr, rf->ell)))
        return rc;
      fa.rows = rf->rows + r0;
      fa.level = l;
      fa.last = l + 1 == L;
      hipLaunchKernelGGL(k_refine_finish, dim3((unsigned)count), dim3(256), 0, st, fa);
      HIP_TRY(hipGetLastError());
    }
  }
  // behind the refine pass too: a reload or a download of the batch waits for it
  HIP_TRY(hipEventRecord(b->ev_done, st));
  if (c->timing) {
    HIP_TRY(hipEventRecord(ev.e1, st));
    HIP_TRY(hipEventSynchronize(ev.e1));
    float ms = -1.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    t_refine_ms = (double)ms;
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_download_refined(gpdla_context *c, gpdla_batch *b, const int64_t *selection, int64_t num_selected,
                                 gpdla_refined_results *r) try {
  int rc = check_refinable(c, b);
  if (rc) return rc;
  if (!r) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null results");
  if ((rc = check_selection(b->nq, selection, num_selected))) return rc;
  RefineBuffers *rf = b->rf;
  if (!rf || rf->levels < 1 || rf->nq != b->nq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the batch has not been refined");
  // the caller states what its arrays were sized for: a mismatch would write past them
  if (r->levels != rf->levels)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "results->levels = %d, but the batch was refined with %d levels", (int)r->levels, (int)rf->levels);
  if (r->num_points != rf->Sr)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "results->num_points = %lld, but the batch was refined on %lld points", (long long)r->num_points,
                (long long)rf->Sr);
  if (num_selected == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(c->device_id));
  const size_t nq = (size_t)b->nq, Sr = (size_t)rf->Sr, L = (size_t)rf->levels;
  std::vector<double> box(nq * kRefineBoxStride), scal(nq * kRefineScalars);
  std::vector<int32_t> status(nq);
  hipStream_t ds = c->down_stream;
  StreamDrain drain{ds};
  HIP_TRY(hipStreamWaitEvent(ds, b->ev_done, 0));
  HIP_TRY(hipMemcpyAsync(box.data(), rf->box, box.size() * sizeof(double), hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipMemcpyAsync(scal.data(), rf->scal, scal.size() * sizeof(double), hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipMemcpyAsync(status.data(), rf->status, nq * sizeof(int32_t), hipMemcpyDeviceToHost, ds));
  // the two tables: the selected rows only, straight into the caller's arrays
  for (int64_t s = 0; s < num_selected; ++s) {
    const size_t q = (size_t)(selection ? selection[s] : s);
    if (r->sample_log_likelihoods_refined)
      HIP_TRY(hipMemcpyAsync(r->sample_log_likelihoods_refined + (size_t)s * Sr, rf->ell + q * Sr, Sr * sizeof(double), hipMemcpyDeviceToHost, ds));
    if (r->sample_log_posteriors_refined)
      HIP_TRY(hipMemcpyAsync(r->sample_log_posteriors_refined + (size_t)s * Sr, rf->lam + q * Sr, Sr * sizeof(double), hipMemcpyDeviceToHost, ds));
  }
  HIP_TRY(hipStreamSynchronize(ds));
  double *const scalars[kRefineScalars] = {r->log_likelihoods_dla_refined, r->log_posteriors_dla_refined, r->MAP_z_dlas_refined,
                                           r->MAP_log_nhis_refined, r->MAP_inds_refined};
  for (int64_t s = 0; s < num_selected; ++s) {
    const size_t q = (size_t)(selection ? selection[s] : s);
    if (r->boxes) std::memcpy(r->boxes + (size_t)s * L * 4, box.data() + q * kRefineBoxStride, L * 4 * sizeof(double));
    for (int f = 0; f < kRefineScalars; ++f)
      if (scalars[f]) scalars[f][s] = scal[q * kRefineScalars + f];
    if (r->status) r->status[s] = status[q];
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_refined_summaries(gpdla_context *c, gpdla_batch *b, const int64_t *selection, int64_t num_selected,
                                  const gpdla_summary_request *request, gpdla_parameter_summaries *outputs) try {
  int rc = check_refinable(c, b);
  if (rc) return rc;
  if (!outputs) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null outputs");
  if ((rc = validate_summary_request(request))) return rc;
  if (request->num_models != 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_models = %d: the refined table holds one model", request->num_models);
  if ((rc = check_selection(b->nq, selection, num_selected))) return rc;
  RefineBuffers *rf = b->rf;
  if (!rf || rf->levels < 1 || rf->nq != b->nq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the batch has not been refined");
  if (rf->Sr != c->Sr || rf->points_gen != c->refine_points_gen)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the refine points changed after the batch was refined");
  const int64_t nsel = num_selected, Sr = rf->Sr;
  if (nsel == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  std::vector<double> box((size_t)b->nq * kRefineBoxStride);
  {
    StreamDrain drain{st};
    HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
    HIP_TRY(hipMemcpyAsync(box.data(), rf->box, box.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // the last level's box is the row's range of z and the affine reading of v
  std::vector<double> z_lo((size_t)nsel), z_hi((size_t)nsel), n_lo((size_t)nsel), n_hi((size_t)nsel);
  std::vector<int64_t> row_start((size_t)nsel), none;
  for (int64_t s = 0; s < nsel; ++s) {
    const int64_t q = selection ? selection[s] : s;
    const double *bx = box.data() + (size_t)q * kRefineBoxStride + 4 * (rf->levels - 1);
    z_lo[(size_t)s] = bx[0];
    z_hi[(size_t)s] = bx[1];
    n_lo[(size_t)s] = bx[2];
    n_hi[(size_t)s] = bx[3];
    row_start[(size_t)s] = q * Sr;
  }
  return run_parameter_summaries(nsel, Sr, rf->lam, row_start, nullptr, none, z_lo.data(), z_hi.data(), c->h_ru.data(),
                                 c->h_rv.data(), *request, *outputs, st, n_lo.data(), n_hi.data());
} GPDLA_NO_THROW

int gpdla_batch_refined_posteriors(gpdla_context *c, gpdla_batch *b, const int64_t *selection, int64_t num_selected,
                                   gpdla_refined_posteriors *out) try {
  int rc = check_refinable(c, b);
  if (rc) return rc;
  if (!out) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null outputs");
  if ((rc = check_selection(b->nq, selection, num_selected))) return rc;
  RefineBuffers *rf = b->rf;
  if (!rf || rf->levels < 1 || rf->nq != b->nq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the batch has not been refined");
  const int64_t n = num_selected;
  if (n == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(c->device_id));
  std::vector<int64_t> sel((size_t)n);
  for (int64_t s = 0; s < n; ++s) sel[(size_t)s] = selection ? selection[s] : s;
  std::vector<double> post((size_t)n * 4);
  Staging up(c->stream);  // (after the host buffers of its copies)
  HIP_TRY(hipStreamWaitEvent(c->stream, b->ev_done, 0));
  RefinedPosteriorArgs a{};
  int64_t *d_sel;
  if ((rc = up.put(&d_sel, sel.data(), (size_t)n)) || (rc = up.tmp.alloc(&a.post, (size_t)n * 4)) ||
      (rc = up.tmp.alloc(&a.refined, (size_t)n)))
    return rc;
  a.n = n;
  a.sel = d_sel;
  a.summary = b->d_summary;
  a.scal = rf->scal;
  a.status = rf->status;
  hipLaunchKernelGGL(k_refined_posteriors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, a);
  HIP_TRY(hipGetLastError());
  if ((rc = up.fetch(post.data(), a.post, post.size())) || (rc = up.fetch(out->refined, a.refined, (size_t)n))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int64_t s = 0; s < n; ++s) {
    const double *p = post.data() + 4 * s;
    if (out->model_posteriors_refined) std::memcpy(out->model_posteriors_refined + 2 * s, p, 2 * sizeof(double));
    if (out->p_no_dlas_refined) out->p_no_dlas_refined[s] = p[2];
    if (out->p_dlas_refined) out->p_dlas_refined[s] = p[3];
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

double gpdla_debug_last_refine_ms(void) { return t_refine_ms; }

int gpdla_debug_slim_sweep_blocks_per_cu(int kernel, int *blocks_out) try {
  if (!blocks_out || kernel < 0 || kernel > 3)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "gpdla_debug_slim_sweep_blocks_per_cu: kernel %d", kernel);
  const void *const f[4] = {reinterpret_cast<const void *>(&k_sweep_slim<3>), reinterpret_cast<const void *>(&k_sweep_slim<0>),
                            reinterpret_cast<const void *>(&k_sweep_slim_boxed<3>),
                            reinterpret_cast<const void *>(&k_sweep_slim_boxed<0>)};
  const size_t lds = (size_t)kSlimLdsDoubles * sizeof(double);
  HIP_TRY(hipFuncSetAttribute(f[kernel], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_out, f[kernel], kSlimWaves * 64, lds));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
