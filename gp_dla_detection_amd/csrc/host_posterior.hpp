// host_posterior.hpp -- credible intervals and moments of the absorber parameters:
// the argument checks, the ranks of the samples, and the two entry points over k_parameter_summaries
// (posterior_kernels.hpp) -- host tables, and the resident tables of a processed batch.
#pragma once

static_assert(GPDLA_POSTERIOR_MAX_MODELS == gpdla::kPostMaxModels &&
                  GPDLA_POSTERIOR_MAX_PROBABILITIES == gpdla::kPostMaxProbabilities &&
                  GPDLA_POSTERIOR_MAX_THRESHOLDS == gpdla::kPostMaxThresholds,
              "gpdla.h and posterior_kernels.hpp disagree");

namespace {

// duration of the most recent k_parameter_summaries launch of this thread, from device events
// (gpdla_debug_last_summaries_ms; tools/bench_posteriors.py)
thread_local double t_summaries_ms = -1.0;

int validate_summary_request(const gpdla_summary_request *rq) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  if (rq->num_models < 1 || rq->num_models > GPDLA_POSTERIOR_MAX_MODELS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_models = %d outside [1, %d]", rq->num_models, GPDLA_POSTERIOR_MAX_MODELS);
  if (rq->num_probabilities < 0 || rq->num_probabilities > GPDLA_POSTERIOR_MAX_PROBABILITIES)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_probabilities = %d outside [0, %d]", rq->num_probabilities,
                GPDLA_POSTERIOR_MAX_PROBABILITIES);
  for (int q = 0; q < rq->num_probabilities; ++q) {
    const double p = rq->probabilities[q];
    if (!(p > 0.0 && p < 1.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "probabilities[%d] = %g is not inside (0, 1)", q, p);
    if (q > 0 && !(p > rq->probabilities[q - 1]))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "probabilities must increase strictly (entry %d)", q);
  }
  if (rq->num_thresholds < 0 || rq->num_thresholds > GPDLA_POSTERIOR_MAX_THRESHOLDS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_thresholds = %d outside [0, %d]", rq->num_thresholds,
                GPDLA_POSTERIOR_MAX_THRESHOLDS);
  for (int t = 0; t < rq->num_thresholds; ++t)
    if (std::isnan(rq->thresholds[t])) return fail(GPDLA_ERR_INVALID_ARGUMENT, "thresholds[%d] is NaN", t);
  return GPDLA_OK;
}

// rank[i]: position of sample i in the stable ascending order of v (ties by index); inv[rank] = i
int stable_ranks(const double *v, int64_t S, const char *name, std::vector<int32_t> &rank, std::vector<int32_t> &inv) {
  for (int64_t i = 0; i < S; ++i)
    if (!std::isfinite(v[i])) return fail(GPDLA_ERR_INVALID_ARGUMENT, "%s[%lld] is not finite", name, (long long)i);
  inv.resize((size_t)S);
  rank.resize((size_t)S);
  std::iota(inv.begin(), inv.end(), 0);
  std::stable_sort(inv.begin(), inv.end(), [v](int32_t x, int32_t y) { return v[x] < v[y]; });
  for (int64_t r = 0; r < S; ++r) rank[(size_t)inv[(size_t)r]] = (int32_t)r;
  return GPDLA_OK;
}

// The kernel over n rows of a device table.  row_start / base_start: element offsets of each row's
// first model / first base row; offsets, lnhi, z_min, z_max: host arrays.  n_lo / n_hi (host, [n], optional): the
// per-row affine reading of lnhi (PosteriorArgs::n_lo).
int run_parameter_summaries(int64_t n, int64_t S, const double *d_sll, const std::vector<int64_t> &row_start,
                            const uint32_t *d_base, const std::vector<int64_t> &base_start, const double *z_min,
                            const double *z_max, const double *offsets, const double *lnhi,
                            const gpdla_summary_request &rq, const gpdla_parameter_summaries &out, hipStream_t st,
                            const double *n_lo = nullptr, const double *n_hi = nullptr) {
  const int md = rq.num_models, Q = rq.num_probabilities, nt = rq.num_thresholds;
  if (n * md > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 (row, model) pairs in one call");
  std::vector<int32_t> rank_off, inv_off, rank_n, inv_n;
  int rc;
  if ((rc = stable_ranks(offsets, S, "offset_samples", rank_off, inv_off))) return rc;
  if ((rc = stable_ranks(lnhi, S, "log_nhi_samples", rank_n, inv_n))) return rc;
  const size_t cells = (size_t)n * md * md, models = (size_t)n * md;
  // one device block of doubles: the five moment fields, the two quantile fields, exceedance, ESS
  const size_t n_dbl = 5 * cells + 2 * cells * (size_t)Q + cells * (size_t)nt + models;
  std::vector<double> h_out(n_dbl);
  std::vector<int32_t> h_status(models);
  Staging sg(st);
  double *d_out = nullptr, *d_vec = nullptr, *d_smp = nullptr;
  int32_t *d_status = nullptr, *d_rank = nullptr;
  int64_t *d_start = nullptr;
  if ((rc = sg.tmp.alloc(&d_out, n_dbl)) || (rc = sg.tmp.alloc(&d_status, models)) || (rc = sg.tmp.alloc(&d_vec, (size_t)4 * n)) ||
      (rc = sg.tmp.alloc(&d_smp, (size_t)2 * S)) || (rc = sg.tmp.alloc(&d_rank, (size_t)4 * S)) ||
      (rc = sg.tmp.alloc(&d_start, (size_t)2 * n)))
    return rc;
  auto put = [&](auto *dst, const auto *src, size_t count) -> int {  // into a carved block: no allocation
    if (count) HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(*dst), hipMemcpyHostToDevice, st));
    return GPDLA_OK;
  };
  if ((rc = put(d_vec, z_min, (size_t)n)) || (rc = put(d_vec + n, z_max, (size_t)n)) || (rc = put(d_smp, offsets, (size_t)S)) ||
      (rc = put(d_smp + S, lnhi, (size_t)S)) || (rc = put(d_rank, rank_off.data(), (size_t)S)) ||
      (rc = put(d_rank + S, rank_n.data(), (size_t)S)) || (rc = put(d_rank + 2 * S, inv_off.data(), (size_t)S)) ||
      (rc = put(d_rank + 3 * S, inv_n.data(), (size_t)S)) || (rc = put(d_start, row_start.data(), (size_t)n)))
    return rc;
  if (md > 1 && (rc = put(d_start + n, base_start.data(), (size_t)n))) return rc;
  if (n_lo && ((rc = put(d_vec + 2 * n, n_lo, (size_t)n)) || (rc = put(d_vec + 3 * n, n_hi, (size_t)n)))) return rc;
  HIP_TRY(hipMemsetAsync(d_out, 0xFF, n_dbl * sizeof(double), st));  // NaN: slot > model, unusable models
  HIP_TRY(hipMemsetAsync(d_status, 0, models * sizeof(int32_t), st));
  PosteriorArgs a{};
  a.S = S;
  a.md = md;
  a.Q = Q;
  a.nt = nt;
  for (int q = 0; q < Q; ++q) a.prob[q] = rq.probabilities[q];
  for (int t = 0; t < nt; ++t) a.thresh[t] = rq.thresholds[t];
  a.sll = d_sll;
  a.row_start = d_start;
  a.base = md > 1 ? d_base : nullptr;
  a.base_start = md > 1 ? d_start + n : nullptr;
  a.z_min = d_vec;
  a.z_max = d_vec + n;
  a.n_lo = n_lo ? d_vec + 2 * n : nullptr;
  a.n_hi = n_lo ? d_vec + 3 * n : nullptr;
  a.offsets = d_smp;
  a.lnhi = d_smp + S;
  a.rank_off = d_rank;
  a.rank_n = d_rank + S;
  a.inv_off = d_rank + 2 * S;
  a.inv_n = d_rank + 3 * S;
  double *p = d_out;
  auto carve = [&](size_t count) { double *q = p; p += count; return q; };
  a.mean_z = carve(cells);
  a.std_z = carve(cells);
  a.mean_n = carve(cells);
  a.std_n = carve(cells);
  a.cov = carve(cells);
  a.quant_z = carve(cells * Q);
  a.quant_n = carve(cells * Q);
  a.exceed = carve(cells * nt);
  a.ess = carve(models);
  a.status = d_status;
  EventPair ev;
  if ((rc = ev.create())) return rc;
  HIP_TRY(hipEventRecord(ev.e0, st));
  hipLaunchKernelGGL(k_parameter_summaries, dim3((unsigned)(n * md)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ev.e1, st));
  if ((rc = sg.fetch(h_out.data(), d_out, n_dbl)) || (rc = sg.fetch(h_status.data(), d_status, models))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  float ms = -1.f;
  HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  t_summaries_ms = (double)ms;
  const double *h = h_out.data();
  auto give = [&](double *dst, size_t count) {
    if (dst && count) std::memcpy(dst, h, count * sizeof(double));
    h += count;
  };
  give(out.mean_z, cells);
  give(out.std_z, cells);
  give(out.mean_log_nhi, cells);
  give(out.std_log_nhi, cells);
  give(out.cov, cells);
  give(out.quantiles_z, cells * Q);
  give(out.quantiles_log_nhi, cells * Q);
  give(out.exceedance, cells * nt);
  give(out.effective_samples, models);
  if (out.status) std::memcpy(out.status, h_status.data(), models * sizeof(int32_t));
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_stats_parameter_summaries(int64_t num_rows, int64_t num_samples, const double *sample_log_likelihoods,
                                    int64_t row_stride, const uint32_t *base_sample_inds, const double *min_z_dlas,
                                    const double *max_z_dlas, const double *offset_samples, const double *log_nhi_samples,
                                    const gpdla_summary_request *request, gpdla_parameter_summaries *outputs,
                                    int device_id) try {
  using namespace gpdla;
  int rc = validate_summary_request(request);
  if (rc) return rc;
  const int64_t n = num_rows, S = num_samples, md = request->num_models;
  if (n < 0 || S < 1 || S > (1LL << 30)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "need num_rows >= 0 and 1 <= num_samples <= 2^30");
  if (row_stride < md * S) return fail(GPDLA_ERR_INVALID_ARGUMENT, "row_stride = %lld below num_models * num_samples", (long long)row_stride);
  if (!outputs) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null outputs");
  if (!offset_samples || !log_nhi_samples) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null offset_samples / log_nhi_samples");
  if ((md > 1) != (base_sample_inds != nullptr))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "base_sample_inds must be given exactly when num_models > 1 (num_models = %d)", (int)md);
  if (n > 0 && (!sample_log_likelihoods || !min_z_dlas || !max_z_dlas))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null sample_log_likelihoods / min_z_dlas / max_z_dlas");
  const size_t nbase = (size_t)n * (size_t)(md - 1) * (size_t)S;
  for (size_t i = 0; i < nbase; ++i)
    if ((int64_t)base_sample_inds[i] > S)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "base_sample_inds entry %zu = %u exceeds num_samples", i, base_sample_inds[i]);
  if (n == 0) return GPDLA_OK;
  if ((rc = select_device(device_id))) return rc;
  std::vector<double> rows;
  const double *src = sample_log_likelihoods;
  if (row_stride != md * S) {  // pack the rows: the device copy is [n][md][S]
    rows.resize((size_t)n * md * S);
    for (int64_t s = 0; s < n; ++s) std::memcpy(rows.data() + s * md * S, src + s * row_stride, (size_t)(md * S) * sizeof(double));
    src = rows.data();
  }
  std::vector<int64_t> row_start((size_t)n), base_start((size_t)n);
  for (int64_t s = 0; s < n; ++s) {
    row_start[(size_t)s] = s * md * S;
    base_start[(size_t)s] = s * (md - 1) * S;
  }
  DeviceTemps tmp;
  double *d_sll = nullptr;
  uint32_t *d_base = nullptr;
  if ((rc = tmp.alloc(&d_sll, (size_t)n * md * S)) || (rc = tmp.alloc(&d_base, nbase))) return rc;
  HIP_TRY(hipMemcpy(d_sll, src, (size_t)n * md * S * sizeof(double), hipMemcpyHostToDevice));
  if (nbase) HIP_TRY(hipMemcpy(d_base, base_sample_inds, nbase * sizeof(uint32_t), hipMemcpyHostToDevice));
  return run_parameter_summaries(n, S, d_sll, row_start, d_base, base_start, min_z_dlas, max_z_dlas, offset_samples,
                                 log_nhi_samples, *request, *outputs, nullptr);
} GPDLA_NO_THROW

int gpdla_batch_parameter_summaries(gpdla_context *c, gpdla_batch *b, int multi, int sub_dla, const int64_t *selection,
                                    int64_t num_selected, const gpdla_summary_request *request,
                                    gpdla_parameter_summaries *outputs) try {
  using namespace gpdla;
  int rc = check_batch_pair(c, b, outputs != nullptr);
  if (rc || (rc = validate_summary_request(request))) return rc;
  const int64_t nsel = num_selected, S = b->S;
  const int md = request->num_models;
  if ((rc = check_selection(b->nq, selection, nsel))) return rc;
  if ((multi != 0) != (b->md != 0))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, b->md ? "a multi-DLA batch: pass multi != 0" : "a single-DLA batch: pass multi = 0");
  if (sub_dla && !multi) return fail(GPDLA_ERR_INVALID_ARGUMENT, "sub_dla needs a multi-DLA batch");
  if (sub_dla ? md != 1 : (multi ? md > b->md : md != 1))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_models = %d does not fit the batch (sub_dla and single-DLA: 1; multi: up to %d)",
                md, (int)b->md);
  if ((rc = check_processed(b)) || (rc = check_unchanged(c, b, false))) return rc;
  if (!c->d_log_nhi || (sub_dla && !c->d_lls_nhi))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the context's samples lack log_nhi_samples / lls_nhi_samples");
  if (S > (1LL << 30)) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^30 samples");
  if (nsel == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  std::vector<QuasarMeta> meta((size_t)b->nq);
  std::vector<double> offsets((size_t)S), lnhi((size_t)S), z_min((size_t)nsel), z_max((size_t)nsel);
  std::vector<int64_t> row_start((size_t)nsel), base_start((size_t)nsel);
  {
    StreamDrain drain{st};
    HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
    HIP_TRY(hipMemcpyAsync(meta.data(), b->d_meta, (size_t)b->nq * sizeof(QuasarMeta), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(offsets.data(), c->d_offset, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lnhi.data(), sub_dla ? c->d_lls_nhi : c->d_log_nhi, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (sub_dla)
    for (auto &v : lnhi) v = std::log10(v);
  const SampleTable t = resident_samples(b, sub_dla != 0);
  for (int64_t s = 0; s < nsel; ++s) {
    const int64_t q = selection ? selection[s] : s;
    z_min[(size_t)s] = meta[(size_t)q].min_z_dla;
    z_max[(size_t)s] = meta[(size_t)q].max_z_dla;
    row_start[(size_t)s] = q * t.width;
    base_start[(size_t)s] = b->md ? q * (int64_t)(b->md - 1) * S : 0;
  }
  return run_parameter_summaries(nsel, S, t.table, row_start, b->md ? b->mb->base : nullptr, base_start, z_min.data(),
                                 z_max.data(), offsets.data(), lnhi.data(), *request, *outputs, st);
} GPDLA_NO_THROW

double gpdla_debug_last_summaries_ms(void) { return t_summaries_ms; }

}  // extern "C"
