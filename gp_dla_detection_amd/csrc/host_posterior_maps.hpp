// host_posterior_maps.hpp -- posterior maps of (z_DLA, log10 N_HI), their HPD regions and the absorber
// intensity: the argument checks, the launch groups, and the three entry points over
// k_posterior_maps / k_posterior_maps_mix (posterior_maps_kernels.hpp) -- host tables, the resident tables
// of a processed batch, and the last level of a refined one.
#pragma once

static_assert(GPDLA_MAPS_MAX_SIDE == gpdla::kMapMaxSide && GPDLA_MAPS_MAX_LEVELS == gpdla::kMapMaxLevels &&
                  GPDLA_MAPS_UNUSABLE == gpdla::kMapUnusable && GPDLA_MAPS_BAD_GRID == gpdla::kMapBadGrid &&
                  GPDLA_MAPS_SHORT == gpdla::kMapShort && GPDLA_MAPS_BAD_WEIGHTS == gpdla::kMapBadWeights,
              "gpdla.h and posterior_maps_kernels.hpp disagree");

namespace {

// the maps of the rows of one launch group stay within this much device memory (the model spectra's budget)
constexpr int64_t kMapsScratchBytes = 256LL << 20;

// device time of the two kernels, summed over the launch groups, and the number of groups of this thread's
// most recent successful call (gpdla_debug_last_maps_ms / _launches; tools/bench_posterior_maps.py)
thread_local double t_maps_ms[2] = {-1.0, -1.0};
thread_local int64_t t_maps_launches = 0;

int64_t maps_rows_per_launch(int md, int nz, int nn) {
  const int64_t per_row = (int64_t)md * md * nz * nn * (int64_t)sizeof(double);
  return std::max<int64_t>(1, kMapsScratchBytes / per_row);
}

int validate_maps_request(const gpdla_posterior_maps_request *rq) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  if (rq->num_models < 1 || rq->num_models > GPDLA_POSTERIOR_MAX_MODELS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_models = %d outside [1, %d]", rq->num_models, GPDLA_POSTERIOR_MAX_MODELS);
  if (rq->nz < 1 || rq->nz > GPDLA_MAPS_MAX_SIDE) return fail(GPDLA_ERR_INVALID_ARGUMENT, "nz = %d outside [1, %d]", rq->nz, GPDLA_MAPS_MAX_SIDE);
  if (rq->nn < 1 || rq->nn > GPDLA_MAPS_MAX_SIDE) return fail(GPDLA_ERR_INVALID_ARGUMENT, "nn = %d outside [1, %d]", rq->nn, GPDLA_MAPS_MAX_SIDE);
  if (rq->num_levels < 0 || rq->num_levels > GPDLA_MAPS_MAX_LEVELS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_levels = %d outside [0, %d]", rq->num_levels, GPDLA_MAPS_MAX_LEVELS);
  for (int q = 0; q < rq->num_levels; ++q) {
    const double p = rq->levels[q];
    if (!(p > 0.0 && p < 1.0)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "levels[%d] = %g is not inside (0, 1)", q, p);
    if (q > 0 && !(p > rq->levels[q - 1])) return fail(GPDLA_ERR_INVALID_ARGUMENT, "levels must increase strictly (entry %d)", q);
  }
  return GPDLA_OK;
}

int check_finite_samples(const double *v, int64_t S, const char *name) {
  for (int64_t i = 0; i < S; ++i)
    if (!std::isfinite(v[i])) return fail(GPDLA_ERR_INVALID_ARGUMENT, "%s[%lld] is not finite", name, (long long)i);
  return GPDLA_OK;
}

// The kernels over n rows of a device table, in groups of at most maps_rows_per_launch rows.  row_start /
// base_start as run_parameter_summaries takes them; grid [n][4] and weights [n][md] (null: no mix) are host
// arrays; n_lo / n_hi: the per-row affine reading of lnhi.
int run_posterior_maps(int64_t n, int64_t S, const double *d_sll, const std::vector<int64_t> &row_start, const uint32_t *d_base,
                       const std::vector<int64_t> &base_start, const double *z_min, const double *z_max, const double *offsets,
                       const double *lnhi, const std::vector<double> &grid, const double *weights,
                       const gpdla_posterior_maps_request &rq, const gpdla_posterior_maps &out, hipStream_t st,
                       const double *n_lo = nullptr, const double *n_hi = nullptr) {
  const int md = rq.num_models, L = rq.num_levels;
  const int64_t cells = (int64_t)rq.nz * rq.nn, slots = (int64_t)md * md;
  const int64_t G = std::min<int64_t>(n, maps_rows_per_launch(md, rq.nz, rq.nn));
  if (G * slots > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "more than 2^31 - 1 (row, model, slot) blocks in one launch");
  const bool mix = weights != nullptr;
  std::vector<int32_t> h_slot((size_t)(G * slots)), h_row((size_t)G);
  int rc;
  Staging sg(st);
  double *d_vec = nullptr, *d_smp = nullptr, *d_grid = nullptr, *d_w = nullptr, *d_mass = nullptr, *d_level = nullptr, *d_dbl = nullptr;
  int32_t *d_int = nullptr;
  int64_t *d_start = nullptr;
  // one block of doubles per group: outside, thresholds, intensity, expected; one of ints: mode, cells, the two statuses
  const size_t n_dbl = (size_t)(G * slots * (1 + L) + G * cells + G), n_int = (size_t)(G * slots * (2 + L) + G);
  if ((rc = sg.tmp.alloc(&d_vec, (size_t)4 * n)) || (rc = sg.tmp.alloc(&d_smp, (size_t)2 * S)) || (rc = sg.tmp.alloc(&d_start, (size_t)2 * n)) ||
      (rc = sg.put(&d_grid, grid.data(), (size_t)4 * n)) || (mix && (rc = sg.put(&d_w, weights, (size_t)n * md))) ||
      (rc = sg.tmp.alloc(&d_mass, (size_t)(G * slots * cells))) || (out.hpd_level && (rc = sg.tmp.alloc(&d_level, (size_t)(G * slots * cells)))) ||
      (rc = sg.tmp.alloc(&d_dbl, n_dbl)) || (rc = sg.tmp.alloc(&d_int, n_int)))
    return rc;
  auto put = [&](auto *dst, const auto *src, size_t count) -> int {
    if (count) HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(*dst), hipMemcpyHostToDevice, st));
    return GPDLA_OK;
  };
  if ((rc = put(d_vec, z_min, (size_t)n)) || (rc = put(d_vec + n, z_max, (size_t)n)) || (rc = put(d_smp, offsets, (size_t)S)) ||
      (rc = put(d_smp + S, lnhi, (size_t)S)) || (rc = put(d_start, row_start.data(), (size_t)n)))
    return rc;
  if (md > 1 && (rc = put(d_start + n, base_start.data(), (size_t)n))) return rc;
  if (n_lo && ((rc = put(d_vec + 2 * n, n_lo, (size_t)n)) || (rc = put(d_vec + 3 * n, n_hi, (size_t)n)))) return rc;
  EventPair ev_maps, ev_mix;
  if ((rc = ev_maps.create()) || (rc = ev_mix.create())) return rc;
  double ms_maps = 0.0, ms_mix = 0.0;
  int64_t launches = 0;
  for (int64_t r0 = 0; r0 < n; r0 += G, ++launches) {
    const int64_t g = std::min(G, n - r0);
    const size_t gs = (size_t)(g * slots);
    HIP_TRY(hipMemsetAsync(d_mass, 0xFF, gs * cells * sizeof(double), st));  // NaN: slot > model, unusable models
    if (d_level) HIP_TRY(hipMemsetAsync(d_level, 0xFF, gs * cells * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(d_dbl, 0xFF, n_dbl * sizeof(double), st));
    HIP_TRY(hipMemsetAsync(d_int, 0xFF, n_int * sizeof(int32_t), st));        // -1: mode and cells of such slots
    PosteriorMapsArgs a{};
    a.S = S;
    a.md = md;
    a.nz = rq.nz;
    a.nn = rq.nn;
    a.L = L;
    for (int q = 0; q < L; ++q) a.level[q] = rq.levels[q];
    a.sll = d_sll;
    a.row_start = d_start + r0;
    a.base = md > 1 ? d_base : nullptr;
    a.base_start = md > 1 ? d_start + n + r0 : nullptr;
    a.z_min = d_vec + r0;
    a.z_max = d_vec + n + r0;
    a.offsets = d_smp;
    a.lnhi = d_smp + S;
    a.n_lo = n_lo ? d_vec + 2 * n + r0 : nullptr;
    a.n_hi = n_lo ? d_vec + 3 * n + r0 : nullptr;
    a.grid = d_grid + 4 * r0;
    a.mass = d_mass;
    a.hpd_level = d_level;
    a.outside = d_dbl;
    a.hpd_threshold = d_dbl + gs;
    double *d_intensity = d_dbl + gs * (1 + L), *d_expected = d_intensity + g * cells;
    a.mode = d_int;
    a.hpd_cells = d_int + gs;
    a.slot_status = d_int + gs * (1 + L);
    int32_t *d_row_status = d_int + gs * (2 + L);
    HIP_TRY(hipMemsetAsync(a.slot_status, 0, gs * sizeof(int32_t), st));
    HIP_TRY(hipEventRecord(ev_maps.e0, st));
    hipLaunchKernelGGL(k_posterior_maps, dim3((unsigned)gs), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev_maps.e1, st));
    if (mix) {
      PosteriorMixArgs x{};
      x.md = md;
      x.cells = (int32_t)cells;
      x.mass = d_mass;
      x.slot_status = a.slot_status;
      x.weights = d_w + r0 * md;
      x.intensity = d_intensity;
      x.expected = d_expected;
      x.row_status = d_row_status;
      HIP_TRY(hipEventRecord(ev_mix.e0, st));
      hipLaunchKernelGGL(k_posterior_maps_mix, dim3((unsigned)g), dim3(256), 0, st, x);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ev_mix.e1, st));
    }
    // the group's rows are contiguous in every output: straight into the caller's arrays
    if ((rc = sg.fetch(out.mass ? out.mass + r0 * slots * cells : nullptr, d_mass, gs * cells)) ||
        (rc = sg.fetch(out.hpd_level ? out.hpd_level + r0 * slots * cells : nullptr, d_level, gs * cells)) ||
        (rc = sg.fetch(out.outside ? out.outside + r0 * slots : nullptr, a.outside, gs)) ||
        (rc = sg.fetch(out.hpd_threshold ? out.hpd_threshold + r0 * slots * L : nullptr, a.hpd_threshold, gs * L)) ||
        (rc = sg.fetch(out.mode ? out.mode + r0 * slots : nullptr, a.mode, gs)) ||
        (rc = sg.fetch(out.hpd_cells ? out.hpd_cells + r0 * slots * L : nullptr, a.hpd_cells, gs * L)) ||
        (rc = sg.fetch(h_slot.data(), a.slot_status, gs)))
      return rc;
    if (mix && ((rc = sg.fetch(out.intensity ? out.intensity + r0 * cells : nullptr, d_intensity, (size_t)(g * cells))) ||
                (rc = sg.fetch(out.expected_absorbers ? out.expected_absorbers + r0 : nullptr, d_expected, (size_t)g)) ||
                (rc = sg.fetch(h_row.data(), d_row_status, (size_t)g))))
      return rc;
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev_maps.e0, ev_maps.e1));
    ms_maps += ms;
    if (mix) {
      HIP_TRY(hipEventElapsedTime(&ms, ev_mix.e0, ev_mix.e1));
      ms_mix += ms;
    }
    if (out.status)
      for (int64_t r = 0; r < g; ++r)
        for (int m = 0; m < md; ++m) {
          int32_t s = mix ? h_row[(size_t)r] : 0;
          for (int j = 0; j <= m; ++j) s |= h_slot[(size_t)(r * slots + m * md + j)];
          out.status[(r0 + r) * md + m] = s;
        }
  }
  t_maps_ms[0] = ms_maps;
  t_maps_ms[1] = mix ? ms_mix : -1.0;
  t_maps_launches = launches;
  return GPDLA_OK;
}

// what the three entries ask of their outputs: the mix's arrays need weights
int check_maps_outputs(const gpdla_posterior_maps *out, bool have_weights) {
  if (!out) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null outputs");
  if (!have_weights && (out->intensity || out->expected_absorbers))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "intensity / expected_absorbers need model_weights");
  return GPDLA_OK;
}

// the four grid arrays come together or not at all
int check_grid_arrays(const double *a, const double *b, const double *c, const double *d, bool required) {
  const int given = (a != nullptr) + (b != nullptr) + (c != nullptr) + (d != nullptr);
  if (given != 0 && given != 4) return fail(GPDLA_ERR_INVALID_ARGUMENT, "grid_z_lo, grid_z_hi, grid_n_lo, grid_n_hi: all four or none");
  if (required && !given) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null grid_z_lo / grid_z_hi / grid_n_lo / grid_n_hi");
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int64_t gpdla_posterior_maps_rows_per_launch(int num_models, int nz, int nn) {
  if (num_models < 1 || num_models > GPDLA_POSTERIOR_MAX_MODELS || nz < 1 || nz > GPDLA_MAPS_MAX_SIDE || nn < 1 || nn > GPDLA_MAPS_MAX_SIDE)
    return 0;
  return maps_rows_per_launch(num_models, nz, nn);
}

int gpdla_stats_posterior_maps(int64_t num_rows, int64_t num_samples, const double *sample_log_likelihoods, int64_t row_stride,
                               const uint32_t *base_sample_inds, const double *min_z_dlas, const double *max_z_dlas,
                               const double *offset_samples, const double *log_nhi_samples, const double *grid_z_lo,
                               const double *grid_z_hi, const double *grid_n_lo, const double *grid_n_hi,
                               const double *model_weights, const gpdla_posterior_maps_request *request,
                               gpdla_posterior_maps *outputs, int device_id) try {
  using namespace gpdla;
  int rc = validate_maps_request(request);
  if (rc) return rc;
  const int64_t n = num_rows, S = num_samples, md = request->num_models;
  if (n < 0 || S < 1 || S > (1LL << 30)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "need num_rows >= 0 and 1 <= num_samples <= 2^30");
  if (row_stride < md * S) return fail(GPDLA_ERR_INVALID_ARGUMENT, "row_stride = %lld below num_models * num_samples", (long long)row_stride);
  if ((rc = check_maps_outputs(outputs, model_weights != nullptr))) return rc;
  if (!offset_samples || !log_nhi_samples) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null offset_samples / log_nhi_samples");
  if ((md > 1) != (base_sample_inds != nullptr))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "base_sample_inds must be given exactly when num_models > 1 (num_models = %d)", (int)md);
  if (n > 0 && (!sample_log_likelihoods || !min_z_dlas || !max_z_dlas))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null sample_log_likelihoods / min_z_dlas / max_z_dlas");
  if ((rc = check_grid_arrays(grid_z_lo, grid_z_hi, grid_n_lo, grid_n_hi, n > 0))) return rc;
  if ((rc = check_finite_samples(offset_samples, S, "offset_samples")) || (rc = check_finite_samples(log_nhi_samples, S, "log_nhi_samples")))
    return rc;
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
  std::vector<double> grid((size_t)4 * n);
  for (int64_t s = 0; s < n; ++s) {
    row_start[(size_t)s] = s * md * S;
    base_start[(size_t)s] = s * (md - 1) * S;
    const double g[4] = {grid_z_lo[s], grid_z_hi[s], grid_n_lo[s], grid_n_hi[s]};
    std::memcpy(grid.data() + 4 * s, g, sizeof g);
  }
  DeviceTemps tmp;
  double *d_sll = nullptr;
  uint32_t *d_base = nullptr;
  if ((rc = tmp.alloc(&d_sll, (size_t)n * md * S)) || (rc = tmp.alloc(&d_base, nbase))) return rc;
  HIP_TRY(hipMemcpy(d_sll, src, (size_t)n * md * S * sizeof(double), hipMemcpyHostToDevice));
  if (nbase) HIP_TRY(hipMemcpy(d_base, base_sample_inds, nbase * sizeof(uint32_t), hipMemcpyHostToDevice));
  return run_posterior_maps(n, S, d_sll, row_start, d_base, base_start, min_z_dlas, max_z_dlas, offset_samples, log_nhi_samples,
                            grid, model_weights, *request, *outputs, nullptr);
} GPDLA_NO_THROW

int gpdla_batch_posterior_maps(gpdla_context *c, gpdla_batch *b, int multi, int sub_dla, const int64_t *selection,
                               int64_t num_selected, const double *grid_z_lo, const double *grid_z_hi, const double *grid_n_lo,
                               const double *grid_n_hi, const double *model_weights, const gpdla_posterior_maps_request *request,
                               gpdla_posterior_maps *outputs) try {
  using namespace gpdla;
  int rc = validate_maps_request(request);  // (first: the request is checked whether or not a batch exists)
  if (rc || (rc = check_batch_pair(c, b, outputs != nullptr))) return rc;
  const int64_t nsel = num_selected, S = b->S;
  const int md = request->num_models;
  const bool mix = model_weights != nullptr || request->mix != 0;
  if ((rc = check_maps_outputs(outputs, mix)) || (rc = check_selection(b->nq, selection, nsel)) ||
      (rc = check_grid_arrays(grid_z_lo, grid_z_hi, grid_n_lo, grid_n_hi, false)))
    return rc;
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
  const size_t nq = (size_t)b->nq;
  const size_t wcols = b->md ? (sub_dla ? 1 : 2 + (size_t)b->md) : GPDLA_SUMMARY_COLS;  // the table the default weights come from
  std::vector<QuasarMeta> meta(nq);
  std::vector<double> offsets((size_t)S), lnhi((size_t)S), z_min((size_t)nsel), z_max((size_t)nsel), grid((size_t)4 * nsel), wtab, w;
  std::vector<int64_t> row_start((size_t)nsel), base_start((size_t)nsel);
  const bool own_weights = mix && !model_weights;
  if (own_weights) wtab.resize(nq * wcols);
  {
    StreamDrain drain{st};
    HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
    HIP_TRY(hipMemcpyAsync(meta.data(), b->d_meta, nq * sizeof(QuasarMeta), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(offsets.data(), c->d_offset, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lnhi.data(), sub_dla ? c->d_lls_nhi : c->d_log_nhi, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
    if (own_weights) {  // DLA(1..md) of the model posteriors; p_lls for the sub-DLA table; p_dla of a single-DLA batch
      const double *src = b->md ? (sub_dla ? b->mb->scal + 3 * nq : b->mb->post) : b->d_summary;
      HIP_TRY(hipMemcpyAsync(wtab.data(), src, wtab.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
  }
  if (sub_dla)
    for (auto &v : lnhi) v = std::log10(v);
  if ((rc = check_finite_samples(offsets.data(), S, "offset_samples")) || (rc = check_finite_samples(lnhi.data(), S, "log_nhi_samples")))
    return rc;
  const auto range = std::minmax_element(lnhi.begin(), lnhi.end());  // the default log N axis: the table in use
  const SampleTable t = resident_samples(b, sub_dla != 0);
  if (own_weights) w.resize((size_t)nsel * md);
  for (int64_t s = 0; s < nsel; ++s) {
    const int64_t q = selection ? selection[s] : s;
    z_min[(size_t)s] = meta[(size_t)q].min_z_dla;
    z_max[(size_t)s] = meta[(size_t)q].max_z_dla;
    row_start[(size_t)s] = q * t.width;
    base_start[(size_t)s] = b->md ? q * (int64_t)(b->md - 1) * S : 0;
    double *g = grid.data() + 4 * s;
    g[0] = grid_z_lo ? grid_z_lo[s] : z_min[(size_t)s];
    g[1] = grid_z_lo ? grid_z_hi[s] : z_max[(size_t)s];
    g[2] = grid_z_lo ? grid_n_lo[s] : *range.first;
    g[3] = grid_z_lo ? grid_n_hi[s] : *range.second;
    if (own_weights)
      for (int m = 0; m < md; ++m)
        w[(size_t)s * md + m] = b->md ? (sub_dla ? wtab[(size_t)q] : wtab[(size_t)q * wcols + 2 + m]) : wtab[(size_t)q * wcols + 11];
  }
  return run_posterior_maps(nsel, S, t.table, row_start, b->md ? b->mb->base : nullptr, base_start, z_min.data(), z_max.data(),
                            offsets.data(), lnhi.data(), grid, mix ? (own_weights ? w.data() : model_weights) : nullptr, *request,
                            *outputs, st);
} GPDLA_NO_THROW

int gpdla_batch_refined_posterior_maps(gpdla_context *c, gpdla_batch *b, const int64_t *selection, int64_t num_selected,
                                       const double *grid_z_lo, const double *grid_z_hi, const double *grid_n_lo,
                                       const double *grid_n_hi, const double *model_weights,
                                       const gpdla_posterior_maps_request *request, gpdla_posterior_maps *outputs) try {
  using namespace gpdla;
  int rc = validate_maps_request(request);
  if (rc || (rc = check_refinable(c, b))) return rc;
  if (request->num_models != 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_models = %d: the refined table holds one model", request->num_models);
  const bool mix = model_weights != nullptr || request->mix != 0;
  if ((rc = check_maps_outputs(outputs, mix)) || (rc = check_selection(b->nq, selection, num_selected)) ||
      (rc = check_grid_arrays(grid_z_lo, grid_z_hi, grid_n_lo, grid_n_hi, false)))
    return rc;
  RefineBuffers *rf = b->rf;
  if (!rf || rf->levels < 1 || rf->nq != b->nq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the batch has not been refined");
  if (rf->Sr != c->Sr || rf->points_gen != c->refine_points_gen)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the refine points changed after the batch was refined");
  const int64_t nsel = num_selected, Sr = rf->Sr;
  if (nsel == 0) return GPDLA_OK;
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  const size_t nq = (size_t)b->nq;
  const bool own_weights = mix && !model_weights;
  std::vector<double> box(nq * kRefineBoxStride), summary(own_weights ? nq * GPDLA_SUMMARY_COLS : 0);
  {
    StreamDrain drain{st};
    HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
    HIP_TRY(hipMemcpyAsync(box.data(), rf->box, box.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (own_weights) HIP_TRY(hipMemcpyAsync(summary.data(), b->d_summary, summary.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  // the last level's box is the row's range of z, the affine reading of v and the default grid
  std::vector<double> z_lo((size_t)nsel), z_hi((size_t)nsel), n_lo((size_t)nsel), n_hi((size_t)nsel), grid((size_t)4 * nsel), w;
  std::vector<int64_t> row_start((size_t)nsel), none;
  if (own_weights) w.resize((size_t)nsel);
  for (int64_t s = 0; s < nsel; ++s) {
    const int64_t q = selection ? selection[s] : s;
    const double *bx = box.data() + (size_t)q * kRefineBoxStride + 4 * (rf->levels - 1);
    z_lo[(size_t)s] = bx[0];
    z_hi[(size_t)s] = bx[1];
    n_lo[(size_t)s] = bx[2];
    n_hi[(size_t)s] = bx[3];
    row_start[(size_t)s] = q * Sr;
    double *g = grid.data() + 4 * s;
    g[0] = grid_z_lo ? grid_z_lo[s] : bx[0];
    g[1] = grid_z_lo ? grid_z_hi[s] : bx[1];
    g[2] = grid_z_lo ? grid_n_lo[s] : bx[2];
    g[3] = grid_z_lo ? grid_n_hi[s] : bx[3];
    if (own_weights) w[(size_t)s] = summary[(size_t)q * GPDLA_SUMMARY_COLS + 11];  // the first pass's p_dla
  }
  return run_posterior_maps(nsel, Sr, rf->lam, row_start, nullptr, none, z_lo.data(), z_hi.data(), c->h_ru.data(), c->h_rv.data(),
                            grid, mix ? (own_weights ? w.data() : model_weights) : nullptr, *request, *outputs, st, n_lo.data(),
                            n_hi.data());
} GPDLA_NO_THROW

double gpdla_debug_last_maps_ms(int kernel) { return (kernel == 0 || kernel == 1) ? t_maps_ms[kernel] : -1.0; }

int64_t gpdla_debug_last_maps_launches(void) { return t_maps_launches; }

}  // extern "C"
