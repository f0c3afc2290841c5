// host_sweep.hpp -- the single-DLA sweep of a resident batch (process_qsos.m:102-233): the one
// launcher of every sweep kernel, the record plan, k_prepare, the record builders,
// gpdla_batch_process, the download of its results, and the two stand-alone surfaces.
#pragma once

namespace {

// One launch of a sweep kernel on the context's stream: `samples_per_block` of the S + 1 passes of
// a quasar (S samples and the null model) per block, the quasars rounded up to a multiple of 8.
template <typename Args>
int launch_sweep_kernel(gpdla_context *c, void (*kernel)(Args), int threads, size_t lds, int samples_per_block,
                        int64_t num_quasars, Args args) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  args.blocks_per_quasar = (int32_t)((args.S + 1 + samples_per_block - 1) / samples_per_block);
  const int64_t nblocks = 8 * ((num_quasars + 7) / 8) * (int64_t)args.blocks_per_quasar;
  if (nblocks > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "batch too large for one launch");
  hipLaunchKernelGGL(kernel, dim3((unsigned)nblocks), dim3(threads), lds, c->stream, args);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// The kernels of the multi-DLA sweeps are compiled per number of DLAs: f(integral_constant<int, ND>)
// for the ND that `mode` stands for (0, the sub-DLA pass, multiplies one profile per sample like 1).
template <class F>
int dispatch_nd(int mode, F &&f) {
  switch (mode == 0 ? 1 : mode) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return fail(GPDLA_ERR_UNSUPPORTED, "max_dlas = %d > 4", mode);
  }
}

// LDS of the epilogue of the sweeps that split 56 tiles over four waves (two sample groups a block)
constexpr size_t kSplitEpilogueDoubles = (size_t)2 * EpilogueShape<52, 4>::SPP * EpilogueShape<52, 4>::stride(56);

// k_sweep: pre-expanded records (the fp32 study; in fp64 the legacy library only)
template <typename T, int WAVES, int NTW, int TS, int CH, int TW, int LINES>
int launch_sweep_expanded(gpdla_context *c, gpdla_batch *b, const SweepArgs &args) {
  constexpr int groups = WAVES / TS;
  const int L = args.num_lines;
  const size_t RD = (size_t)record_doubles(b->ntiles, sizeof(T) == 4);
  const size_t stage_doubles = 2 * (size_t)CH * RD;
  const size_t epi_doubles = (size_t)groups * EpilogueShape<TW, TS>::SPP * EpilogueShape<TW, TS>::stride(logical_tiles(b->ntiles));
  // the epilogue reuses the whole dynamic array (stage buffers, then rings etc.: all dead by then)
  const size_t loop_doubles = stage_doubles + (size_t)WAVES * kSamplesPerWave * kRing2 + kExpTab +
                              (size_t)groups * kSamplesPerWave * L;
  const size_t lds = std::max(loop_doubles, epi_doubles + kExpTab) * sizeof(double);  // (the epilogue rows start after the exp table)
  if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "sweep needs %zu B of LDS", lds);
  return launch_sweep_kernel(c, &k_sweep<T, WAVES, NTW, TS, CH, TW, LINES>, WAVES * 64, lds, groups * kSamplesPerWave, b->nq, args);
}

// Plan the record pool of a batch for records of `per_step` doubles: offsets per quasar, groups of
// quasars (in dealing order) whose records fit the pool budget, the pool itself.  Remade only when
// the record class, the budget or the batch's contents changed.
int plan_records(gpdla_context *c, gpdla_batch *b, int64_t per_step, bool single_group) {
  const int64_t budget_bytes = c->cfg.record_pool_bytes > 0 ? c->cfg.record_pool_bytes : (int64_t)16 << 30;
  const int64_t budget = single_group ? INT64_MAX : std::max<int64_t>(1, budget_bytes / (per_step * 8));
  if (b->plan_per_step != per_step || b->plan_budget != budget) {
    const int64_t nq = b->nq;
    // h_rec_off is the source of an asynchronous copy enqueued by the previous plan, in front of
    // that process call's kernels: it may be rewritten once they have run (a no-op after a reload,
    // which has waited for the same event)
    HIP_TRY(hipEventSynchronize(b->ev_done));
    b->h_rec_off.assign((size_t)nq, 0);
    b->groups.clear();
    int64_t cur = 0, g0 = 0, most = 0;
    for (int64_t i = 0; i < nq; ++i) {
      const int64_t q = b->h_order[(size_t)i], n = b->h_recs[(size_t)q];
      if (cur > 0 && cur + n > budget) {
        b->groups.emplace_back(g0, i);
        most = std::max(most, cur);
        g0 = i;
        cur = 0;
      }
      b->h_rec_off[(size_t)q] = cur;
      cur += n;
    }
    b->groups.emplace_back(g0, nq);
    most = std::max(most, cur);
    b->plan_pool_records = most + kRecordPoolPad;
    b->plan_per_step = per_step;
    b->plan_budget = budget;
    // (h_rec_off lives as long as the batch: the copy may complete after this call returns)
    HIP_TRY(hipMemcpyAsync(b->d_rec_off, b->h_rec_off.data(), (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  }
  return reserve(&b->d_records, &b->cap.records, (size_t)b->plan_pool_records * (size_t)per_step);
}

// k_prepare for a batch (multi: the mean-flux / Lyman-series variant)
int launch_prepare(gpdla_context *c, gpdla_batch *b, bool multi) {
  hipStream_t st = c->stream;
  Config cfg;
  cfg.min_lambda = c->cfg.min_lambda;
  cfg.max_lambda = c->cfg.max_lambda;
  cfg.lya_wavelength = c->cfg.lya_wavelength;
  cfg.lyman_limit = c->cfg.lyman_limit;
  cfg.pixel_spacing = c->cfg.pixel_spacing;
  cfg.max_z_cut = c->cfg.max_z_cut;
  cfg.min_z_cut = c->cfg.min_z_cut;
  cfg.num_lines = c->cfg.num_lines;
  PrepareArgs pa;
  pa.nq = b->nq;
  pa.offsets = b->d_offsets;
  pa.wavelengths = b->d_wl;
  pa.flux = b->d_flux;
  pa.noise_variance = b->d_nv;
  pa.pixel_mask = b->d_mask;
  pa.z_qsos = b->d_z;
  pa.model = c->model;
  pa.cfg = cfg;
  pa.meta = b->d_meta;
  pa.pix = b->d_pix;
  pa.Mi = b->d_Mi;
  pa.lam_pad = b->d_lam;
  pa.rec_off = b->d_rec_off;
  pa.multi = multi ? 1 : 0;
  pa.num_forest_lines = c->cfg.num_forest_lines;
  pa.prev_tau_0 = c->cfg.prev_tau_0;
  pa.prev_beta = c->cfg.prev_beta;
  hipLaunchKernelGGL(k_prepare, dim3((unsigned)b->nq), dim3(256), 0, st, pa);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// The K-step records of the quasars h_order[g0 .. g1) into the pool, in one of three classes:
// pre-expanded MFMA tiles (k_sweep and the legacy / diagnostic paths), the 896-byte records of the
// k <= 20 slim sweeps, the 1536-byte records of the k <= 40 slim sweeps.
enum RecordClass { kRecExpanded = 0, kRecSlim20 = 1, kRecSlim40 = 2 };
int64_t record_class_doubles(RecordClass rc, int ntiles, bool f32_tiles) {
  return rc == kRecSlim20 ? kSlimRec : rc == kRecSlim40 ? kS40Rec : record_doubles(ntiles, f32_tiles ? 1 : 0);
}
int launch_build_records(gpdla_context *c, gpdla_batch *b, int64_t g0, int64_t g1, bool f32_tiles, RecordClass cls) {
  const bool slim = cls != kRecExpanded;
  BuildRecordsArgs ba;
  ba.meta = b->d_meta;
  ba.pix = b->d_pix;
  ba.Mi = b->d_Mi;
  ba.lam_pad = b->d_lam;
  ba.records = b->d_records;
  ba.k = b->k;
  ba.tiles_w = b->tiles_w;
  ba.ntiles = b->ntiles;
  ba.blocks_per_quasar = slim ? 4 : 16;
  ba.f32_tiles = f32_tiles ? 1 : 0;
  ba.order = b->d_order + g0;
  const unsigned grid = (unsigned)((g1 - g0) * ba.blocks_per_quasar);
  if (cls == kRecSlim20)
    hipLaunchKernelGGL(k_build_slim_records, dim3(grid), dim3(256), 0, c->stream, ba);
  else if (cls == kRecSlim40)
    hipLaunchKernelGGL(k_build_slim40_records, dim3(grid), dim3(256), 0, c->stream, ba);
  else
    hipLaunchKernelGGL(k_build_records, dim3(grid), dim3(256), 0, c->stream, ba);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// What libgpdla_legacy.so adds to the sweeps (host_legacy.hpp; the product library's versions do nothing):
// the record class its environment switches ask for instead of `product`, and the fp64 sweeps on
// pre-expanded records (KMAX: rank class, 20 or 40).  The two that launch kernels are templates so that
// those kernels are instantiated where the call stands: the legacy code object keeps its kernel order.
RecordClass legacy_record_class(int k, RecordClass product);
template <int KMAX>
int legacy_sweep(gpdla_context *c, gpdla_batch *b, const SweepArgs &args);
template <class Args>
int legacy_sweep_multi(gpdla_context *c, gpdla_batch *b, const Args &args);

// A batch conditioned on fixed absorbers (host_condition.hpp): k_condition_rows behind
// k_prepare, and k_condition_mask on a swept table of S entries per quasar -- the first pass's (rows ==
// nullptr: every quasar of the batch, z over its search range) or a boxed level's (the `count` quasars of
// `rows`, z over box + q * kRefineBoxStride, the rows of refine status != 0 skipped).
bool is_conditioned(const gpdla_batch *b) { return b->fx && b->fx->on; }
int check_conditionable(const gpdla_context *c, const gpdla_batch *b);
int launch_condition_rows(gpdla_context *c, gpdla_batch *b);
int launch_condition_mask(gpdla_context *c, gpdla_batch *b, const int32_t *rows, int64_t count, const int32_t *status,
                          const double *box, const double *su, int64_t S, double *table);

// The sweep of one group of quasars (args.order, args.nq) over records of class `cls`; three
// lines at compile time, any other count at run time.  fp64 sweeps slim records, the fp32 study
// pre-expanded ones.  (The grids of all but k_sweep_split_slim cover the batch's quasars: the blocks
// behind the group's end at once.)
int launch_sweep(gpdla_context *c, gpdla_batch *b, RecordClass cls, bool f32, const SweepArgs &args) {
  const bool three = args.num_lines == 3;
  if (b->k <= 20) {
    if (cls == kRecSlim20)  // vech(m m') formed inside the sweep
      return launch_sweep_kernel(c, three ? &k_sweep_slim<3> : &k_sweep_slim<0>, kSlimWaves * 64,
                                 (size_t)kSlimLdsDoubles * sizeof(double), kSlimWaves * kSamplesPerWave, b->nq, args);
    if (!f32) return legacy_sweep<20>(c, b, args);
    // compact class: 13 w-tiles + 1 u-tile on the matrix cores, 2 + 4 columns on the VALU
    return three ? launch_sweep_expanded<float, 8, 14, 1, 8, 13, 3>(c, b, args) : launch_sweep_expanded<float, 8, 14, 1, 4, 13, 0>(c, b, args);
  }
  if (cls == kRecSlim40) {  // 52 w-tiles (<= 820 columns) + 3 u-tiles split over the 8 waves of a block
    const size_t lds = std::max(sweep_split_slim_lds_doubles(false), kExpTab + kSplitEpilogueDoubles) * sizeof(double);
    if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "split sweep needs %zu B of LDS", lds);
    return launch_sweep_kernel(c, three ? &k_sweep_split_slim<3, 0, SweepArgs> : &k_sweep_split_slim<0, 0, SweepArgs>, 512, lds,
                               2 * kSamplesPerWave, args.nq, args);
  }
  if (!f32) return legacy_sweep<40>(c, b, args);
  // 224 accumulator registers fit one wave (4-wave blocks, one wave per SIMD)
  return three ? launch_sweep_expanded<float, 4, 56, 1, 4, 52, 3>(c, b, args) : launch_sweep_expanded<float, 4, 56, 1, 4, 52, 0>(c, b, args);
}

}  // namespace

extern "C" {

int gpdla_batch_process(gpdla_context *c, gpdla_batch *b) try {
  if (!c || !b || b->ctx != c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched context or batch");
  if (b->S != c->S || b->k != c->model.k)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "model/samples changed after the batch was uploaded");
  if (b->md) return fail(GPDLA_ERR_INVALID_ARGUMENT, "multi-DLA batch: use gpdla_batch_process_multi");
  if (b->k > 40) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d needs %d B tiles (max 56)", b->k, b->ntiles);
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  // fp64 sweeps slim step records (k <= 20: k_sweep_slim; 20 < k <= 40: k_sweep_split_slim); the fp32
  // study (contraction_precision == 1) sweeps pre-expanded ones (k_sweep<float, ...>)
  const bool f32 = c->cfg.contraction_precision == 1;
  const RecordClass cls = legacy_record_class(b->k, f32 ? kRecExpanded : b->k <= 20 ? kRecSlim20 : kRecSlim40);
  const bool conditioned = is_conditioned(b);
  int rc = conditioned ? check_conditionable(c, b) : GPDLA_OK;  // (the configuration may have changed since the lists were set)
  if (rc || (rc = plan_records(c, b, record_class_doubles(cls, b->ntiles, false), false))) return rc;
  if ((rc = launch_prepare(c, b, conditioned && b->fx->meanflux))) return rc;
  if (conditioned && (rc = launch_condition_rows(c, b))) return rc;

  // NaN pre-fill, as process_qsos.m:74-82 does for quasars that are skipped
  HIP_TRY(hipMemsetAsync(b->d_sample_ll, 0xFF, (size_t)b->nq * b->S * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(b->d_ll_no, 0xFF, (size_t)b->nq * sizeof(double), st));

  SweepArgs sa;
  sa.meta = b->d_meta;
  sa.records = b->d_records;
  sa.lam_pad = b->d_lam;
  sa.offset_samples = c->d_offset;
  sa.nhi_samples = c->d_nhi;
  sa.perm = c->d_perm;
  sa.pix = b->d_pix;
  sa.S = b->S;
  sa.k = b->k;
  sa.tiles_w = b->tiles_w;
  sa.ntiles = b->ntiles;
  sa.num_lines = c->cfg.num_lines;
  sa.sample_ll = b->d_sample_ll;
  sa.ll_no_dla = b->d_ll_no;
  sa.blocks_per_quasar = 0;  // set by launch_sweep_kernel
  // the timed region of gpdla_context_last_sweep_ms spans the sweeps of all groups (one group unless
  // the records exceed cfg.record_pool_bytes)
  if ((rc = begin_timing(c, st))) return rc;
  for (const auto &g : b->groups) {
    if ((rc = launch_build_records(c, b, g.first, g.second, f32, cls))) return rc;
    sa.order = b->d_order + g.first;
    sa.nq = g.second - g.first;
    if ((rc = launch_sweep(c, b, cls, f32, sa))) return rc;
  }
  if ((rc = end_timing(c, st))) return rc;
  if (conditioned && (rc = launch_condition_mask(c, b, nullptr, b->nq, nullptr, nullptr, c->d_offset, b->S, b->d_sample_ll))) return rc;

  EvidenceArgs ea;
  ea.meta = b->d_meta;
  ea.sample_ll = b->d_sample_ll;
  ea.ll_no_dla = b->d_ll_no;
  ea.log_prior_no_dla = b->d_lp_no;
  ea.log_prior_dla = b->d_lp_dla;
  ea.offset_samples = c->d_offset;
  ea.nhi_samples = c->d_nhi;
  ea.log_nhi_samples = c->d_log_nhi;
  ea.S = b->S;
  ea.summary = b->d_summary;
  hipLaunchKernelGGL(k_evidence, dim3((unsigned)b->nq), dim3(256), 0, st, ea);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b->ev_done, st));
  b->processed = true;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_summary_device_ptr(gpdla_batch *b, double **table, int64_t *nq) try {
  if (!b || !table) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (b->md) return fail(GPDLA_ERR_INVALID_ARGUMENT, "multi-DLA batch: use gpdla_batch_summary_multi_device_ptr");
  *table = b->d_summary;
  if (nq) *nq = b->nq;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_samples_device_ptr(gpdla_batch *b, double **table, int64_t *nq, int64_t *S) try {
  if (!b || !table) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (b->md) return fail(GPDLA_ERR_INVALID_ARGUMENT, "multi-DLA batch: use gpdla_batch_samples_multi_device_ptr");
  *table = b->d_sample_ll;
  if (nq) *nq = b->nq;
  if (S) *S = b->S;
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"

namespace {

// gpdla_results: the arrays that are columns of a batch's summary table (member, doubles per quasar,
// first column); sample_log_likelihoods_dla and status are copied from tables of their own
struct ResultColumn {
  double *gpdla_results::*member;
  int width, col;
};
constexpr ResultColumn kResultColumns[] = {
    {&gpdla_results::min_z_dlas, 1, 0},           {&gpdla_results::max_z_dlas, 1, 1},
    {&gpdla_results::log_likelihoods_no_dla, 1, 4}, {&gpdla_results::log_likelihoods_dla, 1, 5},
    {&gpdla_results::log_posteriors_no_dla, 1, 6}, {&gpdla_results::log_posteriors_dla, 1, 7},
    {&gpdla_results::model_posteriors, 2, 8},     {&gpdla_results::p_no_dlas, 1, 10},
    {&gpdla_results::p_dlas, 1, 11},              {&gpdla_results::MAP_inds, 1, 12},
    {&gpdla_results::MAP_z_dlas, 1, 13},          {&gpdla_results::MAP_log_nhis, 1, 14}};

// The results of a batch into rows [row0, row0 + nq) of the caller's arrays (row0 > 0: a block of a
// one-shot call, host_pipeline.hpp)
int batch_download(gpdla_context *c, gpdla_batch *b, const gpdla_results &r, int64_t row0) {
  if (!c || !b || b->ctx != c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched argument");
  if (b->md) return fail(GPDLA_ERR_INVALID_ARGUMENT, "multi-DLA batch: use gpdla_batch_download_multi");
  HIP_TRY(hipSetDevice(c->device_id));
  const size_t nq = (size_t)b->nq;
  std::vector<double> summary(nq * GPDLA_SUMMARY_COLS);
  std::vector<QuasarMeta> meta(nq);
  // on the download stream, behind this batch's last kernel: a sweep of ANOTHER batch that is in
  // flight on the compute stream is not waited for
  hipStream_t ds = c->down_stream;
  StreamDrain drain{ds};
  HIP_TRY(hipStreamWaitEvent(ds, b->ev_done, 0));
  HIP_TRY(hipMemcpyAsync(summary.data(), b->d_summary, summary.size() * sizeof(double),
                         hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipMemcpyAsync(meta.data(), b->d_meta, nq * sizeof(QuasarMeta), hipMemcpyDeviceToHost, ds));
  if (r.sample_log_likelihoods_dla)
    HIP_TRY(hipMemcpyAsync(r.sample_log_likelihoods_dla + row0 * b->S, b->d_sample_ll, nq * b->S * sizeof(double),
                           hipMemcpyDeviceToHost, ds));
  HIP_TRY(hipStreamSynchronize(ds));
  for (const ResultColumn &f : kResultColumns)
    if (double *dst = r.*f.member)
      for (size_t q = 0; q < nq; ++q)
        for (int j = 0; j < f.width; ++j) dst[(row0 + q) * f.width + j] = summary[q * GPDLA_SUMMARY_COLS + f.col + j];
  if (r.status)
    for (size_t q = 0; q < nq; ++q) r.status[row0 + q] = meta[q].status;
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_batch_download(gpdla_context *c, gpdla_batch *b, gpdla_results *r) try {
  if (!r) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched argument");
  return batch_download(c, b, *r, 0);
} GPDLA_NO_THROW

/* ------------------------------ stand-alone surfaces ------------------------------ */

int gpdla_voigt(const double *lambdas, int64_t n_padded, double z, double N, int num_lines,
                double *profile_out, int device_id) try {
  if (!lambdas || !profile_out) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null pointer");
  if (n_padded <= 6) return fail(GPDLA_ERR_INVALID_ARGUMENT, "n_padded = %lld must exceed 2*width = 6", (long long)n_padded);
  if (num_lines < 1 || num_lines > kMaxLines)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_lines %d outside [1, 31]", num_lines);
  int rc = select_device(device_id);
  if (rc) return rc;
  if ((rc = ensure_line_table(device_id))) return rc;
  double *d_lam = nullptr, *d_raw = nullptr, *d_prof = nullptr;
  const int64_t n_out = n_padded - 6;
  auto cleanup = [&]() {
    dev_free(d_lam);
    dev_free(d_raw);
    dev_free(d_prof);
  };
  if ((rc = dev_alloc(&d_lam, (size_t)n_padded)) || (rc = dev_alloc(&d_raw, (size_t)n_padded)) ||
      (rc = dev_alloc(&d_prof, (size_t)n_out))) {
    cleanup();
    return rc;
  }
  hipError_t e = hipMemcpy(d_lam, lambdas, (size_t)n_padded * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_voigt_raw, dim3((unsigned)((n_padded + 255) / 256)), dim3(256), 0, 0, d_lam,
                       n_padded, z, N, num_lines, d_raw);
    hipLaunchKernelGGL(k_voigt_broaden, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, 0, d_raw,
                       n_out, d_prof);
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = hipMemcpy(profile_out, d_prof, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost);
  cleanup();
  if (e != hipSuccess) return fail(GPDLA_ERR_HIP, "gpdla_voigt: %s", hipGetErrorString(e));
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_log_mvnpdf_low_rank(const double *y, const double *mu, const double *M, const double *d,
                              int64_t n, int k, double *log_p, int device_id) try {
  if (!y || !mu || !M || !d || !log_p) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null pointer");
  if (n < 1 || k < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "n and k must be positive");
  if (k > 256) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d too large", k);
  int rc = select_device(device_id);
  if (rc) return rc;
  // one packed upload (y | mu | d | M), one packed download (log_p | status)
  double *buf = nullptr;
  const size_t nn = (size_t)n, ws = (size_t)k * (k + 1) / 2 + k + 2;
  const size_t n_in = 3 * nn + nn * k, total = n_in + ws + 2;
  if ((rc = dev_alloc(&buf, total))) return rc;
  std::vector<double> host(n_in);
  std::memcpy(host.data(), y, nn * sizeof(double));
  std::memcpy(host.data() + nn, mu, nn * sizeof(double));
  std::memcpy(host.data() + 2 * nn, d, nn * sizeof(double));
  std::memcpy(host.data() + 3 * nn, M, nn * k * sizeof(double));
  double *dy = buf, *dmu = dy + nn, *dd = dmu + nn, *dM = dd + nn, *dws = dM + nn * k, *dlp = dws + ws;
  int *d_status = reinterpret_cast<int *>(dlp + 1);
  hipError_t e = hipMemcpy(buf, host.data(), n_in * sizeof(double), hipMemcpyHostToDevice);
  double back[2] = {NAN, 0.0};
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_lowrank_single, dim3(1), dim3(256), 0, 0, dy, dmu, dM, dd, n, k, dws, dlp, d_status);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(back, dlp, 2 * sizeof(double), hipMemcpyDeviceToHost);
  dev_free(buf);
  if (e != hipSuccess) return fail(GPDLA_ERR_HIP, "gpdla_log_mvnpdf_low_rank: %s", hipGetErrorString(e));
  int status;
  std::memcpy(&status, &back[1], sizeof(int));
  *log_p = back[0];
  if (status) {
    *log_p = NAN;
    return fail(GPDLA_ERR_NOT_POSITIVE_DEFINITE, "B = I + M' D^-1 M is not positive definite");
  }
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"

// Test hook (gpdla.h): k_prepare alone, then the rows of one quasar.
extern "C" int gpdla_debug_prepared_rows(gpdla_context *c, gpdla_batch *b, int multi, int64_t quasar,
                                         double *rows_out, int64_t capacity_rows, int64_t *num_rows_out) {
  if (!c || !b || b->ctx != c || !rows_out || !num_rows_out)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched argument");
  if (quasar < 0 || quasar >= b->nq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "quasar %lld outside the batch", (long long)quasar);
  if (b->fx && b->fx->on) return fail(GPDLA_ERR_UNSUPPORTED, "prepared rows: the batch is conditioned on fixed absorbers (gpdla_debug_conditioned_rows)");
  HIP_TRY(hipSetDevice(c->device_id));
  int rc = plan_records(c, b, b->k <= 20 ? kSlimRec : record_doubles(b->ntiles, 0), true);
  if (rc) return rc;
  if ((rc = launch_prepare(c, b, multi != 0))) return rc;
  QuasarMeta m;
  HIP_TRY(hipMemcpyAsync(&m, b->d_meta + quasar, sizeof(m), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int64_t n = std::min<int64_t>(m.n_u, capacity_rows);
  static_assert(sizeof(PixelRow) == 4 * sizeof(double), "rows_out is [n][4] doubles");
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(rows_out, b->d_pix + m.pix_off, (size_t)n * sizeof(PixelRow), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  *num_rows_out = n;
  return GPDLA_OK;
}
