// host_multi.hpp -- the multi-DLA sweep of a resident batch
// (multi_dlas/process_qsos_multiple_dlas_meanflux.m:141-495): the result tables and the context's
// profile table, gpdla_batch_process_multi, the download of its results.
#pragma once

namespace {

// One pass (args.mode) over a sub-batch of the profile table, on records of class `cls`
int launch_sweep_multi(gpdla_context *c, gpdla_batch *b, RecordClass cls, const SweepMultiArgs &args) {
  if (cls == kRecSlim20)  // k <= 20 (k_sweep_multi with k_sweep_slim's in-sweep vech expansion)
    return dispatch_nd(args.mode, [&](auto nd) {
      return launch_sweep_kernel(c, &k_sweep_multi_slim<decltype(nd)::value>, 512, sweep_multi_slim_lds_doubles() * sizeof(double),
                                 kSweepWaves * kSamplesPerWave, args.nq_sub, args);
    });
  if (cls == kRecSlim40) {  // 20 < k <= 40 (k_sweep_split_slim with gathers in place of the Voigt stages)
    const size_t lds = std::max(sweep_split_slim_lds_doubles(true), kExpTab + kSplitEpilogueDoubles) * sizeof(double);
    if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "multi split sweep needs %zu B of LDS", lds);
    return dispatch_nd(args.mode, [&](auto nd) {
      return launch_sweep_kernel(c, &k_sweep_split_slim<0, decltype(nd)::value, SweepMultiArgs>, 512, lds, 2 * kSamplesPerWave,
                                 args.nq_sub, args);
    });
  }
  return legacy_sweep_multi(c, b, args);
}

// Result tables of a multi-DLA batch (allocated on first use, kept while the batch does not grow)
// and the context's profile table.
int multi_alloc(gpdla_batch *b) {
  MultiBuffers &mb = *b->mb;
  gpdla_context *c = b->ctx;
  const size_t nqs = (size_t)b->nq, S = (size_t)b->S;
  const int md = b->md;
  int rc = GPDLA_OK;
  auto chk = [&](int x) { if (x && !rc) rc = x; };
  if (mb.sll_dla && (b->nq > mb.cap_nq || b->S != mb.cap_S || md != mb.cap_md)) mb.free_tables();
  if (!mb.sll_dla) {
    chk(dev_alloc(&mb.sll_dla, nqs * md * S));
    chk(dev_alloc(&mb.sll_lls, nqs * S));
    chk(dev_alloc(&mb.ll_no, nqs));
    chk(dev_alloc(&mb.ll_dla, nqs * md));
    chk(dev_alloc(&mb.ll_lls, nqs));
    chk(dev_alloc(&mb.map_z, nqs * md * md));
    chk(dev_alloc(&mb.map_n, nqs * md * md));
    chk(dev_alloc(&mb.map_i, nqs * md * md));
    chk(dev_alloc(&mb.base, nqs * (md > 1 ? md - 1 : 1) * S));
    chk(dev_alloc(&mb.alive, nqs));
    chk(dev_alloc(&mb.post, nqs * (2 + md)));
    chk(dev_alloc(&mb.scal, nqs * (5 + md)));
    chk(dev_alloc(&mb.summary, nqs * GPDLA_SUMMARY_COLS_MULTI(md)));
    if (rc) {
      mb.free_tables();
      return rc;
    }
    mb.cap_nq = b->nq;
    mb.cap_S = b->S;
    mb.cap_md = md;
  }
  // profile table: rows of `stride` doubles, 2 S rows per quasar, sub-batches sized to the budget
  const int64_t stride = ((4 * ((b->max_pix + 3) / 4) + 4 + 15) / 16) * 16;
  const double per_q = 2.0 * (double)S * (double)stride * sizeof(double);
  const double budget = c->cfg.multi_profile_bytes > 0 ? (double)c->cfg.multi_profile_bytes : 16.0 * 1073741824.0;
  int64_t nq_sub = (int64_t)std::max(1.0, std::floor(budget / per_q));
  nq_sub = std::min(nq_sub, b->nq);
  const size_t need = (size_t)nq_sub * 2 * S * stride;
  if (c->prof_capacity < need) {
    HIP_TRY(hipStreamSynchronize(c->stream));  // an earlier call's sweeps may still read the old table
    dev_free(c->d_prof);
    c->d_prof = nullptr;
    c->prof_capacity = 0;
    if ((rc = dev_alloc(&c->d_prof, need))) return rc;
    c->prof_capacity = need;
    // (Touching the fresh table once here -- a 15 GB hipMemsetAsync -- was tried in round 4 against the
    // slower first k_profiles launch into never-written memory: no change in the call, 46.35 vs 46.34 ms,
    // k_profiles still 4.2-5.1 ms; the memset costs what it saves.  Dropped.)
  }
  mb.prof_quasars = nq_sub;
  mb.prof_stride = stride;
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_batch_process_multi(gpdla_context *c, gpdla_batch *b, const uint32_t *base_in) try {
  if (!c || !b || b->ctx != c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched context or batch");
  if (!b->md) return fail(GPDLA_ERR_INVALID_ARGUMENT, "not a multi-DLA batch (upload it with log_priors_lls)");
  if (b->S != c->S || b->k != c->model.k)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "model/samples changed after the batch was uploaded");
  const int64_t nq = b->nq, S = b->S;
  const int md = b->md;
  if (md != c->cfg.max_dlas)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "max_dlas changed after the batch was uploaded (%d -> %d)", md, c->cfg.max_dlas);
  if (!c->d_lls_nhi || !c->d_log_nhi)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "multi-DLA needs lls_nhi_samples and log_nhi_samples");
  const size_t nqs = (size_t)nq;
  const size_t nbase = nqs * (md > 1 ? md - 1 : 0) * S;
  if (base_in)  // 0 = never drawn (the sample is NaN); anything above S cannot be an index
    for (size_t e = 0; e < nbase; ++e)
      if (base_in[e] > (uint64_t)S)
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "base_sample_inds[%zu] = %u exceeds num_dla_samples = %lld",
                    e, base_in[e], (long long)S);
  HIP_TRY(hipSetDevice(c->device_id));
  std::lock_guard<std::mutex> multi_lock(c->multi_mu);  // the profile table is the context's: one call's launches at a time
  hipStream_t st = c->stream;
  int rc = multi_alloc(b);
  if (rc) return rc;
  MultiBuffers &mb = *b->mb;
  if ((rc = begin_timing(c, st))) return rc;
  // (the multi-DLA sweeps walk the batch in profile-table sub-batches of their own: all records
  // are built up front, one group)
  const RecordClass cls = legacy_record_class(b->k, b->k <= 20 ? kRecSlim20 : kRecSlim40);
  if ((rc = plan_records(c, b, record_class_doubles(cls, b->ntiles, false), true))) return rc;
  if ((rc = launch_prepare(c, b, true))) return rc;
  if ((rc = launch_build_records(c, b, 0, b->nq, false, cls))) return rc;
  // NaN pre-fill (multi :110-131); alive != 0; base = 0 (multi :116) or the caller's indices
  HIP_TRY(hipMemsetAsync(mb.sll_dla, 0xFF, nqs * md * S * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.sll_lls, 0xFF, nqs * S * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.ll_no, 0xFF, nqs * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.ll_dla, 0xFF, nqs * md * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.ll_lls, 0xFF, nqs * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.map_z, 0xFF, nqs * md * md * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.map_n, 0xFF, nqs * md * md * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.map_i, 0xFF, nqs * md * md * sizeof(double), st));
  HIP_TRY(hipMemsetAsync(mb.alive, 0x01, nqs * sizeof(int32_t), st));
  if (base_in && nbase) {
    // the caller's buffer is consumed before this call returns (gpdla.h): a pageable source may
    // otherwise still be read by the copy engine after the caller has freed it
    HIP_TRY(hipMemcpyAsync(mb.base, base_in, nbase * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
  } else
    HIP_TRY(hipMemsetAsync(mb.base, 0, (nbase ? nbase : 1) * sizeof(uint32_t), st));

  const int64_t nq_sub = mb.prof_quasars, stride = mb.prof_stride;
  const double log_S = std::log((double)S);
  for (int64_t q0 = 0; q0 < nq; q0 += nq_sub) {
    const int32_t nsub = (int32_t)std::min(nq_sub, nq - q0);
    ProfilesArgs pa;
    pa.meta = b->d_meta;
    pa.lam_pad = b->d_lam;
    pa.offset_samples = c->d_offset;
    pa.nhi_samples = c->d_nhi;
    pa.lls_nhi_samples = c->d_lls_nhi;
    pa.perm = c->d_perm;
    pa.S = S;
    pa.num_lines = c->cfg.num_lines;
    pa.q0 = q0;
    pa.nq_sub = nsub;
    pa.stride = stride;
    pa.prof = c->d_prof;
    const int64_t waves = (int64_t)nsub * ((S + 63) / 64);  // one wave per 64 samples, both kinds
    hipLaunchKernelGGL(k_profiles, dim3((unsigned)((waves + kProfWaves - 1) / kProfWaves)), dim3(kProfWaves * 64), 0, st, pa);
    HIP_TRY(hipGetLastError());
    for (int mode = 1; mode <= md; ++mode) {
      for (int pass = (mode == 1 ? 0 : 1); pass < 2; ++pass) {  // the LLS pass (mode 0) rides with model 1
        SweepMultiArgs sa;
        sa.meta = b->d_meta;
        sa.records = b->d_records;
        sa.prof = c->d_prof;
        sa.base_inds = mb.base;
        sa.alive = mb.alive;
        sa.S = S;
        sa.q0 = q0;
        sa.stride = stride;
        sa.nq_sub = nsub;
        sa.blocks_per_quasar = 0;
        sa.k = b->k;
        sa.mode = pass == 0 ? 0 : mode;
        sa.max_dlas = md;
        sa.log_S = log_S;
        sa.sample_ll_dla = mb.sll_dla;
        sa.sample_ll_lls = mb.sll_lls;
        sa.ll_no_dla = mb.ll_no;
        sa.pix = b->d_pix;
        if ((rc = launch_sweep_multi(c, b, cls, sa))) return rc;
      }
      // evidence, MAP, early-exit flags for the quasars of this sub-batch
      MultiEvidenceArgs ea;
      ea.meta = b->d_meta + q0;
      ea.offset_samples = c->d_offset;
      ea.log_nhi_samples = c->d_log_nhi;
      ea.base_inds = mb.base + (size_t)q0 * (md > 1 ? md - 1 : 0) * S;
      ea.alive = mb.alive + q0;
      ea.S = S;
      ea.nd = mode;
      ea.max_dlas = md;
      ea.min_z_separation = c->cfg.min_z_separation;
      ea.log_S = log_S;
      ea.sample_ll_dla = mb.sll_dla + (size_t)q0 * md * S;
      ea.sample_ll_lls = mb.sll_lls + (size_t)q0 * S;
      ea.ll_dla = mb.ll_dla + (size_t)q0 * md;
      ea.ll_lls = mb.ll_lls + q0;
      ea.map_z = mb.map_z + (size_t)q0 * md * md;
      ea.map_lognhi = mb.map_n + (size_t)q0 * md * md;
      ea.map_ind = mb.map_i + (size_t)q0 * md * md;
      hipLaunchKernelGGL(k_multi_evidence, dim3((unsigned)nsub), dim3(256), 0, st, ea);
      HIP_TRY(hipGetLastError());
      if (mode < md && !base_in) {  // multi :467-472
        MultiResampleArgs ra;
        ra.meta = b->d_meta + q0;
        ra.alive = mb.alive + q0;
        ra.sample_ll_dla = mb.sll_dla + (size_t)q0 * md * S;
        ra.S = S;
        ra.first_quasar_index = c->cfg.first_quasar_index + q0;
        ra.seed = c->cfg.rng_seed;
        ra.nd = mode;
        ra.max_dlas = md;
        ra.base_inds = mb.base + (size_t)q0 * (md - 1) * S;
        const size_t lds = (size_t)S * sizeof(double);
        if (lds > 150 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "resampling supports S <= 19200");
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_multi_resample),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_multi_resample, dim3((unsigned)nsub), dim3(256), lds, st, ra);
        HIP_TRY(hipGetLastError());
      }
    }
  }
  // posteriors over (no DLA, LLS, 1..max_dlas DLAs) + the summary row
  MultiPostArgs pp;
  pp.meta = b->d_meta;
  pp.nq = nq;
  pp.max_dlas = md;
  pp.lp_no = b->d_lp_no;
  pp.lp_lls = mb.lp_lls;
  pp.lp_dla = mb.lp_dla;
  pp.ll_no = mb.ll_no;
  pp.ll_lls = mb.ll_lls;
  pp.ll_dla = mb.ll_dla;
  pp.lpost_no = mb.scal;
  pp.lpost_lls = mb.scal + nqs;
  pp.p_no = mb.scal + 2 * nqs;
  pp.p_lls = mb.scal + 3 * nqs;
  pp.p_dla = mb.scal + 4 * nqs;
  pp.lpost_dla = mb.scal + 5 * nqs;
  pp.post = mb.post;
  pp.map_z = mb.map_z;
  pp.map_lognhi = mb.map_n;
  pp.map_ind = mb.map_i;
  pp.summary = mb.summary;
  hipLaunchKernelGGL(k_multi_posteriors, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, pp);
  HIP_TRY(hipGetLastError());
  if ((rc = end_timing(c, st))) return rc;
  HIP_TRY(hipEventRecord(b->ev_done, st));
  mb.processed = true;
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"

namespace {

// The results of a batch into rows [row0, row0 + nq) of the caller's arrays; each array of
// gpdla_results_multi is named here once, with its elements per quasar
int batch_download_multi(gpdla_context *c, gpdla_batch *b, const gpdla_results_multi &r, int64_t row0) {
  if (!c || !b || b->ctx != c) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched argument");
  if (!b->md || !b->mb || !b->mb->processed)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "no multi-DLA results: call gpdla_batch_process_multi first");
  HIP_TRY(hipSetDevice(c->device_id));
  MultiBuffers &mb = *b->mb;
  hipStream_t st = c->down_stream;  // behind this batch's last kernel, beside other batches' sweeps
  const size_t nqs = (size_t)b->nq, S = (size_t)b->S, md = (size_t)b->md;
  int rc = GPDLA_OK;
  auto chk = [&](int x) { if (x && !rc) rc = x; };
  std::vector<QuasarMeta> meta(nqs);
  StreamDrain drain{st};  // (also covers the caller's arrays: nothing is in flight once this returns)
  HIP_TRY(hipStreamWaitEvent(st, b->ev_done, 0));
  HIP_TRY(hipMemcpyAsync(meta.data(), b->d_meta, nqs * sizeof(QuasarMeta), hipMemcpyDeviceToHost, st));
  auto dl = [&](auto *dst, const void *src, size_t width) -> int {
    if (dst && width) HIP_TRY(hipMemcpyAsync(dst + row0 * width, src, nqs * width * sizeof(*dst), hipMemcpyDeviceToHost, st));
    return GPDLA_OK;
  };
  chk(dl(r.log_likelihoods_no_dla, mb.ll_no, 1));
  chk(dl(r.sample_log_likelihoods_dla, mb.sll_dla, md * S));
  chk(dl(r.sample_log_likelihoods_lls, mb.sll_lls, S));
  chk(dl(r.log_likelihoods_dla, mb.ll_dla, md));
  chk(dl(r.log_likelihoods_lls, mb.ll_lls, 1));
  chk(dl(r.log_posteriors_no_dla, mb.scal, 1));
  chk(dl(r.log_posteriors_lls, mb.scal + nqs, 1));
  chk(dl(r.log_posteriors_dla, mb.scal + 5 * nqs, md));
  chk(dl(r.model_posteriors, mb.post, 2 + md));
  chk(dl(r.p_no_dlas, mb.scal + 2 * nqs, 1));
  chk(dl(r.p_lls, mb.scal + 3 * nqs, 1));
  chk(dl(r.p_dlas, mb.scal + 4 * nqs, 1));
  chk(dl(r.MAP_z_dlas, mb.map_z, md * md));
  chk(dl(r.MAP_log_nhis, mb.map_n, md * md));
  chk(dl(r.MAP_inds, mb.map_i, md * md));
  chk(dl(r.base_sample_inds, mb.base, (md - 1) * S));
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t q = 0; q < nqs; ++q) {
    if (r.min_z_dlas) r.min_z_dlas[row0 + q] = meta[q].min_z_dla;
    if (r.max_z_dlas) r.max_z_dlas[row0 + q] = meta[q].max_z_dla;
    if (r.status) r.status[row0 + q] = meta[q].status;
  }
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_batch_download_multi(gpdla_context *c, gpdla_batch *b, gpdla_results_multi *r) try {
  if (!r) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched argument");
  return batch_download_multi(c, b, *r, 0);
} GPDLA_NO_THROW

int gpdla_batch_summary_multi_device_ptr(gpdla_batch *b, double **table, int64_t *nq, int32_t *cols) try {
  if (!b || !table) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (!b->md || !b->mb || !b->mb->summary)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "no multi-DLA results: call gpdla_batch_process_multi first");
  *table = b->mb->summary;
  if (nq) *nq = b->nq;
  if (cols) *cols = GPDLA_SUMMARY_COLS_MULTI(b->md);
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_batch_samples_multi_device_ptr(gpdla_batch *b, double **sll_dla, double **sll_lls,
                                         uint32_t **base) try {
  if (!b) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (!b->md || !b->mb || !b->mb->sll_dla)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "no multi-DLA results: call gpdla_batch_process_multi first");
  if (sll_dla) *sll_dla = b->mb->sll_dla;
  if (sll_lls) *sll_lls = b->mb->sll_lls;
  if (base) *base = b->mb->base;
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
