// host_pipeline.hpp -- the one-shot entries of include/gpdla.h: host buffers in, host buffers out, the
// quasars cut into blocks that go through a three-stage pipeline of uploads, sweeps and downloads.
#pragma once

/* ------------------------------ one-shot entries: the host pipeline ------------------------------ */

namespace {

// Touch every page of a caller-owned output array without changing its contents, so that the
// device-to-host copies into it do not run at page-fault speed (4 GB/s measured into untouched
// pageable memory, 10+ once the pages exist).  MADV_POPULATE_WRITE where the kernel has it.
void prefault_pages(void *p, size_t bytes) {
  if (!p || !bytes) return;
  const uintptr_t page = 4096, lo = ((uintptr_t)p + page - 1) & ~(page - 1), hi = ((uintptr_t)p + bytes) & ~(page - 1);
  if (hi <= lo) return;
#ifdef MADV_POPULATE_WRITE
  if (madvise(reinterpret_cast<void *>(lo), hi - lo, MADV_POPULATE_WRITE) == 0) return;
#endif
  for (uintptr_t a = lo; a < hi; a += page) {
    volatile char *c = reinterpret_cast<volatile char *>(a);
    *c = *c;
  }
}

// Three stages over `nblocks` blocks of quasars and `slots` HBM-resident batch slots, the loop of
// process_qsos.m:88 as a pipeline: an upload thread fills slot i % slots with block i (once the slot's
// previous results are on the host), the calling thread launches the sweeps in order, a download
// thread copies block i's results into the caller's arrays.  The library's copy streams run beside
// the compute stream (gpdla.h, gpdla_batch_download), so while block i is swept block i+1 is
// uploaded and block i-1 downloaded.  The first error of any stage stops all three; its message
// becomes the calling thread's gpdla_last_error().
struct HostPipeline {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<char> uploaded, processed, downloaded;
  int err = GPDLA_OK;
  std::string msg;

  explicit HostPipeline(size_t n) : uploaded(n, 0), processed(n, 0), downloaded(n, 0) {}
  void raise(int rc) {  // called on the failing thread: t_error is that thread's message
    std::lock_guard<std::mutex> lock(mu);
    if (!err) {
      err = rc;
      msg = t_error;
    }
    cv.notify_all();
  }
  bool wait(const std::vector<char> &flag, size_t i) {
    std::unique_lock<std::mutex> lock(mu);
    cv.wait(lock, [&] { return err || flag[i]; });
    return !err;
  }
  void set(std::vector<char> &flag, size_t i) {
    std::lock_guard<std::mutex> lock(mu);
    flag[i] = 1;
    cv.notify_all();
  }
};

template <class Up, class Proc, class Down, class Warm>
int run_host_pipeline(size_t nblocks, size_t slots, Up up, Proc proc, Down down, Warm warm) {
  HostPipeline ps(nblocks);
  auto guarded = [&](auto &&body) {
    try {
      body();
    } catch (const std::bad_alloc &) {
      fail(GPDLA_ERR_HOST, "host pipeline: out of host memory");
      ps.raise(GPDLA_ERR_HOST);
    } catch (const std::exception &e) {
      fail(GPDLA_ERR_HOST, "host pipeline: %s", e.what());
      ps.raise(GPDLA_ERR_HOST);
    } catch (...) {  // (a stage thread that lets an exception escape ends the process)
      fail(GPDLA_ERR_HOST, "host pipeline: unexpected C++ exception");
      ps.raise(GPDLA_ERR_HOST);
    }
  };
  auto upload_stage = [&] {
    guarded([&] {
      for (size_t i = 0; i < nblocks; ++i) {
        if (i >= slots && !ps.wait(ps.downloaded, i - slots)) return;
        if (int rc = up(i, i % slots)) return ps.raise(rc);
        ps.set(ps.uploaded, i);
      }
    });
  };
  auto download_stage = [&] {
    guarded([&] {
      warm();
      for (size_t i = 0; i < nblocks; ++i) {
        if (!ps.wait(ps.processed, i)) return;
        if (int rc = down(i, i % slots)) return ps.raise(rc);
        ps.set(ps.downloaded, i);
      }
    });
  };
  // (a thread that cannot be started -- std::system_error -- must not leave the other one running, nor
  // an exception cross the C boundary: the stages that did start are told to stop and joined)
  std::thread uploader, downloader;
  try {
    uploader = std::thread(upload_stage);
    downloader = std::thread(download_stage);
  } catch (const std::exception &e) {
    fail(GPDLA_ERR_HOST, "host pipeline: cannot start a thread: %s", e.what());
    ps.raise(GPDLA_ERR_HOST);
  }
  guarded([&] {
    for (size_t i = 0; i < nblocks; ++i) {
      if (!ps.wait(ps.uploaded, i)) return;
      if (int rc = proc(i, i % slots)) return ps.raise(rc);
      ps.set(ps.processed, i);
    }
  });
  if (uploader.joinable()) uploader.join();
  if (downloader.joinable()) downloader.join();
  if (ps.err) return fail(ps.err, "%s", ps.msg.c_str());
  return GPDLA_OK;
}

// api.record_bytes_per_quasar / resident_bytes_per_quasar: what a quasar of `npix` stored pixels
// occupies in a resident batch
int64_t batch_bytes_per_quasar(int64_t npix, int k, int64_t S, int multi_models) {
  const double rows = (double)(npix + 8) * (k + 4 + 1 + 3.2) * 8.0;
  int64_t per_q = (int64_t)(rows + 8.0 * (double)S * std::max(1, 2 * multi_models));
  if (multi_models)  // the multi-DLA sweeps build all records of a batch up front
    per_q += (int64_t)(((double)npix / 4.0 + 2.0) * (k <= 20 ? 896 : 1536));
  return per_q;
}

struct BlockPlan {
  size_t slots = 1;
  std::vector<std::pair<int64_t, int64_t>> blocks;
};

int plan_blocks(int64_t nq, int64_t longest, const gpdla_config &cfg, int k, int64_t S, int multi_models, BlockPlan *plan) {
  if (cfg.pipeline_slots < 0 || cfg.max_quasars_per_batch < 0)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "pipeline_slots and max_quasars_per_batch must be >= 0");
  const int slots = cfg.pipeline_slots > 0 ? cfg.pipeline_slots : 3;
  const int64_t per_batch = cfg.max_quasars_per_batch > 0
                                ? cfg.max_quasars_per_batch
                                : gpdla_default_batch_quasars(nq, longest, k, S, slots, 0, multi_models);
  for (int64_t lo = 0; lo < nq; lo += per_batch) plan->blocks.emplace_back(lo, std::min(lo + per_batch, nq));
  // (Measured and not kept, profiles/r05_one_shot_timing.txt: a short last block -- an eighth of a block, so
  // that the one download nothing overlaps is small.  The call ends ~4 ms behind its last sweep either
  // way: that tail is the latency of the stage hand-offs and of the copies' synchronisation, not bytes.)
  plan->slots = std::min<size_t>((size_t)slots, plan->blocks.size());
  return GPDLA_OK;
}

// Where a one-shot call's spectra come from: CSR arrays (a block is a pointer shift, nothing is
// copied on the host) or one array per quasar, as preloaded_qsos.mat's cell arrays hold them (a
// block is flattened into its batch slot's staging vectors by the upload thread, beside the sweeps).
struct CsrSource {
  const gpdla_spectra *sp;
  int md;
  int validate(int64_t *longest) const {
    if (sp->num_quasars < 1 || !sp->offsets || !sp->z_qsos || !sp->log_priors_no_dla || !sp->log_priors_dla)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/empty spectra field");
    *longest = 1;
    for (int64_t q = 0; q < sp->num_quasars; ++q) {
      if (sp->offsets[q + 1] < sp->offsets[q])
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing (quasar %lld)", (long long)q);
      *longest = std::max(*longest, sp->offsets[q + 1] - sp->offsets[q]);
    }
    return GPDLA_OK;
  }
  int64_t num_quasars() const { return sp->num_quasars; }
  int block(int64_t lo, int64_t hi, size_t, gpdla_spectra *out) const {
    *out = *sp;  // the pixel arrays are indexed through offsets
    out->num_quasars = hi - lo;
    out->offsets = sp->offsets + lo;
    out->z_qsos = sp->z_qsos + lo;
    out->log_priors_no_dla = sp->log_priors_no_dla + lo;
    out->log_priors_dla = sp->log_priors_dla + lo * (md ? md : 1);
    if (sp->log_priors_lls) out->log_priors_lls = sp->log_priors_lls + lo;
    return GPDLA_OK;
  }
};

struct CellSource {
  const gpdla_spectra_cells *sp;
  int md;
  struct Staging {
    std::vector<int64_t> offsets;
    std::vector<double> wl, flux, nv;
    std::vector<uint8_t> mask;
  };
  mutable std::vector<Staging> staging;  // one per batch slot; touched by the upload thread only
  CellSource(const gpdla_spectra_cells *cells, int max_dlas, const gpdla_config &cfg)
      : sp(cells), md(max_dlas), staging(cfg.pipeline_slots > 0 ? (size_t)cfg.pipeline_slots : 3) {}
  int validate(int64_t *longest) const {
    if (sp->num_quasars < 1 || !sp->num_pixels || !sp->wavelengths || !sp->flux || !sp->noise_variance || !sp->pixel_mask ||
        !sp->z_qsos || !sp->log_priors_no_dla || !sp->log_priors_dla)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/empty spectra field");
    *longest = 1;
    for (int64_t q = 0; q < sp->num_quasars; ++q) {
      const int64_t n = sp->num_pixels[q];
      if (n < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_pixels[%lld] is negative", (long long)q);
      if (n > 0 && (!sp->wavelengths[q] || !sp->flux[q] || !sp->noise_variance[q] || !sp->pixel_mask[q]))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "quasar %lld: null cell", (long long)q);
      *longest = std::max(*longest, n);
    }
    return GPDLA_OK;
  }
  int64_t num_quasars() const { return sp->num_quasars; }
  int block(int64_t lo, int64_t hi, size_t slot, gpdla_spectra *out) const {
    Staging &st = staging[slot];
    const size_t nq = (size_t)(hi - lo);
    st.offsets.resize(nq + 1);
    st.offsets[0] = 0;
    for (size_t q = 0; q < nq; ++q) st.offsets[q + 1] = st.offsets[q] + sp->num_pixels[lo + (int64_t)q];
    const size_t total = (size_t)st.offsets[nq];
    st.wl.resize(total);
    st.flux.resize(total);
    st.nv.resize(total);
    st.mask.resize(total);
    for (size_t q = 0; q < nq; ++q) {
      const size_t at = (size_t)st.offsets[q], n = (size_t)sp->num_pixels[lo + (int64_t)q];
      if (!n) continue;
      std::memcpy(st.wl.data() + at, sp->wavelengths[lo + (int64_t)q], n * sizeof(double));
      std::memcpy(st.flux.data() + at, sp->flux[lo + (int64_t)q], n * sizeof(double));
      std::memcpy(st.nv.data() + at, sp->noise_variance[lo + (int64_t)q], n * sizeof(double));
      std::memcpy(st.mask.data() + at, sp->pixel_mask[lo + (int64_t)q], n);
    }
    std::memset(out, 0, sizeof *out);
    out->num_quasars = (int64_t)nq;
    out->offsets = st.offsets.data();
    out->wavelengths = st.wl.data();
    out->flux = st.flux.data();
    out->noise_variance = st.nv.data();
    out->pixel_mask = st.mask.data();
    out->z_qsos = sp->z_qsos + lo;
    out->log_priors_no_dla = sp->log_priors_no_dla + lo;
    out->log_priors_dla = sp->log_priors_dla + lo * (md ? md : 1);
    out->log_priors_lls = sp->log_priors_lls ? sp->log_priors_lls + lo : nullptr;
    return GPDLA_OK;
  }
};

struct OneShot {  // context + batch slots of a one-shot call, released on every exit path
  gpdla_context *c = nullptr;
  std::vector<gpdla_batch *> batches;
  ~OneShot() {
    for (gpdla_batch *b : batches) gpdla_batch_destroy(b);
    gpdla_context_destroy(c);
  }
  int open(const gpdla_model *model, const gpdla_samples *samples, const gpdla_config &cfg, int device_id) {
    int rc = gpdla_context_create(device_id, &c);
    if (!rc) rc = gpdla_context_set_config(c, &cfg);
    if (!rc) rc = gpdla_context_set_model(c, model);
    if (!rc) rc = gpdla_context_set_samples(c, samples);
    return rc;
  }
};

gpdla_config config_or_default(const gpdla_config *config) {
  gpdla_config cfg;
  gpdla_default_config(&cfg);
  if (config) cfg = *config;
  return cfg;
}

// The times of a one-shot call, in ms from its entry (kOneShotTiming, host_common.hpp)
struct OneShotReport {
  double t_in = wall_ms();
  double open = 0, staged0 = 0, up0 = 0, proc0 = 0, proc_last = 0, down_last = 0, pipeline = 0;
  void mark(double &what, bool when = true) {
    if (kOneShotTiming && when) what = wall_ms() - t_in;
  }
  ~OneShotReport() {
    if (kOneShotTiming)
      std::fprintf(stderr, "[one-shot] context open %.2f ms | block 0 staged at %.2f, uploaded at %.2f, launched at %.2f | last launch at %.2f, "
                   "last download done at %.2f, pipeline returned at %.2f, context closed at %.2f\n", open, staged0, up0, proc0, proc_last,
                   down_last, pipeline, wall_ms() - t_in);
  }
};

// Every quasar of `src` through the pipeline (run_host_pipeline): blocks planned for `multi_models`
// models (0: single-DLA), a context of the call's own, one batch slot per pipeline slot filled by
// the upload stage.  proc(ctx, batch, lo) sweeps the block that starts at quasar lo,
// down(ctx, batch, lo) copies its results out, warm() runs on the download thread in front of them.
template <class Source, class Proc, class Down, class Warm>
int one_shot(const gpdla_model *model, const gpdla_samples *samples, const Source &src, const gpdla_config &cfg,
             int multi_models, int device_id, Proc proc, Down down, Warm warm) {
  int64_t longest = 1;
  int rc = src.validate(&longest);
  if (rc) return rc;
  BlockPlan plan;
  if ((rc = plan_blocks(src.num_quasars(), longest, cfg, model->k, samples->num_dla_samples, multi_models, &plan))) return rc;
  OneShotReport report;  // (declared in front of `os`: destroyed behind it)
  OneShot os;
  if ((rc = os.open(model, samples, cfg, device_id))) return rc;
  report.mark(report.open);
  os.batches.assign(plan.slots, nullptr);
  const size_t last = plan.blocks.size() - 1;
  auto up = [&](size_t i, size_t slot) {
    gpdla_spectra sp;
    if (int r = src.block(plan.blocks[i].first, plan.blocks[i].second, slot, &sp)) return r;
    report.mark(report.staged0, i == 0);
    const int r = os.batches[slot] ? gpdla_batch_reload(os.c, os.batches[slot], &sp) : gpdla_batch_upload(os.c, &sp, &os.batches[slot]);
    report.mark(report.up0, i == 0);
    return r;
  };
  auto proc_stage = [&](size_t i, size_t slot) {
    const int r = proc(os.c, os.batches[slot], plan.blocks[i].first);
    report.mark(report.proc0, i == 0);
    report.mark(report.proc_last, i == last);
    return r;
  };
  auto down_stage = [&](size_t i, size_t slot) {
    const int r = down(os.c, os.batches[slot], plan.blocks[i].first);
    report.mark(report.down_last, i == last);
    return r;
  };
  rc = run_host_pipeline(plan.blocks.size(), plan.slots, up, proc_stage, down_stage, warm);
  report.mark(report.pipeline);
  return rc;
}

// process_qsos.m:88-233 for every quasar of `src`
template <class Source>
int one_shot_single(const gpdla_model *model, const gpdla_samples *samples, const Source &src, const gpdla_config &cfg,
                    gpdla_results *results, int device_id) {
  const int64_t S = samples->num_dla_samples;
  return one_shot(
      model, samples, src, cfg, 0, device_id,
      [&](gpdla_context *c, gpdla_batch *b, int64_t) { return gpdla_batch_process(c, b); },
      [&](gpdla_context *c, gpdla_batch *b, int64_t lo) { return batch_download(c, b, *results, lo); },
      [&] { prefault_pages(results->sample_log_likelihoods_dla, (size_t)src.num_quasars() * S * sizeof(double)); });
}

// multi_dlas/process_qsos_multiple_dlas_meanflux.m:141-495 for every quasar of `src`
template <class Source>
int one_shot_multi(const gpdla_model *model, const gpdla_samples *samples, const Source &src, const uint32_t *base_sample_inds,
                   const gpdla_config &cfg, gpdla_results_multi *results, int device_id) {
  const int md = cfg.max_dlas;
  if (md < 1 || md > 4) return fail(GPDLA_ERR_UNSUPPORTED, "max_dlas = %d outside [1, 4]", md);
  const int64_t S = samples->num_dla_samples, nbase_row = (int64_t)(md - 1) * S;
  return one_shot(
      model, samples, src, cfg, md + 1, device_id,
      [&](gpdla_context *c, gpdla_batch *b, int64_t lo) {
        // the draws of the resampling are keyed by the quasar's index in the whole call (multi :467-472)
        int rc = gpdla_context_set_first_quasar_index(c, cfg.first_quasar_index + lo);
        if (rc) return rc;
        return gpdla_batch_process_multi(c, b, base_sample_inds ? base_sample_inds + lo * nbase_row : nullptr);
      },
      [&](gpdla_context *c, gpdla_batch *b, int64_t lo) { return batch_download_multi(c, b, *results, lo); },
      [&] {
        const size_t nq = (size_t)src.num_quasars();
        prefault_pages(results->sample_log_likelihoods_dla, nq * md * S * sizeof(double));
        prefault_pages(results->sample_log_likelihoods_lls, nq * S * sizeof(double));
        prefault_pages(results->base_sample_inds, nq * nbase_row * sizeof(uint32_t));
      });
}

}  // namespace

extern "C" {

int64_t gpdla_default_batch_quasars(int64_t num_quasars, int64_t longest_spectrum, int k, int64_t num_dla_samples,
                                    int slots, int64_t budget_bytes, int multi_models) {
  const double budget = budget_bytes > 0 ? (double)budget_bytes : 96.0 * 1073741824.0;
  const int64_t per_q = batch_bytes_per_quasar(std::max<int64_t>(longest_spectrum, 1), k, num_dla_samples, multi_models);
  const int64_t cap = std::max<int64_t>(1, (int64_t)(budget / std::max(slots, 1) / (double)per_q));
  const int64_t want = std::max<int64_t>(128, (num_quasars + 7) / 8);
  return std::max<int64_t>(1, std::min({cap, want, (int64_t)4096}));
}

int gpdla_process_batch(const gpdla_model *model, const gpdla_samples *samples,
                        const gpdla_spectra *spectra, const gpdla_config *config,
                        gpdla_results *results, int device_id) try {
  if (!model || !samples || !spectra || !results)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (spectra->log_priors_lls)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "log_priors_lls given: use gpdla_process_batch_multi");
  return one_shot_single(model, samples, CsrSource{spectra, 0}, config_or_default(config), results, device_id);
} GPDLA_NO_THROW

int gpdla_process_cells(const gpdla_model *model, const gpdla_samples *samples,
                        const gpdla_spectra_cells *spectra, const gpdla_config *config,
                        gpdla_results *results, int device_id) try {
  if (!model || !samples || !spectra || !results)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (spectra->log_priors_lls)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "log_priors_lls given: use gpdla_process_cells_multi");
  const gpdla_config cfg = config_or_default(config);
  return one_shot_single(model, samples, CellSource(spectra, 0, cfg), cfg, results, device_id);
} GPDLA_NO_THROW

int gpdla_process_batch_multi(const gpdla_model *model, const gpdla_samples *samples,
                              const gpdla_spectra *spectra, const uint32_t *base_sample_inds,
                              const gpdla_config *config, gpdla_results_multi *results,
                              int device_id) try {
  if (!model || !samples || !spectra || !results)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (!spectra->log_priors_lls) return fail(GPDLA_ERR_INVALID_ARGUMENT, "multi-DLA needs log_priors_lls");
  const gpdla_config cfg = config_or_default(config);
  return one_shot_multi(model, samples, CsrSource{spectra, cfg.max_dlas}, base_sample_inds, cfg, results, device_id);
} GPDLA_NO_THROW

int gpdla_process_cells_multi(const gpdla_model *model, const gpdla_samples *samples,
                              const gpdla_spectra_cells *spectra, const uint32_t *base_sample_inds,
                              const gpdla_config *config, gpdla_results_multi *results,
                              int device_id) try {
  if (!model || !samples || !spectra || !results)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (!spectra->log_priors_lls) return fail(GPDLA_ERR_INVALID_ARGUMENT, "multi-DLA needs log_priors_lls");
  const gpdla_config cfg = config_or_default(config);
  return one_shot_multi(model, samples, CellSource(spectra, cfg.max_dlas, cfg), base_sample_inds, cfg, results, device_id);
} GPDLA_NO_THROW

}  // extern "C"
