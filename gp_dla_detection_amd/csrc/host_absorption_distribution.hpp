// host_absorption_distribution.hpp -- the per-pixel distribution of the absorption over the sample tables and the models
// (DESIGN.md 4.29): exceedance probabilities, minimum / maximum, histogram and quantiles, on a resident batch.  The
// selection, the weights, the staging of host tables and the model weights are MixturePlan's (host_grid.hpp), opened
// without the continuum's scratch rows; the single-DLA and the multi-DLA entry run one group loop.
// Kernels: absorption_distribution_kernels.hpp.
#pragma once

namespace {

// What the two requests ask of the reduction (the fields have the same names)
struct DistributionRequest {
  int32_t num_thresholds;
  const double *thresholds;
  int32_t num_bins;
  int32_t num_levels;
  const double *levels;
  template <typename Request>
  explicit DistributionRequest(const Request &q)
      : num_thresholds(q.num_thresholds), thresholds(q.thresholds), num_bins(q.num_bins), num_levels(q.num_levels), levels(q.levels) {}
};

// the checks of this product alone (the mixture's are validate_mixture / validate_mixture_multi)
int validate_distribution(const DistributionRequest &d) {
  if (d.num_thresholds < 0 || d.num_thresholds > kDistMaxThresholds)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_thresholds = %d outside [0, %d]", d.num_thresholds, kDistMaxThresholds);
  if (d.num_levels < 0 || d.num_levels > kDistMaxLevels)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_levels = %d outside [0, %d]", d.num_levels, kDistMaxLevels);
  if (d.num_thresholds > 0 && !d.thresholds) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_thresholds = %d but thresholds is null", d.num_thresholds);
  if (d.num_levels > 0 && !d.levels) return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_levels = %d but levels is null", d.num_levels);
  for (int j = 0; j < d.num_thresholds; ++j)
    if (!(d.thresholds[j] > 0.0 && d.thresholds[j] < 1.0))  // (a NaN fails both)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "thresholds[%d] = %g: thresholds lie strictly inside (0, 1)", j, d.thresholds[j]);
  for (int j = 0; j < d.num_levels; ++j)
    if (!(d.levels[j] > 0.0 && d.levels[j] < 1.0))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "levels[%d] = %g: quantile levels lie strictly inside (0, 1)", j, d.levels[j]);
  if (d.num_bins != 0 && (d.num_bins < kDistMinBins || d.num_bins > kDistMaxBins))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_bins = %d: 0 (no histogram) or %d .. %d", d.num_bins, kDistMinBins, kDistMaxBins);
  if (d.num_levels > 0 && d.num_bins == 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "quantiles are read off the histogram: num_bins = 0");
  if (d.num_thresholds == 0 && d.num_bins == 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "nothing requested: no thresholds and no bins");
  return GPDLA_OK;
}

int validate_absorption_distribution(const gpdla_absorption_distribution_request *rq, int64_t nq, int64_t S, bool has_lls, int *tables_out) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  int rc = validate_mixture(MixtureRequest(*rq), nq, S, has_lls, tables_out);
  return rc ? rc : validate_distribution(DistributionRequest(*rq));
}

template <int STAGE>
int launch_absorption_dist(const AbsorptionDistArgs &da, int64_t n, int max_nu, bool hist, hipStream_t st) {
  AbsorptionDistArgs a = da;
  const int range = (hist ? 1 : kDistTilesPlain) * kProfTile;
  a.ranges = std::max(1, (max_nu + range - 1) / range);
  if (n * a.ranges > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
  // the most waves whose histograms fit the CU's 160 KiB of LDS
  int nw = kDistMaxWaves;
  while (nw > 1 && absorption_dist_lds_doubles(nw, hist, a.num_bins) * sizeof(double) > (size_t)160 * 1024) --nw;
  const size_t lds = absorption_dist_lds_doubles(nw, hist, a.num_bins) * sizeof(double);
  const void *f = hist ? reinterpret_cast<const void *>(&k_absorption_dist<STAGE, true>)
                       : reinterpret_cast<const void *>(&k_absorption_dist<STAGE, false>);
  HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 grid((unsigned)(n * a.ranges)), block((unsigned)(nw * 64));
  if (hist) hipLaunchKernelGGL((k_absorption_dist<STAGE, true>), grid, block, lds, st, a);
  else hipLaunchKernelGGL((k_absorption_dist<STAGE, false>), grid, block, lds, st, a);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

// The product of an opened plan into the caller's arrays (out.offsets are written already; any other may be null)
int run_absorption_distribution(MixturePlan &plan, const DistributionRequest &d, const gpdla_absorption_distribution_multi &out) {
  gpdla_context *c = plan.c;
  const gpdla_batch *b = plan.b;
  Staging &sg = plan.sg;
  hipStream_t st = plan.st;
  const int64_t nsel = plan.nsel, nsub = plan.nsub, total = plan.gs.total;
  const size_t tot = plan.tot;
  const int T = d.num_thresholds, B = d.num_bins, Q = d.num_levels;
  const bool hist = B > 0 && (out.histogram || (Q > 0 && out.quantiles));  // a call that fetches no bins pays for none
  const int Bd = hist ? B : 0;
  int rc;

  double *d_prob = nullptr, *d_min = nullptr, *d_max = nullptr, *d_hist = nullptr, *d_quant = nullptr;
  int32_t *d_status = nullptr;
  if ((rc = sg.tmp.alloc(&d_prob, (size_t)std::max(T, 1) * tot)) || (rc = sg.tmp.alloc(&d_min, tot)) || (rc = sg.tmp.alloc(&d_max, tot)) ||
      (rc = sg.tmp.alloc(&d_hist, (size_t)std::max(Bd, 1) * tot)) || (rc = sg.tmp.alloc(&d_quant, (size_t)std::max(Q, 1) * tot)) ||
      (rc = sg.tmp.alloc(&d_status, (size_t)nsel)))
    return rc;
  // (gpdla_context_set_timing: the kernels from here on are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  AbsorptionInitArgs ia;
  ia.total = total;
  ia.num_thresholds = T;
  ia.num_bins = Bd;
  ia.prob = d_prob, ia.amin = d_min, ia.amax = d_max, ia.hist = d_hist;
  hipLaunchKernelGGL(k_absorption_init, dim3((unsigned)std::min<int64_t>(4096, (total + 255) / 256 + 1)), dim3(256), 0, st, ia);
  HIP_TRY(hipGetLastError());

  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    if ((rc = plan.begin_group(s0, n))) return rc;
    int max_nu = 0;
    for (int64_t s = s0; s < s0 + n; ++s) max_nu = std::max(max_nu, (int)plan.gs.meta[(size_t)plan.gs.sel[(size_t)s]].n_u);
    for (int comp = 0; comp < plan.ncomp; ++comp) {
      if (!plan.reaches(comp)) continue;
      const bool boxed = plan.boxed(comp);
      AbsorptionDistArgs da = {};
      da.meta = b->d_meta;
      da.lam_pad = b->d_lam;
      da.offset_samples = boxed ? c->d_ru : c->d_offset;
      da.nhi = boxed ? c->d_rv : plan.nhi(comp);
      da.perm = plan.perm(comp);
      da.sel = plan.gs.d_sel + s0;
      da.out_off = plan.gs.d_off + s0;
      da.w = plan.w(comp);
      da.pm = plan.pm(comp, s0);
      da.flag = plan.d_flag + (size_t)comp * nsel + s0;
      da.S = plan.samples(comp);
      da.num_lines = c->cfg.num_lines;
      da.num_bins = Bd;
      da.num_thresholds = T;
      for (int j = 0; j < kDistMaxThresholds; ++j) da.thresholds[j] = j < T ? d.thresholds[j] : -1.0;
      da.total = total;
      da.prob = d_prob, da.amin = d_min, da.amax = d_max, da.hist = d_hist;
      if (boxed) {
        da.rmeta = plan.sp.refined->rmeta;
        da.box = plan.sp.refined->box;
        da.rstatus = plan.sp.refined->d_status;
        rc = launch_absorption_dist<kDistBoxed>(da, n, max_nu, hist, st);
      } else if (comp >= 2) {
        da.base = plan.tab_base;
        da.base_start = plan.d_rows_base + s0;
        da.nslots = comp;
        rc = launch_absorption_dist<kDistProduct>(da, n, max_nu, hist, st);
      } else {
        rc = launch_absorption_dist<kDistOwn>(da, n, max_nu, hist, st);
      }
      if (rc) return rc;
    }
  }
  AbsorptionCombineArgs ca = {};
  ca.meta = b->d_meta;
  ca.sel = plan.gs.d_sel;
  ca.out_off = plan.gs.d_off;
  ca.pw = plan.d_pw;
  ca.flag = plan.d_flag;
  ca.flag_stride = nsel;
  ca.sampled = plan.ncomp;
  ca.num_thresholds = T;
  ca.num_bins = Bd;
  ca.num_levels = Q;
  for (int j = 0; j < Q; ++j) ca.levels[j] = d.levels[j];
  ca.total = total;
  ca.prob = d_prob, ca.amin = d_min, ca.amax = d_max, ca.hist = d_hist;
  ca.quant = hist && Q > 0 ? d_quant : nullptr;
  ca.status = d_status;
  hipLaunchKernelGGL(k_absorption_combine, dim3((unsigned)nsel), dim3(256), 0, st, ca);
  HIP_TRY(hipGetLastError());
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out.prob_below, d_prob, (size_t)T * total)) || (rc = sg.fetch(out.absorption_min, d_min, (size_t)total)) ||
      (rc = sg.fetch(out.absorption_max, d_max, (size_t)total)) || (rc = sg.fetch(out.histogram, d_hist, (size_t)Bd * total)) ||
      (rc = sg.fetch(out.quantiles, d_quant, (size_t)(hist ? Q : 0) * total)))
    return rc;
  return plan.close(d_status, out.status, out.model_flags);
}

}  // namespace

extern "C" {

int gpdla_absorption_distribution_validate(const gpdla_absorption_distribution_request *rq, int64_t num_quasars, int64_t num_samples,
                                           int has_lls_nhi_samples) try {
  int tables = 0;
  return validate_absorption_distribution(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, &tables);
} GPDLA_NO_THROW

int gpdla_absorption_distribution_multi_validate(const gpdla_absorption_distribution_multi_request *rq, int64_t num_quasars,
                                                 int64_t num_samples, int has_lls_nhi_samples, int batch_max_dlas,
                                                 int batch_processed) try {
  int rc = validate_mixture_multi_request(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, batch_max_dlas, batch_processed != 0);
  return rc ? rc : validate_distribution(DistributionRequest(*rq));
} GPDLA_NO_THROW

int gpdla_batch_absorption_distribution(gpdla_context *c, gpdla_batch *b, const gpdla_absorption_distribution_request *rq,
                                        gpdla_absorption_distribution *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  int tables = 0;
  if (rc || (rc = check_unconditioned(b, "absorption distribution")) ||
      (rc = validate_absorption_distribution(rq, b->nq, b->S, c->d_lls_nhi != nullptr, &tables)) || (rc = check_unchanged(c, b, true)) ||
      (tables && rq->weights_source != GPDLA_SPECTRA_WEIGHTS_HOST && (rc = check_processed(b, "resident weights: "))))
    return rc;
  RefinedTable refined;  // (before the plan: the plan reads its host copy of the refine status)
  const bool use_refined = (tables & 2) && rq->weights_source == GPDLA_SPECTRA_WEIGHTS_REFINED;
  if (use_refined && (rc = refined_table(c, b, &refined))) return rc;
  MixtureSpec spec = mixture_spec(b, MixtureRequest(*rq), tables, use_refined ? &refined : nullptr);
  spec.no_scratch = true;
  MixturePlan plan(c, b, spec);
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  const gpdla_absorption_distribution_multi arrays = {out->offsets, out->prob_below, out->absorption_min, out->absorption_max,
                                                      out->histogram, out->quantiles, out->status, nullptr};
  return run_absorption_distribution(plan, DistributionRequest(*rq), arrays);
} GPDLA_NO_THROW

int gpdla_batch_absorption_distribution_multi(gpdla_context *c, gpdla_batch *b, const gpdla_absorption_distribution_multi_request *rq,
                                              gpdla_absorption_distribution_multi *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  MixtureSpec spec;
  if (rc || (rc = mixture_multi_spec(c, b, rq, "absorption distribution", &spec)) || (rc = validate_distribution(DistributionRequest(*rq))))
    return rc;
  spec.no_scratch = true;
  MixturePlan plan(c, b, spec);
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  return run_absorption_distribution(plan, DistributionRequest(*rq), *out);
} GPDLA_NO_THROW

}  // extern "C"
