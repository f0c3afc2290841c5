// host_predictive_flux.hpp -- the posterior predictive flux: per-pixel mean and variance of
// absorption times continuum over the sample tables and the models, on a resident batch.  The multi-DLA entry
// (4.25, host_mixture_multi.hpp) runs the same group loop, run_predictive_flux.
// Kernels: predictive_flux_kernels.hpp (and the contraction of marginal_continuum_kernels.hpp).
#pragma once

namespace {

int validate_predictive_flux(const gpdla_predictive_flux_request *rq, int64_t nq, int64_t S, bool has_lls, int *tables_out) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  return validate_mixture(MixtureRequest(*rq), nq, S, has_lls, tables_out);
}

// The product of an opened plan into the caller's arrays (out.offsets are written already; any other may be null)
int run_predictive_flux(MixturePlan &plan, const gpdla_predictive_flux_multi &out) {
  gpdla_context *c = plan.c;
  const gpdla_batch *b = plan.b;
  Staging &sg = plan.sg;
  hipStream_t st = plan.st;
  const int64_t nsel = plan.nsel, nsub = plan.nsub, total = plan.gs.total;
  const int chunks = plan.chunks;
  const size_t tot = plan.tot;
  int rc;

  double *d_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // mean, var, within, between, noise
  double *d_sums = nullptr;
  int32_t *d_status = nullptr, *d_list = nullptr, *d_count = nullptr;
  for (int j = 0; j < 5; ++j)
    if ((rc = sg.tmp.alloc(&d_out[j], tot))) return rc;
  if ((rc = sg.tmp.alloc(&d_status, (size_t)nsel))) return rc;
  if (plan.reach && ((rc = sg.tmp.alloc(&d_sums, (size_t)plan.ncomp * tot * 4)) || (rc = sg.tmp.alloc(&d_list, (size_t)nsub * plan.Smax)) ||
                     (rc = sg.tmp.alloc(&d_count, (size_t)nsub))))
    return rc;
  // (gpdla_context_set_timing: the kernels of this loop are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    int64_t longest = 1;
    for (int64_t s = s0; s < s0 + n; ++s) longest = std::max<int64_t>(longest, plan.gs.meta[(size_t)plan.gs.sel[(size_t)s]].n_u);
    const int64_t tiles = (longest + kPfPixTile - 1) / kPfPixTile;
    if (n * tiles > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
    if ((rc = plan.begin_group(s0, n))) return rc;
    for (int comp = 0; comp < plan.ncomp; ++comp) {
      if (!plan.reaches(comp)) continue;
      if ((rc = plan.contract(comp, s0, n))) return rc;
      hipLaunchKernelGGL(k_pf_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, plan.solve_args(comp, s0), plan.d_scratch);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(k_pf_live, dim3((unsigned)n), dim3(256), 0, st, plan.live_args(comp, s0, d_list, d_count));
      HIP_TRY(hipGetLastError());
      const PfPixelsMultiArgs pa = plan.pixels_args(comp, s0, tiles, d_list, d_count, d_sums + (size_t)comp * tot * 4);
      if (plan.boxed(comp)) hipLaunchKernelGGL(k_pf_pixels_boxed, dim3((unsigned)(n * tiles)), dim3(256), 0, st, plan.pixels_boxed_args(pa.p));
      else if (comp < 2) hipLaunchKernelGGL(k_pf_pixels, dim3((unsigned)(n * tiles)), dim3(256), 0, st, pa.p);
      else hipLaunchKernelGGL(k_pf_pixels_multi, dim3((unsigned)(n * tiles)), dim3(256), 0, st, pa);
      HIP_TRY(hipGetLastError());
    }
    PfFinishArgs fa;
    fa.meta = b->d_meta;
    fa.pix = b->d_pix;
    fa.Mi = b->d_Mi;
    fa.lam_pad = b->d_lam;
    fa.z_qsos = b->d_z;
    fa.offsets = b->d_offsets;
    fa.wavelengths = b->d_wl;
    fa.pixel_mask = b->d_mask;
    fa.min_lambda = c->cfg.min_lambda;
    fa.max_lambda = c->cfg.max_lambda;
    fa.sel = plan.gs.d_sel + s0;
    fa.out_off = plan.gs.d_off + s0;
    fa.g = plan.g;
    fa.mix = plan.mixture_args(s0);
    fa.sums = d_sums;
    fa.sums_stride = (int64_t)(tot * 4);
    fa.mean = d_out[0];
    fa.var = d_out[1];
    fa.var_within = d_out[2];
    fa.var_between = d_out[3];
    fa.noise_var = d_out[4];
    fa.status = d_status + s0;
    hipLaunchKernelGGL(k_pf_finish, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out.flux_mean, d_out[0], (size_t)total)) || (rc = sg.fetch(out.flux_var, d_out[1], (size_t)total)) ||
      (rc = sg.fetch(out.flux_var_within, d_out[2], (size_t)total)) || (rc = sg.fetch(out.flux_var_between, d_out[3], (size_t)total)) ||
      (rc = sg.fetch(out.noise_var, d_out[4], (size_t)total)))
    return rc;
  return plan.close(d_status, out.status, out.model_flags);
}

}  // namespace

extern "C" {

int gpdla_predictive_flux_validate(const gpdla_predictive_flux_request *rq, int64_t num_quasars, int64_t num_samples,
                                   int has_lls_nhi_samples) try {
  int tables = 0;
  return validate_predictive_flux(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, &tables);
} GPDLA_NO_THROW

int gpdla_batch_predictive_flux(gpdla_context *c, gpdla_batch *b, const gpdla_predictive_flux_request *rq,
                                gpdla_predictive_flux *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  int tables = 0;
  if (rc || (rc = check_unconditioned(b, "predictive flux")) ||
      (rc = validate_predictive_flux(rq, b->nq, b->S, c->d_lls_nhi != nullptr, &tables)) || (rc = check_unchanged(c, b, true)) ||
      (tables && rq->weights_source != GPDLA_SPECTRA_WEIGHTS_HOST && (rc = check_processed(b, "resident weights: "))))
    return rc;
  RefinedTable refined;  // (before the plan: the plan reads its host copy of the refine status)
  const bool use_refined = (tables & 2) && rq->weights_source == GPDLA_SPECTRA_WEIGHTS_REFINED;
  if (use_refined && (rc = refined_table(c, b, &refined))) return rc;
  MixturePlan plan(c, b, mixture_spec(b, MixtureRequest(*rq), tables, use_refined ? &refined : nullptr));
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  const gpdla_predictive_flux_multi arrays = {out->offsets, out->flux_mean, out->flux_var, out->flux_var_within, out->flux_var_between,
                                              out->noise_var, out->status, nullptr};
  return run_predictive_flux(plan, arrays);
} GPDLA_NO_THROW

}  // extern "C"
