// host_marginal_continuum.hpp -- the marginal continuum: the GP posterior mean and
// variance of the low-rank continuum over the sample tables and the models, on a resident batch.  The multi-DLA
// entry (4.25, host_mixture_multi.hpp) runs the same group loop, run_marginal_continuum.
// Kernels: marginal_continuum_kernels.hpp.
#pragma once

namespace {

// the mixture's checks, then the one of this entry alone
int validate_marginal_continuum(const gpdla_marginal_continuum_request *rq, int64_t nq, int64_t S, bool has_lls, int *tables_out) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  int rc = validate_mixture(MixtureRequest(*rq), nq, S, has_lls, tables_out);
  if (rc) return rc;
  if (rq->sample_coefficients && *tables_out != 1 && *tables_out != 2)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "sample_coefficients are those of ONE sampled component: the model weights reach %s",
                *tables_out == 3 ? "both tables" : "none");
  return GPDLA_OK;
}

// The product of an opened plan into the caller's arrays (out.offsets are written already; any other may be null).
// sample_coefficients: [nsel][S][k] of the ONE sampled component the model weights reach, or nullptr.  S is decided by the
// REQUEST, as the caller sized its array: S' where the plan runs the DLA component on a refined table (the validated request
// then reaches the DLA table alone), the batch's S otherwise -- never by which rows survive the normalisation.
int run_marginal_continuum(MixturePlan &plan, const gpdla_marginal_continuum_multi &out, double *sample_coefficients) {
  gpdla_context *c = plan.c;
  const gpdla_batch *b = plan.b;
  Staging &sg = plan.sg;
  hipStream_t st = plan.st;
  const int64_t nsel = plan.nsel, S = sample_coefficients && plan.sp.refined ? plan.sp.refined->Sr : plan.S, nsub = plan.nsub, total = plan.gs.total;
  const int k = plan.k, nb = plan.nb, plen = k + 2 * nb, chunks = plan.chunks;
  const size_t tot = plan.tot, part_stride = (size_t)nsub * chunks * plen;
  int rc;

  double *d_mean = nullptr, *d_var = nullptr, *d_btw = nullptr, *d_c = nullptr, *d_W = nullptr, *d_V = nullptr, *d_part = nullptr,
         *d_sc = nullptr;
  int32_t *d_status = nullptr;
  if ((rc = sg.tmp.alloc(&d_mean, tot)) || (rc = sg.tmp.alloc(&d_var, tot)) || (rc = sg.tmp.alloc(&d_btw, tot)) ||
      (rc = sg.tmp.alloc(&d_c, (size_t)nsel * k)) || (rc = sg.tmp.alloc(&d_W, (size_t)nsel * nb)) ||
      (rc = sg.tmp.alloc(&d_V, (size_t)nsel * nb)) || (rc = sg.tmp.alloc(&d_status, (size_t)nsel)) ||
      (plan.reach && (rc = sg.tmp.alloc(&d_part, (size_t)plan.ncomp * part_stride))))
    return rc;
  if (sample_coefficients && (rc = sg.tmp.alloc(&d_sc, (size_t)nsel * S * k))) return rc;
  // (gpdla_context_set_timing: the kernels of this loop are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    if ((rc = plan.begin_group(s0, n))) return rc;
    for (int comp = 0; comp < plan.ncomp; ++comp) {
      if (!plan.reaches(comp)) continue;
      if ((rc = plan.contract(comp, s0, n))) return rc;
      McSolveArgs sa = plan.solve_args(comp, s0);
      sa.part = d_part + (size_t)comp * part_stride;
      sa.sample_coef = d_sc ? d_sc + (size_t)s0 * S * k : nullptr;
      hipLaunchKernelGGL(k_mc_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, sa);
      HIP_TRY(hipGetLastError());
    }
    McFinishArgs fa;
    fa.meta = b->d_meta;
    fa.pix = b->d_pix;
    fa.Mi = b->d_Mi;
    fa.lam_pad = b->d_lam;
    fa.z_qsos = b->d_z;
    fa.sel = plan.gs.d_sel + s0;
    fa.out_off = plan.gs.d_off + s0;
    fa.g = plan.g;
    fa.mix = plan.mixture_args(s0);
    fa.part = d_part;
    fa.part_stride = (int64_t)part_stride;
    fa.mean = d_mean;
    fa.var = d_var;
    fa.var_between = d_btw;
    fa.coef_mean = d_c + (size_t)s0 * k;
    fa.cov_within = d_W + (size_t)s0 * nb;
    fa.cov_between = d_V + (size_t)s0 * nb;
    fa.status = d_status + s0;
    hipLaunchKernelGGL(k_mc_finish, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out.continuum_mean, d_mean, (size_t)total)) || (rc = sg.fetch(out.continuum_var, d_var, (size_t)total)) ||
      (rc = sg.fetch(out.continuum_var_between, d_btw, (size_t)total)) || (rc = sg.fetch(out.coef_mean, d_c, (size_t)nsel * k)) ||
      (rc = sg.fetch(out.coef_cov_within, d_W, (size_t)nsel * nb)) || (rc = sg.fetch(out.coef_cov_between, d_V, (size_t)nsel * nb)) ||
      (rc = sg.fetch(sample_coefficients, d_sc, (size_t)nsel * S * k)))
    return rc;
  return plan.close(d_status, out.status, out.model_flags);
}

}  // namespace

extern "C" {

int gpdla_marginal_continuum_validate(const gpdla_marginal_continuum_request *rq, int64_t num_quasars, int64_t num_samples,
                                      int has_lls_nhi_samples) try {
  int tables = 0;
  return validate_marginal_continuum(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, &tables);
} GPDLA_NO_THROW

int gpdla_batch_marginal_continuum(gpdla_context *c, gpdla_batch *b, const gpdla_marginal_continuum_request *rq,
                                   gpdla_marginal_continuum *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  int tables = 0;
  if (rc || (rc = check_unconditioned(b, "marginal continuum")) ||
      (rc = validate_marginal_continuum(rq, b->nq, b->S, c->d_lls_nhi != nullptr, &tables)) || (rc = check_unchanged(c, b, true)) ||
      (tables && rq->weights_source != GPDLA_SPECTRA_WEIGHTS_HOST && (rc = check_processed(b, "resident weights: "))))
    return rc;
  RefinedTable refined;  // (before the plan: the plan reads its host copy of the refine status)
  const bool use_refined = (tables & 2) && rq->weights_source == GPDLA_SPECTRA_WEIGHTS_REFINED;
  if (use_refined && (rc = refined_table(c, b, &refined))) return rc;
  MixturePlan plan(c, b, mixture_spec(b, MixtureRequest(*rq), tables, use_refined ? &refined : nullptr));
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  const gpdla_marginal_continuum_multi arrays = {out->offsets, out->continuum_mean, out->continuum_var, out->continuum_var_between,
                                                 out->coef_mean, out->coef_cov_within, out->coef_cov_between, out->status, nullptr};
  return run_marginal_continuum(plan, arrays, rq->sample_coefficients ? out->sample_coefficients : nullptr);
} GPDLA_NO_THROW

}  // extern "C"
