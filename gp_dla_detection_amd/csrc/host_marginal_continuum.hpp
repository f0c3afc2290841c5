// host_marginal_continuum.hpp -- the marginal continuum: the GP posterior mean and
// variance of the low-rank continuum over the sample tables and the models, on a resident batch.
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
      (rc = validate_marginal_continuum(rq, b->nq, b->S, c->d_lls_nhi != nullptr, &tables)))
    return rc;
  MixturePlan plan(c, b, tables);
  if ((rc = plan.open(MixtureRequest(*rq), out->offsets)) || plan.nsel == 0) return rc;
  Staging &sg = plan.sg;
  hipStream_t st = plan.st;
  const int64_t nsel = plan.nsel, S = plan.S, nsub = plan.nsub, total = plan.gs.total;
  const int k = plan.k, nb = plan.nb, plen = k + 2 * nb, chunks = plan.chunks;
  const size_t tot = plan.tot;
  const int64_t *d_sel = plan.gs.d_sel;

  double *d_mean = nullptr, *d_var = nullptr, *d_btw = nullptr, *d_c = nullptr, *d_W = nullptr, *d_V = nullptr, *d_sc = nullptr;
  double *d_part[2] = {nullptr, nullptr};
  int32_t *d_status = nullptr;
  if ((rc = sg.tmp.alloc(&d_mean, tot)) || (rc = sg.tmp.alloc(&d_var, tot)) || (rc = sg.tmp.alloc(&d_btw, tot)) ||
      (rc = sg.tmp.alloc(&d_c, (size_t)nsel * k)) || (rc = sg.tmp.alloc(&d_W, (size_t)nsel * nb)) ||
      (rc = sg.tmp.alloc(&d_V, (size_t)nsel * nb)) || (rc = sg.tmp.alloc(&d_status, (size_t)nsel)))
    return rc;
  const bool want_sc = rq->sample_coefficients && out->sample_coefficients;
  if (want_sc && (rc = sg.tmp.alloc(&d_sc, (size_t)nsel * S * k))) return rc;
  for (int comp = 0; comp < 2; ++comp)
    if (plan.reaches(comp) && (rc = sg.tmp.alloc(&d_part[comp], (size_t)nsub * chunks * plen))) return rc;
  // (gpdla_context_set_timing: the three kernels of this call are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    for (int comp = 0; comp < 2; ++comp) {
      if (!plan.reaches(comp)) continue;
      if ((rc = plan.contract(comp, s0, n))) return rc;
      McSolveArgs sa;
      sa.meta = b->d_meta;
      sa.perm = c->d_perm;
      sa.sel = d_sel;
      sa.w = plan.d_w[comp];
      sa.pm = plan.d_pm[comp];
      sa.S = S;
      sa.k = k;
      sa.s0 = s0;
      sa.chunks = chunks;
      sa.scratch = plan.d_scratch;
      sa.part = d_part[comp];
      sa.notpd = plan.d_notpd[comp];
      sa.sample_coef = want_sc ? d_sc : nullptr;
      hipLaunchKernelGGL(k_mc_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, sa);
      HIP_TRY(hipGetLastError());
    }
    McFinishArgs fa;
    fa.meta = b->d_meta;
    fa.pix = b->d_pix;
    fa.Mi = b->d_Mi;
    fa.lam_pad = b->d_lam;
    fa.z_qsos = b->d_z;
    fa.sel = d_sel;
    fa.out_off = plan.gs.d_off;
    fa.g = continuum_model_args(c, rq->meanflux != 0);
    fa.pw = plan.d_pw;
    for (int comp = 0; comp < 2; ++comp) {
      fa.flag[comp] = plan.d_flag[comp];
      fa.part[comp] = d_part[comp];
      fa.notpd[comp] = plan.d_notpd[comp];
    }
    fa.s0 = s0;
    fa.chunks = chunks;
    fa.mean = d_mean;
    fa.var = d_var;
    fa.var_between = d_btw;
    fa.coef_mean = d_c;
    fa.cov_within = d_W;
    fa.cov_between = d_V;
    fa.status = d_status;
    hipLaunchKernelGGL(k_mc_finish, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out->continuum_mean, d_mean, (size_t)total)) || (rc = sg.fetch(out->continuum_var, d_var, (size_t)total)) ||
      (rc = sg.fetch(out->continuum_var_between, d_btw, (size_t)total)) || (rc = sg.fetch(out->coef_mean, d_c, (size_t)nsel * k)) ||
      (rc = sg.fetch(out->coef_cov_within, d_W, (size_t)nsel * nb)) || (rc = sg.fetch(out->coef_cov_between, d_V, (size_t)nsel * nb)) ||
      (rc = sg.fetch(plan.status.data(), d_status, (size_t)nsel)))
    return rc;
  if (want_sc && (rc = sg.fetch(out->sample_coefficients, d_sc, (size_t)nsel * S * k))) return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (out->status) std::memcpy(out->status, plan.status.data(), (size_t)nsel * sizeof(int32_t));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
