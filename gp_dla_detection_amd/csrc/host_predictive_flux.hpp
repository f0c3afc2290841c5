// host_predictive_flux.hpp -- the posterior predictive flux: per-pixel mean and variance of
// absorption times continuum over the sample tables and the models, on a resident batch.
// Kernels: predictive_flux_kernels.hpp (and k_mc_contract of marginal_continuum_kernels.hpp).
#pragma once

namespace {

int validate_predictive_flux(const gpdla_predictive_flux_request *rq, int64_t nq, int64_t S, bool has_lls, int *tables_out) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  return validate_mixture(MixtureRequest(*rq), nq, S, has_lls, tables_out);
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
      (rc = validate_predictive_flux(rq, b->nq, b->S, c->d_lls_nhi != nullptr, &tables)))
    return rc;
  MixturePlan plan(c, b, tables);
  if ((rc = plan.open(MixtureRequest(*rq), out->offsets)) || plan.nsel == 0) return rc;
  Staging &sg = plan.sg;
  hipStream_t st = plan.st;
  const int64_t nsel = plan.nsel, S = plan.S, nsub = plan.nsub, total = plan.gs.total;
  const int chunks = plan.chunks;
  const size_t tot = plan.tot;
  const int64_t *d_sel = plan.gs.d_sel, *d_off = plan.gs.d_off;

  double *d_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // mean, var, within, between, noise
  double *d_sums[2] = {nullptr, nullptr};
  int32_t *d_status = nullptr, *d_list = nullptr, *d_count = nullptr;
  for (int j = 0; j < 5; ++j)
    if ((rc = sg.tmp.alloc(&d_out[j], tot))) return rc;
  if ((rc = sg.tmp.alloc(&d_status, (size_t)nsel))) return rc;
  for (int comp = 0; comp < 2; ++comp)
    if (plan.reaches(comp) && (rc = sg.tmp.alloc(&d_sums[comp], tot * 4))) return rc;
  if (tables && ((rc = sg.tmp.alloc(&d_list, (size_t)nsub * S)) || (rc = sg.tmp.alloc(&d_count, (size_t)nsub)))) return rc;
  const ContinuumModelArgs g = continuum_model_args(c, rq->meanflux != 0);
  // (gpdla_context_set_timing: the kernels of this call are what gpdla_context_last_sweep_ms reports)
  if ((rc = begin_timing(c, st))) return rc;
  for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {
    const int64_t n = std::min(nsub, nsel - s0);
    int64_t longest = 1;
    for (int64_t s = s0; s < s0 + n; ++s) longest = std::max<int64_t>(longest, plan.gs.meta[(size_t)plan.gs.sel[(size_t)s]].n_u);
    const int64_t tiles = (longest + kPfPixTile - 1) / kPfPixTile;
    if (n * tiles > 2147483647LL) return fail(GPDLA_ERR_UNSUPPORTED, "selection too large for one launch");
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
      sa.k = plan.k;
      sa.s0 = s0;
      sa.chunks = chunks;
      sa.scratch = plan.d_scratch;
      sa.part = nullptr;
      sa.notpd = plan.d_notpd[comp];
      sa.sample_coef = nullptr;
      hipLaunchKernelGGL(k_pf_solve, dim3((unsigned)(n * chunks)), dim3(256), 0, st, sa, plan.d_scratch);
      HIP_TRY(hipGetLastError());
      PfLiveArgs la;
      la.meta = b->d_meta;
      la.perm = c->d_perm;
      la.sel = d_sel;
      la.w = plan.d_w[comp];
      la.pm = plan.d_pm[comp];
      la.S = S;
      la.s0 = s0;
      la.list = d_list;
      la.count = d_count;
      hipLaunchKernelGGL(k_pf_live, dim3((unsigned)n), dim3(256), 0, st, la);
      HIP_TRY(hipGetLastError());
      PfPixelsArgs pa;
      pa.meta = b->d_meta;
      pa.pix = b->d_pix;
      pa.lam_pad = b->d_lam;
      pa.z_qsos = b->d_z;
      pa.offset_samples = c->d_offset;
      pa.nhi = plan.nhi(comp);
      pa.perm = c->d_perm;
      pa.sel = d_sel;
      pa.out_off = d_off;
      pa.w = plan.d_w[comp];
      pa.pm = plan.d_pm[comp];
      pa.g = g;
      pa.S = S;
      pa.num_lines = c->cfg.num_lines;
      pa.s0 = s0;
      pa.tiles = (int32_t)tiles;
      pa.scratch = plan.d_scratch;
      pa.list = d_list;
      pa.count = d_count;
      pa.sums = d_sums[comp];
      hipLaunchKernelGGL(k_pf_pixels, dim3((unsigned)(n * tiles)), dim3(256), 0, st, pa);
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
    fa.sel = d_sel;
    fa.out_off = d_off;
    fa.g = g;
    fa.pw = plan.d_pw;
    for (int comp = 0; comp < 2; ++comp) {
      fa.flag[comp] = plan.d_flag[comp];
      fa.sums[comp] = d_sums[comp];
      fa.notpd[comp] = plan.d_notpd[comp];
    }
    fa.s0 = s0;
    fa.chunks = chunks;
    fa.mean = d_out[0];
    fa.var = d_out[1];
    fa.var_within = d_out[2];
    fa.var_between = d_out[3];
    fa.noise_var = d_out[4];
    fa.status = d_status;
    hipLaunchKernelGGL(k_pf_finish, dim3((unsigned)n), dim3(256), 0, st, fa);
    HIP_TRY(hipGetLastError());
  }
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out->flux_mean, d_out[0], (size_t)total)) || (rc = sg.fetch(out->flux_var, d_out[1], (size_t)total)) ||
      (rc = sg.fetch(out->flux_var_within, d_out[2], (size_t)total)) || (rc = sg.fetch(out->flux_var_between, d_out[3], (size_t)total)) ||
      (rc = sg.fetch(out->noise_var, d_out[4], (size_t)total)) || (rc = sg.fetch(plan.status.data(), d_status, (size_t)nsel)))
    return rc;
  HIP_TRY(hipStreamSynchronize(st));
  if (out->status) std::memcpy(out->status, plan.status.data(), (size_t)nsel * sizeof(int32_t));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
