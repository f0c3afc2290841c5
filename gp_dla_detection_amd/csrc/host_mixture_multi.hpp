// host_mixture_multi.hpp -- the marginal continuum and the posterior predictive flux over all models of a multi-DLA
// run: the mixtures of host_marginal_continuum.hpp and host_predictive_flux.hpp over the components
// (null, sub-DLA table, DLA(1), .., DLA(max_dlas)), from the resident tables of a processed multi-DLA batch or from
// host tables.  Here: the request checks and the two entries; the plan is MixturePlan (host_grid.hpp) with 1 + max_dlas
// sampled components, the group loops are run_marginal_continuum and run_predictive_flux.
#pragma once

namespace {

// What gpdla_marginal_continuum_multi_request and gpdla_predictive_flux_multi_request share (the same fields)
struct MixtureMultiRequest {
  int64_t num_selected;
  const int64_t *selection;
  int32_t max_dlas, tables_source;
  const double *sample_log_likelihoods_dla;
  const uint32_t *base_sample_inds;
  const double *sample_log_likelihoods_lls, *model_weights;
  int32_t meanflux;
  int64_t capacity;
  template <typename Request>
  explicit MixtureMultiRequest(const Request &q)
      : num_selected(q.num_selected), selection(q.selection), max_dlas(q.max_dlas), tables_source(q.tables_source),
        sample_log_likelihoods_dla(q.sample_log_likelihoods_dla), base_sample_inds(q.base_sample_inds),
        sample_log_likelihoods_lls(q.sample_log_likelihoods_lls), model_weights(q.model_weights), meanflux(q.meanflux),
        capacity(q.capacity) {}
};

// reach_out: the sampled components some row weighs, bit 0 the sub-DLA table, bit n model DLA(n); without
// model_weights (the resident model_posteriors, known only on the device) every one
int validate_mixture_multi(const MixtureMultiRequest &rq, int64_t nq, int64_t S, bool has_lls, int batch_max_dlas,
                           bool batch_processed, unsigned *reach_out) {
  int rc = check_selection(nq, rq.selection, rq.num_selected);
  if (rc) return rc;
  const int md = rq.max_dlas;
  if (md < 1 || md > GPDLA_POSTERIOR_MAX_MODELS)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "max_dlas = %d outside [1, %d]", md, GPDLA_POSTERIOR_MAX_MODELS);
  if (S < 1 || S > (1LL << 30)) return fail(GPDLA_ERR_INVALID_ARGUMENT, "need 1 <= num_samples <= 2^30");
  const int ncols = 2 + md;
  unsigned reach = 0;
  if (!rq.model_weights) {
    reach = rq.num_selected > 0 ? (2u << md) - 1u : 0u;
  } else {
    for (int64_t s = 0; s < rq.num_selected; ++s) {
      const double *p = rq.model_weights + (size_t)ncols * (size_t)s;
      bool undefined = false;
      for (int mm = 0; mm < ncols; ++mm) undefined = undefined || p[mm] != p[mm];
      if (undefined) continue;  // (NaN rows and GPDLA_SPECTRA_AVERAGE_UNDEFINED for that quasar, not a refusal)
      double sum = 0.0;
      for (int mm = 0; mm < ncols; ++mm) {
        if (!(p[mm] >= 0.0) || !std::isfinite(p[mm]))
          return fail(GPDLA_ERR_INVALID_ARGUMENT, "model_weights[%lld][%d] = %g: weights are not negative and not infinite", (long long)s, mm, p[mm]);
        sum += p[mm];
      }
      if (!(sum > 0.0) || !std::isfinite(sum))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "model_weights row %lld sums to %g: a row needs a positive finite sum", (long long)s, sum);
      for (int comp = 0; comp <= md; ++comp)
        if (p[1 + comp] > 0.0) reach |= 1u << comp;
    }
  }
  if (rq.tables_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT) {
    if (!batch_max_dlas) return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: not a multi-DLA batch (upload it with log_priors_lls)");
    if (batch_max_dlas != md)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: the batch holds max_dlas = %d, the request says %d", batch_max_dlas, md);
    if (!batch_processed) return fail(GPDLA_ERR_INVALID_ARGUMENT, "resident tables: the batch has not been processed (gpdla_batch_process_multi)");
  } else if (rq.tables_source == GPDLA_SPECTRA_WEIGHTS_HOST) {
    if (!rq.model_weights) return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables need model_weights (the resident model_posteriors go with the resident tables)");
    if ((reach & ~1u) && !rq.sample_log_likelihoods_dla)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables: sample_log_likelihoods_dla is null");
    if ((reach & 1u) && !rq.sample_log_likelihoods_lls)
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables: sample_log_likelihoods_lls is null");
    if ((reach >> 2) && !rq.base_sample_inds) return fail(GPDLA_ERR_INVALID_ARGUMENT, "host tables: base_sample_inds is null");
    if (rq.base_sample_inds) {
      const size_t nbase = (size_t)rq.num_selected * (size_t)(md - 1) * (size_t)S;
      for (size_t e = 0; e < nbase; ++e)
        if ((int64_t)rq.base_sample_inds[e] > S)
          return fail(GPDLA_ERR_INVALID_ARGUMENT, "base_sample_inds entry %zu = %u exceeds num_samples = %lld", e,
                      rq.base_sample_inds[e], (long long)S);
    }
  } else {
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "tables_source = %d: GPDLA_SPECTRA_WEIGHTS_RESIDENT or _HOST", rq.tables_source);
  }
  if ((reach & 1u) && !has_lls) return fail(GPDLA_ERR_INVALID_ARGUMENT, "the sub-DLA component needs lls_nhi_samples in the context's samples");
  if (rq.capacity < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");
  *reach_out = reach;
  return GPDLA_OK;
}

template <typename Request>
int validate_mixture_multi_request(const Request *rq, int64_t nq, int64_t S, bool has_lls, int batch_max_dlas, bool batch_processed) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  unsigned reach = 0;
  return validate_mixture_multi(MixtureMultiRequest(*rq), nq, S, has_lls, batch_max_dlas, batch_processed, &reach);
}

// The refusals of a multi entry, then its plan's description: the tables of the processed multi-DLA batch with its
// model_posteriors where the request gives no weights, or the caller's
template <typename Request>
int mixture_multi_spec(const gpdla_context *c, const gpdla_batch *b, const Request *rq, const char *what, MixtureSpec *spec) {
  int rc;
  if ((rc = check_unconditioned(b, what)) ||
      (rc = validate_mixture_multi_request(rq, b->nq, b->S, c->d_lls_nhi != nullptr, b->md, b->md && b->mb && b->mb->processed)) ||
      (rc = check_unchanged(c, b, true)))
    return rc;
  MixtureSpec sp = {};
  sp.num_selected = rq->num_selected;
  sp.selection = rq->selection;
  sp.md = rq->max_dlas;
  sp.resident = rq->tables_source == GPDLA_SPECTRA_WEIGHTS_RESIDENT;
  sp.lls = sp.resident ? b->mb->sll_lls : rq->sample_log_likelihoods_lls;
  sp.dla = sp.resident ? b->mb->sll_dla : rq->sample_log_likelihoods_dla;
  sp.base = sp.resident ? b->mb->base : rq->base_sample_inds;
  sp.lls_stride = b->S;
  sp.dla_stride = (int64_t)sp.md * b->S;
  sp.model_weights = rq->model_weights;
  sp.posteriors = sp.resident ? b->mb->post : nullptr;
  sp.meanflux = rq->meanflux != 0;
  sp.capacity = rq->capacity;
  *spec = sp;
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_marginal_continuum_multi_validate(const gpdla_marginal_continuum_multi_request *rq, int64_t num_quasars, int64_t num_samples,
                                            int has_lls_nhi_samples, int batch_max_dlas, int batch_processed) try {
  return validate_mixture_multi_request(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, batch_max_dlas, batch_processed != 0);
} GPDLA_NO_THROW

int gpdla_predictive_flux_multi_validate(const gpdla_predictive_flux_multi_request *rq, int64_t num_quasars, int64_t num_samples,
                                         int has_lls_nhi_samples, int batch_max_dlas, int batch_processed) try {
  return validate_mixture_multi_request(rq, num_quasars, num_samples, has_lls_nhi_samples != 0, batch_max_dlas, batch_processed != 0);
} GPDLA_NO_THROW

int gpdla_batch_marginal_continuum_multi(gpdla_context *c, gpdla_batch *b, const gpdla_marginal_continuum_multi_request *rq,
                                         gpdla_marginal_continuum_multi *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  MixtureSpec spec;
  if (rc || (rc = mixture_multi_spec(c, b, rq, "marginal continuum", &spec))) return rc;
  MixturePlan plan(c, b, spec);
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  return run_marginal_continuum(plan, *out, nullptr);
} GPDLA_NO_THROW

int gpdla_batch_predictive_flux_multi(gpdla_context *c, gpdla_batch *b, const gpdla_predictive_flux_multi_request *rq,
                                      gpdla_predictive_flux_multi *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->offsets);
  MixtureSpec spec;
  if (rc || (rc = mixture_multi_spec(c, b, rq, "predictive flux", &spec))) return rc;
  MixturePlan plan(c, b, spec);
  if ((rc = plan.open(out->offsets)) || plan.nsel == 0) return rc;
  return run_predictive_flux(plan, *out);
} GPDLA_NO_THROW

}  // extern "C"
