// mixture_validate_check.hip -- the request checks of the marginal continuum and the predictive flux
// (csrc/host_grid.hpp: MixtureRequest, validate_mixture) called through the two *_validate entries from a
// program of its own, for a host sanitizer build.  The entries need no device.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Wno-inline-asm -Xarch_host -fsanitize=address,undefined \
//         tools/mixture_validate_check.hip -o mixture_validate_check && ./mixture_validate_check
//
// Exit status 0 and "ok" when every request is answered as expected (and the sanitizers stayed silent).
#include "../gp_dla_detection_amd/csrc/gpdla.hip"

namespace {

int failures = 0;

void expect(const char *what, int rc, int want_rc, const char *want_text) {
  const char *msg = rc ? gpdla_last_error() : "";
  const bool ok = rc == want_rc && (!want_text || std::strstr(msg, want_text));
  std::printf("%-58s rc %2d %s%s\n", what, rc, msg, ok ? "" : "   <-- UNEXPECTED");
  if (!ok) ++failures;
}

// the same request through both entries (the predictive flux's struct lacks sample_coefficients)
void both(const char *what, const gpdla_marginal_continuum_request *mq, int64_t nq, int64_t S, int has_lls, int want_rc,
          const char *want_text) {
  std::string label = std::string("marginal continuum: ") + what;
  expect(label.c_str(), gpdla_marginal_continuum_validate(mq, nq, S, has_lls), want_rc, want_text);
  label = std::string("predictive flux:    ") + what;
  if (!mq) {
    expect(label.c_str(), gpdla_predictive_flux_validate(nullptr, nq, S, has_lls), want_rc, want_text);
    return;
  }
  gpdla_predictive_flux_request pq;
  pq.num_selected = mq->num_selected;
  pq.selection = mq->selection;
  pq.weights_source = mq->weights_source;
  pq.sample_log_likelihoods_dla = mq->sample_log_likelihoods_dla;
  pq.sample_log_likelihoods_lls = mq->sample_log_likelihoods_lls;
  pq.model_weights = mq->model_weights;
  pq.meanflux = mq->meanflux;
  pq.capacity = mq->capacity;
  expect(label.c_str(), gpdla_predictive_flux_validate(&pq, nq, S, has_lls), want_rc, want_text);
}

}  // namespace

int main() {
  const int64_t nq = 4, S = 8;
  // heap arrays of exactly the documented sizes, so that a read past them is seen
  std::vector<int64_t> sel = {2, 0};
  std::vector<double> dla((size_t)2 * S, -1.0), lls((size_t)2 * S, -2.0), pw = {0.2, 0.3, 0.5, 1.0, 0.0, 0.0};
  gpdla_marginal_continuum_request rq = {};
  rq.num_selected = 2;
  rq.selection = sel.data();
  rq.weights_source = GPDLA_SPECTRA_WEIGHTS_HOST;
  rq.sample_log_likelihoods_dla = dla.data();
  rq.sample_log_likelihoods_lls = lls.data();
  rq.model_weights = pw.data();

  both("a good request", &rq, nq, S, 1, GPDLA_OK, nullptr);
  both("a null request", nullptr, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "null request");

  gpdla_marginal_continuum_request empty = rq;
  empty.num_selected = 0;
  empty.selection = nullptr;
  empty.model_weights = nullptr;
  empty.weights_source = GPDLA_SPECTRA_WEIGHTS_NONE;
  both("an empty selection", &empty, nq, S, 1, GPDLA_OK, nullptr);
  std::vector<int64_t> none;
  std::vector<double> no_weights;
  empty.selection = none.data();
  empty.model_weights = no_weights.data();
  both("an empty selection, empty arrays", &empty, nq, S, 1, GPDLA_OK, nullptr);

  std::vector<int64_t> outside = {0, 4};
  gpdla_marginal_continuum_request bad = rq;
  bad.selection = outside.data();
  both("selection[1] = 4 of 4 quasars", &bad, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "selection[1] = 4 outside the batch of 4 quasars");
  outside[1] = -1;
  both("selection[1] = -1", &bad, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "selection[1] = -1 outside");
  bad = rq;
  bad.selection = nullptr;
  bad.num_selected = 5;
  bad.model_weights = nullptr;
  both("no selection, num_selected = 5 of 4", &bad, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "num_selected = 5 outside [0, 4]");

  std::vector<double> zero = {0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
  bad = rq;
  bad.model_weights = zero.data();
  both("a weights row of zero sum", &bad, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "model_weights row 1 sums to 0: a row needs a positive finite sum");
  std::vector<double> nan = {0.0, 0.0, 1.0, 0.0, (double)NAN, 1.0};
  bad.model_weights = nan.data();
  both("a NaN weight", &bad, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "model_weights[1][1] = nan: weights are finite and not negative");
  std::vector<double> inf = {0.0, 0.0, 1.0, 0.0, 0.0, (double)INFINITY};
  bad.model_weights = inf.data();
  both("an infinite weight", &bad, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "weights are finite and not negative");

  both("the sub-DLA table without lls_nhi_samples", &rq, nq, S, 0, GPDLA_ERR_INVALID_ARGUMENT, "lls_nhi_samples");
  both("no samples", &rq, nq, 0, 1, GPDLA_ERR_INVALID_ARGUMENT, "no samples");
  bad = rq;
  bad.capacity = -1;
  both("negative capacity", &bad, nq, S, 1, GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");

  // the marginal continuum's own check, after the shared ones
  bad = rq;
  bad.sample_coefficients = 1;
  expect("marginal continuum: sample_coefficients, both tables", gpdla_marginal_continuum_validate(&bad, nq, S, 1),
         GPDLA_ERR_INVALID_ARGUMENT, "both tables");
  bad.model_weights = nullptr;
  expect("marginal continuum: sample_coefficients, one table", gpdla_marginal_continuum_validate(&bad, nq, S, 1), GPDLA_OK, nullptr);

  std::printf(failures ? "%d UNEXPECTED\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
