"""GPU check that the module-level drivers of the grid products (gp.model_spectra, gp.marginal_continuum, gp.predictive_flux)
do not depend on the batching on the paths tests/test_gpu_marginal_continuum.py and tests/test_gpu_predictive_flux.py do not
cover: ``multi_models`` and ``refined=`` of all three.  Five quasars of 5, 31, 33, 17 and 64 grid pixels (S = 16, k = 20) in
blocks of two -- one upload, then reloads; the selection of all five ends on a short block -- against the same call with all
of them in one batch: every returned array bit for bit, with its key order, dtype and shape."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd.parameters import Parameters

import marginal_continuum_cases as MC

pytestmark = pytest.mark.gpu

REFINED = dict(levels=2, points=16)


@pytest.fixture(scope="module")
def case():
    """The batching case swept once as the multi-DLA run it is, and once with the single-DLA parameters of the same setup:
    the refined forms take their priors from that run's results."""
    model, samples, spectra, p, log_priors = MC.batching_case()
    n = len(spectra)
    single_p = Parameters(num_lines=p.num_lines)
    return dict(model=model, samples=samples, spectra=spectra, multi_p=p, single_p=single_p,
                multi=gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, log_priors, params=p),
                single=gp.process_qsos(model, samples, spectra, log_priors=(np.full(n, np.log(0.9)), np.full(n, np.log(0.1))),
                                       params=single_p))


def _multi(driver, **more):
    return lambda c, **kw: driver(c["model"], c["samples"], c["spectra"], c["multi"], params=c["multi_p"], multi_models=True,
                                  **more, **kw)


def _refined(driver, **more):
    return lambda c, **kw: driver(c["model"], c["samples"], c["spectra"], c["single"], params=c["single_p"], refined=REFINED,
                                  **more, **kw)


MIXED = dict(components=("null", "dla"), model_weights="posteriors")
# path -> (the call, keys the result must hold)
PATHS = {
    "marginal_continuum_multi": (_multi(gp.marginal_continuum), ("model_flags", "continuum_mean", "coef_cov_between")),
    "predictive_flux_multi": (_multi(gp.predictive_flux, residuals=True), ("model_flags", "flux_mean", "residual", "num_kept")),
    "model_spectra_multi": (_multi(gp.model_spectra), ("model_flags", "map_absorption", "mean_absorption_models",
                                                        "expected_absorption")),
    "marginal_continuum_refined": (_refined(gp.marginal_continuum, **MIXED), ("boxes", "refine_status", "continuum_mean")),
    "predictive_flux_refined": (_refined(gp.predictive_flux, residuals=True, **MIXED), ("boxes", "flux_mean", "residual", "chi2")),
    "model_spectra_refined": (_refined(gp.model_spectra), ("boxes", "refine_status", "mean_absorption", "model_flux")),
}


@pytest.mark.parametrize("which", list(MC.BATCHING_SELECTIONS))
@pytest.mark.parametrize("path", list(PATHS))
def test_results_do_not_depend_on_the_batching(case, path, which):
    call, keys = PATHS[path]
    sel = MC.BATCHING_SELECTIONS[which]
    blocks = call(case, selection=sel, max_quasars_per_batch=2)
    whole = call(case, selection=sel, max_quasars_per_batch=5)
    assert set(keys) <= set(whole) and list(whole)[:3] == ["selection", "offsets", "status"]
    np.testing.assert_array_equal(whole["selection"], sel)
    np.testing.assert_array_equal(np.diff(whole["offsets"]), [MC.BATCHING_NUS[q] for q in sel])
    MC.assert_same_results(blocks, whole)
