"""CPU checks of the per-pixel products on refined tables: the constants of the C boundary, the three
validate entries (which need no GPU) and the glue of tests/refined_products_cases.py that turns boxes into inputs of the
existing restatements, on a tiny hand-made case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gp_dla_detection_amd import _lib

import model_spectra_restatement as R
import refined_products_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp, _i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_constants_in_the_header_and_the_bindings(lib):
    header = open(os.path.join(ROOT, "include", "gpdla.h")).read()
    assert re.search(r"#define GPDLA_SPECTRA_WEIGHTS_REFINED 3\b", header)
    assert re.search(r"#define GPDLA_SPECTRA_NOT_REFINED 16\b", header)
    assert _lib.SPECTRA_WEIGHTS_REFINED == 3 and _lib.SPECTRA_NOT_REFINED == 16
    # a bit no product's status uses: 1, 3 (sweep), 4 (not positive definite), 8 (average undefined)
    assert all(_lib.SPECTRA_NOT_REFINED & s == 0 for s in (1, 3, 4, _lib.SPECTRA_AVERAGE_UNDEFINED))
    assert "#define GPDLA_ABI_VERSION 6" in header and lib.gpdla_abi_version() == 6


def _mixture_request(cls, source, model_weights=None, nsel=2):
    rq = cls()
    rq.num_selected = nsel
    rq.weights_source = source
    keep = []
    if model_weights is not None:
        pw = np.ascontiguousarray(model_weights, dtype=np.float64)
        keep.append(pw)
        rq.model_weights = pw.ctypes.data_as(_dp)
    rq.capacity = 1000
    return rq, keep


@pytest.mark.parametrize("cls, entry", [(_lib.MarginalContinuumRequest, "gpdla_marginal_continuum_validate"),
                                        (_lib.PredictiveFluxRequest, "gpdla_predictive_flux_validate")])
def test_mixture_validate_accepts_the_refined_source_without_a_host_table(lib, cls, entry):
    validate = getattr(lib, entry)
    for pw in (None, [[0.2, 0.0, 0.8], [0.0, 0.0, 1.0]], [[0.2, 0.3, 0.5], [1.0, 0.0, 0.0]]):
        rq, keep = _mixture_request(cls, _lib.SPECTRA_WEIGHTS_REFINED, pw)
        assert validate(C.byref(rq), 4, 8, 1) == 0, (pw, lib.gpdla_last_error())
    # what was refused stays refused: no source at all, an unknown one, the sub-DLA table without LLS samples
    rq, keep = _mixture_request(cls, _lib.SPECTRA_WEIGHTS_NONE)
    assert validate(C.byref(rq), 4, 8, 1) == -1
    rq, keep = _mixture_request(cls, 4)
    assert validate(C.byref(rq), 4, 8, 1) == -1
    rq, keep = _mixture_request(cls, _lib.SPECTRA_WEIGHTS_REFINED, [[0.2, 0.3, 0.5], [1.0, 0.0, 0.0]])
    assert validate(C.byref(rq), 4, 8, 0) == -1 and b"lls_nhi_samples" in lib.gpdla_last_error()
    del keep


def test_marginal_continuum_validate_sample_coefficients_with_the_refined_source(lib):
    rq, keep = _mixture_request(_lib.MarginalContinuumRequest, _lib.SPECTRA_WEIGHTS_REFINED)
    rq.sample_coefficients = 1
    assert lib.gpdla_marginal_continuum_validate(C.byref(rq), 4, 8, 1) == 0
    rq, keep = _mixture_request(_lib.MarginalContinuumRequest, _lib.SPECTRA_WEIGHTS_REFINED, [[0.2, 0.3, 0.5], [0.0, 0.5, 0.5]])
    rq.sample_coefficients = 1
    assert lib.gpdla_marginal_continuum_validate(C.byref(rq), 4, 8, 1) == -1


def test_model_spectra_validate_accepts_refined_and_refuses_it_with_sub_dla(lib):
    def request(source, sub_dla=0):
        rq = _lib.ModelSpectraRequest()
        rq.num_selected = 2
        rq.weights_source = source
        rq.sub_dla = sub_dla
        rq.products = _lib.SPECTRA_MOMENTS
        rq.capacity = 1000
        return rq
    v = lib.gpdla_model_spectra_validate
    assert v(C.byref(request(_lib.SPECTRA_WEIGHTS_REFINED)), 4, 8, 1) == 0, lib.gpdla_last_error()
    assert v(C.byref(request(_lib.SPECTRA_WEIGHTS_REFINED)), 4, 8, 0) == 0     # (no LLS samples needed)
    assert v(C.byref(request(_lib.SPECTRA_WEIGHTS_REFINED, 1)), 4, 8, 1) == -1 and b"sub_dla" in lib.gpdla_last_error()
    assert v(C.byref(request(_lib.SPECTRA_WEIGHTS_RESIDENT, 1)), 4, 8, 1) == 0  # (as before)
    assert v(C.byref(request(_lib.SPECTRA_WEIGHTS_NONE)), 4, 8, 1) == -1
    assert v(C.byref(request(4)), 4, 8, 1) == -1


def test_the_python_layer_names_the_source():
    import inspect

    from gp_dla_detection_amd import api
    for method in (api.Batch.model_spectra, api.Batch.marginal_continuum, api.Batch.predictive_flux):
        doc = " ".join(inspect.getdoc(method).split())
        assert '"refined"' in doc and "outside the last box" in doc, method.__name__


def test_sample_coefficient_rows_follow_the_library_rule():
    """Batch.marginal_continuum sizes ``sample_coefficients [nsel, rows, k]`` by the rule the library writes by: S' only
    where the refined source meets a model weight on the DLA column (the request then runs the DLA component on the refined
    table); a refined source whose DLA column is 0 in every row is evaluated on the first pass's tables, S rows long."""
    from gp_dla_detection_amd.api import Batch
    rows = Batch._coefficient_samples
    S, Sr = 200, 63
    dla, lls, both = [[0, 0, 1.0], [0.5, 0, 0.5]], [[0, 1.0, 0], [0.5, 0.5, 0]], [[0, 1.0, 0], [0, 0, 1e-300]]
    assert rows(_lib.SPECTRA_WEIGHTS_REFINED, dla, S, Sr) == Sr
    assert rows(_lib.SPECTRA_WEIGHTS_REFINED, lls, S, Sr) == S        # components ("sub_dla", "dla") with the DLA column at 0
    assert rows(_lib.SPECTRA_WEIGHTS_REFINED, both, S, Sr) == Sr      # any positive entry, as the validate entry counts it
    assert rows(_lib.SPECTRA_WEIGHTS_REFINED, np.zeros((0, 3)), S, Sr) == S
    for source in (_lib.SPECTRA_WEIGHTS_RESIDENT, _lib.SPECTRA_WEIGHTS_HOST, _lib.SPECTRA_WEIGHTS_NONE):
        assert rows(source, dla, S, Sr) == S and rows(source, dla, S, None) == S
    assert rows(_lib.SPECTRA_WEIGHTS_REFINED, lls, S, None) == S
    with pytest.raises(_lib.GpdlaError):
        rows(_lib.SPECTRA_WEIGHTS_REFINED, dla, S, None)


# ---- the glue, on a hand-made case ----

def test_boxed_inputs_by_hand():
    g = dict(min_z=2.0, max_z=3.0, n_u=5, pad=np.arange(11.0), kept=np.ones(5, dtype=bool), marker="kept as it is")
    box = (2.25, 2.5, 20.0, 21.0)
    u, v = np.array([0.0, 0.5, 0.75]), np.array([0.0, 0.25, 0.5])
    lam = np.array([-3.0, np.nan, -np.inf])
    gb, sb, row = XC.boxed_inputs(g, box, u, v, lam)
    # the box is the range; everything else of the grid is the quasar's own, and the caller's grid is not touched
    assert gb["min_z"] == 2.25 and gb["max_z"] == 2.5 and gb["marker"] == "kept as it is" and gb["pad"] is g["pad"]
    assert g["min_z"] == 2.0 and g["max_z"] == 3.0
    # the restatements' own expression for z on these inputs gives z' = z_lo + (z_hi - z_lo) u
    z = gb["min_z"] + (gb["max_z"] - gb["min_z"]) * sb["offset_samples"]
    np.testing.assert_array_equal(z, [2.25, 2.375, 2.4375])
    np.testing.assert_array_equal(sb["nhi_samples"], [1e20, 10.0 ** 20.25, 10.0 ** 20.5])
    np.testing.assert_array_equal(row, lam)
    zp, npr = XC.refined_sample_parameters(box, u, v)
    np.testing.assert_array_equal(zp, z)
    np.testing.assert_array_equal(npr, [20.0, 20.25, 20.5])
    # the weights are those of mean_absorption on lambda: a NaN weighs 0, and so does a masked (-inf) entry
    np.testing.assert_array_equal(R.weights(row), [1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        XC.boxed_inputs(g, box, u, v[:2], lam)
    # a box of no width in z: every sample at z_lo
    gb, sb, _ = XC.boxed_inputs(g, (2.5, 2.5, 20.0, 20.0), u, v, lam)
    assert (gb["min_z"] + (gb["max_z"] - gb["min_z"]) * sb["offset_samples"] == 2.5).all() and (sb["nhi_samples"] == 1e20).all()


def test_restated_moments_on_a_box(oracle):
    """The glue through a restatement: two refined samples of equal weight, against the two profiles by hand."""
    from gp_dla_detection_amd import synthetic
    model = synthetic.make_model(4)
    sp = synthetic.make_spectrum(7000, 40, model)
    g = R.grid(oracle, model, sp)
    z_lo = g["min_z"] + 0.4 * (g["max_z"] - g["min_z"])
    z_hi = g["min_z"] + 0.6 * (g["max_z"] - g["min_z"])
    box = (z_lo, z_hi, 20.5, 21.0)
    u, v = np.array([0.25, 0.75, 0.5]), np.array([0.5, 0.25, 0.9])
    lam = np.array([-7.0, -7.0, np.nan])
    mean, var = XC.moments(oracle, g, box, u, v, lam, 3)
    a0 = oracle.voigt(g["pad"], z_lo + (z_hi - z_lo) * 0.25, 10.0 ** 20.75, 3)
    a1 = oracle.voigt(g["pad"], z_lo + (z_hi - z_lo) * 0.75, 10.0 ** 20.625, 3)
    np.testing.assert_allclose(mean, 0.5 * (a0 + a1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(var, 0.25 * (a0 - a1) ** 2, rtol=0, atol=1e-15)
    assert var.max() > 1e-4   # (the case tells the two samples apart)
