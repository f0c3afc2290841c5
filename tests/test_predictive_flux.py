"""CPU checks of the posterior predictive flux: the C-ABI surface and its refusals (no device work), and
the restatement against itself -- dense against Woodbury, the law of total variance against a brute-force mixture over
(model, sample) pairs, a one-hot row against absorption x the conditional continuum of model_spectra_restatement, and the
dense-vs-Woodbury disagreement of every setup of the case lists, which must stay under the cap of the tolerance rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, synthetic

import model_spectra_edge_cases as E
import model_spectra_restatement as R
import predictive_flux_cases as PC
import predictive_flux_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_the_entries_and_the_bindings_load(lib):
    header = open(os.path.join(ROOT, "include", "gpdla.h")).read()
    assert "#define GPDLA_ABI_VERSION 6" in header and lib.gpdla_abi_version() == 6
    for name in ("gpdla_predictive_flux_request;", "gpdla_predictive_flux;", "int gpdla_predictive_flux_validate(",
                 "int gpdla_batch_predictive_flux("):
        assert name in header, name
    names = [s[0] for s in _lib.SYMBOLS]
    assert "gpdla_predictive_flux_validate" in names and "gpdla_batch_predictive_flux" in names
    assert lib.gpdla_batch_predictive_flux.argtypes[2]._type_ is _lib.PredictiveFluxRequest
    assert lib.gpdla_batch_predictive_flux.argtypes[3]._type_ is _lib.PredictiveFlux
    # the fields of the two structs, in the header's order
    fields = {}
    for struct, cname in ((_lib.PredictiveFluxRequest, "gpdla_predictive_flux_request"), (_lib.PredictiveFlux, "gpdla_predictive_flux")):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields[cname] = re.findall(r"[\s\*](\w+)\s*[,;]", body)
        assert fields[cname] == [f[0] for f in struct._fields_], cname
    # the request is the marginal continuum's minus sample_coefficients
    assert fields["gpdla_predictive_flux_request"] == [f[0] for f in _lib.MarginalContinuumRequest._fields_ if f[0] != "sample_coefficients"]
    assert fields["gpdla_predictive_flux"] == ["offsets"] + list(PR.PRODUCTS_MEAN) + ["flux_var", "flux_var_within", "flux_var_between",
                                                                                      "noise_var", "status"]
    assert os.path.join(_lib.CSRC, "host_predictive_flux.hpp") in _lib.host_sources()


def test_kernel_constants_of_the_case_lists():
    src = open(os.path.join(_lib.CSRC, "predictive_flux_kernels.hpp")).read()
    src += open(os.path.join(_lib.CSRC, "pf_pixels_body.hpp")).read()      # the body of k_pf_pixels(_multi)
    host = open(os.path.join(_lib.CSRC, "host_predictive_flux.hpp")).read()
    assert f"constexpr int kPfRowTiles = {PC.SAMPLES // 16};" in src and "constexpr int kPfSamples = 16 * kPfRowTiles;" in src
    assert f"constexpr int kPfPixTile = {PC.PIXEL_TILE};" in src
    mc = open(os.path.join(_lib.CSRC, "marginal_continuum_kernels.hpp")).read()
    assert f"constexpr int kMcSolveChunk = {PC.SOLVE_CHUNK};" in mc
    assert "atomic" not in src.replace("atomics", "")     # (the header says there are none)
    # the request checks, the launch groups and their budget are the shared front end's (host_grid.hpp), not copies
    grid = open(os.path.join(_lib.CSRC, "host_grid.hpp")).read()
    assert "validate_mixture(" in host and "int validate_mixture(" in grid and "MixturePlan plan(" in host
    assert "mc_scratch_bytes()" in grid and "getenv" not in host and "getenv" not in src
    for copied in ("check_selection(", "model_weights[", "mc_scratch_bytes", "McContractArgs", "k_spectra_weights"):
        assert copied not in host, copied


def _request(nsel=2, S=8, **kw):
    rq = _lib.PredictiveFluxRequest()
    rq.num_selected = nsel
    rq.weights_source = _lib.SPECTRA_WEIGHTS_HOST
    keep = [np.zeros((nsel, S)), np.zeros((nsel, S))]
    rq.sample_log_likelihoods_dla = keep[0].ctypes.data_as(_dp)
    rq.sample_log_likelihoods_lls = keep[1].ctypes.data_as(_dp)
    for name, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data_as(_i64p if v.dtype == np.int64 else _dp)
        setattr(rq, name, v)
    return rq, keep


def test_validate_refuses_bad_requests(lib):
    def rc(rq, nq=4, S=8, lls=1):
        return lib.gpdla_predictive_flux_validate(C.byref(rq[0]), nq, S, lls)
    w3 = lambda *rows: np.array(rows, dtype=np.float64)   # noqa: E731
    assert rc(_request()) == 0
    assert rc(_request(model_weights=w3([0.2, 0.3, 0.5], [1, 0, 0]))) == 0
    assert rc(_request(selection=np.array([0, 4], dtype=np.int64))) == -1 and b"selection" in lib.gpdla_last_error()
    assert rc(_request(selection=np.array([0, -1], dtype=np.int64))) == -1
    assert rc(_request(num_selected=5)) == -1
    assert rc(_request(sample_log_likelihoods_dla=None)) == -1 and b"sample_log_likelihoods_dla" in lib.gpdla_last_error()
    assert rc(_request(sample_log_likelihoods_lls=None, model_weights=w3([0, 1, 0], [0, 0, 1]))) == -1
    assert b"sample_log_likelihoods_lls" in lib.gpdla_last_error()
    assert rc(_request(sample_log_likelihoods_lls=None)) == 0          # the default mixture does not reach the sub-DLA table
    assert rc(_request(weights_source=0)) == -1 and b"weights source" in lib.gpdla_last_error()
    assert rc(_request(weights_source=7)) == -1
    assert rc(_request(weights_source=0, model_weights=w3([1, 0, 0], [2, 0, 0]))) == 0   # null only: no table at all
    assert rc(_request(model_weights=w3([0, 1, 1], [0, 0, 1])), lls=0) == -1 and b"lls_nhi_samples" in lib.gpdla_last_error()
    assert rc(_request(model_weights=w3([0, 0, 1], [0, -0.1, 1]))) == -1 and b"model_weights" in lib.gpdla_last_error()
    assert rc(_request(model_weights=w3([0, 0, 1], [0, np.nan, 1]))) == -1
    assert rc(_request(model_weights=w3([0, 0, 1], [0, np.inf, 1]))) == -1
    assert rc(_request(model_weights=w3([0, 0, 1], [0, 0, 0]))) == -1 and b"positive" in lib.gpdla_last_error()
    assert rc(_request(), S=0) == -1 and b"no samples" in lib.gpdla_last_error()
    assert rc(_request(capacity=-1)) == -1
    assert lib.gpdla_predictive_flux_validate(None, 4, 8, 1) == -1


@pytest.fixture(scope="module")
def small(oracle):
    """k = 4, 60 pixels (masked at 5 %), S = 12, sweep-like rows for both tables."""
    model, samples = synthetic.make_model(4), synthetic.make_samples(12)
    sp = synthetic.make_spectrum(6001, 60, model, mask_fraction=0.05)
    g = R.grid(oracle, model, sp)
    assert not g["kept"].all()
    rng = np.random.default_rng(5)
    tables = {"dla": rng.normal(-20.0, 3.0, 12), "sub_dla": rng.normal(-22.0, 2.0, 12)}
    tables["dla"][4] = np.nan
    return model, samples, g, tables


@pytest.mark.parametrize("meanflux", [False, True])
def test_dense_and_woodbury_restatements_agree(oracle, small, meanflux):
    model, samples, g, tables = small
    p = (0.2, 0.3, 0.5)
    dense = PR.predictive_flux(oracle, model, g, samples, tables, p, meanflux, 3, "dense")
    wood = PR.predictive_flux(oracle, model, g, samples, tables, p, meanflux, 3, "woodbury")
    dis = PC.disagreement(dict(dense=[dense], woodbury=[wood]))
    print({n: f"{v:.2e}" for n, v in dis.items()})
    assert max(dis.values()) < 1e-9 and dense["status"] == 0
    assert (dense["flux_var"] == dense["flux_var_within"] + dense["flux_var_between"]).all()
    assert (dense["flux_var_between"] >= 0).all() and (dense["flux_var_within"] > 0).all()
    # noise_var: NaN exactly on the masked pixels
    assert np.array_equal(np.isnan(dense["noise_var"]), ~g["kept"]) and np.isfinite(dense["flux_mean"]).all()


def test_law_of_total_variance_against_the_brute_force_mixture(oracle, small):
    model, samples, g, tables = small
    p = np.array([0.25, 0.35, 0.4])
    parts, none = PR.components(oracle, model, g, samples, tables, p, False, 3, "dense")
    assert not none and len(parts[2]["pairs"]) == 11       # (the NaN entry weighs 0 and is never touched)
    mean, var = PR.brute_force_mixture(parts, p)
    got = PR.predictive_flux(oracle, model, g, samples, tables, p, False, 3, "dense")
    d_mean, d_var = PR.deviation(got["flux_mean"], mean), PR.deviation(got["flux_var"], var)
    print(f"|delta mean| {d_mean:.2e}, |delta var| {d_var:.2e}")
    assert d_mean < 1e-13 and d_var < 1e-13
    # E[a t] is not E[a] E[t]: the product of the two marginal means differs from the predictive mean by far more
    Ea = sum(pm * sum(w * a for w, a, _, _ in part["pairs"]) for part, pm in zip(parts, p))
    Et = sum(pm * sum(w * t for w, _, t, _ in part["pairs"]) for part, pm in zip(parts, p))
    print(f"max |E[a t] - E[a] E[t]| {np.abs(got['flux_mean'] - Ea * Et).max():.2e}")
    assert np.abs(got["flux_mean"] - Ea * Et).max() > 1e-6
    # a component of weight 0 is not evaluated: an all-NaN table there changes nothing
    a = PR.predictive_flux(oracle, model, g, samples, dict(tables, sub_dla=np.full(12, np.nan)), (0.5, 0, 0.5), False, 3)
    b = PR.predictive_flux(oracle, model, g, samples, tables, (0.5, 0, 0.5), False, 3)
    assert np.array_equal(a["flux_var"], b["flux_var"]) and np.isfinite(a["flux_var"]).all()
    # and with weight it makes the rows NaN, status 0
    c = PR.predictive_flux(oracle, model, g, samples, dict(tables, sub_dla=np.full(12, -np.inf)), p, False, 3)
    assert all(np.isnan(c[n]).all() for n in PR.PRODUCTS) and c["status"] == 0


def test_one_hot_row_is_absorption_times_the_conditional_continuum(oracle, small):
    model, samples, g, _ = small
    order = E.z_order(samples)
    i = int(order[7])
    row = np.full(12, -5000.0)
    row[i] = 0.0
    for meanflux in (False, True):
        got = PR.predictive_flux(oracle, model, g, samples, {"dla": row}, (0, 0, 1), meanflux, 3, "dense")
        z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"][i]
        a = oracle.voigt(g["pad"], z, samples["nhi_samples"][i], 3)
        cont, flux = R.continuum(oracle, model, g, a, meanflux, "dense")
        d = PR.deviation(got["flux_mean"], a * cont)
        print(f"meanflux {meanflux}: |flux_mean - a x R.continuum| {d:.2e}")
        assert d < 1e-12 and np.array_equal(a * cont, flux)
        assert (got["flux_var_between"] == 0).all() and (got["flux_var"] == got["flux_var_within"]).all()


@pytest.mark.parametrize("name", [s["name"] for s in PC.SETUPS])
def test_no_setup_reaches_the_cap_of_the_tolerance_rule(oracle, name):
    """The dense-vs-Woodbury disagreement of every setup of the case lists, on a synthetic table (no sweep here): ten times
    it must stay under 1e-8, or the tolerance of the GPU comparison would be the cap and not the restatement's own error."""
    st = PC.setup(name)
    model, samples, spectra = PC.build(st)
    table = PC.synthetic_table(samples, len(spectra))
    pw = [0.0, 1.0, 0.0] if st["table"] == "sub_dla" else [0.0, 0.0, 1.0]
    want = PC.wanted(oracle, ("cpu", name), model, samples, spectra, {st["table"]: table}, pw, st["multi"], st["lines"])
    dis = PC.disagreement(want)
    tol = PR.tolerances(dis)
    for n in PR.PRODUCTS:
        print(f"{name} {n}: dense-vs-Woodbury {dis[n]:.2e} -> tolerance {tol[n]:.2e}")
    assert all(w["status"] == 0 for w in want["dense"])
    assert 10.0 * max(dis.values()) < 1e-8, dis


def test_residuals_helper_and_what_the_api_rejects_before_the_library():
    from gp_dla_detection_amd import api
    pf = dict(offsets=np.array([0, 3, 5]), flux_mean=np.array([1.0, 1.0, 1.0, 2.0, 2.0]), flux_var=np.full(5, 0.03),
              noise_var=np.array([0.01, np.nan, 0.01, 0.01, np.nan]))
    out = api.predictive_residuals(pf, np.array([1.2, 9.0, 0.8, 2.0, 7.0]), np.array([True, False, True, True, False]))
    np.testing.assert_allclose(out["residual"][[0, 2, 3]], [1.0, -1.0, 0.0], atol=1e-12)
    assert np.isnan(out["residual"][[1, 4]]).all() and out["num_kept"].tolist() == [2, 1]
    np.testing.assert_allclose(out["chi2"], [2.0, 0.0], atol=1e-12)
    with pytest.raises(ValueError):
        api.predictive_flux(synthetic.make_model(2), synthetic.make_samples(4), [], None, model_weights="posteriors")
    doc = api.Batch.predictive_flux.__doc__
    assert "in-sample" in doc.lower() and "leave-one-out" in doc and "replicate" in doc
