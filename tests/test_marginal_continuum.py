"""CPU checks of the marginal continuum: the C-ABI surface and its refusals (no device work), and the
restatement against itself -- dense against Woodbury, a one-hot row against the conditional continuum of
model_spectra_restatement, the mixture against a brute-force law of total variance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, synthetic

import marginal_continuum_cases as MC
import marginal_continuum_restatement as MR
import model_spectra_edge_cases as E
import model_spectra_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_the_entries_and_the_bindings_load(lib):
    header = open(os.path.join(ROOT, "include", "gpdla.h")).read()
    assert "#define GPDLA_ABI_VERSION 6" in header and lib.gpdla_abi_version() == 6
    for name in ("gpdla_marginal_continuum_request;", "gpdla_marginal_continuum;", "int gpdla_marginal_continuum_validate(",
                 "int gpdla_batch_marginal_continuum("):
        assert name in header, name
    names = [s[0] for s in _lib.SYMBOLS]
    assert "gpdla_marginal_continuum_validate" in names and "gpdla_batch_marginal_continuum" in names
    assert lib.gpdla_batch_marginal_continuum.argtypes[2]._type_ is _lib.MarginalContinuumRequest
    # the fields of the two structs, in the header's order
    for struct, cname in ((_lib.MarginalContinuumRequest, "gpdla_marginal_continuum_request"), (_lib.MarginalContinuum, "gpdla_marginal_continuum")):
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = re.findall(r"[\s\*](\w+)\s*[,;]", body)
        assert declared == [f[0] for f in struct._fields_], cname


def test_kernel_constants_of_the_case_lists():
    src = open(os.path.join(_lib.CSRC, "marginal_continuum_kernels.hpp")).read()
    src += open(os.path.join(_lib.CSRC, "mc_contract_body.hpp")).read()      # the body of k_mc_contract(_multi)
    host = open(os.path.join(_lib.CSRC, "host_grid.hpp")).read()      # MixturePlan::contract, which the predictive flux shares
    assert f"constexpr int kMcSolveChunk = {MC.SOLVE_CHUNK};" in src and f"constexpr int kMcPixTile = {MC.FINISH_TILE};" in src
    lo, hi = MC.CONTRACT[20], MC.CONTRACT[40]
    assert f"launch_mc_contract<{lo['samples'] // 16}, 4, {lo['pixels']}>" in host
    assert f"launch_mc_contract<{hi['samples'] // 16}, 14, {hi['pixels']}>" in host
    assert "atomic" not in src.replace("atomics", "")     # (the header says there are none)


def _request(nsel=2, S=8, **kw):
    rq = _lib.MarginalContinuumRequest()
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
        return lib.gpdla_marginal_continuum_validate(C.byref(rq[0]), nq, S, lls)
    w3 = lambda *rows: np.array(rows, dtype=np.float64)   # noqa: E731
    assert rc(_request()) == 0
    assert rc(_request(model_weights=w3([0.2, 0.3, 0.5], [1, 0, 0]))) == 0
    assert rc(_request(selection=np.array([0, 4], dtype=np.int64))) == -1 and b"selection" in lib.gpdla_last_error()
    assert rc(_request(num_selected=5)) == -1
    assert rc(_request(sample_log_likelihoods_dla=None)) == -1 and b"sample_log_likelihoods_dla" in lib.gpdla_last_error()
    assert rc(_request(sample_log_likelihoods_lls=None, model_weights=w3([0, 1, 0], [0, 0, 1]))) == -1
    assert rc(_request(sample_log_likelihoods_lls=None)) == 0          # the default mixture does not reach the sub-DLA table
    assert rc(_request(weights_source=0)) == -1 and b"weights source" in lib.gpdla_last_error()
    assert rc(_request(weights_source=0, model_weights=w3([1, 0, 0], [2, 0, 0]))) == 0   # null only: no table at all
    assert rc(_request(model_weights=w3([0, 1, 1], [0, 0, 1])), lls=0) == -1 and b"lls_nhi_samples" in lib.gpdla_last_error()
    assert rc(_request(model_weights=w3([0, 0, 1], [0, -0.1, 1]))) == -1 and b"model_weights" in lib.gpdla_last_error()
    assert rc(_request(model_weights=w3([0, 0, 1], [0, np.nan, 1]))) == -1
    assert rc(_request(model_weights=w3([0, 0, 1], [0, np.inf, 1]))) == -1
    assert rc(_request(model_weights=w3([0, 0, 1], [0, 0, 0]))) == -1 and b"positive" in lib.gpdla_last_error()
    assert rc(_request(sample_coefficients=1)) == 0
    assert rc(_request(sample_coefficients=1, model_weights=w3([0, 1, 0], [0, 0, 1]))) == -1 and b"both tables" in lib.gpdla_last_error()
    assert rc(_request(sample_coefficients=1, model_weights=w3([1, 0, 0], [1, 0, 0]))) == -1
    assert rc(_request(capacity=-1)) == -1
    assert lib.gpdla_marginal_continuum_validate(None, 4, 8, 1) == -1


@pytest.fixture(scope="module")
def small(oracle):
    """k = 4, 60 pixels (masked at 5 %), S = 12, sweep-like rows for both tables."""
    model, samples = synthetic.make_model(4), synthetic.make_samples(12)
    sp = synthetic.make_spectrum(6001, 60, model, mask_fraction=0.05)
    g = R.grid(oracle, model, sp)
    rng = np.random.default_rng(5)
    tables = {"dla": rng.normal(-20.0, 3.0, 12), "sub_dla": rng.normal(-22.0, 2.0, 12)}
    tables["dla"][4] = np.nan
    return model, samples, g, tables


@pytest.mark.parametrize("meanflux", [False, True])
def test_dense_and_woodbury_restatements_agree(oracle, small, meanflux):
    model, samples, g, tables = small
    p = (0.2, 0.3, 0.5)
    dense = MR.marginal_continuum(oracle, model, g, samples, tables, p, meanflux, 3, "dense")
    wood = MR.marginal_continuum(oracle, model, g, samples, tables, p, meanflux, 3, "woodbury")
    dis = MC.disagreement(dict(dense=[dense], woodbury=[wood]))
    print({n: f"{v:.2e}" for n, v in dis.items()})
    assert max(dis.values()) < 1e-9 and dense["status"] == 0
    assert (dense["continuum_var"] >= dense["continuum_var_between"] - 1e-15).all() and (dense["continuum_var_between"] > -1e-15).all()


def test_one_hot_row_is_the_conditional_continuum(oracle, small):
    model, samples, g, _ = small
    order = E.z_order(samples)
    i = int(order[7])
    row = np.full(12, -5000.0)
    row[i] = 0.0
    for meanflux in (False, True):
        got = MR.marginal_continuum(oracle, model, g, samples, {"dla": row}, (0, 0, 1), meanflux, 3, "dense")
        z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"][i]
        a = oracle.voigt(g["pad"], z, samples["nhi_samples"][i], 3)
        cont, _ = R.continuum(oracle, model, g, a, meanflux, "dense")
        d = MR.deviation(got["continuum_mean"], cont)
        print(f"meanflux {meanflux}: |delta| {d:.2e}")
        assert d < 1e-12
        assert (got["coef_cov_between"] == 0).all() and (got["continuum_var_between"] == 0).all()
        assert np.isnan(got["sample_coefficients"][np.arange(12) != i]).all() and np.isfinite(got["sample_coefficients"][i]).all()


def test_law_of_total_variance_against_the_brute_force_mixture(oracle, small):
    model, samples, g, tables = small
    p = np.array([0.25, 0.35, 0.4])
    rows = MR.prepared_rows(oracle, model, g, False)
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"]
    comps = [[(1.0,) + MR.sample_dense(*rows, np.ones(rows[0].size))]]
    for name in ("sub_dla", "dla"):
        w = R.weights(tables[name])
        comps.append([(w[i],) + MR.sample_dense(*rows, oracle.voigt(g["pad"], z[i], samples[MR.NHI_KEY[name]][i], 3)[g["kept"]])
                      for i in range(12) if w[i] > 0])
    mean, cov = MR.brute_force_mixture(comps, p)
    got = MR.marginal_continuum(oracle, model, g, samples, tables, p, False, 3, "dense")
    k = 4
    W, V = np.zeros((k, k)), np.zeros((k, k))
    W[np.tril_indices(k)], V[np.tril_indices(k)] = got["coef_cov_within"], got["coef_cov_between"]
    total = np.tril(W + V)
    d_mean, d_cov = MR.deviation(got["coef_mean"], mean), MR.deviation(total, np.tril(cov))
    print(f"|delta mean| {d_mean:.2e}, |delta cov| {d_cov:.2e}")
    assert d_mean < 1e-13 and d_cov < 1e-13
    # a component of weight 0 is not evaluated: an all-NaN table there changes nothing
    a = MR.marginal_continuum(oracle, model, g, samples, dict(tables, sub_dla=np.full(12, np.nan)), (0.5, 0, 0.5), False, 3)
    b = MR.marginal_continuum(oracle, model, g, samples, tables, (0.5, 0, 0.5), False, 3)
    assert np.array_equal(a["continuum_var"], b["continuum_var"]) and np.isfinite(a["continuum_var"]).all()
    # and with weight it makes the rows NaN, status 0
    c = MR.marginal_continuum(oracle, model, g, samples, dict(tables, sub_dla=np.full(12, -np.inf)), p, False, 3)
    assert np.isnan(c["continuum_mean"]).all() and c["status"] == 0


def test_api_rejects_what_it_can_before_the_library():
    from gp_dla_detection_amd import api
    with pytest.raises(ValueError):
        api.marginal_continuum(synthetic.make_model(2), synthetic.make_samples(4), [], None, model_weights="posteriors")
    w = api.posterior_model_weights(dict(p_no_dlas=[0.5, np.nan], p_dlas=[0.5, 1.0]))
    assert w.tolist() == [[0.5, 0.0, 0.5], [0.0, 0.0, 1.0]]
    w = api.posterior_model_weights(dict(p_no_dlas=[1.0], p_lls=[1e-9], p_dlas=[-5.3e-166]))
    assert w.tolist() == [[1.0, 1e-9, 0.0]]
