"""CPU checks of the marginal continuum and the predictive flux over all models of a multi-DLA run: the
C-ABI surface and its refusals (no device work), and the restatements against themselves -- dense against Woodbury on every
setup of tests/mixture_multi_cases.py, the n = 1 seam with the restatements of 4.23 / 4.24 bit for bit, a one-hot row
against the conditional continuum of model_spectra_restatement, the mixture against a brute-force law of total variance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, synthetic

import marginal_continuum_multi_restatement as MMR
import marginal_continuum_restatement as MR
import mixture_multi_cases as XC
import model_spectra_edge_cases as E
import model_spectra_multi_cases as MSC
import model_spectra_multi_restatement as RM
import model_spectra_restatement as R
import predictive_flux_multi_restatement as PMR
import predictive_flux_restatement as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_u32p = C.POINTER(C.c_uint32)

STRUCTS = ((_lib.MarginalContinuumMultiRequest, "gpdla_marginal_continuum_multi_request"),
           (_lib.MarginalContinuumMulti, "gpdla_marginal_continuum_multi"),
           (_lib.PredictiveFluxMultiRequest, "gpdla_predictive_flux_multi_request"),
           (_lib.PredictiveFluxMulti, "gpdla_predictive_flux_multi"))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declares_the_entries_and_the_bindings_load(lib):
    header = open(os.path.join(ROOT, "include", "gpdla.h")).read()
    assert "#define GPDLA_ABI_VERSION 6" in header and lib.gpdla_abi_version() == 6
    names = [s[0] for s in _lib.SYMBOLS]
    for entry in ("marginal_continuum_multi", "predictive_flux_multi"):
        assert f"int gpdla_{entry}_validate(" in header and f"int gpdla_batch_{entry}(" in header
        assert f"gpdla_{entry}_validate" in names and f"gpdla_batch_{entry}" in names
    assert lib.gpdla_batch_marginal_continuum_multi.argtypes[2]._type_ is _lib.MarginalContinuumMultiRequest
    assert lib.gpdla_batch_predictive_flux_multi.argtypes[3]._type_ is _lib.PredictiveFluxMulti
    for struct, cname in STRUCTS:       # the fields of the four structs, in the header's order
        body = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = re.findall(r"[\s\*](\w+)\s*[,;]", body)
        assert declared == [f[0] for f in struct._fields_], cname


C_CONSUMER = r"""
#include <stddef.h>
#include <stdio.h>
#include "gpdla.h"
#define SIZE(T) printf("sizeof " #T " %zu\n", sizeof(T))
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  SIZE(gpdla_marginal_continuum_multi_request); SIZE(gpdla_marginal_continuum_multi);
  SIZE(gpdla_predictive_flux_multi_request); SIZE(gpdla_predictive_flux_multi);
  OFF(gpdla_marginal_continuum_multi_request, tables_source); OFF(gpdla_marginal_continuum_multi_request, base_sample_inds);
  OFF(gpdla_marginal_continuum_multi_request, capacity); OFF(gpdla_marginal_continuum_multi, model_flags);
  OFF(gpdla_predictive_flux_multi_request, model_weights); OFF(gpdla_predictive_flux_multi_request, capacity);
  OFF(gpdla_predictive_flux_multi, noise_var); OFF(gpdla_predictive_flux_multi, model_flags);
  /* the validators need no GPU */
  if (gpdla_marginal_continuum_multi_validate(NULL, 1, 1, 1, 2, 1) != GPDLA_ERR_INVALID_ARGUMENT) return 2;
  if (gpdla_predictive_flux_multi_validate(NULL, 1, 1, 1, 2, 1) != GPDLA_ERR_INVALID_ARGUMENT) return 3;
  return 0;
}
"""


def test_struct_sizes_against_a_c_consumer(lib, tmp_path):
    src, exe = tmp_path / "consumer.c", tmp_path / "consumer"
    src.write_text(C_CONSUMER)
    hip_rt = os.path.dirname(_lib._preload_hip_runtime()._name)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    _lib.DEFAULT_LIB_PATH, "-L", hip_rt, "-lamdhip64", f"-Wl,-rpath,{os.path.dirname(_lib.DEFAULT_LIB_PATH)}",
                    f"-Wl,-rpath,{hip_rt}"], check=True, capture_output=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    seen = dict(line.rsplit(" ", 1) for line in res.stdout.strip().splitlines())
    mirrors = {cname: struct for struct, cname in STRUCTS}
    for cname, mirror in mirrors.items():
        assert int(seen[f"sizeof {cname}"]) == C.sizeof(mirror), cname
    offsets = [key for key in seen if "." in key]
    assert len(offsets) == 8
    for key in offsets:
        cname, field = key.split(".")
        assert int(seen[key]) == getattr(mirrors[cname], field).offset, key


def _request(cls, nsel=2, S=8, md=3, **kw):
    """A valid host-table request with weight on every component; ``kw`` overrides fields (None: a null pointer)."""
    rq = cls()
    rq.num_selected, rq.max_dlas, rq.tables_source = nsel, md, _lib.SPECTRA_WEIGHTS_HOST
    keep = dict(sample_log_likelihoods_dla=np.zeros((nsel, md, S)), sample_log_likelihoods_lls=np.zeros((nsel, S)),
                base_sample_inds=np.ones((nsel, max(md - 1, 1), S), dtype=np.uint32), model_weights=np.ones((nsel, 2 + md)))
    keep.update(kw)
    for name, v in keep.items():
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v)
            keep[name] = v
            v = v.ctypes.data_as({np.dtype(np.int64): _i64p, np.dtype(np.uint32): _u32p}.get(v.dtype, _dp))
        setattr(rq, name, v)
    return rq, keep


@pytest.mark.parametrize("entry", ["marginal_continuum_multi", "predictive_flux_multi"])
def test_validate_refuses_bad_requests(lib, entry):
    cls = _lib.MarginalContinuumMultiRequest if entry.startswith("marginal") else _lib.PredictiveFluxMultiRequest
    validate = getattr(lib, f"gpdla_{entry}_validate")

    def rc(rq, nq=4, S=8, lls=1, batch_md=0, processed=0):
        return validate(C.byref(rq[0]), nq, S, lls, batch_md, processed)
    err = lib.gpdla_last_error
    rows = lambda *r: np.array(r, dtype=np.float64)   # noqa: E731
    RESIDENT = _lib.SPECTRA_WEIGHTS_RESIDENT
    assert rc(_request(cls)) == 0
    assert validate(None, 4, 8, 1, 0, 0) == -1
    assert rc(_request(cls, selection=np.array([0, 4], dtype=np.int64))) == -1 and b"selection" in err()
    assert rc(_request(cls, num_selected=5)) == -1
    assert rc(_request(cls, max_dlas=0)) == -1 and b"max_dlas" in err()
    assert rc(_request(cls, max_dlas=5)) == -1
    assert rc(_request(cls, tables_source=7)) == -1 and b"tables_source" in err()
    assert rc(_request(cls, capacity=-1)) == -1
    # resident tables: a single-DLA batch, another max_dlas, an unprocessed batch
    assert rc(_request(cls, tables_source=RESIDENT), batch_md=0, processed=0) == -1 and b"not a multi-DLA batch" in err()
    assert rc(_request(cls, tables_source=RESIDENT), batch_md=4, processed=1) == -1 and b"max_dlas" in err()
    assert rc(_request(cls, tables_source=RESIDENT), batch_md=3, processed=0) == -1 and b"not been processed" in err()
    assert rc(_request(cls, tables_source=RESIDENT), batch_md=3, processed=1) == 0
    assert rc(_request(cls, tables_source=RESIDENT, model_weights=None), batch_md=3, processed=1) == 0    # the resident posteriors
    assert rc(_request(cls, tables_source=RESIDENT, model_weights=None), batch_md=3, processed=1, lls=0) == -1
    # host tables: model_weights, the tables a weighted component needs, the base indices
    assert rc(_request(cls, model_weights=None)) == -1 and b"model_weights" in err()
    assert rc(_request(cls, sample_log_likelihoods_dla=None)) == -1 and b"sample_log_likelihoods_dla" in err()
    assert rc(_request(cls, sample_log_likelihoods_lls=None)) == -1 and b"sample_log_likelihoods_lls" in err()
    assert rc(_request(cls, base_sample_inds=None)) == -1 and b"base_sample_inds" in err()
    only = lambda *cols: rows(*[[1.0 if c in cols else 0.0 for c in range(5)]] * 2)   # noqa: E731
    assert rc(_request(cls, sample_log_likelihoods_lls=None, model_weights=only(0, 2, 4))) == 0   # the sub-DLA column weighs nothing
    assert rc(_request(cls, base_sample_inds=None, sample_log_likelihoods_lls=None, model_weights=only(0, 2))) == 0   # DLA(1) only
    assert rc(_request(cls, sample_log_likelihoods_dla=None, base_sample_inds=None, model_weights=only(0, 1))) == 0
    assert rc(_request(cls, sample_log_likelihoods_dla=None, base_sample_inds=None, sample_log_likelihoods_lls=None,
                       model_weights=only(0))) == 0                                                # the null model alone
    big = np.ones((2, 2, 8), dtype=np.uint32)
    big[1, 1, 3] = 9
    assert rc(_request(cls, base_sample_inds=big)) == -1 and b"exceeds" in err()
    big[1, 1, 3] = 8
    assert rc(_request(cls, base_sample_inds=big)) == 0
    big[1, 1, 3] = 0
    assert rc(_request(cls, base_sample_inds=big)) == 0                                            # never drawn
    # the sub-DLA column without lls_nhi_samples
    assert rc(_request(cls), lls=0) == -1 and b"lls_nhi_samples" in err()
    assert rc(_request(cls, model_weights=only(0, 2, 3)), lls=0) == 0
    # weight rows: negative, infinite, no positive sum are refused; a NaN is not
    w = np.ones((2, 5))
    for bad, word in ((-0.1, b"model_weights"), (np.inf, b"model_weights"), (-np.inf, b"model_weights")):
        w2 = w.copy()
        w2[1, 3] = bad
        assert rc(_request(cls, model_weights=w2)) == -1 and word in err()
    assert rc(_request(cls, model_weights=rows([1, 1, 1, 1, 1], [0, 0, 0, 0, 0]))) == -1 and b"positive" in err()
    w2 = w.copy()
    w2[1, 3] = np.nan
    assert rc(_request(cls, model_weights=w2)) == 0
    w2[1, 2] = -1.0     # (a NaN row is not looked at)
    assert rc(_request(cls, model_weights=w2)) == 0
    assert rc(_request(cls, model_weights=np.full((2, 5), np.nan), sample_log_likelihoods_dla=None, base_sample_inds=None,
                       sample_log_likelihoods_lls=None)) == 0


# ------------------------------------------------------------------------------------------------
# the restatements against themselves
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [s["name"] for s in XC.SETUPS])
def test_dense_and_woodbury_restatements_agree(oracle, name):
    """Every setup of the cases file on a seeded table.  The GPU tolerances are 10 x this disagreement per product family,
    floored at 1e-12 and capped at 1e-8; the cap is a condition: every setup stays below 1e-9, so no tolerance comes near it."""
    st = XC.setup(name)
    model, samples, spectra = XC.build(st)
    tables = XC.host_tables(st, samples, *XC.synthetic_sweep(st))
    P = XC.model_weights(st)
    want = XC.wanted(oracle, ("cpu", name), model, samples, spectra, tables, P, st["meanflux"], st["lines"], p=XC.params(st))
    dis = {**MMR.disagreement(want["mc"]["dense"], want["mc"]["woodbury"]), **PMR.disagreement(want["pf"]["dense"], want["pf"]["woodbury"])}
    print(name, {n: f"{v:.2e}" for n, v in dis.items()})
    assert 10.0 * max(dis.values()) < 1e-9
    for q, kind in enumerate(st["kinds"]):
        for d in (want["mc"]["dense"][q], want["pf"]["dense"][q]):
            arrays = [v for n, v in d.items() if n not in ("status", "model_flags", "noise_var")]
            if kind == "none":
                assert d["status"] == 0 and d["model_flags"] == XC.all_flags(st["md"]) and all(np.isnan(a).all() for a in arrays)
            else:
                assert d["status"] == 0 and d["model_flags"] == 0 and all(np.isfinite(a).all() for a in arrays), (q, kind)


@pytest.fixture(scope="module")
def small(oracle):
    """k = 4, 60 pixels (masked at 5 %), S = 12, max_dlas = 3, sweep-like rows, random base indices with two zeros."""
    model, samples = synthetic.make_model(4), synthetic.make_samples(12)
    sp = synthetic.make_spectrum(6001, 60, model, mask_fraction=0.05)
    g = R.grid(oracle, model, sp)
    rng = np.random.default_rng(5)
    tables = dict(sample_log_likelihoods_dla=rng.normal(-20.0, 3.0, (3, 12)), sample_log_likelihoods_lls=rng.normal(-22.0, 2.0, 12),
                  base_sample_inds=MSC.base_rows("random", 12, 3, samples, seed=1))
    tables["sample_log_likelihoods_dla"][0, 4] = np.nan
    tables["base_sample_inds"][1, [2, 9]] = 0
    return model, samples, g, tables


@pytest.mark.parametrize("meanflux", [False, True])
def test_n1_is_the_three_component_restatement_bit_for_bit(oracle, small, meanflux):
    """Weights on (null, sub-DLA, DLA(1)) only: the restatements of DESIGN 4.23 / 4.24 on the DLA(1) row."""
    model, samples, g, tables = small
    P = np.array([0.2, 0.3, 0.5, 0.0, 0.0])
    old = {"dla": tables["sample_log_likelihoods_dla"][0], "sub_dla": tables["sample_log_likelihoods_lls"]}
    for form in ("dense", "woodbury"):
        a = MMR.marginal_continuum_multi(oracle, model, g, samples, tables, P, meanflux, 3, form)
        b = MR.marginal_continuum(oracle, model, g, samples, old, P[:3], meanflux, 3, form)
        for name in MMR.ARRAYS + MMR.ROWS:
            assert np.isfinite(a[name]).all() and np.array_equal(a[name], b[name]), (form, name)
        c = PMR.predictive_flux_multi(oracle, model, g, samples, tables, P, meanflux, 3, form)
        d = PR.predictive_flux(oracle, model, g, samples, old, P[:3], meanflux, 3, form)
        for name in PR.PRODUCTS:
            assert np.array_equal(c[name], d[name], equal_nan=True) and np.isfinite(c["flux_mean"]).all(), (form, name)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_one_hot_row_is_the_conditional_continuum_of_the_slot_absorbers(oracle, small, n):
    model, samples, g, tables = small
    i = int(E.z_order(samples)[7])
    assert RM.slots(tables["base_sample_inds"], 3, i) is not None
    row = np.full(12, -5000.0)
    row[i] = 0.0
    hot = dict(tables, sample_log_likelihoods_dla=np.tile(row, (3, 1)))
    P = np.zeros(5)
    P[1 + n] = 1.0
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"]
    a = np.ones(g["n_u"])
    for sj in RM.slots(tables["base_sample_inds"], n, i):
        a = a * oracle.voigt(g["pad"], z[sj], samples["nhi_samples"][sj], 3)
    for meanflux in (False, True):
        cont, _ = R.continuum(oracle, model, g, a, meanflux, "dense")
        mc = MMR.marginal_continuum_multi(oracle, model, g, samples, hot, P, meanflux, 3, "dense")
        pf = PMR.predictive_flux_multi(oracle, model, g, samples, hot, P, meanflux, 3, "dense")
        d_c, d_f = MR.deviation(mc["continuum_mean"], cont), MR.deviation(pf["flux_mean"], a * cont)
        print(f"model {n} meanflux {meanflux}: |d continuum| {d_c:.2e}, |d flux| {d_f:.2e}")
        assert d_c < 1e-13 and d_f < 1e-13
        assert (mc["coef_cov_between"] == 0).all() and (mc["continuum_var_between"] == 0).all() and (pf["flux_var_between"] == 0).all()


def test_law_of_total_variance_against_the_brute_force_mixture(oracle, small):
    model, samples, g, tables = small
    P = np.array([0.15, 0.2, 0.25, 0.3, 0.1])
    mc_parts, flags = MMR.parts_of(oracle, model, g, samples, tables, P, False, 3, "dense")
    pf_parts, flags2 = PMR.parts_of(oracle, model, g, samples, tables, P, False, 3, "dense")
    assert flags == flags2 == 0
    # the samples that consume a 0 drop out of model 3, and only there
    assert [len(part["pairs"]) for part in mc_parts] == [1, 12, 11, 12, 10]
    mean, cov = MR.brute_force_mixture([part["pairs"] for part in mc_parts], P)
    got = MMR.marginal_continuum_multi(oracle, model, g, samples, tables, P, False, 3, "dense")
    k = 4
    W, V = np.zeros((k, k)), np.zeros((k, k))
    W[np.tril_indices(k)], V[np.tril_indices(k)] = got["coef_cov_within"], got["coef_cov_between"]
    d_mean, d_cov = MR.deviation(got["coef_mean"], mean), MR.deviation(np.tril(W + V), np.tril(cov))
    fmean, fvar = PR.brute_force_mixture(pf_parts, P)
    pf = PMR.predictive_flux_multi(oracle, model, g, samples, tables, P, False, 3, "dense")
    d_f, d_v = MR.deviation(pf["flux_mean"], fmean), MR.deviation(pf["flux_var"], fvar)
    print(f"|d coef mean| {d_mean:.2e}, |d coef cov| {d_cov:.2e}, |d flux mean| {d_f:.2e}, |d flux var| {d_v:.2e}")
    assert max(d_mean, d_cov, d_f, d_v) < 1e-13
    # a component of weight 0 is not evaluated; with weight, a row without weights makes the rows NaN and is flagged
    dead = dict(tables, sample_log_likelihoods_dla=np.array(tables["sample_log_likelihoods_dla"]))
    dead["sample_log_likelihoods_dla"][1] = np.nan
    P0 = np.array([0.2, 0.2, 0.3, 0.0, 0.3])
    a = MMR.marginal_continuum_multi(oracle, model, g, samples, dead, P0, False, 3)
    b = MMR.marginal_continuum_multi(oracle, model, g, samples, tables, P0, False, 3)
    assert np.array_equal(a["continuum_var"], b["continuum_var"]) and np.isfinite(a["continuum_var"]).all() and a["model_flags"] == 0
    c = PMR.predictive_flux_multi(oracle, model, g, samples, dead, P, False, 3)
    assert np.isnan(c["flux_mean"]).all() and c["status"] == 0 and c["model_flags"] == 2
    e = MMR.marginal_continuum_multi(oracle, model, g, samples, tables, [0.2, np.nan, 0.3, 0.2, 0.3], False, 3)
    assert np.isnan(e["continuum_mean"]).all() and e["status"] == MMR.UNDEFINED == _lib.SPECTRA_AVERAGE_UNDEFINED
    assert MMR.FLAG_LLS == _lib.SPECTRA_MULTI_FLAG_LLS
