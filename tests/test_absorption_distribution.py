"""The absorption distribution where no GPU is needed: the validate entries, api.forest_mask, the field
table and the saver, the restatement's own properties, and the non-vacuity of the bounds the GPU test compares against."""
import ctypes as C
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, grid_fields, io

import absorption_distribution_restatement as D

_dp, _i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _fill(rq, keep, thresholds, bins, levels):
    thr = None if thresholds is None else np.array(thresholds, dtype=np.float64)
    lev = None if levels is None else np.array(levels, dtype=np.float64)
    keep += [thr, lev]
    rq.num_thresholds = 0 if thr is None else thr.size
    rq.thresholds = None if thr is None else thr.ctypes.data_as(_dp)
    rq.num_levels = 0 if lev is None else lev.size
    rq.levels = None if lev is None else lev.ctypes.data_as(_dp)
    rq.num_bins = bins
    return rq, keep


def _request(thresholds=(0.8,), bins=0, levels=None, weights_source=_lib.SPECTRA_WEIGHTS_HOST, model_weights=None, nsel=2, S=8, **over):
    rq = _lib.AbsorptionDistributionRequest()
    table = np.zeros((nsel, S))
    pw = None if model_weights is None else np.array(model_weights, dtype=np.float64)
    rq.num_selected = nsel
    rq.weights_source = weights_source
    rq.sample_log_likelihoods_dla = table.ctypes.data_as(_dp)
    rq.model_weights = None if pw is None else pw.ctypes.data_as(_dp)
    rq, keep = _fill(rq, [table, pw], thresholds, bins, levels)
    for k, v in over.items():
        setattr(rq, k, v)
    return rq, keep


def _request_multi(thresholds=(0.8,), bins=0, levels=None, md=2, nsel=2, S=8):
    rq = _lib.AbsorptionDistributionMultiRequest()
    dla, lls = np.zeros((nsel, md, S)), np.zeros((nsel, S))
    base = np.ones((nsel, md - 1, S), dtype=np.uint32)
    pw = np.full((nsel, 2 + md), 1.0)
    rq.num_selected, rq.max_dlas, rq.tables_source = nsel, md, _lib.SPECTRA_WEIGHTS_HOST
    rq.sample_log_likelihoods_dla = dla.ctypes.data_as(_dp)
    rq.sample_log_likelihoods_lls = lls.ctypes.data_as(_dp)
    rq.base_sample_inds = base.ctypes.data_as(C.POINTER(C.c_uint32))
    rq.model_weights = pw.ctypes.data_as(_dp)
    return _fill(rq, [dla, lls, base, pw], thresholds, bins, levels)


REFUSED = {
    "five thresholds": dict(thresholds=(0.1, 0.2, 0.3, 0.4, 0.5)),
    "nine levels": dict(bins=64, levels=tuple(np.linspace(0.1, 0.9, 9))),
    "a threshold of 0": dict(thresholds=(0.0,)),
    "a threshold of 1": dict(thresholds=(1.0,)),
    "a NaN threshold": dict(thresholds=(0.5, float("nan"))),
    "an infinite threshold": dict(thresholds=(float("inf"),)),
    "a level of 0": dict(bins=64, levels=(0.0,)),
    "a level of 1": dict(bins=64, levels=(0.5, 1.0)),
    "a NaN level": dict(bins=64, levels=(float("nan"),)),
    "7 bins": dict(bins=7),
    "257 bins": dict(bins=257),
    "negative bins": dict(bins=-64),
    "levels without bins": dict(bins=0, levels=(0.5,)),
    "nothing requested": dict(thresholds=None, bins=0),
    "a count without its array": dict(thresholds=None, num_thresholds=2),
    "a negative count": dict(num_thresholds=-1),
}


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_validate_refuses(lib, what):
    rq, keep = _request(**REFUSED[what])
    assert lib.gpdla_absorption_distribution_validate(C.byref(rq), 4, 8, 1) == -1, what
    assert lib.gpdla_last_error()
    kw = {k: v for k, v in REFUSED[what].items() if k in ("thresholds", "bins", "levels")}
    rq, keep = _request_multi(**kw)
    for k, v in REFUSED[what].items():
        if k not in kw:
            setattr(rq, k, v)
    assert lib.gpdla_absorption_distribution_multi_validate(C.byref(rq), 4, 8, 1, 0, 0) == -1, what


def test_validate_keeps_the_mixtures_refusals(lib):
    v = lib.gpdla_absorption_distribution_validate
    rq, keep = _request(weights_source=_lib.SPECTRA_WEIGHTS_NONE)
    assert v(C.byref(rq), 4, 8, 1) == -1 and b"weights source" in lib.gpdla_last_error()
    rq, keep = _request(weights_source=_lib.SPECTRA_WEIGHTS_RESIDENT, model_weights=[[0.2, 0.3, 0.5], [1, 0, 0]])
    assert v(C.byref(rq), 4, 8, 0) == -1 and b"lls_nhi_samples" in lib.gpdla_last_error()
    rq, keep = _request(model_weights=[[0.0, 0.0, -1.0], [1, 0, 0]])
    assert v(C.byref(rq), 4, 8, 1) == -1
    rq, keep = _request(nsel=5)
    assert v(C.byref(rq), 4, 8, 1) == -1 and b"num_selected" in lib.gpdla_last_error()
    assert v(None, 4, 8, 1) == -1
    rq, keep = _request_multi(md=9)
    assert lib.gpdla_absorption_distribution_multi_validate(C.byref(rq), 4, 8, 1, 0, 0) == -1
    assert lib.gpdla_absorption_distribution_multi_validate(None, 4, 8, 1, 0, 0) == -1


def test_validate_accepts_the_legal_requests(lib):
    v = lib.gpdla_absorption_distribution_validate
    rq, keep = _request()
    assert v(C.byref(rq), 4, 8, 1) == 0, lib.gpdla_last_error()
    # null-only, no weights source
    rq, keep = _request(weights_source=_lib.SPECTRA_WEIGHTS_NONE, model_weights=[[1, 0, 0], [2, 0, 0]], bins=64, levels=(0.5,))
    assert v(C.byref(rq), 4, 8, 0) == 0, lib.gpdla_last_error()
    # at the limits
    for B in (8, 256):
        rq, keep = _request(thresholds=D.THRESHOLDS4, bins=B, levels=D.LEVELS8)
        assert v(C.byref(rq), 4, 8, 1) == 0, lib.gpdla_last_error()
        rq, keep = _request_multi(thresholds=D.THRESHOLDS4, bins=B, levels=D.LEVELS8)
        assert lib.gpdla_absorption_distribution_multi_validate(C.byref(rq), 4, 8, 1, 0, 0) == 0, lib.gpdla_last_error()
    # bins alone
    rq, keep = _request(thresholds=None, bins=64)
    assert v(C.byref(rq), 4, 8, 1) == 0


def test_header_declares_the_entries(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpdla.h")).read()
    assert "#define GPDLA_ABI_VERSION 6" in header and lib.gpdla_abi_version() == 6
    for name in ("} gpdla_absorption_distribution_request;", "} gpdla_absorption_distribution;",
                 "} gpdla_absorption_distribution_multi_request;", "} gpdla_absorption_distribution_multi;",
                 "int gpdla_absorption_distribution_validate(", "int gpdla_batch_absorption_distribution(",
                 "int gpdla_absorption_distribution_multi_validate(", "int gpdla_batch_absorption_distribution_multi("):
        assert name in header, name
    # the mixture's fields first, under the same names
    names = [f[0] for f in _lib.AbsorptionDistributionRequest._fields_]
    assert names[:8] == [f[0] for f in _lib.PredictiveFluxRequest._fields_]
    names = [f[0] for f in _lib.AbsorptionDistributionMultiRequest._fields_]
    assert names[:10] == [f[0] for f in _lib.MarginalContinuumMultiRequest._fields_]


def test_forest_mask():
    nan = float("nan")
    res = {"prob_below": np.array([[0.0, 0.49, 0.5, 0.51, 1.0, nan], [0.9, 0.1, nan, 0.3, 0.31, 0.0]])}
    np.testing.assert_array_equal(gp.forest_mask(res), [False, False, True, True, True, False])
    np.testing.assert_array_equal(gp.forest_mask(res, threshold_index=1, probability=0.3), [True, False, False, True, True, False])
    assert gp.forest_mask(res).dtype == bool
    assert gp.forest_mask({"prob_below": np.zeros((1, 0))}).shape == (0,)


def test_field_table_serves_the_named_planes(tmp_path):
    dims = dict(k=20, samples=100, max_dlas=3, thresholds=2, levels=5, bins=64)
    by_name = {f.name: f for f in grid_fields.fields("absorption_distribution")}
    assert grid_fields.empty(by_name["prob_below"], dims).shape == (2, 0)
    assert grid_fields.empty(by_name["quantiles"], dims).shape == (5, 0)
    assert grid_fields.empty(by_name["histogram"], dims).shape == (64, 0)
    assert grid_fields.empty(by_name["absorption_min"], dims).shape == (0,)
    # a plane without a name keeps max_dlas
    old = {f.name: f for f in grid_fields.fields("model_spectra_multi")}["mean_absorption_models"]
    assert old.leading is None and grid_fields.empty(old, dims).shape == (3, 0)
    parts = [np.arange(6.0).reshape(2, 3), 10 + np.arange(4.0).reshape(2, 2)]
    joined = grid_fields.join(by_name["prob_below"], parts)
    assert joined.shape == (2, 5) and np.array_equal(joined[:, 3:], parts[1])
    assert grid_fields.names("absorption_distribution", options=(None,)) == ("prob_below", "absorption_min", "absorption_max")
    assert [f.name for f in grid_fields.requested("absorption_distribution", ("levels",))] == \
        ["prob_below", "absorption_min", "absorption_max", "quantiles"]

    # the saver: cells of [pixels x D] matrices, and the request beside them
    rng = np.random.default_rng(3)
    off = np.array([0, 4, 4, 9])
    res = dict(selection=np.array([5, 2, 7]), offsets=off, status=np.array([0, 1, 0], dtype=np.int32),
               prob_below=rng.uniform(size=(2, 9)), absorption_min=rng.uniform(size=9), absorption_max=rng.uniform(size=9),
               quantiles=rng.uniform(size=(3, 9)), histogram=rng.uniform(size=(8, 9)))
    path = str(tmp_path / "dist.mat")
    io.save_absorption_distribution(path, res, thresholds=(0.8, 0.5), levels=(0.16, 0.5, 0.84), num_bins=8)
    back = io.loadmat73(path)
    np.testing.assert_array_equal(np.asarray(back["thresholds"]).reshape(-1), [0.8, 0.5])
    np.testing.assert_array_equal(np.asarray(back["levels"]).reshape(-1), [0.16, 0.5, 0.84])
    assert float(np.asarray(back["num_bins"]).reshape(-1)[0]) == 8
    np.testing.assert_array_equal(np.asarray(back["quasar_ind"]).reshape(-1), [6, 3, 8])
    for name, D_ in (("prob_below", 2), ("quantiles", 3), ("histogram", 8)):
        cells = back[name]
        for i in range(3):
            want = res[name][:, off[i]:off[i + 1]].T
            got = np.asarray(cells[i]).reshape(want.shape) if want.size else np.asarray(cells[i])
            assert got.size == want.size
            if want.size:
                np.testing.assert_array_equal(got, want)
    for i in range(3):
        np.testing.assert_array_equal(np.asarray(back["absorption_min"][i]).reshape(-1), res["absorption_min"][off[i]:off[i + 1]])


# ------------------------------------------------------------------------------------------------
# the restatement on the GPU test's inputs
# ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def restated(oracle):
    out = []
    for S in D.SAMPLE_COUNTS:
        cases = [c for c in D.shape_cases() if c[0] == S]
        model, samples, spectra, table = D.case_inputs(S, [c[1] for c in cases], seed=100 + S)
        for (S_, n_u, request), sp, row in zip(cases, spectra, table):
            out.append((S, n_u, request, D.restate_single(oracle, model, samples, sp, row, request)))
    return out


def test_restatement_properties(restated):
    for S, n_u, request, d in restated:
        assert d["absorption_min"].shape == (n_u,)
        F = d["prob_below"]
        order = np.argsort(request["thresholds"])
        assert (np.diff(F[order], axis=0) >= 0).all(), "F is non-decreasing in t"
        assert ((F >= 0) & (F <= 1 + 1e-12)).all()
        assert (d["prob_below_lo"] <= F).all() and (F <= d["prob_below_hi"]).all()
        if "histogram" in d:
            assert np.abs(d["histogram"].sum(axis=0) - 1.0).max() < 1e-12
            assert (d["cumulative_lo"] <= d["cumulative"] + 1e-15).all() and (d["cumulative"] <= d["cumulative_hi"] + 1e-15).all()
        if "quantiles" in d:
            q = d["quantiles"]
            assert (np.diff(q, axis=0) >= 0).all(), "quantiles are non-decreasing in the level"
            assert (q >= d["absorption_min"]).all() and (q <= d["absorption_max"]).all()
            assert (d["quantiles_lo"] <= q).all() and (q <= d["quantiles_hi"]).all()


@pytest.fixture(scope="module")
def restated_further(oracle):
    """The other host-table cases of the GPU test: the production-shape quasar, the three-component mixture, the multi-DLA
    models on tables of their own (products of up to three profiles) and the windows of the scale test."""
    return {"production": D.production_restated(oracle), "mixture": D.mixture_restated(oracle), "multi": D.multi_restated(oracle),
            "scale": D.scale_restated(oracle)}


def test_bounds_are_not_vacuous(restated, restated_further):
    """Over ALL host-table cases the GPU test compares: at most 1 % of the compared entries may have a loose bound."""
    loose = compared = 0
    for S, n_u, request, d in restated:
        l, c = D.loose_counts(d)
        loose, compared = loose + l, compared + c
    print(f"sample and pixel edges: {loose} loose of {compared}")
    for name, ds in restated_further.items():
        l, c = (sum(x) for x in zip(*(D.loose_counts(d) for d in ds)))
        print(f"{name}: {l} loose of {c}")
        loose, compared = loose + l, compared + c
    share = loose / compared
    print(f"loose bounds: {loose} of {compared} compared entries ({100 * share:.3f} %)")
    assert compared > 10000 and share <= 0.01


def test_restatement_properties_of_the_further_cases(restated_further):
    for name, ds in restated_further.items():
        for d in ds:
            assert np.abs(d["histogram"].sum(axis=0) - 1.0).max() < 1e-12, name
            assert (np.diff(d["quantiles"], axis=0) >= 0).all(), name
            assert (d["quantiles"] >= d["absorption_min"]).all() and (d["quantiles"] <= d["absorption_max"]).all(), name
            assert (d["prob_below_lo"] <= d["prob_below"]).all() and (d["prob_below"] <= d["prob_below_hi"]).all(), name
