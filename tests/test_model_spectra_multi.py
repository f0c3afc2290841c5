"""CPU-side checks of the model spectra of a multi-DLA run: the restatement the GPU tests compare
against is anchored to the single-profile restatement and, through one-hot rows, to the product of listed absorbers;
request validation without a device; the declared surface; the renormalised model weights."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, api, synthetic

import model_spectra_edge_cases as E
import model_spectra_multi_cases as MC
import model_spectra_multi_restatement as RM
import model_spectra_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def small(oracle):
    """One quasar of 33 pixels, S = 65, its grid and every sample's profile."""
    model, spectra = MC.batch((33,))
    samples = synthetic.make_samples(65)
    g = R.grid(oracle, model, spectra[0])
    return g, samples, RM.sample_profiles(oracle, g, samples["offset_samples"], samples["nhi_samples"], 3)


def test_one_slot_is_the_single_profile_restatement(oracle, small):
    g, samples, _ = small
    S = 65
    base = MC.base_rows("random", S, 4, samples)
    for kind in ("flat", "half_nan", ("hot", 64)):
        row = MC.model_row(kind, S, samples, seed=3)
        want = R.moments(oracle, g, samples["offset_samples"], samples["nhi_samples"], row, 3)
        got = RM.moments_multi(oracle, g, samples["offset_samples"], samples["nhi_samples"], row, base, 1, 3)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kind


@pytest.mark.parametrize("pattern", MC.BASE_PATTERNS)
def test_one_hot_rows_are_the_product_of_the_slots_absorbers(oracle, small, pattern):
    """The independent path that anchors the gather and the slot order: the whole weight on sample i makes mean_n
    the map absorption of the absorbers {s_j(i)}, with no spread."""
    g, samples, profiles = small
    S, md = 65, 4
    base = MC.base_rows(pattern, S, md, samples, seed=5)
    order = E.z_order(samples)
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"]
    for n in range(1, md + 1):
        for p in MC.own_positions(S):
            i = int(order[p])
            row = MC.model_row(("hot", p), S, samples, seed=0)
            mean, var = RM.moments_multi(oracle, g, samples["offset_samples"], samples["nhi_samples"], row, base, n, 3, profiles)
            s = RM.slots(base, n, i)
            assert s[0] == i and len(s) == n and s[1:] == [int(base[j][i]) - 1 for j in range(n - 1)]
            want = R.map_absorption(oracle, g["pad"], z[s], samples["log_nhi_samples"][s], 3)
            d = float(np.abs(mean - want).max())
            print(f"{pattern} model {n} own position {p}: slots {s}: |mean - map| {d:.2e}, max var {var.max():.1e}")
            assert np.isfinite(want).all() and d < 1e-15 and (var == 0.0).all()


def test_base_index_zero_is_a_nan_log_likelihood(oracle, small):
    g, samples, profiles = small
    S, md = 65, 3
    base = MC.base_rows("cyclic", S, md, samples)
    base[1, 7] = 0                                   # slot 3 of sample 7 was never drawn
    row = MC.model_row("flat", S, samples, 0)
    masked = row.copy()
    masked[7] = np.nan
    args = (oracle, g, samples["offset_samples"], samples["nhi_samples"])
    for n, same in ((2, False), (3, True)):          # model 2 does not consume slot 3
        a = RM.moments_multi(*args, row, base, n, 3, profiles)
        b = RM.moments_multi(*args, masked, base, n, 3, profiles)
        assert np.isfinite(a[0]).all() and np.isfinite(b[0]).all()
        assert np.array_equal(a[0], b[0]) == same and np.array_equal(a[1], b[1]) == same
    base[0, :] = 0                                   # every sample of models 2 and 3 consumes a 0: flagged
    for n in (2, 3):
        mean, var = RM.moments_multi(*args, row, base, n, 3, profiles)
        assert np.isnan(mean).all() and np.isnan(var).all()
    assert np.isfinite(RM.moments_multi(*args, row, base, 1, 3, profiles)[0]).all()


def test_model_average_arithmetic():
    rng = np.random.default_rng(4)
    md, n_u = 3, 9
    mb = rng.uniform(0, 1, (1 + md, n_u))
    m2 = mb ** 2 + rng.uniform(0, 0.01, (1 + md, n_u))
    P = np.array([0.4, 0.1, 0.3, 0.0, 0.2])
    ex, var, undefined = RM.model_average(P, mb, m2, [False, False, True, False])      # weight 0 on the flagged model
    assert not undefined and np.allclose(ex, 1 - (0.1 * mb[0] + 0.3 * mb[1] + 0.2 * mb[3]), atol=1e-15) and (var >= 0).all()
    assert RM.model_average(P, mb, m2, [False, True, False, False])[2]                 # weight on a flagged model
    assert RM.model_average([0.5, np.nan, 0.5, 0, 0], mb, m2, [False] * 4)[2]
    ex, var, undefined = RM.model_average([1, 0, 0, 0, 0], mb, m2, [True] * 4)
    assert not undefined and (ex == 1.0).all() and (var == 0.0).all()


# ------------------------------------------------------------------------------------------------
# request validation: before any device call
# ------------------------------------------------------------------------------------------------

def _request(nsel=2, S=8, md=3, host=True, **kw):
    rq = _lib.ModelSpectraMultiRequest()
    rq.num_selected, rq.max_dlas, rq.first_model, rq.last_model = nsel, md, 1, md
    rq.products = _lib.SPECTRA_MULTI_MODELS
    keep = {}
    if host:
        rq.tables_source = _lib.SPECTRA_WEIGHTS_HOST
        keep = dict(sample_log_likelihoods_dla=np.zeros((nsel, md, S)), sample_log_likelihoods_lls=np.zeros((nsel, S)),
                    base_sample_inds=np.ones((nsel, max(md - 1, 1), S), dtype=np.uint32))
    else:
        rq.tables_source = _lib.SPECTRA_WEIGHTS_RESIDENT
    keep.update({k: v for k, v in kw.items() if isinstance(v, np.ndarray)})
    for k, v in list(keep.items()) + [(k, v) for k, v in kw.items() if not isinstance(v, np.ndarray)]:
        if isinstance(v, np.ndarray):
            ct = {np.dtype(np.int64): C.c_int64, np.dtype(np.uint32): C.c_uint32}.get(v.dtype, C.c_double)
            v = v.ctypes.data_as(C.POINTER(ct))
        setattr(rq, k, v)
    return rq, keep


def test_invalid_requests_are_rejected_without_a_device(lib):
    f = lib.gpdla_model_spectra_multi_validate
    nq, S = 5, 8

    def rc(rq, has_lls=1, batch_md=0, processed=0):
        return f(C.byref(rq), nq, S, has_lls, batch_md, processed)

    ok, keep = _request()
    assert rc(ok) == 0                                                  # host tables: any batch will do
    assert rc(ok, batch_md=3, processed=0) == 0
    ok1, keep1 = _request(md=1, base_sample_inds=None)                  # one model: no base table
    assert rc(ok1) == 0
    avg, keep2 = _request(products=_lib.SPECTRA_MULTI_MODELS | _lib.SPECTRA_MULTI_AVERAGE, model_weights=np.full((2, 5), 0.2))
    assert rc(avg) == 0
    res, _ = _request(host=False, products=_lib.SPECTRA_MULTI_AVERAGE)   # resident: model_posteriors weigh the models
    assert rc(res, batch_md=3, processed=1) == 0

    bad = []
    for first, last in ((0, 3), (1, 4), (3, 2)):
        bad.append(_request(first_model=first, last_model=last))
    bad.append(_request(md=0))
    bad.append(_request(md=5))
    for missing in ("sample_log_likelihoods_dla", "sample_log_likelihoods_lls", "base_sample_inds"):
        bad.append(_request(**{missing: None}))
    over = np.ones((2, 2, S), dtype=np.uint32)
    over[1, 1, 3] = S + 1
    bad.append(_request(base_sample_inds=over))
    bad.append(_request(products=_lib.SPECTRA_MULTI_AVERAGE))            # host tables, no weights
    bad.append(_request(products=0))
    bad.append(_request(products=4))
    bad.append(_request(tables_source=_lib.SPECTRA_WEIGHTS_NONE))
    bad.append(_request(selection=np.array([0, 5], dtype=np.int64)))
    bad.append(_request(num_selected=-1))
    for rq, _keep in bad:
        assert rc(rq) == _lib.ERR_INVALID_ARGUMENT, lib.gpdla_last_error()
        assert lib.gpdla_last_error()
    at_s = np.full((2, 2, S), S, dtype=np.uint32)
    at_s[0, 0, 0] = 0
    edge, _k = _request(base_sample_inds=at_s)                           # 0 and S are indices
    assert rc(edge) == 0
    assert rc(ok, has_lls=0) == _lib.ERR_INVALID_ARGUMENT                # the sub-DLA model needs its column densities
    # a resident source
    assert rc(res, batch_md=0, processed=0) == _lib.ERR_INVALID_ARGUMENT and b"multi-DLA batch" in lib.gpdla_last_error()
    assert rc(res, batch_md=3, processed=0) == _lib.ERR_INVALID_ARGUMENT and b"processed" in lib.gpdla_last_error()
    assert rc(res, batch_md=4, processed=1) == _lib.ERR_INVALID_ARGUMENT
    del keep, keep1, keep2


# ------------------------------------------------------------------------------------------------
# the declared surface
# ------------------------------------------------------------------------------------------------

def test_header_declares_the_entries_under_abi_6(lib):
    with open(os.path.join(ROOT, "include", "gpdla.h")) as f:
        header = f.read()
    assert re.search(r"#define GPDLA_ABI_VERSION 6\b", header) and lib.gpdla_abi_version() == 6
    for name in ("gpdla_model_spectra_multi_validate", "gpdla_batch_model_spectra_multi"):
        assert re.search(rf"\bint {name}\(", header), name
        assert getattr(lib, name)
    for name in ("gpdla_model_spectra_multi_request", "gpdla_model_spectra_multi", "GPDLA_SPECTRA_MULTI_MODELS",
                 "GPDLA_SPECTRA_MULTI_AVERAGE", "GPDLA_SPECTRA_AVERAGE_UNDEFINED"):
        assert name in header
    # the structures of the binding follow the header's field order
    for struct, cls in (("gpdla_model_spectra_multi_request", _lib.ModelSpectraMultiRequest),
                        ("gpdla_model_spectra_multi", _lib.ModelSpectraMulti)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", header).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(None, 1)[1] if decl.strip() else "")]
        assert names == [n for n, _ in cls._fields_], (struct, names)


def test_python_surface_exists():
    import inspect
    sig = inspect.signature(gp.Batch.model_spectra_multi)
    for name in ("selection", "tables", "model_weights", "models", "products", "meanflux"):
        assert name in sig.parameters
    assert sig.parameters["tables"].default == "resident"
    assert inspect.signature(api.model_spectra).parameters["multi_models"].default is False
    from gp_dla_detection_amd import model_spectra as cli
    with pytest.raises(SystemExit) as e:
        cli.main(["--help"])
    assert e.value.code == 0
    ap_source = inspect.getsource(cli.main)
    assert '"--multi-models"' in ap_source


def test_renormalised_model_posteriors():
    md = 3
    res = dict(log_posteriors_no_dla=np.array([-10.0, -3.0, np.nan]), log_posteriors_lls=np.array([-12.0, -4.0, np.nan]),
               log_posteriors_dla=np.array([[-9.0, -11.0, -15.0], [-2.0, np.nan, np.nan], [np.nan] * md]))
    P = gp.renormalised_model_posteriors(res)
    assert P.shape == (3, 2 + md)
    lp = np.array([-10.0, -12.0, -9.0, -11.0, -15.0])
    np.testing.assert_allclose(P[0], np.exp(lp - lp.max()) / np.exp(lp - lp.max()).sum(), rtol=1e-15)
    # the early exit after DLA(1) (multi :460-464): the models it did not reach are NaN, and so is the saved row
    assert abs(P[1].sum() - 1.0) < 1e-15 and (P[1, 3:] == 0.0).all() and (P[1, :3] > 0).all()
    np.testing.assert_allclose(P[1, :3], np.exp([-1.0, -2.0, 0.0]) / np.exp([-1.0, -2.0, 0.0]).sum(), rtol=1e-15)
    assert np.isnan(P[2]).all()                     # nothing was evaluated: nothing to renormalise
