"""The sweeps and the stand-alone low-rank function against 50-digit arithmetic where the arithmetic is hard
(tests/hard_conditioning_cases.py; tests/golden/exact_hard_conditioning.npz): S/N 100 .. 1000, a mixed, five times
larger model with two nearly collinear columns (cond(B) ~ 5e6), fluxes the model does not fit (|log-likelihood| up to
1e7), saturated absorbers whose absorption is exactly 0 over more than half the spectrum, and fewer kept pixels than
the rank.  There a faithful fp64 evaluation of log_mvnpdf_low_rank.m:11-32 is itself 1e-9 .. 1e-6 from the exact value,
so the project's 1e-8 says nothing.  The rule here, per class:

    e_gpu = max |GPU - exact| over the null model and all 65 samples (multi-DLA: the sub-DLA table and both models too)
    e_gpu <= max(10 x e_oracle, 1e-9),  e_oracle = the as-written fp64 oracle's worst error on the SAME class

10 x is the project's convention (R.continuum_tolerance, posterior_restatement.tolerances); 1e-9 is what the two older
exact fixtures hold the HIP path to; ``control`` (the shipped model and noise) must also still meet the plain 1e-9.  No
case may pass on NaN: status 0, every table finite exactly where the exact one is.  MAP columns equal the oracle's
(test_hard_conditioning.py shows that no class has its two largest exact values within twice the tolerance).  The slim
kernels stay bit-identical with the pre-expanded ones of libgpdla_legacy.so on the correlated model at k = 20 and 40.

Kernels: k_sweep_slim<3>, k_sweep_slim<0> (31 lines), k_sweep_split_slim (k = 33, 40), k_profiles +
k_sweep_multi_slim<1>, <2> + the sub-DLA sweep, k_lowrank_single.  Hot loops: process_qsos.m:185-199,
process_qsos_multiple_dlas_meanflux.m:340-381."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
import hard_conditioning_cases as H

pytestmark = pytest.mark.gpu

TOL_Z = 1e-14     # production_shapes.TOL_Z: min / max z_DLA and the MAP redshifts
_got = {}


def got_case(cls):
    """the product library's result of a class, computed once and shared"""
    if cls not in _got:
        out = H.run_gpu(H.build_case(cls))
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _got[cls] = out
    return _got[cls]


def ratio(e_gpu, e_oracle):
    return e_gpu / e_oracle if e_oracle > 0 else float("inf")


@pytest.fixture(scope="module")
def fixture(golden):
    return H.load_fixture(golden)


@pytest.mark.parametrize("cls", H.CLASSES, ids=H.class_name)
def test_class_against_exact_arithmetic(cls, fixture):
    name = H.class_name(cls)
    e = fixture[name]
    exact, stored = H.stored_values(e, "exact_"), H.stored_values(e, "oracle_")
    got = got_case(cls)
    assert (np.asarray(got["status"]) == 0).all(), got["status"]
    assert abs(got["min_z_dlas"][0] - float(e["min_z_dla"])) < TOL_Z
    assert abs(got["max_z_dlas"][0] - float(e["max_z_dla"])) < TOL_Z
    for t, v in exact.items():   # finite exactly where the exact values are: nothing passes on NaN
        assert np.array_equal(np.isfinite(got[t]), np.isfinite(v)), (name, t)
    assert np.isfinite(exact["dla"]).all() and np.isfinite(got["log_likelihoods_dla"]).all()
    failures, e_gpu, e_oracle, tol = H.class_failures(name, got, exact, stored,
                                                      extra_bound=H.TOL_FLOOR if cls[0] == "control" else None)
    largest = max(float(np.nanmax(np.abs(v))) for v in exact.values())
    print(f"{name}: cond(B) {float(e['cond_B']):.2e}, max |ll| {largest:.2e}, e_oracle {e_oracle:.3e}, e_gpu {e_gpu:.3e}, "
          f"ratio {ratio(e_gpu, e_oracle):.2f}, tolerance {tol:.3e}")
    assert not failures, failures
    # MAP columns: the oracle's
    if cls[1] == "single":
        i = int(np.argmax(stored["dla"]))
        assert got["MAP_inds"][0] == i + 1.0
        assert abs(got["MAP_z_dlas"][0] - e["sample_z_dlas"][i]) < TOL_Z
        assert abs(got["MAP_log_nhis"][0] - e["log_nhi_samples"][i]) < 1e-12
    else:
        np.testing.assert_array_equal(got["MAP_inds"][0], e["oracle_MAP_inds"])
        np.testing.assert_allclose(got["MAP_z_dlas"][0], e["oracle_MAP_z_dlas"], rtol=0, atol=TOL_Z, equal_nan=True)
        np.testing.assert_allclose(got["MAP_log_nhis"][0], e["oracle_MAP_log_nhis"], rtol=0, atol=1e-12, equal_nan=True)
        np.testing.assert_array_equal(got["base_sample_inds"][0], e["base_sample_inds"])


@pytest.mark.parametrize("k", H.LOWRANK_KS)
def test_low_rank_function_against_exact_arithmetic(k, fixture):
    """gpdla_log_mvnpdf_low_rank on hand-made inputs, n = 128, two columns collinear to 1e-6, cond(B) 1e4, 1e8, 1e12:
    the linear algebra alone, no Voigt profile in it"""
    bad = []
    for c in H.LOWRANK_CONDS:
        name = H.lowrank_name(k, c)
        e = fixture[name]
        got = dict(null=gp.log_mvnpdf_low_rank(e["y"], e["mu"], e["M"], e["d"]))
        failures, e_gpu, e_oracle, tol = H.class_failures(name, got, H.stored_values(e, "exact_"), H.stored_values(e, "oracle_"))
        print(f"{name}: cond(B) {float(e['cond_B']):.2e}, |ll| {abs(float(e['exact_null'])):.2e}, e_oracle {e_oracle:.3e}, "
              f"e_gpu {e_gpu:.3e}, ratio {ratio(e_gpu, e_oracle):.2f}, tolerance {tol:.3e}")
        bad += failures
    assert not bad, bad


def test_slim_records_stay_bit_identical_on_the_correlated_model(tmp_path):
    """k_sweep_slim<3> and k_sweep_split_slim against k_sweep / k_sweep_split on the pre-expanded records
    (libgpdla_legacy.so with GPDLA_EXPANDED_RECORDS=1 in a clean child, as test_gpu_sweep_chunk_edges.py): the same
    products and the same MFMA sequence per column, so every output is bit-identical here too"""
    from gp_dla_detection_amd import _lib
    classes = [("correlated", "single", 20, 3), ("correlated", "single", 40, 3)]
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    env = {"GPDLA_EXPANDED_RECORDS": "1", "GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH}
    out = tmp_path / "expanded.npz"
    pr = mp.get_context("forkserver").Process(target=H.run_gpu_child, args=(classes, env, str(out)))
    pr.start()
    pr.join(600)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
    assert pr.exitcode == 0
    want = np.load(out)
    for cls in classes:
        got, prefix, checked = got_case(cls), H.class_name(cls) + "/", 0
        assert np.isfinite(got["sample_log_likelihoods_dla"]).all()
        for full in want.files:
            if not full.startswith(prefix):
                continue
            a, b = np.asarray(got[full[len(prefix):]]), want[full]
            assert a.shape == b.shape, full
            if a.dtype.kind == "f":
                assert np.array_equal(a, b, equal_nan=True), (full, float(np.nanmax(np.abs(a - b))))
            else:
                assert np.array_equal(a, b), full
            checked += 1
        assert checked >= 10, (cls, checked)
