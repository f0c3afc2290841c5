"""The HIP learning front end (csrc/learn_kernels.hpp: k_learn_rest_grid, k_learn_colsum / k_learn_colfinish, k_learn_center,
k_learn_rowflag, k_learn_gram / k_learn_gram_finish) against 50-digit arithmetic on the classes of tests/learn_hard_cases.py,
one test per class.  With e = learn_hard_cases.deviation(., exact) per block -- rest flux, lya_1pzs, rest noise, mu, centred
flux, std, pairwise and complete-rows covariance -- the rule is e_gpu <= max(10 x e_restatement, floor), e_restatement from
the numpy restatement run in the same test and the floors the bounds of test_gpu_learn.py.  Also: NaN placement, +-inf
placement with sign, the count vector and the count matrices equal the fixture's exactly; std is finite and >= 0 wherever
two quasars are, and its logarithm finite on the ulp-scattered columns; two handles agree bit for bit.
The figures measured on the MI355X are the "Checks" table of DESIGN.md section 4.10."""
import numpy as np
import pytest

import learn_hard_cases as LC


@pytest.fixture(scope="module")
def fixture(golden):
    return LC.load_fixture(golden)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", LC.CLASSES, ids=LC.class_name)
def test_gpu_front_end_against_exact(cls, fixture):
    exact = fixture[LC.class_name(cls)]
    csr, p = LC.problem(cls)
    LC.check_digest(cls, exact, csr, p)
    got, again = LC.evaluate(csr, p, cls[1]), LC.evaluate(csr, p, cls[1])
    for key in got:
        assert np.array_equal(got[key], again[key], equal_nan=True), f"two handles differ in {key}"
    e_rest = LC.deviation(LC.restated(cls, csr, p), exact)
    e_gpu = LC.deviation(got, exact)
    print(LC.report(cls, e_gpu, e_rest))
    bad = LC.patterns(got, exact)
    assert not bad, bad
    n_c = float(exact["rows_complete"])
    assert np.array_equal(got["N_complete"], np.full_like(got["N_complete"], n_c))
    for key in ("cov_pairwise", "cov_complete"):
        assert np.array_equal(got[key], got[key].T, equal_nan=True)
    some = exact["count"] >= 1
    assert np.all(np.isfinite(got["std"][some])) and np.all(got["std"][some] >= 0.0)
    if cls[0] == "constant_columns":
        assert np.all(got["std"][list(LC.CONST_COLUMNS)] == 0.0)
        assert np.all(np.isfinite(np.log(got["std"][list(LC.ULP_COLUMNS)])))
    bad = LC.failures(cls, e_gpu, e_rest)
    assert not bad, bad
