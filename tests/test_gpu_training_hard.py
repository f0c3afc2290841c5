"""The HIP training objective (csrc/training_mfma_kernels.hpp: k_train_build, k_train_factor / k_train_factor16, k_train_core /
k_train_core_wide, k_train_contract, LY = false and true) against 50-digit arithmetic on the classes of
tests/training_hard_cases.py, one test per class.  With e = objective_deviation(., exact) per block -- f, each column of M,
log omega, each of the three scalars -- the rule is e_gpu <= max(10 x e_oracle, 1e-9), e_oracle from the oracle run in the
same test.  Also: no class reports "not positive definite", every entry is finite, two evaluations agree bit for bit.
The figures measured on the MI355X are the table of DESIGN.md section 5 ("Training objective against exact arithmetic")."""
import numpy as np
import pytest

import training_hard_cases as TC
from test_training import objective_deviation


@pytest.fixture(scope="module")
def fixture(golden):
    return TC.load_fixture(golden)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", TC.CLASSES, ids=TC.class_name)
def test_gpu_objective_against_exact(cls, fixture, oracle):
    from gp_dla_detection_amd import training
    stratum, nq, G, k, lines = cls
    name = TC.class_name(cls)
    e = fixture[name]
    x, F, L1, NV = TC.problem(cls)
    TC.check_digest(cls, e, (x, F, L1, NV))
    f_exact, g_exact = float(e["f"]), e["g"]
    t = training.TrainingSet(F, L1, NV)
    try:
        if lines:
            t.set_lyseries(lines, *(TC.series_tables() if lines == 31 else (None, None)))
        f, g = t.objective(x)          # (raises GpdlaError on any error code: -4 is "not positive definite")
        f2, g2 = t.objective(x)
    finally:
        t.close()
    assert np.isfinite(f) and np.isfinite(g).all() and g.shape == g_exact.shape
    assert f == f2 and np.array_equal(g, g2)
    e_oracle = objective_deviation(*TC.run_oracle(oracle, cls, x, F, L1, NV), f_exact, g_exact, G, k)
    e_gpu = objective_deviation(f, g, f_exact, g_exact, G, k)
    worst = max(e_gpu, key=lambda b: TC.ratio(e_gpu[b], TC.tolerance(e_oracle[b])))
    so, sg = TC.summary(e_oracle, k), TC.summary(e_gpu, k)
    print(f"{name}: cond(B) {float(e['cond_B']):.1e} |f| {abs(f_exact):.2e}  worst block {worst} "
          f"({e_gpu[worst]:.1e} against a bound of {TC.tolerance(e_oracle[worst]):.1e});  e_oracle / e_gpu / ratio  "
          + "  ".join(f"{b} {so[b]:.1e} {sg[b]:.1e} {TC.ratio(sg[b], so[b]):.2g}"
                      for b in ("f", "M", "log_omega", "log_c0", "log_tau0", "log_beta")))
    bad = TC.failures(name, e_gpu, e_oracle)
    assert not bad, bad
