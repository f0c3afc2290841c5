"""The exact fixture of the training objective (tests/golden/exact_training_hard.npz and exact_training_hard_k33_k40.npz,
made by tests/golden/make_exact_training_hard.py from tests/training_hard_cases.py) on the CPU: the inputs are the ones the
exact values were computed on, the stored central differences of the exact value confirm the exact gradient, the
as-written fp64 oracle stays within its cap of the 50-digit values in every block of every class, the comparison the GPU
test uses notices noise variances rounded to float32 in every hard class, and an fp64 restatement of the HIP kernels'
algebra shows where that algebra lost digits before the core contracted B^-1.  Figures of the committed fixture are in LABBOOK.md ("Training objective
against exact arithmetic")."""
import numpy as np
import pytest

import training_hard_cases as TC
from test_training import objective_deviation, training_problem

NAMES = [TC.class_name(cls) for cls in TC.CLASSES]


@pytest.fixture(scope="module")
def fixture(golden):
    return TC.load_fixture(golden)


_cache = {}


def inputs(cls):
    if cls not in _cache:
        _cache[cls] = TC.problem(cls)
    return _cache[cls]


def oracle_errors(oracle, fixture, cls, NV=None):
    """objective_deviation(oracle, exact) per block; ``NV`` replaces the noise variances"""
    e = fixture[TC.class_name(cls)]
    x, F, L1, nv = inputs(cls)
    key = (cls, "oracle", NV is None)
    if key not in _cache:
        f, g = TC.run_oracle(oracle, cls, x, F, L1, nv if NV is None else NV)
        _cache[key] = objective_deviation(f, g, float(e["f"]), e["g"], cls[2], cls[3])
    return _cache[key]


def test_classes_are_the_ones_the_kernels_need():
    assert len(TC.CLASSES) == len(set(TC.CLASSES)) == 19
    assert {c[0] for c in TC.CLASSES if c[1:] == TC.SHAPE20 + (0,)} == set(TC.STRATA) and len(TC.STRATA) == 11
    assert {c[0] for c in TC.CLASSES if c[1:] == TC.SHAPE40 + (0,)} == {"correlated", "bad_continuum", "high_snr", "few_pixels"}
    assert {c[0] for c in TC.CLASSES if c[1:] == TC.SHAPE33 + (0,)} == {"correlated", "omega_tiny"}
    assert [c for c in TC.CLASSES if c[4]] == [("correlated",) + TC.SHAPE20 + (6,), ("high_snr",) + TC.SHAPE33 + (31,)]
    for _, nq, G, k, _ in TC.CLASSES:      # ragged in the 16-quasar and 16-pixel tilings, more than one group of each
        assert nq % 16 and G % 16 and nq > 16 and G > 16


def test_control_is_training_problem_and_every_class_carries_the_edges():
    cls = TC.CLASSES[0]
    assert cls[0] == "control"
    x, F, L1, NV = inputs(cls)
    x0, F0, L10, NV0 = training_problem(nq=cls[1], G=cls[2], k=cls[3], seed=TC.BASE_SEED)
    assert np.array_equal(x, x0) and np.array_equal(L1, L10) and np.array_equal(NV, NV0)
    same = ~np.isnan(F)
    same[TC.ONE_PIXEL_QUASAR, TC.ONE_PIXEL] = False        # (0.0 if training_problem had it missing)
    assert np.array_equal(F[same], F0[same]) and not np.isnan(F0[same]).any()
    for cls in TC.CLASSES:
        stratum, nq, G, k, lines = cls
        x, F, L1, NV = inputs(cls)
        valid = ~np.isnan(F)
        assert x.shape == (G * (k + 1) + 3,) and F.shape == L1.shape == NV.shape == (nq, G)
        assert np.isfinite(x).all() and np.isfinite(L1).all() and (NV > 0).all() and (L1 > 1).all()
        assert not valid[TC.ALL_NAN_QUASAR].any()
        assert np.flatnonzero(valid[TC.ONE_PIXEL_QUASAR]).tolist() == [TC.ONE_PIXEL]
        assert not valid[TC.GROUP_QUASAR, 16 * TC.GROUP:16 * TC.GROUP + 16].any() and valid[TC.GROUP_QUASAR].any()
        assert not valid[:, TC.MISSING_PIXEL].any()
        assert valid.sum(axis=0)[np.arange(G) != TC.MISSING_PIXEL].min() >= 2      # every other pixel is observed
        few = valid.sum(axis=1) < k
        if TC.STRATA[stratum]["few"]:
            assert few.sum() >= nq // 2 and (valid.sum(axis=1)[~few] > G // 2).all()
        else:
            assert few.sum() == 2                                                  # the all-NaN and the one-pixel quasar
            assert 0.05 < 1 - valid[~few].mean() < 0.2
        if TC.STRATA[stratum]["quiet"]:
            assert (NV[:, TC.QUIET_PIXEL] == 1e-10).all() and valid[:, TC.QUIET_PIXEL].sum() > nq // 2
        if lines:
            assert (np.diff(L1, axis=1) > 0).all()                                 # the last column is 1 + z_qso
        # (1+z)^beta stays far from overflow, and the forest strata are what they claim
        od = np.stack([TC.optical_depth(cls, np.exp(x[-2]), np.exp(x[-1]), L1[q]) for q in range(nq)])
        assert np.isfinite(od).all()
        if stratum == "opaque_forest":
            assert 5e3 < od.min() and od.max() < 5e4 and (np.exp(-od) == 0).all()
        if stratum == "thin_forest":
            assert od.max() < 1e-12 and (1 - np.exp(-od) < 1e-12).all()


@pytest.mark.parametrize("cls", TC.CLASSES, ids=TC.class_name)
def test_inputs_are_the_ones_the_exact_values_belong_to(cls, fixture):
    assert sorted(fixture) == sorted(NAMES)
    TC.check_digest(cls, fixture[TC.class_name(cls)], inputs(cls))


def test_finite_differences_of_the_exact_value_confirm_the_exact_gradient(fixture):
    """The generator asserts, at 50 digits, that central differences of the exact value (step 1e-15) agree with the closed
    form without the prior terms to 1e-20 relative; both were rounded to fp64 when stored, so here they agree to two
    roundings, on the sampled entries (at least 8 of M, 4 of log omega, the scalars), and the stored gradient is the
    closed form plus the stored prior terms."""
    for cls in TC.CLASSES:
        _, nq, G, k, lines = cls
        e = fixture[TC.class_name(cls)]
        idx, fd, closed, g, prior = e["fd_index"], e["fd"], e["fd_closed"], e["g"], e["prior"]
        assert np.array_equal(idx, TC.fd_indices(cls))
        assert (idx < G * k).sum() >= 8 and ((idx >= G * k) & (idx < G * (k + 1))).sum() >= 4
        assert idx[-1] == G * (k + 1) + (1 if lines else 2)
        assert g.shape == (G * (k + 1) + 3,) and np.isfinite(g).all() and np.isfinite(float(e["f"]))
        # FD_ATOL |f|: what a difference of two 50-digit values over 2e-15 cannot resolve (opaque_forest's log tau0: 0 against 1e-2600)
        assert (np.abs(fd - closed) <= 2.0 ** -51 * np.abs(closed) + TC.FD_ATOL * abs(float(e["f"]))).all(), TC.class_name(cls)
        assert np.count_nonzero(closed) == closed.size - (2 if cls[0] == "opaque_forest" else 0)      # (e^-tau = 1e-2600)
        full = closed.copy()
        for i, j in enumerate(idx):
            if j >= G * (k + 1) + 1:
                full[i] += prior[j - G * (k + 1) - 1]
        np.testing.assert_allclose(full, g[idx], rtol=2.0 ** -50, atol=0)
        assert (np.abs(prior - TC.prior_terms(inputs(cls)[0])) <= 1e-12 * np.maximum(1, np.abs(prior))).all()


@pytest.mark.parametrize("cls", TC.CLASSES, ids=TC.class_name)
def test_oracle_stays_under_its_cap(cls, fixture, oracle):
    """A condition on the choice of inputs, not a measurement: the as-written fp64 oracle is within ORACLE_CAP of the exact
    value in every block, so that 10 x its error is a bound that still says something; and no block of the exact gradient
    is identically 0 (the measure divides by the block's largest entry)."""
    e = fixture[TC.class_name(cls)]
    G, k = cls[2], cls[3]
    g = e["g"]
    blocks = [g[c * G:(c + 1) * G] for c in range(k + 1)] + [g[(k + 1) * G + i:(k + 1) * G + i + 1] for i in range(3)]
    assert float(e["f"]) != 0 and all(np.abs(b).max() > 0 for b in blocks)
    dev = oracle_errors(oracle, fixture, cls)
    s = TC.summary(dev, k)
    print(f"{TC.class_name(cls)}: cond(B) {float(e['cond_B']):.1e} |f| {abs(float(e['f'])):.2e}  oracle f {s['f']:.1e} M {s['M']:.1e} "
          f"(column {s['M_col']}) log_omega {s['log_omega']:.1e} c0 {s['log_c0']:.1e} tau0 {s['log_tau0']:.1e} beta {s['log_beta']:.1e}")
    bad = {b: v for b, v in dev.items() if not v <= TC.ORACLE_CAP}
    assert not bad, (TC.class_name(cls), bad)
    if cls[0] == "opaque_forest":      # the prior terms ARE the log tau0 and log beta entries there
        assert abs(e["prior"][0] - g[-2]) <= 1e-9 * abs(g[-2]) and abs(e["prior"][1] - g[-1]) <= 1e-9 * abs(g[-1])


def test_comparison_notices_float32_noise_variances(fixture, oracle):
    """The oracle itself passes the rule the GPU is held to; fed noise variances rounded to float32 (a relative 6e-8 on
    every d that the noise dominates) it fails in every hard class but ``omega_large`` and ``opaque_forest``, where the noise
    is little beside omega2 sf^2 and log omega rounded to float32 takes its place, and so does a NaN in one entry."""
    for cls in TC.CLASSES:
        name = TC.class_name(cls)
        e_oracle = oracle_errors(oracle, fixture, cls)
        assert TC.failures(name, e_oracle, e_oracle) == []
        NV = inputs(cls)[3]
        e32 = oracle_errors(oracle, fixture, cls, NV.astype(np.float32).astype(np.float64))
        bad = TC.failures(name, e32, e_oracle)
        worst = max(TC.ratio(e32[b], TC.tolerance(e_oracle[b])) for b in e32)
        print(f"{name}: float32 noise variances fail {len(bad)} of {len(e32)} blocks; worst error / tolerance {worst:.3g}")
        if cls[0] in TC.NOISE_BLIND_STRATA:        # the noise is a few per cent of d at the most: log omega rounded to float32 instead
            x, F, L1, _ = inputs(cls)
            G, k = cls[2], cls[3]
            od = np.stack([TC.optical_depth(cls, np.exp(x[-2]), np.exp(x[-1]), L1[q]) for q in range(cls[1])])
            an = np.exp(2 * x[G * k:G * (k + 1)]) * (1 - np.exp(-od) + np.exp(x[-3])) ** 2
            assert not bad and (NV / an).max() < 0.05 and np.median(NV / an) < 2e-3
            x32 = x.copy()
            x32[G * k:G * (k + 1)] = x32[G * k:G * (k + 1)].astype(np.float32)
            e = fixture[name]
            e32 = objective_deviation(*TC.run_oracle(oracle, cls, x32, F, L1, NV), float(e["f"]), e["g"], G, k)
            bad = TC.failures(name, e32, e_oracle)
            print(f"{name}: float32 log omega fails {len(bad)} of {len(e32)} blocks")
        if cls[0] in TC.HARD_STRATA:
            assert bad, (name, worst)
    cls = TC.CLASSES[1]
    e = fixture[TC.class_name(cls)]
    g = e["g"].copy()
    g[7] = np.nan
    broken = objective_deviation(float(e["f"]), g, float(e["f"]), e["g"], cls[2], cls[3])
    assert TC.failures("nan", broken, oracle_errors(oracle, fixture, cls)) and broken["M[:, 0]"] == np.inf


RESTATED = tuple(c for c in TC.CLASSES if c[1:] == TC.SHAPE20 + (0,)) + (("correlated",) + TC.SHAPE40 + (0,),)


def test_restatement_of_the_gpu_algebra_loses_digits_where_T_is_contracted(fixture, oracle):
    """``TC.gpu_algebra`` restates in fp64 the forms of csrc/training_mfma_kernels.hpp, with B^-1 contracted for diag K^-1
    (as shipped) or T = B^-1 + z z' (as before these tests).  Recovering m'B^-1 m as m'T m - (m'z)^2 costs
    log10((m'z)^2 / m'B^-1 m) digits of (K^-1)_pp: contracting B^-1 lowers the error of the log omega block where S/N is
    high.  Reported per class; asserted on the three strata in which the cancellation is the block's leading error, and
    that on ``omega_tiny`` the T form breaks the rule the GPU is held to while the B^-1 form keeps it."""
    for cls in RESTATED:
        e = fixture[TC.class_name(cls)]
        G, k = cls[2], cls[3]
        dev = {form: objective_deviation(*TC.gpu_algebra(cls, *inputs(cls), contract=form), float(e["f"]), e["g"], G, k)
               for form in ("T", "Binv")}
        o = TC.summary(oracle_errors(oracle, fixture, cls), k)
        t, b = TC.summary(dev["T"], k), TC.summary(dev["Binv"], k)
        print(f"{TC.class_name(cls)}: oracle / T form / B^-1 form  f {o['f']:.1e} {t['f']:.1e} {b['f']:.1e}  M {o['M']:.1e} {t['M']:.1e} "
              f"{b['M']:.1e}  log_omega {o['log_omega']:.1e} {t['log_omega']:.1e} {b['log_omega']:.1e}  "
              f"c0 {o['log_c0']:.1e} {t['log_c0']:.1e} {b['log_c0']:.1e}  tau0 {o['log_tau0']:.1e} {t['log_tau0']:.1e} {b['log_tau0']:.1e}  "
              f"beta {o['log_beta']:.1e} {t['log_beta']:.1e} {b['log_beta']:.1e}")
        assert all(np.isfinite(v) for form in dev for v in dev[form].values())
        assert dev["T"]["f"] == dev["Binv"]["f"] and all(dev["T"][f"M[:, {c}]"] == dev["Binv"][f"M[:, {c}]"] for c in range(k))
        if cls[0] in TC.BINV_LOWERS_LOG_OMEGA:
            assert dev["Binv"]["log_omega"] < 0.1 * dev["T"]["log_omega"], (cls, dev["T"]["log_omega"], dev["Binv"]["log_omega"])
        if cls[0] == "omega_tiny":
            e_oracle = oracle_errors(oracle, fixture, cls)
            assert "log_omega" in " ".join(TC.failures("T", dev["T"], e_oracle)) and not TC.failures("Binv", dev["Binv"], e_oracle)
