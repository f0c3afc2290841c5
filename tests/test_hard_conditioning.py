"""The hard-conditioning fixture (tests/golden/exact_hard_conditioning.npz, made by tests/golden/make_exact_hard.py
from tests/hard_conditioning_cases.py) on the CPU: the inputs and the oracle reproduce, the oracle stays within its
cap of the 50-digit values, the hard classes are hard, no MAP index hangs on a near-tie, and the comparison the GPU
tests use notices a loss of precision.  Figures of the committed fixture (worst |oracle - exact| per class):
control 2.3e-12; high S/N 7e-8; the correlated model 4e-7 .. 9e-7; the stand-alone function 1.4e-12 / 1.6e-8 / 1.3e-4
at cond(B) 1e4 / 1e8 / 1e12.  Hot loops: process_qsos.m:185-199, log_mvnpdf_low_rank.m:11-32."""
import numpy as np
import pytest

import hard_conditioning_cases as H

TINY = np.finfo(np.float64).tiny


@pytest.fixture(scope="module")
def fixture(golden):
    return H.load_fixture(golden)


@pytest.fixture(scope="module")
def cases():
    return {H.class_name(cls): H.build_case(cls) for cls in H.CLASSES}


@pytest.fixture(scope="module")
def runs(oracle, cases):
    return {name: H.run_oracle(oracle, case) for name, case in cases.items()}


def e_oracle(entry) -> float:
    return H.worst_error(H.stored_values(entry, "oracle_"), H.stored_values(entry, "exact_"))


def test_fixture_holds_every_class(fixture):
    names = [H.class_name(cls) for cls in H.CLASSES] + [H.lowrank_name(k, c) for k in H.LOWRANK_KS for c in H.LOWRANK_CONDS]
    assert sorted(fixture) == sorted(names) and len(set(names)) == 13 + 12
    for cls in H.CLASSES:
        e = fixture[H.class_name(cls)]
        tables = ("dla", "lls", "dla2") if cls[1] == "multi" else ("dla",)
        assert np.isfinite(e["exact_null"]) and all(e["exact_" + t].shape == (H.S,) for t in tables)
        assert np.isfinite(e["exact_dla"]).all()           # the null model and ALL 65 samples
        if cls[1] == "multi":
            assert np.isfinite(e["exact_lls"]).all() and np.isfinite(e["exact_dla2"]).sum() >= H.S // 2


def test_inputs_reproduce(fixture, cases):
    """the regenerated cases equal the stored inputs bit for bit"""
    for name, case in cases.items():
        e, sp, sm = fixture[name], case["spectrum"], case["samples"]
        for key in ("wavelengths", "noise_variance", "pixel_mask"):
            np.testing.assert_array_equal(sp[key], e[key], err_msg=f"{name} {key}")
        np.testing.assert_array_equal(np.nan_to_num(sp["flux"]), np.nan_to_num(e["flux"]), err_msg=name)
        assert sp["z_qso"] == float(e["z_qso"])
        for key in ("offset_samples", "log_nhi_samples", "nhi_samples", "lls_nhi_samples"):
            np.testing.assert_array_equal(sm[key], e[key], err_msg=f"{name} {key}")
        if case["bsi"] is not None:
            np.testing.assert_array_equal(case["bsi"], e["base_sample_inds"])
        # the shape every stratum shares: 131 in-range pixels = 33 K-steps, masked the way preload_qsos.m leaves them
        inside = H.in_range(sp)
        masked = sp["pixel_mask"] == 1
        assert inside.sum() == H.N_PIX and -(-H.N_PIX // 4) == 33 and sm["offset_samples"].size == H.S
        assert np.isnan(sp["flux"][masked]).all() and np.isinf(sp["noise_variance"][masked]).all()
        assert np.isfinite(sp["flux"][~masked]).all()
        if case["cls"][0] == "few_pixels":
            assert (inside & ~masked).sum() == H.FEW_KEPT < case["cls"][2]
        else:
            assert masked.sum() == 5 and np.ptp(np.flatnonzero(masked)) == 4
    for k, c, y, mu, M, d in H.lowrank_cases():
        e = fixture[H.lowrank_name(k, c)]
        for key, v in (("y", y), ("mu", mu), ("M", M), ("d", d)):
            np.testing.assert_array_equal(v, e[key], err_msg=f"{k} {c} {key}")
        assert M.shape == (H.LOWRANK_N, k) and np.abs(M[:, 1] / M[:, 0] - 1).max() < 1e-3
        assert c / 3 < float(e["cond_B"]) < 3 * c and c / 3 < H.cond_B(y, mu, M, d) < 3 * c


def test_oracle_reproduces(fixture, cases, runs, oracle):
    """The oracle gives its stored values, from the stored intermediates.  The exact values belong to the STORED
    rows and absorption vectors, and every comparison uses the stored ones; this test shows that the fixture is what
    the generator makes.  The regenerated intermediates may differ from them by the last bits of another libm's exp,
    log and pow (1e-13 relative, the rule of test_golden_spectrum_config1; below 1e-290, where a denormal holds few
    bits, absolutely), which moves a log-likelihood of 1e7 by less than 1e-8; the oracle's values then come back to
    within a twentieth of the class's own error (floored at 1e-11: an ulp of |ll| = 5e3 is 9e-13)."""
    close = dict(rtol=1e-13, atol=1e-290)
    identical = True
    for name, case in cases.items():
        e, r = fixture[name], runs[name]
        for key in ("this_mu", "this_M", "this_omega2", "padded_wavelengths", "sample_z_dlas"):
            np.testing.assert_allclose(r[key], e[key], err_msg=f"{name} {key}", **close)
        assert abs(r["min_z_dla"] - float(e["min_z_dla"])) < 1e-15 and abs(r["max_z_dla"] - float(e["max_z_dla"])) < 1e-15
        assert r["n_kept"] == int(e["n_kept"]) and r["n_unmasked"] == int(e["n_unmasked"]) == H.N_PIX
        tabs = H.absorption_tables(oracle, case, r)
        np.testing.assert_allclose(tabs["dla"], e["absorption_dla"], err_msg=name, **close)
        assert np.array_equal(tabs["dla"] == 0, e["absorption_dla"] == 0)
        identical &= np.array_equal(tabs["dla"], e["absorption_dla"]) and np.array_equal(r["this_M"], e["this_M"])
        if case["bsi"] is not None:
            np.testing.assert_allclose(tabs["lls"], e["absorption_lls"], err_msg=name, **close)
            np.testing.assert_array_equal(r["MAP_inds"], e["oracle_MAP_inds"], err_msg=name)
            np.testing.assert_allclose(r["MAP_z_dlas"], e["oracle_MAP_z_dlas"], rtol=0, atol=1e-15, equal_nan=True)
            np.testing.assert_array_equal(r["MAP_log_nhis"], e["oracle_MAP_log_nhis"], err_msg=name)
        bound = max(0.05 * e_oracle(e), 1e-11)
        for t, v in H.stored_values(e, "oracle_").items():
            assert np.array_equal(np.isfinite(r[t]), np.isfinite(v)), (name, t)
            d = np.abs(np.asarray(r[t]) - v)
            identical &= np.array_equal(r[t], v, equal_nan=True)
            assert np.nanmax(d) <= bound, (name, t, float(np.nanmax(d)), bound)
    for k, c, y, mu, M, d in H.lowrank_cases():
        e = fixture[H.lowrank_name(k, c)]
        lp, rc = oracle.log_mvnpdf_low_rank(y, mu, M, d)
        assert rc == 0 and abs(lp - float(e["oracle_null"])) <= max(0.05 * e_oracle(e), 1e-11)
        identical &= lp == float(e["oracle_null"])
    print("intermediates and oracle values bit-identical with the stored ones:", bool(identical))


def test_oracle_stays_under_its_cap(fixture):
    """A condition on the choice of inputs (hard_conditioning_cases.TUNING), not a measurement: on every class of
    the drivers the as-written fp64 evaluation is within 1e-6 of the exact value.  The stand-alone function's inputs
    are held to it up to cond(B) 1e8; at 1e12 fp64 cannot resolve B's unit eigenvalue beyond 1e12 x 2^-53 = 1e-4."""
    for cls in H.CLASSES:
        name = H.class_name(cls)
        e = e_oracle(fixture[name])
        print(f"{name}: worst |oracle - exact| = {e:.3e}")
        assert e <= H.ORACLE_CAP, (name, e)
    for k in H.LOWRANK_KS:
        for c in H.LOWRANK_CONDS:
            e = e_oracle(fixture[H.lowrank_name(k, c)])
            print(f"{H.lowrank_name(k, c)}: |oracle - exact| = {e:.3e}")
            assert e <= (H.ORACLE_CAP if c < 1e12 else 1e-3), (k, c, e)


def test_hard_classes_are_hard(fixture):
    control = e_oracle(fixture[H.class_name(H.CLASSES[0])])
    assert H.CLASSES[0][0] == "control" and control < 1e-10 and float(fixture[H.class_name(H.CLASSES[0])]["cond_B"]) < 1e3
    for cls in H.CLASSES[1:]:
        e = fixture[H.class_name(cls)]
        if cls[0] in H.ON_CORRELATED_MODEL:
            assert float(e["cond_B"]) >= 1e6, (cls, float(e["cond_B"]))
        assert e_oracle(e) >= 10 * control, cls
    # the census of the saturated stratum's absorption vectors
    for driver in ("single", "multi"):
        a = fixture[H.class_name(("saturated", driver, 20, 3))]["absorption_dla"]
        placed = a[:H.NUM_PLACED]
        zeros, denormal, deep = (placed == 0).sum(axis=1), ((placed > 0) & (placed < TINY)).sum(axis=1), (placed < 1e-300).sum(axis=1)
        print(f"saturated ({driver}): per placed sample zeros {zeros.tolist()}, denormal {denormal.tolist()}, below 1e-300 "
              f"{deep.tolist()} of {a.shape[1]} pixels; smallest absorption of the eight in the box {placed[:8].min(axis=1).max():.1e}")
        assert zeros.sum() > 0 and denormal.sum() > 0
        assert (deep > a.shape[1] // 2).any() and (deep[8:] >= 10).all()
        assert (placed[:8].min(axis=1) < 1e-9).all()                     # log N_HI = 23 and 22.5 on line cores: black
        assert (a[H.NUM_PLACED:].min(axis=1) > 0).all()
    two = fixture[H.class_name(("saturated", "multi", 20, 3))]
    pair = two["absorption_dla"][:H.NUM_PLACED] * two["absorption_dla"][two["base_sample_inds"][0, :H.NUM_PLACED].astype(int) - 1]
    assert ((pair > 0) & (pair < TINY)).any() or (pair == 0).any()


def test_no_map_index_hangs_on_a_near_tie(fixture):
    """the GPU tests compare MAP columns with the oracle exactly; that is fair only while the two largest exact
    values of every table are further apart than twice the class's tolerance"""
    for cls in H.CLASSES:
        e = fixture[H.class_name(cls)]
        tol = H.tolerance(e_oracle(e))
        for t in H.TABLES:
            if "exact_" + t in e:
                gap = H.closest_top_two(e["exact_" + t])
                assert gap > 2 * tol, (cls, t, gap, tol)
                assert int(np.nanargmax(e["exact_" + t])) == int(np.nanargmax(e["oracle_" + t])), (cls, t)


def test_comparison_helper_notices_a_precision_loss(fixture, cases, oracle):
    """``class_failures`` fed the oracle's own values passes; fed the oracle's values computed from noise variances
    rounded to float32 (a relative 6e-8 on every d, what one tile accumulated in single precision would do) it
    fails in every hard class, and so it does on a NaN in one slot or a finite value where the exact one is NaN."""
    for cls in H.CLASSES:
        name = H.class_name(cls)
        e, case = fixture[name], cases[name]
        exact, stored = H.stored_values(e, "exact_"), H.stored_values(e, "oracle_")
        failures, e_got, e_orc, tol = H.class_failures(name, stored, exact, stored)
        assert failures == [] and e_got == e_orc and tol == max(10 * e_orc, 1e-9)
        nv = case["spectrum"]["noise_variance"]
        rounded = H.run_oracle(oracle, case, noise_variance=nv.astype(np.float32).astype(np.float64), dump=False)
        failures, e_got, _, tol = H.class_failures(name, rounded, exact, stored)
        print(f"{name}: float32 noise variances move the log-likelihoods by {e_got:.3e} (tolerance {tol:.3e})")
        if cls[0] in H.HARD_STRATA:
            assert len(failures) == 1 and name in failures[0], (name, e_got, tol)
        broken = {t: np.array(v, dtype=np.float64) for t, v in stored.items()}
        broken["dla"][7] = np.nan
        assert H.class_failures(name, broken, exact, stored)[1] == np.inf
        if "dla2" in exact and np.isnan(exact["dla2"]).any():
            broken = {t: np.array(v, dtype=np.float64) for t, v in stored.items()}
            broken["dla2"][np.flatnonzero(np.isnan(exact["dla2"]))[0]] = 0.0
            assert H.class_failures(name, broken, exact, stored)[0]
    # the fixed bound of the control class
    e = fixture[H.class_name(H.CLASSES[0])]
    exact, stored = H.stored_values(e, "exact_"), H.stored_values(e, "oracle_")
    off = dict(stored, null=float(stored["null"]) + 2e-9)
    assert H.class_failures("control", off, exact, stored, extra_bound=1e-9)[0]
