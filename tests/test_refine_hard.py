"""The refine / fixed-absorber hard fixture (tests/golden/exact_refine_hard.npz, made by
tests/golden/make_exact_refine_hard.py from tests/refine_hard_cases.py) on the CPU: the conditions on the inputs hold
at every level (no exact value near its cut, no sample near a box edge), the oracle stays within its cap of the
50-digit values, the boxes are those of the restatement on the stored exact tables, the oracle reproduces its stored
values, every conditioned list leaves at least 40 samples, and the comparison the GPU tests use notices a loss of
precision.  Figures of the committed fixture (worst |oracle - exact|): refined levels 1e-8 .. 9e-7, conditioned
tables 4e-7 .. 9.4e-7.  Hot loops: process_qsos.m:185-199, log_mvnpdf_low_rank.m:11-32."""
import os

import numpy as np
import pytest

import hard_conditioning_cases as H
import refine_hard_cases as RH
import refine_restatement as RR


@pytest.fixture(scope="module")
def fixture(golden):
    return RH.load_fixture(golden)


@pytest.fixture(scope="module")
def first_fixture(golden):
    return H.load_fixture(golden)


@pytest.fixture(scope="module")
def prepared(oracle):
    out = {}
    for cls in dict.fromkeys(RH.REFINE_CLASSES + RH.COND_CLASSES):
        case = H.build_case(cls)
        out[cls] = (case, H.run_oracle(oracle, case))
    return out


def level_errors(entry):
    return [RH.table_error(entry["oracle_ell"][lev], entry["exact_ell"][lev]) for lev in range(RH.LEVELS)]


def cond_error(entry):
    return max(RH.table_error(entry["oracle_dla"], entry["exact_dla"]), abs(float(entry["oracle_null"]) - float(entry["exact_null"])))


def test_fixture_holds_every_class(fixture, golden):
    names = [RH.refine_name(c) for c in RH.REFINE_CLASSES] + [RH.cond_name(c, w) for c in RH.COND_CLASSES for w in RH.LISTS]
    assert sorted(fixture) == sorted(names) and len(set(names)) == 6 + 8
    for cls in RH.REFINE_CLASSES:
        e = fixture[RH.refine_name(cls)]
        assert e["boxes"].shape == (RH.LEVELS, 4) and all(e[key].shape == (RH.LEVELS, RH.SR) for key in ("z", "n", "exact_ell", "oracle_ell", "exact_lam"))
        assert np.isfinite(e["exact_ell"]).all() and np.isfinite(e["log_z"]).all()
        assert (int(e["first_index"]), float(e["delta"])) == RH.tuning(cls)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, RH.FIXTURE)) <= os.path.getsize(os.path.join(here, "exact_continuum_hard.npz"))


def test_margins_and_edge_distances_hold_at_every_level(fixture, first_fixture):
    """from the stored values: the source of level 1's box is the exact first-pass table, of every later box the exact
    lambda of the level before"""
    for cls in RH.REFINE_CLASSES:
        e, f = fixture[RH.refine_name(cls)], first_fixture[H.class_name(cls)]
        z, n = RH.first_pass_coordinates(f)
        src, parent = np.asarray(f["exact_dla"], dtype=np.float64), (float(f["min_z_dla"]), float(f["max_z_dla"])) + RH.n_range(n)
        for lev in range(RH.LEVELS):
            box = tuple(e["boxes"][lev])
            cut, edge = RH.box_margins(src, z, n, parent, box, float(e["delta"]))
            print(f"{RH.refine_name(cls)} level {lev + 1}: nearest value to the cut {cut:.3g}, nearest sample to an edge {edge:.3g} (relative), "
                  f"top-two gap {float(e['gap'][lev]):.3g}")
            assert cut == float(e["cut_margin"][lev]) and edge == float(e["edge_margin"][lev])
            assert cut > RH.MARGIN and edge > RH.EDGE_REL, (cls, lev)
            assert (np.abs(src - np.max(src)) <= float(e["delta"])).sum() >= 1
            src, z, n, parent = e["exact_lam"][lev], e["z"][lev], e["n"][lev], box
        # the margin is wide against what may move a table: a thousand oracle caps
        assert RH.MARGIN >= 1000 * H.ORACLE_CAP


def test_oracle_stays_under_its_cap(fixture):
    """a condition on the choice of inputs (refine_hard_cases.TUNING, FIXED), not a measurement"""
    for cls in RH.REFINE_CLASSES:
        for lev, err in enumerate(level_errors(fixture[RH.refine_name(cls)])):
            print(f"{RH.refine_name(cls)} level {lev + 1}: worst |oracle - exact| = {err:.3e}")
            assert err <= H.ORACLE_CAP, (cls, lev, err)
    for cls in RH.COND_CLASSES:
        for which in RH.LISTS:
            err = cond_error(fixture[RH.cond_name(cls, which)])
            print(f"{RH.cond_name(cls, which)}: worst |oracle - exact| = {err:.3e}")
            assert err <= H.ORACLE_CAP, (cls, which, err)


def test_boxes_are_the_restatement_on_the_stored_tables(fixture, first_fixture):
    """RR.refine_row on the stored exact first-pass table, handed the stored exact l' as its sweep: the same boxes, the
    same z' and n', bit for bit; its float64 evidence and MAP agree with the 50-digit ones"""
    for cls in RH.REFINE_CLASSES:
        e, f = fixture[RH.refine_name(cls)], first_fixture[H.class_name(cls)]
        u, v = RH.points(int(e["first_index"]))
        seen = []

        def sweep(lev, z, n):
            seen.append((z, n))
            return e["exact_ell"][lev]
        for levels in range(1, RH.LEVELS + 1):
            del seen[:]
            row = RR.refine_row(f["exact_dla"], f["offset_samples"], f["log_nhi_samples"], float(f["min_z_dla"]), float(f["max_z_dla"]), 0,
                                u, v, sweep, levels, float(e["delta"]), RH.PAD)
            assert row["status"] == 0
            np.testing.assert_array_equal(row["boxes"], e["boxes"][:levels], err_msg=str(cls))
            for lev, (z, n) in enumerate(seen):
                np.testing.assert_array_equal(z, e["z"][lev])
                np.testing.assert_array_equal(n, e["n"][lev])
            np.testing.assert_array_equal(np.asarray(row["lam"][-1], dtype=np.float64), e["exact_lam"][levels - 1])
            assert row["map_ind"] == float(e["map_ind"][levels - 1])
            assert abs(row["ambiguity"] - float(e["gap"][levels - 1])) <= 1e-9 * abs(float(e["gap"][levels - 1]))
            assert abs(float(row["log_z"]) - float(e["log_z"][levels - 1])) <= 1e-12 * abs(float(e["log_z"][levels - 1]))
            bound = RH.evidence_bound(f, e, levels)
            assert float(e["gap"][levels - 1]) > 2 * bound, (cls, levels)      # no MAP index hangs on a near-tie


def test_oracle_reproduces(fixture, prepared, oracle):
    """The oracle's values recomputed today, from absorption vectors recomputed today, against the stored ones: the
    fixture and the oracle have not drifted apart.  The rule of test_hard_conditioning.py::test_oracle_reproduces:
    another libm's last bits move a value by less than a twentieth of the class's own error (floored at 1e-11)."""
    identical = True
    for cls in RH.REFINE_CLASSES:
        e = fixture[RH.refine_name(cls)]
        case, run = prepared[cls]
        errs = level_errors(e)
        for lev in range(RH.LEVELS):
            tabs = RH.refined_absorption(oracle, run, e["z"][lev], e["n"][lev], case["params"].num_lines)
            got = RH.oracle_values(oracle, [H.lowrank_inputs(case, run, a) for a in tabs])
            d = float(np.abs(got - e["oracle_ell"][lev]).max())
            identical &= d == 0.0
            assert d <= max(0.05 * errs[lev], 1e-11), (cls, lev, d)
    for cls in RH.COND_CLASSES:
        case, run = prepared[cls]
        lists = RH.fixed_lists(run)
        tabs = H.absorption_tables(oracle, case, run)["dla"]
        for which in RH.LISTS:
            e = fixture[RH.cond_name(cls, which)]
            np.testing.assert_allclose(np.array(lists[which]), e["fixed"], rtol=1e-15, atol=0)
            fixed = [tuple(a) for a in e["fixed"]]
            null, table = conditioned_oracle(oracle, case, run, tabs, fixed)
            assert np.array_equal(np.isneginf(table), np.isneginf(e["oracle_dla"]))
            ok = np.isfinite(table)
            d = max(float(np.abs(table[ok] - e["oracle_dla"][ok]).max()), abs(null - float(e["oracle_null"])))
            identical &= d == 0.0
            assert d <= max(0.05 * cond_error(e), 1e-11), (cls, which, d)
    print("oracle values bit-identical with the stored ones:", bool(identical))


def conditioned_oracle(oracle, case, run, tabs, fixed, noise_variance=None):
    """(null, table [S]) of the as-written fp64 evaluation on the conditioned rows, -inf inside the separation"""
    if noise_variance is not None:
        case = dict(case, spectrum=dict(case["spectrum"], noise_variance=noise_variance))
    A = RH.fixed_absorption(run, fixed, case["params"].num_lines)
    close = RH.CR.close(run["sample_z_dlas"], fixed, RH.SEPARATION)
    table = np.full(H.S, -np.inf)
    table[~close] = RH.oracle_values(oracle, [RH.conditioned_inputs(case, run, A, tabs[i]) for i in np.flatnonzero(~close)])
    return float(RH.oracle_values(oracle, [RH.conditioned_inputs(case, run, A)])[0]), table


def test_conditioned_lists(fixture, prepared):
    for cls in RH.COND_CLASSES:
        case, run = prepared[cls]
        for which in RH.LISTS:
            e = fixture[RH.cond_name(cls, which)]
            zs = e["fixed"][:, 0]
            assert e["fixed"].shape == (len(RH.FIXED[which]), 2) and list(e["fixed"][:, 1]) == [ln for _, ln in RH.FIXED[which]]
            assert all(abs(a - b) >= 3 * RH.SEPARATION for i, a in enumerate(zs) for b in zs[:i])
            masked = np.isneginf(e["exact_dla"])
            np.testing.assert_array_equal(masked, RH.CR.close(run["sample_z_dlas"], [tuple(a) for a in e["fixed"]], RH.SEPARATION))
            assert np.isfinite(e["exact_dla"][~masked]).all() and np.array_equal(masked, np.isneginf(e["oracle_dla"]))
            print(f"{RH.cond_name(cls, which)}: {int((~masked).sum())} of {H.S} samples outside the separation, cond(B) {float(e['cond_B']):.2e}, "
                  f"deepest absorption on kept pixels {float(e['trough']):.1e}")
            assert masked.any() and (~masked).sum() >= RH.MIN_FINITE
            assert float(e["cond_B"]) >= 9e5
            if which == "three":      # the log N_HI = 23 trough lies on kept pixels
                assert float(e["trough"]) < 1e-25
            gap = H.closest_top_two(e["exact_dla"])
            assert gap > 2 * H.tolerance(cond_error(e))


def test_comparison_notices_a_precision_loss(fixture, prepared, oracle):
    """test_hard_conditioning.py::test_comparison_helper_notices_a_precision_loss on these tables: the oracle's own
    values pass; computed from noise variances rounded to float32 its l' of every level and its conditioned tables
    break H.tolerance(e_oracle) on every hard class; a NaN, or a finite value inside the separation, is an infinite
    error."""
    for cls in RH.REFINE_CLASSES:
        e = fixture[RH.refine_name(cls)]
        case, run = prepared[cls]
        nv = case["spectrum"]["noise_variance"]
        rounded = dict(case, spectrum=dict(case["spectrum"], noise_variance=nv.astype(np.float32).astype(np.float64)))
        for lev, e_orc in enumerate(level_errors(e)):
            assert RH.failures("oracle", RH.table_error(e["oracle_ell"][lev], e["exact_ell"][lev]), e_orc)[0] == []
            tabs = RH.refined_absorption(oracle, run, e["z"][lev], e["n"][lev], case["params"].num_lines)
            got = RH.oracle_values(oracle, [H.lowrank_inputs(rounded, run, a) for a in tabs])
            e_got = RH.table_error(got, e["exact_ell"][lev])
            bad, tol = RH.failures(RH.refine_name(cls), e_got, e_orc)
            print(f"{RH.refine_name(cls)} level {lev + 1}: float32 noise variances move l' by {e_got:.3e} (tolerance {tol:.3e})")
            assert len(bad) == 1, (cls, lev, e_got, tol)
        broken = np.array(e["oracle_ell"][0])
        broken[7] = np.nan
        assert RH.table_error(broken, e["exact_ell"][0]) == np.inf
    for cls in RH.COND_CLASSES:
        case, run = prepared[cls]
        tabs = H.absorption_tables(oracle, case, run)["dla"]
        nv = case["spectrum"]["noise_variance"]
        for which in RH.LISTS:
            e = fixture[RH.cond_name(cls, which)]
            null, table = conditioned_oracle(oracle, case, run, tabs, [tuple(a) for a in e["fixed"]], nv.astype(np.float32).astype(np.float64))
            e_got = max(RH.table_error(table, e["exact_dla"]), abs(null - float(e["exact_null"])))
            bad, tol = RH.failures(RH.cond_name(cls, which), e_got, cond_error(e))
            print(f"{RH.cond_name(cls, which)}: float32 noise variances move the table by {e_got:.3e} (tolerance {tol:.3e})")
            assert len(bad) == 1, (cls, which, e_got, tol)
            broken = np.array(e["oracle_dla"])
            broken[np.flatnonzero(np.isneginf(broken))[0]] = 0.0
            assert RH.table_error(broken, e["exact_dla"]) == np.inf
            broken = np.array(e["oracle_dla"])
            broken[np.flatnonzero(np.isfinite(broken))[0]] = np.nan
            assert RH.table_error(broken, e["exact_dla"]) == np.inf
