"""The refine pass and the batch conditioned on fixed absorbers (4.20) against 50-digit arithmetic
where the arithmetic is hard (tests/refine_hard_cases.py; tests/golden/exact_refine_hard.npz): the strata of
hard_conditioning_cases.py -- S/N 100 .. 1000, cond(B) ~ 5e6, |log-likelihood| 1e5 .. 5e6, one-hot posteriors, saturated
troughs, fewer kept pixels than the rank -- reached through the boxed prologue (N' = exp10(n') and z' formed on the
device, in boxes a quarter, an eighth and a sixteenth of the range wide) and through k_condition_rows (a fixed absorber
of log N_HI = 23 zeroes mu, M and omega2 on a run of kept pixels).  The rule, per class and per level or list, is that
of test_gpu_hard_conditioning.py:

    e_gpu = max |GPU - exact| <= max(10 x e_oracle, 1e-9),   e_oracle = the as-written fp64 oracle's worst error on
                                                             the SAME values (stored in the fixture)

Refine: status 0; the GPU's boxes equal the fixture's -- those of EXACT arithmetic -- bit for bit (a condition the
inputs were chosen for, refine_hard_cases.py; a difference names the level and the sample that flipped and ends the
test); l' and lambda of every level by the rule; log Z_ref of a call with 1, 2 and 3 levels against the 50-digit
evidence at max(10 E, 1e-9), E the oracle's worst error over the first-pass table and the levels of the call
(log-sum-exp is 1-Lipschitz in the sup norm); the MAP index equals the exact one wherever the exact top-two gap exceeds
twice that bound, and MAP z and log N are then z' and n' of that index, bit for bit.
Conditioned: the null model and the table by the rule, the -inf pattern exactly, nothing passes on NaN.

Kernels: k_refine_boxes, k_sweep_slim_boxed<3>, <0>, k_sweep_split_slim<3, 0, BoxedSweepArgs>, k_refine_finish;
k_condition_rows, k_sweep_slim<3>, k_sweep_split_slim, k_condition_mask.  Hot loops: process_qsos.m:185-199,
process_qsos_multiple_dlas_meanflux.m:340-392.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import hard_conditioning_cases as H
import refine_hard_cases as RH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture(golden):
    return RH.load_fixture(golden)


@pytest.fixture(scope="module")
def first_fixture(golden):
    return H.load_fixture(golden)


def flipped(e, f, got_boxes, lev, source):
    """which sample of the level's source table changed sides of the cut max - delta, for the failure message"""
    z, n = (RH.first_pass_coordinates(f) if lev == 0 else (e["z"][lev - 1], e["n"][lev - 1]))
    want = np.asarray(f["exact_dla"] if lev == 0 else e["exact_lam"][lev - 1], dtype=np.float64)
    delta = float(e["delta"])
    a, b = want >= want.max() - delta, source >= np.nanmax(source) - delta
    who = np.flatnonzero(a != b)
    return (f"level {lev + 1}: box {got_boxes[lev].tolist()} is not the exact tables' {e['boxes'][lev].tolist()}; samples whose membership of A "
            f"flipped: {who.tolist()} (exact {want[who].tolist()}, GPU {source[who].tolist()})")


@pytest.mark.parametrize("cls", RH.REFINE_CLASSES, ids=RH.refine_name)
def test_refined_class_against_exact_arithmetic(cls, fixture, first_fixture):
    name = RH.refine_name(cls)
    e, f = fixture[name], first_fixture[H.class_name(cls)]
    r = RH.run_gpu_refine(H.build_case(cls), *RH.points(int(e["first_index"])), float(e["delta"]))
    first, bad = r["first"], []
    assert (np.asarray(first["status"]) == 0).all()
    # the box of level 1 starts from the search range: the fixture's, bit for bit
    assert first["min_z_dlas"][0] == float(f["min_z_dla"]) and first["max_z_dlas"][0] == float(f["max_z_dla"])
    source = first["sample_log_likelihoods_dla"][0]
    for lev, out in enumerate(r["levels"]):
        assert out["status"][0] == 0, (name, lev, out["status"])
        assert out["boxes"].shape == (1, lev + 1, 4)
        if not np.array_equal(out["boxes"][0], e["boxes"][:lev + 1]):
            pytest.fail(f"{name}: " + flipped(e, f, out["boxes"][0], lev, source))
        ell, lam = out["sample_log_likelihoods_refined"][0], out["sample_log_posteriors_refined"][0]
        assert np.isfinite(ell).all() and np.isfinite(lam).all()          # nothing passes on NaN
        e_oracle = RH.table_error(e["oracle_ell"][lev], e["exact_ell"][lev])
        e_gpu, e_lam = RH.table_error(ell, e["exact_ell"][lev]), RH.table_error(lam, e["exact_lam"][lev])
        bound = RH.evidence_bound(f, e, lev + 1)
        log_z, exact_z = float(out["log_likelihoods_dla_refined"][0]), float(e["log_z"][lev])
        e_z = abs(log_z - exact_z) if np.isfinite(log_z) else np.inf
        j, gap = int(e["map_ind"][lev]), float(e["gap"][lev])
        print(f"{name} level {lev + 1}: cond(B) {float(e['cond_B']):.2e}, max |ll| {np.abs(e['exact_ell'][lev]).max():.2e}, e_oracle {e_oracle:.3e}, "
              f"e_gpu {e_gpu:.3e}, ratio {RH.ratio(e_gpu, e_oracle):.2f}, lambda {e_lam:.3e}, tolerance {H.tolerance(e_oracle):.3e}; "
              f"log Z_ref {log_z!r} exact {exact_z!r} |delta| {e_z:.3e} bound {bound:.3e}; MAP {out['MAP_inds_refined'][0]:.0f} exact {j} "
              f"(top-two gap {gap:.3g})")
        bad += RH.failures(f"{name} level {lev + 1} l'", e_gpu, e_oracle)[0]
        bad += RH.failures(f"{name} level {lev + 1} lambda", e_lam, e_oracle)[0]
        if not e_z <= bound:
            bad.append(f"{name} with {lev + 1} levels: log Z_ref {log_z!r}, exact {exact_z!r}: {e_z:.3e} > {bound:.3e}")
        if out["log_posteriors_dla_refined"][0] != np.log(0.1) + out["log_likelihoods_dla_refined"][0]:
            bad.append(f"{name} with {lev + 1} levels: the refined log posterior is not log prior + log Z_ref")
        if gap > 2 * bound:
            if not (out["MAP_inds_refined"][0] == float(j) and out["MAP_z_dlas_refined"][0] == e["z"][lev][j - 1]
                    and out["MAP_log_nhis_refined"][0] == e["n"][lev][j - 1]):
                bad.append(f"{name} with {lev + 1} levels: MAP ({out['MAP_inds_refined'][0]}, {out['MAP_z_dlas_refined'][0]!r}, "
                           f"{out['MAP_log_nhis_refined'][0]!r}), exact ({j}, {e['z'][lev][j - 1]!r}, {e['n'][lev][j - 1]!r})")
        source = lam
    assert not bad, bad


@pytest.mark.parametrize("cls", RH.COND_CLASSES, ids=H.class_name)
def test_conditioned_class_against_exact_arithmetic(cls, fixture):
    entries = {which: fixture[RH.cond_name(cls, which)] for which in RH.LISTS}
    got = RH.run_gpu_conditioned(H.build_case(cls), {which: e["fixed"] for which, e in entries.items()})
    bad = []
    for which, e in entries.items():
        name, out = RH.cond_name(cls, which), got[which]
        assert (np.asarray(out["status"]) == 0).all(), (name, out["status"])
        null, table = float(out["log_likelihoods_no_dla"][0]), out["sample_log_likelihoods_dla"][0]
        masked = np.isneginf(e["exact_dla"])
        assert not np.isnan(table).any() and np.isfinite(null)            # nothing passes on NaN
        np.testing.assert_array_equal(np.isneginf(table), masked, err_msg=name)   # the -inf pattern, exactly
        assert np.isfinite(table[~masked]).all() and np.isfinite(out["log_likelihoods_dla"][0])
        e_oracle = max(RH.table_error(e["oracle_dla"], e["exact_dla"]), abs(float(e["oracle_null"]) - float(e["exact_null"])))
        e_null = abs(null - float(e["exact_null"]))
        e_gpu = max(RH.table_error(table, e["exact_dla"]), e_null)
        print(f"{name}: cond(B) {float(e['cond_B']):.2e}, max |ll| {np.abs(e['exact_dla'][~masked]).max():.2e}, {int((~masked).sum())} samples outside "
              f"the separation, deepest fixed absorption {float(e['trough']):.1e}, e_oracle {e_oracle:.3e}, e_gpu {e_gpu:.3e} (null model "
              f"{e_null:.3e}), ratio {RH.ratio(e_gpu, e_oracle):.2f}, tolerance {H.tolerance(e_oracle):.3e}")
        bad += RH.failures(name, e_gpu, e_oracle)[0]
        i = int(np.argmax(e["exact_dla"]))                                 # test_refine_hard.py: no near-tie
        if out["MAP_inds"][0] != i + 1.0:
            bad.append(f"{name}: MAP index {out['MAP_inds'][0]}, exact {i + 1}")
    assert not bad, bad
