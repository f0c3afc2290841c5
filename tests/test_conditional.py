"""CPU checks of the batch conditioned on fixed absorbers: the library's validation (no GPU), the
restatement of tests/conditional_restatement.py against Python loops, the identity the feature rests on
(conditioning IS the multi-DLA model), what the CPU twin shows on the synthetic batch of
tests/conditional_cases.py, and the host-side writers.  Every figure is printed before it is asserted."""
import ctypes as C
import math

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, catalog, conditional, io

import conditional_cases as CC
import conditional_restatement as CR

SEP = CC.SEPARATION


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _validate(lib, offsets, z, ln, sep):
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    z, ln = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(ln, dtype=np.float64)
    i64p, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    rc = lib.gpdla_fixed_absorbers_validate(off.size - 1, off.ctypes.data_as(i64p), z.ctypes.data_as(dp), ln.ctypes.data_as(dp), float(sep))
    return rc, lib.gpdla_last_error().decode()


def test_validation_names_the_field_and_the_quasar(lib):
    z, ln = np.array([2.0, 2.5, 3.0, 3.5]), np.array([20.5, 21.0, 20.3, 20.9])
    assert _validate(lib, [0, 2, 2, 4], z, ln, SEP)[0] == 0
    assert _validate(lib, [0, 0, 0], z[:0], ln[:0], 0.0)[0] == 0               # no absorbers anywhere
    nine = 2.0 + 0.1 * np.arange(9)
    cases = [(([0, 3, 2, 4], z, ln, SEP), ("offsets", "quasar 1")),
             (([0, 0, 9], nine, np.full(9, 20.5), SEP), ("offsets", "quasar 1", "9")),
             (([0, 2, 4], [2.0, np.nan, 3.0, 3.5], ln, SEP), ("z_dlas[1]", "quasar 0")),
             (([0, 2, 4], [2.0, 2.5, 3.0, np.inf], ln, SEP), ("z_dlas[3]", "quasar 1")),
             (([0, 2, 4], z, [20.5, 21.0, np.nan, 20.9], SEP), ("log_nhis[2]", "quasar 1")),
             (([0, 2, 4], z, [20.5, -np.inf, 20.3, 20.9], SEP), ("log_nhis[1]", "quasar 0")),
             (([0, 2, 4], z, ln, -1e-3), ("min_z_separation",)),
             (([0, 2, 4], z, ln, np.nan), ("min_z_separation",)),
             (([0, 2, 4], z, ln, np.inf), ("min_z_separation",)),
             (([0, 1, 4], [2.0, 3.0, 3.5, 3.0 + 0.5 * SEP], ln, SEP), ("z_dlas[1]", "z_dlas[3]", "quasar 1", "min_z_separation"))]
    for args, words in cases:
        rc, msg = _validate(lib, *args)
        print(rc, msg)
        assert rc == _lib.ERR_INVALID_ARGUMENT and all(w in msg for w in words), (msg, words)
    # two separations apart is accepted; the same pair in two different quasars is no pair
    assert _validate(lib, [0, 2], [3.0, 3.0 + 2 * SEP], ln[:2], SEP)[0] == 0
    assert _validate(lib, [0, 1, 2], [3.0, 3.0], ln[:2], SEP)[0] == 0
    assert lib.gpdla_fixed_absorbers_validate(1, None, None, None, SEP) == _lib.ERR_INVALID_ARGUMENT


def _oracle_params(nl):
    from oracle import oracle
    return oracle.OracleParams(num_lines=nl)


def _first(model, sp, nl):
    """The quasar's search range from the oracle."""
    from oracle import oracle
    r = oracle.process_spectrum(model, np.array([0.5]), np.array([1e20]), sp["wavelengths"], sp["flux"], sp["noise_variance"],
                                sp["pixel_mask"], sp["z_qso"], _oracle_params(nl))
    return r["min_z_dla"], r["max_z_dla"]


def test_restatement_against_python_loops():
    """One two-absorber row conditioned on its first absorber: A, the conditioned rows, the separation rule, the
    boxes, the evidence and the new list, each read literally in Python loops with math.fsum."""
    from oracle import oracle
    k, nl, Sr, L = CC.CONFIGS[0]
    model, samples, spectra, truth = CC.make_batch(k, nl, extra=False)
    q = CC.KINDS.index("two_far")
    sp, fixed = spectra[q], [list(truth[q][0]), [truth[q][0][0] + 6 * SEP, 20.3]]
    # A and the rows
    rows = CR.dense_rows(model, sp, _oracle_params(nl))
    A = CR.absorption(rows["padded"], fixed, nl)
    profs = [oracle.voigt(rows["padded"], z, 10.0 ** ln, nl) for z, ln in fixed]
    A_loop = [float(profs[0][i]) * float(profs[1][i]) for i in range(A.size)]
    np.testing.assert_array_equal(A, np.array(A_loop))
    grid_rows = np.stack([rows["y"], rows["mu"], rows["omega2"], rows["nu"]], 1)
    got_rows, got_M = CR.conditioned_rows(grid_rows, rows["M"], A[rows["kept"]])
    for r, i in enumerate(rows["kept"]):
        a = A_loop[i]
        assert got_rows[r, 0] == rows["y"][r] and got_rows[r, 3] == rows["nu"][r]
        assert got_rows[r, 1] == float(rows["mu"][r]) * a and got_rows[r, 2] == float(rows["omega2"][r]) * (a * a)
        assert all(got_M[r, c] == float(rows["M"][r, c]) * a for c in range(k))
    # one pass on the multi-DLA route, one fixed absorber
    fixed = fixed[:1]
    min_z, max_z = _first(model, sp, nl)
    u, v = CC.halton_points(Sr)
    cond_at, _ = CR.twin_table(model, sp, _oracle_params(nl), min_z, max_z, fixed, SEP, prev_tau_0=0.0)
    row = CR.refine_pass(cond_at, samples, min_z, max_z, fixed, u, v, L, CC.DELTA, CC.PAD, SEP)
    assert row["status"] == 0
    # the raw tables of the brute force: the conditional ones with the rule undone (a finite number where it put -inf),
    # so that the loops have to find the same entries from the redshifts alone
    off, lnhi = samples["offset_samples"], samples["log_nhi_samples"]
    raw_first = np.where(np.isneginf(row["first"]), 0.0, row["first"])
    raw_levels = [np.where(np.isneginf(e), 0.0, e) for e in row["ell"]]
    boxes, log_z, (map_z, map_n), (first, masked) = CR.brute_force_pass(list(raw_first), [list(e) for e in raw_levels], list(off), list(lnhi),
                                                                        min_z, max_z, fixed, list(u), list(v), CC.DELTA, CC.PAD, SEP)
    np.testing.assert_array_equal(np.array(first), row["first"])
    for lev in range(L):
        np.testing.assert_array_equal(np.array(masked[lev]), row["ell"][lev])
    np.testing.assert_array_equal(np.array(boxes), row["boxes"])
    assert (map_z, map_n) == (row["map_z"], row["map_n"])
    inside = int(np.isneginf(row["first"]).sum())
    print(f"two_far | first: {inside} of {off.size} first-pass samples inside the separation; log Z_ref {row['log_z']:.12f} loops {log_z:.12f}")
    assert inside > 0 and abs(row["log_z"] - log_z) <= 1e-13 * abs(log_z)
    # the orchestration: one discovery from [first] appends the pass's MAP, exactly
    lists, hist = CR.run(lambda qq, fx: row, [fixed], 1, 0)
    assert lists == [fixed + [[map_z, map_n]]] and hist[0][0] == "discover 0"


@pytest.mark.parametrize("k,nl", [(8, 3), (24, 5)])
@pytest.mark.parametrize("F", [1, 2])
def test_conditioning_is_the_multi_dla_model(k, nl, F):
    """The dense route (process_qsos.m's rows x A, one log_mvnpdf_low_rank per sample) against column F of the oracle's
    multi-DLA driver with the fixed absorbers as constant base samples.  With one forest line and prev_tau_0 = 0 the
    multi-DLA driver's rows are process_qsos.m's."""
    model, samples, spectra, truth = CC.make_batch(k, nl, extra=False)
    q = CC.KINDS.index("two_unequal")
    sp = spectra[q]
    fixed = [list(a) for a in truth[q]][:F]
    rows = CR.dense_rows(model, sp, _oracle_params(nl))
    off, nhi = samples["offset_samples"], samples["nhi_samples"]
    z = rows["min_z"] + (rows["max_z"] - rows["min_z"]) * off
    dense, dense_null = CR.dense_table(rows, nl, z, nhi, fixed, SEP)
    multi, multi_null = CR.multi_table(model, sp, _oracle_params(nl), off, nhi, fixed, rows["min_z"], rows["max_z"], SEP,
                                       prev_tau_0=0.0, num_forest_lines=1)
    np.testing.assert_array_equal(np.isneginf(dense), np.isneginf(multi))
    ok = ~np.isneginf(dense)
    worst = float(np.abs(dense[ok] - multi[ok]).max())
    print(f"k {k} lines {nl} F {F}: {int(ok.sum())} samples, {int((~ok).sum())} inside the separation, worst |dense - multi| {worst:.3e}, "
          f"null {abs(dense_null - multi_null):.3e}")
    assert (~ok).sum() > 0 and worst <= 1e-9 and abs(dense_null - multi_null) <= 1e-9


_TWIN = {}


def twin(k, nl, Sr, L):
    """extra = 2, rounds = 2 on the science rows at MultiParameters(prev_tau_0 = 0), the multi-DLA route."""
    key = (k, nl, Sr, L)
    if key not in _TWIN:
        model, samples, spectra, truth = CC.make_batch(k, nl, extra=False)
        u, v = CC.halton_points(Sr)
        ranges = [_first(model, sp, nl) for sp in spectra]

        def pass_of(q, fixed):
            mn, mx = ranges[q]
            table_at, state = CR.twin_table(model, spectra[q], _oracle_params(nl), mn, mx, fixed, SEP, prev_tau_0=0.0)
            row = CR.refine_pass(table_at, samples, mn, mx, fixed, u, v, L, CC.DELTA, CC.PAD, SEP)
            row["null"] = state["null"]
            return row
        _TWIN[key] = (truth, *CR.run(pass_of, [[] for _ in spectra], 2, 2))
    return _TWIN[key]


@pytest.mark.parametrize("k,nl,Sr,L", CC.CONFIGS)
def test_twin_bayes_factors_and_recovery(k, nl, Sr, L):
    truth, lists, hist = twin(k, nl, Sr, L)
    kinds = [r[0] for r in CC.SCIENCE]
    bf = {name: {kinds[q]: r["log_z"] - r["null"] for q, r in res.items()} for name, _, res, _ in hist}
    print(f"k {k} lines {nl} S' {Sr} levels {L}: log Bayes factor, nothing fixed {bf['discover 0']}")
    print(f"  first absorber fixed {bf['discover 1']}")
    for kind in kinds:
        if kind == "none":
            assert bf["discover 0"][kind] < 0 and bf["discover 1"][kind] < 0
        else:
            assert bf["discover 0"][kind] > 300
            assert bf["discover 1"][kind] > 100 if kind in CC.TWO else bf["discover 1"][kind] < 0, kind
    for q, kind in enumerate(kinds):
        for z, ln in truth[q]:
            dz, dn = min((abs(a[0] - z), abs(a[1] - ln)) for a in lists[q])
            print(f"  {kind}: injected ({z:.5f}, {ln}) nearest slot |dz| {dz:.2e} |dlogN| {dn:.3f}")
            assert dz <= 3e-3 and dn <= 0.25, kind


def _hand_made():
    """Three quasars of a 2-DLA run: a 2-DLA winner with both slots refined, a 1-DLA winner whose refine was
    unusable, a null winner; and a conditional result for them."""
    mp = np.array([[0.01, 0.01, 0.08, 0.9], [0.05, 0.05, 0.8, 0.1], [0.9, 0.05, 0.03, 0.02]])
    map_z = np.full((3, 2, 2), np.nan)
    map_n = np.full((3, 2, 2), np.nan)
    map_z[0, 0, 0], map_n[0, 0, 0] = 2.4, 20.7
    map_z[0, 1], map_n[0, 1] = (2.5, 2.9), (21.0, 20.4)
    map_z[1, 0, 0], map_n[1, 0, 0] = 3.1, 20.9
    map_z[1, 1], map_n[1, 1] = (3.1, np.nan), (20.9, np.nan)
    results = dict(model_posteriors=mp, MAP_z_dlas=map_z, MAP_log_nhis=map_n, min_z_dlas=np.array([2.0, 2.6, 2.2]),
                   max_z_dlas=np.array([3.0, 3.6, 3.2]))
    info = dict(ras=np.arange(3.0), decs=np.arange(3.0), snrs=np.ones(3), plates=np.arange(3), mjds=np.arange(3), fiber_ids=np.arange(3),
                thing_ids=np.arange(3), z_qsos=np.array([3.1, 3.7, 3.3]))
    P = 5
    c = dict(z_dlas=np.array([[2.501, 2.899], [3.1, np.nan], [np.nan, np.nan]]), log_nhis=np.array([[21.05, 20.45], [20.9, np.nan], [np.nan] * 2]),
             start_z_dlas=np.array([[2.5, 2.9], [3.1, np.nan], [np.nan] * 2]), start_log_nhis=np.array([[21.0, 20.4], [20.9, np.nan], [np.nan] * 2]),
             status=np.array([[0, 0], [1, -1], [-1, -1]], dtype=np.int32), probabilities=np.array([0.025, 0.16, 0.5, 0.84, 0.975]),
             num_absorbers=np.array([2, 1, 0]))
    for name in ("mean_z", "std_z", "mean_log_nhi", "std_log_nhi", "effective_samples", "log_bayes_factor"):
        c[name] = np.arange(6.0).reshape(3, 2) + len(name)
    c["quantiles_z"] = np.arange(6.0 * P).reshape(3, 2, P)
    c["quantiles_log_nhi"] = 100 + np.arange(6.0 * P).reshape(3, 2, P)
    return results, info, c


def test_json_catalogue_conditional():
    results, info, c = _hand_made()
    plain = catalog.generate_json_catalogue(results, info, occams_razor=1.0)
    got = catalog.generate_json_catalogue_conditional(results, info, c, occams_razor=1.0)
    assert [r["num_dlas"] for r in got] == [2, 1, 0]
    for j in range(2):   # both slots replaced
        d = got[0]["dlas"][j]
        assert d["refined"] and (d["z_dla"], d["log_nhi"]) == (c["z_dlas"][0, j], c["log_nhis"][0, j])
        assert d["z_dla_q0.5"] == c["quantiles_z"][0, j, 2] and d["log_nhi_q0.975"] == c["quantiles_log_nhi"][0, j, 4]
        assert d["effective_samples"] == c["effective_samples"][0, j] and d["log_bayes_factor"] == c["log_bayes_factor"][0, j]
        assert d["z_dla_mean"] == c["mean_z"][0, j] and d["log_nhi_std"] == c["std_log_nhi"][0, j]
    # an unusable slot, and a record without absorbers: as generate_json_catalogue writes them
    assert got[1]["dlas"] == [dict(plain[1]["dlas"][0], refined=False)] and got[2]["dlas"] == []
    for a, b in zip(got, plain):
        assert {k: v for k, v in a.items() if k != "dlas"} == {k: v for k, v in b.items() if k != "dlas"}
    # a record whose reported model is not the one map_absorbers chose: its absorber (2.4, 20.7) was never a starting value
    mp = results["model_posteriors"].copy()
    mp[0] = [0.01, 0.01, 0.9, 0.08]
    moved = catalog.generate_json_catalogue_conditional(dict(results, model_posteriors=mp), info, c, occams_razor=1.0)
    assert moved[0]["dlas"] == [dict(log_nhi=20.7, z_dla=2.4, refined=False)]
    # a NaN slot of the reported model stays NaN and unrefined
    mp[1] = [0.05, 0.05, 0.1, 0.8]
    nan_slot = catalog.generate_json_catalogue_conditional(dict(results, model_posteriors=mp), info, c, occams_razor=1.0)
    assert nan_slot[1]["dlas"][0]["refined"] is False and math.isnan(nan_slot[1]["dlas"][1]["z_dla"]) and not nan_slot[1]["dlas"][1]["refined"]
    with pytest.raises(ValueError, match="quasars"):
        catalog.generate_json_catalogue_conditional(results, info, {k: (v[:2] if k != "probabilities" else v) for k, v in c.items()})


def test_lists_and_files_round_trip(tmp_path):
    lists = [[[2.5, 21.0], [2.9, 20.4]], [], [[3.1, 20.9]]]
    off, z, n = conditional.csr_of(lists)
    assert off.tolist() == [0, 2, 2, 3] and conditional.lists_of((off, z, n), 3) == lists
    assert conditional.lists_of(None, 2) == [[], []]
    pz, pn = conditional.padded(lists, 2)
    np.testing.assert_array_equal(pz, [[2.5, 2.9], [np.nan, np.nan], [3.1, np.nan]])
    with pytest.raises(ValueError, match="offsets"):
        conditional.lists_of((off[:-1], z, n), 3)
    _, _, c = _hand_made()
    c["boxes"] = np.arange(3 * 2 * 2 * 4.0).reshape(3, 2, 2, 4)
    c["discovered"] = np.array([[0, 1], [0, 0], [0, 0]], dtype=np.int32)
    c["num_start"] = np.array([1, 1, 0])
    c["history"] = [dict(name="not stored")]
    path = str(tmp_path / "conditional.mat")
    io.save_conditional_results(path, c, rounds=np.float64(2))
    back = io.load_conditional_results(path)
    assert "history" not in back and float(np.asarray(back["rounds"]).reshape(-1)[0]) == 2.0
    for key, val in c.items():
        if key != "history":
            np.testing.assert_array_equal(back[key], val, err_msg=key)
            assert back[key].dtype == np.asarray(val).dtype or key in ("num_absorbers", "num_start"), key
    assert back["status"].dtype == np.int32 and back["num_absorbers"].dtype == np.int64
