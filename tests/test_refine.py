"""CPU checks of the refine pass: the NumPy restatement against a brute-force reading of the
definitions, the library's request checks (made before a device is touched), the file round trip, and the
twin of the whole feature -- the restatement's boxes around the CPU oracle's sweep -- on the batch of
tests/refine_cases.py: the conditions that tests/test_gpu_refine.py asserts on the GPU hold for the
reference alone."""
import math

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, io, refine

import posterior_restatement as PR
import refine_cases as RC
import refine_restatement as RR


def _toy_sweep(zc, nc, sz, sn, holes=()):
    def sweep(level, z, n):
        l = 40.0 - 0.5 * ((z - zc) / sz) ** 2 - 0.5 * ((n - nc) / sn) ** 2
        l[list(holes)] = np.nan
        return l
    return sweep


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("S,Sr,min_z,max_z,pad,delta", [
    (17, 11, 2.0, 3.0, 2.0, 12.5), (9, 23, 2.0, 3.0, 0.5, 3.0), (12, 12, 2.5, 2.5, 2.0, 12.5), (7, 5, 2.0, 3.0, 0.0, 1e-9)])
def test_restatement_against_a_brute_force_reading(levels, S, Sr, min_z, max_z, pad, delta):
    rng = np.random.default_rng(S * 100 + Sr)
    offsets, lnhi = rng.uniform(size=S), 20.0 + 3.0 * rng.uniform(size=S)
    u, v = rng.uniform(size=Sr), rng.uniform(size=Sr)
    sweep = _toy_sweep(2.6 if max_z > min_z else 2.5, 21.1, 0.02, 0.1, holes=(1,))
    l = sweep(0, min_z + (max_z - min_z) * offsets, lnhi)
    l[0] = np.nan
    row = RR.refine_row(l, offsets, lnhi, min_z, max_z, 0, u, v, sweep, levels, delta, pad)
    assert row["status"] == 0
    boxes, log_z, ind = RR.brute_force_row(l.tolist(), offsets.tolist(), lnhi.tolist(), min_z, max_z, u.tolist(), v.tolist(),
                                           [e.tolist() for e in row["ell"]], delta, pad, float(lnhi.min()), float(lnhi.max()))
    np.testing.assert_array_equal(row["boxes"], np.array(boxes))
    assert row["map_ind"] == ind
    assert abs(row["log_z"] - log_z) <= 1e-13 * abs(log_z), (row["log_z"], log_z)
    ext = RR.refine_row(l, offsets, lnhi, min_z, max_z, 0, u, v, sweep, levels, delta, pad, dtype=np.longdouble)
    assert abs(float(ext["log_z"]) - log_z) <= 1e-13 * abs(log_z)
    if max_z == min_z:   # a zero-width range: every box is that point, its width fraction counts as 1
        assert (row["boxes"][:, 0] == min_z).all() and (row["boxes"][:, 1] == min_z).all() and np.isfinite(row["log_z"])
    if pad == 0.0:       # one sample in A and no pad: a zero-width box holds no prior volume
        assert row["boxes"][0, 0] == row["boxes"][0, 1] and row["boxes"][0, 2] == row["boxes"][0, 3]


def test_restatement_evidence_of_a_flat_likelihood_is_the_likelihood():
    """l == c everywhere: every box is the whole range and Z_ref = exp(c) (uniform prior: V W / (N_hi - N_lo) = 1)."""
    S = Sr = 64
    rng = np.random.default_rng(3)
    offsets, lnhi, u, v = rng.uniform(size=S), 20 + 3 * rng.uniform(size=S), rng.uniform(size=Sr), rng.uniform(size=Sr)
    row = RR.refine_row(np.full(S, 7.5), offsets, lnhi, 2.0, 3.0, 0, u, v, lambda lev, z, n: np.full(Sr, 7.5), 2, 12.5, 1e3)
    np.testing.assert_array_equal(row["boxes"], np.tile([2.0, 3.0, lnhi.min(), lnhi.max()], (2, 1)))
    assert abs(row["log_z"] - 7.5) < 1e-13


def test_restatement_unusable_rows():
    S = Sr = 8
    x = np.linspace(0.1, 0.9, S)
    sweep = lambda lev, z, n: np.zeros(Sr)
    for l, lo, hi, status in ((np.full(S, np.nan), 2.0, 3.0, 0), (np.r_[np.inf, np.zeros(S - 1)], 2.0, 3.0, 0),
                              (np.zeros(S), np.nan, 3.0, 0), (np.zeros(S), 2.0, np.nan, 0), (np.zeros(S), 2.0, 3.0, 3),
                              (np.full(S, -np.inf), 2.0, 3.0, 0)):
        row = RR.refine_row(l, x, 20 + x, lo, hi, status, x, x, sweep, 2)
        assert row["status"] == 1 and np.isnan(row["boxes"]).all() and np.isnan(row["log_z"]) and np.isnan(row["map_ind"])
    # a level whose lambda has no finite entry ends the row; the boxes reached before are kept
    row = RR.refine_row(np.zeros(S), x, 20 + x, 2.0, 3.0, 0, x, x, lambda lev, z, n: np.full(Sr, np.nan), 2)
    assert row["status"] == 1 and not np.isnan(row["boxes"][0]).any() and np.isnan(row["boxes"][1]).all()


def test_requests_are_refused_before_a_device_is_touched():
    refine.validate()
    refine.validate(levels=_lib.REFINE_MAX_LEVELS, delta=1e-3, pad=0.0, u=[0.0, 0.5], v=[0.25, 1 - 2 ** -53])
    for kw, field in ((dict(levels=0), "levels"), (dict(levels=5), "levels"), (dict(delta=0.0), "delta"),
                      (dict(delta=float("inf")), "delta"), (dict(delta=float("nan")), "delta"), (dict(pad=-0.5), "pad"),
                      (dict(pad=float("nan")), "pad"), (dict(u=[0.5, 1.0], v=[0.1, 0.2]), r"u\[1\]"),
                      (dict(u=[0.5], v=[-0.1]), r"v\[0\]"), (dict(u=[float("nan")], v=[0.1]), r"u\[0\]"),
                      (dict(u=[], v=[]), "num_points")):
        with pytest.raises(_lib.GpdlaError, match=field) as e:
            refine.validate(**kw)
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    bad = _lib.NhiPrior((0.0, 0.0, -1.0), 21.0, 1.5, 20.0, 23.0, 20.0, float("nan"), 1.0)
    with pytest.raises(_lib.GpdlaError, match="alpha"):
        refine.validate(prior=bad)
    lib = _lib.load()
    assert lib.gpdla_refine_validate(None, None, 0, None, None) == _lib.ERR_INVALID_ARGUMENT
    # the calls on handles refuse null handles without a device as well
    rq = refine.request()
    assert lib.gpdla_batch_refine(None, None, None, 0, rq, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_context_set_refine_points(None, 1, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_batch_download_refined(None, None, None, 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_batch_refined_summaries(None, None, None, 0, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.gpdla_debug_last_refine_ms() == -1.0
    with pytest.raises(ValueError):
        refine.validate(u=[0.1, 0.2], v=[0.1])


def test_file_round_trip(tmp_path):
    rng = np.random.default_rng(11)
    n, L, Sr = 5, 3, 7
    out = refine.empty_results(n, L, Sr)
    for k in refine.SCALARS + refine.TABLES + ("boxes",):
        out[k][...] = rng.normal(size=out[k].shape)
    out["MAP_inds_refined"][:] = [1, 7, 3, 2, 5]
    out["log_likelihoods_dla_refined"][2] = np.nan
    out["status"][:] = [0, 0, 1, 0, _lib.REFINE_NOT_REFINED]
    out["selection"] = np.array([4, 0, 9, 2, 11])
    out["summaries"] = dict(mean_z=rng.normal(size=(n, 1, 1)), quantiles_z=rng.normal(size=(n, 1, 1, 2)),
                            effective_samples=rng.uniform(1, 9, size=(n, 1)), status=np.array([[0], [0], [3], [0], [3]], dtype=np.int32),
                            probabilities=np.array([0.025, 0.975]), thresholds=np.array([20.3]), selection=out["selection"])
    path = str(tmp_path / "refined.mat")
    io.save_refined_results(path, out, levels=np.float64(L), note="unit test")
    back = io.load_refined_results(path)
    for k in refine.SCALARS + refine.TABLES + ("boxes", "status", "selection"):
        np.testing.assert_array_equal(back[k], out[k], err_msg=k)
        assert back[k].dtype == out[k].dtype, k
    for k, v in out["summaries"].items():
        np.testing.assert_array_equal(back["summaries"][k], v, err_msg=k)
    assert back["summaries"]["status"].dtype == np.int32 and float(np.asarray(back["levels"]).reshape(-1)[0]) == L
    # without the tables and the summaries
    slim = {k: v for k, v in out.items() if k not in refine.TABLES + ("summaries",)}
    io.save_refined_results(path, slim)
    back = io.load_refined_results(path)
    assert "summaries" not in back and not any(k in back for k in refine.TABLES)
    np.testing.assert_array_equal(back["boxes"], out["boxes"])


def test_empty_results_and_default_request():
    out = refine.empty_results(3, 2, 5, with_samples=False)
    assert out["boxes"].shape == (3, 2, 4) and (out["status"] == _lib.REFINE_NOT_REFINED).all() and "sample_log_likelihoods_refined" not in out
    rq = refine.request()
    assert (rq.levels, rq.delta, rq.pad) == (2, 12.5, 2.0)


@pytest.mark.parametrize("k,nl", RC.CONFIGS)
def test_the_twin_meets_what_the_gpu_test_asserts(k, nl):
    """On the CPU oracle alone: the two status rows are unusable and every other row is refined; at most 2 % of
    the rows have an ambiguous MAP (two largest lambda closer than 1e-9, far above any tolerance the GPU test
    derives); on the peaked rows the last level's ESS exceeds the first pass's and [q(0.025), q(0.975)] of the
    last level holds the injected absorber; the edge row's box is clipped at the end of the search range."""
    rows_seen = ambiguous = 0
    for Sr in RC.SR_VALUES:
        (model, samples, spectra, truth), first, rows = RC.twin(k, nl, Sr)
        u, v = RC.halton_points(Sr)
        for kind, ref, row, tr in zip(RC.KINDS, first, rows, truth):
            assert row["status"] == (1 if kind.startswith("status") else 0), kind
            if row["status"]:
                continue
            rows_seen += 1
            ambiguous += row["ambiguity"] <= 1e-9
            b = row["boxes"]
            assert (b[1:, 0] >= b[:-1, 0]).all() and (b[1:, 1] <= b[:-1, 1]).all() and (b[:, 0] >= ref["min_z_dla"]).all()
            if kind in RC.PEAKED:
                e0, e1 = RC.ess(ref["sample_log_likelihoods_dla"]), RC.ess(row["lam"][-1])
                s = PR.summaries(np.asarray(row["lam"][-1])[None, :], u, row["n"], b[-1, :1], b[-1, 1:2], probabilities=(0.025, 0.975))
                qz, qn = s["quantiles_z"][0, 0, 0], s["quantiles_log_nhi"][0, 0, 0]
                print(f"k {k} lines {nl} S' {Sr} {kind}: ESS {e0:.5f} -> {e1:.3f}; z [{qz[0]:.6f}, {qz[1]:.6f}] truth {tr[0]:.6f}; "
                      f"log N [{qn[0]:.4f}, {qn[1]:.4f}] truth {tr[1]}")
                assert e0 < 1.01 and e1 > e0
                assert qz[0] <= tr[0] <= qz[1] and qn[0] <= tr[1] <= qn[1], kind
        if k == 8:
            edge = rows[RC.KINDS.index("edge")]["boxes"]
            assert (edge[:, 1] == first[RC.KINDS.index("edge")]["max_z_dla"]).any()
    print(f"k {k} lines {nl}: {ambiguous} of {rows_seen} rows with an ambiguous MAP")
    assert rows_seen == 18 and ambiguous <= 0.02 * rows_seen


def test_twin_is_consistent_across_levels():
    """A run with fewer levels makes the leading boxes of a run with more (what lets the GPU test read level l's
    tables from a call with l levels)."""
    _, _, four = RC.twin(8, 3, 127, 4)
    _, _, two = RC.twin(8, 3, 127, 2)
    for a, b in zip(two, four):
        np.testing.assert_array_equal(a["boxes"], b["boxes"][:2])
        if not a["status"]:
            np.testing.assert_array_equal(a["lam"][1], b["lam"][1])


@pytest.mark.parametrize("k,nl", RC.CONFIGS)
def test_the_twin_on_a_search_range_of_zero_width(k, nl):
    """One kept pixel and max_z_cut = 0: the oracle's range is a point, the row is usable, every box stays on that z
    and the evidence is finite (the box's share of the prior's z range counts as 1)."""
    _, first, rows = RC.twin(k, nl, RC.ZR_SR, zero_range=True)
    i = RC.ZR_KINDS.index("zero_range")
    z0 = first[i]["min_z_dla"]
    assert first[i]["rc"] == 0 and z0 == first[i]["max_z_dla"] and first[0]["min_z_dla"] < first[0]["max_z_dla"]
    assert rows[i]["status"] == 0 and (rows[i]["boxes"][:, :2] == z0).all() and np.isfinite(rows[i]["log_z"])
    assert rows[i]["map_z"] == z0 and rows[i]["ambiguity"] > 1e-9 and rows[0]["status"] == 0
    b = rows[i]["boxes"]
    assert (b[1:, 2] >= b[:-1, 2]).all() and (b[1:, 3] <= b[:-1, 3]).all() and b[-1, 3] - b[-1, 2] < b[0, 3] - b[0, 2]


def test_restatement_log_prior_against_the_formula_read_literally():
    d = RC.test_prior()
    n = np.array([20.0, 20.1, 20.2, 20.25, 20.3, 20.7, 21.3, 21.300001, 22.5])
    got, ext = RR.log_prior(n, d, 20.0, 23.0), RR.log_prior(n, d, 20.0, 23.0, np.longdouble)
    c0, c1, c2 = d["coeff"]
    for x, g, e in zip(n, got, ext):
        t = max(x, d["flat_below"])
        p = d["alpha"] * math.exp(c0 + c1 * (t - d["centre"]) + c2 * (t - d["centre"]) ** 2) / d["Z"]
        if d["uniform_min"] <= x <= d["uniform_max"]:
            p += (1 - d["alpha"]) / (d["uniform_max"] - d["uniform_min"])
        assert abs(g - math.log(p)) <= 1e-14 * abs(math.log(p)) + 1e-15 and abs(float(e) - math.log(p)) <= 1e-14 * abs(math.log(p)) + 1e-15
    assert got[0] == got[1] == got[2]            # held flat below flat_below
    assert got[4] > got[3] and got[7] < got[6]    # the uniform component switches on at uniform_min and off above uniform_max
    assert (RR.log_prior(n, None, 20.0, 23.0) == -math.log(3.0)).all()
    # with a prior, a row's lambda is l' + log p_N(n') and the boxes follow lambda
    rng = np.random.default_rng(4)
    S = Sr = 40
    off, lnhi, u, v = rng.uniform(size=S), 20 + 3 * rng.uniform(size=S), rng.uniform(size=Sr), rng.uniform(size=Sr)
    sweep = _toy_sweep(2.4, 20.6, 0.05, 0.3)
    l = sweep(0, 2.0 + off, lnhi)
    a, b = RR.refine_row(l, off, lnhi, 2.0, 3.0, 0, u, v, sweep, 2), RR.refine_row(l, off, lnhi, 2.0, 3.0, 0, u, v, sweep, 2, prior=d)
    np.testing.assert_array_equal(a["boxes"][0], b["boxes"][0])
    np.testing.assert_array_equal(b["lam"][0], b["ell"][0] + RR.log_prior(b["boxes"][0][2] + (b["boxes"][0][3] - b["boxes"][0][2]) * v, d, 20.0, 23.0))
    assert a["log_z"] != b["log_z"]
