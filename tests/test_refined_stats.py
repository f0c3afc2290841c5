"""CPU checks of what carries the refine pass into P(DLA), the catalogue and the CDDF: the
restatement (tests/refined_stats_restatement.py) against plain Python loops, the library's argument checks
of gpdla_stats_bin_posteriors_boxed (they run before the device is touched), the file round trip of the new
keys, and the refined JSON catalogue on a hand-made run.

test_restatement_against_loops and test_refined_posteriors_restatement check the yardstick itself: they run no
code of the package's new entries, pass without the feature, and do not count among the tests that fail
without it.  Every other test here does."""
import math

import numpy as np
import pytest

import refined_stats_restatement as RS
from gp_dla_detection_amd import _lib, catalog, cddf, io, refine

EDGES_Z = tuple(np.linspace(2.0, 5.0, 19))
EDGES_N = tuple(np.linspace(20.0, 23.0, 7))


def requests():
    return [cddf.BinRequest("z", EDGES_Z, 2.0, 5.0, 20.3, 23.0, lowzcut=True),
            cddf.BinRequest("lnhi", EDGES_N, 2.0, 5.0, 20.0, 23.0),
            cddf.BinRequest("z", EDGES_Z, 2.0, 5.0, 20.3, 23.0, histogram=True, moment=True),
            cddf.BinRequest("lnhi", EDGES_N, 1.0, 6.0, 19.0, 24.0, histogram=True)]


# ---------------------------------------------------------------------------------------------
# the contract in loops
# ---------------------------------------------------------------------------------------------

def loop_shift(row):
    finite = [float(x) for x in row if not math.isnan(x)]
    if not finite:
        return math.nan
    m = max(finite)
    if math.isinf(m):
        return math.nan
    return m + math.log(math.fsum(math.exp(x - m) for x in finite))


def loop_row(row, shift, p_dla, box, upper_z, u, v, req):
    """One row and one request, sample by sample."""
    z_lo, z_hi, n_lo, n_hi = box
    e = req.edges
    nb = len(e) - 1
    small = [[] for _ in range(nb)]
    kept = []
    wm_terms, wv_terms = [[] for _ in range(nb)], [[] for _ in range(nb)]
    poison = [False] * nb
    for j in range(len(row)):
        x = row[j] - shift
        p = (math.nan if math.isnan(x) else math.exp(x)) * p_dla
        z = z_lo + (z_hi - z_lo) * u[j]
        l = n_lo + (n_hi - n_lo) * v[j]
        q = l if req.quantity == "lnhi" else z
        if not req.histogram:
            z_up = min(upper_z, req.z_hi) if req.lowzcut else req.z_hi
            if not (req.lnhi_lo < l < req.lnhi_hi and req.z_lo < z < z_up and p > req.p_thresh_sample):
                continue
            for b in range(nb):
                if e[b] < q < e[b + 1]:
                    if p < req.p_switch:
                        small[b].append(p)
                    else:
                        kept.append((b, p))
        else:
            if not (req.lnhi_lo < l < req.lnhi_hi and req.z_lo < z < req.z_hi):
                continue
            w = 10.0 ** l if req.moment else 1.0
            wm, wv = w * p, w * w * (1 - p) * p
            for b in range(nb):
                below = q <= e[b + 1] if b == nb - 1 else q < e[b + 1]
                if q >= e[b] and below:
                    wm_terms[b].append(wm)
                    wv_terms[b].append(wv)
                if below and math.isnan(wm):
                    poison[b] = True
    if req.histogram:
        mean = [math.nan if poison[b] else math.fsum(wm_terms[b]) for b in range(nb)]
        var = [math.nan if poison[b] else math.fsum(wv_terms[b]) for b in range(nb)]
        return dict(mean=mean, var=var)
    return dict(pois=[math.fsum(s) for s in small], kept=kept)


def make_rows(rng, n, S):
    u, v = rng.uniform(0, 1, S), rng.uniform(0, 1, S)
    z_lo = rng.uniform(2.0, 3.0, n)
    n_lo = rng.uniform(20.1, 21.0, n)
    boxes = np.stack([z_lo, z_lo + rng.uniform(0.01, 0.8, n), n_lo, n_lo + rng.uniform(0.05, 1.5, n)], axis=1)
    lam = np.empty((n, S))
    for s in range(n):
        lam[s] = np.log(np.maximum(rng.dirichlet(np.full(S, 0.3)), 1e-300)) + rng.normal(-900, 200)
    return lam, rng.uniform(0.06, 1.0, n), boxes, boxes[:, 1] + rng.uniform(-0.3, 0.3, n), u, v


def test_restatement_against_loops():
    rng = np.random.default_rng(3)
    lam, p_dla, boxes, upper_z, u, v = make_rows(rng, 7, 90)
    lam[1, ::7] = np.nan                      # NaN entries
    lam[2] = np.nan                           # an all-NaN row
    boxes[3, 1] = boxes[3, 0]                 # a zero-width box in z
    boxes[4, 3] = boxes[4, 2] = 21.25         # ... and in log N
    lam[5, :] = -np.inf                       # no finite entry
    lam[6, 11] = np.inf
    lam[4, :3] = lam[4].max() + 3.0           # large p: kept pairs
    p_dla[4] = 0.95
    shift = RS.row_shifts(lam)
    assert np.isnan(shift[[2, 5, 6]]).all() and np.isfinite(shift[[0, 1, 3, 4]]).all()
    for s in range(lam.shape[0]):
        want = loop_shift(lam[s])
        assert (math.isnan(want) and math.isnan(shift[s])) or abs(shift[s] - want) <= 4 * np.spacing(abs(want)), s
    got = RS.bin_posteriors_boxed(lam, shift, p_dla, boxes, upper_z, u, v, requests())
    some = 0
    for r, req in enumerate(requests()):
        for s in range(lam.shape[0]):
            want = loop_row(lam[s], shift[s], p_dla[s], boxes[s], upper_z[s], u, v, req)
            if req.histogram:
                for k in ("mean", "var"):
                    np.testing.assert_array_equal(np.isnan(got[r][k][s]), np.isnan(want[k]), err_msg=f"{k} row {s}")
                    np.testing.assert_allclose(got[r][k][s], want[k], rtol=1e-13, atol=0, equal_nan=True)
                some += int(np.nansum(np.asarray(want["mean"]) > 0))
            else:
                np.testing.assert_allclose(got[r]["pois"][s], want["pois"], rtol=1e-13, atol=0)
                assert got[r]["count"][s] == len(want["kept"])
                for i, (b, p) in enumerate(want["kept"][:cddf.KEPT_CAPACITY]):
                    assert got[r]["kept_bin"][s, i] == b
                    np.testing.assert_allclose(got[r]["kept_p"][s, i], p, rtol=1e-13)
                some += len(want["kept"]) + int(np.sum(np.asarray(want["pois"]) > 0))
    assert some > 20
    # a NaN shift poisons every histogram bin a sample of the window reaches, and keeps nothing
    assert np.isnan(got[3]["mean"][2]).any() and got[1]["count"][2] == 0 and not got[1]["pois"][2].any()
    assert got[1]["count"][4] >= 1                                     # the zero-width log N box keeps its pairs
    # one sample
    one = make_rows(rng, 2, 1)
    sh = RS.row_shifts(one[0])
    np.testing.assert_array_equal(sh, one[0][:, 0])                    # m + log(1)
    g = RS.bin_posteriors_boxed(one[0], sh, *one[1:], requests())
    for r, req in enumerate(requests()):
        for s in range(2):
            want = loop_row(one[0][s], sh[s], one[1][s], one[2][s], one[3][s], one[4], one[5], req)
            for k in ("mean", "var") if req.histogram else ("pois",):
                np.testing.assert_allclose(g[r][k][s], want[k], rtol=1e-13, atol=0)


def test_refined_posteriors_restatement():
    lp_no = np.array([-1000.0, -990.0, np.nan, -1000.0])
    lp_dla = np.array([-995.0, -1200.0, -900.0, np.nan])
    status = np.array([0, 0, 1, -1])
    first = np.array([[0.3, 0.7], [0.6, 0.4], [np.nan, np.nan], [0.9, 0.1]])
    mp, p_no, p_dla, refined = RS.refined_posteriors(lp_no, lp_dla, status, first, first[:, 0], 1 - first[:, 0])
    assert refined.tolist() == [1, 1, 0, 0]
    assert mp[0, 1] == pytest.approx(1 / (1 + math.exp(-5.0)), rel=1e-15) and p_dla[0] == 1 - mp[0, 0]
    assert mp[1, 0] == 1.0 and mp[1, 1] == math.exp(-210.0) and p_dla[1] == 0.0
    np.testing.assert_array_equal(mp[2:], first[2:])
    np.testing.assert_array_equal(p_no[2:], first[2:, 0])


# ---------------------------------------------------------------------------------------------
# the library's argument checks need no GPU
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def _call(lib, n=1, S=2, stride=2, lam=True, p=True, boxes=True, upper=True, u=(0.25, 0.5), v=(0.25, 0.5), R=1,
          edges=(2.0, 3.0, 4.0), reqs=True, outs=True, shift=True):
    e = np.array(edges, dtype=np.float64)
    rq = (_lib.BinRequest * 5)(*[_lib.BinRequest(0, e.size - 1, _lib.ptr(e), 2.0, 4.0, 20.0, 23.0, 0, 0, 0, 1e-4, 0.25)] * 5)
    hold = [np.zeros((n, e.size - 1)) for _ in range(2)] + [np.zeros(n, dtype=np.int32), np.zeros((n, 8), dtype=np.int32),
                                                               np.zeros((n, 8))]
    ot = (_lib.BinOutput * 5)(*[_lib.BinOutput(_lib.ptr(hold[0]), None, None, hold[2].ctypes.data_as(_lib._i32p),
                                                hold[3].ctypes.data_as(_lib._i32p), _lib.ptr(hold[4]))] * 5)
    a = dict(lam=np.zeros((n, stride)), p=np.ones(n), boxes=np.tile([2.0, 3.0, 20.0, 21.0], (n, 1)), upper=np.full(n, 3.0),
             u=np.array(u, dtype=np.float64), v=np.array(v, dtype=np.float64), shift=np.zeros(n))
    ptr = lambda key, on: _lib.ptr(a[key]) if on else None   # noqa: E731
    return lib.gpdla_stats_bin_posteriors_boxed(n, S, ptr("lam", lam), stride, ptr("p", p), ptr("boxes", boxes), ptr("upper", upper),
                                                ptr("u", u is not None), ptr("v", v is not None), R, rq if reqs else None,
                                                ot if outs else None, ptr("shift", shift), 0)


@pytest.mark.parametrize("kw,what", [
    (dict(lam=False), "null per-row"), (dict(p=False), "null per-row"), (dict(boxes=False), "null per-row"),
    (dict(upper=False), "null per-row"), (dict(shift=False), "null shift"), (dict(reqs=False), "bin requests"),
    (dict(outs=False), "bin requests"), (dict(stride=1), "row_stride"), (dict(S=0), "S' >= 1"),
    (dict(edges=(2.0, 3.0, 3.0)), "strictly increasing"), (dict(edges=(2.0, np.nan, 3.0)), "strictly increasing"),
    (dict(R=5), "bin requests"), (dict(R=0), "bin requests"),
    (dict(u=(0.25, 1.0)), r"u\[1\]"), (dict(u=(-0.1, 0.5)), r"u\[0\]"), (dict(v=(0.25, np.nan)), r"v\[1\]"),
    (dict(v=(1.5, 0.5)), r"v\[0\]"),
])
def test_boxed_entry_refuses_before_the_device(lib, kw, what):
    import re
    assert _call(lib, **kw) == _lib.ERR_INVALID_ARGUMENT
    assert re.search(what, lib.gpdla_last_error().decode())


def test_boxed_entry_null_points_and_empty_block(lib):
    e = np.array([2.0, 3.0])
    rq = (_lib.BinRequest * 1)(_lib.BinRequest(0, 1, _lib.ptr(e), 2.0, 3.0, 20.0, 23.0, 1, 0, 0, 1e-4, 0.25))
    ot = (_lib.BinOutput * 1)()
    u = np.array([0.5])
    assert lib.gpdla_stats_bin_posteriors_boxed(0, 1, None, 1, None, None, None, None, _lib.ptr(u), 1, rq, ot, None, 0) \
        == _lib.ERR_INVALID_ARGUMENT
    # no rows: the checks pass and the device is not needed
    assert lib.gpdla_stats_bin_posteriors_boxed(0, 1, None, 1, None, None, None, _lib.ptr(u), _lib.ptr(u), 1, rq, ot, None, 0) == 0


def test_python_wrapper_checks_shapes():
    with pytest.raises(ValueError, match="boxes"):
        cddf.bin_posteriors_boxed(np.zeros((2, 3)), np.ones(2), np.zeros((2, 3)), np.ones(2), np.zeros(3), np.zeros(3), requests())
    with pytest.raises(ValueError, match="3 sample columns"):
        cddf.bin_posteriors_boxed(np.zeros((2, 3)), np.ones(2), np.zeros((2, 4)), np.ones(2), np.zeros(2), np.zeros(3), requests())


# ---------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------

def hand_refined(n=3, levels=2, Sr=5, with_tables=True, with_posteriors=True):
    rng = np.random.default_rng(8)
    out = refine.empty_results(n, levels, Sr, with_tables)
    for k in refine.SCALARS:
        out[k] = rng.normal(size=n)
    out["boxes"] = rng.normal(size=(n, levels, 4))
    out["status"] = np.array([0, 1, 0][:n], dtype=np.int32)
    out["selection"] = np.array([4, 1, 7][:n])
    if with_tables:
        for k in refine.TABLES:
            out[k] = rng.normal(size=(n, Sr))
        out["refine_u"], out["refine_v"] = rng.uniform(size=Sr), rng.uniform(size=Sr)
    if with_posteriors:
        p = rng.uniform(size=n)
        out.update(model_posteriors_refined=np.stack([p, 1 - p], axis=1), p_no_dlas_refined=p, p_dlas_refined=1 - p,
                   refined=np.array([1, 0, 1][:n], dtype=np.int32))
    return out


@pytest.mark.parametrize("slab", [None, 48])   # 48 B: the tables go out two sample columns at a time
def test_refined_results_round_trip_with_the_new_keys(tmp_path, monkeypatch, slab):
    if slab:
        monkeypatch.setattr(io, "REFINED_SLAB_BYTES", slab)
    ref = hand_refined()
    path = str(tmp_path / "refined.mat")
    io.save_refined_results(path, ref, levels=np.float64(2))
    back = io.load_refined_results(path)
    for k in refine.POSTERIORS + refine.POINTS + refine.TABLES + refine.SCALARS + ("boxes", "status", "selection"):
        np.testing.assert_array_equal(back[k], ref[k], err_msg=k)
        assert back[k].shape == np.asarray(ref[k]).shape, k
    assert back["refined"].dtype == np.int32
    # a file written without the switches holds what it held before
    plain = hand_refined(with_tables=False, with_posteriors=False)
    io.save_refined_results(path, plain)
    back = io.load_refined_results(path)
    assert not any(k in back for k in refine.POSTERIORS + refine.POINTS + refine.TABLES)
    assert set(back) == set(refine.SCALARS) | {"boxes", "status", "selection"}


def test_statistics_refuse_refined_results_without_tables(tmp_path):
    n, S = 9, 4
    res = dict(model_posteriors=np.full((n, 2), 0.5), log_likelihoods_dla=np.zeros(n), sample_log_likelihoods_dla=np.zeros((n, S)),
               min_z_dlas=np.full(n, 2.0), max_z_dlas=np.full(n, 3.0))
    smp = dict(offset_samples=np.linspace(0.1, 0.9, S), log_nhi_samples=np.full(S, 21.0))
    path = str(tmp_path / "refined.mat")
    io.save_refined_results(path, hand_refined(with_tables=False))
    for given in (path, hand_refined(with_tables=False)):
        with pytest.raises(ValueError, match="--tables"):
            cddf.DLAStatistics(res, smp, np.ones(n), sub_dla=False, refined=given)
    with pytest.raises(ValueError, match="--posteriors"):
        cddf.DLAStatistics(res, smp, np.ones(n), sub_dla=False, refined=hand_refined(with_posteriors=False))
    multi = dict(res, sample_log_likelihoods_dla=np.zeros((n, 2, S)), model_posteriors=np.full((n, 4), 0.25),
                 log_likelihoods_dla=np.zeros((n, 2)))
    with pytest.raises(ValueError, match="single-DLA"):
        cddf.DLAStatistics(multi, smp, np.ones(n), sub_dla=True, refined=hand_refined())
    # accepted: the refined P(DLA) of the status-0 rows (Occam's razor on the refined pair) enters the selection
    ref = hand_refined()
    ref["model_posteriors_refined"][0] = (1e-9, 1 - 1e-9)
    ref["model_posteriors_refined"][2] = (0.999, 0.001)
    st = cddf.DLAStatistics(res, smp, np.ones(n), sub_dla=False, refined=ref, p_thresh_spec=1e-3)
    want = catalog.occams_model_posteriors(ref["model_posteriors_refined"][[0, 2]])[:, 1]
    np.testing.assert_array_equal(st.p_dla[[4, 7]], want)
    assert st.p_dla[1] == st.p_dla[0] and 4 in st.selected and 7 not in st.selected and 1 not in st.selected


# ---------------------------------------------------------------------------------------------
# the refined catalogue
# ---------------------------------------------------------------------------------------------

def hand_run():
    nq = 5
    mp = np.array([[0.2, 0.8], [1e-12, 1.0], [np.nan, np.nan], [0.999, 0.001], [1e-10, 1.0]])
    results = dict(model_posteriors=mp, p_dlas=mp[:, 1], p_no_dlas=mp[:, 0], min_z_dlas=np.full(nq, 2.0),
                   max_z_dlas=np.full(nq, 3.0), MAP_z_dlas=np.array([2.1, 2.2, np.nan, 2.4, 2.5]),
                   MAP_log_nhis=np.array([20.1, 20.2, np.nan, 20.4, 20.5]))
    info = dict(ras=np.arange(nq) * 1.5, snrs=np.full(nq, 3.0), decs=np.arange(nq) * -1.0, plates=np.arange(nq) + 4000,
                mjds=np.arange(nq) + 55000, fiber_ids=np.arange(nq) + 1, thing_ids=np.arange(nq) + 100, z_qsos=np.full(nq, 3.2))
    # quasar 1: refined; quasar 4: in the selection but unusable; quasar 2: NaN (skipped by the sweep), in the selection
    refined = dict(selection=np.array([1, 4, 2]), refined=np.array([1, 0, 0], dtype=np.int32),
                   status=np.array([0, 1, 1], dtype=np.int32),
                   model_posteriors_refined=np.array([[1e-30, 1.0], [1e-10, 1.0], [np.nan, np.nan]]),
                   MAP_z_dlas_refined=np.array([2.2345, np.nan, np.nan]), MAP_log_nhis_refined=np.array([21.234, np.nan, np.nan]))
    Q, T = 3, 1
    summ = dict(selection=refined["selection"], probabilities=np.array([0.16, 0.5, 0.84]), thresholds=np.array([20.3]),
                status=np.array([[0], [1], [1]], dtype=np.int32), effective_samples=np.array([[41.5], [np.nan], [np.nan]]),
                mean_z=np.full((3, 1, 1), 2.23), std_z=np.full((3, 1, 1), 0.01), mean_log_nhi=np.full((3, 1, 1), 21.2),
                std_log_nhi=np.full((3, 1, 1), 0.05), cov=np.zeros((3, 1, 1)), quantiles_z=np.full((3, 1, 1, Q), 2.23),
                quantiles_log_nhi=np.full((3, 1, 1, Q), 21.2), exceedance=np.full((3, 1, 1, T), 1.0))
    return results, info, refined, summ


def test_refined_catalogue():
    results, info, refined, summ = hand_run()
    out = catalog.generate_json_catalogue_refined(results, info, refined)
    assert [r["thing_id"] for r in out] == [100, 101, 103, 104]          # the NaN quasar is dropped
    assert [r["refined"] for r in out] == [False, True, False, False]
    first = catalog.generate_json_catalogue(dict(results, MAP_z_dlas=results["MAP_z_dlas"].reshape(-1, 1, 1),
                                                 MAP_log_nhis=results["MAP_log_nhis"].reshape(-1, 1, 1)), info, sub_dla=False)
    for got, want in zip(out, first):                                    # the layout, and the unrefined records
        assert set(got) == set(want) | {"refined"}
        if not got["refined"]:
            assert {k: v for k, v in got.items() if k != "refined"} == want
    rec = out[1]
    mp = catalog.occams_model_posteriors(refined["model_posteriors_refined"][:1])
    assert rec["p_dla"] == mp[0, 1] and rec["p_no_dla"] == mp[0, 0] and rec["p_dla"] != first[1]["p_dla"]
    assert rec["num_dlas"] == 1 and rec["dlas"] == [{"log_nhi": 21.234, "z_dla": 2.2345}]
    assert out[3]["dlas"] == [{"log_nhi": 20.5, "z_dla": 2.5}]           # unusable in the refine: the first pass's
    # keeping the NaN quasar
    assert len(catalog.generate_json_catalogue_refined(results, info, refined, drop_nan=False)) == 5
    # with the refined summaries: the interval fields on the refined quasar alone
    full = catalog.generate_json_catalogue_refined(results, info, refined, summ)
    assert full[1]["effective_samples"] == 41.5 and full[1]["dlas"][0]["log_nhi_mean"] == 21.2
    assert full[1]["dlas"][0]["z_dla_std"] == 0.01 and any(k.startswith("z_dla_q") for k in full[1]["dlas"][0])
    assert full[3]["effective_samples"] is None and set(full[3]["dlas"][0]) == {"log_nhi", "z_dla"}
    assert full[0]["effective_samples"] is None and [r["refined"] for r in full] == [r["refined"] for r in out]


def test_refined_catalogue_writes_a_file_and_refuses_multi_dla(tmp_path):
    import json
    results, info, refined, _ = hand_run()
    path = str(tmp_path / "cat.json")
    out = catalog.generate_json_catalogue_refined(results, info, refined, outfile=path)
    assert json.load(open(path)) == out
    multi = dict(results, model_posteriors=np.full((5, 6), 1 / 6), MAP_z_dlas=np.zeros((5, 4, 4)), MAP_log_nhis=np.zeros((5, 4, 4)))
    with pytest.raises(ValueError, match="single-DLA"):
        catalog.generate_json_catalogue_refined(multi, info, refined)
    with pytest.raises(ValueError, match="model_posteriors_refined"):
        catalog.generate_json_catalogue_refined(results, info, {k: v for k, v in refined.items() if k != "model_posteriors_refined"})
