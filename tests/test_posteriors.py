"""CPU checks of the parameter summaries: the NumPy restatement against a brute-force
reading of the definitions, the C entry's argument checks (no device needed), the JSON catalogue with
intervals, the summaries file, and the streaming reader against the in-memory path."""
import ctypes as C
import glob
import json
import math
import os

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, catalog, io, posteriors, synthetic

import posterior_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
CONS = os.path.join(HERE, "golden", "consumer")


# ---- the restatement against the definitions, by brute force ----

def brute(sll, base, off, lnhi, zmin, zmax, r, m, j, probs, thresholds):
    """Sort the (value, weight) pairs and search linearly; every sum by math.fsum."""
    S = sll.shape[2]
    l = [float(x) for x in sll[r, m - 1]]
    for i in range(S):
        if any(base[r, jj, i] == 0 for jj in range(m - 1)):
            l[i] = float("nan")
    real = [x for x in l if not math.isnan(x)]
    if not real or not math.isfinite(max(real)):
        return None
    mx = max(real)
    w = [0.0 if math.isnan(x) else float(np.exp(np.float64(x) - mx)) for x in l]
    b = [i if j == 0 else int(base[r, j - 1, i]) - 1 for i in range(S)]
    keep = [i for i in range(S) if w[i] > 0]
    z = {i: zmin + (zmax - zmin) * off[b[i]] for i in keep}
    n = {i: lnhi[b[i]] for i in keep}
    T = math.fsum(w[i] for i in keep)
    res = dict(ess=T * T / math.fsum(w[i] ** 2 for i in keep))
    for name, v in (("z", z), ("n", n)):
        mean = math.fsum(w[i] * v[i] for i in keep) / T
        res["mean_" + name] = mean
        res["std_" + name] = math.sqrt(math.fsum(w[i] * (v[i] - mean) ** 2 for i in keep) / T)
        pairs = sorted((v[i], w[i]) for i in keep)
        qs = []
        for p in probs:
            ans, run = pairs[-1][0], []
            for val, wt in pairs:
                run.append(wt)
                # F(val) counts every pair with the same value
                if math.fsum(x for vv, x in pairs if vv <= val) >= p * T:
                    ans = val
                    break
            qs.append(ans)
        res["q_" + name] = qs
    res["cov"] = math.fsum(w[i] * (z[i] - res["mean_z"]) * (n[i] - res["mean_n"]) for i in keep) / T
    res["exceed"] = [math.fsum(w[i] for i in keep if n[i] >= t) / T for t in thresholds]
    return res


@pytest.mark.parametrize("S,md", [(1, 1), (2, 2), (7, 3), (12, 4)])
def test_restatement_against_brute_force(S, md):
    sll, base, off, lnhi, z_min, z_max = R.make_case(S, md)
    if md > 1 and S >= 4:   # duplicated base samples in slots >= 2: equal values
        base[1, 0, :4] = 3
    probs, thr = R.PROBABILITIES, R.THRESHOLDS
    got = R.summaries(sll, off, lnhi, z_min, z_max, base, probs, thr)
    kinds = R.ROW_KINDS
    assert got["status"][kinds.index("all_nan")].tolist() == [1] * md
    assert got["status"][kinds.index("nan_max_z")].tolist() == [2] * md
    for r in range(len(kinds)):
        for m in range(1, md + 1):
            for j in range(md):
                at = (r, m - 1, j)
                want = brute(sll, base, off, lnhi, z_min[r], z_max[r], r, m, j, probs, thr) if j < m else None
                if want is None:
                    for k in R.FIELDS3:
                        assert np.isnan(got[k][at])
                    assert np.isnan(got["quantiles_z"][at]).all() and np.isnan(got["quantiles_log_nhi"][at]).all()
                    continue
                z_ok = not np.isnan(z_max[r])
                np.testing.assert_allclose(got["mean_log_nhi"][at], want["mean_n"], rtol=0, atol=1e-13)
                np.testing.assert_allclose(got["std_log_nhi"][at], want["std_n"], rtol=0, atol=1e-13)
                np.testing.assert_allclose(got["exceedance"][at], want["exceed"], rtol=0, atol=1e-13)
                np.testing.assert_allclose(got["effective_samples"][r, m - 1], want["ess"], rtol=1e-13)
                np.testing.assert_array_equal(got["quantiles_log_nhi"][at], want["q_n"])
                if z_ok:
                    np.testing.assert_allclose(got["mean_z"][at], want["mean_z"], rtol=0, atol=1e-13)
                    np.testing.assert_allclose(got["std_z"][at], want["std_z"], rtol=0, atol=1e-13)
                    np.testing.assert_allclose(got["cov"][at], want["cov"], rtol=0, atol=1e-13)
                    np.testing.assert_array_equal(got["quantiles_z"][at], want["q_z"])
                else:
                    assert np.isnan(got["mean_z"][at]) and np.isnan(got["quantiles_z"][at]).all()
    peaked = got["effective_samples"][kinds.index("peaked")]
    assert np.all(np.abs(peaked - 1.0) < 1e-6)   # the collapse is visible, not a precise measurement


def test_the_seeded_gpu_cases_are_rarely_ambiguous():
    """What tests/test_gpu_posteriors.py relies on, from the restatement alone: every compared case has
    an acceptable value, the restatement's own answer is one, and more than one value is acceptable in
    at most 2 % of all compared (row, model, slot, quantity, p) cases."""
    total = many = 0
    for S in R.S_VALUES:
        for md in R.MD_VALUES:
            ref = R.case_reference(S, md)
            for (r, m, j, qy, q), vals in ref["accept"].items():
                mine = ref["f64"]["quantiles_log_nhi" if qy else "quantiles_z"][r, m, j, q]
                assert vals.size >= 1 and mine in vals, (S, md, r, m, j, qy, q)
                total += 1
                many += vals.size > 1
    print(f"{many} of {total} compared cases have more than one acceptable value")
    assert total > 15000 and many <= 0.02 * total


# ---- the C entry: arguments are checked before the device is touched ----

def _call(lib, n=2, S=8, md=1, probs=(0.5,), thr=(20.3,), base="auto", stride=None):
    sll = np.zeros((n, md, S))
    off, lnhi, z0, z1 = np.linspace(0, 1, S), np.linspace(20, 23, S), np.full(n, 2.0), np.full(n, 3.0)
    rq = _lib.SummaryRequest()
    rq.num_models, rq.num_probabilities, rq.num_thresholds = md, len(probs), len(thr)
    for i, x in enumerate(probs[:8]):
        rq.probabilities[i] = x
    for i, x in enumerate(thr[:4]):
        rq.thresholds[i] = x
    out, ps = posteriors._outputs(n, max(md, 1), min(len(probs), 8), min(len(thr), 4))
    b = None
    if isinstance(base, np.ndarray):
        b = base
    elif base == "auto" and md > 1:
        b = np.ones((n, md - 1, S), dtype=np.uint32)
    rc = lib.gpdla_stats_parameter_summaries(n, S, _lib.ptr(sll), md * S if stride is None else stride,
                                             b.ctypes.data_as(_lib._u32p) if b is not None else None, _lib.ptr(z0),
                                             _lib.ptr(z1), _lib.ptr(off), _lib.ptr(lnhi), C.byref(rq), C.byref(ps), 0)
    return rc, lib.gpdla_last_error().decode()


def test_argument_validation_needs_no_gpu():
    lib = _lib.load()
    bad = [
        (dict(probs=(0.0,)), "probabilities[0]"), (dict(probs=(1.0,)), "probabilities[0]"),
        (dict(probs=(0.5, float("nan"))), "probabilities[1]"), (dict(probs=(0.5, 0.5)), "probabilities"),
        (dict(probs=(0.6, 0.4)), "probabilities"), (dict(probs=tuple(np.linspace(0.1, 0.9, 9))), "num_probabilities"),
        (dict(thr=(1.0,) * 5), "num_thresholds"), (dict(thr=(float("nan"),)), "thresholds[0]"),
        (dict(md=0), "num_models"), (dict(md=5), "num_models"),
        (dict(md=2, base=None), "base_sample_inds"), (dict(md=1, base=np.ones((2, 1, 8), dtype=np.uint32)), "base_sample_inds"),
        (dict(md=2, base=np.full((2, 1, 8), 9, dtype=np.uint32)), "base_sample_inds"),
        (dict(md=2, stride=8), "row_stride"),
    ]
    for kw, field in bad:
        rc, msg = _call(lib, **kw)
        assert rc == _lib.ERR_INVALID_ARGUMENT and field in msg, (kw, rc, msg)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    rc, msg = _call(lib, md=2)
    assert rc == (0 if has_gpu else _lib.ERR_NO_DEVICE), (rc, msg)
    with pytest.raises(ValueError):
        posteriors.check_request((0.5, 0.4), (20.3,))
    with pytest.raises(ValueError):
        posteriors.check_request((0.5,), (1, 2, 3, 4, 5))


# ---- JSON catalogue, summaries file, streaming reader: the kernel call answered by the restatement ----

def _restated(sll, base, z_min, z_max, offsets, lnhi, p, t, device):
    return R.summaries(sll, offsets, lnhi, z_min, z_max, base, p, t)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The committed multi-DLA consumer chunks as one processed file, and samples of its size."""
    tmp = tmp_path_factory.mktemp("posteriors")
    paths = sorted(glob.glob(os.path.join(CONS, "processed_qsos_multi_meanfluxsynth_[0-9]*.mat")))
    out = str(tmp / "processed.mat")
    io.combine_processed_chunks(paths, out)
    res = io.load_processed_qsos(out)
    S = res["sample_log_likelihoods_dla"].shape[2]
    return out, res, synthetic.make_samples(S)


def test_streaming_reader_equals_the_in_memory_path(run, monkeypatch):
    path, res, samples = run
    monkeypatch.setattr(posteriors, "_run", _restated)
    whole = posteriors.parameter_summaries(res["sample_log_likelihoods_dla"], samples, res["min_z_dlas"],
                                           res["max_z_dlas"], res["base_sample_inds"])
    nq, md = whole["status"].shape
    assert md >= 2 and (whole["status"] == 0).any()
    for bs in (1, 5, 2048):
        got = posteriors.from_processed_file(path, samples, block_size=bs)
        np.testing.assert_array_equal(got["selection"], np.arange(nq))
        for k in posteriors.FIELDS + ("correlation",):
            np.testing.assert_array_equal(got[k], whole[k], err_msg=f"{k} at block_size {bs}")
    sel = np.array([1, 2, 9, 20, nq - 1])
    for bs in (1, 3, 2048):
        got = posteriors.from_processed_file(path, samples, selection=sel, block_size=bs)
        for k in posteriors.FIELDS:
            np.testing.assert_array_equal(got[k], whole[k][sel], err_msg=f"{k} at block_size {bs}")
    got = posteriors.from_processed_file(path, samples, p_dla=0.5, block_size=4)
    np.testing.assert_array_equal(got["selection"], np.flatnonzero(res["p_dlas"] >= 0.5))
    sub = posteriors.from_processed_file(path, samples, sub_dla=True, block_size=7)
    want = posteriors.parameter_summaries(res["sample_log_likelihoods_lls"], posteriors.sub_dla_samples(samples),
                                          res["min_z_dlas"], res["max_z_dlas"])
    assert sub["status"].shape == (nq, 1)
    for k in posteriors.FIELDS:
        np.testing.assert_array_equal(sub[k], want[k])


def test_summaries_file_round_trip(run, monkeypatch, tmp_path):
    path, res, samples = run
    monkeypatch.setattr(posteriors, "_run", _restated)
    sel = np.array([0, 3, 4, 17])
    out = posteriors.from_processed_file(path, samples, selection=sel, thresholds=(20.3, 21.5))
    f = str(tmp_path / "summaries.mat")
    io.save_parameter_summaries(f, out, processed_file=path)
    back = io.load_parameter_summaries(f)
    assert back["processed_file"] == path and back["status"].dtype == np.int32
    for k in posteriors.FIELDS + ("correlation", "probabilities", "thresholds", "selection"):
        assert back[k].shape == np.asarray(out[k]).shape, k
        np.testing.assert_array_equal(back[k], out[k], err_msg=k)
    raw = io.loadmat73(f)
    assert raw["quantiles_z"].shape == out["quantiles_z"].shape and raw["quasar_ind"].ravel().tolist() == (sel + 1).tolist()


def test_json_catalogue_with_intervals(run, monkeypatch, tmp_path):
    path, res, samples = run
    monkeypatch.setattr(posteriors, "_run", _restated)
    inputs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=40, num_samples=24, empty_quasar=None)
    t, c = inputs["test_ind"], inputs["catalog"]
    info = {k: c[k][t] for k in ("ras", "decs", "plates", "mjds", "fiber_ids", "thing_ids", "z_qsos", "snrs")}
    summ = posteriors.from_processed_file(path, samples, thresholds=(20.3, 21.0))
    plain = catalog.generate_json_catalogue(res, info)
    assert plain == json.load(open(os.path.join(CONS, "expected_predictions_multi_DLAs.json")))
    rich = catalog.generate_json_catalogue_with_intervals(res, info, summ, outfile=str(tmp_path / "rich.json"))
    assert len(rich) == len(plain) and any(r["dlas"] for r in rich)
    added = {"log_nhi_mean", "log_nhi_std", "z_dla_mean", "z_dla_std", "p_log_nhi_ge_20.3", "p_log_nhi_ge_21"} | {
        f"{n}_q{p:.6g}" for n in ("log_nhi", "z_dla") for p in posteriors.DEFAULT_PROBABILITIES}
    _, _, keep = catalog.loader_view(res, info)
    for a, b, i in zip(rich, plain, keep):
        a = json.loads(json.dumps(a))
        ess = a.pop("effective_samples")
        n = a["num_dlas"]
        assert (ess is None) == (n == 0)
        for j, d in enumerate(a["dlas"]):
            assert added <= set(d), sorted(added - set(d))
            assert d["log_nhi_q0.025"] <= d["log_nhi_q0.5"] <= d["log_nhi_q0.975"]
            assert d["z_dla_mean"] == summ["mean_z"][i, n - 1, j] and ess == summ["effective_samples"][i, n - 1]
            for k in added:
                del d[k]
        assert a == b
    assert json.load(open(tmp_path / "rich.json")) == json.loads(json.dumps(rich))
    # NaN summaries serialise (as the reference's json.dump writes NaN), and a selection is honoured
    part = posteriors.from_processed_file(path, samples, selection=keep[:3])
    for k in ("mean_z", "quantiles_z", "effective_samples"):
        part[k][...] = np.nan
    text = json.dumps(catalog.generate_json_catalogue_with_intervals(res, info, part))
    assert json.loads(text)[5]["effective_samples"] is None


def test_command_line_writes_summaries_and_json(run, monkeypatch, tmp_path, capsys):
    path, res, _ = run
    monkeypatch.setattr(posteriors, "_run", _restated)
    inputs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=40, num_samples=24, empty_quasar=None)
    out, js = str(tmp_path / "summaries.mat"), str(tmp_path / "with_intervals.json")
    assert posteriors.main([path, inputs["paths"]["samples"], out, "--thresholds", "20.3", "21", "--block-size", "5",
                            "--json", js, "--catalog", inputs["paths"]["catalog"]]) == 0
    back = io.load_parameter_summaries(out)
    samples = io.load_dla_samples(inputs["paths"]["samples"])
    want = posteriors.parameter_summaries(res["sample_log_likelihoods_dla"], samples, res["min_z_dlas"], res["max_z_dlas"],
                                          res["base_sample_inds"], thresholds=(20.3, 21.0))
    for k in posteriors.FIELDS + ("correlation",):
        np.testing.assert_array_equal(back[k], want[k], err_msg=k)
    recs = json.load(open(js))
    ref = json.load(open(os.path.join(CONS, "expected_predictions_multi_DLAs.json")))
    assert len(recs) == len(ref) and [r["thing_id"] for r in recs] == [r["thing_id"] for r in ref]
    assert any("log_nhi_q0.5" in d for r in recs for d in r["dlas"])
    # a selection by p_dla, the sub-DLA table
    assert posteriors.main([path, inputs["paths"]["samples"], out, "--p-dla", "0.5", "--sub-dla"]) == 0
    back = io.load_parameter_summaries(out)
    np.testing.assert_array_equal(back["selection"], np.flatnonzero(res["p_dlas"] >= 0.5))
    assert back["status"].shape[1] == 1 and back["sub_dla"] == 1.0
