"""k_path_lengths and k_bootstrap_sums against their restatements, and DLAStatistics.sample_errors on the
consumer fixture run."""
import json
import math

import numpy as np
import pytest

import sample_error_restatement as R
from gp_dla_detection_amd import cddf, io
from test_cddf import combined, inputs  # noqa: F401  (module fixture)
from test_gpu_cddf import make_block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lowzcut", [False, True])
@pytest.mark.parametrize("snr_thresh", [-2, 1.0])
def test_path_length_matrix_against_path_length(lowzcut, snr_thresh):
    rng = np.random.default_rng(3)
    n = 400
    zmin = rng.uniform(1.5, 3.5, n)
    zmax = zmin + rng.uniform(0.0, 2.0, n)
    zmax[:5] = zmin[:5] + [0.0, 0.05, 0.1, 1e-9, 0.100001]              # empty and nearly empty ranges, the proximity zone
    zmin[5], zmax[5] = np.nan, 3.0
    zmin[6], zmax[6] = 2.0, np.nan
    zmin[7], zmax[7] = 0.5, 7.0                                          # covers every bin
    snrs = rng.uniform(-5, 5, n)
    snrs[:8] = 3.0
    for edges in (cddf.z_bins(2, 4), cddf.z_bins(2, 5), np.array([1.0, 6.0]), np.array([2.0, 2.05, 3.7, 3.71])):
        rows, dX = cddf.path_length_matrix(zmin, zmax, snrs, edges, snr_thresh=snr_thresh, lowzcut=lowzcut)
        np.testing.assert_array_equal(rows, np.flatnonzero(snrs > snr_thresh))
        assert dX.shape == (rows.size, len(edges) - 1) and np.all(np.isfinite(dX)) and np.all(dX >= 0)
        hi = np.maximum(np.minimum(zmax, zmax - 0.1), zmin) if lowzcut else zmax
        for b, (a, c) in enumerate(zip(edges[:-1], edges[1:])):
            want = cddf.path_length(zmin, zmax, snrs, a, c, snr_thresh=snr_thresh, lowzcut=lowzcut)
            got = math.fsum(dX[:, b])
            assert abs(got - want) <= 1e-12 * abs(want), (a, c, got, want)
            inside = (zmin[rows] < c) & (hi[rows] > a)
            assert np.all(dX[~inside, b] == 0.0) and np.count_nonzero(~inside) > 0      # exactly 0 outside the bin
            reach = inside & (np.minimum(hi[rows], c) > np.maximum(zmin[rows], a))
            assert np.all(dX[reach, b] > 0)
            k = int(np.flatnonzero(reach)[0])                            # one term against the host rule
            one = cddf.gauss_legendre_path(max(a, zmin[rows][k]), min(c, hi[rows][k]))
            assert abs(dX[k, b] - one) <= 1e-14 * one
    assert cddf.path_length_matrix(zmin, zmax, np.full(n, -9.0), [2.0, 3.0])[1].shape == (0, 1)


def bootstrap_case(n=700, C=70, seed=5):
    rng = np.random.default_rng(seed)
    V = rng.uniform(0, 1, (n, C)) * 10.0 ** rng.integers(-3, 22, C)[None, :]    # counts, N_HI moments, paths
    V[rng.uniform(size=(n, C)) < 0.6] = 0.0
    V[:, -1] = rng.normal(0.0, 1e15, n)                                  # a column whose terms cancel
    stratum = np.sort(rng.integers(0, 6, n)).astype(np.int32)
    stratum[stratum == 3] = 9                                            # labels need not be dense
    return V, np.sort(stratum)


def test_bootstrap_sums_against_fsum_and_bit_identity():
    V, stratum = bootstrap_case()
    seed = 0xC0FFEE123456789
    got = cddf.bootstrap_sums(V, stratum, 64, seed)
    want = R.bootstrap_sums(V, stratum, 64, seed)
    assert got.shape == want.shape == (64, 70)
    np.testing.assert_array_equal(got == 0, want == 0)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    assert np.unique(got[:, 0]).size > 60                               # replicates differ
    np.testing.assert_array_equal(cddf.bootstrap_sums(V, stratum, 64, seed), got)          # run to run
    split = np.concatenate([cddf.bootstrap_sums(V, stratum, 7, seed),
                            cddf.bootstrap_sums(V, stratum, 57, seed, first_replicate=7)])
    np.testing.assert_array_equal(split, got)                           # 64 = 7 + 57
    assert not np.array_equal(cddf.bootstrap_sums(V, stratum, 64, seed + 1), got)
    # shapes at the corners: one row, one column, 256 columns, a row count that is no multiple of 64 or 256
    for n, C in ((1, 1), (63, 3), (257, 256), (1000, 65)):
        V2, s2 = bootstrap_case(n, max(C, 2), seed=n)
        V2 = np.ascontiguousarray(V2[:, :C])
        np.testing.assert_allclose(cddf.bootstrap_sums(V2, s2, 5, 11), R.bootstrap_sums(V2, s2, 5, 11), rtol=1e-13, atol=1e-300)
    one = cddf.bootstrap_sums(np.arange(6.0).reshape(1, 6), np.zeros(1, dtype=np.int32), 3, 1)
    np.testing.assert_array_equal(one, np.tile(np.arange(6.0), (3, 1)))


def test_every_stratum_keeps_its_size():
    """An indicator column per stratum: every replicate sums it to the stratum's size, exactly."""
    sizes = [1, 10, 63, 64, 65, 300]
    stratum = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    V = (stratum[:, None] == np.arange(len(sizes))[None, :]).astype(np.float64)
    got = cddf.bootstrap_sums(V, stratum, 40, 99)
    np.testing.assert_array_equal(got, np.tile(np.asarray(sizes, dtype=np.float64), (40, 1)))


def test_replicate_variance_is_the_bootstrap_variance():
    """N iid sightlines in one stratum: the variance over replicates of a column sum estimates N times
    the (population) variance of the column.  A variance from R = 2000 draws has relative standard
    error sqrt(2 / R) = 3.2 %; the bound is five of them."""
    rng = np.random.default_rng(8)
    N, reps = 4000, 2000
    V = np.column_stack([rng.poisson(0.08, N).astype(np.float64), rng.exponential(1.0, N) * (rng.uniform(size=N) < 0.1),
                         rng.uniform(0.0, 0.7, N), np.ones(N)])
    sums = cddf.bootstrap_sums(V, np.zeros(N, dtype=np.int32), reps, 2024)
    for c in range(3):
        ratio = np.var(sums[:, c], ddof=1) / (N * np.var(V[:, c]))
        print(f"column {c}: replicate variance / (N x sample variance) = {ratio:.4f}")
        assert abs(ratio - 1) < 0.16
        assert abs(sums[:, c].mean() - V[:, c].sum()) < 5 * math.sqrt(N * np.var(V[:, c]) / reps)
    np.testing.assert_array_equal(sums[:, 3], np.full(reps, float(N)))


def synthetic_statistics(n=900, S=400, **kw):
    rng = np.random.default_rng(7)
    sll, shift, p_dla, zmin, zmax, _, off, lnhi = make_block(rng, n, S, edge_cases=False)
    p_dla[::3] = 0.01                                                   # a third is not selected but carries path
    res = dict(model_posteriors=np.stack([1 - p_dla, p_dla], axis=1), log_likelihoods_dla=shift - np.log(S),
               sample_log_likelihoods_dla=sll, min_z_dlas=zmin, max_z_dlas=zmax)
    snrs = rng.uniform(0, 8, n)
    return cddf.DLAStatistics(res, dict(offset_samples=off, log_nhi_samples=lnhi), snrs, sub_dla=False, occams_razor=1,
                              snr_thresh=1.0, **kw)


def test_sample_errors_do_not_depend_on_block_size_or_on_the_split_of_the_replicates():
    outs = [synthetic_statistics(block_size=bs).sample_errors(2, 5, replicates=64, seed=3, replicates_per_call=per)
            for bs, per in ((2048, None), (2048, None), (1, None), (7, None), (2048, 7), (2048, 57))]
    assert outs[0]["strata"].size > 1 and outs[0]["strata"].min() >= 10
    for o in outs[1:]:
        assert sorted(o) == sorted(outs[0])
        for k in outs[0]:
            np.testing.assert_array_equal(np.asarray(o[k]), np.asarray(outs[0][k]), err_msg=k)
    o = outs[0]
    assert o["dndx_replicates"].shape == (64, o["z_centres"].size) and o["cddf_replicates"].shape == (64, 30)
    assert np.all(np.isfinite(o["dndx_replicates"])) and np.all(o["dndx_point"] > 0) and np.all(o["omega_point"] > 0)
    # the point statistic is the expected count over the path: against the pieces it is made of
    st = synthetic_statistics()
    req = st._line_request(2, 5)
    (part,) = st.partials([req])
    zb = np.asarray(req.edges)
    dX = np.array([st.path_length(a, b) for a, b in zip(zb[:-1], zb[1:])])
    want = cddf.expected_counts(part, zb.size - 1).sum(axis=0) / dX
    np.testing.assert_allclose(o["dndx_point"], want[dX > 0], rtol=1e-12)
    om = st.omega_dla(2, 5)[1]
    np.testing.assert_allclose(o["omega_point"], om[dX > 0], rtol=1e-12)


def check_sample_errors(err, st, z_min, z_max):
    centres = st.line_density(z_min, z_max)[0]
    np.testing.assert_array_equal(err["z_centres"], centres)            # bins without path dropped as line_density drops them
    for name in ("dndx", "omega", "cddf"):
        med, r68, r95 = err[f"{name}_sample"], err[f"{name}_68_sample"], err[f"{name}_95_sample"]
        pt = err[f"{name}_point"]
        assert r68.shape == r95.shape == (2, med.size) and pt.shape == med.shape
        ok = np.isfinite(med)
        assert ok.any()
        assert np.all(r95[1][ok] <= r68[1][ok]) and np.all(r68[1][ok] <= med[ok])       # 2.5 <= 16 <= median
        assert np.all(med[ok] <= r68[0][ok]) and np.all(r68[0][ok] <= r95[0][ok])       # median <= 84 <= 97.5
        # the replicate median lies within the replicates' 2.5 / 97.5 range laid around the point estimate
        assert np.all(pt[ok] - (med[ok] - r95[1][ok]) <= med[ok] + 1e-300)
        assert np.all(med[ok] <= pt[ok] + (r95[0][ok] - med[ok]) + 1e-300)


def test_sample_errors_on_the_consumer_run(tmp_path, inputs):  # noqa: F811
    path = combined(tmp_path, False)
    res = io.load_processed_qsos(path)
    snrs = inputs["catalog"]["snrs"][inputs["test_ind"]]
    st = cddf.DLAStatistics(res, inputs["samples"], snrs, sub_dla=False)
    err = st.sample_errors(z_min=2, z_max=5, replicates=500, seed=1, lnhi_nbins=6)
    assert err["strata"].sum() == 32 and (err["strata"].size == 1 or err["strata"].min() >= 10)
    assert err["dndx_replicates"].shape == (500, err["z_centres"].size) and 0 < err["z_centres"].size <= 18
    check_sample_errors(err, st, 2, 5)
    assert np.nanmax(err["dndx_sample"]) > 0 and np.nanmax(err["omega_sample"]) > 0
    with pytest.raises(ValueError):
        st.sample_errors(replicates=0)
    with pytest.raises(ValueError):
        st.sample_errors(seed=float("nan"))
    big = synthetic_statistics()
    check_sample_errors(big.sample_errors(2, 5, replicates=300, seed=2), big, 2, 5)


def test_cli_adds_its_keys_and_leaves_the_rest(tmp_path, inputs):  # noqa: F811
    path = combined(tmp_path, False)
    plain, with_err = str(tmp_path / "plain.json"), str(tmp_path / "err.json")
    common = [path, inputs["paths"]["samples"], "--snrs", inputs["paths"]["snrs"], "--z-min", "2", "--z-max", "5",
              "--lnhi-nbins", "6"]
    cddf.main(common + ["--json", plain])
    cddf.main(common + ["--json", with_err, "--sample-errors", "50", "--seed", "7"])
    a, b = json.load(open(plain)), json.load(open(with_err))
    assert sorted(a) == ["column_density_function", "line_density", "omega_dla"]
    added = sorted(set(b) - set(a))
    assert added and all(k.startswith("sample_errors_") for k in added)
    for k in ("sample_errors_dndx_68_sample", "sample_errors_omega_95_sample", "sample_errors_cddf_sample",
              "sample_errors_z_centres", "sample_errors_seed", "sample_errors_replicates"):
        assert k in b
    assert b["sample_errors_seed"] == 7 and b["sample_errors_replicates"] == 50
    assert not any(k.endswith("_replicates") and k != "sample_errors_replicates" for k in b)
    assert list(b)[:len(a)] == list(a)
    assert json.dumps({k: b[k] for k in a}) == open(plain).read().strip()    # the rest of the JSON is unchanged
