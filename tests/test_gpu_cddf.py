"""k_bin_posteriors and k_poisson_binomial_cf against the numpy restatement (tests/cddf_restatement.py),
and DLAStatistics on the GPU against the reference's own DLACatalogue numbers."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import cddf_restatement as R
from gp_dla_detection_amd import _lib, cddf, io
from test_cddf import CONS, assert_reproduces, combined, inputs  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu

EDGES_Z = tuple(np.linspace(2.0, 5.0, 19))
EDGES_N = tuple(np.linspace(20.0, 23.0, 7))


def requests():
    return [cddf.BinRequest("z", EDGES_Z, 2.0, 5.0, 20.3, 23.0, lowzcut=True),
            cddf.BinRequest("lnhi", EDGES_N, 2.0, 5.0, 20.0, 23.0),
            cddf.BinRequest("z", EDGES_Z, 2.0, 5.0, 20.3, 23.0, histogram=True, moment=True),
            cddf.BinRequest("lnhi", EDGES_N, 1.0, 6.0, 19.0, 24.0, histogram=True)]


def fused(a, b, c):
    """fma(a, b, c) rounded once (exact rational arithmetic)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def edge_offset(zmin, zmax, e):
    """An offset whose z = zmin + (zmax - zmin) * off lands exactly on e when each operation is
    rounded, and off e when the multiply-add is fused; None if there is none nearby."""
    dz = zmax - zmin
    up = down = (e - zmin) / dz
    for _ in range(200):
        for cand in (up, down):
            if zmin + dz * cand == e and fused(dz, cand, zmin) != e:
                return float(cand)
        up, down = np.nextafter(up, 2.0), np.nextafter(down, -1.0)
    return None


def make_block(rng, n, S, edge_cases=True):
    """A block of selected spectra with peaked posteriors, and its sample set."""
    off = rng.uniform(0, 1, S)
    lnhi = rng.uniform(19.5, 23.2, S)
    zmin = rng.uniform(1.8, 2.6, n)
    zmax = zmin + rng.uniform(0.8, 2.8, n)
    p_dla = rng.uniform(0.06, 1.0, n)
    sll = np.empty((n, S))
    shift = rng.normal(-5000, 100, n)
    for s in range(n):
        w = rng.dirichlet(np.full(S, 0.05))
        sll[s] = np.log(np.maximum(w, 1e-300)) + shift[s]
    if edge_cases:
        lnhi[:5] = 21.2
        off[:5] = np.linspace(0.30, 0.34, 5)
        j = 5
        for s in range(0, n, 3):  # a sample exactly on a z edge, which a fused z would move
            for e in EDGES_Z[1:-1][s % 17:]:
                o = edge_offset(zmin[s], zmax[s], e)
                if o is not None and 0.0 <= o <= 1.0 and j < S:
                    off[j] = o
                    lnhi[j] = 21.0
                    sll[s, j] = shift[s] + math.log(0.2 / p_dla[s])
                    j += 1
                    break
        lnhi[-4:] = [20.0, 20.5, 21.5, 23.0]  # on lnhi edges
        if n > 6:
            sll[1] = np.nan                                    # a NaN row
            sll[2] = shift[2] - 1e4                            # nothing above p_thresh_sample
            sll[3, :] = shift[3] - 1e4                         # p exactly 1e-4 and exactly 0.25
            p_dla[3], p_dla[4] = 1e-4, 0.25
            sll[3, :5] = shift[3]
            sll[4, :] = shift[4] - 1e4
            sll[4, :5] = shift[4]
            sll[5, S // 2] = np.nan                            # one NaN sample
    return sll, shift, p_dla, zmin, zmax, zmax - 0.1, off, lnhi


def assert_partials_equal(got, want, rtol=1e-13):
    for g, w in zip(got, want):
        for k in ("pois", "mean", "var"):
            np.testing.assert_array_equal(np.isnan(g[k]), np.isnan(w[k]), err_msg=k)
            np.testing.assert_array_equal(g[k] == 0, w[k] == 0, err_msg=k)
            np.testing.assert_allclose(g[k], w[k], rtol=rtol, atol=0, equal_nan=True, err_msg=k)
        np.testing.assert_array_equal(g["count"], w["count"])
        np.testing.assert_array_equal(g["kept_bin"], w["kept_bin"])
        np.testing.assert_allclose(g["kept_p"], w["kept_p"], rtol=rtol, atol=0)


def test_bin_posteriors_against_the_restatement():
    rng = np.random.default_rng(11)
    blk = make_block(rng, 40, 3000)
    got = cddf.bin_posteriors(*blk, requests())
    want = R.bin_posteriors(*blk, requests())
    assert_partials_equal(got, want)
    # the edge cases took effect
    assert np.isnan(got[2]["mean"][1]).any() and np.isnan(got[3]["mean"][1]).any()
    assert not got[0]["pois"][2].any() and got[0]["count"][2] == 0
    assert got[1]["count"][4] >= 1 and not got[1]["pois"][3].any()   # p = 0.25 kept; p = 1e-4 dropped
    assert any(w["count"].sum() > 0 for w in want) and np.any(got[0]["pois"] > 0)


def test_bin_posteriors_short_rows_and_strides():
    rng = np.random.default_rng(5)
    sll, *rest = make_block(rng, 9, 1500, edge_cases=False)
    wide = np.full((9, 1600), np.inf)
    wide[:, :1500] = sll
    got = cddf.bin_posteriors(wide[:, :1500], *rest, requests()[:2])
    assert_partials_equal(got, R.bin_posteriors(sll, *rest, requests()[:2]))
    one = make_block(rng, 3, 1, edge_cases=False)
    assert_partials_equal(cddf.bin_posteriors(*one, requests()), R.bin_posteriors(*one, requests()))


def test_kept_capacity_overflow_names_the_spectrum():
    rng = np.random.default_rng(2)
    sll, shift, p_dla, zmin, zmax, up, off, lnhi = make_block(rng, 5, 200, edge_cases=False)
    lnhi[:] = 21.2
    sll[3] = shift[3] - 1e4
    sll[3, :10] = shift[3] + math.log(0.9 / p_dla[3])    # ten samples at p = 0.9, all in the window
    off[:10] = np.linspace(0.05, 0.35, 10)
    zmin[3], zmax[3] = 2.1, 4.9
    req = cddf.BinRequest("lnhi", EDGES_N, 2.0, 5.0, 20.0, 23.0)
    with pytest.raises(cddf.KeptCapacityError, match="spectrum 3 keeps 10"):
        cddf.bin_posteriors(sll, shift, p_dla, zmin, zmax, up, off, lnhi, [req])
    # through DLAStatistics, in the second of several blocks: the error names the quasar
    res = dict(model_posteriors=np.stack([1 - p_dla, p_dla], axis=1), log_likelihoods_dla=shift - np.log(200),
               sample_log_likelihoods_dla=sll, min_z_dlas=zmin, max_z_dlas=zmax)
    st = cddf.DLAStatistics(res, dict(offset_samples=off, log_nhi_samples=lnhi), np.ones(5), sub_dla=False,
                            occams_razor=1, block_size=2)
    assert st.selected.tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(cddf.KeptCapacityError, match="quasar 3 keeps 10"):
        st.partials([req])


def test_kept_probability_just_above_one():
    """A strong absorber: one sample carries the row, p_dla = 1, and p = exp(sll - shift) p_dla comes
    out one ulp above 1.  Both kernels take it, and the statistics come out as the restatement's."""
    above = np.nextafter(1.0, 2.0)
    segs = [np.array([0.5, above, 0.3]), np.array([above])]
    for (gl, ga), (wl, wa) in zip(cddf.poisson_binomial_cf(segs), R.cf_segments(segs)):
        np.testing.assert_allclose(gl, wl, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(ga, wa, rtol=1e-12, atol=1e-15)
    S = 50
    off = np.linspace(0.01, 0.99, S)
    lnhi = np.full(S, 21.2)
    sll = np.full((3, S), -1e4)
    shift = np.zeros(3)   # log_likelihoods_dla + log S == 0 exactly
    sll[:, 10] = 2.0 ** -52                  # p = exp(2^-52) * 1 = 1 + 2^-52
    sll[1, 30] = math.log(0.6)
    mp = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 1.0]])
    res = dict(model_posteriors=mp, log_likelihoods_dla=shift - np.log(S), sample_log_likelihoods_dla=sll,
               min_z_dlas=np.full(3, 2.1), max_z_dlas=np.full(3, 3.9))
    smp = dict(offset_samples=off, log_nhi_samples=lnhi)
    st = cddf.DLAStatistics(res, smp, np.ones(3), sub_dla=False, occams_razor=1)
    req = st._line_request(2, 4)
    (part,) = st.partials([req])
    assert part["count"].sum() == 4 and part["kept_p"].max() > 1.0
    zb = np.asarray(req.edges)
    dX = [st.path_length(a, b) for a, b in zip(zb[:-1], zb[1:])]
    got = st.line_density(2, 4)
    want_part = R.bin_posteriors(sll, st._shift, st.p_dla, res["min_z_dlas"], res["max_z_dlas"], st._upper_z, off,
                                 lnhi, [req])[0]
    want = cddf.line_density_from(want_part, zb, dX, R.cf_segments)
    for x, y in zip(got, want):
        np.testing.assert_allclose(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), rtol=1e-12)
    assert got[1].max() > 0


def test_abi_rejects_bad_requests():
    lib = _lib.load()
    e = np.array([2.0, 3.0, 3.0])
    reqs = (_lib.BinRequest * 1)(_lib.BinRequest(0, 2, _lib.ptr(e), 2.0, 3.0, 20.0, 23.0, 0, 0, 0, 1e-4, 0.25))
    outs = (_lib.BinOutput * 1)()
    one = np.zeros(1)
    rc = lib.gpdla_stats_bin_posteriors(1, 1, _lib.ptr(one), 1, *[_lib.ptr(one)] * 7, 1, reqs, outs, 0)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    rc = lib.gpdla_stats_bin_posteriors(1, 0, _lib.ptr(one), 1, *[_lib.ptr(one)] * 7, 1, reqs, outs, 0)
    assert rc == _lib.ERR_INVALID_ARGUMENT
    rc = lib.gpdla_stats_bin_posteriors(1, 1, _lib.ptr(one), 1, *[_lib.ptr(one)] * 7, 5, reqs, outs, 0)
    assert rc == _lib.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("multi", [False, True])
def test_dla_statistics_reproduce_the_reference(tmp_path, inputs, multi):  # noqa: F811
    exp = np.load(os.path.join(CONS, f"expected_dlacatalogue_{'multi' if multi else 'single'}.npz"))
    path = combined(tmp_path, multi)
    res = io.load_processed_qsos(path)
    snrs = inputs["catalog"]["snrs"][inputs["test_ind"]]
    st = cddf.DLAStatistics(res, inputs["samples"], snrs, sub_dla=multi)
    got = dict(line_density=st.line_density(z_min=2, z_max=5),
               column_density_function=st.column_density_function(z_min=2., z_max=5., lnhi_nbins=6),
               omega_dla=st.omega_dla(z_min=2, z_max=5))
    assert_reproduces(got, exp)
    # the streamed reader gives the same, and so does the one-pass statistics()
    f = cddf.DLAStatistics.from_processed_file(path, inputs["paths"]["samples"], inputs["paths"]["snrs"],
                                               sub_dla=multi, block_size=4)
    try:
        for req in list(st._cache):
            a, b = st.partials([req])[0], f.partials([req])[0]
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        one = f.statistics(z_min=2, z_max=5, lnhi_nbins=6)
        for name in got:
            for x, y in zip(got[name], one[name]):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    finally:
        f.close()


def test_bit_identical_across_runs_and_block_sizes():
    rng = np.random.default_rng(7)
    n, S = 60, 2000
    sll, shift, p_dla, zmin, zmax, _, off, lnhi = make_block(rng, n, S, edge_cases=False)
    mp = np.stack([1 - p_dla, p_dla], axis=1)
    lld = shift - np.log(S)
    res = dict(model_posteriors=mp, log_likelihoods_dla=lld, sample_log_likelihoods_dla=sll,
               min_z_dlas=zmin, max_z_dlas=zmax)
    smp = dict(offset_samples=off, log_nhi_samples=lnhi)
    outs = []
    for bs in (n, n, 1, 7):
        st = cddf.DLAStatistics(res, smp, np.ones(n), sub_dla=False, occams_razor=1, block_size=bs)
        outs.append(st.partials(requests()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_bin_posteriors_at_scale():
    """20 000 spectra x 10^4 samples; a random subset against the restatement."""
    rng = np.random.default_rng(13)
    n, S = 20000, 10000
    off = rng.uniform(0, 1, S)
    lnhi = rng.uniform(19.5, 23.2, S)
    zmin = rng.uniform(1.8, 2.6, n)
    zmax = zmin + rng.uniform(0.8, 2.8, n)
    p_dla = rng.uniform(0.06, 1.0, n)
    shift = rng.normal(-8000, 300, n)
    centre = rng.integers(0, S, n)
    sll = np.empty((n, S))
    j = np.arange(S)
    for s in range(n):  # peaked: a few hundred samples carry the mass, or (every fifth) a handful
        d = np.abs(j - centre[s])
        sll[s] = shift[s] - 3.0 * d - math.log(1.1) if s % 5 == 0 else shift[s] - 0.02 * d - math.log(100.0)
    sub = np.sort(rng.choice(n, 40, replace=False))
    sub[:3] = [0, 5, 10]  # peaked ones among them
    parts = []
    for a in range(0, n, 4096):
        parts.append(cddf.bin_posteriors(sll[a:a + 4096], shift[a:a + 4096], p_dla[a:a + 4096], zmin[a:a + 4096],
                                         zmax[a:a + 4096], zmax[a:a + 4096] - 0.1, off, lnhi, requests()))
    got = [{k: np.concatenate([p[r][k] for p in parts]) for k in parts[0][r]} for r in range(4)]
    want = R.bin_posteriors(sll[sub], shift[sub], p_dla[sub], zmin[sub], zmax[sub], zmax[sub] - 0.1, off, lnhi,
                            requests())
    assert_partials_equal([{k: g[k][sub] for k in g} for g in got], want)
    assert np.count_nonzero(got[0]["pois"]) > 1000 and got[2]["mean"].sum() > 0
    assert got[1]["count"].sum() > 100 and want[1]["count"].sum() > 0


def test_poisson_binomial_cf_at_5000():
    rng = np.random.default_rng(17)
    p = rng.uniform(0.25, 1.0, 5000)
    small = [rng.uniform(0, 1, k) for k in (1, 2, 30)]
    segs = [p, *small, np.zeros(0)]
    got = cddf.poisson_binomial_cf(segs)
    want = R.cf_segments(segs[:-1])
    for (gl, ga), (wl, wa), s in zip(got, want, segs):
        assert gl.size == (s.size + 1) // 2 + 1
        np.testing.assert_allclose(gl, wl, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ga, wa, rtol=1e-12, atol=1e-12)
    assert got[-1][0].tolist() == [0.0]
    # the pdf from the GPU sums against the long-double restatement of the whole product
    pdf = cddf.pdf_from_cf(*got[0], p.size).astype(np.float64)
    ref = cddf.pdf_from_cf(*want[0], p.size).astype(np.float64)
    np.testing.assert_allclose(pdf, ref, rtol=0, atol=1e-10)
    assert abs(math.fsum(pdf) - 1) < 1e-9
