"""The CDDF statistics' host side (gp_dla_detection_amd/cddf.py) driven from the numpy restatement
of the per-spectrum pass (tests/cddf_restatement.py), against the numbers the reference's own
DLACatalogue produced on the committed chunk files (tests/golden/make_consumer_fixtures.py)."""
import glob
import math
import os

import numpy as np
import pytest

import cddf_restatement as R
from gp_dla_detection_amd import _lib, cddf, io, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
CONS = os.path.join(HERE, "golden", "consumer")
NQ, S = 40, 24


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return synthetic.write_file_set(str(tmp_path_factory.mktemp("cddf_in")), num_quasars=NQ, num_samples=S,
                                    empty_quasar=None)


def combined(tmp_path, multi):
    stem = "processed_qsos_multi_meanfluxsynth_" if multi else "processed_qsos_synth_"
    chunks = sorted(glob.glob(os.path.join(CONS, stem + "[0-9]*.mat")))
    out = str(tmp_path / f"combined_{int(multi)}.mat")
    io.combine_processed_chunks(chunks, out)
    return out


def restated_statistics(res, samples, snrs, multi, z_min=2, z_max=5, lnhi_nbins=6):
    """The three methods as make_consumer_fixtures.py called them, from the restatement."""
    p_dla, lld = cddf.posterior_inputs(res["model_posteriors"], res["log_likelihoods_dla"], sub_dla=multi)
    sel = cddf.selected_spectra(p_dla, snrs)
    sll = res["sample_log_likelihoods_dla"]
    sll = sll[:, 0, :] if sll.ndim == 3 else sll
    shift = lld[sel] + np.log(sll.shape[1])
    zlo, zhi = res["min_z_dlas"], res["max_z_dlas"]

    def part(req):
        return R.bin_posteriors(sll[sel], shift, p_dla[sel], zlo[sel], zhi[sel], zhi[sel] - 0.1,
                                samples["offset_samples"], samples["log_nhi_samples"], [req])[0]

    def dX(edges):
        return [cddf.path_length(zlo, zhi, snrs, a, b) for a, b in zip(edges[:-1], edges[1:])]

    rl = cddf.line_density_request(z_min, z_max)
    rc = cddf.column_density_request(float(z_min), float(z_max), lnhi_nbins)
    ro = cddf.omega_dla_request(z_min, z_max)
    return dict(line_density=cddf.line_density_from(part(rl), rl.edges, dX(rl.edges), R.cf_segments),
                column_density_function=cddf.column_density_from(
                    part(rc), rc.edges, cddf.path_length(zlo, zhi, snrs, float(z_min), float(z_max)), R.cf_segments),
                omega_dla=cddf.omega_dla_from(part(ro), ro.edges, dX(ro.edges)))


def assert_reproduces(got, exp):
    n = 0
    for name, parts in got.items():
        for j, x in enumerate(parts):
            e = exp[f"{name}_{j}"]
            x = np.asarray(x, dtype=np.float64)
            assert x.shape == e.shape, (name, j, x.shape, e.shape)
            np.testing.assert_array_equal(np.isnan(x), np.isnan(e), err_msg=f"{name}_{j}")
            np.testing.assert_array_equal(x == 0, e == 0, err_msg=f"{name}_{j} zero bins")
            np.testing.assert_allclose(x, e, rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{name}_{j}")
            n += 1
    assert n == 14
    # bin centres and edges exactly
    np.testing.assert_array_equal(np.asarray(got["line_density"][0]), exp["line_density_0"])
    np.testing.assert_array_equal(np.asarray(got["column_density_function"][0]), exp["column_density_function_0"])
    np.testing.assert_array_equal(np.asarray(got["omega_dla"][0]), exp["omega_dla_0"])
    np.testing.assert_array_equal(np.asarray(got["omega_dla"][3]), exp["omega_dla_3"])


@pytest.mark.parametrize("multi", [False, True])
def test_restatement_reproduces_the_references_statistics(tmp_path, inputs, multi):
    """line_density_0..4, column_density_function_0..4 and omega_dla_0..3 of the reference's
    DLACatalogue; the multi-DLA fixture was made with second=1, which the DLA(1)-only reading
     must reproduce."""
    exp = np.load(os.path.join(CONS, f"expected_dlacatalogue_{'multi' if multi else 'single'}.npz"))
    res = io.load_processed_qsos(combined(tmp_path, multi))
    snrs = inputs["catalog"]["snrs"][inputs["test_ind"]]
    p_dla, _ = cddf.posterior_inputs(res["model_posteriors"], res["log_likelihoods_dla"], sub_dla=multi)
    np.testing.assert_array_equal(cddf.selected_spectra(p_dla, snrs), exp["cached_spectra"])
    got = restated_statistics(res, inputs["samples"], snrs, multi)
    assert any(np.asarray(got["line_density"][1]) > 0)
    assert_reproduces(got, exp)


def test_path_length_against_quad():
    from scipy.integrate import quad
    rng = np.random.default_rng(3)
    zmin = rng.uniform(1.5, 3.5, 60)
    zmax = zmin + rng.uniform(0.0, 2.0, 60)
    snrs = rng.uniform(-5, 5, 60)
    f = lambda z: (1 + z) ** 2 / math.sqrt(0.279 * (1 + z) ** 3 + 0.721)
    for a, b, lowzcut in ((2.0, 2.5, False), (2.2, 4.0, True), (1.0, 6.0, False), (3.1, 3.2, True)):
        hi = np.maximum(np.minimum(zmax, zmax - 0.1), zmin) if lowzcut else zmax
        want = math.fsum(quad(f, max(a, lo), min(b, h))[0] for lo, h, s in zip(zmin, hi, snrs)
                         if s > -2 and lo < b and h > a)
        got = cddf.path_length(zmin, zmax, snrs, a, b, lowzcut=lowzcut)
        assert abs(got - want) <= 1e-12 * abs(want), (a, b, got, want)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 30])
def test_poisson_binomial_pdf_against_convolution(n):
    rng = np.random.default_rng(n)
    p = rng.uniform(0.25, 1.0, n)
    p[0] = np.nextafter(1.0, 2.0)   # a strong absorber's kept sample: p_dla and the normalisation round up
    direct = np.ones(1)
    for v in p:
        direct = np.convolve(direct, [1 - v, v])
    (pdf,) = cddf.poisson_binomial_pdfs([p], R.cf_segments)
    assert pdf.shape == (n + 1,)
    np.testing.assert_allclose(np.asarray(pdf, dtype=np.float64), direct, rtol=0, atol=1e-13)
    (empty,) = cddf.poisson_binomial_pdfs([[]], R.cf_segments)
    np.testing.assert_array_equal(empty, [1.0])


def test_interval_is_the_executed_branch():
    cdf = np.cumsum([0.1, 0.2, 0.4, 0.2, 0.1])
    assert cddf.central_range(cdf, 0.68) == (1, 4)
    assert cddf.central_range(cdf, 0.0) == (2, 3)
    assert cddf.central_range(np.ones(1), 0.95, offset=4) == (4, 4)
    # no entry above 0.975: the upper end is the cdf's length, without the offset (:1264)
    assert cddf.central_range(np.array([0.1, 0.5, 0.97]), 0.95, offset=2) == (2, 3)
    assert cddf.count_levels(np.array([0.1, 0.2, 0.4, 0.2, 0.1]), 3) == (5, (4, 7), (3, 8))


def test_restatement_edge_rules():
    """Strict edges drop a sample on an edge; np.histogram's bins take it (the last one closed)."""
    edges = (2.0, 2.5, 3.0)
    off = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 0.4])       # z = 2.0 2.25 2.5 2.75 3.0 2.4
    w = np.array([0.1, 0.2, 0.1, 0.3, 0.2, 0.1])
    args = (np.log(w)[None, :], [0.0], [1.0], [2.0], [3.0], [2.9], off, np.full(6, 21.0))
    strict = cddf.BinRequest("z", edges, 1.0, 4.0, 20.0, 23.0)
    hist = cddf.BinRequest("z", edges, 1.0, 4.0, 20.0, 23.0, histogram=True)
    (s,) = R.bin_posteriors(*args, [strict])
    np.testing.assert_allclose(s["pois"][0], [0.3, 0.0], rtol=1e-15)
    assert s["count"][0] == 1 and s["kept_bin"][0, 0] == 1
    np.testing.assert_allclose(s["kept_p"][0, 0], 0.3, rtol=1e-15)
    (h,) = R.bin_posteriors(*args, [hist])
    np.testing.assert_allclose(h["mean"][0], [0.4, 0.6], rtol=1e-15)


def test_bad_requests_are_rejected_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_device)
    good = dict(quantity="z", edges=(2.0, 3.0), z_lo=2.0, z_hi=3.0, lnhi_lo=20.0, lnhi_hi=23.0)
    sll = np.zeros((2, 4))
    args = (sll, [0.0, 0.0], [0.5, 0.5], [2.0, 2.0], [3.0, 3.0], [2.9, 2.9], np.linspace(0, 1, 4), np.full(4, 21.0))
    bad = [dict(good, edges=(2.0, 2.0, 3.0)), dict(good, edges=(3.0, 2.0)), dict(good, edges=tuple(np.linspace(2, 3, 66))),
           dict(good, edges=(2.0,)), dict(good, quantity="nhi"), dict(good, edges=(2.0, np.nan)),
           dict(good, p_switch=np.nan)]
    for b in bad:
        with pytest.raises(ValueError):
            cddf.bin_posteriors(*args, [cddf.BinRequest(**b)])
    with pytest.raises(ValueError):
        cddf.bin_posteriors(*args, [cddf.BinRequest(**good)] * 5)
    with pytest.raises(ValueError):
        cddf.bin_posteriors(*args, [])
    with pytest.raises(ValueError):  # S < 1
        cddf.bin_posteriors(np.zeros((2, 0)), *args[1:6], np.zeros(0), np.zeros(0), [cddf.BinRequest(**good)])
    with pytest.raises(ValueError):  # samples do not match the table
        cddf.bin_posteriors(sll, *args[1:6], np.zeros(3), np.zeros(3), [cddf.BinRequest(**good)])
    with pytest.raises(ValueError):
        cddf.DLAStatistics(dict(model_posteriors=np.full((2, 2), 0.5), log_likelihoods_dla=np.zeros(2),
                                sample_log_likelihoods_dla=np.zeros((2, 4)), min_z_dlas=np.full(2, 2.0),
                                max_z_dlas=np.full(2, 3.0)),
                           dict(offset_samples=np.zeros(5), log_nhi_samples=np.zeros(5)), np.ones(2), sub_dla=False)


def test_kept_capacity_is_an_error_not_a_truncation():
    part = dict(count=np.array([2, 9]), kept_bin=np.zeros((2, 8), dtype=np.int32), kept_p=np.zeros((2, 8)),
                pois=np.zeros((2, 1)))
    with pytest.raises(cddf.KeptCapacityError, match="spectrum 1 keeps 9"):
        cddf.split_partials(part, 1)


def test_abi_declares_the_stats_entries():
    h = open(os.path.join(HERE, "..", "include", "gpdla.h")).read()
    for name in ("gpdla_stats_bin_posteriors", "gpdla_stats_poisson_binomial_cf", "gpdla_bin_request",
                 "gpdla_bin_output"):
        assert name in h
    assert "#define GPDLA_ABI_VERSION 6" in h
    assert f"#define GPDLA_STATS_MAX_BINS {cddf.MAX_BINS}" in h
    assert f"#define GPDLA_STATS_KEPT_CAPACITY {cddf.KEPT_CAPACITY}" in h
    names = [s[0] for s in _lib.SYMBOLS]
    assert "gpdla_stats_bin_posteriors" in names and "gpdla_stats_poisson_binomial_cf" in names
