"""CPU-side checks of the sample generator (gp_dla_detection_amd/samples.py): the
boundary it adds to include/gpdla.h, its argument checks (made before the GPU is touched), the
reverse-radix permutation, the samples file it writes, and the restatement the GPU tests use."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sample_restatement as R
from gp_dla_detection_amd import _lib, hdf5, io, samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gpdla_samples_kde", "gpdla_samples_fit_prior", "gpdla_samples_prior_eval", "gpdla_samples_halton",
           "gpdla_samples_draw")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_header_declares_the_entries_and_keeps_the_abi_version(lib):
    text = open(os.path.join(ROOT, "include", "gpdla.h")).read()
    assert re.search(r"^#define GPDLA_ABI_VERSION 6$", text, flags=re.M)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    typed = {n for n, _, _ in _lib.SYMBOLS}
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in typed and hasattr(lib, name)
    assert "} gpdla_nhi_prior;" in code and "} gpdla_sample_draw;" in code
    assert lib.gpdla_abi_version() == 6
    # the ctypes mirrors: ten doubles; six pointers
    assert C.sizeof(_lib.NhiPrior) == 80 and _lib.NhiPrior.Z.offset == 72 and _lib.NhiPrior.centre.offset == 24
    assert C.sizeof(_lib.SampleDraw) == 6 * C.sizeof(C.c_void_p)


def good_prior():
    return _lib.NhiPrior((C.c_double * 3)(0.1, -1.0, -0.13), 21.0, 0.9, 20.0, 23.0, 20.0, math.nan, 0.95)


def test_validation_fails_before_the_gpu_is_touched(lib):
    """Every refusal is GPDLA_ERR_INVALID_ARGUMENT (-1) with a message, with or without a device."""
    v = np.array([20.1, 20.4, 21.0, 20.2])
    x = np.linspace(20.0, 22.0, 5)
    out = np.zeros(5)
    ptr = _lib.ptr

    def refused(rc, text):
        assert rc == -1, (rc, lib.gpdla_last_error())
        assert text in lib.gpdla_last_error().decode(), lib.gpdla_last_error()

    refused(lib.gpdla_samples_kde(1, ptr(v), 5, ptr(x), 0.0, ptr(out), None, 0), "at least 2")
    bad = v.copy()
    bad[2] = np.nan
    refused(lib.gpdla_samples_kde(4, ptr(bad), 5, ptr(x), 0.0, ptr(out), None, 0), "catalogue value 2 is not finite")
    refused(lib.gpdla_samples_kde(4, ptr(v), 5, ptr(x), -0.1, ptr(out), None, 0), "bandwidth")
    refused(lib.gpdla_samples_kde(4, ptr(v), 5, ptr(x), math.inf, ptr(out), None, 0), "bandwidth")
    xb = x.copy()
    xb[4] = np.inf
    refused(lib.gpdla_samples_kde(4, ptr(v), 5, ptr(xb), 0.0, ptr(out), None, 0), "grid point 4")

    pr = _lib.NhiPrior()
    fit = lambda *a: lib.gpdla_samples_fit_prior(4, ptr(v), *a, C.byref(pr), 0)
    refused(fit(20.0, 22.0, 1.5, 20.0, 23.0, 20.0, math.nan, 0.0), "alpha")
    refused(fit(20.0, 22.0, -0.1, 20.0, 23.0, 20.0, math.nan, 0.0), "alpha")
    refused(fit(22.0, 20.0, 0.9, 20.0, 23.0, 20.0, math.nan, 0.0), "fit range")
    refused(fit(20.0, 22.0, 0.9, 23.0, 20.0, 20.0, math.nan, 0.0), "uniform range")
    refused(fit(20.0, 22.0, 0.9, 20.0, 23.0, 25.0, math.nan, 0.0), "lower limit")
    refused(fit(20.0, 22.0, 0.9, 20.0, math.nan, 20.0, math.nan, 0.0), "not finite")
    refused(lib.gpdla_samples_fit_prior(1, ptr(v), 20.0, 22.0, 0.9, 20.0, 23.0, 20.0, math.nan, 0.0, C.byref(pr), 0),
            "at least 2")

    p = good_prior()
    p.alpha = 1.01
    refused(lib.gpdla_samples_prior_eval(C.byref(p), 5, ptr(x), None, ptr(out), 0), "alpha")
    p = good_prior()
    p.Z = 0.0
    refused(lib.gpdla_samples_prior_eval(C.byref(p), 5, ptr(x), None, ptr(out), 0), "Z must be positive")
    refused(lib.gpdla_samples_prior_eval(C.byref(good_prior()), 5, ptr(xb), None, ptr(out), 0), "point 4")

    bases = np.array([2, 3, 5], dtype=np.int32)
    bp = bases.ctypes.data_as(C.POINTER(C.c_int32))
    h = np.zeros((4, 3))
    refused(lib.gpdla_samples_halton(2 ** 32 - 3, 4, 3, bp, ptr(h), 0), "2^32")
    refused(lib.gpdla_samples_halton(-1, 4, 3, bp, ptr(h), 0), "2^32")
    refused(lib.gpdla_samples_halton(0, 4, 9, bp, ptr(h), 0), "9 bases")
    one = np.array([1, 3, 5], dtype=np.int32)
    refused(lib.gpdla_samples_halton(0, 4, 3, one.ctypes.data_as(C.POINTER(C.c_int32)), ptr(h), 0), "base 1")

    cols = [np.zeros(4) for _ in range(6)]
    d3 = _lib.SampleDraw(*[ptr(c) for c in cols[:3]])
    g = good_prior()
    refused(lib.gpdla_samples_draw(C.byref(g), 2 ** 32 - 3, 4, None, 0, 19.5, 20.0, C.byref(d3), 0), "2^32")
    seq = np.full((4, 2), 0.5)
    refused(lib.gpdla_samples_draw(C.byref(g), 0, 4, ptr(seq), 4, 19.5, 20.0, C.byref(d3), 0), "2 or 3 columns")
    seq[3, 1] = 1.5
    refused(lib.gpdla_samples_draw(C.byref(g), 0, 4, ptr(seq), 2, 19.5, 20.0, C.byref(d3), 0), "sequence value 7")
    seq[3, 1] = 0.5
    d6 = _lib.SampleDraw(*[ptr(c) for c in cols])
    refused(lib.gpdla_samples_draw(C.byref(g), 0, 4, ptr(seq), 2, 19.5, 20.0, C.byref(d6), 0), "third column")
    refused(lib.gpdla_samples_draw(C.byref(g), 0, 4, None, 0, 20.0, 19.5, C.byref(d6), 0), "LLS range")
    d4 = _lib.SampleDraw(*[ptr(c) for c in cols[:4]])
    refused(lib.gpdla_samples_draw(C.byref(g), 0, 4, None, 0, 19.5, 20.0, C.byref(d4), 0), "together")
    # the Python layer refuses the same things by raising
    with pytest.raises(_lib.GpdlaError, match="at least 2"):
        samples.kde([20.5], x)
    with pytest.raises(ValueError, match="not finite"):
        samples.kde([20.5, np.nan], x)
    with pytest.raises(_lib.GpdlaError, match="2\\^32"):
        samples.scrambled_halton(2 ** 32, 1)


def test_rr2_permutation_known_answers():
    assert samples.rr2_permutation(2) == (0, 1)
    assert samples.rr2_permutation(3) == (0, 2, 1)
    assert samples.rr2_permutation(5) == (0, 4, 2, 1, 3)
    assert samples.rr2_permutation(7) == (0, 4, 2, 6, 1, 5, 3)
    for b in range(2, 65):   # a permutation that leaves 0 alone, and the restatement's
        p = samples.rr2_permutation(b)
        assert sorted(p) == list(range(b)) and p[0] == 0 and list(p) == R.rr2_permutation(b)
    with pytest.raises(ValueError):
        samples.rr2_permutation(1)


def test_sample_parameters_restate_the_three_scripts():
    s, m = samples.SampleParameters.single(), samples.SampleParameters.multi()
    assert (s.alpha, m.alpha) == (0.9, 0.97)
    for p in (s, m):
        assert (p.uniform_min_log_nhi, p.uniform_max_log_nhi, p.fit_min_log_nhi, p.fit_max_log_nhi) == (20.0, 23.0, 20.0, 22.0)
        assert p.num_dla_samples == 10000
        l = p.lls()
        assert (l.alpha, l.uniform_min_log_nhi, l.uniform_max_log_nhi, l.fit_min_log_nhi, l.fit_max_log_nhi) == (
            0.97, 19.5, 23.0, 20.0, 22.0)
        assert (p.min_lls_log_nhi, p.extrapolate_min_log_nhi, p.lls_break_log_nhi) == (19.5, 19.5, 20.03269)


def fake_samples(S, lls):
    rng = np.random.default_rng(5)
    out = dict(offset_samples=rng.uniform(size=S), log_nhi_samples=20 + 3 * rng.uniform(size=S), alpha=0.97,
               uniform_min_log_nhi=20.0, uniform_max_log_nhi=23.0, fit_min_log_nhi=20.0, fit_max_log_nhi=22.0)
    out["nhi_samples"] = 10.0 ** out["log_nhi_samples"]
    if lls:
        out["lls_log_nhi_samples"] = 19.5 + 0.5 * rng.uniform(size=S)
        out["lls_nhi_samples"] = 10.0 ** out["lls_log_nhi_samples"]
        out.update(Z_lls=0.4821, Z_dla=0.5176)
    return out


@pytest.mark.parametrize("lls", [False, True])
def test_samples_file_round_trip(tmp_path, lls):
    S = 37
    smp = fake_samples(S, lls)
    path = str(tmp_path / "dla_samples.mat")
    io.save_dla_samples(path, smp)
    back = io.load_dla_samples(path)
    vectors = [k for k in smp if k.endswith("_samples")]
    assert sorted(back) == sorted(vectors)   # load_dla_samples returns what it always did
    for k in vectors:
        assert back[k].shape == (S,)
        np.testing.assert_array_equal(back[k], smp[k])
    assert io.load_sample_normalisers(path) == ((0.4821, 0.5176) if lls else None)
    # the layout the reference's consumers index: row vectors, stored [S x 1]; scalars 1 x 1
    with hdf5.File(path) as f:
        for k in vectors:
            assert f[k].read().shape == (S, 1), k
            np.testing.assert_array_equal(f[k].read()[:, 0], smp[k])
            assert f[k].attrs["MATLAB_class"] == "double"
        for k in ("alpha", "uniform_min_log_nhi", "uniform_max_log_nhi", "fit_min_log_nhi", "fit_max_log_nhi"):
            assert f[k].read().shape == (1, 1) and f[k].read()[0, 0] == smp[k]
    m = io.loadmat73(path)
    assert m["offset_samples"].shape == (1, S) and m["alpha"][0, 0] == 0.97
    with pytest.raises(KeyError):
        io.save_dla_samples(path, {k: v for k, v in smp.items() if k != "nhi_samples"})


def test_synthetic_samples_file_has_no_normalisers(tmp_path):
    from gp_dla_detection_amd import synthetic
    path = str(tmp_path / "s.mat")
    io.savemat73(path, {k: v.reshape(1, -1) for k, v in synthetic.make_samples(16).items()})
    assert io.load_sample_normalisers(path) is None
    io.savemat73(path, dict(Z_lls=np.float64(0.4)))   # one of the two is not enough
    assert io.load_sample_normalisers(path) is None


def test_log_nhis_readers(tmp_path):
    v = R.make_catalogue()[:50]
    np.savez(tmp_path / "a.npz", log_nhis=v)
    np.savetxt(tmp_path / "a.txt", v, fmt="%.17g")
    io.savemat73(str(tmp_path / "a.mat"), dict(log_nhis=v.reshape(-1, 1)))
    for name in ("a.npz", "a.txt", "a.mat"):
        np.testing.assert_array_equal(samples.load_log_nhis(str(tmp_path / name)), v)
    io.savemat73(str(tmp_path / "b.mat"), dict(other=v.reshape(-1, 1)))
    with pytest.raises(KeyError, match="containers.Map"):
        samples.load_log_nhis(str(tmp_path / "b.mat"))


def test_restatement_raw_and_centred_fits_agree():
    """The raw-t polyfit of the scripts (Vandermonde condition ~1e6) and the centred one give the same
    quadratic on the grid to 1e-12 (5.9e-14 observed), so the GPU's centred coefficients can be held
    to the raw restatement; and the restatement reproduces the figures its tests lean on."""
    v = R.make_catalogue()
    x = R.fit_grid()
    k = R.ksdensity(v, x)
    raw = R.fit_raw(x, k)
    cen, c = R.fit_centred(x, k)
    assert c == 21.0
    assert np.abs(np.polyval(raw, x) - np.polyval(cen, x - c)).max() <= 1e-12
    assert abs(raw[0] - (-0.132)) < 5e-4   # concave
    p = R.Prior(v)
    assert abs(p.cdf(23.0) - 0.99941) < 1e-5 and abs(p.cdf(25.0) - 1.0) < 1e-14
    u3 = R.halton(0, 10 ** 4, bases=(3,))[:, 0]
    assert np.count_nonzero(u3 > p.cdf(23.0)) == 5
    lp = R.Prior(v, lls=True)
    assert abs(lp.cdf(20.0) - 0.4821) < 1e-4 and abs(lp.cdf(23.0) - lp.cdf(20.0) - 0.5176) < 1e-4


def test_restatement_halton_known_answers():
    h = R.halton(0, 4)
    assert (h[0] == 0).all()
    assert [R.radical_inverse(i, 3) for i in (1, 2, 3)] == [R.Fraction(2, 3), R.Fraction(1, 3), R.Fraction(2, 9)]
    assert R.radical_inverse(1, 5) == R.Fraction(4, 5) and R.radical_inverse(1, 2) == R.Fraction(1, 2)
