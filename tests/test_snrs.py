"""The sightline S/N's NumPy restatement (tests/snr_restatement.py) against the numbers the reference's own
compute_all_snrs produced on the synthetic file set (tests/golden/make_snr_fixtures.py), and the host
checks of gp_dla_detection_amd/snrs.py.  The GPU side is tests/test_gpu_snrs.py."""
import os

import numpy as np
import pytest

import snr_restatement as R
from gp_dla_detection_amd import _lib, snrs, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
SNRS = os.path.join(HERE, "golden", "snrs")
NQ, S = 40, 24


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return synthetic.write_file_set(str(tmp_path_factory.mktemp("snr_in")), num_quasars=NQ, num_samples=S,
                                    empty_quasar=None)


def fixture_set(inputs, tag):
    """(searched spectra, max_z_dlas, normalizers or None, the reference's snrs) of fixture set ``tag``."""
    fx = np.load(os.path.join(SNRS, f"set_{tag}.npz"))
    np.testing.assert_array_equal(fx["test_ind"], inputs["test_ind"])
    real = np.flatnonzero(fx["test_ind"])
    spectra = [inputs["spectra"][i] for i in real]
    if tag == "c":
        spectra = R.set_c_spectra(spectra)
    norm = fx["normalizers"][real] if tag == "b" else None
    return spectra, fx["max_z_dlas"], norm, fx["snrs"]


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_equals_the_reference_value_for_value(inputs, tag):
    """Every step is one correctly rounded IEEE operation (compare, divide, multiply, sqrt, abs, a
    sort, one add and a halving), so the restatement equals what the reference computed under
    NumPy 1.26 bit for bit.  Seen here: equal on all three sets, NaN positions included."""
    spectra, zmax, norm, want = fixture_set(inputs, tag)
    got = R.sightline_snrs(spectra, zmax, norm)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got, want)


def test_the_fixture_sets_cover_what_they_should(inputs):
    _, zmax, _, a = fixture_set(inputs, "a")
    assert np.isfinite(a).sum() >= 8 and np.isnan(a).sum() >= 8
    spectra_b, _, norm, b = fixture_set(inputs, "b")
    assert np.all(norm != 1) and np.isfinite(b).sum() >= 8
    assert np.any(b[np.isfinite(b)] != a[np.isfinite(a)])                 # the other floor branch was taken
    spectra_c, _, _, c = fixture_set(inputs, "c")
    assert np.isfinite(c).sum() * 4 >= 3 * c.size
    counts = [int(R.selected_pixels(s, z).sum()) for s, z in zip(spectra_c, zmax)]
    assert min(counts) >= 1 and any(n % 2 == 0 for n in counts) and any(n % 2 == 1 for n in counts)
    assert any(np.any(np.asarray(s["flux"])[R.selected_pixels(s, z)] < R.FLOOR) for s, z in zip(spectra_c, zmax))


def test_median_rules():
    assert np.isnan(R.median_as_numpy([]))
    assert np.isnan(R.median_as_numpy([1.0, np.nan, 0.5]))
    assert R.median_as_numpy([3.0]) == 3.0
    assert R.median_as_numpy([4.0, 1.0, 3.0, 2.0]) == 2.5
    assert R.median_as_numpy([np.inf, 1.0, 2.0]) == 2.0
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 18, 301):
        v = rng.uniform(0, 3, n)
        assert R.median_as_numpy(v) == np.median(v)
    one = dict(wavelengths=np.array([4000.0, 5000.0]), flux=np.array([1.0, 0.01]), noise_variance=np.array([4.0, 0.25]))
    assert np.isnan(R.sightline_snr(**one, max_z_dla=np.nan))
    assert np.isnan(R.sightline_snr(**one, max_z_dla=9.0))                # nothing redward
    assert R.sightline_snr(**one, max_z_dla=2.5) == 1 / (0.5 / 0.1)       # one pixel, floored
    assert R.sightline_snr(**one, max_z_dla=2.5, normalizer=0.05) == 1 / (0.5 / 0.01)   # 0.01 / 0.05 >= 0.1 stays
    assert R.sightline_snr(**one, max_z_dla=2.0) == 1 / ((2.0 / 1.0 + 0.5 / 0.1) / 2.0)


def test_bad_inputs_are_rejected_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_device)
    sp = [dict(wavelengths=np.arange(5.0), flux=np.ones(5), noise_variance=np.ones(5))]
    with pytest.raises(ValueError):
        snrs.sightline_snrs(sp, [2.0, 3.0])
    with pytest.raises(ValueError):
        snrs.sightline_snrs(sp, [2.0], normalizers=[1.0, 2.0])
    with pytest.raises(ValueError):
        snrs.sightline_snrs(dict(offsets=[0, 5], wavelengths=np.arange(5.0), flux=np.ones(4), noise_variance=np.ones(5)), [2.0])
    with pytest.raises(ValueError):
        snrs.sightline_snrs(dict(offsets=[0, 5, 3], wavelengths=np.arange(5.0), flux=np.ones(5), noise_variance=np.ones(5)),
                            [2.0, 2.0])
    assert snrs.sightline_snrs([], []).size == 0


def test_abi_declares_the_entry():
    h = open(os.path.join(HERE, "..", "include", "gpdla.h")).read()
    assert "gpdla_stats_sightline_snrs" in h and "#define GPDLA_ABI_VERSION 6" in h
    assert "gpdla_stats_sightline_snrs" in [s[0] for s in _lib.SYMBOLS]
