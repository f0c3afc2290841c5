"""k_sightline_snr against the NumPy restatement (tests/snr_restatement.py), which tests/test_snrs.py holds
to the reference's own numbers, and the S/N table's round trip into DLAStatistics."""
import numpy as np
import pytest

import snr_restatement as R
from gp_dla_detection_amd import api, cddf, io, snrs
from test_cddf import combined
from test_snrs import fixture_set, inputs  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu


def assert_identical(got, want):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_fixture_sets_equal_the_restatement_and_the_reference(inputs, tag):  # noqa: F811
    spectra, zmax, norm, reference = fixture_set(inputs, tag)
    got = snrs.sightline_snrs(spectra, zmax, norm)
    assert_identical(got, R.sightline_snrs(spectra, zmax, norm))
    assert_identical(got, reference)
    assert_identical(snrs.sightline_snrs(api.spectra_to_csr([dict(s, z_qso=0.0) for s in spectra]), zmax, norm), got)


def ragged_set():
    """Sightlines built for the median's corners; returns (spectra, max_z_dlas, what each one is)."""
    rng = np.random.default_rng(21)
    spectra, zmax, what = [], [], []

    def add(name, n, z, wl=None, **edit):
        wl = np.sort(rng.uniform(3600.0, 10400.0, n)) if wl is None else wl
        s = dict(wavelengths=wl, flux=rng.normal(1.0, 0.8, n), noise_variance=rng.uniform(0.01, 2.0, n))
        for k, (idx, v) in edit.items():
            s[k] = s[k].copy()
            s[k][idx] = v
        spectra.append(s)
        zmax.append(z)
        what.append(name)

    grid = np.linspace(3600.0, 10400.0, 600)
    last = lambda k: (grid[-k - 1] + grid[-k]) / 2 / R.LYA - 1     # the max_z_dla that selects the last k pixels
    add("empty selection", 600, 8.0, grid)
    add("one pixel", 600, last(1), grid)
    add("two pixels", 600, last(2), grid)
    add("even count", 600, last(40), grid)
    add("odd count", 600, last(41), grid)
    add("whole spectrum", 600, 1.0, grid)
    add("NaN max_z_dla", 600, np.nan, grid)
    add("no pixels at all", 0, 2.5)
    add("NaN flux in the selection", 600, 1.0, grid, flux=(599, np.nan))
    add("NaN flux outside the selection", 600, 4.0, grid, flux=(0, np.nan))
    add("negative noise variance", 600, 1.0, grid, noise_variance=(300, -1.0))
    add("infinite noise variance", 600, 1.0, grid, noise_variance=(slice(0, 200), np.inf))
    add("zero flux and zero noise", 40, 1.0, grid[:40], flux=(3, 0.0), noise_variance=(slice(0, 40), 0.0))
    add("ties", 301, 1.0, grid[:301], flux=(slice(0, 301), 0.5), noise_variance=(slice(0, 301), 0.25))
    add("unsorted wavelengths", 500, 3.0, rng.uniform(3600.0, 10400.0, 500))
    add("exactly one tile", 2048, 1.0, np.linspace(3600.0, 10400.0, 2048))
    add("one more than a tile", 2049, 1.0, np.linspace(3600.0, 10400.0, 2049))
    add("three tiles, ties across them", 5000, 1.0, np.linspace(3600.0, 10400.0, 5000),
        flux=(slice(0, 5000, 3), 2.0), noise_variance=(slice(0, 5000, 3), 1.0))
    add("two tiles, even count", 4096, 1.0, np.linspace(3600.0, 10400.0, 4096))
    add("long spectrum, short selection", 4600, 2.0, np.linspace(3600.0, 10400.0, 4600))
    return spectra, np.array(zmax), what


@pytest.mark.parametrize("with_norm", [False, True])
def test_ragged_set(with_norm):
    spectra, zmax, what = ragged_set()
    norm = np.random.default_rng(4).uniform(0.4, 3.0, len(spectra)) if with_norm else None
    want = R.sightline_snrs(spectra, zmax, norm)
    got = snrs.sightline_snrs(spectra, zmax, norm)
    for name, g, w in zip(what, got, want):
        assert (np.isnan(g) and np.isnan(w)) or g == w, (name, g, w)
    by = dict(zip(what, got))
    for name in ("empty selection", "NaN max_z_dla", "no pixels at all", "NaN flux in the selection", "negative noise variance"):
        assert np.isnan(by[name]), name
    for name in ("one pixel", "even count", "whole spectrum", "NaN flux outside the selection", "three tiles, ties across them"):
        assert np.isfinite(by[name]) and by[name] > 0, name
    counts = {n: int(R.selected_pixels(s, z).sum()) for n, s, z in zip(what, spectra, zmax)}
    assert counts["one pixel"] == 1 and counts["two pixels"] == 2 and counts["even count"] == 40
    assert counts["whole spectrum"] == 600 and counts["three tiles, ties across them"] == 5000
    assert counts["odd count"] == 41 and counts["long spectrum, short selection"] < 4600
    assert by["infinite noise variance"] > 0 and by["zero flux and zero noise"] == np.inf
    if not with_norm:
        assert by["ties"] == 1.0


def test_snr_table_round_trip_into_dla_statistics(tmp_path, inputs):  # noqa: F811
    """python -m gp_dla_detection_amd.snrs writes the column DLAStatistics.from_processed_file reads."""
    processed = combined(tmp_path, False)
    out = str(tmp_path / "snrs_out.mat")
    snrs.main([inputs["paths"]["preloaded"], processed, out])
    spectra, zmax, _, reference = fixture_set(inputs, "a")
    stored = np.asarray(io.loadmat73(out, ["snrs"])["snrs"])
    assert stored.shape == (reference.size, 1)                     # the column synthetic.write_file_set writes
    np.testing.assert_array_equal(np.asarray(io.loadmat73(processed, ["max_z_dlas"])["max_z_dlas"]).reshape(-1), zmax)
    assert_identical(stored.reshape(-1), reference)
    cut = float(np.nanmedian(reference))
    st = cddf.DLAStatistics.from_processed_file(processed, inputs["paths"]["samples"], out, sub_dla=False, snr_thresh=cut)
    try:
        assert_identical(st.snrs, reference)
        keep = np.flatnonzero(reference > cut)
        assert 0 < keep.size < reference.size and set(st.selected) <= set(keep)
        res = io.load_processed_qsos(processed)
        want = cddf.path_length(res["min_z_dlas"], res["max_z_dlas"], reference, 2.0, 5.0, snr_thresh=cut)
        assert st.path_length(2.0, 5.0) == want > 0
    finally:
        st.close()
