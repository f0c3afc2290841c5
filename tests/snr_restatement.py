"""The sightline S/N (gp_dla_detection_amd/snrs.py, k_sightline_snr) restated in NumPy, one correctly
rounded IEEE operation per step, and the two edits of the synthetic file set behind the fixtures of
tests/golden/snrs/ (tests/golden/make_snr_fixtures.py applies them to the files the reference reads,
the tests to the arrays in memory).  DESIGN.md section 4.14 states the definition."""
import numpy as np

LYA = 1215.67
FLOOR = 0.1


def median_as_numpy(values):
    """NaN for no values or any NaN; else the middle value of the sorted ones, or the mean of the
    middle two."""
    v = np.asarray(values, dtype=np.float64)
    if v.size == 0 or np.isnan(v).any():
        return np.nan
    v = np.sort(v)
    mid = v.size // 2
    return v[mid] if v.size % 2 else (v[mid - 1] + v[mid]) / 2.0


def sightline_snr(wavelengths, flux, noise_variance, max_z_dla, normalizer=None):
    wl = np.asarray(wavelengths, dtype=np.float64)
    red = wl > LYA * (1 + max_z_dla)                    # a NaN max_z_dla selects nothing
    f = np.array(flux, dtype=np.float64)[red]
    nv = np.asarray(noise_variance, dtype=np.float64)[red]
    with np.errstate(all="ignore"):
        if normalizer is None:
            f[f < FLOOR] = FLOOR                        # a NaN flux fails the test and stays NaN
        else:
            f[f / normalizer < FLOOR] = normalizer * FLOOR
        return 1 / np.float64(median_as_numpy(np.sqrt(nv) / np.abs(f)))


def sightline_snrs(spectra, max_z_dlas, normalizers=None):
    return np.array([sightline_snr(s["wavelengths"], s["flux"], s["noise_variance"], z,
                                   None if normalizers is None else normalizers[i])
                     for i, (s, z) in enumerate(zip(spectra, max_z_dlas))])


def selected_pixels(spectrum, max_z_dla):
    return np.asarray(spectrum["wavelengths"]) > LYA * (1 + max_z_dla)


def set_b_normalizers(num_quasars):
    """The ``all_normalizers`` of fixture set (b): one per raw quasar, none equal to 1."""
    return 0.56 + 0.15 * (np.arange(num_quasars) % 7)


def set_c_fill(num_pixels):
    """What fixture set (c) puts in place of masked pixels: (flux, noise variance); the fluxes are
    below the floor, every other one negative."""
    flux = np.where(np.arange(num_pixels) % 2 == 0, 0.03, -0.4)
    return flux, np.full(num_pixels, 0.01)


def set_c_spectra(spectra):
    """Fixture set (c): copies of the spectra with every masked pixel given a finite flux below the
    floor and a finite noise variance, so that no selection holds a NaN."""
    out = []
    for s in spectra:
        masked = np.asarray(s["pixel_mask"]) != 0
        fill_f, fill_v = set_c_fill(masked.size)
        t = dict(s)
        t["flux"] = np.where(masked, fill_f, np.asarray(s["flux"], dtype=np.float64))
        t["noise_variance"] = np.where(masked, fill_v, np.asarray(s["noise_variance"], dtype=np.float64))
        out.append(t)
    return out
