"""read_spec.m and preload_qsos.m restated in NumPy, line by line, independently of
csrc/preload_kernels.hpp.  It is the yardstick k_preload is held to (tests/test_gpu_preload.py);
tests/test_preload.py holds it to one spectrum worked out by hand.

Every step is one correctly rounded IEEE double operation on the float32 columns widened exactly
(``fitsread`` without ``'raw'`` returns doubles), except ``10 .^ loglam``, which is libm's pow here.
"""
import numpy as np

DEFAULTS = dict(loading_min_lambda=910.0, loading_max_lambda=1217.0, normalization_min_lambda=1310.0,
                normalization_max_lambda=1325.0, min_lambda=911.75, max_lambda=1215.75, min_num_pixels=200)

BRIGHTSKY = 24   # read_spec.m:9; bitget counts from 1, so this is bit 23 counted from 0


def read_spec(flux, loglam, ivar, and_mask):
    """read_spec.m:11-38 on the four columns of HDU 1."""
    flux = np.asarray(flux, dtype=np.float32).astype(np.float64)                 # :16
    log_wavelengths = np.asarray(loglam, dtype=np.float32).astype(np.float64)    # :19
    inverse_noise_variance = np.asarray(ivar, dtype=np.float32).astype(np.float64)   # :22
    and_mask = np.asarray(and_mask, dtype=np.int32)                              # :25
    wavelengths = 10.0 ** log_wavelengths                                        # :28
    with np.errstate(divide="ignore"):
        noise_variance = 1.0 / inverse_noise_variance                            # :31
    bit = (and_mask.view(np.uint32) >> np.uint32(BRIGHTSKY - 1)) & np.uint32(1)  # :38 bitget(and_mask, 24)
    pixel_mask = (inverse_noise_variance == 0) | (bit != 0)                      # :36-38
    return wavelengths, flux, noise_variance, pixel_mask


def nanmedian(v):
    """MATLAB's nanmedian of a vector: NaNs dropped, NaN for an empty rest, the mean of the middle two
    for an even count (see DESIGN.md 4.16 on median's a + (b - a) / 2 form)."""
    v = np.asarray(v, dtype=np.float64)
    v = np.sort(v[~np.isnan(v)], kind="stable")
    if v.size == 0:
        return np.nan
    a, b = v[(v.size - 1) // 2], v[v.size // 2]
    if v.size % 2:
        return a
    with np.errstate(invalid="ignore"):
        return (a + b) / 2.0


def preload_one(flux, loglam, ivar, and_mask, z_qso, filter_flag=0, **params):
    """preload_qsos.m:18-71 for one quasar: (wavelengths, flux, noise_variance, pixel_mask, normalizer,
    filter_flag).  The four arrays are empty where the .m file `continue`s."""
    p = dict(DEFAULTS, **params)
    empty = (np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.uint8))
    filter_flag = int(filter_flag)
    if filter_flag > 0:                                                          # :19-21
        return empty + (0.0, filter_flag)
    wl, fl, nv, mask = read_spec(flux, loglam, ivar, and_mask)                   # :23-24
    rest = wl / (1.0 + z_qso)                                                    # :26
    ind = (rest >= p["normalization_min_lambda"]) & (rest <= p["normalization_max_lambda"]) & ~mask   # :29-31
    this_median = nanmedian(fl[ind])                                             # :33
    if np.isnan(this_median):                                                    # :36-39
        return empty + (0.0, filter_flag | 4)
    ind = (rest >= p["min_lambda"]) & (rest <= p["max_lambda"]) & ~mask          # :41-43
    if np.count_nonzero(ind) < p["min_num_pixels"]:                              # :46-49
        return empty + (0.0, filter_flag | 8)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fl = fl / this_median                                                    # :53
        nv = nv / (this_median * this_median)                                    # :54
    ind = (rest >= p["loading_min_lambda"]) & (rest <= p["loading_max_lambda"])  # :56-57
    available = np.flatnonzero(~ind & ~mask)                                     # :60
    sel = np.flatnonzero(ind)
    if sel.size:   # (an empty find() makes both comparisons empty: nothing is added)
        above = available[available > sel[-1]]                                   # :61
        below = available[available < sel[0]]                                    # :62
        ind = ind.copy()
        if above.size:
            ind[above.min()] = True
        if below.size:
            ind[below.max()] = True
    return wl[ind], fl[ind], nv[ind], mask[ind].astype(np.uint8), float(this_median), filter_flag   # :64-67, :51


def preload(raw, z_qsos, filter_flags, **params):
    """A raw CSR set (offsets, flux, loglam, ivar, and_mask) -> the dict gpdla's preload returns."""
    off = np.asarray(raw["offsets"], dtype=np.int64)
    n = off.size - 1
    parts = [preload_one(*(raw[k][off[i]:off[i + 1]] for k in ("flux", "loglam", "ivar", "and_mask")),
                         float(z_qsos[i]), int(filter_flags[i]), **params) for i in range(n)]
    counts = np.array([q[0].size for q in parts], dtype=np.int64)
    cat = lambda j, dt: (np.concatenate([q[j] for q in parts]).astype(dt) if n else np.zeros(0, dtype=dt))
    return dict(offsets=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
                wavelengths=cat(0, np.float64), flux=cat(1, np.float64), noise_variance=cat(2, np.float64),
                pixel_mask=cat(3, np.uint8), all_normalizers=np.array([q[4] for q in parts], dtype=np.float64),
                filter_flags=np.array([q[5] for q in parts], dtype=np.uint8),
                z_qsos=np.asarray(z_qsos, dtype=np.float64).reshape(-1).copy())


def rest_wavelengths(raw, z_qsos):
    """lambda_rest of every pixel of a raw CSR set (for the tests' distance-from-threshold condition)."""
    off = np.asarray(raw["offsets"], dtype=np.int64)
    z = np.repeat(np.asarray(z_qsos, dtype=np.float64), np.diff(off))
    return 10.0 ** np.asarray(raw["loglam"], dtype=np.float32).astype(np.float64) / (1.0 + z)
