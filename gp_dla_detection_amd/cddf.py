"""The column density distribution f(N_HI), the line density dN/dX and Omega_DLA of a processed run
(CDDF_analysis/calc_cddf.py, class DLACatalogue), with 68 % / 95 % intervals from its
Poisson-binomial count model.  DESIGN.md section 4.11 states the contract.

The per-spectrum pass over the sample table runs on the GPU (k_bin_posteriors: one read of each
selected spectrum's S log-likelihoods serves up to four bin requests), as does the O(N^2) part of
the Poisson-binomial pdf (k_poisson_binomial_cf).  Everything after that -- the sums across spectra
in quasar order, the pdf's exp and inverse FFT, the combined Poisson levels, the intervals and the
path length -- is host work on small arrays, kept as plain functions of the per-spectrum partials.
There is no CPU fallback for the GPU part.

Only DLA(1) enters: the reference's DLA(k >= 2) branch (:922-943) yields -1e30
for every sample, so it never passes ``p_thresh_sample``.

    python -m gp_dla_detection_amd.cddf PROCESSED SAMPLES [--snrs F] [--z-min 2 --z-max 4 ...] [--json OUT]
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import catalog

MAX_BINS = 64          # GPDLA_STATS_MAX_BINS
MAX_REQUESTS = 4       # GPDLA_STATS_MAX_REQUESTS
KEPT_CAPACITY = 8      # GPDLA_STATS_KEPT_CAPACITY

PROTON_MASS = 1.67262178e-24     # g (:870)
H100 = 3.2407789e-18             # 100 km/s/Mpc in 1/s (:873)
LIGHT = 2.99e10                  # cm/s (:875)
GRAV_CGS = 6.674e-8              # (:1331)


@dataclass(frozen=True)
class BinRequest:
    """One binning of the per-spectrum pass.  ``histogram=False``: the strict rule of
    _split_distributions_single (:1002-1034) -- samples with lnhi_lo < lnhi < lnhi_hi,
    z_lo < z < upper (upper = min(z_max - proximity_zone, z_hi) with ``lowzcut``, else z_hi),
    p > p_thresh_sample, in bin b when edges[b] < q < edges[b+1]; p < p_switch is summed, the rest
    kept one by one.  ``histogram=True``: _get_z_nhi_hist (:1101-1125) -- the same window without
    lowzcut and without a p cut, np.histogram bins, sums of w p and w^2 (1 - p) p with
    w = 10**lnhi (``moment``) or 1."""
    quantity: str            # "z" or "lnhi"
    edges: tuple
    z_lo: float
    z_hi: float
    lnhi_lo: float
    lnhi_hi: float
    histogram: bool = False
    moment: bool = False
    lowzcut: bool = False
    p_thresh_sample: float = 1e-4
    p_switch: float = 0.25


class KeptCapacityError(RuntimeError):
    """A spectrum holds more than KEPT_CAPACITY directly kept samples in one request.  ``spectrum``
    is its row in the block it came in, or -- raised by DLAStatistics -- its quasar index."""

    def __init__(self, spectrum, count, what="spectrum"):
        super().__init__(f"{what} {spectrum} keeps {count} samples directly (capacity {KEPT_CAPACITY})")
        self.spectrum, self.count = spectrum, count


def check_requests(requests) -> None:
    """The rules gpdla_stats_bin_posteriors enforces, checked before any device call."""
    requests = list(requests)
    if not 1 <= len(requests) <= MAX_REQUESTS:
        raise ValueError(f"{len(requests)} bin requests; one pass takes 1 to {MAX_REQUESTS}")
    for r in requests:
        e = np.asarray(r.edges, dtype=np.float64)
        if r.quantity not in ("z", "lnhi"):
            raise ValueError(f"quantity must be 'z' or 'lnhi', not {r.quantity!r}")
        if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
            raise ValueError(f"{e.size - 1} bins; a request takes 1 to {MAX_BINS}")
        if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
            raise ValueError("bin edges must be finite and strictly increasing")
        if any(math.isnan(v) for v in (r.z_lo, r.z_hi, r.lnhi_lo, r.lnhi_hi, r.p_thresh_sample, r.p_switch)):
            raise ValueError("request windows and thresholds must not be NaN")


# ---------------------------------------------------------------------------------------------
# the three requests (:673, :715, :866)
# ---------------------------------------------------------------------------------------------

def z_bins(z_min, z_max, bins_per_z=6):
    """bins_per_z bins per unit redshift, truncated, at least one (:712-713)."""
    count = max(int((z_max - z_min) * bins_per_z), 1)
    return np.linspace(z_min, z_max, count + 1)


def line_density_request(z_min=2, z_max=4, *, bins_per_z=6, lowzcut=False, p_thresh_sample=1e-4, p_switch=0.25):
    return BinRequest("z", tuple(z_bins(z_min, z_max, bins_per_z)), float(z_min), float(z_max), 20.3, 23.,
                      lowzcut=lowzcut, p_thresh_sample=p_thresh_sample, p_switch=p_switch)


def column_density_request(z_min=1., z_max=6., lnhi_nbins=30, lnhi_min=20., lnhi_max=23., *, lowzcut=False,
                           p_thresh_sample=1e-4, p_switch=0.25):
    edges = np.linspace(lnhi_min, lnhi_max, lnhi_nbins + 1)                   # :671
    # the window's upper lnhi is _get_confidence_intervals' default, 23 (:673)
    return BinRequest("lnhi", tuple(edges), float(z_min), float(z_max), float(lnhi_min), 23.,
                      lowzcut=lowzcut, p_thresh_sample=p_thresh_sample, p_switch=p_switch)


def omega_dla_request(z_min=2, z_max=4, lnhi_max=23., lnhi_min=20.3, *, bins_per_z=6):
    return BinRequest("z", tuple(z_bins(z_min, z_max, bins_per_z)), float(z_min), float(z_max), float(lnhi_min),
                      float(lnhi_max), histogram=True, moment=True)


# ---------------------------------------------------------------------------------------------
# per-spectrum inputs (:162-235, :477-511)
# ---------------------------------------------------------------------------------------------

def posterior_inputs(model_posteriors, log_likelihoods_dla, *, sub_dla, occams_razor=10000):
    """(p_dla, log_likelihoods_dla of DLA(1)) per quasar: Occam's razor on the posteriors
    (:175-178), p_dla = model_posteriors[:, 1 + sub_dla:].sum(1)."""
    mp = catalog.occams_model_posteriors(model_posteriors, occams_razor)
    p_dla = mp[:, 1 + int(bool(sub_dla)):].sum(axis=1)
    ll = np.asarray(log_likelihoods_dla, dtype=np.float64)
    return p_dla, (ll[:, 0] if ll.ndim == 2 else ll)


def selected_spectra(p_dla, snrs, p_thresh_spec=5e-2, snr_thresh=-2):
    """filter_dla_spectra (:482-491): p_dla > p_thresh_spec and snr > snr_thresh (the SNRs cut to
    the length of p_dla, :486-489)."""
    snrs = np.asarray(snrs, dtype=np.float64).reshape(-1)[:len(p_dla)]
    return np.flatnonzero((p_dla > p_thresh_spec) & (snrs > snr_thresh))


# ---------------------------------------------------------------------------------------------
# host statistics
# ---------------------------------------------------------------------------------------------

def central_range(cdf, level, offset=0):
    """The count range the reference reports for a cdf (interval, :1247-1266, as it executes: the
    ``if True or`` branch always runs).  Lower end: one past the last index whose cdf is below
    (1 - level) / 2; upper end: one past the first index whose cdf is above (1 + level) / 2, or
    the cdf's length when there is none (without the offset, as :1264 has it).  A one-entry cdf
    gives (offset, offset)."""
    cdf = np.asarray(cdf)
    if cdf.size == 1:
        return offset, offset
    under = np.flatnonzero(cdf < 0.5 - level / 2)
    over = np.flatnonzero(cdf > 0.5 + level / 2)
    lower = offset + (int(under[-1]) + 1 if under.size else 0)
    upper = offset + 1 + int(over[0]) if over.size else cdf.size
    return (lower, upper)


def count_levels(pdf, offset):
    """(most likely count, 68 % range, 95 % range) of a count pdf starting at ``offset``
    (pdf_confidence, :1268-1280); the three must nest."""
    cdf = np.cumsum(pdf)
    mode = central_range(cdf, 0., offset)[0]
    r68 = central_range(cdf, 0.68, offset)
    r95 = central_range(cdf, 0.95, offset)
    if not (r95[0] <= r68[0] <= mode <= r68[1] <= r95[1]):
        raise ArithmeticError("count ranges do not nest (:1278-1279)")
    return mode, r68, r95


def pdf_from_cf(logsum, argsum, nsamp):
    """Poisson-binomial pdf of ``nsamp`` trials from its characteristic function's two sums
    (get_poisson_binomial_pdf, :1295-1305): the coefficients exp(logsum + i argsum) in long double
    (:1317), then an inverse real FFT of length nsamp + 1 in double, as NumPy < 2 computes it."""
    coeffs = np.exp(np.asarray(logsum, dtype=np.float64) + 1j * np.asarray(argsum, dtype=np.float64),
                    dtype=np.clongdouble)
    if not np.any(np.absolute(coeffs) > 0):
        raise ArithmeticError("characteristic function underflowed (:1298)")
    pdf = np.fft.irfft(coeffs.astype(np.complex128), n=nsamp + 1)
    if np.any(np.isinf(pdf)) or abs(math.fsum(pdf) - 1.) >= 1e-7:
        raise ArithmeticError("Poisson-binomial pdf is not normalised (:1302-1304)")
    return pdf


def poisson_binomial_pdfs(segments, cf):
    """One pdf per list of kept probabilities (empty: P(0) = 1, :1285-1286); ``cf(segments)``
    returns each non-empty segment's (logsum, argsum)."""
    segments = [np.asarray(s, dtype=np.float64) for s in segments]
    full = [s for s in segments if s.size]
    sums = iter(cf(full) if full else [])
    out = []
    for s in segments:
        if s.size == 0:
            out.append(np.ones(1))
        else:
            ls, as_ = next(sums)
            out.append(pdf_from_cf(ls, as_, s.size))
    return out


def convolve_poisson(kept_pdf, pmean):
    """The count pdf of the kept samples (``kept_pdf``) plus a Poisson(pmean) count of the small
    ones (_get_combined_levels, :1041-1059), each cut to its central 1 - 1e-4 range: total k gets
    fsum_i Poisson(k - i) kept_pdf[i].  Returns (pdf, count of its first entry); pmean = 0 returns
    ``kept_pdf`` unchanged."""
    if pmean == 0.:
        return (kept_pdf, 0)
    from scipy.stats import poisson
    lo_p, hi_p = (int(v) for v in poisson.interval(1 - 1e-4, pmean))
    lo_b, hi_b = central_range(np.cumsum(kept_pdf), 1 - 1e-4)
    kept = np.arange(lo_b, min(hi_b + 1, np.size(kept_pdf)))
    totals = np.arange(lo_p + lo_b, hi_p + hi_b + 1)
    terms = poisson.pmf(totals[:, None] - kept[None, :], pmean) * np.asarray(kept_pdf)[kept][None, :]
    out = np.array([math.fsum(row) for row in terms])
    if not 0.99 < math.fsum(out) < 1.00:
        raise ArithmeticError("combined pdf is not normalised (:1058)")
    return (out, lo_p + lo_b)


def split_partials(partials, nbins):
    """Per bin, the kept probabilities (spectrum order, then sample order) and the fsum of the
    per-spectrum Poisson sums, from the partials of one strict request in quasar order: what
    _split_distributions_single collects (:1035)."""
    count = np.asarray(partials["count"])
    if np.any(count > KEPT_CAPACITY):
        s = int(np.flatnonzero(count > KEPT_CAPACITY)[0])
        raise KeptCapacityError(s, int(count[s]))
    kept = [[] for _ in range(nbins)]
    kb, kp = np.asarray(partials["kept_bin"]), np.asarray(partials["kept_p"])
    for s in np.flatnonzero(count):
        for i in range(int(count[s])):
            kept[int(kb[s, i])].append(float(kp[s, i]))
    pois = np.asarray(partials["pois"])
    return kept, np.array([math.fsum(pois[:, b]) for b in range(nbins)])


def count_ranges(partials, nbins, cf):
    """Per bin, the most likely number of absorbers and its 68 % / 95 % ranges
    (_get_confidence_intervals, :1061-1088)."""
    kept, pmeans = split_partials(partials, nbins)
    levels = [count_levels(*convolve_poisson(pdf, pmean))
              for pdf, pmean in zip(poisson_binomial_pdfs(kept, cf), pmeans)]
    return [m for m, _, _ in levels], [r for _, r, _ in levels], [r for _, _, r in levels]


def dX_dz(z, omega_m=0.279):
    """Absorption distance per unit redshift, (1 + z)^2 / sqrt(Omega_m (1 + z)^3 + 1 - Omega_m)
    (:1239-1245, :1319-1324)."""
    return (1 + z) ** 2 / math.sqrt(omega_m * (1 + z) ** 3 + (1 - omega_m))


def path_length(min_z_dlas, max_z_dlas, snrs, z_min, z_max, *, snr_thresh=-2, lowzcut=False, proximity_zone=0.1):
    """Absorption path searched between z_min and z_max (path_length, :552-603, without noisy-pixel
    filtering): the spectra over the SNR cut, each over the part of its search range inside the
    interval (with ``lowzcut`` the range ends proximity_zone below max_z_dla, but not below
    min_z_dla).  Spectra that cover the whole interval share one integral; the others are
    integrated one by one and added in quasar order."""
    from scipy.integrate import quad
    if not z_min < z_max:
        raise ValueError("path_length needs z_min < z_max")
    n = len(min_z_dlas)
    over = (np.asarray(snrs, dtype=np.float64).reshape(-1) > snr_thresh)[:n]
    lo = np.asarray(min_z_dlas, dtype=np.float64)[over]
    hi = np.asarray(max_z_dlas, dtype=np.float64)[over]
    if lowzcut:
        hi = np.maximum(np.minimum(hi, hi - proximity_zone), lo)
    if np.any(hi - lo < 0):
        raise ValueError("a search range ends below its start")
    inside = (lo < z_max) & (hi > z_min)
    lo, hi = lo[inside], hi[inside]
    covers = (hi > z_max) & (lo < z_min)
    whole, _ = quad(dX_dz, z_min, z_max)
    total = np.count_nonzero(covers) * whole
    for a, b in zip(lo[~covers], hi[~covers]):
        part, err = quad(dX_dz, max(z_min, a), min(z_max, b))
        if not err < 1e-6:
            raise ArithmeticError(f"path length integral error {err}")
        total += part
    return total


def critical_density(hubble=0.7):
    """rho_crit = 3 H0^2 / (8 pi G) in g cm^-3 (:1326-1333)."""
    h0 = H100 * hubble
    return 3 * h0 ** 2 / (8 * math.pi * GRAV_CGS)


def _centres(edges):
    return (edges[1:] + edges[:-1]) / 2.


def line_density_from(partials, z_bins_, dX, cf):
    """line_density's tuple (:715-725) -- bin centres, dN/dX, its 68 % and 95 % ranges, the
    half-widths -- over the bins with a non-zero path, from the partials of line_density_request
    and the path length of each bin."""
    edges = np.asarray(z_bins_, dtype=np.float64)
    counts, r68, r95 = count_ranges(partials, edges.size - 1, cf)
    dX = np.asarray(dX, dtype=np.float64)
    live = dX > 0
    path = dX[live]
    centres = _centres(edges)
    return (centres[live], np.asarray(counts)[live] / path, np.asarray(r68)[live] / path[:, None],
            np.asarray(r95)[live] / path[:, None],
            (centres[live] - edges[:-1][live], edges[1:][live] - centres[live]))


def column_density_from(partials, l_nhi, dX, cf):
    """column_density_function's tuple (:673-682) -- log10 N_HI bin centres, f(N_HI) =
    count / dX / dN, its 68 % and 95 % ranges, the bins' half-widths in N_HI -- from the partials
    of column_density_request and the path length of its redshift range."""
    edges = np.asarray(l_nhi, dtype=np.float64)
    counts, r68, r95 = count_ranges(partials, edges.size - 1, cf)
    width = np.power(10., edges[1:]) - np.power(10., edges[:-1])
    centres = _centres(edges)
    return (centres, np.asarray(counts) / dX / width, np.asarray(r68) / dX / width[:, None],
            np.asarray(r95) / dX / width[:, None],
            (np.power(10., centres) - np.power(10., edges[:-1]), np.power(10., edges[1:]) - np.power(10., centres)))


def omega_dla_from(partials, z_bins_, dX, hubble=0.7):
    """omega_dla's tuple (:866-880) -- bin centres, Omega_DLA, its error, the edges -- from the
    partials of omega_dla_request: the N_HI moments summed over spectra in quasar order, the
    variance plus the mean (:1130), and Omega_DLA = m_p H0 / (c rho_crit) * sum N_HI / dX.  As at
    :876, rho_crit is taken at h = 0.7 whatever ``hubble`` is."""
    edges = np.asarray(z_bins_)
    nb = edges.size - 1
    m, v = np.asarray(partials["mean"]), np.asarray(partials["var"])
    nhi = np.array([math.fsum(m[:, b]) for b in range(nb)])
    spread = np.array([math.fsum(v[:, b]) for b in range(nb)]) + nhi
    grams_per_atom = PROTON_MASS * (H100 * hubble) / LIGHT
    with np.errstate(divide="ignore", invalid="ignore"):
        per_column = grams_per_atom / np.asarray(dX, dtype=np.float64) / critical_density()
        return (_centres(edges), nhi * per_column, np.sqrt(spread) * per_column, edges)


# ---------------------------------------------------------------------------------------------
# the GPU passes
# ---------------------------------------------------------------------------------------------

def bin_posteriors(sll, shift, p_dla, z_min, z_max, upper_z, offset_samples, log_nhi_samples, requests,
                   device=0):
    """k_bin_posteriors on one block of selected spectra (rows of ``sll``, [n, S]).  Returns, per
    request, dict(pois, mean, var [n, B], count [n], kept_bin, kept_p [n, KEPT_CAPACITY])."""
    from . import _lib
    requests = list(requests)
    check_requests(requests)
    sll = np.asarray(sll, dtype=np.float64)
    if sll.ndim != 2 or sll.shape[1] < 1 or sll.strides[1] != 8:
        raise ValueError("sample log-likelihoods must be [n, S] with S >= 1 and unit sample stride")
    n, S = sll.shape
    vec = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (shift, p_dla, z_min, z_max, upper_z)]
    if any(a.size != n for a in vec):
        raise ValueError("shift, p_dla, z_min, z_max and upper_z need one entry per spectrum")
    off = np.ascontiguousarray(offset_samples, dtype=np.float64).reshape(-1)
    lnhi = np.ascontiguousarray(log_nhi_samples, dtype=np.float64).reshape(-1)
    if off.size != S or lnhi.size != S:
        raise ValueError(f"{S} sample columns but {off.size} offsets and {lnhi.size} log N_HI samples")
    lib = _lib.load()
    reqs = (_lib.BinRequest * len(requests))()
    outs = (_lib.BinOutput * len(requests))()
    keep, res = [], []
    for i, r in enumerate(requests):
        e = np.ascontiguousarray(r.edges, dtype=np.float64)
        nb = e.size - 1
        o = dict(pois=np.zeros((n, nb)), mean=np.zeros((n, nb)), var=np.zeros((n, nb)),
                 count=np.zeros(n, dtype=np.int32), kept_bin=np.zeros((n, KEPT_CAPACITY), dtype=np.int32),
                 kept_p=np.zeros((n, KEPT_CAPACITY)))
        keep.append(e)
        res.append(o)
        reqs[i] = _lib.BinRequest(1 if r.quantity == "lnhi" else 0, nb, _lib.ptr(e), r.z_lo, r.z_hi, r.lnhi_lo,
                                  r.lnhi_hi, int(r.histogram), int(r.moment), int(r.lowzcut), r.p_thresh_sample,
                                  r.p_switch)
        outs[i] = _lib.BinOutput(_lib.ptr(o["pois"]), _lib.ptr(o["mean"]), _lib.ptr(o["var"]),
                                 o["count"].ctypes.data_as(_lib._i32p), o["kept_bin"].ctypes.data_as(_lib._i32p),
                                 _lib.ptr(o["kept_p"]))
    rc = lib.gpdla_stats_bin_posteriors(n, S, sll.ctypes.data_as(_lib._dp), sll.strides[0] // 8,
                                        *[_lib.ptr(a) for a in vec], _lib.ptr(off), _lib.ptr(lnhi),
                                        len(requests), reqs, outs, int(device))
    if rc == _lib.ERR_UNSUPPORTED:  # the outputs are written; a count above the capacity names the spectrum
        for o in res:
            over = np.flatnonzero(o["count"] > KEPT_CAPACITY)
            if over.size:
                raise KeptCapacityError(int(over[0]), int(o["count"][over[0]]))
    _lib.check(rc)
    return res


def poisson_binomial_cf(segments, device=0):
    """k_poisson_binomial_cf: for each segment of N probabilities, (logsum, argsum) over
    n = 0 .. (N+1)//2 (get_poisson_binomial_pdf's characteristic function, :1293-1295).  The
    probabilities must be finite and >= 0; a kept sample of a strong absorber may exceed 1 by a
    few ulps (p_dla and the normalisation each round), which the reference accepts too."""
    from . import _lib
    segments = [np.asarray(s, dtype=np.float64).reshape(-1) for s in segments]
    if not segments:
        return []
    offsets = np.zeros(len(segments) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([s.size for s in segments])
    p = np.ascontiguousarray(np.concatenate(segments)) if offsets[-1] else np.zeros(1)
    m = np.array([(s.size + 1) // 2 + 1 for s in segments], dtype=np.int64)
    out_off = np.concatenate([[0], np.cumsum(m)])
    logsum, argsum = np.zeros(int(out_off[-1])), np.zeros(int(out_off[-1]))
    lib = _lib.load()
    _lib.check(lib.gpdla_stats_poisson_binomial_cf(len(segments), offsets.ctypes.data_as(_lib._i64p), _lib.ptr(p),
                                                   _lib.ptr(logsum), _lib.ptr(argsum), int(device)))
    return [(logsum[a:b], argsum[a:b]) for a, b in zip(out_off[:-1], out_off[1:])]


# ---------------------------------------------------------------------------------------------
# the user-facing object
# ---------------------------------------------------------------------------------------------

class DLAStatistics:
    """DLACatalogue's statistics (calc_cddf.py:43-160) of one processed run.

    ``results``: the dict process_qsos, process_qsos_multiple_dlas_meanflux or
    io.load_processed_qsos returns; ``samples``: the sample dict (offset_samples,
    log_nhi_samples); ``snrs``: one per searched quasar.  The sample table is read by the GPU pass
    in blocks of ``block_size`` selected spectra; results do not depend on the block size."""

    def __init__(self, results, samples, snrs, *, sub_dla, occams_razor=10000, snr_thresh=-2, lowzcut=False,
                 p_thresh_spec=5e-2, p_thresh_sample=1e-4, p_switch=0.25, proximity_zone=0.1, bins_per_z=6,
                 block_size=2048, device=0):
        p_dla, lld = posterior_inputs(results["model_posteriors"], results["log_likelihoods_dla"],
                                      sub_dla=sub_dla, occams_razor=occams_razor)
        sll = np.asarray(results["sample_log_likelihoods_dla"])
        first = sll[:, 0, :] if sll.ndim == 3 else sll                       # DLA(1) (:217-220)
        self._init(p_dla, lld, np.asarray(results["min_z_dlas"], dtype=np.float64),
                   np.asarray(results["max_z_dlas"], dtype=np.float64), samples, snrs, first.shape[1],
                   occams_razor=occams_razor, snr_thresh=snr_thresh, lowzcut=lowzcut, p_thresh_spec=p_thresh_spec,
                   p_thresh_sample=p_thresh_sample, p_switch=p_switch, proximity_zone=proximity_zone,
                   bins_per_z=bins_per_z, block_size=block_size, device=device)
        self._rows = lambda sel: first[sel]

    def _init(self, p_dla, lld, z_min, z_max, samples, snrs, num_samples, *, occams_razor, snr_thresh, lowzcut,
              p_thresh_spec, p_thresh_sample, p_switch, proximity_zone, bins_per_z, block_size, device):
        if block_size < 1:
            raise ValueError("block_size must be >= 1")
        self.occams_razor, self.snr_thresh, self.lowzcut = occams_razor, snr_thresh, lowzcut
        self.p_thresh_spec, self.p_thresh_sample, self.p_switch = p_thresh_spec, p_thresh_sample, p_switch
        self.proximity_zone, self.bins_per_z = proximity_zone, bins_per_z
        self.block_size, self.device = int(block_size), device
        self.p_dla, self.z_min, self.z_max = p_dla, z_min, z_max
        self.snrs = np.asarray(snrs, dtype=np.float64).reshape(-1)
        self.offset_samples = np.asarray(samples["offset_samples"], dtype=np.float64).reshape(-1)
        self.log_nhi_samples = np.asarray(samples["log_nhi_samples"], dtype=np.float64).reshape(-1)
        if self.offset_samples.size != num_samples:
            raise ValueError(f"the sample table has {num_samples} columns, the samples {self.offset_samples.size}")
        self.selected = selected_spectra(p_dla, self.snrs, p_thresh_spec, snr_thresh)
        sel = self.selected
        self._shift = lld[sel] + np.log(num_samples)                         # :228
        self._upper_z = z_max[sel] - proximity_zone                          # proximity() (:965-968)
        self._cache = {}

    @classmethod
    def from_processed_file(cls, processed, samples_file, snrs, *, sub_dla, **kw):
        """The same statistics from a processed_qsos file, its sample table streamed in quasar
        blocks (hdf5.Dataset.read_slab).  Each read spans at most ``block_size`` quasars, so the host
        holds at most 2 x block_size rows of S samples: the block of selected rows being built and
        one read.  ``samples_file`` / ``snrs``: a path or the arrays (dict / vector)."""
        from . import hdf5, io
        small = io.loadmat73(processed, ["model_posteriors", "log_likelihoods_dla", "min_z_dlas", "max_z_dlas"])
        mp = np.asarray(small["model_posteriors"], dtype=np.float64)
        lld = np.asarray(small["log_likelihoods_dla"], dtype=np.float64)
        lld = lld.reshape(-1) if (lld.ndim == 2 and 1 in lld.shape) else lld
        samples = io.load_dla_samples(samples_file) if isinstance(samples_file, str) else samples_file
        if isinstance(snrs, str):
            snrs = np.asarray(io.loadmat73(snrs, ["snrs"])["snrs"]).reshape(-1)
        p_dla, lld1 = posterior_inputs(mp, lld, sub_dla=sub_dla, occams_razor=kw.get("occams_razor", 10000))
        self = cls.__new__(cls)
        f = hdf5.File(processed)
        ds = f["sample_log_likelihoods_dla"]                                  # HDF5: [S, nq] or [md, S, nq]
        S = ds.shape[-2]
        opts = {k: kw.pop(k) for k in list(kw) if k not in ("block_size", "device")}
        self._init(p_dla, lld1, np.asarray(small["min_z_dlas"], dtype=np.float64).reshape(-1),
                   np.asarray(small["max_z_dlas"], dtype=np.float64).reshape(-1), samples, snrs, S,
                   **{**dict(occams_razor=10000, snr_thresh=-2, lowzcut=False, p_thresh_spec=5e-2,
                             p_thresh_sample=1e-4, p_switch=0.25, proximity_zone=0.1, bins_per_z=6), **opts,
                      **dict(block_size=kw.get("block_size", 2048), device=kw.get("device", 0))})

        span = self.block_size

        def rows(sel):
            sel = np.asarray(sel)
            out = np.empty((sel.size, S))
            i = 0
            while i < sel.size:  # one read per run of selected quasars within `span` of its first
                lo = int(sel[i])
                j = int(np.searchsorted(sel, lo + span))
                hi = int(sel[j - 1]) + 1
                slab = (ds.read_slab(0, S, axis1=(lo, hi)) if len(ds.shape) == 2
                        else ds.read_slab(0, 1, axis1=(0, S), axis2=(lo, hi))[0])  # [S, hi - lo]
                out[i:j] = slab[:, sel[i:j] - lo].T
                i = j
            return out
        self._rows = rows
        self._file = f
        return self

    def close(self):
        f = getattr(self, "_file", None)
        if f is not None:
            f.close()
            self._file = None

    # -- the pass ------------------------------------------------------------------------------
    def partials(self, requests):
        """Per-spectrum partials of up to four requests, from one read of the selected spectra's
        rows; memoised per request."""
        requests = list(requests)
        check_requests(requests)
        todo = [r for r in dict.fromkeys(requests) if r not in self._cache]
        if todo:
            sel = self.selected
            parts = [[] for _ in todo]
            for a in range(0, sel.size, self.block_size):
                b = sel[a:a + self.block_size]
                i = slice(a, a + b.size)
                try:
                    res = bin_posteriors(self._rows(b), self._shift[i], self.p_dla[b], self.z_min[b],
                                         self.z_max[b], self._upper_z[i], self.offset_samples,
                                         self.log_nhi_samples, todo, device=self.device)
                except KeptCapacityError as e:
                    raise KeptCapacityError(int(b[e.spectrum]), e.count, "quasar") from None
                for k, r in enumerate(res):
                    parts[k].append(r)
            for r, ps in zip(todo, parts):
                nb = len(r.edges) - 1
                self._cache[r] = {k: (np.concatenate([p[k] for p in ps]) if ps else
                                      (np.zeros((0, nb)) if k in ("pois", "mean", "var") else
                                       np.zeros((0,) + ((KEPT_CAPACITY,) if k.startswith("kept") else ()))))
                                  for k in ("pois", "mean", "var", "count", "kept_bin", "kept_p")}
        return [self._cache[r] for r in requests]

    def _cf(self, segments):
        return poisson_binomial_cf(segments, device=self.device)

    # -- the reference's methods --------------------------------------------------------------
    def path_length(self, z_min, z_max):
        return path_length(self.z_min, self.z_max, self.snrs, z_min, z_max, snr_thresh=self.snr_thresh,
                           lowzcut=self.lowzcut, proximity_zone=self.proximity_zone)

    def _line_request(self, z_min, z_max):
        return line_density_request(z_min, z_max, bins_per_z=self.bins_per_z, lowzcut=self.lowzcut,
                                    p_thresh_sample=self.p_thresh_sample, p_switch=self.p_switch)

    def _cddf_request(self, z_min, z_max, lnhi_nbins, lnhi_min, lnhi_max):
        return column_density_request(z_min, z_max, lnhi_nbins, lnhi_min, lnhi_max, lowzcut=self.lowzcut,
                                      p_thresh_sample=self.p_thresh_sample, p_switch=self.p_switch)

    def column_density_function(self, z_min=1., z_max=6., lnhi_nbins=30, lnhi_min=20., lnhi_max=23.):
        req = self._cddf_request(z_min, z_max, lnhi_nbins, lnhi_min, lnhi_max)
        (part,) = self.partials([req])
        return column_density_from(part, req.edges, self.path_length(z_min, z_max), self._cf)

    def line_density(self, z_min=2, z_max=4):
        req = self._line_request(z_min, z_max)
        (part,) = self.partials([req])
        zb = np.asarray(req.edges)
        dX = np.array([self.path_length(z_m, z_x) for (z_m, z_x) in zip(zb[:-1], zb[1:])])
        return line_density_from(part, zb, dX, self._cf)

    def omega_dla(self, z_min=2, z_max=4, hubble=0.7, lnhi_max=23., lnhi_min=20.3):
        req = omega_dla_request(z_min, z_max, lnhi_max, lnhi_min, bins_per_z=self.bins_per_z)
        (part,) = self.partials([req])
        zb = np.asarray(req.edges)
        dX = np.array([self.path_length(z_m, z_x) for (z_m, z_x) in zip(zb[:-1], zb[1:])])
        return omega_dla_from(part, zb, dX, hubble)

    def statistics(self, z_min=2, z_max=4, lnhi_nbins=30, hubble=0.7):
        """The three statistics over one redshift range from ONE pass over the sample table:
        {"line_density": ..., "column_density_function": ..., "omega_dla": ...}."""
        self.partials([self._line_request(z_min, z_max),
                       self._cddf_request(z_min, z_max, lnhi_nbins, 20., 23.),
                       omega_dla_request(z_min, z_max, bins_per_z=self.bins_per_z)])
        return dict(line_density=self.line_density(z_min, z_max),
                    column_density_function=self.column_density_function(z_min, z_max, lnhi_nbins),
                    omega_dla=self.omega_dla(z_min, z_max, hubble))


def _jsonable(x):
    if isinstance(x, (tuple, list)):
        return [_jsonable(v) for v in x]
    a = np.asarray(x, dtype=np.float64)
    return [None if not np.isfinite(v) else float(v) for v in a.reshape(-1)] if a.ndim == 1 else \
        [_jsonable(r) for r in a] if a.ndim > 1 else (float(a) if np.isfinite(a) else None)


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="python -m gp_dla_detection_amd.cddf",
                                 description="f(N_HI), dN/dX and Omega_DLA of a processed run, as JSON")
    ap.add_argument("processed")
    ap.add_argument("samples")
    ap.add_argument("--snrs", help="snrs file (one entry per searched quasar); default: no SNR cut")
    ap.add_argument("--sub-dla", action="store_true", help="the posteriors hold a sub-DLA model (multi-DLA runs)")
    ap.add_argument("--z-min", type=float, default=2.)
    ap.add_argument("--z-max", type=float, default=4.)
    ap.add_argument("--lnhi-nbins", type=int, default=30)
    ap.add_argument("--lowzcut", action="store_true")
    ap.add_argument("--snr-thresh", type=float, default=-2)
    ap.add_argument("--occams-razor", type=float, default=10000)
    ap.add_argument("--block-size", type=int, default=2048)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", help="output file (default: stdout)")
    a = ap.parse_args(argv)
    from . import io
    snrs = a.snrs
    if snrs is None:
        nq = np.asarray(io.loadmat73(a.processed, ["min_z_dlas"])["min_z_dlas"]).size
        snrs = np.full(nq, np.inf)
    st = DLAStatistics.from_processed_file(a.processed, a.samples, snrs, sub_dla=a.sub_dla,
                                           occams_razor=a.occams_razor, snr_thresh=a.snr_thresh,
                                           lowzcut=a.lowzcut, block_size=a.block_size, device=a.device)
    try:
        out = {k: _jsonable(v) for k, v in st.statistics(a.z_min, a.z_max, a.lnhi_nbins).items()}
    finally:
        st.close()
    text = json.dumps(out)
    if a.json:
        with open(a.json, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
