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
                                        [--sample-errors R [--seed N]] [--refined FILE]

``--snrs`` takes the table ``python -m gp_dla_detection_amd.snrs`` writes.  ``--sample-errors`` adds the
stratified bootstrap over sightlines (DLAStatistics.sample_errors): sample-variance
percentiles of dN/dX, Omega_DLA and f(N_HI), the sightline draws and their sums on the GPU
(k_path_lengths, k_bootstrap_sums).  ``--refined`` takes the file ``python -m gp_dla_detection_amd.refine ...
--tables --posteriors`` writes: the quasars it refined enter with their refined P(DLA) and are binned from their
own refined sample tables (k_bin_posteriors_boxed).
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
    reqs, outs, keep, res = _bin_structs(requests, n)
    rc = lib.gpdla_stats_bin_posteriors(n, S, sll.ctypes.data_as(_lib._dp), sll.strides[0] // 8,
                                        *[_lib.ptr(a) for a in vec], _lib.ptr(off), _lib.ptr(lnhi),
                                        len(requests), reqs, outs, int(device))
    _check_kept(rc, res)
    return res


def _bin_structs(requests, n):
    """The gpdla_bin_request / gpdla_bin_output arrays of a per-spectrum pass over ``n`` rows, the edge
    arrays they point into, and the result dicts the outputs point into."""
    from . import _lib
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
    return reqs, outs, keep, res


def _check_kept(rc, res):
    from . import _lib
    if rc == _lib.ERR_UNSUPPORTED:  # the outputs are written; a count above the capacity names the spectrum
        for o in res:
            over = np.flatnonzero(o["count"] > KEPT_CAPACITY)
            if over.size:
                raise KeptCapacityError(int(over[0]), int(o["count"][over[0]]))
    _lib.check(rc)


def bin_posteriors_boxed(lam, p_dla, boxes, upper_z, u, v, requests, device=0):
    """k_bin_posteriors_boxed on one block of refined rows: ``lam`` [n, S'] the
    ``sample_log_posteriors_refined`` of each row, ``boxes`` [n, 4] its (z_lo, z_hi, n_lo, n_hi) of the
    last level, ``u`` / ``v`` the shared unit points.  The row's samples are z = z_lo + (z_hi - z_lo) u,
    log N = n_lo + (n_hi - n_lo) v, p = exp(lam - shift) p_dla with shift = log Sum exp(lam) formed on the
    GPU (NaN for a row without a finite entry).  Returns (what :func:`bin_posteriors` returns, shift [n])."""
    from . import _lib
    requests = list(requests)
    check_requests(requests)
    lam = np.asarray(lam, dtype=np.float64)
    if lam.ndim != 2 or lam.shape[1] < 1 or lam.strides[1] != 8:
        raise ValueError("refined sample log-posteriors must be [n, S'] with S' >= 1 and unit sample stride")
    n, S = lam.shape
    if lam.strides[0] < 8 * S:   # (reversed or overlapping rows: the library takes a forward stride of at least S')
        lam = np.ascontiguousarray(lam)
    vec = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (p_dla, upper_z)]
    if any(a.size != n for a in vec):
        raise ValueError("p_dla and upper_z need one entry per row")
    boxes = np.ascontiguousarray(boxes, dtype=np.float64)
    if boxes.shape != (n, 4):
        raise ValueError(f"boxes must be [n, 4] = {(n, 4)}, got {boxes.shape}")
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    if u.size != S or v.size != S:
        raise ValueError(f"{S} sample columns but {u.size} u and {v.size} v")
    reqs, outs, keep, res = _bin_structs(requests, n)
    shift = np.full(n, np.nan)
    rc = _lib.load().gpdla_stats_bin_posteriors_boxed(n, S, lam.ctypes.data_as(_lib._dp), lam.strides[0] // 8, _lib.ptr(vec[0]),
                                                      _lib.ptr(boxes), _lib.ptr(vec[1]), _lib.ptr(u), _lib.ptr(v),
                                                      len(requests), reqs, outs, _lib.ptr(shift), int(device))
    _check_kept(rc, res)
    return res, shift


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
# path length per sightline and bin, and the stratified bootstrap
# ---------------------------------------------------------------------------------------------

BOOTSTRAP_MAX_COLUMNS = 256   # GPDLA_BOOTSTRAP_MAX_COLUMNS
PATH_PANEL = 0.25             # widest quadrature panel in z (kPathPanel)
#: the positive nodes of the 8-point Gauss-Legendre rule and their weights (kGaussX, kGaussW)
GAUSS_NODES = (0.1834346424956498, 0.525532409916329, 0.7966664774136267, 0.9602898564975363)
GAUSS_WEIGHTS = (0.362683783378362, 0.31370664587788727, 0.22238103445337448, 0.10122853629037626)


def gauss_legendre_path(z_lo, z_hi, omega_m=0.279):
    """The integral of dX_dz over [z_lo, z_hi] by the rule k_path_lengths uses, on the host: 8
    nodes on each of ceil((z_hi - z_lo) / 0.25) equal panels."""
    width = z_hi - z_lo
    panels = max(int(math.ceil(width / PATH_PANEL)), 1)
    half = width / (2.0 * panels)
    terms = []
    for p in range(panels):
        mid = z_lo + (2.0 * p + 1.0) * half
        for x, w in zip(GAUSS_NODES, GAUSS_WEIGHTS):
            terms.append(w * (dX_dz(mid - half * x, omega_m) + dX_dz(mid + half * x, omega_m)))
    return half * math.fsum(terms)


def _check_edges(edges):
    e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
    if not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError(f"{e.size - 1} bins; a request takes 1 to {MAX_BINS}")
    if not np.all(np.isfinite(e)) or not np.all(np.diff(e) > 0):
        raise ValueError("bin edges must be finite and strictly increasing")
    if not e[0] > -1 or e[-1] - e[0] > 1000:
        raise ValueError("bin edges must lie above z = -1 and span at most 1000")
    return e


def path_length_matrix(min_z_dlas, max_z_dlas, snrs, edges, *, snr_thresh=-2, lowzcut=False, proximity_zone=0.1,
                       omega_m=0.279, device=0):
    """(rows, dX): for the sightlines over the SNR cut (``rows``: their indices), the absorption
    path of each inside each bin [edges[b], edges[b + 1]] -- the terms path_length adds up, by
    k_path_lengths.  A sightline that does not reach into a bin has exactly 0 there."""
    from . import _lib
    e = _check_edges(edges)
    if not (math.isfinite(proximity_zone) and 0 < omega_m <= 1):
        raise ValueError("need a finite proximity zone and 0 < omega_m <= 1")
    n = len(min_z_dlas)
    rows = np.flatnonzero((np.asarray(snrs, dtype=np.float64).reshape(-1) > snr_thresh)[:n])
    lo = np.ascontiguousarray(np.asarray(min_z_dlas, dtype=np.float64).reshape(-1)[rows])
    hi = np.ascontiguousarray(np.asarray(max_z_dlas, dtype=np.float64).reshape(-1)[rows])
    end = np.maximum(np.minimum(hi, hi - proximity_zone), lo) if lowzcut else hi
    if np.any(end - lo < 0):
        raise ValueError("a search range ends below its start")
    dX = np.zeros((rows.size, e.size - 1))
    if rows.size:
        _lib.check(_lib.load().gpdla_stats_path_lengths(rows.size, _lib.ptr(lo), _lib.ptr(hi), e.size - 1, _lib.ptr(e),
                                                        int(bool(lowzcut)), float(proximity_zone), float(omega_m),
                                                        _lib.ptr(dX), int(device)))
    return rows, dX


def bootstrap_strata(max_z_dlas, min_count=10, num_strata=9):
    """A stratum label per sightline (dense, from 0, rising with max_z_dla) for the bootstrap.
    As the reference's resample (:299-310): ``num_strata`` equal-width strata in max_z_dla between
    two ends that are pulled in from the extremes in steps of 0.2 until the sightlines beyond each
    end number at least ``min_count``; the end strata are extended to cover everything.  Unlike
    the reference, a stratum still under ``min_count`` is merged into its lower neighbour (the
    lowest into the one above), and every loop is bounded: all-equal redshifts, fewer than
    2 x min_count sightlines or ends that cross give one stratum."""
    z = np.asarray(max_z_dlas, dtype=np.float64).reshape(-1)
    if np.any(np.isnan(z)):
        raise ValueError("max_z_dlas must not be NaN")
    if min_count < 1 or num_strata < 1:
        raise ValueError("min_count and num_strata must be >= 1")
    label = np.zeros(z.size, dtype=np.int32)
    if z.size < 2 * min_count or num_strata == 1:
        return label
    z_lo, z_hi = float(z.min()), float(z.max())
    if not (math.isfinite(z_lo) and math.isfinite(z_hi)) or z_lo == z_hi:
        return label
    steps = int(math.ceil((z_hi - z_lo) / 0.2)) + 1
    top = next((z_hi - 0.2 * k for k in range(1, steps + 1) if np.count_nonzero(z > z_hi - 0.2 * k) >= min_count), z_lo)
    bottom = next((z_lo + 0.2 * k for k in range(1, steps + 1) if np.count_nonzero(z <= z_lo + 0.2 * k) >= min_count), z_hi)
    if not bottom < top:
        return label
    inner = np.linspace(bottom, top, num_strata + 1)[1:-1]         # the end strata reach to -inf / +inf
    raw = np.searchsorted(inner, z, side="left")                    # inner[s-1] < z <= inner[s]
    counts = np.bincount(raw, minlength=num_strata)
    group = np.arange(num_strata)
    for b in range(num_strata - 1, 0, -1):                          # small strata join the one below
        if counts[b] < min_count:
            counts[b - 1] += counts[b]
            counts[b] = 0
            group[group == b] = b - 1
    if counts[0] < min_count:                                       # the lowest joins the next one that is left
        up = np.flatnonzero(counts[1:] > 0)
        if up.size:
            group[group == 0] = 1 + int(up[0])
    _, dense = np.unique(group, return_inverse=True)
    return dense[raw].astype(np.int32)


def _check_seed(seed):
    """The bootstrap's seed as an int in [0, 2^64); NaN, fractions and other types are ValueErrors."""
    if isinstance(seed, (float, np.floating)):
        if not (math.isfinite(seed) and float(seed).is_integer()):
            raise ValueError(f"seed must be an integer, not {seed!r}")
        seed = int(seed)
    try:
        seed = int(np.asarray(seed).astype(object).item()) if not isinstance(seed, int) else seed
    except (TypeError, ValueError):
        raise ValueError(f"seed must be an integer, not {seed!r}") from None
    if isinstance(seed, bool) or not 0 <= seed < 2 ** 64:
        raise ValueError("seed must lie in [0, 2^64)")
    return seed


def bootstrap_sums(V, stratum, replicates, seed, *, first_replicate=0, path_columns=None, device=0):
    """k_bootstrap_sums: for replicates first_replicate .. first_replicate + replicates - 1, the
    column sums of ``V`` [N, C] over the rows each replicate draws.  ``stratum``: one label per row,
    non-decreasing (rows sorted by stratum); position j of a stratum of m rows starting at row f
    draws row f + ((w * m) >> 32), w the first word of Philox4x32-10 at counter (lo32(j), hi32(j),
    r, 2) keyed by the seed.  ``path_columns``: columns that must be finite (the dX ones).
    Returns [replicates, C]; a replicate's sums do not depend on how a run is split into calls."""
    from . import _lib
    V = np.ascontiguousarray(V, dtype=np.float64)
    if V.ndim != 2 or V.shape[0] < 1 or not 1 <= V.shape[1] <= BOOTSTRAP_MAX_COLUMNS:
        raise ValueError(f"V must be [N >= 1, 1 .. {BOOTSTRAP_MAX_COLUMNS}]")
    lab = np.asarray(stratum)
    if lab.shape != (V.shape[0],) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError("stratum needs one integer label per row of V")
    if lab.min() < 0 or np.any(np.diff(lab) < 0):
        raise ValueError("rows must be sorted by stratum, labels >= 0")
    seed = _check_seed(seed)
    if isinstance(replicates, (float, np.floating)) and not float(replicates).is_integer():
        raise ValueError("replicates must be an integer")
    replicates, first_replicate = int(replicates), int(first_replicate)
    if replicates < 1:
        raise ValueError("replicates must be >= 1")
    if first_replicate < 0 or first_replicate + replicates > 2 ** 32:
        raise ValueError("replicate indices must lie in [0, 2^32)")
    if path_columns is not None and not np.all(np.isfinite(V[:, path_columns])):
        raise ValueError("the path-length columns of V must be finite")
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    out = np.zeros((replicates, V.shape[1]))
    _lib.check(_lib.load().gpdla_stats_bootstrap_sums(V.shape[0], V.shape[1], _lib.ptr(V), lab.ctypes.data_as(_lib._i32p),
                                                      seed, first_replicate, replicates, _lib.ptr(out), int(device)))
    return out


def expected_counts(partials, nbins):
    """[n, nbins]: each spectrum's expected number of absorbers per bin from the partials of a
    strict request -- its Poisson sum plus its directly kept probabilities, scattered to their bins."""
    out = np.array(partials["pois"], dtype=np.float64).reshape(-1, nbins)
    count = np.asarray(partials["count"])
    if np.any(count > KEPT_CAPACITY):
        s = int(np.flatnonzero(count > KEPT_CAPACITY)[0])
        raise KeptCapacityError(s, int(count[s]))
    kb, kp = np.asarray(partials["kept_bin"]), np.asarray(partials["kept_p"])
    for s in np.flatnonzero(count):
        for i in range(int(count[s])):
            out[s, int(kb[s, i])] += kp[s, i]
    return out


def sample_percentiles(replicates):
    """(median, [84th, 16th], [97.5th, 2.5th]) over the finite replicates of each column, shaped
    like the reference's dndx_sample / dndx_68_sample / dndx_95_sample (:338-344).  A column with no
    finite replicate gives NaN."""
    r = np.asarray(replicates, dtype=np.float64)
    r = np.where(np.isfinite(r), r, np.nan)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        q = np.nanpercentile(r, [50., 84., 16., 97.5, 2.5], axis=0)
    return q[0], q[1:3], q[3:5]


# ---------------------------------------------------------------------------------------------
# the user-facing object
# ---------------------------------------------------------------------------------------------

class DLAStatistics:
    """DLACatalogue's statistics (calc_cddf.py:43-160) of one processed run.

    ``results``: the dict process_qsos, process_qsos_multiple_dlas_meanflux or
    io.load_processed_qsos returns; ``samples``: the sample dict (offset_samples,
    log_nhi_samples); ``snrs``: one per searched quasar.  The sample table is read by the GPU pass
    in blocks of ``block_size`` selected spectra; results do not depend on the block size.

    ``refined`` (single-DLA runs): the dict of ``refine.refine_absorbers(with_samples=True,
    posteriors=True)`` or of ``io.load_refined_results``.  The quasars of its ``selection`` with status 0 enter
    with the refined P(DLA) (Occam's razor applied to the refined pair), also into the choice of the selected
    spectra, and their partials come from their own refined tables (:func:`bin_posteriors_boxed`: S' points in
    each quasar's last box, S' need not equal S); every other quasar goes through :func:`bin_posteriors` as
    without ``refined``.  The sightline's own ``min_z_dlas`` / ``max_z_dlas`` stay the path-length limits and the
    source of the proximity cut."""

    def __init__(self, results, samples, snrs, *, sub_dla, occams_razor=10000, snr_thresh=-2, lowzcut=False,
                 p_thresh_spec=5e-2, p_thresh_sample=1e-4, p_switch=0.25, proximity_zone=0.1, bins_per_z=6,
                 block_size=2048, device=0, refined=None):
        p_dla, lld = posterior_inputs(results["model_posteriors"], results["log_likelihoods_dla"],
                                      sub_dla=sub_dla, occams_razor=occams_razor)
        sll = np.asarray(results["sample_log_likelihoods_dla"])
        first = sll[:, 0, :] if sll.ndim == 3 else sll                       # DLA(1) (:217-220)
        self._init(p_dla, lld, np.asarray(results["min_z_dlas"], dtype=np.float64),
                   np.asarray(results["max_z_dlas"], dtype=np.float64), samples, snrs, first.shape[1],
                   occams_razor=occams_razor, snr_thresh=snr_thresh, lowzcut=lowzcut, p_thresh_spec=p_thresh_spec,
                   p_thresh_sample=p_thresh_sample, p_switch=p_switch, proximity_zone=proximity_zone,
                   bins_per_z=bins_per_z, block_size=block_size, device=device, refined=refined,
                   single_dla=sll.ndim == 2 and not sub_dla)
        self._rows = lambda sel: first[sel]

    def _init(self, p_dla, lld, z_min, z_max, samples, snrs, num_samples, *, occams_razor, snr_thresh, lowzcut,
              p_thresh_spec, p_thresh_sample, p_switch, proximity_zone, bins_per_z, block_size, device, refined=None,
              single_dla=True):
        if block_size < 1:
            raise ValueError("block_size must be >= 1")
        self._refined = None
        if refined is not None:
            if not single_dla:
                raise ValueError("refined results belong to a single-DLA run (no multi-DLA tables, no sub_dla)")
            p_dla = self._take_refined(refined, p_dla, occams_razor)
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

    def _take_refined(self, refined, p_dla, occams_razor):
        """Checks ``refined`` and keeps what the boxed pass reads: per refined quasar (status 0) its row of
        the refined arrays.  Returns ``p_dla`` with the refined P(DLA) of those quasars."""
        if isinstance(refined, str):
            from . import io
            refined = io.load_refined_results(refined)
        need = ("selection", "status", "boxes", "sample_log_posteriors_refined", "refine_u", "refine_v")
        if any(k not in refined for k in need):
            raise ValueError("the refined results hold no sample table: " + ", ".join(k for k in need if k not in refined)
                             + " missing (refine_absorbers(with_samples=True), or refine's --tables)")
        if "model_posteriors_refined" not in refined:
            raise ValueError("the refined results hold no model_posteriors_refined "
                             "(refine_absorbers(posteriors=True), or refine's --posteriors)")
        sel = np.asarray(refined["selection"], dtype=np.int64).reshape(-1)
        lam = np.asarray(refined["sample_log_posteriors_refined"], dtype=np.float64)
        u = np.asarray(refined["refine_u"], dtype=np.float64).reshape(-1)
        v = np.asarray(refined["refine_v"], dtype=np.float64).reshape(-1)
        boxes = np.asarray(refined["boxes"], dtype=np.float64)
        if lam.ndim != 2 or lam.shape != (sel.size, u.size) or v.size != u.size or boxes.shape[::2] != (sel.size, 4):
            raise ValueError("the refined tables do not fit their selection and unit points")
        if sel.size and (sel.min() < 0 or sel.max() >= p_dla.size or np.unique(sel).size != sel.size):
            raise ValueError("the refined selection must name quasars of the run, each once")
        rows = np.flatnonzero(np.asarray(refined["status"]).reshape(-1) == 0)
        mp = catalog.occams_model_posteriors(np.asarray(refined["model_posteriors_refined"], dtype=np.float64)[rows], occams_razor)
        p_dla = np.array(p_dla, dtype=np.float64)
        p_dla[sel[rows]] = mp[:, 1]
        row_of = np.full(p_dla.size, -1, dtype=np.int64)
        row_of[sel[rows]] = rows
        self._refined = dict(row_of=row_of, lam=lam, boxes=boxes[:, -1, :], u=u, v=v)
        return p_dla

    @classmethod
    def from_processed_file(cls, processed, samples_file, snrs, *, sub_dla, **kw):
        """The same statistics from a processed_qsos file, its sample table streamed in quasar
        blocks (hdf5.Dataset.read_slab).  Each read spans at most ``block_size`` quasars, so the host
        holds at most 2 x block_size rows of S samples: the block of selected rows being built and
        one read.  ``samples_file`` / ``snrs``: a path or the arrays (dict / vector).  ``refined``: the file
        ``refine --tables --posteriors`` wrote, or the dict (see the class)."""
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
        refined = kw.pop("refined", None)
        opts = {k: kw.pop(k) for k in list(kw) if k not in ("block_size", "device")}
        self._init(p_dla, lld1, np.asarray(small["min_z_dlas"], dtype=np.float64).reshape(-1),
                   np.asarray(small["max_z_dlas"], dtype=np.float64).reshape(-1), samples, snrs, S,
                   **{**dict(occams_razor=10000, snr_thresh=-2, lowzcut=False, p_thresh_spec=5e-2,
                             p_thresh_sample=1e-4, p_switch=0.25, proximity_zone=0.1, bins_per_z=6), **opts,
                      **dict(block_size=kw.get("block_size", 2048), device=kw.get("device", 0), refined=refined,
                             single_dla=lld.ndim == 1 and not sub_dla)})

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
            # the spectra with a refined table are binned from it, the others from the first pass's; both in
            # blocks of block_size, and `at` remembers where each block's rows belong in quasar order
            ref = self._refined
            boxed = ref["row_of"][sel] >= 0 if ref is not None else np.zeros(sel.size, dtype=bool)
            at = []
            for group in (np.flatnonzero(~boxed), np.flatnonzero(boxed)):
                for a in range(0, group.size, self.block_size):
                    i = group[a:a + self.block_size]
                    b = sel[i]
                    try:
                        if boxed[i[0]]:
                            rows = ref["row_of"][b]
                            res, _ = bin_posteriors_boxed(ref["lam"][rows], self.p_dla[b], ref["boxes"][rows], self._upper_z[i],
                                                          ref["u"], ref["v"], todo, device=self.device)
                        else:
                            res = bin_posteriors(self._rows(b), self._shift[i], self.p_dla[b], self.z_min[b],
                                                 self.z_max[b], self._upper_z[i], self.offset_samples,
                                                 self.log_nhi_samples, todo, device=self.device)
                    except KeptCapacityError as e:
                        raise KeptCapacityError(int(b[e.spectrum]), e.count, "quasar") from None
                    at.append(i)
                    for k, part in enumerate(res):
                        parts[k].append(part)
            order = np.argsort(np.concatenate(at), kind="stable") if at else None   # the identity without `refined`
            for r, ps in zip(todo, parts):
                nb = len(r.edges) - 1
                self._cache[r] = {k: (np.concatenate([p[k] for p in ps])[order] if ps else
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


    def sample_errors(self, z_min=2, z_max=4, replicates=1000, seed=0x9E3779B97F4A7C15, hubble=0.7, lnhi_nbins=30,
                      min_count=10, num_strata=9, replicates_per_call=None):
        """Sample-variance errors of dN/dX, Omega_DLA and f(N_HI) from a stratified bootstrap over
        the sightlines above the SNR cut: sightlines are resampled with
        replacement inside strata of max_z_dla (bootstrap_strata), every stratum keeping its size.
        Replicate statistics: sum of expected counts / sum dX per z bin; omega_dla_from's conversion
        of sum of N_HI moments / sum dX; sum of expected counts / sum dX / dN per column-density
        bin.  z bins without path in the data are dropped, as line_density drops them; a replicate
        that draws no path into a bin is left out of that bin's percentiles.

        Returns a dict: ``z_centres``, ``lnhi_centres``; for name in dndx / omega / cddf:
        ``<name>_sample`` (median), ``<name>_68_sample`` ([84th, 16th] percentiles, shape [2, bins]),
        ``<name>_95_sample`` ([97.5th, 2.5th]), ``<name>_replicates`` ([replicates, bins]) and
        ``<name>_point`` (the same statistic of the data itself); ``strata`` (sizes); ``seed``."""
        seed = _check_seed(seed)
        if int(replicates) != replicates or replicates < 1:
            raise ValueError("replicates must be an integer >= 1")
        replicates = int(replicates)
        line, col = self._line_request(z_min, z_max), self._cddf_request(z_min, z_max, lnhi_nbins, 20., 23.)
        om = omega_dla_request(z_min, z_max, bins_per_z=self.bins_per_z)
        p_line, p_col, p_om = self.partials([line, col, om])
        zb, nb_edges = np.asarray(line.edges), np.asarray(col.edges)
        nz, nn = zb.size - 1, nb_edges.size - 1
        rows, dX = path_length_matrix(self.z_min, self.z_max, self.snrs, zb, snr_thresh=self.snr_thresh,
                                      lowzcut=self.lowzcut, proximity_zone=self.proximity_zone, device=self.device)
        _, dX_all = path_length_matrix(self.z_min, self.z_max, self.snrs, [float(z_min), float(z_max)],
                                       snr_thresh=self.snr_thresh, lowzcut=self.lowzcut,
                                       proximity_zone=self.proximity_zone, device=self.device)
        if rows.size == 0:
            raise ValueError("no sightline is above the SNR cut")
        V = np.zeros((rows.size, 3 * nz + nn + 1))
        at = np.searchsorted(rows, self.selected)               # selected spectra are all over the cut
        V[at, :nz] = expected_counts(p_line, nz)
        V[at, nz:nz + nn] = expected_counts(p_col, nn)
        V[at, nz + nn:2 * nz + nn] = np.asarray(p_om["mean"]).reshape(-1, nz)
        V[:, 2 * nz + nn:3 * nz + nn] = dX
        V[:, -1] = dX_all[:, 0]
        path_cols = slice(2 * nz + nn, 3 * nz + nn + 1)
        label = bootstrap_strata(self.z_max[rows], min_count, num_strata)
        order = np.argsort(label, kind="stable")
        Vs, ls = np.ascontiguousarray(V[order]), label[order]
        step = replicates if replicates_per_call is None else max(int(replicates_per_call), 1)
        sums = np.concatenate([bootstrap_sums(Vs, ls, min(step, replicates - r0), seed, first_replicate=r0,
                                              path_columns=path_cols, device=self.device)
                               for r0 in range(0, replicates, step)])
        point = np.array([math.fsum(V[:, c]) for c in range(V.shape[1])])[None, :]
        live = point[0, 2 * nz + nn:3 * nz + nn] > 0
        width = np.power(10., nb_edges[1:]) - np.power(10., nb_edges[:-1])
        per_atom = PROTON_MASS * (H100 * hubble) / LIGHT / critical_density()

        def ratios(t):
            with np.errstate(divide="ignore", invalid="ignore"):
                path = t[:, 2 * nz + nn:3 * nz + nn][:, live]
                return dict(dndx=t[:, :nz][:, live] / path, omega=per_atom * t[:, nz + nn:2 * nz + nn][:, live] / path,
                            cddf=t[:, nz:nz + nn] / t[:, -1:] / width[None, :])

        rep, pt = ratios(sums), ratios(point)
        out = dict(z_centres=_centres(zb)[live], lnhi_centres=_centres(nb_edges), seed=seed, replicates=replicates,
                   strata=np.bincount(label))
        for name in ("dndx", "omega", "cddf"):
            med, r68, r95 = sample_percentiles(rep[name])
            out.update({f"{name}_sample": med, f"{name}_68_sample": r68, f"{name}_95_sample": r95,
                        f"{name}_replicates": rep[name], f"{name}_point": pt[name][0]})
        return out


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
    ap.add_argument("--sample-errors", type=int, metavar="R",
                    help="add bootstrap sample errors from R replicates (keys sample_errors_*)")
    ap.add_argument("--seed", type=int, default=None, help="seed of the bootstrap")
    ap.add_argument("--refined", metavar="FILE",
                    help="refined results with tables and posteriors (refine --tables --posteriors): single-DLA runs")
    a = ap.parse_args(argv)
    from . import io
    snrs = a.snrs
    if snrs is None:
        nq = np.asarray(io.loadmat73(a.processed, ["min_z_dlas"])["min_z_dlas"]).size
        snrs = np.full(nq, np.inf)
    st = DLAStatistics.from_processed_file(a.processed, a.samples, snrs, sub_dla=a.sub_dla,
                                           occams_razor=a.occams_razor, snr_thresh=a.snr_thresh,
                                           lowzcut=a.lowzcut, block_size=a.block_size, device=a.device,
                                           **({} if a.refined is None else dict(refined=a.refined)))
    try:
        out = {k: _jsonable(v) for k, v in st.statistics(a.z_min, a.z_max, a.lnhi_nbins).items()}
        if a.sample_errors is not None:
            kw = {} if a.seed is None else dict(seed=a.seed)
            err = st.sample_errors(a.z_min, a.z_max, replicates=a.sample_errors, lnhi_nbins=a.lnhi_nbins, **kw)
            out.update({f"sample_errors_{k}": (v if isinstance(v, int) else _jsonable(v)) for k, v in err.items()
                        if not k.endswith("_replicates")})
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
