"""A numpy restatement of the per-spectrum pass of the CDDF statistics (CDDF_analysis/calc_cddf.py,
class DLACatalogue), written from the contract in DESIGN.md section 4.11, independently of
csrc/stats_kernels.hpp.  It is the yardstick k_bin_posteriors and k_poisson_binomial_cf are held to
by tests/test_gpu_cddf.py; tests/test_cddf.py drives gp_dla_detection_amd.cddf's host statistics
from it against the numbers the reference itself produced."""
import math

import numpy as np

from gp_dla_detection_amd.cddf import KEPT_CAPACITY


def sample_probabilities(sll_row, shift, p_dla):
    """exp(log_norm_like) * p_dla with log_norm_like = sll - (log_likelihoods_dla + log(S))
    (:223-228, :931); ``shift`` is the bracket, formed by the caller."""
    return np.exp(np.asarray(sll_row, dtype=np.float64) - shift) * p_dla


def sample_redshifts(z_min, z_max, offsets):
    """z_min + (z_max - z_min) * offset (:913), each operation rounded on its own."""
    return z_min + (z_max - z_min) * np.asarray(offsets, dtype=np.float64)


def _strict(req, p, z, lnhi, z_up, nb):
    """_split_distributions_single (:994-1034) for one spectrum: per-bin sums of the probabilities
    below p_switch and the (bin, p) pairs at or above it, in sample order."""
    q = lnhi if req.quantity == "lnhi" else z
    e = req.edges
    pois = np.zeros(nb)
    kept = []
    with np.errstate(invalid="ignore"):
        sel = (lnhi > req.lnhi_lo) & (lnhi < req.lnhi_hi) & (z < z_up) & (z > req.z_lo)   # :1002
        sel &= p > req.p_thresh_sample                                                  # :1014
        for b in range(nb):
            inb = sel & (q > e[b]) & (q < e[b + 1])                                     # :1023
            small = p[inb & (p < req.p_switch)]
            if small.size:
                pois[b] = math.fsum(small)                                              # :1030
        for j in np.flatnonzero(sel & (p >= req.p_switch)):                             # :1032
            b = np.flatnonzero((q[j] > e[:-1]) & (q[j] < e[1:]))
            if b.size:
                kept.append((int(b[0]), float(p[j])))
    return pois, kept


def _histogram(req, p, z, lnhi, nb):
    """_get_z_nhi_hist (:1101-1125) for one spectrum: np.histogram's bins ([a, b), the last one
    closed) of w p and w^2 (1 - p) p, w = 10**lnhi (moment) or 1.  A NaN weight makes its own bin
    NaN and, as np.histogram's cumulative sums do, every later bin."""
    q = lnhi if req.quantity == "lnhi" else z
    e = req.edges
    w = np.power(10.0, lnhi) if req.moment else np.ones_like(p)
    with np.errstate(invalid="ignore"):
        sel = (lnhi > req.lnhi_lo) & (lnhi < req.lnhi_hi) & (z < req.z_hi) & (z > req.z_lo)   # :1105
    mean = np.zeros(nb)
    var = np.zeros(nb)
    wm = w * p
    wv = w * w * (1 - p) * p
    for b in range(nb):
        inb = sel & (q >= e[b]) & ((q < e[b + 1]) if b < nb - 1 else (q <= e[b + 1]))
        if inb.any():
            mean[b] = math.fsum(wm[inb]) if not np.isnan(wm[inb]).any() else np.nan
            var[b] = math.fsum(wv[inb]) if not np.isnan(wv[inb]).any() else np.nan
    bad = sel & np.isnan(wm)
    if bad.any():
        lowest = q[bad].min()
        first = np.flatnonzero(lowest < e[1:])
        if nb and lowest == e[-1]:
            first = np.array([nb - 1])
        if first.size:
            mean[first[0]:] = np.nan
            var[first[0]:] = np.nan
    return mean, var


def bin_posteriors(sll, shift, p_dla, z_min, z_max, upper_z, offsets, lnhi, requests):
    """What k_bin_posteriors writes for a block of selected spectra: per request, ``pois`` / ``mean``
    / ``var`` [n, B] and ``count`` [n], ``kept_bin`` / ``kept_p`` [n, KEPT_CAPACITY] (unused slots
    -1 / 0).  ``count`` is the true number of kept pairs, even above the capacity."""
    sll = np.asarray(sll, dtype=np.float64)
    n = sll.shape[0]
    lnhi = np.asarray(lnhi, dtype=np.float64)
    out = []
    for req in requests:
        nb = len(req.edges) - 1
        r = dict(pois=np.zeros((n, nb)), mean=np.zeros((n, nb)), var=np.zeros((n, nb)),
                 count=np.zeros(n, dtype=np.int32), kept_bin=np.full((n, KEPT_CAPACITY), -1, dtype=np.int32),
                 kept_p=np.zeros((n, KEPT_CAPACITY)))
        for s in range(n):
            p = sample_probabilities(sll[s], shift[s], p_dla[s])
            z = sample_redshifts(z_min[s], z_max[s], offsets)
            if req.histogram:
                r["mean"][s], r["var"][s] = _histogram(req, p, z, lnhi, nb)
                continue
            z_up = min(upper_z[s], req.z_hi) if req.lowzcut else req.z_hi             # :998-1000
            r["pois"][s], kept = _strict(req, p, z, lnhi, z_up, nb)
            r["count"][s] = len(kept)
            for i, (b, v) in enumerate(kept[:KEPT_CAPACITY]):
                r["kept_bin"][s, i] = b
                r["kept_p"][s, i] = v
        out.append(r)
    return out


def cf_sums(pp):
    """stable_complex_product's two sums (:1293-1295, :1315-1317) for every n in 0 .. (N+1)//2:
    fsum_j log|1 + p_j (e^{-2 pi i n/(N+1)} - 1)| and fsum_j arg(...)."""
    pp = np.asarray(pp, dtype=np.float64)
    nsamp = pp.size
    logs, args = [], []
    for nn in range(((nsamp + 1) // 2) + 1):
        nco = complex(math.cos(-2 * math.pi * nn / (nsamp + 1)), math.sin(-2 * math.pi * nn / (nsamp + 1))) - 1
        c = 1 + pp * nco
        logs.append(math.fsum(np.log(np.absolute(c))))
        args.append(math.fsum(np.angle(c)))
    return np.array(logs), np.array(args)


def cf_segments(segments):
    """cf_sums of every segment: the host side's ``cf`` callable."""
    return [cf_sums(s) for s in segments]
