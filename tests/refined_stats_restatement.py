"""A NumPy restatement of what carries the refine pass into P(DLA) and the CDDF statistics,
written from the contract in include/gpdla.h, independently of csrc/refine_kernels.hpp and
csrc/stats_bin_body.hpp:

 - refined_posteriors: the model posteriors of the first pass's log_posteriors_no_dla against the refined
   log_posteriors_dla, by the five operations of the first pass, with the fallback to the first pass's numbers;
 - row_shift: the normaliser of a refined row, m + log Sum exp(lambda - m), the sum by math.fsum;
 - bin_posteriors_boxed: the per-row partials, by the EXISTING tests/cddf_restatement.py called row by row with
   that row's own mapped samples -- z_min / z_max = the box, offsets = u, log N = n_lo + (n_hi - n_lo) v (whose
   10** the existing restatement takes itself) -- and the shift given."""
import math

import numpy as np

import cddf_restatement as R


def refined_posteriors(lp_no, lp_dla_refined, refine_status, first_model_posteriors, first_p_no, first_p_dla):
    """What k_refined_posteriors writes for quasars with these columns: (model_posteriors_refined [n, 2],
    p_no_dlas_refined, p_dlas_refined, refined)."""
    n = len(refine_status)
    mp, p_no, p_dla = np.array(first_model_posteriors, dtype=np.float64), np.array(first_p_no, dtype=np.float64), \
        np.array(first_p_dla, dtype=np.float64)
    refined = np.zeros(n, dtype=np.int32)
    for i in range(n):
        if refine_status[i] != 0:
            continue
        a, b = np.float64(lp_no[i]), np.float64(lp_dla_refined[i])
        with np.errstate(invalid="ignore"):
            mx = np.fmax(a, b)
            p0, p1 = np.exp(a - mx), np.exp(b - mx)
            tot = p0 + p1
            p0, p1 = p0 / tot, p1 / tot
        mp[i] = (p0, p1)
        p_no[i], p_dla[i] = p0, 1 - p0
        refined[i] = 1
    return mp, p_no, p_dla, refined


def row_shift(lam_row):
    """m + log(Sum_j exp(lambda_j - m)) with m the maximum, NaN entries skipped by both, the sum exact before
    its one rounding (math.fsum); NaN for a row without a finite entry or with +inf."""
    l = np.asarray(lam_row, dtype=np.float64)
    l = l[~np.isnan(l)]
    if l.size == 0:
        return np.nan
    m = float(l.max())
    if not math.isfinite(m):
        return np.nan
    return m + math.log(math.fsum(np.exp(l - m)))


def row_shifts(lam):
    return np.array([row_shift(row) for row in np.asarray(lam, dtype=np.float64)])


def mapped_samples(box, u, v):
    """(z, log N) of a row: the unit points through its box, each operation rounded on its own."""
    z_lo, z_hi, n_lo, n_hi = (np.float64(x) for x in box)
    return z_lo + (z_hi - z_lo) * np.asarray(u, dtype=np.float64), n_lo + (n_hi - n_lo) * np.asarray(v, dtype=np.float64)


def bin_posteriors_boxed(lam, shift, p_dla, boxes, upper_z, u, v, requests):
    """What k_bin_posteriors_boxed writes for the rows ``lam`` [n, S'] given their ``shift``: the existing
    restatement, one row at a time on that row's own samples."""
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.shape[0]
    rows = []
    for s in range(n):
        _, lnhi = mapped_samples(boxes[s], u, v)
        rows.append(R.bin_posteriors(lam[s:s + 1], [shift[s]], [p_dla[s]], [boxes[s][0]], [boxes[s][1]], [upper_z[s]],
                                     u, lnhi, requests))
    return [{k: np.concatenate([row[r][k] for row in rows]) for k in rows[0][r]} for r in range(len(requests))] if n else \
        R.bin_posteriors(lam, [], [], [], [], [], u, np.asarray(v, dtype=np.float64), requests)
