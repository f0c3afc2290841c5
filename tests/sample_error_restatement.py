"""The stratified bootstrap of gp_dla_detection_amd/cddf.py (k_bootstrap_sums) restated in NumPy:
Philox4x32-10, the draw mapping, and the replicate sums by math.fsum.  DESIGN.md section 4.14."""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
STREAM = 2    # counter word 3 of the bootstrap (resampling: 0, mocks: 1)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counter words (uint64 holding 32-bit values); returns the four
    output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def stratum_extents(stratum):
    """(first row, size) of the stratum of every position of a stratum-sorted set."""
    lab = np.asarray(stratum)
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    sizes = np.diff(np.r_[starts, lab.size])
    which = np.searchsorted(starts, np.arange(lab.size), side="right") - 1
    return starts[which], sizes[which]


def drawn_rows(stratum, replicate, seed):
    """The row every position draws in one replicate."""
    first, size = stratum_extents(stratum)
    j = np.arange(len(first), dtype=np.uint64)
    w = philox4x32_10(j & MASK, j >> np.uint64(32), np.uint64(replicate), np.uint64(STREAM),
                      seed & 0xFFFFFFFF, seed >> 32)[0]
    return first + ((w * size.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)


def bootstrap_sums(V, stratum, replicates, seed, first_replicate=0):
    V = np.asarray(V, dtype=np.float64)
    out = np.empty((replicates, V.shape[1]))
    for r in range(replicates):
        rows = drawn_rows(stratum, first_replicate + r, seed)
        for c in range(V.shape[1]):
            out[r, c] = math.fsum(V[rows, c])
    return out
