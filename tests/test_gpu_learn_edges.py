"""The paths and branches of csrc/learn_kernels.hpp that BOSS-like synthetic spectra never reach, each held to the numpy
restatement (tests/learn_restatement.py) under the bounds of test_gpu_learn.py, with exact counts and exact NaN / +-inf
placement (learn_hard_cases.against_restatement):

    unstaged     k_learn_rest_grid reads the rest wavelengths from HBM above kLearnStage = 4096 pixels: spectra of 4096
                 (staged), 4097, 4098, 4396 and 4101 pixels whose pixels over the grid are the same give the same rows, bit
                 for bit, in one batch that mixes both paths (and holds three shorter spectra of its own)
    bracket      queries exactly on pixels (z_qso = 1, observed wavelengths 2 x grid points): X(0), X(n - 1) with the bracket
                 clipped to n - 2, a masked last pixel, a masked interior pixel, n = 2, 1, 0, spectra blue of, red of and
                 one grid point wide; on the reference's dyadic grid and on 911.3 + 0.3 p, which rounds
    splits       the quasar splits of k_learn_colsum (ceil(nq / 64), at most 64) and k_learn_gram (4-quasar steps, 256 a
                 split, at most 8), at their boundaries and caps, every nq mod 4, and npairs x nsplit leaving 1, 2 and 3
                 idle waves in the last block; the count matrix is the exact check of every split edge
    complete     no complete row, exactly one (0 / 0 everywhere), exactly two
"""
import numpy as np
import pytest

import learn_hard_cases as LC
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

pytestmark = pytest.mark.gpu

STAGE = 4096          # kLearnStage


def params(meanflux, **kw):
    return MultiParameters(**kw) if meanflux else Parameters(**kw)


def small_grid(meanflux, G, lo=None, dlambda=0.25):
    lo = (1020.0 if meanflux else 1100.0) if lo is None else lo
    return params(meanflux, min_lambda=lo, max_lambda=lo + dlambda * (G - 1), dlambda=dlambda)


def check(csr, p, meanflux):
    got = LC.evaluate(csr, p, meanflux)
    bad = LC.against_restatement(got, LC.restated(("edges", meanflux), csr, p), meanflux)
    assert not bad, bad
    return got


# ---------------------------------------------------------------- the unstaged path

@pytest.mark.parametrize("meanflux", [False, True], ids=["single", "meanflux"])
def test_unstaged_rows_equal_the_staged_row(meanflux):
    p = params(meanflux)
    rng = np.random.default_rng(77)
    z = 2.5
    # A: exactly 4096 pixels over [911.5, 1216.0], the whole default rest grid
    rest = 911.5 + (1216.0 - 911.5) / (STAGE - 1) * (np.arange(STAGE) + rng.uniform(-0.3, 0.3, STAGE))
    nv = 10 ** rng.uniform(-2.0, -0.3, STAGE)
    nv[1000:1010] = 3.0 * p.max_noise_variance
    flux = 1 + 0.3 * np.sin(rest / 7) + np.sqrt(nv) * rng.standard_normal(STAGE)
    mask = (rng.uniform(size=STAGE) < 0.02).astype(np.uint8)
    A = [rest * (1 + z), flux, nv, mask]

    def extended(before, after):
        blue = (rest[0] - 0.1 * np.arange(before, 0, -1)) * (1 + z)
        red = (rest[-1] + 0.1 * np.arange(1, after + 1)) * (1 + z)
        return [np.concatenate([blue, A[0], red]), np.concatenate([np.full(before, 7.0), A[1], np.full(after, 7.0)]),
                np.concatenate([np.full(before, 0.1), A[2], np.full(after, 0.1)]),
                np.concatenate([np.zeros(before, np.uint8), A[3], np.zeros(after, np.uint8)])]

    quasars = [A, extended(0, 1), extended(0, 2), extended(0, 300), extended(5, 0)]
    assert [q[0].size for q in quasars] == [4096, 4097, 4098, 4396, 4101]
    for i in range(3):      # three staged spectra of their own, unmasked, so that the covariances are of something
        quasars.append([A[0][i::2], 1 + 0.3 * np.sin(rest[i::2] / 7 + i) + 0.2 * rng.standard_normal(rest[i::2].size),
                        np.full(rest[i::2].size, 0.05), np.zeros(rest[i::2].size, np.uint8)])
    csr = LC._pack(quasars, np.full(len(quasars), z))
    got = check(csr, p, meanflux)
    assert np.isfinite(got["rest_flux"][0]).sum() > 1000 and np.isnan(got["rest_flux"][0]).sum() > 10
    for key in ("rest_flux", "lya_1pzs", "rest_noise"):
        for q in range(1, 5):
            np.testing.assert_array_equal(got[key][q], got[key][0], err_msg=f"{key}, spectrum {q}")


# ---------------------------------------------------------------- bracket edges

def on_grid_spectra(p, G):
    """z_qso = 1, observed wavelengths 2 x (grid points): the rest wavelengths are the grid points exactly"""
    xq = p.min_lambda + np.arange(G) * p.dlambda
    rng = np.random.default_rng(5)

    def at(points, masked=(), rest=None):
        rest = xq[list(points)] if rest is None else np.asarray(rest, dtype=np.float64)
        n = rest.size
        mk = np.zeros(n, np.uint8)
        mk[list(masked)] = 1
        return [2.0 * rest, 1 + rng.uniform(-0.5, 0.5, n), 10 ** rng.uniform(-2.0, -0.5, n), mk]

    every, other = range(G), range(0, G, 2)
    lo, hi, d = xq[0], xq[-1], p.dlambda
    return [at(every),                                       # X(0) and X(n - 1) on the first and last grid point
            at(every, masked=[G - 1]),                       # the last observed pixel masked
            at(every, masked=[10]),                          # an interior masked pixel, a query on it
            at(other, masked=[5]),                           # ... and queries inside both of its intervals
            at(other, masked=[len(other) - 1]),
            at([3, 7]), at([3, 4]), at([5]), at([]),         # n = 2 (wide, adjacent), 1, 0
            at([], rest=[lo - 40.0, lo - 30.0, lo - 20.0]),  # entirely blue of the grid
            at([], rest=[hi + 20.0, hi + 30.0, hi + 40.0]),  # entirely red
            at([], rest=[xq[16] - 0.4 * d, xq[16] + 0.4 * d]),   # one grid point wide
            at([], rest=[xq[16], xq[16] + 0.4 * d]),         # ... with X(0) on it
            at([], rest=[xq[16] - 0.4 * d, xq[16]]),         # ... with X(n - 1) on it
            at(range(4, 21))]                                # part of the grid, both ends on grid points


@pytest.mark.parametrize("meanflux", [False, True], ids=["single", "meanflux"])
@pytest.mark.parametrize("grid", [(None, 0.25), (911.3, 0.3)], ids=["dyadic", "rounded"])
def test_queries_on_pixels_and_spectrum_ends(grid, meanflux):
    G = 33
    p = small_grid(meanflux, G, *grid)
    quasars = on_grid_spectra(p, G)
    csr = LC._pack(quasars, np.ones(len(quasars)))
    got = check(csr, p, meanflux)
    F = got["rest_flux"]
    assert np.isfinite(F[0]).all()                                          # both ends are inside
    assert np.isfinite(F[1, :G - 2]).all() and np.isnan(F[1, G - 2:]).all()   # t = 0 and t = 1 next to the masked last pixel
    assert np.isnan(F[2, 9:11]).all() and np.isfinite(F[2, 11]) and np.isfinite(F[2, 8])
    assert np.isnan(F[3, 8:12]).all() and np.isfinite(F[3, 12]) and np.isfinite(F[3, 7])
    assert np.isfinite(F[5, 3:8]).all() and np.isnan(F[5, :3]).all() and np.isnan(F[5, 8:]).all()
    for q in (7, 8, 9, 10):
        assert np.isnan(F[q]).all() and np.isnan(got["lya_1pzs"][q]).all()
    for q in (11, 12, 13):
        assert np.flatnonzero(np.isfinite(F[q])).tolist() == [16]
    assert np.flatnonzero(np.isfinite(F[14])).tolist() == list(range(4, 21))


# ---------------------------------------------------------------- split and tile edges

def short_spectra(nq, G, p, seed=0):
    """nq quasars of G + 1 pixels that bracket every grid point (the midpoint construction of learn_hard_cases, built in
    one piece): distinct amplitudes 1 + q / nq, a tenth of the pixels masked in two quasars of three"""
    rng = np.random.default_rng(1000 + seed)
    z = rng.uniform(2.2, 4.5, nq)
    n = G + 1
    rest = p.min_lambda + (np.arange(n)[None, :] - 0.5 + rng.uniform(-0.3, 0.3, (nq, n))) * p.dlambda
    amp = 1.0 + np.arange(nq) / nq
    flux = amp[:, None] * (1 + 0.3 * np.sin(rest / 3 + rng.uniform(0, 6, (nq, 1))) + 0.1 * rng.standard_normal((nq, n)))
    mask = (rng.uniform(size=(nq, n)) < 0.1) & (np.arange(nq) % 3 != 0)[:, None]
    return dict(offsets=np.arange(nq + 1, dtype=np.int64) * n, wavelengths=(rest * (1 + z[:, None])).ravel(), flux=flux.ravel(),
                noise_variance=np.full(nq * n, 0.05), pixel_mask=mask.ravel().astype(np.uint8), z_qsos=z)


def gram_splits(nq):
    return max(1, min(8, -(-(-(-nq // 4)) // 256)))


def idle_waves(nq, G):
    tiles = -(-G // 16)
    return -(tiles * (tiles + 1) // 2 * gram_splits(nq)) % 4


#       nq: the column splits' edges {63, 64, 65, 128, 129, 4096, 4097, 4161} and the gram's {1 .. 5, 1023, 1024, 1025, 1028,
#       1029, 7168, 7169, 7173, 8195}; G in {1, 15, 16, 17, 33, 49}
SPLIT_CASES = [(1, 1), (2, 15), (3, 16), (4, 17), (5, 33), (63, 17), (64, 49), (65, 16), (128, 17), (129, 33), (1023, 17),
               (1024, 16), (1025, 1), (1025, 17), (1028, 33), (1029, 49), (4096, 17), (4097, 16), (4161, 17), (7168, 1),
               (7168, 17), (7169, 17), (7173, 33), (8195, 17), (8195, 49)]


def test_the_split_cases_cover_the_idle_waves():
    """(no kernel runs here) more than one split with 1, 2 and 3 idle waves in the last block of k_learn_gram"""
    assert {idle_waves(nq, G) for nq, G in SPLIT_CASES if gram_splits(nq) > 1} == {0, 1, 2, 3}
    assert [gram_splits(n) for n in (1024, 1025, 7168, 7169, 8195)] == [1, 2, 7, 8, 8]
    assert (idle_waves(7168, 1), idle_waves(1025, 17), idle_waves(7168, 17)) == (1, 2, 3)


@pytest.mark.parametrize("nq,G", SPLIT_CASES)
def test_quasar_splits_and_tiles(nq, G):
    p = small_grid(False, G)
    csr = short_spectra(nq, G, p, seed=nq + G)
    got = check(csr, p, False)
    if nq >= 63:
        assert got["rows_complete"] >= 2 and (got["N_pairwise"] < nq).any()


# ---------------------------------------------------------------- complete rows at the limits

@pytest.mark.parametrize("complete", [0, 1, 2])
def test_complete_rows_at_the_limits(complete):
    G, nq = 17, 6
    p = small_grid(False, G)
    csr = short_spectra(nq, G, p, seed=50)
    mask = csr["pixel_mask"].reshape(nq, G + 1)
    mask[:] = 0
    mask[np.arange(complete, nq), 2 + np.arange(complete, nq)] = 1      # every quasar past the first ``complete`` lacks a pixel
    got = check(csr, p, False)
    assert got["rows_complete"] == complete
    if complete == 1:
        assert np.isnan(got["cov_complete"]).all()
    if complete == 2:
        assert np.isfinite(got["cov_complete"]).all()
