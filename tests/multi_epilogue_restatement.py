"""Exact restatement of the multi-DLA epilogue (plain module: tests/test_multi_epilogue.py and
tests/test_gpu_multi_epilogue.py import it; no package compute code is used).

Written from the definitions in csrc/multi_kernels.hpp and the reference lines it cites
(multi_dlas/process_qsos_multiple_dlas_meanflux.m, "multi :N"):

* ``uniforms``: the 53-bit uniform of draw j of model step nd of quasar qid, as an exact integer over 2^53
  (Philox4x32-10 from mock_restatement; counter (lo32 j, hi32 j, nd, 0), key (lo32(seed ^ qid),
  hi32(seed) ^ hi32(qid) ^ 0x5851F42D), u = ((r0 >> 5) 2^26 + (r1 >> 6)) / 2^53);
* ``weights_exact`` / ``acceptable``: the weights W_i = exp(l_i - max) (NaN -> 0, multi :467-470), their exact
  prefix sums at 50 digits, and the set of indices a correct inverse-CDF draw may return;
* ``evidence_exact``: first NaN-skipping maximum, max + log(nanmean(exp(l - max))), Occam term (multi :400-409);
* ``separation_mask`` (multi :386-392), ``map_chain`` (multi :439-445), ``posteriors_exact`` (multi :482-495);
* ``emulate_resample``: k_multi_resample's own float64 order in NumPy, with named mutations -- it exists so that
  the CPU test can show that the acceptance rule rejects a wrong kernel (and what the 40-bin chi-square of
  tests/test_gpu_configs.py::test_resampling_follows_the_weights, restated in ``chi_square_40``, makes of it).
"""
from __future__ import annotations

import numpy as np
import mpmath as mp

from mock_restatement import philox4x32_10

DPS = 50
M32 = np.uint64(0xFFFFFFFF)
TWO53 = 2 ** 53
UNIFORM_MUTATIONS = ("same_stream_every_model", "key_low_word_only", "uniform_from_r0_only")
SCAN_MUTATIONS = ("index_minus_one", "inclusive_offsets")
MUTATIONS = SCAN_MUTATIONS + UNIFORM_MUTATIONS


# ------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------

def uniforms(seed: int, qid: int, nd: int, S: int, mutate: str | None = None) -> np.ndarray:
    """m[j], j < S, uint64 with u_j = m[j] / 2^53 exactly (m < 2^53, so ``m * 2.0 ** -53`` is u_j as a double).

    ``mutate`` (for the emulation only): "same_stream_every_model" puts 0 in the counter word that carries nd;
    "key_low_word_only" drops the high halves of seed and qid from the key; "uniform_from_r0_only" drops the 26
    bits that come from r1."""
    assert mutate is None or mutate in UNIFORM_MUTATIONS
    seed, qid = int(seed) & (2 ** 64 - 1), int(qid) & (2 ** 64 - 1)
    k0 = (seed ^ qid) & 0xFFFFFFFF
    k1 = ((seed >> 32) ^ (qid >> 32) ^ 0x5851F42D) & 0xFFFFFFFF
    if mutate == "key_low_word_only":
        k1 = 0x5851F42D
    j = np.arange(S, dtype=np.uint64)
    word = 0 if mutate == "same_stream_every_model" else int(nd)
    r = philox4x32_10(j & M32, j >> np.uint64(32), word, 0, k0, k1)
    hi = (r[0] >> np.uint64(5)) << np.uint64(26)
    return hi if mutate == "uniform_from_r0_only" else hi + (r[1] >> np.uint64(6))


# ------------------------------------------------------------------------------------------------
# the weighted draw
# ------------------------------------------------------------------------------------------------

def nan_first_max(col):
    """(max, first index attaining it) over the non-NaN entries; (nan, 0) for an all-NaN column (MATLAB's
    nanmax returns index 1 there, multi :439)."""
    col = np.asarray(col, dtype=np.float64)
    ok = ~np.isnan(col)
    if not ok.any():
        return np.nan, 0
    mx = col[ok].max()
    return float(mx), int(np.flatnonzero(ok & (col == mx))[0])


def weights_exact(col) -> dict:
    """W_i = exp(l_i - max) at 50 digits (0 where l_i is NaN), the inclusive prefix sums C_i, the total T and the
    normalised prefix sums F_i = C_i / T; ``Ff`` is F rounded to double (non-decreasing, for bracketing only)."""
    col = np.asarray(col, dtype=np.float64)
    mx, _ = nan_first_max(col)
    with mp.workdps(DPS):
        m = mp.mpf(mx)
        W = [mp.mpf(0) if np.isnan(v) else mp.exp(mp.mpf(float(v)) - m) for v in col]
        C, acc = [], mp.mpf(0)
        for w in W:
            acc += w
            C.append(acc)
        T = acc
        F = [c / T for c in C]
    return dict(col=col, nan=np.isnan(col), max=mx, W=W, C=C, T=T, F=F, Ff=np.array([float(f) for f in F]))


def eps_of(S: int) -> float:
    """(ceil(S / 256) + 260) 2^-52: see ``acceptable``."""
    return (-(-int(S) // 256) + 260) * 2.0 ** -52


def _accept_exact(ex, i, m, eps):
    F = ex["F"]
    with mp.workdps(DPS):
        u = mp.mpf(int(m)) / TWO53
        lo = F[i - 1] if i > 0 else mp.mpf(0)
        return (not ex["nan"][i]) and lo - eps <= u <= F[i] + eps


def acceptable_all(col, m, ex: dict | None = None):
    """All draws of one column at once.  Returns ``(unique, other)``: ``unique[j]`` is THE acceptable index of draw j
    where the set has exactly one member and -1 elsewhere; ``other[j]`` is the sorted list of acceptable indices of
    every draw whose set has another size.  See ``acceptable`` for the rule."""
    ex = ex or weights_exact(col)
    S = ex["col"].size
    eps, Ff = eps_of(S), ex["Ff"]
    u = np.asarray(m, dtype=np.uint64).astype(np.float64) * 2.0 ** -53       # exact
    # i qualifies only if F_i >= u - eps and F_{i-1} <= u + eps: bracket with doubles and a doubled margin,
    # decide with the 50-digit values
    lo = np.searchsorted(Ff, u - 2 * eps, side="left")
    hi = np.minimum(np.searchsorted(Ff, u + 2 * eps, side="right"), S - 1)
    unique = np.where(lo == hi, lo, -1).astype(np.int64)   # Ff[lo-1] < u - 2 eps and Ff[lo] > u + 2 eps: inside
    other = {}
    for j in np.flatnonzero(lo != hi):
        got = [i for i in range(int(lo[j]), int(hi[j]) + 1) if _accept_exact(ex, i, m[j], eps)]
        if len(got) == 1:
            unique[j] = got[0]
        else:
            other[int(j)] = got
    return unique, other


def acceptable(col, u, ex: dict | None = None) -> set:
    """The indices (0-based) a correct kernel may return for the draw u = m / 2^53 (``u`` is the integer m).

    k_multi_resample returns the first i with cdf_i > u * total, cdf being its float64 prefix sums of
    exp(l - max) and total their last entry.  In exact arithmetic that is the i with C_{i-1}/T <= u < C_i/T.
    Index i qualifies here if l_i is not NaN and

        C_{i-1}/T - eps <= u <= C_i/T + eps,        eps = (ceil(S/256) + 260) 2^-52,

    with C, T the exact prefix sums.  Derivation of eps, in units of 2^-52 relative to T (every cdf_i <= total):
    a thread's serial sum over its chunk of ceil(S/256) samples rounds once per add (ceil(S/256)); the serial
    exclusive offsets round once per thread (256); the device exp is good to one ulp (1); ``u * total`` rounds
    once (1) and the final add ``cdf_i += off`` once (1): ceil(S/256) + 259, rounded up to 260.  Each rounding is
    at most 2^-53 of a partial sum that does not exceed T, so counting 2^-52 for each bounds the distance of
    cdf_i / total from C_i / T twice over, which also pays for the same roundings in ``total`` itself.  (The
    subtraction l_i - max is exact for
    every sample that carries weight when |l| is large against the spread, by Sterbenz; where it rounds, the
    relative error |l_i - max| 2^-53 of W_i is weighted by W_i / T and stays inside the same margin.)

    A sample with l_i - max < -700 has W_i / T < 1e-304, far below eps: whether the device's exp gives it a
    subnormal weight or none, it is returned only for a u that this rule already allows, and it is never the only
    member of a set unless u is within eps of its interval -- so it is allowed either way and never required."""
    ex = ex or weights_exact(col)
    unique, other = acceptable_all(ex["col"], np.array([int(u)], dtype=np.uint64), ex)
    return {int(unique[0])} if unique[0] >= 0 else set(other[0])


def emulate_resample(col, u, mutate: str | None = None, key=None) -> np.ndarray:
    """k_multi_resample in float64 NumPy, in the kernel's own order: thread t < 256 owns the chunk
    [t c, (t + 1) c), c = ceil(S / 256), and sums it serially; thread 0 turns the 256 chunk sums into exclusive
    offsets, serially; every thread adds its offset; a draw is the first index with cdf > u * cdf[S - 1], found by
    bisection.  ``u``: the integers of ``uniforms``.  Returns 0-based indices (int64; -1 where the kernel would
    have written 0).

    ``mutate``: "index_minus_one" (the ``+ 1`` of the 1-based index dropped), "inclusive_offsets"
    (``s_part[t] = acc`` after the add), or one of the generator mutations of ``uniforms``, for which
    ``key = (seed, qid, nd)`` is needed and ``u`` is replaced."""
    assert mutate is None or mutate in MUTATIONS
    col = np.asarray(col, dtype=np.float64)
    S = col.size
    if mutate in UNIFORM_MUTATIONS:
        u = uniforms(key[0], key[1], key[2], S, mutate=mutate)
    mx, _ = nan_first_max(col)
    with np.errstate(invalid="ignore", under="ignore"):
        w = np.where(np.isnan(col), 0.0, np.exp(col - mx))
    c = -(-S // 256)
    pad = np.zeros(256 * c)
    pad[:S] = w
    run = np.cumsum(pad.reshape(256, c), axis=1)          # serial within a chunk
    part = run[:, -1]
    incl = np.cumsum(part)                                # acc after the add, serially
    off = incl if mutate == "inclusive_offsets" else np.concatenate([[0.0], incl[:-1]])
    cdf = (run + off[:, None]).reshape(-1)[:S]
    target = np.asarray(u, dtype=np.uint64).astype(np.float64) * 2.0 ** -53 * cdf[S - 1]
    idx = np.minimum(np.searchsorted(cdf, target, side="right"), S - 1).astype(np.int64)
    return idx - 1 if mutate == "index_minus_one" else idx


def check_draws(col, m, drawn, ex: dict | None = None):
    """(number of draws outside their acceptable set, number of draws whose set has more than one member)."""
    unique, other = acceptable_all(col, m, ex)
    drawn = np.asarray(drawn, dtype=np.int64)
    bad = int(((unique >= 0) & (drawn != unique)).sum())
    bad += sum(1 for j, s in other.items() if int(drawn[j]) not in s)
    return bad, sum(1 for s in other.values() if len(s) > 1)


def chi_square_40(col, drawn):
    """The statistic of tests/test_gpu_configs.py::test_resampling_follows_the_weights on one column and its draws
    (0-based): (statistic, its 99.99 % quantile, draws landing where W = 0)."""
    from scipy.stats import chi2
    col = np.asarray(col, dtype=np.float64)
    S = col.size
    with np.errstate(invalid="ignore", under="ignore"):
        w = np.exp(col - np.nanmax(col))
    w[np.isnan(w)] = 0.0
    w /= w.sum()
    cum = np.concatenate([[0.0], np.cumsum(w)])
    edges = np.searchsorted(cum, np.arange(1, 40) / 40.0)
    bins = np.searchsorted(edges, np.asarray(drawn, dtype=np.int64), side="right")
    observed = np.bincount(bins, minlength=40).astype(np.float64)
    expected = S * np.diff(np.concatenate([[0.0], cum[edges], [1.0]]))
    ok = expected > 5
    stat = float(((observed - expected)[ok] ** 2 / expected[ok]).sum())
    return stat, float(chi2.ppf(0.9999, int(ok.sum()))), int(observed[expected == 0].sum())


# ------------------------------------------------------------------------------------------------
# evidences, mask, MAP, posteriors
# ------------------------------------------------------------------------------------------------

def evidence_exact(col, nd: int = 1):
    """(max, first index of the max, max + log(mean(exp(l - max))) - (nd - 1) log S) over the non-NaN entries
    (multi :400-409); the last as an mpf at 50 digits, NaN for an all-NaN column."""
    col = np.asarray(col, dtype=np.float64)
    mx, arg = nan_first_max(col)
    if np.isnan(mx):
        return mx, arg, mp.nan
    with mp.workdps(DPS):
        m = mp.mpf(mx)
        live = [mp.mpf(float(v)) for v in col[~np.isnan(col)]]
        mean = mp.fsum(mp.exp(v - m) for v in live) / len(live)
        return mx, arg, m + mp.log(mean) - (nd - 1) * mp.log(col.size)


def evidence_bound(mx: float, S: int) -> float:
    """2 spacing(|max|) + (ceil(S/256) + 16) 2^-52: the strided partial sums of nan_evidence (ceil(S/256) adds
    per thread, 6 + 3 in the reduction), one exp, the division, one log, the final add and the Occam term."""
    return 2 * float(np.spacing(abs(mx))) + (-(-int(S) // 256) + 16) * 2.0 ** -52


def separation_mask(z, base, nd: int, min_sep: float) -> np.ndarray:
    """True where the nd absorbers of a sample -- its own and those of base[0 .. nd-2] (1-based; 0 = never drawn)
    -- hold two closer than ``min_sep``: any(diff(sort(z)) < min_sep), multi :386-392."""
    z = np.asarray(z, dtype=np.float64)
    if nd == 1:
        return np.zeros(z.size, dtype=bool)
    b = np.asarray(base)[:nd - 1].astype(np.int64) - 1
    zs = np.concatenate([z[None], z[np.maximum(b, 0)]], axis=0)
    return (np.diff(np.sort(zs, axis=0), axis=0) < min_sep).any(axis=0) | (b < 0).any(axis=0)


def closest_to_separation(z, base, nd: int, min_sep: float) -> float:
    """min over samples and absorber pairs of | |z_x - z_y| - min_sep |, in units of spacing(min_sep)."""
    z = np.asarray(z, dtype=np.float64)
    b = np.asarray(base)[:nd - 1].astype(np.int64) - 1
    zs = np.concatenate([z[None], z[np.maximum(b, 0)]], axis=0)
    worst = np.inf
    for x in range(nd):
        for y in range(x + 1, nd):
            worst = min(worst, float(np.abs(np.abs(zs[x] - zs[y]) - min_sep).min()))
    return worst / float(np.spacing(min_sep))


def map_chain(col, base, nd: int) -> np.ndarray:
    """MAP_inds[model nd, :] as 1-based doubles (multi :439-445): the first NaN-skipping maximum (index 1 for an
    all-NaN column), then its chain through base[0 .. nd-2]; a never-drawn (zero) link leaves NaN."""
    _, arg = nan_first_max(col)
    out = [float(arg + 1)]
    for j in range(nd - 1):
        b = int(np.asarray(base)[j][arg])
        out.append(float(b) if b >= 1 else np.nan)
    return np.array(out)


def posteriors_exact(lp, ll):
    """(log posteriors as doubles, model posteriors as mpf, p_dla as mpf) from the log priors and the log
    evidences in the order (no DLA, sub-DLA, 1 .. max_dlas DLAs): lpost = fl(lp + ll), one rounding each; the
    maximum skips NaN, the sum does not (multi :482-491); p_dla = 1 - p_no - p_lls (:493-495)."""
    lpost = np.asarray(lp, dtype=np.float64) + np.asarray(ll, dtype=np.float64)
    ok = ~np.isnan(lpost)
    with mp.workdps(DPS):
        if not ok.all():
            return lpost, [mp.nan] * lpost.size, mp.nan
        m = mp.mpf(float(lpost.max()))
        e = [mp.exp(mp.mpf(float(v)) - m) for v in lpost]
        tot = mp.fsum(e)
        post = [x / tot for x in e]
        return lpost, post, 1 - post[0] - post[1]


def ulps(got: float, want) -> float:
    """|got - want| in units of spacing(|want|), ``want`` an mpf or a float (0 only for an exact 0)."""
    with mp.workdps(DPS):
        w = float(want)
        if w == 0.0:
            return 0.0 if got == 0.0 else np.inf
        return float(abs(mp.mpf(float(got)) - want) / mp.mpf(float(np.spacing(abs(w)))))


# ------------------------------------------------------------------------------------------------
# the tables of the CPU test
# ------------------------------------------------------------------------------------------------

TABLE_SIZES = (1, 63, 255, 256, 257, 513, 769, 1024, 19200)
TABLE_KINDS = ("broad", "peaked", "nans", "equal_maxima")


def table(kind: str, S: int) -> np.ndarray:
    """A column of log-likelihoods: "broad" -- normal, sigma 2, around -3000; "peaked" -- the same with one sample 800
    above the rest, so that every other weight underflows to 0; "nans" -- broad with a run of NaN at the head, one
    in the middle and one at the tail (none where S = 1); "equal_maxima" -- broad with its maximum repeated."""
    rng = np.random.default_rng(1000 * TABLE_KINDS.index(kind) + S)
    col = -3000.0 + 2.0 * rng.standard_normal(S)
    if kind == "peaked":
        col[(2 * S) // 3] += 800.0
    elif kind == "nans" and S > 1:
        col[:max(1, S // 9)] = np.nan
        col[S // 2] = np.nan
        col[S - 1] = np.nan
    elif kind == "equal_maxima" and S > 1:
        col[(int(np.nanargmax(col)) + S // 2) % S] = np.nanmax(col)
    return col
