"""NumPy-and-oracle restatement of the model spectra of a multi-DLA run (a plain module beside
tests/model_spectra_restatement.py, which it builds on: the grid, the weights and the moments of one profile are
that module's).  No package compute code is used.

Per quasar, model n and sample i:

* slots    s_1(i) = i, s_j(i) = base[j - 2][i] - 1 for j = 2 .. n (``base``: the quasar's ``[max_dlas - 1, S]`` rows of
           ``base_sample_inds``, 1-based, 0 = never drawn);
* profile  A_{n,i} = Prod_j oracle.voigt(pad, z_{s_j(i)}, N_{s_j(i)}) in slot order -- a product of broadened
           profiles (multi :342-351);
* weights  ``R.weights`` of the model's row with the entries of samples that consume a 0 set to NaN; a row
           without an entry above -inf, or with +inf, has none: NaN moments, the model is flagged;
* moments  mean = Sum w A, var = Sum w (A - mean)^2, as ``R.moments`` forms them;
* average  Eb = P_lls mb_lls + Sum_n P_n mb_n and Eb2 likewise with m2, terms added in the order sub-DLA, DLA(1),
           .., DLA(md); expected = 1 - Eb, variance = max(Eb2 - Eb^2, 0); P_m == 0 skips the model, a NaN weight or a
           weight on a flagged model leaves the rows NaN.
"""
from __future__ import annotations

import numpy as np

import model_spectra_restatement as R


def slots(base, n: int, i: int):
    """The 0-based samples of the n slots of sample i, or None when one of them was never drawn."""
    out = [i]
    for j in range(2, n + 1):
        b = int(base[j - 2][i])
        if b == 0:
            return None
        out.append(b - 1)
    return out


def effective_row(ll_n, base, n: int) -> np.ndarray:
    """The model's row of log-likelihoods with a NaN where a slot of the sample was never drawn."""
    ll = np.array(ll_n, dtype=np.float64)
    for j in range(2, n + 1):
        ll[np.asarray(base[j - 2]) == 0] = np.nan
    return ll


def flagged(ll) -> bool:
    """No entry above -inf, or a +inf entry: the row has no weights."""
    ll = np.asarray(ll, dtype=np.float64)
    return bool(np.isposinf(ll).any() or not (ll[~np.isnan(ll)] > -np.inf).any())


def sample_profiles(oracle, g, offset_samples, nhi_samples, num_lines: int) -> np.ndarray:
    """[S, n_u]: the broadened profile of every sample on the grid -- what the slots gather from."""
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.asarray(offset_samples)
    return np.stack([oracle.voigt(g["pad"], z[i], nhi_samples[i], num_lines) for i in range(z.size)])


def moments_multi(oracle, g, offset_samples, nhi_samples, ll_n, base, n: int, num_lines: int, profiles=None):
    """(mean, var) of model DLA(n) over ALL samples; NaN rows for a flagged model or a quasar without a grid.
    ``profiles``: ``sample_profiles`` of the same arguments, when the caller has them already."""
    n_u = g["n_u"]
    ll = effective_row(ll_n, base, n)
    if "pad" not in g or flagged(ll):
        return np.full(n_u, np.nan), np.full(n_u, np.nan)
    w = R.weights(ll)
    C = sample_profiles(oracle, g, offset_samples, nhi_samples, num_lines) if profiles is None else profiles
    A = np.empty((w.size, n_u))
    for i in range(w.size):
        s = slots(base, n, i)
        if s is None:           # weight 0: any finite row does
            A[i] = 1.0
            continue
        A[i] = C[s[0]]
        for sj in s[1:]:
            A[i] = A[i] * C[sj]
    mean = w @ A
    return mean, w @ (A - mean) ** 2


def model_average(P, mb, m2, flags):
    """(expected, variance, undefined).  ``P``: (null, sub-DLA, DLA(1 .. md)); ``mb`` / ``m2``: [1 + md] rows of
    Sum w b and Sum w b^2 in the order sub-DLA, DLA(1), .., DLA(md); ``flags``: [1 + md] booleans."""
    P = np.asarray(P, dtype=np.float64)
    n_u = np.asarray(mb[0]).size
    undefined = bool(np.isnan(P).any() or any(P[1 + r] != 0 and flags[r] for r in range(len(flags))))
    if undefined:
        return np.full(n_u, np.nan), np.full(n_u, np.nan), True
    eb, eb2 = np.zeros(n_u), np.zeros(n_u)
    for r in range(len(flags)):
        if P[1 + r] == 0:
            continue
        eb = eb + P[1 + r] * np.asarray(mb[r])
        eb2 = eb2 + P[1 + r] * np.asarray(m2[r])
    return 1.0 - eb, np.maximum(eb2 - eb * eb, 0.0), False


def absorbed_moments(mean, var):
    """(mb, m2) of a model from its returned rows: mb = 1 - mean, m2 = var + mb^2."""
    mb = 1.0 - np.asarray(mean)
    return mb, np.asarray(var) + mb * mb
