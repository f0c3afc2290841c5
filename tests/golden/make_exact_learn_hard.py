#!/usr/bin/env python3
"""Exact-arithmetic anchor of the learning front end where the arithmetic is hard.  For every class of
tests/learn_hard_cases.py: learn_qso_model.m:37-87 (mean-flux legs: learn_qso_model_meanflux.m:43-157) up to the matrix pca
decomposes, in mpmath at 50 digits (+ 10 guard digits) on the very float64 inputs ``learn_hard_cases.problem`` forms:
interp1 of flux, noise variance and 1 + z, the noise mask, the 31-line optical depth and the division by e^-tau and its
square, nanmean, the centring, nanstd (n - 1), the pairwise second moment over N_ab - 1 and the complete-rows covariance;
rounded to float64 only when stored.

Which float64 intermediates the yardstick keeps, because the contract fixes them as data:

    rest = lambda / (1 + z)     rounded once, with 1 + z rounded: the reference stores the emitted wavelengths as a float64
                                array before interp1 sees them, and the bracket search compares those numbers.  Between
                                rounded neighbours x1 - x0 is exact in float64, so under this reading tight pixel pairs
                                cost no digits; under the other (t from unrounded wavelengths) they cost 1e-16 / spacing,
                                which test_learn_hard.py uses as a deliberately worse variant.
    xq = min_lambda + p dlambda rounded (exact on the reference's grid, rounded for a non-dyadic one): the query points are
                                data too.
    tau0_j                      prev_tau_0 f_j / f_lya lambda_j / lambda_lya in that order, in float64: a table entry.
    line indicators             the as-written float64 comparison 1 + z_j <= 1 + z_qso (v0 + t (v1 - v0) with
                                v = 1 + (lambda - lambda_j) / lambda_j, two roundings); where the 50-digit comparison
                                says otherwise the pixel is recorded in ``excluded`` (learn_hard_cases docstring).

Everything else is exact: t, 1 + z_j = lambda / lambda_j interpolated, pow, exp, the sums.  The bound rule (10 x the
restatement's own error, floored) absorbs either reading, since the restatement takes the same one.

Writes tests/golden/exact_learn_hard.npz (single-DLA legs) and exact_learn_hard_meanflux.npz (data only): per class the
eight blocks, count, N_pairwise, rows_complete, excluded and the SHA-256 of the inputs' bytes; the inputs themselves are
not stored.  Prints per class the restatement's per-block error against exact.

Usage:  python tests/golden/make_exact_learn_hard.py [workers]        (default 8 workers)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

GUARD = 10
LYA_OSCILLATOR_STRENGTH = 0.416400  # set_parameters_multi.m:144


def exact_quasar(mp, wl, fl, nv, mk, z, p, G, lines):
    """One quasar's rows of rest flux, lya_1pzs and rest noise (mpf or None = NaN) and its excluded pixels"""
    mpf = mp.mpf
    n = wl.size
    F, L, N, excl = [None] * G, [None] * G, [None] * G, np.zeros(G, bool)
    if n < 2:
        return F, L, N, excl
    opz = 1.0 + z
    x = wl / opz
    xq = p.min_lambda + np.arange(G) * p.dlambda
    lya, cut = mpf(p.lya_wavelength), mpf(p.max_noise_variance)
    for g in range(G):
        if not (x[0] <= xq[g] <= x[-1]):
            continue
        j = min(max(int(np.searchsorted(x, xq[g], side="right")) - 1, 0), n - 2)
        t = (mpf(xq[g]) - mpf(x[j])) / (mpf(x[j + 1]) - mpf(x[j]))
        nan = bool(mk[j]) or bool(mk[j + 1])
        f = None if nan or np.isnan(fl[j]) or np.isnan(fl[j + 1]) else mpf(fl[j]) + t * (mpf(fl[j + 1]) - mpf(fl[j]))
        v = None if nan or np.isnan(nv[j]) or np.isnan(nv[j + 1]) else mpf(nv[j]) + t * (mpf(nv[j + 1]) - mpf(nv[j]))
        w0, w1 = mpf(wl[j]), mpf(wl[j + 1])
        obs = w0 + t * (w1 - w0)
        if v is not None and v > cut:
            continue
        if lines and (f is not None or v is not None):
            t64 = (xq[g] - x[j]) / (x[j + 1] - x[j])
            tau = mpf(0)
            for i, (lj, tau0) in enumerate(lines):
                v0, v1 = 1.0 + (wl[j] - lj) / lj, 1.0 + (wl[j + 1] - lj) / lj
                counted = i == 0 or bool(v0 + t64 * (v1 - v0) <= opz)
                zj = obs / mpf(lj)
                if i > 0 and counted != bool(zj <= mpf(opz)):
                    excl[g] = True
                if counted:
                    tau += mpf(tau0) * mp.exp(mpf(p.prev_beta) * mp.log(zj))
            f, v = (None if f is None else f * mp.exp(tau)), (None if v is None else v * mp.exp(2 * tau))
        F[g], L[g], N[g] = f, obs / lya, v
    return F, L, N, excl


def _quotient(P, N):
    """P / (N - 1) in float64 as IEEE has it at N = 1 (+-inf, 0 / 0 = NaN) and N = 0 (-0)"""
    if N == 1:
        return float("nan") if P == 0 else (float("inf") if P > 0 else float("-inf"))
    return float(P / (N - 1))


def exact_class(cls):
    """{key: array} of one class"""
    import mpmath as mp
    import learn_hard_cases as LC
    csr, p = LC.problem(cls)
    G = LC.grid_size(p)
    lines = None
    if cls[1]:
        wl_a = LC.line_wavelengths()
        lines = [(float(wl_a[i]), p.prev_tau_0 * LC.LINES[i][1] / LYA_OSCILLATOR_STRENGTH * float(wl_a[i]) / p.lya_wavelength)
                 for i in range(p.num_forest_lines)]
    off = csr["offsets"]
    nq = off.size - 1
    with mp.workdps(LC.DPS + GUARD):
        mpf = mp.mpf
        rows = [exact_quasar(mp, *(csr[k][off[q]:off[q + 1]] for k in ("wavelengths", "flux", "noise_variance", "pixel_mask")),
                             float(csr["z_qsos"][q]), p, G, lines) for q in range(nq)]
        F = [r[0] for r in rows]
        to64 = lambda M: np.array([[np.nan if v is None else float(v) for v in row] for row in M]).reshape(len(M), -1)  # noqa: E731
        col = [[q for q in range(nq) if F[q][g] is not None] for g in range(G)]
        mu = [mp.fsum(F[q][g] for q in col[g]) / len(col[g]) if col[g] else None for g in range(G)]
        C = [[None if F[q][g] is None else F[q][g] - mu[g] for g in range(G)] for q in range(nq)]
        std = []
        for g in range(G):
            c = len(col[g])
            std.append(None if c == 0 else mpf(0) if c == 1 else mp.sqrt(mp.fsum(C[q][g] ** 2 for q in col[g]) / (c - 1)))
        cov_p, N_p = np.empty((G, G)), np.empty((G, G))
        sets = [set(c) for c in col]
        for a in range(G):
            for b in range(a + 1):
                both = sorted(sets[a] & sets[b])
                cov_p[a, b] = cov_p[b, a] = _quotient(mp.fsum(C[q][a] * C[q][b] for q in both), len(both))
                N_p[a, b] = N_p[b, a] = len(both)
        complete = [q for q in range(nq) if all(v is not None for v in F[q])]
        nc = len(complete)
        mean_c = [mp.fsum(F[q][g] for q in complete) / nc for g in range(G)] if nc else [mpf(0)] * G
        X = [[F[q][g] - mean_c[g] for g in range(G)] for q in complete]
        cov_c = np.empty((G, G))
        for a in range(G):
            for b in range(a + 1):
                cov_c[a, b] = cov_c[b, a] = _quotient(mp.fsum(r[a] * r[b] for r in X), nc)
        vec = lambda v: np.array([np.nan if a is None else float(a) for a in v])  # noqa: E731
        out = dict(rest_flux=to64(F), lya_1pzs=to64([r[1] for r in rows]), rest_noise=to64([r[2] for r in rows]), mu=vec(mu),
                   centered=to64(C), std=vec(std), cov_pairwise=cov_p, cov_complete=cov_c,
                   count=np.array([len(c) for c in col], dtype=np.int64), N_pairwise=N_p, rows_complete=np.array(nc),
                   excluded=np.array([r[3] for r in rows]).reshape(nq, G), sha256=np.array(LC.digest(cls, csr, p)))
    return out


def main(workers: int = 8, only=None):
    import multiprocessing
    import learn_hard_cases as LC
    classes = [c for c in LC.CLASSES if only is None or LC.class_name(c) in only]
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        done = pool.map(exact_class, classes, chunksize=1)
    outs = {name: {} for name in LC.FIXTURES}
    for cls, exact in zip(classes, done):
        name = LC.class_name(cls)
        for key in LC.KEYS:
            outs[LC.fixture_of(cls)][f"{name}/{key}"] = exact[key]
        csr, p = LC.problem(cls)
        got = LC.restated(cls, csr, p)
        e = LC.deviation(got, exact)
        fin = np.isfinite(exact["rest_flux"])
        print(f"{name:32s} nq {csr['z_qsos'].size:3d}  finite {int(fin.sum()):5d}  excluded {int(exact['excluded'].sum()):3d}  "
              f"patterns {LC.patterns(got, exact) or 'equal'}  restatement: " + "  ".join(f"{b} {e[b]:.1e}" for b in LC.BLOCKS),
              flush=True)
    if only is None:
        for fname, out in outs.items():
            path = os.path.join(HERE, fname)
            LC.save_npz(path, out)
            print("wrote", fname, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8, set(sys.argv[2:]) or None)
