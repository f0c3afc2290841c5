#!/usr/bin/env python3
"""Exact-arithmetic anchor of the training objective where the arithmetic is hard (run in the BUILD container only).  For
every class of tests/training_hard_cases.py: objective.m:12-75 over spectrum_loss.m:14-76 (Lyman-series classes:
objective_lyseries.m over spectrum_loss_lyseries.m:22-39, with the as-written log beta expression of :90) in mpmath at 50
digits on the very fp64 inputs ``training_hard_cases.problem`` forms -- the fp64 log parameters exponentiated, and every
pow, exp and log taken, at 50 digits; only the line indicator of spectrum_loss_lyseries.m:32 is the as-written fp64
comparison -- the value f and the closed-form gradient in all G (k + 1) + 3 entries, prior terms included and stored
separately as well; rounded to fp64 only when stored.

The exact gradient is verified independently of its formula: central differences of the exact VALUE at step 1e-15 on 8
entries of M, 4 of log omega and the scalars (``training_hard_cases.fd_indices``) must agree with the closed form without
the prior terms to 1e-20 relative.  Everything here works with 20 guard digits on top of the 50 (``GUARD``): -log p is
formed as Sum y^2 w - t'z + ..., two terms of up to 1e7 |f| at S/N 1000, so that at 50 digits the quotient over 2e-15 of
two such values resolves an entry of 1e-9 (log omega in ``omega_tiny``) to 3e-20 only -- measured, and more than the
1e-20 asked for.  (Plus 1e-40 |f|, which matters only where the data's share of an entry is nothing: log tau0 with
e^-tau = 1e-2600.)  A perturbed entry of M or log omega changes one pixel's term of B_q, t_q, Sum y^2 w and Sum log d: those
values are re-factored from the updated sums; a perturbed scalar rebuilds everything.

Writes tests/golden/exact_training_hard.npz (the k = 20 classes) and exact_training_hard_k33_k40.npz (data only): per class
f, g, prior, fd_index, fd, fd_closed, cond_B of the first quasar and the SHA-256 of the inputs' bytes; the inputs
themselves are not stored.  Prints per class the oracle's per-block error against exact.

Usage:  python tests/golden/make_exact_training_hard.py [workers]        (default 8 workers)
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

LOG_2PI = 1.83787706640934534      # spectrum_loss.m:17, the fp64 number the literal parses to


def _factor(mp, B, k):
    """lower Cholesky factor of the symmetric B (lists of mpf, lower triangle used)"""
    L = [[None] * k for _ in range(k)]
    for i in range(k):
        Li = L[i]
        for j in range(i):
            Li[j] = (B[i][j] - mp.fdot(Li[:j], L[j][:j])) / L[j][j]
        s = B[i][i] - mp.fdot(Li[:i], Li[:i])
        assert s > 0
        Li[i] = mp.sqrt(s)
    return L


def _value(mp, B, t, y2w, logd, n, k):
    """spectrum_loss.m:48-52 from the quasar's sums: (-log p, L)"""
    L = _factor(mp, B, k)
    v = []
    for i in range(k):
        v.append((t[i] - mp.fdot(L[i][:i], v)) / L[i][i])
    logdet = 2 * mp.fsum(mp.log(L[i][i]) for i in range(k))
    return (y2w - mp.fdot(v, v) + logd + logdet + n * mp.mpf(LOG_2PI)) / 2, L


def exact_quasar(args):
    """One quasar at 50 + 20 digits: its -log p, its share of every gradient entry (without priors), and its share of
    f(x + h e_j) - f(x - h e_j) for the sampled entries j."""
    import mpmath as mp
    import training_hard_cases as TC
    cls, x, Frow, L1row, NVrow, fd_idx = args
    t_start = time.perf_counter()
    _, nq, G, k, lines = cls
    ok = np.flatnonzero(~np.isnan(Frow))
    n = ok.size
    if n == 0:
        return None
    with mp.workdps(TC.DPS + TC.GUARD):
        mpf = mp.mpf
        M, lo, scal = TC.split(x, G, k)
        y = [mpf(float(v)) for v in Frow[ok]]
        nv = [mpf(float(v)) for v in NVrow[ok]]
        rows = [[mpf(float(v)) for v in M[p]] for p in ok]
        log_l1 = [mp.log(mpf(float(v))) for v in L1row[ok]]
        on = [[0]] * n          # per pixel the lines that count, by the as-written fp64 comparison (:29-33)
        coef, logr = [mpf(1)], [mpf(0)]
        if lines:
            wl, fs = TC.series_tables()
            for i in range(1, lines):
                coef.append(mpf(float(wl[i])) * mpf(float(fs[i])) / (mpf(float(wl[0])) * mpf(float(fs[0]))))
                logr.append(mp.log(mpf(float(wl[0])) / mpf(float(wl[i]))))
            on = [[0] + [i for i in range(1, lines) if wl[0] * L1row[p] / wl[i] <= L1row[-1]] for p in ok]

        def pixel(pos, lo_p, c_0, tau_0, beta):
            od = tau_0 * mp.fsum(coef[i] * mp.exp(beta * (log_l1[pos] + logr[i])) for i in on[pos])
            ab = mp.exp(-od)
            sf = 1 - ab + c_0
            om = mp.exp(2 * lo_p)
            return od, ab, sf, om, om * sf * sf

        def sums(d, rows_):
            w = [1 / di for di in d]
            cols = [[r[j] for r in rows_] for j in range(k)]
            B = [[None] * k for _ in range(k)]
            for i in range(k):
                wc = [a * b for a, b in zip(w, cols[i])]
                for j in range(i + 1):
                    B[i][j] = mp.fdot(wc, cols[j])
                B[i][i] += 1
            t = [mp.fdot([a * b for a, b in zip(w, cols[i])], y) for i in range(k)]
            return B, t, mp.fdot([a * a for a in y], w), mp.fsum(mp.log(di) for di in d), w

        lo_v = [mpf(float(lo[p])) for p in ok]
        c_0, tau_0, beta = (mp.exp(mpf(float(v))) for v in scal)
        px = [pixel(pos, lo_v[pos], c_0, tau_0, beta) for pos in range(n)]
        d = [nv[pos] + px[pos][4] for pos in range(n)]
        B, t, y2w, logd, w = sums(d, rows)
        f, L = _value(mp, B, t, y2w, logd, n, k)
        # B^-1 = L^-T L^-1
        Linv = [[mpf(0)] * k for _ in range(k)]
        for c in range(k):
            for i in range(c, k):
                s = (1 if i == c else 0) - mp.fdot(L[i][c:i], [Linv[j][c] for j in range(c, i)])
                Linv[i][c] = s / L[i][i]
        LinvT = [[Linv[j][i] for j in range(k)] for i in range(k)]         # column i of L^-1
        Binv = [[mp.fdot(LinvT[i][max(i, j):], LinvT[j][max(i, j):]) for j in range(k)] for i in range(k)]
        z = [mp.fdot(Binv[i], t) for i in range(k)]
        gM, glo, gsc = [], [], [mpf(0)] * 3
        for pos in range(n):
            m = rows[pos]
            od, ab, sf, om, an = px[pos]
            wp = w[pos]
            Bm = [mp.fdot(Binv[i], m) for i in range(k)]                   # K^-1 M = D^-1 M B^-1 (:55)
            alpha = wp * (y[pos] - mp.fdot(m, z))                          # (K^-1 y)_p (:46)
            diag = wp - wp * wp * mp.fdot(m, Bm)                           # :59
            gM.append([wp * Bm[j] - alpha * z[j] for j in range(k)])       # :56
            core = alpha * alpha - diag
            glo.append(-an * core)                                         # :62
            da = om * sf * od * ab                                         # :69
            gsc = [gsc[0] - core * c_0 * om * sf, gsc[1] - core * da, gsc[2] - core * da * log_l1[pos] * beta]   # :65-74

        # central differences of the value
        h = mpf(TC.FD_STEP)
        where = {int(p): pos for pos, p in enumerate(ok)}
        fd = []
        for j in (int(v) for v in fd_idx):
            diff = []
            if j < G * (k + 1):
                p = j % G
                if p not in where:
                    fd.append(mpf(0))
                    continue
                pos = where[p]
                m = rows[pos]
                for sign in (1, -1):
                    m2, lo2 = list(m), lo_v[pos]
                    if j < G * k:
                        m2[j // G] = m2[j // G] + sign * h
                    else:
                        lo2 = lo2 + sign * h
                    d2 = nv[pos] + pixel(pos, lo2, c_0, tau_0, beta)[4]
                    w1, w2 = w[pos], 1 / d2
                    B2 = [[B[i][c] - w1 * m[i] * m[c] + w2 * m2[i] * m2[c] for c in range(i + 1)] for i in range(k)]
                    t2 = [t[i] - w1 * m[i] * y[pos] + w2 * m2[i] * y[pos] for i in range(k)]
                    diff.append(_value(mp, B2, t2, y2w + y[pos] * y[pos] * (w2 - w1), logd - mp.log(d[pos]) + mp.log(d2), n, k)[0])
            else:
                for sign in (1, -1):
                    s2 = [mpf(float(v)) for v in scal]
                    s2[j - G * (k + 1)] += sign * h
                    e = [mp.exp(v) for v in s2]
                    d2 = [nv[pos] + pixel(pos, lo_v[pos], *e)[4] for pos in range(n)]
                    diff.append(_value(mp, *sums(d2, rows)[:4], n, k)[0])
            fd.append(diff[0] - diff[1])
    return dict(ok=ok, f=f, gM=gM, glo=glo, gsc=gsc, fd=fd, seconds=time.perf_counter() - t_start)


def main(workers: int = 8, only=None):
    import multiprocessing
    import mpmath as mp
    import training_hard_cases as TC
    from oracle import oracle
    from test_training import objective_deviation
    oracle.load()
    classes = [c for c in TC.CLASSES if only is None or TC.class_name(c) in only]
    inputs = {cls: TC.problem(cls) for cls in classes}
    jobs = []
    for cls in classes:
        x, F, L1, NV = inputs[cls]
        idx = TC.fd_indices(cls)
        jobs += [(cls, q, (cls, x, F[q], L1[q], NV[q], idx)) for q in range(cls[1])]
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][0][3] ** 2 * jobs[i][0][2])
    print(f"{len(jobs)} exact per-quasar evaluations on {workers} workers", flush=True)
    t0 = time.perf_counter()
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        done = pool.map(exact_quasar, [jobs[i][2] for i in order], chunksize=1)
    results = dict(zip(((jobs[i][0], jobs[i][1]) for i in order), done))
    print(f"{time.perf_counter() - t0:.0f} s", flush=True)

    outs = {name: {} for name in TC.FIXTURES}
    mp.mp.dps = TC.DPS + TC.GUARD
    for cls in classes:
        _, nq, G, k, lines = cls
        name = TC.class_name(cls)
        x, F, L1, NV = inputs[cls]
        f, g = mp.mpf(0), [mp.mpf(0)] * (G * (k + 1) + 3)
        idx = TC.fd_indices(cls)
        fd = [mp.mpf(0)] * idx.size
        seconds = 0.0
        for q in range(nq):
            r = results[cls, q]
            if r is None:
                continue
            seconds += r["seconds"]
            f += r["f"]
            for pos, p in enumerate(r["ok"]):
                for j in range(k):
                    g[j * G + p] += r["gM"][pos][j]
                g[k * G + p] += r["glo"][pos]
            for i in range(3):
                g[(k + 1) * G + i] += r["gsc"][i]
            fd = [a + b for a, b in zip(fd, r["fd"])]
        fd = [v / (2 * mp.mpf(TC.FD_STEP)) for v in fd]
        closed = [g[int(j)] for j in idx]          # before the priors are added
        for j, a, b in zip(idx, fd, closed):
            assert abs(a - b) <= mp.mpf(TC.FD_RTOL) * abs(b) + mp.mpf(TC.FD_ATOL) * abs(f), (name, int(j), mp.nstr(a, 30), mp.nstr(b, 30))
        tau_0, beta = mp.exp(mp.mpf(float(x[-2]))), mp.exp(mp.mpf(float(x[-1])))
        prior = [tau_0 * (tau_0 - mp.mpf(0.0023)) / mp.mpf(0.0007) ** 2, beta * (beta - mp.mpf(3.65)) / mp.mpf(0.21) ** 2]
        g[-2] += prior[0]
        g[-1] += prior[1]
        to64 = lambda v: np.array([float(a) for a in v])   # noqa: E731
        out = outs[TC.fixture_of(cls)]
        f64, g64 = float(f), to64(g)
        out[f"{name}/f"] = np.array(f64)
        out[f"{name}/g"] = g64
        out[f"{name}/prior"] = to64(prior)
        out[f"{name}/fd_index"] = idx
        out[f"{name}/fd"] = to64(fd)
        out[f"{name}/fd_closed"] = to64(closed)
        out[f"{name}/cond_B"] = np.array(TC.cond_B(cls, x, F, L1, NV))
        out[f"{name}/sha256"] = np.array(TC.digest(cls, x, F, L1, NV))
        worst_fd = max((float(abs(a - b) / abs(b)) for a, b in zip(fd, closed) if b != 0), default=0.0)
        e = objective_deviation(*TC.run_oracle(oracle, cls, x, F, L1, NV), f64, g64, G, k)
        s = TC.summary(e, k)
        block = max(e, key=e.get)
        print(f"{name:36s} {seconds:5.0f} s  cond(B) {float(out[name + '/cond_B']):.1e}  |f| {abs(f64):.2e}  fd {worst_fd:.1e}  oracle: "
              f"worst {e[block]:.1e} ({block})  f {s['f']:.1e}  M {s['M']:.1e}  log_omega {s['log_omega']:.1e}  "
              f"c0 {s['log_c0']:.1e}  tau0 {s['log_tau0']:.1e}  beta {s['log_beta']:.1e}", flush=True)
    if only is None:
        for fname, out in outs.items():
            path = os.path.join(HERE, fname)
            TC.save_npz(path, out)
            print("wrote", fname, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8, set(sys.argv[2:]) or None)
