#!/usr/bin/env python3
"""Exact-arithmetic anchor of the marginal continuum and the posterior predictive flux where the arithmetic is hard (run
in the BUILD container only).  For every class of tests/hard_conditioning_cases.py the fp64 inputs the restatement forms
(``continuum_hard_cases.inputs``), then in mpmath at 50 digits: per sample of every table B_i, Sigma_i = B_i^-1,
c_i = Sigma_i M'(a (y - a mu) / d) and, on the whole grid, t = mu + m'c and s = m' Sigma m -- once per (class, table,
sample), shared by all rows -- the null component, and per weight row and mixture the seven marginal-continuum and five
predictive-flux products; rounded to fp64 only when stored.

Writes tests/golden/exact_continuum_hard.npz (the k = 20 classes) and exact_continuum_hard_k33_k40.npz (data only): per
class the inputs, the weight rows, the exact products per (row, mixture), the exact per-sample continua of three samples
of ``top8_flat`` and, where a mixture asks for them, the exact c_i of all samples.  An array equal to an earlier one, or to
one of exact_hard_conditioning.npz, is stored as a reference.  Prints per (class, row, mixture) cond(B) of the null
model, n_eff, max |V| and the error of both fp64 restatement forms against exact per product family.

One exact per-sample evaluation over 126 kept and 131 grid pixels takes 0.27 s at k = 20, 0.72 s at k = 33 and 1.2 s at
k = 40 (measured, one core each of 8 busy ones); the whole run, 988 evaluations, 72 s on 8 cores.

Usage:  python tests/golden/make_exact_continuum_hard.py [workers]        (default 8 workers)
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]


def _sample(args):
    import continuum_hard_cases as CH
    t0 = time.perf_counter()
    r = CH.exact_sample(*args)
    return r, time.perf_counter() - t0


def _products(args):
    import continuum_hard_cases as CH
    per_sample, combos, mu_all, M_all = args
    return [CH.exact_products(per_sample, rows, p, mu_all, M_all) for rows, p in combos]


def main(workers: int = 8):
    import multiprocessing as mp

    import continuum_hard_cases as CH
    import hard_conditioning_cases as H
    from oracle import oracle
    oracle.load()
    parent = np.load(os.path.join(HERE, H.FIXTURE))
    hard = H.load_fixture(lambda name: parent)
    prepared, jobs = [], []
    for cls in H.CLASSES:
        case = H.build_case(cls)
        inp = CH.inputs(oracle, case)
        rows = CH.rows_of(inp)
        ones = np.ones(inp["kept"].size)
        jobs.append((rows, inp["mu_all"], inp["M_all"], ones, inp["kept"]))
        for t in CH.tables_of(cls):
            jobs += [(rows, inp["mu_all"], inp["M_all"], a, inp["kept"]) for a in inp["profiles_" + t]]
        prepared.append((case, inp))
    print(f"{len(jobs)} exact per-sample evaluations on {workers} workers", flush=True)
    with mp.get_context("fork").Pool(workers) as pool:
        done = pool.map(_sample, jobs, chunksize=1)
        values = iter(done)
        combos_jobs, layout = [], []
        for case, inp in prepared:
            cls = case["cls"]
            per_sample = {"null": [next(values)]}
            for t in CH.tables_of(cls):
                per_sample[t] = [next(values) for _ in range(H.S)]
            cost = float(np.mean([dt for group in per_sample.values() for _, dt in group]))
            per_sample = {t: [r for r, _ in group] for t, group in per_sample.items()}
            e = hard[case["name"]]
            rows = {t: CH.weight_rows(e[CH.EXACT_TABLE[t]], case["samples"]["offset_samples"]) for t in CH.tables_of(cls)}
            combos = [(row, m) for row in CH.ROWS for m in range(len(CH.mixtures_of(cls)))]
            combos_jobs.append((per_sample, [({t: rows[t][row] for t in rows}, CH.mixtures_of(cls)[m][0]) for row, m in combos],
                                inp["mu_all"], inp["M_all"]))
            layout.append((case, inp, per_sample, rows, combos, cost))
        assert next(values, None) is None
        exact_all = pool.map(_products, combos_jobs, chunksize=1)

    outs, seen = {name: {} for name in CH.FIXTURES}, {}
    for full in parent.files:
        a = parent[full]
        if not full.endswith("@") and a.nbytes > 256:
            seen.setdefault((a.dtype.str, a.shape, a.tobytes()), CH.PARENT + full)

    def put(out, name, key, a):
        a = np.asarray(a)
        tag = (a.dtype.str, a.shape, a.tobytes())
        where = seen.get(tag)
        if a.nbytes > 256 and where is not None and (where.startswith(CH.PARENT) or where in out):
            out[f"{name}/{key}@"] = np.array(where)
        else:
            out[f"{name}/{key}"] = a
            if a.nbytes > 256 and where is None:
                seen[tag] = f"{name}/{key}"

    print(f"{'class row mixture':52s} {'cond(B)':>8s} {'n_eff':>6s} {'max|V|':>8s}   "
          + "  ".join(f"{f + ' W/D':>19s}" for f in CH.FAMILIES) + "   rel W/D")
    for (case, inp, per_sample, rows, combos, cost), exacts in zip(layout, exact_all):
        cls, name = case["cls"], case["name"]
        out = outs[CH.fixture_of(cls)]
        for key in CH.INPUT_KEYS:
            put(out, name, key, inp[key])
        for t in CH.tables_of(cls):
            put(out, name, "profiles_" + t, inp["profiles_" + t])
            for row in CH.ROWS:
                put(out, name, f"row/{t}/{row}", rows[t][row])
        cond = H.cond_B(inp["y"], inp["mu"], inp["M"], inp["omega2"] + inp["nu"])
        put(out, name, "cond_B", cond)
        three = CH.spectra_samples(rows["dla"]["top8_flat"], case["samples"]["offset_samples"])
        put(out, name, "spectra_samples", three)
        put(out, name, "exact_spectra_continuum", np.array([[float(x) for x in per_sample["dla"][int(i)]["t"]] for i in three]))
        if any(sc for _, sc in CH.mixtures_of(cls)):
            put(out, name, "exact_sample_coefficients", CH.exact_rows(dict(enumerate(per_sample["dla"])), H.S))
        fp64 = {form: CH.restatement_samples(inp, CH.tables_of(cls), form) for form in ("woodbury", "dense")}
        print(f"{name}: {cost:.2f} s per exact evaluation")
        for (row, m), exact in zip(combos, exacts):
            p, sc = CH.mixtures_of(cls)[m]
            for product, v in exact.items():
                put(out, name, f"exact/{row}/{m}/{product}", v)
            exact = dict(exact)
            if sc:
                exact["sample_coefficients"] = CH.live_rows(out[f"{name}/exact_sample_coefficients"], rows["dla"][row])
            r = {form: CH.restatement_products(inp, fp64[form], {t: rows[t][row] for t in rows}, p, sc) for form in fp64}
            fam = {form: {f: max(CH.error(r[form][n], exact[n]) for n in names if n in exact) for f, names in CH.FAMILIES.items()}
                   for form in fp64}
            rel = {form: max(CH.rel_error(r[form][n], exact[n]) for n in CH.REL_PRODUCTS) for form in fp64}
            print(f"{name + ' ' + row + ' ' + str(p):52s} {cond:8.1e} {CH.n_eff(rows['dla'][row]):6.3f} "
                  f"{np.abs(exact['coef_cov_between']).max():8.1e}   "
                  + "  ".join(f"{fam['woodbury'][f]:9.2e}/{fam['dense'][f]:9.2e}" for f in CH.FAMILIES)
                  + f"   {rel['woodbury']:.1e}/{rel['dense']:.1e}", flush=True)
    for fname, out in outs.items():
        path = os.path.join(HERE, fname)
        CH.save_npz(path, out)
        print("wrote", fname, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
