#!/usr/bin/env python3
"""Exact-arithmetic anchor of the marginal continuum, the predictive flux and the absorption moments over ALL models of a
multi-DLA run where the arithmetic is hard (run in the BUILD container only).  For every class of
tests/mixture_multi_hard_cases.py the fp64 inputs the restatement forms (``mixture_multi_hard_cases.inputs``) and the base
sample indices; the profile of sample i of model DLA(n) is the product of its n gathered ``oracle.voigt`` profiles,
multiplied in slot order in fp64.  Then in mpmath at 50 digits, AT those products: ``continuum_hard_cases.exact_sample`` once
per live (component, sample) pair and for the null model, and per (row kind, mixture) the seven marginal-continuum and five
predictive-flux products; for the two mean-flux classes also the per-model mean and variance of the absorption and their
model average on the first mixture.  Rounded to fp64 only when stored.

Writes tests/golden/exact_mixture_multi_hard.npz (data only): per class the inputs, the base indices, the weight rows, the
exact products per (row, mixture) and the exact moments per row.  An array equal to an earlier one, or to one of
exact_hard_conditioning.npz or exact_continuum_hard*.npz, is stored as a reference.  Prints per (class, row, mixture)
cond(B) of the null model and the error of both fp64 restatement forms against exact per product family.

One exact per-sample evaluation over 126 kept and 131 grid pixels takes 0.09 s at k = 20 and 0.33 s at k = 40 (measured, one
core each of 8 busy ones); the whole run, 1280 evaluations (320 per class: the null model and every drawn sample of the five
sampled components), 31 s on 8 cores.  The same arrays give the same bytes (``continuum_hard_cases.save_npz``).

Usage:  python tests/golden/make_exact_mixture_multi_hard.py [workers]        (default 8 workers)
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
    import mixture_multi_hard_cases as XH
    per_sample, combos, mu_all, M_all = args
    return [XH.exact_products(per_sample, rows, p, mu_all, M_all) for rows, p in combos]


def _moments(args):
    import mixture_multi_hard_cases as XH
    return XH.exact_moments(*args)


def main(workers: int = 8):
    import multiprocessing as mp

    import continuum_hard_cases as CH
    import hard_conditioning_cases as H
    import mixture_multi_hard_cases as XH
    from oracle import oracle
    oracle.load()
    t_start = time.perf_counter()
    golden = lambda name: np.load(os.path.join(HERE, name))      # noqa: E731
    parent = golden(H.FIXTURE)
    hard = H.load_fixture(golden)
    continuum = CH.load_fixture(golden)
    prepared, jobs = [], []
    for cls in XH.CLASSES:
        case = H.build_case(cls)
        bsi = XH.base_sample_inds(cls[0], case["samples"])
        inp = XH.inputs(oracle, case)
        full = XH.with_products(inp, bsi)
        rows = XH.weight_rows(hard[case["name"]], case["samples"]["offset_samples"])
        flat = XH.effective_rows({c: rows[c]["flat"] for c in XH.SAMPLED}, bsi)
        pairs = XH.live_pairs(flat, np.ones(len(XH.COMPONENTS)))            # the flat row reaches every drawn sample
        args = (CH.rows_of(inp), inp["mu_all"], inp["M_all"])
        jobs.append(args + (np.ones(inp["kept"].size), inp["kept"]))
        jobs += [args + (full["profiles_" + c][i], inp["kept"]) for c, i in pairs]
        prepared.append((case, bsi, inp, full, rows, pairs))
    print(f"{len(jobs)} exact per-sample evaluations on {workers} workers", flush=True)
    with mp.get_context("fork").Pool(workers) as pool:
        values = iter(pool.map(_sample, jobs, chunksize=1))
        combos_jobs, moment_jobs, layout = [], [], []
        for case, bsi, inp, full, rows, pairs in prepared:
            null, cost = next(values)
            per_sample, costs = {"null": [null], **{c: {} for c in XH.SAMPLED}}, [cost]
            for c, i in pairs:
                per_sample[c][i], cost = next(values)
                costs.append(cost)
            eff = {row: XH.effective_rows({c: rows[c][row] for c in XH.SAMPLED}, bsi) for row in XH.ROWS}
            combos_jobs.append((per_sample, [(eff[row], XH.MIXTURES[m]) for row, m in XH.COMBOS], inp["mu_all"], inp["M_all"]))
            if case["cls"] in XH.MOMENT_CLASSES:
                moment_jobs += [(full, eff[row], XH.MIXTURES[0]) for row in XH.MOMENT_ROWS]
            layout.append((case, bsi, inp, full, rows, eff, float(np.mean(costs))))
        assert next(values, None) is None
        exact_all = pool.map(_products, combos_jobs, chunksize=1)
        moments_all = iter(pool.map(_moments, moment_jobs, chunksize=1))

    out, seen = {}, {}
    for full_key in parent.files:
        a = parent[full_key]
        if not full_key.endswith("@") and a.nbytes > 256:
            seen.setdefault((a.dtype.str, a.shape, a.tobytes()), CH.PARENT + full_key)
    for name in sorted(continuum):
        for key in sorted(continuum[name]):
            a = np.asarray(continuum[name][key])
            if a.nbytes > 256:
                seen.setdefault((a.dtype.str, a.shape, a.tobytes()), f"{XH.CONTINUUM}{name}/{key}")

    def put(name, key, a):
        a = np.asarray(a)
        tag = (a.dtype.str, a.shape, a.tobytes())
        where = seen.get(tag)
        if a.nbytes > 256 and where is not None:
            out[f"{name}/{key}@"] = np.array(where)
        else:
            out[f"{name}/{key}"] = a
            if a.nbytes > 256:
                seen[tag] = f"{name}/{key}"

    print(f"{'class row mixture':80s} {'cond(B)':>8s}   " + "  ".join(f"{f + ' W/D':>19s}" for f in CH.FAMILIES) + "   rel W/D")
    for (case, bsi, inp, full, rows, eff, cost), exacts in zip(layout, exact_all):
        cls, name = case["cls"], case["name"]
        for key in XH.INPUT_KEYS:
            put(name, key, inp[key])
        put(name, "base_sample_inds", bsi)
        for c in XH.SAMPLED:
            for row in XH.ROWS:
                put(name, f"row/{c}/{row}", rows[c][row])
        cond = H.cond_B(inp["y"], inp["mu"], inp["M"], inp["omega2"] + inp["nu"])
        put(name, "cond_B", cond)
        fp64 = {form: XH.restatement_samples(full, form) for form in ("woodbury", "dense")}
        print(f"{name}: {cost:.2f} s per exact evaluation")
        for (row, m), exact in zip(XH.COMBOS, exacts):
            for product, v in exact.items():
                put(name, f"exact/{row}/{m}/{product}", v)
            r = {form: XH.restatement_products(full, fp64[form], eff[row], XH.MIXTURES[m]) for form in fp64}
            fam = {form: {f: max(CH.error(r[form][n], exact[n]) for n in names if n in exact) for f, names in CH.FAMILIES.items()}
                   for form in fp64}
            rel = {form: max(CH.rel_error(r[form][n], exact[n]) for n in CH.REL_PRODUCTS) for form in fp64}
            print(f"{name + ' ' + row + ' ' + str(XH.MIXTURES[m]):80s} {cond:8.1e}   "
                  + "  ".join(f"{fam['woodbury'][f]:9.2e}/{fam['dense'][f]:9.2e}" for f in CH.FAMILIES)
                  + f"   {rel['woodbury']:.1e}/{rel['dense']:.1e}", flush=True)
        if cls in XH.MOMENT_CLASSES:
            for row in XH.MOMENT_ROWS:
                exact = next(moments_all)
                for product, v in exact.items():
                    put(name, f"moments/{row}/{product}", v)
                rest = XH.restatement_moments(full, eff[row], XH.MIXTURES[0])
                print(f"{name} {row} moments: restatement error {max(CH.error(rest[n], exact[n]) for n in XH.MOMENTS):.2e}")
    assert next(moments_all, None) is None
    path = os.path.join(HERE, XH.FIXTURE)
    CH.save_npz(path, out)
    print("wrote", XH.FIXTURE, os.path.getsize(path), "bytes;", f"{time.perf_counter() - t_start:.0f} s")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
