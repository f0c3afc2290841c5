#!/usr/bin/env python3
"""Exact-arithmetic anchor where the arithmetic is hard (run in the BUILD container only): the method of
make_exact_boss.py -- the oracle with ``dump=True``, ``oracle.voigt`` absorption vectors, then ``exact_log_mvnpdf``
(50 digits) at the very fp64 inputs process_qsos.m:190-198 forms -- for every class of
tests/hard_conditioning_cases.py: the null model and ALL 65 samples of each, the sub-DLA table and both DLA models
of the multi-DLA classes, and the twelve hand-made inputs of the stand-alone low-rank function.

Writes tests/golden/exact_hard_conditioning.npz (data only): per class the spectrum, the sample table, the
interpolated model rows the exact evaluation consumed, padded wavelengths and sample redshifts, the absorption
vectors, the exact values and the oracle's values at generation time; an array a class shares with an earlier one
(the sightline and the sample table are common, so most absorption tables are) is stored once and referred to.
Prints per class cond(B) of the null model, the largest |log-likelihood| and the worst |oracle - exact|.

Usage:  python tests/golden/make_exact_hard.py [workers]        (about five CPU-minutes; default 8 workers)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from make_exact import exact_log_mvnpdf  # noqa: E402

OUT = os.path.join(HERE, "exact_hard_conditioning.npz")


def _exact(args):
    return exact_log_mvnpdf(*args)


def main(workers: int = 8):
    import multiprocessing as mp

    import hard_conditioning_cases as H
    from oracle import oracle
    prepared, jobs = [], []
    for cls in H.CLASSES:
        case = H.build_case(cls)
        run = H.run_oracle(oracle, case)
        tabs = H.absorption_tables(oracle, case, run)
        prepared.append((case, run, tabs))
        jobs.append(H.lowrank_inputs(case, run))
        for t in H.TABLES:
            if t in tabs:
                jobs += [H.lowrank_inputs(case, run, tabs[t][i]) for i in range(H.S) if np.isfinite(run[t][i])]
    lowrank = H.lowrank_cases()
    jobs += [c[2:] for c in lowrank]
    print(f"{len(jobs)} exact evaluations on {workers} workers", flush=True)
    with mp.get_context("fork").Pool(workers) as pool:
        values = iter(pool.map(_exact, jobs, chunksize=4))

    out, seen = {}, {}

    def put(name, key, a):
        a = np.asarray(a)
        tag = (a.dtype.str, a.shape, a.tobytes())
        if a.nbytes > 256 and tag in seen:
            out[f"{name}/{key}@"] = np.array(seen[tag])
        else:
            out[f"{name}/{key}"] = a
            seen[tag] = f"{name}/{key}"

    print(f"{'class':34s} {'cond(B)':>9s} {'max |ll|':>9s} {'|oracle - exact|':>17s}")
    for case, run, tabs in prepared:
        name, sp, sm = case["name"], case["spectrum"], case["samples"]
        for key in ("wavelengths", "flux", "noise_variance", "pixel_mask"):
            put(name, key, sp[key])
        put(name, "z_qso", sp["z_qso"])
        for key in ("offset_samples", "log_nhi_samples", "nhi_samples", "lls_nhi_samples"):
            put(name, key, sm[key])
        for key in ("this_mu", "this_M", "this_omega2", "padded_wavelengths", "sample_z_dlas", "min_z_dla", "max_z_dla",
                    "n_kept", "n_unmasked"):
            put(name, key, run[key])
        shift = H.shift_of(case)
        exact = {"null": next(values)}
        for t in H.TABLES:
            if t in tabs:
                put(name, f"absorption_{t}" if t != "dla2" else "base_sample_inds", tabs[t] if t != "dla2" else case["bsi"])
                exact[t] = np.array([next(values) - shift if np.isfinite(run[t][i]) else np.nan for i in range(H.S)])
        for t, v in exact.items():
            put(name, f"exact_{t}", v)
            put(name, f"oracle_{t}", run[t])
        if case["bsi"] is not None:
            for key in ("MAP_inds", "MAP_z_dlas", "MAP_log_nhis"):
                put(name, "oracle_" + key, run[key])
        cond = H.cond_B(*H.lowrank_inputs(case, run))
        put(name, "cond_B", cond)
        largest = max(abs(exact["null"]), *(float(np.nanmax(np.abs(v))) for t, v in exact.items() if t != "null"))
        print(f"{name:34s} {cond:9.2e} {largest:9.2e} {H.worst_error(run, exact):17.3e}", flush=True)
    for k, c, y, mu, M, d in lowrank:
        name = H.lowrank_name(k, c)
        for key, v in (("y", y), ("mu", mu), ("M", M), ("d", d)):
            put(name, key, v)
        lp, rc = oracle.log_mvnpdf_low_rank(y, mu, M, d)
        assert rc == 0
        ex = next(values)
        put(name, "exact_null", ex)
        put(name, "oracle_null", lp)
        put(name, "cond_B", H.cond_B(y, mu, M, d))
        print(f"{name:34s} {H.cond_B(y, mu, M, d):9.2e} {abs(ex):9.2e} {abs(lp - ex):17.3e}", flush=True)
    assert next(values, None) is None
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.basename(OUT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
