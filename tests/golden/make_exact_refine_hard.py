#!/usr/bin/env python3
"""Exact-arithmetic anchor of the refine pass and of the batch conditioned on fixed absorbers where the arithmetic is
hard (run in the BUILD container only): the method of make_exact_hard.py -- ``oracle.voigt`` absorption vectors, then
``exact_log_mvnpdf`` (50 digits) at the very fp64 inputs the sweep is defined on -- for the classes of
tests/refine_hard_cases.py.

Refine: level 1's box comes from the exact first-pass table stored in exact_hard_conditioning.npz (rounded to fp64),
by refine_restatement.level_box; z', n' in fp64 as the contract writes them; N' = 10.0**n' on the host; the exact l'
of all 65 points; lambda = exact l' + log p_N (uniform prior) is the source of the next box.  The oracle's value is
``oracle.log_mvnpdf_low_rank`` on the very same (y, mu, M, d).  log Z_ref of a call with 1, 2 and 3 levels is summed in
50 digits from the exact tables and the contract's (max, scaled sum) pieces.

Conditioned: A = the product in list order of ``oracle.voigt`` over the fixed absorbers; the null model
(y, mu A, M A, omega2 A^2 + nu) and every sample outside the separation (conditional_restatement.mask).

Writes tests/golden/exact_refine_hard.npz (data only; absorption tables are not stored).  Prints per class cond(B),
the largest |log-likelihood| and the worst |oracle - exact|, and asserts the conditions refine_hard_cases.py states:
the margins at every level and the oracle cap on every value.

Usage:  python tests/golden/make_exact_refine_hard.py [workers]      (a minute and a half on 8 workers, the default)
"""
from __future__ import annotations

import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from make_exact import exact_log_mvnpdf  # noqa: E402  (sets 50 digits)

OUT = os.path.join(HERE, "exact_refine_hard.npz")


def _exact(args):
    return exact_log_mvnpdf(*args)


def exact_log_z(pieces) -> float:
    """log Sum_t f_t Sum_x exp(x) over ``pieces`` = [(factor f_t, list of exponents)], in 50 digits"""
    M = max(max(xs) for _, xs in pieces if len(xs))
    tot = mp.mpf(0)
    for f, xs in pieces:
        tot += mp.mpf(f) * mp.fsum(mp.exp(x - M) for x in xs)
    return float(M + mp.log(tot))


def main(workers: int = 8):
    import multiprocessing as mproc

    import hard_conditioning_cases as H
    import refine_hard_cases as RH
    import refine_restatement as RR
    from oracle import oracle
    first_fixture = H.load_fixture(lambda name: np.load(os.path.join(HERE, name)))
    out, problems = {}, []

    classes = list(dict.fromkeys(RH.REFINE_CLASSES + RH.COND_CLASSES))
    prepared = {}
    for cls in classes:
        case = H.build_case(cls)
        prepared[cls] = (case, H.run_oracle(oracle, case))

    with mproc.get_context("fork").Pool(workers) as pool:
        # ------------------------------------------------------------ conditioned (submitted first, collected last)
        cond_jobs, cond_meta = [], []
        for cls in RH.COND_CLASSES:
            case, run = prepared[cls]
            lines = case["params"].num_lines
            tabs = H.absorption_tables(oracle, case, run)["dla"]
            for which, fixed in RH.fixed_lists(run).items():
                A = RH.fixed_absorption(run, fixed, lines)
                close = RH.CR.close(run["sample_z_dlas"], fixed, RH.SEPARATION)
                inputs = [RH.conditioned_inputs(case, run, A)] + [RH.conditioned_inputs(case, run, A, tabs[i])
                                                                  for i in range(H.S) if not close[i]]
                cond_meta.append((cls, which, fixed, A, close, inputs, len(cond_jobs)))
                cond_jobs += inputs
        cond_async = pool.map_async(_exact, cond_jobs, chunksize=4)
        print(f"{len(cond_jobs)} conditioned and {len(RH.REFINE_CLASSES) * RH.LEVELS * RH.SR} refined exact evaluations "
              f"on {workers} workers", flush=True)

        # ------------------------------------------------------------ refine, level by level over all classes
        state = {}
        for cls in RH.REFINE_CLASSES:
            e = first_fixture[H.class_name(cls)]
            first_index, delta = RH.tuning(cls)
            z0, n0 = RH.first_pass_coordinates(e)
            N_lo, N_hi = RH.n_range(n0)
            min_z, max_z = float(e["min_z_dla"]), float(e["max_z_dla"])
            state[cls] = dict(src=np.asarray(e["exact_dla"], dtype=np.float64), src_z=z0, src_n=n0, parent=(min_z, max_z, N_lo, N_hi),
                              sqrt_s=np.sqrt(H.S), uv=RH.points(first_index), delta=delta, pieces=[], factor=mp.mpf(1) / H.S,
                              boxes=[], z=[], n=[], exact_ell=[], oracle_ell=[], exact_lam=[], cut_margin=[], edge_margin=[],
                              log_z=[], map_ind=[], gap=[], log_prior=mp.mpf(-1) * mp.log(mp.mpf(N_hi - N_lo)),
                              range=(min_z, max_z))
        for lev in range(RH.LEVELS):
            jobs, spans = [], {}
            for cls in RH.REFINE_CLASSES:
                case, run = prepared[cls]
                st = state[cls]
                box, mx, outside = RR.level_box(st["src"], st["src_z"], st["src_n"], st["parent"], st["delta"], RH.PAD, st["sqrt_s"])
                cm, em = RH.box_margins(st["src"], st["src_z"], st["src_n"], st["parent"], box, st["delta"])
                st["cut_margin"].append(cm)
                st["edge_margin"].append(em)
                st["pieces"].append((st["factor"], [st["src_exact"][i] if lev else mp.mpf(float(st["src"][i]))
                                                    for i in np.flatnonzero(outside)]))
                z, n = RH.refined_coordinates(box, *st["uv"])
                inputs = [H.lowrank_inputs(case, run, a) for a in RH.refined_absorption(oracle, run, z, n, case["params"].num_lines)]
                st["oracle_ell"].append(RH.oracle_values(oracle, inputs))
                st["boxes"].append(box)
                st["z"].append(z)
                st["n"].append(n)
                spans[cls] = (len(jobs), len(jobs) + len(inputs))
                jobs += inputs
            values = pool.map(_exact, jobs, chunksize=2)
            for cls in RH.REFINE_CLASSES:
                st = state[cls]
                ell = np.array(values[slice(*spans[cls])])
                lam_exact = [mp.mpf(float(x)) + st["log_prior"] for x in ell]
                lam = np.array([float(x) for x in lam_exact])
                box = st["boxes"][-1]
                min_z, max_z = st["range"]
                V = 1.0 if max_z == min_z else (box[1] - box[0]) / (max_z - min_z)
                st["factor"] = mp.mpf(V * (box[3] - box[2])) / RH.SR
                st["log_z"].append(exact_log_z(st["pieces"] + [(st["factor"], lam_exact)]))
                order = np.argsort(lam)
                st["map_ind"].append(int(order[-1]) + 1)
                st["gap"].append(float(lam_exact[order[-1]] - lam_exact[order[-2]]))
                st["exact_ell"].append(ell)
                st["exact_lam"].append(lam)
                st.update(src=lam, src_exact=lam_exact, src_z=st["z"][-1], src_n=st["n"][-1], parent=box, sqrt_s=np.sqrt(RH.SR))
            print(f"level {lev + 1} done", flush=True)
        cond_values = cond_async.get()

    print(f"{'class':44s} {'cond(B)':>9s} {'max |ll|':>9s} {'|oracle - exact|':>17s}")
    for cls in RH.REFINE_CLASSES:
        st, name = state[cls], RH.refine_name(cls)
        case, run = prepared[cls]
        first_index, delta = RH.tuning(cls)
        for key in ("boxes", "z", "n", "exact_ell", "oracle_ell", "exact_lam", "cut_margin", "edge_margin", "log_z", "map_ind", "gap"):
            out[f"{name}/{key}"] = np.array(st[key])
        out[f"{name}/first_index"], out[f"{name}/delta"] = np.array(first_index), np.array(delta)
        out[f"{name}/cond_B"] = np.array(H.cond_B(*H.lowrank_inputs(case, run)))
        for lev in range(RH.LEVELS):
            err = RH.table_error(st["oracle_ell"][lev], st["exact_ell"][lev])
            print(f"{name + ' level ' + str(lev + 1):44s} {float(out[name + '/cond_B']):9.2e} {np.abs(st['exact_ell'][lev]).max():9.2e} "
                  f"{err:17.3e}   cut margin {st['cut_margin'][lev]:.3g} edge margin {st['edge_margin'][lev]:.3g} "
                  f"top-two gap {st['gap'][lev]:.3g} MAP {st['map_ind'][lev]} log Z_ref {st['log_z'][lev]:.6f}", flush=True)
            if not err <= H.ORACLE_CAP:
                problems.append(f"{name} level {lev + 1}: oracle error {err:.3e} over the cap")
            if not (st["cut_margin"][lev] > RH.MARGIN and st["edge_margin"][lev] > RH.EDGE_REL):
                problems.append(f"{name} level {lev + 1}: margins {st['cut_margin'][lev]:.3g}, {st['edge_margin'][lev]:.3g}")

    for cls, which, fixed, A, close, inputs, at in cond_meta:
        name = RH.cond_name(cls, which)
        case, run = prepared[cls]
        kept = ~case["spectrum"]["pixel_mask"].astype(bool)[H.in_range(case["spectrum"])]
        exact = np.full(H.S, -np.inf)
        orc = np.full(H.S, -np.inf)
        exact[~close] = cond_values[at + 1:at + len(inputs)]
        orc[~close] = RH.oracle_values(oracle, inputs[1:])
        exact_null, oracle_null = cond_values[at], float(RH.oracle_values(oracle, inputs[:1])[0])
        assert np.array_equal(np.isneginf(RH.CR.mask(orc, run["sample_z_dlas"], fixed, RH.SEPARATION)), close)
        out[f"{name}/fixed"] = np.array(fixed, dtype=np.float64)
        out[f"{name}/exact_null"], out[f"{name}/oracle_null"] = np.array(exact_null), np.array(oracle_null)
        out[f"{name}/exact_dla"], out[f"{name}/oracle_dla"] = exact, orc
        out[f"{name}/cond_B"] = np.array(H.cond_B(*inputs[0]))
        out[f"{name}/trough"] = np.array(A[kept].min())
        err = max(RH.table_error(orc, exact), abs(oracle_null - exact_null))
        largest = max(abs(exact_null), float(np.abs(exact[~close]).max()))
        print(f"{name:44s} {float(out[name + '/cond_B']):9.2e} {largest:9.2e} {err:17.3e}   {int((~close).sum())} finite, "
              f"deepest A on kept pixels {A[kept].min():.2e}, top-two gap {H.closest_top_two(exact):.3g}", flush=True)
        if not err <= H.ORACLE_CAP:
            problems.append(f"{name}: oracle error {err:.3e} over the cap")
        if not (RH.MIN_FINITE <= (~close).sum() < H.S):
            problems.append(f"{name}: {int((~close).sum())} samples outside the separation")
        if which == "three" and not A[kept].min() < 1e-25:
            problems.append(f"{name}: the log N = 23 trough is not on kept pixels")
    np.savez_compressed(OUT, **out)
    print("wrote", os.path.basename(OUT), os.path.getsize(OUT), "bytes")
    assert not problems, problems


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
