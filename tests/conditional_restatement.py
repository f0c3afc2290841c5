"""NumPy restatement of the batch conditioned on fixed absorbers (the contract is the comment
in include/gpdla.h): the absorption A of the fixed absorbers from the oracle's voigt, the conditioned rows, the
separation rule, the two CPU routes to the conditional table, and the orchestration of
gp_dla_detection_amd/conditional.py around tests/refine_restatement.refine_row.

Two routes give the conditional table l(z, N | fixed) on the CPU:

 * :func:`multi_table` -- the identity the feature rests on.  The oracle's multi-DLA driver with the fixed
   absorbers appended as extra samples and ``base_sample_inds`` rows held constant at them: column F of its sample
   table is the (F + 1)-DLA likelihood with F absorbers fixed, on the rows of the multi-DLA driver (meanflux rows).
 * :func:`dense_table` -- the rows of ``oracle.process_spectrum(dump=True)`` (process_qsos.m's) times A, then
   ``oracle.log_mvnpdf_low_rank`` per sample: what single-DLA rows need.
"""
import math

import numpy as np

import refine_restatement as RR

NEG_INF = -np.inf


def absorption(padded_wavelengths, fixed, num_lines):
    """A on the unmasked-range grid: the product, in list order, of the instrument-broadened profiles."""
    from oracle import oracle
    A = np.ones(len(padded_wavelengths) - 6)
    for j, (z, ln) in enumerate(fixed):
        prof = oracle.voigt(padded_wavelengths, z, 10.0 ** ln, num_lines)
        A = prof if j == 0 else A * prof
    return A


def conditioned_rows(rows, M, A):
    """(rows [n, 4] as (y, mu, omega2, nu), M [n, k]) with one multiplication each, in the contract's order."""
    out = np.array(rows, dtype=np.float64)
    out[:, 1] = out[:, 1] * A
    out[:, 2] = out[:, 2] * (A * A)
    return out, np.asarray(M, dtype=np.float64) * A[:, None]


def close(z, fixed, sep):
    """The separation rule: True where z lies strictly closer than ``sep`` to a fixed redshift."""
    z = np.asarray(z, dtype=np.float64)
    out = np.zeros(z.shape, dtype=bool)
    for zf, _ in fixed:
        out |= (np.maximum(z, zf) - np.minimum(z, zf)) < sep
    return out


def mask(l, z, fixed, sep):
    """-inf inside the separation."""
    return np.where(close(z, fixed, sep), NEG_INF, np.asarray(l, dtype=np.float64))


def multi_table(model, sp, oparams, offsets, nhis, fixed, min_z, max_z, sep, prev_tau_0=0.0023, prev_beta=3.65,
                num_forest_lines=31):
    """(table, null): the conditional log-likelihoods at (offsets, nhis) of the quasar's search range [min_z, max_z]
    with ``fixed`` = [(z, log N), ...] held, NaN -> -inf, and the likelihood of the fixed absorbers alone."""
    from oracle import oracle
    offsets, nhis = np.asarray(offsets, dtype=np.float64), np.asarray(nhis, dtype=np.float64)
    S, F = offsets.size, len(fixed)
    md = max(2, F + 1)
    o = np.concatenate([offsets, [(z - min_z) / (max_z - min_z) for z, _ in fixed]])
    nh = np.concatenate([nhis, [10.0 ** ln for _, ln in fixed]])
    bsi = np.ones((md - 1, S + F), dtype=np.uint32)
    for j in range(F):
        bsi[j, :] = S + j + 1
    r = oracle.process_spectrum_multi(model, o, nh, np.log10(nh), nh, bsi, sp["wavelengths"], sp["flux"], sp["noise_variance"],
                                      sp["pixel_mask"], sp["z_qso"], oparams, max_dlas=md, num_forest_lines=num_forest_lines,
                                      min_z_separation=sep, prev_tau_0=prev_tau_0, prev_beta=prev_beta)
    assert r["rc"] == 0, r["rc"]
    # the driver stores every sample's log-likelihood less log(number of samples) (multi :359-361), here S + F: undone
    log_s = math.log(S + F)
    col = r["sample_log_likelihoods_dla"][:S, F] + log_s
    null = r["log_likelihood_no_dla"] if F == 0 else r["sample_log_likelihoods_dla"][S + F - 1, F - 1] + log_s
    return np.where(np.isnan(col), NEG_INF, col), float(null)


def dense_rows(model, sp, oparams):
    """The rows of process_qsos.m on the kept pixels, the padded wavelengths of the unmasked-range grid and the
    positions of the kept pixels on that grid."""
    from oracle import oracle
    d = oracle.process_spectrum(model, np.array([0.5]), np.array([1e20]), sp["wavelengths"], sp["flux"], sp["noise_variance"],
                                sp["pixel_mask"], sp["z_qso"], oparams, dump=True)
    assert d["rc"] == 0
    wl = np.asarray(sp["wavelengths"])
    rest = wl / (1 + sp["z_qso"])
    inside = (rest >= oparams.min_lambda) & (rest <= oparams.max_lambda)
    kept = np.flatnonzero(np.asarray(sp["pixel_mask"])[inside] == 0)
    take = inside & (np.asarray(sp["pixel_mask"]) == 0)
    return dict(y=np.asarray(sp["flux"])[take], nu=np.asarray(sp["noise_variance"])[take], mu=d["this_mu"], M=d["this_M"],
                omega2=d["this_omega2"], padded=d["padded_wavelengths"], kept=kept, min_z=d["min_z_dla"], max_z=d["max_z_dla"])


def dense_table(rows, num_lines, z, nhis, fixed, sep):
    """(table, null) by the dense route: rows x A, then one log_mvnpdf_low_rank per sample."""
    from oracle import oracle
    A = absorption(rows["padded"], fixed, num_lines)[rows["kept"]]
    mu, M, om = rows["mu"] * A, rows["M"] * A[:, None], rows["omega2"] * (A * A)
    null, rc = oracle.log_mvnpdf_low_rank(rows["y"], mu, M, om + rows["nu"])
    assert rc == 0
    out = np.empty(len(z))
    for i, (zi, ni) in enumerate(zip(z, nhis)):
        a = oracle.voigt(rows["padded"], zi, ni, num_lines)[rows["kept"]]
        out[i], rc = oracle.log_mvnpdf_low_rank(rows["y"], mu * a, M * a[:, None], om * (a * a) + rows["nu"])
        assert rc == 0
    return mask(out, z, fixed, sep), float(null)


def refine_pass(table_at, samples, min_z, max_z, fixed, u, v, levels, delta, pad, sep, status=0, dtype=np.float64):
    """One quasar, one pass.  ``table_at(z, log_n)`` -> the UNMASKED conditional log-likelihoods at those points (any
    route, or a table another implementation produced); the separation rule is applied here, at the first pass and at
    every level, as the contract orders it.  Returns refine_row's dict plus ``first`` (the masked first-pass table)."""
    off, lnhi = np.asarray(samples["offset_samples"], dtype=np.float64), np.asarray(samples["log_nhi_samples"], dtype=np.float64)
    if status != 0 or not (min_z <= max_z):
        row = RR.refine_row(np.full(off.size, np.nan), off, lnhi, min_z, max_z, 1, u, v, None, levels, delta, pad, dtype=dtype)
        row["first"] = np.full(off.size, np.nan)
        return row
    z0 = min_z + (max_z - min_z) * off
    first = mask(table_at(z0, lnhi), z0, fixed, sep)
    row = RR.refine_row(first, off, lnhi, min_z, max_z, 0, u, v, lambda lev, z, n: mask(table_at(z, n), z, fixed, sep),
                        levels, delta, pad, dtype=dtype)
    row["first"] = first
    return row


def twin_table(model, sp, oparams, min_z, max_z, fixed, sep, **multi_kw):
    """``table_at`` and the null likelihood of the multi-DLA route for one quasar and one list."""
    state = {}

    def table_at(z, log_n):
        off = np.zeros_like(z) if max_z == min_z else (z - min_z) / (max_z - min_z)
        t, state["null"] = multi_table(model, sp, oparams, off, 10.0 ** np.asarray(log_n), fixed, min_z, max_z, sep, **multi_kw)
        return t
    return table_at, state


def run(pass_of, lists, extra, rounds, cap=8):
    """The orchestration of conditional.refine_conditional on per-quasar lists of [z, log N]:
    ``pass_of(q, fixed)`` -> dict(status, map_z, map_n, ...) of quasar q conditioned on ``fixed``.  Returns the final
    lists and the history [(name, slot, {q: pass result}, lists after)]."""
    lists = [[list(a) for a in x] for x in lists]
    hist = []
    for e in range(extra):
        res = {q: pass_of(q, list(lists[q])) for q in range(len(lists))}
        for q, r in res.items():
            if r["status"] == 0 and len(lists[q]) < cap:
                lists[q].append([float(r["map_z"]), float(r["map_n"])])
        hist.append((f"discover {e}", -1, res, [[list(a) for a in x] for x in lists]))
    for rd in range(rounds):
        for j in range(max((len(x) for x in lists), default=0)):
            res = {q: pass_of(q, lists[q][:j] + lists[q][j + 1:]) for q in range(len(lists)) if len(lists[q]) > j}
            for q, r in res.items():
                if r["status"] == 0:
                    lists[q][j] = [float(r["map_z"]), float(r["map_n"])]
            hist.append((f"round {rd} slot {j}", j, res, [[list(a) for a in x] for x in lists]))
    return lists, hist


def brute_force_pass(raw_first, raw_levels, offsets, lnhi, min_z, max_z, fixed, u, v, delta, pad, sep):
    """The definitions read literally in Python loops with math.fsum (uniform prior): the separation rule entry by
    entry on the raw tables, then refine_restatement.brute_force_row.  ``raw_levels``: the unmasked l' of each level,
    swept at the boxes this function must reproduce.  Returns (boxes, log Z_ref, MAP (z, n), masked tables)."""
    def rule(values, zs):
        out = []
        for val, z in zip(values, zs):
            inside = False
            for zf, _ in fixed:
                hi, lo = (z, zf) if z > zf else (zf, z)
                if hi - lo < sep:
                    inside = True
            out.append(-math.inf if inside else float(val))
        return out
    N_lo, N_hi = float(min(lnhi)), float(max(lnhi))
    first = rule(raw_first, [min_z + (max_z - min_z) * o for o in offsets])
    masked, parent_boxes = [], []
    # the boxes depend on the masked tables of the levels before them: level by level
    for lev in range(len(raw_levels)):
        boxes, _, _ = RR.brute_force_row(first, offsets, lnhi, min_z, max_z, u, v, masked + [raw_levels[lev]], delta, pad, N_lo, N_hi)
        b = boxes[lev]
        masked.append(rule(raw_levels[lev], [b[0] + (b[1] - b[0]) * x for x in u]))
        parent_boxes.append(b)
    boxes, log_z, map_ind = RR.brute_force_row(first, offsets, lnhi, min_z, max_z, u, v, masked, delta, pad, N_lo, N_hi)
    b = boxes[-1]
    j = map_ind - 1
    return boxes, log_z, (b[0] + (b[1] - b[0]) * u[j], b[2] + (b[3] - b[2]) * v[j]), (first, masked)
