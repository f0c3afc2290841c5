"""NumPy restatement of the posterior maps, the yardstick of k_posterior_maps and
k_posterior_maps_mix.  It implements the contract of include/gpdla.h literally and is built on
tests/posterior_restatement.py (model_weights, slot_table, make_case): np.add.at for the sample-ordered
cell sums and np.cumsum for C, both sequential.  ``brute_*`` state the same a second time in Python loops
with math.fsum and a linear search over the edges, for tiny tables."""
from __future__ import annotations

import math

import numpy as np

import posterior_restatement as pr

UNUSABLE, BAD_GRID, SHORT, BAD_WEIGHTS = 1, 4, 8, 16


def edges(lo, hi, n):
    """The n + 1 edges of an axis: lo + (hi - lo) (c / n) for c < n, and hi itself."""
    lo, hi = np.float64(lo), np.float64(hi)
    return np.append(lo + (hi - lo) * (np.arange(n, dtype=np.float64) / np.float64(n)), hi)


def cells_of(v, lo, hi, n):
    """Cell of every v: the largest c with e_c <= v for lo <= v < hi, n - 1 for v == hi, -1 outside / NaN."""
    v = np.asarray(v, dtype=np.float64)
    e = edges(lo, hi, n)
    with np.errstate(invalid="ignore"):
        inside = (v >= lo) & (v <= hi)
    c = np.searchsorted(e[:n], np.where(inside, v, lo), side="right") - 1
    c = np.where(v == hi, n - 1, c)
    return np.where(inside, c, -1).astype(np.int64)


def grid_ok(grid):
    g = np.asarray(grid, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.all(np.isfinite(g)) and g[1] > g[0] and g[3] > g[2] and np.isfinite(g[1] - g[0]) and np.isfinite(g[3] - g[2]))


def slot_mass(w, z, ln, grid, nz, nn, dtype=np.float64):
    """(mass [nz nn], outside) of one slot on a good grid: sample-ordered sums over T."""
    pos = w > 0
    cz, cn = cells_of(z, grid[0], grid[1], nz), cells_of(ln, grid[2], grid[3], nn)
    inside = (cz >= 0) & (cn >= 0)
    wd = w.astype(dtype)
    T = dtype(w.sum()) if dtype is np.float64 else wd.sum()
    acc = np.zeros(nz * nn, dtype=dtype)
    np.add.at(acc, (cz * nn + cn)[inside & pos], wd[inside & pos])
    out = dtype(0)
    for x in wd[~inside & pos]:       # in sample order
        out = out + x
    return acc / T, out / T


def hpd(mass, levels):
    """(hpd_level [cells], mode, hpd_cells [L], hpd_threshold [L], short) of one slot's masses."""
    mass = np.asarray(mass, dtype=np.float64)
    order = np.argsort(-mass, kind="stable")          # mass descending, ties by index ascending
    order = order[mass[order] > 0]
    C = np.cumsum(mass[order])
    level = np.full(mass.size, np.nan)
    level[order] = C
    npos = order.size
    cells, thr, short = [], [], False
    for p in levels:
        hit = np.flatnonzero(C >= p)
        if hit.size:
            k = int(hit[0]) + 1
        else:
            k, short = npos, True
        cells.append(k)
        thr.append(mass[order[k - 1]] if k else np.nan)
    return level, (int(order[0]) if npos else -1), np.array(cells, dtype=np.int32), np.array(thr, dtype=np.float64), short


def mix(mass, slot_unusable, bad_grid, weights):
    """(intensity [cells], expected_absorbers, bit 16) of one row: mass [md, md, cells]."""
    md, cells = mass.shape[0], mass.shape[2]
    nan = np.full(cells, np.nan)
    if bad_grid:
        return nan, np.nan, 0
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bad = bool(np.any(~(w >= 0)) or np.any((w > 0) & np.asarray(slot_unusable, dtype=bool)))
    if bad:
        return nan, np.nan, BAD_WEIGHTS
    acc = np.zeros(cells)
    for m in range(md):
        if w[m] == 0.0:
            continue
        s = np.zeros(cells)
        for j in range(m + 1):
            s = s + mass[m, j]
        acc = acc + w[m] * s
    return acc, float(np.cumsum(acc)[-1]), 0


def maps(sll, offsets, lnhi, z_min, z_max, grids, shape, base=None, levels=(), model_weights=None, n_lo=None, n_hi=None,
         extended=False):
    """sll [n, md, S] (or [n, S]), base [n, md - 1, S] or None, grids [n, 4] -> the arrays of
    gpdla_posterior_maps.  ``extended``: the cell sums, T and the division in np.longdouble, returned as
    float64 (mass and outside only mean something then)."""
    sll = np.asarray(sll, dtype=np.float64)
    if sll.ndim == 2:
        sll = sll[:, None, :]
    n, md, S = sll.shape
    nz, nn = shape
    cells, L = nz * nn, len(levels)
    offsets, lnhi = np.asarray(offsets, dtype=np.float64), np.asarray(lnhi, dtype=np.float64)
    grids = np.asarray(grids, dtype=np.float64).reshape(n, 4)
    out = dict(mass=np.full((n, md, md, nz, nn), np.nan), hpd_level=np.full((n, md, md, nz, nn), np.nan),
               outside=np.full((n, md, md), np.nan), mode=np.full((n, md, md), -1, dtype=np.int32),
               hpd_cells=np.full((n, md, md, L), -1, dtype=np.int32), hpd_threshold=np.full((n, md, md, L), np.nan),
               status=np.zeros((n, md), dtype=np.int32))
    dt = np.longdouble if extended else np.float64
    for r in range(n):
        ok = grid_ok(grids[r])
        for m in range(1, md + 1):
            st = 0 if ok else BAD_GRID
            rows = None if m == 1 else np.asarray(base[r, :m - 1])
            w, usable = pr.model_weights(sll[r, m - 1], rows, S)
            if not usable:
                st |= UNUSABLE
            if st == 0:
                for j in range(m):
                    b = pr.slot_base(rows, j, S)
                    with np.errstate(invalid="ignore"):
                        z = float(z_min[r]) + (float(z_max[r]) - float(z_min[r])) * offsets[b]
                    ln = lnhi[b] if n_lo is None else float(n_lo[r]) + (float(n_hi[r]) - float(n_lo[r])) * lnhi[b]
                    ms, o = slot_mass(w, z, ln, grids[r], nz, nn, dt)
                    ms = ms.astype(np.float64)
                    out["mass"][r, m - 1, j] = ms.reshape(nz, nn)
                    out["outside"][r, m - 1, j] = float(o)
                    lv, mode, hc, th, short = hpd(ms, levels)
                    out["hpd_level"][r, m - 1, j] = lv.reshape(nz, nn)
                    out["mode"][r, m - 1, j] = mode
                    out["hpd_cells"][r, m - 1, j] = hc
                    out["hpd_threshold"][r, m - 1, j] = th
                    if short:
                        st |= SHORT
            out["status"][r, m - 1] = st
    if model_weights is not None:
        out.update(mix_of(out["mass"], out["status"], model_weights))
        out["status"] = out["status"] | out.pop("row_status")[:, None]
    return out


def hpd_of(mass, status, levels):
    """The HPD outputs and bit 8 the contract derives from given masses [n, md, md, nz, nn] (the GPU's own,
    in the tests): {hpd_level, mode, hpd_cells, hpd_threshold, short [n, md] bool}."""
    n, md = mass.shape[:2]
    L = len(levels)
    out = dict(hpd_level=np.full(mass.shape, np.nan), mode=np.full((n, md, md), -1, dtype=np.int32),
               hpd_cells=np.full((n, md, md, L), -1, dtype=np.int32), hpd_threshold=np.full((n, md, md, L), np.nan),
               short=np.zeros((n, md), dtype=bool))
    for r in range(n):
        for m in range(md):
            if status[r, m] & (UNUSABLE | BAD_GRID):
                continue
            for j in range(m + 1):
                lv, mode, hc, th, short = hpd(mass[r, m, j].reshape(-1), levels)
                out["hpd_level"][r, m, j] = lv.reshape(mass.shape[3:])
                out["mode"][r, m, j], out["hpd_cells"][r, m, j], out["hpd_threshold"][r, m, j] = mode, hc, th
                out["short"][r, m] |= short
    return out


def mix_of(mass, status, model_weights):
    """{intensity [n, nz, nn], expected_absorbers [n], row_status [n]} the contract derives from given masses."""
    n, md = mass.shape[:2]
    shape = mass.shape[3:]
    out = dict(intensity=np.full((n,) + shape, np.nan), expected_absorbers=np.full(n, np.nan),
               row_status=np.zeros(n, dtype=np.int32))
    for r in range(n):
        inten, e, bit = mix(mass[r].reshape(md, md, -1), (status[r] & UNUSABLE) != 0, bool(status[r, 0] & BAD_GRID),
                            np.asarray(model_weights, dtype=np.float64).reshape(n, md)[r])
        out["intensity"][r], out["expected_absorbers"][r], out["row_status"][r] = inten.reshape(shape), e, bit
    return out


# ---------------------------------------------------------------------------------------------
# the same in Python loops, for tiny tables
# ---------------------------------------------------------------------------------------------

def brute_cell(v, lo, hi, n):
    if not (v >= lo and v <= hi):
        return -1
    if v == hi:
        return n - 1
    c = -1
    for k in range(n):                      # linear search: the largest c with e_c <= v
        if float(np.float64(lo) + np.float64(hi - lo) * (np.float64(k) / np.float64(n))) <= v:
            c = k
    return c


def brute_slot(w, z, ln, grid, nz, nn, levels):
    """(mass, outside, hpd_level, mode, ranks, hpd_cells) of one slot: math.fsum sums, a Python sort."""
    T = math.fsum(float(x) for x in w)
    members = [[] for _ in range(nz * nn)]
    out = []
    cell = []
    for wi, zi, ni in zip(w, z, ln):
        cz, cn = brute_cell(float(zi), grid[0], grid[1], nz), brute_cell(float(ni), grid[2], grid[3], nn)
        cell.append(-1 if cz < 0 or cn < 0 else cz * nn + cn)
        if wi > 0:
            (out if cell[-1] < 0 else members[cell[-1]]).append(float(wi))
    mass = [math.fsum(x) / T for x in members]
    ranks = sorted((c for c in range(nz * nn) if mass[c] > 0), key=lambda c: (-mass[c], c))
    level = [float("nan")] * (nz * nn)
    run = []
    for c in ranks:
        run.append(mass[c])
        level[c] = math.fsum(run)
    hc = []
    for p in levels:
        k = next((i + 1 for i, c in enumerate(ranks) if level[c] >= p), len(ranks))
        hc.append(k)
    return (np.array(mass), math.fsum(out) / T, np.array(level), ranks[0] if ranks else -1, ranks, hc, np.array(cell))


# ---------------------------------------------------------------------------------------------
# seeded inputs shared by tests/test_posterior_maps.py (CPU) and tests/test_gpu_posterior_maps.py
# ---------------------------------------------------------------------------------------------

# (not k / S for the small S of the flat rows: there C_k would meet the level within rounding, and the order of
# the additions, which the loops with math.fsum do not share, would decide the count)
LEVELS = (0.4839, 0.6827, 0.9545)


def default_grids(z_min, z_max, lnhi):
    """One grid per row over the row's search range and the table's log N range (NaN and empty ranges as they are)."""
    n = len(z_min)
    return np.stack([np.asarray(z_min, dtype=np.float64), np.asarray(z_max, dtype=np.float64),
                     np.full(n, float(np.min(lnhi))), np.full(n, float(np.max(lnhi)))], axis=1)


def edge_case(nz=8, nn=5, md=2):
    """Rows whose samples sit bitwise on the edges of a (nz, nn) grid over z in [2, 3] (nz a power of two) and
    log N in [20, 23]: one row whose offsets are c / nz and whose log N are the restatement's own edges (each
    opens its cell; hi falls in the last), one with the nextafter value below each (each closes the cell
    before), and a flat copy of the first row's geometry with equal weights (exact ties).  Returns (sll, base,
    offsets, lnhi, z_min, z_max, grids, on_edge [S] bool)."""
    rng = np.random.default_rng(77)
    ez, en = edges(2.0, 3.0, nz), edges(20.0, 23.0, nn)
    offs, lns, on = [], [], []
    for c in range(nz + 1):                       # z on an edge (offset c / nz is exact), log N inside a cell
        for k in range(nn):
            offs.append(c / nz)
            lns.append(0.5 * (en[k] + en[k + 1]))
            on.append(True)
    for k in range(nn + 1):                       # log N on an edge, z inside a cell
        for c in range(nz):
            offs.append((c + 0.5) / nz)
            lns.append(en[k])
            on.append(True)
    off, ln = np.array(offs), np.array(lns)
    S0 = off.size
    # the value below each edge: offsets whose z = 2 + offset is the double below the edge (the difference is
    # exact), log N the double below the edge
    off_b = np.nextafter(2.0 + off, 0.0) - 2.0
    assert np.array_equal(2.0 + off_b, np.nextafter(2.0 + off, 0.0))
    ln_b = np.nextafter(ln, 0.0)
    offsets = np.concatenate([off, off_b, rng.random(16)])
    lnhi = np.concatenate([ln, ln_b, 20.0 + 3.0 * rng.random(16)])
    on_edge = np.concatenate([np.array(on), np.zeros(S0 + 16, dtype=bool)])
    S = offsets.size
    n = 3
    sll = 1.5 * rng.standard_normal((n, md, S)) - 40.0
    sll[1] = sll[0]
    sll[2] = 3.25                                 # flat: exact ties, the region goes by index
    base = rng.integers(1, S + 1, size=(n, md - 1, S)).astype(np.uint32) if md > 1 else None
    z_min, z_max = np.full(n, 2.0), np.full(n, 3.0)
    grids = np.tile(np.array([2.0, 3.0, 20.0, 23.0]), (n, 1))
    return sll, base, offsets, lnhi, z_min, z_max, grids, on_edge


def maps_case(S, md, seed=0):
    """The 12 rows of make_case and a 13th whose models above the first are unusable (every base index 0; for
    one model: a second all-NaN row), so that two rows carry unusable models."""
    sll, base, off, lnhi, z_min, z_max = pr.make_case(S, md, seed)
    k = pr.ROW_KINDS.index("broad" if md > 1 else "all_nan")
    sll = np.concatenate([sll, sll[k:k + 1]])
    if md > 1:
        base = np.concatenate([base, np.zeros((1, md - 1, S), dtype=np.uint32)])
    z_min, z_max = np.append(z_min, 2.05), np.append(z_max, 3.55)
    return sll, base, off, lnhi, z_min, z_max


def grid_variants(z_min, z_max, lnhi):
    """Named per-row grids on the rows of make_case: the default, the lower half of the z range (outside mass),
    and a reversed and a NaN grid on alternating rows (bit 4)."""
    full = default_grids(z_min, z_max, lnhi)
    if not np.all(full[:, 3] > full[:, 2]):       # one sample, or equal ones: no log N range to speak of
        full[:, 2], full[:, 3] = full[:, 2] - 0.5, full[:, 3] + 0.5
    half = full.copy()
    half[:, 1] = z_min + 0.5 * (np.asarray(z_max) - z_min)
    bad = full.copy()
    bad[0::2, [0, 1]] = bad[0::2, [1, 0]]         # reversed
    bad[1::2, 2] = np.nan
    return {"full": full, "half": half, "bad": bad}


def peak_excluding_grids(sll, base, offsets, lnhi, z_min, z_max):
    """Per row a grid over the z range on the far side of the row's model-1 MAP sample (so a peaked posterior's
    mass is outside: bit 8)."""
    n = sll.shape[0]
    g = default_grids(z_min, z_max, lnhi)
    for r in range(n):
        row = sll[r, 0]
        if np.all(np.isnan(row)):
            continue
        o = offsets[int(np.nanargmax(row))]
        lo, hi = (z_min[r] + (z_max[r] - z_min[r]) * min(o + 0.05, 0.95), z_max[r]) if o < 0.5 else \
            (z_min[r], z_min[r] + (z_max[r] - z_min[r]) * max(o - 0.05, 0.05))
        g[r, 0], g[r, 1] = lo, hi
    return g


def weight_cases(status):
    """Model-weight rows [n, md] for the rows of a case with this status [n, md]: random positive weights
    with a zero on every unusable model (legal: skipped), then row 0 with a NaN, row 1 with a negative entry,
    and the first row that has an unusable model with a positive weight on it (bit 16)."""
    rng = np.random.default_rng(5)
    n, md = status.shape
    w = rng.random((n, md)) + 0.1
    w /= w.sum(axis=1, keepdims=True)
    unusable = (status & UNUSABLE) != 0
    w[unusable] = 0.0
    w[0, 0] = np.nan
    w[1, md - 1] = -0.25
    rows = np.flatnonzero(unusable.any(axis=1))
    assert rows.size >= 2 and rows[0] > 1, "the case needs two rows with unusable models beyond rows 0 and 1"
    r = rows[-1]
    w[r, np.flatnonzero(unusable[r])[0]] = 0.5
    return w


def mass_tolerance(f64, ext):
    """tol of mass and outside: 10 x the restatement's own float64-versus-extended disagreement, floored at
    1e-13 absolute.  Returns (tol, disagreement)."""
    with np.errstate(invalid="ignore"):
        d = max(np.nanmax(np.abs(f64["mass"] - ext["mass"]), initial=0.0), np.nanmax(np.abs(f64["outside"] - ext["outside"]), initial=0.0))
    return max(10.0 * float(d), 1e-13), float(d)
