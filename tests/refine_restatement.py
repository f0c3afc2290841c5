"""NumPy restatement of the refine pass (the contract is the comment in include/gpdla.h):
per-quasar zoom boxes of (z_DLA, log10 N_HI), the refined samples, lambda, the refined evidence and MAP.
Every operation is written in the order the contract gives, one rounding each.  ``dtype=np.longdouble``
repeats the sums and the transcendental functions in extended precision (the boxes and the refined
coordinates are float64 in both: they are part of the contract's data, not of its arithmetic error).

The sweep itself is a callable ``sweep(level, z, nhi) -> l'`` (level 0-based): the CPU oracle per quasar
(:func:`oracle_sweep`, the "twin" of the whole feature) or a table the GPU produced.
"""
import math

import numpy as np

UNUSABLE = 1


def level_box(l, z, n, parent, delta, pad, sqrt_s):
    """The box of the next level from (l, z, n) of the source level whose own box is ``parent`` = (z_lo, z_hi,
    n_lo, n_hi): (box, max l, mask of the samples strictly outside the box), or None for an unusable row."""
    l = np.asarray(l, dtype=np.float64)
    ok = ~np.isnan(l)
    if not ok.any():
        return None
    mx = np.max(l[ok])
    if not (mx > -np.inf and mx < np.inf):
        return None
    with np.errstate(invalid="ignore"):
        A = l >= mx - delta
    pz_lo, pz_hi, pn_lo, pn_hi = parent
    padz = pad * (pz_hi - pz_lo) / sqrt_s
    padn = pad * (pn_hi - pn_lo) / sqrt_s
    box = (max(pz_lo, np.min(z[A]) - padz), min(pz_hi, np.max(z[A]) + padz),
           max(pn_lo, np.min(n[A]) - padn), min(pn_hi, np.max(n[A]) + padn))
    outside = (z < box[0]) | (z > box[1]) | (n < box[2]) | (n > box[3])
    return box, mx, outside


def log_prior(n, prior, N_lo, N_hi, dtype=np.float64):
    """log p_N(n): ``prior`` None -> -log(N_hi - N_lo); else the dict of gpdla_nhi_prior's fields (coeff,
    centre, alpha, uniform_min, uniform_max, flat_below, Z), evaluated as gpdla_samples_prior_eval does."""
    n = np.asarray(n, dtype=np.float64)
    if prior is None:
        return np.full(n.shape, -math.log(N_hi - N_lo) if dtype is np.float64 else -np.log(dtype(N_hi - N_lo)), dtype=dtype)
    c0, c1, c2 = prior["coeff"]
    t = n.copy()
    fb = prior["flat_below"]
    if fb == fb:
        t = np.where(t < fb, fb, t)
    s = (t - prior["centre"]).astype(dtype)
    fit = dtype(prior["alpha"]) * (np.exp(dtype(c0) + s * (dtype(c1) + s * dtype(c2))) / dtype(prior["Z"]))
    uni = (1.0 - prior["alpha"]) * (1.0 / (prior["uniform_max"] - prior["uniform_min"]))
    p = np.where((n >= prior["uniform_min"]) & (n <= prior["uniform_max"]), fit + dtype(uni), fit)
    with np.errstate(divide="ignore"):
        return np.log(p)


def _outside_term(l, outside, dtype):
    """(m, Sum exp(l - m)) over the samples outside the box, m their own maximum; (-inf, 0) where there is none, or
    -inf only"""
    l = np.asarray(l, dtype=np.float64)
    take = outside & ~np.isnan(l)
    m = np.max(l[take]) if take.any() else -np.inf
    if not m > -np.inf:
        return -np.inf, dtype(0.0)
    return m, np.sum(np.exp((l[take] - m).astype(dtype)), dtype=dtype)


def refine_row(l, offsets, lnhi, min_z, max_z, status, u, v, sweep, levels=2, delta=12.5, pad=2.0, prior=None,
               N_range=None, dtype=np.float64, lam_tables=None):
    """One quasar.  Returns boxes [levels, 4], ``ell`` and ``lam`` (lists per level; lam in ``dtype``), z', n' of
    the last level, log Z_ref, MAP (z, n, 1-based index) and status, NaN where the contract says NaN.
    ``lam_tables`` (per level, float64): the source of the next level's box and outside sum, and of the final
    sum and MAP, instead of this function's own lambda (a test hands over the tables another implementation
    produced; ``lam`` in the result stays this function's own)."""
    l = np.asarray(l, dtype=np.float64)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    S, Sr = l.size, u.size
    N_lo, N_hi = (float(np.min(lnhi)), float(np.max(lnhi))) if N_range is None else N_range
    out = dict(boxes=np.full((levels, 4), np.nan), ell=[], lam=[], z=np.full(Sr, np.nan), n=np.full(Sr, np.nan),
               log_z=np.nan, map_z=np.nan, map_n=np.nan, map_ind=np.nan, status=UNUSABLE, ambiguity=np.inf)
    if status != 0 or not (min_z <= max_z):
        return out
    prior_dz = max_z - min_z
    parent = (min_z, max_z, N_lo, N_hi)
    src_l, src_z, src_n, sqrt_s = l, min_z + (max_z - min_z) * np.asarray(offsets, dtype=np.float64), np.asarray(lnhi, dtype=np.float64), math.sqrt(S)
    terms = []   # (m, s) in extended or double
    for lev in range(levels):
        got = level_box(src_l, src_z, src_n, parent, delta, pad, sqrt_s)
        if got is None:
            return out
        box, mx, outside = got
        omx, scaled = _outside_term(src_l, outside, dtype)
        scaled = scaled / dtype(len(src_l))
        if lev:
            V = 1.0 if prior_dz == 0.0 else (parent[1] - parent[0]) / prior_dz
            scaled = dtype(V * (parent[3] - parent[2])) * scaled
        terms.append((omx, scaled))
        out["boxes"][lev] = box
        z = box[0] + (box[1] - box[0]) * u
        n = box[2] + (box[3] - box[2]) * v
        ell = np.asarray(sweep(lev, z, n), dtype=np.float64)
        lam = ell.astype(dtype) + log_prior(n, prior, N_lo, N_hi, dtype)
        out["ell"].append(ell)
        out["lam"].append(lam)
        if lam_tables is not None:
            lam = np.asarray(lam_tables[lev], dtype=np.float64).astype(dtype)
        parent, src_l, src_z, src_n, sqrt_s = box, lam.astype(np.float64), z, n, math.sqrt(Sr)
    ok = ~np.isnan(lam)
    if not ok.any():
        return out
    mx = np.max(lam[ok])
    if not (mx > -np.inf and mx < np.inf):
        return out
    V = 1.0 if prior_dz == 0.0 else (box[1] - box[0]) / prior_dz
    total = np.sum(np.exp(lam[ok] - mx), dtype=dtype)
    terms.append((mx, dtype(V * (box[3] - box[2])) * (total / dtype(Sr))))
    terms = [(m, s) for m, s in terms if s > 0]   # a term of 0 has no say in the shift
    M = max((float(m) for m, _ in terms), default=-np.inf)
    tot = dtype(0.0)
    for m, s in terms:
        tot = tot + np.exp(dtype(m) - dtype(M)) * s
    with np.errstate(divide="ignore"):
        out["log_z"] = dtype(M) + np.log(tot)
    lam64 = lam.astype(np.float64)
    j = int(np.flatnonzero(lam64 == np.max(lam64[ok]))[0])
    srt = np.sort(lam64[ok])
    out.update(z=z, n=n, map_z=z[j], map_n=n[j], map_ind=float(j + 1), status=0,
               ambiguity=float(srt[-1] - srt[-2]) if srt.size > 1 else np.inf)
    return out


def brute_force_row(l, offsets, lnhi, min_z, max_z, u, v, ell_levels, delta, pad, N_lo, N_hi):
    """The definitions read literally, in Python loops with math.fsum, for a usable row and a uniform prior.
    ``ell_levels``: the swept l' per level.  Returns (boxes, log Z_ref, MAP index 1-based)."""
    S, Sr, L = len(l), len(u), len(ell_levels)
    zs = [min_z + (max_z - min_z) * o for o in offsets]
    ns = list(lnhi)
    ls = list(l)
    parent = (min_z, max_z, N_lo, N_hi)
    count = S
    pieces, boxes = [], []   # pieces: (log of the piece's factor, list of exponents)
    factor = 1.0 / S
    for lev in range(L):
        fin = [x for x in ls if x == x]
        mx = max(fin)
        A = [i for i in range(count) if ls[i] == ls[i] and ls[i] >= mx - delta]
        wz, wn = parent[1] - parent[0], parent[3] - parent[2]
        box = (max(parent[0], min(zs[i] for i in A) - pad * wz / math.sqrt(count)),
               min(parent[1], max(zs[i] for i in A) + pad * wz / math.sqrt(count)),
               max(parent[2], min(ns[i] for i in A) - pad * wn / math.sqrt(count)),
               min(parent[3], max(ns[i] for i in A) + pad * wn / math.sqrt(count)))
        boxes.append(box)
        outside = [ls[i] for i in range(count) if ls[i] == ls[i] and
                   (zs[i] < box[0] or zs[i] > box[1] or ns[i] < box[2] or ns[i] > box[3])]
        pieces.append((factor, outside))
        V = 1.0 if max_z == min_z else (box[1] - box[0]) / (max_z - min_z)
        factor = V * (box[3] - box[2]) / Sr
        zs = [box[0] + (box[1] - box[0]) * x for x in u]
        ns = [box[2] + (box[3] - box[2]) * x for x in v]
        ls = [e - math.log(N_hi - N_lo) for e in ell_levels[lev]]
        parent, count = box, Sr
    pieces.append((factor, [x for x in ls if x == x]))
    M = max(x for _, xs in pieces for x in xs)
    z_ref = math.fsum(f * math.fsum(math.exp(x - M) for x in xs) for f, xs in pieces)
    best = max(x for x in ls if x == x)
    return boxes, M + math.log(z_ref), ls.index(best) + 1


def oracle_sweep(model, spectrum, min_z, max_z, params=3):
    """The twin's sweep: oracle.process_spectrum at offset = (z' - min_z) / (max_z - min_z), nhi = 10^n'.
    ``params``: oracle.OracleParams, or the number of lines."""
    from oracle import oracle
    if not isinstance(params, oracle.OracleParams):
        params = oracle.OracleParams(num_lines=int(params))

    def sweep(level, z, n):
        off = np.zeros_like(z) if max_z == min_z else (z - min_z) / (max_z - min_z)
        ref = oracle.process_spectrum(model, off, 10.0 ** n, spectrum["wavelengths"], spectrum["flux"],
                                      spectrum["noise_variance"], spectrum["pixel_mask"], spectrum["z_qso"], params)
        return ref["sample_log_likelihoods_dla"]
    return sweep


def tolerance(f64, ext, scale):
    """10 x the restatement's own float64-versus-extended disagreement in units of ``scale``, floored at
    1e-13: (absolute tolerance, disagreement / scale)."""
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(f64, dtype=np.longdouble) - np.asarray(ext, dtype=np.longdouble))
    dis = float(np.nanmax(d) / scale) if np.isfinite(d).any() else 0.0
    return max(10.0 * dis, 1e-13) * scale, dis
