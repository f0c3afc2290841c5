"""NumPy restatement of the parameter summaries, deliberately naive: one argsort and
one cumsum per row, model, slot and quantity.  It is the yardstick of k_parameter_summaries and
implements the definitions of include/gpdla.h literally.  The moments, and the cumulative sums the
quantile acceptance rests on, are evaluated a second time in extended precision (np.longdouble,
products and sums alike)."""
from __future__ import annotations

import numpy as np

FIELDS3 = ("mean_z", "std_z", "mean_log_nhi", "std_log_nhi", "cov")
EPS = 1e-11   # the quantile acceptance band, in units of F / T


def model_weights(l_row, base_rows, S):
    """(w, usable) of one (row, model): base_rows = the model's [m - 1, S] base indices (or None)."""
    l = np.array(l_row, dtype=np.float64)
    if base_rows is not None:
        for b in base_rows:
            l[(b == 0) | (b > S)] = np.nan
    ok = ~np.isnan(l)
    if not ok.any():
        return None, False
    mx = l[ok].max()
    if not np.isfinite(mx):
        return None, False
    w = np.zeros(S)
    with np.errstate(over="ignore"):
        w[ok] = np.exp(l[ok] - mx)
    return w, True


def slot_base(base_rows, j, S):
    """0-based base sample of every sample in slot j (0-based)."""
    if j == 0:
        return np.arange(S)
    b = base_rows[j - 1].astype(np.int64)
    return np.where((b == 0) | (b > S), 0, b - 1)


def weighted_quantiles(v, w, T, probabilities):
    """Per probability p the smallest value v* among the samples of positive weight with F(v*) >= p T;
    the largest such value when rounding leaves the total short of p T."""
    pos = w > 0
    vv, ww = v[pos], w[pos]
    order = np.argsort(vv, kind="stable")
    cum = np.cumsum(ww[order])
    out = []
    for p in probabilities:
        hit = np.flatnonzero(cum >= p * T)
        k = hit[0] if hit.size else order.size - 1
        out.append(vv[order[k]])      # equal values share the answer: it is the value that is returned
    return out


def weighted_quantile(v, w, T, p):
    return weighted_quantiles(v, w, T, [p])[0]


def acceptable_values(v, w, probabilities, eps=EPS):
    """Per probability p the values a quantile routine may name: positive weight, F-(v) / T < p + eps and
    F(v) / T >= p - eps, with F(v) = sum over v_i <= v and F-(v) = sum over v_i < v in extended precision."""
    pos = w > 0
    vv, ww = v[pos], w[pos].astype(np.longdouble)
    order = np.argsort(vv, kind="stable")
    vs, cum = vv[order], np.cumsum(ww[order])
    T = cum[-1]
    last = np.flatnonzero(np.append(vs[1:] != vs[:-1], True))       # last index of each value group
    first = np.append(0, last[:-1] + 1)
    F = cum[last] / T
    Fm = np.where(first > 0, cum[np.maximum(first - 1, 0)], np.longdouble(0)) / T
    return [vs[last][(Fm < p + eps) & (F >= p - eps)] for p in probabilities]


def _moments(w, z, ln, T, thresholds, dtype):
    w, z, ln = w.astype(dtype), z.astype(dtype), ln.astype(dtype)
    T = dtype(T)
    pos = w > 0
    w, z, ln = w[pos], z[pos], ln[pos]
    mz, mn = (w * z).sum() / T, (w * ln).sum() / T
    vz, vn = (w * (z - mz) ** 2).sum() / T, (w * (ln - mn) ** 2).sum() / T
    cov = (w * ((z - mz) * (ln - mn))).sum() / T
    ex = [w[ln >= dtype(t)].sum() / T for t in thresholds]
    return mz, np.sqrt(vz), mn, np.sqrt(vn), cov, ex


def summaries(sll, offsets, lnhi, z_min, z_max, base=None, probabilities=(0.025, 0.16, 0.5, 0.84, 0.975),
              thresholds=(20.3,), extended=False):
    """sll [n, md, S] (or [n, S]), base [n, md - 1, S] uint32 or None -> the arrays of
    gpdla_parameter_summaries.  ``extended``: moments, exceedance and ESS summed in np.longdouble (the
    weights stay the float64 exponentials) and returned as float64; the quantiles are left out (NaN)."""
    sll = np.asarray(sll, dtype=np.float64)
    if sll.ndim == 2:
        sll = sll[:, None, :]
    n, md, S = sll.shape
    offsets, lnhi = np.asarray(offsets, dtype=np.float64), np.asarray(lnhi, dtype=np.float64)
    Q, nt = len(probabilities), len(thresholds)
    out = {k: np.full((n, md, md), np.nan) for k in FIELDS3}
    out["quantiles_z"] = np.full((n, md, md, Q), np.nan)
    out["quantiles_log_nhi"] = np.full((n, md, md, Q), np.nan)
    out["exceedance"] = np.full((n, md, md, nt), np.nan)
    out["effective_samples"] = np.full((n, md), np.nan)
    out["status"] = np.zeros((n, md), dtype=np.int32)
    dt = np.longdouble if extended else np.float64
    for r in range(n):
        zmin, zmax = float(z_min[r]), float(z_max[r])
        z_ok = not (np.isnan(zmin) or np.isnan(zmax))
        for m in range(1, md + 1):
            rows = None if m == 1 else np.asarray(base[r, :m - 1])
            out["status"][r, m - 1] = 0 if z_ok else 2
            w, usable = model_weights(sll[r, m - 1], rows, S)
            if not usable:
                out["status"][r, m - 1] |= 1
                continue
            wd = w.astype(dt)
            T = wd.sum()
            out["effective_samples"][r, m - 1] = T * T / (wd * wd).sum()
            T64 = float(w.sum())
            for j in range(m):
                b = slot_base(rows, j, S)
                with np.errstate(invalid="ignore"):
                    z = zmin + (zmax - zmin) * offsets[b]
                ln = lnhi[b]
                mz, sz, mn, sn, cov, ex = _moments(w, z if z_ok else np.zeros(S), ln, T, thresholds, dt)
                o = (r, m - 1, j)
                out["mean_log_nhi"][o], out["std_log_nhi"][o] = mn, sn
                if z_ok:
                    out["mean_z"][o], out["std_z"][o], out["cov"][o] = mz, sz, cov
                out["exceedance"][o] = ex
                if Q and not extended:
                    out["quantiles_log_nhi"][o] = weighted_quantiles(ln, w, T64, probabilities)
                    if z_ok:
                        out["quantiles_z"][o] = weighted_quantiles(z, w, T64, probabilities)
    return out


def slot_table(sll, offsets, lnhi, z_min, z_max, base, r, m, j):
    """(w, z, log N) of slot j (0-based) of model m (1-based) of row r, or None if unusable."""
    sll = np.asarray(sll, dtype=np.float64)
    if sll.ndim == 2:
        sll = sll[:, None, :]
    S = sll.shape[2]
    rows = None if m == 1 else np.asarray(base[r, :m - 1])
    w, usable = model_weights(sll[r, m - 1], rows, S)
    if not usable:
        return None
    b = slot_base(rows, j, S)
    with np.errstate(invalid="ignore"):
        z = float(z_min[r]) + (float(z_max[r]) - float(z_min[r])) * np.asarray(offsets)[b]
    return w, z, np.asarray(lnhi)[b]


# ---------------------------------------------------------------------------------------------
# seeded inputs shared by tests/test_posteriors.py (CPU) and tests/test_gpu_posteriors.py
# ---------------------------------------------------------------------------------------------

TILE = 1024   # kPostTile of posterior_kernels.hpp
S_VALUES = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 10004, 16501)   # 16501: B = 65 > 64
MD_VALUES = (1, 2, 4)
PROBABILITIES = (0.025, 0.16, 0.5, 0.84, 0.975)
THRESHOLDS = (20.3, 21.0)
ROW_KINDS = ("peaked", "broad", "flat", "one_finite", "all_nan", "minus_inf_one_finite", "nan_scattered",
             "same_base", "base_zeros", "nan_max_z", "zero_width", "bimodal_z")


def make_case(S, md, seed=0):
    """One row of every kind of ROW_KINDS: (sll [12, md, S], base [12, md - 1, S] or None, offsets, lnhi,
    z_min, z_max)."""
    rng = np.random.default_rng(1000 * md + S + seed)
    n = len(ROW_KINDS)
    off, lnhi = rng.random(S), 20.0 + 3.0 * rng.random(S)
    if S >= 8:            # equal values under different indices: the ranks break the tie by index
        off[5], lnhi[6] = off[1], lnhi[2]
    sll = 1.5 * rng.standard_normal((n, md, S)) - 300.0
    base = rng.integers(1, S + 1, size=(n, md - 1, S)).astype(np.uint32) if md > 1 else None
    z_min = 2.0 + 0.1 * np.arange(n)
    z_max = z_min + 1.0
    k = ROW_KINDS.index
    for m in range(md):
        sll[k("peaked"), m, rng.integers(S)] += 800.0
        sll[k("flat"), m] = 3.25
        one = np.full(S, np.nan)
        one[rng.integers(S)] = -12.5
        sll[k("one_finite"), m] = one
        sll[k("all_nan"), m] = np.nan
        one = np.full(S, -np.inf)
        one[rng.integers(S)] = 7.0
        sll[k("minus_inf_one_finite"), m] = one
        sll[k("nan_scattered"), m, rng.random(S) < 0.3] = np.nan
        sll[k("bimodal_z"), m] = np.logaddexp(-0.5 * ((off - 0.2) / 0.05) ** 2, -0.5 * ((off - 0.8) / 0.05) ** 2) \
            + 0.1 * rng.standard_normal(S)
    if md > 1:
        base[k("same_base"), 0] = 7 % S + 1
        base[k("base_zeros")][rng.random((md - 1, S)) < 0.25] = 0
    z_max[k("nan_max_z")] = np.nan
    z_max[k("zero_width")] = z_min[k("zero_width")]
    return sll, base, off, lnhi, z_min, z_max


_CASES = {}


def case_reference(S, md):
    """The inputs of make_case(S, md), the restatement's float64 and extended summaries of them, and
    per compared (row, model - 1, slot, quantity, probability index) the values a quantile routine may
    name (quantity 0: z, 1: log N).  Computed once per process."""
    if (S, md) in _CASES:
        return _CASES[(S, md)]
    sll, base, off, lnhi, z_min, z_max = make_case(S, md)
    f64 = summaries(sll, off, lnhi, z_min, z_max, base, PROBABILITIES, THRESHOLDS)
    ext = summaries(sll, off, lnhi, z_min, z_max, base, PROBABILITIES, THRESHOLDS, extended=True)
    accept = {}
    for r in range(sll.shape[0]):
        for m in range(1, md + 1):
            if f64["status"][r, m - 1] & 1:
                continue
            for j in range(m):
                w, z, ln = slot_table(sll, off, lnhi, z_min, z_max, base, r, m, j)
                for qy, v in ((0, z), (1, ln)):
                    if qy == 0 and f64["status"][r, m - 1] & 2:
                        continue
                    for q, vals in enumerate(acceptable_values(v, w, PROBABILITIES)):
                        accept[(r, m - 1, j, qy, q)] = vals
    ref = dict(inputs=(sll, base, off, lnhi, z_min, z_max), f64=f64, ext=ext, accept=accept)
    _CASES[(S, md)] = ref
    return ref


def tolerances(ref):
    """tol x scale per class of output: 10 x the restatement's own float64-versus-extended disagreement
    on these inputs in units of the scale, floored at 1e-13 and capped at 1e-9.  Returns {field:
    (absolute tolerance array broadcastable to the field, disagreement in scale units)}; ESS relative."""
    sll, base, off, lnhi, z_min, z_max = ref["inputs"]
    with np.errstate(invalid="ignore"):
        z_scale = np.fmax(np.abs(z_min), np.abs(z_max))
    n_scale = float(np.max(np.abs(lnhi)))
    scales = dict(mean_z=z_scale[:, None, None], std_z=z_scale[:, None, None], cov=(z_scale * n_scale)[:, None, None],
                  mean_log_nhi=n_scale, std_log_nhi=n_scale, exceedance=1.0,
                  effective_samples=np.abs(ref["ext"]["effective_samples"]))
    out = {}
    for k, sc in scales.items():
        with np.errstate(invalid="ignore"):
            d = np.abs(ref["f64"][k] - ref["ext"][k]) / (sc if np.ndim(sc) != 3 or ref["f64"][k].ndim == 3 else sc[..., None])
        dis = float(np.nanmax(d)) if np.isfinite(d).any() else 0.0
        tol = min(max(10.0 * dis, 1e-13), 1e-9)
        out[k] = (tol * sc, dis, tol)
    return out
