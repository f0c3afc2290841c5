"""The marginal continuum and the posterior predictive flux where the arithmetic is hard (plain module, like
hard_conditioning_cases.py: the fixture generator tests/golden/make_exact_continuum_hard.py, test_continuum_hard.py and
test_gpu_continuum_hard.py import it, nothing else does).

Both subsystems do more delicate algebra than the sweeps on the same capacitance matrix B_i = I + M' diag(a^2/d) M: an
explicit inverse, Sigma_i = B_i^-1 and c_i = Sigma_i M' (a (y - a mu) / d), and one-pass between-sample variances
V = Sum w c c' - cbar cbar' and F2 - F1^2.  On the classes of hard_conditioning_cases.py (cond(B) up to 1e7) the two fp64
restatements of tests/marginal_continuum_restatement.py disagree by more than the cap of ``R.continuum_tolerance``, so
neither is a yardstick there.  The yardstick is a 50-digit evaluation (``exact_sample``, ``exact_products``) of the very
fp64 inputs the restatement forms, and the bound is set by what the Woodbury-form restatement attains on the same inputs.

    classes     H.CLASSES (one sightline: 131 in-range pixels, 65 samples, k = 20 / 33 / 40, 3 and 31 lines); the multi
                classes use the mean-flux rows and have a sub-DLA table
    rows        host log-likelihood rows placed by hand (ROWS): the hard classes' own sweep rows are one-hot after
                normalisation, so only a placed row exercises the between-sample sums
    mixtures    (null, sub-DLA, DLA) weights, ``mixtures_of``

The error of a product on one (class, row, mixture) is max |got - exact| over its entries divided by
max(1, max |exact|) (``error``: hard-class covariances reach 1e3); for the three products bounded away from 0
(REL_PRODUCTS) also the worst per-pixel relative error (``rel_error``).  The bound is ``tolerance``:
max(10 x e_restatement, 1e-12), e_restatement the Woodbury restatement's largest error over the product's family
(FAMILIES) on the same (class, row, mixture), computed from the fixture alone.  There is no upper cap on the bound;
RESTATEMENT_CAP on the choice of inputs takes its place.  The per-sample continua mu + M c_i that
``Batch.model_spectra`` is compared with have no row: their e_restatement is the Woodbury restatement's error on the
same three continua, under the same rule.

The exact values fill two files (FIXTURES): with the second mixture of the two ``correlated`` classes they come to
1.3 MB of incompressible doubles, more than one committed file may hold, so the k = 33 and k = 40 classes have their own.
"""
from __future__ import annotations

import zipfile

import numpy as np

import hard_conditioning_cases as H
import marginal_continuum_restatement as MR
import model_spectra_restatement as R
import predictive_flux_restatement as PR

ROWS = ("sweep", "top8_flat", "adjacent_pair", "near_one_hot", "flat")
DEAD = -1e6                    # exp(-1e6 - max) is exactly 0 in fp64: a sample that is never evaluated (MC.skip_row)
RESTATEMENT_CAP = 1e-6         # a condition on the choice of inputs, like H.ORACLE_CAP
TOL_FACTOR = H.TOL_FACTOR      # 10: the project's convention
TOL_FLOOR = 1e-12              # R.continuum_tolerance's
DPS = 50
FIXTURES = ("exact_continuum_hard.npz", "exact_continuum_hard_k33_k40.npz")
PARENT = "hard:"               # a reference into tests/golden/exact_hard_conditioning.npz

MC_PRODUCTS = MR.PRODUCTS_COEF[1:] + MR.PRODUCTS_COV            # without sample_coefficients
FAMILIES = {"coef": MR.PRODUCTS_COEF, "cov": MR.PRODUCTS_COV, "flux_mean": PR.PRODUCTS_MEAN, "flux_var": PR.PRODUCTS_VAR}
REL_PRODUCTS = ("continuum_var", "flux_var", "flux_var_within")
FAMILY_OF = {n: f for f, names in FAMILIES.items() for n in names}
SAMPLE_COEFFICIENT_CLASSES = (("correlated", "single", 20, 3), ("correlated", "single", 40, 3))


def fixture_of(cls) -> str:
    return FIXTURES[0] if cls[2] <= 20 else FIXTURES[1]


def tables_of(cls):
    return ("sub_dla", "dla") if cls[1] == "multi" else ("dla",)


def mixtures_of(cls):
    """[((null, sub-DLA, DLA) weights, sample_coefficients)]"""
    out = [((0.2, 0.3, 0.5), False)] if cls[1] == "multi" else [((0.2, 0.0, 0.8), False)]
    if cls in SAMPLE_COEFFICIENT_CLASSES:
        out.append(((0.0, 0.0, 1.0), True))
    return out


def components_of(p):
    return tuple(n for n, pm in zip(MR.COMPONENTS, p) if pm > 0)


EXACT_TABLE = {"dla": "exact_dla", "sub_dla": "exact_lls"}


def weight_rows(exact_table, offset_samples) -> dict:
    """{row name: [S] host log-likelihood row} from a class's stored exact table; positions depend on no run."""
    ll = np.asarray(exact_table, dtype=np.float64)
    assert np.isfinite(ll).all()
    by_ll = np.argsort(-ll, kind="stable")
    z_order = np.argsort(np.asarray(offset_samples), kind="stable")
    best = int(by_ll[0])
    pos = int(np.flatnonzero(z_order == best)[0])
    neighbour = int(z_order[pos + 1] if pos + 1 < ll.size else z_order[pos - 1])

    def placed(idx, values):
        row = np.full(ll.size, DEAD)
        row[np.asarray(idx)] = values
        return row
    return {"sweep": ll.copy(), "top8_flat": placed(by_ll[:8], 0.0), "adjacent_pair": placed([best, neighbour], 0.0),
            "near_one_hot": placed(by_ll[:2], [0.0, np.log(1e-6)]), "flat": placed(np.arange(ll.size), 0.0)}


def n_eff(row) -> float:
    w = R.weights(row)
    return float(1.0 / np.sum(w * w))


def spectra_samples(row_top8, offset_samples):
    """the three live samples of lowest, median and highest z_DLA of the ``top8_flat`` row"""
    live = np.flatnonzero(R.weights(row_top8) > 0)
    live = live[np.argsort(np.asarray(offset_samples)[live], kind="stable")]
    return np.array([live[0], live[live.size // 2], live[-1]])


# ---------------------------------------------------------------- the fp64 inputs, as the restatement forms them

INPUT_KEYS = ("y", "mu", "M", "omega2", "nu", "kept", "mu_all", "M_all", "z_dlas")


def inputs(oracle, case) -> dict:
    """Everything the evaluation consumes: ``MR.prepared_rows`` on the kept pixels, ``R.interp_rows`` on all n_u pixels
    (mean-flux suppressed for a multi class), the ``oracle.voigt`` profiles of every sample of every table on the whole
    grid, z_DLA from min_z, max_z and the offsets."""
    cls, model, sp, sm = case["cls"], case["model"], case["spectrum"], case["samples"]
    meanflux, lines = cls[1] == "multi", cls[3]
    g = R.grid(oracle, model, sp)
    y, mu, M, omega2, nu = MR.prepared_rows(oracle, model, g, meanflux)
    mu_all, M_all = R.interp_rows(model, g["wl"], g["z_qso"])
    if meanflux:
        f = oracle.mean_flux_suppression(g["wl"], g["z_qso"], 0.0023, 3.65, 31, 1215.6701)
        mu_all, M_all = mu_all * f, M_all * f[:, None]
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.asarray(sm["offset_samples"])
    out = dict(y=np.array(y), mu=np.array(mu), M=np.ascontiguousarray(M), omega2=np.array(omega2), nu=np.array(nu),
               kept=np.array(g["kept"]), mu_all=mu_all, M_all=np.ascontiguousarray(M_all), z_dlas=z)
    for t in tables_of(cls):
        nhi = sm[MR.NHI_KEY[t]]
        out["profiles_" + t] = np.stack([oracle.voigt(g["pad"], z[i], nhi[i], lines) for i in range(z.size)])
    assert out["kept"].size == H.N_PIX and out["M_all"].shape == (H.N_PIX, cls[2])
    return out


def rows_of(inp, nu=None):
    return inp["y"], inp["mu"], inp["M"], inp["omega2"], inp["nu"] if nu is None else nu


# ---------------------------------------------------------------- the restatement on stored inputs

def restatement_samples(inp, tables, form: str, nu=None) -> dict:
    """Per table the (c_i, Sigma_i, t_i, s_i) of all samples, and under "null" those of a = 1, by ``MR.sample_dense`` /
    ``MR.sample_woodbury``; ``nu`` replaces the noise variances of the kept pixels."""
    rows = rows_of(inp, nu)
    solve = MR.sample_dense if form == "dense" else MR.sample_woodbury
    mu_all, M_all, kept = inp["mu_all"], inp["M_all"], inp["kept"]

    def one(a_full):
        c, Sig = solve(*rows, a_full[kept])
        return c, Sig, mu_all + M_all @ c, np.einsum("pi,ij,pj->p", M_all, Sig, M_all)
    out = {"null": [one(np.ones(kept.size))], "nu": rows[4]}
    for t in tables:
        out[t] = [one(a) for a in inp["profiles_" + t]]
    return out


def restatement_products(inp, per_sample, rows_by_table, p, sample_coefficients=False, components=MR.COMPONENTS) -> dict:
    """The seven marginal-continuum and five predictive-flux products of one (row, mixture) in fp64, with the sums in
    the order of ``MR.sampled_component`` / ``PR.component`` and the mixing of ``MR.mix`` / ``PR.mix``.  ``components``:
    the names behind ``p``, "null" first; a sampled one has ``inp["profiles_" + name]``, a row and per-sample results."""
    p = np.asarray(p, dtype=np.float64)
    p = p / p.sum()
    kept, n_u = inp["kept"], inp["kept"].size
    k = inp["M"].shape[1]
    omega2, nu = np.full(n_u, np.nan), np.full(n_u, np.nan)
    omega2[kept], nu[kept] = inp["omega2"], per_sample["nu"]
    mc_parts, pf_parts, ci = [], [], None
    for name, pm in zip(components, p):
        if not pm > 0:
            mc_parts.append(None)
            pf_parts.append(None)
            continue
        if name == "null":
            w, profiles, live = np.ones(1), [np.ones(n_u)], [0]
        else:
            wt = R.weights(rows_by_table[name])
            live = np.flatnonzero(wt > 0)
            w, profiles = wt[live], inp["profiles_" + name][live]
        cbar, W, S2 = np.zeros(k), np.zeros((k, k)), np.zeros((k, k))
        F1, F2, FW, FD = np.zeros(n_u), np.zeros(n_u), np.zeros(n_u), np.zeros(n_u)
        if name != "null":
            ci = np.full((wt.size, k), np.nan)
        for wi, a, i in zip(w, profiles, live):
            c, Sig, t, s = per_sample[name][i]
            if name != "null":
                ci[i] = c
            cbar += wi * c
            W += wi * Sig
            S2 += wi * np.outer(c, c)
            f = a * t
            F1 += wi * f
            F2 += wi * f * f
            FW += wi * a * a * s
            FD += wi * (a * a * omega2 + nu)
        mc_parts.append(dict(cbar=cbar, W=W, S2=S2))
        pf_parts.append(dict(F1=F1, F2=F2, FW=FW, FD=FD))
    c, W, V = MR.mix(mc_parts, p)
    M_all = inp["M_all"]
    out = dict(continuum_mean=inp["mu_all"] + M_all @ c, continuum_var=np.einsum("pi,ij,pj->p", M_all, W + V, M_all),
               continuum_var_between=np.einsum("pi,ij,pj->p", M_all, V, M_all), coef_mean=c, coef_cov_within=MR.vech(W),
               coef_cov_between=MR.vech(V))
    out.update(PR.mix(pf_parts, p))
    if sample_coefficients:
        out["sample_coefficients"] = ci
    return out


# ---------------------------------------------------------------- the same in mpmath

def _mpf_list(mp, a):
    return [mp.mpf(x) for x in np.asarray(a, dtype=np.float64).tolist()]


def exact_sample(inp_rows, mu_all, M_all, a_full, kept, dps: int = DPS) -> dict:
    """One sample (``a_full`` of ones: the null model) at ``dps`` digits: c [k], Sigma as its packed lower triangle, and
    on the whole grid t = mu + m'c, s = m' Sigma m and d = a^2 omega2 + nu (None on masked pixels), as lists of mpf."""
    import mpmath as mp
    with mp.workdps(dps):
        y, mu, M, omega2, nu = inp_rows
        k = M.shape[1]
        idx = np.flatnonzero(kept)
        a_all = _mpf_list(mp, a_full)
        a = [a_all[p] for p in idx]
        y, mu, omega2, nu = (_mpf_list(mp, v) for v in (y, mu, omega2, nu))
        cols = [_mpf_list(mp, M[:, j]) for j in range(k)]
        d = [ai * ai * o + n for ai, o, n in zip(a, omega2, nu)]
        q = [ai * ai / di for ai, di in zip(a, d)]
        v = [ai * (yi - ai * mi) / di for ai, yi, mi, di in zip(a, y, mu, d)]
        B = mp.matrix(k, k)
        for i in range(k):
            qcol = [qi * m for qi, m in zip(q, cols[i])]
            for j in range(i + 1):
                B[i, j] = B[j, i] = mp.fdot(qcol, cols[j]) + (1 if i == j else 0)
        Sig = mp.inverse(B)
        Sig = [[(Sig[i, j] + Sig[j, i]) / 2 for j in range(k)] for i in range(k)]
        u = [mp.fdot(cols[i], v) for i in range(k)]
        c = [mp.fdot(Sig[i], u) for i in range(k)]
        t, s = [], []
        for p in range(M_all.shape[0]):
            m = _mpf_list(mp, M_all[p])
            t.append(mp.mpf(float(mu_all[p])) + mp.fdot(m, c))
            s.append(mp.fdot(m, [mp.fdot(Sig[i], m) for i in range(k)]))
        dn = [None] * len(a_all)
        for pos, p in enumerate(idx):
            dn[p] = d[pos]
        return dict(c=c, Sig=[Sig[i][j] for i in range(k) for j in range(i + 1)], t=t, s=s, dn=dn, a=a_all)


def exact_weights(row, dps: int = DPS):
    """(live indices, their weights as mpf): the softmax of ``R.weights``; the samples whose fp64 weight is exactly 0
    (every DEAD one) are not live."""
    import mpmath as mp
    live = np.flatnonzero(R.weights(row) > 0)
    with mp.workdps(dps):
        top = mp.mpf(float(np.nanmax(row)))
        e = [mp.exp(mp.mpf(float(row[i])) - top) for i in live]
        total = mp.fsum(e)
        return live, [x / total for x in e]


def exact_products(per_sample, rows_by_table, p, mu_all, M_all, dps: int = DPS, raw: bool = False,
                   components=MR.COMPONENTS) -> dict:
    """The products of one (row, mixture) from ``exact_sample`` results ({"null": [one], table: {index: result}}),
    rounded to fp64 at the very end (``raw``: the mpf lists themselves).  ``components``: the names behind ``p``."""
    import mpmath as mp
    with mp.workdps(dps):
        total = mp.fsum(mp.mpf(float(x)) for x in p)
        pm_all = [mp.mpf(float(x)) / total for x in p]
        k, n_u = M_all.shape[1], M_all.shape[0]
        nb = k * (k + 1) // 2
        zero = mp.mpf(0)
        c, W, S2 = [zero] * k, [zero] * nb, [zero] * nb
        F1, F2, FW, FD = [zero] * n_u, [zero] * n_u, [zero] * n_u, [zero] * n_u
        masked = None
        for name, pm in zip(components, pm_all):
            if not pm > 0:
                continue
            if name == "null":
                pairs = [(mp.mpf(1), per_sample["null"][0])]
            else:
                live, w = exact_weights(rows_by_table[name], dps)
                pairs = [(wi, per_sample[name][int(i)]) for i, wi in zip(live, w)]
            for wi, r in pairs:
                pw = pm * wi
                ci = r["c"]
                c = [x + pw * y for x, y in zip(c, ci)]
                W = [x + pw * y for x, y in zip(W, r["Sig"])]
                cc = [ci[i] * ci[j] for i in range(k) for j in range(i + 1)]
                S2 = [x + pw * y for x, y in zip(S2, cc)]
                f = [ai * ti for ai, ti in zip(r["a"], r["t"])]
                F1 = [x + pw * fi for x, fi in zip(F1, f)]
                F2 = [x + pw * fi * fi for x, fi in zip(F2, f)]
                FW = [x + pw * ai * ai * si for x, ai, si in zip(FW, r["a"], r["s"])]
                masked = [dn is None for dn in r["dn"]]
                FD = [x + pw * (dn if dn is not None else 0) for x, dn in zip(FD, r["dn"])]
        V = [S2[i * (i + 1) // 2 + j] - c[i] * c[j] for i in range(k) for j in range(i + 1)]

        def full(packed):
            return [[packed[max(i, j) * (max(i, j) + 1) // 2 + min(i, j)] for j in range(k)] for i in range(k)]
        Vf, Tf = full(V), full([w_ + v_ for w_, v_ in zip(W, V)])
        mean, var, btw = [], [], []
        for px in range(n_u):
            m = _mpf_list(mp, M_all[px])
            mean.append(mp.mpf(float(mu_all[px])) + mp.fdot(m, c))
            var.append(mp.fdot(m, [mp.fdot(Tf[i], m) for i in range(k)]))
            btw.append(mp.fdot(m, [mp.fdot(Vf[i], m) for i in range(k)]))
        fb = [b - a_ * a_ for a_, b in zip(F1, F2)]
        out = dict(continuum_mean=mean, continuum_var=var, continuum_var_between=btw, coef_mean=c, coef_cov_within=W,
                   coef_cov_between=V, flux_mean=F1, flux_var=[x + y for x, y in zip(FW, fb)], flux_var_within=FW,
                   flux_var_between=fb, noise_var=[mp.nan if dead else x for x, dead in zip(FD, masked)])
        if raw:
            return out
        return {n: np.array([float(x) for x in v]) for n, v in out.items()}


def exact_rows(results, S: int) -> np.ndarray:
    """[S, k] of c_i rounded to fp64 from {index: exact_sample result}; NaN rows where there is none"""
    k = len(next(iter(results.values()))["c"])
    out = np.full((S, k), np.nan)
    for i, r in results.items():
        out[int(i)] = [float(x) for x in r["c"]]
    return out


def live_rows(ci_all, row) -> np.ndarray:
    """``sample_coefficients`` as the library returns them: c_i of the samples of weight > 0, NaN rows elsewhere"""
    out = np.array(ci_all, dtype=np.float64)
    out[~(R.weights(row) > 0)] = np.nan
    return out


# ---------------------------------------------------------------- the error measure and the bound

def error(got, exact) -> float:
    """max |got - exact| / max(1, max |exact|); inf where the NaN patterns or shapes differ"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    if got.shape != exact.shape or not np.array_equal(np.isnan(got), np.isnan(exact)):
        return float("inf")
    ok = ~np.isnan(exact)
    if not ok.any():
        return 0.0
    worst = float(np.abs(got[ok] - exact[ok]).max())
    return worst / max(1.0, float(np.abs(exact[ok]).max())) if np.isfinite(worst) else float("inf")


def rel_error(got, exact) -> float:
    """the worst per-entry |got - exact| / |exact| (products bounded away from 0)"""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    if got.shape != exact.shape or not np.array_equal(np.isnan(got), np.isnan(exact)):
        return float("inf")
    ok = ~np.isnan(exact)
    worst = float((np.abs(got[ok] - exact[ok]) / np.abs(exact[ok])).max())
    return worst if np.isfinite(worst) else float("inf")


def tolerance(e_restatement: float) -> float:
    return max(TOL_FACTOR * e_restatement, TOL_FLOOR)


def figures(got: dict, exact: dict, restatement: dict) -> list:
    """[(label, e_restatement of the family, e_got, tolerance)] for every product of ``exact`` that ``got`` has to carry,
    scaled measure first, then the per-pixel relative one ("<product> rel") of REL_PRODUCTS; the family's e_restatement
    is the largest over the family's products present."""
    e_rest = {n: error(restatement[n], exact[n]) for n in exact}
    r_rest = {n: rel_error(restatement[n], exact[n]) for n in exact if n in REL_PRODUCTS}
    out = []
    for n in exact:
        fam = max(e_rest[m] for m in FAMILIES[FAMILY_OF[n]] if m in e_rest)
        out.append((n, fam, error(got[n], exact[n]), tolerance(fam)))
    for n in r_rest:
        fam = max(r_rest[m] for m in FAMILIES[FAMILY_OF[n]] if m in r_rest)
        out.append((n + " rel", fam, rel_error(got[n], exact[n]), tolerance(fam)))
    return out


def failures(label: str, figs: list) -> list:
    return [f"{label} {n}: error {e:.3e} > {tol:.3e} = max(10 x {er:.3e}, 1e-12)" for n, er, e, tol in figs if not e <= tol]


def ratio(e, e_rest):
    return e / e_rest if e_rest > 0 else float("inf")


# ---------------------------------------------------------------- the fixture

def save_npz(path, arrays: dict):
    """np.savez_compressed with fixed member dates, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def load_fixture(golden) -> dict:
    """{class name: {key: array}} of both files; "<key>@" holds where an array stored once lives: a full key of these
    files, or PARENT + a full key of tests/golden/exact_hard_conditioning.npz"""
    parent = golden(H.FIXTURE)
    files = [golden(name) for name in FIXTURES]
    flat = {full: z[full] for z in files for full in z.files}
    out = {}
    for full, v in flat.items():
        name, key = full.split("/", 1)
        if key.endswith("@"):
            ref = str(v)
            v = parent[ref[len(PARENT):]] if ref.startswith(PARENT) else flat[ref]
        out.setdefault(name, {})[key.rstrip("@")] = v
    return out


def stored_inputs(entry: dict, cls) -> dict:
    return {key: entry[key] for key in INPUT_KEYS + tuple("profiles_" + t for t in tables_of(cls))}


def stored_rows(entry: dict, cls, row: str) -> dict:
    return {t: entry[f"row/{t}/{row}"] for t in tables_of(cls)}


def stored_exact(entry: dict, cls, row: str, mix: int) -> dict:
    """the exact products of (row, mixture number), ``sample_coefficients`` among them where the mixture asks for them"""
    prefix = f"exact/{row}/{mix}/"
    out = {key[len(prefix):]: v for key, v in entry.items() if key.startswith(prefix)}
    if mixtures_of(cls)[mix][1]:
        out["sample_coefficients"] = live_rows(entry["exact_sample_coefficients"], entry[f"row/dla/{row}"])
    return out
