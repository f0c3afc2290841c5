"""NumPy-and-oracle restatement of the marginal continuum over all models of a multi-DLA run (a plain
module: tests/test_mixture_multi.py and tests/test_gpu_mixture_multi.py import it; no package compute code is used).

Everything per sample is tests/marginal_continuum_restatement.py's (the dense and the Woodbury form, the reduction over the
samples of a component, the per-pixel arrays); the profiles, the slots and the weights of model DLA(n) are
tests/model_spectra_multi_restatement.py's.  What is new is the list of components -- (null, sub-DLA, DLA(1), ..,
DLA(max_dlas)) -- and the mixture over them:

* component "sub_dla": the profiles of ``lls_nhi_samples``, the weights of ``sample_log_likelihoods_lls``;
* component n:         A_{n,i} = Prod_j C[s_j(i)] in slot order, C the broadened profiles of ``nhi_samples``; the weights
                       of row n - 1 of ``sample_log_likelihoods_dla`` with a NaN where a slot was never drawn;
* model weights P = (P_null, P_lls, P_1 .. P_md) normalised by their sum; a NaN entry: NaN rows, status 8; a component of
  positive weight without weights: NaN rows, status 0, its bit in model_flags.

``tables`` of one quasar: ``sample_log_likelihoods_dla [max_dlas, S]``, ``base_sample_inds [max_dlas - 1, S]``,
``sample_log_likelihoods_lls [S]``.
"""
from __future__ import annotations

import numpy as np

import marginal_continuum_restatement as MR
import model_spectra_multi_restatement as RM
import model_spectra_restatement as R

FLAG_LLS = 0x40000000           # GPDLA_SPECTRA_MULTI_FLAG_LLS
UNDEFINED = 8                   # GPDLA_SPECTRA_AVERAGE_UNDEFINED
ARRAYS = ("continuum_mean", "continuum_var", "continuum_var_between")
ROWS = ("coef_mean", "coef_cov_within", "coef_cov_between")
PRODUCTS_COEF = ("coef_mean", "continuum_mean")
PRODUCTS_COV = MR.PRODUCTS_COV


def components(md: int) -> tuple:
    """The sampled components in mixture order: "sub_dla", then the model numbers 1 .. md."""
    return ("sub_dla",) + tuple(range(1, md + 1))


def flag_bit(comp) -> int:
    return FLAG_LLS if comp == "sub_dla" else 1 << (comp - 1)


def effective_row(tables: dict, comp) -> np.ndarray:
    """The component's row of log-likelihoods, NaN where a slot of the sample was never drawn."""
    if comp == "sub_dla":
        return np.array(tables["sample_log_likelihoods_lls"], dtype=np.float64)
    return RM.effective_row(tables["sample_log_likelihoods_dla"][comp - 1], tables.get("base_sample_inds"), comp)


def live_samples(oracle, g, samples, tables: dict, comp, num_lines: int, cache: dict | None = None):
    """[(i, w_i, a_i on the whole grid)] of the samples of weight > 0 in index order, or None: the row has no weights.  A
    sample of weight exactly 0 is never touched.  ``cache``: the gathered profiles, kept between calls for ONE quasar."""
    ll = effective_row(tables, comp)
    if RM.flagged(ll):
        return None
    w = R.weights(ll)
    live = np.flatnonzero(w > 0)
    if comp == "sub_dla":
        z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.asarray(samples["offset_samples"])
        return [(i, w[i], oracle.voigt(g["pad"], z[i], samples["lls_nhi_samples"][i], num_lines)) for i in live]
    cache = {} if cache is None else cache
    z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.asarray(samples["offset_samples"])

    def profile(j):     # RM.sample_profiles' row j, formed when a live sample first gathers it
        if j not in cache:
            cache[j] = oracle.voigt(g["pad"], z[j], samples["nhi_samples"][j], num_lines)
        return cache[j]
    out = []
    for i in live:
        s = RM.slots(tables.get("base_sample_inds"), comp, i)
        a = profile(s[0])
        for sj in s[1:]:
            a = a * profile(sj)
        out.append((i, w[i], a))
    return out


def component_flags(tables: dict, p) -> int:
    """The model_flags word: the components of positive weight whose row has no weights (whatever the quasar's status)."""
    flags = 0
    for comp, pm in zip(components(len(p) - 2), p[1:]):
        if pm > 0 and RM.flagged(effective_row(tables, comp)):
            flags |= flag_bit(comp)
    return flags


def reduce_component(rows, kept, live, form: str) -> dict:
    """cbar, W, S2 = Sum w c c' of one sampled component (``MR.sampled_component``'s sums), and its (w, c, Sigma) list."""
    k = rows[2].shape[1]
    solve = MR.sample_dense if form == "dense" else MR.sample_woodbury
    cbar, W, S2 = np.zeros(k), np.zeros((k, k)), np.zeros((k, k))
    pairs = []
    for _i, w, a in live:
        c, Sig = solve(*rows, a[kept])
        cbar += w * c
        W += w * Sig
        S2 += w * np.outer(c, c)
        pairs.append((w, c, Sig))
    return dict(cbar=cbar, W=W, S2=S2, pairs=pairs)


def normalised(P) -> np.ndarray:
    P = np.asarray(P, dtype=np.float64)
    return P / P.sum()


def parts_of(oracle, model, g, samples, tables, p, meanflux: bool, num_lines: int, form: str, cache=None):
    """(parts, flags): per component (null first) its dict where the weight is positive (None otherwise), and the
    model_flags word -- the components of positive weight whose row has no weights."""
    md = p.size - 2
    rows = MR.prepared_rows(oracle, model, g, meanflux)
    parts, flags = [], 0
    if p[0] > 0:
        null = MR.null_component(rows, form)
        parts.append(dict(null, pairs=[(1.0, null["cbar"], null["W"])]))
    else:
        parts.append(None)
    for comp, pm in zip(components(md), p[1:]):
        live = live_samples(oracle, g, samples, tables, comp, num_lines, cache) if pm > 0 else None
        if pm > 0 and live is None:
            flags |= flag_bit(comp)
        parts.append(reduce_component(rows, g["kept"], live, form) if live is not None else None)
    return parts, flags


def marginal_continuum_multi(oracle, model, g, samples, tables: dict, P, meanflux: bool, num_lines: int = 3, form: str = "dense",
                             cache=None) -> dict:
    """Everything gpdla_batch_marginal_continuum_multi returns for one quasar.  ``P``: (null, sub-DLA, DLA(1..md)) weights,
    not yet normalised."""
    k = np.asarray(model["M"]).shape[1]
    nb, n_u = k * (k + 1) // 2, g["n_u"]
    nan = dict(continuum_mean=np.full(n_u, np.nan), continuum_var=np.full(n_u, np.nan), continuum_var_between=np.full(n_u, np.nan),
               coef_mean=np.full(k, np.nan), coef_cov_within=np.full(nb, np.nan), coef_cov_between=np.full(nb, np.nan))
    undefined = bool(np.isnan(np.asarray(P, dtype=np.float64)).any())
    if "pad" not in g:
        return dict(nan, status=1, model_flags=0 if undefined else component_flags(tables, normalised(P)))
    if undefined:
        return dict(nan, status=UNDEFINED, model_flags=0)
    p = normalised(P)
    parts, flags = parts_of(oracle, model, g, samples, tables, p, meanflux, num_lines, form, cache)
    if flags:
        return dict(nan, status=0, model_flags=flags)
    c, W, V = MR.mix(parts, p)
    mean, var, btw = MR.on_grid(oracle, model, g, meanflux, c, W, V)
    return dict(continuum_mean=mean, continuum_var=var, continuum_var_between=btw, coef_mean=c, coef_cov_within=MR.vech(W),
                coef_cov_between=MR.vech(V), status=0, model_flags=0)


def disagreement(dense: list, woodbury: list) -> dict:
    """The worst dense-vs-Woodbury disagreement per product over a list of quasars."""
    return {name: max(MR.deviation(d[name], w[name]) for d, w in zip(dense, woodbury)) for name in PRODUCTS_COEF + PRODUCTS_COV}


def tolerances(dis: dict) -> dict:
    """R.continuum_tolerance per product family: 10 x the disagreement of that family, floored at 1e-12, capped at 1e-8."""
    coef = R.continuum_tolerance(max(dis[n] for n in PRODUCTS_COEF))
    cov = R.continuum_tolerance(max(dis[n] for n in PRODUCTS_COV))
    return {**{n: coef for n in PRODUCTS_COEF}, **{n: cov for n in PRODUCTS_COV}}
