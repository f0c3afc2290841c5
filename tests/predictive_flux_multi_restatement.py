"""NumPy-and-oracle restatement of the posterior predictive flux over all models of a multi-DLA run (a
plain module beside tests/marginal_continuum_multi_restatement.py, whose components, live samples and model weights these
are; the per-sample arithmetic and the mixture of the four sums are tests/predictive_flux_restatement.py's).
"""
from __future__ import annotations

import numpy as np

import marginal_continuum_multi_restatement as MMR
import predictive_flux_restatement as PR
from predictive_flux_restatement import PRODUCTS, PRODUCTS_MEAN, PRODUCTS_VAR, deviation, tolerances  # noqa: F401  (re-exported)


def reduce_component(rows, mu_all, M_all, omega2, nu, kept, profiles, form: str) -> dict:
    """F1, F2, FW, FD of [(w_i, a_i on the whole grid)] in list order (``PR.component``'s sums) and the (w, a, t, s) list."""
    n_u = mu_all.size
    F1, F2, FW, FD = np.zeros(n_u), np.zeros(n_u), np.zeros(n_u), np.zeros(n_u)
    pairs = []
    for wi, a in profiles:
        t, s, f = PR.per_sample(rows, mu_all, M_all, a, kept, form)
        F1 += wi * f
        F2 += wi * f * f
        FW += wi * a * a * s
        FD += wi * (a * a * omega2 + nu)
        pairs.append((wi, a, t, s))
    return dict(F1=F1, F2=F2, FW=FW, FD=FD, pairs=pairs)


def parts_of(oracle, model, g, samples, tables, p, meanflux: bool, num_lines: int, form: str, cache=None):
    """(parts, flags) as ``MMR.parts_of``: per component (null first) its four sums where the weight is positive."""
    md = p.size - 2
    mu_all, M_all, omega2, nu, rows = PR.grid_rows(oracle, model, g, meanflux)
    args = (rows, mu_all, M_all, omega2, nu, g["kept"])
    parts, flags = [reduce_component(*args, [(1.0, np.ones(g["n_u"]))], form) if p[0] > 0 else None], 0
    for comp, pm in zip(MMR.components(md), p[1:]):
        live = MMR.live_samples(oracle, g, samples, tables, comp, num_lines, cache) if pm > 0 else None
        if pm > 0 and live is None:
            flags |= MMR.flag_bit(comp)
        parts.append(reduce_component(*args, [(w, a) for _i, w, a in live], form) if live is not None else None)
    return parts, flags


def predictive_flux_multi(oracle, model, g, samples, tables: dict, P, meanflux: bool, num_lines: int = 3, form: str = "dense",
                          cache=None) -> dict:
    """Everything gpdla_batch_predictive_flux_multi returns for one quasar.  ``P``: (null, sub-DLA, DLA(1..md)) weights,
    not yet normalised."""
    nan = {name: np.full(g["n_u"], np.nan) for name in PRODUCTS}
    undefined = bool(np.isnan(np.asarray(P, dtype=np.float64)).any())
    if "pad" not in g:
        return dict(nan, status=1, model_flags=0 if undefined else MMR.component_flags(tables, MMR.normalised(P)))
    if undefined:
        return dict(nan, status=MMR.UNDEFINED, model_flags=0)
    p = MMR.normalised(P)
    parts, flags = parts_of(oracle, model, g, samples, tables, p, meanflux, num_lines, form, cache)
    if flags:
        return dict(nan, status=0, model_flags=flags)
    return dict(PR.mix(parts, p), status=0, model_flags=0)


def disagreement(dense: list, woodbury: list) -> dict:
    return {name: max(deviation(d[name], w[name]) for d, w in zip(dense, woodbury)) for name in PRODUCTS}
