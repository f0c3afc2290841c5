"""The fields of the grid products -- model spectra, marginal continuum, predictive flux, absorption distribution (DESIGN.md
4.12, 4.21, 4.23-4.25, 4.28, 4.29) -- declared once: the drivers of :mod:`api` stitch their blocks by this table and the savers of :mod:`io` write their
files by it, so a field is returned and saved, or neither.  No package imports: both modules import it.

A result holds ``offsets [n + 1]`` and ``status [n]`` (and, refined, ``boxes`` and ``refine_status``), then these fields.
Quasar s of the selection owns pixels ``[offsets[s], offsets[s + 1])`` of its ``total`` grid pixels.

=========  =========================================  ==========================================================
kind       shape                                      in a file
=========  =========================================  ==========================================================
``pixel``  ``[total]``, joined along the last axis     a cell of column vectors
``plane``  ``[D, total]``, last axis                   a cell of ``[pixels x D]`` matrices
``row``    ``[n, *trailing]``, joined along axis 0     a matrix; a cell of matrices for two trailing dimensions
``column`` ``[n]`` of ``dtype``                        a column
=========  =========================================  ==========================================================

``leading`` names the first dimension D of a plane: ``thresholds``, ``levels``, ``bins`` (the absorption distribution's, what
the call asked for); a plane without a name has ``max_dlas`` rows.
``trailing`` names the dimensions of a row after the first: ``k`` (the rank), ``tri`` (k (k + 1) / 2, a packed lower
triangle), ``samples`` (S, or the S' refine points where the DLA component runs on the refined table); None: the caller's.
``option``: the switch of the call that asks for the field (None: always); ``"caller"``: no driver returns it, the
command line adds it before it saves.  The order within a product is the order in the file.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

Field = namedtuple("Field", "product name kind dtype trailing option leading", defaults=(None,))


def _f(product, name, kind, dtype=np.float64, trailing=None, option=None, leading=None):
    return Field(product, name, kind, np.dtype(dtype), trailing, option, leading)


FIELDS = (
    _f("model_spectra", "map_absorption", "pixel", option="map"),
    _f("model_spectra", "mean_absorption", "pixel", option="moments"),
    _f("model_spectra", "var_absorption", "pixel", option="moments"),
    _f("model_spectra", "continuum", "pixel", option="continuum"),
    _f("model_spectra", "model_flux", "pixel", option="continuum"),
    # what multi_models adds to the model spectra
    _f("model_spectra_multi", "mean_absorption_lls", "pixel"),
    _f("model_spectra_multi", "var_absorption_lls", "pixel"),
    _f("model_spectra_multi", "expected_absorption", "pixel"),
    _f("model_spectra_multi", "expected_var_absorption", "pixel"),
    _f("model_spectra_multi", "mean_absorption_models", "plane"),
    _f("model_spectra_multi", "var_absorption_models", "plane"),
    _f("marginal_continuum", "continuum_mean", "pixel"),
    _f("marginal_continuum", "continuum_var", "pixel"),
    _f("marginal_continuum", "continuum_var_between", "pixel"),
    _f("marginal_continuum", "coef_mean", "row", trailing=("k",)),
    _f("marginal_continuum", "coef_cov_within", "row", trailing=("tri",)),
    _f("marginal_continuum", "coef_cov_between", "row", trailing=("tri",)),
    _f("marginal_continuum", "model_weights", "row", option="caller"),
    _f("marginal_continuum", "sample_coefficients", "row", trailing=("samples", "k"), option="sample_coefficients"),
    _f("predictive_flux", "flux_mean", "pixel"),
    _f("predictive_flux", "flux_var", "pixel"),
    _f("predictive_flux", "flux_var_within", "pixel"),
    _f("predictive_flux", "flux_var_between", "pixel"),
    _f("predictive_flux", "noise_var", "pixel"),
    _f("predictive_flux", "residual", "pixel", option="residuals"),
    _f("predictive_flux", "chi2", "column", option="residuals"),
    _f("predictive_flux", "num_kept", "column", np.int64, option="residuals"),
    _f("predictive_flux", "model_weights", "row", option="caller"),
    # the absorption distribution
    _f("absorption_distribution", "prob_below", "plane", leading="thresholds"),
    _f("absorption_distribution", "absorption_min", "pixel"),
    _f("absorption_distribution", "absorption_max", "pixel"),
    _f("absorption_distribution", "quantiles", "plane", option="levels", leading="levels"),
    _f("absorption_distribution", "histogram", "plane", option="histogram", leading="bins"),
    _f("absorption_distribution", "model_weights", "row", option="caller"),
    # every multi_models form: a result carries it right after ``status``, a file holds it last
    _f("multi_models", "model_flags", "column", np.uint32),
)


def fields(product: str, kind: str | None = None, options=None) -> tuple:
    """The fields of ``product`` in file order: of one ``kind`` (None: any) and asked for by one of ``options`` (a None
    among them: the fields every call returns; ``options=None``: whatever asks for them)."""
    return tuple(f for f in FIELDS if f.product == product and kind in (None, f.kind) and (options is None or f.option in options))


def requested(product: str, switches=()) -> tuple:
    """The fields a call of ``product`` returns with the ``switches`` that are on."""
    return fields(product, options=(None,) + tuple(switches))


def names(*args, **kw) -> tuple:
    return tuple(f.name for f in fields(*args, **kw))


def join(field: Field, parts: list) -> np.ndarray:
    """The blocks' arrays of ``field`` as one, in block order."""
    return np.concatenate(parts, axis=0 if field.kind in ("row", "column") else -1).astype(field.dtype, copy=False)


def empty(field: Field, dims: dict) -> np.ndarray:
    """``field`` of an empty selection; ``dims``: ``k``, ``samples`` and ``max_dlas`` (and the named leading dimension of a
    plane that has one)."""
    sizes = dict(dims, tri=dims["k"] * (dims["k"] + 1) // 2)
    shape = {"pixel": (0,), "column": (0,), "plane": (dims[field.leading or "max_dlas"], 0),
             "row": (0,) + tuple(sizes[d] for d in field.trailing or ())}[field.kind]
    return np.zeros(shape, dtype=field.dtype)
