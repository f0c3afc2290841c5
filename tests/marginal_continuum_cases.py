"""The shapes at which the marginal-continuum kernels (csrc/marginal_continuum_kernels.hpp) take another path, as case
lists and builders shared by tests/test_marginal_continuum.py (CPU) and tests/test_gpu_marginal_continuum.py.  A plain
module, like model_spectra_edge_cases.py.

n_u is the number of pixels of a quasar's unmasked-range grid (``synthetic.make_spectrum(index, n, ...)``: n_u = n),
S the number of samples, k the rank.  The restatement of a setup is computed once (``wanted``) and shared.
"""
import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import marginal_continuum_restatement as MR
import model_spectra_edge_cases as E
import model_spectra_restatement as R
import production_shapes as ps

# The kernels' own constants (tests/test_marginal_continuum.py reads them back from the sources).
SOLVE_CHUNK = 64            # kMcSolveChunk: z-order positions per block of k_mc_solve
CONTRACT = {20: dict(samples=64, pixels=32), 40: dict(samples=16, pixels=64)}   # k <= 20, k <= 40: k_mc_contract<RT, CPW, PT>
FINISH_TILE = 64            # kMcPixTile
RANKS = (1, 2, 20, 21, 22, 23, 40)     # the LDS-slot straddles of DESIGN 4.12; 230 and 860 columns at k = 20 and 40


def contract_shape(k: int) -> dict:
    return CONTRACT[20 if k <= 20 else 40]


def pixel_counts(k: int):
    pt = contract_shape(k)["pixels"]
    return (1, 2, 3, 4, 5, pt - 1, pt, pt + 1, 257)


# One setup = one batch and one call: (name, k, S, n_u list or production strata, num_lines, multi (mean-flux rows, a multi-DLA
# batch), table).  Every rank, every pixel count of both tile widths, S = 1, 63, 64, 65 (the k <= 20 sample chunk and the solve
# chunk +- 1), 15, 16, 17 (the k > 20 sample chunk +- 1) and 513, 3 and 31 lines, both kinds of rows, both tables.  The dense
# restatement costs n_kept^3 per sample: 257 pixels meet S = 513 once, the production shapes (~1000 pixels) meet S = 17.
SETUPS = (
    dict(name="k20_S513", k=20, S=513, nus=pixel_counts(20), lines=3, multi=False, table="dla"),
    dict(name="k40_S65_meanflux", k=40, S=65, nus=pixel_counts(40), lines=3, multi=True, table="dla"),
    dict(name="k1_S1", k=1, S=1, nus=(1, 2, 33), lines=3, multi=False, table="dla"),
    dict(name="k2_S63", k=2, S=63, nus=(1, 5, 33), lines=3, multi=False, table="dla"),
    dict(name="k21_S64_lls_31lines", k=21, S=64, nus=(3, 63, 65), lines=31, multi=False, table="sub_dla"),
    dict(name="k22_S15_meanflux_lls", k=22, S=15, nus=(4, 64, 65), lines=3, multi=True, table="sub_dla"),
    dict(name="k23_S17", k=23, S=17, nus=(2, 63, 129), lines=3, multi=False, table="dla"),
    dict(name="k20_S16_31lines_meanflux", k=20, S=16, nus=(5, 31, 33), lines=31, multi=True, table="dla"),
    dict(name="k40_S513", k=40, S=513, nus=(5, 65), lines=3, multi=False, table="dla"),
    dict(name="k20_production_shapes", k=20, S=17, nus=("tile_boundary_run", "both_ends_masked_runs", "confined_40px"), lines=3,
         multi=False, table="dla"),
    dict(name="k40_confined_fewer_kept_than_k", k=40, S=17, nus=("confined_40px",), lines=3, multi=True, table="dla"),
)


def setup(name: str) -> dict:
    return next(s for s in SETUPS if s["name"] == name)


def params(st):
    return MultiParameters(max_dlas=2, num_lines=st["lines"]) if st["multi"] else Parameters(num_lines=st["lines"])


def build(st):
    """(model, samples, spectra) of a setup; from 31 pixels up every second synthetic quasar is masked at 5 %."""
    k = st["k"]
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(st["S"])
    spectra = []
    strat = None
    for i, n in enumerate(st["nus"]):
        if isinstance(n, str):
            strat = strat or ps.stratified_quasars(k)
            spectra.append(strat[ps.by_stratum(strat, n)])
        else:
            spectra.append(synthetic.make_spectrum(6100 + 2 * i + 40 * k, n, model, mask_fraction=0.05 if (i % 2 and n >= 31) else 0.0))
    return model, samples, spectra


_WANTED = {}


def wanted(oracle, key, model, samples, spectra, tables, p, meanflux: bool, lines: int, forms=("dense", "woodbury")):
    """Per quasar the restatement in both forms, once per ``key``: {form: [dict per quasar]}.  ``tables``: {name: [nq, S]};
    ``p``: [nq, 3] or one row."""
    if key not in _WANTED:
        p = np.broadcast_to(np.asarray(p, dtype=np.float64), (len(spectra), 3))
        grids = [R.grid(oracle, model, sp) for sp in spectra]
        out = {}
        for form in forms:
            out[form] = [MR.marginal_continuum(oracle, model, g, samples, {n: t[q] for n, t in tables.items()}, p[q], meanflux,
                                               lines, form) for q, g in enumerate(grids)]
        _WANTED[key] = out
    return _WANTED[key]


def disagreement(want) -> dict:
    """The worst dense-vs-Woodbury disagreement per product over the quasars of ``wanted``."""
    out = {}
    for name in MR.PRODUCTS_COEF + MR.PRODUCTS_COV:
        out[name] = max(MR.deviation(d[name], w[name]) for d, w in zip(want["dense"], want["woodbury"]))
    return out


def tolerances(dis: dict) -> dict:
    """R.continuum_tolerance: per product family, 10 x the disagreement of that family, floored at 1e-12, capped at 1e-8."""
    coef = R.continuum_tolerance(max(dis[n] for n in MR.PRODUCTS_COEF))
    cov = R.continuum_tolerance(max(dis[n] for n in MR.PRODUCTS_COV))
    return {**{n: coef for n in MR.PRODUCTS_COEF}, **{n: cov for n in MR.PRODUCTS_COV}}


def split(res, k: int, with_samples: bool = True) -> list:
    """What Batch.marginal_continuum returns as one dict per selected quasar, in the restatement's layout."""
    off = res["offsets"]
    out = []
    for s in range(off.size - 1):
        d = {n: res[n][off[s]:off[s + 1]] for n in ("continuum_mean", "continuum_var", "continuum_var_between")}
        d.update({n: res[n][s] for n in ("coef_mean", "coef_cov_within", "coef_cov_between")})
        if with_samples and "sample_coefficients" in res:
            d["sample_coefficients"] = res["sample_coefficients"][s]
        d["status"] = int(res["status"][s])
        out.append(d)
    return out


# ---- weight rows ----

ROW_SETUPS = (dict(k=20, S=130, nus=(33, 65)), dict(k=40, S=33, nus=(5, 65)))


def row_hot_positions(k: int, S: int):
    c = contract_shape(k)["samples"]
    return sorted({p for p in (0, 63, 64, c - 1, c, S - 1) if p < S})


def row_kinds(k: int, S: int):
    return ["sweep", "flat", "half_nan"] + [("hot", p) for p in row_hot_positions(k, S)] + list(E.NAN_ROWS)


# ---- the batching of the module-level drivers (api.marginal_continuum, api.predictive_flux) ----

BATCHING_NUS = (5, 31, 33, 17, 64)          # five quasars of unequal length
# a permutation with quasar 2 left out (blocks of 2, 2 at two a batch), and one of all five (2, 2 and a short last block)
BATCHING_SELECTIONS = {"one_left_out": (3, 0, 4, 1), "all_five": (3, 0, 4, 1, 2)}


def batching_case(k: int = 20):
    """(model, samples, spectra, params, log_priors) of the smallest k = 20 setup (S = 16, 31 lines, mean-flux rows of a
    multi-DLA run, so that all three components have a table and a posterior) on BATCHING_NUS; ``k`` replaces its rank."""
    st = dict(setup("k20_S16_31lines_meanflux"), k=k, nus=BATCHING_NUS)
    model, samples, spectra = build(st)
    p = params(st)
    n = len(spectra)
    log_priors = (np.full(n, np.log(0.85)), np.full(n, np.log(0.05)), np.log(np.full((n, p.max_dlas), 0.1) ** np.arange(1, p.max_dlas + 1)))
    return model, samples, spectra, p, log_priors


def assert_same_results(a: dict, b: dict):
    """Every returned array bit for bit (NaN equal to NaN), with its dtype and shape."""
    assert list(a) == list(b)
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), name


# ---- the zero-weight skip ----

SKIP_S, SKIP_LIVE = 200, (3, 70, 199)      # z-order positions of the three samples of weight > 0 (blocks 0, 1 and 3 of 4)
SKIP_POISON = 71                           # z-order position of the zero-weight sample whose column density is NaN


def skip_row(samples) -> np.ndarray:
    order = E.z_order(samples)
    row = np.full(SKIP_S, -1e6)
    row[order[list(SKIP_LIVE)]] = (-1.0, 0.0, -2.5)
    return row
