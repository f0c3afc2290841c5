"""The shapes, base-index patterns and weight rows at which the marginal continuum and the predictive flux over all models
of a multi-DLA run (csrc/marginal_continuum_kernels.hpp, csrc/predictive_flux_kernels.hpp, csrc/host_mixture_multi.hpp) can go wrong, as case
lists and builders shared by tests/test_mixture_multi.py (CPU) and tests/test_gpu_mixture_multi.py.  A plain module beside
marginal_continuum_cases.py and model_spectra_multi_cases.py, whose builders it reuses.

One setup = one multi-DLA batch of 1 to 3 quasars and one call of each entry with weight on EVERY component, so every
axis value below meets every model n of a max_dlas = 4 setup:

    rank k          1, 2, 20, 21, 40                 both shapes of k_mc_contract(_multi) and their boundary
    grid pixels     1, 31, 32, 33, 63, 64, 65, 257   the 32- and 64-pixel tiles +- 1; one production-shape stratum
    samples S       1, 15, 16, 17, 63, 64, 65, 257, 513   the 16- and 64-sample blocks, the solve and list chunks +- 1
    max_dlas        2, 4;   lines 3, 31;   rows plain, mean-flux
    base indices    cyclic, all on one sample, seeded random, the two ends of the z order, some entries 0
    weight rows     as the sweep left them, flat, half NaN, one-hot at z-order positions 15 / 16 / 63 / 64 / 65 / S - 1,
                    no weights at all (one row kind per quasar, used for every model's row and the sub-DLA row)

The dense restatement costs n_kept^3 per live sample and component: 257 pixels meet S = 65, S = 257 and 513 meet short
grids, the production stratum is the one confined to 36 kept pixels of 1249.
"""
import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters

import marginal_continuum_multi_restatement as MMR
import model_spectra_edge_cases as E
import model_spectra_multi_cases as MSC
import model_spectra_restatement as R
import predictive_flux_multi_restatement as PMR
import production_shapes as ps

LAST = "last"       # ("hot", LAST): the one-hot row at z-order position S - 1

SETUPS = (
    dict(name="k20_S65_md4_cyclic", k=20, S=65, nus=(1, 31, 257), md=4, lines=3, meanflux=False, base="cyclic",
         kinds=("flat", "half_nan", "sweep")),
    dict(name="k40_S17_md4_random_meanflux", k=40, S=17, nus=(32, 33, 63), md=4, lines=3, meanflux=True, base="random",
         kinds=(("hot", 15), ("hot", 16), ("hot", LAST))),
    dict(name="k21_S16_md4_ends_31lines", k=21, S=16, nus=(64, 65), md=4, lines=31, meanflux=False, base="ends",
         kinds=("flat", "sweep")),
    dict(name="k2_S257_md4_one_meanflux", k=2, S=257, nus=(33, 65, 31), md=4, lines=3, meanflux=True, base="one",
         kinds=(("hot", 63), ("hot", 64), ("hot", 65))),
    dict(name="k1_S1_md4", k=1, S=1, nus=(1, 33), md=4, lines=3, meanflux=False, base="cyclic", kinds=("flat", "sweep")),
    dict(name="k20_S63_md4_zeros_meanflux", k=20, S=63, nus=(63,), md=4, lines=3, meanflux=True, base="zeros", kinds=("sweep",)),
    dict(name="k20_S64_md4_zeros", k=20, S=64, nus=(31, 64), md=4, lines=3, meanflux=False, base="zeros", kinds=("half_nan", "flat")),
    dict(name="k40_S15_md4_production_shape", k=40, S=15, nus=("confined_40px",), md=4, lines=3, meanflux=False, base="random",
         kinds=("flat",)),
    dict(name="k20_S513_md4_random", k=20, S=513, nus=(33,), md=4, lines=3, meanflux=False, base="random", kinds=("half_nan",)),
    dict(name="k20_S17_md4_no_weights", k=20, S=17, nus=(33,), md=4, lines=3, meanflux=True, base="cyclic", kinds=("none",)),
    dict(name="k20_S65_md2_ends_31lines_meanflux", k=20, S=65, nus=(32, 257, 33), md=2, lines=31, meanflux=True, base="ends",
         kinds=("sweep", "half_nan", "none")),
    dict(name="k40_S64_md2_one", k=40, S=64, nus=(1, 63), md=2, lines=3, meanflux=False, base="one", kinds=(("hot", LAST), "flat")),
    dict(name="k21_S257_md2_cyclic", k=21, S=257, nus=(65,), md=2, lines=3, meanflux=False, base="cyclic", kinds=("sweep",)),
)


def setup(name: str) -> dict:
    return next(s for s in SETUPS if s["name"] == name)


def params(st) -> MultiParameters:
    return MultiParameters(max_dlas=st["md"], num_lines=st["lines"])


def build(st):
    """(model, samples, spectra) of a setup; from 31 pixels up every second synthetic quasar is masked at 5 %."""
    k = st["k"]
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(st["S"])
    spectra, strat = [], None
    for i, n in enumerate(st["nus"]):
        if isinstance(n, str):
            strat = strat or ps.stratified_quasars(k)
            spectra.append(strat[ps.by_stratum(strat, n)])
        else:
            spectra.append(synthetic.make_spectrum(6700 + 2 * i + 40 * k, n, model, mask_fraction=0.05 if (i % 2 and n >= 31) else 0.0))
    return model, samples, spectra


def base_in(st, samples) -> np.ndarray:
    """base_sample_inds [nq, md - 1, S] a sweep is given, every entry drawn ("zeros": the seeded random rows)."""
    pattern = "random" if st["base"] == "zeros" else st["base"]
    return np.stack([MSC.base_rows(pattern, st["S"], st["md"], samples, seed=q) for q in range(len(st["nus"]))])


def zeroed(base: np.ndarray) -> np.ndarray:
    """... with every fifth sample never drawn in one of its slots (slot 2 + i mod (md - 1) of sample i = 2, 7, ..)."""
    out = base.copy()
    nrows, S = out.shape[1], out.shape[2]
    for i in range(2, S, 5):
        out[:, i % nrows, i] = 0
    return out


def synthetic_sweep(st):
    """Seeded tables in place of a sweep's (the CPU tests): (sample_log_likelihoods_dla [nq, md, S], ..._lls [nq, S])."""
    rng = np.random.default_rng(sum(map(ord, st["name"])))
    nq = len(st["nus"])
    return -1000.0 + 6.0 * rng.standard_normal((nq, st["md"], st["S"])), -1000.0 + 6.0 * rng.standard_normal((nq, st["S"]))


def row(kind, S: int, samples, sweep_row, which: int) -> np.ndarray:
    """One row of sample log-likelihoods; ``which`` numbers the component (the rows without weights take turns)."""
    if kind == "none":
        return E.moment_row(E.NAN_ROWS[which % len(E.NAN_ROWS)], S, samples, None)
    if isinstance(kind, tuple):
        return E.moment_row(("hot", S - 1 if kind[1] == LAST else kind[1]), S, samples, None)
    return E.moment_row(kind, S, samples, sweep_row)


def host_tables(st, samples, sweep_dla, sweep_lls) -> dict:
    """The host tables of the setup's call from a sweep's: each quasar's rows replaced by its row kind."""
    S, md = st["S"], st["md"]
    dla, lls = np.array(sweep_dla, dtype=np.float64), np.array(sweep_lls, dtype=np.float64)
    for q, kind in enumerate(st["kinds"]):
        lls[q] = row(kind, S, samples, sweep_lls[q], 0)
        for m in range(md):
            dla[q, m] = row(kind, S, samples, sweep_dla[q, m], 1 + m)
    base = base_in(st, samples)
    return dict(sample_log_likelihoods_dla=dla, base_sample_inds=zeroed(base) if st["base"] == "zeros" else base,
                sample_log_likelihoods_lls=lls)


def model_weights(st) -> np.ndarray:
    """[nq, 2 + md]: weight on every component, seeded, not normalised."""
    rng = np.random.default_rng(500 + sum(map(ord, st["name"])))
    return 0.05 + rng.random((len(st["nus"]), 2 + st["md"]))


def quasar_tables(tables: dict, q: int) -> dict:
    return {name: (None if t is None else np.asarray(t)[q]) for name, t in tables.items()}


_WANTED = {}


def wanted(oracle, key, model, samples, spectra, tables: dict, P, meanflux: bool, lines: int, forms=("dense", "woodbury"), p=None):
    """Per quasar both restatements in the given forms, once per ``key``: {"mc": {form: [dict]}, "pf": {form: [dict]}}.
    ``tables``: the call's host tables [nq, ...]; ``P``: [nq, 2 + md]; ``p``: the batch's parameters (the grid's range)."""
    if key not in _WANTED:
        grids = [R.grid(oracle, model, sp, p) for sp in spectra]
        out = {"mc": {}, "pf": {}}
        caches = [{} for _ in grids]
        for form in forms:
            out["mc"][form] = [MMR.marginal_continuum_multi(oracle, model, g, samples, quasar_tables(tables, q), P[q], meanflux, lines,
                                                            form, caches[q]) for q, g in enumerate(grids)]
            out["pf"][form] = [PMR.predictive_flux_multi(oracle, model, g, samples, quasar_tables(tables, q), P[q], meanflux, lines,
                                                         form, caches[q]) for q, g in enumerate(grids)]
        _WANTED[key] = out
    return _WANTED[key]


def split_mc(res) -> list:
    """What Batch.marginal_continuum_multi returns as one dict per selected quasar, in the restatement's layout."""
    off = res["offsets"]
    out = []
    for s in range(off.size - 1):
        d = {n: res[n][off[s]:off[s + 1]] for n in MMR.ARRAYS}
        d.update({n: res[n][s] for n in MMR.ROWS})
        d.update(status=int(res["status"][s]), model_flags=int(res["model_flags"][s]))
        out.append(d)
    return out


def split_pf(res) -> list:
    off = res["offsets"]
    out = []
    for s in range(off.size - 1):
        d = {n: res[n][off[s]:off[s + 1]] for n in PMR.PRODUCTS}
        d.update(status=int(res["status"][s]), model_flags=int(res["model_flags"][s]))
        out.append(d)
    return out


def all_flags(md: int) -> int:
    return MMR.FLAG_LLS | ((1 << md) - 1)
