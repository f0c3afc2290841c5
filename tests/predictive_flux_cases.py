"""The shapes at which the predictive-flux kernels (csrc/predictive_flux_kernels.hpp) take another path, as case lists and
builders shared by tests/test_predictive_flux.py (CPU) and tests/test_gpu_predictive_flux.py.  A plain module, like
marginal_continuum_cases.py, whose builders (``build``, ``params``) it uses.

n_u is the number of pixels of a quasar's unmasked-range grid, S the number of samples, k the rank.  The restatement of a
setup is computed once (``wanted``) and shared.
"""
import numpy as np

import marginal_continuum_cases as MC
import model_spectra_edge_cases as E
import model_spectra_restatement as R
import predictive_flux_restatement as PR

# The kernels' own constants (tests/test_predictive_flux.py reads them back from the sources).  k_pf_pixels has ONE shape
# for every rank (DESIGN 4.24 says why), so the packing width is the same for k <= 20 and k <= 40.
SAMPLES = 64                # kPfSamples: z-order positions k_pf_pixels takes at a time (the packing width)
PIXEL_TILE = 64             # kPfPixTile: pixels per block of k_pf_pixels
SOLVE_CHUNK = MC.SOLVE_CHUNK
RANKS = MC.RANKS            # 1, 2, 20, 21, 22, 23, 40: nb mod 4 = 1, 3, 2, 3, 1, 0, 0 and k mod 4 = 1, 2, 0, 1, 2, 3, 0 (the zero
                            # columns behind the vech part and behind the c part), and the LDS-slot straddles of DESIGN 4.12
PIXEL_COUNTS = (1, 2, 3, 4, 5, PIXEL_TILE - 1, PIXEL_TILE, PIXEL_TILE + 1, 257)

# One setup = one batch and one call, in the layout of MC.SETUPS.  Every rank; every pixel count at k = 20 and k = 40;
# S = 1, 63, 64, 65 (the packing width and the solve chunk +- 1) and 513 once per rank class; 3 and 31 lines; both kinds of
# rows; both tables; the production strata at S = 17.  From 31 pixels up every second quasar is masked at 5 % (MC.build).
SETUPS = (
    dict(name="k20_S513", k=20, S=513, nus=PIXEL_COUNTS, lines=3, multi=False, table="dla"),
    dict(name="k40_S65_meanflux", k=40, S=65, nus=PIXEL_COUNTS, lines=3, multi=True, table="dla"),
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


build, params = MC.build, MC.params

_WANTED = {}


def wanted(oracle, key, model, samples, spectra, tables, p, meanflux: bool, lines: int, forms=("dense", "woodbury")):
    """Per quasar the restatement in both forms, once per ``key``: {form: [dict per quasar]}.  ``tables``: {name: [nq, S]};
    ``p``: [nq, 3] or one row."""
    if key not in _WANTED:
        p = np.broadcast_to(np.asarray(p, dtype=np.float64), (len(spectra), 3))
        grids = [R.grid(oracle, model, sp) for sp in spectra]
        _WANTED[key] = {form: [PR.predictive_flux(oracle, model, g, samples, {n: t[q] for n, t in tables.items()}, p[q], meanflux,
                                                  lines, form) for q, g in enumerate(grids)] for form in forms}
    return _WANTED[key]


def disagreement(want) -> dict:
    """The worst dense-vs-Woodbury disagreement per product over the quasars of ``wanted``."""
    return {name: max(PR.deviation(d[name], w[name]) for d, w in zip(want["dense"], want["woodbury"])) for name in PR.PRODUCTS}


def split(res) -> list:
    """What Batch.predictive_flux returns as one dict per selected quasar, in the restatement's layout."""
    off = res["offsets"]
    out = []
    for s in range(off.size - 1):
        d = {n: res[n][off[s]:off[s + 1]] for n in PR.PRODUCTS}
        d["status"] = int(res["status"][s])
        out.append(d)
    return out


# ---- a synthetic table for the CPU file (no sweep there): smooth in z, a few nats deep ----

def synthetic_table(samples, nq: int, seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed)
    off = np.asarray(samples["offset_samples"])
    return np.array([-6.0 * (off - rng.uniform(0.2, 0.8)) ** 2 / 0.02 + rng.normal(0, 0.5, off.size) for _ in range(nq)])


# ---- weight rows ----

ROW_SETUPS = (dict(k=20, S=130, nus=(33, 65)), dict(k=40, S=67, nus=(5, 65)))
LIVE_COUNTS = (1, SAMPLES - 1, SAMPLES, SAMPLES + 1)      # live samples of a row: 1 and the packing width +- 1


def row_hot_positions(S: int):
    """One-hot rows at the edges of the sample chunks of k_pf_pixels (and of k_pf_solve: the same width) in z order."""
    return sorted({p for p in (0, SAMPLES - 1, SAMPLES, 2 * SAMPLES - 1, 2 * SAMPLES, S - 1) if p < S})


def live_row(samples, S: int, n: int, sweep_row) -> np.ndarray:
    """The sweep's row with all but ``n`` samples at l = -1e6 (weight exactly 0); the live ones are spread over the z order."""
    order = E.z_order(samples)
    row = np.full(S, -1e6)
    pos = (np.arange(n) * S) // n
    base = np.array(sweep_row, dtype=np.float64)
    row[order[pos]] = np.clip(base[order[pos]] - np.nanmax(base[order[pos]]), -8.0, 0.0)
    return row


def row_kinds(S: int):
    return (["sweep", "flat", "half_nan"] + [("hot", p) for p in row_hot_positions(S)]
            + [("live", n) for n in LIVE_COUNTS if n <= S] + list(E.NAN_ROWS))


def make_row(kind, S: int, samples, sweep_row) -> np.ndarray:
    if isinstance(kind, tuple) and kind[0] == "live":
        return live_row(samples, S, kind[1], sweep_row)
    return E.moment_row(kind, S, samples, sweep_row)


# ---- the zero-weight skip (the positions of marginal_continuum_cases) ----

SKIP_S, SKIP_LIVE, SKIP_POISON, skip_row = MC.SKIP_S, MC.SKIP_LIVE, MC.SKIP_POISON, MC.skip_row
