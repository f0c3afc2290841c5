"""The shapes at which the model-spectra kernels (csrc/spectra_kernels.hpp, csrc/host_spectra.hpp) and
k_mock_draw (csrc/mock_kernels.hpp) take another path, as case lists and builders shared by
tests/test_model_spectra_edges.py (the CPU side: the lists hold every edge, the restatement accepts every
case), tests/test_gpu_model_spectra_edges.py and tests/test_gpu_mock_edges.py.  A plain module, like
refine_cases.py.

n_u is the number of pixels of a quasar's unmasked-range grid, S the number of samples.  Spectra come from
``synthetic.make_spectrum(index, n, model, mask_fraction, edge_pixels)``: exactly n pixels in the rest
range, so n_u = n, and n + 2 * edge_pixels stored pixels.
"""
import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import Parameters

import model_spectra_restatement as R

# The kernels' own constants (tests/test_model_spectra_edges.py reads them back from the sources).
MAP_TILE = 250              # kMapTile: output pixels of a tile of k_spectra_map (256 raw values)
MAX_ABSORBERS = 8           # kSpectraMaxAbsorbers
MOM_TILE = 16               # kProfTile: pixels of a tile of k_spectra_moments
MOM_WAVES = 4               # kMomWaves: a block of k_spectra_moments is MOM_WAVES * 64 samples
MOM_CHUNK = MOM_WAVES * 64
CONT_TILE = 128             # kContTile
CONT_THREADS = 256          # a thread of k_spectra_continuum owns entries tid + 256 t of [vech(B) | v]
MOCK_TILE = 256             # stored pixels of a tile of k_mock_draw
PARTIAL_BYTES = 256 << 20   # kSpectraPartialBytes
LYA = 1215.6701

# The project's tolerances, restated (the CPU test holds them to their sources).
TOL_MAP = 1e-12             # tests/test_gpu_model_spectra.py
TOL_MOMENTS = 1e-11         # tests/test_gpu_model_spectra.py
ONE_HOT_VAR = 1e-25         # test_moments_special_rows_and_the_lls_choice: one sample, no spread


def masked_out(sp) -> dict:
    """The quasar with every stored pixel masked the way preload_qsos.m leaves them: status 1, NaN rows."""
    n = np.asarray(sp["wavelengths"]).size
    return dict(sp, pixel_mask=np.ones(n, dtype=np.uint8), flux=np.full(n, np.nan), noise_variance=np.full(n, np.inf))


def mask_stored(sp, idx) -> dict:
    out = dict(sp)
    for key in ("flux", "noise_variance", "pixel_mask"):
        out[key] = np.array(sp[key])
    out["pixel_mask"][idx] = 1
    out["flux"][idx] = np.nan
    out["noise_variance"][idx] = np.inf
    return out


def in_range(sp, p=None) -> np.ndarray:
    p = p or Parameters()
    rest = np.asarray(sp["wavelengths"]) / (1 + sp["z_qso"])
    return (rest >= p.min_lambda) & (rest <= p.max_lambda)


# ------------------------------------------------------------------------------------------------
# P1: k_spectra_map
# ------------------------------------------------------------------------------------------------

MAP_NU = (1, 2, 6, 7, 243, 244, 245, 249, 250, 251, 255, 256, 257, 499, 500, 501)
MAP_LINES = (3, 31)
# One absorber list per quasar.  ("seam", p, log N): centred on grid pixel p, z = wl[p] / 1215.6701 - 1, with
# log N >= 21 so that the trough spans the seam; ("last", log N): centred on the last pixel; ("at", f, log N): at
# fraction f of the search range.  Every count of 0, 1, 4 and 8 (kSpectraMaxAbsorbers) occurs, on either side
# of a tile edge.
_FILL = tuple(("at", f, ln) for f, ln in ((0.07, 20.3), (0.31, 22.4), (0.52, 20.9), (0.66, 21.7), (0.81, 20.1), (0.93, 22.8),
                                          (0.44, 21.2), (0.18, 20.6)))
MAP_ABSORBERS = {
    1: (("last", 21.0),),
    2: (),
    6: _FILL[:4],
    7: _FILL[:8],
    243: (("last", 20.4),),
    244: _FILL[:3] + (("last", 21.5),),
    245: (),
    249: _FILL[:7] + (("last", 21.1),),
    250: (("last", 21.3),),                                     # the last pixel of tile 0
    251: (("seam", 249, 21.0), ("seam", 250, 21.6), ("last", 20.2), _FILL[1]),   # the last pixel is tile 1's only one
    255: _FILL[:7] + (("seam", 250, 21.2),),
    256: (("seam", 249, 21.4),),
    257: (),
    499: (("seam", 250, 21.0),) + _FILL[2:5],
    500: _FILL[:6] + (("seam", 249, 21.8), ("seam", 499, 21.0)),
    501: (("seam", 499, 21.3), ("seam", 500, 21.0), ("seam", 250, 22.0), _FILL[5]),
}
MAP_DEAD = (("at", 0.5, 21.0),)                                 # the fully masked quasar is given one too


def map_batch(k: int = 20):
    """(model, spectra): one quasar per n_u of MAP_NU, every second one masked at 5 %, then a fully masked
    one (a NaN row with status 1)."""
    model = synthetic.make_model(k)
    spectra = [synthetic.make_spectrum(5000 + 2 * i, n, model, mask_fraction=0.05 if i % 2 else 0.0) for i, n in enumerate(MAP_NU)]
    spectra.append(masked_out(synthetic.make_spectrum(5100, 300, model)))
    return model, spectra


def map_lists():
    return [MAP_ABSORBERS[n] for n in MAP_NU] + [MAP_DEAD]


def resolve_absorbers(lists, grids):
    """The CSR triple (offsets, z_dlas, log_nhis) ``Batch.model_spectra`` takes, from one list of
    ("seam" | "last" | "at", ...) entries and one ``R.grid`` per quasar."""
    off, zs, lns = [0], [], []
    for items, g in zip(lists, grids):
        lo, hi = (g["min_z"], g["max_z"]) if "pad" in g else (2.0, 2.5)
        for item in items:
            if item[0] == "seam":
                zs.append(g["wl"][item[1]] / LYA - 1)
            elif item[0] == "last":
                zs.append(g["wl"][-1] / LYA - 1)
            else:
                zs.append(lo + (hi - lo) * item[1])
            lns.append(item[-1])
        off.append(len(zs))
    return np.array(off, dtype=np.int64), np.array(zs), np.array(lns)


def seam_pixels(items, n_u: int):
    """[(item, pixels)]: the pixels either side of the tile edge a "seam" absorber sits on (those the grid has)."""
    out = []
    for item in items:
        if item[0] == "seam":
            edge = (item[1] + 1) // MAP_TILE * MAP_TILE        # 249, 250 -> 250; 499, 500 -> 500
            out.append((item, [p for p in (edge - 1, edge) if p < n_u]))
    return out


# ------------------------------------------------------------------------------------------------
# P2: k_spectra_weights, k_spectra_moments, k_spectra_combine
# ------------------------------------------------------------------------------------------------

MOM_NU = (1, 2, 15, 16, 17, 31, 32, 33, 250, 257)
MOM_NU_31 = (17, 33)        # the run at 31 lines
MOM_S_31 = 257
MOM_S = (1, 63, 64, 65, 255, 256, 257, 513)
RESIDENT_S = (65, 257)      # resident weights against the same table from the host
HOT_POSITIONS = (0, 62, 63, 64, 254, 255, 256)      # in z order; and S - 1
NAN_ROWS = ("all_nan", "all_neg_inf", "one_pos_inf")
MOM_REPEATS = 3             # times a row kind occurs in a call (moment_entries)


def moments_batch(nus=MOM_NU, k: int = 20):
    """(model, spectra): from 16 pixels up every second quasar is masked at 5 %."""
    model = synthetic.make_model(k)
    spectra = [synthetic.make_spectrum(5200 + 2 * i, n, model, mask_fraction=0.05 if (i % 2 and n >= 16) else 0.0)
               for i, n in enumerate(nus)]
    return model, spectra


def hot_positions(S: int):
    return sorted({p for p in HOT_POSITIONS if p < S} | {S - 1})


def row_kinds(S: int):
    return ["flat", "sweep", "half_nan"] + [("hot", p) for p in hot_positions(S)] + list(NAN_ROWS)


def z_order(samples) -> np.ndarray:
    """The order k_spectra_moments walks the samples in: the context's perm, a stable sort of the offsets."""
    return np.argsort(np.asarray(samples["offset_samples"]), kind="stable")


def moment_row(kind, S: int, samples, sweep_row) -> np.ndarray:
    """One row of sample log-likelihoods of the host table."""
    if kind == "flat":
        return np.full(S, -1234.5)
    if kind == "sweep":
        return np.array(sweep_row, dtype=np.float64)
    if kind == "half_nan":
        row = np.array(sweep_row, dtype=np.float64) if S > 1 else np.full(S, -3.0)
        row[1::2] = np.nan
        return row
    if kind == "all_nan":
        return np.full(S, np.nan)
    if kind == "all_neg_inf":
        return np.full(S, -np.inf)
    if kind == "one_pos_inf":
        row = np.linspace(-40.0, -1.0, S)
        row[S // 2] = np.inf
        return row
    assert kind[0] == "hot"
    row = np.full(S, -5000.0)
    row[z_order(samples)[kind[1]]] = 0.0
    return row


def moment_entries(S: int, num_quasars: int = len(MOM_NU), repeats: int = MOM_REPEATS):
    """[(quasar, kind)] of one call, a repeated selection: every row kind ``repeats`` times, kind i on quasars
    i, i + 4, i + 8 (mod the number of quasars), so that a kind meets several grid lengths and every quasar
    is used."""
    kinds = row_kinds(S)
    return [((i + 4 * r) % num_quasars, kind) for r in range(repeats) for i, kind in enumerate(kinds)]


def expects_nan(kind, row) -> bool:
    """A row without an entry above -inf, or with +inf: NaN mean and variance (k_spectra_weights' header)."""
    return kind in NAN_ROWS or not np.isfinite(np.asarray(row)).any()


def want_moments(oracle, g, samples, row, nhi_key="nhi_samples", num_lines=3):
    """R.moments, with the rows the restatement has no words for -- all -inf, +inf -- spelled out: NaN."""
    row = np.asarray(row, dtype=np.float64)
    if np.isposinf(row).any() or not (row[~np.isnan(row)] > -np.inf).any():
        return np.full(g["n_u"], np.nan), np.full(g["n_u"], np.nan)
    return R.moments(oracle, g, samples["offset_samples"], samples[nhi_key], row, num_lines)


# ---- the launch split ----

SPLIT_QUASARS, SPLIT_NU, SPLIT_S = 8, 1500, 10000
SPLIT_ENTRIES = 600


def launch_group(S: int, max_stored_pixels: int) -> int:
    """Selected quasars of one launch of k_spectra_moments (gpdla_batch_model_spectra, before its min with
    nsel): chunks = ceil(S / 256), stride = 16 ceil(max stored pixels / 16), two partial sums per pixel and
    chunk in doubles, as many quasars as fit kSpectraPartialBytes."""
    chunks = -(-S // MOM_CHUNK)
    stride = MOM_TILE * -(-max(max_stored_pixels, 1) // MOM_TILE)
    return max(1, PARTIAL_BYTES // (chunks * 2 * stride * 8))


def split_batch(k: int = 20):
    model = synthetic.make_model(k)
    return model, synthetic.make_spectra(SPLIT_QUASARS, SPLIT_NU, model, mask_fraction=0.03, first_index=7100)


def split_selection(nsel: int = SPLIT_ENTRIES, nq: int = SPLIT_QUASARS) -> np.ndarray:
    """The quasar indices repeated in a fixed shuffled order."""
    rng = np.random.default_rng(278)
    return np.concatenate([rng.permutation(nq) for _ in range(-(-nsel // nq))])[:nsel].astype(np.int64)


SPLIT_NAN_EVERY, SPLIT_NAN_AT = 41, 7      # entry j with j % 41 == 7 is an all-NaN row: its flag is set


def split_nan_entries(nsel: int) -> np.ndarray:
    return np.arange(nsel) % SPLIT_NAN_EVERY == SPLIT_NAN_AT


def split_rows(sel, sweep_rows, samples) -> np.ndarray:
    """Host weights [nsel, S]: a quasar's own sweep row at its first occurrence and at every fifth entry,
    one-hot rows (the hot sample moving with the entry) and flat rows elsewhere, so that neighbours differ;
    an all-NaN row at every 41st entry, so that the flags of the entries differ from group to group too."""
    S = sweep_rows.shape[1]
    order = z_order(samples)
    rows = np.empty((sel.size, S))
    seen = set()
    nan_row = split_nan_entries(sel.size)
    for j, q in enumerate(sel):
        if nan_row[j]:
            rows[j] = np.nan
        elif q not in seen or j % 5 == 0:
            rows[j] = sweep_rows[q]
            seen.add(q)
        elif j % 2:
            rows[j] = -5000.0
            rows[j, order[(j * 37) % S]] = 0.0
        else:
            rows[j] = -1234.5
    return rows


def split_checked_entries(nsel: int, nsub: int):
    """Entries compared with the same (quasar, row) computed alone: all within 2 of a group seam, every 16th."""
    near = {j for seam in range(nsub, nsel, nsub) for j in range(seam - 2, seam + 2) if 0 <= j < nsel}
    return sorted(near | set(range(0, nsel, 16)) | {nsel - 1})


# ------------------------------------------------------------------------------------------------
# P3: k_spectra_continuum
# ------------------------------------------------------------------------------------------------

CONT_RANKS = (1, 2, 21, 22, 23, 40)
CONT_NU = (2, 127, 128, 129, 256, 257)
CONT_MEANFLUX_RANKS = (22, 40)      # with and without the mean-flux model
CONT_FRACTIONS, CONT_LOG_NHIS = (0.35, 0.8), (20.6, 21.4)


def continuum_entries(k: int) -> int:
    """Entries of [vech(B) | v]."""
    return k * (k + 1) // 2 + k


def continuum_batch(k: int):
    """(model, spectra): masked at 5 % from 127 pixels up; n_u = 2 has fewer kept pixels than k >= 21."""
    model = synthetic.make_model(k)
    spectra = [synthetic.make_spectrum(5300 + 2 * i + 20 * k, n, model, mask_fraction=0.05 if n >= 127 else 0.0)
               for i, n in enumerate(CONT_NU)]
    return model, spectra


def continuum_variants(k: int):
    """[(meanflux, with_absorbers)]"""
    return [(mf, ab) for mf in ((False, True) if k in CONT_MEANFLUX_RANKS else (False,)) for ab in (False, True)]


def continuum_lists(with_absorbers: bool):
    items = tuple(("at", f, ln) for f, ln in zip(CONT_FRACTIONS, CONT_LOG_NHIS)) if with_absorbers else ()
    return [items for _ in CONT_NU]


_CONT = {}


def continuum_wanted(oracle, k: int):
    """Per rank, once: dict(model, spectra, grids, variants: {(meanflux, with_absorbers): dict(absorbers, dense,
    woodbury)}), dense / woodbury being lists of (continuum, model_flux) per quasar."""
    if k not in _CONT:
        model, spectra = continuum_batch(k)
        grids = [R.grid(oracle, model, sp) for sp in spectra]
        variants = {}
        for mf, ab in continuum_variants(k):
            absorbers = resolve_absorbers(continuum_lists(ab), grids)
            off, zs, lns = absorbers
            dense, wood = [], []
            for i, g in enumerate(grids):
                a = R.map_absorption(oracle, g["pad"], zs[off[i]:off[i + 1]], lns[off[i]:off[i + 1]], 3)
                dense.append(R.continuum(oracle, model, g, a, mf, "dense"))
                wood.append(R.continuum(oracle, model, g, a, mf, "woodbury"))
            variants[(mf, ab)] = dict(absorbers=absorbers, dense=dense, woodbury=wood)
        _CONT[k] = dict(model=model, spectra=spectra, grids=grids, variants=variants)
    return _CONT[k]


def continuum_disagreement(oracle, ranks=CONT_RANKS) -> float:
    """The worst dense-vs-Woodbury disagreement of the restatement over every case of ``ranks``."""
    worst = 0.0
    for k in ranks:
        for v in continuum_wanted(oracle, k)["variants"].values():
            for d, w in zip(v["dense"], v["woodbury"]):
                worst = max(worst, float(np.abs(d[0] - w[0]).max()), float(np.abs(d[1] - w[1]).max()))
    return worst


# ------------------------------------------------------------------------------------------------
# k_mock_draw
# ------------------------------------------------------------------------------------------------

# (n, edge_pixels, mask): n + 2 edge_pixels stored pixels.  mask: "none", "5%" or "first" (the first in-range
# pixel masked).  5 % on every second quasar; an absorber (MOCK_ABSORBER) on quasars 0, 1, 4, 5, 8: every second
# one, with and without a mask.
MOCK_CASES = (
    (251, 2, "none"),       # 255 stored
    (252, 2, "5%"),         # 256 stored
    (253, 2, "none"),       # 257 stored
    (40, 0, "5%"),          # nothing outside the range
    (40, 256, "none"),      # the first and the last tile are wholly out of range
    (40, 300, "5%"),
    (300, 106, "none"),     # 512 stored: the in-range edges inside tile 0 and tile 1
    (1, 0, "none"),
    (40, 256, "first"),     # the range starts on a tile edge, with a masked pixel
)
MOCK_RANKS = (20, 40)
MOCK_ABSORBER = (("at", 0.5, 21.0),)


def mock_case(oracle, k: int) -> dict:
    """dict(model, samples, templates, truth) in the form of mock_restatement.recovery_case."""
    model, samples = synthetic.make_model(k), synthetic.make_samples(16)
    templates = []
    for i, (n, edge, mask) in enumerate(MOCK_CASES):
        sp = synthetic.make_spectrum(5400 + 2 * i, n, model, mask_fraction=0.05 if mask == "5%" else 0.0, edge_pixels=edge)
        if mask == "first":
            sp = mask_stored(sp, [int(np.flatnonzero(in_range(sp))[0])])
        templates.append(sp)
    grids = [R.grid(oracle, model, sp) for sp in templates]
    truth = resolve_absorbers([MOCK_ABSORBER if i % 4 < 2 else () for i in range(len(templates))], grids)
    return dict(model=model, samples=samples, templates=templates, truth=truth, grids=grids)
