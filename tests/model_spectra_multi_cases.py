"""The shapes, base-index patterns and weight rows at which the model spectra of a multi-DLA run (DESIGN.md 4.21;
csrc/spectra_multi_kernels.hpp, csrc/host_spectra_multi.hpp) can go wrong, as case lists and builders shared by
tests/test_model_spectra_multi.py (CPU) and tests/test_gpu_model_spectra_multi.py.  A plain module beside
model_spectra_edge_cases.py, whose grids, z order and NaN rows it reuses.

An ENTRY of a call is (quasar, base pattern, row kind): its tables are sample_log_likelihoods_dla [max_dlas, S] (one
row of the kind per model, each with its own numbers), base_sample_inds [max_dlas - 1, S] and
sample_log_likelihoods_lls [S].
"""
import numpy as np

from gp_dla_detection_amd import synthetic

import model_spectra_edge_cases as E

NU = (1, 2, 15, 16, 17, 33)             # pixels either side of the 16-pixel tile, and three tiles
SAMPLES = (1, 63, 64, 65, 257)          # either side of a wave (64) and of a chunk (256)
MAX_DLAS = (2, 4)
NU_31, S_31, MAX_DLAS_31 = (17,), 65, 2  # the run at 31 lines
OWN_POSITIONS = (62, 63, 64, 255, 256)  # z-order positions of the own sample of a one-hot row ("ends" pattern)
BASE_PATTERNS = ("cyclic", "one", "random", "ends")
PARTIAL_BYTES = E.PARTIAL_BYTES


def batch(nus=NU, k: int = 20):
    """(model, spectra): one quasar per n_u, from 16 pixels up every second one masked at 5 %."""
    model = synthetic.make_model(k)
    spectra = [synthetic.make_spectrum(6200 + 2 * i, n, model, mask_fraction=0.05 if (i % 2 and n >= 16) else 0.0)
               for i, n in enumerate(nus)]
    return model, spectra


def base_rows(pattern: str, S: int, md: int, samples, seed: int = 0) -> np.ndarray:
    """base_sample_inds [md - 1, S] of one entry, 1-based.
    cyclic: row j - 2 holds (i + j - 1) mod S + 1 (slot 2: b(i) = (i + 1) mod S + 1);
    one:    every slot of every sample points at sample S // 2;
    random: seeded, uniform in 1 .. S;
    ends:   the slots alternate between the samples at z-order positions 0 and S - 1."""
    i = np.arange(S, dtype=np.int64)
    order = E.z_order(samples)
    rows = np.zeros((md - 1, S), dtype=np.uint32)
    for r in range(md - 1):
        if pattern == "cyclic":
            rows[r] = (i + r + 1) % S + 1
        elif pattern == "one":
            rows[r] = S // 2 + 1
        elif pattern == "random":
            rows[r] = np.random.default_rng(9000 + 17 * seed + r).integers(1, S + 1, S)
        else:
            assert pattern == "ends"
            rows[r] = order[0 if r % 2 == 0 else S - 1] + 1
    return rows


def own_positions(S: int):
    return sorted({p for p in OWN_POSITIONS if p < S} | {S - 1})


def row_kinds(S: int):
    return ["flat", "half_nan"] + [("hot", p) for p in own_positions(S)] + list(E.NAN_ROWS)


def model_row(kind, S: int, samples, seed: int) -> np.ndarray:
    """One model's row of sample log-likelihoods.  flat; half_nan: seeded numbers of a spread of ~ 8 with every second
    entry NaN; ("hot", p): the whole weight on the sample at z-order position p; the rows without weight."""
    if kind == "half_nan":
        row = -1000.0 + 8.0 * np.random.default_rng(7000 + seed).standard_normal(S)
        row[1::2] = np.nan
        return row
    return E.moment_row(kind, S, samples, None)


def entries(S: int, num_quasars: int = len(NU)):
    """[(quasar, pattern, kind)]: every row kind under every base pattern, walking the quasars so that each kind and
    each pattern meets several grid lengths."""
    out = []
    for a, pattern in enumerate(BASE_PATTERNS):
        for b, kind in enumerate(row_kinds(S)):
            out.append(((a * 5 + b) % num_quasars, pattern, kind))
    return out


def entry_tables(entry_list, S: int, md: int, samples):
    """Host tables of a call: (sample_log_likelihoods_dla [n, md, S], base_sample_inds [n, md - 1, S],
    sample_log_likelihoods_lls [n, S])."""
    n = len(entry_list)
    dla, base, lls = np.empty((n, md, S)), np.zeros((n, md - 1, S), dtype=np.uint32), np.empty((n, S))
    for e, (_, pattern, kind) in enumerate(entry_list):
        base[e] = base_rows(pattern, S, md, samples, seed=e)
        for m in range(md):
            dla[e, m] = model_row(kind, S, samples, seed=10 * e + m)
        lls[e] = model_row(kind, S, samples, seed=10 * e + 9)
    return dla, base, lls


def launch_group(S: int, max_stored_pixels: int, md: int) -> int:
    """Entries of one group of gpdla_batch_model_spectra_multi (before its min with nsel): the partial sums of the
    1 + md models of an entry, chunks = ceil(S / 256), stride = 16 ceil(max stored pixels / 16), two sums per pixel
    and chunk in doubles, as many entries as fit kSpectraPartialBytes."""
    chunks = -(-S // E.MOM_CHUNK)
    stride = E.MOM_TILE * -(-max(max_stored_pixels, 1) // E.MOM_TILE)
    return max(1, PARTIAL_BYTES // (chunks * 2 * stride * (1 + md) * 8))


# the grouping test: few quasars of a long grid and many samples, so that a group holds few entries
GROUP_QUASARS, GROUP_NU, GROUP_S, GROUP_MD, GROUP_DISTINCT = 3, 1500, 10000, 2, 5


def group_batch(k: int = 20):
    model = synthetic.make_model(k)
    return model, synthetic.make_spectra(GROUP_QUASARS, GROUP_NU, model, mask_fraction=0.03, first_index=7300)
