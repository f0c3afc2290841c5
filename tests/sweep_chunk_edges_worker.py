"""Worker of test_gpu_sweep_chunk_edges.py and test_gpu_sweep_pipeline_edges.py: short spectra whose K-step
counts sit on and around the edges of the slim sweeps' 8-step chunks (and, for the k <= 40 kernels, the
20-step priming length and the 32-step ring wrap; for the multi-DLA k <= 20 kernel, the 4-step gather
lead), run in this process or (run_child) in a clean child forked from conftest.py's fork server with
GPDLA_LIB_PATH = libgpdla_legacy.so and its diagnostic switches set BEFORE the library is loaded
(record_class_worker.py explains why).  kind is "single" (process_qsos) or "multi"
(process_qsos_multiple_dlas_meanflux, MultiParameters(max_dlas=4))."""
import os

import numpy as np

# pixels inside the modelled rest range.  A spectrum takes ceil(n_u / 4) K-steps, n_u counting the in-range pixels
# masked or not (masked ones are swept as neutral rows), so masking leaves the counts alone: 2 3 7 8 8 9 9 15 16 16
# 17 25 if n_u equals these -- the test reads n_u from the uploaded batch and does not rely on this line
PIXELS = [5, 9, 28, 29, 32, 33, 36, 60, 61, 64, 65, 97]

# k_sweep_split_slim (20 < k <= 40, single- and multi-DLA): 2 7 8 9 15 16 17 19 20 21 24 25 27 28 29 31 32 33 40 41
# K-steps; the last K-step holds 1, 2, 3 or 4 pixels in turn
PIXELS_SPLIT = [5, 26, 31, 36, 57, 62, 67, 76, 77, 82, 95, 100, 105, 110, 115, 124, 125, 130, 159, 164]
K_STEPS_SPLIT = {2, 7, 8, 9, 15, 16, 17, 19, 20, 21, 24, 25, 27, 28, 29, 31, 32, 33, 40, 41}

# k_sweep_multi_slim (k <= 20, multi-DLA): 1 1 3 4 5 7 8 9 12 15 16 17 25 K-steps (a half and a full first step; not
# a single pixel: its search range [min_z_dla, max_z_dla] has no width, so every pair of samples is closer than
# min_z_separation, the two-DLA model is all NaN and the quasar's loop ends there -- in the reference as here)
PIXELS_MULTI_SLIM = [2, 4, 10, 15, 20, 25, 30, 35, 48, 57, 62, 67, 100]
K_STEPS_MULTI_SLIM = {1, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 25}

MAX_DLAS = 4
Z_LLS, Z_DLA = 0.31, 0.69

# spectrum seeds: 5200 + 11 i + k unless a (kind, k, i) is listed here -- a spectrum whose multi-DLA loop ended
# early (an all-NaN model) is replaced by changing its seed, never skipped.  ("multi", 13, 4): at S = 128 the
# drawn indices made samples 30 and 72 of the four-DLA model name the same four absorbers in a different order
# (30 -> 54, 72, 81 and 72 -> 54, 30, 81): one likelihood in exact arithmetic, so the MAP index was a tie that
# the GPU and the oracle, 1e-11 apart, broke differently
SEEDS = {("multi", 13, 4): 6257}


def build_case(k, num_lines, num_samples, kind="single", pixels=None):
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd import synthetic
    from gp_dla_detection_amd.parameters import MultiParameters, Parameters
    pixels = PIXELS if pixels is None else pixels
    model = synthetic.make_model(k)
    spectra = [synthetic.make_spectrum(SEEDS.get((kind, k, i), 5200 + 11 * i + k), n, model,
                                       mask_fraction=0.05 if i % 2 else 0.0)
               for i, n in enumerate(pixels)]
    cat = synthetic.make_prior_catalog()
    z = np.array([s["z_qso"] for s in spectra])
    samples = synthetic.make_samples(num_samples)
    if kind == "single":
        return model, samples, spectra, gp.dla_existence_prior(cat["z_qsos"], cat["dla_ind"], z), \
            Parameters(num_lines=num_lines)
    p = MultiParameters(max_dlas=MAX_DLAS, num_lines=num_lines)
    return model, samples, spectra, gp.dla_existence_prior_multi(cat["z_qsos"], cat["dla_ind"], z, Z_LLS, Z_DLA, p), p


def edge_indices(num_quasars, num_samples, block):
    """base_sample_inds [nq, MAX_DLAS - 1, S] to supply to both libraries: seeded draws from 1 .. S, and in
    the sample slots on each side of every block edge and in the last sample the values 0 (never drawn: the
    sample's chain_ok = 0), 1 and S (kk = S - 1), rotated so that every row of the array holds each of them:
    the chain breaks at the two-, the three- and the four-DLA model in turn, behind rows that follow 1 and S;
    every fourth slot follows S and then its own draws, so that it is evaluated by all four models"""
    S = num_samples
    rng = np.random.default_rng(977 + S)
    bsi = rng.integers(1, S + 1, size=(num_quasars, MAX_DLAS - 1, S), dtype=np.uint32)
    slots = sorted({e + d for e in range(block, S, block) for d in (-1, 0)} | {S - 1})
    patterns = ((1, S, 0), (S, 0, 1), (0, 1, S), (S, None, None))
    for n, slot in enumerate(slots):
        for row, value in enumerate(patterns[n % 4]):
            if value is not None:
                bsi[:, row, slot] = value
    return bsi, slots


def run_case(k, num_lines, num_samples, kind="single", pixels=None, supplied_block=0):
    """supplied_block > 0 (multi-DLA only): base_sample_inds = edge_indices(.., supplied_block) instead of
    the GPU's own draws"""
    import gp_dla_detection_amd as gp
    model, samples, spectra, lp, p = build_case(k, num_lines, num_samples, kind, pixels)
    if kind == "single":
        return gp.process_qsos(model, samples, spectra, log_priors=lp, params=p)
    bsi = edge_indices(len(spectra), num_samples, supplied_block)[0] if supplied_block else None
    return gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p, base_sample_inds=bsi)


def k_steps(k, num_lines, num_samples, kind="single", pixels=None):
    """ceil(n_u / 4) of every spectrum of the case, n_u from the uploaded batch itself"""
    import gp_dla_detection_amd as gp
    model, samples, spectra, lp, p = build_case(k, num_lines, num_samples, kind, pixels)
    ctx = gp.Context(0, p)
    ctx.set_model(model)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra, lp[0], lp[1]) if kind == "single" else ctx.upload(spectra, lp[0], lp[2], lp[1])
    steps = [int(-(-int(n) // 4)) for n in batch.unmasked_counts()]
    batch.close()
    ctx.close()
    return steps


def run_child(k, num_lines, num_samples, env, out_path, kind="single", pixels=None, supplied_block=0):
    """num_samples: one count (arrays saved under their own names) or a list of counts (one .npz for all of
    them, names prefixed "S<count>/": one process start-up for the whole list)"""
    os.environ.update(env)
    arrays = {}
    many = not isinstance(num_samples, int)
    for S in (num_samples if many else [num_samples]):
        out = run_case(k, num_lines, S, kind, pixels, supplied_block)
        prefix = f"S{S}/" if many else ""
        arrays.update({prefix + name: np.asarray(v) for name, v in out.items() if isinstance(v, np.ndarray)})
    np.savez(out_path, **arrays)
