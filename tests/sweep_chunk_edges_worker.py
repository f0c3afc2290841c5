"""Worker of test_gpu_sweep_chunk_edges.py: short spectra whose K-step counts sit on and around the
edges of the slim sweep's 8-step chunks, run in this process or (run_child) in a clean child forked
from conftest.py's fork server with GPDLA_LIB_PATH = libgpdla_legacy.so and its diagnostic switches
set BEFORE the library is loaded (record_class_worker.py explains why)."""
import os

import numpy as np

# pixels inside the modelled rest range.  A spectrum takes ceil(n_u / 4) K-steps, n_u counting the in-range pixels
# masked or not (masked ones are swept as neutral rows), so masking leaves the counts alone: 2 3 7 8 8 9 9 15 16 16
# 17 25 if n_u equals these -- the test reads n_u from the uploaded batch and does not rely on this line
PIXELS = [5, 9, 28, 29, 32, 33, 36, 60, 61, 64, 65, 97]


def build_case(k, num_lines, num_samples):
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd import synthetic
    from gp_dla_detection_amd.parameters import Parameters
    model = synthetic.make_model(k)
    spectra = [synthetic.make_spectrum(5200 + 11 * i + k, n, model, mask_fraction=0.05 if i % 2 else 0.0)
               for i, n in enumerate(PIXELS)]
    cat = synthetic.make_prior_catalog()
    z = np.array([s["z_qso"] for s in spectra])
    samples = synthetic.make_samples(num_samples)
    return model, samples, spectra, gp.dla_existence_prior(cat["z_qsos"], cat["dla_ind"], z), \
        Parameters(num_lines=num_lines)


def run_case(k, num_lines, num_samples):
    import gp_dla_detection_amd as gp
    model, samples, spectra, lp, p = build_case(k, num_lines, num_samples)
    return gp.process_qsos(model, samples, spectra, log_priors=lp, params=p)


def k_steps(k, num_lines, num_samples):
    """ceil(n_u / 4) of every spectrum of the case, n_u from the uploaded batch itself"""
    import gp_dla_detection_amd as gp
    model, samples, spectra, lp, p = build_case(k, num_lines, num_samples)
    ctx = gp.Context(0, p)
    ctx.set_model(model)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra, lp[0], lp[1])
    return [int(-(-int(n) // 4)) for n in batch.unmasked_counts()]


def run_child(k, num_lines, num_samples, env, out_path):
    os.environ.update(env)
    out = run_case(k, num_lines, num_samples)
    np.savez(out_path, **{name: np.asarray(v) for name, v in out.items() if isinstance(v, np.ndarray)})
