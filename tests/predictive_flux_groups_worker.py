"""Worker of test_gpu_predictive_flux.py::test_bit_identity_across_launch_groups: one seeded predictive-flux call, run in
the test's own process with the product library and in a clean child process (forked from conftest.py's fork server, which
predates any GPU use) with GPDLA_LIB_PATH = libgpdla_legacy.so and its debug-only scratch budget GPDLA_MC_SCRATCH_BYTES set
BEFORE the library is loaded."""
import os

import numpy as np

K, S = 20, 130
NUS = (5, 33, 65, 129, 31)


def run_case():
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd import synthetic
    from gp_dla_detection_amd.parameters import Parameters
    model = synthetic.make_model(K)
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(6500 + 2 * i, n, model, mask_fraction=0.05 if i % 2 else 0.0) for i, n in enumerate(NUS)]
    ctx = gp.Context(0, Parameters())
    ctx.set_model(model)
    ctx.set_samples(samples)
    n = len(spectra)
    batch = ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))
    try:
        batch.process()
        return batch.predictive_flux(weights="resident", components=("null", "dla"))
    finally:
        batch.close()
        ctx.close()


def run_child(env, out_path):
    os.environ.update(env)
    out = run_case()
    np.savez(out_path, **{name: np.asarray(v) for name, v in out.items()})
