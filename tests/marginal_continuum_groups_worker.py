"""Worker of test_gpu_marginal_continuum.py::test_bit_identity_across_launch_groups: two seeded marginal-continuum calls (resident weights;
host tables under a selection that is neither the identity nor sorted),
run in the test's own process with the product library and in a clean child process (forked from conftest.py's fork
server, which predates any GPU use) with GPDLA_LIB_PATH = libgpdla_legacy.so and its debug-only scratch budget
GPDLA_MC_SCRATCH_BYTES set BEFORE the library is loaded."""
import os

import numpy as np

K, S = 20, 130
NUS = (5, 33, 65, 129, 31)
HOST_SELECTION = (4, 0, 3, 1, 2)


def host_tables():
    """Seeded host tables [5, S] in selection order and unequal model weights (null, sub-DLA, DLA): a launch group stages
    rows of the SELECTION, so a row of the staged slice and a row of the batch cannot be confused."""
    rng = np.random.default_rng(23)
    n = len(HOST_SELECTION)
    weights = {"dla": -1000.0 + 6.0 * rng.standard_normal((n, S)), "sub_dla": -1000.0 + 6.0 * rng.standard_normal((n, S))}
    return weights, 0.05 + rng.random((n, 3))


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
        out = batch.marginal_continuum(weights="resident", components=("null", "dla"), sample_coefficients=True)
        weights, P = host_tables()
        host = batch.marginal_continuum(selection=np.array(HOST_SELECTION), weights=weights, components=("null", "sub_dla", "dla"), model_weights=P)
        return {**out, **{f"host_{name}": v for name, v in host.items()}}
    finally:
        batch.close()
        ctx.close()


def run_child(env, out_path):
    os.environ.update(env)
    out = run_case()
    np.savez(out_path, **{name: np.asarray(v) for name, v in out.items()})
