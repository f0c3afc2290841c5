"""Worker of test_gpu_refined_products.py::test_bit_identity_across_launch_groups: the marginal continuum and the predictive
flux on a refined table (the DLA component alone, and the three-component mixture whose sub-DLA component has 200 samples and
whose DLA component has S' = 65), run in the test's own process with the product library and in a clean child process
(forked from conftest.py's fork server, which predates any GPU use) with GPDLA_LIB_PATH = libgpdla_legacy.so and its
debug-only scratch budget GPDLA_MC_SCRATCH_BYTES set BEFORE the library is loaded."""
import os

import numpy as np

K, LINES, SR = 8, 3, 65
MIX = (0.2, 0.3, 0.5)


def run_case():
    import gp_dla_detection_amd as gp

    import refine_cases as RC
    import refined_products_cases as XC
    model, samples, spectra, _ = RC.make_batch(K, LINES)
    ctx = gp.Context(0, RC.batch_parameters(LINES))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(SR))
    n = len(spectra)
    batch = ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))
    try:
        batch.process()
        batch.refine(levels=XC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        sel = np.array([6, 0, 3, 1, 7, 2, 5, 4], dtype=np.int64)
        pw = np.tile(np.array(MIX), (n, 1))
        out = {}
        for tag, res in (("mc", batch.marginal_continuum(selection=sel, weights="refined", sample_coefficients=True)),
                         ("pf", batch.predictive_flux(selection=sel, weights="refined")),
                         ("mc3", batch.marginal_continuum(selection=sel, weights="refined", components=("null", "sub_dla", "dla"),
                                                          model_weights=pw)),
                         ("pf3", batch.predictive_flux(selection=sel, weights="refined", components=("null", "sub_dla", "dla"),
                                                       model_weights=pw))):
            out.update({f"{tag}_{name}": np.asarray(v) for name, v in res.items()})
        return out
    finally:
        batch.close()
        ctx.close()


def run_child(env, out_path):
    os.environ.update(env)
    np.savez(out_path, **run_case())
