"""Worker of test_gpu_absorption_distribution.py::test_bit_identity_across_launch_groups: seeded absorption-distribution calls
-- resident weights; host tables under a selection that is neither the identity nor sorted; the multi-DLA entry on host
tables with base rows of its own -- run in the test's own process with the product library and in a clean child process
(forked from conftest.py's fork server, which predates any GPU use) with GPDLA_LIB_PATH = libgpdla_legacy.so and its
debug-only budget GPDLA_MC_SCRATCH_BYTES set BEFORE the library is loaded.  This product allocates no scratch rows: the
budget bounds a group's weight rows, S x (sampled components) x 8 bytes a quasar."""
import os

import numpy as np

K, S, MD = 20, 130, 3
NUS = (5, 33, 65, 129, 31)
HOST_SELECTION = (4, 0, 3, 1, 2)
REQUEST = dict(thresholds=(0.8, 0.5, 0.2), bins=64, levels=(0.16, 0.5, 0.84), histogram=True)
ARRAYS = ("prob_below", "absorption_min", "absorption_max", "histogram", "quantiles")
BUDGET = 2 * S * 2 * 8    # the single-DLA entry: two quasars a group (three groups); the multi entry (4 components): one


def host_tables():
    """Seeded host tables in selection order and unequal model weights: a launch group stages rows of the SELECTION, so a
    row of the staged slice and a row of the batch cannot be confused."""
    rng = np.random.default_rng(29)
    n = len(HOST_SELECTION)
    weights = {"dla": -1000.0 + 6.0 * rng.standard_normal((n, S)), "sub_dla": -1000.0 + 6.0 * rng.standard_normal((n, S))}
    multi = dict(sample_log_likelihoods_dla=-1000.0 + 6.0 * rng.standard_normal((n, MD, S)),
                 sample_log_likelihoods_lls=-1000.0 + 6.0 * rng.standard_normal((n, S)),
                 base_sample_inds=rng.integers(0, S + 1, size=(n, MD - 1, S)).astype(np.uint32))
    return weights, 0.05 + rng.random((n, 3)), multi, 0.05 + rng.random((n, 2 + MD))


def run_case():
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd import synthetic
    from gp_dla_detection_amd.parameters import MultiParameters, Parameters
    model = synthetic.make_model(K)
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(6700 + 2 * i, n, model, mask_fraction=0.05 if i % 2 else 0.0) for i, n in enumerate(NUS)]
    weights, P, multi, PM = host_tables()
    n = len(spectra)
    sel = np.array(HOST_SELECTION)
    out = {}
    ctx = gp.Context(0, Parameters())
    ctx.set_model(model)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))
    try:
        batch.process()
        out.update(batch.absorption_distribution(weights="resident", components=("null", "dla"), **REQUEST))
        host = batch.absorption_distribution(selection=sel, weights=weights, components=("null", "sub_dla", "dla"), model_weights=P,
                                             **REQUEST)
        plain = batch.absorption_distribution(selection=sel, weights=weights, components=("null", "sub_dla", "dla"), model_weights=P,
                                              thresholds=REQUEST["thresholds"])
    finally:
        batch.close()
        ctx.close()
    out.update({f"host_{name}": v for name, v in host.items()})
    out.update({f"plain_{name}": v for name, v in plain.items()})
    p = MultiParameters(max_dlas=MD)
    ctx = gp.Context(0, p)
    ctx.set_model(model)
    ctx.set_samples(samples)
    lp_dla = np.log(np.full((n, MD), 0.1) ** np.arange(1, MD + 1))
    batch = ctx.upload(spectra, np.full(n, np.log(0.85)), lp_dla, np.full(n, np.log(0.05)))
    try:
        res = batch.absorption_distribution_multi(selection=sel, tables=multi, model_weights=PM, **REQUEST)
    finally:
        batch.close()
        ctx.close()
    out.update({f"multi_{name}": v for name, v in res.items()})
    return out


def run_child(env, out_path):
    os.environ.update(env)
    out = run_case()
    np.savez(out_path, **{name: np.asarray(v) for name, v in out.items()})
