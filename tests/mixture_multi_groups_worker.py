"""Worker of test_gpu_mixture_multi.py::test_bit_identity_across_launch_groups: one seeded call of each multi-model entry
on host tables, run in the test's own process with the product library and in a clean child process (forked from
conftest.py's fork server, which predates any GPU use) with GPDLA_LIB_PATH = libgpdla_legacy.so and its debug-only scratch
budget GPDLA_MC_SCRATCH_BYTES set BEFORE the library is loaded."""
import os

import numpy as np

K, S, MD = 20, 65, 3
NUS = (5, 33, 65, 129, 31)


def case():
    """(model, samples, spectra, host tables, model weights): five quasars, every base pattern, some slots never drawn, one
    quasar without weight on DLA(2)."""
    from gp_dla_detection_amd import synthetic
    import model_spectra_multi_cases as MSC
    model = synthetic.make_model(K)
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(6900 + 2 * i, n, model, mask_fraction=0.05 if i % 2 else 0.0) for i, n in enumerate(NUS)]
    n = len(spectra)
    rng = np.random.default_rng(21)
    tables = dict(sample_log_likelihoods_dla=-1000.0 + 6.0 * rng.standard_normal((n, MD, S)),
                  base_sample_inds=np.stack([MSC.base_rows(("random", "cyclic", "one", "ends", "random")[q], S, MD, samples, seed=q)
                                             for q in range(n)]),
                  sample_log_likelihoods_lls=-1000.0 + 6.0 * rng.standard_normal((n, S)))
    tables["base_sample_inds"][4, 1, ::7] = 0
    P = 0.05 + rng.random((n, 2 + MD))
    P[2, 3] = 0.0
    return model, samples, spectra, tables, P


def run_case(selection=None):
    """Both entries on ``selection`` of the case (default: all five, in order), as {"mc_<name>", "pf_<name>"}."""
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd.parameters import Parameters
    model, samples, spectra, tables, P = case()
    n = len(spectra)
    sel = np.arange(n) if selection is None else np.asarray(selection, dtype=np.int64)
    ctx = gp.Context(0, Parameters())
    ctx.set_model(model)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))
    try:
        kw = dict(selection=sel, tables={name: t[sel] for name, t in tables.items()}, model_weights=P[sel], meanflux=False)
        mc = batch.marginal_continuum_multi(**kw)
        pf = batch.predictive_flux_multi(**kw)
    finally:
        batch.close()
        ctx.close()
    return {**{f"mc_{name}": v for name, v in mc.items()}, **{f"pf_{name}": v for name, v in pf.items()}}


def run_child(env, out_path):
    os.environ.update(env)
    out = run_case()
    np.savez(out_path, **{name: np.asarray(v) for name, v in out.items()})
