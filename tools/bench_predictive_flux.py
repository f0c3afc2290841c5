"""Times the posterior predictive flux at production scale: ``--quasars`` x ``--pixels`` x ``--samples``
(default 1000 x 1500 x 10^4) at rank ``--k`` (20 or 40).  In ONE process, from device events
(gpdla_context_last_sweep_ms), medians of ``--repeats``:

* the sweep of the same quasars and samples (``Batch.process``): the first yardstick;
* ``Batch.marginal_continuum`` on the same batch with the RESIDENT table: the second yardstick -- the predictive flux runs
  its contraction and its solve and then k_pf_pixels on top;
* k_mc_contract + k_pf_solve + k_pf_pixels + k_pf_finish with a FLAT host table (every sample weighs 1 / S: nothing is
  skipped), and with the batch's RESIDENT table after the sweep, and the fraction of samples whose weight is exactly 0 there.

Prints one JSON line with the library's hash.  The share of k_pf_pixels: run under rocprofv3 --kernel-trace --stats, in a
run of its own."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gp_dla_detection_amd as gp  # noqa: E402
from gp_dla_detection_amd import _lib, synthetic  # noqa: E402
from gp_dla_detection_amd.parameters import Parameters  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quasars", type=int, default=1000)
    ap.add_argument("--pixels", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    nq, n, S, k = a.quasars, a.pixels, a.samples, a.k
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(S)
    distinct = [synthetic.make_spectrum(9000 + i, n, model, mask_fraction=0.03) for i in range(min(nq, 64))]
    spectra = [distinct[i % len(distinct)] for i in range(nq)]
    out = dict(quasars=nq, pixels=n, samples=S, k=k,
               libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16])
    ctx = gp.Context(0, Parameters())
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        ctx.set_timing(True)
        batch = ctx.upload(spectra, np.full(nq, np.log(0.9)), np.full(nq, np.log(0.1)))
        flat = np.zeros((nq, S))
        batch.process()                                                                                  # warm-up
        batch.predictive_flux(selection=np.arange(min(nq, 4)), weights=flat[:4])
        batch.marginal_continuum(selection=np.arange(min(nq, 4)), weights=flat[:4])
        sweep_ms, mc_ms, flat_ms, res_ms, wall_s = [], [], [], [], []
        for _ in range(a.repeats):
            batch.process()
            ctx.synchronize()
            sweep_ms.append(ctx.last_sweep_ms())
            batch.marginal_continuum(weights="resident")
            mc_ms.append(ctx.last_sweep_ms())
            t0 = time.perf_counter()
            f = batch.predictive_flux(weights=flat)
            wall_s.append(time.perf_counter() - t0)
            flat_ms.append(ctx.last_sweep_ms())
            r = batch.predictive_flux(weights="resident")
            res_ms.append(ctx.last_sweep_ms())
        table = np.asarray(batch.download()["sample_log_likelihoods_dla"])
        batch.close()
    finally:
        ctx.close()
    assert np.isfinite(f["flux_var"]).all() and np.isfinite(r["flux_var"]).all()
    with np.errstate(invalid="ignore"):
        w = np.exp(table - np.nanmax(table, axis=1, keepdims=True))
    sw, mc, fl, rs = (float(np.median(x)) for x in (sweep_ms, mc_ms, flat_ms, res_ms))
    out.update(sweep_ms=sweep_ms, marginal_continuum_resident_ms=mc_ms, flat_ms=flat_ms, resident_ms=res_ms,
               sweep_ms_per_quasar=sw / nq, flat_ms_per_quasar=fl / nq, resident_ms_per_quasar=rs / nq,
               flat_over_sweep=fl / sw, resident_over_sweep=rs / sw, resident_over_marginal_continuum=rs / mc,
               resident_fraction_skipped=float(np.mean(~(w > 0))), predictive_flux_call_s=float(np.median(wall_s)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
