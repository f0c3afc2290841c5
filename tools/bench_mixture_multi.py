"""Times the marginal continuum and the predictive flux over all models of a multi-DLA run on the
``--multi-models`` workload of tools/bench_model_spectra.py: ``--distinct`` quasars (default 16) x ``--pixels`` swept once
by ``process_multi`` at ``--max-dlas`` (default 4) with ``--samples`` samples and seeded random base indices (the worst case
for the gathers: the slots of a wave are no neighbours in redshift), and a selection of ``--quasars`` entries (default 1000)
repeating them.  In ONE process, from device events (gpdla_context_last_sweep_ms), medians of ``--repeats``:

* the sweep (``Batch.process_multi``), and the existing ``Batch.marginal_continuum`` / ``Batch.predictive_flux`` on the
  resident DLA(1) table of the same batch: the yardsticks;
* each new entry with the resident ``model_posteriors`` (what a user runs);
* each new entry with flat model weights on every model (every component evaluated);
* with ``--flat-tables``, each new entry with flat weights AND flat host tables (every sample of every model live: the cost
  of n profiles a sample with nothing skipped), against the existing entries on a flat DLA(1) table.

Prints one JSON line with the library's hash.  The per-kernel split: run under rocprofv3 --kernel-trace --stats with
``--repeats 1``, in a run of its own."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gp_dla_detection_amd as gp  # noqa: E402
from gp_dla_detection_amd import _lib, synthetic  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quasars", type=int, default=1000)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--pixels", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--max-dlas", type=int, default=4)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--flat-tables", action="store_true")
    a = ap.parse_args()
    nq, n, S, md, k = a.quasars, a.pixels, a.samples, a.max_dlas, a.k
    nd = min(nq, a.distinct)
    model = synthetic.make_model(k)
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(9000 + i, n, model, mask_fraction=0.03) for i in range(nd)]
    sel = (np.arange(nq) % nd).astype(np.int64)
    out = dict(entries=nq, distinct_quasars=nd, pixels=n, samples=S, max_dlas=md, k=k,
               libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16])
    ctx = gp.Context(0, MultiParameters(max_dlas=md))
    times = {}

    def timed(name, call):
        res = call()
        times.setdefault(name, []).append(ctx.last_sweep_ms())
        return res
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        ctx.set_timing(True)
        lp_dla = np.log(np.full((nd, md), 0.1) ** np.arange(1, md + 1))
        batch = ctx.upload(spectra, np.full(nd, np.log(0.85)), lp_dla, np.full(nd, np.log(0.05)))
        base = np.random.default_rng(5).integers(1, S + 1, (nd, md - 1, S)).astype(np.uint32)
        flat_w = np.ones((nq, 2 + md))
        old_w = np.tile([0.0, 0.0, 1.0], (nq, 1))
        batch.process_multi(base)                                                                        # warm-up
        batch.marginal_continuum_multi(selection=sel[:4], model_weights=flat_w[:4])
        batch.predictive_flux_multi(selection=sel[:4], model_weights=flat_w[:4])
        batch.marginal_continuum(selection=sel[:4])
        batch.predictive_flux(selection=sel[:4])
        for _ in range(a.repeats):
            batch.process_multi(base)
            ctx.synchronize()
            times.setdefault("sweep", []).append(ctx.last_sweep_ms())
            timed("marginal_continuum_dla1", lambda: batch.marginal_continuum(selection=sel, model_weights=old_w))
            timed("predictive_flux_dla1", lambda: batch.predictive_flux(selection=sel, model_weights=old_w))
            mc = timed("marginal_continuum_multi_posteriors", lambda: batch.marginal_continuum_multi(selection=sel))
            pf = timed("predictive_flux_multi_posteriors", lambda: batch.predictive_flux_multi(selection=sel))
            mcf = timed("marginal_continuum_multi_flat_weights", lambda: batch.marginal_continuum_multi(selection=sel, model_weights=flat_w))
            pff = timed("predictive_flux_multi_flat_weights", lambda: batch.predictive_flux_multi(selection=sel, model_weights=flat_w))
        down = batch.download_multi()
        if a.flat_tables:
            tables = dict(sample_log_likelihoods_dla=np.zeros((nq, md, S)), base_sample_inds=base[sel],
                          sample_log_likelihoods_lls=np.zeros((nq, S)))
            for _ in range(a.repeats):
                timed("marginal_continuum_dla1_flat_table", lambda: batch.marginal_continuum(selection=sel, weights=tables["sample_log_likelihoods_lls"]))
                timed("predictive_flux_dla1_flat_table", lambda: batch.predictive_flux(selection=sel, weights=tables["sample_log_likelihoods_lls"]))
                timed("marginal_continuum_multi_flat_tables", lambda: batch.marginal_continuum_multi(selection=sel, tables=tables, model_weights=flat_w))
                timed("predictive_flux_multi_flat_tables", lambda: batch.predictive_flux_multi(selection=sel, tables=tables, model_weights=flat_w))
        batch.close()
    finally:
        ctx.close()
    post = np.asarray(down["model_posteriors"])
    live = {}
    with np.errstate(invalid="ignore"):
        dla = np.asarray(down["sample_log_likelihoods_dla"])
        for m in range(md):
            row = dla[:, m, :].copy()
            for j in range(m):
                row[np.asarray(down["base_sample_inds"])[:, j, :] == 0] = np.nan
            w = np.exp(row - np.nanmax(row, axis=1, keepdims=True))
            live[f"dla{m + 1}"] = float(np.mean(w > 0))
    med = {name: float(np.median(v)) for name, v in times.items()}
    out.update(ms=times, median_ms=med, model_posteriors_mean=np.nanmean(post, axis=0).tolist(), live_fraction=live,
               usable_posteriors=int((mc["status"] == 0).sum()), usable_flat=int((mcf["status"] == 0).sum()),
               finite_flat=bool(np.isfinite(mcf["continuum_var"][: mcf["offsets"][nd]]).all() and np.isfinite(pff["flux_var"][: pff["offsets"][nd]]).all()),
               flags_flat=sorted({int(f) for f in pff["model_flags"]}), flags_posteriors=sorted({int(f) for f in pf["model_flags"]}))
    for kind in ("marginal_continuum", "predictive_flux"):
        for which in ("posteriors", "flat_weights") + (("flat_tables",) if a.flat_tables else ()):
            ref = f"{kind}_dla1_flat_table" if which == "flat_tables" else f"{kind}_dla1"
            out[f"{kind}_multi_{which}_over_dla1"] = med[f"{kind}_multi_{which}"] / med[ref]
            out[f"{kind}_multi_{which}_over_sweep"] = med[f"{kind}_multi_{which}"] / med["sweep"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
