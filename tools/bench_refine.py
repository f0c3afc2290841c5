"""Times one refine level of every quasar of bench.py's headline batch (``--spectra`` x
``--pixels`` synthetic quasars, ``--samples`` DLA samples, rank ``--k``; defaults 1000 x 1500, 10^4, 20)
with as many refine points as samples, against the first pass's sweep of the same batch in the same
process: gpdla_context_last_sweep_ms (the sweeps of all record groups) versus gpdla_debug_last_refine_ms
(record rebuild, k_refine_boxes, the boxed sweep, k_refine_finish), both from device events; medians of
``--steps`` after ``--warmup``.  Prints one JSON line."""
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
from gp_dla_detection_amd.parameters import Parameters  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--spectra", type=int, default=1000)
    ap.add_argument("--pixels", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--num-lines", type=int, default=3)
    ap.add_argument("--levels", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args(argv)
    model, samples = synthetic.make_model(args.k), synthetic.make_samples(args.samples)
    spectra = synthetic.make_spectra(args.spectra, args.pixels, model)
    cat = synthetic.make_prior_catalog()
    lp = gp.dla_existence_prior(cat["z_qsos"], cat["dla_ind"], np.array([s["z_qso"] for s in spectra]))
    ctx = gp.Context(0, Parameters(num_lines=args.num_lines))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points()
    ctx.set_timing(True)
    batch = ctx.upload(spectra, *lp)
    sweep, fine = [], []
    try:
        for i in range(args.warmup + args.steps):
            batch.process()
            ctx.synchronize()
            t_sweep = ctx.last_sweep_ms()
            batch.refine(levels=args.levels, download=False)
            ctx.synchronize()
            if i >= args.warmup:
                sweep.append(t_sweep)
                fine.append(float(ctx.lib.gpdla_debug_last_refine_ms()))
        out = batch.download_refined(None, args.levels, with_samples=False)
        first = batch.download(with_samples=False)
        ess_first = batch.parameter_summaries(probabilities=(), thresholds=())["effective_samples"][:, 0]
        ess_refined = batch.parameter_summaries(refined=True, probabilities=(), thresholds=())["effective_samples"][:, 0]
    finally:
        batch.close()
        ctx.close()
    with open(_lib.lib_path(), "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    ok = out["status"] == 0
    print(json.dumps({
        "what": f"{args.levels} refine level(s) of {args.spectra} quasars x {args.pixels} pixels, S' = S = {args.samples}, k = {args.k}, "
                f"{args.num_lines} lines, against the first pass's sweep of the same batch",
        "library": lib_hash, "sweep_ms": sorted(sweep), "refine_ms": sorted(fine),
        "sweep_ms_median": float(np.median(sweep)), "refine_ms_median": float(np.median(fine)),
        "ratio": float(np.median(fine) / (args.levels * np.median(sweep))), "refined_rows": int(ok.sum()),
        "ess_first_pass_quartiles": [float(x) for x in np.nanpercentile(ess_first[ok], (25, 50, 75))],
        "ess_refined_quartiles": [float(x) for x in np.nanpercentile(ess_refined[ok], (25, 50, 75))],
        "rows_with_first_pass_ess_below_1.01": int((ess_first[ok] < 1.01).sum()),
        "median_log_evidence_gain": float(np.nanmedian(out["log_likelihoods_dla_refined"][ok] - first["log_likelihoods_dla"][ok])),
    }))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
