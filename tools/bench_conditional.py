"""Times gpdla_batch_process on bench.py's headline batch (``--spectra`` x ``--pixels`` synthetic quasars, ``--samples``
DLA samples, rank ``--k``; defaults 1000 x 1500, 10^4, 20) conditioned on one fixed absorber per quasar (DESIGN.md
4.20) against the same batch unconditioned, in the same process: device events on the context's stream around the
whole call (k_prepare, k_condition_rows, the record builders, the sweeps, k_condition_mask, k_evidence) and
gpdla_context_last_sweep_ms (record builders and sweeps alone), alternating, medians of ``--steps`` after ``--warmup``.
The sweeps are the same kernels on rows of the same shape: the figure expected to differ is the two small kernels'
time.  Also the wall time of one full pass of conditional.refine_conditional (one discovery pass over the batch:
context, uploads, process, refine, downloads, summaries).  A measurement, not a test.  Prints one JSON line."""
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
from gp_dla_detection_amd import _lib, conditional, synthetic  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters, Parameters  # noqa: E402


def main(argv=None):
    import torch
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--spectra", type=int, default=1000)
    ap.add_argument("--pixels", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--num-lines", type=int, default=3)
    ap.add_argument("--levels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-pass", action="store_true", help="skip the refine_conditional pass")
    args = ap.parse_args(argv)
    model, samples = synthetic.make_model(args.k), synthetic.make_samples(args.samples)
    spectra = synthetic.make_spectra(args.spectra, args.pixels, model)
    cat = synthetic.make_prior_catalog()
    lp = gp.dla_existence_prior(cat["z_qsos"], cat["dla_ind"], np.array([s["z_qso"] for s in spectra]))
    p = Parameters(num_lines=args.num_lines)
    # one fixed absorber per quasar: the injected one, or the middle of the quasar's wavelengths at log N = 20.5
    lists = [[[s["true_z_dla"], s["true_log_nhi"]]] if s.get("true_z_dla") is not None else
             [[float(np.median(s["wavelengths"])) / p.lya_wavelength - 1, 20.5]] for s in spectra]
    csr = conditional.csr_of(lists)
    stream = torch.cuda.Stream()
    ctx = gp.Context(0, p, stream=stream)
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_timing(True)
    batch = ctx.upload(spectra, *lp)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {"plain": [], "conditioned": []}
    sweeps = {"plain": [], "conditioned": []}
    try:
        for i in range(args.warmup + args.steps):
            for name in ("plain", "conditioned"):
                batch.set_fixed_absorbers(csr if name == "conditioned" else None, meanflux_rows=False)
                e0.record(stream)
                batch.process()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    times[name].append(float(e0.elapsed_time(e1)))
                    sweeps[name].append(ctx.last_sweep_ms())
    finally:
        batch.close()
        ctx.close()
    pass_s = None
    if not args.no_pass:
        t0 = time.perf_counter()
        out = conditional.refine_conditional(model, samples, spectra, csr, extra=1, rounds=0, levels=args.levels,
                                             params=MultiParameters(num_lines=args.num_lines))
        pass_s = time.perf_counter() - t0
    with open(_lib.lib_path(), "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:16]
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({
        "what": f"gpdla_batch_process of {args.spectra} quasars x {args.pixels} pixels, S = {args.samples}, k = {args.k}, {args.num_lines} lines: "
                "one fixed absorber per quasar against none, device ms of the whole call and of its sweeps",
        "library": lib_hash, "process_ms": {k: sorted(v) for k, v in times.items()}, "sweep_ms": {k: sorted(v) for k, v in sweeps.items()},
        "process_ms_median": med, "sweep_ms_median": {k: float(np.median(v)) for k, v in sweeps.items()},
        "conditioned_minus_plain_ms": med["conditioned"] - med["plain"],
        "spread_ms": {k: float(max(v) - min(v)) for k, v in times.items()},
        "refine_conditional_pass_s": pass_s,
        "discovered": None if pass_s is None else int(out["discovered"].sum()),
    }))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
