"""Times the mock-spectra draw on the DR12Q shard: ``--quasars`` templates (default
20 358) with the real length mix (``synthetic.make_dr12q_mix``), single-DLA rows and mean-flux rows,
with 0 .. ``--max-absorbers`` absorbers per quasar.  Per variant, from ONE process:

* the wall time of the synchronised ``Batch.draw_mocks`` call (prepare, absorption, draw, the copy of
  the flux back to the host), after a warm-up, median of ``--repeats``;
* the device time of k_mock_draw alone (gpdla_context_last_sweep_ms with timing enabled);
* what the draw must move -- the prepared rows (4 + k doubles per grid pixel), wavelength, noise
  variance and mask per stored pixel, the flux written -- and what it must compute: Faddeeva
  evaluations of the absorption (absorbers x (n_u + 6) x lines) and, for the preparation kernel, ``pow``
  calls (1 per kept pixel; 2 x num_forest_lines with the mean-flux rows).  ``bound`` names which of the
  two a variant is closer to, from the peak figures given with ``--hbm-gbs`` / ``--gevals``.

and once, for context, the time of the NumPy restatement (tests/mock_restatement.py) on ``--cpu-quasars``
templates, scaled to the shard and divided by the CPUs of this process.

Prints one JSON line.  Per-kernel times: run under ``rocprofv3 --kernel-trace --stats`` in a run of its
own."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gp_dla_detection_amd as gp  # noqa: E402
from gp_dla_detection_amd import _lib, mocks, synthetic  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters, Parameters  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quasars", type=int, default=20358)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--max-absorbers", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "16")))
    ap.add_argument("--cpu-quasars", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM bandwidth the bound is judged by (GB/s)")
    ap.add_argument("--gevals", type=float, default=1180.0,
                    help="Faddeeva evaluations per second the bound is judged by (1e9/s; default: what k_spectra_moments sustains, DESIGN.md 4.12)")
    a = ap.parse_args()
    nq, k = a.quasars, a.k
    model, samples = synthetic.make_model(k), synthetic.make_samples(64)
    t0 = time.perf_counter()
    templates = synthetic.make_dr12q_mix_parallel(0, nq, k, a.workers)
    t_templates = time.perf_counter() - t0
    stored = int(sum(t["wavelengths"].size for t in templates))
    out = dict(quasars=nq, k=k, stored_pixels=stored, make_templates_s=t_templates,
               libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16], variants=[])
    for meanflux in (False, True):
        p = MultiParameters() if meanflux else Parameters()
        ctx = gp.Context(0, p)
        try:
            ctx.set_model(model)
            ctx.set_samples(samples)
            ctx.set_timing(True)
            lp = (np.zeros(nq), np.zeros((nq, p.max_dlas)), np.zeros(nq)) if meanflux else (np.zeros(nq), np.zeros(nq))
            batch = ctx.upload(templates, *lp)
            n_u = batch.unmasked_counts()
            kept = synthetic.kept_pixel_counts(templates)
            for na in range(a.max_absorbers + 1):
                probs = [0.0] * na + [1.0]
                truth = mocks.draw_truth(templates, None, probs, (20.0, 22.5), None, 0.01, seed=na, params=p)
                batch.draw_mocks(truth, seed=1, write_resident=False)                                  # warm-up
                wall, dev = [], []
                for r in range(a.repeats):
                    t0 = time.perf_counter()
                    res = batch.draw_mocks(truth, seed=2 + r, write_resident=False)
                    wall.append(time.perf_counter() - t0)
                    dev.append(ctx.last_sweep_ms())
                assert int((res["status"] == 0).sum()) > 0.99 * nq
                absorbers = int(truth[0][-1])
                lines = p.num_lines
                bytes_moved = 8 * (int(n_u.sum()) * (4 + k + (1 if absorbers else 0)) + stored * 3) + stored
                faddeeva = float(np.sum(np.diff(truth[0]) * (n_u + 6))) * lines
                pows = float(kept.sum()) * (2 * p.num_forest_lines if meanflux else 1)
                t_bytes, t_evals = bytes_moved / (a.hbm_gbs * 1e9), faddeeva / (a.gevals * 1e9)
                out["variants"].append(dict(
                    meanflux=meanflux, absorbers_per_quasar=na, absorbers=absorbers, wall_s=wall, wall_median_s=float(np.median(wall)),
                    draw_kernel_ms=float(np.median(dev)), grid_pixels=int(n_u.sum()), kept_pixels=int(kept.sum()),
                    bytes_moved=bytes_moved, faddeeva_evaluations=faddeeva, prepare_pow_calls=pows,
                    bound="bytes" if t_bytes >= t_evals else "faddeeva",
                    draw_kernel_gbs=bytes_moved / (float(np.median(dev)) * 1e-3) / 1e9,
                    spectra_per_s=nq / float(np.median(wall))))
            batch.close()
        finally:
            ctx.close()
    if not a.no_cpu:
        import mock_restatement as R
        from oracle import oracle
        sub = min(a.cpu_quasars, nq)
        truth = mocks.draw_truth(templates[:sub], None, [0.0, 1.0], (20.0, 22.5), seed=1)
        t0 = time.perf_counter()
        for i in range(sub):
            z, ln = R.absorbers_of(truth, i)
            R.draw(oracle, model, templates[i], i, 1, z, ln)
        per = (time.perf_counter() - t0) / sub
        out.update(cpu_restatement_quasars=sub, cpu_restatement_s_per_quasar=per,
                   cpu_restatement_shard_s_on_workers=per * nq / max(1, a.workers), cpu_workers=a.workers)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
