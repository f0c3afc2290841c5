"""Times the parameter summaries at production scale: ``--rows`` x ``--samples``
(default 1000 x 10^4) synthetic sample tables handed over as host tables (no sweep is run), for one
model and for four (ten slot tables per row, slots gathered through random ``base_sample_inds``).
Reports, in ONE process,

* k_parameter_summaries per row from device events (gpdla_debug_last_summaries_ms), and the wall time of
  the whole gpdla_stats_parameter_summaries call (ranks, copies, kernel);
* two yardsticks on the same one-model table: the wall time of gpdla_stats_bin_posteriors with one
  request (the kernel that reads the same rows once; its own kernel time: run this tool under rocprofv3
  --kernel-trace --stats), and the NumPy restatement (tests/posterior_restatement.py) on ``--cpu-rows``
  rows, per row.

A third of the rows are peaked (ESS near 1), a third broad, a third bimodal in z.  Prints one JSON line."""
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

from gp_dla_detection_amd import _lib, cddf, posteriors, synthetic  # noqa: E402


def tables(n, md, S, seed=1):
    rng = np.random.default_rng(seed)
    smp = synthetic.make_samples(S)
    off = smp["offset_samples"]
    sll = np.empty((n, md, S))
    for r in range(n):
        c = rng.random()
        width = (0.002, 0.1, 0.03)[r % 3]
        for m in range(md):
            row = -0.5 * ((off - c) / width) ** 2
            if r % 3 == 2:
                row = np.logaddexp(row, -0.5 * ((off - (1 - c)) / width) ** 2)
            sll[r, m] = row - 8000.0 + 0.3 * rng.standard_normal(S)
    base = rng.integers(1, S + 1, size=(n, md - 1, S)).astype(np.uint32) if md > 1 else None
    z_min = 2.0 + rng.random(n)
    return sll, base, smp, z_min, z_min + 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-rows", type=int, default=4)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    n, S = a.rows, a.samples
    lib = _lib.load()
    out = dict(rows=n, samples=S, libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16])
    for md in (1, 4):
        sll, base, smp, z_min, z_max = tables(n, md, S)
        posteriors.parameter_summaries(sll[:8], smp, z_min[:8], z_max[:8], None if base is None else base[:8])   # warm-up
        ker, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = posteriors.parameter_summaries(sll, smp, z_min, z_max, base)
            wall.append(time.perf_counter() - t0)
            ker.append(float(lib.gpdla_debug_last_summaries_ms()))
        assert (res["status"] == 0).all() and np.isfinite(res["quantiles_z"][:, md - 1, md - 1]).all()
        k = float(np.median(ker))
        out[f"md{md}"] = dict(kernel_ms=ker, kernel_ms_per_row=k / n, call_s=float(np.median(wall)),
                              dr12q_shard_20358_rows_s=k / n * 20358 / 1e3,
                              ess_median=float(np.median(res["effective_samples"])))
        if md == 1:
            rows = sll[:, 0, :]
            shift = rows.max(axis=1)
            req = cddf.BinRequest("lnhi", tuple(np.linspace(20.0, 23.0, 31)), 1.0, 6.0, 20.0, 23.0, histogram=True)
            args = (rows, shift, np.ones(n), z_min, z_max, z_max, smp["offset_samples"], smp["log_nhi_samples"], [req])
            cddf.bin_posteriors(*[x[:8] if i < 6 else x for i, x in enumerate(args)])                            # warm-up
            bw = []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                cddf.bin_posteriors(*args)
                bw.append(time.perf_counter() - t0)
            out["bin_posteriors_one_request_call_s"] = float(np.median(bw))
        if not a.no_cpu:
            import posterior_restatement as R
            sub = min(a.cpu_rows, n)
            t0 = time.perf_counter()
            R.summaries(sll[:sub], smp["offset_samples"], smp["log_nhi_samples"], z_min[:sub], z_max[:sub],
                        None if base is None else base[:sub])
            out[f"md{md}"]["numpy_restatement_ms_per_row"] = (time.perf_counter() - t0) / sub * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
