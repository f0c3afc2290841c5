"""Times the posterior maps on the table of tools/bench_posteriors.py: ``--rows`` x
``--samples`` (default 1000 x 10^4) synthetic sample tables handed over as host tables, for one model and
for four (ten slot tables per row), on 32 x 32 and 64 x 64 grids.  Reports, in ONE process,

* k_posterior_maps and k_posterior_maps_mix from device events, summed over the launch groups
  (gpdla_debug_last_maps_ms), and the number of groups;
* the wall time of the whole gpdla_stats_posterior_maps call with the per-cell outputs (mass, hpd_level)
  and without them;
* the yardstick: k_parameter_summaries on the same table (gpdla_debug_last_summaries_ms).

Prints one JSON line.  No ratio is fixed in advance; nothing here asserts a time."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_posteriors import tables  # noqa: E402
from gp_dla_detection_amd import _lib, posteriors  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    n, S = a.rows, a.samples
    lib = _lib.load()
    out = dict(rows=n, samples=S, libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16])
    for md in (1, 4):
        sll, base, smp, z_min, z_max = tables(n, md, S)
        w = np.full((n, md), 1.0 / md)
        few = slice(0, 8)
        posteriors.parameter_summaries(sll[few], smp, z_min[few], z_max[few], None if base is None else base[few])       # warm-up
        summ = []
        for _ in range(a.repeats):
            posteriors.parameter_summaries(sll, smp, z_min, z_max, base)
            summ.append(float(lib.gpdla_debug_last_summaries_ms()))
        rec = dict(parameter_summaries_kernel_ms=float(np.median(summ)))
        for shape in ((32, 32), (64, 64)):
            kw = dict(shape=shape, model_weights=w)
            posteriors.posterior_maps(sll[few], smp, z_min[few], z_max[few], None if base is None else base[few],
                                      shape=shape, model_weights=w[few])                                            # warm-up
            maps_ms, mix_ms, full, lean = [], [], [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                res = posteriors.posterior_maps(sll, smp, z_min, z_max, base, **kw)
                full.append(time.perf_counter() - t0)
                maps_ms.append(float(lib.gpdla_debug_last_maps_ms(0)))
                mix_ms.append(float(lib.gpdla_debug_last_maps_ms(1)))
                launches = int(lib.gpdla_debug_last_maps_launches())
                t0 = time.perf_counter()
                posteriors.posterior_maps(sll, smp, z_min, z_max, base, with_maps=False, **kw)
                lean.append(time.perf_counter() - t0)
            assert (res["status"] & ~8 == 0).all() and np.isfinite(res["expected_absorbers"]).all()
            k = float(np.median(maps_ms))
            rec[f"{shape[0]}x{shape[1]}"] = dict(
                maps_kernel_ms=k, mix_kernel_ms=float(np.median(mix_ms)), launches=launches, maps_kernel_ms_per_row=k / n,
                call_with_cells_s=float(np.median(full)), call_without_cells_s=float(np.median(lean)),
                dr12q_shard_20358_rows_s=k / n * 20358 / 1e3,
                cells_in_95_region_median=float(np.median(res["hpd_cells"][:, md - 1, md - 1, -1])))
        out[f"md{md}"] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
