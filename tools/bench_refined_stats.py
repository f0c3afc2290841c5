"""Times k_bin_posteriors_boxed against its parent k_bin_posteriors on the same table:
``--rows`` x ``--samples`` (default 2048 x 10^4) refined rows with four requests -- the three of
DLAStatistics.statistics() and a 30-bin log N_HI histogram -- from device events
(gpdla_debug_time_bin_kernels, gpdla_debug_last_bin_ms), medians of ``--repeats`` after a warm-up, in ONE process.  The yardstick is the
parent's kernel, which is handed the boxed kernel's own shift, each row's box as its z range and the
unit points mapped into [20, 23] as its shared log N_HI table: the same rows, samples and requests.

The boxed kernel reads each row twice and takes one exp10 per sample.  To show where its first pass goes it is
also timed on all-NaN rows, where pass 1 is the maximum loop alone (no finite entry: the exp-and-sum loop is
skipped) and pass 2 is unchanged.  Prints one JSON line."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gp_dla_detection_amd import _lib, cddf, synthetic  # noqa: E402


def tables(n, S, seed=1):
    rng = np.random.default_rng(seed)
    u, v = synthetic.halton(S, 2), synthetic.halton(S, 3)
    z_lo = rng.uniform(2.0, 3.5, n)
    boxes = np.stack([z_lo, z_lo + rng.uniform(0.005, 0.4, n), np.full(n, 20.0), np.full(n, 23.0)], axis=1)
    cu, cv = rng.random(n), rng.random(n)
    wu, wv = rng.uniform(0.02, 0.3, n), rng.uniform(0.02, 0.3, n)
    lam = -0.5 * (((u[None, :] - cu[:, None]) / wu[:, None]) ** 2 + ((v[None, :] - cv[:, None]) / wv[:, None]) ** 2)
    lam += -900.0 + 0.3 * rng.standard_normal((n, S))
    return lam, rng.uniform(0.3, 1.0, n), boxes, boxes[:, 1] - 0.1, u, v


def requests():
    return [cddf.line_density_request(2, 4), cddf.column_density_request(2., 4.), cddf.omega_dla_request(2, 4),
            cddf.BinRequest("lnhi", tuple(np.linspace(20.0, 23.0, 31)), 2.0, 4.0, 20.0, 23.0, histogram=True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    n, S = a.rows, a.samples
    lib = _lib.load()
    lib.gpdla_debug_time_bin_kernels(1)
    lam, p_dla, boxes, upper_z, u, v = tables(n, S)
    reqs = requests()
    lnhi = 20.0 + 3.0 * v

    def boxed(table):
        res, shift = cddf.bin_posteriors_boxed(table, p_dla, boxes, upper_z, u, v, reqs)
        return res, shift, float(lib.gpdla_debug_last_bin_ms())

    def parent(shift):
        res = cddf.bin_posteriors(lam, shift, p_dla, boxes[:, 0], boxes[:, 1], upper_z, u, lnhi, reqs)
        return res, float(lib.gpdla_debug_last_bin_ms())

    res_b, shift, _ = boxed(lam)            # warm-up of both kernels at the timed shape
    res_p, _ = parent(shift)
    nan_rows = np.full_like(lam, np.nan)
    t_boxed, t_parent, t_nan = [], [], []
    for _ in range(a.repeats):              # alternating
        t_parent.append(parent(shift)[1])
        t_boxed.append(boxed(lam)[2])
        t_nan.append(boxed(nan_rows)[2])
    # the two kernels computed the same thing (10^lnhi apart in the moment request)
    worst = 0.0
    for g, w in zip(res_b, res_p):
        assert np.array_equal(g["count"], w["count"]) and np.array_equal(g["kept_bin"], w["kept_bin"])
        for k in ("pois", "mean", "var"):
            with np.errstate(invalid="ignore", divide="ignore"):
                d = np.abs(g[k] - w[k]) / np.abs(w[k])
            worst = max(worst, float(np.nanmax(np.where(np.isfinite(d), d, 0.0))))
    assert worst < 1e-12 and any(np.any(g["pois"] > 0) for g in res_b)
    mb, mp, mn = (float(np.median(t)) for t in (t_boxed, t_parent, t_nan))
    print(json.dumps(dict(rows=n, samples=S, requests=len(reqs),
                          libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16],
                          k_bin_posteriors_ms=t_parent, k_bin_posteriors_boxed_ms=t_boxed,
                          k_bin_posteriors_boxed_all_nan_rows_ms=t_nan, parent_median_ms=mp, boxed_median_ms=mb,
                          boxed_over_parent=mb / mp, boxed_minus_parent_ms=mb - mp,
                          pass1_sum_loop_ms=mb - mn, max_loop_and_staging_ms=mn - mp,
                          boxed_us_per_row=mb / n * 1e3, worst_relative_difference=worst)))


if __name__ == "__main__":
    main()
