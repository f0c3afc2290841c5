#!/usr/bin/env python
"""Call times of the sample generator on the GPU: the KDE of N = 1e5 catalogue values on
the 1000-point fit grid (rule bandwidth, i.e. both rank-selection passes included), the fit of a prior
(KDE + quadratic + the table of g for Z), the table build alone (a one-point F evaluation), and a
1e4-sample draw.  Each figure is a host clock around one library call -- upload, kernels, download;
every call ends in a device-to-host copy -- after a warm-up, the median and the extremes of `--repeat`
calls.  Needs a GPU; prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp_dla_detection_amd import _lib, samples  # noqa: E402


def timed(fn, repeat, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(t)), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--values", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_samples.py needs a GPU: there is nothing to time without one")
    rng = np.random.default_rng(1)
    v = 20 + rng.exponential(0.45, args.values)
    x = np.linspace(20.0, 22.0, 1000)
    small = v[:6000]
    prior = samples.fit_nhi_prior(small, device=args.device)
    import ctypes as C
    lib = _lib.load()
    cols = [np.empty(args.samples) for _ in range(3)]
    draw = _lib.SampleDraw(*[_lib.ptr(c) for c in cols])

    def draw_only():
        _lib.check(lib.gpdla_samples_draw(C.byref(prior._s), 0, args.samples, None, 0, 19.5, 20.0, C.byref(draw), args.device))

    out = dict(values=args.values, samples=args.samples, repeat=args.repeat,
               kde_rule_bandwidth=timed(lambda: samples.kde(v, x, device=args.device), args.repeat),
               kde_given_bandwidth=timed(lambda: samples.kde(v, x, bandwidth=0.05, device=args.device), args.repeat),
               fit_prior_6000_values=timed(lambda: samples.fit_nhi_prior(small, device=args.device), args.repeat),
               table_build_and_one_point=timed(lambda: prior.cdf(21.0), args.repeat),
               draw_with_its_table=timed(draw_only, args.repeat),
               generate_samples=timed(lambda: samples.generate_dla_samples(small, num=args.samples, device=args.device),
                                      args.repeat))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
