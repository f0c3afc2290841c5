#!/usr/bin/env python
"""Timing of the preload stage on synthetic spec files: files/s of the reader (native, with
`--threads` threads, and the Python reader on a subset; the files are read once before timing, so they come
from the page cache), the time of one `gpdla_preload_spectra` call per block (host clock: upload, the three
kernels, download), and the whole stage -- files to preloaded_qsos.mat -- against the NumPy restatement of
the two .m files on the same raw columns.  Needs a GPU; prints one JSON line with the library's hash."""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gp_dla_detection_amd import _lib, fits, io, preload, synthetic  # noqa: E402


def best(fn, repeat):
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--quasars", type=int, default=2048)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_preload.py needs a GPU: there is nothing to time without one")
    import preload_restatement as R
    n = args.quasars
    with tempfile.TemporaryDirectory() as d:
        spectra = synthetic.make_raw_spectra(n)
        cat = dict(z_qsos=np.array([s["z_qso"] for s in spectra]), plates=3586.0 + np.arange(n) // 500,
                   mjds=55181.0 + np.arange(n) % 7, fiber_ids=1.0 + np.arange(n) % 1000)
        cat["mjds"] += np.arange(n) // 1000          # (plate, mjd, fibre) unique
        paths = synthetic.write_spec_files(os.path.join(d, "spectra"), spectra, cat)
        io.savemat73(os.path.join(d, "catalog.mat"), dict({k: v.reshape(-1, 1) for k, v in cat.items()},
                                                           filter_flags=np.zeros((n, 1), np.uint8)))
        raw = fits.read_spec_files(paths, threads=args.threads)          # warms the page cache and the library
        t_native, _ = best(lambda: fits.read_spec_files(paths, native=True, threads=args.threads), args.repeat)
        t_one, _ = best(lambda: fits.read_spec_files(paths, native=True, threads=1), args.repeat)
        sub = paths[:max(1, n // 8)]
        t_python, _ = best(lambda: fits.read_spec_files(sub, native=False), 1)
        z, flags = cat["z_qsos"], np.zeros(n, np.uint8)
        off = raw["offsets"]

        def block(lo, hi):
            return dict(offsets=off[lo:hi + 1] - off[lo], **{k: raw[k][off[lo]:off[hi]] for k in ("flux", "loglam", "ivar", "and_mask")})
        first = block(0, min(args.block, n))
        preload.preload_raw(first, z[:args.block], flags[:args.block], device=args.device)     # first launch
        t_block, got = best(lambda: preload.preload_raw(first, z[:args.block], flags[:args.block], device=args.device), args.repeat)
        t_stage, _ = best(lambda: preload.preload_qsos(os.path.join(d, "catalog.mat"), os.path.join(d, "spectra"),
                                                       os.path.join(d, "preloaded.mat"), os.path.join(d, "catalog_out.mat"),
                                                       device=args.device, block=args.block), 1)
        m = max(1, min(n, 256))
        t_numpy, want = best(lambda: R.preload(block(0, m), z[:m], flags[:m]), 1)
        same = bool(np.array_equal(want["offsets"], got["offsets"][:m + 1]) and
                    np.array_equal(want["flux"], got["flux"][:want["flux"].size], equal_nan=True)) if m <= args.block else None
    with open(_lib.lib_path(), "rb") as f:
        lib_hash = hashlib.sha256(f.read()).hexdigest()[:12]
    pixels = int(first["offsets"][-1])
    print(json.dumps(dict(
        quasars=n, block=args.block, threads=args.threads, library=lib_hash,
        reader_files_per_s=round(n / t_native, 1), reader_one_thread_files_per_s=round(n / t_one, 1),
        python_reader_files_per_s=round(len(sub) / t_python, 1),
        preload_call_ms_per_block=round(t_block * 1e3, 3), block_quasars=int(first["offsets"].size - 1), block_pixels=pixels,
        preload_call_quasars_per_s=round((first["offsets"].size - 1) / t_block, 1),
        stage_s=round(t_stage, 3), stage_quasars_per_s=round(n / t_stage, 1),
        numpy_restatement_quasars_per_s=round(m / t_numpy, 1), matches_restatement_on_first=same)))


if __name__ == "__main__":
    main()
