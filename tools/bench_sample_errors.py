"""Times the three GPU passes behind the S/N table and the bootstrap sample errors at
DR12Q-like scale: N sightlines (20 358 and 162 861 by default), R = 1000 replicates.

  snr        k_sightline_snr over N ragged BOSS-like spectra (gp_dla_detection_amd.snrs.sightline_snrs:
             upload of the pixels included), in blocks of at most 20 358 sightlines as
             snrs.compute_all_snrs reads a file; the blocks reuse one set of pixel arrays (2.2 GB) with
             each block's own max_z_dlas
  path       k_path_lengths: dX[N, 12] for the bins of z in [2, 4]
  bootstrap  k_bootstrap_sums: R replicate sums of V[N, C], C = 67 columns (12 + 30 + 12 counts and
             moments, 12 + 1 paths), nine strata

each against the NumPy restatement of the same work (tests/snr_restatement.py, cddf.gauss_legendre_path,
tests/sample_error_restatement.py), timed on a sub-sample -- ``--cpu-sightlines`` sightlines,
``--cpu-replicates`` replicates -- and scaled linearly to the full size: the ``*_cpu_est_s`` figures are
estimates and say so (``bootstrap_cpu_est_s``: the fsum restatement; ``bootstrap_numpy_sum_est_s``: the same
draws with NumPy's own sum).  Times are wall-clock around the Python calls (host packing, copies and the
kernel); kernel times: run under rocprofv3 --kernel-trace --stats.  Prints one JSON line per N."""
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

import sample_error_restatement as RB  # noqa: E402
import snr_restatement as RS  # noqa: E402

from gp_dla_detection_amd import _lib, cddf, snrs  # noqa: E402

NZ, NN = 12, 30


BLOCK = 20358


def synthetic_ranges(n, seed=1):
    """(min_z_dlas, max_z_dlas) of n sightlines with redshifts like DR12Q's."""
    rng = np.random.default_rng(seed)
    z_qso = 2.0 + rng.gamma(2.0, 0.35, n)
    return np.maximum(911.75 * (1 + z_qso) / 1215.67 - 1, 3600.0 / 1215.67 - 1), z_qso - 0.01


def synthetic_pixels(n, seed=3):
    """CSR spectra on a BOSS-like grid: 4 300 to 4 700 pixels from 3 600 A at 1e-4 in log10."""
    rng = np.random.default_rng(seed)
    npix = rng.integers(4300, 4700, n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(npix, out=offsets[1:])
    total = int(offsets[-1])
    within = np.arange(total) - np.repeat(offsets[:-1], npix)
    wl = 3600.0 * 10.0 ** (1e-4 * within)
    flux = rng.normal(1.0, 0.6, total)
    nv = rng.uniform(0.02, 1.5, total)
    return dict(offsets=offsets, wavelengths=wl, flux=flux, noise_variance=nv)


def block_of(csr, m):
    o = csr["offsets"]
    return {k: (v[:m + 1] if k == "offsets" else v[:int(o[m])]) for k, v in csr.items()}


def time_of(f, repeats=3):
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sightlines", type=int, nargs="+", default=[20358, 162861])
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--cpu-sightlines", type=int, default=500)
    ap.add_argument("--cpu-replicates", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    sha = hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16]
    edges = cddf.z_bins(2, 4)
    csr = synthetic_pixels(min(BLOCK, max(a.sightlines)))
    for n in a.sightlines:
        zmin, zmax = synthetic_ranges(n)
        rng = np.random.default_rng(2)
        out = dict(sightlines=n, replicates=a.replicates, libgpdla_sha256=sha)
        snrs.sightline_snrs(block_of(csr, 64), zmax[:64])                        # warm-up: library load, first launch
        blocks = [(lo, min(lo + BLOCK, n)) for lo in range(0, n, BLOCK)]
        t, parts = time_of(lambda: [snrs.sightline_snrs(block_of(csr, hi - lo), zmax[lo:hi]) for lo, hi in blocks], repeats=2)
        s = np.concatenate(parts)
        out.update(snr_s=t, snr_blocks=len(blocks), snr_pixels=int(sum(csr["offsets"][hi - lo] for lo, hi in blocks)),
                   snr_finite=int(np.isfinite(s).sum()), snr_sightlines_per_s=n / t)
        t, (rows, dX) = time_of(lambda: cddf.path_length_matrix(zmin, zmax, s, edges, snr_thresh=-2))
        out.update(path_s=t, path_sightlines=int(rows.size), path_total=float(dX.sum()))
        C = 3 * NZ + NN + 1
        V = np.zeros((rows.size, C))
        V[:, :2 * NZ + NN] = rng.uniform(0, 1, (rows.size, 2 * NZ + NN)) * (rng.uniform(size=(rows.size, 2 * NZ + NN)) < 0.1)
        V[:, 2 * NZ + NN:3 * NZ + NN] = dX
        V[:, -1] = dX.sum(axis=1)
        label = cddf.bootstrap_strata(zmax[rows])
        order = np.argsort(label, kind="stable")
        Vs, ls = np.ascontiguousarray(V[order]), label[order]
        cddf.bootstrap_sums(Vs[:256], np.zeros(256, dtype=np.int32), 2, 1)
        t, sums = time_of(lambda: cddf.bootstrap_sums(Vs, ls, a.replicates, 7))
        out.update(bootstrap_s=t, columns=C, strata=int(label.max()) + 1, v_mb=Vs.nbytes / 1e6,
                   bootstrap_rows_per_s=rows.size * a.replicates / t, bootstrap_gathered_gb_per_s=Vs.nbytes * a.replicates / t / 1e9)
        if not a.no_cpu:
            m = min(a.cpu_sightlines, n, BLOCK)
            o = csr["offsets"]
            sub = [dict(wavelengths=csr["wavelengths"][o[i]:o[i + 1]], flux=csr["flux"][o[i]:o[i + 1]],
                        noise_variance=csr["noise_variance"][o[i]:o[i + 1]]) for i in range(m)]
            c0 = time.perf_counter()
            RS.sightline_snrs(sub, zmax[:m])
            c1 = time.perf_counter()
            for i in rows[:m]:
                for lo, hi in zip(edges[:-1], edges[1:]):
                    if zmin[i] < hi and zmax[i] > lo:
                        cddf.gauss_legendre_path(max(lo, zmin[i]), min(hi, zmax[i]))
            c2 = time.perf_counter()
            RB.bootstrap_sums(Vs, ls, a.cpu_replicates, 7)
            c3 = time.perf_counter()
            for r in range(a.cpu_replicates):   # the same draws, summed by NumPy's pairwise sum instead of fsum
                Vs[RB.drawn_rows(ls, r, 7)].sum(axis=0)
            c4 = time.perf_counter()
            out.update(bootstrap_numpy_sum_est_s=(c4 - c3) * a.replicates / a.cpu_replicates)
            out.update(cpu_subsample=dict(sightlines=m, replicates=a.cpu_replicates),
                       snr_cpu_est_s=(c1 - c0) * n / m, path_cpu_est_s=(c2 - c1) * rows.size / m,
                       bootstrap_cpu_est_s=(c3 - c2) * a.replicates / a.cpu_replicates)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
