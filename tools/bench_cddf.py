"""Times the CDDF statistics at DR12Q-like scale: 20 358 selected quasars x 10^4 samples with peaked
synthetic posteriors.  One DLAStatistics.statistics() pass (line density, column density function
and Omega_DLA from one read of the sample table: upload, k_bin_posteriors, the Poisson-binomial CF
on the GPU, the host statistics), against the numpy restatement of the per-spectrum pass on the CPU
(timed on a subset and scaled per spectrum).  Prints one JSON line.  Kernel times: run under
rocprofv3 --kernel-trace --stats."""
import argparse
import hashlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cddf_restatement as R  # noqa: E402

from gp_dla_detection_amd import _lib, cddf  # noqa: E402


def synthetic_run(nq, S, seed=1):
    """Peaked posteriors: each quasar's likelihood mass sits within a few dozen samples of a centre
    (every fifth within a handful), and its p_dla is high enough to pass the spectrum filter."""
    rng = np.random.default_rng(seed)
    off = rng.uniform(0, 1, S)
    lnhi = rng.uniform(19.5, 23.0, S)
    zmin = rng.uniform(1.9, 2.6, nq)
    zmax = zmin + rng.uniform(0.5, 2.8, nq)
    p_dla = rng.uniform(0.06, 1.0, nq)
    lld = rng.normal(-8000, 300, nq)
    centre = rng.integers(0, S, nq)
    j = np.arange(S)
    sll = np.empty((nq, S))
    for s in range(nq):
        d = np.abs(j - centre[s])
        scale, norm = (3.0, math.log(1.1)) if s % 5 == 0 else (0.05, math.log(40.0))
        sll[s] = lld[s] + math.log(S) - scale * d - norm
    mp = np.stack([1 - p_dla, p_dla], axis=1)
    return (dict(model_posteriors=mp, log_likelihoods_dla=lld, sample_log_likelihoods_dla=sll, min_z_dlas=zmin,
                 max_z_dlas=zmax), dict(offset_samples=off, log_nhi_samples=lnhi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quasars", type=int, default=20358)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--cpu-subset", type=int, default=200)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    res, smp = synthetic_run(a.quasars, a.samples)
    snrs = np.ones(a.quasars)
    out = dict(quasars=a.quasars, samples=a.samples, table_gb=a.quasars * a.samples * 8 / 1e9,
               libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16])
    warm = cddf.DLAStatistics({k: (v[:64] if np.ndim(v) else v) for k, v in res.items()}, smp, snrs[:64],
                              sub_dla=False, occams_razor=1)
    warm.statistics(2, 5, 30)
    st = cddf.DLAStatistics(res, smp, snrs, sub_dla=False, occams_razor=1)
    reqs = [st._line_request(2, 5), st._cddf_request(2, 5, 30, 20., 23.), cddf.omega_dla_request(2, 5)]
    t0 = time.perf_counter()
    parts = st.partials(reqs)
    t1 = time.perf_counter()
    stats = st.statistics(2, 5, 30)
    t2 = time.perf_counter()
    kept = int(parts[0]["count"].sum())
    out.update(selected=int(st.selected.size), gpu_pass_s=t1 - t0, host_statistics_s=t2 - t1,
               kept_line_density=kept, gpu_pass_gb_per_s=out["table_gb"] / (t1 - t0),
               dndx_first_bins=[float(x) for x in stats["line_density"][1][:3]])
    if not a.no_cpu:
        sub = st.selected[:a.cpu_subset]
        sll = res["sample_log_likelihoods_dla"][sub]
        c0 = time.perf_counter()
        R.bin_posteriors(sll, st._shift[:sub.size], st.p_dla[sub], st.z_min[sub], st.z_max[sub], st._upper_z[:sub.size],
                         smp["offset_samples"], smp["log_nhi_samples"], reqs)
        c1 = time.perf_counter()
        per = (c1 - c0) / sub.size
        out.update(cpu_restatement_subset=int(sub.size), cpu_restatement_s_per_spectrum=per,
                   cpu_restatement_full_s_est=per * st.selected.size)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
