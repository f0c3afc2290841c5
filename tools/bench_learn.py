"""Times learning the model at the reference's training scale (4997 quasars x 1217 rest pixels, k = 20),
single-DLA and mean-flux: TrainingSet.from_spectra (upload + rest grid), the column statistics, the PCA
covariance, the numpy restatement of the same steps on the CPU, and a few fit iterations.  Prints one
JSON line.  Kernel times: run under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import learn_restatement as R  # noqa: E402
import torch  # noqa: E402

from gp_dla_detection_amd import synthetic  # noqa: E402
from gp_dla_detection_amd.api import spectra_to_csr  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters, Parameters  # noqa: E402
from gp_dla_detection_amd.training import TrainingSet, fit_training_set, pca_initial_M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quasars", type=int, default=4997)
    ap.add_argument("--fit-iters", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    model = synthetic.make_model(20)
    z = synthetic.sample_dr12q_redshifts(a.quasars)
    spectra = [synthetic.make_boss_spectrum(2 * i, float(z[i]), model, mask_fraction=0.0 if i % 2 == 0 else 0.05)
               for i in range(a.quasars)]
    csr = spectra_to_csr(spectra)
    out = dict(quasars=a.quasars, rest_pixels=1217, k=20, pixels_in=int(csr["offsets"][-1]))
    for name, meanflux in (("single", False), ("meanflux", True)):
        p = MultiParameters() if meanflux else Parameters()
        TrainingSet.from_spectra(csr, p, meanflux).close()  # warm-up (module load, first allocations)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = TrainingSet.from_spectra(csr, p, meanflux)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        _, std, _ = t.column_stats()
        t2 = time.perf_counter()
        cov, _, rows = t.pca_covariance(meanflux)
        t3 = time.perf_counter()
        r = dict(from_spectra_ms=1e3 * (t1 - t0), column_stats_ms=1e3 * (t2 - t1), covariance_ms=1e3 * (t3 - t2),
                 rows_used=rows)
        if rows > 20:
            t4 = time.perf_counter()
            M0, _ = pca_initial_M(cov, 20)
            r["eigh_ms"] = 1e3 * (time.perf_counter() - t4)
            x0 = np.concatenate([M0.ravel(order="F"), np.log(std), [np.log(0.1), np.log(0.0023), np.log(3.65)]])
            if meanflux:
                t.set_lyseries(31)
            t5 = time.perf_counter()
            _, _, res = fit_training_set(t, x0, max_iter=a.fit_iters, max_fun_evals=4 * a.fit_iters + 10)
            r.update(fit_s=time.perf_counter() - t5, fit_iterations=res.nit, fit_evaluations=res.nfev)
        t.close()
        if not a.no_cpu:
            c0 = time.perf_counter()
            F, _, _ = R.rest_grid(csr, 1217, max_noise_variance=p.max_noise_variance,
                                  num_forest_lines=31 if meanflux else 0)
            c1 = time.perf_counter()
            _, centered, _, _ = R.column_stats(F)
            R.pca_covariance(centered, meanflux)
            c2 = time.perf_counter()
            r.update(cpu_numpy_rest_grid_s=c1 - c0, cpu_numpy_stats_and_covariance_s=c2 - c1)
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
