#!/opt/conda/bin/python3.9
"""BUILD CONTAINER ONLY: golden vectors for ``dla_model_mean`` -- the reference's ``this_mu``
(QSOLoader.plot_this_mu, CDDF_analysis/qso_loader.py:1685-1711) -- from the reference's OWN
``Voigt_absorption`` (CDDF_analysis/voigt.py:230-275) and ``QSOLoader.total_scale_factor``
(qso_loader.py:1777-1822).  Importing the module needs h5py, hence the conda interpreter.

    /opt/conda/bin/python3.9 tests/golden/make_model_mean.py   ->  tests/golden/model_mean.npz

Inputs and the numbers the reference computed are stored: a rest grid and a mean vector shaped like
the package's synthetic model, and per case z_qso, the absorbers, the line counts and ``this_mu``."""
import os
import sys

import numpy as np

np.bool, np.int, np.float = bool, int, float  # aliases the reference still uses (removed in NumPy 1.24)
sys.path.insert(0, "/root/reference")
from CDDF_analysis.qso_loader import QSOLoader  # noqa: E402
from CDDF_analysis.voigt import Voigt_absorption  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
G = 1217
rest = 911.75 + 0.25 * np.arange(G)
u = (rest - rest[0]) / (rest[-1] - rest[0])
mu = 1.0 + 0.3 * np.exp(-0.5 * ((u - 0.95) / 0.08) ** 2) + 0.1 * np.exp(-0.5 * ((u - 0.38) / 0.03) ** 2)

# (z_qso, [(z_dla, log_nhi)], num_voigt_lines, num_forest_lines, suppressed)
CASES = [
    (2.6, [], 3, 31, True),
    (2.6, [], 3, 31, False),
    (3.1, [(2.85, 20.9)], 1, 31, True),
    (3.1, [(2.85, 20.9)], 3, 31, False),
    (3.6, [(3.05, 20.3), (3.41, 21.6)], 3, 5, True),
    (4.2, [(3.3, 20.05), (3.71, 22.4), (4.02, 20.6)], 31, 31, True),
    (2.9, [(2.2, 20.2), (2.45, 21.1), (2.6, 20.7), (2.81, 22.9)], 31, 1, True),
    (3.3, [(2.75, 23.0), (3.1, 20.0), (3.18, 21.3), (3.25, 20.45)], 1, 31, False),
]
out = dict(rest_wavelengths=rest, mu=mu, num_cases=len(CASES), tau=0.0023, beta=3.65)
for i, (z_qso, absorbers, nv, nf, suppressed) in enumerate(CASES):
    this_mu = mu
    if suppressed:
        this_mu = this_mu * QSOLoader.total_scale_factor(0.0023, 3.65, z_qso, rest, num_lines=nf)
    for z_dla, log_nhi in absorbers:
        this_mu = this_mu * Voigt_absorption(rest * (1 + z_qso), 10 ** log_nhi, z_dla, num_lines=nv)
    out[f"z_qso_{i}"] = z_qso
    out[f"z_dlas_{i}"] = np.array([a[0] for a in absorbers], dtype=np.float64)
    out[f"log_nhis_{i}"] = np.array([a[1] for a in absorbers], dtype=np.float64)
    out[f"num_voigt_lines_{i}"], out[f"num_forest_lines_{i}"], out[f"suppressed_{i}"] = nv, nf, suppressed
    out[f"this_mu_{i}"] = this_mu
np.savez_compressed(os.path.join(HERE, "model_mean.npz"), **out)
print("wrote model_mean.npz:", [float(out[f"this_mu_{i}"].min()) for i in range(len(CASES))])
