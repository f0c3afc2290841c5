#!/usr/bin/env python3
"""Exact-arithmetic anchor on the production shape (run in the BUILD container only): the method of
make_exact.py (``exact_log_mvnpdf``: 50-digit Woodbury at the very fp64 inputs) for ONE quasar of
tests/production_shapes.py -- ``first_masked_za``: BOSS grid, z_qso = 2.5, the spectrograph's blue edge
inside the modelled range, its first six in-range pixels masked, so the search range starts at the
first KEPT pixel (the ``za`` branch of set_parameters.m:70-73), 677 kept of 727 pixels, k = 20.

Writes tests/golden/exact_boss_blue_edge.npz: the quasar, what the oracle dumps for it (interpolated
model, padded wavelengths, sample redshifts), the exact null log-likelihood (process_qsos.m:149-151)
and the exact log-likelihood of 32 samples of ``production_samples(1000)`` -- 28 picked at random plus
the four corners of the sample box (offset exactly 0 / 1 at N_HI 1e20 / 1e23) -- at the fp64 inputs
process_qsos.m:190-198 forms from the oracle's absorption vectors, which are stored too.

Usage:  python tests/golden/make_exact_boss.py        (about a minute)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]

from make_exact import exact_log_mvnpdf  # noqa: E402

STRATUM, K, S = "first_masked_za", 20, 1000


def main():
    import production_shapes as P
    from gp_dla_detection_amd import synthetic
    from oracle import oracle
    model = synthetic.make_model(K)
    samples = P.production_samples(S)
    spectra = P.stratified_quasars(K)
    sp = spectra[P.by_stratum(spectra, STRATUM)]
    c = P.census([sp])[0]
    assert c["za_wins"] and c["first_masked"] and c["leading_masked"] == P.FIRST_RUN
    r = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"],
                                sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"],
                                num_threads=0, dump=True)
    assert r["rc"] == 0 and r["n_kept"] == c["n_kept"] and r["n_unmasked"] == c["n_unmasked"]
    out = dict(wavelengths=sp["wavelengths"], flux=sp["flux"], noise_variance=sp["noise_variance"],
               pixel_mask=sp["pixel_mask"], z_qso=np.array(sp["z_qso"]), n_kept=np.array(r["n_kept"]),
               n_unmasked=np.array(r["n_unmasked"]), min_z_dla=np.array(r["min_z_dla"]),
               max_z_dla=np.array(r["max_z_dla"]))
    for key in ("this_mu", "this_M", "this_omega2", "padded_wavelengths", "sample_z_dlas"):
        out[key] = r[key]
    inside = P.in_range(sp)
    mask = sp["pixel_mask"].astype(bool)
    ind = inside & ~mask                                           # process_qsos.m:110
    keep_u = ~mask[inside]                                         # :181
    y, nv = sp["flux"][ind], sp["noise_variance"][ind]
    mu, M, om2 = r["this_mu"], r["this_M"], r["this_omega2"]
    null = exact_log_mvnpdf(y, mu, M, om2 + nv)                    # :149-151
    out["null_log_p_exact"] = np.array(null)
    worst = abs(r["log_likelihood_no_dla"] - null)
    print(f"null: exact {null!r}  oracle-exact {r['log_likelihood_no_dla'] - null:+.3e}", flush=True)
    rng = np.random.default_rng(20260103)
    pick = np.concatenate([np.sort(rng.choice(S, 28, replace=False)), S + np.arange(4)])
    absorptions, exact = [], []
    for i in pick:
        a_u = oracle.voigt(r["padded_wavelengths"], float(r["sample_z_dlas"][i]),
                           float(samples["nhi_samples"][i]), 3)    # :187-188
        a = a_u[keep_u]                                            # :190
        ex = exact_log_mvnpdf(y, mu * a, M * a[:, None], om2 * a ** 2 + nv)   # :192-198
        absorptions.append(a)
        exact.append(ex)
        d = float(r["sample_log_likelihoods_dla"][i]) - ex
        worst = max(worst, abs(d))
        print(f"sample {i} (offset {samples['offset_samples'][i]:.4f}, log N_HI {samples['log_nhi_samples'][i]:.3f}): "
              f"exact {ex!r}  oracle-exact {d:+.3e}", flush=True)
    out["sample_indices"] = pick
    out["absorption"] = np.stack(absorptions)
    out["sample_log_p_exact"] = np.array(exact)
    path = os.path.join(HERE, "exact_boss_blue_edge.npz")
    np.savez_compressed(path, **out)
    print(f"worst |oracle - exact| = {worst:.3e}")
    print("wrote exact_boss_blue_edge.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
