"""The synthetic batch of the refine tests (tests/test_refine.py on the CPU twin, tests/test_gpu_refine.py on
the GPU): eight quasars of 150-400 pixels, one of every kind the refine pass treats differently, and the
twin itself -- the restatement's boxes around the CPU oracle's sweep -- computed once per (k, lines, S')."""
import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import Parameters

import refine_restatement as RR

S = 200
SR_VALUES = (127, 128, 300)   # S' + 1 just below, on and above a 128-sample block of the k <= 20 sweep
KINDS = ("strong", "broad", "none", "edge", "status1", "status3", "masked_run", "strong_masked")
PIXELS = (300, 257, 150, 400, 180, 220, 333, 260)
PEAKED = ("strong", "strong_masked")   # the rows whose injected absorber the first pass finds (the twin shows it)
# four levels: with S = 200 a level shrinks the box by about 4 / sqrt(S') only, so two levels (the default, made
# for S = 10^4) do not reach the width of a peaked posterior here
LEVELS, DELTA, PAD = 4, 12.5, 2.0
# A search range of zero width (max_z == min_z) needs a quasar with ONE kept pixel and max_z_cut = 0 (k_prepare:
# max_z = kept_max / lya - 1 - max_z_cut, min_z = kept_min / lya - 1).  max_z_cut belongs to the context, so
# that row lives in a second small batch of its own, next to an ordinary strong row.
ZR_KINDS = ("strong", "zero_range")
ZR_PIXELS = (300, 240)
ZR_SR = 128
CONFIGS = ((8, 3), (24, 5))   # (k, lines): the 896-B and the 1536-B record class; compile-time and run-time lines


def halton_points(n):
    """Plain Halton points of bases 2 and 3 from index 1: the CPU stand-in for the default point set (the
    tests hand the same arrays to the GPU, so the twin and the GPU see one set)."""
    return synthetic.halton(n, 2), synthetic.halton(n, 3)


def batch_parameters(num_lines, zero_range=False):
    return Parameters(num_lines=num_lines, max_z_cut=0.0) if zero_range else Parameters(num_lines=num_lines)


def make_batch(k, num_lines, zero_range=False):
    """(model, samples, spectra, truth): truth[i] = (z_dla, log_nhi) of the injected absorber or None.
    ``zero_range``: the two-quasar batch of ZR_KINDS, for a context with max_z_cut = 0."""
    p = batch_parameters(num_lines, zero_range)
    model, samples = synthetic.make_model(k), synthetic.make_samples(S)
    spectra, truth = [], []
    for i, (kind, n) in enumerate(zip(ZR_KINDS, ZR_PIXELS) if zero_range else zip(KINDS, PIXELS)):
        sp = synthetic.make_spectrum(7000 + 2 * i, n, model, p)   # even index: no absorber of its own
        wl = sp["wavelengths"]
        rest = wl / (1 + sp["z_qso"])
        inside = wl[(rest >= p.min_lambda) & (rest <= p.max_lambda)]   # the search range is that of these pixels
        zmin, zmax = p.min_z_dla(inside, sp["z_qso"]), p.max_z_dla(inside, sp["z_qso"])
        inject = None
        if kind in ("strong", "strong_masked"):
            inject = (zmin + 0.45 * (zmax - zmin), 21.2)
        elif kind == "broad":
            inject = (zmin + 0.6 * (zmax - zmin), 20.1)
        elif kind == "edge":
            inject = (zmax - 1e-4 * (zmax - zmin), 20.9)
        if inject is not None:
            sp["flux"] = sp["flux"] * synthetic._injected_absorption(wl, inject[0], 10.0 ** inject[1], num_lines)
        mask = np.zeros(wl.size, dtype=np.uint8)
        if kind == "status1":
            mask[:] = 1
        elif kind == "masked_run":
            mask[n // 3:n // 3 + 12] = 1
        elif kind == "strong_masked":
            mask[np.random.default_rng(5).uniform(size=wl.size) < 0.05] = 1
        elif kind == "zero_range":   # one kept pixel in the middle of the modelled range
            mask[:] = 1
            mask[wl.size // 2] = 0
        if kind == "status3":
            sp["noise_variance"] = sp["noise_variance"].copy()
            sp["noise_variance"][n // 2] = 0.0
        sp["noise_variance"] = np.where(mask == 1, np.inf, sp["noise_variance"])
        sp["flux"] = np.where(mask == 1, np.nan, sp["flux"])
        sp["pixel_mask"] = mask
        spectra.append(sp)
        truth.append(inject)
    return model, samples, spectra, truth


_TWINS = {}


def oracle_parameters(num_lines, zero_range=False):
    from oracle import oracle
    return oracle.OracleParams(num_lines=num_lines, max_z_cut=0.0) if zero_range else oracle.OracleParams(num_lines=num_lines)


def twin(k, num_lines, Sr, levels=LEVELS, zero_range=False):
    """The whole feature on the CPU: the oracle's first pass per quasar, then the restatement with the
    oracle as its sweep, in float64.  Returns (batch, first-pass list, refined rows)."""
    key = (k, num_lines, Sr, levels, zero_range)
    if key not in _TWINS:
        from oracle import oracle
        batch = make_batch(k, num_lines, zero_range)
        model, samples, spectra, _ = batch
        u, v = halton_points(Sr)
        first, rows = [], []
        for kind, sp in zip(ZR_KINDS if zero_range else KINDS, spectra):
            if kind == "status3":   # (the oracle, like the reference, does not look at noise variances)
                ref = dict(rc=3, min_z_dla=np.nan, max_z_dla=np.nan, sample_log_likelihoods_dla=np.full(S, np.nan))
            else:
                ref = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"],
                                              sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"],
                                              oracle_parameters(num_lines, zero_range))
            first.append(ref)
            status = 0 if ref["rc"] == 0 else 1
            rows.append(RR.refine_row(ref["sample_log_likelihoods_dla"], samples["offset_samples"], samples["log_nhi_samples"],
                                      ref["min_z_dla"], ref["max_z_dla"], status, u, v,
                                      RR.oracle_sweep(model, sp, ref["min_z_dla"], ref["max_z_dla"], oracle_parameters(num_lines, zero_range)), levels,
                                      DELTA, PAD))
        _TWINS[key] = (batch, first, rows)
    return _TWINS[key]


def ess(l):
    """T^2 / Sum w^2 of a row of log weights."""
    l = np.asarray(l, dtype=np.float64)
    l = l[~np.isnan(l)]
    w = np.exp(l - l.max())
    return float(w.sum() ** 2 / (w * w).sum())


def test_prior():
    """A column density prior whose breaks fall inside the boxes of the batch: the uniform component on [20.3, 21.3]
    only and the fitted density held flat below 20.2 (the fields of gpdla_nhi_prior; Z is not renormalised, which
    the refine pass does not ask for)."""
    return dict(coeff=(-0.4, -1.1, -0.35), centre=21.0, alpha=0.9, uniform_min=20.3, uniform_max=21.3, lower=20.0,
                flat_below=20.2, Z=0.83)
