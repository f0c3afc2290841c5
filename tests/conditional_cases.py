"""The synthetic batch of the fixed-absorber tests (tests/test_conditional.py on the CPU twin,
tests/test_gpu_conditional.py on the GPU): five quasars with zero, one or two injected absorbers,
the "science" rows, and four rows of parity only -- one of every kind the conditioning treats differently."""
import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import refine_cases as RC

S = 200
DELTA, PAD = 12.5, 2.0
# (k, lines, S', levels): both slim record classes; compile-time and run-time line counts
CONFIGS = ((8, 3, 128, 4), (24, 5, 300, 4))
# kind, index of synthetic.make_spectrum (even: no absorber of its own), pixels, injected (fraction of the range, log N)
SCIENCE = (("two_far", 7100, 400, ((0.25, 21.2), (0.75, 20.9))),
           ("two_near", 7102, 400, ((0.45, 21.1), (0.55, 21.0))),
           ("strong", 7104, 300, ((0.45, 21.2),)),
           ("none", 7106, 150, ()),
           ("two_unequal", 7110, 333, ((0.3, 21.3), (0.8, 20.5))))
# parity only: no science condition is asked of these
EXTRA = (("status1", 7112, 180, ()),            # all pixels masked
         ("status3", 7114, 220, ()),            # one noise variance 0
         ("strong_masked", 7104, 300, ((0.45, 21.2),)),   # `strong` with 5 % of its pixels masked
         ("outside", 7116, 260, ((0.5, 20.8),)))          # takes a fixed absorber whose Lyman alpha lies outside the spectrum
KINDS = tuple(r[0] for r in SCIENCE + EXTRA)
TWO = ("two_far", "two_near", "two_unequal")
SEPARATION = MultiParameters().min_z_separation


def search_range(sp, p):
    """(zmin, zmax) of the pixels inside the modelled range, as tests/refine_cases.make_batch computes it."""
    wl = sp["wavelengths"]
    rest = wl / (1 + sp["z_qso"])
    inside = wl[(rest >= p.min_lambda) & (rest <= p.max_lambda)]
    return p.min_z_dla(inside, sp["z_qso"]), p.max_z_dla(inside, sp["z_qso"])


_BATCHES = {}


def make_batch(k, num_lines, extra=True):
    """(model, samples, spectra, truth): truth[i] = [(z_dla, log_nhi), ...] of the injected absorbers.  Cached:
    the arrays are shared and must not be written to."""
    key = (k, num_lines, bool(extra))
    if key in _BATCHES:
        return _BATCHES[key]
    p = Parameters(num_lines=num_lines)
    model, samples = synthetic.make_model(k), synthetic.make_samples(S)
    spectra, truth = [], []
    for kind, index, n, injected in SCIENCE + (EXTRA if extra else ()):
        sp = synthetic.make_spectrum(index, n, model, p)
        wl = sp["wavelengths"]
        zmin, zmax = search_range(sp, p)
        inj = [(zmin + f * (zmax - zmin), ln) for f, ln in injected]
        for z, ln in inj:
            sp["flux"] = sp["flux"] * synthetic._injected_absorption(wl, z, 10.0 ** ln, num_lines)
        mask = np.zeros(wl.size, dtype=np.uint8)
        if kind == "status1":
            mask[:] = 1
        elif kind == "strong_masked":
            mask[np.random.default_rng(5).uniform(size=wl.size) < 0.05] = 1
        if kind == "status3":
            sp["noise_variance"] = sp["noise_variance"].copy()
            sp["noise_variance"][n // 2] = 0.0
        sp["noise_variance"] = np.where(mask == 1, np.inf, sp["noise_variance"])
        sp["flux"] = np.where(mask == 1, np.nan, sp["flux"])
        sp["pixel_mask"] = mask
        spectra.append(sp)
        truth.append(inj)
    _BATCHES[key] = (model, samples, spectra, truth)
    return _BATCHES[key]


def parity_lists(k, num_lines, F):
    """Lists of F fixed absorbers per quasar of make_batch for the parity tests: the injected absorbers first, then
    points spread over the search range at least four separations from everything listed; the `outside` row's first
    fixed absorber lies redward of the quasar's Lyman alpha emission (z > z_qso: no pixel of the spectrum is near its
    Lyman alpha line)."""
    p = Parameters(num_lines=num_lines)
    _, _, spectra, truth = make_batch(k, num_lines)
    lists = []
    for kind, sp, inj in zip(KINDS, spectra, truth):
        zmin, zmax = search_range(sp, p)
        out = [[sp["z_qso"] + 0.3, 20.6]] if kind == "outside" else []
        out += [[z, ln] for z, ln in inj]
        cand = [zmin + f * (zmax - zmin) for f in (0.12, 0.62, 0.9, 0.37, 0.05, 0.97, 0.5, 0.2, 0.7, 0.83, 0.3)]
        lnhis = (20.4, 20.9, 20.2, 21.4, 20.6, 20.1, 20.7, 21.0)
        for z in cand:
            if len(out) >= F:
                break
            if all(abs(z - a[0]) >= 4 * SEPARATION for a in out):
                out.append([z, lnhis[len(out)]])
        assert len(out) >= F, (kind, F)
        lists.append(out[:F])
    return lists


def halton_points(Sr):
    return RC.halton_points(Sr)


def edge_spectrum(n_u, model, num_lines, masked):
    """A quasar of exactly n_u pixels in the modelled range (the tile edges of the conditioning kernel), 5 % of them
    masked where asked."""
    p = Parameters(num_lines=num_lines)
    sp = synthetic.make_spectrum(7200 + 2 * n_u, n_u, model, p)
    mask = np.zeros(sp["wavelengths"].size, dtype=np.uint8)
    if masked:
        mask[np.random.default_rng(n_u).uniform(size=mask.size) < 0.05] = 1
        mask[sp["wavelengths"].size // 2] = 0   # (at least one pixel is kept)
    sp["noise_variance"] = np.where(mask == 1, np.inf, sp["noise_variance"])
    sp["flux"] = np.where(mask == 1, np.nan, sp["flux"])
    sp["pixel_mask"] = mask
    return sp
