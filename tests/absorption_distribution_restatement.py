"""NumPy-and-oracle restatement of the absorption distribution (include/gpdla.h) -- a plain module:
tests/test_absorption_distribution.py and tests/test_gpu_absorption_distribution.py import it.  The grid, the weights and the
profile matrices are those of tests/model_spectra_restatement.py and tests/model_spectra_multi_restatement.py, imported.

From the definitions: an ATOM is (mass p_m w_{m,i}, abar_{m,i}(p) = clip(a, 0, 1)), the null component one atom of mass
p_null at abar = 1; only atoms of positive mass are in the support.
  F_p(t) = Sum mass [abar <= t];  min / max over the support;  H_b = Sum mass [bin(abar) = b],
  bin(x) = min(B - 1, (int)(x B));  C_b = H_0 + .. + H_b;  the quantile of level l: b* the first b with C_b >= l (none: B - 1),
  q = (b* + clamp((l - C_{b*-1}) / H_{b*}, 0, 1)) / B, clamped to [min, max].

The library and this module agree on a profile to the Voigt parity only (2e-13 per profile), and an indicator flips at
abar = t.  So every quantity also comes as BOUNDS, from profiles moved by DELTA = 1e-12 (four profiles' worth, which covers a
product of up to four): F_lo with abar + DELTA, F_hi with abar - DELTA; the cumulative histogram likewise (bin edges moved
by -/+ DELTA); min and max -/+ DELTA; the quantile as the stated function of the moved cumulative sums (it falls when they
rise) and of the moved clamp.  EPS = 1e-11 is what a convex sum over S profiles may round by.
"""
from __future__ import annotations

import numpy as np

import model_spectra_multi_restatement as RM
import model_spectra_restatement as R

DELTA = 1e-12   # TOL_MAP of tests/test_gpu_model_spectra.py
EPS = 1e-11     # TOL_MOMENTS of the same file
LOOSE = 1e-9    # a bound wider than this says little (the non-vacuity condition counts them)

grid, weights, sample_profiles = R.grid, R.weights, RM.sample_profiles


def product_profiles(C, base, n: int) -> np.ndarray:
    """[S, n_u]: the profile of every sample of model DLA(n) from the gathered rows of C = sample_profiles(..), in slot
    order; a sample one of whose slots was never drawn gets ones (its weight is 0)."""
    A = np.ones_like(C)
    for i in range(C.shape[0]):
        s = RM.slots(base, n, i)
        if s is None:
            continue
        A[i] = C[s[0]]
        for sj in s[1:]:
            A[i] = A[i] * C[sj]
    return A


def atoms(components, p_null: float, n_u: int):
    """``(mass [N], abar [N, n_u], is_null [N])`` of the support.  ``components``: (p_m, w [S_m], A [S_m, n_u]) in
    component order, p_m already normalised."""
    mass, rows, null = [], [], []
    for p_m, w, A in components:
        if not p_m > 0:
            continue
        keep = np.asarray(w) > 0
        mass.append(p_m * np.asarray(w)[keep])
        rows.append(np.clip(np.asarray(A)[keep], 0.0, 1.0))
        null.append(np.zeros(int(keep.sum()), dtype=bool))
    if p_null > 0:
        mass.append(np.array([p_null]))
        rows.append(np.ones((1, n_u)))
        null.append(np.ones(1, dtype=bool))
    return np.concatenate(mass), np.vstack(rows), np.concatenate(null)


def _moved(X, is_null, shift):
    return np.where(is_null[:, None], X, X + shift)   # (the null atom is exact)


def prob_below(mass, X, is_null, thresholds, shift: float = 0.0) -> np.ndarray:
    Y = _moved(X, is_null, shift)
    return np.stack([mass @ (Y <= t) for t in thresholds]) if len(thresholds) else np.zeros((0, X.shape[1]))


def bins_of(Y, B: int) -> np.ndarray:
    return np.minimum(B - 1, np.maximum(np.floor(Y * float(B)), 0)).astype(np.int64)


def histogram(mass, X, is_null, B: int, shift: float = 0.0) -> np.ndarray:
    """[B, n_u]"""
    b = bins_of(_moved(X, is_null, shift), B)
    H = np.zeros((B, X.shape[1]))
    for p in range(X.shape[1]):
        H[:, p] = np.bincount(b[:, p], weights=mass, minlength=B)
    return H


def quantile_of(C, level: float, lo, hi) -> np.ndarray:
    """The stated function of a cumulative histogram C [B, n_u] (C_{-1} = 0) and the clamp [lo, hi]."""
    B, n = C.shape
    Cp = np.vstack([np.zeros((1, n)), C[:-1]])
    H = C - Cp
    reach = C >= level
    bstar = np.where(reach.any(axis=0), reach.argmax(axis=0), B - 1)
    cols = np.arange(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = (level - Cp[bstar, cols]) / H[bstar, cols]
    frac = np.clip(np.nan_to_num(frac, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
    return np.clip((bstar + frac) / float(B), lo, hi)


def distribution(components, p_null: float, n_u: int, thresholds=(), B: int = 0, levels=()) -> dict:
    """Everything, with its bounds: ``prob_below`` (and ``_lo`` / ``_hi``), ``absorption_min`` / ``_max``, ``histogram``,
    ``cumulative`` (``_lo`` / ``_hi``), ``quantiles`` (``_lo`` / ``_hi``)."""
    mass, X, is_null = atoms(components, p_null, n_u)
    out = dict(prob_below=prob_below(mass, X, is_null, thresholds),
               prob_below_lo=prob_below(mass, X, is_null, thresholds, +DELTA),
               prob_below_hi=prob_below(mass, X, is_null, thresholds, -DELTA),
               absorption_min=X.min(axis=0), absorption_max=X.max(axis=0))
    if B:
        out["histogram"] = histogram(mass, X, is_null, B)
        out["cumulative"] = np.cumsum(out["histogram"], axis=0)
        out["cumulative_lo"] = np.cumsum(histogram(mass, X, is_null, B, +DELTA), axis=0)
        out["cumulative_hi"] = np.cumsum(histogram(mass, X, is_null, B, -DELTA), axis=0)
        mn, mx = out["absorption_min"], out["absorption_max"]
        if len(levels):
            out["quantiles"] = np.stack([quantile_of(out["cumulative"], l, mn, mx) for l in levels])
            out["quantiles_lo"] = np.stack([quantile_of(out["cumulative_hi"] + EPS, l, mn - DELTA, mx - DELTA) for l in levels])
            out["quantiles_hi"] = np.stack([quantile_of(np.maximum(out["cumulative_lo"] - EPS, 0.0), l, mn + DELTA, mx + DELTA)
                                            for l in levels])
    return out


def loose_counts(d: dict) -> tuple:
    """(loose, compared) over the entries a GPU comparison of ``d`` makes: (pixel, threshold), (pixel, bin edge),
    (pixel, level)."""
    loose = compared = 0
    for lo, hi in (("prob_below_lo", "prob_below_hi"), ("cumulative_lo", "cumulative_hi"), ("quantiles_lo", "quantiles_hi")):
        if lo in d:
            width = np.abs(d[hi] - d[lo])
            loose += int((width > LOOSE).sum())
            compared += int(width.size)
    return loose, compared


def failures(got: dict, want: dict, sl: slice, label: str = "") -> list:
    """``lo - EPS <= gpu <= hi + EPS`` for every compared entry of pixels ``sl`` of a library result against
    :func:`distribution`; min / max within DELTA.  Returns the violations as text; every figure is printed."""
    bad = []

    def check(name, g, lo, hi, tol):
        g = np.asarray(g)
        if np.isnan(g).any():
            bad.append(f"{label} {name}: NaN where the restatement is finite")
            return
        over = max(float((lo - g).max(initial=0.0)), float((g - hi).max(initial=0.0)))
        print(f"{label} {name}: worst excursion beyond the bounds {over:.3e} (allowed {tol:.1e})")
        if over > tol:
            bad.append(f"{label} {name}: {over:.3e} beyond the bounds")
    if "prob_below" in got and got["prob_below"].shape[0]:
        check("prob_below", got["prob_below"][:, sl], want["prob_below_lo"], want["prob_below_hi"], EPS)
    check("absorption_min", got["absorption_min"][sl], want["absorption_min"] - DELTA, want["absorption_min"] + DELTA, 0.0)
    check("absorption_max", got["absorption_max"][sl], want["absorption_max"] - DELTA, want["absorption_max"] + DELTA, 0.0)
    if "histogram" in got:
        check("cumulative histogram", np.cumsum(got["histogram"][:, sl], axis=0), want["cumulative_lo"], want["cumulative_hi"], EPS)
    if "quantiles" in got:
        check("quantiles", got["quantiles"][:, sl], want["quantiles_lo"], want["quantiles_hi"], EPS)
    return bad


# ------------------------------------------------------------------------------------------------
# the cases the CPU test and the GPU test share: host tables, so that no sweep is needed to state them
# ------------------------------------------------------------------------------------------------

SAMPLE_COUNTS = (1, 63, 64, 257, 300)     # around the lane, the wave's 64-sample group and the block's four groups
PIXEL_COUNTS = (1, 15, 16, 17, 33, 63, 64, 65)  # the 16-pixel tile and the 64-pixel range of the kernel without bins
THRESHOLDS4 = (0.8, 0.5, 0.2, 0.95)
LEVELS8 = (0.025, 0.16, 0.3, 0.5, 0.7, 0.84, 0.9, 0.975)


def table_row(samples, rng, width=0.08, S=None) -> np.ndarray:
    """A row of sample log-likelihoods peaked at a random (offset, log N): a posterior of a few dozen live samples."""
    u, n = np.asarray(samples["offset_samples"]), np.asarray(samples["log_nhi_samples"])
    u0, n0 = rng.uniform(0.2, 0.8), rng.uniform(20.3, 22.0)
    return -0.5 * ((u - u0) / width) ** 2 - 0.5 * ((n - n0) / (4 * width)) ** 2 + rng.normal(0, 0.3, u.size)


def shape_cases() -> list:
    """(S, n_u, request) over the sample and pixel edges; every request form appears."""
    requests = [dict(thresholds=(0.8,)), dict(thresholds=THRESHOLDS4), dict(thresholds=(0.8,), bins=8, levels=(0.5,), histogram=True),
                dict(thresholds=(0.8, 0.5), bins=50, levels=LEVELS8, histogram=True), dict(thresholds=(0.8,), bins=64, levels=LEVELS8, histogram=True),
                dict(thresholds=THRESHOLDS4, bins=256, levels=(0.16,), histogram=True), dict(thresholds=(0.8,), bins=64, levels=(0.16, 0.84))]
    cases, r = [], 0
    for S in SAMPLE_COUNTS:
        for n_u in PIXEL_COUNTS:
            cases.append((S, n_u, requests[r % len(requests)]))
            r += 1
    return cases


def case_inputs(S: int, n_u_list, seed: int):
    """(model, samples, spectra, host table [n, S]) of one sample count: a ``synthetic.make_spectrum`` quasar per pixel count."""
    from gp_dla_detection_amd import synthetic
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(5200 + n, n, model) for n in n_u_list]
    rng = np.random.default_rng(seed)
    table = np.stack([table_row(samples, rng) for _ in spectra])
    return model, samples, spectra, table


def restate_single(oracle, model, samples, sp, row, request: dict, num_lines: int = 3, window=None) -> dict:
    """The DLA component alone (weight 1) of one quasar under a host row.  ``window`` = (first pixel, count): those grid
    pixels only (the profiles of a pixel need its own seven padded wavelengths and nothing else)."""
    g = grid(oracle, model, sp)
    if window is not None:
        g = dict(g, pad=g["pad"][window[0]:window[0] + window[1] + 6], n_u=window[1])
    A = sample_profiles(oracle, g, samples["offset_samples"], samples["nhi_samples"], num_lines)
    return distribution([(1.0, weights(row), A)], 0.0, g["n_u"], request.get("thresholds", ()),
                        request.get("bins", 0) if (request.get("histogram") or request.get("levels")) else 0,
                        request.get("levels") or ())


# the four further host-table cases of the GPU test, built here so that the CPU test can count their loose bounds too

REQUEST_ALL = dict(thresholds=THRESHOLDS4, bins=64, levels=LEVELS8, histogram=True)
REQUEST_MIX = dict(thresholds=(0.8, 0.5), bins=64, levels=(0.16, 0.5, 0.84), histogram=True)
SCALE_WINDOWS = ((0, 0), (21, 696), (63, 1420))   # (quasar, first pixel) of 80 pixels: across pixels 64; 704 and 768; 1472


def _restate(request, components, p_null, n_u):
    return distribution(components, p_null, n_u, request["thresholds"], request["bins"], request["levels"])


def production_case():
    """The tile-boundary run of tests/production_shapes.py and a 33-pixel quasar, S = 300."""
    import production_shapes as ps
    from gp_dla_detection_amd import synthetic
    model = synthetic.make_model(20)
    strat = ps.stratified_quasars(20)
    spectra = [strat[ps.by_stratum(strat, "tile_boundary_run")], synthetic.make_spectrum(5300, 33, model)]
    samples = synthetic.make_samples(300)
    rng = np.random.default_rng(41)
    return model, samples, spectra, np.stack([table_row(samples, rng) for _ in spectra])


def production_restated(oracle) -> list:
    model, samples, spectra, table = production_case()
    return [restate_single(oracle, model, samples, sp, table[s], REQUEST_ALL) for s, sp in enumerate(spectra)]


def mixture_case():
    """(null, sub-DLA, DLA) with unequal weights, S = 257."""
    from gp_dla_detection_amd import synthetic
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(257)
    spectra = [synthetic.make_spectrum(5500, 65, model), synthetic.make_spectrum(5501, 33, model)]
    rng = np.random.default_rng(9)
    dla = np.stack([table_row(samples, rng) for _ in spectra])
    lls = np.stack([table_row(samples, rng) for _ in spectra])
    return model, samples, spectra, dla, lls, np.array([[0.2, 0.3, 0.5], [0.7, 0.0, 0.6]])   # (row 1 sums to 1.3)


def mixture_restated(oracle) -> list:
    model, samples, spectra, dla, lls, pw = mixture_case()
    out = []
    for s, sp in enumerate(spectra):
        g = grid(oracle, model, sp)
        p = pw[s] / pw[s].sum()
        A_dla = sample_profiles(oracle, g, samples["offset_samples"], samples["nhi_samples"], 3)
        A_lls = sample_profiles(oracle, g, samples["offset_samples"], samples["lls_nhi_samples"], 3)
        out.append(_restate(REQUEST_MIX, [(p[1], weights(lls[s]), A_lls), (p[2], weights(dla[s]), A_dla)], p[0], g["n_u"]))
    return out


def multi_case():
    """max_dlas = 3, S = 300: host tables with peaked rows for every model and base rows that draw (almost) everywhere."""
    from gp_dla_detection_amd import synthetic
    from gp_dla_detection_amd.parameters import MultiParameters
    params = MultiParameters(max_dlas=3)
    model = synthetic.make_model(20)
    S = 300
    samples = synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(5700 + i, 33 + 16 * i, model) for i in range(2)]
    rng = np.random.default_rng(12)
    t2 = dict(sample_log_likelihoods_dla=np.stack([[table_row(samples, rng) for _ in range(3)] for _ in spectra]),
              sample_log_likelihoods_lls=np.stack([table_row(samples, rng) for _ in spectra]),
              base_sample_inds=rng.integers(1, S + 1, size=(2, 2, S)).astype(np.uint32))
    t2["base_sample_inds"][1, 1, ::7] = 0                   # never drawn: those samples of DLA(3) weigh 0
    return params, model, samples, spectra, t2, np.array([[0.1, 0.1, 0.3, 0.3, 0.2], [0.0, 0.2, 0.0, 0.4, 0.4]])


def multi_restated(oracle) -> list:
    params, model, samples, spectra, t2, pw = multi_case()
    out = []
    for s, sp in enumerate(spectra):
        g = grid(oracle, model, sp, params)
        Cd = sample_profiles(oracle, g, samples["offset_samples"], samples["nhi_samples"], params.num_lines)
        Cl = sample_profiles(oracle, g, samples["offset_samples"], samples["lls_nhi_samples"], params.num_lines)
        base = t2["base_sample_inds"][s]
        comps = [(pw[s, 1], weights(t2["sample_log_likelihoods_lls"][s]), Cl)]
        for n in (1, 2, 3):
            comps.append((pw[s, 1 + n], weights(RM.effective_row(t2["sample_log_likelihoods_dla"][s, n - 1], base, n)),
                          product_profiles(Cd, base, n)))
        out.append(_restate(REQUEST_MIX, comps, pw[s, 0], g["n_u"]))
    return out


def scale_case():
    """64 quasars (four spectra of 1500 pixels, repeated) x 10^4 samples, a host row each."""
    from gp_dla_detection_amd import synthetic
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(10000)
    base = [synthetic.make_spectrum(5900 + i, 1500, model) for i in range(4)]
    spectra = [base[i % 4] for i in range(64)]
    rng = np.random.default_rng(77)
    return model, samples, spectra, np.stack([table_row(samples, rng, width=0.03) for _ in spectra])


def scale_restated(oracle, case=None) -> list:
    model, samples, spectra, table = case or scale_case()
    return [restate_single(oracle, model, samples, spectra[s], table[s], REQUEST_MIX, window=(first, 80)) for s, first in SCALE_WINDOWS]
