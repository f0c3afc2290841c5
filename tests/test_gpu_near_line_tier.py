"""The accurate Voigt tier of the three-line sweeps, taken line by line (near_lines3 in csrc/voigt_tiers.hpp): in a
K-step whose wave votes, only the lanes within 30 Doppler widths of a line replace that line's term, by the
piecewise polynomial on the reference's velocity (voigt.c:282-289); every other lane and line keeps its wing-tier
term.  k_sweep_slim<3> and, through one refine level, k_sweep_slim_boxed<3> against the CPU oracle:

 - k = 20, three lines; spectra of 1, 3, 4, 5, 8, 9 and 13 K-steps (3 .. 51 pixels) in one batch: chunks of 4
   K-steps that are full, short and single, record offsets that are not zero, and the last quasar's chunk copy
   running into the record pool's padding;
 - S = 16, 63, 64, 65 samples: one wave that holds the whole z range; the null slot last in a block, alone in a
   block with its idle slots, and behind one sample;
 - samples placed on the spectra by the method of tests/test_gpu_sweep_fp64_ops.py (near_line_cases.py): line cores
   on pixels at |x| = 0, 8, 29.99, 30.01 and 31.9 Doppler widths, a pair of samples that puts Lyman-alpha and
   Lyman-beta on ONE pixel (the short synthetic spectra reach two lines from one K-step: the pair sits on the
   3-K-step spectrum, no longer one was needed), a lone near sample, and a last sample in z that is near a line
   (the one the null-model and idle slots evaluate).
The host side computes x for every lane, wave and K-step from the z order and asserts that the cases are there:
(a) a voted wave with exactly one lane near one line, (b) lanes on both sides of |x| = 30 in one voted K-step,
(c) at S = 16 one lane near Lyman-alpha and another near Lyman-beta in one K-step, (d) at S = 64, 65 the null
slot and idle slots in a voted wave.  Every sample log-likelihood and the null evidence are compared at 1e-8
absolute, the project's tolerance; every figure is printed before it is asserted."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import Parameters

import near_line_cases as NC
import refine_restatement as RR

pytestmark = pytest.mark.gpu

TOL = 1e-8
_runs = {}


def run(S):
    """GPU and oracle at S samples and S refine points: computed once, never modified"""
    if S in _runs:
        return _runs[S]
    from oracle import oracle
    p = Parameters(num_lines=3)
    model = synthetic.make_model(20)
    spectra = NC.make_spectra(model)
    ranges = NC.z_ranges(spectra)
    samples, placed = NC.make_samples(S, spectra, ranges)
    nq = len(spectra)
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        ctx.set_refine_points(synthetic.halton(S, 2), synthetic.halton(S, 3))
        batch = ctx.upload(spectra, np.full(nq, np.log(0.9)), np.full(nq, np.log(0.1)))
        try:
            batch.process()
            got = batch.download()
            boxes = np.asarray(batch.refine(levels=1)["boxes"])[:, 0].copy()
            # u of the refine points: placed in the same way inside each quasar's own box
            box_ranges = [(b[0], b[1]) for b in boxes]
            u = NC.box_offsets(S, spectra, box_ranges)
            v = synthetic.halton(S, 3)
            ctx.set_refine_points(u, v)
            refined = batch.refine(levels=1)
        finally:
            batch.close()
    finally:
        ctx.close()
    want = [oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"], sp["flux"],
                                    sp["noise_variance"], sp["pixel_mask"], sp["z_qso"], oracle.OracleParams(num_lines=3))
            for sp in spectra]
    _runs[S] = dict(model=model, spectra=spectra, ranges=ranges, samples=samples, placed=placed, got=got, want=want,
                    boxes=boxes, box_ranges=box_ranges, refined=refined, u=u, v=v)
    return _runs[S]


def test_the_shapes():
    r = run(NC.SAMPLE_COUNTS[0])
    steps = [-(-(sp["wavelengths"].size - 2 * NC.EDGE) // 4) for sp in r["spectra"]]
    print("K-steps per spectrum:", steps, "; placed samples:", r["placed"])
    assert tuple(steps) == NC.K_STEPS
    for i, (lo, hi) in enumerate(r["ranges"]):
        assert abs(r["got"]["min_z_dlas"][i] - lo) < 1e-14 and abs(r["got"]["max_z_dlas"][i] - hi) < 1e-14


@pytest.mark.parametrize("S", NC.SAMPLE_COUNTS)
def test_the_cases_are_there(S):
    r = run(S)
    found = NC.find_cases(S, r["samples"]["offset_samples"], r["spectra"], r["ranges"])
    print(f"S = {S}: cases and one (quasar, wave, pixel group) of each: {found}")
    assert "a" in found and "b" in found
    if S == 16:
        assert "c" in found
    if S in (64, 65):
        assert "d" in found
    # the boxed sweep takes the same branch: its points, in every quasar's own box
    boxed = NC.find_cases(S, r["u"], r["spectra"], r["box_ranges"])
    print(f"S' = {S}: cases among the refine points: {boxed}")
    assert boxed, "no voted wave among the refine points"


@pytest.mark.parametrize("S", NC.SAMPLE_COUNTS)
def test_sweep_against_the_oracle(S):
    r = run(S)
    got, worst = r["got"], [0.0, 0.0, 0.0]
    assert (np.asarray(got["status"]) == 0).all()
    for i, ref in enumerate(r["want"]):
        assert np.isfinite(ref["sample_log_likelihoods_dla"]).all()
        d = (float(np.abs(got["sample_log_likelihoods_dla"][i] - ref["sample_log_likelihoods_dla"]).max()),
             abs(got["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]),
             abs(got["log_likelihoods_dla"][i] - ref["log_likelihood_dla"]))
        print(f"S = {S}, {NC.K_STEPS[i]} K-steps: |delta| of the sample table {d[0]:.3e}, no-DLA evidence {d[1]:.3e}, "
              f"DLA evidence {d[2]:.3e}")
        worst = [max(a, b if b == b else np.inf) for a, b in zip(worst, d)]
    print(f"S = {S}: worst |delta| vs the oracle: table {worst[0]:.3e}, no-DLA {worst[1]:.3e}, DLA {worst[2]:.3e}")
    assert max(worst) <= TOL


@pytest.mark.parametrize("S", NC.SAMPLE_COUNTS)
def test_boxed_sweep_against_the_oracle(S):
    r = run(S)
    ref = r["refined"]
    assert (np.asarray(ref["status"]) == 0).all()
    assert np.array_equal(np.asarray(ref["boxes"])[:, 0], r["boxes"]), "the boxes do not depend on the point set"
    worst, compared = 0.0, 0
    for i, sp in enumerate(r["spectra"]):
        b = r["boxes"][i]
        sweep = RR.oracle_sweep(r["model"], sp, r["got"]["min_z_dlas"][i], r["got"]["max_z_dlas"][i], 3)
        want = sweep(0, b[0] + (b[1] - b[0]) * r["u"], b[2] + (b[3] - b[2]) * r["v"])
        got = ref["sample_log_likelihoods_refined"][i]
        ok = ~np.isnan(want)   # (no exclusion but what the oracle itself returns as NaN)
        assert ok.any() and not np.isnan(got[ok]).any(), i
        d = float(np.abs(got[ok] - want[ok]).max())
        print(f"S' = {S}, {NC.K_STEPS[i]} K-steps, box z in [{b[0]:.4f}, {b[1]:.4f}]: |delta| of l' {d:.3e}")
        worst, compared = max(worst, d), compared + int(ok.sum())
    print(f"S' = {S}: {compared} refined log-likelihoods, worst |delta| vs the oracle {worst:.3e}")
    assert compared > 0 and worst <= TOL
