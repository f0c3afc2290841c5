"""The K-step arithmetic of k_sweep_slim<3> and k_sweep_slim_boxed<3> (csrc/sweep_slim_body.hpp: degree-4 wing and
exp series, the profile summed in units of the leading line's strength, the broadening on symmetric tap pairs)
against the CPU oracle, at the shapes where that arithmetic can go wrong (hot loop: process_qsos.m:185-199,
voigt.c:282-299):

 - spectra of 2, 5 and 13 K-steps (7, 18 and 51 pixels), and a second one of 13 K-steps with a run of five masked
   pixels, one pixel of noise variance 1e-280 (its flux 0, so that a saturated core leaves r = 0, d = 1e-280 there)
   and, four pixels on -- the same lane of the next K-step -- one of 1e99;
 - S = 63 / 64 / 65 samples: the null slot last in a block, alone in a block with three idle waves, and in the
   ordinary place;
 - samples placed on the spectra: for every spectrum and each of the three lines a pixel the line's core can reach,
   and z_DLA that put the pixel at x = 0, 8, 29.99 and 30.01 Doppler widths from the line centre.  Sorted by z,
   those share their waves with the other spectra's and with Halton samples: waves that take the wing tier, waves
   that take the accurate tier, and within the latter lanes on either side of the hand-over at |x| = 30;
 - the boxed kernel through the refine entry on the same spectra: one level, the points' u placed in the same way
   inside each quasar's own box (read from a first call), l' against the oracle at the GPU's own (z', N').
Everything is compared at 1e-8 absolute, the project's tolerance; every figure is printed before it is asserted."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd._lyman import C_CGS, LINES, SIGMA_CGS
from gp_dla_detection_amd.parameters import Parameters

import refine_restatement as RR

pytestmark = pytest.mark.gpu

TOL = 1e-8
PIXELS = (7, 18, 51, 51)
K_STEPS = (2, 5, 13, 13)
SAMPLE_COUNTS = (63, 64, 65)
DETUNINGS = (0.0, 8.0, 29.99, 30.01)          # |x| of the chosen pixel, Doppler widths
X_PER_UNIT = C_CGS / (np.sqrt(2.0) * SIGMA_CGS)  # x = X_PER_UNIT (lambda / (lambda_j (1 + z)) - 1), voigt.c:287
LINE_A = [LINES[j][0] * 1e8 for j in range(3)]   # Angstrom
LOW, HIGH = 1e-280, 1e99
EDGE = 2                                          # synthetic.make_spectrum: pixels in front of the modelled range


def make_spectra(model):
    spectra = [synthetic.make_spectrum(7300 + i, n, model) for i, n in enumerate(PIXELS)]
    sp = spectra[3]
    for key in ("flux", "noise_variance", "pixel_mask"):
        sp[key] = sp[key].copy()
    run = slice(EDGE + 40, EDGE + 45)              # the way preload_qsos.m leaves masked pixels
    sp["pixel_mask"][run], sp["noise_variance"][run], sp["flux"][run] = 1, np.inf, np.nan
    return spectra


def core_redshifts(wl, lo, hi):
    """For each line the modelled pixel nearest the middle of what its core can reach with z in (lo, hi), and the
    z that put that pixel DETUNINGS Doppler widths from the line centre: [(line, pixel, [z])]."""
    out = []
    for j, line in enumerate(LINE_A):
        z0 = wl[EDGE:-EDGE] / line - 1
        ok = np.flatnonzero((z0 > lo + 0.02 * (hi - lo)) & (z0 < hi - 0.02 * (hi - lo)))
        if ok.size == 0:
            continue
        p = EDGE + int(ok[ok.size // 2])
        out.append((j, p, [wl[p] / (line * (1 + x / X_PER_UNIT)) - 1 for x in DETUNINGS]))
    return out


def placed_samples(S, spectra, ranges):
    off, placed = [], 0
    for sp, (lo, hi) in zip(spectra, ranges):
        for _, _, zs in core_redshifts(sp["wavelengths"], lo, hi):
            off += [(z - lo) / (hi - lo) for z in zs]
    off = np.asarray(off)
    assert off.size <= S and ((off >= 0) & (off < 1)).all()
    placed = off.size
    fill = synthetic.halton(S, 2)[: S - placed]
    offset = np.concatenate([off, fill])
    log_nhi = 20.0 + 2.5 * synthetic.halton(S, 3)
    return dict(offset_samples=offset, log_nhi_samples=log_nhi, nhi_samples=10.0 ** log_nhi), placed


_runs = {}


def run(S):
    """GPU and oracle at S samples and S refine points: computed once, never modified"""
    if S in _runs:
        return _runs[S]
    from oracle import oracle
    p = Parameters(num_lines=3)
    model = synthetic.make_model(20)
    spectra = make_spectra(model)
    ranges = [(p.min_z_dla(sp["wavelengths"][EDGE:-EDGE], sp["z_qso"]), p.max_z_dla(sp["wavelengths"][EDGE:-EDGE], sp["z_qso"]))
              for sp in spectra]   # process_qsos.m:159-160: over the pixels of the modelled range
    # the two special pixels: where the Lyman-alpha core of the fourth spectrum's own placed samples lands
    (_, pa, _), = [c for c in core_redshifts(spectra[3]["wavelengths"], *ranges[3]) if c[0] == 0]
    assert spectra[3]["pixel_mask"][pa] == 0 and spectra[3]["pixel_mask"][pa + 4] == 0
    spectra[3]["noise_variance"][pa], spectra[3]["flux"][pa] = LOW, 0.0
    spectra[3]["noise_variance"][pa + 4] = HIGH
    samples, placed = placed_samples(S, spectra, ranges)
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
            # u of the refine points: line cores on pixels, inside each quasar's own box
            u = []
            for sp, b in zip(spectra, boxes):
                for _, _, zs in core_redshifts(sp["wavelengths"], b[0], b[1]):
                    u += [(z - b[0]) / (b[1] - b[0]) for z in zs]
            u = np.asarray(u)[:S]
            assert ((u >= 0) & (u < 1)).all()
            u = np.concatenate([u, synthetic.halton(S, 2)[: S - u.size]])
            v = synthetic.halton(S, 3)
            ctx.set_refine_points(u, v)
            refined = batch.refine(levels=1)
        finally:
            batch.close()
    finally:
        ctx.close()
    want = []
    for sp in spectra:
        r = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"], sp["flux"],
                                    sp["noise_variance"], sp["pixel_mask"], sp["z_qso"], oracle.OracleParams(num_lines=3))
        want.append(r)
    _runs[S] = dict(model=model, spectra=spectra, ranges=ranges, samples=samples, placed=placed, got=got, want=want,
                    boxes=boxes, refined=refined, u=u, v=v, special=pa)
    return _runs[S]


def test_the_shapes():
    r = run(SAMPLE_COUNTS[0])
    steps = [-(-(sp["wavelengths"].size - 2 * EDGE) // 4) for sp in r["spectra"]]
    lines = [[c[0] for c in core_redshifts(sp["wavelengths"], lo, hi)] for sp, (lo, hi) in zip(r["spectra"], r["ranges"])]
    print("K-steps per spectrum:", steps, "; lines whose core is placed on a pixel:", lines, "; placed samples:", r["placed"])
    assert tuple(steps) == K_STEPS
    assert all(l == [0, 1, 2] for l in lines)
    sp = r["spectra"][3]
    assert sp["noise_variance"][r["special"]] == LOW and sp["noise_variance"][r["special"] + 4] == HIGH
    assert sp["pixel_mask"].sum() == 5
    for i, (lo, hi) in enumerate(r["ranges"]):
        assert abs(r["got"]["min_z_dlas"][i] - lo) < 1e-14 and abs(r["got"]["max_z_dlas"][i] - hi) < 1e-14


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_sweep_against_the_oracle(S):
    r = run(S)
    got, worst = r["got"], [0.0, 0.0, 0.0]
    assert (np.asarray(got["status"]) == 0).all()
    for i, ref in enumerate(r["want"]):
        assert np.isfinite(ref["sample_log_likelihoods_dla"]).all()
        d = (float(np.abs(got["sample_log_likelihoods_dla"][i] - ref["sample_log_likelihoods_dla"]).max()),
             abs(got["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]),
             abs(got["log_likelihoods_dla"][i] - ref["log_likelihood_dla"]))
        print(f"S = {S}, {K_STEPS[i]} K-steps: |delta| of the sample table {d[0]:.3e}, no-DLA evidence {d[1]:.3e}, "
              f"DLA evidence {d[2]:.3e}")
        worst = [max(a, b if b == b else np.inf) for a, b in zip(worst, d)]
    print(f"S = {S}: worst |delta| vs the oracle: table {worst[0]:.3e}, no-DLA {worst[1]:.3e}, DLA {worst[2]:.3e}")
    assert max(worst) <= TOL


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_boxed_sweep_against_the_oracle(S):
    r = run(S)
    ref = r["refined"]
    assert (np.asarray(ref["status"]) == 0).all()
    assert np.array_equal(np.asarray(ref["boxes"])[:, 0], r["boxes"]), "the boxes do not depend on the point set"
    worst, compared = 0.0, 0
    for i, sp in enumerate(r["spectra"]):
        b = r["boxes"][i]
        on_cores = [c[0] for c in core_redshifts(sp["wavelengths"], b[0], b[1])]
        sweep = RR.oracle_sweep(r["model"], sp, r["got"]["min_z_dlas"][i], r["got"]["max_z_dlas"][i], 3)
        want = sweep(0, b[0] + (b[1] - b[0]) * r["u"], b[2] + (b[3] - b[2]) * r["v"])
        got = ref["sample_log_likelihoods_refined"][i]
        ok = ~np.isnan(want)   # (no exclusion but what the oracle itself returns as NaN)
        assert ok.any() and not np.isnan(got[ok]).any(), i
        d = float(np.abs(got[ok] - want[ok]).max())
        print(f"S' = {S}, {K_STEPS[i]} K-steps, box z in [{b[0]:.4f}, {b[1]:.4f}], lines with a core on a pixel {on_cores}: "
              f"|delta| of l' {d:.3e}")
        worst, compared = max(worst, d), compared + int(ok.sum())
    print(f"S' = {S}: {compared} refined log-likelihoods, worst |delta| vs the oracle {worst:.3e}")
    assert compared > 0 and worst <= TOL
