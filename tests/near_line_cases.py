"""Inputs of tests/test_gpu_near_line_tier.py and the host-side model of which lanes of k_sweep_slim<3> are within
reach of which line: no GPU here, so that the cases the test is about can be checked wherever Python runs.

The kernel's geometry (csrc/sweep_slim_body.hpp): the samples are taken in order of z_DLA; slot 16 w + s is lane
(s, .) of wave w (four waves to a block); slot S is the null model and the slots behind it up to the end of its
block are idle, and all of those evaluate the LAST sample in z order.  A wave evaluates the raw profile of four
padded pixels 4 g + jj (jj = 0..3) at a time -- in the priming for g < 3, in K-step g - 3 after that -- and votes
there: some lane within 30 Doppler widths of some line.  Padded pixel 3 + u is pixel u of the modelled range
(k_prepare); only groups made of modelled pixels alone are looked at here (the three pad pixels in front and behind
are left out: the cases below need none of them)."""
import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd._lyman import C_CGS, LINES, SIGMA_CGS
from gp_dla_detection_amd.parameters import Parameters

EDGE = 2                                           # synthetic.make_spectrum: pixels in front of the modelled range
K_STEPS = (1, 3, 4, 5, 8, 9, 13)
PIXELS = (3, 10, 16, 18, 30, 35, 51)               # modelled pixels: K-steps = ceil(pixels / 4)
SAMPLE_COUNTS = (16, 63, 64, 65)
DETUNINGS = (0.0, 8.0, 29.99, 30.01, 31.9)         # |x| of the chosen pixel, Doppler widths
X_PER_UNIT = C_CGS / (np.sqrt(2.0) * SIGMA_CGS)    # x = X_PER_UNIT (lambda / (lambda_j (1 + z)) - 1), voigt.c:287
LINE_A = [LINES[j][0] * 1e8 for j in range(3)]     # Angstrom
Y2 = [(LINES[j][4] / np.sqrt(2.0) / SIGMA_CGS) ** 2 for j in range(3)]


def make_spectra(model):
    return [synthetic.make_spectrum(7400 + i, n, model) for i, n in enumerate(PIXELS)]


def z_ranges(spectra):
    p = Parameters(num_lines=3)
    return [(p.min_z_dla(sp["wavelengths"][EDGE:-EDGE], sp["z_qso"]), p.max_z_dla(sp["wavelengths"][EDGE:-EDGE], sp["z_qso"]))
            for sp in spectra]   # process_qsos.m:159-160: over the pixels of the modelled range


def core_redshifts(wl, lo, hi, lines=(0, 1, 2)):
    """tests/test_gpu_sweep_fp64_ops.py's method: for each line the modelled pixel nearest the middle of what its
    core can reach with z in (lo, hi), and the z that put that pixel DETUNINGS Doppler widths from the line centre:
    [(line, pixel, [z])]."""
    out = []
    for j in lines:
        z0 = wl[EDGE:-EDGE] / LINE_A[j] - 1
        ok = np.flatnonzero((z0 > lo + 0.02 * (hi - lo)) & (z0 < hi - 0.02 * (hi - lo)))
        if ok.size == 0:
            continue
        p = EDGE + int(ok[ok.size // 2])
        out.append((j, p, [wl[p] / (LINE_A[j] * (1 + x / X_PER_UNIT)) - 1 for x in DETUNINGS]))
    return out


def two_lines_from_one_step(wl, lo, hi):
    """A pixel and two redshifts inside (lo, hi): z_a puts Lyman-alpha 8 Doppler widths from the pixel, z_b puts
    Lyman-beta 8 widths from the same pixel -- two lanes (two samples, one pixel) of one K-step, near different
    lines.  (1 + z_b) / (1 + z_a) = lambda_alpha / lambda_beta = 1.185, so the pixel lies in the blue third."""
    for u, lam in enumerate(wl[EDGE:-EDGE]):
        za = lam / (LINE_A[0] * (1 + 8.0 / X_PER_UNIT)) - 1
        zb = lam / (LINE_A[1] * (1 - 8.0 / X_PER_UNIT)) - 1
        margin = 0.02 * (hi - lo)
        if za > lo + margin and zb < hi - margin:
            return u, za, zb
    return None


def last_sample_near(wl, lo, hi):
    """The largest z below hi that puts Lyman-alpha 8 Doppler widths from a modelled pixel."""
    z0 = wl[EDGE:-EDGE] / (LINE_A[0] * (1 + 8.0 / X_PER_UNIT)) - 1
    ok = z0[(z0 > lo) & (z0 < hi - 1e-3 * (hi - lo))]
    return float(ok.max())


def placed_offsets(S, spectra, ranges):
    """Offsets in [0, 1) of the placed samples, each for one quasar's own z range (the sample set is shared: to
    the other quasars they are ordinary samples).  At every S: the two-line pair on the 3-K-step spectrum.  From
    S = 63 on: the five detunings of line i mod 3 on spectrum i, of all three lines on the 13-K-step one, one lone
    sample 8 widths from Lyman-beta on the 8-K-step one, and, last in z of ALL samples, one that is 8 widths from
    Lyman-alpha on a pixel of the 13-K-step spectrum (what the null-model and idle slots evaluate).  At S = 16
    the five detunings on the 1- and 3-K-step spectra only."""
    off = []
    u, za, zb = two_lines_from_one_step(spectra[1]["wavelengths"], *ranges[1])
    lo, hi = ranges[1]
    off += [(za - lo) / (hi - lo), (zb - lo) / (hi - lo)]
    for i, (sp, (lo, hi)) in enumerate(zip(spectra, ranges)):
        if S < 63 and i > 1:
            break
        lines = (0, 1, 2) if (i == len(spectra) - 1 and S >= 63) else (i % 3,)
        for _, _, zs in core_redshifts(sp["wavelengths"], lo, hi, lines):
            off += [(z - lo) / (hi - lo) for z in zs]
    top = None
    if S >= 63:
        lo, hi = ranges[4]
        (_, p, _), = core_redshifts(spectra[4]["wavelengths"], lo, hi, (1,))
        p_lone = p + 5 if p + 5 < spectra[4]["wavelengths"].size - EDGE else p - 5
        z = spectra[4]["wavelengths"][p_lone] / (LINE_A[1] * (1 + 8.0 / X_PER_UNIT)) - 1
        assert lo < z < hi
        off.append((z - lo) / (hi - lo))
        lo, hi = ranges[-1]
        top = (last_sample_near(spectra[-1]["wavelengths"], lo, hi) - lo) / (hi - lo)
    off = np.asarray(off)
    assert ((off >= 0) & (off < 1)).all()
    return off, top


def box_offsets(S, spectra, boxes):
    """u of the refine points, as tests/test_gpu_sweep_fp64_ops.py places them: the five detunings of every line
    whose core a pixel can reach inside each quasar's own box (a box is too narrow for the two-line pair),
    the first S of them, then Halton points."""
    u = []
    for sp, (lo, hi) in zip(spectra, boxes):
        for _, _, zs in core_redshifts(sp["wavelengths"], lo, hi):
            u += [(z - lo) / (hi - lo) for z in zs]
    u = np.asarray(u)[:S]
    assert ((u >= 0) & (u < 1)).all()
    return np.concatenate([u, synthetic.halton(S, 2)[: S - u.size]])


def make_samples(S, spectra, ranges):
    off, top = placed_offsets(S, spectra, ranges)
    assert off.size + (top is not None) <= S, (off.size, S)
    fill = synthetic.halton(4 * S, 2)
    if top is not None:
        assert (off < top).all()
        fill = fill[fill < top]   # nothing behind the last placed sample
    fill = fill[: S - off.size - (top is not None)]
    offset = np.concatenate([off, fill] + ([[top]] if top is not None else []))
    assert offset.size == S
    log_nhi = 20.0 + 2.5 * synthetic.halton(S, 3)
    return dict(offset_samples=offset, log_nhi_samples=log_nhi, nhi_samples=10.0 ** log_nhi), off.size + (top is not None)


def lane_map(S, offsets, spectra, ranges):
    """For every quasar, wave and group of four modelled pixels that share a K-step: x[lane s, pixel jj, line] in
    Doppler widths, with the role of every lane's slot ('sample', 'null', 'idle').  Yields
    (quasar, wave, group, x [16, 4, 3], roles [16])."""
    order = np.argsort(offsets, kind="stable")
    slots = -(-(S + 1) // 64) * 64
    for q, (sp, (lo, hi)) in enumerate(zip(spectra, ranges)):
        wl = sp["wavelengths"][EDGE:-EDGE]
        n = wl.size
        for w in range(slots // 16):
            ids = [order[min(16 * w + s, S - 1)] if 16 * w + s < S else order[S - 1] for s in range(16)]
            roles = ["sample" if 16 * w + s < S else "null" if 16 * w + s == S else "idle" for s in range(16)]
            z = lo + (hi - lo) * offsets[ids]                                   # process_qsos.m:162-164
            for g in range(1, (n + 6) // 4 + 1):
                u = 4 * g + np.arange(4) - 3                                    # modelled pixels of padded 4 g + jj
                if u[0] < 0 or u[-1] >= n:
                    continue
                x = np.stack([X_PER_UNIT * (wl[u][None, :] / (LINE_A[j] * (1 + z[:, None])) - 1) for j in range(3)], -1)
                yield q, w, g, x, roles


def near_of(x):
    """The kernels' own test, per line: x^2 + y^2 < 900"""
    return np.stack([x[..., j] ** 2 + Y2[j] < 900.0 for j in range(3)], -1)


def find_cases(S, offsets, spectra, ranges):
    """Which of the cases the test is about occur, each with one place (quasar, wave, group) where it does:
      a: a voted wave in which exactly one lane is near exactly one line;
      b: a voted wave with, for one line, a lane inside |x| = 30 and another lane in 30 <= |x| < 32;
      c: a wave and K-step with one lane near Lyman-alpha and ANOTHER lane near Lyman-beta or Lyman-gamma;
      d: a voted wave that holds the null slot and idle slots."""
    found = {}
    for q, w, g, x, roles in lane_map(S, offsets, spectra, ranges):
        near = near_of(x)
        if not near.any():
            continue
        real = np.array([r == "sample" for r in roles])
        where = (q, w, g)
        if near.sum() == 1 and real.all():
            found.setdefault("a", where)
        for j in range(3):
            ax = np.abs(x[..., j])
            if near[..., j].any() and ((ax >= 30.0) & (ax < 32.0) & ~near[..., j]).any() and real.all():
                found.setdefault("b", where)
        la = near[..., 0].reshape(-1)
        lb = (near[..., 1] | near[..., 2]).reshape(-1)
        if la.any() and lb.any() and (np.flatnonzero(la)[:, None] != np.flatnonzero(lb)[None, :]).any() and real.all():
            found.setdefault("c", where)
        if "null" in roles and "idle" in roles:
            found.setdefault("d", where)
    return found
