"""Inputs and worker of tests/test_gpu_sweep_kstep_slots.py: one batch of short spectra for k_sweep_slim, built on
the geometry model of near_line_cases.py (which lane of which wave is within reach of which line, from the z order
alone: no GPU needed for that part).

Spectra of 1 3 4 5 8 9 12 13 K-steps: one chunk of 4 K-steps that is short and that is full; exactly two and three
chunks; odd and even chunk counts (the loop takes two chunks per trip); a last chunk with 1 and with 4 live K-steps;
the copies of chunk c + 1 and of the rows of chunk c + 2 taken and not taken.  The 9-K-step spectrum carries a run of
masked pixels across the edge between its first two chunks.

Samples, at every count S: near_line_cases.placed_offsets' line cores on pixels, and ALWAYS, last in z of all
samples, one that puts Lyman-alpha 8 Doppler widths from a pixel of the longest spectrum: the null-model and idle
slots evaluate that sample, so a wave made of such slots alone votes for the accurate Voigt tier there."""
import os

import numpy as np

import near_line_cases as NC
from gp_dla_detection_amd import synthetic

PIXELS = (3, 10, 16, 18, 30, 35, 48, 51)           # modelled pixels: K-steps = ceil(pixels / 4)
K_STEPS = (1, 3, 4, 5, 8, 9, 12, 13)
SAMPLE_COUNTS = (15, 16, 63, 64, 65)
MASKED = (5, 13, 19)                               # spectrum, first and one past the last masked modelled pixel
assert PIXELS[1] == NC.PIXELS[1] and PIXELS[4] == NC.PIXELS[4] and PIXELS[-1] == NC.PIXELS[-1]  # what placed_offsets indexes


def make_spectra(model):
    spectra = [synthetic.make_spectrum(7400 + i, n, model) for i, n in enumerate(PIXELS)]
    q, lo, hi = MASKED
    assert lo // 4 == 3 and (hi - 1) // 4 == 4     # K-steps 3 and 4: the last of chunk 0, the first of chunk 1
    sp = spectra[q]
    sl = slice(NC.EDGE + lo, NC.EDGE + hi)
    sp["pixel_mask"][sl] = 1                       # (as synthetic.make_spectrum masks: no flux, infinite variance)
    sp["noise_variance"][sl] = np.inf
    sp["flux"][sl] = np.nan
    return spectra


def make_samples(S, spectra, ranges):
    """near_line_cases.make_samples with the last-in-z sample near a line at EVERY S"""
    off, _ = NC.placed_offsets(S, spectra, ranges)
    lo, hi = ranges[-1]
    top = (NC.last_sample_near(spectra[-1]["wavelengths"], lo, hi) - lo) / (hi - lo)
    assert off.size + 1 <= S and (off < top).all()
    fill = synthetic.halton(4 * S, 2)
    fill = fill[fill < top][: S - off.size - 1]    # nothing behind the last placed sample
    offset = np.concatenate([off, fill, [top]])
    assert offset.size == S
    log_nhi = 20.0 + 2.5 * synthetic.halton(S, 3)
    return dict(offset_samples=offset, log_nhi_samples=log_nhi, nhi_samples=10.0 ** log_nhi)


def null_waves(S, offsets, spectra, ranges):
    """Where the slots without an absorber vote: {"alone": (quasar, wave, group) of a voted wave made of the null
    slot and / or idle slots only, "mixed": one of a voted wave that holds the null slot next to real samples}"""
    found = {}
    for q, w, g, x, roles in NC.lane_map(S, offsets, spectra, ranges):
        if not NC.near_of(x).any():
            continue
        if "sample" not in roles:
            found.setdefault("alone", (q, w, g))
        elif "null" in roles:
            found.setdefault("mixed", (q, w, g))
    return found


def build_case(k, num_lines, S):
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd.parameters import Parameters
    model = synthetic.make_model(k)
    spectra = make_spectra(model)
    ranges = NC.z_ranges(spectra)
    samples = make_samples(S, spectra, ranges)
    cat = synthetic.make_prior_catalog()
    z = np.array([s["z_qso"] for s in spectra])
    return model, samples, spectra, ranges, gp.dla_existence_prior(cat["z_qsos"], cat["dla_ind"], z), \
        Parameters(num_lines=num_lines)


def run_case(k, num_lines, S):
    import gp_dla_detection_amd as gp
    model, samples, spectra, _, lp, p = build_case(k, num_lines, S)
    return gp.process_qsos(model, samples, spectra, log_priors=lp, params=p)


def run_child(cases, env, out_path):
    """cases: [(k, num_lines, S)], all in this (clean) process with `env` set before the library is loaded; one
    .npz, names prefixed "k<k>_<lines>_S<S>/" """
    os.environ.update(env)
    arrays = {}
    for k, num_lines, S in cases:
        out = run_case(k, num_lines, S)
        arrays.update({f"k{k}_{num_lines}_S{S}/{name}": np.asarray(v) for name, v in out.items() if isinstance(v, np.ndarray)})
    np.savez(out_path, **arrays)
