"""The K-step of k_sweep_slim / k_sweep_slim_boxed with fewer bookkeeping instructions (csrc/sweep_slim_body.hpp;
LABBOOK, "Bookkeeping instructions of the K-step"): what is carried from K-step to K-step lives across the chunk
loop, the chunk is a callable that takes its parity, and a constant of the wing series stays in a vector register.
Work on that part of the kernel -- the null-model select, the landing addresses of the LDS-DMA copies, the parity
addresses, the chunk loop's shape -- changes no floating-point operation, operand or order, so k_sweep_slim<3> must
agree BIT FOR BIT with k_sweep on pre-expanded records, which keeps its own select and addressing
(libgpdla_legacy.so with GPDLA_EXPANDED_RECORDS=1, in one clean child process for all cases).  One batch
(kstep_slots_cases.py), at the places where such work can go wrong:

 - spectra of 1 3 4 5 8 9 12 13 K-steps: one, two and three chunks exactly, odd and even chunk counts, a last chunk
   with 1 and with 4 live K-steps, the copies for chunk c + 1 and c + 2 taken and not taken; a masked run across a
   chunk edge;
 - S = 15, 16 (the null slot inside, and alone at the head of, a wave), 63, 64, 65 (last in a block; opening a block
   of otherwise idle slots; next to one real sample);
 - the last sample in z puts a line core on a pixel: the host asserts from the z order that a wave made of null and
   idle slots alone votes for the accurate tier (S = 15, 16, 64), and that the null slot sits in a voted wave next
   to real samples (S = 15, 63, 65);
 - every output against the CPU oracle at 1e-8 absolute, the suite's tolerance;
 - a run-time line count (k_sweep_slim<0>: k = 13, 5 lines, S = 64) under the 1e-9 rule of
   test_gpu_sweep_half_blocks.py against the legacy library, and against the oracle at 1e-8;
 - the boxed kernel once through the refine entry (S' = 64 points), l' against the oracle at the GPU's own box.
Hot loop: process_qsos.m:185-199.  Every figure is printed before it is asserted."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import kstep_slots_cases as KC
import near_line_cases as NC
import refine_restatement as RR

pytestmark = pytest.mark.gpu

TOL = 1e-8
RUNTIME_LINES = (13, 5, 64)   # k, lines, S
_runs = {}


def run(k, num_lines, S):
    """this library's outputs of one case: computed once, never modified"""
    key = (k, num_lines, S)
    if key not in _runs:
        _runs[key] = KC.run_case(k, num_lines, S)
    return _runs[key]


@pytest.fixture(scope="module")
def legacy(tmp_path_factory):
    """k_sweep on pre-expanded records, every case in one child process: never modified"""
    from gp_dla_detection_amd import _lib
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    env = {"GPDLA_EXPANDED_RECORDS": "1", "GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH}
    out = tmp_path_factory.mktemp("kstep_slots") / "legacy.npz"
    cases = [(20, 3, S) for S in KC.SAMPLE_COUNTS] + [RUNTIME_LINES]
    pr = mp.get_context("forkserver").Process(target=KC.run_child, args=(cases, env, str(out)))
    pr.start()
    pr.join(600)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
    assert pr.exitcode == 0
    return np.load(out)


@pytest.fixture(scope="module")
def oracle_tables():
    """the CPU oracle per (case, quasar): computed on demand, once"""
    from oracle import oracle
    cache = {}

    def get(k, num_lines, S):
        if (k, num_lines, S) not in cache:
            model, samples, spectra, _, _, _ = KC.build_case(k, num_lines, S)
            cache[(k, num_lines, S)] = [
                oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"], sp["flux"],
                                        sp["noise_variance"], sp["pixel_mask"], sp["z_qso"], oracle.OracleParams(num_lines=num_lines))
                for sp in spectra]
        return cache[(k, num_lines, S)]
    return get


def test_the_shapes():
    import gp_dla_detection_amd as gp
    model, samples, spectra, ranges, lp, p = KC.build_case(20, 3, 64)
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        batch = ctx.upload(spectra, lp[0], lp[1])
        steps = [int(-(-int(n) // 4)) for n in batch.unmasked_counts()]
        batch.close()
    finally:
        ctx.close()
    print("K-steps per spectrum:", steps)
    assert tuple(steps) == KC.K_STEPS
    got = run(20, 3, 64)
    for i, (lo, hi) in enumerate(ranges):
        assert abs(got["min_z_dlas"][i] - lo) < 1e-14 and abs(got["max_z_dlas"][i] - hi) < 1e-14


@pytest.mark.parametrize("S", KC.SAMPLE_COUNTS)
def test_the_null_waves_vote(S):
    _, samples, spectra, ranges, _, _ = KC.build_case(20, 3, S)
    found = KC.null_waves(S, samples["offset_samples"], spectra, ranges)
    print(f"S = {S}: voted waves without an absorber, (quasar, wave, pixel group): {found}")
    if S in (15, 16, 64):
        assert "alone" in found
    if S in (15, 63, 65):
        assert "mixed" in found


@pytest.mark.parametrize("S", KC.SAMPLE_COUNTS)
def test_three_lines_bit_for_bit(S, legacy):
    got = run(20, 3, S)
    prefix = f"k20_3_S{S}/"
    names = [n for n in legacy.files if n.startswith(prefix)]
    assert len(names) >= 10
    for name in names:
        a, b = np.asarray(got[name[len(prefix):]]), legacy[name]
        assert a.shape == b.shape, name
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), (name, float(np.nanmax(np.abs(a - b))))
        else:
            assert np.array_equal(a, b), name
    table = np.asarray(got["sample_log_likelihoods_dla"])
    assert table.shape == (len(KC.PIXELS), S) and np.isfinite(table).all()
    assert np.isfinite(np.asarray(got["log_likelihoods_no_dla"])).all()


def _against_the_oracle(got, want, label):
    worst = [0.0, 0.0, 0.0]
    assert (np.asarray(got["status"]) == 0).all()
    for i, ref in enumerate(want):
        assert np.isfinite(ref["sample_log_likelihoods_dla"]).all()
        d = (float(np.abs(got["sample_log_likelihoods_dla"][i] - ref["sample_log_likelihoods_dla"]).max()),
             abs(got["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]),
             abs(got["log_likelihoods_dla"][i] - ref["log_likelihood_dla"]))
        print(f"{label}, {KC.K_STEPS[i]} K-steps: |delta| of the sample table {d[0]:.3e}, no-DLA evidence {d[1]:.3e}, "
              f"DLA evidence {d[2]:.3e}")
        worst = [max(a, b if b == b else np.inf) for a, b in zip(worst, d)]
    print(f"{label}: worst |delta| vs the oracle: table {worst[0]:.3e}, no-DLA {worst[1]:.3e}, DLA {worst[2]:.3e}")
    assert max(worst) <= TOL


@pytest.mark.parametrize("S", KC.SAMPLE_COUNTS)
def test_three_lines_against_the_oracle(S, oracle_tables):
    _against_the_oracle(run(20, 3, S), oracle_tables(20, 3, S), f"S = {S}")


def test_run_time_line_count(legacy, oracle_tables):
    k, num_lines, S = RUNTIME_LINES
    got = run(k, num_lines, S)
    prefix = f"k{k}_{num_lines}_S{S}/"
    table = "sample_log_likelihoods_dla"
    a, b = np.asarray(got[table]), legacy[prefix + table]
    assert a.shape == b.shape and np.isfinite(a).all()
    print("max |delta| of the sample table vs the legacy library:", float(np.max(np.abs(a - b))))
    assert np.max(np.abs(a - b)) < 1e-9 * max(1.0, float(np.max(np.abs(b))))
    for name in ("log_likelihoods_no_dla", "log_posteriors_dla", "MAP_z_dlas", "MAP_log_nhis"):
        if prefix + name in legacy.files:
            assert np.allclose(np.asarray(got[name]), legacy[prefix + name], rtol=1e-9, atol=1e-8, equal_nan=True), name
    _against_the_oracle(got, oracle_tables(k, num_lines, S), f"{num_lines} lines, k = {k}, S = {S}")


def test_boxed_sweep_against_the_oracle():
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd import synthetic
    S = 64
    model, samples, spectra, ranges, lp, p = KC.build_case(20, 3, S)
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        ctx.set_refine_points(synthetic.halton(S, 2), synthetic.halton(S, 3))
        batch = ctx.upload(spectra, lp[0], lp[1])
        try:
            batch.process()
            first = batch.download()
            boxes = np.asarray(batch.refine(levels=1)["boxes"])[:, 0].copy()
            # u of the refine points: line cores on pixels inside each quasar's own box (near_line_cases.box_offsets)
            u, v = NC.box_offsets(S, spectra, [(b[0], b[1]) for b in boxes]), synthetic.halton(S, 3)
            ctx.set_refine_points(u, v)
            refined = batch.refine(levels=1)
        finally:
            batch.close()
    finally:
        ctx.close()
    assert (np.asarray(refined["status"]) == 0).all()
    assert np.array_equal(np.asarray(refined["boxes"])[:, 0], boxes), "the boxes do not depend on the point set"
    voted = NC.find_cases(S, u, spectra, [(b[0], b[1]) for b in boxes])
    print("voted waves among the refine points:", voted)
    assert voted
    worst, compared = 0.0, 0
    for i, sp in enumerate(spectra):
        b = boxes[i]
        sweep = RR.oracle_sweep(model, sp, first["min_z_dlas"][i], first["max_z_dlas"][i], 3)
        want = sweep(0, b[0] + (b[1] - b[0]) * u, b[2] + (b[3] - b[2]) * v)
        got = refined["sample_log_likelihoods_refined"][i]
        ok = ~np.isnan(want)   # (no exclusion but what the oracle itself returns as NaN)
        assert ok.any() and not np.isnan(got[ok]).any(), i
        d = float(np.abs(got[ok] - want[ok]).max())
        print(f"S' = {S}, {KC.K_STEPS[i]} K-steps, box z in [{b[0]:.4f}, {b[1]:.4f}]: |delta| of l' {d:.3e}")
        worst, compared = max(worst, d), compared + int(ok.sum())
    print(f"{compared} refined log-likelihoods, worst |delta| vs the oracle {worst:.3e}")
    assert compared > 0 and worst <= TOL
