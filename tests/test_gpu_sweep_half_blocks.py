"""k_sweep_slim and k_sweep_slim_boxed as blocks of 4 waves on 4-step chunks, two blocks to a compute unit
(csrc/sweep_slim_kernel.hpp, "Block shape").  What that shape can get wrong lies where a 4-step chunk ends, in
the last, partly filled chunk of either parity, in the record-by-record chunk copy (3584 B, no whole number of
KiB), in the 13 tiles a wave now expands per chunk, and in the 64-slot block that holds the null model.  Here:

 - spectra of 2 3 4 4 5 7 8 9 11 12 12 13 K-steps (one short of, on and one past an edge of the 4-step chunks,
   at 1 to 4 chunks, both parities last) at sample counts that put the null slot last in a block (63), alone
   with three idle waves in a block of its own (64), and in the ordinary place (65), against k_sweep on the
   pre-expanded records (libgpdla_legacy.so with GPDLA_EXPANDED_RECORDS=1 in ONE clean child process for the
   three counts): the same products and the same MFMA sequence per column, so every output is bit-identical;
 - a run-time line count (k_sweep_slim<0>: k = 13, 5 lines, S = 64) under the 1e-9 rule of
   test_gpu_record_classes.py;
 - the boxed form through the refine entry: spectra of 5 and 9 K-steps, 100 refine points (two blocks, the second
   partly filled), l' against the CPU oracle at the GPU's own (z', N') to 1e-8 absolute, as
   test_gpu_refine.py compares;
 - hipOccupancyMaxActiveBlocksPerMultiprocessor at the launch's own shape: 2 blocks per compute unit for every
   instantiation.
Hot loop: process_qsos.m:185-199.  Every figure is printed before it is asserted."""
import ctypes as C
import multiprocessing as mp
import os

import numpy as np
import pytest

import sweep_chunk_edges_worker as w

pytestmark = pytest.mark.gpu

PIXELS = [5, 9, 13, 16, 17, 28, 29, 33, 44, 45, 48, 49]
K_STEPS = [2, 3, 4, 4, 5, 7, 8, 9, 11, 12, 12, 13]
SAMPLE_COUNTS = [63, 64, 65]


def _child(k, num_lines, num_samples, out):
    from gp_dla_detection_amd import _lib
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    env = {"GPDLA_EXPANDED_RECORDS": "1", "GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH}
    pr = mp.get_context("forkserver").Process(target=w.run_child, args=(k, num_lines, num_samples, env, str(out)),
                                              kwargs=dict(pixels=PIXELS))
    pr.start()
    pr.join(600)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
    assert pr.exitcode == 0
    return np.load(out)


@pytest.fixture(scope="module")
def expanded_three_lines(tmp_path_factory):
    """k_sweep on pre-expanded records at the three sample counts: one child process, never modified"""
    return _child(20, 3, SAMPLE_COUNTS, tmp_path_factory.mktemp("half_blocks") / "k20_3.npz")


def test_the_spectra_cover_the_edges_of_the_4_step_chunks():
    steps = w.k_steps(20, 3, 64, pixels=PIXELS)
    print("K-steps per spectrum:", steps)
    assert steps == K_STEPS


@pytest.mark.parametrize("num_samples", SAMPLE_COUNTS)
def test_three_lines_bit_for_bit(num_samples, expanded_three_lines):
    got = w.run_case(20, 3, num_samples, pixels=PIXELS)
    prefix = f"S{num_samples}/"
    names = [n for n in expanded_three_lines.files if n.startswith(prefix)]
    assert len(names) >= 10
    for name in names:
        a, b = np.asarray(got[name[len(prefix):]]), expanded_three_lines[name]
        assert a.shape == b.shape, name
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), (name, float(np.nanmax(np.abs(a - b))))
        else:
            assert np.array_equal(a, b), name
    table = np.asarray(got["sample_log_likelihoods_dla"])
    assert table.shape == (len(PIXELS), num_samples) and np.isfinite(table).any()


def test_run_time_line_count(tmp_path):
    k, num_lines, num_samples = 13, 5, 64
    want = _child(k, num_lines, num_samples, tmp_path / "k13_5.npz")
    got = w.run_case(k, num_lines, num_samples, pixels=PIXELS)
    table = "sample_log_likelihoods_dla"
    a, b = np.asarray(got[table]), want[table]
    assert a.shape == b.shape and np.isfinite(a).any()
    assert np.array_equal(np.isnan(a), np.isnan(b))
    print("max |delta| of the sample table:", float(np.nanmax(np.abs(a - b))))
    assert np.nanmax(np.abs(a - b)) < 1e-9 * max(1.0, float(np.nanmax(np.abs(b))))
    for name in ("log_likelihoods_no_dla", "log_posteriors_dla", "MAP_z_dlas", "MAP_log_nhis"):
        if name in want.files:
            x, y = np.asarray(got[name]), want[name]
            assert np.allclose(x, y, rtol=1e-9, atol=1e-8, equal_nan=True), name


def test_boxed_sweep_against_the_oracle():
    import gp_dla_detection_amd as gp
    from gp_dla_detection_amd import synthetic
    from gp_dla_detection_amd.parameters import Parameters

    import refine_restatement as RR

    k, num_lines, S, Sr, levels = 20, 3, 200, 100, 2
    assert Sr % 64 and (Sr + 1) % 64
    model, samples = synthetic.make_model(k), synthetic.make_samples(S)
    spectra = [synthetic.make_spectrum(5300 + 11 * i + k, n, model) for i, n in enumerate((17, 33))]
    u, v = synthetic.halton(Sr, 2), synthetic.halton(Sr, 3)
    ctx = gp.Context(0, Parameters(num_lines=num_lines))
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        ctx.set_refine_points(u, v)
        batch = ctx.upload(spectra, np.full(2, np.log(0.9)), np.full(2, np.log(0.1)))
        try:
            steps = [int(-(-int(n) // 4)) for n in batch.unmasked_counts()]
            print("K-steps per spectrum:", steps)
            assert steps == [5, 9]
            batch.process()
            first = batch.download()
            runs = [batch.refine(levels=l + 1) for l in range(levels)]   # (a call's tables are those of its last level)
        finally:
            batch.close()
    finally:
        ctx.close()
    print("refine status:", runs[-1]["status"])
    assert (np.asarray(runs[-1]["status"]) == 0).all()
    worst, compared = 0.0, 0
    for i, sp in enumerate(spectra):
        sweep = RR.oracle_sweep(model, sp, first["min_z_dlas"][i], first["max_z_dlas"][i], num_lines)
        for l in range(levels):
            b = runs[l]["boxes"][i, l]
            want = sweep(l, b[0] + (b[1] - b[0]) * u, b[2] + (b[3] - b[2]) * v)
            got = runs[l]["sample_log_likelihoods_refined"][i]
            ok = ~np.isnan(want)   # (no exclusion but what the oracle itself returns as NaN)
            assert ok.any() and not np.isnan(got[ok]).any(), i
            worst = max(worst, float(np.abs(got[ok] - want[ok]).max()))
            compared += int(ok.sum())
    print(f"{compared} refined log-likelihoods, worst |delta| vs the oracle {worst:.3e}")
    assert compared > 0 and worst <= 1e-8


@pytest.mark.parametrize("kernel,name", [(0, "k_sweep_slim<3>"), (1, "k_sweep_slim<0>"), (2, "k_sweep_slim_boxed<3>"),
                                         (3, "k_sweep_slim_boxed<0>")])
def test_two_blocks_share_a_compute_unit(kernel, name):
    from gp_dla_detection_amd import _lib
    lib = _lib.load()
    blocks = C.c_int(-1)
    _lib.check(lib.gpdla_debug_slim_sweep_blocks_per_cu(kernel, C.byref(blocks)))
    print(name, "blocks per compute unit:", blocks.value)
    assert blocks.value == 2
