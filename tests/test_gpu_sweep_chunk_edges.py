"""k_sweep_slim at the edges of its 8-step chunks.  The kernel requests the ring taps and the pixel row
of K-step t + 1 inside K-step t's MFMA burst and carries them across the unrolled steps of a chunk; the
first step of a chunk reads its own row behind the chunk barrier.  That schedule can only go wrong where a
chunk ends, in the last, partly filled chunk, and in the block that holds the null slot -- which the long
spectra at one sample count of test_gpu_record_classes.py do not probe.  Here: spectra of 2 .. 25 K-steps
(one short of, on, and one past a chunk edge) at sample counts that put the null slot last in a block
(127), alone with 15 idle copies in a block of its own (128), and in the ordinary place (300), against
k_sweep on the pre-expanded records (libgpdla_legacy.so with GPDLA_EXPANDED_RECORDS=1 in a clean child
process): the same products and the same MFMA sequence per column, so every output is bit-identical at
three lines; at a run-time line count (k_sweep_slim<0>) the 1e-9 rule of test_gpu_record_classes.py
holds.  Hot loop: process_qsos.m:185-199."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import sweep_chunk_edges_worker as w

pytestmark = pytest.mark.gpu

K_STEPS_WANTED = {2, 3, 7, 8, 9, 15, 16, 17, 25}


def expanded(k, num_lines, num_samples, tmp_path):
    out = tmp_path / f"{k}_{num_lines}_{num_samples}.npz"
    from gp_dla_detection_amd import _lib
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    env = {"GPDLA_EXPANDED_RECORDS": "1", "GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH}
    pr = mp.get_context("forkserver").Process(target=w.run_child, args=(k, num_lines, num_samples, env, str(out)))
    pr.start()
    pr.join(600)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
    assert pr.exitcode == 0
    return np.load(out)


def test_the_spectra_cover_the_chunk_edges():
    steps = w.k_steps(20, 3, 128)
    print("K-steps per spectrum:", steps)
    assert K_STEPS_WANTED <= set(steps), sorted(K_STEPS_WANTED - set(steps))


@pytest.mark.parametrize("num_samples", [127, 128, 300])
def test_three_lines_at_chunk_edges_bit_for_bit(num_samples, tmp_path):
    want = expanded(20, 3, num_samples, tmp_path)
    got = w.run_case(20, 3, num_samples)
    checked = 0
    for name in want.files:
        a, b = np.asarray(got[name]), want[name]
        assert a.shape == b.shape, name
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), (name, float(np.nanmax(np.abs(a - b))))
        else:
            assert np.array_equal(a, b), name
        checked += 1
    assert checked >= 10
    assert np.isfinite(np.asarray(got["sample_log_likelihoods_dla"])).any()


def test_run_time_line_count_at_chunk_edges(tmp_path):
    k, num_lines, num_samples = 13, 5, 128
    want = expanded(k, num_lines, num_samples, tmp_path)
    got = w.run_case(k, num_lines, num_samples)
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
