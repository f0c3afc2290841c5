"""The other three production sweeps at the places where their software pipelines can go wrong, as
test_gpu_sweep_chunk_edges.py does for k_sweep_slim.

k_sweep_split_slim<LINES, 0> (20 < k <= 40, single DLA) and <0, ND> (multi-DLA, ND = 1 .. 4 and the sub-DLA
pass): one loop iteration is one 8-step chunk and one block barrier, stage W runs one iteration ahead of
stage C, stage R is primed 20 raw steps ahead into a ring of 32 K-steps per sample (multi-DLA: profile
gathers, clamped at the last padded pixel, in its place).  Spectra of
    2, 7 | 8 | 9, 15 | 16 | 17, 24 | 25, 31 | 32 | 33, 40 | 41   one short of, on, one past a chunk edge
    19 | 20 | 21                                                the priming length
    27 | 28 | 29                                                the first raw step written beyond the priming
    32 | 33, 40 | 41                                            the ring wrap, and a whole chunk beyond it
K-steps, whose last K-step holds 1, 2, 3 or 4 pixels in turn, at S = 15 (null slot last in group 0, group 1
idle), 16 (first in group 1), 31 (last in the block), 32 (alone with 31 idle copies in a block of its own)
and 80 (the ordinary place).

k_sweep_multi_slim<ND> (k <= 20, multi-DLA): 8-step chunks, wave w expanding K-step w of the next chunk,
profile gathers issued as inline assembly four K-steps ahead and waited for by a hand-computed vmcnt that
depends on ND.  Spectra of 1 (two pixels, and four), 3 | 4 | 5 (shorter than, equal to, just past the
gather lead), 7 | 8 | 9, 15 | 16 | 17 (chunk edges), 12 and 25 K-steps at S = 127 (null slot last in the
block), 128 (alone in a block of its own) and 200; 127 / 128 / 200 also straddle the 64-sample waves of
k_profiles.  The list starts at ONE K-step: spectra of 1 .. 4 pixels upload with status 0.  (A single pixel
is not in the list: its search range has no width, every pair of samples is closer than min_z_separation,
and the quasar's loop ends at the two-DLA model -- on the GPU and in the oracle alike.)

Every case is compared bit for bit with the pre-expanded kernels (libgpdla_legacy.so with
GPDLA_EXPANDED_RECORDS=1 in a clean child process: k_sweep_split, k_sweep_multi_split, k_sweep_multi), the
same products and the same MFMA sequence per column -- at MultiParameters(max_dlas=4), so that ND = 4 is
run -- and, because those kernels share k_prepare, k_profiles, the record builder's source rows and the
epilogue with the slim ones, with the CPU oracle at the sample count that leaves the null slot alone in a
block.  No comparison may pass on NaN tables: every spectrum of every case has status 0, wholly finite
model-1 / sub-DLA / single-DLA sample tables and a finite evidence for every model (an all-NaN model would
have ended the quasar's loop and the ND >= 2 kernels would have returned at once).  Hot loops:
process_qsos.m:185-199, process_qsos_multiple_dlas_meanflux.m:340-381."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import sweep_chunk_edges_worker as w

pytestmark = pytest.mark.gpu

S_SPLIT = [15, 16, 31, 32, 80]      # 32 slots a block, two groups of 16
S_MULTI_SLIM = [127, 128, 200]      # 128 slots a block
FAMILY = {"split": (w.PIXELS_SPLIT, w.K_STEPS_SPLIT, S_SPLIT, 32),
          "multi_slim": (w.PIXELS_MULTI_SLIM, w.K_STEPS_MULTI_SLIM, S_MULTI_SLIM, 128)}
TOL = 1e-8  # test_gpu_parity.py, test_gpu_multi.py

_got, _steps = {}, {}


def family_of(kind, k):
    assert kind == "multi" or k > 20   # (single DLA at k <= 20: test_gpu_sweep_chunk_edges.py)
    return "split" if k > 20 else "multi_slim"


def steps_of(kind, k):
    """K-steps per spectrum from the uploaded batch (they depend on the pixel list alone; read once per
    kernel family and kind)"""
    fam = family_of(kind, k)
    if (kind, fam) not in _steps:
        _steps[kind, fam] = w.k_steps(k, 3, 16, kind, FAMILY[fam][0])
    return _steps[kind, fam]


def got_case(kind, k, num_lines, num_samples, supplied_block=0):
    """The product library's result of a case, computed once and shared by the tests that compare it"""
    key = (kind, k, num_lines, num_samples, supplied_block)
    if key not in _got:
        out = w.run_case(k, num_lines, num_samples, kind, FAMILY[family_of(kind, k)][0], supplied_block)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _got[key] = out
    return _got[key]


def expanded(kind, k, num_lines, num_samples, tmp_path, supplied_block=0):
    """The same case(s) on the pre-expanded records: num_samples is one count or a list (one child for all)"""
    out = tmp_path / f"{kind}_{k}_{num_lines}.npz"
    from gp_dla_detection_amd import _lib
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    env = {"GPDLA_EXPANDED_RECORDS": "1", "GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH}
    pr = mp.get_context("forkserver").Process(
        target=w.run_child, args=(k, num_lines, num_samples, env, str(out), kind, FAMILY[family_of(kind, k)][0],
                                  supplied_block))
    pr.start()
    pr.join(600)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
    assert pr.exitcode == 0
    return np.load(out)


def assert_not_vacuous(got, kind, k, label):
    """Section "no comparison may pass on NaN tables" of the module docstring, for every spectrum"""
    steps = steps_of(kind, k)
    wanted = FAMILY[family_of(kind, k)][1]
    assert (np.asarray(got["status"]) == 0).all(), (label, got["status"])
    sll = np.asarray(got["sample_log_likelihoods_dla"])
    if kind == "single":
        finite = [int(np.isfinite(sll).sum())]
        good = np.isfinite(sll).all(axis=1) & np.isfinite(got["log_likelihoods_dla"]) \
            & np.isfinite(got["log_likelihoods_no_dla"])
    else:
        finite = [int(np.isfinite(sll[:, nd]).sum()) for nd in range(sll.shape[1])]
        good = np.isfinite(sll[:, 0]).all(axis=1) & np.isfinite(got["sample_log_likelihoods_lls"]).all(axis=1) \
            & np.isfinite(got["log_likelihoods_dla"]).all(axis=1) & np.isfinite(got["log_likelihoods_lls"]) \
            & np.isfinite(got["log_likelihoods_no_dla"])
    print(f"{label}: finite entries per model {finite} of {sll.shape[0] * sll.shape[-1]}")
    assert good.all(), (label, "spectra with NaN tables or an early exit:", np.flatnonzero(~good).tolist())
    assert wanted <= {s for s, ok in zip(steps, good) if ok}
    return finite


def assert_bit_identical(got, want, prefix, label):
    checked = 0
    for full in want.files:
        if not full.startswith(prefix):
            continue
        name = full[len(prefix):]
        a, b = np.asarray(got[name]), want[full]
        assert a.shape == b.shape, (label, name)
        if a.dtype.kind == "f":
            assert np.array_equal(a, b, equal_nan=True), (label, name, float(np.nanmax(np.abs(a - b))))
        else:
            assert np.array_equal(a, b), (label, name)
        checked += 1
    return checked


@pytest.mark.parametrize("kind,k", [("single", 40), ("multi", 40), ("multi", 20)])
def test_the_spectra_cover_the_pipeline_edges(kind, k):
    steps = steps_of(kind, k)
    print(f"{kind}, k = {k}: K-steps per spectrum:", steps)
    wanted = FAMILY[family_of(kind, k)][1]
    assert wanted <= set(steps), sorted(wanted - set(steps))


@pytest.mark.parametrize("kind,k,num_lines", [("single", 40, 3), ("single", 33, 3),      # k_sweep_split_slim<3, 0>
                                              ("multi", 40, 3), ("multi", 33, 3),        # k_sweep_split_slim<0, 1..4>
                                              ("multi", 20, 3), ("multi", 13, 3),        # k_sweep_multi_slim<1..4>
                                              ("multi", 20, 31), ("multi", 40, 31)])     # k_profiles' run-time tier
def test_pipeline_edges_bit_for_bit(kind, k, num_lines, tmp_path):
    """Every array of the result, base_sample_inds included, at every sample count of the kernel's family
    (the 31-line cases: at the count that leaves the null slot alone in a block)"""
    counts = FAMILY[family_of(kind, k)][2]
    if num_lines != 3:
        counts = [c for c in counts if c % FAMILY[family_of(kind, k)][3] == 0]
    want = expanded(kind, k, num_lines, counts, tmp_path)
    for S in counts:
        label = f"{kind}, k = {k}, {num_lines} lines, S = {S}"
        got = got_case(kind, k, num_lines, S)
        assert_not_vacuous(got, kind, k, label)
        checked = assert_bit_identical(got, want, f"S{S}/", label)
        assert checked >= (20 if kind == "multi" else 10), (label, checked)
        if kind == "multi":
            bsi = np.asarray(got["base_sample_inds"])
            assert f"S{S}/base_sample_inds" in want.files and bsi.min() >= 1 and bsi.max() <= S


def test_run_time_line_count_at_pipeline_edges(tmp_path):
    """k_sweep_split_slim<0, 0>: the 1e-9 rule of test_gpu_record_classes.py (there: why not bit for bit)"""
    k, num_lines, num_samples = 27, 5, 32
    want = expanded("single", k, num_lines, num_samples, tmp_path)
    got = got_case("single", k, num_lines, num_samples)
    assert_not_vacuous(got, "single", k, f"single, k = {k}, {num_lines} lines, S = {num_samples}")
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


@pytest.mark.parametrize("k,num_samples", [(40, 80), (20, 200)])
def test_supplied_indices_at_block_edges_bit_for_bit(k, num_samples, tmp_path):
    """base_sample_inds supplied to both libraries: 0 (never drawn), 1 and S in the sample slots on each
    side of every block edge and in the last sample, so that those rows go through chain_ok = 0 (the
    sample is NaN from that model on) and through kk = S - 1"""
    block = FAMILY[family_of("multi", k)][3]
    bsi, slots = w.edge_indices(len(FAMILY[family_of("multi", k)][0]), num_samples, block)
    assert {block - 1, block, num_samples - 1} <= set(slots)
    for row in range(w.MAX_DLAS - 1):
        assert {0, 1, num_samples} <= set(bsi[0, row, slots].tolist())
    label = f"multi, k = {k}, S = {num_samples}, supplied indices"
    want = expanded("multi", k, 3, num_samples, tmp_path, supplied_block=block)
    got = got_case("multi", k, 3, num_samples, supplied_block=block)
    assert_not_vacuous(got, "multi", k, label)
    assert assert_bit_identical(got, want, "", label) >= 20
    np.testing.assert_array_equal(got["base_sample_inds"], bsi)
    sll = np.asarray(got["sample_log_likelihoods_dla"])
    for nd in range(1, w.MAX_DLAS):  # a sample is NaN from the first model whose index was never drawn
        never = (bsi[:, :nd] == 0).any(axis=1)
        assert np.isnan(sll[:, nd][never]).all() and never[:, slots].any()
        # the edge slots whose chain is whole up to this model (and does not name the sample itself, which
        # min_z_separation rejects) follow 1 or S and are evaluated; S = 200 has three edge slots, one break
        # per model, so none is left for the four-DLA model
        whole = [s for s in slots if not never[0, s] and not (bsi[0, :nd, s] == s + 1).any()]
        assert whole or (nd == 3 and len(slots) == 3), (nd, slots)
        if whole:
            assert {1, num_samples} & set(bsi[0, :nd][:, whole].ravel().tolist())
            assert np.isfinite(sll[:, nd][:, whole]).any(), nd


@pytest.mark.parametrize("k", [40, 33])
def test_single_dla_pipeline_edges_vs_oracle(oracle, k):
    """As test_ranks_between_the_tile_classes, on the short spectra, null slot alone in a block (S = 32)"""
    from test_gpu_parity import run_oracle
    S = 32
    model, samples, spectra, _, _ = w.build_case(k, 3, S, "single", w.PIXELS_SPLIT)
    got = got_case("single", k, 3, S)
    assert_not_vacuous(got, "single", k, f"single, k = {k}, S = {S}")
    dev = []
    for i, sp in enumerate(spectra):
        ref = run_oracle(oracle, model, samples, sp)
        dev.append(max(abs(got["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]),
                       float(np.abs(got["sample_log_likelihoods_dla"][i] - ref["sample_log_likelihoods_dla"]).max())))
    dev = [d if d == d else np.inf for d in dev]
    print(f"single DLA, k = {k}, S = {S}: worst |delta| vs the oracle = {max(dev):.3e} "
          f"(spectrum {int(np.argmax(dev))}, {steps_of('single', k)[int(np.argmax(dev))]} K-steps)")
    assert max(dev) < TOL, [f"{d:.2e}" for d in dev]


@pytest.mark.parametrize("k,S", [(40, 32), (33, 32), (20, 128), (13, 128)])
def test_multi_dla_pipeline_edges_vs_oracle(oracle, k, S):
    """As test_gpu_resampling_then_oracle: indices drawn on the GPU, replayed by the oracle; null slot
    alone in a block"""
    from test_gpu_multi import compare, oracle_multi
    fam = family_of("multi", k)
    model, samples, spectra, _, p = w.build_case(k, 3, S, "multi", FAMILY[fam][0])
    got = got_case("multi", k, 3, S)
    assert_not_vacuous(got, "multi", k, f"multi, k = {k}, S = {S}")
    refs, dev, dev_map = [], [], []
    for i, sp in enumerate(spectra):
        ref = oracle_multi(oracle, model, samples, sp, got["base_sample_inds"][i], p)
        refs.append(ref)
        d = [abs(got["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]),
             abs(got["log_likelihoods_lls"][i] - ref["log_likelihood_lls"]),
             np.abs(got["sample_log_likelihoods_lls"][i] - ref["sample_log_likelihoods_lls"]).max(),
             np.abs(got["log_likelihoods_dla"][i] - ref["log_likelihoods_dla"]).max()]
        with np.errstate(invalid="ignore"):
            d.append(np.nanmax(np.abs(got["sample_log_likelihoods_dla"][i].T - ref["sample_log_likelihoods_dla"])))
            dev_map.append(max(float(np.nanmax(np.abs(got[key][i] - ref[key])))
                               for key in ("MAP_inds", "MAP_z_dlas", "MAP_log_nhis")))
        d = float(max(d))
        dev.append(d if d == d else np.inf)
    print(f"multi-DLA, k = {k}, S = {S}: worst |delta| vs the oracle = {max(dev):.3e} "
          f"(spectrum {int(np.argmax(dev))}, {steps_of('multi', k)[int(np.argmax(dev))]} K-steps), "
          f"MAP columns {max(dev_map):.3e}")
    for i in range(len(spectra)):
        compare(got, i, refs[i], p)
