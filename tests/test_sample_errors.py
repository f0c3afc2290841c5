"""Host side of the bootstrap sample errors (gp_dla_detection_amd/cddf.py): the strata,
the draw mapping against the library's own Philox, the validation that runs before any device call and
the quadrature rule of k_path_lengths against 30-digit integration.  The GPU side is
tests/test_gpu_sample_errors.py."""
import ctypes as C
import os

import numpy as np
import pytest

import sample_error_restatement as R
from gp_dla_detection_amd import _lib, cddf

HERE = os.path.dirname(os.path.abspath(__file__))


def assert_strata(z, label, min_count):
    z = np.asarray(z, dtype=np.float64)
    assert label.shape == z.shape and label.dtype == np.int32
    counts = np.bincount(label)
    assert label.min() == 0 and np.all(counts > 0)                       # dense labels: each sightline in exactly one
    if counts.size > 1:
        assert counts.min() >= min_count
    order = np.argsort(z, kind="stable")
    assert np.all(np.diff(label[order]) >= 0)                            # strata are intervals of max_z_dla


@pytest.mark.parametrize("name, z", [
    ("all equal", np.full(500, 3.0)),
    ("three sightlines", np.array([2.0, 3.0, 4.0])),
    ("one", np.array([2.5])),
    ("one far outlier", np.r_[np.random.default_rng(1).uniform(2.0, 2.5, 200), 400.0]),
    ("two clumps", np.r_[np.full(40, 2.0), np.full(40, 5.0)]),
    ("nineteen", np.linspace(2, 5, 19)),
    ("infinite", np.r_[np.linspace(2, 5, 50), np.inf]),
    ("dr12q-like", 2.0 + np.random.default_rng(2).gamma(2.0, 0.4, 20000)),
])
def test_bootstrap_strata_terminates_and_keeps_min_count(name, z):
    label = cddf.bootstrap_strata(z)
    assert_strata(z, label, 10)
    if name == "dr12q-like":
        assert np.bincount(label).size >= 5
    if name in ("all equal", "three sightlines", "one", "nineteen", "infinite"):
        assert label.max() == 0


def test_bootstrap_strata_options_and_errors():
    z = np.random.default_rng(3).uniform(2, 5, 3000)
    for min_count, num in ((1, 9), (10, 1), (10, 3), (500, 9), (2000, 9)):
        label = cddf.bootstrap_strata(z, min_count=min_count, num_strata=num)
        assert_strata(z, label, min_count)
        assert np.bincount(label).size <= num
    assert np.bincount(cddf.bootstrap_strata(z, 10, 9)).size == 9
    assert cddf.bootstrap_strata(np.zeros(0)).size == 0
    with pytest.raises(ValueError):
        cddf.bootstrap_strata([2.0, np.nan, 3.0])
    with pytest.raises(ValueError):
        cddf.bootstrap_strata(z, min_count=0)


def test_draw_mapping_reproduces_the_librarys_philox():
    _lib.build()
    lib = _lib.load()
    seed = 0x0123456789ABCDEF
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
    stratum = np.repeat([0, 1, 4], [7, 1, 30])
    first, size = R.stratum_extents(stratum)
    assert first.tolist() == [0] * 7 + [7] + [8] * 30 and size.tolist() == [7] * 7 + [1] + [30] * 30
    for r in (0, 1, 63, 2 ** 32 - 1):
        rows = R.drawn_rows(stratum, r, seed)
        for j in range(stratum.size):
            out = (C.c_uint32 * 4)()
            lib.gpdla_debug_philox4x32_10((C.c_uint32 * 4)(j, 0, r, 2), key, out)
            assert rows[j] == first[j] + ((out[0] * int(size[j])) >> 32)
        assert np.all((rows >= first) & (rows < first + size))          # a draw stays inside its stratum
    # a position past 2^32 uses the high counter word
    w = R.philox4x32_10(np.uint64(5), np.uint64(1), np.uint64(3), np.uint64(2), seed & 0xFFFFFFFF, seed >> 32)[0]
    out = (C.c_uint32 * 4)()
    lib.gpdla_debug_philox4x32_10((C.c_uint32 * 4)(5, 1, 3, 2), key, out)
    assert int(w) == out[0]
    # replicates and seeds give different draws; the stream word keeps them apart from resampling and mocks
    big = np.zeros(4000, dtype=np.int64)
    a, b, c = R.drawn_rows(big, 0, seed), R.drawn_rows(big, 1, seed), R.drawn_rows(big, 0, seed + 1)
    assert np.mean(a == b) < 0.01 and np.mean(a == c) < 0.01
    assert abs(np.mean(a) - 1999.5) < 5 * 4000 / np.sqrt(12 * 4000)      # uniform over the stratum


def test_bad_bootstrap_inputs_are_rejected_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_device)
    V = np.ones((6, 3))
    lab = np.array([0, 0, 0, 1, 1, 1])
    for seed in (np.nan, 1.5, -1, 2 ** 64, "seed", None):
        with pytest.raises(ValueError):
            cddf.bootstrap_sums(V, lab, 4, seed)
    for reps in (0, -3, 2.5):
        with pytest.raises(ValueError):
            cddf.bootstrap_sums(V, lab, reps, 1)
    bad = V.copy()
    bad[2, 2] = np.inf
    with pytest.raises(ValueError, match="path-length"):
        cddf.bootstrap_sums(bad, lab, 4, 1, path_columns=slice(2, 3))
    bad[2, 2] = np.nan
    with pytest.raises(ValueError, match="path-length"):
        cddf.bootstrap_sums(bad, lab, 4, 1, path_columns=[2])
    with pytest.raises(ValueError):
        cddf.bootstrap_sums(V, lab[::-1], 4, 1)                          # not sorted by stratum
    with pytest.raises(ValueError):
        cddf.bootstrap_sums(V, lab[:5], 4, 1)
    with pytest.raises(ValueError):
        cddf.bootstrap_sums(np.ones((6, 257)), lab, 4, 1)
    with pytest.raises(ValueError):
        cddf.bootstrap_sums(V, lab, 4, 1, first_replicate=2 ** 32 - 2)
    # edges of the path-length matrix
    z = np.array([2.0, 2.5]), np.array([3.0, 3.5]), np.ones(2)
    for edges in ([2.0, np.nan], [2.0, 2.0], [3.0, 2.0], [2.0], np.linspace(2, 3, 67), [-2.0, 1.0], [0.0, 2000.0]):
        with pytest.raises(ValueError):
            cddf.path_length_matrix(*z, edges)
    with pytest.raises(ValueError, match="ends below"):
        cddf.path_length_matrix(np.array([3.0]), np.array([2.0]), np.ones(1), [2.0, 3.0])
    with pytest.raises(ValueError):
        cddf.path_length_matrix(*z, [2.0, 3.0], proximity_zone=np.nan)


def test_gauss_legendre_rule_against_30_digit_quadrature():
    """The 8-node rule on panels no wider than 0.25, with the nodes the kernel holds, against
    mpmath.quad at 30 digits: the bins of the default requests and [1, 6] as one bin."""
    import mpmath
    mpmath.mp.dps = 30
    om = mpmath.mpf(0.279)                                               # the double the code uses

    def f(z):
        return (1 + z) ** 2 / mpmath.sqrt(om * (1 + z) ** 3 + 1 - om)

    zb = cddf.line_density_request(2, 4).edges
    assert zb == cddf.omega_dla_request(2, 4).edges
    cases = list(zip(zb[:-1], zb[1:])) + [(1.0, 6.0), (2.0, 4.0), (2.0, 5.0), (2.31, 2.3100001), (0.0, 0.26), (5.9, 7.4)]
    worst = 0.0
    for a, b in cases:
        want = mpmath.quad(f, mpmath.linspace(mpmath.mpf(a), mpmath.mpf(b), 9))
        got = cddf.gauss_legendre_path(a, b)
        worst = max(worst, abs(float((mpmath.mpf(got) - want) / want)))
    print("worst relative error of the rule:", worst)
    assert worst < 1e-13
    # the nodes and weights are those of the 8-point rule, correctly rounded
    P = lambda x: mpmath.legendre(8, x)
    for x, w in zip(cddf.GAUSS_NODES, cddf.GAUSS_WEIGHTS):
        root = mpmath.findroot(P, (x - 1e-3, x + 1e-3), solver="anderson")
        assert float(root) == x and float(2 / ((1 - root * root) * mpmath.diff(P, root) ** 2)) == w
    assert sum(cddf.GAUSS_WEIGHTS) == 1.0
    src = open(os.path.join(_lib.CSRC, "stats_kernels.hpp")).read()
    for v in cddf.GAUSS_NODES + cddf.GAUSS_WEIGHTS:
        assert repr(v) in src                                            # the kernel holds the same constants


def test_expected_counts_and_percentiles():
    part = dict(pois=np.array([[0.1, 0.0], [0.0, 0.2], [0.0, 0.0]]), count=np.array([2, 0, 1]),
                kept_bin=np.array([[1, 1] + [-1] * 6, [-1] * 8, [0] + [-1] * 7], dtype=np.int32),
                kept_p=np.array([[0.5, 0.25] + [0] * 6, [0] * 8, [0.9] + [0] * 7]))
    np.testing.assert_array_equal(cddf.expected_counts(part, 2), [[0.1, 0.75], [0.0, 0.2], [0.9, 0.0]])
    with pytest.raises(cddf.KeptCapacityError):
        cddf.expected_counts(dict(part, count=np.array([2, 9, 1])), 2)
    reps = np.column_stack([np.arange(101.0), np.r_[np.arange(100.0), np.nan], np.full(101, np.nan)])
    med, r68, r95 = cddf.sample_percentiles(reps)
    assert med[0] == 50 and r68[:, 0].tolist() == [84, 16] and r95[:, 0].tolist() == [97.5, 2.5]
    assert med[1] == 49.5 and np.isnan(med[2]) and r68.shape == r95.shape == (2, 3)


def test_abi_declares_the_entries():
    h = open(os.path.join(HERE, "..", "include", "gpdla.h")).read()
    names = [s[0] for s in _lib.SYMBOLS]
    for name in ("gpdla_stats_path_lengths", "gpdla_stats_bootstrap_sums"):
        assert name in h and name in names
    assert f"#define GPDLA_BOOTSTRAP_MAX_COLUMNS {cddf.BOOTSTRAP_MAX_COLUMNS}" in h
    assert "#define GPDLA_ABI_VERSION 6" in h
