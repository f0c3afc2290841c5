"""CPU-side checks of the restatement the GPU test of the multi-DLA epilogue compares against
(tests/multi_epilogue_restatement.py): the generator against the Random123 known answers and the
library's own Philox, and the acceptance rule of the weighted draw against a float64 emulation of
k_multi_resample -- accepted as written, rejected under each of five one-line mutations -- with the counts that
show the rule is neither vacuous (every draw has exactly one acceptable index) nor weaker than the 40-bin
chi-square of test_gpu_configs.py::test_resampling_follows_the_weights, whose statistic is computed on the same
emulated draws.

The mutation table below (tables that reject / fraction of draws moved / chi-square verdict at S = 19200):

    index_minus_one           every table                    1.00      not caught
    inclusive_offsets         every table that has a second  0.20-1.0  caught (statistic 318 .. 698 against 82)
                              weight or a second chunk
    same_stream_every_model   every table with > 1 weight    0.87-1.0  not caught
    key_low_word_only         every table with > 1 weight    0.87-1.0  not caught
    uniform_from_r0_only      broad and equal_maxima at      1e-4      not caught
                              S = 19200 (one draw each)
"""
import ctypes as C

import numpy as np
import pytest

from gp_dla_detection_amd import _lib

import multi_epilogue_restatement as R
from mock_restatement import philox4x32_10

SEED = 0x0123456789ABCDEF          # both halves non-zero
KAT = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]   # Random123 kat_vectors: philox4x32 10


def key_of(S):
    """(seed, qid, nd) of a table of size S: odd sizes take a quasar index above 2^32, every third size model 2."""
    return SEED, (2 ** 32 + 5 if S % 2 else 3), 1 + (S % 3 == 0)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


@pytest.fixture(scope="module")
def runs():
    """Every table once: its exact weights, its uniforms, the emulated draws as written and under each mutation."""
    out = {}
    for kind in R.TABLE_KINDS:
        for S in R.TABLE_SIZES:
            col = R.table(kind, S)
            key = key_of(S)
            m = R.uniforms(*key, S)
            ex = R.weights_exact(col)
            draws = {None: R.emulate_resample(col, m)}
            for mut in R.MUTATIONS:
                draws[mut] = R.emulate_resample(col, m, mut, key)
            out[kind, S] = dict(col=col, m=m, ex=ex, draws=draws)
    return out


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert [int(x) for x in philox4x32_10(*ctr, *key)] == want


def test_uniforms_against_the_librarys_philox(lib):
    """Twelve (j, nd, qid) triples, quasar indices on both sides of 2^32, a seed with a non-zero high half: the
    words come from gpdla_debug_philox4x32_10 (the function k_multi_resample calls), the key, the counter and the
    53 bits are assembled here from the text of the kernel."""
    triples = [(0, 1, 0), (1, 1, 0), (255, 2, 7), (256, 1, 7), (19199, 3, 2 ** 32 + 5), (3, 2, 2 ** 32 + 5),
               (1024, 1, 2 ** 32), (17, 4, 2 ** 40 + 9), (5, 1, 2 ** 32 - 1), (5, 2, 2 ** 32 - 1), (700, 1, 123456789),
               (63, 3, 2 ** 63 - 1)]
    for seed in (SEED, 0x9E3779B97F4A7C15):
        for j, nd, qid in triples:
            k = (C.c_uint32 * 2)((seed ^ qid) & 0xFFFFFFFF, ((seed >> 32) ^ (qid >> 32) ^ 0x5851F42D) & 0xFFFFFFFF)
            o = (C.c_uint32 * 4)()
            lib.gpdla_debug_philox4x32_10((C.c_uint32 * 4)(j, 0, nd, 0), k, o)
            want = (o[0] >> 5) * 2 ** 26 + (o[1] >> 6)
            m = R.uniforms(seed, qid, nd, j + 1)
            assert int(m[j]) == want and want < 2 ** 53, (seed, j, nd, qid)
            # and the mutated generators are other generators
            for mut in ("same_stream_every_model", "uniform_from_r0_only"):
                assert int(R.uniforms(seed, qid, nd, j + 1, mutate=mut)[j]) != want
            assert (int(R.uniforms(seed, qid, nd, j + 1, mutate="key_low_word_only")[j]) != want) == \
                bool((seed >> 32) ^ (qid >> 32))
    # models 1 and 2 of one quasar, and two quasars 2^32 apart, draw different streams
    assert (R.uniforms(SEED, 5, 1, 64) != R.uniforms(SEED, 5, 2, 64)).all()
    assert (R.uniforms(SEED, 5, 1, 64) != R.uniforms(SEED, 2 ** 32 + 5, 1, 64)).all()


def test_tables_are_what_they_say():
    for S in R.TABLE_SIZES:
        for kind in R.TABLE_KINDS:
            col = R.table(kind, S)
            d = col - np.nanmax(col)
            assert col.shape == (S,) and not ((d > -745) & (d < -700)).any()      # every weight is 0 or normal
        if S > 1:
            peaked, nans, eq = R.table("peaked", S), R.table("nans", S), R.table("equal_maxima", S)
            assert (np.exp(np.delete(peaked, (2 * S) // 3) - peaked.max()) == 0).all()
            assert np.isnan(nans[0]) and np.isnan(nans[S // 2]) and np.isnan(nans[-1]) and np.isfinite(nans).sum() >= S // 2
            assert (eq == eq.max()).sum() == 2


def test_the_emulation_as_written_is_accepted_and_every_draw_is_decided(runs):
    """Non-vacuity: over all tables at most one draw in 10^5 may have more than one acceptable index (about
    2 S eps per draw, below 1e-8, are expected); and no draw of the unmutated emulation is outside its set."""
    total = ambiguous = 0
    for (kind, S), r in runs.items():
        bad, amb = R.check_draws(r["col"], r["m"], r["draws"][None], r["ex"])
        assert bad == 0, (kind, S, bad)
        total += S
        ambiguous += amb
    print(f"{ambiguous} of {total} draws have more than one acceptable index")
    assert total == 4 * sum(R.TABLE_SIZES) and ambiguous * 10 ** 5 <= total


def test_acceptable_is_the_exact_interval():
    """The single-draw form on a column whose prefix sums are exact binary fractions: weights 1/2, 1/4, NaN, 1/4."""
    col = np.array([0.0, -np.log(2.0), np.nan, -np.log(2.0)]) - 7.0
    for u, want in ((0, {0}), (2 ** 51, {0}), (2 ** 52 - 2 ** 20, {0}), (2 ** 52, {0, 1}), (2 ** 52 + 2 ** 20, {1}),
                    (3 * 2 ** 51, {1, 3}), (2 ** 53 - 1, {3})):
        assert R.acceptable(col, u) == want, u
    assert R.eps_of(257) == 262 * 2.0 ** -52 and R.eps_of(256) == 261 * 2.0 ** -52 and R.eps_of(19200) == 335 * 2.0 ** -52


def test_every_mutation_is_rejected_and_where(runs):
    """The acceptance rule against five wrong kernels, table by table; the fraction of draws each one moves; and
    the verdict of the 40-bin chi-square (99.99 % quantile, as test_resampling_follows_the_weights) on the same
    draws at S = 19200, which only notices the inclusive offsets."""
    rejected = {mut: set() for mut in R.MUTATIONS}
    moved = {mut: {} for mut in R.MUTATIONS}
    for (kind, S), r in runs.items():
        for mut in R.MUTATIONS:
            bad, _ = R.check_draws(r["col"], r["m"], r["draws"][mut], r["ex"])
            moved[mut][kind, S] = float((r["draws"][mut] != r["draws"][None]).mean())
            assert bad == int((r["draws"][mut] != r["draws"][None]).sum())     # rejected draw by draw: every moved one
            if bad:
                rejected[mut].add((kind, S))
    everything = set(runs)
    several_weights = {(k, S) for k, S in everything if S > 1 and k != "peaked"}
    assert rejected["index_minus_one"] == everything
    # one weight: the offsets matter only if the peak's thread is not the last with samples (S = 257: chunk 2,
    # the peak at 171 in thread 85 of 129; S = 1024, 19200: thread 170 of 256)
    assert rejected["inclusive_offsets"] == several_weights | {("peaked", 257), ("peaked", 1024), ("peaked", 19200)}
    assert rejected["same_stream_every_model"] == several_weights
    assert rejected["key_low_word_only"] == several_weights
    assert rejected["uniform_from_r0_only"] == {("broad", 19200), ("equal_maxima", 19200)}
    caught = {}
    for mut in (None,) + R.MUTATIONS:
        verdicts = []
        for kind in ("broad", "nans", "equal_maxima"):
            r = runs[kind, 19200]
            stat, quantile, on_zero = R.chi_square_40(r["col"], np.maximum(r["draws"][mut], 0))
            verdicts.append(stat >= quantile or on_zero > 0)
            print(f"{str(mut):24s} {kind:13s} S=19200: moved {moved[mut][kind, 19200] if mut else 0.0:.4f}, "
                  f"chi-square {stat:6.1f} against {quantile:.1f}")
        caught[mut] = any(verdicts)
    assert caught == {None: False, "index_minus_one": False, "inclusive_offsets": True,
                      "same_stream_every_model": False, "key_low_word_only": False, "uniform_from_r0_only": False}
    for mut in R.MUTATIONS:
        f = [v for key, v in moved[mut].items() if key in rejected[mut]]
        print(f"{mut:24s} rejected on {len(rejected[mut]):2d} of {len(everything)} tables, moves {min(f):.4f} .. {max(f):.4f} of their draws")
    assert min(moved["index_minus_one"].values()) == 1.0
    assert max(moved["uniform_from_r0_only"].values()) < 1e-3


def test_evidence_map_mask_and_posteriors_restated():
    """The small restatements on cases done by hand."""
    import mpmath as mp
    col = np.array([np.nan, -5.0, -3.0, np.nan, -3.0, -4.0])
    mx, arg, ev = R.evidence_exact(col, nd=2)
    assert (mx, arg) == (-3.0, 2)
    want = -3.0 + np.log((np.exp(-2.0) + 2 + np.exp(-1.0)) / 4) - np.log(6)
    assert abs(float(ev) - want) < 1e-15
    assert R.evidence_bound(-3.0, 6) == 2 * 2.0 ** -51 + 17 * 2.0 ** -52
    assert np.isnan(R.evidence_exact(np.full(3, np.nan))[0]) and R.evidence_exact(np.full(3, np.nan))[1] == 0
    base = np.array([[3, 1, 6, 2, 0, 4], [1, 1, 1, 1, 1, 1]], dtype=np.uint32)
    np.testing.assert_array_equal(R.map_chain(col, base, 3), [3.0, 6.0, 1.0])
    np.testing.assert_array_equal(R.map_chain(np.where(np.arange(6) == 4, 0.0, col), base, 2), [5.0, np.nan])
    np.testing.assert_array_equal(R.map_chain(np.full(6, np.nan), base, 2), [1.0, 3.0])
    z = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0])
    np.testing.assert_array_equal(R.separation_mask(z, base, 1, 1.5), np.zeros(6, bool))
    np.testing.assert_array_equal(R.separation_mask(z, base, 2, 1.5), [False, True, False, False, True, False])
    np.testing.assert_array_equal(R.separation_mask(z, base, 3, 1.5), [True, True, False, True, True, False])
    assert R.closest_to_separation(z, base, 2, 1.5) == 0.5 / np.spacing(1.5)
    lpost, post, p_dla = R.posteriors_exact([-1.0, -2.0, -3.0, -4.0], [-10.0, -1000.0, -8.0, -9.0])
    np.testing.assert_array_equal(lpost, [-11.0, -1002.0, -11.0, -13.0])
    assert float(post[1]) == 0.0 and 0 < post[1] < mp.mpf(10) ** -400       # a 50-digit value, not a double
    assert abs(float(post[0]) - 1 / (2 + np.exp(-2.0))) < 1e-16 and abs(float(p_dla) - (1 - float(post[0]))) < 1e-16
    lpost, post, p_dla = R.posteriors_exact([-1.0, -2.0, -3.0], [-10.0, -8.0, np.nan])
    assert np.isnan(lpost[2]) and all(mp.isnan(x) for x in post) and mp.isnan(p_dla)
    assert R.ulps(1.0 + 2.0 ** -50, mp.mpf(1)) == 4.0 and R.ulps(0.0, mp.mpf(0)) == 0.0
