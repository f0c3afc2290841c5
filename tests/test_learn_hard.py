"""CPU checks of the hard classes of the learning front end (tests/learn_hard_cases.py) and their 50-digit fixture
(tests/golden/exact_learn_hard*.npz), from the numpy restatement alone: the inputs are the ones the fixture was computed on,
the restatement stays within ORACLE_CAP of exact in every block with the fixture's NaN / +-inf placement and counts, the
excluded share is capped, the generator reproduces a class bit for bit, and every hard class is hard for a reason: a
deliberately worse float64 variant of the restatement misses the bound of test_gpu_learn_hard.py there and passes on
``control``."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import learn_hard_cases as LC  # noqa: E402
import learn_restatement as R  # noqa: E402


@pytest.fixture(scope="module")
def fixture(golden):
    return LC.load_fixture(golden)


@pytest.fixture(scope="module")
def problems():
    return {cls: LC.problem(cls) for cls in LC.CLASSES}


def test_fixture_holds_every_class(fixture):
    assert sorted(fixture) == sorted(LC.class_name(c) for c in LC.CLASSES)
    for name, entry in fixture.items():
        assert sorted(entry) == sorted(LC.KEYS), name
    for fname in LC.FIXTURES:
        assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", fname)) < 1 << 20


@pytest.mark.parametrize("cls", LC.CLASSES, ids=LC.class_name)
def test_restatement_stays_within_the_cap(cls, fixture, problems):
    csr, p = problems[cls]
    exact = fixture[LC.class_name(cls)]
    LC.check_digest(cls, exact, csr, p)
    nq = csr["z_qsos"].size
    assert nq <= 70 and LC.grid_size(p) <= 49 and np.diff(csr["offsets"]).max() <= 60
    got = LC.restated(cls, csr, p)
    assert not LC.patterns(got, exact)
    e = LC.deviation(got, exact)
    assert all(e[b] <= LC.ORACLE_CAP for b in LC.BLOCKS), e
    finite = np.isfinite(exact["rest_flux"])
    assert exact["excluded"].sum() <= LC.EXCLUDED_CAP * finite.sum()
    assert not (exact["excluded"] & ~finite).any()
    if cls[0].startswith("indicator_edge"):     # the class is at the edge: ties that float64 decides do occur
        assert exact["excluded"].sum() > 0


def test_the_classes_reach_what_they_are_for(fixture, problems):
    """the properties the class table of learn_hard_cases.py promises, read off the restatement and the fixture"""
    for mf in (False, True):
        got = LC.restated(("constant_columns", mf), *problems["constant_columns", mf])
        for g, count in {**LC.CONST_COLUMNS, **LC.ULP_COLUMNS}.items():
            assert got["count"][g] == count
        assert np.all(got["std"][list(LC.CONST_COLUMNS)] == 0.0)
        ulp = got["std"][list(LC.ULP_COLUMNS)]
        assert np.all(ulp > 0) and np.all(ulp < 1e-15) and np.all(np.isfinite(np.log(ulp)))
        assert got["rows_complete"] == 2
        sp = fixture[LC.class_name(("sparse_pairs", mf))]
        N = sp["N_pairwise"]
        assert np.all(N[np.ix_(range(16), range(16))] <= 2) and N[0, 0] == 2 and N[5, 5] == 1 and N[20, 20] == 0
        keep = lambda lo, holes: [g for g in range(lo, lo + 16) if g not in holes]  # noqa: E731
        assert np.all(N[np.ix_(keep(16, (20, 21)), keep(0, (5, 6)))] == 1) and np.all(N[16:32, 0:16] <= 1)
        assert np.all(N[32, 0:32] == 0) and N[32, 32] == 2 and sp["rows_complete"] == 0
        block = sp["cov_pairwise"][16:32, 0:16]
        assert np.isposinf(block).any() and np.isneginf(block).any()
        nc = LC.restated(("noise_cut", mf), *problems["noise_cut", mf])
        csr, p = problems["noise_cut", mf]
        cols = list(LC.CUT_COLUMNS)
        raw = np.array([csr["noise_variance"][o + 1:o + LC.G_SMALL:3] for o in csr["offsets"][:-1]])[:, :len(cols)]
        assert (raw == p.max_noise_variance).any() and (raw > p.max_noise_variance).any() and (raw < p.max_noise_variance).any()
        assert np.array_equal(np.isnan(nc["rest_noise"][:, cols]), raw > p.max_noise_variance)
    hz = fixture[LC.class_name(("high_z_tau100", True))]
    csr, p = problems["high_z_tau100", True]
    plain = LC.restated(("high_z_tau100", False), csr, p)     # the same spectra without the division
    with np.errstate(all="ignore"):
        absorption = plain["rest_flux"] / hz["rest_flux"]
    assert np.nanmin(absorption) < 1e-100 and np.all(np.isfinite(hz["rest_noise"][np.isfinite(plain["rest_noise"])]))


def test_generator_reproduces_a_class_bit_for_bit(fixture):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_exact_learn_hard as gen
    for cls in (("sparse_pairs", False), ("sparse_pairs", True)):
        again = gen.exact_class(cls)
        stored = fixture[LC.class_name(cls)]
        for key in LC.KEYS:
            assert np.array_equal(np.asarray(again[key]), stored[key], equal_nan=key != "sha256"), (cls, key)


# ---------------------------------------------------------------- sensitivity: a worse variant per hard class

def _one_pass_std(F):
    """the mean not subtracted before the std: sqrt((S2 - S1^2 / n) / (n - 1)) on the uncentred flux"""
    mu, centered, std, count = R.column_stats(F)
    fin = np.isfinite(F)
    X = np.where(fin, F, 0.0)
    n = count.astype(np.float64)
    with np.errstate(all="ignore"):
        worse = np.sqrt((np.sum(X * X, axis=0) - np.sum(X, axis=0) ** 2 / n) / (n - 1))
    return mu, centered, np.where(count > 1, worse, std), count


def _float32_bracket(x, v, xq):
    """interp1 with the bracket searched on float32 copies of the wavelengths"""
    x, v, xq = (np.asarray(a, dtype=np.float64) for a in (x, v, xq))
    out = np.full(xq.shape, np.nan)
    n = x.size
    if n < 2:
        return out
    j = np.clip(np.searchsorted(x.astype(np.float32), xq.astype(np.float32), side="right") - 1, 0, n - 2)
    val = v[j] + (xq - x[j]) / (x[j + 1] - x[j]) * (v[j + 1] - v[j])
    inside = (xq >= x[0]) & (xq <= x[-1])
    out[inside] = val[inside]
    return out


def _one_ulp_up(x, v, xq):
    """interp1 moved up by an ulp: 1 + z_j <= 1 + z_qso becomes 1 + z_j < 1 + z_qso"""
    return np.nextafter(_KEEP_INTERP1(x, v, xq), np.inf)


_KEEP_INTERP1 = R.interp1


def variant(name, cls, csr, p):
    """every block of a deliberately worse float64 evaluation"""
    if name == "one_pass_std":
        return LC.statistics(*LC.rest_grid(cls, csr, p), column_stats=_one_pass_std)
    if name == "tiny_flux_is_zero":          # an absolute epsilon where a relative one belongs
        F, L, N = LC.rest_grid(cls, csr, p)
        return LC.statistics(np.where(np.abs(F) < 1e-5, 0.0, F), L, N)
    if name == "float32_bracket":
        return LC.statistics(*LC.rest_grid(cls, csr, p, interp1=_float32_bracket))
    if name == "guarded_quotient":           # P / (N - 1) with the division by zero "made safe"
        out = LC.restated(cls, csr, p)
        out["cov_pairwise"] = np.where(out["N_pairwise"] == 1, 0.0, out["cov_pairwise"])
        return out
    if name == "equal_is_noisy":             # v >= max_noise_variance
        return LC.restated(cls, csr, dataclasses.replace(p, max_noise_variance=float(np.nextafter(p.max_noise_variance, -np.inf))))
    if name == "eight_lines":              # the Lyman series cut short
        return LC.restated(cls, csr, dataclasses.replace(p, num_forest_lines=8) if cls[1] else p)
    if name == "guarded_absorption":         # flux / max(e^-tau, 1e-60), noise / max(e^-tau, 1e-60)^2
        F, L, N = LC.rest_grid(cls, csr, p)
        if cls[1]:
            F0, _, N0 = LC.rest_grid((cls[0], False), csr, p)
            with np.errstate(all="ignore"):
                a = np.maximum(F0 / F, 1e-60)
                F, N = F0 / a, N0 / (a * a)
        return LC.statistics(F, L, N)
    if name == "strict_indicator":
        return LC.statistics(*LC.rest_grid(cls, csr, p, interp1=_one_ulp_up))
    raise ValueError(name)


VARIANT_OF = {"offset_flux_1e6": "one_pass_std", "offset_flux_1e-6": "one_pass_std", "constant_columns": "one_pass_std",
              "dynamic_range": "tiny_flux_is_zero", "tight_pixels": "float32_bracket", "sparse_pairs": "guarded_quotient",
              "noise_cut": "equal_is_noisy", "high_z": "eight_lines", "high_z_tau100": "guarded_absorption",
              "indicator_edge_beta": "strict_indicator", "indicator_edge_gamma": "strict_indicator"}


def passes(cls, got, exact, e_rest) -> bool:
    """what test_gpu_learn_hard.py asks of the GPU, asked of ``got``"""
    return not LC.patterns(got, exact) and not LC.failures(cls, LC.deviation(got, exact), e_rest)


@pytest.mark.parametrize("cls", LC.HARD_CLASSES, ids=LC.class_name)
def test_a_worse_variant_fails_here_and_passes_control(cls, fixture, problems):
    name = VARIANT_OF[cls[0]]
    control = ("control", cls[1])
    verdict = {}
    for c in (cls, control):
        csr, p = problems[c]
        exact = fixture[LC.class_name(c)]
        e_rest = LC.deviation(LC.restated(c, csr, p), exact)
        assert passes(c, LC.restated(c, csr, p), exact, e_rest)
        verdict[c] = passes(c, variant(name, c, csr, p), exact, e_rest)
    assert verdict[control] and not verdict[cls], (name, verdict)
