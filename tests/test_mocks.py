"""CPU-side checks of the mock-spectra subsystem: the generator and the normal map
of the restatement the GPU tests compare against, the restatement itself as a draw from the model the
likelihood evaluates, the host truth table, request validation without a device and the layout of the
new structs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, mocks, synthetic
from gp_dla_detection_amd.parameters import Parameters

import mock_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------
# normals
# ------------------------------------------------------------------------------------------------

KAT = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]   # Random123 kat_vectors: philox4x32 10


def test_restatement_philox_known_answers(lib):
    for ctr, key, want in KAT:
        assert [int(x) for x in R.philox4x32_10(*ctr, *key)] == want
    # vectorised over counters, and equal to the library's generator on random counters / keys
    rng = np.random.default_rng(8)
    ctr = rng.integers(0, 2 ** 32, size=(4, 64), dtype=np.uint64)
    k0, k1 = (int(x) for x in rng.integers(0, 2 ** 32, 2))
    got = np.stack(R.philox4x32_10(*ctr, k0, k1))
    for j in range(64):
        c, k, o = (C.c_uint32 * 4)(*[int(x) for x in ctr[:, j]]), (C.c_uint32 * 2)(k0, k1), (C.c_uint32 * 4)()
        lib.gpdla_debug_philox4x32_10(c, k, o)
        assert list(o) == [int(x) for x in got[:, j]]


def test_key_and_counter_layout():
    """key = (seed ^ qid, (seed >> 32) ^ (qid >> 32) ^ 0x5851F42D); counter = (lo32, hi32, stream, 1)."""
    seed, qid = 0x0123456789ABCDEF, (5 << 32) | 77
    assert R.key(seed, qid) == (0x89ABCDEF ^ 77, 0x01234567 ^ 5 ^ 0x5851F42D)
    k0, k1 = R.key(seed, qid)
    idx = np.array([3, (9 << 32) | 4], dtype=np.uint64)
    for stream in (0, 1):
        want = [R.normal_from_mantissas(*R.mantissas(R.philox4x32_10(int(i) & 0xFFFFFFFF, int(i) >> 32, stream, 1, k0, k1)))
                for i in idx]
        np.testing.assert_array_equal(R.normals(seed, qid, stream, idx), np.array(want).reshape(-1))
    assert not np.array_equal(R.normals(seed, qid, 0, idx), R.normals(seed, qid, 1, idx))
    assert not np.array_equal(R.normals(seed, qid, 0, idx), R.normals(seed, qid + 1, 0, idx))


def test_uniform_to_normal_map_at_its_ends():
    top = float(2 ** 53 - 1)
    assert R.normal_from_mantissas(0.0, 0.0) == np.sqrt(106 * np.log(2.0))        # u1 = 2^-53, cos 0 = 1
    assert abs(R.normal_from_mantissas(0.0, 0.0) - 8.5717) < 1e-4                  # the largest |n|
    assert R.normal_from_mantissas(top, 0.0) == 0.0                                # u1 = 1: log 1 = 0
    assert R.normal_from_mantissas(top, 12345.0) == 0.0
    n = R.normal_from_mantissas(np.full(5, 2.0 ** 52), np.array([0.0, 2.0 ** 51, 2.0 ** 52, 3 * 2.0 ** 51, top]))
    r = np.sqrt(-2 * np.log((2.0 ** 52 + 1) * 2.0 ** -53))
    np.testing.assert_allclose(n, r * np.array([1.0, 0.0, -1.0, 0.0, 1.0]), rtol=0, atol=1e-15)   # m2 = 0: cos = 1
    m1, m2 = R.mantissas([np.uint64(0xFFFFFFFF)] * 4)
    assert m1 == m2 == top                                                         # 27 + 26 bits
    x = R.normals(1, 2, 1, np.arange(200000))
    assert np.abs(x).max() <= 8.58 and abs(x.mean()) < 0.01 and abs(x.std() - 1) < 0.01


# ------------------------------------------------------------------------------------------------
# the restatement is the likelihood's model
# ------------------------------------------------------------------------------------------------

def _statistics(oracle, meanflux, seed, drop_low_rank=False, num=96):
    model = synthetic.make_model(20)
    zq = synthetic.sample_dr12q_redshifts(num, seed=99)
    rng = np.random.default_rng(5)
    q1 = q2 = 0.0
    n1 = n2 = 0
    for i in range(num):
        sp = synthetic.make_boss_spectrum(3000 + i, float(zq[i]), model, mask_fraction=0.05)
        g = R.msr.grid(oracle, model, sp)
        na = i % 3
        z = g["min_z"] + (g["max_z"] - g["min_z"]) * np.sort(rng.uniform(0.1, 0.9, size=na))
        ln = rng.uniform(20.3, 21.8, size=na)
        d = R.draw(oracle, model, sp, i, seed, z, ln, meanflux=meanflux)
        y = d["y"]
        if drop_low_rank:   # the same draw without M z
            y = y - d["a"] * (d["M"] @ d["latents"])
        a, b, n, k = R.whitened_statistics(y, d["a"], d["mu"], d["M"], d["omega2"], d["nu"])
        q1, q2, n1, n2 = q1 + a, q2 + b, n1 + n, n2 + k
    return q1, n1, q2, n2


@pytest.mark.parametrize("meanflux", [False, True])
def test_restatement_draws_are_draws_from_the_likelihoods_model(oracle, meanflux):
    """Q1 = Sum_q r' K^-1 r ~ chi^2(Sum n_kept) and Q2 = Sum_q g' [(B - I) B]^-1 g ~ chi^2(k Q) over 96
    BOSS-grid templates with 0 .. 2 absorbers; each within 5 sqrt(2 dof) of its dof (fixed seed)."""
    q1, n1, q2, n2 = _statistics(oracle, meanflux, R.MOCK_SEED)
    print(f"meanflux={meanflux}: Q1 = {q1:.1f} for {n1} ({(q1 - n1) / np.sqrt(2 * n1):+.2f} sigma), "
          f"Q2 = {q2:.1f} for {n2} ({(q2 - n2) / np.sqrt(2 * n2):+.2f} sigma)")
    assert n2 == 96 * 20 and n1 > 50000
    assert abs(q1 - n1) <= R.chi2_bound(n1)
    assert abs(q2 - n2) <= R.chi2_bound(n2)


def test_q2_collapses_without_the_low_rank_term(oracle):
    """What makes Q2 a check of the M z term: the same draws with it left out fail Q2 by far."""
    _, _, q2, n2 = _statistics(oracle, False, R.MOCK_SEED, drop_low_rank=True, num=48)
    assert q2 < n2 - R.chi2_bound(n2)


# ------------------------------------------------------------------------------------------------
# draw_truth
# ------------------------------------------------------------------------------------------------

def test_draw_truth():
    model = synthetic.make_model(8)
    templates = synthetic.make_dr12q_mix(60, model)
    dead = templates[5]
    dead["pixel_mask"] = np.ones_like(dead["pixel_mask"])
    sep = 0.05
    off, z, ln = mocks.draw_truth(templates, None, (0.3, 0.4, 0.2, 0.1), (20.3, 22.0), min_z_separation=sep, seed=3)
    assert off.shape == (61,) and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == z.size == ln.size
    counts = np.diff(off)
    assert set(counts.tolist()) == {0, 1, 2, 3} and counts[5] == 0
    assert (ln >= 20.3).all() and (ln <= 22.0).all()
    p = Parameters()
    for i, t in enumerate(templates):
        zi = z[off[i]:off[i + 1]]
        if zi.size:
            lo, hi = mocks.search_range(t, p)
            assert (zi >= lo).all() and (zi <= hi).all()
            assert (np.diff(zi) >= sep).all()           # ascending, separated
    again = mocks.draw_truth(templates, None, (0.3, 0.4, 0.2, 0.1), (20.3, 22.0), min_z_separation=sep, seed=3)
    for a, b in zip((off, z, ln), again):
        np.testing.assert_array_equal(a, b)
    samples = synthetic.make_samples(64)
    _, _, ln2 = mocks.draw_truth(templates, None, (0.0, 1.0), samples=samples, seed=4)
    assert np.isin(ln2, samples["log_nhi_samples"]).all() and ln2.size == 59
    with pytest.raises(ValueError):
        mocks.draw_truth(templates, None, [0.1] * 10)
    # the search range is the sweep's: set_parameters.m:65-73 on the kept pixels in the modelled range
    t = templates[0]
    rest = t["wavelengths"] / (1 + t["z_qso"])
    keep = (rest >= p.min_lambda) & (rest <= p.max_lambda) & (t["pixel_mask"] == 0)
    assert mocks.search_range(t, p) == (p.min_z_dla(t["wavelengths"][keep], t["z_qso"]),
                                        p.max_z_dla(t["wavelengths"][keep], t["z_qso"]))


# ------------------------------------------------------------------------------------------------
# the C boundary
# ------------------------------------------------------------------------------------------------

def _request(off=None, z=None, n=None, **fields):
    keep = []
    rq = _lib.MockRequest()
    if off is not None:
        off, z, n = np.asarray(off, dtype=np.int64), np.asarray(z, dtype=np.float64), np.asarray(n, dtype=np.float64)
        keep += [off, z, n]
        rq.absorber_offsets = off.ctypes.data_as(C.POINTER(C.c_int64))
        rq.absorber_z, rq.absorber_nhi = _lib.ptr(z), _lib.ptr(n)
    for k, v in fields.items():
        setattr(rq, k, v)
    return rq, keep


def test_mock_validate_needs_no_gpu(lib):
    ok, keep = _request([0, 1, 3], [2.1, 2.2, 2.3], [1e20, 1e21, 1e22])
    assert lib.gpdla_mock_validate(C.byref(ok), 2) == 0
    none, _ = _request()
    assert lib.gpdla_mock_validate(C.byref(none), 5) == 0
    assert lib.gpdla_mock_validate(None, 5) == -1
    many, keep = _request([0, 9], np.full(9, 2.5), np.full(9, 1e21))
    assert lib.gpdla_mock_validate(C.byref(many), 1) == -1 and b"at most 8" in lib.gpdla_last_error()
    assert lib.gpdla_last_error() == b"9 absorbers for entry 0: at most 8"
    eight, keep = _request([0, 8], np.full(8, 2.5), np.full(8, 1e21))
    assert lib.gpdla_mock_validate(C.byref(eight), 1) == 0
    dec, keep = _request([0, 2, 1], [2.1, 2.2], [1e20, 1e21])
    assert lib.gpdla_mock_validate(C.byref(dec), 2) == -1 and b"non-decreasing" in lib.gpdla_last_error()
    for bad in (np.nan, 0.0, -1e20, np.inf):
        rq, keep = _request([0, 2], [2.1, 2.2], [1e20, bad])
        assert lib.gpdla_mock_validate(C.byref(rq), 1) == -1 and b"column density" in lib.gpdla_last_error(), bad
    rq, keep = _request([0, 1], [np.nan], [1e20])
    assert lib.gpdla_mock_validate(C.byref(rq), 1) == -1 and b"absorber_z" in lib.gpdla_last_error()
    for name in ("capacity_stored", "capacity_grid"):
        rq, keep = _request(**{name: -1})
        assert lib.gpdla_mock_validate(C.byref(rq), 1) == -1 and b"capacity" in lib.gpdla_last_error()
    # the draw itself refuses a null batch before it looks for a device
    out = _lib.MockSpectra()
    assert lib.gpdla_batch_draw_mocks(None, None, C.byref(ok), C.byref(out)) == -1


C_CONSUMER = r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "gpdla.h"
#define OFF(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("sizeof gpdla_mock_request %zu\n", sizeof(gpdla_mock_request));
  printf("sizeof gpdla_mock_spectra %zu\n", sizeof(gpdla_mock_spectra));
  OFF(gpdla_mock_request, seed); OFF(gpdla_mock_request, absorber_offsets); OFF(gpdla_mock_request, absorber_z);
  OFF(gpdla_mock_request, absorber_nhi); OFF(gpdla_mock_request, meanflux); OFF(gpdla_mock_request, write_resident);
  OFF(gpdla_mock_request, capacity_stored); OFF(gpdla_mock_request, capacity_grid);
  OFF(gpdla_mock_spectra, flux); OFF(gpdla_mock_spectra, grid_offsets); OFF(gpdla_mock_spectra, absorption);
  OFF(gpdla_mock_spectra, continuum); OFF(gpdla_mock_spectra, sigma); OFF(gpdla_mock_spectra, latents);
  OFF(gpdla_mock_spectra, status);
  if (gpdla_abi_version() != GPDLA_ABI_VERSION || GPDLA_ABI_VERSION != 6) return 2;
  gpdla_mock_request rq;
  memset(&rq, 0, sizeof rq);
  if (gpdla_mock_validate(&rq, 3) != GPDLA_OK) return 3;
  rq.capacity_grid = -1;
  if (gpdla_mock_validate(&rq, 3) != GPDLA_ERR_INVALID_ARGUMENT) return 4;
  gpdla_mock_spectra out;
  memset(&out, 0, sizeof out);
  if (gpdla_batch_draw_mocks(NULL, NULL, &rq, &out) != GPDLA_ERR_INVALID_ARGUMENT) return 5;
  return 0;
}
"""


def test_new_structs_match_their_ctypes_mirrors(lib, tmp_path):
    """The additive entry: ABI version still 6, the header compiles as C99, and the layouts the C
    compiler gives the two new structs equal the ctypes mirrors."""
    src, exe = tmp_path / "consumer.c", tmp_path / "consumer"
    src.write_text(C_CONSUMER)
    hip_rt = os.path.dirname(_lib._preload_hip_runtime()._name)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe), _lib.DEFAULT_LIB_PATH, "-L", hip_rt, "-lamdhip64",
                    f"-Wl,-rpath,{os.path.dirname(_lib.DEFAULT_LIB_PATH)}", f"-Wl,-rpath,{hip_rt}"],
                   check=True, capture_output=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    seen = dict(line.rsplit(" ", 1) for line in res.stdout.strip().splitlines())
    mirrors = {"gpdla_mock_request": _lib.MockRequest, "gpdla_mock_spectra": _lib.MockSpectra}
    for cname, mirror in mirrors.items():
        assert int(seen[f"sizeof {cname}"]) == C.sizeof(mirror), cname
        fields = [f for f, _ in mirror._fields_]
        assert sorted(k.split(".")[1] for k in seen if k.startswith(cname + ".")) == sorted(fields)
        for f in fields:
            assert int(seen[f"{cname}.{f}"]) == getattr(mirror, f).offset, (cname, f)
    typed = {n for n, _, _ in _lib.SYMBOLS}
    assert {"gpdla_mock_validate", "gpdla_batch_draw_mocks"} <= typed
    assert lib.gpdla_abi_version() == 6
