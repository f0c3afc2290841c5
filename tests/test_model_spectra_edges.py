"""CPU side of the edge cases of the model-spectra kernels and k_mock_draw (tests/model_spectra_edge_cases.py):
the case lists hold every tile, chunk and launch-split edge the kernels have, the constants the lists
restate are the ones in the sources, and the restatement ALONE accepts every case -- so that a GPU failure on
one of them (tests/test_gpu_model_spectra_edges.py, tests/test_gpu_mock_edges.py) is the kernel's."""
import os
import re

import numpy as np
import pytest

from gp_dla_detection_amd import _lib, synthetic

import mock_restatement as MR
import model_spectra_edge_cases as E
import model_spectra_restatement as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gp_dla_detection_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------
# the lists
# ------------------------------------------------------------------------------------------------

def _around(*edges):
    return {e + d for e in edges for d in (-1, 0, 1)}


def test_the_map_cases_cover_the_tile_edges():
    assert _around(E.MAP_TILE - 6, E.MAP_TILE, 256, 2 * E.MAP_TILE) <= set(E.MAP_NU)     # 244, 250, 256, 500
    assert {1, 2, 6, 7} <= set(E.MAP_NU)                                                # n_pad = 7 .. 13
    assert set(E.MAP_LINES) == {3, 31}
    counts = {len(E.MAP_ABSORBERS[n]) for n in E.MAP_NU}
    assert {0, 1, 4, E.MAX_ABSORBERS} <= counts and max(counts) == E.MAX_ABSORBERS
    for edge in (E.MAP_TILE, 2 * E.MAP_TILE):
        for p in (edge - 1, edge):
            hosts = [n for n in E.MAP_NU if any(it[0] == "seam" and it[1] == p for it in E.MAP_ABSORBERS[n])]
            assert hosts and all(n > p for n in hosts), (p, hosts)
            assert any(n >= edge + 1 for n in hosts), (p, hosts)                        # the trough reaches over the seam
    for n in E.MAP_NU:
        for it in E.MAP_ABSORBERS[n]:
            assert it[0] != "seam" or (it[2] >= 21.0 and n > it[1])
    assert sum(any(it[0] == "last" for it in E.MAP_ABSORBERS[n]) for n in E.MAP_NU) >= 4
    assert any(it[0] == "last" for it in E.MAP_ABSORBERS[E.MAP_TILE])                     # the last pixel of a full tile
    assert any(it[0] == "last" for it in E.MAP_ABSORBERS[E.MAP_TILE + 1])                 # ... and a tile of one pixel
    _, spectra = E.map_batch()
    masks = [int(np.asarray(sp["pixel_mask"]).sum()) for sp in spectra]
    assert len(spectra) == len(E.MAP_NU) + 1 and masks[-1] == np.asarray(spectra[-1]["pixel_mask"]).size
    assert all(m == 0 for m in masks[:-1:2]) and sum(m > 0 for m in masks[1:-1:2]) >= 4  # unmasked and masked alternate


def test_the_moment_cases_cover_the_tile_chunk_and_wave_edges():
    assert {1, 2} | _around(E.MOM_TILE, 2 * E.MOM_TILE) <= set(E.MOM_NU)
    assert {E.MAP_TILE, 257} <= set(E.MOM_NU) and set(E.MOM_NU_31) == {17, 33} <= set(E.MOM_NU)
    assert {1, 2 * E.MOM_CHUNK + 1} | _around(64, E.MOM_CHUNK) <= set(E.MOM_S)
    assert set(E.RESIDENT_S) == {65, 257} <= set(E.MOM_S) and E.MOM_S_31 in E.MOM_S
    for S in E.MOM_S:
        pos = E.hot_positions(S)
        assert pos == sorted({p for p in (0, 62, 63, 64, 254, 255, 256, S - 1) if p < S})
        kinds = E.row_kinds(S)
        assert kinds[:3] == ["flat", "sweep", "half_nan"] and set(E.NAN_ROWS) <= set(kinds)
        entries = E.moment_entries(S)
        assert {kind for _, kind in entries} == set(kinds)                              # every row kind is used
        assert {q for q, _ in entries} == set(range(len(E.MOM_NU)))                     # ... and every quasar
        # rows of one kind go to different quasars
        for kind in kinds:
            hosts = [q for q, kd in entries if kd == kind]
            assert len(hosts) == len(set(hosts)) == 3, (S, kind, hosts)
    # the last live lane of the last chunk is the first, the 63rd, the 64th lane of a wave, and a chunk's last and first
    assert {(S - 1) % 64 for S in E.MOM_S} >= {0, 62, 63} and {(S - 1) % E.MOM_CHUNK for S in E.MOM_S} >= {0, 255, 254}
    # the hot sample is chosen through the order the kernel walks: the stable sort the context makes
    for S in (64, 257):
        samples = synthetic.make_samples(S)
        order = E.z_order(samples)
        assert np.unique(samples["offset_samples"]).size == S                           # Halton offsets are distinct
        row = E.moment_row(("hot", S - 1), S, samples, None)
        assert row[order[-1]] == 0.0 and (np.delete(row, order[-1]) == -5000.0).all()
        assert samples["offset_samples"][order[-1]] == samples["offset_samples"].max()
    # the NaN rows: nothing above -inf, or +inf
    assert np.isnan(E.moment_row("all_nan", 5, None, None)).all()
    assert (E.moment_row("all_neg_inf", 5, None, None) == -np.inf).all()
    row = E.moment_row("one_pos_inf", 65, None, None)
    assert np.isposinf(row).sum() == 1 and np.isfinite(row).sum() == 64


def test_the_continuum_cases_cover_the_tile_edges_and_the_entry_slots():
    assert {1, 2, 40} <= set(E.CONT_RANKS) and _around(E.CONT_TILE, 2 * E.CONT_TILE) - {255} <= set(E.CONT_NU) and 2 in E.CONT_NU
    T = E.CONT_THREADS
    nb = {k: k * (k + 1) // 2 for k in E.CONT_RANKS}
    assert E.continuum_entries(21) <= T                       # the last rank whose entries fit slot 0
    assert nb[22] <= T < E.continuum_entries(22)              # v straddles slots 0 and 1
    assert nb[23] > T                                         # vech(B) itself straddles
    assert E.continuum_entries(40) > 3 * T                    # every slot is used
    assert set(E.CONT_MEANFLUX_RANKS) == {22, 40}
    for k in E.CONT_RANKS:
        want = [(mf, ab) for mf in ((False, True) if k in (22, 40) else (False,)) for ab in (False, True)]
        assert E.continuum_variants(k) == want
    assert len(E.continuum_lists(True)[0]) == 2 and E.CONT_FRACTIONS == (0.35, 0.8) and E.continuum_lists(False)[0] == ()


def test_the_mock_cases_cover_the_tile_edges():
    stored = [n + 2 * e for n, e, _ in E.MOCK_CASES]
    assert _around(E.MOCK_TILE) <= set(stored) and 2 * E.MOCK_TILE in stored and 1 in stored
    assert {(251, 2), (252, 2), (253, 2), (40, 0), (40, 256), (40, 300), (300, 106), (1, 0)} <= {(n, e) for n, e, _ in E.MOCK_CASES}
    assert set(E.MOCK_RANKS) == {20, 40}
    model = synthetic.make_model(20)
    kinds = set()
    for i, (n, edge, mask) in enumerate(E.MOCK_CASES):
        sp = synthetic.make_spectrum(5400 + 2 * i, n, model, edge_pixels=edge)
        inside = E.in_range(sp)
        assert inside.sum() == n and inside.size == n + 2 * edge
        first, last = np.flatnonzero(inside)[[0, -1]]
        assert first == edge and last == edge + n - 1
        tiles = [inside[t:t + E.MOCK_TILE] for t in range(0, inside.size, E.MOCK_TILE)]
        if not tiles[0].any():
            kinds.add("first tile wholly out of range")
        if not tiles[-1].any():
            kinds.add("last tile wholly out of range")
        if first % E.MOCK_TILE == 0 and first > 0:
            kinds.add("the range starts on a tile edge")
        if len(tiles) == 2 and tiles[0].any() and tiles[1].any() and not tiles[0].all() and not tiles[1].all():
            kinds.add("the in-range edges inside tile 0 and tile 1")
    assert kinds == {"first tile wholly out of range", "last tile wholly out of range", "the range starts on a tile edge",
                     "the in-range edges inside tile 0 and tile 1"}, kinds
    assert [m for _, _, m in E.MOCK_CASES].count("first") == 1
    assert all(m == "5%" for _, _, m in E.MOCK_CASES[1:7:2]) and all(m == "none" for _, _, m in E.MOCK_CASES[0:8:2])


# ------------------------------------------------------------------------------------------------
# the mirrored constants and the launch split
# ------------------------------------------------------------------------------------------------

def test_the_tolerances_are_the_projects_own():
    import test_gpu_mocks
    import test_gpu_model_spectra
    assert E.TOL_MAP == test_gpu_model_spectra.TOL_MAP == test_gpu_mocks.TOL_MAP == 1e-12
    assert E.TOL_MOMENTS == test_gpu_model_spectra.TOL_MOMENTS == 1e-11
    assert R.continuum_tolerance(0.0) == 1e-12 and R.continuum_tolerance(1e-13) == 1e-12
    assert test_gpu_mocks.TOL_DRAW == 1e-11 and test_gpu_mocks.TOL_NORMAL == 1e-13


def test_constants_and_launch_split_mirror_follow_the_source():
    """The tile sizes the case lists are built around, and the arithmetic by which gpdla_batch_model_spectra
    cuts a selection into launches (E.launch_group), are still the library's."""
    kern, multi, mock = _read("spectra_kernels.hpp"), _read("multi_kernels.hpp"), _read("mock_kernels.hpp")
    kern += _read("spectra_moments_body.hpp")  # the body k_spectra_moments includes
    solve = _read("continuum_solve.hpp")  # continuum_null_solve: what k_spectra_continuum accumulates and factorises with
    assert "continuum_null_solve<kContTile>(" in kern[kern.index("void k_spectra_continuum("):]
    assert "const int e = tid + %d * t;" % E.CONT_THREADS in solve[solve.index("void continuum_null_solve("):]
    host = "".join(open(path).read() for path in _lib.host_sources())
    assert os.path.join(CSRC, "host_spectra.hpp") in _lib.host_sources()
    assert re.search(r"constexpr int kMapTile = %d;" % E.MAP_TILE, kern)
    assert re.search(r"constexpr int kSpectraMaxAbsorbers = %d;" % E.MAX_ABSORBERS, kern)
    assert re.search(r"constexpr int kContTile = %d;" % E.CONT_TILE, kern)
    assert re.search(r"constexpr int kProfTile = %d;" % E.MOM_TILE, multi)
    assert "const int e = tid + %d * t;" % E.CONT_THREADS in kern
    assert "for (int tile = 0; tile < npix; tile += %d)" % E.MOCK_TILE in mock
    waves = int(re.search(r"constexpr int kMomWaves = (\d+);", kern).group(1))
    assert waves == E.MOM_WAVES and waves * 64 == E.MOM_CHUNK
    assert "__launch_bounds__(kMomWaves * 64) void k_spectra_moments" in kern
    assert "const int64_t pos = (int64_t)chunk * (kMomWaves * 64) + wave * 64 + lane;" in kern
    m = re.search(r"constexpr size_t kSpectraPartialBytes = \(size_t\)(\d+) << (\d+);", host)
    assert m and int(m.group(1)) << int(m.group(2)) == E.PARTIAL_BYTES == 256 * 2 ** 20
    body = host[host.index("int gpdla_batch_model_spectra("):]
    body = body[:body.index("\n} GPDLA_NO_THROW")]
    for line in ("const int chunks = (int)((S + kMomWaves * 64 - 1) / (kMomWaves * 64));",
                 "const int64_t stride = ((std::max<int64_t>(b->max_pix, 1) + 15) / 16) * 16;",
                 "const size_t per_q = (size_t)chunks * 2 * (size_t)stride;",
                 "const int64_t nsub = std::min<int64_t>(nsel, std::max<int64_t>(1, (int64_t)(kSpectraPartialBytes / (per_q * sizeof(double)))));",
                 "for (int64_t s0 = 0; s0 < nsel; s0 += nsub) {"):
        assert line in body, line
    # groups of 278 quasars at S = 10^4 and 1500 + 2 x 2 stored pixels
    assert E.launch_group(10000, 1504) == 278 == (256 << 20) // (40 * 2 * 1504 * 8)
    assert E.launch_group(1, 1) == (256 << 20) // (2 * 16 * 8) and E.launch_group(257, 17) == (256 << 20) // (2 * 2 * 32 * 8)
    assert E.launch_group(10 ** 6, 10 ** 5) == 1
    # the split case: three launches, the last partly filled
    _, spectra = E.split_batch()
    stored = max(np.asarray(sp["wavelengths"]).size for sp in spectra)
    nsub = E.launch_group(E.SPLIT_S, stored)
    assert stored == E.SPLIT_NU + 4 and nsub == 278
    assert E.SPLIT_ENTRIES > 2 * nsub and E.SPLIT_ENTRIES % nsub != 0 and E.SPLIT_ENTRIES <= 3 * nsub
    sel = E.split_selection()
    assert sel.size == E.SPLIT_ENTRIES and set(sel) == set(range(E.SPLIT_QUASARS)) and (np.diff(sel) != 0).mean() > 0.8
    assert sel.tolist() == E.split_selection().tolist()                                 # a fixed order
    checked = E.split_checked_entries(E.SPLIT_ENTRIES, nsub)
    assert {nsub - 2, nsub - 1, nsub, nsub + 1, 2 * nsub - 2, 2 * nsub - 1, 2 * nsub, 2 * nsub + 1} <= set(checked)
    assert len(checked) <= 56
    nan_row = E.split_nan_entries(E.SPLIT_ENTRIES)
    # an entry and the one a group before it never both hold the all-NaN row: a flag read at the index within
    # the launch instead of the index within the selection shows (the GPU test looks at the NaN pattern of EVERY entry)
    assert nan_row[nsub:].any() and nan_row[2 * nsub:].any() and not (nan_row[nsub:] & nan_row[:-nsub]).any()
    S = 64
    samples = synthetic.make_samples(S)
    rows = E.split_rows(sel, np.arange(E.SPLIT_QUASARS * S, dtype=np.float64).reshape(E.SPLIT_QUASARS, S), samples)
    assert np.array_equal(np.isnan(rows).all(axis=1), nan_row)
    same = [np.array_equal(rows[j], rows[j + 1], equal_nan=True) and sel[j] == sel[j + 1] for j in range(sel.size - 1)]
    assert not any(same)                                                                # neighbouring entries differ
    first = [int(np.flatnonzero(sel == q)[0]) for q in range(E.SPLIT_QUASARS)]
    assert all(np.array_equal(rows[j], np.arange(q * S, (q + 1) * S)) for q, j in enumerate(first) if not nan_row[j])


# ------------------------------------------------------------------------------------------------
# the restatement accepts every case
# ------------------------------------------------------------------------------------------------

def test_restatement_accepts_the_map_cases(oracle):
    model, spectra = E.map_batch()
    grids = [R.grid(oracle, model, sp) for sp in spectra]            # (R.grid asserts rc 0 and the oracle's own n_u)
    assert [g["n_u"] for g in grids[:-1]] == list(E.MAP_NU) and "pad" not in grids[-1]
    assert grids[0]["min_z"] > grids[0]["max_z"]                      # n_u = 1: an inverted search range, in the oracle too
    lists = E.map_lists()
    off, zs, lns = E.resolve_absorbers(lists, grids)
    assert np.diff(off).tolist() == [len(items) for items in lists] and np.isfinite(zs).all()
    seams = 0
    for num_lines in E.MAP_LINES:
        for i, g in enumerate(grids[:-1]):
            want = R.map_absorption(oracle, g["pad"], zs[off[i]:off[i + 1]], lns[off[i]:off[i + 1]], num_lines)
            assert want.size == g["n_u"] and np.isfinite(want).all() and (want <= 1.0 + 1e-15).all() and (want >= 0).all()
            if not lists[i]:
                assert (want == 1.0).all()
            for item, pixels in E.seam_pixels(lists[i], g["n_u"]):
                assert pixels and (want[pixels] < 0.5).all(), (E.MAP_NU[i], item, want[pixels])
                seams += 1
            if any(it[0] == "last" for it in lists[i]):
                assert want[-1] < 0.5
    assert seams == 2 * 10


def test_restatement_accepts_the_moment_cases(oracle):
    """Every (S, quasar, row kind) of the GPU test with the oracle's sweep standing in for the GPU's: finite wanted
    moments wherever the row has weight, NaN where it has none, one-hot rows giving that sample's own profile."""
    model, spectra = E.moments_batch()
    grids = [R.grid(oracle, model, sp) for sp in spectra]
    assert [g["n_u"] for g in grids] == list(E.MOM_NU) and all("pad" in g for g in grids)
    assert grids[0]["min_z"] > grids[0]["max_z"]
    for S in E.MOM_S:
        samples = synthetic.make_samples(S)
        order = E.z_order(samples)
        sweep = {}
        for q, kind in E.moment_entries(S):
            sp, g = spectra[q], grids[q]
            if q not in sweep:
                r = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"], sp["flux"],
                                            sp["noise_variance"], sp["pixel_mask"], sp["z_qso"])
                assert r["rc"] == 0 and np.isfinite(r["sample_log_likelihoods_dla"]).all(), (S, q)
                sweep[q] = r["sample_log_likelihoods_dla"]
            row = E.moment_row(kind, S, samples, sweep[q])
            for key in ("nhi_samples", "lls_nhi_samples"):
                mean, var = E.want_moments(oracle, g, samples, row, key)
                assert mean.shape == var.shape == (g["n_u"],)
                if E.expects_nan(kind, row):
                    assert np.isnan(mean).all() and np.isnan(var).all(), (S, q, kind)
                    continue
                assert np.isfinite(mean).all() and np.isfinite(var).all() and (var >= -1e-18).all(), (S, q, kind)
                if kind[0] == "hot":
                    i = order[kind[1]]
                    z = g["min_z"] + (g["max_z"] - g["min_z"]) * samples["offset_samples"][i]
                    assert np.array_equal(mean, oracle.voigt(g["pad"], z, samples[key][i], 3)) and (np.abs(var) < E.ONE_HOT_VAR).all()
    # a sample dropped from a flat row shows far above the tolerance: the last one in z order at S = 513, n_u = 257
    S, g = 513, grids[-1]
    samples = synthetic.make_samples(S)
    flat = E.moment_row("flat", S, samples, None)
    dropped = flat.copy()
    dropped[E.z_order(samples)[-1]] = np.nan
    a = R.moments(oracle, g, samples["offset_samples"], samples["nhi_samples"], flat, 3)[0]
    b = R.moments(oracle, g, samples["offset_samples"], samples["nhi_samples"], dropped, 3)[0]
    print(f"a sample dropped from a flat row at S = {S}, n_u = {g['n_u']}: the mean moves by {np.abs(a - b).max():.2e}")
    assert np.abs(a - b).max() > 1e4 * E.TOL_MOMENTS


def test_restatement_accepts_the_31_line_moment_case(oracle):
    model, spectra = E.moments_batch(E.MOM_NU_31)
    samples = synthetic.make_samples(E.MOM_S_31)
    for sp, n in zip(spectra, E.MOM_NU_31):
        g = R.grid(oracle, model, sp)
        mean, var = R.moments(oracle, g, samples["offset_samples"], samples["nhi_samples"], E.moment_row("flat", E.MOM_S_31, samples, None), 31)
        assert g["n_u"] == n and np.isfinite(mean).all() and np.isfinite(var).all()


def test_dense_and_woodbury_continuum_agree_on_the_edge_cases(oracle):
    worst = 0.0
    for k in E.CONT_RANKS:
        c = E.continuum_wanted(oracle, k)
        assert [g["n_u"] for g in c["grids"]] == list(E.CONT_NU)
        kept = [int(g["kept"].sum()) for g in c["grids"]]
        assert kept[0] == 2 and (k <= 2 or kept[0] < k)                       # fewer kept pixels than k
        assert all(kept[i] < n for i, n in enumerate(E.CONT_NU) if n >= 127)  # a masked pixel inside each grid
        assert set(c["variants"]) == set(E.continuum_variants(k))
        for (mf, ab), v in c["variants"].items():
            assert np.diff(v["absorbers"][0]).tolist() == [2 if ab else 0] * len(E.CONT_NU)
            for g, d, w in zip(c["grids"], v["dense"], v["woodbury"]):
                assert d[0].size == d[1].size == g["n_u"] and np.isfinite(d[0]).all() and np.isfinite(d[1]).all()
                dis = max(float(np.abs(d[0] - w[0]).max()), float(np.abs(d[1] - w[1]).max()))
                worst = max(worst, dis)
        print(f"k = {k}: dense vs Woodbury so far {worst:.2e}")
    assert worst == E.continuum_disagreement(oracle)
    print(f"worst dense-vs-Woodbury disagreement on the edge cases: {worst:.2e} -> GPU tolerance {R.continuum_tolerance(worst):.2e}")
    assert worst < 1e-13


@pytest.mark.parametrize("k", E.MOCK_RANKS)
def test_restatement_accepts_the_mock_cases(oracle, k):
    c = E.mock_case(oracle, k)
    off = c["truth"][0]
    assert np.diff(off).tolist() == [1, 1, 0, 0, 1, 1, 0, 0, 1]
    for i, (sp, (n, edge, mask)) in enumerate(zip(c["templates"], E.MOCK_CASES)):
        z, ln = MR.absorbers_of(c["truth"], i)
        want = MR.draw(oracle, c["model"], sp, i, MR.MOCK_SEED, z, ln)
        inside, masked = E.in_range(sp), np.asarray(sp["pixel_mask"]) != 0
        assert want["status"] == 0 and want["grid"]["n_u"] == n and inside.size == n + 2 * edge
        assert np.isfinite(want["latents"]).all() and want["latents"].size == k
        assert np.isfinite(want["flux"][inside & ~masked]).all() and np.isnan(want["flux"][inside & masked]).all()
        assert np.array_equal(want["flux"][~inside].view(np.uint64), np.asarray(sp["flux"])[~inside].view(np.uint64))
        assert np.isfinite(want["absorption"]).all()
        for name in ("continuum", "sigma"):
            assert np.array_equal(np.isnan(want[name]), masked[inside])
        if mask == "first":
            assert masked[inside][0] and masked.sum() == 1
        if mask == "5%":
            assert masked[inside].any() or n <= 40
        if len(z):
            assert want["absorption"].min() < 0.5
