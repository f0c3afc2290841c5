"""CPU-side checks of the model-spectra subsystem: the restatement the GPU tests
compare against is itself held to reference-produced numbers, the host helper that picks the MAP
absorbers, request validation without a device, the file round trip, and the dense-versus-Woodbury
agreement of the restatement's continuum that sets the GPU test's tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, io, synthetic

import model_spectra_restatement as R


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def test_restatement_reproduces_the_references_this_mu(oracle, golden):
    """tests/golden/model_mean.npz holds what the reference's own Voigt_absorption and
    QSOLoader.total_scale_factor computed (tests/golden/make_model_mean.py): 0-4 absorbers, 1/3/31 Voigt
    lines, suppressed and not."""
    g = golden("model_mean.npz")
    assert int(g["num_cases"]) >= 6
    counts, lines = set(), set()
    for i in range(int(g["num_cases"])):
        got = R.model_mean(oracle, g["rest_wavelengths"], g["mu"], float(g[f"z_qso_{i}"]), g[f"z_dlas_{i}"],
                           g[f"log_nhis_{i}"], bool(g[f"suppressed_{i}"]), int(g[f"num_voigt_lines_{i}"]),
                           int(g[f"num_forest_lines_{i}"]), float(g["tau"]), float(g["beta"]))
        worst = float(np.abs(got - g[f"this_mu_{i}"]).max())
        print(f"case {i}: {g[f'z_dlas_{i}'].size} absorbers, {int(g[f'num_voigt_lines_{i}'])} lines: {worst:.2e}")
        assert worst < 1e-13, (i, worst)
        counts.add(int(g[f"z_dlas_{i}"].size))
        lines.add(int(g[f"num_voigt_lines_{i}"]))
    assert counts == {0, 1, 2, 3, 4} and lines == {1, 3, 31}


# ------------------------------------------------------------------------------------------------
# map_absorbers
# ------------------------------------------------------------------------------------------------

def _multi_results(rows, md=4):
    """Hand-built multi-DLA results: model_posteriors rows as given, MAP[q, model, slot] = q + model/10 +
    slot/100 (z) and 20 + the same (log N_HI), NaN above the diagonal as the driver leaves them."""
    mp = np.array(rows, dtype=np.float64)
    nq = mp.shape[0]
    z = np.full((nq, md, md), np.nan)
    for q in range(nq):
        for m in range(md):
            for s in range(m + 1):
                z[q, m, s] = q + m / 10 + s / 100
    return dict(model_posteriors=mp, MAP_z_dlas=z, MAP_log_nhis=20 + z)


def test_map_absorbers_multi_each_model_winning():
    md = 4
    rows = [np.eye(2 + md)[w] * 0.8 + 0.2 / (2 + md) for w in range(2 + md)]   # winner: null, sub-DLA, DLA(1..4)
    res = _multi_results(rows, md)
    off, z, n = gp.map_absorbers(res, sub_dla=True)
    assert off.tolist() == [0, 0, 0, 1, 3, 6, 10]
    for q, nth in zip(range(2, 6), range(md)):   # qso_loader.py:285-301: slots 0 .. nth of model nth
        np.testing.assert_array_equal(z[off[q]:off[q + 1]], res["MAP_z_dlas"][q, nth, :nth + 1])
        np.testing.assert_array_equal(n[off[q]:off[q + 1]], res["MAP_log_nhis"][q, nth, :nth + 1])


def test_map_absorbers_sub_dla_offset_off():
    """Posteriors without a sub-DLA column (sub_dla=False, qso_loader.py:1695): column 1 is DLA(1)."""
    md = 3
    rows = [np.eye(1 + md)[w] * 0.7 + 0.3 / (1 + md) for w in range(1 + md)]
    res = _multi_results(rows, md)
    off, z, _ = gp.map_absorbers(res, sub_dla=False)
    assert off.tolist() == [0, 0, 1, 3, 6]
    np.testing.assert_array_equal(z[off[3]:off[4]], res["MAP_z_dlas"][3, 2, :3])
    # the same rows read WITH the offset: column 1 is the sub-DLA model and has no absorbers
    off2, _, _ = gp.map_absorbers(res, sub_dla=True)
    assert off2.tolist() == [0, 0, 0, 1, 3]


def test_map_absorbers_nan_rows():
    res = _multi_results([[np.nan] * 6, [0.1, np.nan, 0.6, 0.3, np.nan, np.nan], [0.05, 0.05, 0.1, 0.8, 0.0, 0.0]])
    res["MAP_z_dlas"][2, 1, 1] = np.nan          # a NaN slot of the chosen model is dropped
    off, z, n = gp.map_absorbers(res)
    assert off.tolist() == [0, 0, 1, 2]
    assert z[0] == res["MAP_z_dlas"][1, 0, 0] and z[1] == res["MAP_z_dlas"][2, 1, 0]
    assert np.isfinite(z).all() and np.isfinite(n).all()


def test_map_absorbers_single_dla_form():
    res = dict(model_posteriors=np.array([[0.9, 0.1], [0.2, 0.8], [np.nan, np.nan], [0.5, 0.5], [0.3, 0.7]]),
               MAP_z_dlas=np.array([2.1, 2.2, 2.3, 2.4, np.nan]), MAP_log_nhis=np.array([20.1, 20.2, 20.3, 20.4, 20.5]))
    off, z, n = gp.map_absorbers(res)
    assert off.tolist() == [0, 0, 1, 1, 1, 1]    # a tie goes to the null model (argmax takes the first)
    assert z.tolist() == [2.2] and n.tolist() == [20.2]


# ------------------------------------------------------------------------------------------------
# request validation: before any device call
# ------------------------------------------------------------------------------------------------

def _request(nsel=2, **kw):
    rq = _lib.ModelSpectraRequest()
    rq.num_selected = nsel
    rq.products = _lib.SPECTRA_MAP
    keep = []
    for k, v in kw.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            ct = C.c_int64 if v.dtype == np.int64 else C.c_double
            v = v.ctypes.data_as(C.POINTER(ct))
        setattr(rq, k, v)
    return rq, keep


def test_invalid_requests_are_rejected_without_a_device(lib):
    f = lib.gpdla_model_spectra_validate
    ok, _ = _request()
    assert f(C.byref(ok), 3, 10, 0) == 0
    z, n = np.full(9, 2.5), np.full(9, 1e20)
    bad, keep = _request(absorber_offsets=np.array([0, 9, 9], dtype=np.int64), absorber_z=z, absorber_nhi=n)
    assert f(C.byref(bad), 3, 10, 0) == _lib.ERR_INVALID_ARGUMENT and b"at most 8" in lib.gpdla_last_error()
    assert lib.gpdla_last_error() == b"9 absorbers for entry 0: at most 8"
    eight, keep = _request(absorber_offsets=np.array([0, 8, 9], dtype=np.int64), absorber_z=z, absorber_nhi=n)
    assert f(C.byref(eight), 3, 10, 0) == 0
    bad, keep = _request(absorber_offsets=np.array([0, 3, 2], dtype=np.int64), absorber_z=z, absorber_nhi=n)
    assert f(C.byref(bad), 3, 10, 0) == -1 and b"non-decreasing" in lib.gpdla_last_error()
    bad, keep = _request(selection=np.array([0, 3], dtype=np.int64))
    assert f(C.byref(bad), 3, 10, 0) == -1 and b"selection[1] = 3" in lib.gpdla_last_error()
    # (the two selection messages are worded in one place, csrc/host_consumers.hpp, for every entry that takes one)
    assert lib.gpdla_last_error() == b"selection[1] = 3 outside the batch of 3 quasars"
    bad, keep = _request(selection=np.array([-1, 0], dtype=np.int64))
    assert f(C.byref(bad), 3, 10, 0) == -1 and lib.gpdla_last_error() == b"selection[0] = -1 outside the batch of 3 quasars"
    bad, _ = _request(nsel=4)                                   # no selection: the first num_selected quasars
    assert f(C.byref(bad), 3, 10, 0) == -1 and lib.gpdla_last_error() == b"num_selected = 4 outside [0, 3]"
    bad, _ = _request(nsel=-1)
    assert f(C.byref(bad), 3, 10, 0) == -1 and lib.gpdla_last_error() == b"num_selected = -1 outside [0, 3]"
    bad, _ = _request(products=_lib.SPECTRA_MOMENTS)            # no weights source
    assert f(C.byref(bad), 3, 10, 0) == -1 and b"weights source" in lib.gpdla_last_error()
    bad, _ = _request(products=_lib.SPECTRA_MOMENTS, weights_source=_lib.SPECTRA_WEIGHTS_HOST)
    assert f(C.byref(bad), 3, 10, 0) == -1 and b"sample_log_likelihoods is null" in lib.gpdla_last_error()
    lls, _ = _request(products=_lib.SPECTRA_MOMENTS, weights_source=_lib.SPECTRA_WEIGHTS_RESIDENT, sub_dla=1)
    assert f(C.byref(lls), 3, 10, 0) == -1 and b"lls_nhi_samples" in lib.gpdla_last_error()
    assert f(C.byref(lls), 3, 10, 1) == 0
    bad, _ = _request(products=0)
    assert f(C.byref(bad), 3, 10, 0) == -1
    bad, _ = _request(products=8)
    assert f(C.byref(bad), 3, 10, 0) == -1
    assert f(None, 3, 10, 0) == -1
    # the batch entry itself refuses null handles before it touches anything
    out = _lib.ModelSpectra()
    assert lib.gpdla_batch_model_spectra(None, None, C.byref(ok), C.byref(out)) == -1
    assert lib.gpdla_batch_unmasked_counts(None, None, None) == -1


def test_the_consumers_header_is_a_host_source():
    """csrc/host_consumers.hpp is found by the rebuild check and the source-reading tests, between the sweeps
    it builds on and the first entry that uses it."""
    units = [os.path.basename(p) for p in _lib.host_sources()]
    assert "host_consumers.hpp" in units
    assert units.index("host_multi.hpp") < units.index("host_consumers.hpp") < units.index("host_spectra.hpp")


def test_model_mean_validates_before_the_device(lib):
    model = synthetic.make_model(4)
    nine = (np.array([0, 9]), np.full(9, 2.5), np.full(9, 20.5))
    with pytest.raises(_lib.GpdlaError) as e:
        gp.dla_model_mean(model, [3.0], nine)
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT and "at most 8" in str(e.value)
    for kw in (dict(num_voigt_lines=0), dict(num_voigt_lines=32), dict(num_forest_lines=0), dict(num_forest_lines=40)):
        with pytest.raises(_lib.GpdlaError) as e:
            gp.dla_model_mean(model, [3.0], None, **kw)
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(_lib.GpdlaError):
        gp.dla_model_mean(model, [3.0, 3.1], (np.array([0, 1]), np.array([2.5]), np.array([20.5])))
    assert gp.dla_model_mean(model, np.zeros(0)).shape == (0, model["mu"].size)   # nothing to do: no device needed


# ------------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------------

def test_file_round_trip_ragged_cells(tmp_path):
    rng = np.random.default_rng(4)
    counts = np.array([5, 0, 1249, 3])                      # a quasar with n_u = 0 among them
    off = np.concatenate([[0], np.cumsum(counts)])
    sp = dict(selection=np.array([7, 9, 20, 21]), offsets=off, status=np.array([0, 1, 0, 4], dtype=np.int32),
              absorber_offsets=np.array([0, 2, 2, 3, 3]), absorber_z_dlas=np.array([2.5, 2.7, 3.1]),
              absorber_log_nhis=np.array([20.5, 21.0, 22.2]))
    for name in io.MODEL_SPECTRA_CELLS:
        sp[name] = rng.normal(size=off[-1])
    sp["var_absorption"][:5] = np.nan
    path = str(tmp_path / "ms.mat")
    io.save_model_spectra(path, sp, processed_file="processed_qsos_x.mat", multi_dla=np.float64(1))
    back = io.load_model_spectra(path)
    np.testing.assert_array_equal(back["selection"], sp["selection"])
    np.testing.assert_array_equal(back["offsets"], off)
    np.testing.assert_array_equal(back["status"], sp["status"])
    assert back["processed_file"] == "processed_qsos_x.mat"
    for name in io.MODEL_SPECTRA_CELLS:
        assert [c.size for c in back[name]] == counts.tolist()
        for i, cell in enumerate(back[name]):
            np.testing.assert_array_equal(cell, sp[name][off[i]:off[i + 1]])
    assert [c.tolist() for c in back["map_z_dlas"]] == [[2.5, 2.7], [], [3.1], []]
    assert [c.tolist() for c in back["map_log_nhis"]] == [[20.5, 21.0], [], [22.2], []]
    # MATLAB's view of it: N x 1 cells of column vectors
    raw = io.loadmat73(path, ["mean_absorption", "quasar_ind"])
    assert len(raw["mean_absorption"]) == 4 and raw["mean_absorption"][2].shape == (1249, 1)
    assert raw["quasar_ind"].reshape(-1).tolist() == [8, 10, 21, 22]   # 1-based


def test_file_round_trip_empty_selection(tmp_path):
    sp = dict(selection=np.zeros(0, dtype=np.int64), offsets=np.zeros(1, dtype=np.int64), status=np.zeros(0, dtype=np.int32))
    for name in io.MODEL_SPECTRA_CELLS:
        sp[name] = np.zeros(0)
    path = str(tmp_path / "empty.mat")
    io.save_model_spectra(path, sp)
    back = io.load_model_spectra(path)
    assert back["selection"].size == 0 and back["offsets"].tolist() == [0]
    for name in io.MODEL_SPECTRA_CELLS:
        assert back[name] == []


# ------------------------------------------------------------------------------------------------
# the continuum restatement against itself: sets the GPU test's tolerance
# ------------------------------------------------------------------------------------------------

def test_dense_and_woodbury_continuum_agree(oracle):
    """The restatement's dense form (K = A (M M' + Omega) A + N formed and solved) against its Woodbury form
    on the quasars the GPU test uses.  The worst disagreement is printed: the GPU test recomputes it on
    the same cases and takes 10 x it, floored at 1e-12 and capped at 1e-8, as its tolerance."""
    worst = 0.0
    for case in R.continuum_cases(oracle):
        dense = R.continuum(oracle, case["model"], case["grid"], case["absorption"], case["meanflux"], "dense")
        wood = R.continuum(oracle, case["model"], case["grid"], case["absorption"], case["meanflux"], "woodbury")
        d = max(float(np.abs(dense[0] - wood[0]).max()), float(np.abs(dense[1] - wood[1]).max()))
        print(f"{case['name']}: n_kept {int(case['grid']['kept'].sum())} of {case['grid']['n_u']}, dense vs Woodbury {d:.2e}")
        worst = max(worst, d)
        assert np.isfinite(dense[0]).all() and dense[0].size == case["grid"]["n_u"]
    print(f"worst dense-vs-Woodbury disagreement: {worst:.2e} -> GPU tolerance {R.continuum_tolerance(worst):.2e}")
    assert worst < 1e-9, worst     # else the dense reference itself could not carry a 1e-8 comparison
