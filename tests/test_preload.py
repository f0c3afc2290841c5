"""The preload stage without a GPU: the NumPy restatement of read_spec.m / preload_qsos.m
(tests/preload_restatement.py, the yardstick of tests/test_gpu_preload.py) against one spectrum of 12 pixels
worked out by hand; the command line's argument errors; the preloaded file's round trip; the new
``Parameters`` fields; the C boundary."""
import os

import numpy as np
import pytest

import preload_restatement as R
from gp_dla_detection_amd import _lib, hdf5, io, preload
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

# z = 1; rest wavelengths of the 12 pixels (float32 rounding of loglam moves them by < 1e-4 A)
REST = np.array([950.0, 980.0, 990.0, 1005.0, 1050.0, 1095.0, 1105.0, 1150.0, 1210.0, 1250.0, 1290.0, 1350.0])
HAND = dict(loglam=np.log10(2.0 * REST).astype(np.float32),
            flux=np.array([1, 2, 3, 6, 9, 12, 15, 18, 4, np.nan, 2, 7], dtype=np.float32),
            ivar=np.array([1, 4, 0, 0.25, 0, 2, 1, 0.5, 1, 1, 1, 1], dtype=np.float32),
            and_mask=np.array([0, 1 << 24, 0, 0, 0, 0, 1 << 23, 0, 1 << 24, 0, 0, 0], dtype=np.int32))
# loading range: pixels 3 4 5; pixel 2 (ivar 0) and 6 (BRIGHTSKY) are masked, so the edge pixels are 1 and 7;
# pixel 4 is masked but inside the range and stays; the window holds 8 9 10 = 4, NaN, 2: median (2 + 4) / 2
P = dict(loading_min_lambda=1000.0, loading_max_lambda=1100.0, min_lambda=1002.0, max_lambda=1098.0,
         normalization_min_lambda=1200.0, normalization_max_lambda=1300.0, min_num_pixels=2)


def one(**edit):
    s = {k: v.copy() for k, v in HAND.items()}
    params = dict(P)
    flag = edit.pop("flag", 0)
    for k, v in edit.items():
        if k in params:
            params[k] = v
        else:
            s[k][v[0]] = v[1]
    return R.preload_one(s["flux"], s["loglam"], s["ivar"], s["and_mask"], 1.0, flag, **params)


def test_restatement_on_a_spectrum_worked_out_by_hand():
    wl, fl, nv, pm, norm, flag = one()
    assert flag == 0 and norm == 3.0
    # float32 loglam in [2, 4): half an ulp is 2^-23, i.e. ln(10) 2^-23 = 2.75e-7 relative in the wavelength
    np.testing.assert_allclose(wl, 2.0 * REST[[1, 3, 4, 5, 7]], rtol=2.8e-7)
    np.testing.assert_array_equal(wl, 10.0 ** HAND["loglam"].astype(np.float64)[[1, 3, 4, 5, 7]])
    np.testing.assert_array_equal(fl, np.array([2.0, 6.0, 9.0, 12.0, 18.0]) / 3.0)
    np.testing.assert_array_equal(nv, np.array([0.25, 4.0, np.inf, 0.5, 2.0]) / 9.0)
    assert pm.dtype == np.uint8 and pm.tolist() == [0, 0, 1, 0, 0]
    # an odd count; one value; tied values
    assert one(flux=(9, 5.0))[4] == 4.0 and one(flux=([8, 9], np.nan))[4] == 2.0 and one(flux=([8, 9, 10], 2.5))[4] == 2.5
    # bit 24 and bit 31 of and_mask do not mask; bit 23 does, and so does ivar == 0 (a negative ivar does not)
    assert one(and_mask=(7, -(1 << 31)))[3].tolist() == [0, 0, 1, 0, 0]
    assert one(and_mask=(7, 1 << 23))[0].size == 5 and one(and_mask=(7, 1 << 23))[0][-1] == 10.0 ** np.float64(HAND["loglam"][8])
    neg = one(ivar=(3, -4.0))
    assert neg[3].tolist() == [0, 0, 1, 0, 0] and neg[2][1] == -0.25 / 9.0
    # edge pixels several pixels away, or absent
    far = one(ivar=([0, 1], 0.0), and_mask=([7, 8, 9, 10], 1 << 23), flux=(11, 3.0), normalization_max_lambda=1400.0)
    np.testing.assert_array_equal(far[0], 10.0 ** HAND["loglam"].astype(np.float64)[[3, 4, 5, 11]])
    assert far[4] == 3.0 and far[5] == 0


def test_restatement_flags_and_skips():
    for out, flag in ((one(flag=2), 2), (one(flux=([8, 9, 10], np.nan)), 4), (one(ivar=([8, 9, 10], 0.0)), 4),
                      (one(min_num_pixels=3), 8), (one(flag=1, min_num_pixels=3), 1)):
        assert out[5] == flag and out[4] == 0.0 and all(a.size == 0 for a in out[:4])
    assert one(min_num_pixels=3, ivar=(4, 1.0))[5] == 0              # exactly min_num_pixels unmasked pixels
    assert one(flux=([8, 9, 10], np.nan), min_num_pixels=3)[5] == 4   # preload_qsos.m:36-39 `continue`s before :46
    zero = one(flux=([8, 10], 0.0))                                    # a zero median goes through
    assert zero[5] == 0 and zero[4] == 0.0 and np.isinf(zero[1]).all() and np.isinf(zero[2][[0, 1, 3, 4]]).all()
    negative = one(flux=([8, 10], -2.0))
    assert negative[4] == -2.0 and negative[1][0] == -1.0 and negative[2][0] == 0.25 / 4.0
    nothing = one(loading_min_lambda=1000.0, loading_max_lambda=1003.0, min_lambda=1001.0, max_lambda=1002.0, min_num_pixels=0)
    assert nothing[5] == 0 and nothing[4] == 3.0 and nothing[0].size == 0     # nothing selected: nothing added
    csr = R.preload(dict(offsets=np.array([0, 12, 12, 24]), **{k: np.concatenate([v, v]) for k, v in HAND.items()}),
                    [1.0, 1.0, 1.0], [0, 0, 2], **P)
    assert csr["offsets"].tolist() == [0, 5, 5, 5] and csr["filter_flags"].tolist() == [0, 4, 2]
    assert csr["all_normalizers"].tolist() == [3.0, 0.0, 0.0] and csr["pixel_mask"].dtype == np.uint8


def test_nanmedian():
    assert np.isnan(R.nanmedian([])) and np.isnan(R.nanmedian([np.nan, np.nan]))
    assert R.nanmedian([3.0, np.nan, 1.0]) == 2.0 and R.nanmedian([5.0, 1.0, 3.0]) == 3.0
    assert R.nanmedian([np.inf, 1.0]) == np.inf and np.isnan(R.nanmedian([np.inf, -np.inf]))
    a, b = np.float64(np.float32(1.1)), np.float64(np.float32(3.3e7))
    assert R.nanmedian([b, a]) == (a + b) / 2.0 == a + (b - a) / 2.0      # float32-origin values: both forms agree


def test_parameters():
    p = Parameters()
    assert (p.loading_min_lambda, p.loading_max_lambda, p.normalization_min_lambda, p.normalization_max_lambda,
            p.min_num_pixels) == (910.0, 1217.0, 1310.0, 1325.0, 200)
    assert MultiParameters(max_dlas=2).min_num_pixels == 200
    for bad in (dict(loading_min_lambda=912.0), dict(loading_max_lambda=1215.0), dict(min_lambda=900.0), dict(max_lambda=1300.0),
                dict(min_lambda=1216.0), dict(normalization_min_lambda=1330.0), dict(min_num_pixels=-1)):
        with pytest.raises(ValueError):
            Parameters(**bad)
    Parameters(loading_min_lambda=911.75, loading_max_lambda=1215.75, normalization_min_lambda=1150.0, normalization_max_lambda=1150.0)
    cfg = preload._config(Parameters(min_num_pixels=7))
    assert (cfg.loading_min_lambda, cfg.max_lambda, cfg.min_num_pixels) == (910.0, 1215.75, 7)


def test_file_names():
    assert preload.spec_filename("/data/spectra", 3586, 55181, 16) == "/data/spectra/3586/spec-3586-55181-0016.fits"
    assert preload.spec_filename("d", 10000.0, 57346.0, 1000.0) == "d/10000/spec-10000-57346-1000.fits"


def test_command_line_argument_errors(tmp_path, capsys):
    cat = str(tmp_path / "catalog.mat")
    io.savemat73(cat, dict(z_qsos=np.array([[2.5]]), plates=np.array([[1.0]]), mjds=np.array([[2.0]]), fiber_ids=np.array([[3.0]]),
                           filter_flags=np.array([[0]], dtype=np.uint8)))
    d = str(tmp_path)
    for argv, said in (([], "required"), ([cat, d, "a.mat"], "required"), ([str(tmp_path / "none.mat"), d, "a", "b"], "no catalogue"),
                       ([cat, str(tmp_path / "nowhere"), "a", "b"], "no directory"), ([cat, d, "a", "b", "--block", "0"], "--block"),
                       ([cat, d, "a", cat], "never modified"), ([cat, d, "a", "b", "--device"], "--device")):
        with pytest.raises(SystemExit) as e:
            preload.main(argv)
        assert e.value.code == 2 and said in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="never modified"):
        preload.preload_qsos(cat, d, str(tmp_path / "a.mat"), cat)
    bare = str(tmp_path / "bare.mat")
    io.savemat73(bare, dict(z_qsos=np.array([[2.5]])))
    with pytest.raises(KeyError, match="plates"):
        preload.preload_qsos(bare, d, str(tmp_path / "a.mat"), str(tmp_path / "b.mat"))
    # a quasar that is not flagged needs its file: the path is named, nothing is invented
    with pytest.raises(FileNotFoundError, match="spec-1-2-0003.fits"):
        preload.preload_qsos(cat, d, str(tmp_path / "a.mat"), str(tmp_path / "b.mat"))
    assert not os.path.exists(str(tmp_path / "b.mat"))


def test_preloaded_file_round_trip_with_empty_cells(tmp_path):
    rng = np.random.default_rng(8)
    counts = [5, 0, 1300, 0, 0, 17, 1]
    blocks, at = [], 0
    for lo, hi in ((0, 3), (3, 3), (3, 7)):       # three blocks, one of them without quasars
        c = counts[lo:hi]
        n = int(np.sum(c))
        blocks.append(dict(offsets=np.concatenate([[0], np.cumsum(c)]).astype(np.int64), wavelengths=rng.uniform(3600, 10400, n),
                           flux=rng.standard_normal(n), noise_variance=np.where(rng.uniform(size=n) < 0.1, np.inf, rng.uniform(size=n)),
                           pixel_mask=(rng.uniform(size=n) < 0.2).astype(np.uint8),
                           all_normalizers=np.where(np.array(c) > 0, rng.uniform(1, 9, len(c)), 0.0)))
    path = str(tmp_path / "preloaded_qsos.mat")
    p = Parameters(min_num_pixels=150, normalization_max_lambda=1330.0)
    io.save_preloaded_qsos(path, iter(blocks), p)
    small = io.loadmat73(path, list(io.PRELOADED_SCALARS) + ["all_normalizers"])
    assert {k: float(np.asarray(small[k]).ravel()[0]) for k in io.PRELOADED_SCALARS} == dict(
        loading_min_lambda=910.0, loading_max_lambda=1217.0, normalization_min_lambda=1310.0, normalization_max_lambda=1330.0,
        min_num_pixels=150.0)
    assert all(np.asarray(small[k]).shape == (1, 1) for k in io.PRELOADED_SCALARS) and small["all_normalizers"].shape == (7, 1)
    np.testing.assert_array_equal(small["all_normalizers"].ravel(), np.concatenate([b["all_normalizers"] for b in blocks]))
    with hdf5.File(path) as f:
        assert sorted(k for k in f.keys() if not k.startswith("#")) == sorted(
            list(io.PRELOADED_SCALARS) + list(io.PreloadedReader.KEYS) + ["all_normalizers"])
        for key in io.PreloadedReader.KEYS:
            refs = f[key].read().T.ravel(order="F")
            assert f[key].attrs["MATLAB_class"] == "cell" and f[key].shape == (1, 7)
            for r, c in zip(refs, counts):
                ds = f.dereference(r)
                want = "logical" if key == "all_pixel_mask" else "double"
                assert ds.attrs["MATLAB_class"] == want
                if c:
                    assert ds.shape == (1, c) and "MATLAB_empty" not in ds.attrs       # a c x 1 column, dimensions reversed
                else:
                    assert "MATLAB_empty" in ds.attrs and ds.read().tolist() == [0, 0]     # 0 x 0, as cell(n, 1) leaves it
    with io.PreloadedReader(path) as r:
        assert r.num_quasars == 7 and r.pixel_counts().tolist() == counts
        csr = r.read_csr(np.arange(7), np.zeros(7))
        sub = r.read_csr([5, 1, 0], np.zeros(7))
    for k in ("wavelengths", "flux", "noise_variance", "pixel_mask"):
        np.testing.assert_array_equal(csr[k], np.concatenate([b[k] for b in blocks]))
    np.testing.assert_array_equal(sub["flux"], np.concatenate([blocks[2]["flux"][:17], blocks[0]["flux"][:5]]))
    spectra = io.load_preloaded_qsos(path, np.zeros(7))
    assert [s["flux"].size for s in spectra] == counts
    # one block as a dict; no quasar at all
    io.save_preloaded_qsos(str(tmp_path / "one.mat"), blocks[0])
    with io.PreloadedReader(str(tmp_path / "one.mat")) as r:
        assert r.pixel_counts().tolist() == counts[:3]
    io.save_preloaded_qsos(str(tmp_path / "none.mat"), [])
    assert io.loadmat73(str(tmp_path / "none.mat"), ["all_flux"])["all_flux"] == []


def test_c_boundary():
    h = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "gpdla.h")).read()
    assert "gpdla_preload_spectra" in h and "gpdla_preload_config" in h and "#define GPDLA_ABI_VERSION 6" in h
    assert "gpdla_preload_spectra" in [s[0] for s in _lib.SYMBOLS]
    assert [f[0] for f in _lib.PreloadConfig._fields_] == ["loading_min_lambda", "loading_max_lambda", "normalization_min_lambda",
                                                           "normalization_max_lambda", "min_lambda", "max_lambda", "min_num_pixels"]
    units = [os.path.basename(p) for p in _lib.host_sources()]
    assert "host_preload.hpp" in units
    src = open(os.path.join(_lib.CSRC, "preload_kernels.hpp")).read()
    assert "atomic" not in src.replace("No atomics", "")
