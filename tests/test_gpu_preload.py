"""k_preload against the NumPy restatement of read_spec.m and preload_qsos.m (tests/preload_restatement.py,
which tests/test_preload.py holds to a spectrum worked out by hand), on hand-shaped spectra; and the
whole stage, spec files -> python -m gp_dla_detection_amd.preload -> PreloadedReader.

Required agreement: filter_flags, kept counts and offsets, pixel_mask, all_normalizers, flux and
noise_variance (inf and NaN positions included) identical -- every operation on them is one correctly
rounded IEEE step on inputs both sides share; wavelengths to 1e-13 relative (DESIGN.md 4.10's tolerance
for the rest grid: the device pow and libm's need not round alike).  The inputs are held, on the CPU and
before any GPU call, to: no pixel's rest wavelength within 1e-12 relative of any of the six thresholds,
so that a 1e-13 difference cannot flip a selection.
"""
import numpy as np
import pytest

import preload_restatement as R
from gp_dla_detection_amd import io, preload, snrs, synthetic
from gp_dla_detection_amd.parameters import Parameters

pytestmark = pytest.mark.gpu

WAVELENGTH_RTOL = 1e-13
THRESHOLD_MARGIN = 1e-12
BIT23, BIT24, BIT31 = 1 << 23, 1 << 24, -(1 << 31)

GROUPS = dict(
    default={},
    small=dict(min_num_pixels=4),
    zero=dict(min_num_pixels=0),
    wide=dict(min_num_pixels=4, normalization_min_lambda=1230.0, normalization_max_lambda=1400.0),   # > one LDS tile fits
    inner=dict(min_num_pixels=4, normalization_min_lambda=1150.0, normalization_max_lambda=1200.0),  # window inside the loading range
)


def grid(n, z, lo, hi):
    return np.linspace(np.log10(lo * (1 + z)), np.log10(hi * (1 + z)), n).astype(np.float32)


def rest_of(loglam, z):
    return 10.0 ** loglam.astype(np.float64) / (1 + z)


def build_cases():
    """{group: [(name, spectrum dict, z, input flag)]}"""
    rng = np.random.default_rng(20251018)
    groups = {g: [] for g in GROUPS}

    def add(group, name, loglam, z=2.5, flag=0, edit=None):
        n = loglam.size
        s = dict(loglam=loglam.astype(np.float32), flux=rng.normal(5.0, 2.0, n).astype(np.float32),
                 ivar=rng.uniform(0.5, 4.0, n).astype(np.float32), and_mask=np.zeros(n, dtype=np.int32))
        if edit is not None:
            edit(s, rest_of(s["loglam"], z))
        groups[group].append((name, s, z, flag))

    def window(s, rest, lo=1310.0, hi=1325.0):
        return np.flatnonzero((rest >= lo) & (rest <= hi))

    # lengths
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 4650):
        add("small", f"{n} pixels", grid(n, 2.5, 880.0, 1400.0))
    add("default", "4650 pixels, default thresholds", grid(4650, 2.2, 880.0, 1400.0), 2.2)
    # the normalisation window: 0, 1, 2, 3 values
    base = grid(300, 2.5, 880.0, 1300.0)
    for k in range(4):
        extra = np.log10(np.array([1312.0, 1316.0, 1320.0])[:k] * 3.5).astype(np.float32)
        add("small", f"{k} window values", np.concatenate([base, extra]))
    # ... 2048, 2049 and 4097 values under the widened window (one tile, two tiles, three tiles)
    for k in (2048, 2049, 4097):
        add("wide", f"{k} window values", np.concatenate([grid(400, 3.0, 880.0, 1225.0), grid(k, 3.0, 1235.0, 1395.0)]), 3.0)

    def ties(s, rest):
        s["flux"][window(s, rest, 1230.0, 1400.0)[::3]] = np.float32(2.5)
        s["flux"][window(s, rest, 1230.0, 1400.0)[1::3]] = np.float32(7.0)
    add("wide", "three tiles, ties across them", np.concatenate([grid(400, 3.0, 880.0, 1225.0), grid(4500, 3.0, 1235.0, 1395.0)]), 3.0, edit=ties)
    long = grid(800, 2.5, 880.0, 1400.0)

    def tied(values):
        def f(s, rest):
            w = window(s, rest)
            s["flux"][w] = np.resize(np.asarray(values, dtype=np.float32), w.size)
        return f
    add("small", "tied values", long, edit=tied([3, 3, 3, 7, 7, 7, 7, 1, 1, 3]))
    add("small", "all window values equal", long, edit=tied([4.25]))
    add("small", "zero median", long, edit=tied([0.0]))
    add("small", "negative median", long, edit=tied([-3.5, -1.0, -2.0]))
    add("small", "float32 extremes in the window", long, edit=tied([3.4e38, 3.4e38, 1e-45, -1e-45, 3.4e38, 3.4e38]))
    add("small", "negative zero median", long, edit=tied([-0.0]))
    add("small", "infinite flux in the window", long, edit=tied([np.inf, 1.0, 2.0, -np.inf, 3.0]))

    def nan_in_window(s, rest):
        s["flux"][window(s, rest)[2]] = np.nan
    add("small", "a NaN flux inside the window", long, edit=nan_in_window)

    def all_nan(s, rest):
        s["flux"][window(s, rest)] = np.nan
    add("small", "only NaN flux inside the window", long, edit=all_nan)

    def masked_window(how):
        def f(s, rest):
            if how == "ivar":
                s["ivar"][window(s, rest)] = 0.0
            else:
                s["and_mask"][window(s, rest)] = BIT23
        return f
    add("small", "window entirely masked (ivar)", long, edit=masked_window("ivar"))
    add("small", "window entirely masked (and_mask)", long, edit=masked_window("and_mask"))

    # the pixel-count flag, at the default min_num_pixels = 200
    def leave_unmasked(count):
        def f(s, rest):
            inside = np.flatnonzero((rest >= 911.75) & (rest <= 1215.75))
            assert inside.size > 260
            s["ivar"][inside[count:]] = 0.0
        return f
    add("default", "min_num_pixels - 1 unmasked pixels", grid(700, 2.5, 880.0, 1400.0), edit=leave_unmasked(199))
    add("default", "exactly min_num_pixels unmasked pixels", grid(700, 2.5, 880.0, 1400.0), edit=leave_unmasked(200))

    # the edge pixels
    def edges_three_away(s, rest):
        sel = np.flatnonzero((rest >= 910.0) & (rest <= 1217.0))
        s["and_mask"][sel[0] - 3:sel[0]] = BIT23
        s["ivar"][sel[-1] + 1:sel[-1] + 4] = 0.0
    add("small", "edge pixels three masked pixels away", long, edit=edges_three_away)
    add("small", "no edge pixel below", grid(500, 2.5, 950.0, 1400.0))
    add("inner", "no edge pixel above", grid(500, 2.5, 880.0, 1210.0))
    add("inner", "no edge pixel on either side", grid(500, 2.5, 950.0, 1210.0))

    def all_masked_below(s, rest):
        s["ivar"][rest < 910.0] = 0.0
    add("small", "every pixel below is masked", long, edit=all_masked_below)

    def all_masked_above(s, rest):
        s["and_mask"][rest > 1217.0] = BIT23
    add("inner", "every pixel above is masked", grid(600, 2.5, 880.0, 1400.0), edit=all_masked_above)

    # ivar and and_mask
    def scatter(key, value):
        def f(s, rest):
            s[key][::7] = value
        return f
    add("small", "ivar 0", long, edit=scatter("ivar", 0.0))
    add("small", "ivar negative", long, edit=scatter("ivar", -2.0))
    add("small", "and_mask with only bit 23", long, edit=scatter("and_mask", BIT23))
    add("small", "and_mask with only bit 24", long, edit=scatter("and_mask", BIT24))
    add("small", "and_mask with only bit 31", long, edit=scatter("and_mask", BIT31))
    add("small", "and_mask with every bit but 23", long, edit=scatter("and_mask", ~BIT23))
    add("small", "and_mask with every bit", long, edit=scatter("and_mask", -1))
    # other shapes
    add("small", "live, before a flagged one", grid(300, 2.3, 880.0, 1400.0), 2.3)
    add("small", "flagged on input", grid(300, 2.5, 880.0, 1400.0), flag=2)
    add("small", "live, after a flagged one", grid(300, 3.1, 880.0, 1400.0), 3.1)
    add("small", "wavelengths in no order", rng.permutation(grid(700, 2.5, 880.0, 1400.0)))
    add("small", "all pixels masked", long, edit=lambda s, rest: s["ivar"].fill(0.0))
    add("zero", "nothing in the loading range", grid(200, 2.5, 1250.0, 1400.0))
    add("zero", "no unmasked pixel in the modelling range", long, edit=lambda s, rest: s["ivar"].__setitem__(rest < 1230.0, 0.0))
    add("zero", "one pixel, in the window", np.log10(np.array([1318.0 * 3.5])).astype(np.float32))
    for i, s in enumerate(synthetic.make_raw_spectra(5, first_index=40)):   # the whole BOSS grid, as a file holds it
        groups["default"].append((f"BOSS grid {i}", s, s["z_qso"], 0))
    return groups


def as_csr(cases):
    off = np.concatenate([[0], np.cumsum([c[1]["loglam"].size for c in cases])]).astype(np.int64)
    raw = dict(offsets=off)
    for k, dt in (("flux", np.float32), ("loglam", np.float32), ("ivar", np.float32), ("and_mask", np.int32)):
        raw[k] = np.concatenate([c[1][k] for c in cases]).astype(dt) if cases else np.zeros(0, dt)
    return raw, np.array([c[2] for c in cases], dtype=np.float64), np.array([c[3] for c in cases], dtype=np.uint8)


def check_inputs(raw, z, params):
    """No rest wavelength within 1e-12 relative of a threshold."""
    rest = R.rest_wavelengths(raw, z)
    p = dict(R.DEFAULTS, **params)
    for name in ("loading_min_lambda", "loading_max_lambda", "normalization_min_lambda", "normalization_max_lambda",
                 "min_lambda", "max_lambda"):
        if rest.size:
            gap = np.abs(rest / p[name] - 1.0).min()
            assert gap > THRESHOLD_MARGIN, (name, gap)


def assert_agree(got, want):
    for k in ("filter_flags", "offsets", "pixel_mask", "all_normalizers", "flux", "noise_variance"):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)     # NaN == NaN, inf == inf here
    for k in ("flux", "noise_variance", "all_normalizers"):
        np.testing.assert_array_equal(np.signbit(got[k]), np.signbit(want[k]), err_msg=k)
    np.testing.assert_allclose(got["wavelengths"], want["wavelengths"], rtol=WAVELENGTH_RTOL, atol=0.0)


def assert_identical(a, b):
    for k in ("filter_flags", "offsets", "pixel_mask", "all_normalizers", "flux", "noise_variance", "wavelengths"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def runs():
    """{group: (cases, raw, z, flags, restatement)}; the condition on the inputs is asserted here, before
    any GPU call."""
    out = {}
    for g, cases in build_cases().items():
        raw, z, flags = as_csr(cases)
        check_inputs(raw, z, GROUPS[g])
        out[g] = (cases, raw, z, flags, R.preload(raw, z, flags, **GROUPS[g]))
    assert sum(len(v[0]) for v in out.values()) >= 58
    return out


@pytest.fixture(scope="module")
def device_runs(runs):
    return {g: preload.preload_raw(raw, z, flags, Parameters(**GROUPS[g])) for g, (_, raw, z, flags, _) in runs.items()}


@pytest.mark.parametrize("group", list(GROUPS))
def test_kernel_equals_the_restatement(runs, device_runs, group):
    cases, raw, z, flags, want = runs[group]
    got = device_runs[group]
    counts_g, counts_w = np.diff(got["offsets"]), np.diff(want["offsets"])
    for (name, *_), fg, fw, cg, cw, ng, nw in zip(cases, got["filter_flags"], want["filter_flags"], counts_g, counts_w,
                                                   got["all_normalizers"], want["all_normalizers"]):
        assert (fg, cg) == (fw, cw) and (ng == nw or (np.isnan(ng) and np.isnan(nw))), (name, fg, fw, cg, cw, ng, nw)
    assert_agree(got, want)
    np.testing.assert_array_equal(got["z_qsos"], z)


def test_the_cases_are_what_they_are_called(runs):
    """Read off the restatement: every named corner is in fact exercised."""
    by = {}
    for g, (cases, raw, z, flags, want) in runs.items():
        off, src = want["offsets"], raw["offsets"]
        for i, (name, s, zq, flag) in enumerate(cases):
            rest = rest_of(s["loglam"], zq)
            mask = (s["ivar"] == 0) | ((s["and_mask"].view(np.uint32) >> 23) & 1).astype(bool)
            p = dict(R.DEFAULTS, **GROUPS[g])
            win = (rest >= p["normalization_min_lambda"]) & (rest <= p["normalization_max_lambda"]) & ~mask
            by[name] = dict(flag=int(want["filter_flags"][i]), kept=int(off[i + 1] - off[i]), norm=want["all_normalizers"][i],
                            window=int((win & ~np.isnan(s["flux"])).sum()), rest=rest, mask=mask, n=int(src[i + 1] - src[i]),
                            wl=want["wavelengths"][off[i]:off[i + 1]], pm=want["pixel_mask"][off[i]:off[i + 1]],
                            nv=want["noise_variance"][off[i]:off[i + 1]], fl=want["flux"][off[i]:off[i + 1]],
                            loaded=int(((rest >= p["loading_min_lambda"]) & (rest <= p["loading_max_lambda"])).sum()))
    for k in range(4):
        c = by[f"{k} window values"]
        assert c["window"] == k and c["flag"] == (4 if k == 0 else 0)
    for k in (2048, 2049, 4097):
        assert by[f"{k} window values"]["window"] == k and by[f"{k} window values"]["flag"] == 0
    assert by["three tiles, ties across them"]["window"] == 4500
    for name in ("0 pixels", "1 pixels", "only NaN flux inside the window", "window entirely masked (ivar)",
                 "window entirely masked (and_mask)", "all pixels masked"):
        assert by[name]["flag"] == 4 and by[name]["kept"] == 0 and by[name]["norm"] == 0.0, name
    assert by["a NaN flux inside the window"]["flag"] == 0
    assert by["min_num_pixels - 1 unmasked pixels"]["flag"] == 8 and by["min_num_pixels - 1 unmasked pixels"]["kept"] == 0
    assert by["exactly min_num_pixels unmasked pixels"]["flag"] == 0 and by["exactly min_num_pixels unmasked pixels"]["kept"] > 200
    assert by["flagged on input"] ["flag"] == 2 and by["flagged on input"]["kept"] == 0
    for name in ("live, before a flagged one", "live, after a flagged one", "wavelengths in no order", "4650 pixels",
                 "4650 pixels, default thresholds", "257 pixels", "63 pixels"):
        assert by[name]["flag"] == 0 and by[name]["kept"] > 0, name
    for name, extra in (("edge pixels three masked pixels away", 2), ("no edge pixel below", 1), ("no edge pixel above", 1),
                        ("no edge pixel on either side", 0), ("every pixel below is masked", 1),
                        ("every pixel above is masked", 1), ("tied values", 2)):
        assert by[name]["flag"] == 0 and by[name]["kept"] == by[name]["loaded"] + extra, (name, by[name]["kept"], by[name]["loaded"])
    c = by["edge pixels three masked pixels away"]
    first = np.flatnonzero((c["rest"] >= 910.0) & (c["rest"] <= 1217.0))[0]
    assert c["pm"][0] == 0 and c["pm"][-1] == 0 and c["mask"][first - 3:first].all()
    np.testing.assert_allclose(c["wl"][0], c["rest"][first - 4] * 3.5, rtol=1e-12)
    assert by["zero median"]["norm"] == 0.0 and by["zero median"]["flag"] == 0 and np.isinf(by["zero median"]["nv"]).all()
    assert by["negative median"]["norm"] < 0 and (by["negative median"]["nv"][by["negative median"]["pm"] == 0] > 0).all()
    assert by["all window values equal"]["norm"] == 4.25 and by["tied values"]["norm"] == 3.0
    assert by["ivar 0"]["pm"].sum() > 50 and np.isinf(by["ivar 0"]["nv"][by["ivar 0"]["pm"] == 1]).all()
    assert by["ivar negative"]["pm"].sum() == 0 and (by["ivar negative"]["nv"] < 0).sum() > 50
    assert by["and_mask with only bit 23"]["pm"].sum() > 50 and by["and_mask with every bit"]["pm"].sum() > 50
    for name in ("and_mask with only bit 24", "and_mask with only bit 31", "and_mask with every bit but 23"):
        assert by[name]["pm"].sum() == 0 and by[name]["flag"] == 0, name
    assert by["nothing in the loading range"]["flag"] == 0 and by["nothing in the loading range"]["kept"] == 0
    assert by["nothing in the loading range"]["norm"] != 0.0
    assert by["no unmasked pixel in the modelling range"]["flag"] == 0 and by["no unmasked pixel in the modelling range"]["kept"] > 0
    assert by["one pixel, in the window"]["flag"] == 0 and by["one pixel, in the window"]["kept"] == 0
    assert all(by[f"BOSS grid {i}"]["flag"] == 0 and by[f"BOSS grid {i}"]["n"] == 4608 for i in range(5))


def test_two_calls_are_bit_identical(runs, device_runs):
    for g in ("small", "wide"):
        _, raw, z, flags, _ = runs[g]
        assert_identical(preload.preload_raw(raw, z, flags, Parameters(**GROUPS[g])), device_runs[g])


def test_a_split_at_seven_spectra_changes_nothing(runs, device_runs):
    _, raw, z, flags, _ = runs["small"]
    off = raw["offsets"]
    parts = []
    for lo, hi in ((0, 7), (7, z.size)):
        sub = dict(offsets=off[lo:hi + 1] - off[lo], **{k: raw[k][off[lo]:off[hi]] for k in ("flux", "loglam", "ivar", "and_mask")})
        parts.append(preload.preload_raw(sub, z[lo:hi], flags[lo:hi], Parameters(**GROUPS["small"])))
    joined = {k: np.concatenate([p[k] for p in parts]) for k in ("filter_flags", "pixel_mask", "all_normalizers", "flux",
                                                                 "noise_variance", "wavelengths")}
    joined["offsets"] = np.concatenate([parts[0]["offsets"], parts[0]["offsets"][-1] + parts[1]["offsets"][1:]])
    assert_identical(joined, device_runs["small"])


def test_empty_batch_and_argument_errors():
    empty = dict(offsets=np.zeros(1, np.int64), flux=np.zeros(0, np.float32), loglam=np.zeros(0, np.float32),
                 ivar=np.zeros(0, np.float32), and_mask=np.zeros(0, np.int32))
    got = preload.preload_raw(empty, [], [])
    assert got["offsets"].tolist() == [0] and all(got[k].size == 0 for k in ("wavelengths", "flux", "noise_variance", "pixel_mask",
                                                                           "all_normalizers", "filter_flags"))
    only_empty = dict(empty, offsets=np.zeros(4, np.int64))     # three quasars, no pixel at all
    got = preload.preload_raw(only_empty, [2.0, 2.5, 3.0], [0, 1, 0])
    assert got["offsets"].tolist() == [0, 0, 0, 0] and got["filter_flags"].tolist() == [4, 1, 4]
    with pytest.raises(ValueError):
        preload.preload_raw(dict(empty, offsets=np.array([0, 3])), [2.0], [0])
    with pytest.raises(ValueError):
        preload.preload_raw(only_empty, [2.0], [0, 0, 0])


# ---------------------------------------------------------------------------------------------
# end to end: spec files -> python -m gp_dla_detection_amd.preload -> PreloadedReader
# ---------------------------------------------------------------------------------------------

def test_spec_files_to_preloaded_file(tmp_path):
    n = 24
    spectra = synthetic.make_raw_spectra(n, first_index=100)
    spectra[3]["ivar"][(lambda r: (r >= 1310.0) & (r <= 1325.0))(rest_of(spectra[3]["loglam"], spectra[3]["z_qso"]))] = 0.0
    flags_in = np.array([(i % 5 == 4) * 2 for i in range(n)], dtype=np.uint8)
    cat = dict(z_qsos=np.array([s["z_qso"] for s in spectra]), thing_ids=100000.0 + 7 * np.arange(n),
               plates=3586.0 + np.arange(n) // 4, mjds=55181.0 + np.arange(n) % 3, fiber_ids=1.0 + np.arange(n))
    synthetic.write_spec_files(str(tmp_path / "spectra"), spectra, cat)
    catalog = str(tmp_path / "catalog.mat")
    io.savemat73(catalog, dict({k: v.reshape(-1, 1) for k, v in cat.items()}, filter_flags=flags_in.reshape(-1, 1)))
    before = open(catalog, "rb").read()
    out_pre, out_cat = str(tmp_path / "preloaded_qsos.mat"), str(tmp_path / "catalog_preloaded.mat")
    preload.main([catalog, str(tmp_path / "spectra"), out_pre, out_cat, "--block", "7"])
    assert open(catalog, "rb").read() == before                       # the input catalogue is never modified

    new = io.load_catalog(out_cat)
    flags = new["filter_flags"]
    assert flags.dtype == np.uint8 and flags.tolist() == [4 if i == 3 else int(f) for i, f in enumerate(flags_in)]
    for k, v in cat.items():
        np.testing.assert_array_equal(new[k], v)
    small = io.loadmat73(out_pre, ["all_normalizers"] + list(io.PRELOADED_SCALARS))
    assert [float(np.asarray(small[k]).ravel()[0]) for k in io.PRELOADED_SCALARS] == [910.0, 1217.0, 1310.0, 1325.0, 200.0]
    norm = np.asarray(small["all_normalizers"]).reshape(-1)
    assert np.asarray(small["all_normalizers"]).shape == (n, 1)
    with io.PreloadedReader(out_pre) as r:
        assert r.num_quasars == n
        csr = r.read_csr(np.arange(n), cat["z_qsos"])
    off = csr["offsets"]
    for i, s in enumerate(spectra):
        lo, hi = off[i], off[i + 1]
        if flags[i]:
            assert hi == lo and norm[i] == 0.0
            continue
        lam = 10.0 ** s["loglam"].astype(np.float64)
        idx = np.searchsorted(lam, csr["wavelengths"][lo:hi] * (1 - 1e-9))
        assert hi - lo > 200 and np.all(np.diff(idx) > 0)
        np.testing.assert_allclose(csr["wavelengths"][lo:hi], lam[idx], rtol=WAVELENGTH_RTOL, atol=0.0)
        truth = s["flux"].astype(np.float64)
        with np.errstate(divide="ignore"):
            np.testing.assert_array_equal(csr["flux"][lo:hi], truth[idx] / norm[i])
            np.testing.assert_array_equal(csr["noise_variance"][lo:hi], (1.0 / s["ivar"].astype(np.float64))[idx] / (norm[i] * norm[i]))
        np.testing.assert_array_equal(csr["pixel_mask"][lo:hi], ((s["ivar"] == 0) | (((s["and_mask"] >> 23) & 1) > 0))[idx])
        rest = lam[idx] / (1 + s["z_qso"])
        assert np.all((rest[1:-1] >= 910.0) & (rest[1:-1] <= 1217.0)) and rest[-1] > 1217.0
    # the whole file against the restatement, and the S/N table takes the normalisers it wrote
    raw, z, f0 = as_csr([(str(i), s, s["z_qso"], int(flags_in[i])) for i, s in enumerate(spectra)])
    check_inputs(raw, z, {})
    want = R.preload(raw, z, f0)
    assert_agree(dict(csr, all_normalizers=norm, filter_flags=flags, pixel_mask=csr["pixel_mask"].astype(np.uint8)), want)
    live = np.flatnonzero(flags == 0)
    p = Parameters()
    zmax = np.array([p.max_z_dla(csr["wavelengths"][off[i]:off[i + 1]], cat["z_qsos"][i]) for i in live])
    sub = dict(offsets=np.concatenate([[0], np.cumsum(np.diff(off)[live])]),
               **{k: np.concatenate([csr[k][off[i]:off[i + 1]] for i in live]) for k in ("wavelengths", "flux", "noise_variance")})
    table = snrs.sightline_snrs(sub, zmax, norm[live])
    assert table.shape == (live.size,) and np.all(np.isfinite(table)) and np.all(table > 0)
