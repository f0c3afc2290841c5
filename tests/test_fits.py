"""gp_dla_detection_amd/fits.py and csrc/fitsspec.c against files this test lays out
byte by byte with ``struct`` from the FITS standard -- not with fits.write_bintable -- and the other way
round; the native and the Python spec-file readers against each other; the refusals, which name the path;
and csrc/fitsspec.c under the address and undefined-behaviour sanitisers in a stand-alone C program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from gp_dla_detection_amd import fits, io, synthetic

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = 2880


def card(text):
    assert len(text) <= 80
    return text.ljust(80).encode("ascii")


def header(cards):
    raw = b"".join(card(c) for c in cards) + card("END")
    return raw + b" " * (-len(raw) % BLOCK)


def padded(data):
    return data + b"\x00" * (-len(data) % BLOCK)


ROWS = [(True, 7, -300, 2 ** 31 - 1, -2 ** 62, 1.5, -2.5e300, b"ab   "),
        (False, 255, 32767, -2 ** 31, 5, float("inf"), 0.1, b"it's "),
        (True, 0, 0, 0, 0, -0.0, float("nan"), b"     ")]
NAMES = ["FLAG", "BYTE", "SHORT", "INT", "LONG", "FLOAT", "DOUBLE", "TEXT"]


def hand_made(path):
    """Primary header of more than 36 cards (two blocks) with COMMENT, HISTORY, CONTINUE and blank cards;
    a table of eight columns; a table with a variable-length column and PCOUNT > 0; a table of zero rows."""
    primary = ["SIMPLE  =                    T / conforms", "BITPIX  =                    8", "NAXIS   =                    0",
               "EXTEND  =                    T", "COMMENT = this is a comment, not a value", "COMMENT   free text",
               "HISTORY made by hand", "", "OBSERVER= 'O''Brien '           / a doubled quote",
               "LONGSTR = 'the first part&'", "CONTINUE  'and the rest'", "EMPTYSTR= ''", "SLASHSTR= 'a / b'  / comment",
               "EXPTIME =              1.25D+03 / Fortran exponent", "NEGINT  =                  -17", "FLAG    =                    F"]
    primary += [f"KEY{i:<5d}=     {i + 0.5:>15.1f} / filler" for i in range(30)]
    assert len(primary) + 1 > 36
    table = ["XTENSION= 'BINTABLE'", "BITPIX  =                    8", "NAXIS   =                    2",
             "NAXIS1  =                   33", f"NAXIS2  =                    {len(ROWS)}", "PCOUNT  =                    0",
             "GCOUNT  =                    1", "TFIELDS =                    8"]
    for n, (name, form) in enumerate(zip(NAMES, ["L", "1B", "I", "1J", "K", "E", "1D", "5A"]), 1):
        table += [f"TTYPE{n:<3d}= '{name:<8}'", f"TFORM{n:<3d}= '{form:<8}'"]
    table += ["TSCAL6  =                  1.0", "TZERO6  =                    0"]          # the identity scaling is no scaling
    body = b"".join(struct.pack(">cBhiqfd5s", b"T" if r[0] else b"F", *r[1:]) for r in ROWS)
    heap = struct.pack(">3f", 1.0, 2.0, 3.0)
    varlen = ["XTENSION= 'BINTABLE'", "BITPIX  =                    8", "NAXIS   =                    2",
              "NAXIS1  =                   12", "NAXIS2  =                    2", f"PCOUNT  =                   {len(heap)}",
              "GCOUNT  =                    1", "TFIELDS =                    2", "TTYPE1  = 'ID'", "TFORM1  = 'J'",
              "TTYPE2  = 'VALUES'", "TFORM2  = '1PE(2)'"]
    vbody = struct.pack(">iii", 11, 1, 0) + struct.pack(">iii", 12, 2, 4)
    empty = ["XTENSION= 'BINTABLE'", "BITPIX  =                    8", "NAXIS   =                    2",
             "NAXIS1  =                    8", "NAXIS2  =                    0", "PCOUNT  =                    0",
             "GCOUNT  =                    1", "TFIELDS =                    2", "TTYPE1  = 'A'", "TFORM1  = 'E'",
             "TTYPE2  = 'B'", "TFORM2  = 'J'"]
    with open(path, "wb") as f:
        f.write(header(primary) + header(table) + padded(body) + header(varlen) + padded(vbody + heap) + header(empty))


def test_hand_made_file_reads_back_value_for_value(tmp_path):
    p = str(tmp_path / "hand.fits")
    hand_made(p)
    hdus = fits.read_headers(p)
    assert len(hdus) == 4 and hdus[0].data_offset == 2 * BLOCK and hdus[0].data_bytes == 0
    h = dict(hdus[0].cards)
    assert [k for k, _ in hdus[0].cards[:4]] == ["SIMPLE", "BITPIX", "NAXIS", "EXTEND"]
    assert "COMMENT" not in h and "HISTORY" not in h and "CONTINUE" not in h and "" not in h
    assert h["SIMPLE"] is True and h["FLAG"] is False and h["NEGINT"] == -17 and h["EXPTIME"] == 1250.0
    assert h["OBSERVER"] == "O'Brien" and h["LONGSTR"] == "the first part&" and h["EMPTYSTR"] == "" and h["SLASHSTR"] == "a / b"
    assert all(h[f"KEY{i}"] == i + 0.5 for i in range(30)) and len(hdus[0].cards) == 41
    assert hdus[2].data_bytes == 24 + 12 and hdus[3].data_bytes == 0 and hdus[3].data_offset == os.path.getsize(p)

    by_pos = fits.read_bintable(p, 1, range(1, 9))
    by_name = fits.read_bintable(p, 1, NAMES)
    for n, name in enumerate(NAMES, 1):
        want = [r[n - 1] for r in ROWS]
        if name == "TEXT":
            want = [w.rstrip() for w in want]
        got = by_pos[n]
        np.testing.assert_array_equal(got, by_name[name])
        assert got.dtype.isnative and got.dtype == {"FLAG": bool, "BYTE": np.uint8, "SHORT": np.int16, "INT": np.int32,
                                                    "LONG": np.int64, "FLOAT": np.float32, "DOUBLE": np.float64,
                                                    "TEXT": np.dtype("S5")}[name]
        np.testing.assert_array_equal(got, np.array(want, dtype=got.dtype))
    assert np.signbit(by_pos[6][2])
    assert fits.read_bintable(p, 1, ["INT", 1])["INT"].tolist() == [2 ** 31 - 1, -2 ** 31, 0]
    # the table with a heap: its fixed column reads, the variable-length one is refused only when asked for
    assert fits.read_bintable(p, 2, ["ID"])["ID"].tolist() == [11, 12]
    with pytest.raises(fits.FITSError, match="hand.fits.*variable-length"):
        fits.read_bintable(p, 2, ["ID", "VALUES"])
    z = fits.read_bintable(p, 3, [1, "B"])       # behind the heap: PCOUNT bytes were stepped over
    assert z[1].shape == (0,) and z[1].dtype == np.float32 and z["B"].shape == (0,) and z["B"].dtype == np.int32
    for bad in (0, 4):
        with pytest.raises(fits.FITSError, match="hand.fits"):
            fits.read_bintable(p, bad, [1])
    with pytest.raises(fits.FITSError, match="hand.fits"):
        fits.read_bintable(p, 1, ["NOPE"])
    with pytest.raises(fits.FITSError, match="hand.fits"):
        fits.read_bintable(p, 1, [9])


def parse_inline(raw):
    """[(header dict, rows as tuples)] of every table of a file, with struct and the standard's offsets."""
    fmt = {"L": "c", "B": "B", "I": "h", "J": "i", "K": "q", "E": "f", "D": "d"}
    pos, out = 0, []
    while pos < len(raw):
        h = {}
        while True:
            block = raw[pos:pos + BLOCK]
            assert len(block) == BLOCK
            pos += BLOCK
            cards = [block[i:i + 80].decode("ascii") for i in range(0, BLOCK, 80)]
            for c in cards:
                if c[8:10] == "= ":
                    v = c[10:].split("/")[0].strip()
                    h[c[:8].strip()] = v[1:v.rindex("'")].rstrip() if v.startswith("'") else v
            if any(c[:8].strip() == "END" for c in cards):
                break
        if "XTENSION" in h:
            assert h["XTENSION"] == "BINTABLE" and h["BITPIX"] == "8" and h["NAXIS"] == "2" and h["GCOUNT"] == "1"
            row, rows = int(h["NAXIS1"]), int(h["NAXIS2"])
            forms = [h[f"TFORM{n}"] for n in range(1, int(h["TFIELDS"]) + 1)]
            s = ">" + "".join(f[:-1] + "s" if f.endswith("A") else fmt[f[-1]] for f in forms)
            assert struct.calcsize(s) == row
            out.append((h, [struct.unpack(s, raw[pos + i * row:pos + (i + 1) * row]) for i in range(rows)]))
            size = row * rows + int(h["PCOUNT"])
            assert raw[pos + size:pos + size + (-size % BLOCK)].strip(b"\x00") == b""
            pos += size + (-size % BLOCK)
        else:
            assert h["SIMPLE"] == "T" and h["NAXIS"] == "0"
    return out


def test_written_tables_parse_with_the_inline_code(tmp_path):
    p = str(tmp_path / "w.fits")
    rng = np.random.default_rng(5)
    cols = [("flag", rng.uniform(size=5) < 0.5), ("byte", rng.integers(0, 256, 5).astype(np.uint8)),
            ("short", rng.integers(-2 ** 15, 2 ** 15, 5).astype(np.int16)), ("int", rng.integers(-2 ** 31, 2 ** 31, 5).astype(np.int32)),
            ("long", rng.integers(-2 ** 62, 2 ** 62, 5)), ("float", rng.standard_normal(5).astype(np.float32)),
            ("double", rng.standard_normal(5)), ("text", np.array([b"a", b"bc", b"", b"it's", b"xyz"]))]
    fits.write_bintable(p, [cols, [("only", np.zeros(0, np.float32))]], primary_cards=[("ORIGIN", "it's a test"), ("N", 3)])
    raw = open(p, "rb").read()
    assert len(raw) % BLOCK == 0
    (h1, rows1), (h2, rows2) = parse_inline(raw)
    assert [h1[f"TTYPE{n}"] for n in range(1, 9)] == [c[0] for c in cols] and rows2 == [] and h2["TFORM1"] == "E"
    for j, (name, a) in enumerate(cols):
        got = [r[j] for r in rows1]
        if name == "flag":
            got = [g == b"T" for g in got]
        elif name == "text":
            got = [g.rstrip() for g in got]
        assert got == a.tolist(), name
    assert dict(fits.read_headers(p)[0].cards)["ORIGIN"] == "it's a test"
    back = fits.read_bintable(p, 1, [c[0] for c in cols])
    for name, a in cols:
        np.testing.assert_array_equal(back[name], a)


# ---------------------------------------------------------------------------------------------
# spec files: native reader == Python reader; refusals
# ---------------------------------------------------------------------------------------------

def inject(path, hdu, text):
    """Adds one card to the header of HDU `hdu`, in place of its END card (which moves one card on)."""
    raw = bytearray(open(path, "rb").read())
    pos, seen = 0, -1
    while True:
        at = raw.index(b"END" + b" " * 77, pos)
        assert at % 80 == 0
        seen += 1
        if seen == hdu:
            break
        pos = at + 80
    assert (at + 80) % BLOCK != 0
    raw[at:at + 160] = card(text) + card("END")
    open(path, "wb").write(bytes(raw))


@pytest.fixture(scope="module")
def spec_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("spec")
    spectra = synthetic.make_raw_spectra(40, first_index=7)
    lengths = [0, 1, 2, 719, 720, 721, 4608] + list(np.random.default_rng(1).integers(3, 4608, 33))
    for s, n in zip(spectra, lengths):
        for k in ("flux", "loglam", "ivar", "and_mask"):
            s[k] = s[k][:n]
    spectra[5]["flux"][:3] = [np.nan, np.inf, -0.0]
    spectra[5]["and_mask"][:3] = [-1, -2 ** 31, 2 ** 31 - 1]
    cat = dict(plates=4000 + np.arange(40) // 6, mjds=55000 + np.arange(40), fiber_ids=1 + 25 * np.arange(40))
    return spectra, synthetic.write_spec_files(str(d), spectra, cat), d


def test_spec_file_names(spec_files):
    _, paths, d = spec_files
    assert paths[0] == f"{d}/4000/spec-4000-55000-0001.fits" and paths[39] == f"{d}/4006/spec-4006-55039-0976.fits"
    assert all(os.path.getsize(p) % BLOCK == 0 for p in paths)
    assert len(fits.read_headers(paths[3])) == 3 and dict(fits.read_headers(paths[3])[1].cards)["TFIELDS"] == 8


def test_native_and_python_readers_are_identical_on_40_files(spec_files):
    spectra, paths, _ = spec_files
    if io._load_fitsspec() is None:
        pytest.skip("no C compiler: only the Python reader exists here")
    with_gap = paths[:10] + [None] + paths[10:]
    a = fits.read_spec_files(with_gap, native=True)
    b = fits.read_spec_files(with_gap, native=False)
    for k, dt in (("offsets", np.int64), ("flux", np.float32), ("loglam", np.float32), ("ivar", np.float32), ("and_mask", np.int32)):
        assert a[k].dtype == b[k].dtype == dt and a[k].tobytes() == b[k].tobytes(), k
    off = a["offsets"]
    assert off[11] == off[10]
    for i, s in enumerate(spectra):
        j = i + (i >= 10)
        for k in ("flux", "loglam", "ivar", "and_mask"):
            assert a[k][off[j]:off[j + 1]].tobytes() == s[k].tobytes(), (i, k)
    one = fits.read_spec_files(paths[:1] + paths[6:7], native=True, threads=1)
    assert one["offsets"].tolist() == [0, 0, 4608]
    assert fits.read_spec_files([], native=True)["offsets"].tolist() == [0]


def readers():
    return [False] + ([True] if io._load_fitsspec() is not None else [])


def bad_copy(spec_files, tmp_path, name, change):
    spectra, paths, _ = spec_files
    p = str(tmp_path / name)
    shutil.copy(paths[6], p)
    change(p)
    return p


def truncate(n):
    def f(p):
        with open(p, "r+b") as fh:
            fh.truncate(n)
    return f


def retyped(spec_files, col, **kw):
    def f(p):
        s = spec_files[0][6]
        cols = [("flux", s["flux"]), ("loglam", s["loglam"]), ("ivar", s["ivar"]), ("and_mask", s["and_mask"])]
        cols[col] = (kw.get("name", cols[col][0]), cols[col][1].astype(kw.get("dtype", cols[col][1].dtype)))
        fits.write_bintable(p, [cols[:kw.get("keep", 4)]])
    return f


@pytest.mark.parametrize("what, card_named", [
    ("truncated in the data", "truncated"), ("truncated in the second header", "truncated"), ("cut to one block", "HDU 1|truncated"),
    ("flux as D", "TFORM1"), ("and_mask as K", "TFORM4"), ("ivar as I", "TFORM3"), ("loglam named wave", "TTYPE2"),
    ("three columns", "TFIELDS"), ("TSCAL", "TSCAL3"), ("TZERO", "TZERO4"), ("missing", None)])
def test_refusals_name_the_path(spec_files, tmp_path, what, card_named):
    change = {"truncated in the data": truncate(2 * BLOCK + 2 * BLOCK + 4608 * 16),
              "truncated in the second header": truncate(BLOCK + 800), "cut to one block": truncate(BLOCK),
              "flux as D": retyped(spec_files, 0, dtype=np.float64), "and_mask as K": retyped(spec_files, 3, dtype=np.int64),
              "ivar as I": retyped(spec_files, 2, dtype=np.int16), "loglam named wave": retyped(spec_files, 1, name="wave"),
              "three columns": retyped(spec_files, 0, keep=3), "TSCAL": lambda p: inject(p, 1, "TSCAL3  =                  2.0"),
              "TZERO": lambda p: inject(p, 1, "TZERO4  =           2147483648"), "missing": os.remove}[what]
    p = bad_copy(spec_files, tmp_path, "spec-bad.fits", change)
    good = spec_files[1][7]
    for native in readers():
        with pytest.raises((fits.FITSError, FileNotFoundError)) as e:
            fits.read_spec_files([good, p, good], native=native)
        assert "spec-bad.fits" in str(e.value), (native, str(e.value))
        if card_named is None:
            assert isinstance(e.value, FileNotFoundError)
        else:
            import re
            assert re.search(card_named, str(e.value)), (native, str(e.value))


def test_case_of_ttype_does_not_matter_and_identity_scaling_is_accepted(spec_files, tmp_path):
    s = spec_files[0][6]
    p = str(tmp_path / "upper.fits")
    fits.write_bintable(p, [[("FLUX", s["flux"]), ("LogLam", s["loglam"]), ("IVAR", s["ivar"]), ("AND_MASK", s["and_mask"])]])
    inject(p, 1, "TSCAL1  =                  1.0")
    for native in readers():
        got = fits.read_spec_files([p], native=native)
        assert got["flux"].tobytes() == s["flux"].tobytes() and got["and_mask"].tobytes() == s["and_mask"].tobytes()
    # what follows HDU 1 is not looked at: a file cut inside its second table reads the same with both readers
    cut = bad_copy(spec_files, tmp_path, "cut-late.fits", truncate(os.path.getsize(spec_files[1][6]) - BLOCK - 100))
    for native in readers():
        assert fits.read_spec_files([cut], native=native)["ivar"].tobytes() == s["ivar"].tobytes()
    with pytest.raises(fits.FITSError, match="cut-late.fits"):
        fits.read_headers(cut)
    assert dict(fits.read_headers(cut, limit=1)[0].cards)["PLATEID"] == 4001
    assert fits.parse_card("ODD     = 12:30:00".ljust(80)) == ("ODD", "12:30:00")


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_native_reader_under_asan_and_ubsan(spec_files, tmp_path):
    exe = str(tmp_path / "harness")
    src = os.path.join(HERE, "..", "gp_dla_detection_amd", "csrc", "fitsspec.c")
    plain = subprocess.run(["gcc", "-O1", "-Wall", "-fopenmp", os.path.join(HERE, "fitsspec_harness.c"), src, "-o", exe],
                           capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr[-2000:]        # the harness itself compiles; only the runtime may be absent
    build = subprocess.run(["gcc", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fopenmp",
                            os.path.join(HERE, "fitsspec_harness.c"), src, "-o", exe], capture_output=True, text=True)
    if build.returncode:
        pytest.skip("this gcc has no sanitizer runtime: " + build.stderr[-200:])
    _, paths, _ = spec_files
    bad = []
    for i, n in enumerate([0, 79, 80, 2879, 2880, 2881, 5760, 2 * BLOCK + 1000, 3 * BLOCK, 4 * BLOCK + 17, 4 * BLOCK + 4608 * 16]):
        bad.append(bad_copy(spec_files, tmp_path, f"cut{i}.fits", truncate(n)))
    bad.append(bad_copy(spec_files, tmp_path, "tform.fits", retyped(spec_files, 0, dtype=np.float64)))
    bad.append(bad_copy(spec_files, tmp_path, "tscal.fits", lambda p: inject(p, 1, "TSCAL3  =                  2.0")))
    bad.append(bad_copy(spec_files, tmp_path, "noend.fits", lambda p: open(p, "wb").write(card("SIMPLE  =                    T") * 36 * 70)))
    bad.append(bad_copy(spec_files, tmp_path, "huge.fits", lambda p: inject(p, 1, "NAXIS2  =  9223372036854775807")))
    bad.append(str(tmp_path / "absent.fits"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", OMP_NUM_THREADS="4")
    run = subprocess.run([exe] + paths[:12] + bad, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-4000:]
    assert f"ok 12, refused {len(bad)} of {12 + len(bad)}" in run.stdout, run.stdout[-2000:]
