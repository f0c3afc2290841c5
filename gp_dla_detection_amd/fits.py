"""A minimal FITS reader for what the preload stage needs: header cards and
binary tables with scalar columns.  No astropy / fitsio exists where this package runs.

The FITS standard (4.0) in the few lines used here: a file is a sequence of HDUs; an HDU is a header
of 80-character cards in 2880-byte blocks, closed by an ``END`` card, followed by its data, padded to
a whole block.  The data of the primary HDU and of an ``IMAGE`` extension hold ``|BITPIX| / 8 *
prod(NAXISn)`` bytes (none when ``NAXIS = 0``); those of a ``BINTABLE`` extension ``NAXIS1 * NAXIS2``
bytes of rows plus ``PCOUNT`` bytes of heap.  Table data are big-endian; column ``n`` has the format
``TFORMn = 'rT'`` (repeat count, type letter) and the name ``TTYPEn``.

    read_headers(path)                    [HDU(cards, data_offset, data_bytes), ...]
    read_bintable(path, hdu, columns)     {column: array} for 1-based positions or TTYPE names
    read_spec_files(paths)                the four columns of many SDSS spec files as one CSR set
    write_bintable(path, tables)          for the tests and synthetic.py only
"""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

BLOCK, CARD = 2880, 80
SKIPPED = ("COMMENT", "HISTORY", "CONTINUE", "")

HDU = namedtuple("HDU", "cards data_offset data_bytes")

#: type letter -> (bytes per element, big-endian NumPy dtype or None where no scalar reader exists)
TYPES = {"L": (1, "u1"), "X": (0, None), "B": (1, "u1"), "I": (2, ">i2"), "J": (4, ">i4"), "K": (8, ">i8"),
         "A": (1, "S"), "E": (4, ">f4"), "D": (8, ">f8"), "C": (8, None), "M": (16, None), "P": (8, None),
         "Q": (16, None)}

#: the columns read_spec.m reads by position and qso_loader.read_spec by name: (TTYPE, TFORM letter)
SPEC_COLUMNS = (("flux", "E"), ("loglam", "E"), ("ivar", "E"), ("and_mask", "J"))


class FITSError(ValueError):
    pass


def parse_card(card: str):
    """One 80-character card -> (keyword, value), or None for COMMENT / HISTORY / CONTINUE / blank
    cards and cards without a value indicator."""
    key = card[:8].rstrip()
    if key in SKIPPED or card[8:10] != "= ":
        return None
    rest = card[10:]
    s = rest.lstrip()
    if s.startswith("'"):   # a string: '' inside it is one quote; trailing blanks do not count
        out, i = [], 1
        while i < len(s):
            if s[i] == "'":
                if s[i + 1:i + 2] == "'":
                    out.append("'")
                    i += 2
                    continue
                break
            out.append(s[i])
            i += 1
        else:
            raise FITSError(f"card {key}: unterminated string")
        return key, "".join(out).rstrip()
    s = s.split("/", 1)[0].strip()
    if s == "T":
        return key, True
    if s == "F":
        return key, False
    if s == "":
        return key, None
    try:
        return key, int(s)
    except ValueError:
        pass
    try:
        return key, float(s.upper().replace("D", "E"))
    except ValueError:
        return key, s   # not a FITS value (real headers carry such cards): kept as its text


def _data_bytes(h: dict, first: bool) -> int:
    naxis = int(h.get("NAXIS", 0))
    if naxis == 0:
        return 0
    n = 1
    for i in range(1, naxis + 1):
        n *= int(h[f"NAXIS{i}"])
    return abs(int(h["BITPIX"])) // 8 * int(h.get("GCOUNT", 1)) * (int(h.get("PCOUNT", 0)) + n)


def read_headers(path: str, limit: int | None = None) -> list:
    """Every HDU of the file (the first ``limit``, when given): its (keyword, value) cards, and where its
    data lie."""
    path = str(path)
    size = os.path.getsize(path)
    hdus = []
    with open(path, "rb") as f:
        pos = 0
        while pos < size and (limit is None or len(hdus) < limit):
            cards, done = [], False
            while not done:   # a header may span several blocks
                block = f.read(BLOCK)
                if len(block) < BLOCK:
                    raise FITSError(f"{path}: truncated in the header of HDU {len(hdus)}")
                pos += BLOCK
                for c in range(0, BLOCK, CARD):
                    card = block[c:c + CARD].decode("ascii", "replace")
                    if card[:8].rstrip() == "END":
                        done = True
                        break
                    try:
                        kv = parse_card(card)
                    except FITSError as e:
                        raise FITSError(f"{path}: HDU {len(hdus)}: {e}") from None
                    if kv is not None:
                        cards.append(kv)
            h = dict(cards)
            if ("SIMPLE" if not hdus else "XTENSION") not in h:
                raise FITSError(f"{path}: HDU {len(hdus)} does not start with {'SIMPLE' if not hdus else 'XTENSION'}")
            try:
                nbytes = _data_bytes(h, not hdus)
            except KeyError as e:
                raise FITSError(f"{path}: HDU {len(hdus)} lacks the card {e.args[0]}") from None
            if pos + nbytes > size:
                raise FITSError(f"{path}: truncated in the data of HDU {len(hdus)}")
            hdus.append(HDU(cards, pos, nbytes))
            pos += -(-nbytes // BLOCK) * BLOCK   # (the heap of a table is part of nbytes)
            f.seek(pos)
    return hdus


def _tform(path, n, value):
    m = re.fullmatch(r"(\d*)([LXBIJKAEDCMPQ])(.*)", str(value).strip())
    if not m:
        raise FITSError(f"{path}: TFORM{n} = {value!r} is not a binary-table format")
    repeat = int(m.group(1)) if m.group(1) else 1
    letter = m.group(2)
    width = (repeat + 7) // 8 if letter == "X" else repeat * TYPES[letter][0]
    return repeat, letter, width


def table_layout(path: str, hdu: HDU, index: int):
    """[(name, repeat, letter, byte offset in the row)] of a BINTABLE HDU, its row length and row count."""
    h = dict(hdu.cards)
    if str(h.get("XTENSION", "")).strip() != "BINTABLE":
        raise FITSError(f"{path}: HDU {index} is not a binary table (XTENSION = {h.get('XTENSION')!r})")
    cols, at = [], 0
    for n in range(1, int(h["TFIELDS"]) + 1):
        if f"TFORM{n}" not in h:
            raise FITSError(f"{path}: HDU {index} lacks TFORM{n}")
        repeat, letter, width = _tform(path, n, h[f"TFORM{n}"])
        cols.append((str(h.get(f"TTYPE{n}", "")).strip(), repeat, letter, at))
        at += width
    if at != int(h["NAXIS1"]):
        raise FITSError(f"{path}: HDU {index}: the TFORMs add up to {at} bytes a row, NAXIS1 = {h['NAXIS1']}")
    return cols, int(h["NAXIS1"]), int(h["NAXIS2"])


def read_bintable(path: str, hdu: int, columns) -> dict:
    """Scalar columns (types L B I J K E D, and A strings) of binary-table HDU ``hdu`` (0 is the primary
    HDU), addressed by 1-based position or by TTYPE name: {column as given: array in native byte order}.
    A scaled column (TSCALn / TZEROn other than 1 / 0) or a variable-length one (P / Q) raises when it is
    asked for."""
    path = str(path)
    hdus = read_headers(path)
    if not 0 < hdu < len(hdus):
        raise FITSError(f"{path}: no extension HDU {hdu} (the file holds {len(hdus)} HDUs)")
    cols, row_bytes, rows = table_layout(path, hdus[hdu], hdu)
    h = dict(hdus[hdu].cards)
    names = [c[0] for c in cols]
    with open(path, "rb") as f:
        f.seek(hdus[hdu].data_offset)
        raw = f.read(row_bytes * rows)
    if len(raw) < row_bytes * rows:
        raise FITSError(f"{path}: truncated in the data of HDU {hdu}")
    table = np.frombuffer(raw, dtype=np.uint8).reshape(rows, row_bytes)
    out = {}
    for want in columns:
        if isinstance(want, (int, np.integer)):
            n = int(want)
            if not 1 <= n <= len(cols):
                raise FITSError(f"{path}: HDU {hdu} has no column {n}")
        else:
            if names.count(want) != 1:
                raise FITSError(f"{path}: HDU {hdu} has {names.count(want)} columns named {want!r}")
            n = names.index(want) + 1
        _, repeat, letter, at = cols[n - 1]
        if letter in "PQ":
            raise FITSError(f"{path}: TFORM{n} = {h[f'TFORM{n}']!r}: variable-length columns are not read")
        size, dt = TYPES[letter]
        if dt is None or (letter != "A" and repeat != 1):
            raise FITSError(f"{path}: TFORM{n} = {h[f'TFORM{n}']!r}: only scalar L B I J K E D and A columns are read")
        if h.get(f"TSCAL{n}", 1) != 1 or h.get(f"TZERO{n}", 0) != 0:
            raise FITSError(f"{path}: TSCAL{n} / TZERO{n} = {h.get(f'TSCAL{n}', 1)} / {h.get(f'TZERO{n}', 0)}: "
                            "scaled columns are not read")
        width = repeat * size
        cell = np.ascontiguousarray(table[:, at:at + width])
        if letter == "A":
            out[want] = np.char.rstrip(cell.reshape(-1).view(f"S{width}") if width else np.zeros(rows, "S1"))
        elif letter == "L":
            out[want] = cell.reshape(-1) == ord("T")
        else:
            out[want] = cell.reshape(-1).view(dt).astype(np.dtype(dt).newbyteorder("="))
    return out


# ---------------------------------------------------------------------------------------------
# SDSS spec files
# ---------------------------------------------------------------------------------------------

def spec_layout(path: str):
    """(data offset, row bytes, rows) of HDU 1 of a spec file after checking that its first four columns
    are flux E, loglam E, ivar E, and_mask J -- by TFORM and, case-insensitively, by TTYPE -- and carry no
    scaling.  A file that disagrees raises and names the file and the card."""
    path = str(path)
    hdus = read_headers(path, limit=2)   # what follows HDU 1 is not looked at
    if len(hdus) < 2:
        raise FITSError(f"{path}: no HDU 1")
    cols, row_bytes, rows = table_layout(path, hdus[1], 1)
    h = dict(hdus[1].cards)
    if len(cols) < 4:
        raise FITSError(f"{path}: TFIELDS = {len(cols)}: HDU 1 needs the four columns flux, loglam, ivar, and_mask")
    for n, (name, letter) in enumerate(SPEC_COLUMNS, 1):
        got_name, repeat, got_letter, _ = cols[n - 1]
        if got_letter != letter or repeat != 1:
            raise FITSError(f"{path}: TFORM{n} = {h[f'TFORM{n}']!r}, expected '{letter}'")
        if got_name.lower() != name:
            raise FITSError(f"{path}: TTYPE{n} = {got_name!r}, expected '{name}'")
        if h.get(f"TSCAL{n}", 1) != 1 or h.get(f"TZERO{n}", 0) != 0:
            raise FITSError(f"{path}: TSCAL{n} / TZERO{n} = {h.get(f'TSCAL{n}', 1)} / {h.get(f'TZERO{n}', 0)}: "
                            "scaled columns are not read")
    if hdus[1].data_offset + row_bytes * rows > os.path.getsize(path):
        raise FITSError(f"{path}: truncated in the data of HDU 1")
    return hdus[1].data_offset, row_bytes, rows


def _read_spec_files_python(paths) -> dict:
    layouts = [None if p is None else spec_layout(p) for p in paths]
    counts = np.array([0 if l is None else l[2] for l in layouts], dtype=np.int64)
    offsets = np.zeros(len(paths) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[-1])
    out = dict(offsets=offsets, flux=np.empty(total, np.float32), loglam=np.empty(total, np.float32),
               ivar=np.empty(total, np.float32), and_mask=np.empty(total, np.int32))
    for i, (p, l) in enumerate(zip(paths, layouts)):
        if l is None or l[2] == 0:
            continue
        with open(p, "rb") as f:
            f.seek(l[0])
            raw = f.read(l[1] * l[2])
        if len(raw) < l[1] * l[2]:
            raise FITSError(f"{p}: truncated in the data of HDU 1")
        t = np.frombuffer(raw, dtype=np.uint8).reshape(l[2], l[1])
        lo, hi = offsets[i], offsets[i + 1]
        for c, (name, letter) in enumerate(SPEC_COLUMNS):
            out[name][lo:hi] = np.ascontiguousarray(t[:, 4 * c:4 * c + 4]).reshape(-1).view(TYPES[letter][1])
    return out


def read_spec_files(paths, native=None, threads=None) -> dict:
    """Columns 1-4 of HDU 1 of every file of ``paths`` (``None`` entries: no file, no pixel) as one CSR
    set: ``offsets`` int64 [n + 1], ``flux`` / ``loglam`` / ``ivar`` float32 and ``and_mask`` int32.  Read
    by csrc/fitsspec.c over up to 16 threads where it can be built (``native=None``: use it if there),
    else by the Python reader, which returns the same arrays.  A missing, truncated or unexpected file
    raises and names the path."""
    paths = [None if p is None else str(p) for p in paths]
    lib = None
    if native is None or native:
        from . import io
        lib = io._load_fitsspec()
        if lib is None and native:
            raise RuntimeError("the native spec-file reader could not be built")
    if lib is None:
        return _read_spec_files_python(paths)
    import ctypes as C
    n = len(paths)
    threads = threads or max(1, min(16, len(os.sched_getaffinity(0))))
    arr = (C.c_char_p * max(n, 1))(*[None if p is None else os.fsencode(p) for p in paths])
    counts, data_off, row_bytes = (np.zeros(max(n, 1), dtype=np.int64) for _ in range(3))
    err = C.create_string_buffer(1024)

    def check(rc):
        if rc:
            msg = err.value.decode("utf-8", "replace")
            if msg.endswith("cannot be opened"):
                raise FileNotFoundError(msg)
            raise FITSError(msg)
    check(lib.gpdla_fitsspec_sizes(arr, n, counts.ctypes.data, data_off.ctypes.data, row_bytes.ctypes.data, err, 1024,
                                   threads))
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts[:n], out=offsets[1:])
    total = int(offsets[-1])
    out = dict(offsets=offsets, flux=np.empty(total, np.float32), loglam=np.empty(total, np.float32),
               ivar=np.empty(total, np.float32), and_mask=np.empty(total, np.int32))
    check(lib.gpdla_fitsspec_read(arr, n, offsets.ctypes.data, data_off.ctypes.data, row_bytes.ctypes.data,
                                  out["flux"].ctypes.data, out["loglam"].ctypes.data, out["ivar"].ctypes.data,
                                  out["and_mask"].ctypes.data, err, 1024, threads))
    return out


# ---------------------------------------------------------------------------------------------
# writer (tests and synthetic.py only)
# ---------------------------------------------------------------------------------------------

def format_card(key: str, value, comment: str = "") -> bytes:
    if isinstance(value, (bool, np.bool_)):
        v = f"{'T' if value else 'F':>20}"
    elif isinstance(value, (int, np.integer)):
        v = f"{int(value):>20d}"
    elif isinstance(value, (float, np.floating)):
        v = f"{float(value)!r:>20}".upper()
    else:
        v = "'" + f"{str(value).replace(chr(39), chr(39) * 2):<8}" + "'"
    card = f"{key:<8}= {v}" + (f" / {comment}" if comment else "")
    if len(card) > CARD:
        raise FITSError(f"card {key} is longer than 80 characters")
    return card.ljust(CARD).encode("ascii")


def _header(cards) -> bytes:
    raw = b"".join(c if isinstance(c, bytes) else format_card(*c) for c in cards) + b"END".ljust(CARD)
    return raw.ljust(-(-len(raw) // BLOCK) * BLOCK)


_LETTER = {"b": "L", "u1": "B", "i2": "I", "i4": "J", "i8": "K", "f4": "E", "f8": "D"}


def write_bintable(path: str, tables, primary_cards=()) -> None:
    """A FITS file with an empty primary HDU and one BINTABLE extension per entry of ``tables``: a list
    of (TTYPE name, 1-D array) columns of equal length (bool, uint8, int16/32/64, float32/64 or bytes).
    ``primary_cards``: extra (keyword, value[, comment]) cards, or raw 80-byte cards, for the primary
    header."""
    with open(str(path), "wb") as f:
        f.write(_header([("SIMPLE", True), ("BITPIX", 8), ("NAXIS", 0), ("EXTEND", True), *primary_cards]))
        for table in tables:
            cols, forms = [], []
            for name, a in table:
                a = np.asarray(a)
                if a.ndim != 1:
                    raise FITSError(f"column {name}: only scalar columns are written")
                if a.dtype.kind == "S":
                    forms.append(f"{a.dtype.itemsize}A")
                    cols.append(np.char.ljust(a, a.dtype.itemsize).view(np.uint8).reshape(a.size, a.dtype.itemsize))
                elif a.dtype.kind == "b":
                    forms.append("L")
                    cols.append(np.where(a, ord("T"), ord("F")).astype(np.uint8).reshape(-1, 1))
                else:
                    code = a.dtype.kind + str(a.dtype.itemsize)
                    if code not in _LETTER:
                        raise FITSError(f"column {name}: dtype {a.dtype} has no binary-table format")
                    forms.append(_LETTER[code])
                    cols.append(a.astype(a.dtype.newbyteorder(">")).view(np.uint8).reshape(a.size, a.dtype.itemsize))
            rows = cols[0].shape[0] if cols else 0
            if any(c.shape[0] != rows for c in cols):
                raise FITSError("the columns of a table need one length")
            body = np.concatenate(cols, axis=1) if cols else np.zeros((0, 0), np.uint8)
            cards = [("XTENSION", "BINTABLE"), ("BITPIX", 8), ("NAXIS", 2), ("NAXIS1", int(body.shape[1])),
                     ("NAXIS2", rows), ("PCOUNT", 0), ("GCOUNT", 1), ("TFIELDS", len(cols))]
            for n, ((name, _), form) in enumerate(zip(table, forms), 1):
                cards += [(f"TTYPE{n}", name), (f"TFORM{n}", form)]
            f.write(_header(cards))
            raw = body.tobytes()
            f.write(raw.ljust(-(-len(raw) // BLOCK) * BLOCK, b"\x00"))
