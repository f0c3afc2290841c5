"""Readers/writers for the .mat files either side of the hot path.

The reference hands data between stages through MATLAB files saved with ``-v7.3``, i.e. HDF5
behind a 512-byte MATLAB header: ``learned_qso_model_*.mat`` (learn_qso_model.m:113-123),
``dla_samples.mat`` (generate_dla_samples.m:59-63), ``preloaded_qsos.mat`` (preload_qsos.m:64-79),
``catalog.mat`` (build_catalogs.m:86-91) and the outputs ``processed_qsos_*.mat``
(process_qsos.m:236-250; multi_dlas/process_qsos_multiple_dlas_meanflux.m:498-523), which
``CDDF_analysis`` then opens with ``h5py.File`` and indexes as ``f['p_dlas'][0, :]``,
``f['model_posteriors'][()].T``, ``f['test_ind'][0, :]`` (qso_loader.py:84-112, calc_cddf.py:104).

* ``-v7.3`` files are read and written with the package's own minimal HDF5 implementation
  (:mod:`.hdf5`): the interpreter this package runs under has no h5py (libhdf5 and h5py exist in
  the build image's conda environment and are used to cross-validate it, tests/test_consumers.py).  MATLAB's
  conventions are applied on top of it here: arrays are stored with their dimensions reversed
  (column-major data in a row-major container), logicals as uint8 and chars as uint16 with the
  ``MATLAB_class`` / ``MATLAB_int_decode`` attributes, cell arrays as object references into the
  ``#refs#`` group, empty arrays through ``MATLAB_empty``.
* v5/v7 files (``save -v7``) go through ``scipy.io``.

All functions here speak MATLAB orientation (``sample_log_likelihoods_dla`` is [num_quasars x S],
multi-DLA: [num_quasars x S x max_dlas]) unless stated otherwise.
"""
from __future__ import annotations

import datetime
import os

import numpy as np

from . import grid_fields, hdf5

MATLAB_HEADER_TEXT = "MATLAB 7.3 MAT-file, Platform: GLNXA64, Created on: {date} HDF5 schema 1.00 ."


def _is_hdf5(path: str) -> bool:
    with open(path, "rb") as f:
        head = f.read(520)
    return b"MATLAB 7.3" in head[:128] or head[:8] == hdf5.SIGNATURE or head[512:520] == hdf5.SIGNATURE


# ---------------------------------------------------------------------------------------------
# -v7.3 <-> NumPy, MATLAB conventions
# ---------------------------------------------------------------------------------------------

def matlab_userblock(created: str | None = None) -> bytes:
    """The 512-byte block MATLAB puts in front of the HDF5 superblock: 116 bytes of text, 8 bytes
    of subsystem offset, version 0x0200 and the endian indicator 'IM'; zero-filled to 512."""
    date = created or datetime.datetime.now().strftime("%a %b %d %H:%M:%S %Y")
    text = MATLAB_HEADER_TEXT.format(date=date).encode("ascii")[:116].ljust(116, b" ")
    return (text + b"\x00" * 8 + b"\x00\x02" + b"IM").ljust(512, b"\x00")


def _from_dataset(f: hdf5.File, ds, deref_depth: int = 2):
    """One HDF5 object of a -v7.3 file as MATLAB holds it."""
    if isinstance(ds, hdf5.Group):  # struct: fields are the group's members
        return {k: _from_dataset(f, ds[k], deref_depth) for k in ds.keys()}
    cls = ds.attrs.get("MATLAB_class", "")
    if "MATLAB_empty" in ds.attrs:
        dims = tuple(int(x) for x in ds.read().ravel())
        return [] if cls == "cell" else np.zeros(dims, dtype=bool if cls == "logical" else np.float64)
    a = ds.read()
    if ds.is_reference:
        if deref_depth <= 0:
            return a.T
        flat = [_from_dataset(f, f.dereference(r), deref_depth - 1) for r in a.T.ravel(order="F")]
        return flat  # cell arrays come back as flat lists in MATLAB's (column-major) element order
    a = a.T  # undo the dimension reversal
    if cls == "logical":
        return a.astype(bool)
    if cls == "char":
        return "".join(chr(c) for c in a.ravel(order="F"))
    return a


def loadmat73(path: str, names=None) -> dict:
    """Variables of a ``-v7.3`` file in MATLAB orientation ({name: array | str | list (cell) |
    dict (struct)}).  ``names``: the variables wanted (default: all but ``#refs#``)."""
    out = {}
    with hdf5.File(path) as f:
        for n in (names if names is not None else [k for k in f.keys() if not k.startswith("#")]):
            if n in f:
                out[n] = _from_dataset(f, f[n])
    return out


class _MatWriter:
    """savemat for ``-v7.3``: values in MATLAB orientation."""

    def __init__(self, path: str, created: str | None = None):
        self.w = hdf5.FileWriter(path, userblock=matlab_userblock(created))
        self._refs = 0

    @staticmethod
    def _class_of(a: np.ndarray) -> str:
        if a.dtype.kind == "b":
            return "logical"
        if a.dtype.kind == "f":
            return "double" if a.dtype.itemsize == 8 else "single"
        return {"i": "int", "u": "uint"}[a.dtype.kind] + str(8 * a.dtype.itemsize)

    def _array(self, name: str, value, compress: bool):
        a = np.asarray(value)
        if a.dtype.kind == "O":
            raise TypeError(f"{name}: object arrays are written as cells; pass a list")
        if a.ndim < 2:  # MATLAB has no 0-d / 1-d arrays: scalars are 1x1, vectors columns
            a = a.reshape(-1, 1) if a.ndim == 1 else a.reshape(1, 1)
        attrs = {"MATLAB_class": self._class_of(a)}
        if a.dtype.kind == "b":
            attrs["MATLAB_int_decode"] = np.int32(1)
        if a.size == 0:
            attrs["MATLAB_empty"] = np.int32(1)
            return self.w.create_dataset(name, np.array(a.shape, dtype=np.uint64), attrs=attrs)
        data = np.ascontiguousarray(a.T)  # dimensions reversed, as MATLAB stores them
        if compress and data.nbytes >= 4096:
            chunks = list(data.shape)
            while int(np.prod(chunks)) * data.dtype.itemsize > (1 << 20):  # ~1 MiB chunks, as MATLAB
                ax = int(np.argmax(chunks))
                chunks[ax] = (chunks[ax] + 1) // 2
            return self.w.create_dataset(name, data, attrs=attrs, chunks=chunks, compression="gzip")
        return self.w.create_dataset(name, data, attrs=attrs)

    def _string(self, name: str, value: str):
        codes = np.array([ord(c) for c in value], dtype=np.uint16).reshape(-1, 1)  # 1 x len, reversed
        attrs = {"MATLAB_class": "char", "MATLAB_int_decode": np.int32(2)}
        if codes.size == 0:
            attrs["MATLAB_empty"] = np.int32(1)
            return self.w.create_dataset(name, np.array([0, 0], dtype=np.uint64), attrs=attrs)
        return self.w.create_dataset(name, codes, attrs=attrs)

    def _cell(self, name: str, items, compress: bool):
        if "/#refs#" not in self.w._groups:
            self.w.create_group("#refs#")
        refs = []
        for it in items:
            self._refs += 1
            refs.append(self.put(f"#refs#/{self._refs:08d}", it, compress))
        if not refs:
            return self.w.create_dataset(name, np.array([0, 0], dtype=np.uint64),
                                         attrs={"MATLAB_class": "cell", "MATLAB_empty": np.int32(1)})
        arr = np.empty((1, len(refs)), dtype=object)  # an N x 1 cell, dimensions reversed
        arr[0, :] = refs
        return self.w.create_dataset(name, arr, attrs={"MATLAB_class": "cell"})

    def put(self, name: str, value, compress: bool = False):
        if isinstance(value, str):
            return self._string(name, value)
        if isinstance(value, (list, tuple)):
            return self._cell(name, value, compress)
        return self._array(name, value, compress)

    def put_streamed(self, name: str, matlab_shape, dtype, column_blocks):
        """A MATLAB array too large to transpose in memory.  ``column_blocks`` yields consecutive
        slabs of the STORED (dimension-reversed) array along its first axis -- i.e. slabs along the
        LAST MATLAB dimension, each already reversed."""
        a = np.dtype(dtype)
        cls = "double" if a.kind == "f" and a.itemsize == 8 else self._class_of(np.zeros(0, a))
        return self.w.create_dataset_streamed(name, tuple(matlab_shape)[::-1], a, column_blocks,
                                              attrs={"MATLAB_class": cls})

    def open_chunked(self, name: str, matlab_shape, dtype, stored_chunks):
        """A MATLAB array written chunk by chunk while it is being produced
        (:meth:`hdf5.FileWriter.open_chunked_dataset`); ``stored_chunks``: chunk extents of the
        STORED (dimension-reversed) array."""
        a = np.dtype(dtype)
        cls = "double" if a.kind == "f" and a.itemsize == 8 else self._class_of(np.zeros(0, a))
        return self.w.open_chunked_dataset(name, tuple(matlab_shape)[::-1], a, stored_chunks,
                                           attrs={"MATLAB_class": cls})

    def close(self):
        self.w.close()


def savemat73(path: str, variables: dict, compress: bool = False, created: str | None = None) -> None:
    """``save(path, ..., '-v7.3')`` for a dict of variables in MATLAB orientation: arrays, scalars,
    strings, and lists (written as N x 1 cell arrays).  ``compress``: chunked + deflate datasets
    like MATLAB's own files (default: contiguous, which every HDF5 reader takes and which can be
    memory-mapped)."""
    w = _MatWriter(path, created)
    try:
        for k, v in variables.items():
            w.put(k, v, compress)
    finally:
        w.close()


def _load_mat(path: str, names):
    """{name: array} in MATLAB orientation for the requested variables (cells -> lists)."""
    if _is_hdf5(path):
        return loadmat73(path, names)
    from scipy.io import loadmat
    raw = loadmat(path, variable_names=list(names), squeeze_me=False)
    out = {}
    for n in names:
        if n not in raw:
            continue
        v = raw[n]
        out[n] = [np.asarray(c).squeeze() for c in v.ravel()] if v.dtype == object else v
    return out


def _vec(a):
    return np.asarray(a, dtype=np.float64).reshape(-1)


# ---------------------------------------------------------------------------------------------
# inputs of the path
# ---------------------------------------------------------------------------------------------

def load_learned_model(path: str) -> dict:
    """Variables of process_qsos.m:30-35."""
    names = ("rest_wavelengths", "mu", "M", "log_omega", "log_c_0", "log_tau_0", "log_beta")
    m = _load_mat(path, names)
    missing = [n for n in names if n not in m]
    if missing:
        raise KeyError(f"{path} lacks {missing}")
    G = _vec(m["rest_wavelengths"]).size
    M = np.asarray(m["M"], dtype=np.float64)
    if M.shape[0] != G:
        M = M.T
    return dict(rest_wavelengths=_vec(m["rest_wavelengths"]), mu=_vec(m["mu"]), M=np.asfortranarray(M),
                log_omega=_vec(m["log_omega"]), log_c_0=float(_vec(m["log_c_0"])[0]),
                log_tau_0=float(_vec(m["log_tau_0"])[0]), log_beta=float(_vec(m["log_beta"])[0]))


#: learn_qso_model.m:113-118 without its two MATLAB structs, in the reference's order
LEARNED_MODEL_VARIABLES = ("training_release", "train_ind", "max_noise_variance", "rest_wavelengths", "mu",
                           "initial_M", "initial_log_omega", "initial_log_c_0", "initial_tau_0", "initial_beta",
                           "M", "log_omega", "log_c_0", "log_tau_0", "log_beta", "log_likelihood")


def save_learned_model(path: str, model: dict, training_release: str | None = None, train_ind=None,
                       compress: bool = False) -> None:
    """learned_qso_model_*.mat as learn_qso_model.m:113-123 saves it (``-v7.3``): rest_wavelengths, mu,
    log_omega and initial_log_omega as ROW vectors, M and initial_M as [G x k], the scalars as 1 x 1,
    ``train_ind`` as a catalogue-length logical column and ``training_release`` as a string.  Every
    variable of that list present in ``model`` (or passed here) is written, nothing else.
    ``minFunc_options`` and ``minFunc_output`` are MATLAB structs, which this writer does not support:
    they are left out (``model['fit']`` holds what minFunc_output reports)."""
    extra = {}
    if training_release is not None:
        extra["training_release"] = str(training_release)
    if train_ind is not None:
        t = np.asarray(train_ind)
        if t.dtype != bool:
            raise TypeError("train_ind: a catalogue-length boolean mask")
        extra["train_ind"] = t.reshape(-1, 1)
    rows = ("rest_wavelengths", "mu", "log_omega", "initial_log_omega")
    out = {}
    for name in LEARNED_MODEL_VARIABLES:
        if name in extra:
            out[name] = extra[name]
        elif name in model:
            v = model[name]
            if name in rows:
                v = np.asarray(v, dtype=np.float64).reshape(1, -1)
            elif name in ("M", "initial_M"):
                v = np.asarray(v, dtype=np.float64)
            else:
                v = np.float64(v)
            out[name] = v
    savemat73(path, out, compress=compress)


def load_dla_samples(path: str) -> dict:
    """Variables of process_qsos.m:38-40 (+ lls_nhi_samples when present, set_lls_parameters.m:63)."""
    m = _load_mat(path, ("offset_samples", "log_nhi_samples", "nhi_samples", "lls_nhi_samples",
                         "lls_log_nhi_samples"))
    out = {k: _vec(v) for k, v in m.items()}
    for need in ("offset_samples", "log_nhi_samples", "nhi_samples"):
        if need not in out:
            raise KeyError(f"{path} lacks {need}")
    return out


#: generate_dla_samples.m:59-61 + set_lls_parameters.m:59-71, in the reference's order
DLA_SAMPLE_VECTORS = ("offset_samples", "log_nhi_samples", "nhi_samples", "lls_log_nhi_samples", "lls_nhi_samples")
DLA_SAMPLE_SCALARS = ("uniform_min_log_nhi", "uniform_max_log_nhi", "fit_min_log_nhi", "fit_max_log_nhi", "alpha",
                      "Z_lls", "Z_dla")


def save_dla_samples(path: str, samples: dict) -> None:
    """dla_samples.mat as generate_dla_samples.m:59-63 saves it (``-v7.3``): the sample vectors as ROW
    vectors (stored [S x 1]: the reference's DLACatalogue reads ``f['log_nhi_samples'][:, 0]``), the
    scalars as 1 x 1.  Of the names above, those present in ``samples`` are written, nothing else."""
    out = {}
    for name in DLA_SAMPLE_SCALARS[:5] + DLA_SAMPLE_VECTORS + DLA_SAMPLE_SCALARS[5:]:
        if name in samples:
            out[name] = (np.asarray(samples[name], dtype=np.float64).reshape(1, -1) if name in DLA_SAMPLE_VECTORS
                         else np.float64(samples[name]))
    missing = [n for n in DLA_SAMPLE_VECTORS[:3] if n not in out]
    if missing:
        raise KeyError(f"samples lack {missing}")
    savemat73(path, out)


def load_sample_normalisers(path: str):
    """``(Z_lls, Z_dla)`` of set_lls_parameters.m:70-71 when the samples file carries both, else None."""
    m = _load_mat(path, ("Z_lls", "Z_dla"))
    if "Z_lls" not in m or "Z_dla" not in m:
        return None
    return float(_vec(m["Z_lls"])[0]), float(_vec(m["Z_dla"])[0])


def load_catalog(path: str, names=("z_qsos", "thing_ids", "plates", "mjds", "fiber_ids", "snrs",
                                   "filter_flags", "los_inds", "dla_inds")) -> dict:
    """catalog.mat (build_catalogs.m:86-91): the per-quasar columns as flat vectors.  ``los_inds`` /
    ``dla_inds`` are containers.Map objects in the reference's file, which HDF5 stores opaquely; they
    are returned only when they are plain arrays."""
    m = _load_mat(path, names)
    return {k: (np.asarray(v).reshape(-1) if isinstance(v, np.ndarray) else v) for k, v in m.items()}


def load_preloaded_qsos(path: str, z_qsos, test_ind=None) -> list:
    """The ragged cell arrays of preload_qsos.m:64-79 as a list of per-quasar dicts, after the
    ``test_ind`` subset of process_qsos.m:56-61 (boolean mask or index array, 0-based).  In a
    -v7.3 file only the selected cells are dereferenced."""
    keys = ("all_wavelengths", "all_flux", "all_noise_variance", "all_pixel_mask")
    z = _vec(z_qsos)

    def pick(n):
        if n != z.size:
            raise ValueError(f"{n} spectra but {z.size} redshifts")
        if test_ind is None:
            return np.arange(n)
        t = np.asarray(test_ind)
        return np.flatnonzero(t) if t.dtype == bool else t

    if _is_hdf5(path):
        # the native cell reader where it applies (PreloadedReader.read_csr), split back into per-quasar views
        with PreloadedReader(path) as r:
            idx = pick(r.num_quasars)
            csr = r.read_csr(idx, z)
        o = csr["offsets"]
        return [dict(wavelengths=csr["wavelengths"][o[j]:o[j + 1]], flux=csr["flux"][o[j]:o[j + 1]],
                     noise_variance=csr["noise_variance"][o[j]:o[j + 1]], pixel_mask=csr["pixel_mask"][o[j]:o[j + 1]],
                     z_qso=float(z[i])) for j, i in enumerate(idx)]
    else:
        m = _load_mat(path, keys)
        idx = pick(len(m["all_wavelengths"]))
        cells = {k: [m[k][i] for i in idx] for k in keys}
    return [dict(wavelengths=_vec(cells["all_wavelengths"][j]), flux=_vec(cells["all_flux"][j]),
                 noise_variance=_vec(cells["all_noise_variance"][j]),
                 pixel_mask=np.asarray(cells["all_pixel_mask"][j]).reshape(-1).astype(np.uint8),
                 z_qso=float(z[i])) for j, i in enumerate(idx)]


# ---------------------------------------------------------------------------------------------
# native cell reader (csrc/h5cells.c): the cells of a -v7.3 cell array, many at a time, in threads
# ---------------------------------------------------------------------------------------------

_H5CELLS_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "h5cells.c")
_H5CELLS_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libgpdla_h5cells.so")
_h5cells = None


def build_h5cells(force: bool = False) -> str:
    """gcc -O2 -fopenmp csrc/h5cells.c -lz -> csrc/libgpdla_h5cells.so (host code: no GPU involved)."""
    import subprocess
    if force or not os.path.exists(_H5CELLS_LIB) or os.path.getmtime(_H5CELLS_LIB) < os.path.getmtime(_H5CELLS_SRC):
        tmp = f"{_H5CELLS_LIB}.{os.getpid()}.tmp"  # the ranks of a run may all get here at once: publish atomically
        try:
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-fopenmp", "-Wall", _H5CELLS_SRC, "-lz", "-o", tmp],
                                  stderr=subprocess.DEVNULL if not force else None)
            os.replace(tmp, _H5CELLS_LIB)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return _H5CELLS_LIB


def _load_h5cells():
    """The native cell reader, or None when it cannot be built / loaded (no gcc or zlib on the box):
    :class:`PreloadedReader` then reads every cell with the Python reader -- same arrays, slower."""
    global _h5cells
    if _h5cells is None:
        import ctypes as C
        try:
            # an existing library is used as it is (__graft_entry__.build() refreshes it); a missing one is built
            lib = C.CDLL(_H5CELLS_LIB if os.path.exists(_H5CELLS_LIB) else build_h5cells())
            lib.gpdla_h5cells_sizes.restype = C.c_int
            lib.gpdla_h5cells_sizes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_int]
            lib.gpdla_h5cells_read.restype = C.c_int64
            lib.gpdla_h5cells_read.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int64, C.c_int32,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            _h5cells = lib
        except Exception:  # (a missing compiler must not stop a run: the Python reader is complete)
            _h5cells = False
    return _h5cells or None


_FITSSPEC_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "fitsspec.c")
_FITSSPEC_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libgpdla_fitsspec.so")
_fitsspec = None


def build_fitsspec(force: bool = False) -> str:
    """gcc -O2 -fopenmp csrc/fitsspec.c -> csrc/libgpdla_fitsspec.so (host code: no GPU involved)."""
    import subprocess
    if force or not os.path.exists(_FITSSPEC_LIB) or os.path.getmtime(_FITSSPEC_LIB) < os.path.getmtime(_FITSSPEC_SRC):
        tmp = f"{_FITSSPEC_LIB}.{os.getpid()}.tmp"  # published atomically, as build_h5cells does
        try:
            subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-fopenmp", "-Wall", _FITSSPEC_SRC, "-o", tmp],
                                  stderr=subprocess.DEVNULL if not force else None)
            os.replace(tmp, _FITSSPEC_LIB)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return _FITSSPEC_LIB


def _load_fitsspec():
    """The native spec-file reader, or None when it cannot be built / loaded: fits.read_spec_files then
    reads every file with the Python reader -- same arrays, slower."""
    global _fitsspec
    if _fitsspec is None:
        import ctypes as C
        try:
            lib = C.CDLL(_FITSSPEC_LIB if os.path.exists(_FITSSPEC_LIB) else build_fitsspec())
            lib.gpdla_fitsspec_sizes.restype = C.c_int
            lib.gpdla_fitsspec_sizes.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p,
                                                 C.c_int, C.c_int]
            lib.gpdla_fitsspec_read.restype = C.c_int
            lib.gpdla_fitsspec_read.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_char_p, C.c_int, C.c_int]
            _fitsspec = lib
        except Exception:  # (a missing compiler must not stop a run: the Python reader is complete)
            _fitsspec = False
    return _fitsspec or None


class PreloadedReader:
    """Random access to the ragged cell arrays of a ``-v7.3`` preloaded_qsos.mat (preload_qsos.m:64-79):
    the file is opened once, the four reference tables are read, and a rank then dereferences only
    the quasars of its own block -- pixel counts come from the dataset headers alone, so sharding a
    run by pixel count (distributed.shard_bounds) reads no spectrum.  :meth:`read` is the pure-Python
    reader (one thread: ~4000-11000 quasars/s depending on the host core and on whether the cells
    are compressed; header parsing under the GIL, so threads do not help).
    :meth:`read_csr` is the fast path: the same cells through csrc/h5cells.c (object headers, chunk
    B-trees and zlib in C, cells spread over threads), straight into the flat arrays a batch
    upload takes; cells outside that reader's subset, or a box without gcc, fall back to the
    Python reader cell by cell."""

    KEYS = ("all_wavelengths", "all_flux", "all_noise_variance", "all_pixel_mask")
    _DTYPES = (np.float64, np.float64, np.float64, np.uint8)

    def __init__(self, path: str):
        if not _is_hdf5(path):
            raise ValueError(f"{path}: not a -v7.3 file (use load_preloaded_qsos for -v7 files)")
        self.path = path
        self._f = hdf5.File(path)
        self._refs = {}
        for k in self.KEYS:
            if k not in self._f:
                self._f.close()
                raise KeyError(f"{path} lacks {k}")
            self._refs[k] = self._f[k].read().T.ravel(order="F")
        self.num_quasars = int(self._refs[self.KEYS[0]].size)
        self._map = None  # (address, length) of the file's memory map, for the native reader
        self.threads = max(1, min(16, len(os.sched_getaffinity(0))))

    def _native(self):
        lib = _load_h5cells()
        if lib is not None and self._map is None:
            view = np.frombuffer(self._f._mm, dtype=np.uint8)  # the map hdf5.File already holds
            self._map = (view.ctypes.data, view.size, view)
        return lib

    def _python_count(self, i) -> int:
        ds = self._f.dereference(self._refs["all_wavelengths"][i])
        if len(ds.shape) == 1 and "MATLAB_empty" in ds.attrs:
            return 0
        return int(np.prod(ds.shape))

    def pixel_counts(self, indices=None) -> np.ndarray:
        """Stored pixels per quasar (``numel(all_wavelengths{i})``) for the 0-based ``indices``."""
        idx = np.arange(self.num_quasars) if indices is None else np.asarray(indices)
        lib = self._native()
        if lib is None or idx.size == 0:
            return np.array([self._python_count(i) for i in idx], dtype=np.int64)
        addrs = np.ascontiguousarray(self._refs["all_wavelengths"][idx], dtype=np.uint64)
        counts = np.empty(idx.size, dtype=np.int64)
        sizes = np.empty(idx.size, dtype=np.int32)
        lib.gpdla_h5cells_sizes(self._map[0], self._map[1], self._f.userblock_size, addrs.ctypes.data, idx.size, counts.ctypes.data,
                                sizes.ctypes.data, self.threads)
        for j in np.flatnonzero(counts < 0):  # outside the native reader's subset (e.g. an empty cell)
            counts[j] = self._python_count(idx[j])
        return counts

    def read_csr(self, indices, z_qsos) -> dict:
        """The spectra of the 0-based ``indices`` as the flat arrays a batch upload takes
        (``api.spectra_to_csr``'s dict: offsets, wavelengths, flux, noise_variance, pixel_mask,
        z_qsos), read by the native reader where it applies."""
        z = _vec(z_qsos)
        if z.size != self.num_quasars:
            raise ValueError(f"{self.num_quasars} spectra but {z.size} redshifts")
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        counts = self.pixel_counts(idx)
        offsets = np.zeros(idx.size + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        total = int(offsets[-1])
        out = dict(offsets=offsets, z_qsos=np.ascontiguousarray(z[idx], dtype=np.float64))
        lib = self._native()
        for key, dt, name in zip(self.KEYS, self._DTYPES, ("wavelengths", "flux", "noise_variance", "pixel_mask")):
            flat = np.empty(total, dtype=dt)
            status = np.full(idx.size, -1, dtype=np.int8)
            if lib is not None and idx.size:
                addrs = np.ascontiguousarray(self._refs[key][idx], dtype=np.uint64)
                byte_off = np.ascontiguousarray(offsets[:-1] * flat.itemsize)
                lib.gpdla_h5cells_read(self._map[0], self._map[1], self._f.userblock_size, addrs.ctypes.data, idx.size, flat.itemsize,
                                       int(flat.dtype.kind == "f"), flat.ctypes.data, byte_off.ctypes.data,
                                       counts.ctypes.data, status.ctypes.data, self.threads)
            for j in np.flatnonzero(status):  # the Python reader, for whatever the native one left
                v = self._vec(key, idx[j], dt)
                if v.size != counts[j]:
                    raise ValueError(f"{self.path}: {key}{{{idx[j] + 1}}} has {v.size} elements, "
                                     f"all_wavelengths{{{idx[j] + 1}}} {counts[j]}")
                flat[offsets[j]:offsets[j + 1]] = v
            out[name] = flat
        return out

    def _vec(self, key, i, dt):
        # the cells are plain numeric / logical vectors: their class attributes are not needed,
        # only an empty cell (stored as its dimensions, MATLAB_empty) must be told apart
        ds = self._f.dereference(self._refs[key][i])
        if len(ds.shape) == 1 and "MATLAB_empty" in ds.attrs:
            return np.zeros(0, dtype=dt)
        return np.asarray(ds.read(), dtype=dt).reshape(-1)

    def read(self, indices, z_qsos) -> list:
        """Per-quasar dicts (as :func:`load_preloaded_qsos` returns) for the 0-based ``indices``;
        ``z_qsos``: the catalogue's redshift column for ALL quasars of the file."""
        z = _vec(z_qsos)
        if z.size != self.num_quasars:
            raise ValueError(f"{self.num_quasars} spectra but {z.size} redshifts")
        vec = self._vec

        return [dict(wavelengths=vec("all_wavelengths", i, np.float64), flux=vec("all_flux", i, np.float64),
                     noise_variance=vec("all_noise_variance", i, np.float64),
                     pixel_mask=vec("all_pixel_mask", i, np.uint8), z_qso=float(z[i]))
                for i in np.asarray(indices)]

    def close(self):
        self._map = None  # (drops the view of the map before hdf5.File closes it)
        self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


#: preload_qsos.m:73-77: the five scalars, then the four cell arrays and all_normalizers
PRELOADED_SCALARS = ("loading_min_lambda", "loading_max_lambda", "normalization_min_lambda",
                     "normalization_max_lambda", "min_num_pixels")


class PreloadedStreamWriter:
    """preloaded_qsos.mat (preload_qsos.m:73-79, ``-v7.3``) for spectra that arrive block by block: every
    block's cells are written when :meth:`append` gets them -- column vectors, ``all_pixel_mask`` logical,
    a quasar without pixels as the 0 x 0 empty ``cell(n, 1)`` leaves -- and :meth:`finish` writes the four
    N x 1 cell arrays that point at them, ``all_normalizers`` and the five scalars."""

    def __init__(self, path: str, params=None, compress: bool = False):
        from .parameters import Parameters
        self.params = params or Parameters()
        self.compress = compress
        self.w = _MatWriter(path)
        self.w.w.create_group("#refs#")
        self._cells = {k: [] for k in PreloadedReader.KEYS}
        self._norm = []

    def append(self, block: dict) -> None:
        """One block in the shape ``preload.preload_csr`` returns (offsets, wavelengths, flux,
        noise_variance, pixel_mask, all_normalizers)."""
        off = np.asarray(block["offsets"], dtype=np.int64)
        for key, name, dt in zip(PreloadedReader.KEYS, ("wavelengths", "flux", "noise_variance", "pixel_mask"),
                                 (np.float64, np.float64, np.float64, bool)):
            flat = np.asarray(block[name]).astype(dt, copy=False)
            for i in range(off.size - 1):
                v = flat[off[i]:off[i + 1]]
                self.w._refs += 1
                self._cells[key].append(self.w.put(f"#refs#/{self.w._refs:08d}",
                                                   v.reshape(-1, 1) if v.size else np.zeros((0, 0), dtype=dt), self.compress))
        self._norm.append(np.asarray(block["all_normalizers"], dtype=np.float64).reshape(-1))

    def finish(self) -> None:
        try:
            p = self.params
            for k in PRELOADED_SCALARS:
                self.w.put(k, np.float64(getattr(p, k)))
            for key, refs in self._cells.items():
                if not refs:
                    self.w.w.create_dataset(key, np.array([0, 0], dtype=np.uint64),
                                            attrs={"MATLAB_class": "cell", "MATLAB_empty": np.int32(1)})
                    continue
                arr = np.empty((1, len(refs)), dtype=object)  # an N x 1 cell, dimensions reversed
                arr[0, :] = refs
                self.w.w.create_dataset(key, arr, attrs={"MATLAB_class": "cell"})
            self.w.put("all_normalizers", np.concatenate(self._norm) if self._norm else np.zeros((0, 1)))
        finally:
            self.w.close()

    def abort(self) -> None:
        try:
            self.w.close()
        except Exception:
            pass


def save_preloaded_qsos(path: str, blocks, params=None, compress: bool = False) -> None:
    """preloaded_qsos.mat from one block (a dict) or an iterable of blocks, streamed block by block."""
    w = PreloadedStreamWriter(path, params, compress)
    try:
        for b in ([blocks] if isinstance(blocks, dict) else blocks):
            w.append(b)
    except BaseException:
        w.abort()
        raise
    w.finish()


# ---------------------------------------------------------------------------------------------
# outputs of the path
# ---------------------------------------------------------------------------------------------

#: process_qsos.m:236-244 (result variables; the run metadata of :236-238 are keyword arguments)
SAVED_VARIABLES = ("min_z_dlas", "max_z_dlas", "log_priors_no_dla", "log_priors_dla",
                   "log_likelihoods_no_dla", "sample_log_likelihoods_dla", "log_likelihoods_dla",
                   "log_posteriors_no_dla", "log_posteriors_dla", "model_posteriors", "p_no_dlas",
                   "p_dlas")

#: multi_dlas/process_qsos_multiple_dlas_meanflux.m:498-510
SAVED_VARIABLES_MULTI = ("min_z_dlas", "max_z_dlas", "sample_log_likelihoods_dla", "base_sample_inds",
                         "log_priors_no_dla", "log_priors_dla", "log_priors_lls",
                         "log_likelihoods_no_dla", "MAP_z_dlas", "MAP_log_nhis", "log_likelihoods_dla",
                         "log_likelihoods_lls", "log_posteriors_no_dla", "log_posteriors_dla",
                         "log_posteriors_lls", "model_posteriors", "p_no_dlas", "p_dlas", "p_lls",
                         "all_exceptions", "sample_log_likelihoods_lls")

#: how this package's multi-DLA arrays ([nq, model, S] etc.) map onto MATLAB's axes (multi :110-131)
_MULTI_TO_MATLAB = {"sample_log_likelihoods_dla": (0, 2, 1),   # [nq, md, S] -> [nq, S, md]
                    "base_sample_inds": (0, 2, 1)}              # [nq, md-1, S] -> [nq, S, md-1]


def _metadata(w: _MatWriter, results: dict, run_metadata: dict, extra=()):
    for k, v in run_metadata.items():
        w.put(k, v)
    for k in ("prior_z_qso_increase", "max_z_cut", "num_lines") + tuple(extra):
        if k in results and k not in run_metadata:
            w.put(k, np.float64(results[k]))


def _streamed_table(w: _MatWriter, name: str, table: np.ndarray, block_rows: int = 64):
    """[nq, S] -> the MATLAB variable [nq x S], i.e. a stored (S, nq) array, written in slabs of
    ``block_rows`` samples so that the 13 GB table of a DR12Q run is never duplicated."""
    nq, S = table.shape
    w.put_streamed(name, (nq, S), np.float64,
                   (np.ascontiguousarray(table[:, i:i + block_rows].T) for i in range(0, S, block_rows)))


def save_processed_qsos(path: str, results: dict, test_ind=None, **run_metadata) -> None:
    """process_qsos.m:236-250 as a ``-v7.3`` file ``CDDF_analysis`` reads unchanged: the result
    variables (column vectors, ``sample_log_likelihoods_dla`` [nq x S], ``model_posteriors``
    [nq x 2]), ``test_ind`` (logical column, read back as ``f['test_ind'][0, :]``,
    qso_loader.py:95) and the run metadata the script echoes (training_release, training_set_name,
    dla_catalog_name, prior_ind, release, test_set_name, ...)."""
    w = _MatWriter(path)
    try:
        _metadata(w, results, run_metadata)
        if test_ind is not None:
            w.put("test_ind", np.asarray(test_ind, dtype=bool).reshape(-1, 1))
        for k in SAVED_VARIABLES:
            v = np.asarray(results[k], dtype=np.float64)
            if k == "sample_log_likelihoods_dla" and v.nbytes > (256 << 20):
                _streamed_table(w, k, v)
            else:
                w.put(k, v)
        # The MAP sample of generate_ascii_catalog.m:73-80, which the evidence kernel finds anyway: an
        # extra, stored as single_MAP_*.  NOT under the multi-DLA names: QSOLoader takes a file with a
        # 'MAP_log_nhis' key for a multi-DLA file and indexes it [nq, model, slot] (qso_loader.py:106-109,
        # 160-162) -- found by running the reference's loader on these files.
        for k in ("MAP_inds", "MAP_z_dlas", "MAP_log_nhis"):
            if k in results and np.ndim(results[k]) == 1:
                w.put("single_" + k, np.asarray(results[k], dtype=np.float64))
    finally:
        w.close()


def save_processed_qsos_multi(path: str, results: dict, test_ind=None, **run_metadata) -> None:
    """multi_dlas/process_qsos_multiple_dlas_meanflux.m:498-523 as a ``-v7.3`` file:
    ``sample_log_likelihoods_dla`` [nq x S x max_dlas] (read back as ``[max_dlas, S, nq]``,
    calc_cddf.py:266), ``base_sample_inds`` uint32 [nq x S x max_dlas-1] (:116), ``MAP_*``
    [nq x model x slot] (:129-131; ``f['MAP_log_nhis'][()].T``, qso_loader.py:107-109),
    ``model_posteriors`` [nq x 2+max_dlas], ``all_exceptions`` (:139)."""
    w = _MatWriter(path)
    try:
        _metadata(w, results, run_metadata, extra=("k", "min_z_cut", "num_dla_samples",
                                                   "normalization_min_lambda", "normalization_max_lambda"))
        if test_ind is not None:
            w.put("test_ind", np.asarray(test_ind, dtype=bool).reshape(-1, 1))
        for k in SAVED_VARIABLES_MULTI + ("MAP_inds",):
            if k not in results:
                if k == "MAP_inds":
                    continue
                raise KeyError(f"results lack {k}")
            v = np.asarray(results[k])
            if k in _MULTI_TO_MATLAB:
                v = np.transpose(v, _MULTI_TO_MATLAB[k])
            w.put(k, v.astype(np.uint32) if k == "base_sample_inds" else v.astype(np.float64))
    finally:
        w.close()


class ProcessedStreamWriter:
    """``save_processed_qsos`` / ``save_processed_qsos_multi`` for a run whose results arrive batch
    by batch: the per-sample tables -- 1.6 GB for a DR12Q shard, the only large variables -- are
    transposed into MATLAB's order and written as one column of HDF5 chunks per batch WHILE the next
    batch is swept (:meth:`append`, called by the pipeline's download thread); :meth:`finish`
    writes the per-quasar variables and the metadata.  The file holds the same variables with the
    same shapes and classes as the one-shot writers'; the large ones are chunked (as MATLAB's own
    ``-v7.3`` files are) instead of contiguous.  ``batch``: the chunks' extent along the quasar axis --
    every batch but the last must hold a whole multiple of it."""

    _TARGET = 8 << 20  # bytes per chunk, about

    def __init__(self, path: str, num_quasars: int, num_samples: int, batch: int, max_dlas: int = 0):
        self.nq, self.S, self.B, self.md = int(num_quasars), int(num_samples), max(1, int(batch)), int(max_dlas)
        self.w = _MatWriter(path)
        self.done = 0
        S, nq, B = self.S, self.nq, min(self.B, max(1, self.nq))
        self.B = B

        def rows(itemsize):  # chunk extent along the sample axis: about _TARGET bytes per chunk, and an even
            want = max(1, min(S, self._TARGET // (itemsize * B)))  # split of S (every chunk is stored whole:
            return -(-S // -(-S // want))                          # a ragged last chunk row would be padding)
        self.streams = {}
        try:
            if self.md:  # stored (dimension-reversed): [md, S, nq], [md - 1, S, nq], [S, nq]
                self.streams["sample_log_likelihoods_dla"] = (
                    self.w.open_chunked("sample_log_likelihoods_dla", (nq, S, self.md), np.float64, (1, rows(8), B)), 8)
                if self.md > 1:
                    self.streams["base_sample_inds"] = (
                        self.w.open_chunked("base_sample_inds", (nq, S, self.md - 1), np.uint32, (1, rows(4), B)), 4)
                self.streams["sample_log_likelihoods_lls"] = (
                    self.w.open_chunked("sample_log_likelihoods_lls", (nq, S), np.float64, (rows(8), B)), 8)
            else:
                self.streams["sample_log_likelihoods_dla"] = (
                    self.w.open_chunked("sample_log_likelihoods_dla", (nq, S), np.float64, (rows(8), B)), 8)
        except Exception:
            self.w.close()
            raise

    @property
    def streamed(self):
        return tuple(self.streams)

    def append(self, at: int, tables: dict) -> None:
        """The rows ``at .. at + n`` of the run: ``tables[name]`` = this package's orientation,
        [n, S] or [n, model, S]."""
        n, B = None, self.B
        for name, (st, _) in self.streams.items():
            t = np.asarray(tables[name])
            n = t.shape[0] if n is None else n
            if at % B or t.shape[0] != n or (n % B and at + n != self.nq):
                raise ValueError(f"batch [{at}, {at + n}) does not sit on the {B}-quasar chunk grid")
            cs = st.chunks[-2]
            for c0 in range(0, n, B):  # a batch may span several chunk columns
                if t.ndim == 2:
                    tt = np.ascontiguousarray(t[c0:c0 + B].T)  # [S, <= B]
                    for r0 in range(0, self.S, cs):
                        st.write_chunk((r0, at + c0), tt[r0:r0 + cs])
                else:
                    for mdl in range(t.shape[1]):
                        tt = np.ascontiguousarray(t[c0:c0 + B, mdl, :].T)
                        for r0 in range(0, self.S, cs):
                            st.write_chunk((mdl, r0, at + c0), tt[None, r0:r0 + cs])
        self.done += n or 0

    def finish(self, results: dict, test_ind=None, **run_metadata) -> None:
        """The remaining variables of ``results`` (all rows) and the metadata; closes the file."""
        w = self.w
        try:
            if self.done != self.nq:
                raise ValueError(f"{self.done} of {self.nq} quasars were appended")
            for st, _ in self.streams.values():
                st.close()
            extra = ("k", "min_z_cut", "num_dla_samples", "normalization_min_lambda",
                     "normalization_max_lambda") if self.md else ()
            _metadata(w, results, run_metadata, extra=extra)
            if test_ind is not None:
                w.put("test_ind", np.asarray(test_ind, dtype=bool).reshape(-1, 1))
            if self.md:
                for k in SAVED_VARIABLES_MULTI + ("MAP_inds",):
                    if k in self.streams:
                        continue
                    if k not in results:
                        if k in ("MAP_inds", "base_sample_inds"):
                            continue
                        raise KeyError(f"results lack {k}")
                    v = np.asarray(results[k])
                    if k in _MULTI_TO_MATLAB:
                        v = np.transpose(v, _MULTI_TO_MATLAB[k])
                    w.put(k, v.astype(np.uint32) if k == "base_sample_inds" else v.astype(np.float64))
            else:
                for k in SAVED_VARIABLES:
                    if k not in self.streams:
                        w.put(k, np.asarray(results[k], dtype=np.float64))
                for k in ("MAP_inds", "MAP_z_dlas", "MAP_log_nhis"):  # (see save_processed_qsos)
                    if k in results and np.ndim(results[k]) == 1:
                        w.put("single_" + k, np.asarray(results[k], dtype=np.float64))
        finally:
            w.close()

    def abort(self) -> None:
        try:
            self.w.close()
        except Exception:
            pass


def load_processed_qsos(path: str) -> dict:
    """A processed_qsos_*.mat written by the reference or by this package, in this package's
    orientation (vectors flat; multi-DLA 3-D arrays as [nq, model, S] / [nq, model, slot])."""
    m = loadmat73(path) if _is_hdf5(path) else _load_mat(path, SAVED_VARIABLES_MULTI + SAVED_VARIABLES
                                                        + ("test_ind", "MAP_inds"))
    out = {}
    for k, v in m.items():
        if k.startswith("single_MAP_"):  # save_processed_qsos: the single-DLA MAP extras
            k = k[len("single_"):]
        if isinstance(v, np.ndarray):
            if v.ndim == 2 and 1 in v.shape and k not in ("model_posteriors",):
                v = v.reshape(-1)
            elif v.ndim == 3 and k in _MULTI_TO_MATLAB:
                v = np.transpose(v, (0, 2, 1))
        out[k] = v
    return out


# ---------------------------------------------------------------------------------------------
# model spectra
# ---------------------------------------------------------------------------------------------

#: the names of :mod:`grid_fields` by the form they take in a file: per-pixel cells; cells of [pixels x max_dlas];
#: [n x columns] matrices; columns
MODEL_SPECTRA_CELLS = grid_fields.names("model_spectra")
MODEL_SPECTRA_MULTI_CELLS = grid_fields.names("model_spectra_multi", "pixel")
MODEL_SPECTRA_MULTI_PLANE_CELLS = grid_fields.names("model_spectra_multi", "plane")
MARGINAL_CONTINUUM_CELLS = grid_fields.names("marginal_continuum", "pixel")
MARGINAL_CONTINUUM_MATRICES = grid_fields.names("marginal_continuum", "row", (None, "caller"))
PREDICTIVE_FLUX_CELLS = grid_fields.names("predictive_flux", "pixel")
PREDICTIVE_FLUX_COLUMNS = grid_fields.names("predictive_flux", "column")


def _save_grid_product(path: str, res: dict, products, run_metadata: dict) -> None:
    """THE saver of the grid products: ``run_metadata`` as given, ``quasar_ind`` (the selection, 1-based like every MATLAB
    index), ``num_pixels`` and ``status`` as columns; of a refined product (``refined=`` of the drivers in :mod:`api`)
    ``refine_boxes`` [N x 4 levels] with a quasar's level l in columns 4 l .. 4 l + 3 as (z_lo, z_hi, n_lo, n_hi) and
    ``refine_status``; of the model spectra the selected absorbers as the cells ``map_z_dlas`` / ``map_log_nhis`` (when
    ``absorber_offsets``, ``absorber_z_dlas`` and ``absorber_log_nhis`` are present); then every field of ``products`` that ``res`` holds, in the
    order and the form :mod:`grid_fields` declares."""
    off = np.asarray(res["offsets"], dtype=np.int64)
    nsel = off.size - 1
    w = _MatWriter(path)
    try:
        for k, v in run_metadata.items():
            w.put(k, v)
        w.put("quasar_ind", np.asarray(res.get("selection", np.arange(nsel)), dtype=np.float64) + 1)
        w.put("num_pixels", np.diff(off).astype(np.float64))
        w.put("status", np.asarray(res.get("status", np.zeros(nsel)), dtype=np.float64))
        if "boxes" in res:
            b = np.asarray(res["boxes"], dtype=np.float64)
            w.put("refine_boxes", np.ascontiguousarray(b.reshape(b.shape[0], -1)))
            w.put("refine_status", np.asarray(res["refine_status"], dtype=np.float64))
        if "absorber_offsets" in res and "model_spectra" in products:
            a = np.asarray(res["absorber_offsets"], dtype=np.int64)
            for name, key in (("map_z_dlas", "absorber_z_dlas"), ("map_log_nhis", "absorber_log_nhis")):
                v = np.asarray(res[key], dtype=np.float64)
                w.put(name, [v[a[i]:a[i + 1]].reshape(-1, 1) for i in range(nsel)])
        for f in (f for product in products for f in grid_fields.fields(product) if f.name in res):
            v = np.ascontiguousarray(res[f.name], dtype=np.float64)
            if f.kind == "pixel":
                v = [v[off[i]:off[i + 1]].reshape(-1, 1) for i in range(nsel)]
            elif f.kind == "plane":   # [max_dlas, total]: one [pixels x max_dlas] matrix per quasar
                v = [np.ascontiguousarray(v[:, off[i]:off[i + 1]].T) for i in range(nsel)]
            elif f.kind == "row" and len(f.trailing or ()) == 2:   # sample_coefficients: one [S x k] matrix per quasar
                v = [np.ascontiguousarray(v[i]) for i in range(nsel)]
            w.put(f.name, v)
    finally:
        w.close()


def save_model_spectra(path: str, spectra: dict, **run_metadata) -> None:
    """What :func:`api.model_spectra` returns as a ``-v7.3`` file: ``quasar_ind`` (the selection, 1-based
    like every MATLAB index), ``num_pixels`` and ``status`` as columns, the selected absorbers as the
    cells ``map_z_dlas`` / ``map_log_nhis`` (when ``absorber_offsets``, ``absorber_z_dlas`` and
    ``absorber_log_nhis`` are present), and each per-pixel product as a ragged N x 1 cell array with
    one column vector per selected quasar (a quasar with no pixel in the modelled range holds an empty
    one; an empty selection gives empty cells).  The products of ``multi_models`` are written beside them
    when present: the sub-DLA and expected rows as such cells, ``mean_absorption_models`` /
    ``var_absorption_models`` as cells of [pixels x max_dlas] matrices, ``model_flags`` as a column.
    ``run_metadata``: scalars and strings, as given."""
    _save_grid_product(path, spectra, ("model_spectra", "model_spectra_multi", "multi_models"), run_metadata)


def save_marginal_continuum(path: str, mc: dict, **run_metadata) -> None:
    """What :func:`api.marginal_continuum` returns as a ``-v7.3`` file, in the layout of
    :func:`save_model_spectra`: ``quasar_ind`` (1-based), ``num_pixels`` and ``status`` as columns, the three
    per-pixel arrays as ragged N x 1 cell arrays, ``coef_mean`` [N x k], ``coef_cov_within`` and
    ``coef_cov_between`` [N x k (k + 1) / 2] (packed lower triangles, row by row) and, when present,
    ``model_weights`` [N x 3] as matrices and ``sample_coefficients`` as a cell of [S x k] matrices.  With
    ``multi_models`` the same cells hold the mixture over all models, ``model_weights`` is [N x (2 + max_dlas)] and
    ``model_flags`` is an extra column.  :func:`load_model_spectra` reads it."""
    _save_grid_product(path, mc, ("marginal_continuum", "multi_models"), run_metadata)


def save_absorption_distribution(path: str, dist: dict, thresholds=(), levels=(), num_bins: int = 0, **run_metadata) -> None:
    """What :func:`api.absorption_distribution` returns as a ``-v7.3`` file, in the layout of :func:`save_marginal_continuum`:
    ``prob_below``, ``quantiles`` and ``histogram`` as cells of ``[pixels x D]`` matrices (D thresholds, levels, bins),
    ``absorption_min`` / ``absorption_max`` as cells of column vectors, and the ``thresholds``, ``levels`` and ``num_bins`` the
    call was made with, so that the file explains its own columns."""
    meta = dict(run_metadata, thresholds=np.asarray(thresholds, dtype=np.float64).reshape(-1),
                levels=np.asarray(() if levels is None else levels, dtype=np.float64).reshape(-1), num_bins=np.float64(num_bins))
    _save_grid_product(path, dist, ("absorption_distribution", "multi_models"), meta)


def save_predictive_flux(path: str, pf: dict, **run_metadata) -> None:
    """What :func:`api.predictive_flux` returns as a ``-v7.3`` file, in the layout of :func:`save_marginal_continuum`:
    ``quasar_ind`` (1-based), ``num_pixels`` and ``status`` as columns, the five per-pixel arrays (and ``residual``
    when present) as ragged N x 1 cell arrays, ``chi2`` and ``num_kept`` as columns and ``model_weights`` [N x 3] as a
    matrix when present ([N x (2 + max_dlas)], with ``model_flags`` as an extra column, for ``multi_models``).
    :func:`load_predictive_flux` reads it."""
    _save_grid_product(path, pf, ("predictive_flux", "multi_models"), run_metadata)


def load_predictive_flux(path: str) -> dict:
    """The reader of :func:`save_predictive_flux`: :func:`load_model_spectra`'s layout (``selection`` 0-based,
    ``offsets``, ``status``, the per-pixel products as LISTS of per-quasar vectors), ``chi2`` flat and ``num_kept`` as
    integers."""
    out = load_model_spectra(path)
    if "chi2" in out:
        out["chi2"] = _vec(out["chi2"])
    if "num_kept" in out:
        out["num_kept"] = _vec(out["num_kept"]).astype(np.int64)
    return out


def load_model_spectra(path: str) -> dict:
    """The reader of :func:`save_model_spectra`: ``selection`` (0-based), ``offsets``, ``status``, every
    stored product as a LIST of per-quasar vectors, the absorbers as lists, the metadata as stored."""
    m = loadmat73(path)
    out = {}
    for k, v in m.items():
        if k == "quasar_ind":
            out["selection"] = _vec(v).astype(np.int64) - 1
        elif k == "num_pixels":
            out["offsets"] = np.concatenate([[0], np.cumsum(_vec(v).astype(np.int64))])
        elif k == "status":
            out["status"] = _vec(v).astype(np.int32)
        elif isinstance(v, list) and k in MODEL_SPECTRA_MULTI_PLANE_CELLS + ("sample_coefficients",):   # matrices per quasar
            out[k] = [np.asarray(c, dtype=np.float64) for c in v]
        elif isinstance(v, list):
            out[k] = [_vec(c) for c in v]
        else:
            out[k] = v
    return out


# ---------------------------------------------------------------------------------------------
# parameter summaries
# ---------------------------------------------------------------------------------------------

PARAMETER_SUMMARY_FIELDS = ("mean_z", "std_z", "mean_log_nhi", "std_log_nhi", "cov", "correlation", "quantiles_z",
                            "quantiles_log_nhi", "exceedance", "effective_samples")


def save_parameter_summaries(path: str, summaries: dict, **run_metadata) -> None:
    """What :mod:`posteriors` returns as a ``-v7.3`` file: ``quasar_ind`` (the selection, 1-based like
    every MATLAB index), ``probabilities`` and ``thresholds`` as columns, ``status`` and
    ``effective_samples`` [n x models], every other field as MATLAB sees this package's array --
    [n x model x slot], the quantiles [n x model x slot x probability], the exceedance [n x model x
    slot x threshold].  ``run_metadata``: scalars and strings, as given."""
    n = np.asarray(summaries["status"]).shape[0]
    w = _MatWriter(path)
    try:
        for k, v in run_metadata.items():
            w.put(k, v)
        w.put("quasar_ind", np.asarray(summaries.get("selection", np.arange(n)), dtype=np.float64).reshape(-1, 1) + 1)
        w.put("probabilities", np.asarray(summaries["probabilities"], dtype=np.float64).reshape(-1, 1))
        w.put("thresholds", np.asarray(summaries["thresholds"], dtype=np.float64).reshape(-1, 1))
        w.put("status", np.asarray(summaries["status"], dtype=np.float64))
        for k in PARAMETER_SUMMARY_FIELDS:
            if k in summaries:
                w.put(k, np.asarray(summaries[k], dtype=np.float64))
    finally:
        w.close()


def load_parameter_summaries(path: str) -> dict:
    """The reader of :func:`save_parameter_summaries`: this package's shapes again, ``selection``
    0-based, ``status`` int32."""
    m = loadmat73(path)
    out = {}
    for k, v in m.items():
        if k == "quasar_ind":
            out["selection"] = _vec(v).astype(np.int64) - 1
        elif k in ("probabilities", "thresholds"):
            out[k] = _vec(v).astype(np.float64)
        elif k == "status":
            out[k] = np.asarray(v).astype(np.int32)
        else:
            out[k] = v
    return out


# ---------------------------------------------------------------------------------------------
# posterior maps
# ---------------------------------------------------------------------------------------------

POSTERIOR_MAPS_FIELDS = ("mass", "hpd_level", "outside", "hpd_threshold", "intensity", "expected_absorbers", "grid",
                         "edges_z", "edges_log_nhi", "marginal_z", "marginal_log_nhi")
POSTERIOR_MAPS_INT_FIELDS = ("mode", "hpd_cells", "status")


def save_posterior_maps(path: str, maps: dict, **run_metadata) -> None:
    """What :func:`posteriors.posterior_maps` / ``maps_from_processed_file`` / :meth:`api.Batch.posterior_maps`
    return as a ``-v7.3`` file: ``quasar_ind`` (the selection, 1-based), ``levels`` and ``map_shape`` as
    columns, every array present as MATLAB sees this package's array ([n x model x slot x nz x nn] ...);
    ``mode`` stays the 0-based flat index cz * nn + cn (-1: none).  ``run_metadata``: scalars and strings."""
    n = np.asarray(maps["status"]).shape[0]
    w = _MatWriter(path)
    try:
        for k, v in run_metadata.items():
            w.put(k, v)
        w.put("quasar_ind", np.asarray(maps.get("selection", np.arange(n)), dtype=np.float64).reshape(-1, 1) + 1)
        w.put("levels", np.asarray(maps["levels"], dtype=np.float64).reshape(-1, 1))
        w.put("map_shape", np.asarray(maps["shape"], dtype=np.float64).reshape(-1, 1))
        for k in POSTERIOR_MAPS_INT_FIELDS + POSTERIOR_MAPS_FIELDS:
            if k in maps:
                w.put(k, np.asarray(maps[k], dtype=np.float64))
    finally:
        w.close()


def load_posterior_maps(path: str) -> dict:
    """The reader of :func:`save_posterior_maps`: this package's shapes and integer types again."""
    m = loadmat73(path)
    nz, nn = (int(x) for x in _vec(m["map_shape"]))
    L = _vec(m["levels"]).size
    n = _vec(m["quasar_ind"]).size
    md = 1 if n == 0 else int(np.asarray(m["status"]).size // n)
    shapes = {"mass": (n, md, md, nz, nn), "hpd_level": (n, md, md, nz, nn), "outside": (n, md, md), "mode": (n, md, md),
              "hpd_cells": (n, md, md, L), "hpd_threshold": (n, md, md, L), "intensity": (n, nz, nn),
              "expected_absorbers": (n,), "status": (n, md), "grid": (n, 4), "edges_z": (n, nz + 1),
              "edges_log_nhi": (n, nn + 1), "marginal_z": (n, md, md, nz), "marginal_log_nhi": (n, md, md, nn)}
    out = {}
    for k, v in m.items():
        if k == "quasar_ind":
            out["selection"] = _vec(v).astype(np.int64) - 1
        elif k == "levels":
            out[k] = _vec(v).astype(np.float64)
        elif k == "map_shape":
            out["shape"] = _vec(v).astype(np.int64)
        elif k in shapes:   # (MATLAB drops trailing singleton axes)
            a = np.asarray(v).reshape(shapes[k])
            out[k] = a.astype(np.int32) if k in POSTERIOR_MAPS_INT_FIELDS else a.astype(np.float64)
        else:
            out[k] = v
    return out


# ---------------------------------------------------------------------------------------------
# refined absorber posteriors
# ---------------------------------------------------------------------------------------------

#: largest transposed piece of a refined sample table save_refined_results holds at a time
REFINED_SLAB_BYTES = 64 << 20


def save_refined_results(path: str, refined: dict, **run_metadata) -> None:
    """What :meth:`api.Batch.refine` / :func:`refine.refine_absorbers` return as a ``-v7.3`` file:
    ``quasar_ind`` (the selection, 1-based), the per-quasar scalars as columns, ``boxes`` [n x level x 4],
    ``status``, the two sample tables when present, and the refined parameter summaries (the dict under
    ``summaries``) with a ``summary_`` prefix.  When present, too: the refined model posteriors (``refine.POSTERIORS``,
    DESIGN.md 4.19) and the unit points ``refine_u`` / ``refine_v`` the tables were swept on.  ``run_metadata``:
    scalars and strings, as given."""
    from . import refine as _refine
    n = np.asarray(refined["status"]).shape[0]
    w = _MatWriter(path)
    try:
        for k, v in run_metadata.items():
            w.put(k, v)
        w.put("quasar_ind", np.asarray(refined.get("selection", np.arange(n)), dtype=np.float64).reshape(-1, 1) + 1)
        w.put("status", np.asarray(refined["status"], dtype=np.float64).reshape(-1, 1))
        w.put("boxes", np.asarray(refined["boxes"], dtype=np.float64))
        for k in _refine.SCALARS:
            w.put(k, np.asarray(refined[k], dtype=np.float64).reshape(-1, 1))
        for k in _refine.TABLES:
            if k in refined:  # streamed in slabs of sample columns: no transposed copy of the table
                a = np.asarray(refined[k], dtype=np.float64)
                step = max(1, REFINED_SLAB_BYTES // max(8 * a.shape[0], 1))
                if a.size:
                    w.put_streamed(k, a.shape, np.float64, (a[:, j:j + step].T for j in range(0, a.shape[1], step)))
                else:
                    w.put(k, a)
        for k in _refine.POSTERIORS + _refine.POINTS:
            if k in refined:
                a = np.asarray(refined[k], dtype=np.float64)
                w.put(k, a if a.ndim == 2 else a.reshape(-1, 1))
        for k, v in (refined.get("summaries") or {}).items():
            if k != "selection":
                w.put("summary_" + k, np.asarray(v, dtype=np.float64))
    finally:
        w.close()


def load_refined_results(path: str) -> dict:
    """The reader of :func:`save_refined_results`: this package's shapes again, ``selection`` 0-based,
    ``status`` int32, the summaries under ``summaries``."""
    from . import refine as _refine
    m = loadmat73(path)
    out, summ = {}, {}
    for k, v in m.items():
        if k == "quasar_ind":
            out["selection"] = _vec(v).astype(np.int64) - 1
        elif k == "status":
            out[k] = _vec(v).astype(np.int32)
        elif k in _refine.SCALARS or k in _refine.POINTS or k in ("p_no_dlas_refined", "p_dlas_refined"):
            out[k] = _vec(v).astype(np.float64)
        elif k == "refined":
            out[k] = _vec(v).astype(np.int32)
        elif k.startswith("summary_"):
            k = k[len("summary_"):]
            summ[k] = _vec(v).astype(np.float64) if k in ("probabilities", "thresholds") else \
                np.asarray(v).astype(np.int32) if k == "status" else v
        else:
            out[k] = v
    if summ:
        summ["selection"] = out["selection"]
        out["summaries"] = summ
    return out


# ---------------------------------------------------------------------------------------------
# absorbers refined slot by slot
# ---------------------------------------------------------------------------------------------

_CONDITIONAL_INT = {"status": np.int32, "discovered": np.int32, "num_absorbers": np.int64, "num_start": np.int64}


def save_conditional_results(path: str, conditional: dict, **run_metadata) -> None:
    """What :func:`conditional.refine_conditional` returns as a ``-v7.3`` file: every array under its own name
    ([nq x slot ...]; the per-quasar counts and ``probabilities`` as columns), integers as doubles; the history of
    the passes is not stored.  ``run_metadata``: scalars and strings, as given."""
    w = _MatWriter(path)
    try:
        for k, v in run_metadata.items():
            w.put(k, v)
        for k, v in conditional.items():
            if k == "history":
                continue
            a = np.asarray(v, dtype=np.float64)
            w.put(k, a.reshape(-1, 1) if a.ndim == 1 else a)
    finally:
        w.close()


def load_conditional_results(path: str) -> dict:
    """The reader of :func:`save_conditional_results`: this package's shapes and integer types again."""
    out = {}
    for k, v in loadmat73(path).items():
        if k in ("num_absorbers", "num_start", "probabilities"):
            v = _vec(v)
        out[k] = np.asarray(v).astype(_CONDITIONAL_INT[k]) if k in _CONDITIONAL_INT else v
    return out


# ---------------------------------------------------------------------------------------------
# chunk files of a sharded run (CDDF_analysis/sbatch_reunion.py:13-63)
# ---------------------------------------------------------------------------------------------

def chunk_filename(directory: str, test_set_name: str, lo: int, hi: int, multi: bool = False,
                   width: int = 6) -> str:
    """Name of the chunk holding quasars [lo, hi) (0-based positions within the run's ``test_ind``
    selection) of a sharded run: the reference's output name (process_qsos.m:246-248; multi
    :512-521) followed by the zero-padded range, so that sorting the names orders the chunks the
    way ``mat_combine`` must be handed them."""
    stem = f"processed_qsos_multi_meanflux{test_set_name}" if multi else f"processed_qsos_{test_set_name}"
    return f"{directory}/{stem}_{lo:0{width}d}-{hi:0{width}d}.mat"


#: largest piece combine_processed_chunks reads / writes at a time
COMBINE_SLAB_BYTES = 256 << 20


def combine_processed_chunks(paths, out_path: str, test_ind=None) -> None:
    """What ``mat_combine`` (CDDF_analysis/sbatch_reunion.py:13-63) does -- every variable whose
    quasar axis has the first chunk's length is concatenated along that axis, everything else is
    taken from the first chunk -- written as a MATLAB ``-v7.3`` file and streamed in slabs of at
    most 256 MB (``Dataset.read_slab``: memory-mapped for contiguous sources, chunk by chunk for the
    chunked tables the streamed writer produces; the 3-D tables of the multi-DLA driver,
    ``[max_dlas, S, nq]``, by (model, range of samples)), so that the 13 GB sample table of a DR12Q
    run -- 52 GB for four DLA models -- is never held in memory (the reference's script peaks at ~150 GB, sbatch_reunion.py:6-7).  ``test_ind``: the combined run's selection; by default the
    OR of the chunks' own masks (``mat_combine`` keeps the first chunk's, which then selects only
    that chunk's quasars)."""
    paths = list(paths)
    files = [hdf5.File(p) for p in paths]
    try:
        first = files[0]
        names = [k for k in first.keys() if not k.startswith("#")]
        sizes = []
        for f in files:
            sizes.append(int(f["p_dlas"].shape[-1]))
        w = hdf5.FileWriter(out_path, userblock=matlab_userblock())
        try:
            for name in names:
                ds = first[name]
                attrs = {k: v for k, v in ds.attrs.items()}
                if name == "test_ind":
                    mask = test_ind
                    if mask is None:
                        mask = np.zeros(ds.shape, dtype=bool)
                        for f in files:
                            mask |= f["test_ind"].read().astype(bool)
                    w.create_dataset(name, np.asarray(mask, dtype=np.uint8).reshape(ds.shape), attrs=attrs)
                    continue
                per_quasar = len(ds.shape) >= 1 and ds.shape[-1] == sizes[0] and all(
                    name in f and f[name].shape[:-1] == ds.shape[:-1] and f[name].shape[-1] == n
                    for f, n in zip(files, sizes))
                if not per_quasar or "MATLAB_empty" in attrs:
                    w.create_dataset(name, ds.read(), attrs=attrs)
                    continue
                total = sum(sizes)
                shape = ds.shape[:-1] + (total,)
                if len(shape) == 1:
                    w.create_dataset(name, np.concatenate([f[name].read() for f in files]), attrs=attrs)
                    continue
                # slab by slab: contiguous sources are memory-mapped, chunked ones (what
                # ProcessedStreamWriter writes) are read chunk row by chunk row.  2-D tables [S, nq]
                # go by ranges of the slowest dimension; 3-D tables [max_dlas, S, nq] -- whose slowest
                # dimension is the model, one "row" of it 13 GB for a DR12Q run -- by (model, range
                # of samples): consecutive pieces of the row-major bytes either way, <= 256 MB each
                sources = [f[name] for f in files]
                budget = COMBINE_SLAB_BYTES
                if len(shape) == 2:
                    row_bytes = shape[1] * ds.dtype.itemsize
                    step = max(1, budget // max(row_bytes, 1))
                    blocks = (np.concatenate([d.read_slab(i, i + step) for d in sources], axis=-1)
                              for i in range(0, shape[0], step))
                else:
                    row_bytes = int(np.prod(shape[2:])) * ds.dtype.itemsize
                    step = max(1, budget // max(row_bytes, 1))
                    blocks = (np.concatenate([d.read_slab(m_, m_ + 1, axis1=(i, i + step)) for d in sources], axis=-1)
                              for m_ in range(shape[0]) for i in range(0, shape[1], step))
                w.create_dataset_streamed(name, shape, ds.dtype, blocks, attrs=attrs, in_order=True)
        finally:
            w.close()
    finally:
        for f in files:
            f.close()
