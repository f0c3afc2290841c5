"""Preloading the spectra: SDSS ``spec-PLATE-MJD-FIBER.fits`` files -> ``preloaded_qsos.mat`` and the
catalogue's new ``filter_flags`` (preload_qsos.m with read_spec.m as its ``file_loader``).  DESIGN.md
section 4.16.

The files are read on the host (csrc/fitsspec.c over up to 16 threads, or the Python reader of
:mod:`.fits`); everything after that -- wavelengths, noise variance, the pixel mask, the normaliser,
both flags, the normalisation and the cut to the loading range with one unmasked pixel either side --
is one pass of k_preload on the GPU, one block per spectrum.  There is no CPU fallback for that pass.
The catalogue is worked through in blocks of 16 384 quasars: neither the raw columns nor the
output are ever whole in memory.

    python -m gp_dla_detection_amd.preload CATALOG SPECTRA_DIR OUT_PRELOADED OUT_CATALOG
"""
from __future__ import annotations

import os

import numpy as np

from .parameters import Parameters

BLOCK = 16384


def spec_filename(spectra_dir, plate, mjd, fiber_id) -> str:
    """``SPECTRA_DIR/PLATE/spec-PLATE-MJD-FIBER.fits`` with the fibre zero-padded to four digits."""
    return "%s/%i/spec-%i-%i-%04i.fits" % (spectra_dir, int(plate), int(plate), int(mjd), int(fiber_id))


def _config(params):
    from . import _lib
    p = params or Parameters()
    return _lib.PreloadConfig(p.loading_min_lambda, p.loading_max_lambda, p.normalization_min_lambda,
                              p.normalization_max_lambda, p.min_lambda, p.max_lambda, int(p.min_num_pixels))


def preload_raw(raw: dict, z_qsos, filter_flags, params: Parameters | None = None, device: int = 0) -> dict:
    """k_preload on a raw CSR set (``offsets``, float32 ``flux`` / ``loglam`` / ``ivar``, int32
    ``and_mask``: what ``fits.read_spec_files`` returns).  Returns the dict of
    ``PreloadedReader.read_csr`` (offsets, wavelengths, flux, noise_variance, pixel_mask, z_qsos) plus
    ``all_normalizers`` and the updated ``filter_flags``.  A quasar flagged on entry or here holds no
    pixel and normaliser 0."""
    from . import _lib
    offsets = np.ascontiguousarray(raw["offsets"], dtype=np.int64).reshape(-1)
    n = offsets.size - 1
    if n < 0 or offsets[0] != 0 or np.any(np.diff(offsets) < 0):
        raise ValueError("offsets must start at 0 and not decrease")
    total = int(offsets[-1])
    cols = [np.ascontiguousarray(raw[k], dtype=dt).reshape(-1)
            for k, dt in (("flux", np.float32), ("loglam", np.float32), ("ivar", np.float32), ("and_mask", np.int32))]
    if any(c.size != total for c in cols):
        raise ValueError("flux, loglam, ivar and and_mask need one entry per pixel")
    z = np.ascontiguousarray(z_qsos, dtype=np.float64).reshape(-1)
    flags = np.array(filter_flags, dtype=np.uint8).reshape(-1)   # a copy: the call updates it
    if z.size != n or flags.size != n:
        raise ValueError(f"{n} quasars but {z.size} redshifts and {flags.size} filter_flags")
    cfg = _config(params)
    out_off = np.zeros(n + 1, dtype=np.int64)
    room = max(total, 1)
    w, f, nv = (np.empty(room, dtype=np.float64) for _ in range(3))
    m = np.empty(room, dtype=np.uint8)
    norm = np.zeros(max(n, 1), dtype=np.float64)
    if n:
        import ctypes as C
        lib = _lib.load()
        f32 = lambda a: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(_lib._f32p)
        and_mask = cols[3] if total else np.zeros(1, np.int32)
        _lib.check(lib.gpdla_preload_spectra(n, offsets.ctypes.data_as(_lib._i64p), f32(cols[0]), f32(cols[1]), f32(cols[2]),
                                             and_mask.ctypes.data_as(_lib._i32p), _lib.ptr(z), flags.ctypes.data_as(_lib._u8p),
                                             C.byref(cfg), out_off.ctypes.data_as(_lib._i64p), _lib.ptr(w), _lib.ptr(f),
                                             _lib.ptr(nv), m.ctypes.data_as(_lib._u8p), _lib.ptr(norm), int(device)))
    kept = int(out_off[-1])
    return dict(offsets=out_off, wavelengths=w[:kept].copy(), flux=f[:kept].copy(), noise_variance=nv[:kept].copy(),
                pixel_mask=m[:kept].copy(), z_qsos=z.copy(), all_normalizers=norm[:n].copy(), filter_flags=flags)


def preload_csr(spectra_dir, plates, mjds, fiber_ids, z_qsos, filter_flags, params: Parameters | None = None,
                device: int = 0, native=None) -> dict:
    """One block of quasars from their spec files: the files of the quasars whose ``filter_flags`` is 0
    are read (a flagged quasar's file is not opened), then :func:`preload_raw`.  The result goes
    straight to a batch upload or to ``io.PreloadedStreamWriter.append``."""
    from . import fits
    flags = np.asarray(filter_flags).reshape(-1)
    paths = [None if flags[i] > 0 else spec_filename(spectra_dir, plates[i], mjds[i], fiber_ids[i])
             for i in range(flags.size)]
    raw = fits.read_spec_files(paths, native=native)
    return preload_raw(raw, z_qsos, flags, params, device)


def preload_qsos(catalog_file, spectra_dir, out_preloaded, out_catalog, params: Parameters | None = None,
                 device: int = 0, block: int = BLOCK, native=None) -> dict:
    """preload_qsos.m: ``catalog_file`` (z_qsos, plates, mjds, fiber_ids, filter_flags) + the spec files
    under ``spectra_dir`` -> ``out_preloaded`` (the variables of :73-77) and ``out_catalog``, a NEW file
    with the plain per-quasar columns of the catalogue and the updated ``filter_flags``.  The input
    catalogue is never written to.  Returns ``filter_flags`` and ``all_normalizers``."""
    from . import io
    p = params or Parameters()
    if os.path.exists(out_catalog) and os.path.samefile(catalog_file, out_catalog):
        raise ValueError("OUT_CATALOG must not be the input catalogue: that file is never modified")
    cat = io.load_catalog(catalog_file)
    need = ("z_qsos", "plates", "mjds", "fiber_ids", "filter_flags")
    missing = [k for k in need if not isinstance(cat.get(k), np.ndarray)]
    if missing:
        raise KeyError(f"{catalog_file} lacks {missing}")
    n = cat["z_qsos"].size
    if any(cat[k].size != n for k in need):
        raise ValueError(f"{catalog_file}: the per-quasar columns differ in length")
    flags = cat["filter_flags"].astype(np.uint8)
    norm = np.zeros(n)
    w = io.PreloadedStreamWriter(out_preloaded, p)
    try:
        for lo in range(0, n, max(1, int(block))):   # a block's raw columns and output are dropped after it
            hi = min(lo + max(1, int(block)), n)
            b = preload_csr(spectra_dir, cat["plates"][lo:hi], cat["mjds"][lo:hi], cat["fiber_ids"][lo:hi],
                            cat["z_qsos"][lo:hi], flags[lo:hi], p, device, native)
            flags[lo:hi] = b["filter_flags"]
            norm[lo:hi] = b["all_normalizers"]
            w.append(b)
    except BaseException:
        w.abort()
        raise
    w.finish()
    columns = {k: v.reshape(-1, 1) for k, v in cat.items() if isinstance(v, np.ndarray) and v.size == n}
    columns["filter_flags"] = flags.reshape(-1, 1)
    io.savemat73(out_catalog, columns)
    return dict(filter_flags=flags, all_normalizers=norm)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gp_dla_detection_amd.preload",
                                 description="preloaded_qsos.mat and the new filter_flags from SDSS spec files")
    ap.add_argument("catalog")
    ap.add_argument("spectra_dir")
    ap.add_argument("out_preloaded")
    ap.add_argument("out_catalog")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--block", type=int, default=BLOCK, help="quasars read and processed at a time")
    a = ap.parse_args(argv)
    if not os.path.isfile(a.catalog):
        ap.error(f"no catalogue {a.catalog}")
    if not os.path.isdir(a.spectra_dir):
        ap.error(f"no directory {a.spectra_dir}")
    if a.block < 1:
        ap.error("--block must be at least 1")
    if os.path.exists(a.out_catalog) and os.path.samefile(a.catalog, a.out_catalog):
        ap.error("OUT_CATALOG must not be the input catalogue: that file is never modified")
    out = preload_qsos(a.catalog, a.spectra_dir, a.out_preloaded, a.out_catalog, device=a.device, block=a.block)
    f = out["filter_flags"]
    print(f"{f.size} quasars, {int((f == 0).sum())} loaded, {int(((f & 4) > 0).sum())} without a normaliser, "
          f"{int(((f & 8) > 0).sum())} with too few pixels -> {a.out_preloaded}, {a.out_catalog}")


if __name__ == "__main__":
    main()
