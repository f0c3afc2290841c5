"""The S/N of every searched sightline: the table ``cddf.DLAStatistics(..., snrs, snr_thresh=...)``
and ``python -m gp_dla_detection_amd.cddf --snrs F`` take (CDDF_analysis/calc_cddf.py, find_snr
:1167-1185 and compute_all_snrs :1220-1237, as they execute).  DESIGN.md section 4.14.

For searched quasar ``nn`` the pixels with ``wavelength > 1215.67 (1 + max_z_dlas[nn])`` are taken,
masked or not; flux below a tenth of the normaliser (of 1 when the preloaded file has no
``all_normalizers``) is raised to that tenth; ``snr = 1 / median(sqrt(noise_variance) / |flux|)``
with NumPy's median (NaN if any selected value is NaN or none is selected).  The pass over the
pixels runs on the GPU (k_sightline_snr: one block per sightline); there is no CPU fallback.

    python -m gp_dla_detection_amd.snrs PRELOADED PROCESSED OUT
"""
from __future__ import annotations

import numpy as np


def sightline_snrs(spectra, max_z_dlas, normalizers=None, device=0):
    """One S/N per sightline.  ``spectra``: a list of per-quasar dicts (wavelengths, flux,
    noise_variance) or the flat CSR dict of ``api.spectra_to_csr`` / ``PreloadedReader.read_csr``;
    ``max_z_dlas``: one per sightline (NaN: the sightline gets NaN); ``normalizers``: one per
    sightline, or None for the file set without ``all_normalizers``."""
    from . import _lib
    if isinstance(spectra, dict):
        offsets = np.ascontiguousarray(spectra["offsets"], dtype=np.int64).reshape(-1)
        flat = [np.ascontiguousarray(spectra[k], dtype=np.float64).reshape(-1)
                for k in ("wavelengths", "flux", "noise_variance")]
    else:
        sizes = [np.asarray(s["wavelengths"]).size for s in spectra]
        offsets = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=offsets[1:])
        flat = [np.ascontiguousarray(np.concatenate([np.asarray(s[k], dtype=np.float64).reshape(-1) for s in spectra])
                                     if sizes else np.zeros(0)) for k in ("wavelengths", "flux", "noise_variance")]
    n = offsets.size - 1
    if n < 0 or offsets[0] != 0 or np.any(np.diff(offsets) < 0):
        raise ValueError("offsets must start at 0 and not decrease")
    if any(a.size != offsets[-1] for a in flat):
        raise ValueError("wavelengths, flux and noise_variance need one entry per pixel")
    zmax = np.ascontiguousarray(max_z_dlas, dtype=np.float64).reshape(-1)
    if zmax.size != n:
        raise ValueError(f"{n} sightlines but {zmax.size} max_z_dlas")
    norm = None
    if normalizers is not None:
        norm = np.ascontiguousarray(normalizers, dtype=np.float64).reshape(-1)
        if norm.size != n:
            raise ValueError(f"{n} sightlines but {norm.size} normalizers")
    out = np.full(n, np.nan)
    if n == 0:
        return out
    pix = [a if a.size else np.zeros(1) for a in flat]
    lib = _lib.load()
    _lib.check(lib.gpdla_stats_sightline_snrs(n, offsets.ctypes.data_as(_lib._i64p), *[_lib.ptr(a) for a in pix],
                                              _lib.ptr(zmax), None if norm is None else _lib.ptr(norm), _lib.ptr(out),
                                              int(device)))
    return out


def compute_all_snrs(preloaded_file, processed_file, save_file, device=0, block=16384):
    """compute_all_snrs (:1220-1237): the S/N of the quasars the processed file's ``test_ind``
    selects, from the preloaded spectra, written as the ``snrs`` column DLACatalogue and QSOLoader
    read (``ff["snrs"][0, :]``).  The spectra are read and processed ``block`` sightlines at a
    time.  Returns the vector."""
    from . import hdf5, io
    small = io.loadmat73(processed_file, ["test_ind", "max_z_dlas"])
    real_index = np.flatnonzero(np.asarray(small["test_ind"]).reshape(-1) != 0)
    zmax = np.asarray(small["max_z_dlas"], dtype=np.float64).reshape(-1)
    if zmax.size != real_index.size:
        raise ValueError(f"test_ind selects {real_index.size} quasars but the file holds {zmax.size} max_z_dlas")
    with hdf5.File(preloaded_file) as f:
        has_norm = "all_normalizers" in f
    norm = None
    if has_norm:
        norm = np.asarray(io.loadmat73(preloaded_file, ["all_normalizers"])["all_normalizers"],
                          dtype=np.float64).reshape(-1)[real_index]
    snrs = np.empty(real_index.size)
    with io.PreloadedReader(preloaded_file) as r:
        z_unused = np.zeros(r.num_quasars)
        for lo in range(0, real_index.size, block):   # a block's pixels are read, uploaded and dropped
            hi = min(lo + block, real_index.size)
            csr = r.read_csr(real_index[lo:hi], z_unused)
            snrs[lo:hi] = sightline_snrs(csr, zmax[lo:hi], None if norm is None else norm[lo:hi], device=device)
    io.savemat73(save_file, dict(snrs=snrs.reshape(-1, 1)))
    return snrs


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gp_dla_detection_amd.snrs",
                                 description="the S/N table of a processed run's searched sightlines")
    ap.add_argument("preloaded")
    ap.add_argument("processed")
    ap.add_argument("out")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    snrs = compute_all_snrs(a.preloaded, a.processed, a.out, device=a.device)
    print(f"{snrs.size} sightlines, {int(np.isfinite(snrs).sum())} finite S/N -> {a.out}")


if __name__ == "__main__":
    main()
