#!/opt/conda/bin/python3.9
"""BUILD CONTAINER ONLY: the S/N table the reference computes for the synthetic file set.

    /opt/conda/bin/python3.9 tests/golden/make_snr_fixtures.py

Run under the interpreter that has h5py, as make_consumer_fixtures.py (whose helpers it uses: the
seeded file set written by ``gp_dla_detection_amd.synthetic.write_file_set`` and the committed
single-DLA chunk files combined by the reference's own mat_combine).  It calls the reference's
``calc_cddf.compute_all_snrs`` (:1220-1237, find_snr :1167-1185) on three preloaded files and stores
what it wrote, with the ``max_z_dlas`` and ``test_ind`` it read, in tests/golden/snrs/*.npz:

  a  the file set as written: no ``all_normalizers``, masked pixels carry NaN flux
  b  the same with an ``all_normalizers`` dataset (tests/snr_restatement.set_b_normalizers)
  c  every masked pixel given a finite flux below the floor and a finite noise variance
     (tests/snr_restatement.set_c_fill), so the selections hold no NaN

Nothing of the reference is copied: only numbers it computed travel."""
import glob
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_consumer_fixtures as mcf  # noqa: E402  (puts the reference on sys.path, defines the removed aliases)
import h5py  # noqa: E402
import snr_restatement as R  # noqa: E402
from CDDF_analysis import calc_cddf  # noqa: E402

OUT = os.path.join(HERE, "snrs")


def reference_snrs(preloaded, processed, d, tag):
    save = os.path.join(d, f"snrs_{tag}.h5")
    with np.errstate(all="ignore"):
        calc_cddf.compute_all_snrs(raw_file=preloaded, processed_file=processed, save_file=save)
    with h5py.File(save, "r") as f:
        return np.array(f["snrs"])


def floor_hits(preloaded, real_index, max_z):
    """How many selected pixels of the file lie below the flux floor (no normalisers)."""
    hits = 0
    with h5py.File(preloaded, "r") as hh:
        for nn, i in enumerate(real_index):
            wl = hh[hh["all_wavelengths"][0][i]][0]
            fl = hh[hh["all_flux"][0][i]][0]
            hits += int(np.count_nonzero(fl[wl > R.LYA * (1 + max_z[nn])] < R.FLOOR))
    return hits


def main():
    os.makedirs(OUT, exist_ok=True)
    report = {}
    with tempfile.TemporaryDirectory() as d:
        mcf.make_inputs(d)
        chunks = sorted(glob.glob(os.path.join(mcf.OUT, "processed_qsos_synth_[0-9]*.mat")))
        assert len(chunks) == 2, chunks
        processed = os.path.join(d, "combined_single.h5")
        mcf.reference_combine(chunks, processed)
        with h5py.File(processed, "r") as f:
            test_ind = np.array(f["test_ind"][0] != 0)
            max_z = np.array(f["max_z_dlas"][0])
        real_index = np.flatnonzero(test_ind)
        base = os.path.join(d, "preloaded_qsos.mat")
        files = dict(a=base, b=os.path.join(d, "preloaded_b.mat"), c=os.path.join(d, "preloaded_c.mat"))
        shutil.copy(base, files["b"])
        norm = R.set_b_normalizers(test_ind.size)
        with h5py.File(files["b"], "r+") as hh:
            hh["all_normalizers"] = norm.reshape(1, -1)
        shutil.copy(base, files["c"])
        with h5py.File(files["c"], "r+") as hh:
            for i in range(test_ind.size):
                masked = np.array(hh[hh["all_pixel_mask"][0][i]][0]) != 0
                fill_f, fill_v = R.set_c_fill(masked.size)
                for key, fill in (("all_flux", fill_f), ("all_noise_variance", fill_v)):
                    ds = hh[hh[key][0][i]]
                    ds[0, :] = np.where(masked, fill, ds[0])
        for tag, path in files.items():
            snrs = reference_snrs(path, processed, d, tag)
            assert snrs.shape == (real_index.size,)
            finite = int(np.isfinite(snrs).sum())
            extra = dict(normalizers=norm) if tag == "b" else {}
            np.savez_compressed(os.path.join(OUT, f"set_{tag}.npz"), snrs=snrs, max_z_dlas=max_z, test_ind=test_ind, **extra)
            report[tag] = dict(sightlines=int(snrs.size), finite=finite, nan=int(np.isnan(snrs).sum()))
        assert report["a"]["finite"] >= 8 and report["a"]["nan"] >= 8, report
        assert report["c"]["finite"] * 4 >= 3 * report["c"]["sightlines"], report
        report["c"]["selected_pixels_below_floor"] = floor_hits(files["c"], real_index, max_z)
        assert report["c"]["selected_pixels_below_floor"] >= 1, report
    report["versions"] = dict(python=sys.version.split()[0], numpy=np.__version__, h5py=h5py.__version__)
    with open(os.path.join(OUT, "report.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
