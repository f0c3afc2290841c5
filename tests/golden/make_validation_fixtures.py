#!/opt/conda/bin/python3.9
"""BUILD CONTAINER ONLY: what the reference's own scoring code counts on this package's files.

    /opt/conda/bin/python3.9 tests/golden/make_validation_fixtures.py

Run like make_consumer_fixtures.py (same interpreter, same inputs: the committed multi-DLA chunk files
of tests/golden/consumer/, recombined by the reference's ``mat_combine`` and opened by its
``QSOLoader``).  Calls ``QSOLoader.query_least_num_dlas`` (qso_loader.py:838-859) and
``QSOLoader.make_multi_confusion`` (:878-965) with a small seeded stand-in for Parks' catalogue and
stores what they returned -- only numbers -- in ``tests/golden/validation/multi_confusion.npz``;
tests/test_validation.py then checks, without the reference, that
``gp_dla_detection_amd.validation`` counts the same.

The stand-in catalogue: every third searched quasar has no entry (the reference does not score it,
:912), the others have 1 .. 3 entries near or away from their MAP absorbers, one quasar has 6 strong
entries (more than the matrix has columns, :959-960); every confidence is 1 (a truth table has none).
"""
import glob
import os
import sys
import tempfile
from collections import namedtuple

import numpy as np

np.bool, np.int, np.float, np.long = bool, int, float, int  # aliases the reference still uses

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "validation")
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

import make_consumer_fixtures as mcf  # noqa: E402  (make_inputs, reference_combine: the same inputs)
from CDDF_analysis import qso_loader  # noqa: E402

P_THRESHES = (0.98, 0.9, 0.6, 0.35)
MIN_LOG_NHIS = (20.3, 21.0)


def stand_in_catalogue(q, seed=20260117):
    rng = np.random.default_rng(seed)
    nq = q.z_qsos.size
    index, z, n = [], [], []
    for i in range(nq):
        if i % 3 == 2:
            continue
        count = 6 if i == 4 else int(rng.integers(1, 4))
        lo, hi = q.min_z_dlas[i], q.max_z_dlas[i]
        for j in range(count):
            index.append(i)
            z.append(rng.uniform(lo, hi) if i != 4 else rng.uniform(0.5 * (lo + hi), hi))
            n.append(rng.uniform(19.9, 22.0) if i != 4 else rng.uniform(21.2, 22.0))
    index = np.array(index)
    Catalogue = namedtuple("Catalogue", ["raw_unique_ids", "raw_dla_confidences", "raw_z_dlas", "raw_log_nhis"])
    return index, Catalogue(q.unique_ids[index], np.ones(index.size), np.array(z), np.array(n))


def main():
    os.makedirs(OUT, exist_ok=True)
    with tempfile.TemporaryDirectory() as d:
        mcf.make_inputs(d)
        chunks = sorted(glob.glob(os.path.join(mcf.OUT, "processed_qsos_multi_meanfluxsynth_[0-9]*.mat")))
        assert len(chunks) == 2, chunks
        combined = os.path.join(d, "combined_multi.h5")
        mcf.reference_combine(chunks, combined)
        q = qso_loader.QSOLoader(
            preloaded_file=f"{d}/preloaded_qsos.mat", catalogue_file=f"{d}/catalog.mat",
            learned_file=f"{d}/learned_qso_model_synthetic.mat", processed_file=combined,
            dla_concordance=f"{d}/dla_catalog", los_concordance=f"{d}/los_catalog",
            snrs_file=f"{d}/snrs_qsos.mat", sub_dla=True, sample_file=f"{d}/dla_samples.mat", occams_razor=10000)
        q.unique_ids = q.make_unique_id(q.plates, q.mjds, q.fiber_ids)   # as load_dla_parks does (:493)
        index, cat = stand_in_catalogue(q)
        keep = dict(truth_index=index, truth_z_dlas=cat.raw_z_dlas, truth_log_nhis=cat.raw_log_nhis,
                    sightlines=np.flatnonzero(np.isin(q.unique_ids, cat.raw_unique_ids)),
                    p_threshes=np.array(P_THRESHES), min_log_nhis=np.array(MIN_LOG_NHIS), z_qsos=np.asarray(q.z_qsos))
        least = np.array([[q.query_least_num_dlas(np.asarray(row), t) for row in q.model_posteriors] for t in P_THRESHES])
        keep["least_num_dlas"] = least
        top = np.asarray(q.model_posteriors)[:, -1]
        keep["downward_used"] = np.array([(top <= t) & (least[j] > 0) for j, t in enumerate(P_THRESHES)])
        for j, t in enumerate(P_THRESHES):
            for lyb in (False, True):
                for m, mn in enumerate(MIN_LOG_NHIS):
                    conf, uid = q.make_multi_confusion(cat, dla_confidence=0.98, p_thresh=t, lyb=lyb, min_log_nhi=mn)
                    assert np.array_equal(uid[:, 0], q.unique_ids[keep["sightlines"]])
                    keep[f"confusion_{j}_{int(lyb)}_{m}"] = np.asarray(conf)
                    keep[f"counts_{j}_{int(lyb)}_{m}"] = np.asarray(uid[:, 1:], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "multi_confusion.npz"), **keep)
    print("downward re-evaluation used:", keep["downward_used"].sum(axis=1), "true counts up to",
          max(int(keep[k][:, 1].max()) for k in keep if k.startswith("counts_")))


if __name__ == "__main__":
    main()
