"""gp_dla_detection_amd.validation against numbers the reference's own scoring code produced
(DESIGN.md 4.13).

* ``QSOLoader.make_ROC`` and ``make_MAP_comparison`` ran on the committed multi-DLA chunk files when
  tests/golden/make_consumer_fixtures.py was made; their outputs are in
  tests/golden/consumer/expected_qsoloader_multi.npz.
* ``QSOLoader.query_least_num_dlas`` and ``make_multi_confusion`` ran on the same loader with a seeded
  stand-in catalogue (tests/golden/make_validation_fixtures.py ->
  tests/golden/validation/multi_confusion.npz).

The reference is not needed here: only the numbers it computed are read.
"""
import glob
import json
import os

import numpy as np
import pytest

from gp_dla_detection_amd import io, mocks, validation

HERE = os.path.dirname(os.path.abspath(__file__))
CONS = os.path.join(HERE, "golden", "consumer")
VAL = os.path.join(HERE, "golden", "validation")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    chunks = sorted(glob.glob(os.path.join(CONS, "processed_qsos_multi_meanfluxsynth_[0-9]*.mat")))
    assert len(chunks) == 2
    out = str(tmp_path_factory.mktemp("validation") / "combined.mat")
    io.combine_processed_chunks(chunks, out)
    return io.load_processed_qsos(out), out


@pytest.fixture(scope="module")
def loader():
    return np.load(os.path.join(CONS, "expected_qsoloader_multi.npz"))


@pytest.fixture(scope="module")
def confusion():
    return np.load(os.path.join(VAL, "multi_confusion.npz"))


def test_roc_equals_the_references_make_roc(run, loader):
    """Ratios of integers: exact."""
    res, _ = run
    tpr, fpr = validation.roc(res, loader["concordance_real_index"], loader["concordance_real_index_los"])
    assert loader["roc_tpr"].size == 32
    np.testing.assert_array_equal(tpr, loader["roc_tpr"])
    np.testing.assert_array_equal(fpr, loader["roc_fpr"])
    assert len(set(tpr.tolist())) > 3 and len(set(fpr.tolist())) > 10   # a curve, not two points


def test_roc_with_ties_and_skipped_quasars():
    """The sort-based count against the reference's O(N^2) definition (:703-715) written out, on log odds
    with ties; a NaN sightline is left out."""
    rng = np.random.default_rng(3)
    n = 60
    lp = np.round(rng.normal(size=n), 1)           # many ties
    lp[7] = np.nan
    res = dict(log_posteriors_dla=lp, log_posteriors_no_dla=np.zeros(n))
    real = np.flatnonzero(rng.uniform(size=n) < 0.4)
    tpr, fpr = validation.roc(res, real, occams_razor=1.0)
    ok = ~np.isnan(lp)
    odds, has = lp[ok], np.isin(np.arange(n), real)[ok]
    rank = np.argsort(odds)
    odds, has = odds[rank], has[rank]
    want_t, want_f = [], []
    for o in odds:
        ind = odds >= o
        tp, fn, tn, fp = np.sum(has & ind), np.sum(has & ~ind), np.sum(~has & ~ind), np.sum(~has & ind)
        want_t.append(tp / (tp + fn))
        want_f.append(fp / (fp + tn))
    assert tpr.size == n - 1
    np.testing.assert_array_equal(tpr, want_t)
    np.testing.assert_array_equal(fpr, want_f)


def test_map_comparison_equals_the_references(run, loader):
    """A single subtraction each: 1e-15."""
    res, _ = run
    dz, dn = validation.map_comparison(res, loader["concordance_real_index"], loader["concordance_z_dlas"],
                                       loader["concordance_log_nhis"])
    assert loader["map_comparison_dz"].size >= 1
    assert dz.shape == loader["map_comparison_dz"].shape
    np.testing.assert_allclose(dz, loader["map_comparison_dz"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(dn, loader["map_comparison_dlognhi"], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(validation.map_model_index(res), loader["dla_map_model_index"])


def _truth_of(fix, nq):
    """The stand-in catalogue as a CSR truth table over the run's quasars."""
    idx = fix["truth_index"]
    off = np.zeros(nq + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx, minlength=nq), out=off[1:])
    order = np.argsort(idx, kind="stable")
    return off, fix["truth_z_dlas"][order], fix["truth_log_nhis"][order]


def test_least_num_dlas_equals_the_references(run, confusion):
    res, _ = run
    mp = validation.occams_model_posteriors(res["model_posteriors"])
    for j, t in enumerate(confusion["p_threshes"]):
        got = [validation.least_num_dlas(row, float(t), sub_dla=True) for row in mp]
        np.testing.assert_array_equal(got, confusion["least_num_dlas"][j])
    # the fixture exercises the downward re-evaluation: a count found only after a model was removed
    assert confusion["downward_used"].any(axis=1).all()
    assert validation.least_num_dlas([0.1, 0.1, 0.5, 0.3], 0.6, sub_dla=True) == 1      # 0.5 / 0.7 > 0.6
    assert validation.least_num_dlas([0.6, 0.2, 0.1, 0.1], 0.9, sub_dla=True) == 0


def test_multi_confusion_equals_the_references(run, confusion):
    res, _ = run
    nq = res["p_dlas"].size
    truth = _truth_of(confusion, nq)
    sightlines = confusion["sightlines"]
    assert sightlines.size < nq                      # quasars without a catalogue entry are not scored
    beyond = False
    for j, t in enumerate(confusion["p_threshes"]):
        for lyb in (0, 1):
            for m, mn in enumerate(confusion["min_log_nhis"]):
                conf, counts = validation.multi_confusion(res, truth, confusion["z_qsos"], sightlines, p_thresh=float(t),
                                                          lyb=bool(lyb), min_log_nhi=float(mn))
                np.testing.assert_array_equal(conf, confusion[f"confusion_{j}_{lyb}_{m}"])
                np.testing.assert_array_equal(counts[:, 0], sightlines)
                np.testing.assert_array_equal(counts[:, 1:], confusion[f"counts_{j}_{lyb}_{m}"])
                assert conf.shape == (4, 4) and conf.sum() == sightlines.size
                beyond |= bool((counts[:, 2] >= 4).any())
    assert beyond                                    # one quasar's truth count exceeds the matrix size
    # the cuts matter: the Ly-beta cut and the column-density cut each change some matrix
    assert not np.array_equal(confusion["confusion_0_0_0"], confusion["confusion_0_1_0"])
    assert not np.array_equal(confusion["confusion_0_0_0"], confusion["confusion_0_0_1"])


def test_completeness_by_log_nhi_counts():
    """Hand-built: three quasars, four true absorbers."""
    mp = np.array([[0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.1, 0.9]])
    z = np.full((3, 2, 2), np.nan)
    z[0, 0, 0], z[2, 1, :] = 2.5, (2.2, 2.8)
    res = dict(model_posteriors=mp, MAP_z_dlas=z, MAP_log_nhis=20 + z, log_posteriors_lls=np.zeros(3))
    truth = (np.array([0, 1, 2, 4]), np.array([2.5, 2.4, 2.2, 3.5]), np.array([20.5, 20.6, 21.2, 21.4]))
    c = validation.completeness_by_log_nhi(res, truth, [20.0, 21.0, 22.0], occams_razor=1.0)
    np.testing.assert_array_equal(c["total"], [2, 2])
    np.testing.assert_array_equal(c["found"], [1, 2])
    c = validation.completeness_by_log_nhi(res, truth, [20.0, 21.0, 22.0], max_dz=0.01, occams_razor=1.0)
    np.testing.assert_array_equal(c["found"], [1, 1])          # 3.5 has no MAP absorber nearby
    np.testing.assert_array_equal(c["completeness"], [0.5, 0.5])
    assert np.isnan(validation.completeness_by_log_nhi(res, truth, [22.0, 23.0])["completeness"]).all()


def test_command_prints_one_json_object(run, confusion, tmp_path, capsys):
    res, path = run
    nq = res["p_dlas"].size
    truth = _truth_of(confusion, nq)
    tfile = str(tmp_path / "truth.mat")
    mocks.save_truth(tfile, truth)
    for a, b in zip(mocks.load_truth(tfile), truth):
        np.testing.assert_array_equal(a, b)
    assert validation.main(["--processed", path, "--truth", tfile]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    got = json.loads(lines[0])
    want = json.loads(json.dumps(validation.score(res, truth)))
    assert got == want and got["num_quasars"] == nq
    assert np.array(got["confusion_matrix"]).sum() == nq and len(got["roc_tpr"]) == nq
