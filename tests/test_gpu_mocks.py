"""GPU checks of the mock spectra: the draw against the NumPy-and-oracle restatement
(tests/mock_restatement.py), what is left alone, determinism and batch invariance, the closed loop
draw -> sweep against the oracle, the whitened statistics of the GPU's own flux, recovery, and the
file-to-file commands.  Every figure is printed before it is asserted.

The recovery set (mock_restatement.recovery_case: 24 BOSS-grid templates, every third without an
absorber) was first drawn with the restatement ALONE, under the Philox streams of MOCK_SEED, and swept by
the oracle on the CPU with the prior p_DLA = 0.1: the 8 clean quasars got log odds between -811.2 and
-560.5, the 16 injected ones between +69.7 and +2791.8 (the weakest: log N_HI = 21.90 at the very blue
end of a short spectrum); MAP z_DLA within 0.0026 of the truth and MAP log N_HI within 0.21; whitened
chi^2 21 206.0 for 21 100 pixels (+0.52 sigma), Q2 = 442.6 for 480 (-1.21 sigma).  The first seed tried
met the condition "every clean quasar below -10, every injected one above +10", so it was kept.
"""
import json
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import api, io, mocks, synthetic, validation
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import mock_restatement as R
from test_gpu_multi import compare as compare_multi, oracle_multi

pytestmark = pytest.mark.gpu

TOL_NORMAL = 1e-13    # log, cos, sqrt on identical arguments: ~1.2e-14 at |n| <= 8.58, times 10
TOL_MAP = 1e-12       # the project's tolerance of a product of broadened profiles (tests/test_gpu_model_spectra.py)
TOL_DRAW = 1e-11      # x max(1, |value|): 10 x the per-profile tolerance, for the dot product, the 1e-13
                      # interpolation parity and the normal
TOL_LL = 1e-8         # the project's log-likelihood tolerance
SEED = R.MOCK_SEED


def _dev(a, b, relative=False) -> float:
    """max |a - b| (``relative``: over max(1, |b|)) with matching NaN patterns (inf otherwise)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return float("inf")
    ok = ~np.isnan(a)
    d = np.abs(a - b)[ok]
    if relative:
        d = d / np.maximum(1.0, np.abs(b[ok]))
    return float(d.max()) if d.size else 0.0


def _context(model, samples, params=None):
    ctx = gp.Context(0, params or Parameters())
    ctx.set_model(model)
    ctx.set_samples(samples)
    return ctx


def _upload(ctx, spectra):
    n = len(spectra)
    p = ctx.params
    if isinstance(p, MultiParameters):
        lp_dla = np.log(np.full((n, p.max_dlas), R.PRIOR_P_DLA) ** np.arange(1, p.max_dlas + 1))
        return ctx.upload(spectra, np.full(n, np.log(0.85)), lp_dla, np.full(n, np.log(0.05)))
    return ctx.upload(spectra, np.full(n, np.log(1 - R.PRIOR_P_DLA)), np.full(n, np.log(R.PRIOR_P_DLA)))


def _sizes(spectra):
    return np.concatenate([[0], np.cumsum([np.asarray(s["wavelengths"]).size for s in spectra])])


def _with_flux(spectra, flat):
    o = _sizes(spectra)
    return [dict(s, flux=flat[o[i]:o[i + 1]].copy()) for i, s in enumerate(spectra)]


@pytest.fixture(scope="module")
def case(oracle):
    return R.recovery_case(oracle)


@pytest.fixture(scope="module")
def mf_case(oracle):
    return R.meanflux_case(oracle)


@pytest.fixture(scope="module")
def drawn(case):
    """The recovery set drawn, left resident, swept, downloaded."""
    ctx = _context(case["model"], case["samples"])
    batch = _upload(ctx, case["templates"])
    try:
        res = batch.draw_mocks(case["truth"], seed=SEED, write_resident=True,
                               components=("absorption", "continuum", "sigma", "latents"))
        batch.process()
        out = batch.download()
    finally:
        batch.close()
        ctx.close()
    return res, out


# ------------------------------------------------------------------------------------------------
# 1. parity of the draw
# ------------------------------------------------------------------------------------------------

def _parity(oracle, c, res, meanflux, num_lines=3):
    o = _sizes(c["templates"])
    worst = dict(latents=0.0, absorption=0.0, flux=0.0, continuum=0.0, sigma=0.0)
    cells = {k: gp.split_cells(res[k], res["grid_offsets"]) for k in ("absorption", "continuum", "sigma")}
    for i, sp in enumerate(c["templates"]):
        z, ln = R.absorbers_of(c["truth"], i)
        want = R.draw(oracle, c["model"], sp, i, SEED, z, ln, meanflux=meanflux, num_lines=num_lines)
        assert res["status"][i] == want["status"] == 0
        worst["latents"] = max(worst["latents"], _dev(res["latents"][i], want["latents"]))
        worst["absorption"] = max(worst["absorption"], _dev(cells["absorption"][i], want["absorption"]))
        worst["flux"] = max(worst["flux"], _dev(res["flux"][o[i]:o[i + 1]], want["flux"], relative=True))
        for k in ("continuum", "sigma"):
            worst[k] = max(worst[k], _dev(cells[k][i], want[k], relative=True))
    return worst


def test_draw_equals_the_restatement(oracle, case, drawn):
    res, _ = drawn
    worst = _parity(oracle, case, res, meanflux=False)
    print("single-DLA rows, worst |delta|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert np.abs(res["latents"]).max() <= 8.58
    assert worst["latents"] < TOL_NORMAL
    assert worst["absorption"] < TOL_MAP
    assert max(worst["flux"], worst["continuum"], worst["sigma"]) < TOL_DRAW


def test_draw_equals_the_restatement_meanflux(oracle, mf_case):
    c = mf_case
    p = MultiParameters()
    ctx = _context(c["model"], c["samples"], p)
    batch = _upload(ctx, c["templates"])
    try:
        res = batch.draw_mocks(c["truth"], seed=SEED, write_resident=False,
                               components=("absorption", "continuum", "sigma", "latents"))
        single_rows = batch.draw_mocks(c["truth"], seed=SEED, write_resident=False, meanflux=False)
    finally:
        batch.close()
        ctx.close()
    assert np.diff(c["truth"][0]).max() == 3
    worst = _parity(oracle, c, res, meanflux=True)
    print("mean-flux rows, worst |delta|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["latents"] < TOL_NORMAL
    assert worst["absorption"] < TOL_MAP
    assert max(worst["flux"], worst["continuum"], worst["sigma"]) < TOL_DRAW
    assert _dev(res["flux"], single_rows["flux"]) > 1e-3     # the mean-flux rows are other rows


# ------------------------------------------------------------------------------------------------
# 2. what is left alone
# ------------------------------------------------------------------------------------------------

def test_what_is_left_alone(case):
    spectra = [dict(s) for s in case["templates"][:5]]
    dead = spectra[1]                                          # status 1: no kept pixel
    dead["pixel_mask"] = np.ones_like(dead["pixel_mask"])
    dead["flux"] = np.arange(dead["flux"].size, dtype=np.float64)
    bad = spectra[3]                                           # status 3: a kept pixel of noise variance 0
    bad["flux"] = np.where(bad["pixel_mask"] == 0, 0.25, np.nan)
    nv = bad["noise_variance"].copy()
    nv[np.flatnonzero(bad["pixel_mask"] == 0)[40]] = 0.0
    bad["noise_variance"] = nv
    for s in (spectra[0], spectra[2], spectra[4]):             # a recognisable template flux
        s["flux"] = np.where(s["pixel_mask"] == 0, -7.0 - np.arange(s["flux"].size), np.nan)
    ctx = _context(case["model"], case["samples"])
    batch = _upload(ctx, spectra)
    try:
        res = batch.draw_mocks(seed=SEED, write_resident=False, components=("continuum", "sigma", "latents", "absorption"))
    finally:
        batch.close()
        ctx.close()
    np.testing.assert_array_equal(res["status"], [0, 1, 0, 3, 0])
    o = _sizes(spectra)
    p = Parameters()
    cont = gp.split_cells(res["continuum"], res["grid_offsets"])
    for i, s in enumerate(spectra):
        got = res["flux"][o[i]:o[i + 1]]
        rest = s["wavelengths"] / (1 + s["z_qso"])
        inside = (rest >= p.min_lambda) & (rest <= p.max_lambda)
        assert (~inside).sum() >= 2
        if res["status"][i] != 0:
            np.testing.assert_array_equal(got, s["flux"])      # untouched (NaN for NaN)
            assert np.isnan(res["latents"][i]).all() and np.isnan(cont[i]).all()
            continue
        masked = s["pixel_mask"] != 0
        assert np.isnan(got[inside & masked]).all() and (inside & masked).sum() >= 1
        assert np.array_equal(got[~inside].view(np.uint64), s["flux"][~inside].view(np.uint64))   # bit-identical
        drawn_px = got[inside & ~masked]
        assert np.isfinite(drawn_px).all() and (drawn_px > -5).all()                                # none is the template
        assert np.array_equal(np.isnan(cont[i]), masked[inside])
        assert (gp.split_cells(res["absorption"], res["grid_offsets"])[i] == 1.0).all()             # no absorbers


# ------------------------------------------------------------------------------------------------
# 3. determinism and batch invariance
# ------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_determinism_and_batch_invariance(case, drawn):
    res, _ = drawn
    T, truth = case["templates"], case["truth"]
    ctx = _context(case["model"], case["samples"])
    try:
        batch = _upload(ctx, T)
        a = batch.draw_mocks(truth, seed=SEED, write_resident=False, components=("latents", "sigma"))
        b = batch.draw_mocks(truth, seed=SEED, write_resident=False, components=("latents", "sigma"))
        other = batch.draw_mocks(truth, seed=SEED ^ (1 << 40), write_resident=False)
        batch.close()
        for k in ("flux", "latents", "sigma"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
            assert np.array_equal(_bits(a[k]), _bits(res[k])), k          # and the resident draw of the fixture
        assert _dev(a["flux"], other["flux"]) > 0.01
        # batches of 7 + 17 and of 1 x 24 with first_quasar_index set
        for cuts in ([0, 7, 24], list(range(25))):
            parts = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                ctx.set_first_quasar_index(lo)
                bt = _upload(ctx, T[lo:hi])
                parts.append(bt.draw_mocks(api._take_absorbers(truth, range(lo, hi)), seed=SEED, write_resident=False,
                                           components=("latents",)))
                bt.close()
            ctx.set_first_quasar_index(0)
            assert np.array_equal(_bits(np.concatenate([p["flux"] for p in parts])), _bits(a["flux"])), cuts
            assert np.array_equal(_bits(np.concatenate([p["latents"] for p in parts])), _bits(a["latents"])), cuts
        # the front end batches the same way
        many = gp.api.draw_mock_spectra(case["model"], case["samples"], T, truth, seed=SEED, max_quasars_per_batch=5)
        assert np.array_equal(_bits(np.concatenate(many["flux"])), _bits(a["flux"]))
        # one quasar's mask flipped at a few kept pixels: only those pixels change (to NaN)
        q = 4
        flipped = [dict(s) for s in T]
        mask = flipped[q]["pixel_mask"].copy()
        rest = flipped[q]["wavelengths"] / (1 + flipped[q]["z_qso"])
        inner = np.flatnonzero((mask == 0) & (rest > 950) & (rest < 1200))[[5, 6, -5]]
        mask[inner] = 1
        flipped[q]["pixel_mask"] = mask
        bt = _upload(ctx, flipped)
        c = bt.draw_mocks(truth, seed=SEED, write_resident=False)
        bt.close()
        o = _sizes(T)
        changed = np.flatnonzero(_bits(c["flux"]) != _bits(a["flux"]))
        np.testing.assert_array_equal(changed, o[q] + inner)
        assert np.isnan(c["flux"][changed]).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------
# 4. closed loop
# ------------------------------------------------------------------------------------------------

def test_closed_loop_single(oracle, case, drawn):
    res, out = drawn
    T, samples, model = case["templates"], case["samples"], case["model"]
    mock = _with_flux(T, res["flux"])
    ctx = _context(model, samples)
    batch = _upload(ctx, mock)
    try:
        batch.process()
        fresh = batch.download()
    finally:
        batch.close()
        ctx.close()
    for k in ("sample_log_likelihoods_dla", "log_likelihoods_no_dla", "log_likelihoods_dla", "MAP_inds", "p_dlas",
              "model_posteriors", "min_z_dlas", "max_z_dlas"):
        assert np.array_equal(_bits(out[k]), _bits(fresh[k])), k           # the flux never visited the host
    worst = 0.0
    for i, sp in enumerate(mock):
        ref = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"],
                                      sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"])
        worst = max(worst, float(np.abs(out["sample_log_likelihoods_dla"][i] - ref["sample_log_likelihoods_dla"]).max()),
                    abs(out["log_likelihoods_no_dla"][i] - ref["log_likelihood_no_dla"]),
                    abs(out["log_likelihoods_dla"][i] - ref["log_likelihood_dla"]))
        assert int(out["MAP_inds"][i]) - 1 == int(np.nanargmax(ref["sample_log_likelihoods_dla"]))
    print(f"closed loop (single-DLA): worst |delta log-likelihood| vs the oracle {worst:.3e}")
    assert worst < TOL_LL


def test_closed_loop_multi(oracle, mf_case):
    c = mf_case
    p = MultiParameters()
    T = c["templates"]
    ctx = _context(c["model"], c["samples"], p)
    try:
        batch = _upload(ctx, T)
        res = batch.draw_mocks(c["truth"], seed=SEED, write_resident=True)
        batch.process_multi()
        out = batch.download_multi()
        batch.close()
        mock = _with_flux(T, res["flux"])
        batch = _upload(ctx, mock)
        batch.process_multi(out["base_sample_inds"])
        fresh = batch.download_multi()
        batch.close()
    finally:
        ctx.close()
    for k in ("sample_log_likelihoods_dla", "sample_log_likelihoods_lls", "log_likelihoods_no_dla", "log_likelihoods_dla",
              "log_likelihoods_lls", "MAP_inds", "model_posteriors", "base_sample_inds"):
        a, b = out[k], fresh[k]
        assert np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b), k
    for i, sp in enumerate(mock):
        compare_multi(out, i, oracle_multi(oracle, c["model"], c["samples"], sp, out["base_sample_inds"][i], p), p)
    found = validation.map_model_index(out) - 1
    print("mean-flux closed loop: true absorber counts", np.diff(c["truth"][0]), "most probable model's", found.clip(0))


# ------------------------------------------------------------------------------------------------
# 5. statistics on GPU output
# ------------------------------------------------------------------------------------------------

def test_gpu_flux_is_a_draw_from_the_likelihoods_model(oracle, case, drawn):
    """Q1 and Q2 of tests/test_mocks.py from the GPU's flux and the ORACLE's rows."""
    res, _ = drawn
    mock = _with_flux(case["templates"], res["flux"])
    q1 = q2 = 0.0
    n1 = n2 = 0
    for i, sp in enumerate(mock):
        g, mu, M, om = R.rows(oracle, case["model"], sp, False)
        z, ln = R.absorbers_of(case["truth"], i)
        a = R.msr.map_absorption(oracle, g["pad"], z, ln, 3)[g["kept"]]
        s1, s2, n, k = R.whitened_statistics(g["y"], a, mu, M, om, g["nu"])
        q1, q2, n1, n2 = q1 + s1, q2 + s2, n1 + n, n2 + k
    print(f"GPU flux: Q1 = {q1:.1f} for {n1} ({(q1 - n1) / np.sqrt(2 * n1):+.2f} sigma), "
          f"Q2 = {q2:.1f} for {n2} ({(q2 - n2) / np.sqrt(2 * n2):+.2f} sigma)")
    assert n2 == 24 * 20
    assert abs(q1 - n1) <= R.chi2_bound(n1)
    assert abs(q2 - n2) <= R.chi2_bound(n2)


# ------------------------------------------------------------------------------------------------
# 6. recovery
# ------------------------------------------------------------------------------------------------

def test_recovery(case, drawn):
    _, out = drawn
    off, tz, tn = case["truth"]
    real = np.flatnonzero(np.diff(off) > 0)
    odds = validation.log_odds(out, occams_razor=1.0)
    print("log odds, clean:", np.round(odds[np.diff(off) == 0], 1), "injected:", np.round(odds[real], 1))
    tpr, fpr = validation.roc(out, real)
    assert tpr[fpr == 0].max() == 1.0
    comp = validation.completeness_by_log_nhi(out, case["truth"], [20.3, 20.8, 21.3, 22.0])
    dz, dn = validation.map_comparison(out, real, tz, tn)
    print("completeness by log N_HI", comp["found"], "/", comp["total"], "; MAP - truth: |dz| <=",
          f"{np.abs(dz).max():.4f}, |dlogN| <= {np.abs(dn).max():.3f} over {dz.size} quasars")
    conf, _ = validation.multi_confusion(out, case["truth"])
    print("confusion (found x true):", conf.tolist())
    assert conf.sum() == 24


# ------------------------------------------------------------------------------------------------
# 7. file to file
# ------------------------------------------------------------------------------------------------

def test_file_to_file(tmp_path, capsys):
    from gp_dla_detection_amd import run_dr12q
    d = tmp_path / "in"
    fs = synthetic.write_file_set(str(d), num_quasars=14, num_samples=96)
    P = fs["paths"]
    mock_file, truth_file = str(tmp_path / "mock_preloaded_qsos.mat"), str(tmp_path / "mock_truth.mat")
    assert mocks.main(["--preloaded", P["preloaded"], "--catalog", P["catalog"], "--model", P["learned"], "--samples",
                       P["samples"], "--out-preloaded", mock_file, "--out-truth", truth_file, "--p-absorbers", "0.4,0.6",
                       "--log-nhi-range", "20.5,22", "--seed", "11", "--max-quasars-per-batch", "5"]) == 0
    capsys.readouterr()
    run = run_dr12q.run(mock_file, P["catalog"], P["learned"], P["samples"], str(tmp_path / "out"), "mock",
                        prior_catalog=fs["prior"], device=0, max_quasars_per_batch=4)
    assert validation.main(["--processed", run["chunk"], "--truth", truth_file]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1
    from_files = json.loads(lines[0])
    # the same in memory
    truth = mocks.draw_truth(fs["spectra"], None, (0.4, 0.6), (20.5, 22.0), None, 0.0, 11)
    drawn_ = api.draw_mock_spectra(fs["model"], fs["samples"], fs["spectra"], truth, seed=11)
    np.testing.assert_array_equal(drawn_["status"] == 1, [i == 7 for i in range(14)])      # the fully masked quasar
    sel = np.flatnonzero(fs["test_ind"])
    mock = [dict(fs["spectra"][i], flux=drawn_["flux"][i]) for i in sel]
    res = gp.process_qsos(fs["model"], fs["samples"], mock, prior_catalog=fs["prior"])
    in_memory = json.loads(json.dumps(validation.score(res, api._take_absorbers(truth, sel))))
    assert from_files == in_memory
    assert from_files["num_quasars"] == sel.size and from_files["num_with_dla"] >= 3
    # the mock file is a preloaded file: same grids, noise and masks as the templates
    back = io.load_preloaded_qsos(mock_file, fs["catalog"]["z_qsos"])
    for t, m, f in zip(fs["spectra"], back, drawn_["flux"]):
        np.testing.assert_array_equal(m["wavelengths"], t["wavelengths"])
        np.testing.assert_array_equal(m["pixel_mask"], t["pixel_mask"])
        np.testing.assert_array_equal(m["flux"], f)
    assert os.path.getsize(mock_file) > 0
