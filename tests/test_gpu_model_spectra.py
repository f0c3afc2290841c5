"""GPU checks of the model-spectra subsystem against the NumPy-and-oracle restatement
(tests/model_spectra_restatement.py) and the reference-produced fixture tests/golden/model_mean.npz.
Every pixel of every compared quasar counts; each figure is printed before it is asserted."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import model_spectra_restatement as R
import production_shapes as ps

pytestmark = pytest.mark.gpu

TOL_MAP = 1e-12       # 4 x the 2e-13 the Voigt parity test demands of one profile, with margin
TOL_MOMENTS = 1e-11   # a convex combination of profiles within 2e-13 each + S eps ~ 1.1e-12 of summation rounding
TOL_MEAN = 1e-12      # this_mu against the reference's own numbers
TOL_LL = 1e-8         # the project's log-likelihood tolerance


def _dev(a, b) -> float:
    """max |a - b| with matching NaN patterns (inf otherwise)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return float("inf")
    d = np.abs(a - b)[~np.isnan(a)]
    return float(d.max()) if d.size else 0.0


def _single(model, samples, spectra, params=None):
    ctx = gp.Context(0, params or Parameters())
    ctx.set_model(model)
    ctx.set_samples(samples)
    n = len(spectra)
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))


def _multi(model, samples, spectra, params):
    ctx = gp.Context(0, params)
    ctx.set_model(model)
    ctx.set_samples(samples)
    n = len(spectra)
    lp_dla = np.log(np.full((n, params.max_dlas), 0.1) ** np.arange(1, params.max_dlas + 1))
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.85)), lp_dla, np.full(n, np.log(0.05)))


def _masked_out(sp):
    out = dict(sp)
    ps.mask_pixels(out, np.arange(np.asarray(sp["wavelengths"]).size))
    return out


def _quasars(k=20):
    """Production-shape quasars (masked ends, run masks, the tile-boundary run, 36 kept of 1249) and
    synthetic ones."""
    model = synthetic.make_model(k)
    strat = ps.stratified_quasars(k)
    names = ("shortest", "first_masked_za", "both_ends_masked_runs", "tile_boundary_run", "confined_40px", "beyond_5.7")
    spectra = [strat[ps.by_stratum(strat, n)] for n in names]
    spectra += [synthetic.make_spectrum(4200, 300, model, mask_fraction=0.05), synthetic.make_spectrum(4201, 1500, model)]
    return model, spectra


# ------------------------------------------------------------------------------------------------
# P1
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_lines", [1, 3, 31])
def test_map_absorption_against_oracle_products(oracle, num_lines):
    model, spectra = _quasars()
    spectra.append(_masked_out(spectra[0]))            # no kept pixel: no padded grid, a NaN row
    grids = [R.grid(oracle, model, sp) for sp in spectra]
    counts = [0, 1, 2, 3, 4, 1, 2, 4, 2]
    off, zs, lns = [0], [], []
    rng = np.random.default_rng(30 + num_lines)
    for g, c in zip(grids, counts):
        lo, hi = (g["min_z"], g["max_z"]) if "pad" in g else (2.0, 2.5)
        zs += list(lo + (hi - lo) * rng.uniform(0.02, 0.98, c))
        lns += list(rng.uniform(20.0, 22.8, c))
        off.append(len(zs))
    absorbers = (np.array(off), np.array(zs), np.array(lns))
    ctx, batch = _single(model, synthetic.make_samples(16), spectra, Parameters(num_lines=num_lines))
    try:
        res = batch.model_spectra(absorbers=absorbers, products=("map",))
        np.testing.assert_array_equal(batch.unmasked_counts(), [g["n_u"] for g in grids])
    finally:
        batch.close()
        ctx.close()
    np.testing.assert_array_equal(np.diff(res["offsets"]), [g["n_u"] for g in grids])
    got = gp.split_cells(res["map_absorption"], res["offsets"])
    worst = 0.0
    for i, g in enumerate(grids):
        if "pad" not in g:
            assert np.isnan(got[i]).all() and res["status"][i] == 1
            continue
        want = R.map_absorption(oracle, g["pad"], zs[off[i]:off[i + 1]], lns[off[i]:off[i + 1]], num_lines)
        d = _dev(got[i], want)
        print(f"lines {num_lines} quasar {i}: {counts[i]} absorbers, n_u {g['n_u']}, |delta| {d:.2e}")
        worst = max(worst, d)
        if counts[i] == 0:
            assert (got[i] == 1.0).all()
    print(f"P1 worst |delta| at {num_lines} lines: {worst:.3e}")
    assert worst < TOL_MAP


def test_map_absorption_reproduces_the_sweeps_likelihood(oracle):
    """P1 at sample i's (z, N), fed through the oracle's log_mvnpdf_low_rank with the oracle's prepared
    rows, gives the log-likelihood the sweep stored for sample i."""
    model, spectra = _quasars()
    spectra = [spectra[2], spectra[3], spectra[6]]
    samples = synthetic.make_samples(96)
    ctx, batch = _single(model, samples, spectra)
    worst = 0.0
    try:
        batch.process()
        out = batch.download()
        picks = [0, 17, 50, 95]
        for q, sp in enumerate(spectra):
            g = R.grid(oracle, model, sp)
            z = out["min_z_dlas"][q] + (out["max_z_dlas"][q] - out["min_z_dlas"][q]) * samples["offset_samples"][picks]
            for j, i in enumerate(picks):
                res = batch.model_spectra(selection=[q], absorbers=(np.array([0, 1]), z[j:j + 1], samples["log_nhi_samples"][i:i + 1]),
                                          products=("map",))
                # the exact column density of the sample, not 10^log10 of it
                a = oracle.voigt(g["pad"], z[j], samples["nhi_samples"][i], 3)
                assert _dev(res["map_absorption"], a) < TOL_MAP
                a = res["map_absorption"][g["kept"]]
                ll, rc = oracle.log_mvnpdf_low_rank(g["y"], a * g["mu"], a[:, None] * g["M"], a * a * g["omega2"] + g["nu"])
                assert rc == 0
                d = abs(ll - out["sample_log_likelihoods_dla"][q, i])
                print(f"quasar {q} sample {i}: |delta log-likelihood| {d:.2e}")
                worst = max(worst, d)
    finally:
        batch.close()
        ctx.close()
    assert worst < TOL_LL


# ------------------------------------------------------------------------------------------------
# P2
# ------------------------------------------------------------------------------------------------

def _check_moments(oracle, model, spectra, samples, res, rows, nhi_key="nhi_samples", num_lines=3, label=""):
    mean, var = gp.split_cells(res["mean_absorption"], res["offsets"]), gp.split_cells(res["var_absorption"], res["offsets"])
    worst = 0.0
    for i, sp in enumerate(spectra):
        g = R.grid(oracle, model, sp)
        want_mean, want_var = R.moments(oracle, g, samples["offset_samples"], samples[nhi_key], rows[i], num_lines)
        dm, dv = _dev(mean[i], want_mean), _dev(var[i], want_var)
        print(f"{label} quasar {i}: n_u {g['n_u']}, |delta mean| {dm:.2e}, |delta var| {dv:.2e}, "
              f"max var {np.nanmax(want_var) if np.isfinite(want_var).any() else np.nan:.3g}")
        worst = max(worst, dm, dv)
    return worst


def test_moments_production_samples_resident_table(oracle):
    """S = 10 004 (10^4 Halton samples and the four corners of the sample box), weights from the batch's
    own table after process()."""
    model, spectra = _quasars()
    spectra = [spectra[3], spectra[7]]          # the tile-boundary run (968 px) and a full 1500 px one
    samples = ps.production_samples(10000)
    ctx, batch = _single(model, samples, spectra)
    try:
        batch.process()
        rows = batch.download()["sample_log_likelihoods_dla"]
        res = batch.model_spectra(weights="resident", products=("moments",))
    finally:
        batch.close()
        ctx.close()
    worst = _check_moments(oracle, model, spectra, samples, res, rows, label="S=10004")
    print(f"P2 worst |delta| at S = 10004: {worst:.3e}")
    assert worst < TOL_MOMENTS


def test_moments_special_rows_and_the_lls_choice(oracle):
    """S = 1000 on the production-shape and synthetic quasars, weights from a host table: the sweep's own
    rows, rows with NaN entries, an all-NaN row, a flat row, a row so peaked that all but one weight
    underflow; then the same with the sub-DLA column densities."""
    model, spectra = _quasars()
    S = 1000
    samples = synthetic.make_samples(S)
    rng = np.random.default_rng(8)
    ctx, batch = _single(model, samples, spectra)
    try:
        batch.process()
        rows = np.array(batch.download()["sample_log_likelihoods_dla"])
        rows[1, rng.choice(S, 300, replace=False)] = np.nan      # NaN entries
        rows[2, :] = np.nan                                      # an all-NaN row
        rows[3, :] = -1234.5                                     # flat
        rows[4, :] = -5000.0                                     # peaked: every other weight underflows to 0
        rows[4, 617] = 0.0
        rows[5, ::2] = np.nan
        res = batch.model_spectra(weights=rows, products=("moments",))
        res_lls = batch.model_spectra(weights=rows, sub_dla=True, products=("moments",))
    finally:
        batch.close()
        ctx.close()
    assert np.isnan(gp.split_cells(res["mean_absorption"], res["offsets"])[2]).all()
    assert np.isnan(gp.split_cells(res["var_absorption"], res["offsets"])[2]).all()
    assert (gp.split_cells(res["var_absorption"], res["offsets"])[4] < 1e-25).all()   # one sample: no spread
    worst = _check_moments(oracle, model, spectra, samples, res, rows, label="S=1000 dla")
    worst_lls = _check_moments(oracle, model, spectra, samples, res_lls, rows, nhi_key="lls_nhi_samples", label="S=1000 lls")
    print(f"P2 worst |delta| at S = 1000: dla {worst:.3e}, lls {worst_lls:.3e}")
    assert worst < TOL_MOMENTS and worst_lls < TOL_MOMENTS


def test_moments_31_lines(oracle):
    model, spectra = _quasars()
    spectra = [spectra[0], spectra[6]]
    samples = synthetic.make_samples(500)
    ctx, batch = _single(model, samples, spectra, Parameters(num_lines=31))
    try:
        batch.process()
        rows = batch.download()["sample_log_likelihoods_dla"]
        res = batch.model_spectra(weights="resident", products=("moments",))
    finally:
        batch.close()
        ctx.close()
    worst = _check_moments(oracle, model, spectra, samples, res, rows, num_lines=31, label="31 lines")
    print(f"P2 worst |delta| at 31 lines: {worst:.3e}")
    assert worst < TOL_MOMENTS


def test_moments_multi_dla_batch(oracle):
    """A multi-DLA batch: the resident DLA(1) table and the resident sub-DLA table."""
    model, spectra = _quasars()
    spectra = [spectra[1], spectra[3], spectra[6]]
    S = 1000
    samples = synthetic.make_samples(S)
    p = MultiParameters(max_dlas=2)
    ctx, batch = _multi(model, samples, spectra, p)
    try:
        batch.process_multi()
        out = batch.download_multi()
        res = batch.model_spectra(weights="resident", products=("moments",))
        res_lls = batch.model_spectra(weights="resident", sub_dla=True, products=("moments",))
        host = batch.model_spectra(weights=out["sample_log_likelihoods_dla"][:, 0, :], products=("moments",))
    finally:
        batch.close()
        ctx.close()
    for name in ("mean_absorption", "var_absorption"):
        np.testing.assert_array_equal(res[name], host[name])
    worst = _check_moments(oracle, model, spectra, samples, res, out["sample_log_likelihoods_dla"][:, 0, :], label="multi DLA(1)")
    worst_lls = _check_moments(oracle, model, spectra, samples, res_lls, out["sample_log_likelihoods_lls"],
                               nhi_key="lls_nhi_samples", label="multi sub-DLA")
    print(f"P2 worst |delta| on a multi-DLA batch: DLA(1) {worst:.3e}, sub-DLA {worst_lls:.3e}")
    assert worst < TOL_MOMENTS and worst_lls < TOL_MOMENTS


def test_moments_are_bit_identical_however_they_are_asked_for():
    """Resident and host weights, two runs, a permuted selection and another batching give the same bits."""
    model, spectra = _quasars()
    spectra.append(_masked_out(spectra[1]))
    samples = synthetic.make_samples(777)       # not a multiple of 64 or 256
    ctx, batch = _single(model, samples, spectra)
    try:
        batch.process()
        out = batch.download()
        a = batch.model_spectra(weights="resident", products=("moments",))
        b = batch.model_spectra(weights="resident", products=("moments",))
        c = batch.model_spectra(weights=out["sample_log_likelihoods_dla"], products=("moments",))
        perm = np.random.default_rng(2).permutation(len(spectra))
        d = batch.model_spectra(selection=perm, weights="resident", products=("moments",))
    finally:
        batch.close()
        ctx.close()
    for name in ("mean_absorption", "var_absorption"):
        np.testing.assert_array_equal(a[name], b[name])
        np.testing.assert_array_equal(a[name], c[name])
        cells, permuted = gp.split_cells(a[name], a["offsets"]), gp.split_cells(d[name], d["offsets"])
        for j, q in enumerate(perm):
            np.testing.assert_array_equal(permuted[j], cells[q])
    assert np.isnan(gp.split_cells(a["mean_absorption"], a["offsets"])[-1]).all() and a["status"][-1] == 1
    assert np.isfinite(a["mean_absorption"][:a["offsets"][-2]]).all()
    # the script surface: one quasar per batch against three per batch against the resident batch
    results = dict(out)
    one = gp.model_spectra(model, samples, spectra, results, absorbers=None, products=("moments",), max_quasars_per_batch=1)
    three = gp.model_spectra(model, samples, spectra, results, absorbers=None, products=("moments",), max_quasars_per_batch=3)
    np.testing.assert_array_equal(one["offsets"], a["offsets"])
    for name in ("mean_absorption", "var_absorption"):
        np.testing.assert_array_equal(one[name], a[name])
        np.testing.assert_array_equal(three[name], a[name])


# ------------------------------------------------------------------------------------------------
# P3
# ------------------------------------------------------------------------------------------------

def test_continuum_against_the_dense_restatement(oracle):
    """k = 20 and k = 40, with and without the mean-flux model, null model and absorbers, the masked run
    across a tile boundary among them.  Tolerance: 10 x the restatement's own dense-vs-Woodbury
    disagreement on these cases, floored at 1e-12, never looser than 1e-8."""
    cases = R.continuum_cases(oracle)
    want, disagreement = [], 0.0
    for c in cases:
        dense = R.continuum(oracle, c["model"], c["grid"], c["absorption"], c["meanflux"], "dense")
        wood = R.continuum(oracle, c["model"], c["grid"], c["absorption"], c["meanflux"], "woodbury")
        disagreement = max(disagreement, _dev(dense[0], wood[0]), _dev(dense[1], wood[1]))
        want.append(dense)
    tol = R.continuum_tolerance(disagreement)
    print(f"dense-vs-Woodbury disagreement {disagreement:.2e} -> tolerance {tol:.2e}")
    worst = 0.0
    for c, (cont, flux) in zip(cases, want):
        p = MultiParameters() if c["meanflux"] else Parameters()
        samples = synthetic.make_samples(16)
        ctx, batch = (_multi if c["meanflux"] else _single)(c["model"], samples, [c["spectrum"]], p)
        try:
            absorbers = (np.array([0, c["z_dlas"].size]), c["z_dlas"], c["log_nhis"])
            res = batch.model_spectra(absorbers=absorbers, meanflux=c["meanflux"], products=("map", "continuum"))
        finally:
            batch.close()
            ctx.close()
        assert res["status"][0] == 0 and res["continuum"].size == c["grid"]["n_u"]
        dc, df = _dev(res["continuum"], cont), _dev(res["model_flux"], flux)
        print(f"{c['name']}: |delta continuum| {dc:.2e}, |delta model flux| {df:.2e}")
        worst = max(worst, dc, df)
    print(f"P3 worst |delta|: {worst:.3e} (tolerance {tol:.2e})")
    assert worst < tol


def test_continuum_of_a_quasar_without_kept_pixels_is_nan():
    model, spectra = _quasars()
    spectra = [spectra[0], _masked_out(spectra[0])]
    ctx, batch = _single(model, synthetic.make_samples(16), spectra)
    try:
        res = batch.model_spectra(products=("continuum",))
    finally:
        batch.close()
        ctx.close()
    cont = gp.split_cells(res["continuum"], res["offsets"])
    assert res["status"].tolist() == [0, 1]
    assert np.isfinite(cont[0]).all() and cont[1].size == cont[0].size and np.isnan(cont[1]).all()
    assert np.isnan(gp.split_cells(res["model_flux"], res["offsets"])[1]).all()


# ------------------------------------------------------------------------------------------------
# P4
# ------------------------------------------------------------------------------------------------

def test_dla_model_mean_against_the_references_this_mu(golden):
    g = golden("model_mean.npz")
    model = dict(rest_wavelengths=g["rest_wavelengths"], mu=g["mu"])
    worst = 0.0
    for i in range(int(g["num_cases"])):
        z, ln = g[f"z_dlas_{i}"], g[f"log_nhis_{i}"]
        got = gp.dla_model_mean(model, [float(g[f"z_qso_{i}"])], (np.array([0, z.size]), z, ln),
                                suppressed=bool(g[f"suppressed_{i}"]), num_voigt_lines=int(g[f"num_voigt_lines_{i}"]),
                                num_forest_lines=int(g[f"num_forest_lines_{i}"]), prev_tau_0=float(g["tau"]),
                                prev_beta=float(g["beta"]))
        d = _dev(got[0], g[f"this_mu_{i}"])
        print(f"case {i}: {z.size} absorbers, {int(g[f'num_voigt_lines_{i}'])} lines, suppressed {bool(g[f'suppressed_{i}'])}: {d:.2e}")
        worst = max(worst, d)
    # all cases in one call, as a list of (quasar, absorber list)
    n = int(g["num_cases"])
    same = [i for i in range(n) if int(g[f"num_voigt_lines_{i}"]) == 3 and bool(g[f"suppressed_{i}"]) and int(g[f"num_forest_lines_{i}"]) == 31]
    off = np.concatenate([[0], np.cumsum([g[f"z_dlas_{i}"].size for i in same])])
    together = gp.dla_model_mean(model, [float(g[f"z_qso_{i}"]) for i in same],
                                 (off, np.concatenate([g[f"z_dlas_{i}"] for i in same]), np.concatenate([g[f"log_nhis_{i}"] for i in same])))
    for j, i in enumerate(same):
        worst = max(worst, _dev(together[j], g[f"this_mu_{i}"]))
    print(f"P4 worst |delta|: {worst:.3e}")
    assert worst < TOL_MEAN


# ------------------------------------------------------------------------------------------------
# scale
# ------------------------------------------------------------------------------------------------

def test_scale_256_quasars_1500_pixels_10000_samples(oracle):
    model = synthetic.make_model(20)
    nq, n, S = 256, 1500, 10000
    spectra = synthetic.make_spectra(nq, n, model, mask_fraction=0.03, first_index=7000)
    samples = synthetic.make_samples(S)
    ctx, batch = _single(model, samples, spectra)
    try:
        batch.process()
        res = batch.model_spectra(weights="resident", products=("moments",))
        picks = [0, 101, 255]
        rows = batch.download()["sample_log_likelihoods_dla"][picks]
    finally:
        batch.close()
        ctx.close()
    assert res["offsets"][-1] == nq * n and np.isfinite(res["mean_absorption"]).all() and np.isfinite(res["var_absorption"]).all()
    assert (res["mean_absorption"] <= 1 + 1e-12).all() and (res["var_absorption"] >= 0).all()
    mean, var = gp.split_cells(res["mean_absorption"], res["offsets"]), gp.split_cells(res["var_absorption"], res["offsets"])
    sub = dict(offsets=np.concatenate([[0], np.cumsum([mean[q].size for q in picks])]),
               mean_absorption=np.concatenate([mean[q] for q in picks]), var_absorption=np.concatenate([var[q] for q in picks]))
    worst = _check_moments(oracle, model, [spectra[q] for q in picks], samples, sub, rows, label="scale")
    print(f"P2 worst |delta| of three quasars of the 256 x 1500 x 10^4 run: {worst:.3e}")
    assert worst < TOL_MOMENTS


# ------------------------------------------------------------------------------------------------
# file to file
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("multi", [False, True])
def test_command_line_run_equals_the_in_memory_call(tmp_path, multi):
    """python -m gp_dla_detection_amd.model_spectra on -v7.3 files (a fully masked quasar among them): the
    selected rows of the processed file's sample table are streamed, nothing is swept again, and the
    file holds what api.model_spectra gives for the same quasars in memory."""
    from gp_dla_detection_amd import io, model_spectra as cli
    fs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=12, num_samples=96)
    run_pos = np.flatnonzero(fs["test_ind"])
    spectra = [fs["spectra"][i] for i in run_pos]
    z = fs["catalog"]["z_qsos"][run_pos]
    processed = str(tmp_path / "processed.mat")
    if multi:
        p = MultiParameters(max_dlas=3)
        lp = gp.dla_existence_prior_multi(fs["prior"]["z_qsos"], fs["prior"]["dla_ind"], z, fs["Z_lls"], fs["Z_dla"], p)
        results = gp.process_qsos_multiple_dlas_meanflux(fs["model"], fs["samples"], spectra, lp, params=p)
        io.save_processed_qsos_multi(processed, results, test_ind=fs["test_ind"])
    else:
        p = Parameters()
        results = gp.process_qsos(fs["model"], fs["samples"], spectra, prior_catalog=fs["prior"])
        io.save_processed_qsos(processed, results, test_ind=fs["test_ind"])
    thresh = float(np.nanmedian(results["p_dlas"]))
    sel = np.flatnonzero(results["p_dlas"] >= thresh)
    assert 0 < sel.size < len(spectra)
    out = str(tmp_path / "model_spectra.mat")
    rc = cli.main(["--preloaded", fs["paths"]["preloaded"], "--catalog", fs["paths"]["catalog"], "--model", fs["paths"]["learned"],
                   "--samples", fs["paths"]["samples"], "--processed", processed, "--out", out, f"--p-dla={thresh!r}",
                   "--max-quasars-per-batch", "3"])
    assert rc == 0
    want = gp.model_spectra(fs["model"], fs["samples"], spectra, results, params=p, selection=sel)
    back = io.load_model_spectra(out)
    np.testing.assert_array_equal(back["selection"], sel)
    np.testing.assert_array_equal(back["offsets"], want["offsets"])
    np.testing.assert_array_equal(back["status"], want["status"])
    for name in io.MODEL_SPECTRA_CELLS:
        cells = gp.split_cells(want[name], want["offsets"])
        assert len(back[name]) == sel.size
        for got, ref in zip(back[name], cells):
            np.testing.assert_array_equal(got, ref, err_msg=name)
    a_off, a_z, _ = gp.map_absorbers(results, sub_dla=multi)
    assert [c.tolist() for c in back["map_z_dlas"]] == [a_z[a_off[q]:a_off[q + 1]].tolist() for q in sel]
    # an explicit index list, the fully masked quasar included when it is part of the run
    idx = [int(run_pos.size - 1), 0, 3]
    cli.main(["--preloaded", fs["paths"]["preloaded"], "--catalog", fs["paths"]["catalog"], "--model", fs["paths"]["learned"],
              "--samples", fs["paths"]["samples"], "--processed", processed, "--out", out, "--indices", ",".join(map(str, idx)),
              "--products", "map,moments"])
    back = io.load_model_spectra(out)
    assert back["selection"].tolist() == sorted(idx) and "continuum" not in back and len(back["mean_absorption"]) == 3
