"""Parity of the HIP path against the CPU oracle AT THE PRODUCTION SHAPE: BOSS-grid quasars
(production_shapes.py: 1e-4 dex pixels, 283 .. 1250 in-range pixels, the spectrograph's blue edge, run
masks, masked ends, z_qso up to 5.7) and the corners of the sample box (z offset exactly 0 and 1).

For about 70 % of a DR12Q run the search range starts at the first kept pixel (set_parameters.m:70-73,
the ``za`` branch), so the Ly-alpha centre of the bluest samples sits on pixel 0 and the higher series
lines lie blueward of the data; ``synthetic.make_spectrum``, which every other parity test uses, takes
that branch almost never.  The oracle is anchored on the same quasars by
test_oracle_production_shapes.py (NumPy / dense-K restatement to 2.4e-10; 50-digit arithmetic to 7.6e-11).

Tolerances are the project's: 1e-8 absolute on every log-likelihood and evidence, 1e-14 on min / max
z_DLA, 1e-9 on posteriors, indices exact.  Every leg collects all failing quasars into one message and
prints its worst deviation.
"""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
import production_shapes as P
from gp_dla_detection_amd import catalog, synthetic
from gp_dla_detection_amd.parameters import MultiParameters
from production_shapes import TOL, flat_priors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model20():
    return synthetic.make_model(20)


@pytest.fixture(scope="module")
def stratified():
    return P.stratified_quasars(20)


def sweep_and_compare(oracle, model, samples, spectra, label, num_lines=3, **kwargs):
    lp = flat_priors(len(spectra))
    got = gp.process_qsos(model, samples, spectra, log_priors=lp, params=gp.Parameters(num_lines=num_lines), **kwargs)
    want = P.oracle_single(oracle, model, samples, spectra, num_lines)
    failures, worst = P.single_failures(got, want, spectra, lp)
    print(f"{label}: worst |delta| = {worst:.2e} over {len(spectra)} quasars x {samples['offset_samples'].size} samples")
    assert not failures, f"{label}: " + "; ".join(failures)
    return got, want


@pytest.fixture(scope="module")
def leg1(oracle, model20, stratified):
    """Leg 1's batch, kept for the legs that compare with it (a failure here fails them too)."""
    samples = P.production_samples(1000)
    got, want = sweep_and_compare(oracle, model20, samples, stratified, "single-DLA k = 20, 3 lines, S = 1004",
                                  max_quasars_per_batch=len(stratified))
    return samples, got, want


# ---------------------------------------------------------------- 1. k_sweep_slim<3>

def test_single_dla_k20_whole_set(leg1, stratified):
    """The whole stratified set in one batch, production_samples(1000): null, all 1004 samples (the four
    corner samples named apart), evidence, search range, posteriors -- and the MAP columns the evidence
    kernel finds against the host recomputation."""
    samples, got, want = leg1
    assert (got["status"] == 0).all()
    z, lognhi, ind = catalog.map_estimates_host(got, samples)
    np.testing.assert_array_equal(got["MAP_inds"], ind + 1.0)
    np.testing.assert_array_equal(got["MAP_z_dlas"], z)
    np.testing.assert_array_equal(got["MAP_log_nhis"], lognhi)
    # and the index against the ORACLE's table wherever its maximum is clear of the tolerance
    sll = want["sample_log_likelihoods_dla"]
    top2 = np.sort(sll, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2 * TOL
    assert clear.sum() >= len(stratified) - 2
    np.testing.assert_array_equal(got["MAP_inds"][clear], sll[clear].argmax(axis=1) + 1.0)
    # a quasar with a strong injected absorber prefers the DLA model and recovers its redshift
    for i, sp in enumerate(stratified):
        if sp["true_z_dla"] is not None and sp["true_log_nhi"] > 20.5 and sp["edit"] != "confined":
            assert got["log_likelihoods_dla"][i] > got["log_likelihoods_no_dla"][i], sp["stratum"]


# ---------------------------------------------------------------- 2. the other kernels

@pytest.mark.parametrize("k,num_lines,S", [(40, 3, 200), (33, 3, 200), (20, 1, 100), (20, 31, 100), (12, 3, 100)])
def test_other_kernels_on_the_same_set(oracle, k, num_lines, S):
    """k = 40 and 33: k_sweep_split_slim; k = 20 at 1 and 31 lines: k_sweep_slim<0> (at 31 lines and
    z_qso < 2.9 most line centres of the bluest samples are off the data); k = 12."""
    model = synthetic.make_model(k)
    sweep_and_compare(oracle, model, P.production_samples(S), P.stratified_quasars(k),
                      f"single-DLA k = {k}, {num_lines} line(s), S = {S + 4}", num_lines=num_lines)


# ---------------------------------------------------------------- 3. production sample count

def test_production_sample_count(oracle, model20, stratified):
    """S = 10 000 (+ 4) on the shortest, the z_qso = 2.93 and the both-ends-masked quasar: every entry
    against the oracle; and a sample's result does not depend on its place in the table (bit for bit).

    10 004 is not a multiple of the 16 samples of a wave, so the last wave holds four samples (the
    largest z offsets, the corners among them) next to the null-model and idle slots.  Those slots
    used to evaluate input sample 0, and a wave takes the accurate Voigt tier as a whole when any
    lane asks for it: the four samples came out 1e-12 .. 2e-11 apart for different orders of the table
    (the 10 000 samples of test_full_size_properties fill their waves and never showed it).  The idle
    slots now evaluate the last sample in z order."""
    samples = P.production_samples(10000)
    three = [stratified[P.by_stratum(stratified, n)] for n in ("shortest", "crossover_za", "both_ends_masked_runs")]
    got, _ = sweep_and_compare(oracle, model20, samples, three, "single-DLA k = 20, S = 10004")
    perm = np.random.default_rng(0).permutation(samples["offset_samples"].size)
    shuffled = {k: v[perm] for k, v in samples.items()}
    out2 = gp.process_qsos(model20, shuffled, three, log_priors=flat_priors(3))
    np.testing.assert_array_equal(out2["sample_log_likelihoods_dla"], got["sample_log_likelihoods_dla"][:, perm])
    np.testing.assert_array_equal(out2["log_likelihoods_no_dla"], got["log_likelihoods_no_dla"])


# ---------------------------------------------------------------- 4. exact anchor

def test_sweep_against_exact_arithmetic_on_the_blue_edge(golden, leg1, stratified):
    """The fused sweep on the fixture quasar (za wins, first six pixels masked) against the 50-digit
    log-likelihoods of 32 samples (28 random + the four corners) and the null model.  The exact values
    were formed from the oracle's absorption vectors; the kernel's own profile differs from those by
    <= 2e-13, which moves a log-likelihood by up to a few 1e-10: hence 1e-8 on the samples and 1e-9 on
    the null model (no profile in it), as test_sweep_against_exact_arithmetic."""
    samples, got, _ = leg1
    e = golden("exact_boss_blue_edge.npz")
    i = P.by_stratum(stratified, "first_masked_za")
    np.testing.assert_array_equal(stratified[i]["wavelengths"], e["wavelengths"])
    assert got["min_z_dlas"][i] == float(e["min_z_dla"]) and got["max_z_dlas"][i] == float(e["max_z_dla"])
    d0 = abs(got["log_likelihoods_no_dla"][i] - float(e["null_log_p_exact"]))
    d = np.abs(got["sample_log_likelihoods_dla"][i][e["sample_indices"]] - e["sample_log_p_exact"])
    print(f"sweep vs 50-digit exact on the blue-edge quasar: null {d0:.3e}, samples max |delta| = {d.max():.3e}, "
          f"corners {d[-4:].max():.3e}")
    assert d0 < 1e-9, d0
    assert d.max() < TOL, (d.max(), int(e["sample_indices"][d.argmax()]))


# ---------------------------------------------------------------- 5. k_prepare directly

def prepared_rows(model, samples, spectra, params, multi):
    ctx = gp.Context(0, params)
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        n = len(spectra)
        if multi:
            batch = ctx.upload(spectra, np.zeros(n), np.zeros((n, params.max_dlas)), np.zeros(n))
        else:
            batch = ctx.upload(spectra, *flat_priors(n))
        rows = [batch.debug_prepared_rows(q, multi=multi) for q in range(n)]
        batch.close()
    finally:
        ctx.close()
    return rows


def check_rows(rows, sp, mu, omega2, tag):
    """Rows on the unmasked-range grid: masked rows are (0, 0, 0, 1); kept rows carry y and nu bit for
    bit and mu / omega2 within 1e-13 relative (the bound test_gpu_mean_flux_suppression... uses)."""
    inside = P.in_range(sp)
    keep = sp["pixel_mask"][inside] == 0
    bad = []
    if rows.shape != (int(inside.sum()), 4):
        return [f"[{tag}] {rows.shape[0]} rows, n_unmasked = {int(inside.sum())}"], 0.0
    if not np.array_equal(rows[~keep], np.tile([0.0, 0.0, 0.0, 1.0], ((~keep).sum(), 1))):
        bad.append(f"[{tag}] masked rows are not (0, 0, 0, 1)")
    if not (np.array_equal(rows[keep, 0], sp["flux"][inside][keep])
            and np.array_equal(rows[keep, 3], sp["noise_variance"][inside][keep])):
        bad.append(f"[{tag}] y / nu of the kept rows differ from the input")
    d = max(float(np.abs(rows[keep, 1] / mu - 1).max()), float(np.abs(rows[keep, 2] / omega2 - 1).max()))
    if not d < 1e-13:
        bad.append(f"[{tag}] mu / omega2 off by {d:.2e} relative")
    return bad, d


def test_prepare_rows_against_the_oracle_dump(oracle, model20, stratified):
    samples = P.production_samples(24)
    rows = prepared_rows(model20, samples, stratified, gp.Parameters(), multi=False)
    bad, worst = [], 0.0
    for sp, r in zip(stratified, rows):
        ref = oracle.process_spectrum(model20, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"],
                                      sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"], dump=True)
        assert ref["n_unmasked"] == int(P.in_range(sp).sum())
        b, d = check_rows(r, sp, ref["this_mu"], ref["this_omega2"], sp["stratum"])
        bad += b
        worst = max(worst, d)
    print(f"k_prepare rows vs the oracle's dump: worst relative deviation of mu / omega2 = {worst:.2e}")
    assert not bad, "; ".join(bad)


def numpy_prepared_multi(model, sp, p):
    """mu and omega2 of the kept pixels as the multi-DLA driver prepares them (multi :245-293), in the
    words of test_oracle_driver.numpy_driver: its ``dense`` argument records the null model's inputs,
    and with the noise variances set to zero the diagonal it is handed IS omega2."""
    from test_oracle_driver import numpy_driver
    seen = {}

    def record(y, mu, M, d):
        seen.setdefault("mu", mu)
        seen.setdefault("omega2", d)
        return 0.0

    one = {k: v[:1] for k, v in P.production_samples(1).items()}
    noiseless = dict(sp, noise_variance=np.zeros_like(sp["noise_variance"]))
    numpy_driver(model, one, noiseless, p, record, multi=MultiParameters(max_dlas=1), bsi=np.zeros((0, 1), np.uint32))
    return seen["mu"], seen["omega2"]


def test_prepare_rows_multi_against_the_numpy_restatement(model20, stratified):
    p = MultiParameters()
    three = [stratified[P.by_stratum(stratified, n)] for n in ("shortest", "first_masked_za", "beyond_5.7")]
    rows = prepared_rows(model20, P.production_samples(24), three, p, multi=True)
    bad, worst = [], 0.0
    for sp, r in zip(three, rows):
        mu, omega2 = numpy_prepared_multi(model20, sp, p)
        b, d = check_rows(r, sp, mu, omega2, sp["stratum"])
        bad += b
        worst = max(worst, d)
    print(f"k_prepare rows (multi) vs the NumPy restatement: worst relative deviation = {worst:.2e}")
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------- 6. multi-DLA driver

MULTI_SIX = ("shortest", "first_masked_za", "crossover_za", "crossover_zb", "beyond_5.7", "both_ends_masked_runs")


def multi_leg(oracle, k, p, names, S, label):
    """Indices drawn on the GPU, replayed by the oracle; every quasar is compared (test_gpu_multi.compare)
    and all failures are reported together."""
    from test_gpu_multi import compare, oracle_multi, priors
    model = synthetic.make_model(k)
    samples = P.production_samples(S)
    spectra = P.stratified_quasars(k) if names is None else None
    if names is not None:
        allq = P.stratified_quasars(k)
        spectra = [allq[P.by_stratum(allq, n)] for n in names]
    return multi_compare(oracle, model, samples, spectra, p, label, compare, oracle_multi, priors)


def multi_compare(oracle, model, samples, spectra, p, label, compare, oracle_multi, priors):
    out = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, priors(spectra, p), params=p)
    S = samples["offset_samples"].size
    bad, worst = [], 0.0
    for i, (sp, c) in enumerate(zip(spectra, P.census(spectra))):
        bsi = out["base_sample_inds"][i] if p.max_dlas > 1 else np.zeros((0, S), np.uint32)
        ref = oracle_multi(oracle, model, samples, sp, bsi, p)
        got, want = out["sample_log_likelihoods_dla"][i].T, ref["sample_log_likelihoods_dla"]
        d = max(P._dev(out["log_likelihoods_no_dla"][i], ref["log_likelihood_no_dla"]),
                P._dev(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0)),
                P._dev(out["sample_log_likelihoods_lls"][i], ref["sample_log_likelihoods_lls"]),
                P._dev(np.nan_to_num(out["log_likelihoods_dla"][i]), np.nan_to_num(ref["log_likelihoods_dla"])),
                P._dev(out["log_likelihoods_lls"][i], ref["log_likelihood_lls"]))
        dz = max(P._dev(out["min_z_dlas"][i], ref["min_z_dla"]), P._dev(out["max_z_dlas"][i], ref["max_z_dla"]))
        worst = max(worst, d)
        try:
            assert out["status"][i] == 0 and dz < P.TOL_Z, f"status {out['status'][i]}, z range {dz:.1e}"
            compare(out, i, ref, p)
        except AssertionError as err:
            bad.append(f"quasar {i} [{c['stratum']}] z_qso = {c['z_qso']:.4f}, {c['n_kept']} kept of {c['n_unmasked']}, "
                       f"worst {d:.2e}: {str(err).strip().splitlines()[0][:200]}")
    print(f"{label}: worst |delta| = {worst:.2e} over {len(spectra)} quasars")
    assert not bad, f"{label}: " + "; ".join(bad)
    return out


def test_multi_dla_driver_on_six_strata(oracle):
    """k_profiles, k_sweep_multi_slim, evidences and resampling: max_dlas = 4, S = 160 + corners."""
    multi_leg(oracle, 20, MultiParameters(max_dlas=4), MULTI_SIX, 160, "multi-DLA k = 20, max_dlas = 4, S = 164")


def test_multi_dla_driver_rank_40(oracle):
    multi_leg(oracle, 40, MultiParameters(max_dlas=3), ("shortest", "first_masked_za"), 160,
              "multi-DLA k = 40, max_dlas = 3, S = 164")


def test_multi_dla_driver_31_lines(oracle):
    multi_leg(oracle, 20, MultiParameters(max_dlas=4, num_lines=31), ("crossover_za", "both_ends_masked_runs"), 160,
              "multi-DLA k = 20, 31 lines, max_dlas = 4, S = 164")


# ---------------------------------------------------------------- 7. seeded mix

def test_seeded_mix(oracle, model20):
    """48 quasars of the DR12Q mix, S = 200 (+ corners), one batch; none may be dropped."""
    spectra = P.seeded_mix(model20)
    rows = P.census(spectra)
    assert len(rows) == 48 and all(c["n_kept"] >= 200 for c in rows)
    assert sum(c["za_wins"] for c in rows) >= 24, sum(c["za_wins"] for c in rows)
    sweep_and_compare(oracle, model20, P.production_samples(200), spectra, "seeded DR12Q mix, 48 quasars, S = 204",
                      max_quasars_per_batch=48)


def test_seeded_mix_multi(oracle, model20):
    from test_gpu_multi import compare, oracle_multi, priors
    spectra = P.seeded_mix(model20)[:12]
    assert sum(c["za_wins"] for c in P.census(spectra)) >= 6
    multi_compare(oracle, model20, P.production_samples(200), spectra, MultiParameters(max_dlas=3),
                  "seeded DR12Q mix through the multi-DLA driver, 12 quasars, max_dlas = 3, S = 204",
                  compare, oracle_multi, priors)


# ---------------------------------------------------------------- 8. surfaces

def test_cells_pipeline_with_production_lengths(leg1, model20, stratified):
    """gpdla_process_cells (list input) in batches of 3 through 2 slots: lengths 285 .. 1254 regrow the
    slots' buffers as the 20 .. 90-pixel lists of the other pipeline tests do not; bit-equal to leg 1."""
    samples, one, _ = leg1
    many = gp.process_qsos(model20, samples, list(stratified), log_priors=flat_priors(len(stratified)),
                           max_quasars_per_batch=3, pipeline_slots=2)
    for key in one:
        np.testing.assert_array_equal(one[key], many[key], err_msg=key)
