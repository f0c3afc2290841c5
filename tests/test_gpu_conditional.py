"""GPU checks of the batch conditioned on fixed absorbers on the synthetic batch of
tests/conditional_cases.py: k = 8 with three lines (896-B records) and k = 24 with five (1536-B records), S = 200.

 - the conditioned rows == the unconditioned rows times map_absorption of the same lists, bitwise, at the tile edges
   of k_condition_rows, for every rank class, 0 .. 8 fixed absorbers and both preparations;
 - the conditional table against the CPU oracle (the multi-DLA driver with constant base samples for meanflux rows,
   the dense route for process_qsos.m's rows): 1e-8 absolute, the project's parity bound; the -inf pattern exactly;
 - the refine contract on a conditioned batch by DESIGN.md 4.18's rules (tests/test_gpu_refine.py);
 - the orchestration of gp_dla_detection_amd/conditional.py pass by pass, and what it is for;
 - invariances, refusals and the command line.
Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, api, conditional, io, synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import conditional_cases as CC
import conditional_restatement as CR
import posterior_restatement as PR
import refine_restatement as RR

pytestmark = pytest.mark.gpu

SEP = CC.SEPARATION
PROBS, THRESH = (0.025, 0.16, 0.5, 0.84, 0.975), (20.3,)
FIRST = ("sample_log_likelihoods_dla", "log_likelihoods_no_dla", "log_likelihoods_dla", "log_posteriors_dla", "model_posteriors",
         "MAP_inds", "MAP_z_dlas", "MAP_log_nhis", "min_z_dlas", "max_z_dlas", "status")
REFINED = ("log_likelihoods_dla_refined", "log_posteriors_dla_refined", "MAP_z_dlas_refined", "MAP_log_nhis_refined", "MAP_inds_refined",
           "boxes", "status", "sample_log_likelihoods_refined", "sample_log_posteriors_refined")
# the rows a conditioned batch is prepared with: the multi-DLA driver's at its default prev_tau_0 and at 0, process_qsos.m's
VARIANTS = {"meanflux": lambda nl, **kw: MultiParameters(num_lines=nl, **kw),
            "meanflux0": lambda nl, **kw: MultiParameters(num_lines=nl, prev_tau_0=0.0, **kw),
            "single": lambda nl, **kw: Parameters(num_lines=nl, **kw)}


def _same(a, b, keys, rows_a=slice(None), rows_b=slice(None)):
    for key in keys:
        np.testing.assert_array_equal(a[key][rows_a], b[key][rows_b], err_msg=key)   # NaN and -inf patterns included


def _open(params, model, samples, spectra, Sr=None):
    ctx = gp.Context(0, params)
    ctx.set_model(model)
    ctx.set_samples(samples)
    if Sr:
        ctx.set_refine_points(*CC.halton_points(Sr))
    n = len(spectra)
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))


# ---------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------

EDGE_NU = (2, 6, 7, 249, 250, 251, 501)   # around the 7 taps and the 250-pixel tile of k_condition_rows; three tiles


def _exact_log_nhis(count):
    """log N values whose 10^x NumPy's array power (what model_spectra's host side takes) and the C library's pow (what
    the conditioning takes) round alike on the machine that runs the test: the bitwise comparison below is about the kernels' arithmetic,
    not about two correctly-rounded-or-not host functions."""
    out = []
    for i in range(400):
        x = 20.0 + 0.0125 * i
        if float((10.0 ** np.array([x]))[0]) == math.pow(10.0, x):
            out.append(x)
        if len(out) == count:
            return out
    raise AssertionError("fewer than %d log N values on which the two host powers agree" % count)


@pytest.mark.parametrize("meanflux", [False, True])
@pytest.mark.parametrize("k,nl", [(1, 3), (8, 3), (24, 5), (40, 5)])
def test_conditioned_rows_are_the_rows_times_the_absorption(k, nl, meanflux):
    model, samples = synthetic.make_model(k), synthetic.make_samples(16)
    spectra = [CC.edge_spectrum(n_u, model, nl, masked=n_u >= 249) for n_u in EDGE_NU]
    log_nhis = _exact_log_nhis(8)
    ctx, batch = _open(MultiParameters(num_lines=nl) if meanflux else Parameters(num_lines=nl), model, samples, spectra)
    try:
        counts = batch.unmasked_counts()
        np.testing.assert_array_equal(counts, EDGE_NU)
        plain = [batch.debug_conditioned_rows(q, meanflux) for q in range(len(spectra))]
        np.testing.assert_array_equal(plain[3][0], batch.debug_prepared_rows(3, multi=meanflux))   # the hook itself
        checked = 0
        for F in (0, 1, 3, 8):
            lists = []
            for sp in spectra:
                rest = sp["wavelengths"] / (1 + sp["z_qso"])
                inside = sp["wavelengths"][(rest >= 911.75) & (rest <= 1215.75)]
                zc = float(np.median(inside)) / 1215.6701 - 1
                lists.append([[zc + (j - 3.5) * 3 * SEP, log_nhis[j]] for j in range(F)])
            csr = conditional.csr_of(lists)
            A = api.split_cells(batch.model_spectra(absorbers=csr, products=("map",), meanflux=meanflux)["map_absorption"],
                                np.concatenate([[0], np.cumsum(counts)]))
            batch.set_fixed_absorbers(csr, SEP, meanflux)
            for q in range(len(spectra)):
                rows, M = batch.debug_conditioned_rows(q)
                want = plain[q][0].copy()
                if F:
                    want[:, 1] = want[:, 1] * A[q]
                    want[:, 2] = want[:, 2] * (A[q] * A[q])
                np.testing.assert_array_equal(rows, want, err_msg=f"n_u {EDGE_NU[q]} F {F}")
                np.testing.assert_array_equal(M, plain[q][1] * A[q][:, None] if F else plain[q][1], err_msg=f"n_u {EDGE_NU[q]} F {F} M")
                masked = np.flatnonzero(spectra[q]["pixel_mask"][2:-2])
                assert (rows[masked] == [0.0, 0.0, 0.0, 1.0]).all() and (M[masked] == 0.0).all()   # neutral rows stay neutral
                checked += rows.size + M.size
            batch.set_fixed_absorbers(None)
            if F == 8:
                print(f"k {k} lines {nl} meanflux {meanflux}: A in [{min(a.min() for a in A):.3e}, {max(a.max() for a in A):.6f}]")
        for q in range(len(spectra)):   # cleared: the unconditioned rows again
            np.testing.assert_array_equal(batch.debug_conditioned_rows(q, meanflux)[0], plain[q][0])
        print(f"k {k} lines {nl} meanflux {meanflux}: {checked} row entries compared bitwise")
    finally:
        batch.close()
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# one conditioned batch per (configuration, preparation, F): processed, refined at 1 .. L levels
# ---------------------------------------------------------------------------------------------------------------

_RUNS = {}


def run(cfg, variant, F, **params):
    key = (cfg, variant, F, tuple(sorted(params.items())))
    if key not in _RUNS:
        k, nl, Sr, L = cfg
        model, samples, spectra, _ = CC.make_batch(k, nl)
        p = VARIANTS[variant](nl, **params)
        lists = CC.parity_lists(k, nl, F) if F is not None else None
        ctx, batch = _open(p, model, samples, spectra, Sr)
        try:
            if lists is not None:
                batch.set_fixed_absorbers(conditional.csr_of(lists))
            batch.process()
            first = batch.download()
            levels = [batch.refine(levels=l + 1, delta=CC.DELTA, pad=CC.PAD) for l in range(L)]
            summ = batch.parameter_summaries(refined=True, probabilities=PROBS, thresholds=THRESH)
            after = batch.download()
        finally:
            batch.close()
            ctx.close()
        _RUNS[key] = dict(first=first, levels=levels, summ=summ, after=after, lists=lists)
    return _RUNS[key]


def _oracle_params(nl):
    from oracle import oracle
    return oracle.OracleParams(num_lines=nl)


@pytest.mark.parametrize("cfg", CC.CONFIGS)
def test_no_fixed_absorber_is_the_unconditioned_batch(cfg):
    """F = 0 on process_qsos.m's rows: every result, first pass and refined, equals an ordinary batch's bit for bit; on a
    batch that mixes quasars with and without fixed absorbers, the quasars without equal the ordinary batch's too."""
    plain, empty = run(cfg, "single", None), run(cfg, "single", 0)
    _same(empty["first"], plain["first"], FIRST)
    _same(empty["levels"][-1], plain["levels"][-1], REFINED)
    k, nl, Sr, L = cfg
    model, samples, spectra, _ = CC.make_batch(k, nl)
    lists = [x if q % 2 else [] for q, x in enumerate(CC.parity_lists(k, nl, 3))]
    ctx, batch = _open(Parameters(num_lines=nl), model, samples, spectra, Sr)
    try:
        batch.set_fixed_absorbers(conditional.csr_of(lists))
        batch.process()
        mixed = batch.download()
        mixed_ref = batch.refine(levels=L, delta=CC.DELTA, pad=CC.PAD)
    finally:
        batch.close()
        ctx.close()
    even, odd = np.arange(0, len(spectra), 2), np.arange(1, len(spectra), 2)
    _same(mixed, plain["first"], FIRST, even, even)
    _same(mixed_ref, plain["levels"][-1], REFINED, even, even)
    full = run(cfg, "single", 3)
    _same(mixed, full["first"], FIRST, odd, odd)
    _same(mixed_ref, full["levels"][-1], REFINED, odd, odd)


def _reference_tables(cfg, variant, F, q):
    """(table_at(z, log N), null) of the CPU route that matches the preparation."""
    k, nl, Sr, L = cfg
    model, samples, spectra, _ = CC.make_batch(k, nl)
    r = run(cfg, variant, F)
    fixed = r["lists"][q]
    mn, mx = r["first"]["min_z_dlas"][q], r["first"]["max_z_dlas"][q]
    if variant == "single":
        rows = CR.dense_rows(model, spectra[q], _oracle_params(nl))
        state = {}

        def table_at(z, log_n):
            t, state["null"] = CR.dense_table(rows, nl, z, 10.0 ** np.asarray(log_n), fixed, SEP)
            return t
        return table_at, state
    return CR.twin_table(model, spectra[q], _oracle_params(nl), mn, mx, fixed, SEP, prev_tau_0=0.0023 if variant == "meanflux" else 0.0)


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("cfg", CC.CONFIGS)
def test_conditional_table_against_the_oracle(cfg, variant, F):
    k, nl, Sr, L = cfg
    _, samples, _, _ = CC.make_batch(k, nl)
    r = run(cfg, variant, F)
    u, v = CC.halton_points(Sr)
    worst = worst_null = 0.0
    compared = inside = 0
    for q, kind in enumerate(CC.KINDS):
        if kind in ("status1", "status3"):   # (the oracle, like the reference, does not look at noise variances)
            assert r["first"]["status"][q] == (1 if kind == "status1" else 3)
            assert np.isnan(r["first"]["sample_log_likelihoods_dla"][q]).all() and np.isnan(r["first"]["log_likelihoods_no_dla"][q])
            assert r["levels"][-1]["status"][q] == 1
            continue
        table_at, state = _reference_tables(cfg, variant, F, q)
        mn, mx = r["first"]["min_z_dlas"][q], r["first"]["max_z_dlas"][q]
        pairs = [(r["first"]["sample_log_likelihoods_dla"][q], mn + (mx - mn) * samples["offset_samples"], samples["log_nhi_samples"])]
        for l in (0, L - 1):   # the widest and the narrowest box
            b = r["levels"][l]["boxes"][q, l]
            pairs.append((r["levels"][l]["sample_log_likelihoods_refined"][q], b[0] + (b[1] - b[0]) * u, b[2] + (b[3] - b[2]) * v))
        for got, z, n in pairs:
            want = table_at(z, n)
            np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want), err_msg=kind)   # the oracle's NaN pattern
            np.testing.assert_array_equal(np.isneginf(got), CR.close(z, r["lists"][q], SEP), err_msg=kind)
            ok = ~np.isneginf(want)
            assert not np.isnan(got).any() and not np.isnan(want).any(), kind
            if ok.any():
                worst = max(worst, float(np.abs(got[ok] - want[ok]).max()))
            compared += int(ok.sum())
            inside += int((~ok).sum())
        worst_null = max(worst_null, abs(r["first"]["log_likelihoods_no_dla"][q] - state["null"]))
    print(f"k {k} lines {nl} S' {Sr} {variant} F {F}: {compared} conditional log-likelihoods ({inside} inside the separation), "
          f"worst |delta| vs the oracle {worst:.3e}; log_likelihoods_no_dla {worst_null:.3e}")
    assert inside > 0 and worst <= 1e-8 and worst_null <= 1e-8


def _check_against_the_restatement(tag, kinds, first, levels_runs, lists, samples, u, v, L, summ=None):
    """Boxes bitwise, lambda / log Z_ref / MAP by DESIGN.md 4.18's rules, on the GPU's own tables; the separation rule's
    pattern on every table; the refined summaries against tests/posterior_restatement.py."""
    full = levels_runs[-1]
    rows = {}
    for dtype in (np.float64, np.longdouble):
        rows[dtype] = [RR.refine_row(first["sample_log_likelihoods_dla"][i], samples["offset_samples"], samples["log_nhi_samples"],
                                     first["min_z_dlas"][i], first["max_z_dlas"][i], int(first["status"][i] != 0), u, v,
                                     lambda lev, z, n, i=i: levels_runs[lev]["sample_log_likelihoods_refined"][i], L, CC.DELTA, CC.PAD,
                                     dtype=dtype) for i in range(len(kinds))]
    f64, ext = rows[np.float64], rows[np.longdouble]
    usable = 0
    for i, kind in enumerate(kinds):
        np.testing.assert_array_equal(full["boxes"][i], f64[i]["boxes"], err_msg=kind)
        assert full["status"][i] == f64[i]["status"], kind
        if f64[i]["status"]:
            continue
        usable += 1
        for lev in range(L):   # the rule on l' of every level, from the level's own box
            b = full["boxes"][i, lev]
            got = levels_runs[lev]["sample_log_likelihoods_refined"][i]
            np.testing.assert_array_equal(np.isneginf(got), CR.close(b[0] + (b[1] - b[0]) * u, lists[i], SEP), err_msg=f"{kind} level {lev}")
        lam64 = np.asarray(f64[i]["lam"][-1], dtype=np.float64)
        fin = np.isfinite(lam64)   # (-inf inside the separation)
        tol_lam, dis_lam = RR.tolerance(lam64[fin], np.asarray(ext[i]["lam"][-1])[fin], float(np.max(np.abs(lam64[fin]))))
        got = full["sample_log_posteriors_refined"][i]
        np.testing.assert_array_equal(np.isneginf(got), ~fin)
        assert not np.isnan(got).any()
        dev = float(np.max(np.abs(got[fin].astype(np.longdouble) - np.asarray(ext[i]["lam"][-1])[fin])))
        tol_z, dis_z = RR.tolerance(f64[i]["log_z"], ext[i]["log_z"], abs(float(ext[i]["log_z"])))
        dz = abs(float(full["log_likelihoods_dla_refined"][i] - ext[i]["log_z"]))
        print(f"{tag} {kind}: lambda f64 vs extended {dis_lam:.2e} tolerance {tol_lam:.2e} GPU worst {dev:.2e}; log Z_ref "
              f"{float(ext[i]['log_z']):.6f} f64 vs extended {dis_z:.2e} tolerance {tol_z:.2e} GPU {dz:.2e}; ambiguity {f64[i]['ambiguity']:.3g}")
        assert dev <= tol_lam and dz <= tol_z, kind
        if f64[i]["ambiguity"] > tol_lam:
            assert full["MAP_inds_refined"][i] == f64[i]["map_ind"], kind
            assert full["MAP_z_dlas_refined"][i] == f64[i]["map_z"] and full["MAP_log_nhis_refined"][i] == f64[i]["map_n"], kind
        if summ is None:
            continue
        lam, box = full["sample_log_posteriors_refined"][i], full["boxes"][i, -1]
        n = box[2] + (box[3] - box[2]) * v
        ref = [PR.summaries(lam[None, :], u, n, box[:1], box[1:2], probabilities=PROBS, thresholds=THRESH, extended=e) for e in (False, True)]
        assert summ["status"][i, 0] == ref[0]["status"][0, 0] == 0, kind
        w, z, ln = PR.slot_table(lam[None, :], u, n, box[:1], box[1:2], None, 0, 1, 0)
        for name, vals in (("quantiles_z", z), ("quantiles_log_nhi", ln)):
            for qi, ok_vals in enumerate(PR.acceptable_values(vals, w, PROBS)):
                assert summ[name][i, 0, 0, qi] in ok_vals, f"{kind} {name} p {PROBS[qi]}"
        zs, ns = max(abs(box[0]), abs(box[1])), float(np.max(np.abs(n)))
        for name, scale in dict(mean_z=zs, std_z=zs, mean_log_nhi=ns, std_log_nhi=ns, cov=zs * ns, exceedance=1.0,
                                effective_samples=float(ref[1]["effective_samples"][0, 0])).items():
            dis = float(np.max(np.abs(ref[0][name][0] - ref[1][name][0]))) / scale
            tol = min(max(10 * dis, 1e-13), 1e-9)
            dv = float(np.max(np.abs(summ[name][i] - ref[1][name][0]))) / scale
            assert dv <= tol, (kind, name, dv, tol)
    return f64, usable


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("cfg", CC.CONFIGS)
def test_refine_contract_on_a_conditioned_batch(cfg, F):
    k, nl, Sr, L = cfg
    _, samples, _, _ = CC.make_batch(k, nl)
    r = run(cfg, "meanflux0", F)
    u, v = CC.halton_points(Sr)
    _, usable = _check_against_the_restatement(f"k {k} lines {nl} S' {Sr} F {F}", CC.KINDS, r["first"], r["levels"], r["lists"], samples, u, v, L,
                                               r["summ"])
    assert usable == len(CC.KINDS) - 2
    for l in range(L):   # a call with fewer levels makes the leading boxes
        np.testing.assert_array_equal(r["levels"][l]["boxes"], r["levels"][-1]["boxes"][:, :l + 1])
    _same(r["after"], r["first"], FIRST)   # the refine pass leaves the first pass's results alone
    ess = r["summ"]["effective_samples"][:, 0]
    print(f"k {k} lines {nl} S' {Sr} F {F}: refined ESS {np.round(ess, 2)}")


# ---------------------------------------------------------------------------------------------------------------
# orchestration
# ---------------------------------------------------------------------------------------------------------------

_ORCH = {}


def orchestrated(cfg, per_batch=6):
    key = (cfg, per_batch)
    if key not in _ORCH:
        k, nl, Sr, L = cfg
        model, samples, spectra, _ = CC.make_batch(k, nl)
        _ORCH[key] = conditional.refine_conditional(model, samples, spectra, None, extra=2, rounds=2, levels=L, delta=CC.DELTA, pad=CC.PAD,
                                                    points=CC.halton_points(Sr), params=MultiParameters(num_lines=nl, prev_tau_0=0.0),
                                                    max_quasars_per_batch=per_batch, history=True)
    return _ORCH[key]


PASS_KEYS = ("map_z", "map_n", "status", "boxes", "log_likelihoods_fixed", "log_likelihoods_conditional", "log_bayes_factor", "mean_z", "std_z",
             "mean_log_nhi", "std_log_nhi", "quantiles_z", "quantiles_log_nhi", "effective_samples")


@pytest.mark.parametrize("cfg", CC.CONFIGS)
def test_every_pass_is_the_restatement_from_the_list_before_it(cfg):
    k, nl, Sr, L = cfg
    model, samples, spectra, _ = CC.make_batch(k, nl)
    out = orchestrated(cfg)
    u, v = CC.halton_points(Sr)
    lists = [[] for _ in spectra]
    names = [h["name"] for h in out["history"]]
    assert names == ["discover 0", "discover 1"] + [f"round {r} slot {j}" for r in range(2) for j in range(2)]
    for h in out["history"]:
        idx, j = h["quasars"], h["slot"]
        fixed = [list(lists[q]) if j < 0 else lists[q][:j] + lists[q][j + 1:] for q in idx]
        assert conditional.lists_of(h["fixed"], idx.size) == fixed, h["name"]   # conditioned on the GPU's own list before the pass
        ctx, batch = _open(MultiParameters(num_lines=nl, prev_tau_0=0.0), model, samples, [spectra[q] for q in idx], Sr)
        try:
            batch.set_fixed_absorbers(conditional.csr_of(fixed))
            batch.process()
            first = batch.download()
            levels = [batch.refine(levels=l + 1, delta=CC.DELTA, pad=CC.PAD) for l in range(L)]
        finally:
            batch.close()
            ctx.close()
        kinds = [CC.KINDS[q] for q in idx]
        f64, _ = _check_against_the_restatement(f"k {k} {h['name']}", kinds, first, levels, fixed, samples, u, v, L)
        # the pass as the pipeline ran it (other batches, other slots) equals this batch's, bit for bit
        np.testing.assert_array_equal(h["map_z"], levels[-1]["MAP_z_dlas_refined"])
        np.testing.assert_array_equal(h["map_n"], levels[-1]["MAP_log_nhis_refined"])
        np.testing.assert_array_equal(h["boxes"], levels[-1]["boxes"])
        np.testing.assert_array_equal(h["log_likelihoods_fixed"], first["log_likelihoods_no_dla"])
        np.testing.assert_array_equal(h["log_likelihoods_conditional"], levels[-1]["log_likelihoods_dla_refined"])
        # the restatement's orchestration step from the same list
        for i, q in enumerate(idx):
            if f64[i]["status"] != 0:
                assert h["status"][i] != 0
                continue
            new = [float(h["map_z"][i]), float(h["map_n"][i])]
            if j < 0:
                lists[q].append(new)
            else:
                lists[q][j] = new
        z, n = conditional.padded(lists, out["z_dlas"].shape[1])
        np.testing.assert_array_equal(h["z_dlas"], z, err_msg=h["name"])
        np.testing.assert_array_equal(h["log_nhis"], n, err_msg=h["name"])
    np.testing.assert_array_equal(out["z_dlas"], z)
    np.testing.assert_array_equal(out["log_nhis"], n)
    i1, i3 = CC.KINDS.index("status1"), CC.KINDS.index("status3")
    assert out["num_absorbers"][i1] == out["num_absorbers"][i3] == 0 and (out["status"][[i1, i3]] == conditional.NEVER).all()
    assert (np.delete(out["num_absorbers"], [i1, i3]) == 2).all() and (np.delete(out["discovered"], [i1, i3], 0) == 1).all()
    assert np.isnan(out["start_z_dlas"]).all() and (out["num_start"] == 0).all()
    last = out["history"][-1]   # slot 1's last pass is the last pass: what the result reports for it
    np.testing.assert_array_equal(out["log_bayes_factor"][last["quasars"], 1], last["log_bayes_factor"])
    np.testing.assert_array_equal(out["quantiles_z"][last["quasars"], 1], last["quantiles_z"])


@pytest.mark.parametrize("cfg", CC.CONFIGS)
def test_purpose_bayes_factors_and_recovery(cfg):
    k, nl, Sr, L = cfg
    _, _, _, truth = CC.make_batch(k, nl)
    out = orchestrated(cfg)
    h0, h1 = out["history"][0], out["history"][1]
    for name, _, _, _ in CC.SCIENCE:
        q = CC.KINDS.index(name)
        b0, b1 = h0["log_bayes_factor"][q], h1["log_bayes_factor"][q]
        print(f"k {k} lines {nl} S' {Sr} {name}: log Bayes factor of one more absorber, nothing fixed {b0:.2f}, first absorber fixed {b1:.2f}; "
              f"ESS per slot {np.round(out['effective_samples'][q], 2)}")
        if name == "none":
            assert b0 < 0 and b1 < 0
        else:
            assert b0 > 300 and (b1 > 100 if name in CC.TWO else b1 < 0), name
        for z, ln in truth[q]:
            dz, dn = min((abs(out["z_dlas"][q, s] - z), abs(out["log_nhis"][q, s] - ln)) for s in range(out["num_absorbers"][q]))
            print(f"    injected ({z:.5f}, {ln}): nearest slot |dz| {dz:.2e} |dlogN| {dn:.3f}")
            assert dz <= 3e-3 and dn <= 0.25, name
            assert (out["effective_samples"][q, :2] > 1.0).all()


# ---------------------------------------------------------------------------------------------------------------
# invariances and refusals
# ---------------------------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_batching_selection_groups_or_run():
    cfg = CC.CONFIGS[0]
    k, nl, Sr, L = cfg
    six, two = orchestrated(cfg, 6), orchestrated(cfg, 2)
    for key, val in six.items():
        if key != "history":
            np.testing.assert_array_equal(two[key], val, err_msg=key)
    for a, b in zip(six["history"], two["history"]):
        _same(a, b, PASS_KEYS + ("z_dlas", "log_nhis"))
    whole = run(cfg, "meanflux0", 3)
    model, samples, spectra, _ = CC.make_batch(k, nl)
    kw = dict(levels=L, delta=CC.DELTA, pad=CC.PAD)
    ctx, batch = _open(MultiParameters(num_lines=nl, prev_tau_0=0.0), model, samples, spectra, Sr)
    try:
        batch.set_fixed_absorbers(conditional.csr_of(whole["lists"]))
        batch.process()
        _same(batch.download(), whole["first"], FIRST)                       # a second run
        back = batch.refine(selection=np.arange(len(spectra))[::-1], **kw)
        _same(back, whole["levels"][-1], REFINED, rows_a=slice(None, None, -1))
        _same(batch.refine(selection=[4, 0, 4], **kw), whole["levels"][-1], REFINED, rows_b=[4, 0, 4])
        # clear restores the unconditioned results bit for bit; the conditioned ones are gone with it
        batch.set_fixed_absorbers(None)
        with pytest.raises(_lib.GpdlaError, match="not been processed"):
            batch.refine(**kw)
        batch.process()
        plain = run(cfg, "meanflux0", None)   # (an ordinary batch has process_qsos.m's rows, whatever the context's parameters)
        _same(batch.download(), plain["first"], FIRST)
        _same(batch.refine(**kw), plain["levels"][-1], REFINED)
        # reload clears
        batch.set_fixed_absorbers(conditional.csr_of(whole["lists"]))
        batch.reload(spectra, np.full(len(spectra), np.log(0.9)), np.full(len(spectra), np.log(0.1)))
        batch.process()
        _same(batch.download(), plain["first"], FIRST)
        batch.model_spectra(products=("map",))   # an unconditioned batch again: served
    finally:
        batch.close()
        ctx.close()
    # a record pool that holds less than the batch's records: two or more groups, built and swept in turn
    pixels = [r[2] for r in CC.SCIENCE + CC.EXTRA]
    records = sum((p + 4 + 3) // 4 + 1 for p in pixels)
    budget = records // 2 + 8
    assert max((p + 4 + 3) // 4 + 1 for p in pixels) <= budget < records
    small = run(cfg, "meanflux0", 3, record_pool_bytes=896 * budget)
    _same(small["first"], whole["first"], FIRST)
    _same(small["levels"][-1], whole["levels"][-1], REFINED)


def test_refusals():
    k, nl, Sr, L = CC.CONFIGS[0]
    model, samples, spectra, _ = CC.make_batch(k, nl)
    lists = conditional.csr_of(CC.parity_lists(k, nl, 2))
    ctx, batch = _open(MultiParameters(num_lines=nl), model, samples, spectra, Sr)
    try:
        batch.set_fixed_absorbers(lists)
        for call in (lambda: batch.model_spectra(products=("map",)), batch.draw_mocks, batch.unmasked_counts, batch.debug_prepared_rows):
            with pytest.raises(_lib.GpdlaError, match="conditioned on fixed absorbers") as e:
                call()
            assert e.value.code == _lib.ERR_UNSUPPORTED
        # a refused list names the quasar and leaves the batch as it was
        off, z, ln = (a.copy() for a in lists)
        z[3] = z[2] + 0.25 * SEP
        with pytest.raises(_lib.GpdlaError, match="quasar 1") as e:
            batch.set_fixed_absorbers((off, z, ln))
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
        with pytest.raises(_lib.GpdlaError, match="offsets"):
            batch.set_fixed_absorbers((off[:-1], z, ln))
        batch.process()
        np.testing.assert_array_equal(batch.download()["log_likelihoods_no_dla"], run(CC.CONFIGS[0], "meanflux", 2)["first"]["log_likelihoods_no_dla"])
    finally:
        batch.close()
        ctx.close()
    ctx, batch = _open(Parameters(num_lines=nl, contraction_precision=1), model, samples, spectra, Sr)   # the fp32 study class
    try:
        with pytest.raises(_lib.GpdlaError, match="fp64 only") as e:
            batch.set_fixed_absorbers(lists)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        batch.close()
        ctx.close()
    ctx = gp.Context(0, Parameters())   # k = 41 never reaches a batch: the context refuses the model (GPDLA_MAX_K = 40)
    try:
        with pytest.raises(_lib.GpdlaError) as e:
            ctx.set_model(synthetic.make_model(41))
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        ctx.close()
    ctx = gp.Context(0, MultiParameters(max_dlas=2))
    ctx.set_model(model)
    ctx.set_samples(samples)
    batch = ctx.upload(spectra[:2], np.full(2, np.log(0.8)), np.log(np.full((2, 2), 0.1)), np.full(2, np.log(0.05)))
    try:
        with pytest.raises(_lib.GpdlaError, match="single-DLA") as e:
            batch.set_fixed_absorbers((np.array([0, 1, 1]), np.array([2.5]), np.array([20.5])))
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        batch.close()
        ctx.close()


def test_command_line_equals_refine_multi_absorbers(tmp_path):
    files = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=12, num_samples=64, empty_quasar=3)
    paths, test_ind = files["paths"], files["test_ind"]
    spectra = [s for s, t in zip(files["spectra"], test_ind) if t]
    p = MultiParameters(max_dlas=2)
    cat = synthetic.make_prior_catalog()
    lp = gp.dla_existence_prior_multi(cat["z_qsos"], cat["dla_ind"], np.array([s["z_qso"] for s in spectra]), 0.31, 0.69, p)
    samples = io.load_dla_samples(paths["samples"])
    model = io.load_learned_model(paths["learned"])
    results = gp.process_qsos_multiple_dlas_meanflux(model, samples, spectra, lp, params=p)
    processed, out = str(tmp_path / "processed_multi.mat"), str(tmp_path / "conditional.mat")
    io.save_processed_qsos_multi(processed, results, test_ind=test_ind, k=20, num_dla_samples=64, test_set_name="synth")
    args = [paths["preloaded"], paths["catalog"], paths["learned"], paths["samples"], processed, out, "--rounds", "1", "--extra", "1",
            "--levels", "2", "--points", "50", "--batch", "4"]
    assert conditional.main(args) == 0
    from gp_dla_detection_amd import refine
    want = api.refine_multi_absorbers(model, samples, io.load_preloaded_qsos(paths["preloaded"], io.load_catalog(paths["catalog"], names=("z_qsos",))["z_qsos"],
                                                                               np.asarray(test_ind, dtype=bool)),
                                      io.load_processed_qsos(processed), extra=1, rounds=1, levels=2, points=refine.default_points(50),
                                      params=MultiParameters(num_lines=3))
    back = io.load_conditional_results(out)
    assert want["num_start"].sum() >= 2 and want["num_absorbers"].sum() > want["num_start"].sum()
    for key, val in want.items():
        np.testing.assert_array_equal(back[key], val, err_msg=key)
