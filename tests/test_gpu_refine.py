"""GPU checks of the refine pass on the synthetic batch of tests/refine_cases.py: k = 8 with
three lines (k_sweep_slim_boxed<3>, 896-B records) and k = 24 with five (k_sweep_split_slim<0, 0,
BoxedSweepArgs>, 1536-B records), S = 200, S' in {127, 128, 300}, four levels.

 - boxes of every level == the restatement (tests/refine_restatement.py) fed the GPU's own tables, bitwise;
 - l' against the CPU oracle at the GPU's own (z', N'): 1e-8 absolute, the project's parity bound;
 - lambda, log Z_ref and the MAP against the restatement on the GPU's l': 10 x the restatement's own
   float64-versus-longdouble disagreement, floored at 1e-13 relative; the MAP index exactly wherever the two
   largest lambda differ by more than that;
 - the refined summaries against tests/posterior_restatement.py on (lambda, z', n') by the acceptance
   statements of test_gpu_posteriors.py;
 - determinism, record groups, the first pass untouched, the purpose (ESS grows, the interval holds the
   injected absorber) and the command line.
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, io, refine, samples as samples_mod, synthetic
from gp_dla_detection_amd.parameters import Parameters

import posterior_restatement as PR
import refine_cases as RC
import refine_restatement as RR

pytestmark = pytest.mark.gpu

PROBS, THRESH = (0.025, 0.16, 0.5, 0.84, 0.975), (20.3, 21.0)
SCALARS = refine.SCALARS + ("boxes", "status") + refine.TABLES
ALL = [(k, nl, Sr) for k, nl in RC.CONFIGS for Sr in RC.SR_VALUES]
_RUNS = {}


def _context(k, nl, Sr, zero_range=False, **params):
    model, samples, spectra, truth = RC.make_batch(k, nl, zero_range)
    if zero_range:
        params["max_z_cut"] = 0.0
    ctx = gp.Context(0, Parameters(num_lines=nl, **params))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(Sr))
    n = len(spectra)
    batch = ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))
    return ctx, batch


def _same(a, b, keys=SCALARS, rows_a=slice(None), rows_b=slice(None)):
    for key in keys:
        np.testing.assert_array_equal(a[key][rows_a], b[key][rows_b], err_msg=key)   # NaN pattern included


def run(k, nl, Sr):
    """One context per configuration: the first pass, refine at 1 .. LEVELS levels (level l's tables are
    resident only after a call with l levels), the summaries, and the first pass's results read again."""
    key = (k, nl, Sr)
    if key not in _RUNS:
        ctx, batch = _context(k, nl, Sr)
        try:
            batch.process()
            first = batch.download()
            first_summ = batch.parameter_summaries(probabilities=PROBS, thresholds=THRESH)
            levels = [batch.refine(levels=l + 1, delta=RC.DELTA, pad=RC.PAD) for l in range(RC.LEVELS)]
            summ = batch.parameter_summaries(refined=True, probabilities=PROBS, thresholds=THRESH)
            again = batch.refine(levels=RC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
            after = batch.download()
        finally:
            batch.close()
            ctx.close()
        _RUNS[key] = dict(first=first, first_summ=first_summ, levels=levels, summ=summ, again=again, after=after)
    return _RUNS[key]


def _restated(k, nl, Sr, dtype=np.float64, gpu_lambda=True):
    """The restatement per quasar on the GPU's own tables: l' of every level as the sweep and, with
    ``gpu_lambda``, the GPU's lambda as the source of the next box (else the restatement's own)."""
    r = run(k, nl, Sr)
    _, samples, _, _ = RC.make_batch(k, nl)
    u, v = RC.halton_points(Sr)
    rows = []
    for i in range(len(RC.KINDS)):
        rows.append(RR.refine_row(
            r["first"]["sample_log_likelihoods_dla"][i], samples["offset_samples"], samples["log_nhi_samples"],
            r["first"]["min_z_dlas"][i], r["first"]["max_z_dlas"][i], int(r["first"]["status"][i]), u, v,
            lambda lev, z, n, i=i: r["levels"][lev]["sample_log_likelihoods_refined"][i], RC.LEVELS, RC.DELTA, RC.PAD,
            dtype=dtype, lam_tables=[lv["sample_log_posteriors_refined"][i] for lv in r["levels"]] if gpu_lambda else None))
    return rows


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_boxes_equal_the_restatement(k, nl, Sr):
    r = run(k, nl, Sr)
    full = r["levels"][-1]
    rows = _restated(k, nl, Sr)
    for i, kind in enumerate(RC.KINDS):
        np.testing.assert_array_equal(full["boxes"][i], rows[i]["boxes"], err_msg=kind)
        assert full["status"][i] == rows[i]["status"], kind
        for l in range(RC.LEVELS):   # a call with fewer levels makes the leading boxes
            np.testing.assert_array_equal(r["levels"][l]["boxes"][i], full["boxes"][i, :l + 1], err_msg=f"{kind} level {l + 1}")
    st = dict(zip(RC.KINDS, full["status"]))
    assert st["status1"] == 1 and st["status3"] == 1 and all(st[x] == 0 for x in RC.KINDS if not x.startswith("status"))
    for kind in ("status1", "status3"):
        i = RC.KINDS.index(kind)
        assert all(np.isnan(full[key][i]).all() for key in SCALARS if key != "status"), kind
    box = full["boxes"][~np.isnan(full["boxes"][:, 0, 0])]
    assert (box[:, 1:, 0] >= box[:, :-1, 0]).all() and (box[:, 1:, 1] <= box[:, :-1, 1]).all()   # nested
    assert (box[:, 1:, 2] >= box[:, :-1, 2]).all() and (box[:, 1:, 3] <= box[:, :-1, 3]).all()
    print(f"k {k} lines {nl} S' {Sr}: last z widths {box[:, -1, 1] - box[:, -1, 0]}, log N widths {box[:, -1, 3] - box[:, -1, 2]}")


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_refined_log_likelihoods_against_the_oracle(k, nl, Sr):
    r = run(k, nl, Sr)
    model, samples, spectra, _ = RC.make_batch(k, nl)
    u, v = RC.halton_points(Sr)
    worst, compared = 0.0, 0
    for i, kind in enumerate(RC.KINDS):
        if r["levels"][-1]["status"][i]:
            continue
        sweep = RR.oracle_sweep(model, spectra[i], r["first"]["min_z_dlas"][i], r["first"]["max_z_dlas"][i], nl)
        for l in (0, RC.LEVELS - 1):   # the widest and the narrowest box
            b = r["levels"][l]["boxes"][i, l]
            want = sweep(l, b[0] + (b[1] - b[0]) * u, b[2] + (b[3] - b[2]) * v)
            got = r["levels"][l]["sample_log_likelihoods_refined"][i]
            ok = ~np.isnan(want)   # (no exclusion but what the oracle itself returns as NaN)
            assert ok.any() and not np.isnan(got[ok]).any(), kind
            worst = max(worst, float(np.abs(got[ok] - want[ok]).max()))
            compared += int(ok.sum())
    print(f"k {k} lines {nl} S' {Sr}: {compared} refined log-likelihoods, worst |delta| vs the oracle {worst:.3e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_lambda_evidence_and_map_against_the_restatement(k, nl, Sr):
    r = run(k, nl, Sr)
    full = r["levels"][-1]
    f64, ext = _restated(k, nl, Sr, gpu_lambda=False), _restated(k, nl, Sr, np.longdouble, gpu_lambda=False)
    ambiguous = compared = 0
    for i, kind in enumerate(RC.KINDS):
        if f64[i]["status"]:
            continue
        # (the restatement's own lambda led it to the boxes whose l' it was handed)
        np.testing.assert_array_equal(f64[i]["boxes"], full["boxes"][i], err_msg=kind)
        np.testing.assert_array_equal(ext[i]["boxes"], full["boxes"][i], err_msg=kind)
        lam_scale = float(np.nanmax(np.abs(np.asarray(f64[i]["lam"][-1], dtype=np.float64))))
        tol_lam, dis_lam = RR.tolerance(f64[i]["lam"][-1], ext[i]["lam"][-1], lam_scale)
        got = full["sample_log_posteriors_refined"][i]
        with np.errstate(invalid="ignore"):
            dev = np.abs(got.astype(np.longdouble) - ext[i]["lam"][-1])
        np.testing.assert_array_equal(np.isnan(got), np.isnan(np.asarray(ext[i]["lam"][-1], dtype=np.float64)))
        tol_z, dis_z = RR.tolerance(f64[i]["log_z"], ext[i]["log_z"], abs(float(ext[i]["log_z"])))
        dz = abs(float(full["log_likelihoods_dla_refined"][i] - ext[i]["log_z"]))
        print(f"k {k} lines {nl} S' {Sr} {kind}: lambda f64 vs extended {dis_lam:.2e} tolerance {tol_lam:.2e} GPU worst "
              f"{float(np.nanmax(dev)):.2e}; log Z_ref {float(ext[i]['log_z']):.6f} f64 vs extended {dis_z:.2e} tolerance {tol_z:.2e} GPU {dz:.2e}")
        assert float(np.nanmax(dev)) <= tol_lam and dz <= tol_z, kind
        assert full["log_posteriors_dla_refined"][i] == np.log(0.1) + full["log_likelihoods_dla_refined"][i]
        compared += 1
        if f64[i]["ambiguity"] > tol_lam:
            assert full["MAP_inds_refined"][i] == f64[i]["map_ind"], kind
            assert full["MAP_z_dlas_refined"][i] == f64[i]["map_z"] and full["MAP_log_nhis_refined"][i] == f64[i]["map_n"], kind
        else:
            ambiguous += 1
    print(f"MAP: {compared} rows compared, {ambiguous} ambiguous")
    assert compared == 6 and ambiguous == 0   # (tests/test_refine.py asserts the share on the twin)


def _summary_reference(lam, u, n, box, extended):
    return PR.summaries(lam[None, :], u, n, np.array([box[0]]), np.array([box[1]]), probabilities=PROBS, thresholds=THRESH,
                        extended=extended)


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_refined_summaries_against_the_posterior_restatement(k, nl, Sr):
    r = run(k, nl, Sr)
    full, summ = r["levels"][-1], r["summ"]
    u, v = RC.halton_points(Sr)
    for i, kind in enumerate(RC.KINDS):
        lam, box = full["sample_log_posteriors_refined"][i], full["boxes"][i, -1]
        n = box[2] + (box[3] - box[2]) * v
        f64, ext = _summary_reference(lam, u, n, box, False), _summary_reference(lam, u, n, box, True)
        assert summ["status"][i, 0] == f64["status"][0, 0], kind
        if full["status"][i]:
            assert summ["status"][i, 0] == 3 and np.isnan(summ["mean_z"][i]).all() and np.isnan(summ["quantiles_log_nhi"][i]).all()
            continue
        w, z, ln = PR.slot_table(lam[None, :], u, n, box[:1], box[1:2], None, 0, 1, 0)
        for qy, (name, vals) in enumerate((("quantiles_z", z), ("quantiles_log_nhi", ln))):
            for q, ok_vals in enumerate(PR.acceptable_values(vals, w, PROBS)):
                got = summ[name][i, 0, 0, q]
                assert got in ok_vals, f"{kind} {name} p {PROBS[q]}: {got!r} not in {ok_vals!r}"
                if ok_vals.size == 1:
                    assert got == f64[name][0, 0, 0, q]
        zs, ns = max(abs(box[0]), abs(box[1])), float(np.max(np.abs(n)))
        scales = dict(mean_z=zs, std_z=zs, mean_log_nhi=ns, std_log_nhi=ns, cov=zs * ns, exceedance=1.0,
                      effective_samples=float(ext["effective_samples"][0, 0]))
        for name, scale in scales.items():
            dis = float(np.max(np.abs(f64[name][0] - ext[name][0]))) / scale
            tol = min(max(10 * dis, 1e-13), 1e-9)
            dev = float(np.max(np.abs(summ[name][i] - ext[name][0]))) / scale
            print(f"k {k} lines {nl} S' {Sr} {kind} {name}: restatement f64 vs extended {dis:.2e}, tolerance {tol:.2e}, GPU {dev:.2e} (scale units)")
            assert dev <= tol, (kind, name)
        assert box[0] <= summ["quantiles_z"][i, 0, 0, 0] <= summ["quantiles_z"][i, 0, 0, -1] <= box[1]
        assert box[2] <= summ["quantiles_log_nhi"][i, 0, 0, 0] <= summ["quantiles_log_nhi"][i, 0, 0, -1] <= box[3]


@pytest.mark.parametrize("k,nl,Sr", [(8, 3, 127), (24, 5, 300)])
def test_results_do_not_depend_on_selection_order_groups_or_run(k, nl, Sr):
    r = run(k, nl, Sr)
    whole = r["levels"][-1]
    _same(whole, r["again"])
    kw = dict(levels=RC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
    n = len(RC.KINDS)
    ctx, batch = _context(k, nl, Sr)
    try:
        batch.process()
        back = batch.refine(selection=np.arange(n)[::-1], **kw)
        _same(back, whole, rows_a=slice(None, None, -1))
        twice = batch.refine(selection=[3, 0, 3], **kw)   # a duplicate is served once and reported twice
        _same(twice, whole, rows_b=[3, 0, 3])
        other = batch.download_refined([1], RC.LEVELS)     # outside the last selection: not refined
        assert other["status"][0] == _lib.REFINE_NOT_REFINED and np.isnan(other["log_likelihoods_dla_refined"][0])
        for i in range(n):
            _same(batch.refine(selection=[i], **kw), whole, rows_b=[i])
    finally:
        batch.close()
        ctx.close()
    # a record pool that holds less than the batch's records: two or more groups, built and swept in turn
    per_step = 896 if k <= 20 else 1536
    records = sum((p + 4 + 3) // 4 + 1 for p in RC.PIXELS)
    budget = records // 2 + 8   # records the pool holds: host_sweep.hpp plan_records, record_pool_bytes / (bytes a record)
    assert max((p + 4 + 3) // 4 + 1 for p in RC.PIXELS) <= budget < records   # every quasar fits, the batch does not
    ctx, batch = _context(k, nl, Sr, record_pool_bytes=per_step * budget)
    try:
        batch.process()
        _same(batch.refine(**kw), whole)
    finally:
        batch.close()
        ctx.close()


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_first_pass_results_are_untouched(k, nl, Sr):
    r = run(k, nl, Sr)
    for key, val in r["first"].items():
        np.testing.assert_array_equal(r["after"][key], val, err_msg=key)


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_purpose_peaked_rows_gain_samples_and_hold_the_truth(k, nl, Sr):
    r = run(k, nl, Sr)
    _, _, _, truth = RC.make_batch(k, nl)
    lo, hi = PROBS.index(0.025), PROBS.index(0.975)
    for kind in RC.PEAKED:
        i = RC.KINDS.index(kind)
        e0 = r["first_summ"]["effective_samples"][i, 0]
        es = [RC.ess(lv["sample_log_posteriors_refined"][i]) for lv in r["levels"]]
        qz, qn = r["summ"]["quantiles_z"][i, 0, 0], r["summ"]["quantiles_log_nhi"][i, 0, 0]
        print(f"k {k} lines {nl} S' {Sr} {kind}: ESS first pass {e0:.5f}, levels {np.round(es, 3)}; z in [{qz[lo]:.6f}, {qz[hi]:.6f}] "
              f"truth {truth[i][0]:.6f}; log N in [{qn[lo]:.4f}, {qn[hi]:.4f}] truth {truth[i][1]}")
        assert r["summ"]["effective_samples"][i, 0] > e0
        assert abs(r["summ"]["effective_samples"][i, 0] - es[-1]) <= 1e-9 * es[-1]
        assert qz[lo] <= truth[i][0] <= qz[hi] and qn[lo] <= truth[i][1] <= qn[hi], kind


def test_zero_width_boxes():
    """pad = 0 and a delta that only the maximum meets: A is one sample, the box is that point, every refine
    point is swept at the same (z, N), the box holds no prior volume (Z_ref is what lies outside it) and the
    next level stays on the point."""
    k, nl, Sr = 8, 3, 127
    model, samples, spectra, _ = RC.make_batch(k, nl)
    u, v = RC.halton_points(Sr)
    ctx, batch = _context(k, nl, Sr)
    try:
        batch.process()
        first = batch.download()
        one = batch.refine(levels=1, delta=1e-9, pad=0.0)
        two = batch.refine(levels=2, delta=1e-9, pad=0.0)
    finally:
        batch.close()
        ctx.close()
    for i, kind in enumerate(RC.KINDS):
        sll = first["sample_log_likelihoods_dla"][i]
        row = RR.refine_row(sll, samples["offset_samples"], samples["log_nhi_samples"], first["min_z_dlas"][i],
                            first["max_z_dlas"][i], int(first["status"][i]), u, v,
                            lambda lev, z, n, i=i: (one, two)[lev]["sample_log_likelihoods_refined"][i], 2, 1e-9, 0.0,
                            lam_tables=[one["sample_log_posteriors_refined"][i], two["sample_log_posteriors_refined"][i]])
        np.testing.assert_array_equal(two["boxes"][i], row["boxes"], err_msg=kind)
        if row["status"]:
            continue
        j = int(np.nanargmax(sll))
        b = two["boxes"][i]
        assert b[0, 0] == b[0, 1] == first["MAP_z_dlas"][i] and b[0, 2] == b[0, 3] == samples["log_nhi_samples"][j], kind
        np.testing.assert_array_equal(b[1], b[0])
        ell = one["sample_log_likelihoods_refined"][i]
        assert np.abs(ell - sll[j]).max() <= 1e-8, kind          # the first pass's own maximum, S' times
        want = RR.refine_row(sll, samples["offset_samples"], samples["log_nhi_samples"], first["min_z_dlas"][i],
                             first["max_z_dlas"][i], 0, u, v, lambda lev, z, n: ell, 1, 1e-9, 0.0, dtype=np.longdouble)["log_z"]
        got = one["log_likelihoods_dla_refined"][i]
        print(f"{kind}: zero-width box at ({b[0, 0]:.6f}, {b[0, 2]:.4f}); log Z_ref {got:.6f}, restatement {float(want):.6f}")
        assert abs(got - float(want)) <= 1e-13 * max(abs(got), 1.0) or (np.isinf(got) and np.isinf(float(want))), kind
        assert one["MAP_inds_refined"][i] == 1.0 or np.ptp(one["sample_log_posteriors_refined"][i]) > 0


def _gpu_prior():
    d = RC.test_prior()
    return samples_mod.NhiPrior(_lib.NhiPrior(d["coeff"], d["centre"], d["alpha"], d["uniform_min"], d["uniform_max"], d["lower"],
                                              d["flat_below"], d["Z"]))


def _check_rows_against_the_restatement(tag, kinds, first, levels_runs, samples, u, v, prior, L):
    """lambda, log Z_ref and the MAP of every row against the restatement on the GPU's own l' (tolerance: 10 x the
    restatement's float64-versus-longdouble disagreement, floored at 1e-13 relative), and the boxes bitwise."""
    full = levels_runs[-1]
    rows = {}
    for dtype in (np.float64, np.longdouble):
        rows[dtype] = [RR.refine_row(first["sample_log_likelihoods_dla"][i], samples["offset_samples"], samples["log_nhi_samples"],
                                     first["min_z_dlas"][i], first["max_z_dlas"][i], int(first["status"][i]), u, v,
                                     lambda lev, z, n, i=i: levels_runs[lev]["sample_log_likelihoods_refined"][i], L, RC.DELTA,
                                     RC.PAD, prior=prior, dtype=dtype) for i in range(len(kinds))]
    f64, ext = rows[np.float64], rows[np.longdouble]
    for i, kind in enumerate(kinds):
        np.testing.assert_array_equal(full["boxes"][i], f64[i]["boxes"], err_msg=kind)
        assert full["status"][i] == f64[i]["status"], kind
        if f64[i]["status"]:
            continue
        lam_scale = float(np.nanmax(np.abs(np.asarray(f64[i]["lam"][-1], dtype=np.float64))))
        tol_lam, dis_lam = RR.tolerance(f64[i]["lam"][-1], ext[i]["lam"][-1], lam_scale)
        got = full["sample_log_posteriors_refined"][i]
        np.testing.assert_array_equal(np.isnan(got), np.isnan(np.asarray(ext[i]["lam"][-1], dtype=np.float64)))
        with np.errstate(invalid="ignore"):
            dev = float(np.nanmax(np.abs(got.astype(np.longdouble) - ext[i]["lam"][-1])))
        tol_z, dis_z = RR.tolerance(f64[i]["log_z"], ext[i]["log_z"], abs(float(ext[i]["log_z"])))
        dz = abs(float(full["log_likelihoods_dla_refined"][i] - ext[i]["log_z"]))
        print(f"{tag} {kind}: lambda f64 vs extended {dis_lam:.2e} tolerance {tol_lam:.2e} GPU worst {dev:.2e}; log Z_ref "
              f"{float(ext[i]['log_z']):.6f} f64 vs extended {dis_z:.2e} tolerance {tol_z:.2e} GPU {dz:.2e}; ambiguity {f64[i]['ambiguity']:.3g}")
        assert dev <= tol_lam and dz <= tol_z, kind
        if f64[i]["ambiguity"] > tol_lam:
            assert full["MAP_inds_refined"][i] == f64[i]["map_ind"], kind
            assert full["MAP_z_dlas_refined"][i] == f64[i]["map_z"] and full["MAP_log_nhis_refined"][i] == f64[i]["map_n"], kind
    return f64


@pytest.mark.parametrize("k,nl", RC.CONFIGS)
def test_zero_width_search_range(k, nl):
    """max_z == min_z (one kept pixel, max_z_cut = 0): the box of every level is that z, its share of the prior's z
    range counts as 1, the boxed sweep runs on a meta whose range is a point."""
    Sr, L = RC.ZR_SR, RC.LEVELS
    model, samples, spectra, _ = RC.make_batch(k, nl, zero_range=True)
    u, v = RC.halton_points(Sr)
    ctx, batch = _context(k, nl, Sr, zero_range=True)
    try:
        batch.process()
        first = batch.download()
        runs = [batch.refine(levels=l + 1, delta=RC.DELTA, pad=RC.PAD) for l in range(L)]
        summ = batch.parameter_summaries(refined=True, probabilities=PROBS, thresholds=THRESH)
    finally:
        batch.close()
        ctx.close()
    i = RC.ZR_KINDS.index("zero_range")
    z0 = first["min_z_dlas"][i]
    assert first["status"][i] == 0 and z0 == first["max_z_dlas"][i] and first["min_z_dlas"][0] < first["max_z_dlas"][0]
    full = runs[-1]
    assert full["status"][i] == 0 and (full["boxes"][i, :, :2] == z0).all() and full["MAP_z_dlas_refined"][i] == z0
    assert np.isfinite(full["log_likelihoods_dla_refined"][i])
    _check_rows_against_the_restatement(f"k {k} lines {nl} zero range", RC.ZR_KINDS, first, runs, samples, u, v, None, L)
    worst = 0.0
    for q, kind in enumerate(RC.ZR_KINDS):   # l' against the oracle at the GPU's own (z', N')
        sweep = RR.oracle_sweep(model, spectra[q], first["min_z_dlas"][q], first["max_z_dlas"][q], RC.oracle_parameters(nl, True))
        for l in (0, L - 1):
            b = runs[l]["boxes"][q, l]
            want = sweep(l, b[0] + (b[1] - b[0]) * u, b[2] + (b[3] - b[2]) * v)
            got = runs[l]["sample_log_likelihoods_refined"][q]
            assert not np.isnan(want).any() and not np.isnan(got).any(), kind
            worst = max(worst, float(np.abs(got - want).max()))
    print(f"k {k} lines {nl} zero range: worst |delta| of l' vs the oracle {worst:.3e}; ESS first pass "
          f"{RC.ess(first['sample_log_likelihoods_dla'][i]):.3f}, refined {summ['effective_samples'][i, 0]:.3f}")
    assert worst <= 1e-8
    assert summ["status"][i, 0] == 0 and (summ["quantiles_z"][i, 0, 0] == z0).all()
    # every sample has z == z0: the weighted mean Sum w z / T is z0 to the rounding of a compensated sum and one
    # division (within 2 ulp), and the standard deviation about it is at most that distance
    assert abs(summ["mean_z"][i, 0, 0] - z0) <= 2 * np.spacing(z0) and summ["std_z"][i, 0, 0] <= 2 * np.spacing(z0)
    assert np.isnan(summ["correlation"][i, 0, 0])


@pytest.mark.parametrize("k,nl", RC.CONFIGS)
def test_column_density_prior(k, nl):
    """A gpdla_nhi_prior with its breaks inside the boxes: log p_N as the GPU added it against
    gpdla_samples_prior_eval, and lambda, log Z_ref and the MAP against the restatement with the same prior."""
    Sr, L = 128, 2
    model, samples, spectra, _ = RC.make_batch(k, nl)
    u, v = RC.halton_points(Sr)
    prior, fields = _gpu_prior(), RC.test_prior()
    ctx, batch = _context(k, nl, Sr)
    try:
        batch.process()
        first = batch.download()
        runs = [batch.refine(levels=l + 1, delta=RC.DELTA, pad=RC.PAD, prior=prior) for l in range(L)]
        plain = batch.refine(levels=1, delta=RC.DELTA, pad=RC.PAD)
    finally:
        batch.close()
        ctx.close()
    _check_rows_against_the_restatement(f"k {k} lines {nl} prior", RC.KINDS, first, runs, samples, u, v, fields, L)
    below = outside = inside = 0
    for l in range(L):
        for i, kind in enumerate(RC.KINDS):
            if runs[l]["status"][i]:
                continue
            b = runs[l]["boxes"][i, l]
            n = b[2] + (b[3] - b[2]) * v
            ell, lam = runs[l]["sample_log_likelihoods_refined"][i], runs[l]["sample_log_posteriors_refined"][i]
            want = np.log(prior.pdf(n))
            # lambda - l' carries the rounding of the sum (half an ulp of lambda) and of the subtraction; log p_N itself
            # is the device's log of the device's pdf against NumPy's log of the same pdf: 1e-13 relative
            tol = 2.0 ** -52 * float(np.max(np.abs(lam))) + 1e-13 * float(np.max(np.abs(want)))
            dev = float(np.max(np.abs((lam - ell) - want)))
            assert dev <= tol, (kind, l, dev, tol)
            below += int((n < fields["flat_below"]).sum())
            outside += int(((n < fields["uniform_min"]) | (n > fields["uniform_max"])).sum())
            inside += int(((n >= fields["uniform_min"]) & (n <= fields["uniform_max"])).sum())
    print(f"k {k} lines {nl}: log p_N checked at {below} points below flat_below, {outside} outside and {inside} inside the uniform window")
    assert below > 50 and outside > 50 and inside > 50
    # the level-1 l' does not depend on the prior; lambda and the evidence do
    _same(runs[0], plain, ("boxes", "sample_log_likelihoods_refined"))
    ok = plain["status"] == 0
    assert (runs[0]["log_likelihoods_dla_refined"][ok] != plain["log_likelihoods_dla_refined"][ok]).all()


def test_sizes_of_the_last_refine_are_kept_and_checked():
    import ctypes as C
    ctx, batch = _context(8, 3, 127)
    try:
        batch.process()
        batch.refine(levels=3, download=False)
        out = batch.download_refined()                      # sized by what the batch remembers, not by a default
        assert out["boxes"].shape == (len(RC.KINDS), 3, 4) and out["sample_log_likelihoods_refined"].shape[1] == 127
        with pytest.raises(ValueError, match="levels"):
            batch.download_refined(levels=2)
        # the library refuses arrays stated as sized for something else, and writes nothing
        sel = np.arange(2, dtype=np.int64)
        host = refine.empty_results(2, 3, 127)
        for levels, points, field in ((2, 127, "levels"), (3, 100, "num_points")):
            r = _lib.RefinedResults()
            r.levels, r.num_points = levels, points
            r.boxes, r.sample_log_likelihoods_refined = _lib.ptr(host["boxes"]), _lib.ptr(host["sample_log_likelihoods_refined"])
            rc = ctx.lib.gpdla_batch_download_refined(ctx._h, batch._h, sel.ctypes.data_as(C.POINTER(C.c_int64)), 2, C.byref(r))
            assert rc == _lib.ERR_INVALID_ARGUMENT and field in ctx.lib.gpdla_last_error().decode()
            assert np.isnan(host["boxes"]).all() and np.isnan(host["sample_log_likelihoods_refined"]).all()
        # another point set after the refine, of the same size: the summaries would read the wrong (u, v)
        batch.parameter_summaries(refined=True)
        ctx.set_refine_points(*[x[::-1].copy() for x in RC.halton_points(127)])
        with pytest.raises(_lib.GpdlaError, match="refine points changed"):
            batch.parameter_summaries(refined=True)
        assert batch.download_refined()["boxes"].shape == (len(RC.KINDS), 3, 4)   # the tables themselves are still the batch's
        with pytest.raises(ValueError, match="refined=True"):
            batch.parameter_summaries(refined=True, multi=True)
        batch.reload(RC.make_batch(8, 3)[2], np.full(8, np.log(0.9)), np.full(8, np.log(0.1)))
        with pytest.raises(_lib.GpdlaError, match="not been refined"):
            batch.download_refined()
    finally:
        batch.close()
        ctx.close()


def test_refused_requests():
    ctx, batch = _context(8, 3, 127)
    try:
        with pytest.raises(_lib.GpdlaError, match="not been processed"):
            batch.refine()
        batch.process()
        with pytest.raises(_lib.GpdlaError, match="levels"):
            batch.refine(levels=5)
        with pytest.raises(_lib.GpdlaError, match="selection"):
            batch.refine(selection=[len(RC.KINDS)])
        with pytest.raises(_lib.GpdlaError, match="not been refined"):
            batch.download_refined()
    finally:
        batch.close()
        ctx.close()
    # the fp32 study class
    ctx, batch = _context(8, 3, 127, contraction_precision=1)
    try:
        batch.process()
        with pytest.raises(_lib.GpdlaError, match="fp64 only") as e:
            batch.refine()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        batch.close()
        ctx.close()
    # k > 40 never reaches a batch: the context refuses the model (GPDLA_MAX_K = 40)
    ctx = gp.Context(0, Parameters())
    try:
        with pytest.raises(_lib.GpdlaError) as e:
            ctx.set_model(synthetic.make_model(41))
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        ctx.close()
    from gp_dla_detection_amd.parameters import MultiParameters
    model, samples, spectra, _ = RC.make_batch(8, 3)
    ctx = gp.Context(0, MultiParameters(max_dlas=2))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(16))
    batch = ctx.upload(spectra[:2], np.full(2, np.log(0.8)), np.log(np.full((2, 2), 0.1)), np.full(2, np.log(0.05)))
    try:
        with pytest.raises(_lib.GpdlaError, match="single-DLA") as e:
            batch.refine()
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        batch.close()
        ctx.close()


def test_command_line_equals_the_in_memory_path(tmp_path):
    files = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=12, num_samples=64, empty_quasar=3)
    paths, test_ind = files["paths"], files["test_ind"]
    spectra = [s for s, t in zip(files["spectra"], test_ind) if t]
    results = gp.process_qsos(files["model"], files["samples"], spectra, prior_catalog=files["prior"])
    processed, out = str(tmp_path / "processed.mat"), str(tmp_path / "refined.mat")
    io.save_processed_qsos(processed, results, test_ind=test_ind)
    args = [paths["preloaded"], paths["catalog"], paths["learned"], paths["samples"], processed, out, "--p-thresh", "0.3",
            "--levels", "2", "--points", "50", "--batch", "4"]
    assert refine.main(args) == 0
    want = refine.refine_absorbers(files["model"], files["samples"], spectra, results, 0.3, levels=2,
                                   points=refine.default_points(50))
    back = io.load_refined_results(out)
    assert want["selection"].size >= 2 and np.array_equal(back["selection"], want["selection"])
    _same(back, want, refine.SCALARS + ("boxes", "status"))
    for key in ("mean_z", "std_log_nhi", "quantiles_z", "quantiles_log_nhi", "effective_samples", "status"):
        np.testing.assert_array_equal(back["summaries"][key], want["summaries"][key], err_msg=key)
    # once more with a column density prior fitted to a catalogue's log N_HI values
    log_nhis = 20.0 + 2.0 * np.random.default_rng(8).beta(1.2, 3.0, size=400)
    prior_file = str(tmp_path / "log_nhis.txt")
    np.savetxt(prior_file, log_nhis, fmt="%.17g")
    assert refine.main(args + ["--prior", prior_file]) == 0
    with_prior = io.load_refined_results(out)
    want_prior = refine.refine_absorbers(files["model"], files["samples"], spectra, results, 0.3, levels=2,
                                         points=refine.default_points(50), prior=samples_mod.fit_nhi_prior(np.loadtxt(prior_file)))
    _same(with_prior, want_prior, refine.SCALARS + ("boxes", "status"))
    assert (with_prior["log_likelihoods_dla_refined"] != back["log_likelihoods_dla_refined"]).all()
