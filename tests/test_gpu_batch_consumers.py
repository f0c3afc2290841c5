"""GPU checks of what the entries that read a processed batch share (csrc/host_consumers.hpp and the helpers beside
it): one table of refusals run against every entry, the row addressing of the resident sample tables, absorber
lists that do not start at zero, and the timed region.  Nothing here is compared with a tolerance: messages are
compared as text and numbers bit for bit.

Batches: the eight quasars of tests/refine_cases.py (k = 8, three lines, S = 200, 16 refine points) and its first
two quasars as a multi-DLA batch (max_dlas = 2), as in test_gpu_refine.py::test_refused_requests."""
import ctypes as C

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, posteriors, refine, synthetic
from gp_dla_detection_amd.parameters import MultiParameters, Parameters

import refine_cases as RC

pytestmark = pytest.mark.gpu

K, LINES, SR, LEVELS = 8, 3, 16, 2
NQ = len(RC.KINDS)
PERM = [5, 2, 7, 0, 2, 6, 1, 3, 4]   # every quasar, out of order, 2 twice
MULTI_PERM = [1, 0, 1]
I64P = C.POINTER(C.c_int64)


def _single(spectra=None):
    model, samples, all_spectra, _ = RC.make_batch(K, LINES)
    spectra = all_spectra if spectra is None else [all_spectra[i] for i in spectra]
    ctx = gp.Context(0, Parameters(num_lines=LINES))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(SR))
    n = len(spectra)
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))


def _multi():
    model, samples, spectra, _ = RC.make_batch(K, LINES)
    ctx = gp.Context(0, MultiParameters(max_dlas=2))
    ctx.set_model(model)
    ctx.set_samples(samples)
    return ctx, ctx.upload(spectra[:2], np.full(2, np.log(0.8)), np.log(np.full((2, 2), 0.1)), np.full(2, np.log(0.05)))


@pytest.fixture(scope="module")
def single():
    """The single-DLA batch, processed and refined, shared and left as it is by every test that takes it."""
    ctx, batch = _single()
    batch.process()
    batch.refine(levels=LEVELS, download=False)
    yield ctx, batch
    batch.close()
    ctx.close()


@pytest.fixture(scope="module")
def multi():
    ctx, batch = _multi()
    batch.process_multi()
    yield ctx, batch
    batch.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------
# 1. refusals
# ------------------------------------------------------------------------------------------------

def _python_entries(batch):
    """Every entry that takes a selection, through the Python surface."""
    return {"model_spectra": lambda sel: batch.model_spectra(selection=sel, products=("map",)),
            "parameter_summaries": lambda sel: batch.parameter_summaries(selection=sel),
            "refine": lambda sel: batch.refine(selection=sel, levels=LEVELS),
            "download_refined": lambda sel: batch.download_refined(selection=sel),
            "refined_summaries": lambda sel: batch.parameter_summaries(selection=sel, refined=True)}


def _c_entries(ctx, batch):
    """The same entries at the C boundary, taking (selection pointer or None, num_selected): the request is
    otherwise valid and the output arrays are never reached."""
    lib, c, b = ctx.lib, ctx._h, batch._h
    p, t = posteriors.check_request(posteriors.DEFAULT_PROBABILITIES, posteriors.DEFAULT_THRESHOLDS)
    summary_rq = posteriors._request(1, p, t)
    _, summary_out = posteriors._outputs(NQ + 1, 1, len(p), len(t))
    refine_rq = refine.request(LEVELS, RC.DELTA, RC.PAD)
    refined = _lib.RefinedResults()
    refined.levels, refined.num_points = LEVELS, SR
    offsets = np.zeros(NQ + 2, dtype=np.int64)
    spectra_out = _lib.ModelSpectra()
    spectra_out.offsets = offsets.ctypes.data_as(I64P)

    def model_spectra(selp, n):
        rq = _lib.ModelSpectraRequest()
        rq.selection, rq.num_selected, rq.products = selp, n, _lib.SPECTRA_MAP
        return lib.gpdla_batch_model_spectra(c, b, C.byref(rq), C.byref(spectra_out))

    return {"model_spectra": model_spectra,
            "parameter_summaries": lambda selp, n: lib.gpdla_batch_parameter_summaries(c, b, 0, 0, selp, n, C.byref(summary_rq),
                                                                                       C.byref(summary_out)),
            "refine": lambda selp, n: lib.gpdla_batch_refine(c, b, selp, n, C.byref(refine_rq), None),
            "download_refined": lambda selp, n: lib.gpdla_batch_download_refined(c, b, selp, n, C.byref(refined)),
            "refined_summaries": lambda selp, n: lib.gpdla_batch_refined_summaries(c, b, selp, n, C.byref(summary_rq),
                                                                                   C.byref(summary_out))}


SELECTION_CASES = [([NQ], f"selection[0] = {NQ} outside the batch of {NQ} quasars"),
                   ([0, -1], f"selection[1] = -1 outside the batch of {NQ} quasars"),
                   (None, f"num_selected = {NQ + 1} outside [0, {NQ}]")]   # no selection: the first num_selected quasars


@pytest.mark.parametrize("sel,message", SELECTION_CASES)
def test_every_entry_refuses_a_bad_selection_in_the_same_words(single, sel, message):
    ctx, batch = single
    for name, call in _c_entries(ctx, batch).items():
        arr = None if sel is None else np.array(sel, dtype=np.int64)
        rc = call(None if sel is None else arr.ctypes.data_as(I64P), NQ + 1 if sel is None else arr.size)
        assert rc == _lib.ERR_INVALID_ARGUMENT and ctx.lib.gpdla_last_error().decode() == message, name
    if sel is not None:
        for name, call in _python_entries(batch).items():
            with pytest.raises(_lib.GpdlaError) as e:
                call(sel)
            assert e.value.code == _lib.ERR_INVALID_ARGUMENT and message in str(e.value), name
    # nothing was written or launched: the refined tables are still those of the fixture
    assert batch.download_refined()["boxes"].shape == (NQ, LEVELS, 4)


def test_an_unprocessed_batch_is_refused():
    for make, kw in ((lambda: _single([0, 1]), {}), (_multi, dict(multi=True))):
        ctx, batch = make()
        try:
            with pytest.raises(_lib.GpdlaError, match="the batch has not been processed") as e:
                batch.parameter_summaries(**kw)
            assert e.value.code == _lib.ERR_INVALID_ARGUMENT and str(e.value).endswith("the batch has not been processed")
            assert "resident weights" not in str(e.value)
            with pytest.raises(_lib.GpdlaError, match="resident weights: the batch has not been processed"):
                batch.model_spectra(weights="resident", products=("moments",))
            if not kw:
                with pytest.raises(_lib.GpdlaError, match="the batch has not been processed"):
                    batch.refine(levels=1)
            assert batch.model_spectra(products=("map",))["map_absorption"].size > 0   # needs no sweep
        finally:
            batch.close()
            ctx.close()


def test_what_each_entry_holds_against_a_changed_context():
    """Every entry compares the number of samples with the batch's; all but gpdla_batch_parameter_summaries also
    the model's rank; the downloads of the refined tables read the batch alone."""
    model, samples, _, _ = RC.make_batch(K, LINES)
    ctx, batch = _single([0, 1, 3])
    try:
        batch.process()
        batch.refine(levels=1, download=False)
        before = batch.parameter_summaries()
        ctx.set_model(model)                                  # the same model again: nothing to refuse
        for key in posteriors.FIELDS:
            np.testing.assert_array_equal(batch.parameter_summaries()[key], before[key], err_msg=key)
        assert batch.refine(levels=1)["status"].tolist() == [0, 0, 0]
        ctx.set_model(synthetic.make_model(K + 4))            # another rank: the summaries read no model
        for key in posteriors.FIELDS:
            np.testing.assert_array_equal(batch.parameter_summaries()[key], before[key], err_msg=key)
        changed = {"refine": lambda: batch.refine(levels=1), "model_spectra": lambda: batch.model_spectra(products=("map",)),
                   "unmasked_counts": batch.unmasked_counts, "draw_mocks": lambda: batch.draw_mocks(write_resident=False)}
        for name, call in changed.items():
            with pytest.raises(_lib.GpdlaError, match="model/samples changed after the batch was uploaded") as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARGUMENT, name
        ctx.set_model(model)
        ctx.set_samples(synthetic.make_samples(RC.S + 8))     # a set of another size
        changed["parameter_summaries"] = batch.parameter_summaries
        for name, call in changed.items():
            with pytest.raises(_lib.GpdlaError, match="changed after the batch was uploaded") as e:
                call()
            assert e.value.code == _lib.ERR_INVALID_ARGUMENT, name
            assert ("model/samples changed" in str(e.value)) == (name != "parameter_summaries"), name
        assert batch.download_refined()["status"].tolist() == [0, 0, 0]
        assert batch.parameter_summaries(refined=True)["status"].shape == (3, 1)
    finally:
        batch.close()
        ctx.close()


# ------------------------------------------------------------------------------------------------
# 2. row addressing
# ------------------------------------------------------------------------------------------------

def _same_cells(got, want, perm):
    """Per-pixel outputs of a permuted selection against those of the identity selection."""
    for name in ("mean_absorption", "var_absorption"):
        cells, permuted = gp.split_cells(want[name], want["offsets"]), gp.split_cells(got[name], got["offsets"])
        assert len(permuted) == len(perm)
        for j, q in enumerate(perm):
            np.testing.assert_array_equal(permuted[j], cells[q], err_msg=f"{name} entry {j} (quasar {q})")
    np.testing.assert_array_equal(got["status"], want["status"][perm])


def _same_rows(got, want, perm, keys):
    for key in keys:
        np.testing.assert_array_equal(got[key], want[key][perm], err_msg=key)   # NaN pattern included


def test_rows_of_a_permuted_selection_single_dla(single):
    """(A permutation without a repeat: test_gpu_model_spectra.py::test_moments_are_bit_identical_however_they_are_asked_for,
    test_gpu_posteriors.py::test_resident_single_dla_batch_equals_the_host_form; a refine of [3, 0, 3] and its download:
    test_gpu_refine.py::test_results_do_not_depend_on_selection_order_groups_or_run.)"""
    _, batch = single
    moments = dict(products=("moments",), weights="resident")
    _same_cells(batch.model_spectra(selection=PERM, **moments), batch.model_spectra(**moments), PERM)
    _same_rows(batch.parameter_summaries(selection=PERM), batch.parameter_summaries(), PERM, posteriors.FIELDS + ("correlation",))
    whole = batch.download_refined()
    assert (whole["status"] == 0).sum() >= 5 and not np.isnan(whole["boxes"][whole["status"] == 0]).any()
    _same_rows(batch.download_refined(selection=PERM), whole, PERM, [k for k in whole if k != "selection"])
    _same_rows(batch.parameter_summaries(selection=PERM, refined=True), batch.parameter_summaries(refined=True), PERM,
               posteriors.FIELDS + ("correlation",))


@pytest.mark.parametrize("sub_dla", [False, True])
def test_rows_of_a_permuted_selection_multi_dla(multi, sub_dla):
    """The DLA table is [nq][max_dlas][S] and the sub-DLA table [nq][S]: a quasar's row starts at another stride."""
    _, batch = multi
    res = batch.download_multi()
    moments = dict(products=("moments",), weights="resident", sub_dla=sub_dla)
    whole = batch.model_spectra(**moments)
    assert np.isfinite(whole["mean_absorption"]).all() and (whole["status"] == 0).all()
    _same_cells(batch.model_spectra(selection=MULTI_PERM, **moments), whole, MULTI_PERM)
    table = res["sample_log_likelihoods_lls"] if sub_dla else res["sample_log_likelihoods_dla"][:, 0, :]
    assert table.shape == (2, RC.S) and not np.array_equal(table[0], table[1])
    for sel in (None, MULTI_PERM):   # the resident table read in place == its rows handed back by the host
        rows = table if sel is None else table[sel]
        host = batch.model_spectra(selection=sel, products=("moments",), weights=rows, sub_dla=sub_dla)
        resident = batch.model_spectra(selection=sel, **moments)
        for name in ("mean_absorption", "var_absorption"):
            np.testing.assert_array_equal(resident[name], host[name], err_msg=name)
    kw = dict(multi=True, sub_dla=sub_dla)
    summ = batch.parameter_summaries(**kw)
    assert (summ["status"] == 0).all() and not np.array_equal(summ["mean_z"][0], summ["mean_z"][1])
    _same_rows(batch.parameter_summaries(selection=MULTI_PERM, **kw), summ, MULTI_PERM, posteriors.FIELDS + ("correlation",))


# ------------------------------------------------------------------------------------------------
# 3. absorber lists cut out of a longer CSR
# ------------------------------------------------------------------------------------------------

def _lists(z_lo, z_hi, counts, lead=5):
    """(the slice: offsets starting at `lead` beside the full arrays, the same lists rebased to zero).  The
    `lead` entries in front are absorbers of their own right, so reading from the front would show."""
    rng = np.random.default_rng(11)
    off = lead + np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    z = np.concatenate([np.full(lead, 0.5 * (z_lo[0] + z_hi[0])),
                        np.concatenate([z_lo[q] + (z_hi[q] - z_lo[q]) * rng.uniform(0.2, 0.8, size=c) for q, c in enumerate(counts)])])
    log_nhi = np.concatenate([np.full(lead, 21.5), rng.uniform(20.0, 21.0, size=int(np.sum(counts)))])
    assert off[0] == lead and off[-1] == z.size
    return (off, z, log_nhi), (off - lead, z[lead:].copy(), log_nhi[lead:].copy())


def test_absorber_offsets_that_do_not_start_at_zero(single):
    """The wrappers hand the library the offsets as given and pointers to the whole z / N arrays."""
    _, batch = single
    first = batch.download(with_samples=False)
    good = np.flatnonzero(first["status"] == 0)
    counts = np.zeros(NQ, dtype=int)
    counts[good[:3]] = (1, 2, 8)
    z_lo, z_hi = np.nan_to_num(first["min_z_dlas"], nan=2.0), np.nan_to_num(first["max_z_dlas"], nan=2.1)
    sliced, rebased = _lists(z_lo, z_hi, counts)
    a = batch.model_spectra(absorbers=sliced, products=("map", "continuum"))
    b = batch.model_spectra(absorbers=rebased, products=("map", "continuum"))
    for name in ("offsets", "status", "map_absorption", "continuum", "model_flux"):
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    cells = gp.split_cells(a["map_absorption"], a["offsets"])
    assert all((cells[q] < 1).any() == (counts[q] > 0) for q in good)
    # a selection: lists for the three selected quasars only, in the selection's order
    sel = [int(good[2]), int(good[0]), int(good[1])]
    sliced, rebased = _lists(z_lo[sel], z_hi[sel], [2, 0, 3], lead=5)
    a = batch.model_spectra(selection=sel, absorbers=sliced, products=("map",))
    b = batch.model_spectra(selection=sel, absorbers=rebased, products=("map",))
    np.testing.assert_array_equal(a["map_absorption"], b["map_absorption"])
    sliced, rebased = _lists(z_lo, z_hi, counts)
    kw = dict(seed=77, write_resident=False, components=("absorption", "continuum", "sigma", "latents"))
    a, b = batch.draw_mocks(sliced, **kw), batch.draw_mocks(rebased, **kw)
    for name in ("flux", "status", "grid_offsets") + kw["components"]:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    assert (a["absorption"] < 1).any() and not np.array_equal(a["flux"], batch.draw_mocks(**kw)["flux"])


def test_model_mean_absorber_offsets_that_do_not_start_at_zero():
    model = synthetic.make_model(K)
    z_qsos = np.array([2.6, 3.1, 2.9])
    sliced, rebased = _lists(z_qsos - 0.5, z_qsos - 0.1, [2, 0, 1])
    a, b = gp.dla_model_mean(model, z_qsos, sliced), gp.dla_model_mean(model, z_qsos, rebased)
    np.testing.assert_array_equal(a, b)
    none = gp.dla_model_mean(model, z_qsos)
    assert np.isfinite(a).all() and np.array_equal(a[1], none[1]) and (a[0] < none[0]).any() and (a[2] < none[2]).any()


# ------------------------------------------------------------------------------------------------
# 4. the timed region
# ------------------------------------------------------------------------------------------------

def test_the_timed_region_of_each_call():
    ctx, batch = _single([0, 1])
    mctx, mbatch = _multi()
    try:
        calls = [("process", ctx, batch.process), ("process_multi", mctx, mbatch.process_multi),
                 ("model_spectra moments", ctx, lambda: batch.model_spectra(weights="resident", products=("moments",))),
                 ("draw_mocks", ctx, lambda: batch.draw_mocks(write_resident=False))]
        for name, cx, call in calls:
            assert cx.last_sweep_ms() == -1.0, name          # timing off, or just switched on
            cx.set_timing(True)
            assert cx.last_sweep_ms() == -1.0, name
            call()
            ms = cx.last_sweep_ms()
            print(f"{name}: {ms:.4f} ms")
            assert ms > 0.0, name
            cx.set_timing(True)
            assert cx.last_sweep_ms() == -1.0, name
            cx.set_timing(False)
        batch.model_spectra(products=("map",))               # timing off: nothing is recorded
        assert ctx.last_sweep_ms() == -1.0
    finally:
        batch.close()
        ctx.close()
        mbatch.close()
        mctx.close()
