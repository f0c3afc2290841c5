"""GPU checks of the per-pixel products on refined tables: Batch.model_spectra moments,
Batch.marginal_continuum and Batch.predictive_flux with ``weights="refined"`` on the batches of tests/refine_cases.py at
both CONFIGS (k = 8 with three lines at compile time; k = 24 with five at run time: the other record class and the other
contraction shape), S = 200, two refine levels, S' in {63, 65, 257}.

The reference is the existing restatement of every product, fed -- through tests/refined_products_cases.py -- a copy of the
quasar's grid with its last box as the search range, (u, 10**(n_lo + (n_hi - n_lo) v)) as samples and the downloaded
lambda row as the table.  Tolerances are the existing rules, imported: TOL_MOMENTS for the moments;
marginal_continuum_cases.tolerances and predictive_flux_restatement.tolerances of the restatement's own dense-versus-Woodbury
disagreement (10 x, floored at 1e-12, capped at 1e-8).  At S' = 257 one row is restated in the Woodbury form alone (the dense
form costs n^3 per live sample); its tolerance is that of the same quasar at S' = 65, where both forms were run: the
disagreement of the two forms is a property of the quasar's B_i = I + M' diag(a^2/d) M, whose conditioning the sample count
does not change, and the weighted sums are convex combinations whatever S' is.  Measured once on one MI355X's own boxes and
lambda rows, with the dense form run at S' = 257 too (`strong`, both configurations): the disagreement of the fourteen
arrays is 1.5e-18 ... 4.4e-14 at S' = 65 and 2.1e-18 ... 3.6e-14 at S' = 257 -- under a tenth of the 1e-12 floor at both, so
either count gives the floor as the tolerance (profiles/r09_refined_products.txt).
Every figure is printed before it is asserted."""
import multiprocessing as mp
import os

import numpy as np
import pytest

import gp_dla_detection_amd as gp
from gp_dla_detection_amd import _lib, api, synthetic
from gp_dla_detection_amd.parameters import Parameters

import marginal_continuum_cases as MC
import marginal_continuum_restatement as MR
import predictive_flux_cases as PC
import predictive_flux_restatement as PR
import refine_cases as RC
import refined_products_cases as XC
import refined_products_groups_worker as worker
from test_gpu_model_spectra import TOL_MOMENTS

pytestmark = pytest.mark.gpu

ALL = [(k, nl, Sr) for k, nl in RC.CONFIGS for Sr in XC.SR_VALUES]
MIX3 = (0.2, 0.3, 0.5)   # (null, sub-DLA, DLA) of the three-component mixture
_RUNS, _WANT = {}, {}
MS_ARRAYS = ("mean_absorption", "var_absorption")
MC_ARRAYS = MR.PRODUCTS_COEF + MR.PRODUCTS_COV
PF_ARRAYS = PR.PRODUCTS


def _context(k, nl, Sr, zero_range=False):
    model, samples, spectra, _ = RC.make_batch(k, nl, zero_range)
    ctx = gp.Context(0, RC.batch_parameters(nl, zero_range))
    ctx.set_model(model)
    ctx.set_samples(samples)
    ctx.set_refine_points(*RC.halton_points(Sr))
    n = len(spectra)
    return ctx, ctx.upload(spectra, np.full(n, np.log(0.9)), np.full(n, np.log(0.1)))


def _products(batch, selection=None, **kw):
    """The three products on the refined table (DLA component alone) for a selection."""
    return dict(ms=batch.model_spectra(selection=selection, weights="refined", products=("moments",)),
                mc=batch.marginal_continuum(selection=selection, weights="refined", sample_coefficients=True, **kw),
                pf=batch.predictive_flux(selection=selection, weights="refined", **kw))


def run(k, nl, Sr, zero_range=False):
    """One context per configuration: the first pass, two refine levels, and every product the tests compare."""
    key = (k, nl, Sr, zero_range)
    if key not in _RUNS:
        ctx, batch = _context(k, nl, Sr, zero_range)
        try:
            batch.process()
            first = batch.download()
            resident_before = dict(mc=batch.marginal_continuum(weights="resident"), pf=batch.predictive_flux(weights="resident"),
                                   ms=batch.model_spectra(weights="resident", products=("moments",)))
            ref = batch.refine(levels=XC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
            rp = batch.refined_posteriors()
            out = dict(first=first, ref=ref, rp=rp, **_products(batch))
            pw2 = np.stack([rp["p_no_dlas_refined"], np.zeros(rp["p_dlas_refined"].size), rp["p_dlas_refined"]], axis=1)
            pw2 = np.where(np.isnan(pw2), 0.5, pw2)     # (an unusable quasar has no posterior; its rows are NaN anyway)
            pw2[:, 1] = 0.0
            out["pw2"] = pw2
            out["mc2"] = batch.marginal_continuum(weights="refined", components=("null", "dla"), model_weights=pw2)
            out["pf2"] = batch.predictive_flux(weights="refined", components=("null", "dla"), model_weights=pw2)
            pw3 = np.tile(np.array(MIX3), (len(first["status"]), 1))
            out["mc3"] = batch.marginal_continuum(weights="refined", components=("null", "sub_dla", "dla"), model_weights=pw3)
            out["pf3"] = batch.predictive_flux(weights="refined", components=("null", "sub_dla", "dla"), model_weights=pw3)
            out["after"] = batch.download()
            out["resident_before"] = resident_before
            out["resident_after"] = dict(mc=batch.marginal_continuum(weights="resident"), pf=batch.predictive_flux(weights="resident"),
                                         ms=batch.model_spectra(weights="resident", products=("moments",)))
        finally:
            batch.close()
            ctx.close()
        _RUNS[key] = out
    return _RUNS[key]


def restated_rows(Sr, zero_range=False):
    if zero_range:
        return list(RC.ZR_KINDS)
    return list(XC.RESTATED_KINDS) if Sr != 257 else ["strong"]


def forms(Sr):
    return ("dense", "woodbury") if Sr != 257 else ("woodbury",)


def want(oracle, k, nl, Sr, zero_range=False):
    """The restatements of the rows of ``restated_rows`` on the GPU's own boxes and lambda rows, once per configuration:
    {kind: {"ms": (mean, var), "mc": {form: dict}, "pf": {form: dict}, "mc2", "pf2", "mc3", "pf3": {form: dict}}}."""
    key = (k, nl, Sr, zero_range)
    if key not in _WANT:
        r = run(k, nl, Sr, zero_range)
        model, samples, spectra, _ = RC.make_batch(k, nl, zero_range)
        u, v = RC.halton_points(Sr)
        kinds = RC.ZR_KINDS if zero_range else RC.KINDS
        p = RC.batch_parameters(nl, zero_range)
        out = {}
        for kind in restated_rows(Sr, zero_range):
            i = kinds.index(kind)
            assert r["ref"]["status"][i] == 0, kind
            g = XC.grid(oracle, model, spectra[i], p, zero_range)
            box, lam = r["ref"]["boxes"][i, -1], r["ref"]["sample_log_posteriors_refined"][i]
            lls_row = r["first"]["sample_log_likelihoods_dla"][i]   # a single-DLA batch: the sub-DLA component weighs ITS table
            d = {"ms": XC.moments(oracle, g, box, u, v, lam, nl)}
            for name, fn in (("mc", XC.marginal_continuum), ("pf", XC.predictive_flux)):
                d[name] = {f: fn(oracle, model, g, box, u, v, lam, nl, f) for f in forms(Sr)}
                if Sr != 257 and kind in ("strong", "masked_run", "zero_range"):   # the mixtures: two rows a configuration
                    d[name + "2"] = {f: fn(oracle, model, g, box, u, v, lam, nl, f, p=r["pw2"][i]) for f in forms(Sr)}
                    d[name + "3"] = {f: fn(oracle, model, g, box, u, v, lam, nl, f, p=MIX3, samples=samples, lls_row=lls_row)
                                     for f in forms(Sr)}
            out[kind] = d
        _WANT[key] = out
    return _WANT[key]


def _tolerances(oracle, k, nl, Sr, kind, which, zero_range=False):
    """The existing rule on the dense-versus-Woodbury disagreement of this row (S' = 257: of the same row at S' = 65)."""
    w = want(oracle, k, nl, 65 if Sr == 257 else Sr, zero_range)[kind][which]
    both = {"dense": [w["dense"]], "woodbury": [w["woodbury"]]}
    if which.startswith("mc"):
        names = [n for n in MC_ARRAYS if n in w["dense"]]
        dis = {n: MR.deviation(w["dense"][n], w["woodbury"][n]) for n in names}
        dis.setdefault("sample_coefficients", 0.0)
        return {n: t for n, t in MC.tolerances(dis).items() if n in names}, dis
    dis = PC.disagreement(both)
    return PR.tolerances(dis), dis


def _check(oracle, k, nl, Sr, which, got_key, zero_range=False):
    r = run(k, nl, Sr, zero_range)
    kinds = RC.ZR_KINDS if zero_range else RC.KINDS
    split = MC.split(r[got_key], k) if which.startswith("mc") else PC.split(r[got_key])
    checked = 0
    for kind, d in want(oracle, k, nl, Sr, zero_range).items():
        if which not in d:
            continue
        i = kinds.index(kind)
        ref = d[which]["dense" if "dense" in d[which] else "woodbury"]
        tol, dis = _tolerances(oracle, k, nl, Sr, kind, which, zero_range)
        assert split[i]["status"] == 0, kind
        for name, t in tol.items():
            if name not in split[i]:    # (sample_coefficients: asked of the one-component call only)
                continue
            dev = MR.deviation(split[i][name], ref[name])
            print(f"k {k} lines {nl} S' {Sr} {kind} {which} {name}: disagreement {dis[name]:.2e} -> tolerance {t:.2e}; GPU |delta| {dev:.3e}")
            assert dev < t, (kind, which, name, dev, t)
            checked += 1
    assert checked


# ------------------------------------------------------------------------------------------------
# 1. parity of the DLA component of every product
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_moments_against_the_restatement(oracle, k, nl, Sr):
    r = run(k, nl, Sr)
    off = r["ms"]["offsets"]
    for kind, d in want(oracle, k, nl, Sr).items():
        i = RC.KINDS.index(kind)
        mean, var = d["ms"]
        e_mean = float(np.abs(r["ms"]["mean_absorption"][off[i]:off[i + 1]] - mean).max())
        e_var = float(np.abs(r["ms"]["var_absorption"][off[i]:off[i + 1]] - var).max())
        print(f"k {k} lines {nl} S' {Sr} {kind}: mean {e_mean:.3e} var {e_var:.3e} (bound {TOL_MOMENTS:.0e}); "
              f"max var_absorption {var.max():.3e}")
        assert e_mean < TOL_MOMENTS and e_var < TOL_MOMENTS, kind
        assert r["ms"]["status"][i] == 0


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_marginal_continuum_against_the_restatement(oracle, k, nl, Sr):
    """All seven arrays, sample_coefficients [nsel, S', k] among them."""
    r = run(k, nl, Sr)
    assert r["mc"]["sample_coefficients"].shape == (len(RC.KINDS), Sr, k)
    _check(oracle, k, nl, Sr, "mc", "mc")


@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_predictive_flux_against_the_restatement(oracle, k, nl, Sr):
    _check(oracle, k, nl, Sr, "pf", "pf")
    res = run(k, nl, Sr)["pf"]
    ok = np.isfinite(res["flux_mean"])
    assert (res["flux_var"][ok] == res["flux_var_within"][ok] + res["flux_var_between"][ok]).all()


# ------------------------------------------------------------------------------------------------
# 2. mixtures: (null, DLA) by the refined posteriors; (null, sub-DLA, DLA) with components of 200 and S' samples
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,nl,Sr", [c for c in ALL if c[2] != 257])
@pytest.mark.parametrize("which", ["mc2", "pf2", "mc3", "pf3"])
def test_mixtures_against_the_restatement(oracle, k, nl, Sr, which):
    assert Sr != RC.S
    _check(oracle, k, nl, Sr, which, which)


# ------------------------------------------------------------------------------------------------
# 3. the zero-width search range
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,nl", RC.CONFIGS)
def test_zero_width_range(oracle, k, nl):
    Sr = RC.ZR_SR
    r = run(k, nl, Sr, True)
    i = RC.ZR_KINDS.index("zero_range")
    box = r["ref"]["boxes"][i, -1]
    assert r["ref"]["status"][i] == 0 and box[0] == box[1], box
    off = r["ms"]["offsets"]
    for kind, d in want(oracle, k, nl, Sr, True).items():
        j = RC.ZR_KINDS.index(kind)
        mean, var = d["ms"]
        e = max(float(np.abs(r["ms"]["mean_absorption"][off[j]:off[j + 1]] - mean).max()),
                float(np.abs(r["ms"]["var_absorption"][off[j]:off[j + 1]] - var).max()))
        print(f"zero range k {k} {kind}: moments {e:.3e}")
        assert e < TOL_MOMENTS, kind
    for which in ("mc", "pf", "mc3", "pf3"):
        _check(oracle, k, nl, Sr, which, which, True)


# ------------------------------------------------------------------------------------------------
# 4. bit identity: selection order, duplicates, one at a time, launch groups
# ------------------------------------------------------------------------------------------------

def _rows_of(res, names, s):
    off = res["offsets"]
    out = {}
    for n in names:
        a = res[n]
        out[n] = a[off[s]:off[s + 1]] if a.ndim == 1 else a[s]   # (flat per-pixel arrays; per-quasar rows)
    out["status"] = res["status"][s]
    return out


@pytest.mark.parametrize("k,nl", RC.CONFIGS)
def test_bit_identity_over_selections(k, nl):
    Sr = 65
    base = run(k, nl, Sr)
    sel = np.array([6, 0, 3, 1], dtype=np.int64)
    dup = np.array([0, 6, 0], dtype=np.int64)
    ctx, batch = _context(k, nl, Sr)
    try:
        batch.process()
        batch.refine(levels=XC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        a = _products(batch, sel)
        b = _products(batch, sel[::-1].copy())
        d = _products(batch, dup)
        ones = [_products(batch, np.array([q], dtype=np.int64)) for q in sel]
    finally:
        batch.close()
        ctx.close()
    for key, names in (("ms", MS_ARRAYS), ("mc", MC_ARRAYS), ("pf", PF_ARRAYS)):
        n = sel.size
        for s, q in enumerate(sel):
            ref = _rows_of(base[key], names, int(q))
            for label, got in (("selection", _rows_of(a[key], names, s)), ("reverse", _rows_of(b[key], names, n - 1 - s)),
                               ("alone", _rows_of(ones[s][key], names, 0))):
                for name in ref:
                    np.testing.assert_array_equal(got[name], ref[name], err_msg=f"{key} {name} {label} quasar {q}")
        for s, q in enumerate(dup):
            ref = _rows_of(base[key], names, int(q))
            got = _rows_of(d[key], names, s)
            for name in ref:
                np.testing.assert_array_equal(got[name], ref[name], err_msg=f"{key} {name} duplicate quasar {q}")
    assert np.isfinite(base["pf"]["flux_var"][:base["pf"]["offsets"][1]]).all()


def test_bit_identity_across_launch_groups(tmp_path):
    """The calls of the product library against the same calls in a clean child process that loads libgpdla_legacy.so with
    its debug-only scratch budget shrunk to two quasars' scratch rows of the LARGER component: four launch groups, with
    components of 200 and 65 samples in every group."""
    assert os.path.exists(_lib.LEGACY_LIB_PATH), "libgpdla_legacy.so is missing: __graft_entry__.build() makes it"
    wanted = worker.run_case()
    k, S = worker.K, max(RC.S, worker.SR)
    budget = 2 * S * (k * (k + 1) // 2 + k) * 8
    out = tmp_path / "groups.npz"
    env = {"GPDLA_LIB_PATH": _lib.LEGACY_LIB_PATH, "GPDLA_MC_SCRATCH_BYTES": str(budget)}
    pr = mp.get_context("forkserver").Process(target=worker.run_child, args=(env, str(out)))
    pr.start()
    pr.join(300)
    if pr.is_alive():  # our own child, by handle
        pr.kill()
        pr.join()
        raise AssertionError("the child process did not finish")
    assert pr.exitcode == 0
    got = np.load(out)
    assert set(got.files) == set(wanted)
    for name in wanted:
        np.testing.assert_array_equal(got[name], wanted[name], err_msg=name)
    assert np.isfinite(wanted["pf_flux_var"][:10]).all() and np.isfinite(wanted["mc_continuum_var"][:10]).all()


# ------------------------------------------------------------------------------------------------
# 5. a refine pass over a subset
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,nl", RC.CONFIGS)
def test_refine_of_a_subset(k, nl):
    Sr = 63
    base = run(k, nl, Sr)
    kinds = list(RC.KINDS)
    refined_rows = np.array([kinds.index(x) for x in ("strong", "status1", "status3", "masked_run")], dtype=np.int64)
    left_out = kinds.index("broad")
    sel = np.array([left_out, kinds.index("strong"), kinds.index("status1"), kinds.index("status3")], dtype=np.int64)
    null_only = np.tile(np.array([1.0, 0.0, 0.0]), (sel.size, 1))
    ctx, batch = _context(k, nl, Sr)
    try:
        batch.process()
        batch.refine(selection=refined_rows, levels=XC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        got = _products(batch, sel)
        mixed = dict(mc=batch.marginal_continuum(selection=sel, weights="refined", components=("null", "dla"),
                                                 model_weights=np.tile(np.array([0.5, 0.0, 0.5]), (sel.size, 1))),
                     pf=batch.predictive_flux(selection=sel, weights="refined", components=("null", "dla"),
                                              model_weights=np.tile(np.array([0.5, 0.0, 0.5]), (sel.size, 1))))
        null_refined = dict(mc=batch.marginal_continuum(selection=sel, weights="refined", components=("null", "dla"), model_weights=null_only),
                            pf=batch.predictive_flux(selection=sel, weights="refined", components=("null", "dla"), model_weights=null_only))
        null_resident = dict(mc=batch.marginal_continuum(selection=sel, weights="resident", components=("null", "dla"), model_weights=null_only),
                             pf=batch.predictive_flux(selection=sel, weights="resident", components=("null", "dla"), model_weights=null_only))
    finally:
        batch.close()
        ctx.close()
    NR = _lib.SPECTRA_NOT_REFINED
    for key, names in (("ms", MS_ARRAYS), ("mc", MC_ARRAYS), ("pf", PF_ARRAYS)):
        res = got[key]
        print(f"k {k} {key}: status {res['status'].tolist()}")
        assert res["status"].tolist() == [NR, 0, 1, 3], key
        rows = _rows_of(res, names, 0)
        assert all(np.isnan(rows[n]).all() for n in names), key            # the quasar outside the refine's selection
        ref = _rows_of(base[key], names, kinds.index("strong"))           # the refined one: as when all were refined
        rows = _rows_of(res, names, 1)
        for n in names:
            np.testing.assert_array_equal(rows[n], ref[n], err_msg=f"{key} {n}")
        for s in (2, 3):
            rows = _rows_of(res, names, s)
            assert all(np.isnan(rows[n]).all() for n in names), (key, s)
    for key, names in (("mc", MR.PRODUCTS_COEF[1:] + MR.PRODUCTS_COV), ("pf", PF_ARRAYS)):
        assert mixed[key]["status"].tolist() == [NR, 0, 1, 3], key
        assert all(np.isnan(_rows_of(mixed[key], names, 0)[n]).all() for n in names), key
        # where the DLA component weighs exactly 0 the quasar is evaluated as before: the resident source, bit for bit
        assert null_refined[key]["status"].tolist() == [0, 0, 1, 3], key
        for name in names + ("status", "offsets"):
            np.testing.assert_array_equal(null_refined[key][name], null_resident[key][name], err_msg=f"{key} {name}")
        assert np.isfinite(_rows_of(null_refined[key], names, 0)[names[0]]).all()


@pytest.mark.parametrize("Sr", [63, 257])
def test_sample_coefficients_of_a_refined_request_that_reaches_the_sub_dla_table_only(Sr):
    """weights="refined" with "dla" listed but a DLA column of 0 in every row: the one sampled component is the sub-DLA table
    of the first pass, so ``sample_coefficients`` is [nsel, S, k] -- not [nsel, S', k], for S' below S and above it -- and the
    call equals the resident source bit for bit, before any refine too."""
    k, nl = RC.CONFIGS[0]
    n = len(RC.KINDS)
    pw = np.tile(np.array([0.25, 0.75, 0.0]), (n, 1))
    kw = dict(components=("null", "sub_dla", "dla"), model_weights=pw, sample_coefficients=True)
    ctx, batch = _context(k, nl, Sr)
    try:
        batch.process()
        before = batch.marginal_continuum(weights="refined", **kw)
        batch.refine(levels=XC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        got = batch.marginal_continuum(weights="refined", **kw)
        want_ = batch.marginal_continuum(weights="resident", **kw)
        one = batch.marginal_continuum(weights="refined", components=("sub_dla", "dla"), sample_coefficients=True,
                                       model_weights=np.tile(np.array([0.0, 1.0, 0.0]), (n, 1)))
        dla = batch.marginal_continuum(weights="refined", components=("sub_dla", "dla"), sample_coefficients=True,
                                       model_weights=np.tile(np.array([0.0, 0.0, 1.0]), (n, 1)))
    finally:
        batch.close()
        ctx.close()
    assert got["sample_coefficients"].shape == one["sample_coefficients"].shape == (n, RC.S, k)
    assert dla["sample_coefficients"].shape == (n, Sr, k)
    for name in want_:
        np.testing.assert_array_equal(got[name], want_[name], err_msg=name)
        np.testing.assert_array_equal(before[name], want_[name], err_msg=name)
    i = RC.KINDS.index("strong")
    live = ~np.isnan(got["sample_coefficients"][i]).any(axis=1)
    print(f"S' {Sr}: {live.sum()} of {RC.S} sub-DLA samples live on `strong`; status {got['status'].tolist()}")
    assert live.any() and got["status"].tolist() == [0, 0, 0, 0, 1, 3, 0, 0]


# ------------------------------------------------------------------------------------------------
# 6. refusals, with nothing written
# ------------------------------------------------------------------------------------------------

def _calls(batch, **kw):
    return (lambda: batch.model_spectra(weights="refined", products=("moments",), **kw),
            lambda: batch.marginal_continuum(weights="refined", **kw),
            lambda: batch.predictive_flux(weights="refined", **kw))


def _refused(lib, batch, ctx, code, sub_dla=False):
    """The three C entries on sentinel-filled arrays: the return code, and no entry of any output written.  ``sub_dla``: the
    one entry that has the flag, with it set."""
    import ctypes as C
    n = batch.num_quasars
    cap = sum(RC.PIXELS)
    sel = np.arange(n, dtype=np.int64)
    sentinel = -12345.0
    for entry, rq, st, fields in (
            ("model_spectra", _lib.ModelSpectraRequest(), _lib.ModelSpectra(), MS_ARRAYS),
            ("marginal_continuum", _lib.MarginalContinuumRequest(), _lib.MarginalContinuum(), api.MARGINAL_CONTINUUM_ARRAYS),
            ("predictive_flux", _lib.PredictiveFluxRequest(), _lib.PredictiveFlux(), PF_ARRAYS)):
        if sub_dla and entry != "model_spectra":
            continue
        rq.num_selected = n
        rq.selection = sel.ctypes.data_as(C.POINTER(C.c_int64))
        rq.weights_source = _lib.SPECTRA_WEIGHTS_REFINED
        rq.capacity = cap
        if entry == "model_spectra":
            rq.products = _lib.SPECTRA_MOMENTS
            rq.sub_dla = int(sub_dla)
        offsets = np.full(n + 1, -7, dtype=np.int64)
        status = np.full(n, -7, dtype=np.int32)
        st.offsets = offsets.ctypes.data_as(C.POINTER(C.c_int64))
        st.status = status.ctypes.data_as(C.POINTER(C.c_int32))
        arrays = {f: np.full(cap, sentinel) for f in fields}
        for f, a in arrays.items():
            setattr(st, f, a.ctypes.data_as(C.POINTER(C.c_double)))
        rc = getattr(lib, f"gpdla_batch_{entry}")(ctx._h, batch._h, C.byref(rq), C.byref(st))
        print(f"{entry}: rc {rc} {lib.gpdla_last_error()}")
        assert rc == code, (entry, rc, lib.gpdla_last_error())
        assert (status == -7).all() and (offsets == -7).all(), entry
        assert all((a == sentinel).all() for a in arrays.values()), entry


def test_refusals_write_nothing():
    k, nl = RC.CONFIGS[0]
    lib = _lib.load()
    ctx, batch = _context(k, nl, 63)
    try:
        batch.process()
        _refused(lib, batch, ctx, _lib.ERR_INVALID_ARGUMENT)          # before any refine
        assert b"not been refined" in lib.gpdla_last_error()
        for call in _calls(batch):
            with pytest.raises(_lib.GpdlaError):
                call()
        batch.refine(levels=XC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        assert batch.predictive_flux(weights="refined")["status"][0] == 0
        with pytest.raises(_lib.GpdlaError) as e:                    # the refined table is the DLA one
            batch.model_spectra(weights="refined", sub_dla=True, products=("moments",))
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
        _refused(lib, batch, ctx, _lib.ERR_INVALID_ARGUMENT, sub_dla=True)
        assert b"sub_dla" in lib.gpdla_last_error()
        ctx.set_refine_points(*RC.halton_points(63))                  # the same points again are still other points
        _refused(lib, batch, ctx, _lib.ERR_INVALID_ARGUMENT)
        assert b"refine points changed" in lib.gpdla_last_error()
        batch.refine(levels=XC.LEVELS, delta=RC.DELTA, pad=RC.PAD)
        assert batch.predictive_flux(weights="refined")["status"][0] == 0
        # a conditioned batch stays refused as it is
        first = batch.download()
        z = 0.5 * (first["min_z_dlas"][0] + first["max_z_dlas"][0])
        n = len(RC.KINDS)
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = 1                                                   # one absorber, on the first quasar
        batch.set_fixed_absorbers((off, np.array([z]), np.array([20.5])))
        for call in _calls(batch) + (lambda: batch.predictive_flux(weights="resident"),):
            with pytest.raises(_lib.GpdlaError) as e:
                call()
            assert e.value.code == _lib.ERR_UNSUPPORTED
        _refused(lib, batch, ctx, _lib.ERR_UNSUPPORTED)
        assert b"conditioned" in lib.gpdla_last_error()
    finally:
        batch.close()
        ctx.close()


# ------------------------------------------------------------------------------------------------
# 7. the first pass is untouched
# ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,nl,Sr", ALL)
def test_first_pass_untouched(k, nl, Sr):
    r = run(k, nl, Sr)
    for name, a in r["first"].items():
        np.testing.assert_array_equal(r["after"][name], a, err_msg=name)
    for key in ("ms", "mc", "pf"):
        for name, a in r["resident_before"][key].items():
            np.testing.assert_array_equal(r["resident_after"][key][name], a, err_msg=f"{key} {name}")


# ------------------------------------------------------------------------------------------------
# 8. the module-level driver and the command line
# ------------------------------------------------------------------------------------------------

def test_driver_and_command_line_equal_the_batch_path(tmp_path):
    from gp_dla_detection_amd import io, model_spectra as cli
    fs = synthetic.write_file_set(str(tmp_path / "in"), num_quasars=12, num_samples=96)
    run_pos = np.flatnonzero(fs["test_ind"])
    spectra = [fs["spectra"][i] for i in run_pos]
    results = gp.process_qsos(fs["model"], fs["samples"], spectra, prior_catalog=fs["prior"])
    processed = str(tmp_path / "processed.mat")
    io.save_processed_qsos(processed, results, test_ind=fs["test_ind"])
    sel = np.array(sorted([int(run_pos.size - 1), 0, 3, 5]))
    NP, LV = 65, 2
    # the Batch path: one batch of the selected quasars with the run's priors
    ctx = gp.Context(0, Parameters())
    ctx.set_model(fs["model"])
    ctx.set_samples(fs["samples"])
    ctx.set_refine_points(num=NP)
    batch = ctx.upload([spectra[i] for i in sel], results["log_priors_no_dla"][sel], results["log_priors_dla"][sel])
    try:
        batch.process()
        ref = batch.refine(levels=LV, with_samples=False)
        rp = batch.refined_posteriors()
        mw = np.stack([rp["p_no_dlas_refined"], np.zeros(sel.size), rp["p_dlas_refined"]], axis=1)
        mw = np.maximum(np.nan_to_num(mw, nan=0.0), 0.0)
        mw[~(mw.sum(axis=1) > 0)] = (1.0, 0.0, 1.0)
        want_pf = batch.predictive_flux(weights="refined", components=("null", "dla"), model_weights=mw, residuals=True)
        want_mc = batch.marginal_continuum(weights="refined", components=("null", "dla"), model_weights=mw)
        want_ms = batch.model_spectra(weights="refined", products=("moments",))
    finally:
        batch.close()
        ctx.close()
    kw = dict(selection=sel, refined=dict(levels=LV, points=NP))
    got = gp.predictive_flux(fs["model"], fs["samples"], spectra, results, components=("null", "dla"), model_weights="posteriors",
                             residuals=True, max_quasars_per_batch=3, **kw)
    for name in PF_ARRAYS + ("residual", "chi2", "num_kept", "status", "offsets"):
        np.testing.assert_array_equal(got[name], want_pf[name], err_msg=name)
    np.testing.assert_array_equal(got["boxes"], ref["boxes"])
    np.testing.assert_array_equal(got["refine_status"], ref["status"])
    got_mc = gp.marginal_continuum(fs["model"], fs["samples"], spectra, results, components=("null", "dla"), model_weights="posteriors", **kw)
    for name in MC_ARRAYS[1:] + ("status", "offsets"):
        np.testing.assert_array_equal(got_mc[name], want_mc[name], err_msg=name)
    got_ms = gp.model_spectra(fs["model"], fs["samples"], spectra, results, products=("moments",), absorbers=None, **kw)
    for name in MS_ARRAYS + ("status", "offsets"):
        np.testing.assert_array_equal(got_ms[name], want_ms[name], err_msg=name)
    # file to file
    common = ["--preloaded", fs["paths"]["preloaded"], "--catalog", fs["paths"]["catalog"], "--model", fs["paths"]["learned"],
              "--samples", fs["paths"]["samples"], "--processed", processed, "--indices", ",".join(map(str, sel)),
              "--refined", "--levels", str(LV), "--points", str(NP), "--max-quasars-per-batch", "3"]
    out = str(tmp_path / "pf.mat")
    assert cli.main(common + ["--out", out, "--predictive-flux", "--residuals", "--components", "null,dla"]) == 0
    back = io.load_predictive_flux(out)
    np.testing.assert_array_equal(back["selection"], sel)
    np.testing.assert_array_equal(back["status"], want_pf["status"])
    for name in io.PREDICTIVE_FLUX_CELLS:
        for g_, ref_ in zip(back[name], gp.split_cells(want_pf[name], want_pf["offsets"])):
            np.testing.assert_array_equal(g_, ref_, err_msg=name)
    np.testing.assert_array_equal(np.asarray(back["refine_boxes"]).reshape(sel.size, LV, 4), ref["boxes"])
    out = str(tmp_path / "ms.mat")
    assert cli.main(common + ["--out", out, "--products", "moments"]) == 0
    back = io.load_model_spectra(out)
    for name in MS_ARRAYS:
        for g_, ref_ in zip(back[name], gp.split_cells(want_ms[name], want_ms["offsets"])):
            np.testing.assert_array_equal(g_, ref_, err_msg=name)
    out = str(tmp_path / "mc.mat")
    assert cli.main(common + ["--out", out, "--marginal-continuum", "--components", "null,dla"]) == 0
    back = io.load_model_spectra(out)
    for g_, ref_ in zip(back["continuum_mean"], gp.split_cells(want_mc["continuum_mean"], want_mc["offsets"])):
        np.testing.assert_array_equal(g_, ref_)
    assert (want_pf["status"] == 0).any()
