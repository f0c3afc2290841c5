"""Times the posterior-moments kernel of the model-spectra subsystem at production
scale: ``--quasars`` x ``--pixels`` x ``--samples`` (default 1000 x 1500 x 10^4) with peaked synthetic
posteriors supplied as a host table (no sweep is run).  Reports, from device events in ONE process,

* the per-quasar time of k_spectra_moments (+ the combine launch) -- gpdla_context_last_sweep_ms after
  Batch.model_spectra;
* the per-quasar time of k_profiles on the same spectra and samples (gpdla_debug_profiles_ms): the
  Voigt stage of the multi-DLA driver, which evaluates the same line sums, takes one more exponential
  per pixel (two column densities) and stores 2 S n values where the moments kernel reduces them;
* their ratio, the wall time of the whole model_spectra call (prepare, weights, moments, copies), and
  the CPU restatement's time per quasar (tests/model_spectra_restatement.py on ``--cpu-samples``
  samples of one quasar, scaled to S).

``--files NQ`` instead times the file-to-file command on a synthetic DR12Q-like shard of NQ quasars
(``synthetic.write_file_set``, swept once by ``run_dr12q.run`` to make the processed file): every
tenth quasar of the run selected, ``python -m gp_dla_detection_amd.model_spectra``'s ``run`` from the
-v7.3 inputs and the processed file's streamed sample rows to the -v7.3 output.

``--multi-models`` times the moments of the models of two or more absorbers instead:
``--distinct`` quasars (default 16) are swept once by ``process_multi`` at ``--max-dlas`` (default 4) -- with the
driver's own resampled base indices, or uniform random ones (``--multi-base random``: the gathered redshifts of a
wave are then no neighbours at all) -- and a selection of ``--quasars`` entries repeating them is reduced from
the resident tables.  Reports the per-entry time of models 2 .. max_dlas (k_spectra_weights_multi,
k_spectra_moments_multi and their combines: gpdla_context_last_sweep_ms after Batch.model_spectra_multi), the
per-entry time of k_spectra_moments (+ combine) for the DLA(1) rows of the SAME selection in the same process,
their ratio, the profiles evaluated per sample (n (n + 1) / 2 - 1 summed over the models: 9 for max_dlas = 4)
and the (entry, model) rows the kernel skipped because they carry no weight.

Prints one JSON line.  Kernel times: run under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gp_dla_detection_amd as gp  # noqa: E402
from gp_dla_detection_amd import _lib, synthetic  # noqa: E402
from gp_dla_detection_amd.parameters import MultiParameters  # noqa: E402


def peaked_rows(nq, S, seed=1):
    """Each quasar's likelihood mass within a few dozen samples of a centre (every fifth: a handful)."""
    rng = np.random.default_rng(seed)
    centre = rng.integers(0, S, nq)
    j = np.arange(S)
    rows = np.empty((nq, S))
    for s in range(nq):
        rows[s] = -8000.0 - (3.0 if s % 5 == 0 else 0.05) * np.abs(j - centre[s])
    return rows


def files_run(nq, S):
    import tempfile

    from gp_dla_detection_amd import model_spectra as cli, run_dr12q
    d = tempfile.mkdtemp(prefix="gpdla_spectra_")
    t0 = time.perf_counter()
    fs = synthetic.write_file_set(d, num_quasars=nq, num_samples=S, skip_every=10 ** 9, empty_quasar=None)
    t_gen = time.perf_counter() - t0
    paths, prior = fs["paths"], fs["prior"]
    del fs
    t0 = time.perf_counter()
    res = run_dr12q.run(paths["preloaded"], paths["catalog"], paths["learned"], paths["samples"], d + "/out", "synth",
                        prior_catalog=prior, device=0)
    t_sweep = time.perf_counter() - t0
    idx = np.arange(0, nq, 10)
    cli.run(paths["preloaded"], paths["catalog"], paths["learned"], paths["samples"], res["chunk"], d + "/warm.mat",
            indices=idx[:8])                                                                          # warm-up
    t0 = time.perf_counter()
    out = cli.run(paths["preloaded"], paths["catalog"], paths["learned"], paths["samples"], res["chunk"],
                  d + "/model_spectra.mat", indices=idx)
    t_run = time.perf_counter() - t0
    print(json.dumps(dict(mode="files", quasars=nq, samples=S, selected=int(idx.size), generate_inputs_s=t_gen,
                          sweep_file_to_file_s=t_sweep, model_spectra_file_to_file_s=t_run,
                          grid_pixels=int(out["offsets"][-1]), processed_bytes=os.path.getsize(res["chunk"]),
                          output_bytes=os.path.getsize(d + "/model_spectra.mat"),
                          finite_mean_rows=int(sum(np.isfinite(c).all() for c in gp.split_cells(out["mean_absorption"], out["offsets"]))))))


def multi_models_run(a):
    nq, n, S, md = a.quasars, a.pixels, a.samples, a.max_dlas
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(S)
    nd = min(nq, a.distinct)
    spectra = [synthetic.make_spectrum(9000 + i, n, model, mask_fraction=0.03) for i in range(nd)]
    sel = (np.arange(nq) % nd).astype(np.int64)
    out = dict(mode="multi_models", entries=nq, distinct_quasars=nd, pixels=n, samples=S, max_dlas=md, base=a.multi_base,
               libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16])
    p = MultiParameters(max_dlas=md)
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        ctx.set_timing(True)
        lp_dla = np.log(np.full((nd, md), 0.1) ** np.arange(1, md + 1))
        batch = ctx.upload(spectra, np.full(nd, np.log(0.85)), lp_dla, np.full(nd, np.log(0.05)))
        base = None
        if a.multi_base == "random":
            base = np.random.default_rng(5).integers(1, S + 1, (nd, md - 1, S)).astype(np.uint32)
        batch.process_multi(base)
        ctx.synchronize()
        kw = dict(models=(2, md), products=("models",), sub_dla=False)
        batch.model_spectra_multi(selection=sel[:8], **kw)                                              # warm-up
        batch.model_spectra(selection=sel[:8], weights="resident", products=("moments",))
        multi_ms, one_ms, wall_s = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = batch.model_spectra_multi(selection=sel, **kw)
            wall_s.append(time.perf_counter() - t0)
            multi_ms.append(ctx.last_sweep_ms())
            batch.model_spectra(selection=sel, weights="resident", products=("moments",))
            one_ms.append(ctx.last_sweep_ms())
        batch.close()
    finally:
        ctx.close()
    flagged = int(sum(bin(int(f) >> 1 & ((1 << (md - 1)) - 1)).count("1") for f in res["model_flags"]))
    profiles = sum(range(2, md + 1))
    m, o = float(np.median(multi_ms)), float(np.median(one_ms))
    out.update(multi_ms=multi_ms, single_profile_ms=one_ms, multi_ms_per_entry=m / nq, single_profile_ms_per_entry=o / nq,
               multi_over_single_profile=m / o, profiles_per_sample=profiles, ratio_per_profile=m / o / profiles,
               flagged_rows_skipped=flagged, rows=nq * (md - 1), model_spectra_multi_call_s=float(np.median(wall_s)),
               finite_rows=int(np.isfinite(res["mean_absorption_models"][1:]).all(axis=1).sum()))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multi-models", action="store_true", help="time the models of two or more absorbers (DESIGN.md 4.21)")
    ap.add_argument("--max-dlas", type=int, default=4)
    ap.add_argument("--distinct", type=int, default=16, help="--multi-models: quasars swept; the entries repeat them")
    ap.add_argument("--multi-base", choices=("resampled", "random"), default="resampled")
    ap.add_argument("--files", type=int, default=0, help="time the file-to-file command on a shard of this many quasars")
    ap.add_argument("--quasars", type=int, default=1000)
    ap.add_argument("--pixels", type=int, default=1500)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-samples", type=int, default=500)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    if a.files:
        return files_run(a.files, a.samples)
    if a.multi_models:
        return multi_models_run(a)
    nq, n, S = a.quasars, a.pixels, a.samples
    model = synthetic.make_model(20)
    samples = synthetic.make_samples(S)
    distinct = [synthetic.make_spectrum(9000 + i, n, model, mask_fraction=0.03) for i in range(min(nq, 64))]
    spectra = [distinct[i % len(distinct)] for i in range(nq)]
    rows = peaked_rows(nq, S)
    out = dict(quasars=nq, pixels=n, samples=S,
               libgpdla_sha256=hashlib.sha256(open(_lib.lib_path(), "rb").read()).hexdigest()[:16])
    p = MultiParameters(max_dlas=1)
    ctx = gp.Context(0, p)
    try:
        ctx.set_model(model)
        ctx.set_samples(samples)
        ctx.set_timing(True)
        batch = ctx.upload(spectra, np.zeros(nq), np.zeros((nq, 1)), np.zeros(nq))
        batch.model_spectra(selection=np.arange(min(nq, 8)), weights=rows[:8], products=("moments",))   # warm-up
        mom_ms, wall_s = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            res = batch.model_spectra(weights=rows, products=("moments",))
            wall_s.append(time.perf_counter() - t0)
            mom_ms.append(ctx.last_sweep_ms())
        prof_ms = []
        ms = C.c_double()
        for _ in range(a.repeats + 1):                                                                 # first: warm-up
            _lib.check(ctx.lib.gpdla_debug_profiles_ms(ctx._h, batch._h, C.byref(ms)))
            prof_ms.append(ms.value)
        prof_ms = prof_ms[1:]
        batch.close()
    finally:
        ctx.close()
    assert np.isfinite(res["mean_absorption"]).all()
    m, pr = float(np.median(mom_ms)), float(np.median(prof_ms))
    out.update(moments_ms=mom_ms, profiles_ms=prof_ms, moments_ms_per_quasar=m / nq, profiles_ms_per_quasar=pr / nq,
               moments_over_profiles=m / pr, model_spectra_call_s=float(np.median(wall_s)),
               faddeeva_evaluations=float(nq) * S * (n + 6) * 3, moments_gevals_per_s=nq * S * (n + 6) * 3 / (m * 1e-3) / 1e9)
    if not a.no_cpu:
        import model_spectra_restatement as R
        from oracle import oracle
        g = R.grid(oracle, model, spectra[0])
        sub = a.cpu_samples
        c0 = time.perf_counter()
        R.moments(oracle, g, samples["offset_samples"][:sub], samples["nhi_samples"][:sub], rows[0, :sub], 3)
        per = (time.perf_counter() - c0) / sub * S
        out.update(cpu_restatement_samples=sub, cpu_restatement_s_per_quasar=per)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
