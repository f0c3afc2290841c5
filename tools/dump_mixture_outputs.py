"""Writes every array the four mixture entries (Batch.marginal_continuum, .predictive_flux and their ``_multi`` forms,
DESIGN.md 4.23 - 4.25) return on a fixed list of seeded cases to one ``.npz``, for a bit-for-bit comparison of two builds
of the library: run it once per library (GPDLA_LIB_PATH), each run in a process of its own, then

    python tools/dump_mixture_outputs.py --compare a.npz b.npz

prints the number of arrays and of differing elements (NaN patterns count: the arrays are compared as bit patterns).
The cases: the setups of tests/mixture_multi_cases.py on host tables (and on the resident tables with the resident
model_posteriors where the setup sweeps), the two cases of each single-DLA launch-group worker (resident weights; host
tables under an unsorted selection), and one k = 40 case with 31 lines through all four entries."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def multi_case(st, single_too=False):
    import gp_dla_detection_amd as gp
    import mixture_multi_cases as XC
    model, samples, spectra = XC.build(st)
    p, P, n, md = XC.params(st), XC.model_weights(st), len(st["nus"]), st["md"]
    ctx = gp.Context(0, p)
    ctx.set_model(model)
    ctx.set_samples(samples)
    lp_dla = np.log(np.full((n, md), 0.1) ** np.arange(1, md + 1))
    batch = ctx.upload(spectra, np.full(n, np.log(0.85)), lp_dla, np.full(n, np.log(0.05)))
    out = {}
    try:
        swept = "sweep" in st["kinds"]
        if swept:
            batch.process_multi(XC.base_in(st, samples))
            down = batch.download_multi()
            sweep = (np.array(down["sample_log_likelihoods_dla"]), np.array(down["sample_log_likelihoods_lls"]))
        else:
            sweep = XC.synthetic_sweep(st)
        tables = XC.host_tables(st, samples, *sweep)
        calls = {"mc": batch.marginal_continuum_multi, "pf": batch.predictive_flux_multi}
        for tag, call in calls.items():
            out[f"host_{tag}"] = call(tables=tables, model_weights=P, meanflux=st["meanflux"])
            if swept:
                out[f"resident_{tag}"] = call(tables="resident", meanflux=st["meanflux"])
        if single_too:
            w = {"dla": tables["sample_log_likelihoods_dla"][:, 0], "sub_dla": tables["sample_log_likelihoods_lls"]}
            kw = dict(weights=w, components=("null", "sub_dla", "dla"), model_weights=P[:, :3], meanflux=st["meanflux"])
            out["single_mc"] = batch.marginal_continuum(**kw)
            out["single_pf"] = batch.predictive_flux(**kw)
    finally:
        batch.close()
        ctx.close()
    return {f"{st['name']}/{tag}/{name}": np.asarray(v) for tag, res in out.items() for name, v in res.items()}


def dump(path):
    import marginal_continuum_groups_worker as mc_worker
    import mixture_multi_cases as XC
    import predictive_flux_groups_worker as pf_worker
    arrays = {}
    for st in XC.SETUPS:
        arrays.update(multi_case(st))
    arrays.update(multi_case(dict(XC.setup("k40_S64_md2_one"), name="k40_S64_md2_31lines", lines=31, kinds=("flat", "flat")), single_too=True))
    arrays.update({f"mc_groups/{name}": np.asarray(v) for name, v in mc_worker.run_case().items()})
    arrays.update({f"pf_groups/{name}": np.asarray(v) for name, v in pf_worker.run_case().items()})
    np.savez(path, **arrays)
    print(f"{len(arrays)} arrays -> {path}")


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two files hold different arrays"
    differing = 0
    for name in a.files:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        assert x.shape == y.shape and x.dtype == y.dtype, name
        bad = int((x.view(np.uint8) != y.view(np.uint8)).reshape(x.size, -1).any(axis=1).sum()) if x.size else 0
        if bad:
            print(f"{name}: {bad} of {x.size} elements differ")
        differing += bad
    print(f"{len(a.files)} arrays, {sum(a[n].size for n in a.files)} elements, {differing} differing")
    return 1 if differing else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else dump(args.out))
