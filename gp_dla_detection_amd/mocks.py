"""Mock sightlines for injection and recovery:

    python -m gp_dla_detection_amd.mocks --preloaded preloaded_qsos.mat --catalog catalog.mat \\
        --model learned_qso_model.mat --samples dla_samples.mat --out-preloaded mock_preloaded_qsos.mat \\
        --out-truth mock_truth.mat --p-absorbers 0.8,0.15,0.05 --seed 7

reads a ``preloaded_qsos.mat`` -- its wavelengths, noise variances and pixel masks are the templates --
the catalogue (for the redshifts) and a learned model, draws a truth table on the host
(:func:`draw_truth`) and one spectrum per quasar on the GPU from the distribution whose likelihood the
sweeps evaluate (:func:`gp_dla_detection_amd.api.draw_mock_spectra`), and writes a mock
``preloaded_qsos`` file that ``run_dr12q`` reads unchanged plus a truth file
(``truth_offsets`` [nq + 1], ``truth_z_dlas``, ``truth_log_nhis``: CSR over ALL catalogue quasars, and
``status``).  :mod:`gp_dla_detection_amd.validation` scores a processed run against that file.
"""
from __future__ import annotations

import argparse

import numpy as np

from . import api, io
from .parameters import MultiParameters, Parameters


def search_range(template: dict, params: Parameters | None = None):
    """``(min_z_dla, max_z_dla)`` of one quasar (set_parameters.m:65-73 on the kept pixels of the
    modelled rest range, process_qsos.m:159-160), or None when it has no kept pixel."""
    p = params or Parameters()
    wl = np.asarray(template["wavelengths"], dtype=np.float64)
    rest = wl / (1 + float(template["z_qso"]))
    keep = (rest >= p.min_lambda) & (rest <= p.max_lambda) & (np.asarray(template["pixel_mask"]) == 0)
    if not keep.any():
        return None
    return p.min_z_dla(wl[keep], float(template["z_qso"])), p.max_z_dla(wl[keep], float(template["z_qso"]))


def draw_truth(templates, z_qsos=None, num_absorber_probabilities=(0.5, 0.5), log_nhi_range=(20.0, 23.0),
               samples: dict | None = None, min_z_separation: float = 0.0, seed: int = 0,
               params: Parameters | None = None):
    """A truth table for ``templates``, on the host: quasar i gets n absorbers with probability
    ``num_absorber_probabilities[n]`` (at most 8), each with z uniform in the quasar's
    ``[min_z_dla, max_z_dla]`` and log10 N_HI uniform in ``log_nhi_range`` -- or, with ``samples``,
    drawn from its ``log_nhi_samples`` (the finder's own column-density prior).  Absorbers of one
    quasar are at least ``min_z_separation`` apart in redshift (a candidate closer than that to an
    earlier one is drawn again, 1000 times at most).  ``z_qsos``: overrides the templates' ``z_qso``.
    A quasar without a kept pixel or with an empty search range gets none.
    Returns the CSR triple ``(offsets [nq + 1], z_dlas, log_nhis)`` :meth:`Batch.draw_mocks` and
    :meth:`Batch.model_spectra` take; absorbers of a quasar are in ascending redshift."""
    p = params or Parameters()
    rng = np.random.default_rng(seed)
    probs = np.asarray(num_absorber_probabilities, dtype=np.float64)
    if probs.ndim != 1 or probs.size < 1 or probs.size > 9 or (probs < 0).any() or not probs.sum() > 0:
        raise ValueError("num_absorber_probabilities: non-negative weights for 0 .. at most 8 absorbers")
    probs = probs / probs.sum()
    pool = None if samples is None else np.asarray(samples["log_nhi_samples"], dtype=np.float64)
    templates = list(templates)
    offsets = np.zeros(len(templates) + 1, dtype=np.int64)
    zs, ns = [], []
    for i, t in enumerate(templates):
        if z_qsos is not None:
            t = dict(t, z_qso=float(np.asarray(z_qsos).reshape(-1)[i]))
        count = int(rng.choice(probs.size, p=probs))
        rngz = search_range(t, p)
        mine = []
        if rngz is not None and rngz[1] > rngz[0]:
            for _ in range(count):
                for _ in range(1000):
                    z = float(rng.uniform(rngz[0], rngz[1]))
                    if all(abs(z - other) >= min_z_separation for other, _ in mine):
                        ln = float(rng.choice(pool)) if pool is not None else float(rng.uniform(*log_nhi_range))
                        mine.append((z, ln))
                        break
        mine.sort()
        zs += [z for z, _ in mine]
        ns += [ln for _, ln in mine]
        offsets[i + 1] = len(zs)
    return offsets, np.array(zs, dtype=np.float64), np.array(ns, dtype=np.float64)


def save_truth(path: str, truth, status=None, **metadata) -> None:
    off, z, ln = truth
    col = lambda a, dt=np.float64: np.asarray(a, dtype=dt).reshape(-1, 1)  # noqa: E731
    variables = dict(truth_offsets=col(off), truth_z_dlas=col(z), truth_log_nhis=col(ln))
    if status is not None:
        variables["status"] = col(status)
    variables.update(metadata)
    io.savemat73(path, variables)


def load_truth(path: str):
    """The CSR triple of a truth file written by :func:`save_truth`."""
    m = io.loadmat73(path, ("truth_offsets", "truth_z_dlas", "truth_log_nhis"))
    flat = lambda a, dt: np.asarray(a, dtype=np.float64).reshape(-1).astype(dt)  # noqa: E731
    return flat(m["truth_offsets"], np.int64), flat(m["truth_z_dlas"], np.float64), flat(m["truth_log_nhis"], np.float64)


def run(preloaded: str, catalog: str, model_file: str, samples_file: str, out_preloaded: str, out_truth: str,
        num_absorber_probabilities=(0.5, 0.5), log_nhi_range=(20.0, 23.0), nhi_from_samples: bool = False,
        min_z_separation: float | None = None, seed: int = 0, multi: bool = False, device: int = 0,
        max_quasars_per_batch: int | None = None) -> dict:
    """The file-to-file form (see the module docstring).  Every quasar of the catalogue is drawn, so
    the mock file lines up with the catalogue whatever ``test_ind`` a later run selects."""
    p = MultiParameters() if multi else Parameters()
    z_qsos = np.asarray(io.load_catalog(catalog, ("z_qsos",))["z_qsos"], dtype=np.float64)
    templates = io.load_preloaded_qsos(preloaded, z_qsos)
    model, samples = io.load_learned_model(model_file), io.load_dla_samples(samples_file)
    sep = getattr(p, "min_z_separation", 0.0) if min_z_separation is None else min_z_separation
    truth = draw_truth(templates, None, num_absorber_probabilities, log_nhi_range,
                       samples if nhi_from_samples else None, sep, seed, p)
    res = api.draw_mock_spectra(model, samples, templates, truth, params=p, seed=seed, device=device,
                                max_quasars_per_batch=max_quasars_per_batch)
    cells = {}
    for key, src in (("all_wavelengths", [t["wavelengths"] for t in templates]), ("all_flux", res["flux"]),
                     ("all_noise_variance", [t["noise_variance"] for t in templates]),
                     ("all_pixel_mask", [t["pixel_mask"] for t in templates])):
        dt = bool if key == "all_pixel_mask" else np.float64
        cells[key] = [np.asarray(a).astype(dt).reshape(-1, 1) for a in src]
    io.savemat73(out_preloaded, cells, compress=True)
    save_truth(out_truth, truth, res["status"], seed=np.float64(seed), meanflux=np.float64(multi))
    return dict(truth=truth, flux=res["flux"], status=res["status"], templates=templates)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    for name in ("preloaded", "catalog", "model", "samples", "out-preloaded", "out-truth"):
        ap.add_argument(f"--{name}", required=True)
    ap.add_argument("--p-absorbers", type=str, default="0.5,0.5",
                    help="probabilities of 0, 1, 2, ... absorbers per quasar (comma-separated)")
    ap.add_argument("--log-nhi-range", type=str, default="20,23")
    ap.add_argument("--nhi-from-samples", action="store_true", help="column densities from log_nhi_samples")
    ap.add_argument("--min-z-separation", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--multi", action="store_true", help="draw from the mean-flux model of the multi-DLA driver")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-quasars-per-batch", type=int, default=None)
    a = ap.parse_args(argv)
    res = run(a.preloaded, a.catalog, a.model, a.samples, a.out_preloaded, a.out_truth,
              tuple(float(x) for x in a.p_absorbers.split(",")), tuple(float(x) for x in a.log_nhi_range.split(",")),
              a.nhi_from_samples, a.min_z_separation, a.seed, a.multi, a.device, a.max_quasars_per_batch)
    print(f"wrote {a.out_preloaded}: {len(res['flux'])} quasars, {int(res['truth'][0][-1])} absorbers; truth in {a.out_truth}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
