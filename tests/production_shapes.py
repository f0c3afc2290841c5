"""The production input shape, stratified (plain module: the CPU and GPU production-shape tests, the
exact-anchor fixture script and nothing else import it).

Every other parity test draws its quasars from ``synthetic.make_spectrum``: n pixels laid evenly over
the whole modelled rest range.  A DR12Q run looks different (``synthetic.make_boss_spectrum``): the BOSS
grid at 1e-4 dex, 262 .. 1250 in-range pixels set by z_qso, the spectrograph's blue edge at 3600 A and
masks in runs.  There the search range mostly starts at the FIRST KEPT PIXEL (``za`` below) instead of
at the Lyman limit (``zb``), which ``make_spectrum`` almost never produces.  :func:`stratified_quasars`
is a fixed list holding every such case at least once, :func:`census` recomputes from the definitions
which case each quasar is, and :func:`single_failures` is the comparison the GPU tests use -- kept here,
free of any GPU import, so that a CPU test can show that it catches a wrong search range.

    za = kept_min / lambda_Lya - 1                                   (set_parameters.m:70-73)
    zb = lambda_limit (1 + z_qso) / lambda_Lya - 1 + min_z_cut
    min_z_dla = max(za, zb),  max_z_dla = kept_max / lambda_Lya - 1 - max_z_cut   (:65-67)

``kept`` = in the rest range and not masked (process_qsos.m:110-115); the padded wavelengths of the
Voigt evaluation use the in-range pixels whether masked or not (``unmasked_ind``, :104-105, :168-176).
"""
from __future__ import annotations

import numpy as np

from gp_dla_detection_amd import synthetic
from gp_dla_detection_amd.parameters import Parameters

TOL = 1e-8          # every log-likelihood and evidence (absolute)
TOL_Z = 1e-14       # min / max z_DLA
TOL_POST = 1e-9     # posteriors

# (name, spectrum index [odd: a DLA is injected], z_qso, mask_runs, edit)
_PLAN = (
    ("shortest", 0, 2.16, False, None),
    ("za_mid_2.3", 1, 2.3, False, None),
    ("first_masked_za", 2, 2.5, False, "first"),
    ("crossover_za", 3, 2.93, False, None),
    ("crossover_zb", 4, 2.94, False, None),
    ("full_range_zb", 5, 3.5, False, None),
    ("beyond_4.6", 6, 4.6, False, None),
    ("beyond_5.7", 7, 5.7, True, None),
    ("last_masked_za", 8, 2.4, False, "last"),
    ("last_masked_zb", 9, 3.2, False, "last"),
    ("both_ends_masked_runs", 10, 2.6, True, "both"),
    ("tile_boundary_run", 11, 2.7, True, "tile"),
    ("confined_40px", 12, 3.8, False, "confined"),
    ("first_masked_zb", 13, 3.1, False, "first"),
    ("za_mid_2.5", 14, 2.5, True, None),
    ("shortest_dla_runs", 15, 2.17, True, None),
)
FIRST_RUN, LAST_RUN = 6, 5
TILE_RUN = (250, 263)        # stored-pixel indices 250 .. 262: across the 256-pixel tile of k_prepare
CONFINED = 40


def in_range(sp, p: Parameters | None = None) -> np.ndarray:
    p = p or Parameters()
    rest = np.asarray(sp["wavelengths"]) / (1 + sp["z_qso"])
    return (rest >= p.min_lambda) & (rest <= p.max_lambda)


def mask_pixels(sp, idx) -> None:
    """Mask stored pixels ``idx`` the way preload_qsos.m leaves them: NaN flux, infinite variance."""
    for key in ("flux", "noise_variance", "pixel_mask"):
        sp[key] = np.array(sp[key])
    sp["pixel_mask"][idx] = 1
    sp["flux"][idx] = np.nan
    sp["noise_variance"][idx] = np.inf


def _make(name, index, z_qso, runs, edit, model) -> dict:
    sp = synthetic.make_boss_spectrum(index, z_qso, model, mask_runs=runs)
    inside = np.flatnonzero(in_range(sp))
    if edit in ("first", "both"):
        mask_pixels(sp, inside[:FIRST_RUN])
    if edit in ("last", "both"):
        mask_pixels(sp, inside[-LAST_RUN:])
    if edit == "tile":
        mask_pixels(sp, np.arange(*TILE_RUN))
    if edit == "confined":
        mid = inside.size // 2
        keep = inside[mid:mid + CONFINED]
        mask_pixels(sp, np.setdiff1d(inside, keep))
    sp["stratum"], sp["index"], sp["mask_runs"], sp["edit"] = name, index, runs, edit
    return sp


def stratified_quasars(k: int = 20) -> list:
    """The fixed list (16 BOSS-grid quasars) for the default model of rank ``k``."""
    model = synthetic.make_model(k)
    return [_make(*row, model) for row in _PLAN]


def by_stratum(spectra, name) -> int:
    return [s["stratum"] for s in spectra].index(name)


def leading_mask_removed(sp, k: int = 20) -> dict:
    """``sp`` with the masked run at its blue end undone: the finite flux and variance the generator
    drew there are restored, so the first in-range pixel is kept and kept_min = un_min -- the quasar a
    kernel that took the search range from the unmasked-range minimum would in effect sweep."""
    clean = synthetic.make_boss_spectrum(sp["index"], sp["z_qso"], synthetic.make_model(k), mask_fraction=0.0)
    out = dict(sp)
    for key in ("flux", "noise_variance", "pixel_mask"):
        out[key] = np.array(sp[key])
    inside = np.flatnonzero(in_range(sp))
    run = inside[:np.flatnonzero(sp["pixel_mask"][inside] == 0)[0]]   # the leading masked in-range pixels
    assert run.size >= 1
    out["flux"][run] = clean["flux"][run]
    out["noise_variance"][run] = clean["noise_variance"][run]
    out["pixel_mask"][run] = 0
    assert np.isfinite(out["flux"][run]).all() and np.isfinite(out["noise_variance"][run]).all()
    return out


def census(spectra, p: Parameters | None = None) -> list:
    """Per quasar, from the definitions alone (no package code beyond the constants)."""
    p = p or Parameters()
    rows = []
    for sp in spectra:
        wl, mask = np.asarray(sp["wavelengths"]), np.asarray(sp["pixel_mask"]) != 0
        inside = in_range(sp, p)
        kept = inside & ~mask
        ii = np.flatnonzero(inside)
        row = dict(stratum=sp.get("stratum", ""), z_qso=float(sp["z_qso"]), n_stored=int(wl.size),
                   n_unmasked=int(inside.sum()), n_kept=int(kept.sum()),
                   has_dla=sp.get("true_z_dla") is not None)
        if row["n_kept"]:
            kmin, kmax = wl[kept].min(), wl[kept].max()
            za = kmin / p.lya_wavelength - 1
            zb = p.lyman_limit * (1 + sp["z_qso"]) / p.lya_wavelength - 1 + p.min_z_cut
            zmax = kmax / p.lya_wavelength - 1 - p.max_z_cut
            row.update(kept_min=float(kmin), kept_max=float(kmax), un_min=float(wl[inside].min()),
                       un_max=float(wl[inside].max()), za=float(za), zb=float(zb), za_wins=bool(za > zb),
                       min_z_dla=float(max(za, zb)), max_z_dla=float(zmax), z_width=float(zmax - max(za, zb)),
                       first_masked=bool(mask[ii[0]]), last_masked=bool(mask[ii[-1]]),
                       leading_masked=int(np.flatnonzero(~mask[ii])[0]),
                       trailing_masked=int(np.flatnonzero(~mask[ii][::-1])[0]),
                       longest_masked_run=_longest_run(mask[ii]),
                       masked_across_tile=bool(wl.size > 257 and mask[255] and mask[256]))
        rows.append(row)
    return rows


def _longest_run(m) -> int:
    best = cur = 0
    for v in m:
        cur = cur + 1 if v else 0
        best = max(best, cur)
    return best


MIX_FIRST_INDEX = 6000


def seeded_mix(model, num: int = 48) -> list:
    """``num`` quasars of the DR12Q mix: quasar i is what ``make_dr12q_mix(num, model,
    first_index=MIX_FIRST_INDEX, mask_runs=(i odd))`` holds at i -- independent masks on the even,
    run masks on the odd ones."""
    z = synthetic.sample_dr12q_redshifts(MIX_FIRST_INDEX + num)[MIX_FIRST_INDEX:]
    spectra = [synthetic.make_boss_spectrum(MIX_FIRST_INDEX + i, float(z[i]), model, mask_runs=bool(i % 2))
               for i in range(num)]
    for i, sp in enumerate(spectra):
        sp["stratum"] = f"mix {i}"
    return spectra


def production_samples(S: int) -> dict:
    """``make_samples(S)`` and then the four corners of the sample box: z offset exactly 0 and exactly 1
    (the Ly-alpha centre on the first / three thousand km/s inside the last kept pixel), each at the
    smallest and the largest column density (LLS: 10^19.5 and 10^20)."""
    s = synthetic.make_samples(S)
    off = np.array([0.0, 0.0, 1.0, 1.0])
    lognhi = np.array([20.0, 23.0, 20.0, 23.0])
    lls = np.array([19.5, 20.0, 19.5, 20.0])
    return dict(offset_samples=np.concatenate([s["offset_samples"], off]),
                log_nhi_samples=np.concatenate([s["log_nhi_samples"], lognhi]),
                nhi_samples=np.concatenate([s["nhi_samples"], 10.0 ** lognhi]),
                lls_log_nhi_samples=np.concatenate([s["lls_log_nhi_samples"], lls]),
                lls_nhi_samples=np.concatenate([s["lls_nhi_samples"], 10.0 ** lls]))


EDGE_NAMES = ("offset 0, N_HI 1e20", "offset 0, N_HI 1e23", "offset 1, N_HI 1e20", "offset 1, N_HI 1e23")


def flat_priors(n):
    return np.full(n, np.log(0.9)), np.full(n, np.log(0.1))


def oracle_single(oracle, model, samples, spectra, num_lines: int = 3) -> dict:
    """The oracle's results for a list of quasars under the field names ``process_qsos`` returns."""
    from oracle.oracle import OracleParams
    nq, S = len(spectra), samples["offset_samples"].size
    want = dict(min_z_dlas=np.full(nq, np.nan), max_z_dlas=np.full(nq, np.nan),
                log_likelihoods_no_dla=np.full(nq, np.nan), log_likelihoods_dla=np.full(nq, np.nan),
                sample_log_likelihoods_dla=np.full((nq, S), np.nan))
    for i, sp in enumerate(spectra):
        r = oracle.process_spectrum(model, samples["offset_samples"], samples["nhi_samples"], sp["wavelengths"],
                                    sp["flux"], sp["noise_variance"], sp["pixel_mask"], sp["z_qso"],
                                    params=OracleParams(num_lines=num_lines), num_threads=0)
        assert r["rc"] == 0, (i, r["rc"])
        want["min_z_dlas"][i], want["max_z_dlas"][i] = r["min_z_dla"], r["max_z_dla"]
        want["log_likelihoods_no_dla"][i] = r["log_likelihood_no_dla"]
        want["log_likelihoods_dla"][i] = r["log_likelihood_dla"]
        want["sample_log_likelihoods_dla"][i] = r["sample_log_likelihoods_dla"]
    return want


def _dev(a, b) -> float:
    """max |a - b|; inf where either side is not finite or the NaN patterns differ."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    if d.size == 0:
        return 0.0
    return float(np.inf) if not np.isfinite(d).all() else float(d.max())


def single_failures(got: dict, want: dict, spectra, log_priors=None, num_edge: int = 4):
    """Compare single-DLA results (``got``: what ``process_qsos`` returned; ``want``:
    :func:`oracle_single`) quasar by quasar at the project's tolerances.  Returns
    ``(failures, worst)``: one line per failing quasar naming z_qso, kept pixels, stratum and every
    deviation that is out of tolerance -- the last ``num_edge`` samples (the corners of the sample box)
    named apart from the rest -- and the worst log-likelihood deviation over all quasars."""
    rows = census(spectra)
    failures, worst = [], 0.0
    for i, (sp, c) in enumerate(zip(spectra, rows)):
        bad = []
        S = want["sample_log_likelihoods_dla"].shape[1]
        body = slice(0, S - num_edge)
        checks = [("min_z_dla", _dev(got["min_z_dlas"][i], want["min_z_dlas"][i]), TOL_Z),
                  ("max_z_dla", _dev(got["max_z_dlas"][i], want["max_z_dlas"][i]), TOL_Z),
                  ("null", _dev(got["log_likelihoods_no_dla"][i], want["log_likelihoods_no_dla"][i]), TOL),
                  ("samples", _dev(got["sample_log_likelihoods_dla"][i][body],
                                   want["sample_log_likelihoods_dla"][i][body]), TOL),
                  ("evidence", _dev(got["log_likelihoods_dla"][i], want["log_likelihoods_dla"][i]), TOL)]
        for e in range(num_edge):
            j = S - num_edge + e
            checks.append((f"edge sample [{EDGE_NAMES[e] if num_edge == 4 else e}]",
                           _dev(got["sample_log_likelihoods_dla"][i][j], want["sample_log_likelihoods_dla"][i][j]), TOL))
        if log_priors is not None:   # process_qsos.m:153-154, 212-213, 224-233
            post = np.array([log_priors[0][i] + want["log_likelihoods_no_dla"][i],
                             log_priors[1][i] + want["log_likelihoods_dla"][i]])
            mp = np.exp(post - post.max())
            mp /= mp.sum()
            checks += [("log posterior no DLA", _dev(got["log_posteriors_no_dla"][i], post[0]), TOL),
                       ("log posterior DLA", _dev(got["log_posteriors_dla"][i], post[1]), TOL),
                       ("model posteriors", _dev(got["model_posteriors"][i], mp), TOL_POST),
                       ("p_no_dla", _dev(got["p_no_dlas"][i], mp[0]), TOL_POST),
                       ("p_dla", _dev(got["p_dlas"][i], 1 - mp[0]), TOL_POST)]
            if "status" in got:
                checks.append(("status", float(got["status"][i] != 0), 0.5))
        for name, d, tol in checks:
            if tol == TOL:
                worst = max(worst, d)
            if not d < tol:
                bad.append(f"{name} {d:.2e}")
        if bad:
            failures.append(f"quasar {i} [{c['stratum']}] z_qso = {c['z_qso']:.4f}, {c['n_kept']} kept of "
                            f"{c['n_unmasked']} pixels, {'za' if c.get('za_wins') else 'zb'} wins: " + ", ".join(bad))
    return failures, worst
