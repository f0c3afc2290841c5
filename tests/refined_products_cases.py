"""What the tests of the per-pixel products on refined tables share (tests/test_refined_products.py on the
CPU, tests/test_gpu_refined_products.py on the GPU): the glue that turns a refine pass's boxes into inputs of the existing
restatements, and the restated DLA component of every product for one quasar.

The restatements (model_spectra_restatement, marginal_continuum_restatement, predictive_flux_restatement) read the search
range from ``g["min_z"]``, ``g["max_z"]`` and the samples from ``samples["offset_samples"]``, ``samples["nhi_samples"]``.
With a refined source the DLA component is their definition with (S, offset_samples, nhi_samples, l, min_z, max_z) replaced by
(S', u, N', lambda, z_lo, z_hi): a copy of the grid with the last box as range, (u, 10**(n_lo + (n_hi - n_lo) v)) as samples
and the downloaded lambda row as the table."""
import numpy as np

import marginal_continuum_restatement as MR
import model_spectra_restatement as R
import predictive_flux_restatement as PR

# the rows of refine_cases.KINDS restated at S' = 63 and 65 in both forms; one row at S' = 257 in the Woodbury form
RESTATED_KINDS = ("strong", "broad", "masked_run", "strong_masked")
SR_VALUES = (63, 65, 257)   # 64: the k <= 20 sample chunk, the solve chunk, the packing width; 256: a moments block
LEVELS = 2


def grid(oracle, model, sp, p, zero_range: bool = False) -> dict:
    """model_spectra_restatement.grid; for the zero-width batch of refine_cases (a context with max_z_cut = 0, one kept pixel)
    the same quantities with the oracle run at that cut, under which the quasar has a search range at all."""
    if not zero_range:
        return R.grid(oracle, model, sp, p)
    import refine_cases as RC
    wl = np.asarray(sp["wavelengths"], dtype=np.float64)
    rest = wl / (1 + sp["z_qso"])
    inside = (rest >= p.min_lambda) & (rest <= p.max_lambda)
    kept_in = (np.asarray(sp["pixel_mask"])[inside] == 0)
    op = RC.oracle_parameters(1, True)
    r = oracle.process_spectrum(model, np.array([0.5]), np.array([1e20]), wl, sp["flux"], sp["noise_variance"], sp["pixel_mask"],
                                sp["z_qso"], params=op, dump=True)
    assert r["rc"] == 0 and r["n_unmasked"] == inside.sum() and r["n_kept"] == kept_in.sum()
    g = dict(inside=inside, kept=kept_in, n_u=int(inside.sum()), wl=wl[inside], z_qso=float(sp["z_qso"]),
             pad=r["padded_wavelengths"], min_z=r["min_z_dla"], max_z=r["max_z_dla"], mu=r["this_mu"], M=r["this_M"],
             omega2=r["this_omega2"], y=np.asarray(sp["flux"], dtype=np.float64)[inside][kept_in],
             nu=np.asarray(sp["noise_variance"], dtype=np.float64)[inside][kept_in])
    assert np.array_equal(g["pad"][3:-3], g["wl"])
    return g


def boxed_inputs(g: dict, box, u, v, lam):
    """(grid, samples, row) for the restatements from a quasar's grid, its LAST box (z_lo, z_hi, n_lo, n_hi), the refine
    points and its refined sample log-posteriors."""
    z_lo, z_hi, n_lo, n_hi = (float(x) for x in box)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    if not (u.shape == v.shape == lam.shape and u.ndim == 1):
        raise ValueError(f"u {u.shape}, v {v.shape} and lambda {lam.shape} must be one row of S' entries each")
    grid = dict(g, min_z=z_lo, max_z=z_hi)
    samples = dict(offset_samples=u, nhi_samples=10.0 ** (n_lo + (n_hi - n_lo) * v))
    return grid, samples, lam


def refined_sample_parameters(box, u, v):
    """(z', log10 N') of the refined samples of a box."""
    z_lo, z_hi, n_lo, n_hi = (float(x) for x in box)
    return z_lo + (z_hi - z_lo) * np.asarray(u), n_lo + (n_hi - n_lo) * np.asarray(v)


def moments(oracle, g, box, u, v, lam, num_lines):
    gb, sb, row = boxed_inputs(g, box, u, v, lam)
    return R.moments(oracle, gb, sb["offset_samples"], sb["nhi_samples"], row, num_lines)


def marginal_continuum(oracle, model, g, box, u, v, lam, num_lines, form, p=(0.0, 0.0, 1.0), samples=None, lls_row=None):
    """The restated product of one quasar: the DLA component on the refined table; with p[1] > 0 the sub-DLA component on the
    first-pass table ``lls_row`` over ``samples`` (its own S samples and search range)."""
    gb, sb, row = boxed_inputs(g, box, u, v, lam)
    p = np.asarray(p, dtype=np.float64)
    p = p / p.sum()
    rows = MR.prepared_rows(oracle, model, g, False)
    parts = [MR.null_component(rows, form) if p[0] > 0 else None,
             MR.sampled_component(oracle, rows, g, samples["offset_samples"], samples["lls_nhi_samples"], lls_row, num_lines, form)
             if p[1] > 0 else None,
             MR.sampled_component(oracle, rows, gb, sb["offset_samples"], sb["nhi_samples"], row, num_lines, form) if p[2] > 0 else None]
    c, W, V = MR.mix(parts, p)
    mean, var, btw = MR.on_grid(oracle, model, g, False, c, W, V)
    out = dict(continuum_mean=mean, continuum_var=var, continuum_var_between=btw, coef_mean=c, coef_cov_within=MR.vech(W),
               coef_cov_between=MR.vech(V), status=0)
    if p[2] > 0:
        out["sample_coefficients"] = parts[2]["sample_coefficients"]
    return out


def predictive_flux(oracle, model, g, box, u, v, lam, num_lines, form, p=(0.0, 0.0, 1.0), samples=None, lls_row=None):
    gb, sb, row = boxed_inputs(g, box, u, v, lam)
    p = np.asarray(p, dtype=np.float64)
    p = p / p.sum()
    parts = [PR.component(oracle, model, g, None, "null", None, False, num_lines, form) if p[0] > 0 else None,
             PR.component(oracle, model, g, samples, "sub_dla", lls_row, False, num_lines, form) if p[1] > 0 else None,
             PR.component(oracle, model, gb, sb, "dla", row, False, num_lines, form) if p[2] > 0 else None]
    return dict(PR.mix(parts, p), status=0)


def ess(row) -> float:
    """T^2 / Sum w^2 of a row of log weights (refine_cases.ess)."""
    import refine_cases as RC
    return RC.ess(row)
