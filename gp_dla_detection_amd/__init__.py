"""gp_dla_detection_amd -- MI355X-native GP marginal-likelihood sweep for DLA detection.

One hot path of jibanCat/gp_dla_detection (the per-spectrum sweep of ``process_qsos.m``) rebuilt
for gfx950: hand-written HIP kernels behind a C-ABI (``include/gpdla.h``), with this package as the
Python host side mirroring the reference's call surface.  See DESIGN.md.
"""
from .api import (Batch, Context, absorption_distribution, forest_mask, dla_existence_prior, dla_existence_prior_multi, dla_model_mean, draw_mock_spectra,
                  log_mvnpdf_low_rank, map_absorbers, marginal_continuum, predictive_flux, prepare_prior, process_qsos, renormalised_model_posteriors,
                  process_qsos_multiple_dlas_meanflux, spectra_to_csr, split_cells, voigt)
from .parameters import MultiParameters, Parameters, kms_to_z
from .training import learn_qso_model
from . import model_spectra  # the module; calling it is api.model_spectra (it shares the function's name)

__all__ = ["Batch", "Context", "dla_existence_prior", "dla_existence_prior_multi",
           "log_mvnpdf_low_rank", "prepare_prior", "process_qsos", "process_qsos_multiple_dlas_meanflux",
           "spectra_to_csr", "voigt", "dla_model_mean", "draw_mock_spectra", "map_absorbers", "absorption_distribution", "forest_mask", "marginal_continuum", "predictive_flux", "model_spectra", "renormalised_model_posteriors", "split_cells", "Parameters", "MultiParameters", "kms_to_z", "learn_qso_model"]
