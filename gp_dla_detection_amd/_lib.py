"""ctypes binding of libgpdla.so (the C-ABI declared in include/gpdla.h).

The library is built in-tree (``gp_dla_detection_amd/csrc/libgpdla.so``) by ``build()`` below or
``__graft_entry__.build()``.  There is no fallback: if the shared object is missing, or the GPU is,
the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
#: the product library
DEFAULT_LIB_PATH = os.path.join(CSRC, "libgpdla.so")


def lib_path() -> str:
    """The library load() opens: GPDLA_LIB_PATH if set (read at call time, so a child process may
    set it after this module was imported), else the in-tree product library.  GPDLA_LIB_PATH is a
    diagnostic override: library variants made by tools/ab_build.sh;
    libgpdla_legacy.so for the bit-identity tests."""
    return os.environ.get("GPDLA_LIB_PATH") or DEFAULT_LIB_PATH

# -no-hip-rt: libgpdla.so does NOT carry its own DT_NEEDED on libamdhip64.  A process must hold
# exactly one HIP runtime (a second copy cannot open the GPU, and a hipStream_t only means
# something to the runtime that made it), so the library binds to whichever runtime its host
# process already loaded: PyTorch's bundled one under Python (preloaded below), `-lamdhip64` for a
# C / MEX consumer.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared",
               "-std=c++17", "-no-hip-rt", "-Wno-inline-asm"]

#: the second library: the same source with the superseded kernels and their environment switches
#: compiled in (csrc/host_legacy.hpp, GPDLA_WITH_LEGACY).  Only bit-identity and launch-group tests load it,
#: through GPDLA_LIB_PATH; nothing in the package does.
LEGACY_LIB_PATH = os.path.join(CSRC, "libgpdla_legacy.so")

_dp = C.POINTER(C.c_double)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_f32p = C.POINTER(C.c_float)


# gpdla_status (include/gpdla.h)
ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_NOT_POSITIVE_DEFINITE, ERR_UNSUPPORTED, ERR_HOST = -1, -2, -3, -4, -5, -6


class GpdlaError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libgpdla error {code}: {message}")
        self.code = code


class Model(C.Structure):
    _fields_ = [("num_rest_pixels", C.c_int32), ("k", C.c_int32), ("rest_wavelengths", _dp),
                ("mu", _dp), ("M", _dp), ("log_omega", _dp), ("log_c_0", C.c_double),
                ("log_tau_0", C.c_double), ("log_beta", C.c_double)]


class Samples(C.Structure):
    _fields_ = [("num_dla_samples", C.c_int64), ("offset_samples", _dp), ("log_nhi_samples", _dp),
                ("nhi_samples", _dp), ("lls_nhi_samples", _dp)]


class Spectra(C.Structure):
    _fields_ = [("num_quasars", C.c_int64), ("offsets", _i64p), ("wavelengths", _dp),
                ("flux", _dp), ("noise_variance", _dp), ("pixel_mask", _u8p), ("z_qsos", _dp),
                ("log_priors_no_dla", _dp), ("log_priors_dla", _dp), ("log_priors_lls", _dp)]


class SpectraCells(C.Structure):
    """gpdla_spectra_cells: one array per quasar (pointer arrays are passed as void*: uintp NumPy arrays)."""
    _fields_ = [("num_quasars", C.c_int64), ("num_pixels", _i64p), ("wavelengths", C.c_void_p),
                ("flux", C.c_void_p), ("noise_variance", C.c_void_p), ("pixel_mask", C.c_void_p),
                ("z_qsos", _dp), ("log_priors_no_dla", _dp), ("log_priors_dla", _dp), ("log_priors_lls", _dp)]


class Config(C.Structure):
    _fields_ = [("min_lambda", C.c_double), ("max_lambda", C.c_double),
                ("lya_wavelength", C.c_double), ("lyman_limit", C.c_double),
                ("pixel_spacing", C.c_double), ("max_z_cut", C.c_double),
                ("min_z_cut", C.c_double), ("width", C.c_int32), ("num_lines", C.c_int32),
                ("max_dlas", C.c_int32), ("num_forest_lines", C.c_int32),
                ("min_z_separation", C.c_double), ("prev_tau_0", C.c_double),
                ("prev_beta", C.c_double), ("rng_seed", C.c_uint64),
                ("first_quasar_index", C.c_int64), ("contraction_precision", C.c_int32),
                ("multi_profile_bytes", C.c_int64), ("record_pool_bytes", C.c_int64),
                ("pipeline_slots", C.c_int32), ("max_quasars_per_batch", C.c_int64)]


class LearnConfig(C.Structure):
    _fields_ = [("min_lambda", C.c_double), ("dlambda", C.c_double), ("num_rest_pixels", C.c_int64),
                ("lya_wavelength", C.c_double), ("max_noise_variance", C.c_double),
                ("prev_tau_0", C.c_double), ("prev_beta", C.c_double), ("num_forest_lines", C.c_int32)]


class Results(C.Structure):
    _fields_ = [("min_z_dlas", _dp), ("max_z_dlas", _dp), ("log_likelihoods_no_dla", _dp),
                ("sample_log_likelihoods_dla", _dp), ("log_likelihoods_dla", _dp),
                ("log_posteriors_no_dla", _dp), ("log_posteriors_dla", _dp),
                ("model_posteriors", _dp), ("p_no_dlas", _dp), ("p_dlas", _dp),
                ("status", _i32p), ("MAP_inds", _dp), ("MAP_z_dlas", _dp), ("MAP_log_nhis", _dp)]


class ResultsMulti(C.Structure):
    _fields_ = [(n, _dp) for n in (
        "min_z_dlas", "max_z_dlas", "log_likelihoods_no_dla", "sample_log_likelihoods_dla",
        "sample_log_likelihoods_lls", "log_likelihoods_dla", "log_likelihoods_lls",
        "log_posteriors_no_dla", "log_posteriors_lls", "log_posteriors_dla", "model_posteriors",
        "p_no_dlas", "p_lls", "p_dlas", "MAP_z_dlas", "MAP_log_nhis", "MAP_inds")] + [
        ("base_sample_inds", _u32p), ("status", _i32p)]


class BinRequest(C.Structure):
    """gpdla_bin_request"""
    _fields_ = [("quantity", C.c_int32), ("num_bins", C.c_int32), ("edges", _dp), ("z_lo", C.c_double),
                ("z_hi", C.c_double), ("lnhi_lo", C.c_double), ("lnhi_hi", C.c_double), ("histogram", C.c_int32),
                ("moment", C.c_int32), ("lowzcut", C.c_int32), ("p_thresh_sample", C.c_double),
                ("p_switch", C.c_double)]


class BinOutput(C.Structure):
    """gpdla_bin_output"""
    _fields_ = [("pois", _dp), ("mean", _dp), ("var", _dp), ("kept_count", _i32p), ("kept_bin", _i32p),
                ("kept_p", _dp)]


class ModelSpectraRequest(C.Structure):
    """gpdla_model_spectra_request"""
    _fields_ = [("num_selected", C.c_int64), ("selection", _i64p), ("absorber_offsets", _i64p), ("absorber_z", _dp),
                ("absorber_nhi", _dp), ("weights_source", C.c_int32), ("sample_log_likelihoods", _dp),
                ("sub_dla", C.c_int32), ("meanflux", C.c_int32), ("products", C.c_int32), ("capacity", C.c_int64)]


class ModelSpectra(C.Structure):
    """gpdla_model_spectra"""
    _fields_ = [("offsets", _i64p), ("map_absorption", _dp), ("mean_absorption", _dp), ("var_absorption", _dp),
                ("continuum", _dp), ("model_flux", _dp), ("status", _i32p)]


class ModelSpectraMultiRequest(C.Structure):
    """gpdla_model_spectra_multi_request"""
    _fields_ = [("num_selected", C.c_int64), ("selection", _i64p), ("max_dlas", C.c_int32), ("first_model", C.c_int32),
                ("last_model", C.c_int32), ("tables_source", C.c_int32), ("sample_log_likelihoods_dla", _dp),
                ("base_sample_inds", _u32p), ("sample_log_likelihoods_lls", _dp), ("model_weights", _dp),
                ("meanflux", C.c_int32), ("products", C.c_int32), ("capacity", C.c_int64)]


class ModelSpectraMulti(C.Structure):
    """gpdla_model_spectra_multi"""
    _fields_ = [("offsets", _i64p), ("mean_absorption_models", _dp), ("var_absorption_models", _dp),
                ("mean_absorption_lls", _dp), ("var_absorption_lls", _dp), ("expected_absorption", _dp),
                ("expected_var_absorption", _dp), ("status", _i32p), ("model_flags", _u32p)]


class MarginalContinuumRequest(C.Structure):
    """gpdla_marginal_continuum_request"""
    _fields_ = [("num_selected", C.c_int64), ("selection", _i64p), ("weights_source", C.c_int32),
                ("sample_log_likelihoods_dla", _dp), ("sample_log_likelihoods_lls", _dp), ("model_weights", _dp),
                ("meanflux", C.c_int32), ("sample_coefficients", C.c_int32), ("capacity", C.c_int64)]


class MarginalContinuum(C.Structure):
    """gpdla_marginal_continuum"""
    _fields_ = [("offsets", _i64p), ("continuum_mean", _dp), ("continuum_var", _dp), ("continuum_var_between", _dp),
                ("coef_mean", _dp), ("coef_cov_within", _dp), ("coef_cov_between", _dp), ("sample_coefficients", _dp),
                ("status", _i32p)]


class PredictiveFluxRequest(C.Structure):
    """gpdla_predictive_flux_request"""
    _fields_ = [("num_selected", C.c_int64), ("selection", _i64p), ("weights_source", C.c_int32),
                ("sample_log_likelihoods_dla", _dp), ("sample_log_likelihoods_lls", _dp), ("model_weights", _dp),
                ("meanflux", C.c_int32), ("capacity", C.c_int64)]


class PredictiveFlux(C.Structure):
    """gpdla_predictive_flux"""
    _fields_ = [("offsets", _i64p), ("flux_mean", _dp), ("flux_var", _dp), ("flux_var_within", _dp),
                ("flux_var_between", _dp), ("noise_var", _dp), ("status", _i32p)]


class MarginalContinuumMultiRequest(C.Structure):
    """gpdla_marginal_continuum_multi_request"""
    _fields_ = [("num_selected", C.c_int64), ("selection", _i64p), ("max_dlas", C.c_int32), ("tables_source", C.c_int32),
                ("sample_log_likelihoods_dla", _dp), ("base_sample_inds", _u32p), ("sample_log_likelihoods_lls", _dp),
                ("model_weights", _dp), ("meanflux", C.c_int32), ("capacity", C.c_int64)]


class MarginalContinuumMulti(C.Structure):
    """gpdla_marginal_continuum_multi"""
    _fields_ = [("offsets", _i64p), ("continuum_mean", _dp), ("continuum_var", _dp), ("continuum_var_between", _dp),
                ("coef_mean", _dp), ("coef_cov_within", _dp), ("coef_cov_between", _dp), ("status", _i32p),
                ("model_flags", _u32p)]


class PredictiveFluxMultiRequest(C.Structure):
    """gpdla_predictive_flux_multi_request"""
    _fields_ = list(MarginalContinuumMultiRequest._fields_)


class PredictiveFluxMulti(C.Structure):
    """gpdla_predictive_flux_multi"""
    _fields_ = [("offsets", _i64p), ("flux_mean", _dp), ("flux_var", _dp), ("flux_var_within", _dp),
                ("flux_var_between", _dp), ("noise_var", _dp), ("status", _i32p), ("model_flags", _u32p)]


_DISTRIBUTION_FIELDS = [("num_thresholds", C.c_int32), ("thresholds", _dp), ("num_bins", C.c_int32), ("num_levels", C.c_int32),
                        ("levels", _dp)]
_DISTRIBUTION_ARRAYS = [("prob_below", _dp), ("absorption_min", _dp), ("absorption_max", _dp), ("histogram", _dp), ("quantiles", _dp)]
DISTRIBUTION_MAX_THRESHOLDS, DISTRIBUTION_MAX_LEVELS, DISTRIBUTION_MIN_BINS, DISTRIBUTION_MAX_BINS = 4, 8, 8, 256


class AbsorptionDistributionRequest(C.Structure):
    """gpdla_absorption_distribution_request"""
    _fields_ = list(PredictiveFluxRequest._fields_) + _DISTRIBUTION_FIELDS


class AbsorptionDistribution(C.Structure):
    """gpdla_absorption_distribution"""
    _fields_ = [("offsets", _i64p)] + _DISTRIBUTION_ARRAYS + [("status", _i32p)]


class AbsorptionDistributionMultiRequest(C.Structure):
    """gpdla_absorption_distribution_multi_request"""
    _fields_ = list(MarginalContinuumMultiRequest._fields_) + _DISTRIBUTION_FIELDS


class AbsorptionDistributionMulti(C.Structure):
    """gpdla_absorption_distribution_multi"""
    _fields_ = [("offsets", _i64p)] + _DISTRIBUTION_ARRAYS + [("status", _i32p), ("model_flags", _u32p)]


class MockRequest(C.Structure):
    """gpdla_mock_request"""
    _fields_ = [("seed", C.c_uint64), ("absorber_offsets", _i64p), ("absorber_z", _dp), ("absorber_nhi", _dp),
                ("meanflux", C.c_int32), ("write_resident", C.c_int32), ("capacity_stored", C.c_int64),
                ("capacity_grid", C.c_int64)]


class MockSpectra(C.Structure):
    """gpdla_mock_spectra"""
    _fields_ = [("flux", _dp), ("grid_offsets", _i64p), ("absorption", _dp), ("continuum", _dp), ("sigma", _dp),
                ("latents", _dp), ("status", _i32p)]


class NhiPrior(C.Structure):
    """gpdla_nhi_prior"""
    _fields_ = [("coeff", C.c_double * 3), ("centre", C.c_double), ("alpha", C.c_double), ("uniform_min", C.c_double),
                ("uniform_max", C.c_double), ("lower", C.c_double), ("flat_below", C.c_double), ("Z", C.c_double)]


class SampleDraw(C.Structure):
    """gpdla_sample_draw"""
    _fields_ = [("offset", _dp), ("log_nhi", _dp), ("nhi", _dp), ("lls_offset", _dp), ("lls_log_nhi", _dp),
                ("lls_nhi", _dp)]


class PreloadConfig(C.Structure):
    """gpdla_preload_config"""
    _fields_ = [("loading_min_lambda", C.c_double), ("loading_max_lambda", C.c_double),
                ("normalization_min_lambda", C.c_double), ("normalization_max_lambda", C.c_double),
                ("min_lambda", C.c_double), ("max_lambda", C.c_double), ("min_num_pixels", C.c_int64)]


class SummaryRequest(C.Structure):
    """gpdla_summary_request"""
    _fields_ = [("num_models", C.c_int32), ("num_probabilities", C.c_int32), ("probabilities", C.c_double * 8),
                ("num_thresholds", C.c_int32), ("thresholds", C.c_double * 4)]


class ParameterSummaries(C.Structure):
    """gpdla_parameter_summaries"""
    _fields_ = [("mean_z", _dp), ("std_z", _dp), ("mean_log_nhi", _dp), ("std_log_nhi", _dp), ("cov", _dp),
                ("quantiles_z", _dp), ("quantiles_log_nhi", _dp), ("exceedance", _dp), ("effective_samples", _dp),
                ("status", _i32p)]


class RefineRequest(C.Structure):
    """gpdla_refine_request"""
    _fields_ = [("levels", C.c_int32), ("delta", C.c_double), ("pad", C.c_double)]


class RefinedResults(C.Structure):
    """gpdla_refined_results"""
    _fields_ = [("levels", C.c_int32), ("num_points", C.c_int64)] + [(n, _dp) for n in ("boxes", "sample_log_likelihoods_refined", "sample_log_posteriors_refined",
                                   "log_likelihoods_dla_refined", "log_posteriors_dla_refined", "MAP_z_dlas_refined",
                                   "MAP_log_nhis_refined", "MAP_inds_refined")] + [("status", _i32p)]


class RefinedPosteriors(C.Structure):
    """gpdla_refined_posteriors"""
    _fields_ = [("model_posteriors_refined", _dp), ("p_no_dlas_refined", _dp), ("p_dlas_refined", _dp), ("refined", _i32p)]


class PosteriorMapsRequest(C.Structure):
    """gpdla_posterior_maps_request"""
    _fields_ = [("num_models", C.c_int32), ("nz", C.c_int32), ("nn", C.c_int32), ("num_levels", C.c_int32),
                ("levels", C.c_double * 8), ("mix", C.c_int32)]


class PosteriorMaps(C.Structure):
    """gpdla_posterior_maps"""
    _fields_ = [("mass", _dp), ("hpd_level", _dp), ("outside", _dp), ("mode", _i32p), ("hpd_cells", _i32p),
                ("hpd_threshold", _dp), ("intensity", _dp), ("expected_absorbers", _dp), ("status", _i32p)]


MAPS_MAX_SIDE, MAPS_MAX_LEVELS = 64, 8                                                  # GPDLA_MAPS_MAX_*
MAPS_UNUSABLE, MAPS_BAD_GRID, MAPS_SHORT, MAPS_BAD_WEIGHTS = 1, 4, 8, 16                # status bits
REFINE_MAX_LEVELS, REFINE_UNUSABLE, REFINE_NOT_REFINED = 4, 1, -1   # GPDLA_REFINE_*
POSTERIOR_MAX_MODELS, POSTERIOR_MAX_PROBABILITIES, POSTERIOR_MAX_THRESHOLDS = 4, 8, 4   # GPDLA_POSTERIOR_MAX_*
POSTERIOR_UNUSABLE, POSTERIOR_NAN_RANGE = 1, 2                                          # status bits
SPECTRA_MAX_ABSORBERS = 8                                   # GPDLA_SPECTRA_MAX_ABSORBERS
MAX_FIXED_ABSORBERS = 8                                     # GPDLA_MAX_FIXED_ABSORBERS
SPECTRA_MAP, SPECTRA_MOMENTS, SPECTRA_CONTINUUM = 1, 2, 4   # GPDLA_SPECTRA_* product bits
SPECTRA_WEIGHTS_NONE, SPECTRA_WEIGHTS_RESIDENT, SPECTRA_WEIGHTS_HOST = 0, 1, 2
SPECTRA_WEIGHTS_REFINED, SPECTRA_NOT_REFINED = 3, 16        # GPDLA_SPECTRA_WEIGHTS_REFINED; the status bit GPDLA_SPECTRA_NOT_REFINED
SPECTRA_MULTI_MODELS, SPECTRA_MULTI_AVERAGE = 1, 2            # GPDLA_SPECTRA_MULTI_* product bits
SPECTRA_AVERAGE_UNDEFINED, SPECTRA_MULTI_FLAG_LLS = 8, 0x40000000   # status bit; model_flags bit of the sub-DLA model


def ptr(a):
    """double* of a C-contiguous float64 array."""
    return a.ctypes.data_as(_dp)


SUMMARY_COLS = 15  # GPDLA_SUMMARY_COLS


def summary_cols_multi(max_dlas: int) -> int:
    """GPDLA_SUMMARY_COLS_MULTI"""
    return 14 + 4 * max_dlas + 3 * max_dlas * max_dlas


#: every symbol include/gpdla.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("gpdla_abi_version", C.c_int, []),
    ("gpdla_last_error", C.c_char_p, []),
    ("gpdla_voigt", C.c_int, [_dp, C.c_int64, C.c_double, C.c_double, C.c_int, _dp, C.c_int]),
    ("gpdla_log_mvnpdf_low_rank", C.c_int, [_dp, _dp, _dp, _dp, C.c_int64, C.c_int, _dp, C.c_int]),
    ("gpdla_default_config", None, [C.POINTER(Config)]),
    ("gpdla_process_batch", C.c_int, [C.POINTER(Model), C.POINTER(Samples), C.POINTER(Spectra),
                                      C.POINTER(Config), C.POINTER(Results), C.c_int]),
    ("gpdla_process_cells", C.c_int, [C.POINTER(Model), C.POINTER(Samples), C.POINTER(SpectraCells),
                                      C.POINTER(Config), C.POINTER(Results), C.c_int]),
    ("gpdla_process_cells_multi", C.c_int, [C.POINTER(Model), C.POINTER(Samples), C.POINTER(SpectraCells),
                                            _u32p, C.POINTER(Config), C.POINTER(ResultsMulti), C.c_int]),
    ("gpdla_default_batch_quasars", C.c_int64, [C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int]),
    ("gpdla_context_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    ("gpdla_context_destroy", None, [C.c_void_p]),
    ("gpdla_context_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("gpdla_context_set_model", C.c_int, [C.c_void_p, C.POINTER(Model)]),
    ("gpdla_context_set_samples", C.c_int, [C.c_void_p, C.POINTER(Samples)]),
    ("gpdla_context_set_config", C.c_int, [C.c_void_p, C.POINTER(Config)]),
    ("gpdla_context_set_first_quasar_index", C.c_int, [C.c_void_p, C.c_int64]),
    ("gpdla_context_synchronize", C.c_int, [C.c_void_p]),
    ("gpdla_batch_upload", C.c_int, [C.c_void_p, C.POINTER(Spectra), C.POINTER(C.c_void_p)]),
    ("gpdla_batch_reload", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Spectra)]),
    ("gpdla_batch_destroy", None, [C.c_void_p]),
    ("gpdla_batch_process", C.c_int, [C.c_void_p, C.c_void_p]),
    ("gpdla_batch_download", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(Results)]),
    ("gpdla_batch_summary_device_ptr", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _i64p]),
    ("gpdla_batch_samples_device_ptr", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _i64p, _i64p]),
    ("gpdla_context_last_sweep_ms", C.c_double, [C.c_void_p]),
    ("gpdla_context_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("gpdla_process_batch_multi", C.c_int, [C.POINTER(Model), C.POINTER(Samples), C.POINTER(Spectra),
                                            _u32p, C.POINTER(Config), C.POINTER(ResultsMulti), C.c_int]),
    ("gpdla_batch_process_multi", C.c_int, [C.c_void_p, C.c_void_p, _u32p]),
    ("gpdla_batch_download_multi", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ResultsMulti)]),
    ("gpdla_batch_summary_multi_device_ptr", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _i64p, _i32p]),
    ("gpdla_batch_samples_multi_device_ptr", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p),
                                                       C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("gpdla_training_create", C.c_int, [C.c_int, C.c_int64, C.c_int64, _dp, _dp, _dp,
                                        C.POINTER(C.c_void_p)]),
    ("gpdla_training_objective", C.c_int, [C.c_void_p, _dp, C.c_int, _dp, _dp]),
    ("gpdla_training_set_lyseries", C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    ("gpdla_training_destroy", None, [C.c_void_p]),
    ("gpdla_training_create_from_spectra", C.c_int, [C.c_int, C.POINTER(Spectra), C.POINTER(LearnConfig),
                                                     C.POINTER(C.c_void_p)]),
    ("gpdla_training_column_stats", C.c_int, [C.c_void_p, _dp, _dp, _i64p]),
    ("gpdla_training_pca_covariance", C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _i64p]),
    ("gpdla_training_download", C.c_int, [C.c_void_p, _dp, _dp, _dp]),
    ("gpdla_stats_bin_posteriors", C.c_int, [C.c_int64, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                             C.c_int, C.POINTER(BinRequest), C.POINTER(BinOutput), C.c_int]),
    ("gpdla_stats_bin_posteriors_boxed", C.c_int, [C.c_int64, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp,
                                                   C.c_int, C.POINTER(BinRequest), C.POINTER(BinOutput), _dp, C.c_int]),
    ("gpdla_debug_time_bin_kernels", None, [C.c_int]),
    ("gpdla_debug_last_bin_ms", C.c_double, []),
    ("gpdla_stats_poisson_binomial_cf", C.c_int, [C.c_int64, _i64p, _dp, _dp, _dp, C.c_int]),
    ("gpdla_stats_sightline_snrs", C.c_int, [C.c_int64, _i64p, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int]),
    ("gpdla_stats_path_lengths", C.c_int, [C.c_int64, _dp, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_double, _dp,
                                           C.c_int]),
    ("gpdla_stats_bootstrap_sums", C.c_int, [C.c_int64, C.c_int, _dp, _i32p, C.c_uint64, C.c_int64, C.c_int64, _dp,
                                             C.c_int]),
    ("gpdla_model_spectra_validate", C.c_int, [C.POINTER(ModelSpectraRequest), C.c_int64, C.c_int64, C.c_int]),
    ("gpdla_batch_unmasked_counts", C.c_int, [C.c_void_p, C.c_void_p, _i64p]),
    ("gpdla_batch_model_spectra", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ModelSpectraRequest),
                                            C.POINTER(ModelSpectra)]),
    ("gpdla_model_spectra_multi_validate", C.c_int, [C.POINTER(ModelSpectraMultiRequest), C.c_int64, C.c_int64, C.c_int,
                                                     C.c_int, C.c_int]),
    ("gpdla_batch_model_spectra_multi", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ModelSpectraMultiRequest),
                                                  C.POINTER(ModelSpectraMulti)]),
    ("gpdla_marginal_continuum_validate", C.c_int, [C.POINTER(MarginalContinuumRequest), C.c_int64, C.c_int64, C.c_int]),
    ("gpdla_batch_marginal_continuum", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MarginalContinuumRequest),
                                                 C.POINTER(MarginalContinuum)]),
    ("gpdla_predictive_flux_validate", C.c_int, [C.POINTER(PredictiveFluxRequest), C.c_int64, C.c_int64, C.c_int]),
    ("gpdla_marginal_continuum_multi_validate", C.c_int, [C.POINTER(MarginalContinuumMultiRequest), C.c_int64, C.c_int64, C.c_int,
                                                          C.c_int, C.c_int]),
    ("gpdla_batch_marginal_continuum_multi", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MarginalContinuumMultiRequest),
                                                       C.POINTER(MarginalContinuumMulti)]),
    ("gpdla_predictive_flux_multi_validate", C.c_int, [C.POINTER(PredictiveFluxMultiRequest), C.c_int64, C.c_int64, C.c_int,
                                                       C.c_int, C.c_int]),
    ("gpdla_batch_predictive_flux_multi", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PredictiveFluxMultiRequest),
                                                    C.POINTER(PredictiveFluxMulti)]),
    ("gpdla_batch_predictive_flux", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PredictiveFluxRequest),
                                              C.POINTER(PredictiveFlux)]),
    ("gpdla_absorption_distribution_validate", C.c_int, [C.POINTER(AbsorptionDistributionRequest), C.c_int64, C.c_int64, C.c_int]),
    ("gpdla_batch_absorption_distribution", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AbsorptionDistributionRequest),
                                                      C.POINTER(AbsorptionDistribution)]),
    ("gpdla_absorption_distribution_multi_validate", C.c_int, [C.POINTER(AbsorptionDistributionMultiRequest), C.c_int64, C.c_int64,
                                                               C.c_int, C.c_int, C.c_int]),
    ("gpdla_batch_absorption_distribution_multi", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AbsorptionDistributionMultiRequest),
                                                            C.POINTER(AbsorptionDistributionMulti)]),
    ("gpdla_debug_profiles_ms", C.c_int, [C.c_void_p, C.c_void_p, _dp]),
    ("gpdla_model_mean", C.c_int, [C.POINTER(Model), C.c_int64, _dp, _i64p, _dp, _dp, C.c_int, C.c_int, C.c_int,
                                   C.c_double, C.c_double, _dp, C.c_int]),
    ("gpdla_mock_validate", C.c_int, [C.POINTER(MockRequest), C.c_int64]),
    ("gpdla_batch_draw_mocks", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(MockRequest), C.POINTER(MockSpectra)]),
    ("gpdla_samples_kde", C.c_int, [C.c_int64, _dp, C.c_int64, _dp, C.c_double, _dp, _dp, C.c_int]),
    ("gpdla_samples_fit_prior", C.c_int, [C.c_int64, _dp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_double, C.c_double, C.c_double, C.POINTER(NhiPrior), C.c_int]),
    ("gpdla_samples_prior_eval", C.c_int, [C.POINTER(NhiPrior), C.c_int64, _dp, _dp, _dp, C.c_int]),
    ("gpdla_samples_halton", C.c_int, [C.c_int64, C.c_int64, C.c_int, _i32p, _dp, C.c_int]),
    ("gpdla_samples_draw", C.c_int, [C.POINTER(NhiPrior), C.c_int64, C.c_int64, _dp, C.c_int, C.c_double, C.c_double,
                                     C.POINTER(SampleDraw), C.c_int]),
    ("gpdla_preload_spectra", C.c_int, [C.c_int64, _i64p, _f32p, _f32p, _f32p, _i32p, _dp, _u8p, C.POINTER(PreloadConfig),
                                        _i64p, _dp, _dp, _dp, _u8p, _dp, C.c_int]),
    ("gpdla_stats_parameter_summaries", C.c_int, [C.c_int64, C.c_int64, _dp, C.c_int64, _u32p, _dp, _dp, _dp, _dp,
                                                  C.POINTER(SummaryRequest), C.POINTER(ParameterSummaries), C.c_int]),
    ("gpdla_batch_parameter_summaries", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _i64p, C.c_int64,
                                                  C.POINTER(SummaryRequest), C.POINTER(ParameterSummaries)]),
    ("gpdla_debug_last_summaries_ms", C.c_double, []),
    ("gpdla_refine_validate", C.c_int, [C.POINTER(RefineRequest), C.POINTER(NhiPrior), C.c_int64, _dp, _dp]),
    ("gpdla_context_set_refine_points", C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    ("gpdla_batch_refine", C.c_int, [C.c_void_p, C.c_void_p, _i64p, C.c_int64, C.POINTER(RefineRequest),
                                     C.POINTER(NhiPrior)]),
    ("gpdla_batch_download_refined", C.c_int, [C.c_void_p, C.c_void_p, _i64p, C.c_int64, C.POINTER(RefinedResults)]),
    ("gpdla_batch_refined_summaries", C.c_int, [C.c_void_p, C.c_void_p, _i64p, C.c_int64, C.POINTER(SummaryRequest),
                                                C.POINTER(ParameterSummaries)]),
    ("gpdla_batch_refined_posteriors", C.c_int, [C.c_void_p, C.c_void_p, _i64p, C.c_int64, C.POINTER(RefinedPosteriors)]),
    ("gpdla_debug_last_refine_ms", C.c_double, []),
    ("gpdla_fixed_absorbers_validate", C.c_int, [C.c_int64, _i64p, _dp, _dp, C.c_double]),
    ("gpdla_batch_set_fixed_absorbers", C.c_int, [C.c_void_p, C.c_void_p, _i64p, _dp, _dp, C.c_double, C.c_int32]),
    ("gpdla_batch_clear_fixed_absorbers", C.c_int, [C.c_void_p, C.c_void_p]),
    ("gpdla_debug_conditioned_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, _dp, _dp, C.c_int64, _i64p]),
    ("gpdla_stats_posterior_maps", C.c_int, [C.c_int64, C.c_int64, _dp, C.c_int64, _u32p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                             _dp, C.POINTER(PosteriorMapsRequest), C.POINTER(PosteriorMaps), C.c_int]),
    ("gpdla_batch_posterior_maps", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _i64p, C.c_int64, _dp, _dp, _dp, _dp,
                                             _dp, C.POINTER(PosteriorMapsRequest), C.POINTER(PosteriorMaps)]),
    ("gpdla_batch_refined_posterior_maps", C.c_int, [C.c_void_p, C.c_void_p, _i64p, C.c_int64, _dp, _dp, _dp, _dp, _dp,
                                                     C.POINTER(PosteriorMapsRequest), C.POINTER(PosteriorMaps)]),
    ("gpdla_posterior_maps_rows_per_launch", C.c_int64, [C.c_int, C.c_int, C.c_int]),
    ("gpdla_debug_last_maps_ms", C.c_double, [C.c_int]),
    ("gpdla_debug_last_maps_launches", C.c_int64, []),
    ("gpdla_debug_near_poly", C.c_int, [C.c_int, C.c_double, _dp, _dp]),
    ("gpdla_debug_prepared_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, _dp, C.c_int64, _i64p]),
    ("gpdla_debug_philox4x32_10", None, [_u32p, _u32p, _u32p]),
    ("gpdla_debug_throw", C.c_int, [C.c_int]),
    ("gpdla_debug_slim_sweep_blocks_per_cu", C.c_int, [C.c_int, C.POINTER(C.c_int)]),
]

_lib = None


def host_sources() -> list:
    """The host side of the library: csrc/gpdla.hip, the one translation unit, and the host_*.hpp
    headers it includes (one per subsystem), in the order it includes them."""
    import re
    unit = os.path.join(CSRC, "gpdla.hip")
    with open(unit) as f:
        names = re.findall(r'^#include "(host_\w+\.hpp)"', f.read(), flags=re.M)
    return [unit] + [os.path.join(CSRC, n) for n in names]


def _build(out: str, extra_flags, force: bool, verbose: bool) -> str:
    """hipcc of csrc/gpdla.hip into `out`, unless `out` is newer than every source."""
    import glob
    srcs = (host_sources() + glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp"))
            + glob.glob(os.path.join(_HERE, "..", "include", "*.h")))
    if not force and os.path.exists(out):
        if all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
            return out
    cmd = ["hipcc", *HIPCC_FLAGS, *extra_flags, os.path.join(CSRC, "gpdla.hip"), "-o", out]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode:
        print(res.stdout, res.stderr)
    if res.returncode:
        raise RuntimeError(f"hipcc failed building {os.path.basename(out)}:\n" + res.stderr)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile csrc/gpdla.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    return _build(DEFAULT_LIB_PATH, [], force, verbose)


def build_legacy(force: bool = False, verbose: bool = False) -> str:
    """Compile libgpdla_legacy.so: csrc/gpdla.hip with -DGPDLA_WITH_LEGACY, which turns the hooks of
    csrc/host_legacy.hpp on: the pre-expanded-record sweeps behind GPDLA_EXPANDED_RECORDS, the
    GPDLA_MC_SCRATCH_BYTES budget of the launch-group tests, and the round-1 training kernel behind
    GPDLA_TRAIN_LEGACY."""
    return _build(LEGACY_LIB_PATH, ["-DGPDLA_WITH_LEGACY"], force, verbose)


def _preload_hip_runtime():
    """Put ONE HIP runtime in the global symbol scope before libgpdla.so is opened: the copy
    PyTorch-ROCm bundles when torch is installed (so torch streams/tensors and this library share
    a runtime), else the system ROCm one."""
    candidates = []
    try:
        import torch
        candidates.append(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    except Exception:  # torch is optional for the C-ABI itself
        pass
    candidates += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    last = None
    for path in candidates:
        if os.path.isabs(path) and not os.path.exists(path):
            continue
        try:
            return C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError as e:  # try the next candidate
            last = e
    raise OSError(f"no HIP runtime (libamdhip64.so) could be loaded: {last}")


def load():
    """dlopen libgpdla.so and type every declared symbol.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`. "
            "gp_dla_detection_amd has no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(path)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise GpdlaError(rc, load().gpdla_last_error().decode())
