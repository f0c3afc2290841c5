// gpdla.hip -- libgpdla.so: the C-ABI of include/gpdla.h over the HIP kernels of the *_kernel(s).hpp
// headers.  No torch types, no CPU compute path: if the device is missing every compute entry point
// fails with GPDLA_ERR_NO_DEVICE.  This file is the one translation unit (g_lines is one __constant__
// object that the sweeps, k_profiles and gpdla_voigt share); the host code lives in the host_*.hpp
// headers below, one per subsystem, included in this order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <stdexcept>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>
#include <type_traits>

#include <sys/mman.h>

#include "../../include/gpdla.h"
#include "../../include/gpdla_lyman_series.h"
#include "prepare_kernels.hpp"
#include "evidence_kernels.hpp"
#include "multi_kernels.hpp"
#include "sweep_expanded_kernel.hpp"
#include "sweep_multi_slim_kernel.hpp"
#include "sweep_slim_kernel.hpp"
#include "sweep_split_slim_kernel.hpp"
#ifdef GPDLA_WITH_LEGACY
#include "superseded_kernels.hpp"
#endif
#include "learn_kernels.hpp"
#include "stats_kernels.hpp"
#include "spectra_kernels.hpp"
#include "spectra_multi_kernels.hpp"
#include "marginal_continuum_kernels.hpp"
#include "predictive_flux_kernels.hpp"
#include "absorption_distribution_kernels.hpp"
#include "mock_kernels.hpp"
#include "sample_kernels.hpp"
#include "preload_kernels.hpp"
#include "posterior_kernels.hpp"
#include "posterior_maps_kernels.hpp"
#include "refine_kernels.hpp"
#include "condition_kernels.hpp"
#include "training_kernels.hpp"
#include "training_mfma_kernels.hpp"

using namespace gpdla;

#include "host_common.hpp"
#include "host_context.hpp"
#include "host_sweep.hpp"
#include "host_multi.hpp"
#include "host_consumers.hpp"
#include "host_grid.hpp"
#include "host_pipeline.hpp"
#include "host_training.hpp"
#include "host_learn.hpp"
#include "host_stats.hpp"
#include "host_spectra.hpp"
#include "host_spectra_multi.hpp"
#include "host_marginal_continuum.hpp"
#include "host_predictive_flux.hpp"
#include "host_mixture_multi.hpp"
#include "host_absorption_distribution.hpp"
#include "host_mock.hpp"
#include "host_samples.hpp"
#include "host_preload.hpp"
#include "host_posterior.hpp"
#include "host_refine.hpp"
#include "host_condition.hpp"
#include "host_posterior_maps.hpp"
// libgpdla_legacy.so (-DGPDLA_WITH_LEGACY): the superseded kernels and their environment switches
#include "host_legacy.hpp"
