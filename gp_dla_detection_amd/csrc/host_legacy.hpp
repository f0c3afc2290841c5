// host_legacy.hpp -- everything that only libgpdla_legacy.so has.  Superseded kernels and the
// environment switches that select them live in that SECOND library: the same translation unit
// built with -DGPDLA_WITH_LEGACY (gp_dla_detection_amd/_lib.py: build_legacy), loaded through
// GPDLA_LIB_PATH by tests/test_gpu_record_classes.py, the launch-group tests and tools/check_training_legacy.py.
// The product library reads no environment variable: no stray variable can select a slower kernel,
// and the superseded kernels (superseded_kernels.hpp) are not in its code object.
//   GPDLA_EXPANDED_RECORDS  the sweeps on pre-expanded records (k_sweep / k_sweep_split / k_sweep_multi*)
//   GPDLA_MC_SCRATCH_BYTES  the scratch budget that cuts a selection into launch groups (host_grid.hpp)
//   GPDLA_TRAIN_LEGACY      the round-1 training kernel (one block per slot of quasars, training_kernels.hpp): its
//                           three kernels are not templates, so they stand in the product code object as well
// The product functions reach this file through the four legacy_* hooks below (declared in host_sweep.hpp and
// host_training.hpp); the product library's versions, at the end, do nothing.
#pragma once

namespace {

#ifdef GPDLA_WITH_LEGACY

RecordClass legacy_record_class(int, RecordClass product) {
  static const bool expanded = std::getenv("GPDLA_EXPANDED_RECORDS") != nullptr;
  return expanded ? kRecExpanded : product;
}

// fp64 on pre-expanded records.  k <= 20: the compact class of k_sweep; 20 < k <= 40: the same tiles
// split over the 4 waves of a sample group, all four sharing the Voigt / weight pipeline (k_sweep_split)
template <int KMAX>
int legacy_sweep(gpdla_context *c, gpdla_batch *b, const SweepArgs &args) {
  const bool three = args.num_lines == 3;
  if constexpr (KMAX == 20) {
    return three ? launch_sweep_expanded<double, 8, 14, 1, 8, 13, 3>(c, b, args) : launch_sweep_expanded<double, 8, 14, 1, 4, 13, 0>(c, b, args);
  } else {
    const size_t lds = std::max(sweep_split_lds_doubles(three ? 0 : args.num_lines), kExpTab + kSplitEpilogueDoubles) * sizeof(double);
    if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "split sweep needs %zu B of LDS", lds);
    return launch_sweep_kernel(c, three ? &k_sweep_split<3> : &k_sweep_split<0>, 512, lds, 2 * kSamplesPerWave, b->nq, args);
  }
}

// The multi-DLA passes on pre-expanded records: k_sweep_multi (k <= 20) or k_sweep_multi_split
// (20 < k <= 40: the roles of a sample group share the gathers and weights)
template <class Args>
int legacy_sweep_multi(gpdla_context *c, gpdla_batch *b, const Args &args) {
  if (b->k > 20) {
    const size_t lds = std::max(sweep_multi_split_lds_doubles(), kSplitEpilogueDoubles) * sizeof(double);
    if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "multi split sweep needs %zu B of LDS", lds);
    return dispatch_nd(args.mode, [&](auto nd) {
      return launch_sweep_kernel(c, &k_sweep_multi_split<decltype(nd)::value>, 512, lds, 2 * kSamplesPerWave, args.nq_sub, args);
    });
  }
  constexpr int NTW = 14, CH = 8, TW = 13;
  const size_t RD = (size_t)record_doubles(b->ntiles, 0);
  // stage buffers during the loop; the epilogue reuses the array for its factorisation rows
  const size_t lds = std::max(2 * (size_t)CH * RD,
                              (size_t)kSweepWaves * EpilogueShape<TW, 1>::SPP * EpilogueShape<TW, 1>::stride(logical_tiles(b->ntiles))) * sizeof(double);
  if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "multi sweep needs %zu B of LDS", lds);
  return dispatch_nd(args.mode, [&](auto nd) {
    return launch_sweep_kernel(c, &k_sweep_multi<NTW, 1, CH, TW, decltype(nd)::value>, 512, lds, kSweepWaves * kSamplesPerWave, args.nq_sub, args);
  });
}

// GPDLA_TRAIN_LEGACY (diagnostic cross-check): one block per slot of quasars, each slot adding into
// its own copy of g, slots summed in order -- deterministic too (round 1 used fp64 atomics).  x is in
// the pinned staging buffer as well.
int legacy_objective_round1(gpdla_training *t, const double *x, int k, double *f, double *g) {
  const int64_t G = t->G, nx = G * (k + 1) + 3;
  if (t->lines.nfl > 1) return fail(GPDLA_ERR_UNSUPPORTED, "GPDLA_TRAIN_LEGACY has no Lyman-series objective");
  const int num_slots = (int)std::min<int64_t>(t->nq, 512);
  const int64_t slot_n = nx + 1;  // [g | f]
  if ((int64_t)num_slots * slot_n > t->slots_capacity) {
    dev_free(t->d_slots);
    t->d_slots = nullptr;
    t->slots_capacity = 0;
    int rc = dev_alloc(&t->d_slots, (size_t)num_slots * slot_n);
    if (rc) return rc;
    t->slots_capacity = (int64_t)num_slots * slot_n;
  }
  HIP_TRY(hipMemcpy(t->d_x, t->h_stage, (size_t)nx * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(t->d_slots, 0, (size_t)num_slots * slot_n * sizeof(double)));
  HIP_TRY(hipMemset(t->d_flag, 0, sizeof(int32_t)));
  hipLaunchKernelGGL(k_training_omega2, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, 0,
                     t->d_x + G * k, G, t->d_omega2);
  TrainingArgs a;
  a.nq = t->nq;
  a.G = G;
  a.ld = t->ld;
  a.k = k;
  a.flux = t->d_flux;
  a.lya_1pz = t->d_lya;
  a.noise = t->d_noise;
  a.M = t->d_x;
  a.omega2 = t->d_omega2;
  a.c_0 = std::exp(x[G * (k + 1)]);       // objective.m:30-32
  a.tau_0 = std::exp(x[G * (k + 1) + 1]);
  a.beta = std::exp(x[G * (k + 1) + 2]);
  a.slots = t->d_slots;
  a.not_pd = t->d_flag;
  const size_t lds = training_lds_doubles(G, k) * sizeof(double);
  if (lds > 160 * 1024) return fail(GPDLA_ERR_UNSUPPORTED, "training kernel needs %zu B of LDS", lds);
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_training_loss),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_training_loss, dim3((unsigned)num_slots), dim3(256), lds, 0, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_training_reduce, dim3((unsigned)((slot_n + 255) / 256)), dim3(256), 0, 0, t->d_slots,
                     num_slots, slot_n, t->d_g);
  HIP_TRY(hipGetLastError());
  int32_t flag = 0;
  HIP_TRY(hipMemcpy(g, t->d_g, (size_t)nx * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(f, t->d_g + nx, sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&flag, t->d_flag, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (flag) return fail(GPDLA_ERR_NOT_POSITIVE_DEFINITE, "B = I + M' D^-1 M not positive definite for some quasar");
  // priors of Kim et al. (2007) on tau0 and beta, gradient only (objective.m:59-71)
  const double tau_0_mu = 0.0023, tau_0_sigma = 0.0007, beta_mu = 3.65, beta_sigma = 0.21;
  g[G * (k + 1) + 1] += a.tau_0 * (a.tau_0 - tau_0_mu) / (tau_0_sigma * tau_0_sigma);
  g[G * (k + 1) + 2] += a.beta * (a.beta - beta_mu) / (beta_sigma * beta_sigma);
  return GPDLA_OK;
}

bool legacy_training_objective(gpdla_training *t, const double *x, int k, double *f, double *g, int *rc) {
  static const bool round1 = std::getenv("GPDLA_TRAIN_LEGACY") != nullptr;
  if (round1) *rc = legacy_objective_round1(t, x, k, f, g);
  return round1;
}

#else  // the product library

RecordClass legacy_record_class(int, RecordClass product) { return product; }
template <int KMAX>
int legacy_sweep(gpdla_context *, gpdla_batch *, const SweepArgs &) {
  return fail(GPDLA_ERR_UNSUPPORTED, "the fp64 sweeps on pre-expanded records are in libgpdla_legacy.so only");
}
template <class Args>
int legacy_sweep_multi(gpdla_context *, gpdla_batch *, const Args &) {
  return fail(GPDLA_ERR_UNSUPPORTED, "the multi-DLA sweeps on pre-expanded records are in libgpdla_legacy.so only");
}
bool legacy_training_objective(gpdla_training *, const double *, int, double *, double *, int *) { return false; }

#endif

}  // namespace
