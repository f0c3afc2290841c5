// host_training.hpp -- the training objective (objective.m:12-75, spectrum_loss*.m) on a resident
// training set: the handle, the matrix-core evaluation captured once per k into a graph and replayed.
#pragma once

struct gpdla_training {
  int device_id = 0;
  int64_t nq = 0, G = 0, ld = 0;  // ld: row stride of the training arrays (G rounded up to 16)
  // mean-flux model's objective (gpdla_training_set_lyseries): lines.nfl > 1, d_nl = active lines per pixel
  TrainLines lines{};
  uint8_t *d_nl = nullptr;
  double *d_flux = nullptr, *d_lya = nullptr, *d_noise = nullptr, *d_loglya = nullptr;
  double *d_x = nullptr, *d_g = nullptr, *d_omega2 = nullptr, *d_f = nullptr;
  int32_t *d_flag = nullptr;
  int64_t x_capacity = 0;
  // one-block-per-slot path (GPDLA_TRAIN_LEGACY of libgpdla_legacy.so): per-slot copies of [g | f], summed in order
  double *d_slots = nullptr;
  int64_t slots_capacity = 0;
  // workspace of the matrix-core path (training_mfma_kernels.hpp): its sizes do not depend on k.
  // ws_ready is set only after every allocation, the stream and the kernel attributes succeeded.
  bool ws_ready = false;
  int ws_class = 0;  // rank class the workspace was sized for (20 or 40)
  double *h_stage = nullptr;  // pinned host staging for x (in) and [g | f | flag] (out)
  int64_t stage_capacity = 0;
  // one evaluation = H2D of x, six kernels, D2H of [g | f | flag]: captured once per k into a
  // hipGraph and replayed (no kernel argument changes between evaluations)
  hipStream_t stream = nullptr;
  hipGraphExec_t graph = nullptr;
  int graph_k = 0;
  double *d_wB = nullptr, *d_uB = nullptr, *d_part1 = nullptr;
  double *d_recM = nullptr, *d_recP = nullptr, *d_partB = nullptr, *d_recD = nullptr, *d_recE = nullptr;
  double *d_nlogp = nullptr, *d_partD = nullptr, *d_partcol = nullptr, *d_partsc = nullptr;
  // made by gpdla_training_create_from_spectra (learn_kernels.hpp): d_flux holds rest_fluxes until the
  // first gpdla_training_column_stats centres it in place; d_mu / d_std / d_cnt keep that call's results
  bool from_spectra = false, centered = false;
  double *d_mu = nullptr, *d_std = nullptr, *d_cnt = nullptr;
};

namespace {

// The captured graph holds raw pointers to d_x, d_g, h_stage and the workspace: it is destroyed
// BEFORE any of them is freed or replaced, never after.
void training_drop_graph(gpdla_training *t) {
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  if (t->graph) (void)hipGraphExecDestroy(t->graph);
  t->graph = nullptr;
  t->graph_k = 0;
}

void training_free_workspace(gpdla_training *t) {
  training_drop_graph(t);
  for (double **p : {&t->d_wB, &t->d_uB, &t->d_part1, &t->d_recM, &t->d_recP, &t->d_partB,
                     &t->d_recD, &t->d_recE, &t->d_nlogp, &t->d_partD, &t->d_partcol, &t->d_partsc}) {
    dev_free(*p);
    *p = nullptr;
  }
  if (t->stream) (void)hipStreamDestroy(t->stream);
  t->stream = nullptr;
  t->ws_ready = false;
}

void training_release(gpdla_training *t) {
  (void)hipSetDevice(t->device_id);
  (void)hipDeviceSynchronize();
  training_free_workspace(t);  // graph, then stream, then the buffers the graph pointed at
  for (void *p : {(void *)t->d_flux, (void *)t->d_lya, (void *)t->d_noise, (void *)t->d_x, (void *)t->d_g,
                  (void *)t->d_omega2, (void *)t->d_f, (void *)t->d_flag, (void *)t->d_loglya, (void *)t->d_slots,
                  (void *)t->d_nl, (void *)t->d_mu, (void *)t->d_std, (void *)t->d_cnt})
    dev_free(p);
  if (t->h_stage) (void)hipHostFree(t->h_stage);
  delete t;
}

// A handle with the four [nq][ld] data buffers (not filled) and the small objective buffers; ld = G
// rounded up to 16 pixels: the rows start 128-byte aligned and end in missing pixels (NaN flux,
// 1 + z = 1, unit noise, log(1 + z) = 0), so the matrix-core kernels read whole 16-pixel chunks
// without bounds checks.  The caller has selected the device.
int training_alloc(int device_id, int64_t nq, int64_t G, gpdla_training **out) {
  gpdla_training *t = new gpdla_training();
  t->device_id = device_id;
  t->nq = nq;
  t->G = G;
  t->ld = 16 * ((G + 15) / 16);
  const size_t n = (size_t)nq * t->ld;
  int rc;
  if ((rc = dev_alloc(&t->d_flux, n)) || (rc = dev_alloc(&t->d_lya, n)) || (rc = dev_alloc(&t->d_noise, n)) ||
      (rc = dev_alloc(&t->d_loglya, n)) || (rc = dev_alloc(&t->d_omega2, (size_t)t->ld)) ||
      (rc = dev_alloc(&t->d_f, 1)) || (rc = dev_alloc(&t->d_flag, 1))) {
    training_release(t);
    return rc;
  }
  *out = t;
  return GPDLA_OK;
}

}  // namespace

extern "C" {

void gpdla_training_destroy(gpdla_training *t) {
  if (!t) return;
  training_release(t);
}

int gpdla_training_create(int device_id, int64_t nq, int64_t G, const double *flux, const double *lya,
                          const double *noise, gpdla_training **out) try {
  if (!out || !flux || !lya || !noise) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (nq < 1 || G < 1) return fail(GPDLA_ERR_INVALID_ARGUMENT, "empty training set");
  int rc = select_device(device_id);
  if (rc) return rc;
  gpdla_training *t = nullptr;
  if ((rc = training_alloc(device_id, nq, G, &t))) return rc;
  // MATLAB column-major [nq x G] -> quasar-major [nq][ld]
  const int64_t ld = t->ld;
  const size_t n = (size_t)nq * ld;
  std::vector<double> tmp(n);
  auto up = [&](const double *src, double *dst, double pad, bool take_log) -> int {
    for (int64_t i = 0; i < nq; ++i) {
      for (int64_t p = 0; p < G; ++p) tmp[(size_t)i * ld + p] = take_log ? std::log(src[i + p * nq]) : src[i + p * nq];
      for (int64_t p = G; p < ld; ++p) tmp[(size_t)i * ld + p] = pad;
    }
    HIP_TRY(hipMemcpy(dst, tmp.data(), n * sizeof(double), hipMemcpyHostToDevice));
    return GPDLA_OK;
  };
  if ((rc = up(flux, t->d_flux, std::nan(""), false)) || (rc = up(lya, t->d_lya, 1.0, false)) ||
      (rc = up(noise, t->d_noise, 1.0, false)) ||
      (rc = up(lya, t->d_loglya, 0.0, true))) {  // log(1 + z): data, taken once
    gpdla_training_destroy(t);
    return rc;
  }
  *out = t;
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"

namespace {

// What libgpdla_legacy.so adds to training (host_legacy.hpp; the product library's version does nothing and
// returns false): the round-1 objective in place of the matrix-core one (true: *rc is its result).
bool legacy_training_objective(gpdla_training *t, const double *x, int k, double *f, double *g, int *rc);

TrainDims train_dims(const gpdla_training *t, int k) {
  TrainDims d;
  d.nq = t->nq;
  d.G = t->G;
  d.k = k;
  d.NQ16 = (t->nq + 15) / 16;
  d.PG = (t->G + 15) / 16;
  d.T = 4 * d.PG;
  d.TQ = 4 * d.NQ16;
  d.ld = 16 * d.PG;
  d.H = 6;    // 79 row blocks x 6 = 474 blocks of 4 waves for 5000 quasars (two per CU)
  d.H2 = 24;  // 20 row blocks x 24 = 480
  d.GS = 24;  // 20 pixel blocks x 24 = 480 blocks of 4 waves (59 KiB of LDS each: two per CU)
  if (k > 20) {
    d.GS = 24 * kTrWidePB;  // k_train_core_wide: ceil(77 / PB) pixel-group blocks x GS / 4 = 468 blocks at PB = 2
    // four tile groups make the contraction grids four times larger, so they need fewer splits to fill
    // the chip -- and every split is a copy of the partial sums through HBM (246 MB at H = 6, 242 MB at
    // H2 = 24): 79 x 4 x 3 = 948 and 20 x 4 x 12 = 960 blocks.  Measured at k = 40, two rounds (H,H2):
    // 6,24 -> 1.122 ms; 3,24 -> 1.075; 6,12 -> 1.077; 3,12 -> 1.03; 3,8 / 3,6 the same; 2,x worse.
    d.H = 3;
    d.H2 = 12;
  }
  d.H = (int32_t)std::max<int64_t>(d.H, (d.PG + kTrBuildMaxChunks - 1) / kTrBuildMaxChunks);  // a split's omega2 table fits its LDS
  d.GS = (d.GS + 3) / 4 * 4;  // k_train_core_wide: four splits per block
  return d;
}

// One evaluation of objective.m:12-75 on the matrix cores, enqueued on `st`: H2D of x from the pinned
// staging buffer, the kernels, D2H of [g | f | flag] into it.  KMAX: rank class (20 or 40).
template <int KMAX>
int training_enqueue_mfma(gpdla_training *t, int k, hipStream_t st) {
  using K = TrC<KMAX>;
  const TrainDims d = train_dims(t, k);
  const int64_t strideM = (d.T + kTrChunk) * kTrGroupD, strideD = (d.TQ + kTrChunk) * kTrGroupD;
  const int64_t G = t->G, nx = G * (k + 1) + 3;
  HIP_TRY(hipMemcpyAsync(t->d_x, t->h_stage, (size_t)nx * sizeof(double), hipMemcpyHostToDevice, st));
  TrainRecordsArgs ra;
  ra.d = d;
  ra.M = t->d_x;
  ra.recM = t->d_recM;
  ra.recP = t->d_recP;
  ra.group_stride = strideM;
  ra.not_pd = t->d_flag;
  ra.omega2 = t->d_omega2;
  hipLaunchKernelGGL(k_train_records<KMAX>, dim3(1024), dim3(256), 0, st, ra);
  TrainBuildArgs ba;  // B_q, t_q: rows = quasars, steps over pixels, w and u made on the fly
  ba.d = d;
  ba.flux = t->d_flux;
  ba.log_lya_1pz = t->d_loglya;
  ba.noise = t->d_noise;
  ba.omega2 = t->d_omega2;
  ba.x = t->d_x;
  ba.nl = t->d_nl;
  ba.lines = t->lines;
  ba.Brec = t->d_recM;
  ba.groups = K::Groups;
  ba.w_tiles = K::W;
  ba.cols = K::Cols;
  ba.group_stride = strideM;
  ba.out = t->d_partB;
  ba.part1 = t->d_part1;
  const bool ly = t->lines.nfl > 1;
  const dim3 build_grid((unsigned)(((d.NQ16 + kTrCWaves - 1) / kTrCWaves) * d.H * K::Groups));
  if (ly) hipLaunchKernelGGL(k_train_build<true>, build_grid, dim3(kTrCWaves * 64), kTrBuildLds, st, ba);
  else hipLaunchKernelGGL(k_train_build<false>, build_grid, dim3(kTrCWaves * 64), kTrBuildLds, st, ba);
  TrainFactorArgs fa;
  fa.d = d;
  fa.partB = t->d_partB;
  fa.part1 = t->d_part1;
  fa.recD = t->d_recD;
  fa.recE = t->d_recE;
  fa.nlogp = t->d_nlogp;
  fa.not_pd = t->d_flag;
  fa.group_stride = strideD;
  // k <= 40: the per-quasar algebra in registers (k_train_factor16); k <= 20 keeps the round-3 kernel
  const dim3 factor_grid((unsigned)((d.NQ16 * 16 + TrF<KMAX>::FQ - 1) / TrF<KMAX>::FQ));
  if constexpr (KMAX == 40) {
    hipLaunchKernelGGL(k_train_factor16<KMAX>, factor_grid, dim3(kTrF16Threads), 0, st, fa);
  } else {
    hipLaunchKernelGGL(k_train_factor<KMAX>, factor_grid, dim3(256), 0, st, fa);
  }
  TrainCoreArgs co;
  co.d = d;
  co.recP = t->d_recP;
  co.recE = t->d_recE;
  co.flux = t->d_flux;
  co.log_lya_1pz = t->d_loglya;
  co.noise = t->d_noise;
  co.x = t->d_x;
  co.nl = t->d_nl;
  co.lines = t->lines;
  co.wB = t->d_wB;
  co.uB = t->d_uB;
  co.partcol = t->d_partcol;
  co.partsc = t->d_partsc;
  const dim3 core_grid((unsigned)(((d.PG + 3) / 4) * d.GS));
  if (KMAX <= 20) {
    if (ly) hipLaunchKernelGGL(k_train_core<true>, core_grid, dim3(256), kTrCoreLds, st, co);
    else hipLaunchKernelGGL(k_train_core<false>, core_grid, dim3(256), kTrCoreLds, st, co);
  } else {
    const dim3 wide_grid((unsigned)(((d.PG + kTrWidePB - 1) / kTrWidePB) * (d.GS / 4)));  // kTrWidePB pixel groups per block, four splits (train_dims keeps GS % 4 == 0)
    if (ly) hipLaunchKernelGGL(k_train_core_wide<true>, wide_grid, dim3(256), 0, st, co);
    else hipLaunchKernelGGL(k_train_core_wide<false>, wide_grid, dim3(256), 0, st, co);
  }
  TrainContractArgs ca;  // dM: rows = pixels, steps over quasars
  ca.Aw = t->d_wB;
  ca.Au = t->d_uB;
  ca.groups = K::Groups;
  ca.w_tiles = K::W;
  ca.cols = K::Cols;
  ca.Brec = t->d_recD;
  ca.R = d.PG;
  ca.steps = d.TQ;
  ca.nsplit = d.H2;
  ca.group_stride = strideD;
  ca.out = t->d_partD;
  hipLaunchKernelGGL(k_train_contract, dim3((unsigned)(((d.PG + kTrCWaves - 1) / kTrCWaves) * d.H2 * K::Groups)), dim3(kTrCWaves * 64), kTrContractLds, st, ca);
  TrainFinishArgs fi;
  fi.d = d;
  fi.M = t->d_x;
  fi.partD = t->d_partD;
  fi.partcol = t->d_partcol;
  fi.partsc = t->d_partsc;
  fi.nlogp = t->d_nlogp;
  fi.f = t->d_g + nx;        // f and the not-PD flag ride behind g: one copy back
  fi.flag_in = t->d_flag;
  fi.flag_out = t->d_g + nx + 1;
  fi.x = t->d_x;
  fi.g = t->d_g;
  hipLaunchKernelGGL(k_train_finish<KMAX>, dim3((unsigned)(G + 1)), dim3(256), 0, st, fi);
  HIP_TRY(hipMemcpyAsync(t->h_stage, t->d_g, (size_t)(nx + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
  return GPDLA_OK;
}

// objective.m:12-75 on the matrix cores: value and gradient, deterministic.  x is in the pinned
// staging buffer on entry; [g | f | flag] is there on return.  The workspace is sized by the rank
// class (k <= 20: one tile group; k <= 40: four) and rebuilt when the class changes.
int training_objective_mfma(gpdla_training *t, int k, double *f, double *g) {
  const TrainDims d = train_dims(t, k);
  const int64_t G = t->G, nx = G * (k + 1) + 3;
  const int kc = k <= 20 ? 20 : 40;
  const int groups = kc == 20 ? TrC<20>::Groups : TrC<40>::Groups, cols = kc == 20 ? TrC<20>::Cols : TrC<40>::Cols,
            ks = kc == 20 ? TrC<20>::Ks : TrC<40>::Ks;
  int rc;
  if (!t->ws_ready || t->ws_class != kc) {
    training_free_workspace(t);  // another class's workspace, or what an earlier, failed attempt left behind
    auto setup = [&]() -> int {
    if ((rc = dev_alloc(&t->d_wB, (size_t)d.PG * d.TQ * 64)) || (rc = dev_alloc(&t->d_uB, (size_t)d.PG * d.TQ * 64)) ||
        (rc = dev_alloc(&t->d_part1, (size_t)d.NQ16 * 16 * d.H * 3)) ||
        (rc = dev_alloc(&t->d_recM, (size_t)groups * (d.T + kTrChunk) * kTrGroupD)) || (rc = dev_alloc(&t->d_recP, (size_t)d.PG * ks * 64)) ||
        (rc = dev_alloc(&t->d_partB, (size_t)d.NQ16 * d.H * 16 * cols)) ||
        (rc = dev_alloc(&t->d_recD, (size_t)groups * (d.TQ + kTrChunk) * kTrGroupD)) || (rc = dev_alloc(&t->d_recE, (size_t)d.NQ16 * ks * 64)) ||
        (rc = dev_alloc(&t->d_nlogp, (size_t)d.NQ16 * 16)) ||
        (rc = dev_alloc(&t->d_partD, (size_t)d.PG * d.H2 * 16 * cols)) ||
        (rc = dev_alloc(&t->d_partcol, (size_t)d.PG * d.GS * 16)) || (rc = dev_alloc(&t->d_partsc, (size_t)d.PG * d.GS * 3)))
      return rc;
    HIP_TRY(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_train_contract),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrContractLds));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_train_build<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrBuildLds));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_train_build<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrBuildLds));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_train_core<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrCoreLds));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_train_core<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrCoreLds));
    return GPDLA_OK;
    };
    if ((rc = setup())) {
      training_free_workspace(t);
      return rc;
    }
    // the chunk padding behind each tile group of recM / recD is read (never used) by the last chunk copy
    HIP_TRY(hipMemset(t->d_recM, 0, (size_t)groups * (d.T + kTrChunk) * kTrGroupD * sizeof(double)));
    HIP_TRY(hipMemset(t->d_recD, 0, (size_t)groups * (d.TQ + kTrChunk) * kTrGroupD * sizeof(double)));
    // the columns of the padding tiles (k <= 40: 9 tiles of the last group) are never written by the contractions
    HIP_TRY(hipMemset(t->d_partB, 0, (size_t)d.NQ16 * d.H * 16 * cols * sizeof(double)));
    HIP_TRY(hipMemset(t->d_partD, 0, (size_t)d.PG * d.H2 * 16 * cols * sizeof(double)));
    t->ws_ready = true;
    t->ws_class = kc;
  }
  if (!t->graph || t->graph_k != k) {  // capture the evaluation once per k
    training_drop_graph(t);
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamBeginCapture(t->stream, hipStreamCaptureModeThreadLocal));
    rc = kc == 20 ? training_enqueue_mfma<20>(t, k, t->stream) : training_enqueue_mfma<40>(t, k, t->stream);
    hipError_t e = hipStreamEndCapture(t->stream, &graph);
    if (rc) {
      if (graph) (void)hipGraphDestroy(graph);
      return rc;
    }
    if (e != hipSuccess) return fail(GPDLA_ERR_HIP, "training graph capture failed: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(&t->graph, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(GPDLA_ERR_HIP, "training graph instantiation failed: %s", hipGetErrorString(e));
    t->graph_k = k;
  }
#ifdef TR_EXP_TIMING
  static double acc_l = 0, acc_s = 0, acc_m = 0, acc_gap = 0;
  static int n_calls = 0;
  static std::chrono::steady_clock::time_point last_end;
  auto c0 = std::chrono::steady_clock::now();
  if (n_calls) acc_gap += std::chrono::duration<double, std::micro>(c0 - last_end).count();
#endif
  HIP_TRY(hipGraphLaunch(t->graph, t->stream));
#ifdef TR_EXP_TIMING
  auto c1 = std::chrono::steady_clock::now();
#endif
  HIP_TRY(hipStreamSynchronize(t->stream));
#ifdef TR_EXP_TIMING
  auto c2 = std::chrono::steady_clock::now();
#endif
  std::memcpy(g, t->h_stage, (size_t)nx * sizeof(double));
#ifdef TR_EXP_TIMING
  auto c3 = std::chrono::steady_clock::now();
  last_end = c3;
  acc_l += std::chrono::duration<double, std::micro>(c1 - c0).count();
  acc_s += std::chrono::duration<double, std::micro>(c2 - c1).count();
  acc_m += std::chrono::duration<double, std::micro>(c3 - c2).count();
  if (++n_calls % 6 == 0) {
    std::fprintf(stderr, "[timing] launch %.1f us, sync %.1f us, memcpy-out %.1f us, between calls (python + memcpy-in) %.1f us\n",
                 acc_l / 6, acc_s / 6, acc_m / 6, acc_gap / 6);
    acc_l = acc_s = acc_m = acc_gap = 0;
  }
#endif
  *f = t->h_stage[nx];
  if (t->h_stage[nx + 1] != 0.0)
    return fail(GPDLA_ERR_NOT_POSITIVE_DEFINITE, "B = I + M' D^-1 M not positive definite for some quasar");
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_training_set_lyseries(gpdla_training *t, int num_forest_lines, const double *all_transition_wavelengths,
                                const double *all_oscillator_strengths) try {
  if (!t) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null training set");
  if (num_forest_lines < 0 || num_forest_lines > kTrMaxLines)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_forest_lines = %d outside [0, %d]", num_forest_lines, kTrMaxLines);
  HIP_TRY(hipSetDevice(t->device_id));
  training_drop_graph(t);  // the captured kernel arguments carry the line table
  TrainLines L{};
  if (num_forest_lines <= 1) {  // back to objective.m / spectrum_loss.m
    t->lines = L;
    return GPDLA_OK;
  }
  const double *wl = all_transition_wavelengths, *fs = all_oscillator_strengths;
  // default: the Lyman series of voigt.c:20-182 (include/gpdla_lyman_series.h) = set_parameters_multi.m:76-143,
  // wavelengths in Angstrom
#define GPDLA_LINE_WL(i, wl_cm, f, rate, lead, width) wl_cm * 1e8,
#define GPDLA_LINE_FS(i, wl_cm, f, rate, lead, width) f,
  static const double wl_default[] = {GPDLA_LYMAN_SERIES(GPDLA_LINE_WL)};
  static const double fs_default[] = {GPDLA_LYMAN_SERIES(GPDLA_LINE_FS)};
#undef GPDLA_LINE_WL
#undef GPDLA_LINE_FS
  static_assert(sizeof wl_default / sizeof wl_default[0] == kTrMaxLines, "31 Lyman lines");
  if (!wl || !fs) {
    wl = wl_default;
    fs = fs_default;
  }
  for (int l = 0; l < num_forest_lines; ++l) {
    if (!(wl[l] > 0.0) || !(fs[l] > 0.0) || (l && !(wl[l] < wl[l - 1])))
      return fail(GPDLA_ERR_INVALID_ARGUMENT, "line %d: wavelengths must be positive and decreasing, strengths positive", l + 1);
    L.coef[l] = wl[l] * fs[l] / (wl[0] * fs[0]);  // spectrum_loss_lyseries.m:34-35
    L.logr[l] = std::log(wl[0] / wl[l]);
  }
  L.nfl = num_forest_lines;
  int rc;
  if (!t->d_nl && (rc = dev_alloc(&t->d_nl, (size_t)t->nq * t->ld))) return rc;
  HIP_TRY(hipMemset(t->d_flag, 0, sizeof(int32_t)));
  TrainLinesArgs la;
  la.nq = t->nq;
  la.G = t->G;
  la.ld = t->ld;
  la.nfl = num_forest_lines;
  for (int l = 0; l < kTrMaxLines; ++l) la.wl[l] = l < num_forest_lines ? wl[l] : 1.0;
  la.lya_1pz = t->d_lya;
  la.nl = t->d_nl;
  la.not_prefix = t->d_flag;
  const int64_t n = t->nq * t->ld;
  hipLaunchKernelGGL(k_train_lines, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, la);
  HIP_TRY(hipGetLastError());
  int32_t bad = 0;
  HIP_TRY(hipMemcpy(&bad, t->d_flag, sizeof bad, hipMemcpyDeviceToHost));
  if (bad) return fail(GPDLA_ERR_UNSUPPORTED, "the active Lyman lines of some pixel are not a prefix of the series");
  t->lines = L;
  return GPDLA_OK;
} GPDLA_NO_THROW

int gpdla_training_objective(gpdla_training *t, const double *x, int k, double *f, double *g) try {
  if (!t || !x || !f || !g) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null argument");
  if (k < 1 || k > GPDLA_MAX_K) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d outside [1, %d]", k, GPDLA_MAX_K);
  HIP_TRY(hipSetDevice(t->device_id));
  const int64_t G = t->G;
  const int64_t nx = G * (k + 1) + 3;
  if (nx > t->x_capacity) {
    training_drop_graph(t);  // it points at the buffers replaced below
    dev_free(t->d_x);
    dev_free(t->d_g);
    t->d_x = t->d_g = nullptr;
    t->x_capacity = 0;
    if (t->h_stage) (void)hipHostFree(t->h_stage);
    t->h_stage = nullptr;
    int rc;
    if ((rc = dev_alloc(&t->d_x, (size_t)nx)) || (rc = dev_alloc(&t->d_g, (size_t)nx + 2))) return rc;
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&t->h_stage), (size_t)(nx + 2) * sizeof(double), hipHostMallocDefault));
    t->x_capacity = nx;
  }
  // The three contractions on the matrix cores, ordered (deterministic) sums, one graph launch per
  // evaluation (k <= 20: one 16-tile group per contraction step; 20 < k <= 40: four).
  std::memcpy(t->h_stage, x, (size_t)nx * sizeof(double));
  int rc;
  if (legacy_training_objective(t, x, k, f, g, &rc)) return rc;
  return training_objective_mfma(t, k, f, g);
} GPDLA_NO_THROW

}  // extern "C"
