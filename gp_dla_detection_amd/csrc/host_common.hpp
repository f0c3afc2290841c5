// host_common.hpp -- what every host subsystem of libgpdla uses: the thread's error message, the
// handlers that keep C++ exceptions inside the library, device selection, the Lyman-series tables
// in __constant__ memory, device allocation helpers.  Part of the one translation unit gpdla.hip.
#pragma once

namespace {

thread_local std::string t_error = "";

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  t_error = buf;
  return code;
}

// No C++ exception leaves the library: one that reaches an extern "C" frame ends the host process
// (MATLAB through a MEX gateway, Python through ctypes).  Every int-returning entry point is a
// function-try-block closed by this: std::bad_alloc / std::length_error of a host container and
// anything else unexpected become GPDLA_ERR_HOST with a message.
#define GPDLA_NO_THROW                                                                                    \
  catch (const std::bad_alloc &) { return fail(GPDLA_ERR_HOST, "out of host memory"); }                   \
  catch (const std::exception &e) { return fail(GPDLA_ERR_HOST, "unexpected C++ exception: %s", e.what()); } \
  catch (...) { return fail(GPDLA_ERR_HOST, "unexpected C++ exception"); }

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(GPDLA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                  __FILE__, __LINE__);                                                     \
  } while (0)

int select_device(int device_id) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(GPDLA_ERR_NO_DEVICE, "no HIP device available (%s); libgpdla has no CPU fallback",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= n)
    return fail(GPDLA_ERR_NO_DEVICE, "device_id %d out of range [0, %d)", device_id, n);
  HIP_TRY(hipSetDevice(device_id));
  return GPDLA_OK;
}

// Lyman-series tables -> __constant__ memory, once per device.
std::mutex g_table_mutex;
bool g_table_loaded[64] = {false};

// Damping parameters y_j = gamma_j / (sqrt2 sigma) and the accurate-tier polynomial tables built from
// them (near_tables.hpp); host copy, built once per process.
std::vector<double> g_near_host;
double g_line_y[kMaxLines];

void ensure_near_host() {  // caller holds g_table_mutex
  if (!g_near_host.empty()) return;
#define GP_GAM0(i, wl, f, G, lead, gam) gam,
  const double gam[] = {GPDLA_LYMAN_SERIES(GP_GAM0)};
#undef GP_GAM0
  const double sigma = GPDLA_GAUSS_SIGMA_CGS;
  for (int i = 0; i < kMaxLines; ++i) g_line_y[i] = gam[i] / std::sqrt(2.0) / sigma;
  build_near_tables(g_line_y, kMaxLines, g_near_host);
}

int ensure_line_table(int device_id) {
  std::lock_guard<std::mutex> lock(g_table_mutex);
  if (device_id < 64 && g_table_loaded[device_id]) return GPDLA_OK;
  ensure_near_host();
  double *d_near = nullptr;  // lives as long as the process (one per device)
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_near), g_near_host.size() * sizeof(double)));
  HIP_TRY(hipMemcpy(d_near, g_near_host.data(), g_near_host.size() * sizeof(double), hipMemcpyHostToDevice));
  LineTable t;
  t.near_poly = d_near;
#define GP_WL(i, wl, f, G, lead, gam) wl,
#define GP_LEAD(i, wl, f, G, lead, gam) lead,
#define GP_GAM(i, wl, f, G, lead, gam) gam,
#define GP_OSC(i, wl, f, G, lead, gam) f,
  const double wl[] = {GPDLA_LYMAN_SERIES(GP_WL)};
  const double lead[] = {GPDLA_LYMAN_SERIES(GP_LEAD)};
  const double gam[] = {GPDLA_LYMAN_SERIES(GP_GAM)};
  const double osc[] = {GPDLA_LYMAN_SERIES(GP_OSC)};
  const double taps[] = GPDLA_INSTRUMENT_PROFILE;
  const double sigma = GPDLA_GAUSS_SIGMA_CGS;
  for (int i = 0; i < kMaxLines; ++i) {
    t.wavelength_cm[i] = wl[i];
    t.leading[i] = lead[i];
    t.osc[i] = osc[i];
    t.y[i] = gam[i] / std::sqrt(2.0) / sigma;
    t.y2[i] = t.y[i] * t.y[i];
    t.cwing[i] = lead[i] * t.y[i];
    t.t2[i] = kE2 - 2.0 * t.y2[i];
    t.wing[i] = {GPDLA_SPEED_OF_LIGHT_CGS / wl[i] / 1e8 / (std::sqrt(2.0) * sigma), t.y2[i], t.cwing[i], 0.0};
  }
  for (int i = 0; i < 7; ++i) t.taps[i] = taps[i];
  t.c = GPDLA_SPEED_OF_LIGHT_CGS;
  t.inv_sqrt2_sigma = 1.0 / (std::sqrt(2.0) * sigma);
  t.inv_sqrt2pi_sigma = 1.0 / (std::sqrt(2.0 * 3.14159265358979323846) * sigma);
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_lines), &t, sizeof(t)));
  if (device_id < 64) g_table_loaded[device_id] = true;
  return GPDLA_OK;
}

template <typename T>
int dev_alloc(T **p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), count * sizeof(T)));
  return GPDLA_OK;
}

template <typename T>
int upload(T **p, const T *host, size_t count, hipStream_t st) {
  int rc = dev_alloc(p, count);
  if (rc) return rc;
  if (count) HIP_TRY(hipMemcpyAsync(*p, host, count * sizeof(T), hipMemcpyHostToDevice, st));
  return GPDLA_OK;
}

void dev_free(void *p) {
  if (p) (void)hipFree(p);
}

// Drains a stream when it leaves scope.  Declared AFTER the host buffers that asynchronous copies on
// that stream write into, so that on every exit path -- the error returns included -- the copies have
// finished before those buffers are destroyed (a copy engine still writing into a freed std::vector
// would corrupt the heap).
struct StreamDrain {
  hipStream_t stream;
  ~StreamDrain() { (void)hipStreamSynchronize(stream); }
};

// (re)allocate *p for `count` elements unless its capacity already suffices
template <typename T>
int reserve(T **p, size_t *cap, size_t count) {
  if (count == 0) count = 1;
  if (*p && *cap >= count) return GPDLA_OK;
  dev_free(*p);
  *p = nullptr;
  *cap = 0;
  int rc = dev_alloc(p, count);
  if (!rc) *cap = count;
  return rc;
}

// Device buffers of one call, freed on every exit path (hipFree waits for the kernels that use them).
struct DeviceTemps {
  std::vector<void *> ptrs;
  template <typename T>
  int alloc(T **p, size_t count) {
    int rc = dev_alloc(p, count);
    if (!rc) ptrs.push_back(*p);
    return rc;
  }
  ~DeviceTemps() {
    for (void *p : ptrs) dev_free(p);
  }
};

// The device temporaries of one call and its asynchronous copies on one stream.  Declared AFTER every
// host buffer those copies read or write (StreamDrain's rule): on every exit path the stream is
// drained first, then the temporaries are freed, and only then do those host buffers go.
struct Staging {
  hipStream_t st;
  DeviceTemps tmp;
  explicit Staging(hipStream_t stream) : st(stream) {}
  ~Staging() { (void)hipStreamSynchronize(st); }
  template <typename T>  // allocate, then host -> device
  int put(T **dst, const T *src, size_t count) {
    int rc = tmp.alloc(dst, count);
    if (rc) return rc;
    if (count) HIP_TRY(hipMemcpyAsync(*dst, src, count * sizeof(T), hipMemcpyHostToDevice, st));
    return GPDLA_OK;
  }
  template <typename T>  // device -> host, where the caller asked for the array
  int fetch(T *host, const T *dev, size_t count) {
    if (host && count) HIP_TRY(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, st));
    return GPDLA_OK;
  }
};

// Two timing events of one call, destroyed on every exit path.
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int create() {
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    return GPDLA_OK;
  }
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};

// -DONESHOT_EXP_TIMING (diagnostic build, profiles/r05_one_shot_timing.txt): where a one-shot call
// spends what the sweeps do not, on stderr.  The code that reports is compiled in every build and
// does nothing in the normal one.
#ifdef ONESHOT_EXP_TIMING
constexpr bool kOneShotTiming = true;
#else
constexpr bool kOneShotTiming = false;
#endif

double wall_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

extern "C" {

int gpdla_abi_version(void) { return GPDLA_ABI_VERSION; }

const char *gpdla_last_error(void) { return t_error.c_str(); }

void gpdla_debug_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}

int gpdla_debug_throw(int kind) try {
  if (kind == 1) throw std::bad_alloc();
  if (kind == 2) throw std::runtime_error("thrown on request");
  if (kind == 3) throw 42;
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"

// Host evaluation of the accurate-tier table of one Lyman line (0-based) at |x| < 32: what the sweep
// kernel computes for Re w(x + i y_line).  Needs no GPU; tests/test_near_tables.py checks it
// against mpmath.  *y_out (optional) receives the line's damping parameter.
extern "C" int gpdla_debug_near_poly(int line, double x, double *value_out, double *y_out) {
  if (line < 0 || line >= kMaxLines || !value_out || !(std::fabs(x) < 32.0))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "gpdla_debug_near_poly: line %d, x %g", line, x);
  {
    std::lock_guard<std::mutex> lock(g_table_mutex);
    ensure_near_host();
  }
  *value_out = near_poly_host(g_near_host.data() + (size_t)line * kNearLineDoubles, std::fabs(x));
  if (y_out) *y_out = g_line_y[line];
  return GPDLA_OK;
}
