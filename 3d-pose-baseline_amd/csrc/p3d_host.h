// p3d_host.h -- what every host file of the library stands on: the thread's error text (g_err,
// fail, p3d_last_error), HIP_TRY / LAUNCH_CHECK, pad64 / aligned16, the host-side segment timer
// (HostProf / HP) and the per-launch profiler (ProfState, ProfScope, go).  Host code; included by
// p3d.hip behind the kernel headers, include/p3d.h and the standard headers, ahead of every other
// host file.
#pragma once

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) return fail(P3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define LAUNCH_CHECK(what)                                                          \
  do {                                                                              \
    hipError_t e_ = hipGetLastError();                                              \
    if (e_ != hipSuccess) return fail(P3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e_)); \
  } while (0)

int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// Host-side segment timing of serve_impl (dev builds: -DP3D_HOSTPROF; tools/host_prof.sh): per
// segment the summed steady-clock nanoseconds and count, printed at exit.
#ifdef P3D_HOSTPROF
#include <chrono>
struct HostProf {
  double ns[16] = {}; long n[16] = {};
  ~HostProf() {
    fprintf(stderr, "P3D_HOSTPROF");
    for (int i = 0; i < 16; ++i) if (n[i]) fprintf(stderr, " s%d=%.3fus", i, ns[i] / n[i] / 1000.0);
    fprintf(stderr, "\n");
  }
};
static HostProf g_hp;
#define HP_START auto hp_t = std::chrono::steady_clock::now();
#define HP(i) do { auto t_ = std::chrono::steady_clock::now(); \
    g_hp.ns[i] += std::chrono::duration<double, std::nano>(t_ - hp_t).count(); ++g_hp.n[i]; hp_t = t_; } while (0)
#else
#define HP_START
#define HP(i) do { } while (0)
#endif

// live kernel timing (p3d_profile_start/stop): one hipEvent pair per launch
struct ProfState {
  bool on = false;
  std::vector<hipEvent_t> ev;
  std::vector<const char*> ev_tag;
  size_t ev_used = 0;
};

struct ProfScope {  // times one kernel launch when profiling (p3d_profile_start/stop)
  ProfState* p; hipEvent_t e0, e1; bool on;
  ProfScope(ProfState* p_, const char* tag) : p(p_), e0(nullptr), e1(nullptr), on(false) {
    if (p && p->on && 2 * (p->ev_used + 1) <= p->ev.size()) {
      on = true;
      p->ev_tag[p->ev_used] = tag;
      e0 = p->ev[2 * p->ev_used];
      e1 = p->ev[2 * p->ev_used + 1];
    }
  }
  ProfScope(p3d_model* m, const char* tag);   // the model's ProfState (p3d_model.h)
  ~ProfScope() {
    if (on) ++p->ev_used;
  }
};

// Launch `k`; under profiling the event pair is attached to the dispatch itself
// (hipExtLaunchKernel start/stop events = the AQL packet's begin/end timestamps, the
// same interval rocprofv3 --kernel-trace reports), not recorded as separate packets.
template <typename F, typename... A>
void go(const ProfScope& ps, F k, dim3 grid, dim3 block, hipStream_t st, A... args) {
  if (ps.on) hipExtLaunchKernelGGL(k, grid, block, 0, st, ps.e0, ps.e1, 0, args...);
  else k<<<grid, block, 0, st>>>(args...);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

extern "C" const char* p3d_last_error(void) { return g_err.c_str(); }
