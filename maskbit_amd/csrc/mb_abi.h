// Host-side plumbing of the C ABI, shared by every translation unit that defines an entry point (engine.hip, diag.hip, decoder.hip, vq.hip):
// the library's one error path (fail -> mb_last_error), the check after a launch, and the optional per-kernel device timing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

namespace mb {

inline thread_local std::string g_err;   // what mb_last_error() returns

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return mb::fail(-10, "%s failed: %s", #expr, hipGetErrorString(e_));     \
  } while (0)

// the end of an entry point that launched kernels: 0, or the launch error
inline int launched() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(-11, "kernel launch failed: %s", hipGetErrorString(e));
}

// ---- optional per-kernel device timing with HIP events on the launch stream ------------------
struct Prof {
  bool on = false;
  // Generator forwards are sampled: the kernels of every `stride`-th forward are timed -- counted separately for GUIDED forwards (mb_gen_forward_cfg
  // and the guided steps of mb_sample: kernel names as they are) and PLAIN ones (mb_gen_forward, the unguided / zero-scale steps: names + ".plain"),
  // so that a plain forward never lands in a guided kernel's average whatever the step plan and the chunking (round-3 advice).
  int stride = 1, tick[2] = {0, 0};
  bool fwd_live = true, fwd_plain = false;
  void begin_forward(bool plain) { fwd_plain = plain; fwd_live = (tick[plain]++ % stride) == stride / 2; }   // (the middle of every stride)
  struct Rec { hipEvent_t a, b; int kind; };
  std::vector<Rec> recs;
  std::vector<std::string> names;
  std::map<std::string, int> index;
  std::map<int, std::pair<long, double>> acc;   // kind -> (calls, ms)
  int kind(const char* n0, bool in_forward) {
    const std::string n = (in_forward && fwd_plain) ? std::string(n0) + ".plain" : std::string(n0);
    auto it = index.find(n);
    if (it != index.end()) return it->second;
    names.push_back(n);
    return index[n] = (int)names.size() - 1;
  }
  void drain() {
    for (auto& r : recs) {
      float ms = 0.f;
      if (hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
        acc[r.kind].first += 1; acc[r.kind].second += ms;
      }
      (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    recs.clear();
  }
};
inline Prof g_prof;

struct ProfScope {
  hipStream_t s; bool live; hipEvent_t a, b; int kind;
  ProfScope(const char* name, hipStream_t st, bool in_forward = false) : s(st), live(g_prof.on && (!in_forward || g_prof.fwd_live)) {
    if (!live) return;
    kind = g_prof.kind(name, in_forward);
    (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    (void)hipEventRecord(a, s);
  }
  ~ProfScope() {
    if (!live) return;
    (void)hipEventRecord(b, s);
    g_prof.recs.push_back({a, b, kind});
  }
};

}  // namespace mb
