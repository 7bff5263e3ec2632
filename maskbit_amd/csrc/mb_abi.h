// Host-side plumbing of the C ABI, shared by every translation unit that defines an entry point (engine.hip, diag.hip, decoder.hip, taming.hip,
// lpips.hip, inception.hip, vq.hip, ...): the library's one error path (fail -> mb_last_error), the one owner of device allocations (DevArena), the
// check after a launch, the read of a handle's device counter, and the optional per-kernel device timing.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
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

// The owner of a handle's (or of one diagnostic call's) device allocations: hipMalloc through get / zeroed, everything freed in reverse order by
// the destructor.  Failure is sticky -- after the first failed call nothing more is allocated and every later *p stays null -- so a create function
// allocates straight through and asks failed() once at the end.  (vq.hip's stream-ordered hipMallocAsync scratch must not synchronise and is not this.)
struct DevArena {
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() { for (auto it = owned.rbegin(); it != owned.rend(); ++it) (void)hipFree(*it); }
  // n elements (0: 1, so that every pointer of a live arena is valid); *p is null after any failure
  template <class T>
  bool get(T** p, size_t n) {
    *p = nullptr;
    if (err != hipSuccess) return false;
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void* q = nullptr;
    if (!ok(hipMalloc(&q, bytes), "hipMalloc", bytes)) return false;
    owned.push_back(q);
    *p = (T*)q;
    return true;
  }
  // the same, zero-filled (a failed fill leaves *p null too; the memory stays the arena's until it goes)
  template <class T>
  bool zeroed(T** p, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    if (get(p, n) && !ok(hipMemset(*p, 0, bytes), "hipMemset", bytes)) *p = nullptr;
    return *p != nullptr;
  }
  // 0, or the first failure in the name of the entry `who`: -10, the code of HIP_TRY
  int failed(const char* who) const {
    return err == hipSuccess ? 0 : fail(-10, "%s: %s of %zu bytes failed: %s", who, err_call, err_bytes, hipGetErrorString(err));
  }

 private:
  std::vector<void*> owned;
  hipError_t err = hipSuccess;     // of the call that failed ...
  const char* err_call = "";       // ... its name ...
  size_t err_bytes = 0;            // ... and its size
  bool ok(hipError_t e, const char* call, size_t bytes) {
    if (e == hipSuccess) return true;
    err = e; err_call = call; err_bytes = bytes;
    return false;
  }
};

// the end of an entry point that launched kernels: 0, or the launch error
inline int launched() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(-11, "kernel launch failed: %s", hipGetErrorString(e));
}

// the mb_*_saturation_count entries (`what`): *count = the device counter, zeroed afterwards when `reset`.  Synchronises the stream
inline int read_counter(const char* what, unsigned* dev, unsigned* count, int reset, hipStream_t s) {
  if (hipMemcpyAsync(count, dev, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess ||
      (reset && hipMemsetAsync(dev, 0, sizeof(unsigned), s) != hipSuccess) || hipStreamSynchronize(s) != hipSuccess)
    return fail(-10, "%s: copy failed", what);
  return 0;
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
