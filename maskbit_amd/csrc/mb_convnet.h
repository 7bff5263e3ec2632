// What the Conv+BatchNorm feature-network handles (inception.hip: mb_inception, resnet.hip: mb_resnet) both own and both do: the convolution
// records with their device memory, the fp32 head's weights, the saturation counter, the device arena, and the checkpoint key -> slot map with
// its loader and its completeness check.  Host code only; a handle's own file keeps its layer list, its schedule and its entry points.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "mb_abi.h"
#include "mb_incep.h"

namespace mb {

constexpr int CN_BN_PARTS = 4;
const char* const CN_BN_NAMES[CN_BN_PARTS] = {".weight", ".bias", ".running_mean", ".running_var"};

struct CnConv {
  std::string key, bn;                                           // checkpoint key of the weight; prefix of its BatchNorm's entries
  int64_t shape[4] = {0, 0, 0, 0};                               // of the checkpoint's weight
  int cin = 0, cout = 0, kh = 1, kw = 1, stride = 1, ph = 0, pw = 0;   // as the kernel runs it (ResNet's conv1: [64, 3, 7, 7] run as 147 -> 64, 1x1)
  h16* w = nullptr;
  float *bnv = nullptr, *scale = nullptr, *shift = nullptr;      // bnv [4][cout]: gamma, beta, running mean, running variance
};

// where a checkpoint entry goes: a convolution's weight (exact 4-d shape, repacked), part `part` of its BatchNorm block (copied, then folded
// into scale / shift), `n` fp32 values copied to `vec` (fc.*, ResNet's mean / std), or nowhere (*.num_batches_tracked: accepted and ignored)
enum { CN_WEIGHT, CN_BN, CN_VEC, CN_IGNORED };
struct CnSlot { int kind = CN_IGNORED; int conv = -1, part = 0; float* vec = nullptr; size_t n = 0; bool loaded = false; };

struct ConvNet {
  std::vector<CnConv> convs;
  float *fc_w = nullptr, *fc_b = nullptr;                        // [fc_out][fc_in], [fc_out]
  int fc_in = 0, fc_out = 0;
  float bn_eps = 0.f;
  unsigned* sat = nullptr;                                       // device counter: fp16 clamps since the last read
  // checkpoint key -> slot, filled as the handle names its layers (the slots hold indices into convs, which may still grow)
  std::unordered_map<std::string, CnSlot> table;
  size_t missing = 0;                                            // slots that must be loaded and are not yet
  DevArena mem;
};

// ---- building a handle: every add allocates what it names
inline void name_slot(ConvNet& n, const std::string& key, const CnSlot& e) {
  n.table[key] = e;
  if (e.kind != CN_IGNORED) ++n.missing;
}
// `key`: of the weight, `bn`: the prefix of the BatchNorm's entries -- the handle's naming convention is its own; -> the index in convs
inline int add_conv(ConvNet& n, const std::string& key, const std::string& bn, int cin, int cout, int kh, int kw, int stride, int ph, int pw) {
  CnConv c;
  c.key = key; c.bn = bn; c.cin = cin; c.cout = cout; c.kh = kh; c.kw = kw; c.stride = stride; c.ph = ph; c.pw = pw;
  c.shape[0] = cout; c.shape[1] = cin; c.shape[2] = kh; c.shape[3] = kw;
  n.mem.get(&c.w, (size_t)kh * kw * ic_cout_pad(cout) * ic_cin_pad(cin));
  n.mem.zeroed(&c.bnv, (size_t)CN_BN_PARTS * cout); n.mem.zeroed(&c.scale, (size_t)cout); n.mem.zeroed(&c.shift, (size_t)cout);
  const int i = (int)n.convs.size();
  n.convs.push_back(c);
  name_slot(n, key, CnSlot{CN_WEIGHT, i});
  for (int k = 0; k < CN_BN_PARTS; ++k) name_slot(n, bn + CN_BN_NAMES[k], CnSlot{CN_BN, i, k});
  name_slot(n, bn + ".num_batches_tracked", CnSlot{});
  return i;
}
inline void add_vec(ConvNet& n, const std::string& key, float* dst, size_t count) { name_slot(n, key, CnSlot{CN_VEC, -1, 0, dst, count}); }
// the saturation counter and the head `prefix`fc.weight [out, in], `prefix`fc.bias
inline void add_head(ConvNet& n, const std::string& prefix, int in, int out) {
  n.fc_in = in; n.fc_out = out;
  n.mem.zeroed(&n.sat, 1);
  n.mem.get(&n.fc_w, (size_t)out * in); n.mem.get(&n.fc_b, (size_t)out);
  add_vec(n, prefix + "fc.weight", n.fc_w, (size_t)out * in);
  add_vec(n, prefix + "fc.bias", n.fc_b, (size_t)out);
}

// ---- the loaders' common body (`what`: the entry point; `name`: the entry as the caller gave it, `key`: as the table has it): one checkpoint
// entry of fp32 values on the device into its slot.  0, -2 for an entry the handle has no slot for, -4 for one of the wrong shape or size; a
// refused entry leaves the handle as it was
inline int load_entry(const char* what, ConvNet& n, const char* name, const std::string& key, const float* data, const int64_t* shape, int ndim,
                      hipStream_t s) {
  const auto it = n.table.find(key);
  if (it == n.table.end()) return fail(-2, "%s: unknown checkpoint entry '%s'", what, name);
  CnSlot& e = it->second;
  if (e.kind == CN_IGNORED) return 0;
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
  int rc = 0;
  if (e.kind == CN_VEC) {
    if (numel != e.n) return fail(-4, "%s: %s: expected %zu values", what, name, e.n);
    HIP_TRY(hipMemcpyAsync(e.vec, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {
    const CnConv& c = n.convs[e.conv];
    if (e.kind == CN_WEIGHT) {
      if (ndim != 4 || shape[0] != c.shape[0] || shape[1] != c.shape[1] || shape[2] != c.shape[2] || shape[3] != c.shape[3])
        return fail(-4, "%s: %s: expected [%d, %d, %d, %d]", what, name, (int)c.shape[0], (int)c.shape[1], (int)c.shape[2], (int)c.shape[3]);
      // (ResNet's conv1 [64, 3, 7, 7] is read as [64, 147, 1, 1]: the same memory, input channel ci * 49 + ky * 7 + kx)
      launch_repack_convbn(s, data, c.w, c.cout, c.cin, c.kh, c.kw);
    } else {
      if (numel != (size_t)c.cout) return fail(-4, "%s: %s: expected %d values", what, name, c.cout);
      HIP_TRY(hipMemcpyAsync(c.bnv + (size_t)e.part * c.cout, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
      launch_bn_fold(s, c.bnv, c.scale, c.shift, c.cout, n.bn_eps);
    }
    rc = launched();
  }
  if (!e.loaded) { e.loaded = true; --n.missing; }
  return rc;
}

// the diagnostic entries mb_*_folded_bn (`what`; `name`: the BatchNorm's prefix as the caller gave it, `key`: its `.weight` entry as the table has
// it): the folded scale and shift, as the convolution's epilogue reads them, copied to the caller's device buffers.  0, -2 for a prefix that
// names no BatchNorm of the handle, -4 for a wrong channel count -- the loader's codes
inline int folded_bn(const char* what, const ConvNet& n, const char* name, const std::string& key, float* scale_out, float* shift_out, int cout,
                     hipStream_t s) {
  const auto it = n.table.find(key);
  if (it == n.table.end() || it->second.kind != CN_BN) return fail(-2, "%s: unknown BatchNorm '%s'", what, name);
  const CnConv& c = n.convs[it->second.conv];
  if (cout != c.cout) return fail(-4, "%s: %s: expected %d values", what, name, c.cout);
  HIP_TRY(hipMemcpyAsync(scale_out, c.scale, (size_t)cout * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(shift_out, c.shift, (size_t)cout * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}

// 0, or -1 with the name of an entry that is still to be loaded
inline int complete(const char* what, const ConvNet& n) {
  if (!n.missing) return 0;
  for (const auto& kv : n.table)
    if (kv.second.kind != CN_IGNORED && !kv.second.loaded)
      return fail(-1, "%s: the checkpoint is not complete (%zu entries are missing, '%s' among them)", what, n.missing, kv.first.c_str());
  return 0;
}

}  // namespace mb
