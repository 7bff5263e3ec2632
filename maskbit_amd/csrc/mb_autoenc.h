// What the conv-autoencoder tokenizer handles (decoder.hip: mb_dec, taming.hip: mb_taming) both own and both do: the device arena, the three
// ping-pong activation buffers, the GroupNorm scratch, the checkpoint key -> slot map with its loader, and the ResNet block.  Host code only;
// a handle's own file keeps its layer lists, its schedule (encode_to_z / decode_from_z) and its entry points.
#pragma once
#include <string>
#include <unordered_map>

#include "mb_abi.h"
#include "mb_conv.h"

namespace mb {

// where a checkpoint entry goes: a convolution's weight or bias -- all of it (rows = 0: its cout_w rows when it is loaded) or rows
// [row0, row0 + rows) of a stacked 1x1 convolution --, or the `n` values of a norm's gamma / beta.
// fold: the convolution carries a following (y + 1) / 2: weight x 0.5, bias (b + 1) / 2
struct Param { Conv* conv = nullptr; bool bias = false; float* vec = nullptr; int n = 0; int row0 = 0, rows = 0; bool fold = false; };
// nin_shortcut (1x1, cin != cout) comes in two forms.  sc_on_input (Taming, taming_autoencoder.py:112-118): out = nin_shortcut(x) + h, a
// cin -> cout convolution.  Otherwise the conv-VQGAN quirk (autoencoder.py:72-73,93-96): out = h + nin_shortcut(h), cout -> cout, the block
// input is dropped.
struct ResBlock { Norm n1, n2; Conv c1, c2, sc; bool has_sc = false, sc_on_input = false; };

struct AutoEnc {
  h16* buf[3] = {nullptr, nullptr, nullptr};
  float* fold_w = nullptr;       // scratch of the folded convolution's weight x 0.5 before its repack (allocated when one is named)
  unsigned* sat = nullptr;       // device counter: fp16 clamps since the last read
  GnCtx gn;
  h16* h1_tap = nullptr;         // diagnostic (mb_autoenc_block): where run_block copies conv1's output [B, H, W, cout] to, or null
  // checkpoint key -> slot, filled as the create function names each parameter.  The Conv pointers are into the handle and its vectors, which
  // are sized before their elements are named and never again.
  std::unordered_map<std::string, Param> params;
  DevArena mem;
};

static __global__ void affine_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n, float mul, float add) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = fmaf(src[i], mul, add * mul);
}

// ---- building a handle: shape (shape_conv / shape_down_conv), allocate, name
inline void alloc_conv(AutoEnc& a, Conv& c) {
  c.sat = a.sat;
  a.mem.get(&c.w, conv_weight_elems(c));
  if (c.has_bias) a.mem.zeroed(&c.b, (size_t)c.cout_pad);
}
inline void name_conv(AutoEnc& a, Conv& c, const std::string& name, bool fold = false) {
  a.params[name + ".weight"] = Param{&c, false, nullptr, 0, 0, 0, fold};
  if (c.has_bias) a.params[name + ".bias"] = Param{&c, true, nullptr, 0, 0, 0, fold};
  if (fold && !a.fold_w) a.mem.get(&a.fold_w, (size_t)c.cout_w * c.cin * c.ks * c.ks);
}
inline void init_conv(AutoEnc& a, Conv& c, const std::string& name, int cin, int cout, int ks, bool bias, bool up = false, bool final_ = false,
                      bool fold = false) {
  shape_conv(c, cin, cout, ks, bias, up, final_);
  alloc_conv(a, c);
  name_conv(a, c, name, fold);
}
inline void init_norm(AutoEnc& a, Norm& n, const std::string& name, int c) {
  n.c = c;
  a.mem.get(&n.g, (size_t)c);
  a.mem.get(&n.b, (size_t)c);
  a.params[name + ".weight"] = Param{nullptr, false, n.g, c};
  a.params[name + ".bias"] = Param{nullptr, false, n.b, c};
}
// bias: of every convolution of the block
inline void init_block(AutoEnc& a, ResBlock& rb, const std::string& p, int cin, int cout, bool bias, bool sc_on_input) {
  rb.has_sc = cin != cout;
  rb.sc_on_input = sc_on_input;
  init_norm(a, rb.n1, p + ".norm1", cin);
  init_conv(a, rb.c1, p + ".conv1", cin, cout, 3, bias);
  init_norm(a, rb.n2, p + ".norm2", cout);
  init_conv(a, rb.c2, p + ".conv2", cout, cout, 3, bias);
  if (rb.has_sc) init_conv(a, rb.sc, p + ".nin_shortcut", sc_on_input ? cin : cout, cout, 1, bias);
}

// x (buffer index xi, B x H x W pixels) -> the buffer index holding the block output
inline int run_block(hipStream_t s, AutoEnc& a, const ResBlock& rb, int xi, int B, int H, int W) {
  const int t1 = (xi + 1) % 3, t2 = (xi + 2) % 3;
  launch_gn(s, &a.gn, rb.n1, a.buf[xi], B, H * W);
  launch_conv(s, &a.gn, rb.c1, a.buf[xi], a.gn.ss, nullptr, a.buf[t1], nullptr, nullptr, B, H, W, false);
  if (a.h1_tap) (void)hipMemcpyAsync(a.h1_tap, a.buf[t1], (size_t)B * H * W * rb.c1.cout * sizeof(h16), hipMemcpyDeviceToDevice, s);
  launch_gn(s, &a.gn, rb.n2, a.buf[t1], B, H * W);
  if (!rb.has_sc) {
    launch_conv(s, &a.gn, rb.c2, a.buf[t1], a.gn.ss, a.buf[xi], a.buf[t2], nullptr, nullptr, B, H, W, false);
    return t2;
  }
  if (rb.sc_on_input) {
    // The shortcut runs after norm2's statistics are final (they stay in gn.ss) and leaves none of its own: its output is read as a residual,
    // not by a GroupNorm
    launch_conv(s, &a.gn, rb.sc, a.buf[xi], nullptr, nullptr, a.buf[t2], nullptr, nullptr, B, H, W, false, false);
    launch_conv(s, &a.gn, rb.c2, a.buf[t1], a.gn.ss, a.buf[t2], a.buf[xi], nullptr, nullptr, B, H, W, false);
    return xi;
  }
  launch_conv(s, &a.gn, rb.c2, a.buf[t1], a.gn.ss, nullptr, a.buf[t2], nullptr, nullptr, B, H, W, false, false);   // read by the shortcut conv, not by a GroupNorm
  launch_conv(s, &a.gn, rb.sc, a.buf[t2], nullptr, a.buf[t2], a.buf[t1], nullptr, nullptr, B, H, W, false);
  return t1;
}

// The common tail of the handles' loaders (`what`: the entry point): one checkpoint entry of `numel` fp32 values on the device into its slot.
// 0, -2 for an entry the handle has no slot for, -4 for one of the wrong size
inline int load_param(const char* what, AutoEnc& a, const char* name, const float* data, size_t numel, hipStream_t s) {
  const auto it = a.params.find(name);
  if (it == a.params.end()) return fail(-2, "%s: unknown checkpoint entry '%s'", what, name);
  const Param& p = it->second;
  if (!p.conv) {
    if (numel != (size_t)p.n) return fail(-4, "%s: %s: wrong norm size", what, name);
    HIP_TRY(hipMemcpyAsync(p.vec, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    return launched();
  }
  const Conv& c = *p.conv;
  const int rows = p.rows ? p.rows : c.cout_w;
  if (p.bias) {
    if (numel != (size_t)rows) return fail(-4, "%s: %s: wrong bias size", what, name);
    if (p.fold) hipLaunchKernelGGL(affine_kernel, dim3(1), dim3(64), 0, s, data, c.b, numel, 0.5f, 1.0f);
    else HIP_TRY(hipMemcpyAsync(c.b + p.row0, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    return launched();
  }
  // (a stride-2 convolution: the checkpoint's 3x3, whatever the taps it runs as)
  if (numel != (size_t)rows * c.cin * (c.down ? 9 : c.ks * c.ks)) return fail(-4, "%s: %s: wrong weight size", what, name);
  if (p.fold) {
    hipLaunchKernelGGL(affine_kernel, dim3(16), dim3(256), 0, s, data, a.fold_w, numel, 0.5f, 0.0f);
    data = a.fold_w;
  }
  // a slice (q / k / v of a stacked 1x1 convolution) is rows [row0, row0 + rows) of the [cout_pad][cin_pad] image
  launch_repack_conv(s, data, c.w + (size_t)p.row0 * c.cin_pad, rows, c.cin, c.ks, p.rows ? p.rows : c.cout_pad, c.cin_pad, c.down);
  return launched();
}

}  // namespace mb
