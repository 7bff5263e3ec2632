// The convolution, GroupNorm, pool and repack launchers of conv.hip: what the tokenizer handles (decoder.hip and taming.hip, on the scaffold of
// mb_autoenc.h), the VGG16 stack of LPIPS (lpips.hip) and the single-layer diagnostic entries (diag.hip) are made of.  No allocation, no
// synchronisation, no handle: every buffer is the caller's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mb_common.h"

namespace mb {

constexpr int TH8 = 8, TW = 16;          // output pixel tile: TH x 16 pixels, TH = 8 (4 waves) or 16 (8 waves: twice the pixels per weight tile, four waves per SIMD)
constexpr int CK = 64;                   // input-channel chunk = one 128-byte LDS row

struct Conv {
  int cin = 0, cout = 0, ks = 3; bool has_bias = false, up = false;
  bool down = false;       // stride-2 3x3 Conv2dSame, executed as a 2x2 conv on the space-to-depth input (cin_pad = 4*cin)
  int cout_w = 0;          // output channels in the checkpoint (cout may be rounded up for 8-byte stores)
  int cin_pad = 0, cout_pad = 0;
  h16* w = nullptr; float* b = nullptr;
  unsigned* sat = nullptr; // the owner's saturation counter
};
struct Norm { int c = 0; float *g = nullptr, *b = nullptr; };
// GroupNorm scratch of one stream of layers: what launch_conv leaves for launch_gn.  A handle owns one; the single-layer diagnostic entries
// (include/maskbit_hip_diag.h) build one on scratch buffers, so that they run the same two launchers.
struct GnCtx {
  float* part = nullptr;         // [B][tiles or chunks][32 groups][sum, sumsq]: gn_part_elems floats
  float2* ss = nullptr;          // [B][C] (scale, shift) of the last launch_gn
  const void* of = nullptr;      // the tensor whose per-tile GroupNorm partials the last conv left in `part` (null: none) ...
  int ntile = 0;                 // ... and the number of pixel tiles per image they cover
};

// channel padding of a convolution: input channels to whole 64-channel chunks, output channels to whole 128-channel (final layer: 16-channel) tiles
void shape_conv(Conv& c, int cin, int cout, int ks, bool bias, bool up, bool final_);
// DownsamplingStage.down_conv: 3x3, stride 2, bias (autoencoder.py:165), run as a 2x2 conv on the space-to-depth input
void shape_down_conv(Conv& c, int ch);
size_t conv_weight_elems(const Conv& c);
// floats of GnCtx::part for B images of up to H x W pixels: the per-tile partials of a conv epilogue or the chunks of the sweep, whichever are more
// (H = W = 0: the sweep alone)
size_t gn_part_elems(int B, int H, int W);

// fp32 OIHW (device) -> the kernel's fp16 [tap][cout_pad][cin_pad], zero-filled: [cout, cin, ks, ks] as it stands, or (`down`) the 3x3 stride-2
// [cout, cin, 3, 3] as the four taps of the 2x2 conv on the space-to-depth input (cin_pad = 4 cin)
void launch_repack_conv(hipStream_t s, const float* w_oihw, h16* out, int cout, int cin, int ks, int cout_pad, int cin_pad, bool down = false);
inline void launch_repack_conv(hipStream_t s, const Conv& c, const float* w_oihw) {
  launch_repack_conv(s, w_oihw, c.w, c.cout_w, c.cin, c.ks, c.cout_pad, c.cin_pad, c.down);
}

// One convolution of the tokenizer on fp16 NHWC (H % 8 == 0, W % 16 == 0): `gn` (or null) = the (scale, shift) of a GroupNorm + SiLU prologue,
// `residual` (or null) added in the epilogue; final_: fp32 NCHW `img` and / or uint8 NHWC `u8` instead of `out`.  With `stats` the epilogue leaves the
// GroupNorm partials of `out` in gc where the channel count allows it (gc->of == out then), for the launch_gn that follows.
// gn_silu = false (1x1 convolutions only): the prologue is the GroupNorm alone, without SiLU.
void launch_conv(hipStream_t s, GnCtx* gc, const Conv& c, const h16* in, const float2* gn, const h16* residual, h16* out, float* img, uint8_t* u8,
                 int B, int H, int W, bool final_, bool stats = true, bool gn_silu = true);
// GroupNorm(32 groups, eps 1e-6) statistics of x [B, HW, n.c] -> gc->ss: from the partials the last conv left when x is that conv's output, else a sweep
void launch_gn(hipStream_t s, GnCtx* gc, const Norm& n, const h16* x, int B, int HW);

// One convolution (ks 1, or 3 with zero padding 1) + bias + ReLU, without GroupNorm prologue or partials (the VGG16 stack of lpips.hip):
// in [B, H, W, cin_pad] (cin_pad % 64 == 0), w as launch_repack_conv leaves it, bias fp32 [cout_pad], out [B, H, W, cout] (cout % 4 == 0,
// cout_pad % 128 == 0), H % 8 == 0, W % 16 == 0; *sat += the 4-channel output groups clamped at the fp16 range.
// Tiles are per image: an image's result does not depend on B.
struct ConvRelu {
  const h16* in; const h16* w; const float* bias; h16* out; unsigned* sat;
  int B, H, W, cin_pad, cout, cout_pad, ks;
};
void launch_conv_relu(hipStream_t s, const ConvRelu& q);

// x fp16 [B, H, W, C], H and W even, C % 8 == 0
void launch_s2d(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C);        // space-to-depth -> [B, H/2, W/2, 4C]
void launch_avgpool2(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C);   // avg_pool2d(2, 2)
void launch_maxpool2(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C);   // max_pool2d(2, 2)

// the ends of the tokenizer: LFQ tokens -> +-1 latent [npix][64]; image fp32 NCHW -> fp16 NHWC [B, H, W, 64]; z [B*HW][Kp] -> indices (+ zq, zraw or null)
void launch_latent(hipStream_t s, const int64_t* tokens, h16* z, size_t npix, int K);
void launch_pack_image(hipStream_t s, const float* img, h16* out, int B, int C, int H, int W);
void launch_lfq(hipStream_t s, const h16* z, int64_t* idx, float* zq, float* zraw, int B, int HW, int K, int Kp);

}  // namespace mb
