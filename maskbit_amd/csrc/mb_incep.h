// The launchers of inception.hip: what the Inception-v3 handle and the single-kernel diagnostic entries are made of.  No allocation, no
// synchronisation, no handle: every buffer is the caller's.  Activations are fp16 NHWC; a tensor is given as (pointer, channel offset, channel
// stride), so that a branch writes straight into its slice of the concatenation and a layer may read a slice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mb_common.h"

namespace mb {

constexpr int IC_CK = 32;                 // input channels per MFMA step
constexpr int IC_BN = 64;                 // output channels are padded to whole 64-channel tiles in the packed weights
constexpr int IC_SIDE = 299;              // the network's input resolution
constexpr int IC_SPATIAL_C = 7;           // channels of the sFID tap: Mixed_6d.branch1x1[..., :7] on the 17 x 17 map = 2023 values
constexpr int IC_INC = 8;                 // channels of the input image buffer (3 + 5 zeros: one 16-byte slot)

inline int ic_cin_pad(int cin) { return (cin + IC_CK - 1) / IC_CK * IC_CK; }
inline int ic_cout_pad(int cout) { return (cout + IC_BN - 1) / IC_BN * IC_BN; }
inline int ic_out_size(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }
inline int ic_pool_size(int n, int mode) { return mode == 0 ? (n - 3) / 2 + 1 : mode == 3 ? (n - 1) / 2 + 1 : n; }
constexpr float IC_BN_EPS = 1e-3f;        // Inception's BatchNorm epsilon (ResNet's is 1e-5: mb_resnet.h)

// the epilogues of the convolution, v = fma(acc, scale, shift) in fp32:
enum { CONVBN_RELU = 0,                   // fp16(relu(v)): BasicConv2d, and the first two convolutions of a bottleneck
       CONVBN_LINEAR = 1,                 // fp16(v): a bottleneck's downsample branch; saturation is counted on |v|
       CONVBN_RESIDUAL = 2,               // fp16(relu(v + float(identity[p][c]))): the add in fp32, one rounding
       CONVBN_LEAKY = 3 };                // fp16(v >= 0 ? v : v * slope): the discriminator's LeakyReLU; saturation on |v|

// One BasicConv2d: out = fp16(relu(scale * conv(in, w) + shift)), see include/maskbit_hip_diag.h mb_convbn_layer for the geometry taken
struct ConvBn {
  const h16* in; const h16* w; const float* scale; const float* shift; h16* out; unsigned* sat;
  int B, H, W, cin, cout;
  int kh, kw, stride, ph, pw;
  int in_off, in_cs, out_off, out_cs;
  int epi = CONVBN_RELU;
  float slope = 0.f;                      // CONVBN_LEAKY: the negative slope (in what was the padding in front of idn: no other member moves)
  const h16* idn = nullptr;               // CONVBN_RESIDUAL: channels [idn_off, idn_off + cout) of fp16 [B, Ho, Wo, idn_cs]
  int idn_off = 0, idn_cs = 0;
};
// null, or why the geometry is not taken
const char* convbn_refusal(const ConvBn& q);
// variant: 0 = by the size of the launch, 1 = 64 x 64 wave tiles, 2 = 32 x 32 wave tiles; the bits do not depend on it
void launch_convbn(hipStream_t s, const ConvBn& q, int variant = 0);
// fp32 OIHW [cout, cin, kh, kw] (device) -> fp16 [kh * kw][ic_cout_pad(cout)][ic_cin_pad(cin)], zero-filled
void launch_repack_convbn(hipStream_t s, const float* w_oihw, h16* out, int cout, int cin, int kh, int kw);
// bn fp32 [4][cout] = gamma, beta, running mean, running variance -> scale = gamma / sqrt(var + eps), shift = beta - mean * scale
void launch_bn_fold(hipStream_t s, const float* bn, float* scale, float* shift, int cout, float eps);

struct Pool3 {
  const h16* in; h16* out;
  int B, H, W, C, mode;                   // 0 max s2 valid, 1 max s1 p1, 2 avg s1 p1 (divisor = in-image taps), 3 max s2 p1 (in-image taps only)
  int in_off, in_cs, out_off, out_cs;
};
const char* pool3_refusal(const Pool3& q);
void launch_pool3(hipStream_t s, const Pool3& q);

// uint8 [B, 3, H, W] -> fp16 [B, 299, 299, 8]
void launch_inception_input(hipStream_t s, const uint8_t* u8, h16* out, int B, int H, int W);
// x fp16 [B, HW, C] (C % 8 == 0) -> mean fp32 [B, C]: per image a fixed-order fp32 sum, / float(HW)
void launch_spatial_mean(hipStream_t s, const h16* x, float* mean, int B, int HW, int C);
// out fp32 [B, HW * C] = channels [off, off + C) of x fp16 [B, HW, cs], (pixel, channel) order
void launch_channel_tap(hipStream_t s, const h16* x, float* out, int B, int HW, int C, int off, int cs);
// pool fp32 [B, D] x w fp32 [N, D] -> unbiased [B, N] (or null), biased [B, N] = unbiased + bias (or null); D % 256 == 0, D <= 2048
void launch_fc_head(hipStream_t s, const float* pool, const float* w, const float* bias, float* unbiased, float* biased, int B, int D, int N);

}  // namespace mb
