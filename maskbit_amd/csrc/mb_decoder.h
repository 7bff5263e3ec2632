// What decoder.hip offers besides the tokenizer handle's own C entry points (mb_dec_* / mb_enc_*, include/maskbit_hip.h, defined at its end):
// single tokenizer layers on caller buffers for the diagnostic entries in diag.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mb {

// Single tokenizer layers on caller buffers (include/maskbit_hip_diag.h: mb_conv_layer, mb_groupnorm_stats, mb_avgpool2, mb_s2d): the handle's own
// launch_conv / launch_gn / weight repack on a scratch context.  They synchronise the stream (the scratch is freed on return) and report like an
// entry point: 0, or the code of a fail() whose message names the entry (diag_pool: `what`).
struct ConvDiag {
  const void* in; const float* w; const float* bias; const float* gamma; const float* beta; const void* residual;
  void* out; float* img_nchw; uint8_t* img_u8;
  const float* out_gamma; const float* out_beta; float* out_scale_shift; float* out_part; int* part_tiles; unsigned* saturated;
  int B, H, W, Cin, Cout, ks, up, final_layer;
};
int diag_conv(const ConvDiag& q, hipStream_t s);
int diag_groupnorm(const void* x, const float* gamma, const float* beta, float* scale_shift, int B, int HW, int C, hipStream_t s);
int diag_pool(const char* what, bool avg, const void* x, void* y, int B, int H, int W, int C, hipStream_t s);
int diag_maxpool(const void* x, void* y, int B, int H, int W, int C, hipStream_t s);
// mb_conv_relu_layer: w fp32 OIHW, bias fp32 [Cout] or null, in / out fp16 NHWC with the true channel counts
int diag_conv_relu(const void* in, const float* w, const float* bias, void* out, unsigned* saturated, int B, int H, int W, int Cin, int Cout, int ks, hipStream_t s);

// The launches the VGG16 stack of lpips.hip is made of.  No allocation, no synchronisation.
// One convolution (ks 1, or 3 with zero padding 1) + bias + ReLU of conv_kernel: in fp16 [B, H, W, cin_pad] (cin_pad % 64 == 0), w as
// launch_repack_conv leaves it, bias fp32 [cout_pad], out fp16 [B, H, W, cout] (cout % 4 == 0, cout_pad % 128 == 0), H % 8 == 0, W % 16 == 0;
// *sat += the 4-channel output groups clamped at the fp16 range.  Tiles are per image: an image's result does not depend on B.
struct ConvRelu {
  const void* in; const void* w; const float* bias; void* out; unsigned* sat;
  int B, H, W, cin_pad, cout, cout_pad, ks;
};
void launch_conv_relu(hipStream_t s, const ConvRelu& q);
// max_pool2d(2, 2) of x fp16 [B, H, W, C] (H, W even, C % 8 == 0)
void launch_maxpool2(hipStream_t s, const void* x, void* y, int B, int H, int W, int C);
// fp32 OIHW [cout, cin, ks, ks] -> fp16 [tap][cout_pad][cin_pad], zero-filled (repack_conv_kernel)
void launch_repack_conv(hipStream_t s, const float* w_oihw, void* out, int cout, int cin, int ks, int cout_pad, int cin_pad);
}  // namespace mb
