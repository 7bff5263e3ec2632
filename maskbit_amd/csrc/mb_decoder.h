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
}  // namespace mb
