// Decoder engine interface (decoder.hip) used by the C ABI in engine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/maskbit_hip.h"

namespace mb {
// codebook_size > 0: a lookup (VQ) handle with that many entries (mb_dec_create_vq); 0: the LFQ handle of mb_dec_create
mb_dec* dec_create(const mb_dec_cfg& cfg, int max_batch, std::string& err, int codebook_size = 0, int l2_normalize = 0);
void dec_destroy(mb_dec* d);
int dec_load(mb_dec* d, const char* name, const float* data, const int64_t* shape, int ndim, hipStream_t s, std::string& err);
int dec_decode(mb_dec* d, const int64_t* tokens, float* img_nchw, uint8_t* img_nhwc_u8, int B, hipStream_t s, std::string& err);
int dec_saturation_count(mb_dec* d, unsigned* count, bool reset, hipStream_t s);   // synchronises the stream
int dec_decode_latent(mb_dec* d, const float* z_nchw, float* img_nchw, uint8_t* img_nhwc_u8, int B, hipStream_t s, std::string& err);
int enc_encode_vq(mb_dec* d, const float* img, int64_t* indices, float* zq, float* zraw, float* row_dist, int B, hipStream_t s, std::string& err);
int enc_encode(mb_dec* d, const float* img, int64_t* indices, float* zq, float* zraw, int B, hipStream_t s, std::string& err);

// Single tokenizer layers on caller buffers (include/maskbit_hip_diag.h: mb_conv_layer, mb_groupnorm_stats, mb_avgpool2, mb_s2d): the handle's own
// launch_conv / launch_gn / weight repack on a scratch context.  They synchronise the stream (the scratch is freed on return).
struct ConvDiag {
  const void* in; const float* w; const float* bias; const float* gamma; const float* beta; const void* residual;
  void* out; float* img_nchw; uint8_t* img_u8;
  const float* out_gamma; const float* out_beta; float* out_scale_shift; float* out_part; int* part_tiles; unsigned* saturated;
  int B, H, W, Cin, Cout, ks, up, final_layer;
};
int diag_conv(const ConvDiag& q, hipStream_t s, std::string& err);
int diag_groupnorm(const void* x, const float* gamma, const float* beta, float* scale_shift, int B, int HW, int C, hipStream_t s, std::string& err);
int diag_pool(bool avg, const void* x, void* y, int B, int H, int W, int C, hipStream_t s, std::string& err);
}  // namespace mb
