// The launchers of discriminator.hip: what the VQGAN+ discriminator handle (mb_disc) and its single-launch diagnostic entries are made of.  No
// allocation, no synchronisation, no handle: every buffer is the caller's.  Activations are fp16 NHWC; the convolutions are mb_incep.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mb_common.h"

namespace mb {

constexpr int DISC_SIDE = 16;             // AdaptiveMaxPool2d((16, 16)): the map to_logits runs on
constexpr int DISC_NLOGIT = DISC_SIDE * DISC_SIDE;
constexpr int DISC_NSTAT = 5;             // per image: sum l, sum relu(1 - l), sum relu(1 + l), sum softplus(-l), sum softplus(l)
constexpr int DISC_COLS_K = 75;           // block_in's patch: 3 channels x 5 x 5, channel ci * 25 + ky * 5 + kx
constexpr int DISC_COLS_C = 96;           // ... padded to three 32-channel MFMA steps
constexpr double DISC_GN_EPS = 1e-5;      // torch.nn.GroupNorm's default (the tokenizers' GroupNorm has 1e-6: conv.hip)
constexpr float DISC_SLOPE = 0.1f;        // LeakyReLU(negative_slope=0.1)
constexpr int DISC_MAX_CHUNKS = 128;      // pixel chunks per image of the downsample's GroupNorm partials

// BlurBlock's "same" padding of one axis: the total, of which pad / 2 goes in front
inline int disc_blur_pad(int n, int k) { return std::max(((n + 1) / 2 - 1) * 2 + k - n, 0); }
// output size of the downsample: ceil(n / 2) for a blur (K = 3, 4, 5), floor(n / 2) for the average pool (K = 0)
inline int disc_down_size(int n, int K) { return K ? (n + 1) / 2 : n / 2; }
// pixel chunks per image of a downsample to Ho x Wo x C: a function of the map alone, so an image's partials do not depend on the batch.  A
// chunk is ceil(Ho Wo / chunks) pixels, so the last chunks of a map whose size the count does not divide may be short or empty (1030 pixels in
// 128 chunks of 9: 115 are used); an empty chunk's partials are written as zeros and add nothing
inline int disc_down_chunks(int Ho, int Wo, int C) {
  const size_t items = (size_t)Ho * Wo * (C / 8);
  return (int)std::min<size_t>(DISC_MAX_CHUNKS, std::max<size_t>(1, items / 2048));
}

// image fp32 [B, 3, H, W] (clamp01: clamped to [0, 1]) -> block_in's im2col fp16 [B, H, W, 96]: channel ci * 25 + ky * 5 + kx = pixel
// (y - 2 + ky, x - 2 + kx) of channel ci, 0 outside the image; channels 75 .. 95 = 0
void launch_disc_cols(hipStream_t s, const float* img, h16* out, int B, int H, int W, int clamp01);

// The stage's downsample: x fp16 [B, H, W, C] -> y fp16 [B, Ho, Wo, C] (C % 8 == 0, C <= 2048).  K = 3, 4, 5: BlurBlock -- the binomial kernel
// (1,2,1), (1,3,3,1), (1,4,6,4,1) outer-squared over 16, 64, 256, stride 2, zero "same" padding (disc_blur_pad); K = 0: AvgPool2d(2).  fp32
// accumulation, taps in (ky, kx) order, one rounding.  part (may be null; needs C % 32 == 0): float [B][disc_down_chunks][32][2] = the sum and
// the sum of squares of the fp32 values before rounding, per image, pixel chunk and GroupNorm group, in a fixed order without atomics.
void launch_disc_down(hipStream_t s, const h16* x, h16* y, float* part, int B, int H, int W, int C, int K);

// GroupNorm(32, C, eps) + affine + LeakyReLU(slope) in place on x fp16 [B, HW, C] (C % 32 == 0, C <= 2048): the statistics from `part`
// [B][nchunk][32][2] (combined in float64 in a fixed order), ss float2 [B][C] scratch for the per-channel (scale, shift);
// y = fp16(leaky(fma(x, scale, shift))).  *sat += the 8-channel groups clamped at the fp16 range.
void launch_disc_gn(hipStream_t s, h16* x, const float* part, int nchunk, const float* gamma, const float* beta, float2* ss, unsigned* sat, int B,
                    int HW, int C, double eps, float slope);

// AdaptiveMaxPool2d((16, 16)): x fp16 [B, H, W, C] -> y fp16 [B, 16, 16, C] (C % 8 == 0), window i of an axis of n = [floor(i n / 16), ceil((i + 1) n / 16))
void launch_disc_pool(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C);

// to_logits.2.weight fp32 [1, C, 5, 5] -> the logits kernel's [25][C]
void launch_disc_logits_weight(hipStream_t s, const float* w_oihw, float* out, int C);
// to_logits.2: the 5 x 5, C -> 1 convolution (zero padding 2) on x fp16 [B, 16, 16, C] (C % 8 == 0) with w fp32 [25][C] and bias fp32 [1]: four
// fp32 fma chains, each over a quarter of the channels (the first from the bias) and the in-image taps in (ky, kx) order, added in order.  logits (may be null) fp32 [B][256]; stats (may
// be null) double [B][5] = the five sums over the image's 256 logits, in a fixed order; sum (may be null) double [5] += stats in image order
// (needs stats).
void launch_disc_logits(hipStream_t s, const h16* x, const float* w, const float* bias, float* logits, double* stats, double* sum, int B, int C);

}  // namespace mb
