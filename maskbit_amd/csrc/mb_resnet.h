// The launchers of resnet.hip that are not inception.hip's: the input path and the distance of the ResNet-50 perceptual loss.  No allocation, no
// synchronisation, no handle: every buffer is the caller's.  The convolutions, the pool, the spatial mean and the head are mb_incep.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mb_common.h"

namespace mb {

constexpr int RN_SIDE = 224;              // the network's input resolution
constexpr int RN_IMGC = 4;                // channels of the normalised image buffer (3 + 1 zero: one 8-byte pixel)
constexpr int RN_MAXT = 12;               // taps per axis of the antialiased resize at most: 2 * 1024 / 224 + 1 = 10.2 -> 11
constexpr int RN_MIN_HW = 32, RN_MAX_HW = 1024;
constexpr int RN_STEM_K = 147;            // conv1 as a 1x1: the 3 x 7 x 7 patch, channel ci * 49 + ky * 7 + kx (the OIHW weight read as [64, 147])
constexpr int RN_STEM_C = 160;            // ... padded to whole 32-channel MFMA steps
constexpr float RN_BN_EPS = 1e-5f;
constexpr int RN_FEAT = 2048, RN_NCLASS = 1000;

inline int rn_stem_size(int n) { return (n - 1) / 2 + 1; }          // 7x7 stride 2 padding 3, and the 3x3 stride 2 padding 1 pool alike

// The per-axis tables of F.interpolate(size=224, mode="bilinear", antialias=True, align_corners=False) for an H x W source: weights fp32
// [2][224][RN_MAXT] (axis 0 = y), computed in double and normalised there; span int [2][224][2] = first source index, tap count.  One launch
void launch_resize_tables(hipStream_t s, float* weights, int* span, int H, int W);
// real / fake fp32 [B, 3, H, W] -> fp16 [2B, 224, 224, RN_IMGC], real images first: (resize(clamp01 ? clamp(x, 0, 1) : x) - mean_c) / std_c with
// mean_std = {mean[3], std[3]} on the device; fp32 accumulation, rows outer, columns inner, taps in ascending order; channel 3 is 0
void launch_resnet_resize(hipStream_t s, const float* real, const float* fake, const float* mean_std, const float* weights, const int* span, h16* out,
                          int B, int H, int W, int clamp01);
// img fp16 [N, S, S, RN_IMGC] -> fp16 [N, So, So, RN_STEM_C], So = rn_stem_size(S): the 7x7 stride-2 padding-3 patches (0 outside the image), 0 in the pad channels
void launch_stem_cols(hipStream_t s, const h16* img, h16* out, int N, int S);
// logits fp32 [2B, N]; feat fp16 [2B, F] or null (F % 8 == 0).  per_pair[b] = sum_i (l[b][i] - l[B + b][i])^2 / N (+ the same over feat / F), float64 in a
// fixed order; then, sum != null, *sum += per_pair[0 .. B) in pair order.  No atomics
void launch_resnet_distance(hipStream_t s, const float* logits, const h16* feat, int B, int N, size_t F, double* per_pair, double* sum);

}  // namespace mb
