// Spatial self-attention of the Taming VQGAN's AttnBlock (spatial_attention.hip): one head of 512 channels over the N = H W pixels of an image.
// Used by the Taming tokenizer handle (taming.hip) and by the diagnostic entry mb_spatial_attention (diag.hip).  No allocation, no synchronisation.
#pragma once
#include <hip/hip_runtime.h>

#include "mb_common.h"

namespace mb {

constexpr int SPATTN_C = 512;      // the head width (the block's channel count)

// out[b, i, :] = sum_j softmax_j(q[b, i] . k[b, j] * 512^-0.5) v[b, j, :] for B images of N pixels, N % 16 == 0, 16 <= N <= 1024.
// q, k, v: fp16 rows of 512 channels, pixel (b, i) at element (b N + i) * ld (ld % 8 == 0: the three may be slices of one fused projection's
// [B N, 1536] output); out: fp16 [B N] rows at stride ldo (ldo % 4 == 0).  *sat (or null) += the 4-channel output groups clamped at the fp16 range.
// Tiles are per image and nothing is accumulated across workgroups: the result of an image does not depend on B and is bit-stable run to run.
struct SpAttn {
  const h16 *q, *k, *v; h16* out; unsigned* sat;
  int B, N, ld, ldo;
};
// false (nothing launched) for a shape outside the above
bool launch_spatial_attention(hipStream_t s, const SpAttn& a);

}  // namespace mb
