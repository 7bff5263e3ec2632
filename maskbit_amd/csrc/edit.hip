// Image editing with the masked-token sampler (inpainting, outpainting, regenerating a region under another label): the helpers in front of and
// behind a sampling run that starts from a partly known token map (mb_sample_edit, sampler.hip; the per-sample threshold rule is the <true> form of
// sample_thresh_kernel, sampling.hip).  The reference has no counterpart: its sample() always starts from the all-masked state (sampling.py:65-71).
//   edit_token_mask_kernel -- pixel mask -> token mask: a token is regenerated if any pixel of its stride x stride block is.
//   edit_init_kernel       -- the encoder's codes + the token mask -> grouped tokens with the mask token at the slots to regenerate, and their count.
//   edit_load_kernel       -- a caller's grouped tokens -> the engine's token state (clamped to [0, C]) and the count of mask tokens per sample.
//   edit_composite_kernel  -- generated and original image + pixel mask -> the image that keeps the original pixels outside the mask, as fp32 NCHW
//                             and / or uint8 NHWC (the decoder's own conversion, conv.hip: trunc(clamp(x, 0, 1) * 255)).
// Stateless: the caller owns every buffer; nothing is allocated, nothing synchronises.
#include <algorithm>

#include "../../include/maskbit_hip.h"
#include "mb_abi.h"
#include "mb_kernels.h"

namespace mb {

namespace {

constexpr int ED_THREADS = 256;

// Sum of one int per thread over an ED_THREADS workgroup, valid in thread 0: wave sums, then the four partials in wave order -- integer, so the same
// value whatever the order, and no atomics.
__device__ __forceinline__ int block_count(int mine, int* part /* LDS [ED_THREADS / 64] */) {
  mine = (int)wave_sum((float)mine);                  // (<= 8192 slots per sample: exact in fp32)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  int total = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < ED_THREADS / 64; ++w) total += part[w];
  return total;
}

__global__ __launch_bounds__(ED_THREADS) void edit_load_kernel(const int64_t* __restrict__ src, int64_t* __restrict__ dst, int* __restrict__ num_regen, int P, int C) {
  __shared__ int part[ED_THREADS / 64];
  const size_t base = (size_t)blockIdx.x * P;
  int mine = 0;
  for (int p = threadIdx.x; p < P; p += ED_THREADS) {
    int64_t t = src[base + p];
    t = t < 0 ? 0 : (t > C ? (int64_t)C : t);         // device-resident tokens are not range-checked on the host: out-of-range values must not index the embedding tables
    mine += t == C;
    if (dst) dst[base + p] = t;
  }
  const int total = block_count(mine, part);
  if (threadIdx.x == 0) num_regen[blockIdx.x] = total;
}

__global__ __launch_bounds__(ED_THREADS) void edit_init_kernel(const int64_t* __restrict__ codes, const uint8_t* __restrict__ regen, int64_t* __restrict__ tokens,
                                                               int* __restrict__ num_regen, int n, int m, int gbits) {
  __shared__ int part[ED_THREADS / 64];
  const int P = n * m, C = 1 << gbits;
  const size_t base = (size_t)blockIdx.x * P;
  int mine = 0;
  for (int p = threadIdx.x; p < P; p += ED_THREADS) {
    const int pos = p / m, g = p - pos * m;
    const bool r = regen[base + p] != 0;
    const int64_t code = codes[(size_t)blockIdx.x * n + pos];
    tokens[base + p] = r ? (int64_t)C : ((code >> (g * gbits)) & (int64_t)(C - 1));   // split_factorized_tokens (factorization.py:27-44), kept integral
    mine += r;
  }
  const int total = block_count(mine, part);
  if (threadIdx.x == 0) num_regen[blockIdx.x] = total;
}

// One thread per token cell: st rows of st mask bytes, each row read in pieces of VB = min(st, 16) bytes (one load); neighbouring lanes read
// neighbouring pieces of the same pixel rows.
template <typename V> __device__ __forceinline__ bool any_set(V v) { return v != 0; }
template <> __device__ __forceinline__ bool any_set<uint4>(uint4 v) { return (v.x | v.y | v.z | v.w) != 0; }

template <typename V>
__global__ __launch_bounds__(ED_THREADS) void edit_token_mask_kernel(const uint8_t* __restrict__ pm, uint8_t* __restrict__ tm, size_t cells, int H, int W, int st) {
  const int hs = H / st, ws = W / st, pieces = st / (int)sizeof(V);
  for (size_t i = (size_t)blockIdx.x * ED_THREADS + threadIdx.x; i < cells; i += (size_t)gridDim.x * ED_THREADS) {
    const int x = (int)(i % ws), y = (int)((i / ws) % hs);
    const size_t b = i / ((size_t)ws * hs);
    const uint8_t* row = pm + (b * H + (size_t)y * st) * W + (size_t)x * st;
    bool any = false;
    for (int r = 0; r < st; ++r, row += W)
      for (int q = 0; q < pieces; ++q) any |= any_set(((const V*)row)[q]);
    tm[i] = any ? 1 : 0;
  }
}

// One thread per 4 consecutive pixels of a row, all CH channels: one 4-byte mask load, a float4 of each input per channel, a float4 store per channel
// and CH dwords of packed bytes (4 pixels x CH channels are 4 CH consecutive bytes of the NHWC image).
template <int CH>
__global__ __launch_bounds__(ED_THREADS) void edit_composite_kernel(const float* __restrict__ gen, const float* __restrict__ orig, const uint8_t* __restrict__ pm,
                                                                    float* __restrict__ out, uint8_t* __restrict__ out_u8, size_t quads, int H, int W) {
  const size_t plane = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.x * ED_THREADS + threadIdx.x; i < quads; i += (size_t)gridDim.x * ED_THREADS) {
    const size_t pix = i * 4, b = pix / plane, off = pix - b * plane;       // (W % 4 == 0: the four pixels share a row)
    const uint32_t mk = *(const uint32_t*)(pm + pix);
    uint32_t bytes[CH] = {};
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const size_t at = (b * CH + c) * plane + off;
      const float4 gv = *(const float4*)(gen + at), ov = *(const float4*)(orig + at);
      float4 v;
      v.x = (mk & 0xffu) ? gv.x : ov.x;
      v.y = (mk & 0xff00u) ? gv.y : ov.y;
      v.z = (mk & 0xff0000u) ? gv.z : ov.z;
      v.w = (mk & 0xff000000u) ? gv.w : ov.w;
      if (out) *(float4*)(out + at) = v;
      const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t u = (uint32_t)(uint8_t)(fminf(fmaxf(e[j], 0.f), 1.f) * 255.0f);
        const int at8 = j * CH + c;                                        // byte of (pixel j, channel c) among the 4 CH
        bytes[at8 >> 2] |= u << ((at8 & 3) * 8);
      }
    }
    if (out_u8) {
      uint32_t* dst = (uint32_t*)(out_u8 + pix * CH);
#pragma unroll
      for (int w = 0; w < CH; ++w) dst[w] = bytes[w];
    }
  }
}

inline unsigned grid_for(size_t items) { return (unsigned)std::min<size_t>(4096, (items + ED_THREADS - 1) / ED_THREADS); }

}  // namespace

void edit_load_tokens(hipStream_t s, const int64_t* src, int64_t* dst, int* num_regen, int B, int P, int C) {
  hipLaunchKernelGGL(edit_load_kernel, dim3(B), dim3(ED_THREADS), 0, s, src, dst, num_regen, P, C);
}

void edit_init(hipStream_t s, const int64_t* codes, const uint8_t* regen, int64_t* tokens, int* num_regen, int B, int n, int m, int gbits) {
  hipLaunchKernelGGL(edit_init_kernel, dim3(B), dim3(ED_THREADS), 0, s, codes, regen, tokens, num_regen, n, m, gbits);
}

void edit_token_mask(hipStream_t s, const uint8_t* pm, uint8_t* tm, int B, int H, int W, int st) {
  const size_t cells = (size_t)B * (H / st) * (W / st);
  const dim3 grid(grid_for(cells)), block(ED_THREADS);
  if (st == 1) hipLaunchKernelGGL(edit_token_mask_kernel<uint8_t>, grid, block, 0, s, pm, tm, cells, H, W, st);
  else if (st == 2) hipLaunchKernelGGL(edit_token_mask_kernel<uint16_t>, grid, block, 0, s, pm, tm, cells, H, W, st);
  else if (st == 4) hipLaunchKernelGGL(edit_token_mask_kernel<uint32_t>, grid, block, 0, s, pm, tm, cells, H, W, st);
  else if (st == 8) hipLaunchKernelGGL(edit_token_mask_kernel<uint64_t>, grid, block, 0, s, pm, tm, cells, H, W, st);
  else hipLaunchKernelGGL(edit_token_mask_kernel<uint4>, grid, block, 0, s, pm, tm, cells, H, W, st);
}

int edit_composite(hipStream_t s, const float* gen, const float* orig, const uint8_t* pm, float* out, uint8_t* out_u8, int B, int C, int H, int W) {
  if (C < 1 || C > 4 || W % 4) return -1;
  const size_t quads = (size_t)B * H * W / 4;
  const dim3 grid(grid_for(quads)), block(ED_THREADS);
  if (C == 1) hipLaunchKernelGGL(edit_composite_kernel<1>, grid, block, 0, s, gen, orig, pm, out, out_u8, quads, H, W);
  else if (C == 2) hipLaunchKernelGGL(edit_composite_kernel<2>, grid, block, 0, s, gen, orig, pm, out, out_u8, quads, H, W);
  else if (C == 3) hipLaunchKernelGGL(edit_composite_kernel<3>, grid, block, 0, s, gen, orig, pm, out, out_u8, quads, H, W);
  else hipLaunchKernelGGL(edit_composite_kernel<4>, grid, block, 0, s, gen, orig, pm, out, out_u8, quads, H, W);
  return 0;
}

}  // namespace mb

using namespace mb;

extern "C" {

int mb_edit_init(const int64_t* codes, const uint8_t* regen_mask, int64_t* tokens, int32_t* num_regen, int B, int n, int m, int C, mb_stream stream) {
  if (!codes || !regen_mask || !tokens || !num_regen) return fail(-1, "mb_edit_init: null argument");
  if (B <= 0 || n <= 0 || m <= 0 || C < 2 || C > 4096 || (C & (C - 1))) return fail(-1, "mb_edit_init: bad sizes (B = %d, n = %d, m = %d, C = %d: a power of two up to 4096)", B, n, m, C);
  int gbits = 0;
  while ((1 << gbits) < C) ++gbits;
  if ((size_t)n * m > 8192) return fail(-1, "mb_edit_init: n * m = %zu exceeds the step kernel's 8192 positions", (size_t)n * m);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("edit_init", s);
  edit_init(s, codes, regen_mask, tokens, num_regen, B, n, m, gbits);
  return launched();
}

int mb_edit_token_mask(const uint8_t* pixel_mask, uint8_t* token_mask, int B, int H, int W, int stride, mb_stream stream) {
  if (!pixel_mask || !token_mask) return fail(-1, "mb_edit_token_mask: null argument");
  if (B <= 0 || H <= 0 || W <= 0 || stride <= 0 || (stride & (stride - 1)) || H % stride || W % stride)
    return fail(-1, "mb_edit_token_mask: the stride (%d) must be a power of two that divides H and W (%d x %d)", stride, H, W);
  if ((uintptr_t)pixel_mask % (stride < 16 ? stride : 16)) return fail(-1, "mb_edit_token_mask: the pixel mask must be aligned to min(stride, 16) bytes");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("edit_token_mask", s);
  edit_token_mask(s, pixel_mask, token_mask, B, H, W, stride);
  return launched();
}

int mb_edit_composite(const float* gen_nchw, const float* orig_nchw, const uint8_t* pixel_mask, float* out_nchw, uint8_t* out_nhwc_u8, int B, int C, int H,
                      int W, mb_stream stream) {
  if (!gen_nchw || !orig_nchw || !pixel_mask) return fail(-1, "mb_edit_composite: null argument");
  if (!out_nchw && !out_nhwc_u8) return fail(-1, "mb_edit_composite: no output requested");
  if (B <= 0 || H <= 0 || W <= 0) return fail(-1, "mb_edit_composite: bad sizes");
  if (((uintptr_t)gen_nchw | (uintptr_t)orig_nchw | (uintptr_t)out_nchw) % 16 || ((uintptr_t)pixel_mask | (uintptr_t)out_nhwc_u8) % 4)
    return fail(-1, "mb_edit_composite: the fp32 images must be 16-byte aligned, the mask and the uint8 image 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("edit_composite", s);
  if (edit_composite(s, gen_nchw, orig_nchw, pixel_mask, out_nchw, out_nhwc_u8, B, C, H, W))
    return fail(-1, "mb_edit_composite: 1 .. 4 channels and a width that is a multiple of 4 required (got %d channels, width %d)", C, W);
  return launched();
}

}  // extern "C"
