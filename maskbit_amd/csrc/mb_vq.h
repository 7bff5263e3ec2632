// Lookup (VQ) quantizer kernels (vq.hip): nearest-codeword search fused with its argmin, code -> latent gather and the latent pack of
// the lookup tokenizers (SimpleVectorizer, modeling/quantizer/quantizer.py:10-119), and the workspace a handle keeps for them.  Used by the tokenizer
// handles (decoder.hip, taming.hip) and by the diagnostic entry mb_vq_argmin (diag.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mb_abi.h"
#include "mb_common.h"

namespace mb {

constexpr int VQ_ROWS_WG = 128;    // z rows per search workgroup (4 waves x 2 row tiles of 16)
constexpr int VQ_CODES = 64;       // codebook entries per chunk (4 column tiles of 16)
constexpr int VQ_SPLIT_MAX = 64;   // codebook splits of one search (partials buffer: VQ_SPLIT_MAX x rows)

// The prepared codebook of a handle: fp32 rows (L2-normalised when l2), the same rows k-blocked for the search and their squared norms.
struct VqCodebook {
  int C = 0, K = 0, Kp = 0, Cpad = 0, l2 = 0;
  float* cb = nullptr;    // [C][K]
  float* cbT = nullptr;   // [Kp / 4][Cpad][4]: lane-contiguous operand of the f32 MFMA; padding rows / columns are zero
  float* cbn = nullptr;   // [Cpad] ||e||^2; +inf on padding rows (never selected)
};

inline int vq_kp(int K) { return K <= 64 ? 64 : K <= 128 ? 128 : 256; }
inline int vq_cpad(int C) { return (C + VQ_CODES - 1) / VQ_CODES * VQ_CODES; }
inline int vq_npad(int N) { return (N + VQ_ROWS_WG - 1) / VQ_ROWS_WG * VQ_ROWS_WG; }

// data: fp32 [C][K] (quantize.embedding.weight) -> cb / cbT / cbn
void vq_prep_codebook(const VqCodebook& q, const float* data, hipStream_t s);
// z rows (fp16 with a row stride, or fp32 [N][K]) -> zT [Kp / 4][Npad][4] fp32, L2-normalised when q.l2 (F.normalize, eps 1e-12);
// zraw (optional): the rows as given, fp32 NCHW with HW pixels per image
void vq_prep_rows(const VqCodebook& q, const h16* z16, int stride16, const float* z32, int N, int HW, float* zT, float* zraw, hipStream_t s);
// splits = 0: enough codebook splits that search workgroups x splits covers the device's CUs
int vq_splits(const VqCodebook& q, int N, int splits);
// argmin over the codebook of ||e||^2 - 2 z.e (ties -> lowest index), then idx, row_dist = sum_k (z_k - e_idx,k)^2 and zq (fp32 NCHW) per row.
// part_s / part_i: VQ_SPLIT_MAX x Npad partials.  idx / zq / row_dist may each be null.
void vq_search(const VqCodebook& q, const float* zT, int N, int HW, int splits, float* part_s, int* part_i, int64_t* idx, float* zq,
               float* row_dist, hipStream_t s);
// codes int64 [npix] -> fp16 NHWC latent [npix][cin_pad] (codes clamped to [0, C), channels >= K zero), saturating stores counted in *sat
void vq_gather(const VqCodebook& q, const int64_t* codes, size_t npix, h16* z, int cin_pad, unsigned* sat, hipStream_t s);
// fp32 NCHW latent [B][K][HW] -> fp16 NHWC [B*HW][cin_pad], saturating stores counted in *sat
void vq_pack_latent(const float* z, int B, int K, int HW, h16* out, int cin_pad, unsigned* sat, hipStream_t s);

// The lookup quantizer of a handle: the prepared codebook, the search buffers and whether quantize.embedding.weight has arrived
struct VqWorkspace {
  VqCodebook q;
  float* zT = nullptr;    // [Kp / 4][Npad][4] rows of the encoder output (normalised when l2)
  float* ps = nullptr;    // [VQ_SPLIT_MAX][Npad] per-split best score ...
  int* pi = nullptr;      // ... and its entry
  bool loaded = false;
  // C entries of K channels, searched for up to nlat rows at a time
  void alloc(DevArena& m, int C, int K, int l2, size_t nlat) {
    q.C = C; q.K = K; q.Kp = vq_kp(K); q.Cpad = vq_cpad(C); q.l2 = l2 ? 1 : 0;
    const size_t npad = (size_t)vq_npad((int)nlat);
    m.get(&q.cb, (size_t)C * K); m.get(&q.cbT, (size_t)q.Kp * q.Cpad); m.get(&q.cbn, (size_t)q.Cpad);
    m.get(&zT, (size_t)q.Kp * npad); m.get(&ps, VQ_SPLIT_MAX * npad); m.get(&pi, VQ_SPLIT_MAX * npad);
  }
  // quantize.embedding.weight, fp32 [C][K] on the device; false (and nothing done) for any other shape: the message is the handle's
  bool load_codebook(const int64_t* shape, int ndim, const float* data, hipStream_t s) {
    if (ndim != 2 || shape[0] != q.C || shape[1] != q.K) return false;
    vq_prep_codebook(q, data, s);
    return loaded = true;
  }
  // the end of an encode: z rows (fp16, `stride` apart, hw per image) -> idx, zq, zraw, row_dist as vq_prep_rows / vq_search write them
  void encode_rows(const h16* z16, int stride, int N, int hw, int64_t* idx, float* zq, float* zraw, float* row_dist, hipStream_t s) {
    vq_prep_rows(q, z16, stride, nullptr, N, hw, zT, zraw, s);
    vq_search(q, zT, N, hw, vq_splits(q, N, 0), ps, pi, idx, zq, row_dist, s);
  }
};

// Diagnostic (mb_vq_argmin): the whole search on caller buffers, z fp32 [N][K], w fp32 [C][K] codebook; temporaries are stream-ordered.
// 0, or the code of a fail() in that entry's name
int vq_argmin(const float* z, const float* w, int N, int C, int K, int l2, int splits, int64_t* idx, float* dist, hipStream_t s);

}  // namespace mb
