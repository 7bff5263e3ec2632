// Lookup (VQ) quantizer of ConvVQModel (SimpleVectorizer.forward / get_codebook_entry, modeling/quantizer/quantizer.py:45-119) on gfx950.
//
// Search: argmin_j ||z - e_j||^2 = argmin_j (||e_j||^2 - 2 z.e_j) (||z||^2 is constant per row), the distance GEMM on the f32-input MFMA
// (v_mfma_f32_16x16x4_f32: exact fp32 products and sums, the reference computes the same einsum in fp32) fused with a running (min, index) per
// row; the N x C distance matrix is never written.  A wave keeps 32 z rows in registers (two 16-row tiles, k-blocked so that one lane holds one
// element per k step) and streams the codebook in chunks of 64 entries straight from the k-blocked copy made at load time ([Kp/4][Cpad][4]:
// 16 entries x 4 k of a column tile are 256 contiguous bytes); the four waves of a workgroup read the same chunk (L1 / L2 hits).
// Small batches split the codebook across workgroups (grid.y); every split writes its (score, index) per row to a partials buffer and the
// finalize pass reduces them in split order -- no float atomics.  The score of an entry does not depend on which split computed it, and the
// reduction keeps the lowest index among equal scores (torch.argmin), so index and distance are bit-identical for any split count and any
// batch composition.  The finalize pass recomputes the chosen entry's squared distance exactly (sequential fp32) and writes zq.
#include <algorithm>
#include <cmath>

#include "mb_abi.h"
#include "mb_vq.h"

namespace mb {

namespace {

__device__ __forceinline__ bool vq_better(float s, int i, float bs, int bi) { return s < bs || (s == bs && i < bi); }

template <int KQ>
__global__ __launch_bounds__(256) void vq_search_kernel(const float* __restrict__ zT, const float* __restrict__ cbT, const float* __restrict__ cbn,
                                                        int Npad, int Cpad, int splits, float* __restrict__ part_s, int* __restrict__ part_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.x * VQ_ROWS_WG + wave * 32;
  const int split = blockIdx.y, nchunk = Cpad / VQ_CODES;
  const int c_begin = (int)((long long)split * nchunk / splits), c_end = (int)((long long)(split + 1) * nchunk / splits);
  // A operand: lane (l15, g) holds z[row0 + 16 t + l15][4 q + g]
  float za[2][KQ];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < KQ; ++q) za[t][q] = zT[((size_t)q * Npad + row0 + t * 16 + l15) * 4 + g];
  float best[2][4];
  int bidx[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { best[t][r] = INFINITY; bidx[t][r] = 0x7fffffff; }
  for (int c = c_begin; c < c_end; ++c) {
    const int code0 = c * VQ_CODES;
    f32x4 acc[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // B operand: lane (l15, g) holds e[code0 + 16 j + l15][4 q + g]
    const float* eb = cbT + (size_t)(code0 + l15) * 4 + g;
#pragma unroll
    for (int q = 0; q < KQ; ++q) {
      float e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = eb[(size_t)q * Cpad * 4 + j * 64];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[t][q], e[j], acc[t][j], 0, 0, 0);
    }
    // D: lane (l15, g) holds row 16 t + 4 g + r against entry code0 + 16 j + l15; entries visited in increasing order, strict < keeps the lowest
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int code = code0 + j * 16 + l15;
      const float en = cbn[code];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = fmaf(-2.0f, acc[t][j][r], en);
          if (s < best[t][r]) { best[t][r] = s; bidx[t][r] = code; }
        }
    }
  }
  // the 16 lanes of a row group hold different entries of the same rows
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float os = __shfl_xor(best[t][r], o);
        const int oi = __shfl_xor(bidx[t][r], o);
        if (vq_better(os, oi, best[t][r], bidx[t][r])) { best[t][r] = os; bidx[t][r] = oi; }
      }
      if (l15 == 0) {
        const size_t o = (size_t)split * Npad + row0 + t * 16 + g * 4 + r;
        part_s[o] = best[t][r];
        part_i[o] = bidx[t][r];
      }
    }
}

__global__ void vq_finalize_kernel(const float* __restrict__ zT, const float* __restrict__ cb, const float* __restrict__ part_s,
                                   const int* __restrict__ part_i, int N, int Npad, int HW, int C, int K, int splits, int64_t* __restrict__ idx,
                                   float* __restrict__ zq, float* __restrict__ row_dist) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= N) return;
  float bs = INFINITY;
  int bi = 0x7fffffff;
  for (int sp = 0; sp < splits; ++sp) {                 // split order = increasing entries
    const float s = part_s[(size_t)sp * Npad + row];
    const int i = part_i[(size_t)sp * Npad + row];
    if (vq_better(s, i, bs, bi)) { bs = s; bi = i; }
  }
  if (bi < 0 || bi >= C) bi = 0;                        // every score NaN / inf
  const float* e = cb + (size_t)bi * K;
  float dist = 0.f;
  for (int k = 0; k < K; ++k) {
    const float d = zT[((size_t)(k >> 2) * Npad + row) * 4 + (k & 3)] - e[k];
    dist = fmaf(d, d, dist);
  }
  if (idx) idx[row] = bi;
  if (row_dist) row_dist[row] = dist;
  if (zq) {
    const int b = row / HW, yx = row - b * HW;
    for (int k = 0; k < K; ++k) zq[((size_t)b * K + k) * HW + yx] = e[k];
  }
}

// one thread per row: fp16 (row stride stride16) or fp32 [N][K] input -> k-blocked fp32 [Kp/4][Npad][4], normalised when l2
__global__ void vq_prep_rows_kernel(const h16* __restrict__ z16, int stride16, const float* __restrict__ z32, int N, int Npad, int K, int Kp,
                                    int HW, int l2, float* __restrict__ zT, float* __restrict__ zraw) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= Npad) return;
  auto in = [&](int k) -> float { return z16 ? (float)z16[(size_t)row * stride16 + k] : z32[(size_t)row * K + k]; };
  float nrm = 1.f;
  if (row < N && l2) {
    float ss = 0.f;
    for (int k = 0; k < K; ++k) { const float v = in(k); ss = fmaf(v, v, ss); }
    nrm = fmaxf(sqrtf(ss), 1e-12f);                     // F.normalize(dim=-1): x / max(||x||, eps)
  }
  const int b = row / HW, yx = row - b * HW;
  for (int k = 0; k < Kp; ++k) {
    float v = 0.f;
    if (row < N && k < K) {
      const float raw = in(k);
      if (zraw) zraw[((size_t)b * K + k) * HW + yx] = raw;
      v = l2 ? raw / nrm : raw;
    }
    zT[((size_t)(k >> 2) * Npad + row) * 4 + (k & 3)] = v;
  }
}

__global__ void vq_prep_codebook_kernel(const float* __restrict__ w, int C, int Cpad, int K, int Kp, int l2, float* __restrict__ cb,
                                        float* __restrict__ cbT, float* __restrict__ cbn) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= Cpad) return;
  float nrm = 1.f;
  if (c < C && l2) {
    float ss = 0.f;
    for (int k = 0; k < K; ++k) { const float v = w[(size_t)c * K + k]; ss = fmaf(v, v, ss); }
    nrm = fmaxf(sqrtf(ss), 1e-12f);
  }
  float n2 = 0.f;
  for (int k = 0; k < Kp; ++k) {
    float v = 0.f;
    if (c < C && k < K) {
      v = l2 ? w[(size_t)c * K + k] / nrm : w[(size_t)c * K + k];
      cb[(size_t)c * K + k] = v;
      n2 = fmaf(v, v, n2);
    }
    cbT[((size_t)(k >> 2) * Cpad + c) * 4 + (k & 3)] = v;
  }
  cbn[c] = c < C ? n2 : INFINITY;
}

__global__ void vq_gather_kernel(const int64_t* __restrict__ codes, const float* __restrict__ cb, size_t npix, int C, int K, int cin_pad,
                                 h16* __restrict__ z, unsigned* __restrict__ sat) {
  unsigned nsat = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix * cin_pad; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i / cin_pad;
    const int c = (int)(i - p * cin_pad);
    float v = 0.f;
    if (c < K) {
      int64_t code = codes[p];
      code = code < 0 ? 0 : code >= C ? C - 1 : code;   // device-resident codes are clamped (the host checks host-resident ones)
      v = cb[(size_t)code * K + c];
    }
    nsat += fabsf(v) > MB_H16_MAX ? 1u : 0u;
    z[i] = to_h(v);
  }
  if (nsat) atomicAdd(sat, nsat);
}

__global__ void vq_pack_kernel(const float* __restrict__ zin, int B, int K, int HW, int cin_pad, h16* __restrict__ out, unsigned* __restrict__ sat) {
  unsigned nsat = 0;
  const size_t npix = (size_t)B * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix * cin_pad; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i / cin_pad;
    const int c = (int)(i - p * cin_pad);
    float v = 0.f;
    if (c < K) {
      const size_t b = p / HW, yx = p - b * HW;
      v = zin[(b * K + c) * HW + yx];
    }
    nsat += fabsf(v) > MB_H16_MAX ? 1u : 0u;
    out[i] = to_h(v);
  }
  if (nsat) atomicAdd(sat, nsat);
}

int device_cus() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
  return n;
}

}  // namespace

void vq_prep_codebook(const VqCodebook& q, const float* data, hipStream_t s) {
  hipLaunchKernelGGL(vq_prep_codebook_kernel, dim3((q.Cpad + 255) / 256), dim3(256), 0, s, data, q.C, q.Cpad, q.K, q.Kp, q.l2, q.cb, q.cbT, q.cbn);
}

void vq_prep_rows(const VqCodebook& q, const h16* z16, int stride16, const float* z32, int N, int HW, float* zT, float* zraw, hipStream_t s) {
  const int Npad = vq_npad(N);
  hipLaunchKernelGGL(vq_prep_rows_kernel, dim3((Npad + 255) / 256), dim3(256), 0, s, z16, stride16, z32, N, Npad, q.K, q.Kp, HW, q.l2, zT, zraw);
}

int vq_splits(const VqCodebook& q, int N, int splits) {
  const int nchunk = q.Cpad / VQ_CODES, nwg = vq_npad(N) / VQ_ROWS_WG;
  if (splits <= 0) {
    static const int cus = device_cus();
    splits = (cus + nwg - 1) / nwg;
  }
  return std::max(1, std::min(std::min(splits, nchunk), VQ_SPLIT_MAX));
}

void vq_search(const VqCodebook& q, const float* zT, int N, int HW, int splits, float* part_s, int* part_i, int64_t* idx, float* zq,
               float* row_dist, hipStream_t s) {
  const int Npad = vq_npad(N);
  const dim3 grid(Npad / VQ_ROWS_WG, splits);
  if (q.Kp == 64) hipLaunchKernelGGL(vq_search_kernel<16>, grid, dim3(256), 0, s, zT, q.cbT, q.cbn, Npad, q.Cpad, splits, part_s, part_i);
  else if (q.Kp == 128) hipLaunchKernelGGL(vq_search_kernel<32>, grid, dim3(256), 0, s, zT, q.cbT, q.cbn, Npad, q.Cpad, splits, part_s, part_i);
  else hipLaunchKernelGGL(vq_search_kernel<64>, grid, dim3(256), 0, s, zT, q.cbT, q.cbn, Npad, q.Cpad, splits, part_s, part_i);
  hipLaunchKernelGGL(vq_finalize_kernel, dim3((N + 255) / 256), dim3(256), 0, s, zT, q.cb, part_s, part_i, N, Npad, HW, q.C, q.K, splits, idx, zq,
                     row_dist);
}

void vq_gather(const VqCodebook& q, const int64_t* codes, size_t npix, h16* z, int cin_pad, unsigned* sat, hipStream_t s) {
  hipLaunchKernelGGL(vq_gather_kernel, dim3((unsigned)std::min<size_t>(4096, (npix * cin_pad + 255) / 256)), dim3(256), 0, s, codes, q.cb, npix, q.C,
                     q.K, cin_pad, z, sat);
}

void vq_pack_latent(const float* z, int B, int K, int HW, h16* out, int cin_pad, unsigned* sat, hipStream_t s) {
  const size_t n = (size_t)B * HW * cin_pad;
  hipLaunchKernelGGL(vq_pack_kernel, dim3((unsigned)std::min<size_t>(4096, (n + 255) / 256)), dim3(256), 0, s, z, B, K, HW, cin_pad, out, sat);
}

int vq_argmin(const float* z, const float* w, int N, int C, int K, int l2, int splits, int64_t* idx, float* dist, hipStream_t s) {
  if (N < 1 || C < 2 || C > 65536 || K < 1 || K > 256) return fail(-1, "mb_vq_argmin: N >= 1, C in [2, 65536], K in [1, 256] required");
  VqCodebook q;
  q.C = C; q.K = K; q.Kp = vq_kp(K); q.Cpad = vq_cpad(C); q.l2 = l2 ? 1 : 0;
  const int Npad = vq_npad(N);
  splits = vq_splits(q, N, splits);
  float *zT = nullptr, *ps = nullptr;
  int* pi = nullptr;
  bool ok = hipMallocAsync((void**)&q.cb, (size_t)C * K * sizeof(float), s) == hipSuccess &&
            hipMallocAsync((void**)&q.cbT, (size_t)q.Kp * q.Cpad * sizeof(float), s) == hipSuccess &&
            hipMallocAsync((void**)&q.cbn, (size_t)q.Cpad * sizeof(float), s) == hipSuccess &&
            hipMallocAsync((void**)&zT, (size_t)q.Kp * Npad * sizeof(float), s) == hipSuccess &&
            hipMallocAsync((void**)&ps, (size_t)splits * Npad * sizeof(float), s) == hipSuccess &&
            hipMallocAsync((void**)&pi, (size_t)splits * Npad * sizeof(int), s) == hipSuccess;
  if (ok) {
    vq_prep_codebook(q, w, s);
    vq_prep_rows(q, nullptr, 0, z, N, N, zT, nullptr, s);
    vq_search(q, zT, N, N, splits, ps, pi, idx, nullptr, dist, s);
  }
  for (void* p : {(void*)q.cb, (void*)q.cbT, (void*)q.cbn, (void*)zT, (void*)ps, (void*)pi})
    if (p) (void)hipFreeAsync(p, s);
  return ok ? 0 : fail(-10, "mb_vq_argmin: device allocation failed");
}

}  // namespace mb
