// The fp32 reference mode's kernels (mb_gen_cfg.precision = MB_PREC_F32): a GEMM and an attention with every operand, product and sum in fp32.
//   gemm_f32      : out[M,N] = epi(A[M,K] . W[N,K]^T + bias) on the f32-input MFMA (v_mfma_f32_32x32x2_f32), LDS-tiled 128 x 128 x 32
//   attention_f32 : softmax(Q K^T / sqrt(dh)) V per (sequence, head) on the VALU, keys streamed in tiles with a running max and sum
// Neither is tuned past "tiled and correct": the mode is an instrument (maskbit_amd/checkpoint_check.py), not a product path.
//
// NUMERICAL CONTRACT of gemm_f32.  Every output element is
//     acc = 0;  for k = 0 .. K-1:  acc = fmaf(A[m,k], W[n,k], acc);      one chain, ascending k, continued across K-tiles in the same accumulator
//     v = acc + bias[n];                                                  one fp32 add
//     out = v | gelu_erf(v) | v + residual[m,n] | v                       the epilogue
// The f32-input MFMA is bit for bit that chain (one rounding per product-and-add, no wider internal sum); there is no split-K and no reordering, so
// an output element does not depend on the tile it falls in, on M, or on the grid.  K-tile padding multiplies 0 by 0 and adds it: acc + 0 = acc.
#include "mb_kernels.h"

namespace mb {

namespace {

constexpr int FB = 128;    // block tile: FB x FB outputs, four waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32)
constexpr int FBK = 32;    // K-tile
constexpr int FLD = 36;    // LDS row stride (floats): 16-byte aligned rows, consecutive rows four banks apart

using f32x16 = __attribute__((ext_vector_type(16))) float;

// A K-tile row in LDS is stored k-PERMUTED: element k at position (k & 1) * 16 + (k >> 1).  MFMA step s multiplies k = 2s (lanes 0-31) and k = 2s + 1
// (lanes 32-63), so lane half h needs k = h, 2 + h, 4 + h, ...: with the permutation those are the 16 CONSECUTIVE floats at h * 16, four ds_read_b128.
__device__ __forceinline__ void stage_store(float* tile, int row, int kq, const float4& v) {
  *(float2*)(tile + row * FLD + 2 * kq) = make_float2(v.x, v.z);
  *(float2*)(tile + row * FLD + 16 + 2 * kq) = make_float2(v.y, v.w);
}

// global -> registers: 128 rows x 8 float4 per operand = 4 float4 per thread each; a row or a k past the edge is not read (zero)
__device__ __forceinline__ void stage_fetch(const GemmF32Args& a, float4* ra, float4* rw, int tid, int m0, int n0, int kt) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = tid + 256 * r, row = i >> 3, k = kt * FBK + (i & 7) * 4;
    const bool kin = k < a.K;                            // (K % 4 == 0: a float4 is inside or outside as a whole)
    ra[r] = (kin && m0 + row < a.M) ? *(const float4*)(a.A + (size_t)(m0 + row) * a.K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    rw[r] = (kin && n0 + row < a.N) ? *(const float4*)(a.W + (size_t)(n0 + row) * a.K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ float gelu_erf_f32(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmF32Args a) {
  __shared__ __attribute__((aligned(16))) float As[FB * FLD];
  __shared__ __attribute__((aligned(16))) float Ws[FB * FLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int ntn = (a.N + FB - 1) / FB;
  const int mt = blockIdx.x / ntn, nt = blockIdx.x - mt * ntn;
  const int m0 = mt * FB, n0 = nt * FB;
  const int nkt = (a.K + FBK - 1) / FBK;

  float4 ra[4], rw[4];                                   // the next K-tile on its way from global memory to LDS

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  stage_fetch(a, ra, rw, tid, m0, n0, 0);
  const int l31 = lane & 31, half = lane >> 5;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();                                     // the previous K-tile has been read
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = tid + 256 * r;
      stage_store(As, i >> 3, i & 7, ra[r]);
      stage_store(Ws, i >> 3, i & 7, rw[r]);
    }
    __syncthreads();
    if (kt + 1 < nkt) stage_fetch(a, ra, rw, tid, m0, n0, kt + 1);                   // in flight under this tile's MFMAs
#pragma unroll
    for (int q = 0; q < 4; ++q) {                        // four MFMA steps (8 k) per quarter
      float4 fa[2], fw[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        fa[t] = *(const float4*)(As + (wm * 64 + t * 32 + l31) * FLD + half * 16 + q * 4);
        fw[t] = *(const float4*)(Ws + (wn * 64 + t * 32 + l31) * FLD + half * 16 + q * 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float av = e == 0 ? fa[i].x : e == 1 ? fa[i].y : e == 2 ? fa[i].z : fa[i].w;
            const float wv = e == 0 ? fw[j].x : e == 1 ? fw[j].y : e == 2 ? fw[j].z : fw[j].w;
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wv, acc[i][j], 0, 0, 0);
          }
      }
    }
  }

  // epilogue: C/D map of the 32 x 32 MFMA -- column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 64 + j * 32 + l31;
      if (n >= a.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= a.M) continue;
        size_t orow = (size_t)m;
        const float* brow = a.bias;
        if (a.epi == F32_EPI_LOGITS) {
          const int sq = m / a.period, pos = m - sq * a.period;
          if (pos == a.period - 1) continue;             // the class-token row is not a prediction
          orow = (size_t)sq * (a.period - 1) + pos;
          if (a.bias_per_pos) brow = a.bias + (size_t)pos * a.N;
        }
        float v = acc[i][j][r] + brow[n];
        if (a.epi == F32_EPI_GELU) v = gelu_erf_f32(v);
        else if (a.epi == F32_EPI_RES) v = v + a.residual[(size_t)m * a.N + n];   // (out may alias residual: each element is read and written by one lane)
        a.out[orow * a.N + n] = v;
      }
    }
}

// ---- attention -------------------------------------------------------------------------------------------------------------------------------
// One wave per 64 queries of a (sequence, head); a lane owns one query: its pre-scaled q row and its output row live in registers.  Keys and values
// are streamed through LDS in tiles of AKT; every lane reads the same K / V element at a time (LDS broadcast), so the tiles need no padding.  Per
// tile: the lane's AKT scores, the running max m and the rescale exp(m_old - m_new) of (sum, output), then p_j = exp(s_j - m) into both.  A ragged
// last tile is a shorter loop, not a mask; lanes past the last query compute the last query again and store nothing.
constexpr int AKT = 16;

template <int DH>
__global__ __launch_bounds__(64) void attention_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int d, int heads, int qtiles) {
  __shared__ __attribute__((aligned(16))) float Ks[AKT * DH];
  __shared__ __attribute__((aligned(16))) float Vs[AKT * DH];
  const int lane = threadIdx.x;
  const int qt = blockIdx.x % qtiles, sh = blockIdx.x / qtiles;
  const int h = sh % heads, seq = sh / heads;
  const size_t rs = (size_t)3 * d;
  const float* base = qkv + (size_t)seq * N * rs + (size_t)h * DH;
  const int qi = qt * 64 + lane, qr = qi < N ? qi : N - 1;
  const float scale = 1.0f / sqrtf((float)DH);
  float q[DH], o[DH];
#pragma unroll
  for (int c = 0; c < DH; c += 4) {
    const float4 v = *(const float4*)(base + (size_t)qr * rs + c);
    q[c] = v.x * scale; q[c + 1] = v.y * scale; q[c + 2] = v.z * scale; q[c + 3] = v.w * scale;
    o[c] = o[c + 1] = o[c + 2] = o[c + 3] = 0.f;
  }
  float mx = -INFINITY, sum = 0.f;
  for (int k0 = 0; k0 < N; k0 += AKT) {
    const int kc = N - k0 < AKT ? N - k0 : AKT;          // keys of this tile (wave-uniform)
    __syncthreads();
    constexpr int V4 = DH / 4;                            // float4 per row
#pragma unroll
    for (int i = lane; i < AKT * V4; i += 64) {
      const int row = i / V4, c = (i - row * V4) * 4;
      if (row < kc) {
        *(float4*)(Ks + row * DH + c) = *(const float4*)(base + (size_t)(k0 + row) * rs + d + c);
        *(float4*)(Vs + row * DH + c) = *(const float4*)(base + (size_t)(k0 + row) * rs + 2 * d + c);
      }
    }
    __syncthreads();
    float s[AKT];
    float tmax = -INFINITY;
#pragma unroll
    for (int j = 0; j < AKT; ++j) {
      float acc = 0.f;
      if (j < kc) {
#pragma unroll
        for (int c = 0; c < DH; c += 4) {
          const float4 kv = *(const float4*)(Ks + j * DH + c);
          acc = fmaf(q[c], kv.x, acc); acc = fmaf(q[c + 1], kv.y, acc); acc = fmaf(q[c + 2], kv.z, acc); acc = fmaf(q[c + 3], kv.w, acc);
        }
        tmax = fmaxf(tmax, acc);
      }
      s[j] = acc;
    }
    const float mnew = fmaxf(mx, tmax);
    const float alpha = expf(mx - mnew);                 // first tile: exp(-inf) = 0 on (0, 0)
    float tsum = 0.f;                                    // the tile's own sum first: the running sum takes one add per tile
#pragma unroll
    for (int c = 0; c < DH; ++c) o[c] *= alpha;
#pragma unroll
    for (int j = 0; j < AKT; ++j) {
      if (j < kc) {
        const float p = expf(s[j] - mnew);
        tsum += p;
#pragma unroll
        for (int c = 0; c < DH; c += 4) {
          const float4 vv = *(const float4*)(Vs + j * DH + c);
          o[c] = fmaf(p, vv.x, o[c]); o[c + 1] = fmaf(p, vv.y, o[c + 1]); o[c + 2] = fmaf(p, vv.z, o[c + 2]); o[c + 3] = fmaf(p, vv.w, o[c + 3]);
        }
      }
    }
    sum = sum * alpha + tsum;
    mx = mnew;
  }
  if (qi < N) {
    float* op = out + ((size_t)seq * N + qi) * d + (size_t)h * DH;
#pragma unroll
    for (int c = 0; c < DH; c += 4) *(float4*)(op + c) = make_float4(o[c] / sum, o[c + 1] / sum, o[c + 2] / sum, o[c + 3] / sum);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

int gemm_f32(hipStream_t s, const GemmF32Args& a) {
  if (!a.A || !a.W || !a.bias || !a.out || a.M < 1 || a.N < 1 || a.K < 4 || a.K % 4) return -1;
  if (a.epi < F32_EPI_PLAIN || a.epi > F32_EPI_LOGITS || (a.epi == F32_EPI_RES && !a.residual)) return -1;
  if (a.epi == F32_EPI_LOGITS ? (a.period < 2 || a.M % a.period) : a.bias_per_pos) return -1;
  if (!aligned16(a.A) || !aligned16(a.W)) return -1;   // float4 row loads (K % 4 == 0 keeps every row aligned)
  const long long tiles = (long long)((a.M + FB - 1) / FB) * ((a.N + FB - 1) / FB);
  if (tiles > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(gemm_f32_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a);
  return 0;
}

int attention_f32(hipStream_t s, const float* qkv, float* out, int nb, int N, int d, int heads) {
  if (!qkv || !out || nb < 1 || N < 1 || heads < 1 || d < 1 || d % heads || !aligned16(qkv) || !aligned16(out)) return -1;
  const int dh = d / heads, qtiles = (N + 63) / 64;
  const long long blocks = (long long)nb * heads * qtiles;
  if (blocks > 0x7fffffffLL) return -1;
  if (dh == 64) hipLaunchKernelGGL(attention_f32_kernel<64>, dim3((unsigned)blocks), dim3(64), 0, s, qkv, out, N, d, heads, qtiles);
  else if (dh == 32) hipLaunchKernelGGL(attention_f32_kernel<32>, dim3((unsigned)blocks), dim3(64), 0, s, qkv, out, N, d, heads, qtiles);
  else return -1;
  return 0;
}

}  // namespace mb
