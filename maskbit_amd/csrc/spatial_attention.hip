// Spatial self-attention of the Taming VQGAN's AttnBlock (modeling/taming/taming_autoencoder.py:149-173): a single head of 512 channels over the
// N = H W pixels of one image (256 at 256^2, 1 024 at 512^2), out = softmax(q k^T 512^-0.5) v on fp16 rows with fp32 accumulation.
//
// At this width neither K nor V of an image fits in LDS (1 024 x 512 fp16 = 1 MiB), and a head of attention.hip's kernels (32 / 64 channels) keeps
// its whole output row in four accumulators, so this is its own kernel: the flash form over 32-key blocks.
//   Workgroup = 4 waves = 64 queries of ONE image, a wave = one 16-query tile; grid = B x ceil(N / 64).  Tiles never cross images, so the result
//   of an image does not depend on the batch, and there are no atomics on data: bit-stable run to run.
//   Registers (per lane, one wave per SIMD: 512 available): Q of the tile as 16 MFMA B fragments = 64, the output tile O^T [512 channels x 16
//   queries] as 32 accumulators = 128, the rest (K fragments in flight, scores, V fragments) well under 100: no spill.
//   LDS: one 32-key V block, 32 rows x (1 024 + 32) bytes = 33 KiB, filled by LDS-DMA (one row per wave instruction).  The 32 bytes of padding put
//   the 8 rows that a 32-lane half of a transposed read touches on disjoint banks.
//   Per block:  S^T = K Q^T  (2 key tiles x 16 k-steps, K fragments straight from global memory: a lane's 16 bytes of one key row) so that a lane
//   holds the scores of ITS query (column l & 15) for keys 4 g + r of each tile -- the softmax statistics are lane-local plus one reduction over
//   the four lane rows; then  O^T += V^T P^T  with V^T read out of the row-major block by ds_read_b64_tr_b16 (as attention.hip does) and P^T the
//   probabilities as they stand in registers, rounded to fp16.  The k index of that product runs over keys in the order the scores sit in the
//   lane (element j <-> key 16 (j >> 2) + 4 g + (j & 3)); the transposed reads fetch V's rows in the same order.
//   Softmax: fp32, running maximum, exp2((s - m) * 512^-0.5 * log2 e) -- exactly 1 for the maximal key; the row sum is taken over the fp32
//   probabilities, per lane, and reduced over the lane rows once at the end.
#include "mb_spattn.h"

namespace mb {

namespace {
constexpr int KB = 32;                            // keys per block = one k-step of the P V product
constexpr int VROW = SPATTN_C * 2 + 32;           // bytes of a V row in LDS
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__global__ __launch_bounds__(256) void spatial_attention_kernel(SpAttn a) {
  __shared__ __attribute__((aligned(16))) char vs[KB * VROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int N = a.N, nqb = (N + 63) >> 6;
  const int b = blockIdx.x / nqb, qt = (blockIdx.x - b * nqb) * 4 + wave;
  // a wave past the last query tile (N % 64 != 0) keeps loading and passing barriers on the last tile's rows and stores nothing: the transposed
  // reads below need every lane of every wave active
  const bool live = qt * 16 < N;
  const int q0 = live ? qt * 16 : N - 16;
  const size_t row0 = (size_t)b * N;

  h16x8 qf[16];                                   // B fragments of Q^T: [k = channel 32 ks + 8 g + j][column = query l15]
  {
    const h16* qp = a.q + (row0 + q0 + l15) * a.ld + g * 8;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) qf[ks] = *(const h16x8*)(qp + ks * 32);
  }
  f32x4 o[32];                                    // O^T: o[ct][r] = channel 16 ct + 4 g + r of query l15
#pragma unroll
  for (int ct = 0; ct < 32; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;            // running maximum of the query's scores; this lane's share of the running sum
  const float sl2 = 0.044194173824159216f * 1.4426950408889634f;   // 512^-0.5 * log2(e)
  const unsigned vb = (unsigned)(uintptr_t)vs + (4 * g + (l15 >> 2)) * VROW + (l15 & 3) * 8;   // row 4 g + q, columns 4 p .. 4 p + 3 of a block

  for (int kb = 0; kb < N; kb += KB) {
    __syncthreads();                              // every wave is done with the previous V block
#pragma unroll
    for (int j = 0; j < KB / 4; ++j) {
      const int r = wave * (KB / 4) + j;
      const int key = min(kb + r, N - 1);         // (N % 32 == 16: the rows past the end repeat the last key; their probabilities are 0)
      MB_GLDS16(a.v + (row0 + key) * a.ld + lane * 8, vs + r * VROW);
    }
    // ---- S^T = K Q^T: s[t][r] = score of key kb + 16 t + 4 g + r for query l15
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int key = min(kb + 16 * t + l15, N - 1);
      const h16* kp = a.k + (row0 + key) * a.ld + g * 8;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) s[t] = MB_MFMA_16x16x32(*(const h16x8*)(kp + ks * 32), qf[ks], s[t]);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (kb + 16 * t + 4 * g + r >= N) s[t][r] = -INFINITY;
        mx = fmaxf(mx, s[t][r]);
      }
    mx = rows_max(mx);                            // finite: the first key tile of a block always exists
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * sl2);     // 0 in the first block (m_run = -inf)
    float sum = 0.f;
    h16x8 pf;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f((s[t][r] - m_new) * sl2);
        sum += p;
        pf[t * 4 + r] = (h16)p;
      }
    l_run = l_run * alpha + sum;
    m_run = m_new;
#pragma unroll
    for (int ct = 0; ct < 32; ++ct) o[ct] *= alpha;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                              // the V block has landed
    // ---- O^T += V^T P^T: the A fragment of channel tile ct = rows 4 g + q and 16 + 4 g + q of the block, columns 16 ct .. 16 ct + 15, transposed
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4) {
      uint2 v[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned ad = vb + (c4 * 4 + i) * 32;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v[i][0]) : "v"(ad) : "memory");
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v[i][1]) : "v"(ad + 16 * VROW) : "memory");
      }
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0][0]), "+v"(v[0][1]), "+v"(v[1][0]), "+v"(v[1][1]),
                   "+v"(v[2][0]), "+v"(v[2][1]), "+v"(v[3][0]), "+v"(v[3][1])::"memory");
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const u32x4 raw = {v[i][0].x, v[i][0].y, v[i][1].x, v[i][1].y};
        o[c4 * 4 + i] = MB_MFMA_16x16x32(__builtin_bit_cast(h16x8, raw), pf, o[c4 * 4 + i]);
      }
    }
  }
  const float inv = 1.0f / rows_sum(l_run);       // (IEEE division: exact for a power-of-two sum)
  if (live) {
    h16* op = a.out + (row0 + q0 + l15) * a.ldo + 4 * g;
    unsigned nsat = 0;
#pragma unroll
    for (int ct = 0; ct < 32; ++ct) {
      const float v0 = o[ct][0] * inv, v1 = o[ct][1] * inv, v2 = o[ct][2] * inv, v3 = o[ct][3] * inv;
      nsat += fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3))) > MB_H16_MAX ? 1u : 0u;
      *(h16x4*)(op + ct * 16) = h16x4{to_h(v0), to_h(v1), to_h(v2), to_h(v3)};
    }
    if (nsat && a.sat) atomicAdd(a.sat, nsat);
  }
}
}  // namespace

bool launch_spatial_attention(hipStream_t s, const SpAttn& a) {
  if (a.B <= 0 || a.N < 16 || a.N > 1024 || a.N % 16 || a.ld < SPATTN_C || a.ld % 8 || a.ldo < SPATTN_C || a.ldo % 4) return false;
  const int nqb = (a.N + 63) / 64;
  hipLaunchKernelGGL(spatial_attention_kernel, dim3((unsigned)(a.B * nqb)), dim3(256), 0, s, a);
  return true;
}

}  // namespace mb
