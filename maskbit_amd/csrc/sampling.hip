// MaskBit sampling step: everything sample() does between the transformer forward and the
// next forward (modeling/modules/sampling.py:90-131):
//   CFG combine -> softmax -> categorical draw as argmax(p / Exp(1)) (= torch.multinomial(n=1)) ->
//   keep already-decoded tokens -> confidence log p[pred] + scaled Gumbel noise (+inf for decoded
//   positions) -> k-th smallest confidence per image -> re-mask everything <= threshold.
// One 64-lane wave per (position, group) row: the row's C logits live one-per-lane (C/64 per lane
// when C > 64), so max / sum / argmax are wavefront reductions.  The k-th order statistic over the
// n*m confidences is found by rank counting out of LDS (exactly torch.sort(...)[k-1], ties and
// infinities included).  All arithmetic is fp32, as in the reference.
#include "mb_kernels.h"

namespace mb {

// logits_c + scale * (logits_c - logits_u) in the reference's three roundings (sampling.py:98-99).  The __f*_rn functions are plain operators in the HIP
// headers and contract to an fma under the compiler's default; the pragma is what keeps the product and the sum apart.
__device__ __forceinline__ float cfg_combine(float c, float u, float scale) {
#pragma clang fp contract(off)
  const float d = c - u;
  const float m = scale * d;
  return c + m;
}

// ---- seeded noise (include/maskbit_hip.h "per-sample seeded sampling"): Philox4x32-10 keyed by the sample's seed, counter = run-invariant coordinates ----
struct Philox4 { uint32_t w[4]; };
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}
// The one place the two noise values of a slot are made: the step kernel and the diagnostic dump inline this same body, so they produce the same bits.
// stream 0 (categorical): counter (c >> 2, slot, step, 0), word c & 3 -> q = -log u, the Exp(1) value of class c;
// stream 1 (confidence):  counter (0, slot, step, 1), word 0 -> (-log(-log u) * randomize_temperature) * conf_w, two roundings in the reference's order.
// u = float((x >> 8) | 1) * 2^-24: exact in fp32, in [2^-24, 1 - 2^-24].  *u_out (optional) receives the uniform.
__device__ __forceinline__ float seeded_noise(uint64_t seed, int step, int slot, int c, bool conf, float rand_temp, float conf_w, float* u_out) {
#pragma clang fp contract(off)
  const Philox4 r = philox4x32_10(conf ? 0u : (uint32_t)c >> 2, (uint32_t)slot, (uint32_t)step, conf ? 1u : 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const int k = conf ? 0 : c & 3;
  const uint32_t x = k == 0 ? r.w[0] : k == 1 ? r.w[1] : k == 2 ? r.w[2] : r.w[3];
  const float u = (float)((x >> 8) | 1u) * 0x1p-24f;
  if (u_out) *u_out = u;
  const float q = -logf(u);
  if (!conf) return q;
  const float g = -logf(q);
  const float t = g * rand_temp;
  return t * conf_w;
}

// Two launches (round 3; one workgroup per image did both parts, i.e. 64 of 256 CUs ran 32 latency-bound rows per wave: 100 us per step):
//   sample_rows_kernel   -- one wave per (image, position, group) row, 16 rows per 4-wave workgroup over the whole chip: guidance, softmax, draw,
//                           confidence.  Result packed into the int64 slot of tokens_out: low dword = the confidence's float bits, high dword = pred.
//   sample_thresh_kernel -- one workgroup per image: unpack into LDS, k-th smallest confidence by rank counting, re-mask, write tokens (+ pred);
//                           <true>: the per-sample rule of the edit step (sample_step with num_regen).
// The arithmetic per row and the order statistic are unchanged (bit-exact with the oracle: tests/test_hip_parity.py).
// SEEDED: the two noise values are computed in registers from (seeds[row / P], step, slot, class) instead of read (four lanes recompute one Philox block:
// no exchange, no LDS; profiles/seeded_noise.md); everything after the noise is the same code.
// REQ (with SEEDED; include/maskbit_hip.h "per-sample sampling arguments"): scale, temperature, step, randomize temperature and confidence weight are those of
// the sample's record a.req[row / P] instead of the kernel arguments -- one record per wave and row, a uniform read; everything after the constants is the same code.
template <int CPL, bool SEEDED, bool REQ = false>   // logits per lane: C <= 64*CPL
__global__ __launch_bounds__(256) void sample_rows_kernel(StepArgs a, const int64_t* __restrict__ tokens_in) {
  static_assert(SEEDED || !REQ, "the per-sample records go with the seeded noise");
  const int C = a.C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t mask_tok = (int64_t)C;
  const size_t nrows = (size_t)a.B * a.P;
#pragma unroll 1
  for (int it = 0; it < 4; ++it) {
    const size_t row = (size_t)blockIdx.x * 16 + wave * 4 + it;
    if (row >= nrows) return;
    const float* lc = a.logits_c + row * C;
    const float* lu = a.logits_u ? a.logits_u + row * C : nullptr;
    const float* qn = SEEDED ? nullptr : a.exp_noise + row * C;
    uint64_t seed = 0; int slot = 0;
    float scale = a.scale, temperature = a.temperature, rand_temp = a.rand_temp, conf_w = a.conf_w;
    int step = a.step;
    if constexpr (SEEDED) {
      const size_t b = row / (size_t)a.P;
      seed = (uint64_t)a.seeds[b];
      slot = (int)(row - b * (size_t)a.P);
      if constexpr (REQ) {
        const RequestStep rs = a.req[__builtin_amdgcn_readfirstlane((int)b)];   // (a wave works on one row: the index is uniform)
        scale = rs.scale; temperature = rs.temperature; step = rs.step; rand_temp = rs.rand_temp; conf_w = rs.conf_w;
      }
    }
    float l[CPL];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + 64 * i;
      float v = -INFINITY;
      if (c < C) {
        v = lc[c];
        if (lu) v = cfg_combine(v, lu[c], scale);
        v = v / temperature;                            // :105
      }
      l[i] = v;
      mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) { l[i] = (lane + 64 * i < C) ? expf(l[i] - mx) : 0.f; sum += l[i]; }
    sum = wave_sum(sum);
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) { l[i] = l[i] / sum; psum += l[i]; }   // probabilities
    psum = wave_sum(psum);                                               // Categorical re-normalises
    float best = -INFINITY; int bi = 0x7fffffff;
#pragma clang loop unroll(full)   // (full: "#pragma unroll" leaves the seeded CPL = 64 body partly rolled, with l[] in scratch)
    for (int i = 0; i < CPL; ++i) {
      const int c = lane + 64 * i;
      if (c < C) {
        float q;
        if constexpr (SEEDED) {
          int cc = c;
          // (the first Philox round's products of c >> 2 depend on the lane and i alone, and the compiler hoists them out of the row loop: two VGPRs per i
          // live across it.  Up to CPL = 16 that saves a round's multiplies; at CPL = 32 it costs 186 VGPRs instead of 122 and at CPL = 64 scratch: the
          // empty statement makes c opaque there, which keeps the products inside the loop)
          if constexpr (CPL >= 32) asm volatile("" : "+v"(cc));
          q = seeded_noise(seed, step, slot, cc, false, 0.f, 0.f, nullptr);
        }
        else q = qn[c];
        const float ratio = (l[i] / psum) / q;
        if (ratio > best) { best = ratio; bi = c; }      // strict '>' keeps the lowest index in-lane
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    const int64_t tin = tokens_in[row];
    const bool masked = tin == mask_tok;
    const int pred = masked ? bi : (int)tin;                             // :111
    // p[pred]: owned by lane pred%64, slot pred/64
    float pv = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) if (pred == lane + 64 * i) pv = l[i];
    pv = __shfl(pv, pred & 63);
    if (lane == 0) {
      float cn;
      if constexpr (SEEDED) cn = seeded_noise(seed, step, slot, 0, true, rand_temp, conf_w, nullptr);
      else cn = a.conf_noise[row];
      const float conf = (masked ? logf(pv) : INFINITY) + cn;    // :113-118
      a.tokens[row] = (int64_t)(((uint64_t)(uint32_t)pred << 32) | (uint64_t)__float_as_uint(conf));
    }
  }
}

// The threshold stage of both step kernels.  EDIT = false: the reference's rule (one masked count, SAMPLE 0's, and one mask length for the whole batch; the
// Python index k - 1 may wrap).  EDIT = true (sample_step_edit, image editing: samples that start from different masked counts): per sample b
//   mask_len = floor(ratio * M[b]) in fp32 (torch.floor(ratio * num_maskable) with a float32 ratio), nm = sample b's own masked count,
//   nm >= 2: k = min(max(mask_len, 1), nm - 1) -- k - 1 <= nm - 2, so the threshold is a MASKED slot's confidence and a known slot (+inf) is never re-masked;
//   nm <= 1: nothing is re-masked (tokens_out = pred).  The reference's clamp reaches k = 0 there, sorted[-1] = +inf, and every token of the image,
//            the known ones included, would be masked again (DESIGN.md "Editing").
// REQ (with EDIT): the ratio is the sample's own, a.req[b].mask_ratio.
template <bool EDIT, bool REQ = false>
__global__ __launch_bounds__(1024) void sample_thresh_kernel(StepArgs a, const int64_t* __restrict__ tokens_in, float ratio, const int* __restrict__ num_regen) {
  extern __shared__ float sm[];
  const int P = a.P;
  float* conf_s = sm;                    // [P]
  int* pred_s = (int*)(sm + P);          // [P]
  int* cnt_s = pred_s + P;               // [16]: per-wave partial counts
  float* thr_s = (float*)(cnt_s + 16);   // [1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int b = blockIdx.x;
  const int64_t mask_tok = (int64_t)a.C;
  if constexpr (REQ) ratio = a.req[b].mask_ratio;
  // num_masked of SAMPLE 0 (sampling.py:109 reads index [0] for the whole batch); EDIT: of this sample
  const int64_t* tin = EDIT ? tokens_in + (size_t)b * P : tokens_in;
  int mycnt = 0;
  for (int p = tid; p < P; p += blockDim.x) mycnt += tin[p] == mask_tok;
  mycnt = (int)wave_sum((float)mycnt);
  if (lane == 0) cnt_s[wave] = mycnt;
  if (tid == 0) *thr_s = -INFINITY;
  for (int p = tid; p < P; p += blockDim.x) {        // everything of this image is in LDS before any of its slots is overwritten
    const uint64_t v = (uint64_t)a.tokens[(size_t)b * P + p];
    conf_s[p] = __uint_as_float((uint32_t)v);
    pred_s[p] = (int)(uint32_t)(v >> 32);
  }
  __syncthreads();
  int nm = 0;
  for (int w = 0; w < nw; ++w) nm += cnt_s[w];
  // k = clamp(floor(ratio*P), 1, num_masked-1), threshold = sorted[k-1] (python index, may wrap)
  const int mask_len = EDIT ? (int)floorf(__fmul_rn(ratio, (float)num_regen[b])) : a.k_mask_len;
  const bool remask = !EDIT || nm >= 2;
  int k = min(max(mask_len, 1), nm - 1);
  int idx = k - 1;
  if (idx < 0) idx += P;
  if (remask) {
    for (int p = tid; p < P; p += blockDim.x) {
      const float x = conf_s[p];
      int lt = 0, le = 0;
      for (int j = 0; j < P; ++j) { const float y = conf_s[j]; lt += y < x; le += y <= x; }
      if (lt <= idx && idx < le) *thr_s = x;
    }
  }
  __syncthreads();
  const float thr = *thr_s;
  for (int p = tid; p < P; p += blockDim.x) {
    const size_t row = (size_t)b * P + p;
    const int pr = pred_s[p];
    a.tokens[row] = remask && conf_s[p] <= thr ? mask_tok : (int64_t)pr;  // :128-129
    if (a.pred) a.pred[row] = (int64_t)pr;
  }
}

template <bool SEEDED, bool REQ = false>
static void launch_rows(hipStream_t s, const StepArgs& a, const int64_t* tokens_in) {
  const size_t nrows = (size_t)a.B * a.P;
  dim3 grid((unsigned)((nrows + 15) / 16)), block(256);
  if (a.C <= 64) hipLaunchKernelGGL((sample_rows_kernel<1, SEEDED, REQ>), grid, block, 0, s, a, tokens_in);
  else if (a.C <= 128) hipLaunchKernelGGL((sample_rows_kernel<2, SEEDED, REQ>), grid, block, 0, s, a, tokens_in);
  else if (a.C <= 256) hipLaunchKernelGGL((sample_rows_kernel<4, SEEDED, REQ>), grid, block, 0, s, a, tokens_in);
  else if (a.C <= 512) hipLaunchKernelGGL((sample_rows_kernel<8, SEEDED, REQ>), grid, block, 0, s, a, tokens_in);
  else if (a.C <= 1024) hipLaunchKernelGGL((sample_rows_kernel<16, SEEDED, REQ>), grid, block, 0, s, a, tokens_in);   // single-group codebooks (codebook_splits = 1)
  else if (a.C <= 2048) hipLaunchKernelGGL((sample_rows_kernel<32, SEEDED, REQ>), grid, block, 0, s, a, tokens_in);
  else hipLaunchKernelGGL((sample_rows_kernel<64, SEEDED, REQ>), grid, block, 0, s, a, tokens_in);
}

int sample_step(hipStream_t s, const StepArgs& a, const int64_t* tokens_in, const int* num_regen, float mask_ratio) {
  if (a.C > 4096 || a.P > 8192) return -1;
  if (a.seeds && !num_regen) return -1;             // a seeded step re-masks by the per-sample rule only
  if (a.req && !a.seeds) return -1;                 // the per-sample records go with the seeded noise
  if (a.req) launch_rows<true, true>(s, a, tokens_in);
  else if (a.seeds) launch_rows<true>(s, a, tokens_in);
  else launch_rows<false>(s, a, tokens_in);
  const size_t shm = (size_t)a.P * 8 + 16 * 4 + 16;
  const dim3 tblock(a.P >= 1024 ? 1024 : 512);
  if (a.req) hipLaunchKernelGGL((sample_thresh_kernel<true, true>), dim3(a.B), tblock, shm, s, a, tokens_in, 0.f, num_regen);
  else if (num_regen) hipLaunchKernelGGL(sample_thresh_kernel<true>, dim3(a.B), tblock, shm, s, a, tokens_in, mask_ratio, num_regen);
  else hipLaunchKernelGGL(sample_thresh_kernel<false>, dim3(a.B), tblock, shm, s, a, tokens_in, 0.f, (const int*)nullptr);
  return 0;
}

// The noise a seeded step generates for itself, written out in the explicit path's layout (mb_seeded_noise): one thread per (row, class); the thread
// of class 0 also writes the row's confidence noise.
__global__ __launch_bounds__(256) void seeded_noise_kernel(const int64_t* __restrict__ seeds, int step, float rand_temp, float conf_w, float* __restrict__ exp_u,
                                                            float* __restrict__ exp_noise, float* __restrict__ conf_u, float* __restrict__ conf_noise, size_t total, int P, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t row = i / (size_t)C;
  const int c = (int)(i - row * (size_t)C);
  const size_t b = row / (size_t)P;
  const int slot = (int)(row - b * (size_t)P);
  const uint64_t seed = (uint64_t)seeds[b];
  float u;
  const float q = seeded_noise(seed, step, slot, c, false, 0.f, 0.f, &u);
  if (exp_noise) exp_noise[i] = q;
  if (exp_u) exp_u[i] = u;
  if (c == 0) {
    const float cn = seeded_noise(seed, step, slot, 0, true, rand_temp, conf_w, &u);
    if (conf_noise) conf_noise[row] = cn;
    if (conf_u) conf_u[row] = u;
  }
}
int seeded_noise_dump(hipStream_t s, const int64_t* seeds, int step, float rand_temp, float conf_w, float* exp_u, float* exp_noise, float* conf_u,
                      float* conf_noise, int B, int P, int C) {
  if (C > 4096 || P > 8192) return -1;
  const size_t total = (size_t)B * P * C;
  if ((total + 255) / 256 > 0x7fffffffull) return -1;
  hipLaunchKernelGGL(seeded_noise_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, seeds, step, rand_temp, conf_w, exp_u, exp_noise, conf_u,
                     conf_noise, total, P, C);
  return 0;
}

__global__ void fill_i64_kernel(int64_t* dst, int64_t v, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = v;
}
void fill_i64(hipStream_t s, int64_t* dst, int64_t value, size_t n) {
  hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)min((size_t)1024, (n + 255) / 256)), dim3(256), 0, s, dst, value, n);
}

// combine_factorized_tokens (factorization.py:7-24): sum_g tok[..., g] << (g * K/m), kept integral.
__global__ void combine_groups_kernel(const int64_t* __restrict__ tok, int64_t* __restrict__ codes, size_t rows, int m, int gbits) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (size_t)gridDim.x * blockDim.x) {
    int64_t v = 0;
    for (int g = 0; g < m; ++g) v += tok[i * m + g] << (g * gbits);
    codes[i] = v;
  }
}
void combine_groups(hipStream_t s, const int64_t* tokens, int64_t* codes, size_t rows, int m, int gbits) {
  hipLaunchKernelGGL(combine_groups_kernel, dim3((unsigned)min((size_t)1024, (rows + 255) / 256)), dim3(256), 0, s,
                     tokens, codes, rows, m, gbits);
}

}  // namespace mb
