// Masked-token validation of a generator checkpoint on gfx950: the token masking of the reference's training step (get_mask_tokens,
// modeling/modules/masking.py:7-38) and its MLMLoss (modeling/modules/losses.py:289-339) -- label-smoothed cross entropy and argmax accuracy
// over all rows and over the masked rows -- from ONE read of the [B, n, m, C] logits.
//
// mlm_mask_kernel: mask = uniforms < val_to_mask[b] (the fp32 compare of masking.py:35), masked = mask ? mask_token : tokens.  Four slots per
// thread with 16-byte loads and stores of the uniforms and the tokens when n * m is a multiple of 4 and the bases allow it, one slot otherwise.
//
// mlm_loss_kernel<G, VEC>: a row (one (b, position, group) of C logits) belongs to a group of G lanes, G = the power of two at or above C / 4,
// at most 64; a wave holds 64 / G rows at a time.  Lane l of the group reads the elements [4 (l + k G), 4 (l + k G) + 4), k = 0, 1, .. -- a
// float4 when VEC (C % 4 == 0 and a 16-byte aligned base), four guarded scalar loads otherwise: the same elements in the same lanes, so both
// paths give the same bits -- and keeps a running (max, sum exp(x - max), sum x, first argmax, x[target]) in fp32; the group then combines them
// with cross-lane butterflies: max first, one rescale of each lane's sum, then the sums; (value, index) for the argmax, the lower index winning
// on equal values (torch.argmax).  The target's logit is picked up by the lane that reads it and broadcast: memory is never indexed by a
// target.  Per row, as torch's log_softmax evaluates it (x - max - log sum, so the rounding happens at the size of the loss, not of the lse):
//   nll = (max - x[target]) + log sum,  smooth = (max - mean x) + log sum,  loss = (1 - eps) nll + eps smooth   (eps = 0: loss = nll, the
// smoothing term is not formed, as in torch.nn.CrossEntropyLoss).  expf / logf are the accurate ones.  A target outside [0, C) leaves its row out
// of every figure and is counted.  The leader lane of a group adds its rows in fp64; a workgroup reduces in a fixed order and writes ONE slot of
// the workspace: no floating-point atomics.  The rows of a sample are split over workgroups by (n * m, C) alone, so a sample's figures do not
// depend on the batch it sits in.
//
// mlm_finalize_kernel (one workgroup): per sample the slots are summed in a fixed order; then one thread adds the samples to the caller's pooled
// state IN SAMPLE ORDER, so consecutive updates of the parts of a batch leave the bits of one update of the whole.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/maskbit_hip.h"
#include "mb_abi.h"

namespace mb {

namespace {

constexpr int ML_THREADS = 256;
constexpr int ML_WAVES = ML_THREADS / 64;
constexpr int ML_BUCKETS = 10;

// one workspace slot: the figures of a workgroup's rows, or (behind the B * P workgroup slots) of a whole sample
struct MlmPart {
  double loss_all, loss_masked;
  long long correct_all, correct_masked, masked, bad;
};

// the pooled state of include/maskbit_hip.h (37 words of 8 bytes)
struct MlmState {
  double loss_all, loss_masked;
  long long rows, masked, correct_all, correct_masked;
  struct { double loss; long long correct, rows; } bucket[ML_BUCKETS];
  long long out_of_range;
};
static_assert(sizeof(MlmPart) == 48 && sizeof(MlmState) == 37 * 8, "layouts of maskbit_hip.h");

// ---- masking ----------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(ML_THREADS) void mlm_mask_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ uniforms,
                                                              const float* __restrict__ val_to_mask, int64_t mask_token, int R, int64_t total,
                                                              int64_t* __restrict__ masked, uint8_t* __restrict__ mask) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if constexpr (VEC) {                                     // R % 4 == 0: the four slots of an item belong to one sample
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total / 4; i += stride) {
      const float v = val_to_mask[(i * 4) / R];
      const float4 u = reinterpret_cast<const float4*>(uniforms)[i];
      const longlong2 t0 = reinterpret_cast<const longlong2*>(tokens)[2 * i], t1 = reinterpret_cast<const longlong2*>(tokens)[2 * i + 1];
      const bool k0 = u.x < v, k1 = u.y < v, k2 = u.z < v, k3 = u.w < v;
      longlong2 o0, o1;
      o0.x = k0 ? mask_token : t0.x; o0.y = k1 ? mask_token : t0.y;
      o1.x = k2 ? mask_token : t1.x; o1.y = k3 ? mask_token : t1.y;
      reinterpret_cast<longlong2*>(masked)[2 * i] = o0;
      reinterpret_cast<longlong2*>(masked)[2 * i + 1] = o1;
      reinterpret_cast<uchar4*>(mask)[i] = make_uchar4(k0, k1, k2, k3);
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const bool k = uniforms[i] < val_to_mask[i / R];
      masked[i] = k ? mask_token : tokens[i];
      mask[i] = k;
    }
  }
}

// ---- loss -------------------------------------------------------------------------------------------------------------------------------
// (v, i) beats (bv, bi): a larger value, a NaN over a number (torch.argmax takes a NaN for the maximum), or the lower index on equal values
__device__ __forceinline__ bool beats(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return i < bi;
}

// rows a workgroup takes per pass (ML_WAVES * 64 / G) and passes per workgroup: about 1024 logits per wave, from C alone
__host__ __device__ inline int mlm_group(int C) {
  int g = 1;
  while (g < 64 && g * 4 < C) g <<= 1;
  return g;
}
__host__ __device__ inline int mlm_passes(int C) {
  const long long per_pass = (long long)(64 / mlm_group(C)) * C;
  return per_pass >= 1024 ? 1 : (int)(1024 / per_pass);
}
inline int mlm_rows_per_block(int C) { return ML_WAVES * (64 / mlm_group(C)) * mlm_passes(C); }

// grid (P, B); part [B][P]
template <int G, bool VEC>
__global__ __launch_bounds__(ML_THREADS) void mlm_loss_kernel(const float* __restrict__ logits, const int64_t* __restrict__ targets,
                                                              const uint8_t* __restrict__ mask, float eps, int R, int C, int passes,
                                                              MlmPart* __restrict__ part) {
  constexpr int RW = 64 / G;                               // rows of a wave
  __shared__ MlmPart red[ML_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane & (G - 1), grp = lane / G;
  const int b = blockIdx.y;
  const int row0 = blockIdx.x * (ML_WAVES * RW * passes);
  const float inf = INFINITY;
  double a_all = 0.0, a_m = 0.0;
  int c_all = 0, c_m = 0, n_m = 0, n_bad = 0;

  for (int it = 0; it < passes; ++it) {
    const int r = row0 + (it * ML_WAVES + wave) * RW + grp;
    const bool live = r < R;                               // a dead group reads nothing and takes part in the butterflies
    const size_t row = (size_t)b * R + (live ? r : 0);
    const float* __restrict__ x = logits + row * (size_t)C;
    const int64_t t64 = targets[row];
    const bool t_ok = t64 >= 0 && t64 < C;
    const int t = t_ok ? (int)t64 : -1;
    float mx = -inf, s = 0.f, sx = 0.f, bv = -inf, xt = 0.f;
    int bi = INT_MAX;
    for (int c0 = gl * 4; c0 < (live ? C : 0); c0 += G * 4) {
      float v[4];
      int nv = 4;
      if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(x + c0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      } else {
        nv = min(4, C - c0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < nv ? x[c0 + k] : -inf;
      }
      const float nm = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
      const float ref = nm == -inf ? 0.f : nm;             // a chunk of -inf alone: exp(-inf - 0) = 0, never inf - inf
      if (nm > mx) { s *= expf(mx - ref); mx = nm; }
      float e[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool in = k < nv;
        e[k] = in ? expf(v[k] - ref) : 0.f;
        sx += in ? v[k] : 0.f;
        if (in && beats(v[k], c0 + k, bv, bi)) { bv = v[k]; bi = c0 + k; }
        if (c0 + k == t) xt = v[k];
      }
      s += (e[0] + e[1]) + (e[2] + e[3]);
    }
    // the group's maximum, then every lane's sum on that scale
    float M = mx;
#pragma unroll
    for (int o = G >> 1; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
    const float Mref = M == -inf ? 0.f : M;
    s *= expf(mx - Mref);                                  // exp(0) = 1 in the lanes that hold the maximum; 0 * 0 in a lane without elements
#pragma unroll
    for (int o = G >> 1; o >= 1; o >>= 1) {
      s += __shfl_xor(s, o);
      sx += __shfl_xor(sx, o);
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (beats(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    xt = __shfl(xt, t_ok ? (t >> 2) & (G - 1) : 0, G);       // from the lane that read element t
    if (gl == 0 && live) {
      if (!t_ok) {
        ++n_bad;
      } else {
        const float ls = logf(s);
        const float nll = (M - xt) + ls;
        float loss = nll;
        if (eps > 0.f) loss = (1.0f - eps) * nll + eps * ((M - sx / (float)C) + ls);
        const bool mk = mask[row] != 0, hit = bi == t;
        a_all += (double)loss;
        c_all += hit;
        if (mk) { a_m += (double)loss; c_m += hit; ++n_m; }
      }
    }
  }

#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    a_all += __shfl_xor(a_all, o); a_m += __shfl_xor(a_m, o);
    c_all += __shfl_xor(c_all, o); c_m += __shfl_xor(c_m, o); n_m += __shfl_xor(n_m, o); n_bad += __shfl_xor(n_bad, o);
  }
  if (lane == 0) red[wave] = MlmPart{a_all, a_m, c_all, c_m, n_m, n_bad};
  __syncthreads();
  if (threadIdx.x == 0) {
    MlmPart p = red[0];
    for (int w = 1; w < ML_WAVES; ++w) {
      p.loss_all += red[w].loss_all; p.loss_masked += red[w].loss_masked;
      p.correct_all += red[w].correct_all; p.correct_masked += red[w].correct_masked; p.masked += red[w].masked; p.bad += red[w].bad;
    }
    part[(size_t)b * gridDim.x + blockIdx.x] = p;
  }
}

// one workgroup; part [B][P] -> per_sample [B] (workspace), sample_sums [B][2] / sample_counts [B][3] (either may be null), state (may be null)
__global__ __launch_bounds__(ML_THREADS) void mlm_finalize_kernel(const MlmPart* __restrict__ part, int B, int P, int R,
                                                                  MlmPart* __restrict__ per_sample, double* __restrict__ sample_sums,
                                                                  long long* __restrict__ sample_counts, MlmState* __restrict__ state) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += ML_WAVES) {
    MlmPart a = {0.0, 0.0, 0, 0, 0, 0};
    for (int p = lane; p < P; p += 64) {
      const MlmPart q = part[(size_t)b * P + p];
      a.loss_all += q.loss_all; a.loss_masked += q.loss_masked;
      a.correct_all += q.correct_all; a.correct_masked += q.correct_masked; a.masked += q.masked; a.bad += q.bad;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      a.loss_all += __shfl_xor(a.loss_all, o); a.loss_masked += __shfl_xor(a.loss_masked, o);
      a.correct_all += __shfl_xor(a.correct_all, o); a.correct_masked += __shfl_xor(a.correct_masked, o);
      a.masked += __shfl_xor(a.masked, o); a.bad += __shfl_xor(a.bad, o);
    }
    if (lane == 0) {
      per_sample[b] = a;
      if (sample_sums) { sample_sums[(size_t)b * 2] = a.loss_all; sample_sums[(size_t)b * 2 + 1] = a.loss_masked; }
      if (sample_counts) {
        sample_counts[(size_t)b * 3] = a.correct_all; sample_counts[(size_t)b * 3 + 1] = a.correct_masked; sample_counts[(size_t)b * 3 + 2] = a.masked;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x != 0 || !state) return;
  for (int b = 0; b < B; ++b) {                            // sample order
    const MlmPart a = per_sample[b];
    state->loss_all += a.loss_all; state->loss_masked += a.loss_masked;
    state->rows += R - a.bad; state->masked += a.masked; state->correct_all += a.correct_all; state->correct_masked += a.correct_masked;
    const long long k10 = 10 * a.masked / R;
    auto& bk = state->bucket[k10 < ML_BUCKETS - 1 ? k10 : ML_BUCKETS - 1];
    bk.loss += a.loss_masked; bk.correct += a.correct_masked; bk.rows += a.masked;
    state->out_of_range += a.bad;
  }
}

bool mlm_shape_ok(int B, int n, int m, int C) {
  if (B < 1 || B > 65535 || n < 1 || m < 1 || C < 2) return false;
  return (long long)n * m <= INT_MAX / 16;                 // rows of a sample: 10 * masked and the row index stay far inside their types
}

inline int mlm_blocks(int R, int C) { const int rpb = mlm_rows_per_block(C); return (R + rpb - 1) / rpb; }

template <bool VEC>
void launch_loss(int G, dim3 grid, hipStream_t s, const float* logits, const int64_t* targets, const uint8_t* mask, float eps, int R, int C,
                 int passes, MlmPart* part) {
#define MB_MLM_CASE(g)                                                                                                         \
  case g:                                                                                                                      \
    hipLaunchKernelGGL((mlm_loss_kernel<g, VEC>), grid, dim3(ML_THREADS), 0, s, logits, targets, mask, eps, R, C, passes, part); \
    break;
  switch (G) {
    MB_MLM_CASE(1) MB_MLM_CASE(2) MB_MLM_CASE(4) MB_MLM_CASE(8) MB_MLM_CASE(16) MB_MLM_CASE(32) MB_MLM_CASE(64)
  }
#undef MB_MLM_CASE
}

}  // namespace

}  // namespace mb

using namespace mb;

extern "C" {

size_t mb_mlm_workspace_bytes(int B, int n, int m, int C) {
  if (!mlm_shape_ok(B, n, m, C)) return 0;
  return ((size_t)B * mlm_blocks(n * m, C) + (size_t)B) * sizeof(MlmPart);
}

size_t mb_mlm_state_bytes(void) { return sizeof(MlmState); }

int mb_mlm_mask(const int64_t* tokens, const float* uniforms, const float* val_to_mask, int64_t mask_token, int64_t* masked_tokens, uint8_t* mask,
                int B, int n, int m, mb_stream stream) {
  if (!tokens || !uniforms || !val_to_mask || !masked_tokens || !mask) return fail(-1, "mb_mlm_mask: null argument");
  if (B < 1 || n < 1 || m < 1 || (long long)n * m > INT_MAX) return fail(-1, "mb_mlm_mask: B, n, m >= 1 and n * m < 2^31 required (got %d x %d x %d)", B, n, m);
  if (masked_tokens == tokens) return fail(-1, "mb_mlm_mask: masked_tokens must not alias tokens (the input is not modified)");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("mlm_mask", s);
  const int R = n * m;
  const int64_t total = (int64_t)B * R;
  const bool vec = R % 4 == 0 && ((uintptr_t)tokens | (uintptr_t)uniforms | (uintptr_t)masked_tokens) % 16 == 0 && (uintptr_t)mask % 4 == 0;
  const int64_t items = vec ? total / 4 : total;
  const unsigned blocks = (unsigned)std::min<int64_t>(2048, (items + ML_THREADS - 1) / ML_THREADS);
  if (vec) hipLaunchKernelGGL(mlm_mask_kernel<true>, dim3(blocks), dim3(ML_THREADS), 0, s, tokens, uniforms, val_to_mask, mask_token, R, total, masked_tokens, mask);
  else hipLaunchKernelGGL(mlm_mask_kernel<false>, dim3(blocks), dim3(ML_THREADS), 0, s, tokens, uniforms, val_to_mask, mask_token, R, total, masked_tokens, mask);
  return launched();
}

int mb_mlm_loss(const float* logits, const int64_t* targets, const uint8_t* mask, float label_smoothing, int B, int n, int m, int C,
                void* workspace, double* sample_sums, int64_t* sample_counts, void* state, mb_stream stream) {
  if (!logits || !targets || !mask || !workspace) return fail(-1, "mb_mlm_loss: null argument");
  if (!mlm_shape_ok(B, n, m, C)) return fail(-1, "mb_mlm_loss: B in [1, 65535], n, m >= 1, C >= 2 required (got %d x %d x %d x %d)", B, n, m, C);
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return fail(-1, "mb_mlm_loss: label_smoothing in [0, 1] required (got %g)", (double)label_smoothing);
  if ((uintptr_t)workspace % 8 || (uintptr_t)state % 8) return fail(-1, "mb_mlm_loss: workspace and state must be 8-byte aligned");
  if ((uintptr_t)logits % 4) return fail(-1, "mb_mlm_loss: logits must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("mlm_loss", s);
  const int R = n * m, P = mlm_blocks(R, C);
  MlmPart* part = (MlmPart*)workspace;
  const dim3 grid(P, B);
  if (C % 4 == 0 && (uintptr_t)logits % 16 == 0) launch_loss<true>(mlm_group(C), grid, s, logits, targets, mask, label_smoothing, R, C, mlm_passes(C), part);
  else launch_loss<false>(mlm_group(C), grid, s, logits, targets, mask, label_smoothing, R, C, mlm_passes(C), part);
  hipLaunchKernelGGL(mlm_finalize_kernel, dim3(1), dim3(ML_THREADS), 0, s, part, B, P, R, part + (size_t)B * P, sample_sums,
                     (long long*)sample_counts, (MlmState*)state);
  return launched();
}

}  // extern "C"
