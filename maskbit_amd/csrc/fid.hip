// The running statistics behind FID and the Inception Score of the reference's GeneratorEvaluator.update (evaluator/evaluator.py:549-569; the
// tokenizer's rFID, :336-364, keeps the same two states for real and for fake features) on gfx950.
//
// fid_accumulate_kernel: total += sum_n f_n and sigma += F^T F for a batch F [B, D] -- the reference's per-image torch.outer(f, f) (a D x D fp64
// temporary) and `sigma += ...`, B times over -- as ONE read-modify-write of the state, in fp64 on v_mfma_f64_16x16x4_f64.  A workgroup of four
// waves owns one 64 x 64 block of sigma on or above the diagonal; a wave owns a 16 x 64 strip of it, four 16 x 16 accumulators that START from the
// loaded sigma tiles and chain the batch's rows four at a time in increasing order.  Both MFMA operands are row slices of F (A[i][k] = F[n0+k][i0+i],
// B[k][j] = F[n0+k][j0+j]: lane l reads F[n0 + (l >> 4)][x0 + (l & 15)], 16 consecutive values per row), fp32 input is widened exactly, columns
// past D and rows past B load as exact zeros, stores are guarded.  Every output element belongs to one wave and there are no floating-point atomics,
// so the result is bitwise reproducible, and a batch split at a multiple of 4 rows leaves the bits of the unsplit batch.  Blocks BELOW the diagonal
// are not touched (the state is 32 MiB at D = 2048 and this kernel is bound by its read-modify-write): whoever reads the matrix mirrors the upper
// triangle first (GeneratorEvaluator.fid_statistics).  The diagonal blocks also chain `total` column by column in row order.
//
// f64 C/D layout (unlike every other MFMA shape): col = lane & 15, row = (lane >> 4) + 4 * reg.
//
// is_rows_kernel / is_columns_kernel: softmax(logits) in fp64 with the row maximum subtracted -- a workgroup per row leaves (max, sum exp) in the
// workspace, the sum carried as a (hi, lo) pair and rounded once -- then per column p and p * log(p + 1e-16) are added over the batch in a fixed order (four waves take a
// quarter of the rows each, in row order; their sums are added in wave order) into sums that start at zero and are added to the running totals
// once (evaluator.py:553-564: the batch sums are formed first, then added).  Deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/maskbit_hip.h"
#include "mb_abi.h"

namespace mb {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FID_BLOCK = 64;            // side of a workgroup's block of sigma
constexpr int FID_THREADS = 256;         // four waves, one 16-row strip each
constexpr int FID_MAX_D = 1 << 20;
constexpr int FID_MAX_B = 1 << 20;
constexpr int IS_THREADS = 256;

template <class T>
__device__ __forceinline__ double load_or_zero(const T* __restrict__ f, int64_t row_stride, int n, int B, int c, int D) {
  return (n < B && c < D) ? (double)f[(int64_t)n * row_stride + c] : 0.0;
}

// grid (nb, nb), nb = ceil(D / 64); blocks with blockIdx.y > blockIdx.x (below the diagonal) return at once
template <class T>
__global__ __launch_bounds__(FID_THREADS) void fid_accumulate_kernel(const T* __restrict__ f, int B, int D, int64_t row_stride,
                                                                     double* __restrict__ total, double* __restrict__ sigma) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = bi * FID_BLOCK + wave * 16, j0 = bj * FID_BLOCK;
  const int lc = lane & 15, lk = lane >> 4;

  if (i0 < D) {                                            // wave-uniform: a strip wholly past the edge has nothing to store
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + lk + 4 * r, col = j0 + 16 * t + lc;
        acc[t][r] = (row < D && col < D) ? sigma[(size_t)row * D + col] : 0.0;
      }
    }
    // rows in increasing order, four per instruction; 16 rows' loads are issued together, the tail goes four at a time and is zero-padded
    int n0 = 0;
    for (; n0 + 16 <= B; n0 += 16) {
      double a[4], b[4][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int n = n0 + 4 * s + lk;
        a[s] = load_or_zero(f, row_stride, n, B, i0 + lc, D);
#pragma unroll
        for (int t = 0; t < 4; ++t) b[s][t] = load_or_zero(f, row_stride, n, B, j0 + 16 * t + lc, D);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], b[s][t], acc[t], 0, 0, 0);
      }
    }
    for (; n0 < B; n0 += 4) {
      const int n = n0 + lk;
      const double a = load_or_zero(f, row_stride, n, B, i0 + lc, D);
      double b[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) b[t] = load_or_zero(f, row_stride, n, B, j0 + 16 * t + lc, D);
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + lk + 4 * r, col = j0 + 16 * t + lc;
        if (row < D && col < D) sigma[(size_t)row * D + col] = acc[t][r];
      }
    }
  }

  if (bi == bj && threadIdx.x < FID_BLOCK) {               // total: one thread per column of the diagonal block, rows in order
    const int c = j0 + threadIdx.x;
    if (c < D) {
      double t = total[c];
      for (int n = 0; n < B; ++n) t += (double)f[(int64_t)n * row_stride + c];
      total[c] = t;
    }
  }
}

// (hi, lo) += (b_hi, b_lo): hi + b_hi with its exact rounding error (Knuth's TwoSum, symmetric in its operands) collected in lo
__device__ __forceinline__ void two_sum(double& hi, double& lo, double b_hi, double b_lo) {
  const double s = hi + b_hi;
  const double bb = s - hi;
  const double err = (hi - (s - bb)) + (b_hi - bb);
  hi = s;
  lo = (lo + b_lo) + err;
}

// grid (B); rows [B][2] = max_c x, sum_c exp(x - max) (the sum rounded once)
template <class T>
__global__ __launch_bounds__(IS_THREADS) void is_rows_kernel(const T* __restrict__ x, int C, int64_t row_stride, double* __restrict__ rows) {
  __shared__ double red[IS_THREADS / 64], red_lo[IS_THREADS / 64];
  __shared__ double row_max;
  const T* __restrict__ p = x + (int64_t)blockIdx.x * row_stride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double m = -INFINITY;
  for (int c = threadIdx.x; c < C; c += IS_THREADS) m = fmax(m, (double)p[c]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
    for (int w = 1; w < IS_THREADS / 64; ++w) t = fmax(t, red[w]);
    row_max = t;
  }
  __syncthreads();
  m = row_max;
  // the sum of the exponentials as an unevaluated (hi, lo) pair through the whole reduction: next to a dominant 1 a plain sum rounds every small
  // term to the grid of the 1, and log(p + 1e-16) close to p = 1 turns one unit of the sum's last place into an absolute error of the term
  double hi = 0.0, lo = 0.0;
  for (int c = threadIdx.x; c < C; c += IS_THREADS) two_sum(hi, lo, exp((double)p[c] - m), 0.0);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) two_sum(hi, lo, __shfl_xor(hi, o), __shfl_xor(lo, o));
  if (lane == 0) { red[wave] = hi; red_lo[wave] = lo; }    // thread 0 read red[] before the barrier that published row_max
  __syncthreads();
  if (threadIdx.x == 0) {
    hi = red[0]; lo = red_lo[0];
    for (int w = 1; w < IS_THREADS / 64; ++w) two_sum(hi, lo, red[w], red_lo[w]);
    rows[(size_t)blockIdx.x * 2 + 0] = m;
    rows[(size_t)blockIdx.x * 2 + 1] = hi + lo;
  }
}

// grid (ceil(C / 64)); a workgroup owns 64 columns, lane = column; wave w sums the w-th quarter of the batch's rows in row order, then wave 0 adds
// the four partial sums in wave order: a fixed order whatever the launch
template <class T>
__global__ __launch_bounds__(IS_THREADS) void is_columns_kernel(const T* __restrict__ x, int B, int C, int64_t row_stride,
                                                                const double* __restrict__ rows, double* __restrict__ prob_total,
                                                                double* __restrict__ kl_total) {
  __shared__ double part[IS_THREADS / 64][64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int quarter = (B + IS_THREADS / 64 - 1) / (IS_THREADS / 64);
  const int n_end = min(B, (wave + 1) * quarter);
  double sp = 0.0, skl = 0.0;
  if (c < C) {
    for (int n = wave * quarter; n < n_end; ++n) {
      const double p = exp((double)x[(int64_t)n * row_stride + c] - rows[(size_t)n * 2]) / rows[(size_t)n * 2 + 1];
      sp += p;
      skl += p * log(p + 1e-16);                           // _is_eps, evaluator.py:509,558
    }
  }
  part[wave][lane][0] = sp;
  part[wave][lane][1] = skl;
  __syncthreads();
  if (wave != 0 || c >= C) return;
#pragma unroll
  for (int w = 1; w < IS_THREADS / 64; ++w) {
    sp += part[w][lane][0];
    skl += part[w][lane][1];
  }
  prob_total[c] += sp;
  kl_total[c] += skl;
}

bool rows_ok(int B, int N, int64_t row_stride) { return B >= 1 && B <= FID_MAX_B && N >= 1 && N <= FID_MAX_D && row_stride >= N; }

}  // namespace

}  // namespace mb

using namespace mb;

extern "C" {

int mb_fid_accumulate(const void* feats, int dtype, int B, int D, int64_t row_stride, double* total, double* sigma, mb_stream stream) {
  if (!feats || !total || !sigma) return fail(-1, "mb_fid_accumulate: null argument");
  if (dtype != 0 && dtype != 1) return fail(-1, "mb_fid_accumulate: dtype is 0 (fp32) or 1 (fp64), got %d", dtype);
  if (!rows_ok(B, D, row_stride))
    return fail(-1, "mb_fid_accumulate: B, D in [1, %d] and row_stride >= D required (got B %d, D %d, row_stride %lld)", FID_MAX_D, B, D,
                (long long)row_stride);
  if ((uintptr_t)feats % (dtype ? 8 : 4) || (uintptr_t)total % 8 || (uintptr_t)sigma % 8) return fail(-1, "mb_fid_accumulate: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("fid_accumulate", s);
  const unsigned nb = (unsigned)((D + FID_BLOCK - 1) / FID_BLOCK);
  if (dtype) hipLaunchKernelGGL(fid_accumulate_kernel<double>, dim3(nb, nb), dim3(FID_THREADS), 0, s, (const double*)feats, B, D, row_stride, total, sigma);
  else hipLaunchKernelGGL(fid_accumulate_kernel<float>, dim3(nb, nb), dim3(FID_THREADS), 0, s, (const float*)feats, B, D, row_stride, total, sigma);
  return launched();
}

size_t mb_is_workspace_bytes(int B, int C) {
  if (B < 1 || B > FID_MAX_B || C < 1 || C > FID_MAX_D) return 0;
  return (size_t)B * 2 * sizeof(double);
}

int mb_is_accumulate(const void* logits, int dtype, int B, int C, int64_t row_stride, double* prob_total, double* kl_total, void* workspace,
                     mb_stream stream) {
  if (!logits || !prob_total || !kl_total || !workspace) return fail(-1, "mb_is_accumulate: null argument");
  if (dtype != 0 && dtype != 1) return fail(-1, "mb_is_accumulate: dtype is 0 (fp32) or 1 (fp64), got %d", dtype);
  if (!rows_ok(B, C, row_stride))
    return fail(-1, "mb_is_accumulate: B, C in [1, %d] and row_stride >= C required (got B %d, C %d, row_stride %lld)", FID_MAX_D, B, C,
                (long long)row_stride);
  if ((uintptr_t)logits % (dtype ? 8 : 4) || (uintptr_t)prob_total % 8 || (uintptr_t)kl_total % 8 || (uintptr_t)workspace % 8)
    return fail(-1, "mb_is_accumulate: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("is_accumulate", s);
  double* rows = (double*)workspace;
  const unsigned cb = (unsigned)((C + 63) / 64);
  if (dtype) {
    hipLaunchKernelGGL(is_rows_kernel<double>, dim3(B), dim3(IS_THREADS), 0, s, (const double*)logits, C, row_stride, rows);
    hipLaunchKernelGGL(is_columns_kernel<double>, dim3(cb), dim3(IS_THREADS), 0, s, (const double*)logits, B, C, row_stride, rows, prob_total, kl_total);
  } else {
    hipLaunchKernelGGL(is_rows_kernel<float>, dim3(B), dim3(IS_THREADS), 0, s, (const float*)logits, C, row_stride, rows);
    hipLaunchKernelGGL(is_columns_kernel<float>, dim3(cb), dim3(IS_THREADS), 0, s, (const float*)logits, B, C, row_stride, rows, prob_total, kl_total);
  }
  return launched();
}

}  // extern "C"
