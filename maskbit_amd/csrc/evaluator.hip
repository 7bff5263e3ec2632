// Tokenizer evaluation metrics of the reference's TokenizerEvaluator.update (evaluator/evaluator.py:262-375) on gfx950: MAE, MSE, PSNR and SSIM
// from ONE read of the two images, and the codebook histogram behind CodebookUsage / CodebookEntropy.
//
// eval_images_kernel: a workgroup owns one 32 x 32 tile of one (image, channel) plane.  It stages the tile plus the 5-pixel halo of the 11 x 11
// SSIM window of both images in LDS (42 x 42 each), resolving F.pad(mode="reflect") on the load (-i -> i, H-1+i -> H-1-i: H, W >= 6), optionally
// clamping to [0, 1] (the two clamp passes of scripts/eval_tokenizer.py:146-147).  The five fields x, y, x^2, y^2, xy are filtered separably in
// fp32 -- 11 taps along the rows into LDS, 11 taps down the columns in registers -- with the 1-D weights of gaussian(11, 1.5) as the reference
// builds them in fp32 (evaluator.py:44-56; the reference convolves with the fp32-rounded outer product of the same vector), then the SSIM
// expression of evaluator.py:320-333 per pixel in fp32.  |f - r| and (f - r)^2 come from the staged interior: the difference of two fp32 values is
// exact in fp64, its square and absolute value are summed in fp64, and so are the per-pixel SSIM values (evaluator.py:334 sums them in fp64).
// No floating-point atomics: a workgroup reduces in a fixed order and writes its three sums to a workspace slot of its own.  The tiling depends on
// (H, W) alone, so an image's partial sums do not depend on the batch it sits in.
//
// eval_finalize_kernel (one workgroup): per image the partials are summed in a fixed order into per_image[B][3]; then one thread adds the
// reference's per-image terms to the caller's running sums IN IMAGE ORDER (evaluator.py:282-294,334 add the per-image means of a batch), so a
// batch split into consecutive updates leaves bit-identical sums.
//
// eval_codebook_kernel: hist[idx] += 1 with integer vector atomics (exact, order-independent); this one histogram replaces both torch.unique
// calls and the Python set of evaluator.py:370-375.  Indices outside [0, K) are not counted; they increment a counter of their own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <climits>

#include "../../include/maskbit_hip.h"
#include "mb_abi.h"

namespace mb {

namespace {

constexpr int EV_T = 32;                 // tile side
constexpr int EV_R = 5;                  // window radius (11 taps)
constexpr int EV_S = EV_T + 2 * EV_R;    // staged side
constexpr int EV_SP = EV_S + 1;          // staged row pitch
constexpr int EV_THREADS = 256;

// gaussian(11, 1.5) of the reference in fp32, bit for bit (tests/golden/evaluator.npz window_1d; tests/test_evaluator_cpu.py compares)
#define EV_GAUSS_1D                                                                                                                       \
  { 0x1.0d957p-10f, 0x1.f1fdf8p-8f, 0x1.26eb18p-5f, 0x1.bff0fcp-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f, 0x1.b43c3ep-3f, 0x1.bff0fcp-4f,       \
    0x1.26eb18p-5f, 0x1.f1fdf8p-8f, 0x1.0d957p-10f }

__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);          // only positions no counted pixel reads (past the halo of a ragged edge tile) are clamped
}

__device__ __forceinline__ float load_px(const float* __restrict__ p, int clamp01) {
  const float v = *p;
  return clamp01 ? fminf(fmaxf(v, 0.0f), 1.0f) : v;
}

// sums of the workgroup in a fixed order -> part[0..2]
__device__ __forceinline__ void block_sums(double sa, double sq, double ss, double (*red)[3], double* __restrict__ part) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    sa += __shfl_xor(sa, o);
    sq += __shfl_xor(sq, o);
    ss += __shfl_xor(ss, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = sa; red[wave][1] = sq; red[wave][2] = ss; }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = red[0][threadIdx.x];
    for (int w = 1; w < EV_THREADS / 64; ++w) t += red[w][threadIdx.x];
    part[threadIdx.x] = t;
  }
}

// grid (tiles, C, B); part [B][C][tiles][3] = sum |d|, sum d^2, sum SSIM over the tile's pixels inside the image
template <bool SSIM>
__global__ __launch_bounds__(EV_THREADS) void eval_images_kernel(const float* __restrict__ real, const float* __restrict__ fake, int H, int W,
                                                                 int tiles_x, int clamp01, double* __restrict__ part) {
  __shared__ double red[EV_THREADS / 64][3];
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * EV_T, y0 = ty * EV_T;
  const size_t plane = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * (size_t)H * W;
  const float* __restrict__ pf = fake + plane;
  const float* __restrict__ pr = real + plane;
  double* __restrict__ out = part + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 3;
  const int col = tid & (EV_T - 1), row4 = (tid >> 5) * 4;      // this thread's column and the first of its 4 rows
  const bool col_in = x0 + col < W;
  double sa = 0.0, sq = 0.0, ss = 0.0;

  if constexpr (!SSIM) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = y0 + row4 + j;
      if (col_in && y < H) {
        const size_t o = (size_t)y * W + x0 + col;
        const double d = (double)load_px(pf + o, clamp01) - (double)load_px(pr + o, clamp01);
        sa += fabs(d);
        sq += d * d;
      }
    }
    block_sums(sa, sq, ss, red, out);
    return;
  } else {
    __shared__ float sx[EV_S * EV_SP], sy[EV_S * EV_SP];      // fake (the reference's "pred"), real ("target")
    __shared__ float hf[5][EV_S][EV_T];                         // row-filtered x, y, x^2, y^2, xy
    const float g[11] = EV_GAUSS_1D;

    for (int i = tid; i < EV_S * EV_S; i += EV_THREADS) {
      const int r = i / EV_S, c = i - r * EV_S;
      const size_t o = (size_t)reflect(y0 - EV_R + r, H) * W + reflect(x0 - EV_R + c, W);
      sx[r * EV_SP + c] = load_px(pf + o, clamp01);
      sy[r * EV_SP + c] = load_px(pr + o, clamp01);
    }
    __syncthreads();

    // along the rows: one item = 4 consecutive outputs of one staged row
    for (int it = tid; it < EV_S * (EV_T / 4); it += EV_THREADS) {
      const int r = it >> 3, s = (it & 7) * 4;
      float vx[14], vy[14];
#pragma unroll
      for (int k = 0; k < 14; ++k) { vx[k] = sx[r * EV_SP + s + k]; vy[k] = sy[r * EV_SP + s + k]; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int t = 0; t < 11; ++t) {
          const float x = vx[j + t], y = vy[j + t];
          a0 = fmaf(g[t], x, a0);
          a1 = fmaf(g[t], y, a1);
          a2 = fmaf(g[t], x * x, a2);
          a3 = fmaf(g[t], y * y, a3);
          a4 = fmaf(g[t], x * y, a4);
        }
        hf[0][r][s + j] = a0; hf[1][r][s + j] = a1; hf[2][r][s + j] = a2; hf[3][r][s + j] = a3; hf[4][r][s + j] = a4;
      }
    }
    __syncthreads();

    // down the columns: 4 consecutive output rows of one column per thread
    float o[5][4];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      float v[14];
#pragma unroll
      for (int k = 0; k < 14; ++k) v[k] = hf[f][row4 + k][col];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float a = 0.f;
#pragma unroll
        for (int t = 0; t < 11; ++t) a = fmaf(g[t], v[j + t], a);
        o[f][j] = a;
      }
    }
    const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);      // (k1 * data_range)^2, (k2 * data_range)^2: evaluator.py:201-202
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (col_in && y0 + row4 + j < H) {
        const int si = (row4 + j + EV_R) * EV_SP + col + EV_R;
        const double d = (double)sx[si] - (double)sy[si];
        sa += fabs(d);
        sq += d * d;
        const float mu_pp = o[0][j] * o[0][j], mu_tt = o[1][j] * o[1][j], mu_pt = o[0][j] * o[1][j];
        // E[x^2] - mu^2 cancels: the fused form subtracts the exact product
        const float s_pp = fmaf(-o[0][j], o[0][j], o[2][j]), s_tt = fmaf(-o[1][j], o[1][j], o[3][j]), s_pt = fmaf(-o[0][j], o[1][j], o[4][j]);
        const float a1 = 2.0f * mu_pt + c1, a2 = 2.0f * s_pt + c2;
        const float b1 = mu_pp + mu_tt + c1, b2 = s_pp + s_tt + c2;
        ss += (double)((a1 * a2) / (b1 * b2));
      }
    }
    block_sums(sa, sq, ss, red, out);
  }
}

// one workgroup; part [B][P][3] -> per_image [B][3] (0 where the metric was not asked for), sums[4] += per-image MAE, MSE, PSNR, SSIM terms
__global__ __launch_bounds__(EV_THREADS) void eval_finalize_kernel(const double* __restrict__ part, int B, int P, double npix, unsigned metrics,
                                                                   double* __restrict__ per_image, double* __restrict__ sums) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += EV_THREADS / 64) {
    double a[3] = {0.0, 0.0, 0.0};
    for (int p = lane; p < P; p += 64) {
      const double* q = part + ((size_t)b * P + p) * 3;
      a[0] += q[0]; a[1] += q[1]; a[2] += q[2];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      a[0] += __shfl_xor(a[0], o); a[1] += __shfl_xor(a[1], o); a[2] += __shfl_xor(a[2], o);
    }
    if (lane == 0) {
      per_image[(size_t)b * 3 + 0] = (metrics & 1u) ? a[0] : 0.0;
      per_image[(size_t)b * 3 + 1] = (metrics & 2u) ? a[1] : 0.0;
      per_image[(size_t)b * 3 + 2] = (metrics & 4u) ? a[2] : 0.0;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double mae = sums[0], mse = sums[1], psnr = sums[2], ssim = sums[3];
  for (int b = 0; b < B; ++b) {                           // image order
    const double* q = per_image + (size_t)b * 3;
    if (metrics & 1u) mae += q[0] / npix;
    if (metrics & 2u) {
      const double m = q[1] / npix;
      mse += m;
      psnr += 10.0 * log10(1.0 / (m + 1e-10));            // data_range = 1: evaluator.py:291-292
    }
    if (metrics & 4u) ssim += q[2] / npix;
  }
  sums[0] = mae; sums[1] = mse; sums[2] = psnr; sums[3] = ssim;
}

__global__ __launch_bounds__(EV_THREADS) void eval_codebook_kernel(const int64_t* __restrict__ idx, int64_t n, int K,
                                                                   unsigned long long* __restrict__ hist, unsigned* __restrict__ out_of_range) {
  unsigned bad = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t v = idx[i];
    if (v >= 0 && v < K) atomicAdd(hist + v, 1ull);
    else ++bad;
  }
  if (bad) atomicAdd(out_of_range, bad);
}

inline int tiles_of(int n) { return (n + EV_T - 1) / EV_T; }

bool eval_shape_ok(int B, int C, int H, int W) {
  if (B < 1 || B > 65535 || C < 1 || C > 65535 || H <= EV_R || W <= EV_R) return false;      // H, W >= 6: reflect needs n > radius
  return (long long)tiles_of(H) * tiles_of(W) <= INT_MAX / 4 && (long long)C * tiles_of(H) * tiles_of(W) <= INT_MAX / 4;
}

}  // namespace

}  // namespace mb

using namespace mb;

extern "C" {

size_t mb_eval_workspace_bytes(int B, int C, int H, int W) {
  if (!eval_shape_ok(B, C, H, W)) return 0;
  return (size_t)B * C * tiles_of(H) * tiles_of(W) * 3 * sizeof(double);
}

int mb_eval_images(const float* real, const float* fake, int B, int C, int H, int W, unsigned metrics, int clamp01, void* workspace,
                   double* per_image, double* sums, mb_stream stream) {
  if (!real || !fake || !workspace || !per_image || !sums) return fail(-1, "mb_eval_images: null argument");
  if (!eval_shape_ok(B, C, H, W)) return fail(-1, "mb_eval_images: B, C in [1, 65535] and H, W >= 6 required (got %d x %d x %d x %d)", B, C, H, W);
  if (metrics == 0 || (metrics & ~7u)) return fail(-1, "mb_eval_images: metrics is a mask of bits 0 (abs), 1 (sq + psnr), 2 (ssim)");
  if ((metrics & 4u) && C != 3) return fail(-1, "mb_eval_images: SSIM takes 3 channels (evaluator.py:298), got %d", C);
  if ((uintptr_t)workspace % sizeof(double)) return fail(-1, "mb_eval_images: workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("eval_images", s);
  const int tx = tiles_of(W), ty = tiles_of(H);
  const dim3 grid(tx * ty, C, B);
  double* part = (double*)workspace;
  if (metrics & 4u) hipLaunchKernelGGL(eval_images_kernel<true>, grid, dim3(EV_THREADS), 0, s, real, fake, H, W, tx, clamp01 ? 1 : 0, part);
  else hipLaunchKernelGGL(eval_images_kernel<false>, grid, dim3(EV_THREADS), 0, s, real, fake, H, W, tx, clamp01 ? 1 : 0, part);
  hipLaunchKernelGGL(eval_finalize_kernel, dim3(1), dim3(EV_THREADS), 0, s, part, B, C * tx * ty, (double)C * H * W, metrics, per_image, sums);
  return launched();
}

int mb_eval_codebook(const int64_t* indices, int64_t n, int K, int64_t* hist, unsigned* out_of_range, mb_stream stream) {
  if (!indices || !hist || !out_of_range) return fail(-1, "mb_eval_codebook: null argument");
  if (n < 0 || K < 1) return fail(-1, "mb_eval_codebook: n >= 0 and K >= 1 required");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("eval_codebook", s);
  const unsigned blocks = (unsigned)std::min<int64_t>(1024, (n + EV_THREADS - 1) / EV_THREADS);
  hipLaunchKernelGGL(eval_codebook_kernel, dim3(blocks), dim3(EV_THREADS), 0, s, indices, n, K, (unsigned long long*)hist, out_of_range);
  return launched();
}

}  // extern "C"
