// The VQGAN+ discriminator (modeling/modules/discriminator.py NLayerDiscriminatorv2, the `VQGAN+Discriminator` of every MaskBit / VQGAN+ tokenizer
// config) on gfx950, inference only: fp32 images -> the fp32 logits [B, 1, 16, 16] and, per image, the five float64 sums that the GAN losses of
// gan_utils are functions of.  The graph is written out in DESIGN.md "Discriminator"; DiscNet below is its one statement in this library.
//
// Convolutions: inception.hip's convbn_kernel with scale = 1 and shift = the bias -- linear epilogue for the stage convolutions, the LeakyReLU
// epilogue for block_in and to_logits.0.  block_in (5 x 5 on 3 channels, K = 75) through the general walk would take 25 taps of a 32-channel MFMA
// step with 3 live channels: 800 K positions for 75.  disc_cols_kernel writes the im2col instead (96 channels a pixel, straight from the fp32
// image) and block_in runs as a 1 x 1 over 3 steps: 1.6 GFLOP of MFMA and 25 MB of traffic per 256 x 256 image at hidden 128 against 13.4 GFLOP.
//
// blur_down_kernel<K>: BlurBlock (K = 3, 4, 5) or AvgPool2d(2) (K = 0).  One workgroup per (pixel chunk, image); a thread owns an 8-channel slot of
// every npl-th output pixel, accumulates the K x K taps in fp32 ((ky, kx) order, one fma each, one rounding at the store) and keeps the sum and the
// sum of squares of those fp32 values; the workgroup combines them over its pixel lanes and over the channels of a group in a fixed order (each
// of the two upper levels accumulates in float64 and is rounded to fp32 where it is handed on -- the per-channel sum in LDS, the group's sum at
// the store -- as conv.hip's gn_partial_kernel does) and leaves one (sum, sumsq) per group.  disc_gn_finalize_kernel combines the
// chunks in float64 (eps 1e-5) into per-channel (scale, shift); disc_gn_apply_kernel is the pass in place over the quarter-size map.
//
// adaptive_maxpool16_kernel: one thread per (output pixel, 8-channel slot).  disc_logits_kernel: one workgroup per image, four threads per logit.
// Nothing here uses a floating-point atomic and every tile is an image's own: an image's logits and sums do not depend on the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/maskbit_hip.h"
#include "mb_abi.h"
#include "mb_convnet.h"
#include "mb_disc.h"
#include "mb_incep.h"

namespace mb {

namespace {

constexpr int DT = 256;

unsigned disc_grid(size_t n) { return (unsigned)std::min<size_t>(16384, std::max<size_t>(1, (n + DT - 1) / DT)); }

// one thread per (pixel, 8-channel slot)
__global__ __launch_bounds__(DT) void disc_cols_kernel(const float* __restrict__ img, h16* __restrict__ out, int B, int H, int W, int clamp01) {
  constexpr int NS = DISC_COLS_C / 8;
  const size_t HW = (size_t)H * W, total = (size_t)B * HW * NS;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int slot = (int)(i % NS);
    const size_t p = i / NS;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const size_t n = p / HW;
    h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = slot * 8 + e;
      if (k < DISC_COLS_K) {
        const int ci = k / 25, t = k - ci * 25, ky = t / 5, kx = t - ky * 5;
        const int Y = y - 2 + ky, X = x - 2 + kx;
        if (Y >= 0 && Y < H && X >= 0 && X < W) {
          float f = img[(n * 3 + ci) * HW + (size_t)Y * W + X];
          if (clamp01) f = fminf(fmaxf(f, 0.0f), 1.0f);
          v[e] = to_h(f);
        }
      }
    }
    *(h16x8*)(out + p * DISC_COLS_C + slot * 8) = v;
  }
}

// the binomial row of BlurBlock's kernel and the sum of its outer square
template <int K> __device__ __forceinline__ constexpr int blur_tap(int i) { return K == 3 ? (i == 1 ? 2 : 1) : K == 4 ? ((i == 1 || i == 2) ? 3 : 1) : (i == 2 ? 6 : (i == 1 || i == 3) ? 4 : 1); }
template <int K> __device__ __forceinline__ constexpr float blur_norm() { return K == 3 ? 1.0f / 16.0f : K == 4 ? 1.0f / 64.0f : 1.0f / 256.0f; }

// grid (nchunk, B)
template <int K>
__global__ __launch_bounds__(DT) void blur_down_kernel(const h16* __restrict__ x, h16* __restrict__ y, float* __restrict__ part, int H, int W, int Ho, int Wo,
                                                       int C, int nchunk, int pad_t, int pad_l) {
  __shared__ float red[2][DT * 8];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int nslot = C / 8, npl = DT / nslot;        // 8-channel slots per pixel, pixel lanes; threads beyond npl * nslot have no pixel
  const int slot = tid % nslot, pl = tid / nslot;
  const int HWo = Ho * Wo, per = (HWo + nchunk - 1) / nchunk;
  const int p0 = chunk * per, p1 = min(HWo, p0 + per);
  const h16* xb = x + (size_t)b * H * W * C + slot * 8;
  float s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
  if (pl < npl) {
    for (int p = p0 + pl; p < p1; p += npl) {
      const int oy = p / Wo, ox = p - oy * Wo;
      float acc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.f;
      if constexpr (K == 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const h16x8 v = *(const h16x8*)(xb + ((size_t)(2 * oy + (t >> 1)) * W + 2 * ox + (t & 1)) * C);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] = fmaf(0.25f, (float)v[e], acc[e]);
        }
      } else {
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
          const int iy = 2 * oy - pad_t + ky;
          if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
          for (int kx = 0; kx < K; ++kx) {
            const int ix = 2 * ox - pad_l + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const float w = (float)(blur_tap<K>(ky) * blur_tap<K>(kx)) * blur_norm<K>();
            const h16x8 v = *(const h16x8*)(xb + ((size_t)iy * W + ix) * C);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, (float)v[e], acc[e]);
          }
        }
      }
      h16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) { o[e] = to_h(acc[e]); s[e] += acc[e]; q[e] = fmaf(acc[e], acc[e], q[e]); }
      *(h16x8*)(y + ((size_t)b * HWo + p) * C + slot * 8) = o;
    }
  }
  if (!part) return;                                 // (uniform: every thread leaves here or none)
  if (pl < npl) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[0][pl * C + slot * 8 + e] = s[e]; red[1][pl * C + slot * 8 + e] = q[e]; }
  }
  __syncthreads();
  for (int c = tid; c < C; c += DT) {                // fixed-order sum over the pixel lanes
    double ts = 0.0, tq = 0.0;
    for (int l = 0; l < npl; ++l) { ts += (double)red[0][l * C + c]; tq += (double)red[1][l * C + c]; }
    red[0][c] = (float)ts; red[1][c] = (float)tq;    // row 0 of the scratch is only read by thread c here
  }
  __syncthreads();
  if (tid < 32) {
    const int cpg = C / 32;
    double ts = 0.0, tq = 0.0;
    for (int e = 0; e < cpg; ++e) { ts += (double)red[0][tid * cpg + e]; tq += (double)red[1][tid * cpg + e]; }
    float* o = part + (((size_t)b * nchunk + chunk) * 32 + tid) * 2;
    o[0] = (float)ts; o[1] = (float)tq;
  }
}

// grid B: 256 threads = 32 groups x 8 chunk lanes; lane l sums chunks l, l + 8, ... in order, then the 8 lanes are summed in order, in float64
__global__ __launch_bounds__(DT) void disc_gn_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              float2* __restrict__ out, int HW, int C, int nchunk, double eps) {
  __shared__ double red[2][8][32];
  __shared__ float2 ms[32];
  const int b = blockIdx.x, grp = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int cpg = C / 32;
  double ts = 0.0, tq = 0.0;
  for (int k = l; k < nchunk; k += 8) {
    const float* o = part + (((size_t)b * nchunk + k) * 32 + grp) * 2;
    ts += (double)o[0]; tq += (double)o[1];
  }
  red[0][l][grp] = ts; red[1][l][grp] = tq;
  __syncthreads();
  if (threadIdx.x < 32) {
    ts = 0.0; tq = 0.0;
    for (int k = 0; k < 8; ++k) { ts += red[0][k][grp]; tq += red[1][k][grp]; }
    const double n = (double)HW * (double)cpg;
    const double mean = ts / n;
    const double var = fmax(tq / n - mean * mean, 0.0);
    ms[grp] = make_float2((float)mean, (float)(1.0 / sqrt(var + eps)));
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float2 m = ms[c / cpg];
    const float sc = m.y * gamma[c];
    out[(size_t)b * C + c] = make_float2(sc, beta[c] - m.x * sc);
  }
}

// one thread per (pixel, 8-channel slot), in place
__global__ __launch_bounds__(DT) void disc_gn_apply_kernel(h16* __restrict__ x, const float2* __restrict__ ss, unsigned* __restrict__ sat, size_t B, size_t HW,
                                                           int C, float slope) {
  const int c8 = C / 8;
  const size_t per = HW * c8, total = B * per;
  unsigned nsat = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / per;
    const int c0 = (int)(i % c8) * 8;
    const float2* m = ss + b * C + c0;
    h16x8 v = *(const h16x8*)(x + i * 8);
    float big = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float t = fmaf((float)v[e], m[e].x, m[e].y);
      const float r = t >= 0.f ? t : __fmul_rn(t, slope);
      big = fmaxf(big, fabsf(r));
      v[e] = to_h(r);
    }
    nsat += big > MB_H16_MAX ? 1u : 0u;
    *(h16x8*)(x + i * 8) = v;
  }
  if (nsat && sat) atomicAdd(sat, nsat);
}

// one thread per (output pixel, 8-channel slot)
__global__ __launch_bounds__(DT) void adaptive_maxpool16_kernel(const h16* __restrict__ x, h16* __restrict__ y, int B, int H, int W, int C) {
  const int c8 = C / 8;
  const size_t total = (size_t)B * DISC_NLOGIT * c8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int slot = (int)(i % c8);
    const size_t p = i / c8;
    const int ox = (int)(p % DISC_SIDE), oy = (int)((p / DISC_SIDE) % DISC_SIDE);
    const size_t b = p / DISC_NLOGIT;
    const int y0 = oy * H / DISC_SIDE, y1 = ((oy + 1) * H + DISC_SIDE - 1) / DISC_SIDE;
    const int x0 = ox * W / DISC_SIDE, x1 = ((ox + 1) * W + DISC_SIDE - 1) / DISC_SIDE;
    const h16* xb = x + b * H * W * C + slot * 8;
    h16x8 m = *(const h16x8*)(xb + ((size_t)y0 * W + x0) * C);
    for (int yy = y0; yy < y1; ++yy)
      for (int xx = x0; xx < x1; ++xx) {
        const h16x8 v = *(const h16x8*)(xb + ((size_t)yy * W + xx) * C);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
      }
    *(h16x8*)(y + p * C + slot * 8) = m;
  }
}

__global__ void disc_logits_weight_kernel(const float* __restrict__ w, float* __restrict__ out, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 25 * C) return;
  const int tap = i / C, c = i - tap * C;
  out[i] = w[c * 25 + tap];
}

// a fixed tree over the first DT threads of the workgroup (the others pass through the barriers)
__device__ __forceinline__ double disc_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid < DT) red[tid] = v;
  __syncthreads();
  for (int o = DT / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// max(x, 0) + log1p(exp(-|x|)): no overflow at either end
__device__ __forceinline__ double softplus_d(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// grid B.  DISC_LQ threads per logit, each over one run of the channels (a whole number of 8-channel slots): thread (q, logit) chains the
// in-image taps in (ky, kx) order over its channels, q = 0 starting from the bias; the logit is ((p0 + p1) + p2) + p3 in fp32.  One workgroup
// per image alone left the chip to 4 waves an image; this is 16.
constexpr int DISC_LQ = 4;
__global__ __launch_bounds__(DT * DISC_LQ) void disc_logits_kernel(const h16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                   float* __restrict__ logits, double* __restrict__ stats, int C) {
  __shared__ double red[DT];
  __shared__ float part[DISC_LQ][DT];
  const int tid = threadIdx.x, q = tid / DT, lg = tid - q * DT, oy = lg / DISC_SIDE, ox = lg - oy * DISC_SIDE;
  const size_t b = blockIdx.x;
  const h16* xb = x + b * DISC_NLOGIT * C;
  const int run = (C / 8 + DISC_LQ - 1) / DISC_LQ * 8, c0 = min(q * run, C), c1 = min(c0 + run, C);
  float acc = q == 0 ? bias[0] : 0.f;
  for (int ky = 0; ky < 5; ++ky) {
    const int iy = oy - 2 + ky;
    for (int kx = 0; kx < 5; ++kx) {
      const int ix = ox - 2 + kx;
      if ((unsigned)iy >= (unsigned)DISC_SIDE || (unsigned)ix >= (unsigned)DISC_SIDE) continue;
      const h16* px = xb + (size_t)(iy * DISC_SIDE + ix) * C;
      const float* wt = w + (size_t)(ky * 5 + kx) * C;
      for (int c = c0; c < c1; c += 8) {
        const h16x8 v = *(const h16x8*)(px + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __fmaf_rn((float)v[e], wt[c + e], acc);
      }
    }
  }
  part[q][lg] = acc;
  __syncthreads();
  float l32 = part[0][lg];
#pragma unroll
  for (int k = 1; k < DISC_LQ; ++k) l32 = __fadd_rn(l32, part[k][lg]);
  if (logits && q == 0) logits[b * DISC_NLOGIT + lg] = l32;
  if (!stats) return;                                // (uniform)
  const double l = (double)l32;
  const double t[DISC_NSTAT] = {l, fmax(1.0 - l, 0.0), fmax(1.0 + l, 0.0), softplus_d(-l), softplus_d(l)};
#pragma unroll
  for (int k = 0; k < DISC_NSTAT; ++k) {
    const double v = disc_block_sum(t[k], red);      // (the threads of q = 0 hold the logits in order)
    if (tid == 0) stats[b * DISC_NSTAT + k] = v;
  }
}

__global__ void disc_sum_kernel(const double* __restrict__ stats, int B, double* __restrict__ sum) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  for (int k = 0; k < DISC_NSTAT; ++k) {
    double t = sum[k];
    for (int b = 0; b < B; ++b) t += stats[(size_t)b * DISC_NSTAT + k];
    sum[k] = t;
  }
}

}  // namespace

void launch_disc_cols(hipStream_t s, const float* img, h16* out, int B, int H, int W, int clamp01) {
  hipLaunchKernelGGL(disc_cols_kernel, dim3(disc_grid((size_t)B * H * W * (DISC_COLS_C / 8))), dim3(DT), 0, s, img, out, B, H, W, clamp01 ? 1 : 0);
}

void launch_disc_down(hipStream_t s, const h16* x, h16* y, float* part, int B, int H, int W, int C, int K) {
  const int Ho = disc_down_size(H, K), Wo = disc_down_size(W, K), nchunk = disc_down_chunks(Ho, Wo, C);
  const int pt = K ? disc_blur_pad(H, K) / 2 : 0, pl = K ? disc_blur_pad(W, K) / 2 : 0;
  const dim3 grid(nchunk, B), block(DT);
  if (K == 0) hipLaunchKernelGGL(blur_down_kernel<0>, grid, block, 0, s, x, y, part, H, W, Ho, Wo, C, nchunk, pt, pl);
  else if (K == 3) hipLaunchKernelGGL(blur_down_kernel<3>, grid, block, 0, s, x, y, part, H, W, Ho, Wo, C, nchunk, pt, pl);
  else if (K == 4) hipLaunchKernelGGL(blur_down_kernel<4>, grid, block, 0, s, x, y, part, H, W, Ho, Wo, C, nchunk, pt, pl);
  else hipLaunchKernelGGL(blur_down_kernel<5>, grid, block, 0, s, x, y, part, H, W, Ho, Wo, C, nchunk, pt, pl);
}

void launch_disc_gn(hipStream_t s, h16* x, const float* part, int nchunk, const float* gamma, const float* beta, float2* ss, unsigned* sat, int B,
                    int HW, int C, double eps, float slope) {
  hipLaunchKernelGGL(disc_gn_finalize_kernel, dim3(B), dim3(DT), 0, s, part, gamma, beta, ss, HW, C, nchunk, eps);
  hipLaunchKernelGGL(disc_gn_apply_kernel, dim3(disc_grid((size_t)B * HW * (C / 8))), dim3(DT), 0, s, x, ss, sat, (size_t)B, (size_t)HW, C, slope);
}

void launch_disc_pool(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C) {
  hipLaunchKernelGGL(adaptive_maxpool16_kernel, dim3(disc_grid((size_t)B * DISC_NLOGIT * (C / 8))), dim3(DT), 0, s, x, y, B, H, W, C);
}

void launch_disc_logits_weight(hipStream_t s, const float* w_oihw, float* out, int C) {
  hipLaunchKernelGGL(disc_logits_weight_kernel, dim3((25 * C + DT - 1) / DT), dim3(DT), 0, s, w_oihw, out, C);
}

void launch_disc_logits(hipStream_t s, const h16* x, const float* w, const float* bias, float* logits, double* stats, double* sum, int B, int C) {
  hipLaunchKernelGGL(disc_logits_kernel, dim3(B), dim3(DT * DISC_LQ), 0, s, x, w, bias, logits, stats, C);
  if (sum && stats) hipLaunchKernelGGL(disc_sum_kernel, dim3(1), dim3(1), 0, s, stats, B, sum);
}

// ---- the network ------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int DISC_MIN_HW = 32, DISC_MAX_HW = 512, DISC_HW_STEP = 16;
constexpr int DISC_MAX_STAGES = 4, DISC_MAX_C = 2048;

struct DiscNorm { int c = 0; float *g = nullptr, *b = nullptr; };

// cn.convs: block_in.0, blocks.{i}.0 for every stage, to_logits.0 -- each with its bias as the epilogue's shift and a scale of ones
struct DiscNet {
  int hidden = 0, stages = 0, blur = 0, c_last = 0;
  std::vector<DiscNorm> norms;
  std::vector<std::string> blur_keys;                            // blocks.{i}.1.kernel: checked against the binomial kernel, not stored
  float *ones = nullptr, *wl_raw = nullptr, *wl = nullptr, *bl = nullptr;   // to_logits.2: the checkpoint's [1, c, 5, 5], the kernel's [25][c], the bias

  int add(ConvNet& cn, const std::string& prefix, int cin, int cout, int k) {
    CnConv c;
    c.key = prefix + ".weight"; c.cin = cin; c.cout = cout; c.kh = c.kw = k; c.ph = c.pw = k / 2;
    c.shape[0] = cout; c.shape[1] = cin; c.shape[2] = c.shape[3] = k;
    cn.mem.get(&c.w, (size_t)k * k * ic_cout_pad(cout) * ic_cin_pad(cin));
    cn.mem.zeroed(&c.shift, (size_t)cout);
    c.scale = ones;
    const int i = (int)cn.convs.size();
    cn.convs.push_back(c);
    name_slot(cn, c.key, CnSlot{CN_WEIGHT, i});
    add_vec(cn, prefix + ".bias", c.shift, (size_t)cout);
    return i;
  }

  void build(ConvNet& cn, int hidden_, int stages_, int blur_) {
    hidden = hidden_; stages = stages_; blur = blur_;
    c_last = hidden << (stages - 1);
    cn.mem.zeroed(&cn.sat, 1);
    cn.mem.get(&ones, (size_t)c_last);
    CnConv& in = cn.convs[add(cn, "block_in.0", DISC_COLS_K, hidden, 1)];
    in.shape[1] = 3; in.shape[2] = in.shape[3] = 5;              // [h, 3, 5, 5] read as [h, 75, 1, 1]: the same memory
    int cin = hidden;
    for (int i = 0; i < stages; ++i) {
      const std::string p = "blocks." + std::to_string(i);
      const int cout = hidden << i;
      add(cn, p + ".0", cin, cout, 3);
      if (blur) { blur_keys.push_back(p + ".1.kernel"); name_slot(cn, blur_keys.back(), CnSlot{}); }
      DiscNorm n;
      n.c = cout;
      cn.mem.get(&n.g, (size_t)cout); cn.mem.get(&n.b, (size_t)cout);
      add_vec(cn, p + ".2.weight", n.g, (size_t)cout);
      add_vec(cn, p + ".2.bias", n.b, (size_t)cout);
      norms.push_back(n);
      cin = cout;
    }
    add(cn, "to_logits.0", c_last, c_last, 1);
    cn.mem.get(&wl_raw, (size_t)25 * c_last); cn.mem.get(&wl, (size_t)25 * c_last); cn.mem.get(&bl, 1);
    add_vec(cn, "to_logits.2.weight", wl_raw, (size_t)25 * c_last);
    add_vec(cn, "to_logits.2.bias", bl, 1);
  }
};

}  // namespace

}  // namespace mb

struct mb_disc {
  int max_images = 0;
  size_t cap_pix = 0;              // pixels of input image the workspace holds: a chunk is as many images as fit, 4 max_images at the most
  int max_chunk = 0;
  mb::ConvNet cn;                  // the convolutions, the checkpoint table, the saturation counter, the arena (mb_convnet.h)
  mb::DiscNet net;
  h16 *cols = nullptr, *p = nullptr, *q = nullptr;
  float* part = nullptr;
  float2* ss = nullptr;
  double* stats = nullptr;         // the chunk's sums when the caller wants only the running sum
};

using namespace mb;

namespace {

// one chunk of n images through the graph; the buffers p and q hold a layer's input and output in turn
void run_disc(mb_disc* h, const float* img, int n, int H, int W, int clamp01, float* logits, double* stats, double* sum, hipStream_t s) {
  const DiscNet& net = h->net;
  unsigned* sat = h->cn.sat;
  { ProfScope pc("disc_block_in", s);
    launch_disc_cols(s, img, h->cols, n, H, W, clamp01);
    const CnConv& c = h->cn.convs[0];
    launch_convbn(s, ConvBn{h->cols, c.w, c.scale, c.shift, h->p, sat, n, H, W, c.cin, c.cout, 1, 1, 1, 0, 0, 0, DISC_COLS_C, 0, c.cout, CONVBN_LEAKY, DISC_SLOPE}); }
  int hh = H, ww = W, cin = net.hidden;
  for (int i = 0; i < net.stages; ++i) {
    const CnConv& c = h->cn.convs[1 + i];
    { ProfScope pc("disc_conv", s);
      launch_convbn(s, ConvBn{h->p, c.w, c.scale, c.shift, h->q, sat, n, hh, ww, cin, c.cout, 3, 3, 1, 1, 1, 0, cin, 0, c.cout, CONVBN_LINEAR}); }
    const int ho = disc_down_size(hh, net.blur), wo = disc_down_size(ww, net.blur);
    { ProfScope pc("disc_down", s);
      launch_disc_down(s, h->q, h->p, h->part, n, hh, ww, c.cout, net.blur); }
    { ProfScope pc("disc_gn", s);
      const DiscNorm& g = net.norms[i];
      launch_disc_gn(s, h->p, h->part, disc_down_chunks(ho, wo, c.cout), g.g, g.b, h->ss, sat, n, ho * wo, c.cout, DISC_GN_EPS, DISC_SLOPE); }
    hh = ho; ww = wo; cin = c.cout;
  }
  ProfScope pc("disc_head", s);
  launch_disc_pool(s, h->p, h->q, n, hh, ww, cin);
  const CnConv& c = h->cn.convs[1 + net.stages];
  launch_convbn(s, ConvBn{h->q, c.w, c.scale, c.shift, h->p, sat, n, DISC_SIDE, DISC_SIDE, cin, cin, 1, 1, 1, 0, 0, 0, cin, 0, cin, CONVBN_LEAKY, DISC_SLOPE});
  launch_disc_logits(s, h->p, net.wl, net.bl, logits, stats, sum, n, cin);
}

}  // namespace

extern "C" {

int mb_disc_create(int max_images, int hidden, int stages, int blur_kernel, mb_disc** out) {
  if (!out || max_images < 1 || max_images > 256) return fail(-1, "mb_disc_create: bad arguments (1 <= max_images <= 256)");
  if (hidden < 32 || hidden % 32 || stages < 1 || stages > DISC_MAX_STAGES || (hidden << (stages - 1)) > DISC_MAX_C)
    return fail(-1, "mb_disc_create: hidden %d, %d stages: hidden a multiple of 32, 1 .. %d stages, at most %d channels in the last", hidden, stages,
                DISC_MAX_STAGES, DISC_MAX_C);
  if (blur_kernel != 0 && (blur_kernel < 3 || blur_kernel > 5)) return fail(-1, "mb_disc_create: blur kernel %d: 3, 4, 5, or 0 for the average pool", blur_kernel);
  mb_disc* h = new mb_disc();
  h->max_images = max_images;
  h->cap_pix = std::max<size_t>((size_t)max_images * 256 * 256, (size_t)DISC_MAX_HW * DISC_MAX_HW);
  h->max_chunk = 4 * max_images;
  h->net.build(h->cn, hidden, stages, blur_kernel);
  DevArena& m = h->cn.mem;
  const size_t c_last = (size_t)h->net.c_last;
  // the widest map per input pixel: hidden channels at full size, or the pooled 16 x 16 x c_last of a 32 x 32 image
  const size_t width = std::max<size_t>((size_t)hidden, c_last / 4);
  m.get(&h->cols, h->cap_pix * DISC_COLS_C); m.get(&h->p, h->cap_pix * width); m.get(&h->q, h->cap_pix * width);
  m.get(&h->part, (size_t)h->max_chunk * DISC_MAX_CHUNKS * 64); m.get(&h->ss, (size_t)h->max_chunk * c_last);
  m.get(&h->stats, (size_t)h->max_chunk * DISC_NSTAT);
  if (int rc = m.failed("mb_disc_create")) { delete h; return rc; }
  const std::vector<float> one(c_last, 1.0f);
  if (hipMemcpy(h->net.ones, one.data(), c_last * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    delete h;
    return fail(-10, "mb_disc_create: copy failed");
  }
  *out = h;
  return 0;
}

void mb_disc_destroy(mb_disc* h) { delete h; }

int mb_disc_load(mb_disc* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!h || !name || !data || !shape || ndim < 0) return fail(-1, "mb_disc_load: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const std::string key(name);
  if (std::find(h->net.blur_keys.begin(), h->net.blur_keys.end(), key) != h->net.blur_keys.end()) {
    // the blur is the handle's own (blur_down_kernel): the checkpoint's buffer must be that kernel.  Synchronises the stream
    const int K = h->net.blur;
    if (ndim != 4 || shape[0] != 1 || shape[1] != 1 || shape[2] != K || shape[3] != K) return fail(-4, "mb_disc_load: %s: expected [1, 1, %d, %d]", name, K, K);
    float got[25];
    if (hipMemcpyAsync(got, data, (size_t)K * K * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
      return fail(-10, "mb_disc_load: copy failed");
    const int row[3][5] = {{1, 2, 1, 0, 0}, {1, 3, 3, 1, 0}, {1, 4, 6, 4, 1}};
    const float norm = K == 3 ? 16.f : K == 4 ? 64.f : 256.f;
    for (int i = 0; i < K * K; ++i)
      if (got[i] != (float)(row[K - 3][i / K] * row[K - 3][i % K]) / norm)
        return fail(-4, "mb_disc_load: %s is not the binomial blur kernel of size %d that the handle computes", name, K);
    return 0;
  }
  if (int rc = load_entry("mb_disc_load", h->cn, name, key, data, shape, ndim, s)) return rc;
  if (key == "to_logits.2.weight") {
    launch_disc_logits_weight(s, h->net.wl_raw, h->net.wl, h->net.c_last);
    return launched();
  }
  return 0;
}

int mb_disc_forward(mb_disc* h, const float* images, int B, int H, int W, int clamp01, float* logits, double* stats, double* sum, mb_stream stream) {
  if (!h || !images) return fail(-1, "mb_disc_forward: null argument");
  if (int rc = complete("mb_disc_forward", h->cn)) return rc;
  if (B < 1 || B > (1 << 20)) return fail(-1, "mb_disc_forward: batch %d outside [1, %d]", B, 1 << 20);
  if (H < DISC_MIN_HW || W < DISC_MIN_HW || H > DISC_MAX_HW || W > DISC_MAX_HW || H % DISC_HW_STEP || W % DISC_HW_STEP)
    return fail(-1, "mb_disc_forward: images of %d x %d: H and W must be multiples of %d in [%d, %d]", H, W, DISC_HW_STEP, DISC_MIN_HW, DISC_MAX_HW);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("disc", s);
  const int chunk = (int)std::min<size_t>((size_t)h->max_chunk, std::max<size_t>(1, h->cap_pix / ((size_t)H * W)));
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int n = std::min(chunk, B - b0);
    run_disc(h, images + (size_t)b0 * 3 * H * W, n, H, W, clamp01, logits ? logits + (size_t)b0 * DISC_NLOGIT : nullptr,
             stats ? stats + (size_t)b0 * DISC_NSTAT : sum ? h->stats : nullptr, sum, s);
  }
  return launched();
}

// synchronises the stream
int mb_disc_saturation_count(mb_disc* h, unsigned* count, int reset, mb_stream stream) {
  if (!h || !count) return fail(-1, "mb_disc_saturation_count: null argument");
  return read_counter("mb_disc_saturation_count", h->cn.sat, count, reset, (hipStream_t)stream);
}

}  // extern "C"
