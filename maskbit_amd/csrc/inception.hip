// The FID Inception-v3 network (pytorch-fid's pt_inception-2015-12-05, the network behind the reference's metrics.inception.get_inception_model())
// on gfx950: uint8 images -> the 2048 pooled features and the 1008 logits.  The graph is written out in DESIGN.md "Inception-v3"; IcNet::build below
// is its one statement in this library.
//
// convbn_kernel<MJ, NI>: ONE general implicit-GEMM convolution for all 94 BasicConv2d layers (1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1; stride 1 or 2;
// any zero padding; any H, W; channel-slice input and output).  GEMM view: M = the B * Ho * Wo output pixels as ONE flat index (a tile may
// straddle images), N = Cout, K = taps x Cin walked tap-major in 32-channel steps of v_mfma_f32_16x16x32_f16.  A wave owns MJ x 16 pixels by
// NI x 16 output channels and nothing is shared between waves: no LDS, no barrier.  Both operands go straight from memory into the MFMA fragment
// layout -- lane (l15, g) holds k = 8 g .. 8 g + 7 of weight row l15 (A) and of pixel l15 (B), 16 bytes each -- which NHWC activations and
// [tap][cout][cin] weights give as whole 16-byte loads; the next step's fragments are requested before the current step's MFMAs (two register
// sets).  The weights (<= 3 MiB a layer) and the 64-byte pixel rows that the 4 waves of a workgroup share (they differ in the channel tile
// first) come from L1 / L2.  What this leaves on the table against an LDS-staged tile is stated in profiles/inception.md.
//   Masking: for a pixel's tap outside the image, a pixel index >= M and an input-channel slot >= Cin the lane reads the first slot of the slice
// instead (a valid address) and the value is REPLACED by zeros before the MFMA; for Cin % 8 != 0 (the 3-channel image) the elements of the last slot beyond Cin are zeroed one by one.
// Nothing outside the (tap, channel) range ever reaches a multiply, so a neighbouring slice may hold anything.  The packed weights are
// zero-filled to whole 64 x 32 tiles.
//   Every output element is a chain of MFMAs over the same K order whatever the tile shape, the pixel's place in its tile or the batch: a
// pixel's bits do not depend on the variant, on B or on the other images.
//   Epilogue: v = fma(acc, scale[c], shift[c]) in fp32 (BatchNorm in evaluation mode, eps 1e-3; the scale stays out of the fp16 weights because
// the checkpoint's variances span decades), ReLU, fp16 store saturating at 65504 and counted.  Two more epilogues serve ResNet-50's bottlenecks
// (resnet.hip): linear (no ReLU; saturation on |v|) and residual (relu(v + identity), the identity an fp16 channel slice, the add in fp32).
// A fourth serves the VQGAN+ discriminator (discriminator.hip): LeakyReLU with the slope as an argument (scale = 1, shift = the bias).
// The epilogue is a template parameter: the ReLU form's instructions are what they were.
//
// Two instantiations: <4, 4> (64 pixels x 64 channels a wave: 16 MFMAs per 8 fragment loads) from 512 such tiles up, else <2, 2> (the 8 x 8 maps,
// and everything at small batches).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/maskbit_hip.h"
#include "../../include/maskbit_hip_diag.h"
#include "mb_abi.h"
#include "mb_convnet.h"
#include "mb_incep.h"

namespace mb {

namespace {

constexpr int IC_THREADS = 256;
constexpr int IC_FEAT = 2048, IC_NCLASS = 1008;

struct ConvBnArgs {
  ConvBn q;
  int Ho, Wo, M, cin_pad, cout_pad, nch, T, ntn, ntiles, tail;
};

// EPI: the epilogue (mb_incep.h CONVBN_RELU / CONVBN_LINEAR / CONVBN_RESIDUAL); the K walk is the same for all three
template <int MJ, int NI, int EPI>
__global__ __launch_bounds__(IC_THREADS) void convbn_kernel(ConvBnArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x * (IC_THREADS / 64) + wave;
  if (tile >= a.ntiles) return;             // whole waves; there is no barrier in this kernel
  const ConvBn& q = a.q;
  const int tn = tile % a.ntn, tm = tile / a.ntn;
  const int n0 = tn * NI * 16, p0 = tm * MJ * 16;
  const int HoWo = a.Ho * a.Wo;

  // per pixel: the input coordinates of tap (0, 0) and the element offset of that tap's channel slot g -- which may lie outside the image, or
  // the tensor: it is only used for taps that are inside.  A pixel index >= M gets a row no tap brings into the image.
  int iy0[MJ], ix0[MJ];
  long long xb[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    const int p = p0 + j * 16 + l15;
    const int pc = min(p, a.M - 1);
    const int b = pc / HoWo, r = pc - b * HoWo, oy = r / a.Wo, ox = r - oy * a.Wo;
    iy0[j] = p < a.M ? oy * q.stride - q.ph : -(1 << 20);
    ix0[j] = ox * q.stride - q.pw;
    xb[j] = (((long long)b * q.H + iy0[j]) * q.W + ix0[j]) * q.in_cs + q.in_off + g * 8;
  }
  const h16* wrow = q.w + (size_t)(n0 + l15) * a.cin_pad + g * 8;
  const size_t wtap = (size_t)a.cout_pad * a.cin_pad;

  // the position of the next step to load: input-channel chunk inside tap (ky, kx)
  int ch = 0, ky = 0, kx = 0, tap = 0;
  auto load = [&](h16x8 (&wf)[NI], h16x8 (&xf)[MJ]) {
    const int c = ch * IC_CK + g * 8;
    const h16* wp = wrow + tap * wtap + ch * IC_CK;
#pragma unroll
    for (int i = 0; i < NI; ++i) wf[i] = *(const h16x8*)(wp + (size_t)i * 16 * a.cin_pad);
    const bool cok = c < q.cin;
    const long long soff = (long long)(ky * q.W + kx) * q.in_cs + ch * IC_CK;       // wave-uniform: the tap and the chunk
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const bool ok = cok && (unsigned)(iy0[j] + ky) < (unsigned)q.H && (unsigned)(ix0[j] + kx) < (unsigned)q.W;
      h16x8 v = *(const h16x8*)(ok ? q.in + (xb[j] + soff) : q.in + q.in_off);        // masked: the slice's first slot is read instead
      if (a.tail) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (c + e < q.cin) ? v[e] : (h16)0;
      }
      xf[j] = ok ? v : h16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    if (++ch == a.nch) { ch = 0; ++tap; if (++kx == q.kw) { kx = 0; ++ky; } }
  };

  f32x4 acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mma = [&](const h16x8 (&wf)[NI], const h16x8 (&xf)[MJ]) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = MB_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
  };

  h16x8 wf0[NI], xf0[MJ], wf1[NI], xf1[MJ];
  load(wf0, xf0);
  for (int t = 0; t < a.T; t += 2) {
    if (t + 1 < a.T) load(wf1, xf1);
    mma(wf0, xf0);
    if (t + 1 < a.T) {
      if (t + 2 < a.T) load(wf0, xf0);
      mma(wf1, xf1);
    }
  }

  // lane holds out[pixel p0 + j * 16 + l15][channel n0 + i * 16 + g * 4 .. + 3]
  unsigned nsat = 0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int nl = n0 + i * 16 + g * 4;
    if (nl < q.cout) {
      const float4 sc = *(const float4*)(q.scale + nl), sh = *(const float4*)(q.shift + nl);
#pragma unroll
      for (int j = 0; j < MJ; ++j) {
        const int p = p0 + j * 16 + l15;
        if (p < a.M) {
          float v[4];
          if constexpr (EPI == CONVBN_RELU) {
            v[0] = fmaxf(fmaf(acc[i][j][0], sc.x, sh.x), 0.f); v[1] = fmaxf(fmaf(acc[i][j][1], sc.y, sh.y), 0.f);
            v[2] = fmaxf(fmaf(acc[i][j][2], sc.z, sh.z), 0.f); v[3] = fmaxf(fmaf(acc[i][j][3], sc.w, sh.w), 0.f);
            nsat += fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])) > MB_H16_MAX ? 1u : 0u;
          } else if constexpr (EPI == CONVBN_LINEAR) {             // the downsample branch: no ReLU, saturation on |v|
            v[0] = fmaf(acc[i][j][0], sc.x, sh.x); v[1] = fmaf(acc[i][j][1], sc.y, sh.y);
            v[2] = fmaf(acc[i][j][2], sc.z, sh.z); v[3] = fmaf(acc[i][j][3], sc.w, sh.w);
            nsat += fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) > MB_H16_MAX ? 1u : 0u;
          } else if constexpr (EPI == CONVBN_LEAKY) {              // the discriminator's LeakyReLU: v or v * slope, saturation on |v|
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float t = fmaf(acc[i][j][e], e == 0 ? sc.x : e == 1 ? sc.y : e == 2 ? sc.z : sc.w, e == 0 ? sh.x : e == 1 ? sh.y : e == 2 ? sh.z : sh.w);
              v[e] = t >= 0.f ? t : __fmul_rn(t, q.slope);
            }
            nsat += fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) > MB_H16_MAX ? 1u : 0u;
          } else {                                             // the end of a bottleneck: + identity in fp32, ReLU, one rounding
            const h16x4 id = *(const h16x4*)(q.idn + (size_t)p * q.idn_cs + q.idn_off + nl);
            v[0] = fmaxf(__fadd_rn(fmaf(acc[i][j][0], sc.x, sh.x), (float)id[0]), 0.f);
            v[1] = fmaxf(__fadd_rn(fmaf(acc[i][j][1], sc.y, sh.y), (float)id[1]), 0.f);
            v[2] = fmaxf(__fadd_rn(fmaf(acc[i][j][2], sc.z, sh.z), (float)id[2]), 0.f);
            v[3] = fmaxf(__fadd_rn(fmaf(acc[i][j][3], sc.w, sh.w), (float)id[3]), 0.f);
            nsat += fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])) > MB_H16_MAX ? 1u : 0u;
          }
          *(h16x4*)(q.out + (size_t)p * q.out_cs + q.out_off + nl) = h16x4{to_h(v[0]), to_h(v[1]), to_h(v[2]), to_h(v[3])};
        }
      }
    }
  }
  if (nsat) atomicAdd(q.sat, nsat);
}

__global__ void repack_convbn_kernel(const float* __restrict__ w, h16* __restrict__ out, int cout, int cin, int ntap, int cout_pad, int cin_pad) {
  const size_t total = (size_t)ntap * cout_pad * cin_pad;
  for (size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(o % cin_pad), co = (int)((o / cin_pad) % cout_pad), tap = (int)(o / ((size_t)cin_pad * cout_pad));
    out[o] = (co < cout && ci < cin) ? (h16)w[((size_t)co * cin + ci) * ntap + tap] : (h16)0;
  }
}

__global__ void bn_fold_kernel(const float* __restrict__ bn, float* __restrict__ scale, float* __restrict__ shift, int cout, float eps) {
  // five fp32 operations, each rounded to nearest: plain operators under the pragma.  The __f*_rn functions are plain operators inside the HIP
  // headers, out of the pragma's reach: the shift's product and difference written with them contract to one fma; and __fsqrt_rn is the bare
  // v_sqrt_f32 approximation (1 ulp), where sqrtf is the correctly rounded root
#pragma clang fp contract(off)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cout) return;
  const float a = bn[3 * cout + c] + eps;
  const float s = bn[c] / sqrtf(a);
  const float t = bn[2 * cout + c] * s;
  scale[c] = s;
  shift[c] = bn[cout + c] - t;
}

// one thread per (output pixel, 8-channel slot)
template <int MODE>
__global__ __launch_bounds__(IC_THREADS) void pool3_kernel(Pool3 q, int Ho, int Wo) {
  constexpr int ST = (MODE == 0 || MODE == 3) ? 2 : 1, PAD = MODE == 0 ? 0 : 1;
  const int ns = q.C / 8;
  const size_t total = (size_t)q.B * Ho * Wo * ns;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int slot = (int)(i % ns);
    const size_t p = i / ns;
    const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
    const size_t b = p / ((size_t)Wo * Ho);
    float m[8];
    int n = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = MODE == 2 ? 0.f : -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int y = oy * ST - PAD + dy, x = ox * ST - PAD + dx;
        if (y >= 0 && y < q.H && x >= 0 && x < q.W) {
          const h16x8 v = *(const h16x8*)(q.in + ((b * q.H + y) * q.W + x) * q.in_cs + q.in_off + slot * 8);
          ++n;
#pragma unroll
          for (int e = 0; e < 8; ++e) m[e] = MODE == 2 ? __fadd_rn(m[e], (float)v[e]) : fmaxf(m[e], (float)v[e]);
        }
      }
    h16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = MODE == 2 ? to_h(__fdiv_rn(m[e], (float)n)) : (h16)m[e];
    *(h16x8*)(q.out + p * q.out_cs + q.out_off + slot * 8) = o;
  }
}

// one thread per output pixel; out [B, 299, 299, 8]
__global__ __launch_bounds__(IC_THREADS) void inception_input_kernel(const uint8_t* __restrict__ u8, h16* __restrict__ out, int B, int H, int W) {
  const size_t total = (size_t)B * IC_SIDE * IC_SIDE;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % IC_SIDE), y = (int)((i / IC_SIDE) % IC_SIDE);
    const size_t b = i / ((size_t)IC_SIDE * IC_SIDE);
    const int sy = y * H, sx = x * W;
    const int y0 = sy / IC_SIDE, x0 = sx / IC_SIDE, y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float ty = __fdiv_rn((float)(sy - y0 * IC_SIDE), (float)IC_SIDE), tx = __fdiv_rn((float)(sx - x0 * IC_SIDE), (float)IC_SIDE);
    h16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint8_t* img = u8 + (b * 3 + c) * (size_t)H * W;
      const float a00 = img[(size_t)y0 * W + x0], a01 = img[(size_t)y0 * W + x1], a10 = img[(size_t)y1 * W + x0], a11 = img[(size_t)y1 * W + x1];
      const float top = __fadd_rn(a00, __fmul_rn(__fsub_rn(a01, a00), tx)), bot = __fadd_rn(a10, __fmul_rn(__fsub_rn(a11, a10), tx));
      const float v = __fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), ty));
      o[c] = to_h(__fmul_rn(__fsub_rn(v, 128.0f), 0.0078125f));
    }
    *(h16x8*)(out + i * IC_INC) = o;
  }
}

// grid (C / 8, B): thread t sums pixels t, t + 256, .. in fp32, then a fixed tree over the threads
__global__ __launch_bounds__(IC_THREADS) void spatial_mean_kernel(const h16* __restrict__ x, float* __restrict__ mean, int HW, int C) {
  __shared__ float red[IC_THREADS][8];
  const int tid = threadIdx.x, slot = blockIdx.x;
  const size_t b = blockIdx.y;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = tid; p < HW; p += IC_THREADS) {
    const h16x8 v = *(const h16x8*)(x + (b * HW + p) * C + slot * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += (float)v[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tid][e] = s[e];
  __syncthreads();
  for (int o = IC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[tid][e] += red[tid + o][e];
    }
    __syncthreads();
  }
  if (tid < 8) mean[b * C + slot * 8 + tid] = __fdiv_rn(red[0][tid], (float)HW);
}

// one wave per (output n, 8 images): its weight row in registers, the images one after the other
__global__ __launch_bounds__(IC_THREADS) void fc_head_kernel(const float* __restrict__ pool, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ unbiased, float* __restrict__ biased, int B, int D, int N) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * (IC_THREADS / 64) + (threadIdx.x >> 6);
  if (n >= N) return;
  const int nk = D / 256;                  // 16-byte pieces per lane
  float4 wr[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) wr[k] = k < nk ? *(const float4*)(w + (size_t)n * D + (k * 64 + lane) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float bn = bias ? bias[n] : 0.f;
  for (int b = blockIdx.y * 8; b < min(B, (int)blockIdx.y * 8 + 8); ++b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < nk) {
        const float4 p = *(const float4*)(pool + (size_t)b * D + (k * 64 + lane) * 4);
        s = fmaf(p.x, wr[k].x, s); s = fmaf(p.y, wr[k].y, s); s = fmaf(p.z, wr[k].z, s); s = fmaf(p.w, wr[k].w, s);
      }
    s = wave_sum(s);
    if (lane == 0) {
      if (unbiased) unbiased[(size_t)b * N + n] = s;
      if (biased) biased[(size_t)b * N + n] = s + bn;
    }
  }
}

// out fp32 [B][HW][C] = channels [off, off + C) of x fp16 [B, HW, cs]: a tap of the first channels of a map, flattened in (h, w, c) order
__global__ __launch_bounds__(IC_THREADS) void channel_tap_kernel(const h16* __restrict__ x, float* __restrict__ out, size_t n, int C, int off, int cs) {
  for (size_t i = (size_t)blockIdx.x * IC_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * IC_THREADS)
    out[i] = (float)x[(i / C) * cs + off + i % C];
}

unsigned grid_for(size_t n) { return (unsigned)std::min<size_t>(16384, std::max<size_t>(1, (n + IC_THREADS - 1) / IC_THREADS)); }

}  // namespace

const char* convbn_refusal(const ConvBn& q) {
  if (!q.in || !q.scale || !q.shift || !q.out) return "null argument";          // (w and sat are the launcher's caller's own)
  if (q.B < 1 || q.H < 1 || q.W < 1 || q.cin < 1 || q.cout < 1) return "empty shape";
  if (q.kh < 1 || q.kh > 7 || q.kw < 1 || q.kw > 7) return "kernel sizes must be 1 .. 7";
  if (q.stride != 1 && q.stride != 2) return "stride must be 1 or 2";
  if (q.ph < 0 || q.ph >= q.kh || q.pw < 0 || q.pw >= q.kw) return "padding must be smaller than the kernel";
  if (q.H + 2 * q.ph < q.kh || q.W + 2 * q.pw < q.kw) return "the image is smaller than the kernel";
  if (q.in_off < 0 || q.in_off % 8 || q.in_cs % 8 || q.in_off + (q.cin + 7) / 8 * 8 > q.in_cs)
    return "input slice: offset and stride must be multiples of 8 channels and hold Cin rounded up to 8";
  if (q.epi < CONVBN_RELU || q.epi > CONVBN_LEAKY) return "epilogue must be 0 (ReLU), 1 (linear), 2 (residual + ReLU) or 3 (LeakyReLU)";
  if (q.epi == CONVBN_LEAKY && !(q.slope >= 0.f && q.slope <= 1.f)) return "LeakyReLU: the slope must be in [0, 1]";
  if (q.epi == CONVBN_RESIDUAL && (!q.idn || q.idn_off < 0 || q.idn_off % 4 || q.idn_cs % 4 || q.idn_off + q.cout > q.idn_cs))
    return "identity slice: a pointer, and offset and stride multiples of 4 channels that hold Cout";
  if (q.cout % 4 || q.out_off < 0 || q.out_off % 4 || q.out_cs % 4 || q.out_off + q.cout > q.out_cs)
    return "output slice: Cout, offset and stride must be multiples of 4 channels";
  const size_t M = (size_t)q.B * ic_out_size(q.H, q.kh, q.stride, q.ph) * ic_out_size(q.W, q.kw, q.stride, q.pw);
  if (M >= (1u << 30) || (size_t)q.B * q.H * q.W >= (1u << 30)) return "more than 2^30 pixels in one launch";
  if (M * ic_cout_pad(q.cout) >= ((size_t)1 << 40)) return "more than 2^30 wave tiles in one launch";
  return nullptr;
}

void launch_convbn(hipStream_t s, const ConvBn& q, int variant) {
  ConvBnArgs a;
  a.q = q;
  a.Ho = ic_out_size(q.H, q.kh, q.stride, q.ph); a.Wo = ic_out_size(q.W, q.kw, q.stride, q.pw);
  a.M = q.B * a.Ho * a.Wo;
  a.cin_pad = ic_cin_pad(q.cin); a.cout_pad = ic_cout_pad(q.cout);
  a.nch = a.cin_pad / IC_CK; a.T = q.kh * q.kw * a.nch;
  a.tail = q.cin % 8 ? 1 : 0;
  const int big_tiles = ((a.M + 63) / 64) * (a.cout_pad / 64);
  // measured at 64 images (profiles/inception.md): the 17 x 17 maps (578 - 867 big tiles) run 21 % faster on the big tile, the 8 x 8 maps
  // (192 - 448) 15 % faster on the small one
  if (variant == 0) variant = big_tiles >= 512 ? 1 : 2;
  if (variant == 1) {
    a.ntn = a.cout_pad / 64; a.ntiles = big_tiles;
    const dim3 grid((a.ntiles + 3) / 4), block(IC_THREADS);
    if (q.epi == CONVBN_RELU) hipLaunchKernelGGL((convbn_kernel<4, 4, CONVBN_RELU>), grid, block, 0, s, a);
    else if (q.epi == CONVBN_LINEAR) hipLaunchKernelGGL((convbn_kernel<4, 4, CONVBN_LINEAR>), grid, block, 0, s, a);
    else if (q.epi == CONVBN_LEAKY) hipLaunchKernelGGL((convbn_kernel<4, 4, CONVBN_LEAKY>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((convbn_kernel<4, 4, CONVBN_RESIDUAL>), grid, block, 0, s, a);
  } else {
    a.ntn = a.cout_pad / 32; a.ntiles = ((a.M + 31) / 32) * a.ntn;
    const dim3 grid((a.ntiles + 3) / 4), block(IC_THREADS);
    if (q.epi == CONVBN_RELU) hipLaunchKernelGGL((convbn_kernel<2, 2, CONVBN_RELU>), grid, block, 0, s, a);
    else if (q.epi == CONVBN_LINEAR) hipLaunchKernelGGL((convbn_kernel<2, 2, CONVBN_LINEAR>), grid, block, 0, s, a);
    else if (q.epi == CONVBN_LEAKY) hipLaunchKernelGGL((convbn_kernel<2, 2, CONVBN_LEAKY>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((convbn_kernel<2, 2, CONVBN_RESIDUAL>), grid, block, 0, s, a);
  }
}

void launch_repack_convbn(hipStream_t s, const float* w_oihw, h16* out, int cout, int cin, int kh, int kw) {
  const int cop = ic_cout_pad(cout), cip = ic_cin_pad(cin);
  hipLaunchKernelGGL(repack_convbn_kernel, dim3(grid_for((size_t)kh * kw * cop * cip)), dim3(IC_THREADS), 0, s, w_oihw, out, cout, cin, kh * kw, cop, cip);
}

void launch_bn_fold(hipStream_t s, const float* bn, float* scale, float* shift, int cout, float eps) {
  hipLaunchKernelGGL(bn_fold_kernel, dim3((cout + IC_THREADS - 1) / IC_THREADS), dim3(IC_THREADS), 0, s, bn, scale, shift, cout, eps);
}

const char* pool3_refusal(const Pool3& q) {
  if (!q.in || !q.out) return "null argument";
  if (q.mode < 0 || q.mode > 3)
    return "mode must be 0 (max, stride 2), 1 (max, stride 1, padding 1), 2 (average, stride 1, padding 1) or 3 (max, stride 2, padding 1)";
  if (q.B < 1 || q.C < 8 || q.C % 8 || q.H < 1 || q.W < 1 || (q.mode == 0 && (q.H < 3 || q.W < 3))) return "empty shape, or C not a multiple of 8";
  if (q.in_off < 0 || q.in_off % 8 || q.in_cs % 8 || q.in_off + q.C > q.in_cs || q.out_off < 0 || q.out_off % 8 || q.out_cs % 8 || q.out_off + q.C > q.out_cs)
    return "slices: offsets and strides must be multiples of 8 channels and hold C";
  return nullptr;
}

void launch_pool3(hipStream_t s, const Pool3& q) {
  const int Ho = ic_pool_size(q.H, q.mode), Wo = ic_pool_size(q.W, q.mode);
  const dim3 grid(grid_for((size_t)q.B * Ho * Wo * (q.C / 8))), block(IC_THREADS);
  if (q.mode == 0) hipLaunchKernelGGL(pool3_kernel<0>, grid, block, 0, s, q, Ho, Wo);
  else if (q.mode == 1) hipLaunchKernelGGL(pool3_kernel<1>, grid, block, 0, s, q, Ho, Wo);
  else if (q.mode == 2) hipLaunchKernelGGL(pool3_kernel<2>, grid, block, 0, s, q, Ho, Wo);
  else hipLaunchKernelGGL(pool3_kernel<3>, grid, block, 0, s, q, Ho, Wo);
}

void launch_inception_input(hipStream_t s, const uint8_t* u8, h16* out, int B, int H, int W) {
  hipLaunchKernelGGL(inception_input_kernel, dim3(grid_for((size_t)B * IC_SIDE * IC_SIDE)), dim3(IC_THREADS), 0, s, u8, out, B, H, W);
}

void launch_spatial_mean(hipStream_t s, const h16* x, float* mean, int B, int HW, int C) {
  for (int b0 = 0; b0 < B; b0 += 65535) {
    const int nb = std::min(65535, B - b0);
    hipLaunchKernelGGL(spatial_mean_kernel, dim3(C / 8, nb), dim3(IC_THREADS), 0, s, x + (size_t)b0 * HW * C, mean + (size_t)b0 * C, HW, C);
  }
}

void launch_channel_tap(hipStream_t s, const h16* x, float* out, int B, int HW, int C, int off, int cs) {
  const size_t n = (size_t)B * HW * C;
  hipLaunchKernelGGL(channel_tap_kernel, dim3(grid_for(n)), dim3(IC_THREADS), 0, s, x, out, n, C, off, cs);
}

void launch_fc_head(hipStream_t s, const float* pool, const float* w, const float* bias, float* unbiased, float* biased, int B, int D, int N) {
  hipLaunchKernelGGL(fc_head_kernel, dim3((N + 3) / 4, (B + 7) / 8), dim3(IC_THREADS), 0, s, pool, w, bias, unbiased, biased, B, D, N);
}

// ---- the network ------------------------------------------------------------------------------------------------------------------------
namespace {

struct IcView { int buf, off, cs, H, W, C; };                  // channels [off, off + C) of buffer `buf`, [B, H, W, cs]
enum { IC_OP_CONV, IC_OP_POOL, IC_OP_MEAN, IC_OP_MAP, IC_OP_SPATIAL };
struct IcOp { int kind, idx; IcView in, out; std::string scope; };   // idx: the convolution, the pool mode, the fp32 tap (0 .. 2) or the fp16 map (0 .. 3)
constexpr int IC_NBUF = 5;                                     // 0 / 1: a block's input and output in turn; 2 / 3: a branch's intermediates; 4: the pooled input

struct IcNet {
  ConvNet* cn = nullptr;                                       // where conv() puts its records: the handle's
  std::vector<IcOp> ops;
  size_t need[IC_NBUF] = {0, 0, 0, 0, 0};                      // fp16 elements per image
  IcView last{0, 0, 0, 0, 0, 0};
  std::string group = "stem";                                  // of the layers being added: the name of their timing scope

  IcView claim(IcView v) { need[v.buf] = std::max(need[v.buf], (size_t)v.H * v.W * v.cs); return v; }
  IcView conv(const std::string& name, IcView in, int cout, int kh, int kw, int stride, int ph, int pw, int obuf, int ooff = 0, int ocs = 0) {
    const int idx = add_conv(*cn, name + ".conv.weight", name + ".bn", in.C, cout, kh, kw, stride, ph, pw);   // the checkpoint's naming
    const IcView out = claim({obuf, ooff, ocs ? ocs : cout, ic_out_size(in.H, kh, stride, ph), ic_out_size(in.W, kw, stride, pw), cout});
    ops.push_back({IC_OP_CONV, idx, in, out, "inception_conv." + group});
    return out;
  }
  IcView c1(const std::string& name, IcView in, int cout, int obuf, int ooff = 0, int ocs = 0) { return conv(name, in, cout, 1, 1, 1, 0, 0, obuf, ooff, ocs); }
  IcView pool(IcView in, int mode, int obuf, int ooff = 0, int ocs = 0) {
    const int Ho = mode == 0 ? (in.H - 3) / 2 + 1 : in.H, Wo = mode == 0 ? (in.W - 3) / 2 + 1 : in.W;
    const IcView out = claim({obuf, ooff, ocs ? ocs : in.C, Ho, Wo, in.C});
    ops.push_back({IC_OP_POOL, mode, in, out, "inception_pool." + group});
    return out;
  }
  void mean(IcView in, int tap) { ops.push_back({IC_OP_MEAN, tap, in, in, "inception_mean"}); }
  void map(IcView in, int id) { ops.push_back({IC_OP_MAP, id, in, in, ""}); }
  void spatial(IcView in, int channels) { in.C = channels; ops.push_back({IC_OP_SPATIAL, 0, in, in, "inception_spatial"}); }
  static IcView whole(IcView part, int cs) { return {part.buf, 0, cs, part.H, part.W, cs}; }

  IcView block_a(const std::string& n, IcView x, int pf, int y) {
    const int cs = 224 + pf;
    const IcView r = c1(n + ".branch1x1", x, 64, y, 0, cs);
    conv(n + ".branch5x5_2", c1(n + ".branch5x5_1", x, 48, 2), 64, 5, 5, 1, 2, 2, y, 64, cs);
    const IcView d = conv(n + ".branch3x3dbl_2", c1(n + ".branch3x3dbl_1", x, 64, 2), 96, 3, 3, 1, 1, 1, 3);
    conv(n + ".branch3x3dbl_3", d, 96, 3, 3, 1, 1, 1, y, 128, cs);
    c1(n + ".branch_pool", pool(x, 2, 4), pf, y, 224, cs);
    return whole(r, cs);
  }
  IcView block_b(const std::string& n, IcView x, int y) {
    const int cs = 768;
    const IcView r = conv(n + ".branch3x3", x, 384, 3, 3, 2, 0, 0, y, 0, cs);
    const IcView d = conv(n + ".branch3x3dbl_2", c1(n + ".branch3x3dbl_1", x, 64, 2), 96, 3, 3, 1, 1, 1, 3);
    conv(n + ".branch3x3dbl_3", d, 96, 3, 3, 2, 0, 0, y, 384, cs);
    pool(x, 0, y, 480, cs);
    return whole(r, cs);
  }
  IcView block_c(const std::string& n, IcView x, int c7, int y) {
    const int cs = 768;
    const IcView r = c1(n + ".branch1x1", x, 192, y, 0, cs);
    IcView t = c1(n + ".branch7x7_1", x, c7, 2);
    t = conv(n + ".branch7x7_2", t, c7, 1, 7, 1, 0, 3, 3);
    conv(n + ".branch7x7_3", t, 192, 7, 1, 1, 3, 0, y, 192, cs);
    t = c1(n + ".branch7x7dbl_1", x, c7, 2);
    t = conv(n + ".branch7x7dbl_2", t, c7, 7, 1, 1, 3, 0, 3);
    t = conv(n + ".branch7x7dbl_3", t, c7, 1, 7, 1, 0, 3, 2);
    t = conv(n + ".branch7x7dbl_4", t, c7, 7, 1, 1, 3, 0, 3);
    conv(n + ".branch7x7dbl_5", t, 192, 1, 7, 1, 0, 3, y, 384, cs);
    c1(n + ".branch_pool", pool(x, 2, 4), 192, y, 576, cs);
    return whole(r, cs);
  }
  IcView block_d(const std::string& n, IcView x, int y) {
    const int cs = 1280;
    const IcView r = conv(n + ".branch3x3_2", c1(n + ".branch3x3_1", x, 192, 2), 320, 3, 3, 2, 0, 0, y, 0, cs);
    IcView t = c1(n + ".branch7x7x3_1", x, 192, 2);
    t = conv(n + ".branch7x7x3_2", t, 192, 1, 7, 1, 0, 3, 3);
    t = conv(n + ".branch7x7x3_3", t, 192, 7, 1, 1, 3, 0, 2);
    conv(n + ".branch7x7x3_4", t, 192, 3, 3, 2, 0, 0, y, 320, cs);
    pool(x, 0, y, 512, cs);
    return whole(r, cs);
  }
  IcView block_e(const std::string& n, IcView x, int pool_mode, int y) {
    const int cs = 2048;
    const IcView r = c1(n + ".branch1x1", x, 320, y, 0, cs);
    IcView t = c1(n + ".branch3x3_1", x, 384, 2);
    conv(n + ".branch3x3_2a", t, 384, 1, 3, 1, 0, 1, y, 320, cs);
    conv(n + ".branch3x3_2b", t, 384, 3, 1, 1, 1, 0, y, 704, cs);
    t = conv(n + ".branch3x3dbl_2", c1(n + ".branch3x3dbl_1", x, 448, 2), 384, 3, 3, 1, 1, 1, 3);
    conv(n + ".branch3x3dbl_3a", t, 384, 1, 3, 1, 0, 1, y, 1088, cs);
    conv(n + ".branch3x3dbl_3b", t, 384, 3, 1, 1, 1, 0, y, 1472, cs);
    c1(n + ".branch_pool", pool(x, pool_mode, 4), 192, y, 1856, cs);
    return whole(r, cs);
  }

  void build(ConvNet& net) {
    cn = &net;
    IcView x = claim({0, 0, IC_INC, IC_SIDE, IC_SIDE, 3});
    x = conv("Conv2d_1a_3x3", x, 32, 3, 3, 2, 0, 0, 1);
    x = conv("Conv2d_2a_3x3", x, 32, 3, 3, 1, 0, 0, 0);
    x = conv("Conv2d_2b_3x3", x, 64, 3, 3, 1, 1, 1, 1);
    x = pool(x, 0, 0);
    mean(x, 0);
    x = c1("Conv2d_3b_1x1", x, 80, 1);
    x = conv("Conv2d_4a_3x3", x, 192, 3, 3, 1, 0, 0, 0);
    x = pool(x, 0, 1);
    mean(x, 1); map(x, 0);
    group = "Mixed_5";
    x = block_a("Mixed_5b", x, 32, 0);
    x = block_a("Mixed_5c", x, 64, 1);
    x = block_a("Mixed_5d", x, 64, 0);
    map(x, 1);
    group = "Mixed_6";
    x = block_b("Mixed_6a", x, 1);
    x = block_c("Mixed_6b", x, 128, 0);
    x = block_c("Mixed_6c", x, 160, 1);
    x = block_c("Mixed_6d", x, 160, 0);
    spatial(x, IC_SPATIAL_C);                 // the first channels of Mixed_6d.branch1x1, which the block wrote at channel 0 of its output
    x = block_c("Mixed_6e", x, 192, 1);
    mean(x, 2); map(x, 2);
    group = "Mixed_7";
    x = block_d("Mixed_7a", x, 0);
    x = block_e("Mixed_7b", x, 2, 1);          // average pool
    x = block_e("Mixed_7c", x, 1, 0);          // MAX pool: the FID variant of the last block
    map(x, 3);
    last = x;
  }
};

}  // namespace

}  // namespace mb

struct mb_inception {
  int max_images = 0;
  mb::ConvNet cn;                  // the convolutions, the head, the checkpoint table, the arena (mb_convnet.h)
  mb::IcNet net;
  h16* buf[mb::IC_NBUF] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  float* pool = nullptr;
};

using namespace mb;

namespace {

struct IcOut { void* map[4]; float* tap[3]; float *pool, *unbiased, *biased; float* spatial = nullptr; };

int check_inception(const char* what, mb_inception* h, const uint8_t* u8, int B, int H, int W) {
  if (!h || !u8) return fail(-1, "%s: null argument", what);
  if (int rc = complete(what, h->cn)) return rc;
  if (B < 1 || B > h->max_images) return fail(-1, "%s: batch %d outside [1, %d] images", what, B, h->max_images);
  if (H < 2 || W < 2 || H > 16384 || W > 16384) return fail(-1, "%s: images of %d x %d: H and W must be in [2, 16384]", what, H, W);
  return 0;
}

h16* at(mb_inception* h, const IcView& v) { return h->buf[v.buf]; }

void run_inception(mb_inception* h, const uint8_t* u8, int B, int H, int W, const IcOut& o, hipStream_t s) {
  { ProfScope p("inception_input", s); launch_inception_input(s, u8, h->buf[0], B, H, W); }
  for (const IcOp& op : h->net.ops) {
    if (op.kind == IC_OP_CONV) {
      const CnConv& c = h->cn.convs[op.idx];
      ProfScope p(op.scope.c_str(), s);
      launch_convbn(s, ConvBn{at(h, op.in), c.w, c.scale, c.shift, at(h, op.out), h->cn.sat, B, op.in.H, op.in.W, c.cin, c.cout, c.kh, c.kw, c.stride, c.ph, c.pw,
                              op.in.off, op.in.cs, op.out.off, op.out.cs});
    } else if (op.kind == IC_OP_POOL) {
      ProfScope p(op.scope.c_str(), s);
      launch_pool3(s, Pool3{at(h, op.in), at(h, op.out), B, op.in.H, op.in.W, op.in.C, op.idx, op.in.off, op.in.cs, op.out.off, op.out.cs});
    } else if (op.kind == IC_OP_MEAN) {
      ProfScope p(op.scope.c_str(), s);
      if (o.tap[op.idx]) launch_spatial_mean(s, at(h, op.in), o.tap[op.idx], B, op.in.H * op.in.W, op.in.C);
    } else if (op.kind == IC_OP_SPATIAL) {
      if (o.spatial) {
        ProfScope p(op.scope.c_str(), s);
        launch_channel_tap(s, at(h, op.in), o.spatial, B, op.in.H * op.in.W, op.in.C, op.in.off, op.in.cs);
      }
    } else if (o.map[op.idx]) {
      (void)hipMemcpyAsync(o.map[op.idx], at(h, op.in), (size_t)B * op.in.H * op.in.W * op.in.C * sizeof(h16), hipMemcpyDeviceToDevice, s);
    }
  }
  const IcView& f = h->net.last;
  { ProfScope p("inception_head", s);
    launch_spatial_mean(s, at(h, f), h->pool, B, f.H * f.W, f.C);
    if (o.pool) (void)hipMemcpyAsync(o.pool, h->pool, (size_t)B * IC_FEAT * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (o.unbiased || o.biased) launch_fc_head(s, h->pool, h->cn.fc_w, h->cn.fc_b, o.unbiased, o.biased, B, IC_FEAT, IC_NCLASS); }
}

}  // namespace

extern "C" {

int mb_inception_create(int max_images, mb_inception** out) {
  if (!out || max_images < 1 || max_images > 4096) return fail(-1, "mb_inception_create: bad arguments");
  mb_inception* h = new mb_inception();
  h->max_images = max_images;
  h->cn.bn_eps = IC_BN_EPS;
  h->net.build(h->cn);
  add_head(h->cn, "", IC_FEAT, IC_NCLASS);
  DevArena& m = h->cn.mem;
  m.get(&h->pool, (size_t)max_images * IC_FEAT);
  for (int i = 0; i < IC_NBUF; ++i) m.get(&h->buf[i], (size_t)max_images * h->net.need[i]);
  if (int rc = m.failed("mb_inception_create")) { delete h; return rc; }
  *out = h;
  return 0;
}

void mb_inception_destroy(mb_inception* h) { delete h; }

int mb_inception_load(mb_inception* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!h || !name || !data || !shape || ndim < 0) return fail(-1, "mb_inception_load: bad arguments");
  return load_entry("mb_inception_load", h->cn, name, name, data, shape, ndim, (hipStream_t)stream);
}

int mb_inception_forward(mb_inception* h, const uint8_t* u8, int B, int H, int W, float* pool, float* logits_unbiased, float* logits, mb_stream stream) {
  if (int rc = check_inception("mb_inception_forward", h, u8, B, H, W)) return rc;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("inception", s);
  run_inception(h, u8, B, H, W, IcOut{{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, pool, logits_unbiased, logits}, s);
  return launched();
}

int mb_inception_forward_spatial(mb_inception* h, const uint8_t* u8, int B, int H, int W, float* spatial, float* pool, float* logits_unbiased,
                                 float* logits, mb_stream stream) {
  if (int rc = check_inception("mb_inception_forward_spatial", h, u8, B, H, W)) return rc;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("inception", s);
  IcOut o{{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, pool, logits_unbiased, logits};
  o.spatial = spatial;
  run_inception(h, u8, B, H, W, o, s);
  return launched();
}

// synchronises the stream
int mb_inception_saturation_count(mb_inception* h, unsigned* count, int reset, mb_stream stream) {
  if (!h || !count) return fail(-1, "mb_inception_saturation_count: null argument");
  return read_counter("mb_inception_saturation_count", h->cn.sat, count, reset, (hipStream_t)stream);
}

// ---- diagnostic entries (include/maskbit_hip_diag.h) ----
int mb_convbn_layer_leaky(const void* in_h16, const float* w_oihw, const float* scale, const float* shift, void* out_h16, unsigned* saturated, int B,
                          int H, int W, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw, int in_off, int in_cs, int out_off, int out_cs,
                          int variant, int epilogue, float slope, const void* identity_h16, int idn_off, int idn_cs, mb_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!w_oihw || variant < 0 || variant > 2) return fail(-1, "mb_convbn_layer: bad arguments");
  ConvBn q{(const h16*)in_h16, nullptr, scale, shift, (h16*)out_h16, nullptr, B, H, W, Cin, Cout, kh, kw, stride, ph, pw, in_off, in_cs, out_off, out_cs,
           epilogue, slope, (const h16*)identity_h16, idn_off, idn_cs};
  if (const char* why = convbn_refusal(q)) return fail(-1, "mb_convbn_layer: %s", why);
  DevArena m;
  h16* w = nullptr;
  unsigned* sat = nullptr;
  m.get(&w, (size_t)kh * kw * ic_cout_pad(Cout) * ic_cin_pad(Cin)); m.zeroed(&sat, 1);
  if (int rc = m.failed("mb_convbn_layer")) return rc;
  launch_repack_convbn(s, w_oihw, w, Cout, Cin, kh, kw);
  q.w = w; q.sat = sat;
  launch_convbn(s, q, variant);
  const int rc = launched();
  unsigned nsat = 0;
  const bool ok = hipMemcpyAsync(&nsat, sat, sizeof(unsigned), hipMemcpyDeviceToHost, s) == hipSuccess;
  if (hipStreamSynchronize(s) != hipSuccess || !ok) return fail(-10, "mb_convbn_layer: copy failed");
  if (saturated) *saturated = nsat;
  return rc;
}

// the three epilogues of the feature networks; the LeakyReLU one (3) is mb_convbn_layer_leaky's
int mb_convbn_layer_ex(const void* in_h16, const float* w_oihw, const float* scale, const float* shift, void* out_h16, unsigned* saturated, int B, int H,
                       int W, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw, int in_off, int in_cs, int out_off, int out_cs, int variant,
                       int epilogue, const void* identity_h16, int idn_off, int idn_cs, mb_stream stream) {
  if (epilogue < CONVBN_RELU || epilogue > CONVBN_RESIDUAL) return fail(-1, "mb_convbn_layer: epilogue must be 0 (ReLU), 1 (linear) or 2 (residual + ReLU)");
  return mb_convbn_layer_leaky(in_h16, w_oihw, scale, shift, out_h16, saturated, B, H, W, Cin, Cout, kh, kw, stride, ph, pw, in_off, in_cs, out_off, out_cs,
                               variant, epilogue, 0.f, identity_h16, idn_off, idn_cs, stream);
}

int mb_convbn_layer(const void* in_h16, const float* w_oihw, const float* scale, const float* shift, void* out_h16, unsigned* saturated, int B, int H,
                    int W, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw, int in_off, int in_cs, int out_off, int out_cs, int variant,
                    mb_stream stream) {
  return mb_convbn_layer_ex(in_h16, w_oihw, scale, shift, out_h16, saturated, B, H, W, Cin, Cout, kh, kw, stride, ph, pw, in_off, in_cs, out_off, out_cs,
                            variant, CONVBN_RELU, nullptr, 0, 0, stream);
}

int mb_pool3_ex(const void* x_h16, void* y_h16, int B, int H, int W, int C, int mode, int in_off, int in_cs, int out_off, int out_cs, mb_stream stream) {
  const Pool3 q{(const h16*)x_h16, (h16*)y_h16, B, H, W, C, mode, in_off, in_cs, out_off, out_cs};
  if (const char* why = pool3_refusal(q)) return fail(-1, "mb_pool3: %s", why);
  launch_pool3((hipStream_t)stream, q);
  return launched();
}

// the three pools of Inception-v3; mode 3 (ResNet's) is mb_pool3_ex's
int mb_pool3(const void* x_h16, void* y_h16, int B, int H, int W, int C, int mode, int in_off, int in_cs, int out_off, int out_cs, mb_stream stream) {
  if (mode == 3) return fail(-1, "mb_pool3: mode must be 0, 1 or 2 (mode 3 is taken by mb_pool3_ex)");
  return mb_pool3_ex(x_h16, y_h16, B, H, W, C, mode, in_off, in_cs, out_off, out_cs, stream);
}

int mb_inception_input(const uint8_t* u8, void* out_h16, int B, int H, int W, mb_stream stream) {
  if (!u8 || !out_h16 || B < 1 || H < 2 || W < 2 || H > 16384 || W > 16384) return fail(-1, "mb_inception_input: bad arguments");
  launch_inception_input((hipStream_t)stream, u8, (h16*)out_h16, B, H, W);
  return launched();
}

int mb_inception_taps(mb_inception* h, const uint8_t* u8, int B, int H, int W, void* map0, void* map1, void* map2, void* map3, float* tap64,
                      float* tap192, float* tap768, float* pool, float* logits_unbiased, float* logits, mb_stream stream) {
  if (int rc = check_inception("mb_inception_taps", h, u8, B, H, W)) return rc;
  run_inception(h, u8, B, H, W, IcOut{{map0, map1, map2, map3}, {tap64, tap192, tap768}, pool, logits_unbiased, logits}, (hipStream_t)stream);
  return launched();
}

// the tail kernels both networks share, each through its launcher (tests/test_hip_convnet_tail.py)
int mb_bn_fold(const float* bn, float* scale, float* shift, int cout, float eps, mb_stream stream) {
  if (!bn || !scale || !shift) return fail(-1, "mb_bn_fold: null argument");
  if (cout < 1 || !(eps >= 0.f)) return fail(-1, "mb_bn_fold: cout %d, eps %g: cout >= 1 and eps >= 0", cout, (double)eps);
  launch_bn_fold((hipStream_t)stream, bn, scale, shift, cout, eps);
  return launched();
}

int mb_spatial_mean(const void* x_h16, float* mean_f32, int B, int HW, int C, mb_stream stream) {
  if (!x_h16 || !mean_f32) return fail(-1, "mb_spatial_mean: null argument");
  if (B < 1 || HW < 1 || C < 8 || C % 8) return fail(-1, "mb_spatial_mean: [%d, %d, %d]: B >= 1, HW >= 1, C a multiple of 8", B, HW, C);
  launch_spatial_mean((hipStream_t)stream, (const h16*)x_h16, mean_f32, B, HW, C);
  return launched();
}

int mb_fc_head(const float* pool, const float* w, const float* bias, float* unbiased, float* biased, int B, int D, int N, mb_stream stream) {
  if (!pool || !w) return fail(-1, "mb_fc_head: null argument");
  if (!unbiased && !biased) return fail(-1, "mb_fc_head: no output: unbiased and biased are both null");
  // a lane holds D / 256 pieces of 4 values, 8 at the most: another D would lose its tail without a word
  if (D < 256 || D % 256 || D > 2048) return fail(-1, "mb_fc_head: D %d: a multiple of 256 up to 2048", D);
  if (B < 1 || B > 8 * 65535 || N < 1) return fail(-1, "mb_fc_head: B %d, N %d: 1 <= B <= %d, N >= 1", B, N, 8 * 65535);
  launch_fc_head((hipStream_t)stream, pool, w, bias, unbiased, biased, B, D, N);
  return launched();
}

int mb_channel_tap(const void* x_h16, float* out_f32, int B, int HW, int C, int off, int cs, mb_stream stream) {
  if (!x_h16 || !out_f32) return fail(-1, "mb_channel_tap: null argument");
  if (B < 1 || HW < 1 || C < 1) return fail(-1, "mb_channel_tap: empty shape [%d, %d, %d]", B, HW, C);
  if (off < 0 || cs < 1 || (long long)off + C > cs) return fail(-1, "mb_channel_tap: channels [%d, %d + %d) are not inside a pixel of %d", off, off, C, cs);
  launch_channel_tap((hipStream_t)stream, (const h16*)x_h16, out_f32, B, HW, C, off, cs);
  return launched();
}

int mb_inception_folded_bn(mb_inception* h, const char* bn_prefix, float* scale_out, float* shift_out, int cout, mb_stream stream) {
  if (!h || !bn_prefix || !scale_out || !shift_out) return fail(-1, "mb_inception_folded_bn: null argument");
  return folded_bn("mb_inception_folded_bn", h->cn, bn_prefix, std::string(bn_prefix) + CN_BN_NAMES[0], scale_out, shift_out, cout, (hipStream_t)stream);
}

}  // extern "C"
