// LPIPS (modeling/modules/lpips.py: the VGG16 `features` stack, five taps, learned 1x1 weights) on gfx950.
//
// lpips_input_kernel: real and fake fp32 NCHW -> ONE fp16 NHWC batch of 2B images (real first, then fake: every layer's weights are staged once
// for both), already as the input of conv1_1 written as a 1x1 convolution: per pixel the 27 values of the 3 x 3 x 3 patch of the scaled image
// ((2x - 1) - shift_c) / scale_c (ScalingLayer, lpips.py:55-63), channel ci * 9 + ky * 3 + kx -- the order of the OIHW weight read as [64, 27] --,
// taps outside the image 0 (zero padding AFTER the scaling, as conv2d pads), padded to the 64-channel chunk of conv_kernel.  The padded 3x3 on 3 of
// 64 channels would spend 21 x the arithmetic.
//
// The thirteen convolutions are conv.hip's conv_kernel with its bias + ReLU epilogue (mb_conv.h launch_conv_relu), the four pools its
// maxpool2_kernel; activations are fp16 NHWC.  Tiles are per image, so an image's features do not depend on the batch it sits in.
//
// lpips_distance_kernel<C> (HBM-bound, one read of both feature maps of a tap): a pixel's C channels are held by C / 8 lanes, 16 bytes each.  With
// na = |a| + 1e-10, nb = |b| + 1e-10 (eps added to the norm, lpips.py:124-126) the tap's value at the pixel is sum_c w_c d_c^2,
// d_c = a_c / na - b_c / nb.  The squared form is never expanded.  d_c itself still cancels for near-identical maps -- the case the metric exists
// for -- when both quotients are rounded first: each carries 2^-24 of a value that may be 1 000 x the difference.  So where the two norms are
// within a factor 2 the SAME expression is evaluated as
//     d_c = ((a_c - b_c) + b_c q) / na,   q = (|b| - |a|) / nb = t / ((|a| + |b|) nb),   t = sum_c (b_c - a_c)(b_c + a_c),
// in which every rounding is relative to a term of the size of the difference (a_c - b_c of fp16 values is exact in fp32 up to 13 binades apart);
// identical pixels give exactly 0, all-zero pixels give 0 through the eps.  Elsewhere (norms a factor 2 apart: d is of the size of the quotients)
// the two quotients are subtracted as written.  The three sums |a|^2, |b|^2, t are butterflies over the pixel's lanes in fp32.
// Sums over pixels are fp64: per lane, then per workgroup in a fixed order into a slot of its own (no floating-point atomics).  The grid depends
// on (HW, C) alone.  lpips_finalize_kernel sums an image's slots in a fixed order, divides by HW and adds the tap to per_image[b]; after the last
// tap it adds per_image to the caller's running sum in image order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/maskbit_hip.h"
#include "../../include/maskbit_hip_diag.h"
#include "mb_abi.h"
#include "mb_conv.h"

namespace mb {

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_MAXBLK = 256;           // distance workgroups per image at most
constexpr int LP_NCONV = 13, LP_NTAP = 5;
// torchvision's VGG16-D `features` indices of the convolutions, their slice in the reference's vgg16 (lpips.py:94-103), output channels, and whether
// a 2x2 max-pool precedes them (features 4, 9, 16, 23)
constexpr int LP_FEAT[LP_NCONV] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};
constexpr int LP_SLICE[LP_NCONV] = {1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5};
constexpr int LP_COUT[LP_NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_TAPC[LP_NTAP] = {64, 128, 256, 512, 512};

// out [2B, H, W, 64]: one thread per (pixel, 8-channel slot); sc = {shift[3], scale[3]}
__global__ __launch_bounds__(LP_THREADS) void lpips_input_kernel(const float* __restrict__ real, const float* __restrict__ fake, const float* __restrict__ sc,
                                                                 h16* __restrict__ out, int B, int H, int W, int clamp01) {
  const size_t HW = (size_t)H * W, total = (size_t)2 * B * HW * 8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int slot = (int)(i & 7); const size_t p = i >> 3;
    const size_t n = p / HW, yx = p - n * HW;
    const int y = (int)(yx / W), x = (int)(yx - (size_t)y * W);
    const float* __restrict__ img = n < (size_t)B ? real + n * 3 * HW : fake + (n - B) * 3 * HW;
    h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (slot < 4) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int k = slot * 8 + e;
        if (k < 27) {
          const int ci = k / 9, t = k - ci * 9, ky = t / 3, kx = t - ky * 3;
          const int Y = y + ky - 1, X = x + kx - 1;
          if (Y >= 0 && Y < H && X >= 0 && X < W) {
            float f = img[(size_t)ci * HW + (size_t)Y * W + X];
            if (clamp01) f = fminf(fmaxf(f, 0.0f), 1.0f);
            f = __fsub_rn(__fmul_rn(f, 2.0f), 1.0f);                      // lpips.py:62
            v[e] = to_h(__fdiv_rn(__fsub_rn(f, sc[ci]), sc[3 + ci]));    // lpips.py:63
          }
        }
      }
    }
    *(h16x8*)(out + p * 64 + slot * 8) = v;
  }
}

// grid (nblk, B); fa / fb [B][HW][C] fp16, w [C]; part [B][nblk] = sum over the workgroup's pixels of sum_c w_c d_c^2
template <int C>
__global__ __launch_bounds__(LP_THREADS) void lpips_distance_kernel(const h16* __restrict__ fa, const h16* __restrict__ fb, const float* __restrict__ w, int HW,
                                                                    double* __restrict__ part) {
  constexpr int LPP = C / 8, PPI = LP_THREADS / LPP;     // lanes per pixel (8 .. 64: whole lane groups of a wave), pixels per workgroup step
  __shared__ double red[LP_THREADS / 64];
  const int tid = threadIdx.x, sl = tid % LPP, pl = tid / LPP;
  const size_t base = (size_t)blockIdx.y * HW;
  float wv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) wv[e] = w[sl * 8 + e];
  double acc = 0.0;
  const int nstep = (HW + PPI - 1) / PPI;                // every lane of a wave takes every step (the butterflies need them all): p is clamped, the value masked
  for (int st = blockIdx.x; st < nstep; st += gridDim.x) {
    const int p = st * PPI + pl;
    const bool live = p < HW;
    const size_t off = (base + (size_t)min(p, HW - 1)) * C + sl * 8;
    const h16x8 av = *(const h16x8*)(fa + off), bv = *(const h16x8*)(fb + off);
    float a[8], b[8], sa = 0.f, sb = 0.f, t = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a[e] = (float)av[e]; b[e] = (float)bv[e];
      sa = fmaf(a[e], a[e], sa); sb = fmaf(b[e], b[e], sb);
      t = fmaf(b[e] - a[e], b[e] + a[e], t);
    }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1) { sa += __shfl_xor(sa, o); sb += __shfl_xor(sb, o); t += __shfl_xor(t, o); }
    const float ra = sqrtf(sa), rb = sqrtf(sb);
    const float na = ra + 1e-10f, nb = rb + 1e-10f;
    const bool close = na <= 2.0f * nb && nb <= 2.0f * na;
    const float q = (ra + rb) > 0.f ? t / ((ra + rb) * nb) : 0.f;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = close ? ((a[e] - b[e]) + b[e] * q) / na : a[e] / na - b[e] / nb;
      s = fmaf(wv[e] * d, d, s);
    }
    if (live) acc += (double)s;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double v = red[0];
    for (int k = 1; k < LP_THREADS / 64; ++k) v += red[k];
    part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = v;
  }
}

// one workgroup; per_image[b] = (first ? 0 : per_image[b]) + (sum of part[b][0 .. P)) / HW; last: *sum += per_image[0 .. B) in image order
__global__ __launch_bounds__(LP_THREADS) void lpips_finalize_kernel(const double* __restrict__ part, int B, int P, double hw, int first, int last,
                                                                    double* __restrict__ per_image, double* __restrict__ sum) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += LP_THREADS / 64) {
    double a = 0.0;
    for (int p = lane; p < P; p += 64) a += part[(size_t)b * P + p];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
    if (lane == 0) per_image[b] = (first ? 0.0 : per_image[b]) + a / hw;
  }
  __syncthreads();
  if (threadIdx.x != 0 || !last || !sum) return;
  double t = *sum;
  for (int b = 0; b < B; ++b) t += per_image[b];
  *sum = t;
}

int distance_blocks(int HW, int C) {
  const int ppi = LP_THREADS / (C / 8);
  return std::min(LP_MAXBLK, (HW + ppi - 1) / ppi);
}

// the tap's distance into part, then the finalize
void launch_distance(hipStream_t s, const h16* fa, const h16* fb, const float* w, int B, int HW, int C, double* part, int first, int last,
                     double* per_image, double* sum) {
  const int nblk = distance_blocks(HW, C);
  const dim3 grid(nblk, B), block(LP_THREADS);
  if (C == 64) hipLaunchKernelGGL(lpips_distance_kernel<64>, grid, block, 0, s, fa, fb, w, HW, part);
  else if (C == 128) hipLaunchKernelGGL(lpips_distance_kernel<128>, grid, block, 0, s, fa, fb, w, HW, part);
  else if (C == 256) hipLaunchKernelGGL(lpips_distance_kernel<256>, grid, block, 0, s, fa, fb, w, HW, part);
  else hipLaunchKernelGGL(lpips_distance_kernel<512>, grid, block, 0, s, fa, fb, w, HW, part);
  hipLaunchKernelGGL(lpips_finalize_kernel, dim3(1), dim3(LP_THREADS), 0, s, part, B, nblk, (double)HW, first, last, per_image, sum);
}

void launch_input(hipStream_t s, const float* real, const float* fake, const float* sc, h16* out, int B, int H, int W, int clamp01) {
  const size_t n = (size_t)2 * B * H * W * 8;
  hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)std::min<size_t>(8192, (n + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, s, real, fake, sc, out,
                     B, H, W, clamp01 ? 1 : 0);
}

struct LpConv { int cin = 0, cout = 0, cin_pad = 0, cout_pad = 0, ks = 3; h16* w = nullptr; float* b = nullptr; };

}  // namespace

}  // namespace mb

struct mb_lpips {
  int max_pairs = 0, max_h = 0, max_w = 0;
  mb::LpConv conv[mb::LP_NCONV];
  float* lin[mb::LP_NTAP] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  float* sc = nullptr;             // shift[3], scale[3]
  h16* buf[2] = {nullptr, nullptr};
  double* part = nullptr;          // [max_pairs][LP_MAXBLK]
  unsigned* sat = nullptr;
  uint64_t loaded = 0;             // one bit per checkpoint entry: 13 weights, 13 biases, 5 lin vectors, shift, scale
  mb::DevArena mem;
};

using namespace mb;

namespace {

constexpr uint64_t LP_ALL = (1ull << 33) - 1;

const char* size_rule = "H must be a multiple of 128 and W a multiple of 256 (whole 8 x 16-pixel tiles at 1/16 resolution)";

// the checks of forward / features, before any device work
int check_forward(const char* what, mb_lpips* h, const float* real, const float* fake, int B, int H, int W) {
  if (!h || !real || !fake) return fail(-1, "%s: null argument", what);
  if (h->loaded != LP_ALL) return fail(-1, "%s: the checkpoint is not complete (33 entries: scaling_layer.*, net.slice*, lin*)", what);
  if (B < 1 || B > h->max_pairs) return fail(-1, "%s: batch %d outside [1, %d] pairs", what, B, h->max_pairs);
  if (H < 128 || W < 256 || H % 128 || W % 256) return fail(-1, "%s: images of %d x %d: %s", what, H, W, size_rule);
  if ((size_t)H * W > (size_t)h->max_h * h->max_w) return fail(-1, "%s: images of %d x %d exceed the handle's %d x %d", what, H, W, h->max_h, h->max_w);
  return 0;
}

// LPIPS.forward (lpips.py:39-52).  taps (or null): five device buffers that receive the tap features of the 2B images, fp16 NHWC
void run_forward(mb_lpips* h, const float* real, const float* fake, int B, int H, int W, int clamp01, double* per_image, double* sum, void* const* taps,
                 hipStream_t s) {
  const int N = 2 * B;
  { ProfScope p("lpips_input", s); launch_input(s, real, fake, h->sc, h->buf[0], B, H, W, clamp01); }
  int xi = 0, hh = H, ww = W, tap = 0;
  for (int l = 0; l < LP_NCONV; ++l) {
    const LpConv& c = h->conv[l];
    if (l > 0 && LP_SLICE[l] != LP_SLICE[l - 1]) {          // features 4, 9, 16, 23
      { ProfScope p("lpips_pool", s); launch_maxpool2(s, h->buf[xi], h->buf[xi ^ 1], N, hh, ww, c.cin); }
      hh /= 2; ww /= 2; xi ^= 1;
    }
    { ProfScope p("lpips_conv", s); launch_conv_relu(s, ConvRelu{h->buf[xi], c.w, c.b, h->buf[xi ^ 1], h->sat, N, hh, ww, c.cin_pad, c.cout, c.cout_pad, c.ks}); }
    xi ^= 1;
    if (l + 1 == LP_NCONV || LP_SLICE[l + 1] != LP_SLICE[l]) {
      const size_t half = (size_t)B * hh * ww * c.cout;
      if (taps) (void)hipMemcpyAsync(taps[tap], h->buf[xi], 2 * half * sizeof(h16), hipMemcpyDeviceToDevice, s);
      if (per_image) {
        ProfScope p("lpips_distance", s);
        launch_distance(s, h->buf[xi], h->buf[xi] + half, h->lin[tap], B, hh * ww, c.cout, h->part, tap == 0, tap == LP_NTAP - 1, per_image, sum);
      }
      ++tap;
    }
  }
}

}  // namespace

extern "C" {

int mb_lpips_create(int max_pairs, int max_h, int max_w, mb_lpips** out) {
  if (!out || max_pairs < 1 || max_pairs > 32768) return fail(-1, "mb_lpips_create: bad arguments");
  if (max_h < 128 || max_w < 256 || max_h % 128 || max_w % 256) return fail(-1, "mb_lpips_create: capacity %d x %d: %s", max_h, max_w, size_rule);
  mb_lpips* h = new mb_lpips();
  h->max_pairs = max_pairs; h->max_h = max_h; h->max_w = max_w;
  DevArena& m = h->mem;
  m.zeroed(&h->sat, 1); m.get(&h->sc, 6); m.get(&h->part, (size_t)max_pairs * LP_MAXBLK);
  int cin = 3;
  for (int l = 0; l < LP_NCONV; ++l) {
    LpConv& c = h->conv[l];
    c.cin = cin; c.cout = LP_COUT[l];
    c.ks = l == 0 ? 1 : 3;                                 // conv1_1 on the 27-value patches
    c.cin_pad = l == 0 ? 64 : cin; c.cout_pad = (c.cout + 127) / 128 * 128;
    m.get(&c.w, (size_t)c.ks * c.ks * c.cout_pad * c.cin_pad); m.zeroed(&c.b, (size_t)c.cout_pad);
    cin = c.cout;
  }
  for (int k = 0; k < LP_NTAP; ++k) m.get(&h->lin[k], (size_t)LP_TAPC[k]);
  for (int i = 0; i < 2; ++i) m.get(&h->buf[i], (size_t)2 * max_pairs * max_h * max_w * 64);
  if (int rc = m.failed("mb_lpips_create")) { delete h; return rc; }
  *out = h;
  return 0;
}

void mb_lpips_destroy(mb_lpips* h) { delete h; }

int mb_lpips_load(mb_lpips* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!h || !name || !data || !shape || ndim < 0) return fail(-1, "mb_lpips_load: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const std::string n(name);
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
  if (n == "scaling_layer.shift" || n == "scaling_layer.scale") {
    const int which = n == "scaling_layer.scale";
    if (numel != 3) return fail(-4, "mb_lpips_load: %s: expected 3 values", name);
    HIP_TRY(hipMemcpyAsync(h->sc + 3 * which, data, 3 * sizeof(float), hipMemcpyDeviceToDevice, s));
    h->loaded |= 1ull << (31 + which);
    return 0;
  }
  for (int k = 0; k < LP_NTAP; ++k) {                      // lin{k}.model.1.weight (use_dropout) or lin{k}.model.0.weight
    const std::string p = "lin" + std::to_string(k) + ".model.";
    if (n == p + "1.weight" || n == p + "0.weight") {
      if (numel != (size_t)LP_TAPC[k]) return fail(-4, "mb_lpips_load: %s: expected %d values", name, LP_TAPC[k]);
      HIP_TRY(hipMemcpyAsync(h->lin[k], data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
      h->loaded |= 1ull << (26 + k);
      return 0;
    }
  }
  for (int l = 0; l < LP_NCONV; ++l) {
    const std::string p = "net.slice" + std::to_string(LP_SLICE[l]) + "." + std::to_string(LP_FEAT[l]);
    const LpConv& c = h->conv[l];
    if (n == p + ".bias") {
      if (numel != (size_t)c.cout) return fail(-4, "mb_lpips_load: %s: wrong bias size", name);
      HIP_TRY(hipMemcpyAsync(c.b, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
      h->loaded |= 1ull << (13 + l);
      return 0;
    }
    if (n == p + ".weight") {
      if (numel != (size_t)c.cout * c.cin * 9) return fail(-4, "mb_lpips_load: %s: wrong weight size", name);
      // conv1_1 [64, 3, 3, 3] is read as [64, 27, 1, 1]: the same memory, input channel ci * 9 + ky * 3 + kx
      if (l == 0) launch_repack_conv(s, data, c.w, c.cout, 27, 1, c.cout_pad, c.cin_pad);
      else launch_repack_conv(s, data, c.w, c.cout, c.cin, 3, c.cout_pad, c.cin_pad);
      h->loaded |= 1ull << l;
      return launched();
    }
  }
  return fail(-2, "mb_lpips_load: unknown checkpoint entry '%s'", name);
}

int mb_lpips_forward(mb_lpips* h, const float* real, const float* fake, int B, int H, int W, int clamp01, double* per_image, double* sum, mb_stream stream) {
  if (int rc = check_forward("mb_lpips_forward", h, real, fake, B, H, W)) return rc;
  if (!per_image) return fail(-1, "mb_lpips_forward: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("lpips", s);
  run_forward(h, real, fake, B, H, W, clamp01, per_image, sum, nullptr, s);
  return launched();
}

// synchronises the stream
int mb_lpips_saturation_count(mb_lpips* h, unsigned* count, int reset, mb_stream stream) {
  if (!h || !count) return fail(-1, "mb_lpips_saturation_count: null argument");
  return read_counter("mb_lpips_saturation_count", h->sat, count, reset, (hipStream_t)stream);
}

// ---- diagnostic entries (include/maskbit_hip_diag.h) ----
int mb_lpips_input(const float* real, const float* fake, const float* shift_scale, void* out_h16, int B, int H, int W, int clamp01, mb_stream stream) {
  if (!real || !fake || !shift_scale || !out_h16 || B < 1 || H < 1 || W < 1) return fail(-1, "mb_lpips_input: bad arguments");
  launch_input((hipStream_t)stream, real, fake, shift_scale, (h16*)out_h16, B, H, W, clamp01);
  return launched();
}

int mb_lpips_distance(const void* feat_a, const void* feat_b, const float* w, int B, int HW, int C, double* per_image, mb_stream stream) {
  if (!feat_a || !feat_b || !w || !per_image || B < 1 || B > 65535 || HW < 1) return fail(-1, "mb_lpips_distance: bad arguments");
  if (C != 64 && C != 128 && C != 256 && C != 512) return fail(-1, "mb_lpips_distance: C must be 64, 128, 256 or 512");
  hipStream_t s = (hipStream_t)stream;
  DevArena m;
  double* part = nullptr;
  m.get(&part, (size_t)B * LP_MAXBLK);
  if (int rc = m.failed("mb_lpips_distance")) return rc;
  for (int b0 = 0; b0 < B; b0 += LP_THREADS) {              // (the finalize is one workgroup; any B is fine, chunked only to keep it short)
    const int nb = std::min(LP_THREADS, B - b0);
    launch_distance(s, (const h16*)feat_a + (size_t)b0 * HW * C, (const h16*)feat_b + (size_t)b0 * HW * C, w, nb, HW, C, part + (size_t)b0 * LP_MAXBLK, 1, 0,
                    per_image + b0, nullptr);
  }
  const int rc = launched();
  const bool ok = hipStreamSynchronize(s) == hipSuccess;    // the scratch is freed on return
  if (rc) return rc;
  return ok ? 0 : fail(-10, "mb_lpips_distance: synchronise failed");
}

int mb_lpips_features(mb_lpips* h, const float* real, const float* fake, int B, int H, int W, int clamp01, void* tap0, void* tap1, void* tap2, void* tap3,
                      void* tap4, mb_stream stream) {
  if (int rc = check_forward("mb_lpips_features", h, real, fake, B, H, W)) return rc;
  if (!tap0 || !tap1 || !tap2 || !tap3 || !tap4) return fail(-1, "mb_lpips_features: null argument");
  void* const taps[LP_NTAP] = {tap0, tap1, tap2, tap3, tap4};
  run_forward(h, real, fake, B, H, W, clamp01, nullptr, nullptr, taps, (hipStream_t)stream);
  return launched();
}

}  // extern "C"
