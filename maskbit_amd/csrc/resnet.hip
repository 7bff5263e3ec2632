// The ResNet-50 perceptual loss (modeling/modules/perceptual_loss.py PerceptualLoss, "resnet50") on gfx950: two fp32 image batches -> per pair the
// mean squared difference of the 1000 logits (and, in the features form, of the layer4 maps).  The graph is torchvision's resnet50 (v1.5) as written
// out in DESIGN.md "ResNet-50"; RnNet below is its one statement in this library.
//
// Input: resize_tables_kernel computes the per-axis tables of the antialiased bilinear resize to 224 in double (DESIGN.md gives the formula) and
// stores them as fp32; resnet_resize_kernel applies them in fp32 in a fixed order -- per output pixel the rows outer, the columns inner, taps
// ascending, every step one fma -- then (v - mean_c) / std_c with an IEEE division, and writes one fp16 NHWC batch of 2B images, real first.  At
// 224 x 224 the two taps of an axis have the weights 1 and 0: the result is fp16((x - mean) / std) bit for bit.
//
// Stem: conv1 (7x7, stride 2, padding 3, 3 channels) through the general convolution would take 49 taps of a 32-channel MFMA step with 3 live
// channels.  stem_cols_kernel writes the im2col instead -- per 112 x 112 output pixel the 147 patch values in the order of the OIHW weight read as
// [64, 147], padded to 160 -- and conv1 runs as a 1x1 over 5 steps.  (Counts and the alternative: DESIGN.md "ResNet-50: the stem".)
//
// Everything else is inception.hip's: convbn_kernel with its three epilogues (ReLU; linear for `downsample`; residual + ReLU for conv3), the 3x3
// pool in mode 3, the fixed-order spatial mean and the fp32 head.  A pixel's bits do not depend on the batch, so a pair's value does not either.
//
// resnet_distance_kernel: one workgroup per pair, float64 sums of squared differences in a fixed order (thread-strided, then a tree over the
// threads), no atomics; resnet_sum_kernel adds the B values to the caller's running sum in pair order.
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
#include "mb_resnet.h"

namespace mb {

namespace {

constexpr int RN_THREADS = 256;

// one thread per (axis, output index)
__global__ void resize_tables_kernel(float* __restrict__ weights, int* __restrict__ span, int H, int W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * RN_SIDE) return;
  const int axis = i / RN_SIDE, d = i - axis * RN_SIDE, n = axis == 0 ? H : W;
  const double scale = (double)n / (double)RN_SIDE, support = scale > 1.0 ? scale : 1.0, inv = 1.0 / support;
  const double c = scale * ((double)d + 0.5);
  const int lo = max((int)(c - support + 0.5), 0), hi = min((int)(c + support + 0.5), n);
  const int cnt = min(hi - lo, RN_MAXT);
  double w[RN_MAXT], tot = 0.0;
#pragma unroll
  for (int j = 0; j < RN_MAXT; ++j) {
    const double v = 1.0 - fabs(((double)(j + lo) - c + 0.5) * inv);
    w[j] = (j < cnt && v > 0.0) ? v : 0.0;
    tot += w[j];
  }
#pragma unroll
  for (int j = 0; j < RN_MAXT; ++j) weights[(size_t)i * RN_MAXT + j] = (float)(w[j] / tot);
  span[2 * i] = lo; span[2 * i + 1] = cnt;
}

// one thread per output pixel; out [2B, 224, 224, 4]
__global__ __launch_bounds__(RN_THREADS) void resnet_resize_kernel(const float* __restrict__ real, const float* __restrict__ fake, const float* __restrict__ ms,
                                                                   const float* __restrict__ weights, const int* __restrict__ span, h16* __restrict__ out,
                                                                   int B, int H, int W, int clamp01) {
  const size_t HW = (size_t)H * W, total = (size_t)2 * B * RN_SIDE * RN_SIDE;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % RN_SIDE), y = (int)((i / RN_SIDE) % RN_SIDE);
    const size_t n = i / ((size_t)RN_SIDE * RN_SIDE);
    const float* __restrict__ img = n < (size_t)B ? real + n * 3 * HW : fake + (n - B) * 3 * HW;
    const float* wy = weights + (size_t)y * RN_MAXT;
    const float* wx = weights + (size_t)(RN_SIDE + x) * RN_MAXT;
    const int y0 = span[2 * y], ny = span[2 * y + 1], x0 = span[2 * (RN_SIDE + x)], nx = span[2 * (RN_SIDE + x) + 1];
    h16x4 o = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* pl = img + (size_t)c * HW;
      float acc = 0.f;
      for (int a = 0; a < ny; ++a) {
        const float* row = pl + (size_t)(y0 + a) * W + x0;
        float r = 0.f;
        for (int b = 0; b < nx; ++b) {
          float v = row[b];
          if (clamp01) v = fminf(fmaxf(v, 0.0f), 1.0f);
          r = __fmaf_rn(wx[b], v, r);
        }
        acc = __fmaf_rn(wy[a], r, acc);
      }
      o[c] = to_h(__fdiv_rn(__fsub_rn(acc, ms[c]), ms[3 + c]));
    }
    *(h16x4*)(out + i * RN_IMGC) = o;
  }
}

// one thread per (output pixel, 8-channel slot); out [N, So, So, 160]
__global__ __launch_bounds__(RN_THREADS) void stem_cols_kernel(const h16* __restrict__ img, h16* __restrict__ out, int N, int S, int So) {
  constexpr int NS = RN_STEM_C / 8;
  const size_t total = (size_t)N * So * So * NS;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int slot = (int)(i % NS);
    const size_t p = i / NS;
    const int ox = (int)(p % So), oy = (int)((p / So) % So);
    const size_t n = p / ((size_t)So * So);
    h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = slot * 8 + e;
      if (k < RN_STEM_K) {
        const int ci = k / 49, t = k - ci * 49, ky = t / 7, kx = t - ky * 7;
        const int Y = 2 * oy - 3 + ky, X = 2 * ox - 3 + kx;
        if (Y >= 0 && Y < S && X >= 0 && X < S) v[e] = img[((n * S + Y) * S + X) * RN_IMGC + ci];
      }
    }
    *(h16x8*)(out + p * RN_STEM_C + slot * 8) = v;
  }
}

// grid B; a fixed tree over the workgroup's threads
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int o = RN_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(RN_THREADS) void resnet_distance_kernel(const float* __restrict__ logits, const h16* __restrict__ feat, int B, int N, size_t F,
                                                                     double* __restrict__ per_pair) {
  __shared__ double red[RN_THREADS];
  const int tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const float* la = logits + b * N;
  const float* lb = logits + (B + b) * N;
  double s = 0.0;
  for (int i = tid; i < N; i += RN_THREADS) {
    const double d = (double)la[i] - (double)lb[i];
    s += d * d;
  }
  double v = block_sum(s, red) / (double)N;
  if (feat) {
    const h16* fa = feat + b * F;
    const h16* fb = feat + (B + b) * F;
    double t = 0.0;
    for (size_t i = (size_t)tid * 8; i < F; i += (size_t)RN_THREADS * 8) {
      const h16x8 av = *(const h16x8*)(fa + i), bv = *(const h16x8*)(fb + i);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double d = (double)(float)av[e] - (double)(float)bv[e];
        t += d * d;
      }
    }
    v += block_sum(t, red) / (double)F;
  }
  if (tid == 0) per_pair[b] = v;
}

__global__ void resnet_sum_kernel(const double* __restrict__ per_pair, int B, double* __restrict__ sum) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double t = *sum;
  for (int b = 0; b < B; ++b) t += per_pair[b];
  *sum = t;
}

unsigned rn_grid(size_t n) { return (unsigned)std::min<size_t>(16384, std::max<size_t>(1, (n + RN_THREADS - 1) / RN_THREADS)); }

}  // namespace

void launch_resize_tables(hipStream_t s, float* weights, int* span, int H, int W) {
  hipLaunchKernelGGL(resize_tables_kernel, dim3((2 * RN_SIDE + RN_THREADS - 1) / RN_THREADS), dim3(RN_THREADS), 0, s, weights, span, H, W);
}

void launch_resnet_resize(hipStream_t s, const float* real, const float* fake, const float* mean_std, const float* weights, const int* span, h16* out,
                          int B, int H, int W, int clamp01) {
  hipLaunchKernelGGL(resnet_resize_kernel, dim3(rn_grid((size_t)2 * B * RN_SIDE * RN_SIDE)), dim3(RN_THREADS), 0, s, real, fake, mean_std, weights, span, out,
                     B, H, W, clamp01 ? 1 : 0);
}

void launch_stem_cols(hipStream_t s, const h16* img, h16* out, int N, int S) {
  const int So = rn_stem_size(S);
  hipLaunchKernelGGL(stem_cols_kernel, dim3(rn_grid((size_t)N * So * So * (RN_STEM_C / 8))), dim3(RN_THREADS), 0, s, img, out, N, S, So);
}

void launch_resnet_distance(hipStream_t s, const float* logits, const h16* feat, int B, int N, size_t F, double* per_pair, double* sum) {
  hipLaunchKernelGGL(resnet_distance_kernel, dim3(B), dim3(RN_THREADS), 0, s, logits, feat, B, N, F, per_pair);
  if (sum) hipLaunchKernelGGL(resnet_sum_kernel, dim3(1), dim3(1), 0, s, per_pair, B, sum);
}

// ---- the network ------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int RN_LAYERS = 4;
constexpr int RN_BLOCKS[RN_LAYERS] = {3, 4, 6, 3};
const char* const RN_PREFIX = "model.";                           // the reference module holds torchvision's network under this name
enum { RN_A, RN_B, RN_T1, RN_T2, RN_D, RN_COLS, RN_IMG, RN_NBUF };     // A / B: a block's input and output in turn; T1 / T2: its two inner maps; D: downsample

struct RnNet {
  size_t need[RN_NBUF] = {0, 0, 0, 0, 0, 0, 0};                  // fp16 elements per image at 224 x 224

  // cn.convs: conv1, then per block conv1, conv2, conv3 (, downsample.0)
  void build(ConvNet& cn) {
    // the checkpoint's naming, in the reference's layout: model.<conv>.weight with model.<bn>.*
    auto add = [&cn](const std::string& conv, const std::string& bn, int cin, int cout, int k, int stride) {
      return add_conv(cn, RN_PREFIX + conv + ".weight", RN_PREFIX + bn, cin, cout, k, k, stride, k / 2, k / 2);
    };
    CnConv& stem = cn.convs[add("conv1", "bn1", RN_STEM_K, 64, 1, 1)];
    stem.shape[1] = 3; stem.shape[2] = stem.shape[3] = 7;
    int cin = 64;
    for (int L = 0; L < RN_LAYERS; ++L) {
      const int width = 64 << L;
      for (int b = 0; b < RN_BLOCKS[L]; ++b) {
        const std::string p = "layer" + std::to_string(L + 1) + "." + std::to_string(b);
        const int stride = (b == 0 && L > 0) ? 2 : 1;
        add(p + ".conv1", p + ".bn1", cin, width, 1, 1);
        add(p + ".conv2", p + ".bn2", width, width, 3, stride);
        add(p + ".conv3", p + ".bn3", width, 4 * width, 1, 1);
        if (b == 0) add(p + ".downsample.0", p + ".downsample.1", cin, 4 * width, 1, stride);
        cin = 4 * width;
      }
    }
    const size_t s1 = (size_t)rn_stem_size(RN_SIDE), s2 = (size_t)rn_stem_size((int)s1);
    need[RN_IMG] = (size_t)RN_SIDE * RN_SIDE * RN_IMGC;
    need[RN_COLS] = s1 * s1 * RN_STEM_C;
    need[RN_A] = need[RN_B] = need[RN_D] = std::max(s1 * s1 * 64, s2 * s2 * 256);
    need[RN_T1] = need[RN_T2] = s2 * s2 * 128;                   // the widest inner map: layer2.0.conv1 before its stride
  }
};

}  // namespace

}  // namespace mb

struct mb_resnet {
  int max_pairs = 0;
  mb::ConvNet cn;                  // the convolutions, the head, the checkpoint table, the arena (mb_convnet.h)
  mb::RnNet net;
  h16* buf[mb::RN_NBUF] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float *pool = nullptr, *logits = nullptr, *mean_std = nullptr, *rw = nullptr;
  int* rspan = nullptr;
};

using namespace mb;

namespace {

struct RnOut { void* map[RN_LAYERS]; float *pool, *logits; };

// the trunk on buf[RN_IMG] = fp16 [N, S, S, 4]: the layer4 map is left in the returned buffer, logits in h->logits
const h16* run_trunk(mb_resnet* h, const h16* img, int N, int S, const RnOut& o, int* HWout, hipStream_t s) {
  int hw = rn_stem_size(S);
  { ProfScope p("resnet_stem", s);
    launch_stem_cols(s, img, h->buf[RN_COLS], N, S);
    const CnConv& c = h->cn.convs[0];
    launch_convbn(s, ConvBn{h->buf[RN_COLS], c.w, c.scale, c.shift, h->buf[RN_A], h->cn.sat, N, hw, hw, c.cin, c.cout, 1, 1, 1, 0, 0, 0, RN_STEM_C, 0, c.cout}); }
  { ProfScope p("resnet_pool", s);
    launch_pool3(s, Pool3{h->buf[RN_A], h->buf[RN_B], N, hw, hw, 64, 3, 0, 64, 0, 64}); }
  hw = rn_stem_size(hw);
  int xi = RN_B, cin = 64;
  size_t ci = 1;
  for (int L = 0; L < RN_LAYERS; ++L) {
    const int width = 64 << L, cout = 4 * width;
    const std::string scope = "resnet_conv.layer" + std::to_string(L + 1);
    for (int b = 0; b < RN_BLOCKS[L]; ++b) {
      ProfScope p(scope.c_str(), s);
      const CnConv &c1 = h->cn.convs[ci], &c2 = h->cn.convs[ci + 1], &c3 = h->cn.convs[ci + 2];
      const int yi = xi == RN_A ? RN_B : RN_A, ho = ic_out_size(hw, 3, c2.stride, 1);
      const h16* x = h->buf[xi];
      launch_convbn(s, ConvBn{x, c1.w, c1.scale, c1.shift, h->buf[RN_T1], h->cn.sat, N, hw, hw, cin, width, 1, 1, 1, 0, 0, 0, cin, 0, width});
      launch_convbn(s, ConvBn{h->buf[RN_T1], c2.w, c2.scale, c2.shift, h->buf[RN_T2], h->cn.sat, N, hw, hw, width, width, 3, 3, c2.stride, 1, 1, 0, width, 0, width});
      const h16* idn = x;
      if (b == 0) {
        const CnConv& d = h->cn.convs[ci + 3];
        launch_convbn(s, ConvBn{x, d.w, d.scale, d.shift, h->buf[RN_D], h->cn.sat, N, hw, hw, cin, cout, 1, 1, d.stride, 0, 0, 0, cin, 0, cout, CONVBN_LINEAR});
        idn = h->buf[RN_D];
      }
      launch_convbn(s, ConvBn{h->buf[RN_T2], c3.w, c3.scale, c3.shift, h->buf[yi], h->cn.sat, N, ho, ho, width, cout, 1, 1, 1, 0, 0, 0, width, 0, cout,
                              CONVBN_RESIDUAL, 0.f, idn, 0, cout});
      ci += b == 0 ? 4 : 3;
      xi = yi; hw = ho; cin = cout;
    }
    if (o.map[L]) (void)hipMemcpyAsync(o.map[L], h->buf[xi], (size_t)N * hw * hw * cin * sizeof(h16), hipMemcpyDeviceToDevice, s);
  }
  { ProfScope p("resnet_head", s);
    launch_spatial_mean(s, h->buf[xi], h->pool, N, hw * hw, RN_FEAT);
    launch_fc_head(s, h->pool, h->cn.fc_w, h->cn.fc_b, nullptr, h->logits, N, RN_FEAT, RN_NCLASS); }
  if (o.pool) (void)hipMemcpyAsync(o.pool, h->pool, (size_t)N * RN_FEAT * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (o.logits) (void)hipMemcpyAsync(o.logits, h->logits, (size_t)N * RN_NCLASS * sizeof(float), hipMemcpyDeviceToDevice, s);
  *HWout = hw * hw;
  return h->buf[xi];
}

// a checkpoint entry's name as the table has it
std::string table_key(const mb_resnet* h, const std::string& name) { return h->cn.table.count(name) ? name : RN_PREFIX + name; }

}  // namespace

extern "C" {

int mb_resnet_create(int max_pairs, mb_resnet** out) {
  if (!out || max_pairs < 1 || max_pairs > 2048) return fail(-1, "mb_resnet_create: bad arguments");
  mb_resnet* h = new mb_resnet();
  h->max_pairs = max_pairs;
  h->cn.bn_eps = RN_BN_EPS;
  h->net.build(h->cn);
  add_head(h->cn, RN_PREFIX, RN_FEAT, RN_NCLASS);
  DevArena& m = h->cn.mem;
  const size_t N = (size_t)2 * max_pairs;
  m.get(&h->pool, N * RN_FEAT); m.get(&h->logits, N * RN_NCLASS);
  m.get(&h->mean_std, 6); m.get(&h->rw, (size_t)2 * RN_SIDE * RN_MAXT); m.get(&h->rspan, (size_t)4 * RN_SIDE);
  add_vec(h->cn, "mean", h->mean_std, 3);                        // the module's own buffers: outside `model.`
  add_vec(h->cn, "std", h->mean_std + 3, 3);
  for (int i = 0; i < RN_NBUF; ++i) m.get(&h->buf[i], N * h->net.need[i]);
  if (int rc = m.failed("mb_resnet_create")) { delete h; return rc; }
  *out = h;
  return 0;
}

void mb_resnet_destroy(mb_resnet* h) { delete h; }

int mb_resnet_load(mb_resnet* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!h || !name || !data || !shape || ndim < 0) return fail(-1, "mb_resnet_load: bad arguments");
  // the table is in the reference's layout (mean, std, model.<torchvision's key>); torchvision's own has no prefix.  Accepted are the names
  // that stripping one leading `model.` -- after mean / std have been tried -- turns into a torchvision key: `model.mean` is none
  return load_entry("mb_resnet_load", h->cn, name, table_key(h, name), data, shape, ndim, (hipStream_t)stream);
}

int mb_resnet_forward(mb_resnet* h, const float* real, const float* fake, int B, int H, int W, int clamp01, int on_logits, double* per_pair, double* sum,
                      mb_stream stream) {
  if (!h || !real || !fake || !per_pair) return fail(-1, "mb_resnet_forward: null argument");
  if (int rc = complete("mb_resnet_forward", h->cn)) return rc;
  if (B < 1 || B > h->max_pairs) return fail(-1, "mb_resnet_forward: batch %d outside [1, %d] pairs", B, h->max_pairs);
  if (H < RN_MIN_HW || W < RN_MIN_HW || H > RN_MAX_HW || W > RN_MAX_HW)
    return fail(-1, "mb_resnet_forward: images of %d x %d: H and W must be in [%d, %d]", H, W, RN_MIN_HW, RN_MAX_HW);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("resnet", s);
  { ProfScope pi("resnet_input", s);
    launch_resize_tables(s, h->rw, h->rspan, H, W);
    launch_resnet_resize(s, real, fake, h->mean_std, h->rw, h->rspan, h->buf[RN_IMG], B, H, W, clamp01); }
  int HW = 0;
  const h16* feat = run_trunk(h, h->buf[RN_IMG], 2 * B, RN_SIDE, RnOut{{nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr}, &HW, s);
  { ProfScope pd("resnet_distance", s);
    launch_resnet_distance(s, h->logits, on_logits ? nullptr : feat, B, RN_NCLASS, (size_t)HW * RN_FEAT, per_pair, sum); }
  return launched();
}

// synchronises the stream
int mb_resnet_saturation_count(mb_resnet* h, unsigned* count, int reset, mb_stream stream) {
  if (!h || !count) return fail(-1, "mb_resnet_saturation_count: null argument");
  return read_counter("mb_resnet_saturation_count", h->cn.sat, count, reset, (hipStream_t)stream);
}

// ---- diagnostic entries (include/maskbit_hip_diag.h) ----
int mb_resnet_input(const float* real, const float* fake, const float* mean_std, void* image_h16, void* cols_h16, int B, int H, int W, int clamp01,
                    mb_stream stream) {
  if (!real || !fake || !mean_std || !image_h16 || B < 1 || B > 32768 || H < RN_MIN_HW || W < RN_MIN_HW || H > RN_MAX_HW || W > RN_MAX_HW)
    return fail(-1, "mb_resnet_input: bad arguments (H and W in [%d, %d])", RN_MIN_HW, RN_MAX_HW);
  hipStream_t s = (hipStream_t)stream;
  DevArena m;
  float* rw = nullptr;
  int* span = nullptr;
  m.get(&rw, (size_t)2 * RN_SIDE * RN_MAXT); m.get(&span, (size_t)4 * RN_SIDE);
  if (int rc = m.failed("mb_resnet_input")) return rc;
  launch_resize_tables(s, rw, span, H, W);
  launch_resnet_resize(s, real, fake, mean_std, rw, span, (h16*)image_h16, B, H, W, clamp01);
  if (cols_h16) launch_stem_cols(s, (const h16*)image_h16, (h16*)cols_h16, 2 * B, RN_SIDE);
  const int rc = launched();
  const bool ok = hipStreamSynchronize(s) == hipSuccess;    // the tables are freed on return
  if (rc) return rc;
  return ok ? 0 : fail(-10, "mb_resnet_input: synchronise failed");
}

int mb_resnet_stem_cols(const void* image_h16, void* cols_h16, int B, int S, mb_stream stream) {
  if (!image_h16 || !cols_h16 || B < 1 || B > 65536 || S < 7 || S > RN_MAX_HW) return fail(-1, "mb_resnet_stem_cols: bad arguments (7 <= S <= %d)", RN_MAX_HW);
  launch_stem_cols((hipStream_t)stream, (const h16*)image_h16, (h16*)cols_h16, B, S);
  return launched();
}

int mb_resnet_distance(const float* logits, const void* feat_h16, int B, int N, long long F, double* per_pair, double* sum, mb_stream stream) {
  if (!logits || !per_pair || B < 1 || B > 65535 || N < 1 || F < 0 || F % 8 || (feat_h16 && F < 8))
    return fail(-1, "mb_resnet_distance: bad arguments (F a multiple of 8)");
  launch_resnet_distance((hipStream_t)stream, logits, (const h16*)feat_h16, B, N, (size_t)F, per_pair, sum);
  return launched();
}

int mb_resnet_taps(mb_resnet* h, const void* image_h16, int B, int S, void* layer1, void* layer2, void* layer3, void* layer4, float* pool, float* logits,
                   mb_stream stream) {
  if (!h || !image_h16) return fail(-1, "mb_resnet_taps: null argument");
  if (int rc = complete("mb_resnet_taps", h->cn)) return rc;
  if (B < 1 || B > 2 * h->max_pairs) return fail(-1, "mb_resnet_taps: batch %d outside [1, %d] images", B, 2 * h->max_pairs);
  if (S < RN_MIN_HW || S > RN_SIDE || S % 8) return fail(-1, "mb_resnet_taps: side %d: a multiple of 8 in [%d, %d]", S, RN_MIN_HW, RN_SIDE);
  int HW = 0;
  run_trunk(h, (const h16*)image_h16, B, S, RnOut{{layer1, layer2, layer3, layer4}, pool, logits}, &HW, (hipStream_t)stream);
  return launched();
}

int mb_resnet_folded_bn(mb_resnet* h, const char* bn_prefix, float* scale_out, float* shift_out, int cout, mb_stream stream) {
  if (!h || !bn_prefix || !scale_out || !shift_out) return fail(-1, "mb_resnet_folded_bn: null argument");
  return folded_bn("mb_resnet_folded_bn", h->cn, bn_prefix, table_key(h, std::string(bn_prefix) + CN_BN_NAMES[0]), scale_out, shift_out, cout,
                   (hipStream_t)stream);
}

}  // extern "C"
