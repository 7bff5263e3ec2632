// The Taming VQGAN tokenizer handle of libmaskbit_hip.so (mb_taming_*, include/maskbit_hip.h): OriginalVQModel (modeling/taming_vqgan.py:19-69) =
// Encoder / Decoder of modeling/taming/taming_autoencoder.py (:176-267, :270-370) around SimpleVectorizer(1024, 256) with quant_conv / post_quant_conv.
// This file is the layer schedule and the checkpoint ingest; the kernels and their launchers are conv.hip (mb_conv.h), spatial_attention.hip
// (mb_spattn.h) and vq.hip (mb_vq.h).  The network is fixed (taming_vqgan.py:26-37): ch 128, ch_mult (1,1,2,2,4), 2 res blocks per level (the
// decoder runs 3), attention at the 16-pixel level, z_channels 256.
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/maskbit_hip.h"
#include "../../include/maskbit_hip_diag.h"
#include "mb_abi.h"
#include "mb_conv.h"
#include "mb_spattn.h"
#include "mb_vq.h"

namespace mb {
namespace {
constexpr int T_CH = 128, T_LEVELS = 5, T_Z = 256, T_CODES = 1024, T_ATT = 512, T_NATTN = 7;
constexpr int T_MULT[T_LEVELS] = {1, 1, 2, 2, 4};

// ResnetBlock (taming_autoencoder.py:59-118): every conv has a bias; nin_shortcut (1x1, in != out) is applied to the block INPUT
struct TBlock { Norm n1, n2; Conv c1, c2, sc; bool has_sc = false; };
// AttnBlock (:121-173): q, k, v stacked into one 1x1 conv 512 -> 1536 behind the GroupNorm (no SiLU), proj_out with the residual
struct TAttn { Norm n; Conv qkv, proj; int tap = 0; };
struct TLevel { std::vector<TBlock> blocks; std::vector<TAttn> attn; Conv samp; bool has_samp = false; };
// where a checkpoint entry goes: a convolution's weight or bias (rows [row0, row0 + rows) of it: q / k / v inside the stacked conv), or a norm's vector.
// fold: decoder.conv_out carries decode's (y + 1) / 2 (taming_vqgan.py:55): weight x 0.5, bias (b + 1) / 2
struct TParam { Conv* conv = nullptr; bool bias = false; float* vec = nullptr; int n = 0; int row0 = 0, rows = 0; bool fold = false; };
}  // namespace
}  // namespace mb

struct mb_taming {
  int max_batch = 0, latent = 0, res = 0;
  // encoder
  mb::Conv e_conv_in, e_conv_out, quant_conv;
  mb::TLevel e_down[mb::T_LEVELS];
  mb::TBlock e_mid1, e_mid2; mb::TAttn e_mid_attn;
  mb::Norm e_norm_out;
  // decoder: up[i] = level i, 0 the finest (taming_autoencoder.py:330)
  mb::Conv post_quant_conv, d_conv_in, d_conv_out;
  mb::TLevel d_up[mb::T_LEVELS];
  mb::TBlock d_mid1, d_mid2; mb::TAttn d_mid_attn;
  mb::Norm d_norm_out;
  h16* buf[3] = {nullptr, nullptr, nullptr};
  h16* qkv = nullptr;            // [max_batch * latent^2][1536]
  h16* z = nullptr;              // decoder input latent [max_batch * latent^2][256]
  float* fold_w = nullptr;       // scratch: decoder.conv_out.weight x 0.5 before its repack
  bool cb_loaded = false;
  mb::VqCodebook q;
  float* vq_zT = nullptr; float* vq_ps = nullptr; int* vq_pi = nullptr;
  unsigned* sat = nullptr;
  mb::GnCtx gn;
  void* tap[mb::T_NATTN] = {};   // diagnostic (mb_taming_set_tap): where the output of AttnBlock i is copied to, or null
  std::unordered_map<std::string, mb::TParam> params;
  mb::DevArena mem;
};

using namespace mb;

namespace {

__global__ void affine_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n, float mul, float add) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = fmaf(src[i], mul, add * mul);
}
// image fp32 NCHW in [0, 1] -> fp16 NHWC padded to 64 channels, scaled x * 2 - 1 (OriginalVQModel.encode, taming_vqgan.py:46): the scaling cannot
// fold into conv_in, whose zero padding is applied after it
__global__ void pack_image_pm1_kernel(const float* __restrict__ img, h16* __restrict__ out, int B, int C, int H, int W) {
  const size_t npix = (size_t)B * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix * 8; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i >> 3; const int slot = (int)(i & 7);
    const size_t b = p / ((size_t)H * W), yx = p - b * (size_t)H * W;
    h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (slot == 0)
      for (int c = 0; c < C && c < 8; ++c) v[c] = to_h(img[(b * C + c) * (size_t)H * W + yx] * 2.0f - 1.0f);
    *(h16x8*)(out + p * CK + slot * 8) = v;
  }
}

void name_conv(mb_taming* d, Conv& c, const std::string& name, bool fold = false) {
  d->params[name + ".weight"] = TParam{&c, false, nullptr, 0, 0, c.cout_w, fold};
  d->params[name + ".bias"] = TParam{&c, true, nullptr, 0, 0, c.cout_w, fold};
}
void alloc_conv(mb_taming* d, Conv& c) {
  c.sat = d->sat;
  d->mem.get(&c.w, conv_weight_elems(c));
  d->mem.zeroed(&c.b, (size_t)c.cout_pad);
}
void init_conv(mb_taming* d, Conv& c, const std::string& name, int cin, int cout, int ks, bool up = false, bool final_ = false) {
  shape_conv(c, cin, cout, ks, true, up, final_);
  alloc_conv(d, c);
  name_conv(d, c, name, final_);
}
void init_norm(mb_taming* d, Norm& n, const std::string& name, int c) {
  n.c = c;
  d->mem.get(&n.g, (size_t)c);
  d->mem.get(&n.b, (size_t)c);
  d->params[name + ".weight"] = TParam{nullptr, false, n.g, c};
  d->params[name + ".bias"] = TParam{nullptr, false, n.b, c};
}
void init_block(mb_taming* d, TBlock& rb, const std::string& p, int cin, int cout) {
  rb.has_sc = cin != cout;
  init_norm(d, rb.n1, p + ".norm1", cin);
  init_conv(d, rb.c1, p + ".conv1", cin, cout, 3);
  init_norm(d, rb.n2, p + ".norm2", cout);
  init_conv(d, rb.c2, p + ".conv2", cout, cout, 3);
  if (rb.has_sc) init_conv(d, rb.sc, p + ".nin_shortcut", cin, cout, 1);
}
void init_attn(mb_taming* d, TAttn& at, const std::string& p, int tap) {
  at.tap = tap;
  init_norm(d, at.n, p + ".norm", T_ATT);
  shape_conv(at.qkv, T_ATT, 3 * T_ATT, 1, true, false, false);
  alloc_conv(d, at.qkv);
  const char* nm[3] = {".q", ".k", ".v"};
  for (int i = 0; i < 3; ++i) {
    d->params[p + nm[i] + ".weight"] = TParam{&at.qkv, false, nullptr, 0, i * T_ATT, T_ATT};
    d->params[p + nm[i] + ".bias"] = TParam{&at.qkv, true, nullptr, 0, i * T_ATT, T_ATT};
  }
  init_conv(d, at.proj, p + ".proj_out", T_ATT, T_ATT, 1);
}

// x (buffer index xi, B x H x W pixels) -> the buffer index holding the block output
int run_block(hipStream_t s, mb_taming* d, const TBlock& rb, int xi, int B, int H, int W) {
  const int t1 = (xi + 1) % 3, t2 = (xi + 2) % 3;
  launch_gn(s, &d->gn, rb.n1, d->buf[xi], B, H * W);
  launch_conv(s, &d->gn, rb.c1, d->buf[xi], d->gn.ss, nullptr, d->buf[t1], nullptr, nullptr, B, H, W, false);
  launch_gn(s, &d->gn, rb.n2, d->buf[t1], B, H * W);
  if (!rb.has_sc) {
    launch_conv(s, &d->gn, rb.c2, d->buf[t1], d->gn.ss, d->buf[xi], d->buf[t2], nullptr, nullptr, B, H, W, false);
    return t2;
  }
  // out = nin_shortcut(x) + h (taming_autoencoder.py:112-118).  The shortcut runs after norm2's statistics are final (they stay in gn.ss) and
  // leaves none of its own: its output is read as a residual, not by a GroupNorm
  launch_conv(s, &d->gn, rb.sc, d->buf[xi], nullptr, nullptr, d->buf[t2], nullptr, nullptr, B, H, W, false, false);
  launch_conv(s, &d->gn, rb.c2, d->buf[t1], d->gn.ss, d->buf[t2], d->buf[xi], nullptr, nullptr, B, H, W, false);
  return xi;
}
// AttnBlock.forward (taming_autoencoder.py:149-173) on x = buf[xi], the output of the conv that precedes it
int run_attn(hipStream_t s, mb_taming* d, const TAttn& at, int xi, int B, int H, int W) {
  ProfScope p("taming_attn_block", s);
  const int t1 = (xi + 1) % 3, t2 = (xi + 2) % 3, N = H * W;
  launch_gn(s, &d->gn, at.n, d->buf[xi], B, N);
  launch_conv(s, &d->gn, at.qkv, d->buf[xi], d->gn.ss, nullptr, d->qkv, nullptr, nullptr, B, H, W, false, false, false);
  {
    ProfScope pk("spatial_attention", s);
    launch_spatial_attention(s, SpAttn{d->qkv, d->qkv + T_ATT, d->qkv + 2 * T_ATT, d->buf[t1], d->sat, B, N, 3 * T_ATT, T_ATT});
  }
  launch_conv(s, &d->gn, at.proj, d->buf[t1], nullptr, d->buf[xi], d->buf[t2], nullptr, nullptr, B, H, W, false);
  if (d->tap[at.tap]) (void)hipMemcpyAsync(d->tap[at.tap], d->buf[t2], (size_t)B * N * T_ATT * sizeof(h16), hipMemcpyDeviceToDevice, s);
  return t2;
}

// Encoder.forward (taming_autoencoder.py:240-267) + quant_conv (taming_vqgan.py:48) -> index of the buffer holding z [B * latent^2][256]
int encode_to_z(mb_taming* d, const float* img, int B, hipStream_t s) {
  int res = d->res;
  {
    const size_t npix = (size_t)B * res * res;
    hipLaunchKernelGGL(pack_image_pm1_kernel, dim3((unsigned)std::min<size_t>(4096, (npix * 8 + 255) / 256)), dim3(256), 0, s, img, d->buf[2], B, 3, res, res);
  }
  launch_conv(s, &d->gn, d->e_conv_in, d->buf[2], nullptr, nullptr, d->buf[0], nullptr, nullptr, B, res, res, false);
  int xi = 0;
  for (int l = 0; l < T_LEVELS; ++l) {
    TLevel& lv = d->e_down[l];
    for (size_t r = 0; r < lv.blocks.size(); ++r) {
      xi = run_block(s, d, lv.blocks[r], xi, B, res, res);
      if (!lv.attn.empty()) xi = run_attn(s, d, lv.attn[r], xi, B, res, res);
    }
    if (lv.has_samp) {                                     // Downsample (:49-53): zero row / column after, 3x3 stride 2 = the 2x2 conv on space-to-depth
      const int t = (xi + 1) % 3, t2 = (xi + 2) % 3;
      launch_s2d(s, d->buf[xi], d->buf[t], B, res, res, lv.samp.cin);
      res /= 2;
      launch_conv(s, &d->gn, lv.samp, d->buf[t], nullptr, nullptr, d->buf[t2], nullptr, nullptr, B, res, res, false);
      xi = t2;
    }
  }
  xi = run_block(s, d, d->e_mid1, xi, B, res, res);
  xi = run_attn(s, d, d->e_mid_attn, xi, B, res, res);
  xi = run_block(s, d, d->e_mid2, xi, B, res, res);
  launch_gn(s, &d->gn, d->e_norm_out, d->buf[xi], B, res * res);
  const int t = (xi + 1) % 3, t2 = (xi + 2) % 3;
  launch_conv(s, &d->gn, d->e_conv_out, d->buf[xi], d->gn.ss, nullptr, d->buf[t], nullptr, nullptr, B, res, res, false, false);
  launch_conv(s, &d->gn, d->quant_conv, d->buf[t], nullptr, nullptr, d->buf[t2], nullptr, nullptr, B, res, res, false, false);
  return t2;
}

// post_quant_conv + Decoder.forward (taming_vqgan.py:52-56, taming_autoencoder.py:340-370) from the latent in d->z
void decode_from_z(mb_taming* d, float* img_nchw, uint8_t* img_nhwc_u8, int B, hipStream_t s) {
  int res = d->latent;
  launch_conv(s, &d->gn, d->post_quant_conv, d->z, nullptr, nullptr, d->buf[1], nullptr, nullptr, B, res, res, false, false);
  launch_conv(s, &d->gn, d->d_conv_in, d->buf[1], nullptr, nullptr, d->buf[0], nullptr, nullptr, B, res, res, false);
  int xi = 0;
  xi = run_block(s, d, d->d_mid1, xi, B, res, res);
  xi = run_attn(s, d, d->d_mid_attn, xi, B, res, res);
  xi = run_block(s, d, d->d_mid2, xi, B, res, res);
  for (int l = T_LEVELS - 1; l >= 0; --l) {
    TLevel& lv = d->d_up[l];
    for (size_t r = 0; r < lv.blocks.size(); ++r) {
      xi = run_block(s, d, lv.blocks[r], xi, B, res, res);
      if (!lv.attn.empty()) xi = run_attn(s, d, lv.attn[r], xi, B, res, res);
    }
    if (lv.has_samp) {                                     // Upsample (:30-34): nearest 2x fused into the 3x3 conv
      res *= 2;
      const int t = (xi + 1) % 3;
      launch_conv(s, &d->gn, lv.samp, d->buf[xi], nullptr, nullptr, d->buf[t], nullptr, nullptr, B, res, res, false);
      xi = t;
    }
  }
  launch_gn(s, &d->gn, d->d_norm_out, d->buf[xi], B, res * res);
  launch_conv(s, &d->gn, d->d_conv_out, d->buf[xi], d->gn.ss, nullptr, nullptr, img_nchw, img_nhwc_u8, B, res, res, true);
}

}  // namespace

extern "C" {

int mb_taming_create(int max_batch, int latent_size, mb_taming** out) {
  if (!out || max_batch <= 0) return fail(-1, "mb_taming_create: bad arguments");
  if (latent_size != 16 && latent_size != 32) return fail(-1, "mb_taming_create: latent_size must be 16 or 32 (256 x 256 or 512 x 512 images)");
  mb_taming* d = new mb_taming();
  DevArena& m = d->mem;
  d->max_batch = max_batch; d->latent = latent_size; d->res = latent_size << (T_LEVELS - 1);
  m.zeroed(&d->sat, 1);
  const int top = T_CH * T_MULT[T_LEVELS - 1];
  // ---- Encoder.__init__ (taming_autoencoder.py:188-237)
  init_conv(d, d->e_conv_in, "encoder.conv_in", 3, T_CH, 3);
  int cin = T_CH;
  for (int l = 0; l < T_LEVELS; ++l) {
    TLevel& lv = d->e_down[l];
    const int cout = T_CH * T_MULT[l];
    const std::string p = "encoder.down." + std::to_string(l);
    lv.blocks.resize(2);
    if (l == T_LEVELS - 1) lv.attn.resize(2);
    for (int r = 0; r < 2; ++r) {
      init_block(d, lv.blocks[r], p + ".block." + std::to_string(r), cin, cout);
      cin = cout;
      if (!lv.attn.empty()) init_attn(d, lv.attn[r], p + ".attn." + std::to_string(r), r);
    }
    lv.has_samp = l != T_LEVELS - 1;
    if (lv.has_samp) {
      shape_down_conv(lv.samp, cout);
      alloc_conv(d, lv.samp);
      name_conv(d, lv.samp, p + ".downsample.conv");
    }
  }
  init_block(d, d->e_mid1, "encoder.mid.block_1", top, top);
  init_attn(d, d->e_mid_attn, "encoder.mid.attn_1", 2);
  init_block(d, d->e_mid2, "encoder.mid.block_2", top, top);
  init_norm(d, d->e_norm_out, "encoder.norm_out", top);
  init_conv(d, d->e_conv_out, "encoder.conv_out", top, T_Z, 3);
  init_conv(d, d->quant_conv, "quant_conv", T_Z, T_Z, 1);
  // ---- Decoder.__init__ (:283-338)
  init_conv(d, d->post_quant_conv, "post_quant_conv", T_Z, T_Z, 1);
  init_conv(d, d->d_conv_in, "decoder.conv_in", T_Z, top, 3);
  init_block(d, d->d_mid1, "decoder.mid.block_1", top, top);
  init_attn(d, d->d_mid_attn, "decoder.mid.attn_1", 3);
  init_block(d, d->d_mid2, "decoder.mid.block_2", top, top);
  cin = top;
  for (int l = T_LEVELS - 1; l >= 0; --l) {
    TLevel& lv = d->d_up[l];
    const int cout = T_CH * T_MULT[l];
    const std::string p = "decoder.up." + std::to_string(l);
    lv.blocks.resize(3);
    if (l == T_LEVELS - 1) lv.attn.resize(3);
    for (int r = 0; r < 3; ++r) {
      init_block(d, lv.blocks[r], p + ".block." + std::to_string(r), cin, cout);
      cin = cout;
      if (!lv.attn.empty()) init_attn(d, lv.attn[r], p + ".attn." + std::to_string(r), 4 + r);
    }
    lv.has_samp = l != 0;
    if (lv.has_samp) init_conv(d, lv.samp, p + ".upsample.conv", cout, cout, 3, true);
  }
  init_norm(d, d->d_norm_out, "decoder.norm_out", T_CH);
  init_conv(d, d->d_conv_out, "decoder.conv_out", T_CH, 3, 3, false, true);
  m.get(&d->fold_w, (size_t)3 * T_CH * 9);
  // the largest activation: 128 channels at the image resolution (= its space-to-depth form = 64 padded channels of the packed image x 2)
  const size_t max_elems = (size_t)d->res * d->res * T_CH;
  for (int i = 0; i < 3; ++i) m.get(&d->buf[i], (size_t)max_batch * max_elems);
  const size_t nlat = (size_t)max_batch * latent_size * latent_size;
  m.get(&d->qkv, nlat * 3 * T_ATT);
  m.get(&d->z, nlat * T_Z);
  m.get(&d->gn.part, gn_part_elems(max_batch, d->res, d->res));
  m.get(&d->gn.ss, (size_t)max_batch * 4096);
  VqCodebook& q = d->q;
  q.C = T_CODES; q.K = T_Z; q.Kp = vq_kp(q.K); q.Cpad = vq_cpad(q.C); q.l2 = 0;
  const size_t npad = (size_t)vq_npad((int)nlat);
  m.get(&q.cb, (size_t)q.C * q.K); m.get(&q.cbT, (size_t)q.Kp * q.Cpad); m.get(&q.cbn, (size_t)q.Cpad);
  m.get(&d->vq_zT, (size_t)q.Kp * npad); m.get(&d->vq_ps, VQ_SPLIT_MAX * npad); m.get(&d->vq_pi, VQ_SPLIT_MAX * npad);
  if (int rc = m.failed("mb_taming_create")) { delete d; return rc; }
  *out = d;
  return 0;
}
void mb_taming_destroy(mb_taming* d) { delete d; }

int mb_taming_load(mb_taming* d, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!d || !name || !data || (ndim > 0 && !shape)) return fail(-1, "mb_taming_load: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const std::string n(name);
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
  if (n == "quantize.embedding.weight") {                                        // SimpleVectorizer.embedding [1024, 256]
    if (ndim != 2 || shape[0] != d->q.C || shape[1] != d->q.K) return fail(-4, "mb_taming_load: %s: expected [1024, 256]", name);
    vq_prep_codebook(d->q, data, s);
    d->cb_loaded = true;
    return 0;
  }
  const auto it = d->params.find(n);
  if (it == d->params.end()) return fail(-2, "mb_taming_load: unknown checkpoint entry '%s'", name);
  const TParam& p = it->second;
  if (!p.conv) {
    if (numel != (size_t)p.n) return fail(-4, "mb_taming_load: %s: wrong norm size", name);
    HIP_TRY(hipMemcpyAsync(p.vec, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else if (p.bias) {
    if (numel != (size_t)p.rows) return fail(-4, "mb_taming_load: %s: wrong bias size", name);
    if (p.fold) hipLaunchKernelGGL(affine_kernel, dim3(1), dim3(64), 0, s, data, p.conv->b, numel, 0.5f, 1.0f);
    else HIP_TRY(hipMemcpyAsync(p.conv->b + p.row0, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {
    const Conv& c = *p.conv;                                                     // (downsample.conv: the checkpoint's 3x3, whatever the taps it runs as)
    const int taps = c.down ? 9 : c.ks * c.ks;
    if (numel != (size_t)p.rows * c.cin * taps) return fail(-4, "mb_taming_load: %s: wrong weight size", name);
    const float* src = data;
    if (p.fold) {
      hipLaunchKernelGGL(affine_kernel, dim3(16), dim3(256), 0, s, data, d->fold_w, numel, 0.5f, 0.0f);
      src = d->fold_w;
    }
    // a slice of a stacked 1x1 conv (q / k / v): rows [row0, row0 + rows) of its [cout_pad][cin_pad] image
    const int rows_pad = p.rows == c.cout_w ? c.cout_pad : p.rows;
    launch_repack_conv(s, src, c.w + (size_t)p.row0 * c.cin_pad, p.rows, c.cin, c.ks, rows_pad, c.cin_pad, c.down);
  }
  return launched();
}

int mb_taming_encode(mb_taming* d, const float* img_nchw, int64_t* indices, float* zq, float* zraw, float* row_dist, int B, mb_stream stream) {
  if (!d || !img_nchw || !indices) return fail(-1, "mb_taming_encode: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("taming_encode", s);
  if (!d->cb_loaded) return fail(-1, "mb_taming_encode: the codebook (quantize.embedding.weight) is not loaded");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_taming_encode: batch outside [1, max_batch]");
  const int t = encode_to_z(d, img_nchw, B, s);
  const int hw = d->latent * d->latent, N = B * hw;
  vq_prep_rows(d->q, d->buf[t], d->quant_conv.cout, nullptr, N, hw, d->vq_zT, zraw, s);
  vq_search(d->q, d->vq_zT, N, hw, vq_splits(d->q, N, 0), d->vq_ps, d->vq_pi, indices, zq, row_dist, s);
  return launched();
}
int mb_taming_decode(mb_taming* d, const int64_t* tokens, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream) {
  if (!d || !tokens || !(img_nchw || img_nhwc_u8)) return fail(-1, "mb_taming_decode: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("taming_decode", s);
  if (!d->cb_loaded) return fail(-1, "mb_taming_decode: the codebook (quantize.embedding.weight) is not loaded");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_taming_decode: batch outside [1, max_batch]");
  vq_gather(d->q, tokens, (size_t)B * d->latent * d->latent, d->z, T_Z, d->sat, s);
  decode_from_z(d, img_nchw, img_nhwc_u8, B, s);
  return launched();
}
int mb_taming_decode_latent(mb_taming* d, const float* z_nchw, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream) {
  if (!d || !z_nchw || !(img_nchw || img_nhwc_u8)) return fail(-1, "mb_taming_decode_latent: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("taming_decode", s);
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_taming_decode_latent: batch outside [1, max_batch]");
  vq_pack_latent(z_nchw, B, T_Z, d->latent * d->latent, d->z, T_Z, d->sat, s);
  decode_from_z(d, img_nchw, img_nhwc_u8, B, s);
  return launched();
}
// synchronises the stream
int mb_taming_saturation_count(mb_taming* d, unsigned* count, int reset, mb_stream stream) {
  if (!d || !count) return fail(-1, "mb_taming_saturation_count: null argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(count, d->sat, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess ||
      (reset && hipMemsetAsync(d->sat, 0, sizeof(unsigned), s) != hipSuccess) || hipStreamSynchronize(s) != hipSuccess)
    return fail(-10, "mb_taming_saturation_count: copy failed");
  return 0;
}

// ---- diagnostics (include/maskbit_hip_diag.h)
int mb_taming_set_tap(mb_taming* d, int block, void* out_h16) {
  if (!d || block < 0 || block >= T_NATTN) return fail(-1, "mb_taming_set_tap: block outside [0, 7)");
  d->tap[block] = out_h16;
  return 0;
}
}  // extern "C"
