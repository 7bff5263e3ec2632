// The Taming VQGAN tokenizer handle of libmaskbit_hip.so (mb_taming_*, include/maskbit_hip.h): OriginalVQModel (modeling/taming_vqgan.py:19-69) =
// Encoder / Decoder of modeling/taming/taming_autoencoder.py (:176-267, :270-370) around SimpleVectorizer(1024, 256) with quant_conv / post_quant_conv.
// This file is the layer schedule, the attention block and the entry points; the ResNet block and the checkpoint ingest are shared with the
// conv-VQGAN handle (mb_autoenc.h), the kernels and their launchers are conv.hip (mb_conv.h), spatial_attention.hip (mb_spattn.h) and vq.hip
// (mb_vq.h).  The network is fixed (taming_vqgan.py:26-37): ch 128, ch_mult (1,1,2,2,4), 2 res blocks per level (the decoder runs 3), attention
// at the 16-pixel level, z_channels 256.
#include <string>
#include <vector>

#include "../../include/maskbit_hip.h"
#include "../../include/maskbit_hip_diag.h"
#include "mb_autoenc.h"
#include "mb_spattn.h"
#include "mb_vq.h"

namespace mb {
namespace {
constexpr int T_CH = 128, T_LEVELS = 5, T_Z = 256, T_CODES = 1024, T_ATT = 512, T_NATTN = 7;
constexpr int T_MULT[T_LEVELS] = {1, 1, 2, 2, 4};

// AttnBlock (:121-173): q, k, v stacked into one 1x1 conv 512 -> 1536 behind the GroupNorm (no SiLU), proj_out with the residual
struct TAttn { Norm n; Conv qkv, proj; int tap = 0; };
struct TLevel { std::vector<ResBlock> blocks; std::vector<TAttn> attn; Conv samp; bool has_samp = false; };
}  // namespace
}  // namespace mb

struct mb_taming : mb::AutoEnc {
  int max_batch = 0, latent = 0, res = 0;
  // encoder
  mb::Conv e_conv_in, e_conv_out, quant_conv;
  mb::TLevel e_down[mb::T_LEVELS];
  mb::ResBlock e_mid1, e_mid2; mb::TAttn e_mid_attn;
  mb::Norm e_norm_out;
  // decoder: up[i] = level i, 0 the finest (taming_autoencoder.py:330)
  mb::Conv post_quant_conv, d_conv_in, d_conv_out;
  mb::TLevel d_up[mb::T_LEVELS];
  mb::ResBlock d_mid1, d_mid2; mb::TAttn d_mid_attn;
  mb::Norm d_norm_out;
  h16* qkv = nullptr;            // [max_batch * latent^2][1536]
  h16* z = nullptr;              // decoder input latent [max_batch * latent^2][256]
  mb::VqWorkspace vq;            // SimpleVectorizer(1024, 256)
  void* tap[mb::T_NATTN] = {};   // diagnostic (mb_taming_set_tap): where the output of AttnBlock i is copied to, or null
};

using namespace mb;

namespace {

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

void launch_pack_image_pm1(hipStream_t s, const float* img, h16* out, int B, int H, int W) {
  const size_t npix = (size_t)B * H * W;
  hipLaunchKernelGGL(pack_image_pm1_kernel, dim3((unsigned)std::min<size_t>(4096, (npix * 8 + 255) / 256)), dim3(256), 0, s, img, out, B, 3, H, W);
}

// Every convolution of this network has a bias
void init_conv(mb_taming* d, Conv& c, const std::string& name, int cin, int cout, int ks, bool up = false) {
  mb::init_conv(*d, c, name, cin, cout, ks, true, up);
}
// ResnetBlock (taming_autoencoder.py:59-118): nin_shortcut is applied to the block INPUT (ResBlock::sc_on_input)
void init_block(mb_taming* d, ResBlock& rb, const std::string& p, int cin, int cout) { mb::init_block(*d, rb, p, cin, cout, true, true); }
void init_attn(mb_taming* d, TAttn& at, const std::string& p, int tap) {
  at.tap = tap;
  init_norm(*d, at.n, p + ".norm", T_ATT);
  shape_conv(at.qkv, T_ATT, 3 * T_ATT, 1, true, false, false);
  alloc_conv(*d, at.qkv);
  const char* nm[3] = {".q", ".k", ".v"};
  for (int i = 0; i < 3; ++i) {
    d->params[p + nm[i] + ".weight"] = Param{&at.qkv, false, nullptr, 0, i * T_ATT, T_ATT};
    d->params[p + nm[i] + ".bias"] = Param{&at.qkv, true, nullptr, 0, i * T_ATT, T_ATT};
  }
  init_conv(d, at.proj, p + ".proj_out", T_ATT, T_ATT, 1);
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
  launch_pack_image_pm1(s, img, d->buf[2], B, res, res);
  launch_conv(s, &d->gn, d->e_conv_in, d->buf[2], nullptr, nullptr, d->buf[0], nullptr, nullptr, B, res, res, false);
  int xi = 0;
  for (int l = 0; l < T_LEVELS; ++l) {
    TLevel& lv = d->e_down[l];
    for (size_t r = 0; r < lv.blocks.size(); ++r) {
      xi = run_block(s, *d, lv.blocks[r], xi, B, res, res);
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
  xi = run_block(s, *d, d->e_mid1, xi, B, res, res);
  xi = run_attn(s, d, d->e_mid_attn, xi, B, res, res);
  xi = run_block(s, *d, d->e_mid2, xi, B, res, res);
  launch_gn(s, &d->gn, d->e_norm_out, d->buf[xi], B, res * res);
  const int t = (xi + 1) % 3, t2 = (xi + 2) % 3;
  launch_conv(s, &d->gn, d->e_conv_out, d->buf[xi], d->gn.ss, nullptr, d->buf[t], nullptr, nullptr, B, res, res, false, false);
  launch_conv(s, &d->gn, d->quant_conv, d->buf[t], nullptr, nullptr, d->buf[t2], nullptr, nullptr, B, res, res, false, false);
  return t2;
}

// decoder.norm_out + the folded decoder.conv_out (taming_autoencoder.py:366-369, taming_vqgan.py:55) on x = buf[xi] -> the image
void final_layer(mb_taming* d, int xi, float* img_nchw, uint8_t* img_nhwc_u8, int B, int H, int W, hipStream_t s) {
  launch_gn(s, &d->gn, d->d_norm_out, d->buf[xi], B, H * W);
  launch_conv(s, &d->gn, d->d_conv_out, d->buf[xi], d->gn.ss, nullptr, nullptr, img_nchw, img_nhwc_u8, B, H, W, true);
}

// post_quant_conv + Decoder.forward (taming_vqgan.py:52-56, taming_autoencoder.py:340-370) from the latent in d->z
void decode_from_z(mb_taming* d, float* img_nchw, uint8_t* img_nhwc_u8, int B, hipStream_t s) {
  int res = d->latent;
  launch_conv(s, &d->gn, d->post_quant_conv, d->z, nullptr, nullptr, d->buf[1], nullptr, nullptr, B, res, res, false, false);
  launch_conv(s, &d->gn, d->d_conv_in, d->buf[1], nullptr, nullptr, d->buf[0], nullptr, nullptr, B, res, res, false);
  int xi = 0;
  xi = run_block(s, *d, d->d_mid1, xi, B, res, res);
  xi = run_attn(s, d, d->d_mid_attn, xi, B, res, res);
  xi = run_block(s, *d, d->d_mid2, xi, B, res, res);
  for (int l = T_LEVELS - 1; l >= 0; --l) {
    TLevel& lv = d->d_up[l];
    for (size_t r = 0; r < lv.blocks.size(); ++r) {
      xi = run_block(s, *d, lv.blocks[r], xi, B, res, res);
      if (!lv.attn.empty()) xi = run_attn(s, d, lv.attn[r], xi, B, res, res);
    }
    if (lv.has_samp) {                                     // Upsample (:30-34): nearest 2x fused into the 3x3 conv
      res *= 2;
      const int t = (xi + 1) % 3;
      launch_conv(s, &d->gn, lv.samp, d->buf[xi], nullptr, nullptr, d->buf[t], nullptr, nullptr, B, res, res, false);
      xi = t;
    }
  }
  final_layer(d, xi, img_nchw, img_nhwc_u8, B, res, res, s);
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
      alloc_conv(*d, lv.samp);
      name_conv(*d, lv.samp, p + ".downsample.conv");
    }
  }
  init_block(d, d->e_mid1, "encoder.mid.block_1", top, top);
  init_attn(d, d->e_mid_attn, "encoder.mid.attn_1", 2);
  init_block(d, d->e_mid2, "encoder.mid.block_2", top, top);
  init_norm(*d, d->e_norm_out, "encoder.norm_out", top);
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
  init_norm(*d, d->d_norm_out, "decoder.norm_out", T_CH);
  // the final convolution, folded: it carries decode's (y + 1) / 2 (taming_vqgan.py:55)
  mb::init_conv(*d, d->d_conv_out, "decoder.conv_out", T_CH, 3, 3, true, false, true, true);
  // the largest activation: 128 channels at the image resolution (= its space-to-depth form = 64 padded channels of the packed image x 2)
  const size_t max_elems = (size_t)d->res * d->res * T_CH;
  for (int i = 0; i < 3; ++i) m.get(&d->buf[i], (size_t)max_batch * max_elems);
  const size_t nlat = (size_t)max_batch * latent_size * latent_size;
  m.get(&d->qkv, nlat * 3 * T_ATT);
  m.get(&d->z, nlat * T_Z);
  m.get(&d->gn.part, gn_part_elems(max_batch, d->res, d->res));
  m.get(&d->gn.ss, (size_t)max_batch * 4096);
  d->vq.alloc(m, T_CODES, T_Z, 0, nlat);
  if (int rc = m.failed("mb_taming_create")) { delete d; return rc; }
  *out = d;
  return 0;
}
void mb_taming_destroy(mb_taming* d) { delete d; }

int mb_taming_load(mb_taming* d, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!d || !name || !data || (ndim > 0 && !shape)) return fail(-1, "mb_taming_load: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (std::string(name) == "quantize.embedding.weight") {                        // SimpleVectorizer.embedding [1024, 256]
    if (!d->vq.load_codebook(shape, ndim, data, s)) return fail(-4, "mb_taming_load: %s: expected [1024, 256]", name);
    return launched();
  }
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
  return load_param("mb_taming_load", *d, name, data, numel, s);
}

int mb_taming_encode(mb_taming* d, const float* img_nchw, int64_t* indices, float* zq, float* zraw, float* row_dist, int B, mb_stream stream) {
  if (!d || !img_nchw || !indices) return fail(-1, "mb_taming_encode: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("taming_encode", s);
  if (!d->vq.loaded) return fail(-1, "mb_taming_encode: the codebook (quantize.embedding.weight) is not loaded");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_taming_encode: batch outside [1, max_batch]");
  const int t = encode_to_z(d, img_nchw, B, s);
  const int hw = d->latent * d->latent;
  d->vq.encode_rows(d->buf[t], d->quant_conv.cout, B * hw, hw, indices, zq, zraw, row_dist, s);
  return launched();
}
int mb_taming_decode(mb_taming* d, const int64_t* tokens, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream) {
  if (!d || !tokens || !(img_nchw || img_nhwc_u8)) return fail(-1, "mb_taming_decode: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("taming_decode", s);
  if (!d->vq.loaded) return fail(-1, "mb_taming_decode: the codebook (quantize.embedding.weight) is not loaded");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_taming_decode: batch outside [1, max_batch]");
  vq_gather(d->vq.q, tokens, (size_t)B * d->latent * d->latent, d->z, T_Z, d->sat, s);
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
  return read_counter("mb_taming_saturation_count", d->sat, count, reset, (hipStream_t)stream);
}

// ---- diagnostics (include/maskbit_hip_diag.h)
int mb_taming_set_tap(mb_taming* d, int block, void* out_h16) {
  if (!d || block < 0 || block >= T_NATTN) return fail(-1, "mb_taming_set_tap: block outside [0, 7)");
  d->tap[block] = out_h16;
  return 0;
}
int mb_taming_attn_block(mb_taming* d, int block, const void* x_h16, void* qkv_out, void* attn_out, void* out_h16, const float* out_gamma,
                         const float* out_beta, float* out_scale_shift, int B, int H, int W, mb_stream stream) {
  if (!d || !x_h16 || !qkv_out || !attn_out || !out_h16) return fail(-1, "mb_taming_attn_block: null argument");
  if (block < 0 || block >= T_NATTN) return fail(-1, "mb_taming_attn_block: block outside [0, 7)");
  if (out_scale_shift && (!out_gamma || !out_beta)) return fail(-1, "mb_taming_attn_block: output statistics need gamma and beta");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_taming_attn_block: batch outside [1, max_batch]");
  if (H <= 0 || W <= 0 || H % TH8 || W % TW || (int64_t)H * W > (int64_t)d->latent * d->latent)
    return fail(-1, "mb_taming_attn_block: H a multiple of 8, W of 16, H W <= latent^2 required");
  hipStream_t s = (hipStream_t)stream;
  const TAttn& at = block < 2    ? d->e_down[T_LEVELS - 1].attn[block]      // numbered as init_attn's taps
                    : block == 2 ? d->e_mid_attn
                    : block == 3 ? d->d_mid_attn
                                 : d->d_up[T_LEVELS - 1].attn[block - 4];
  const size_t rows = (size_t)B * H * W;
  HIP_TRY(hipMemcpyAsync(d->buf[0], x_h16, rows * T_ATT * sizeof(h16), hipMemcpyDeviceToDevice, s));
  d->gn.of = nullptr;                               // buffer 0 is no convolution's output
  const int oi = run_attn(s, d, at, 0, B, H, W);
  HIP_TRY(hipMemcpyAsync(qkv_out, d->qkv, rows * 3 * T_ATT * sizeof(h16), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(attn_out, d->buf[1], rows * T_ATT * sizeof(h16), hipMemcpyDeviceToDevice, s));   // run_attn's t1 from buffer 0
  HIP_TRY(hipMemcpyAsync(out_h16, d->buf[oi], rows * T_ATT * sizeof(h16), hipMemcpyDeviceToDevice, s));
  if (out_scale_shift) {
    Norm n; n.c = T_ATT; n.g = const_cast<float*>(out_gamma); n.b = const_cast<float*>(out_beta);
    launch_gn(s, &d->gn, n, d->buf[oi], B, H * W);                             // from the state run_attn left in the context
    HIP_TRY(hipMemcpyAsync(out_scale_shift, d->gn.ss, (size_t)B * T_ATT * sizeof(float2), hipMemcpyDeviceToDevice, s));
  }
  return launched();
}
int mb_taming_final(mb_taming* d, const void* x_h16, float* img_nchw, uint8_t* img_nhwc_u8, int B, int H, int W, mb_stream stream) {
  if (!d || !x_h16 || !(img_nchw || img_nhwc_u8)) return fail(-1, "mb_taming_final: null argument");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_taming_final: batch outside [1, max_batch]");
  if (H <= 0 || W <= 0 || H % TH8 || W % TW || (int64_t)H * W > (int64_t)d->res * d->res)
    return fail(-1, "mb_taming_final: H a multiple of 8, W of 16, H W <= the handle's image required");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemcpyAsync(d->buf[0], x_h16, (size_t)B * H * W * T_CH * sizeof(h16), hipMemcpyDeviceToDevice, s));
  d->gn.of = nullptr;
  final_layer(d, 0, img_nchw, img_nhwc_u8, B, H, W, s);
  return launched();
}
int mb_taming_pack_image(const float* img_nchw, void* out_h16, int B, int H, int W, mb_stream stream) {
  if (!img_nchw || !out_h16) return fail(-1, "mb_taming_pack_image: null argument");
  if (B < 1 || H < 1 || W < 1 || (int64_t)B * H * W > (1 << 24)) return fail(-1, "mb_taming_pack_image: B, H, W >= 1, B * H * W <= 2^24 required");
  launch_pack_image_pm1((hipStream_t)stream, img_nchw, (h16*)out_h16, B, H, W);
  return launched();
}
}  // extern "C"
