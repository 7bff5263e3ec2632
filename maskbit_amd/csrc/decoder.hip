// The tokenizer handle of libmaskbit_hip.so (mb_dec_* / mb_enc_*, include/maskbit_hip.h): the conv-VQGAN decoder (ConvDecoder.forward,
// modeling/modules/autoencoder.py:399-423) and, when built, its encoder (ConvEncoder, :230-286) with the LFQ or the lookup (VQ) quantizer.
// This file is the layer schedule and the entry points; the ResNet block and the checkpoint ingest are shared with the Taming handle (mb_autoenc.h),
// the kernels and their launchers are conv.hip (mb_conv.h) and vq.hip (mb_vq.h).
#include <string>
#include <vector>

#include "../../include/maskbit_hip.h"
#include "mb_autoenc.h"
#include "mb_vq.h"

namespace mb {
struct Stage { std::vector<ResBlock> blocks; Conv up; bool has_up = false; };   // `up`: upsample_conv (decoder) / down_conv (encoder)
}  // namespace mb

struct mb_dec : mb::AutoEnc {
  mb_dec_cfg c{};
  int max_batch = 0, out_res = 0;
  mb::Conv conv_in, conv_out;
  mb::Norm norm_out;
  std::vector<mb::ResBlock> mid;
  std::vector<mb::Stage> up;
  // encoder half (built when cfg.build_encoder): conv_in, down stages, mid, norm_out, conv_out
  bool has_enc = false;
  mb::Conv e_conv_in, e_conv_out;
  mb::Norm e_norm_out;
  std::vector<mb::ResBlock> e_mid;
  std::vector<mb::Stage> e_down;
  h16* z = nullptr;              // decoder input latent, [max_batch * latent^2][conv_in.cin_pad]
  // lookup quantizer (mb_dec_create_vq; SimpleVectorizer, modeling/quantizer/quantizer.py): allocated on a lookup handle only
  bool lookup = false;
  mb::VqWorkspace vq;
};

using namespace mb;

namespace {

// ResBlock of autoencoder.py:46-96: convolutions without bias, the shortcut on the block's own output (ResBlock::sc_on_input = false)
void init_block(mb_dec* d, ResBlock& rb, const std::string& p, int cin, int cout) { mb::init_block(*d, rb, p, cin, cout, false, false); }

// ConvDecoder.forward (autoencoder.py:399-423) from the latent in d->z
void decode_from_z(mb_dec* d, float* img_nchw, uint8_t* img_nhwc_u8, int B, hipStream_t s) {
  int res = d->c.latent_size;
  launch_conv(s, &d->gn, d->conv_in, d->z, nullptr, nullptr, d->buf[0], nullptr, nullptr, B, res, res, false);
  int xi = 0;
  for (auto& rb : d->mid) xi = run_block(s, *d, rb, xi, B, res, res);
  for (auto& st : d->up) {
    for (auto& rb : st.blocks) xi = run_block(s, *d, rb, xi, B, res, res);
    if (st.has_up) {
      res *= 2;
      const int t = (xi + 1) % 3;
      launch_conv(s, &d->gn, st.up, d->buf[xi], nullptr, nullptr, d->buf[t], nullptr, nullptr, B, res, res, false);
      xi = t;
    }
  }
  launch_gn(s, &d->gn, d->norm_out, d->buf[xi], B, res * res);
  launch_conv(s, &d->gn, d->conv_out, d->buf[xi], d->gn.ss, nullptr, nullptr, img_nchw, img_nhwc_u8, B, res, res, true);
}

// ConvEncoder.forward (autoencoder.py:264-286) -> index of the buffer holding z (fp16 NHWC, e_conv_out.cout channels per pixel); *res_out = its side
int encode_to_z(mb_dec* d, const float* img, int B, hipStream_t s, int* res_out) {
  const mb_dec_cfg& c = d->c;
  int res = d->out_res;
  launch_pack_image(s, img, d->buf[2], B, c.num_channels, res, res);
  launch_conv(s, &d->gn, d->e_conv_in, d->buf[2], nullptr, nullptr, d->buf[0], nullptr, nullptr, B, res, res, false);
  int xi = 0;
  for (auto& st : d->e_down) {
    for (auto& rb : st.blocks) xi = run_block(s, *d, rb, xi, B, res, res);
    if (st.has_up) {
      const int t = (xi + 1) % 3, t2 = (xi + 2) % 3;
      if (!c.sample_with_conv) {                           // F.avg_pool2d(2, 2) (autoencoder.py:182)
        launch_avgpool2(s, d->buf[xi], d->buf[t], B, res, res, st.up.cin);
        d->gn.of = nullptr;                             // (no conv wrote this tensor: its GroupNorm takes the separate sweep)
        res /= 2;
        xi = t;
        continue;
      }
      launch_s2d(s, d->buf[xi], d->buf[t], B, res, res, st.up.cin);
      res /= 2;
      launch_conv(s, &d->gn, st.up, d->buf[t], nullptr, nullptr, d->buf[t2], nullptr, nullptr, B, res, res, false);
      xi = t2;
    }
  }
  for (auto& rb : d->e_mid) xi = run_block(s, *d, rb, xi, B, res, res);
  launch_gn(s, &d->gn, d->e_norm_out, d->buf[xi], B, res * res);
  const int t = (xi + 1) % 3;
  launch_conv(s, &d->gn, d->e_conv_out, d->buf[xi], d->gn.ss, nullptr, d->buf[t], nullptr, nullptr, B, res, res, false);
  *res_out = res;
  return t;
}

// mb_dec_create / mb_dec_create_vq (`what`).  codebook_size > 0: a lookup (VQ) handle with that many entries; 0: the LFQ handle
int create_handle(const char* what, const mb_dec_cfg& cfg, int max_batch, int codebook_size, int l2_normalize, mb_dec** out) {
  const int R = cfg.num_resolutions;
  const bool vq = codebook_size > 0;
  if (R < 1 || R > 7) return fail(-1, "%s: num_resolutions out of range", what);
  if (cfg.hidden_channels % 64) return fail(-1, "%s: hidden_channels must be a multiple of 64 for the HIP decoder", what);
  if (!vq && (cfg.token_size > CK || cfg.token_size < 1)) return fail(-1, "%s: token_size must be in [1, 64]", what);
  if (vq && (cfg.token_size > 256 || cfg.token_size < 1)) return fail(-1, "%s: token_size must be in [1, 256]", what);
  if (cfg.latent_size % 16) return fail(-1, "%s: latent_size must be a multiple of 16", what);
  if (cfg.num_channels > 4) return fail(-1, "%s: num_channels > 4 unsupported", what);
  mb_dec* d = new mb_dec();
  DevArena& m = d->mem;
  d->c = cfg; d->max_batch = max_batch; d->out_res = cfg.latent_size << (R - 1);
  m.zeroed(&d->sat, 1);
  const int hc = cfg.hidden_channels;
  std::vector<int> mult(cfg.channel_mult, cfg.channel_mult + R);
  mult.push_back(cfg.channel_mult[R - 1]);
  const int top = hc * cfg.channel_mult[R - 1];
  init_conv(*d, d->conv_in, "decoder.conv_in", cfg.token_size, top, 3, true, false, false);
  d->mid.resize(cfg.num_res_blocks);
  for (int r = 0; r < cfg.num_res_blocks; ++r) init_block(d, d->mid[r], "decoder.mid.res_blocks." + std::to_string(r), top, top);
  d->up.resize(R);
  int last = top;
  int res = cfg.latent_size;
  size_t max_elems = std::max((size_t)res * res * top, (size_t)d->out_res * d->out_res * (size_t)std::max(CK, hc));
  for (int s = 0; s < R; ++s) {                          // up.0 = coarsest level (autoencoder.py:384-392)
    const int lvl = R - 1 - s;
    const int cin = hc * mult[lvl + 1], cout = hc * mult[lvl];
    Stage& st = d->up[s];
    st.blocks.resize(cfg.num_res_blocks);
    int c = cin;
    for (int r = 0; r < cfg.num_res_blocks; ++r) {
      init_block(d, st.blocks[r], "decoder.up." + std::to_string(s) + ".res_blocks." + std::to_string(r), c, cout);
      c = cout;
    }
    max_elems = std::max(max_elems, (size_t)res * res * std::max(cin, cout));
    st.has_up = lvl > 0;
    if (st.has_up) {
      init_conv(*d, st.up, "decoder.up." + std::to_string(s) + ".upsample_conv", cout, cout, 3, true, true, false);
      res *= 2;
      max_elems = std::max(max_elems, (size_t)res * res * cout);
    }
    last = cout;
  }
  init_norm(*d, d->norm_out, "decoder.norm_out", last);
  init_conv(*d, d->conv_out, "decoder.conv_out", last, cfg.num_channels, 3, true, false, true);
  if (cfg.build_encoder) {                                // ConvEncoder (autoencoder.py:230-262): mirrors the decoder top-down
    const int enrb = cfg.enc_res_blocks > 0 ? cfg.enc_res_blocks : cfg.num_res_blocks;
    std::vector<int> imult{1};
    imult.insert(imult.end(), cfg.channel_mult, cfg.channel_mult + R);
    init_conv(*d, d->e_conv_in, "encoder.conv_in", cfg.num_channels, hc, 3, false, false, false);
    d->e_down.resize(R);
    for (int s = 0; s < R; ++s) {
      const int cin = hc * imult[s], cout = hc * imult[s + 1];
      Stage& st = d->e_down[s];
      st.blocks.resize(enrb);
      int c = cin;
      for (int r = 0; r < enrb; ++r) {
        init_block(d, st.blocks[r], "encoder.down." + std::to_string(s) + ".res_blocks." + std::to_string(r), c, cout);
        c = cout;
      }
      st.has_up = s < R - 1;                              // a downsampling step follows: down_conv, or avg_pool2d when !sample_with_conv
      st.up.cin = cout;
      if (st.has_up && cfg.sample_with_conv) {            // DownsamplingStage.down_conv: 3x3, stride 2, bias (autoencoder.py:165)
        shape_down_conv(st.up, cout);
        alloc_conv(*d, st.up);
        name_conv(*d, st.up, "encoder.down." + std::to_string(s) + ".down_conv");
      }
    }
    d->e_mid.resize(enrb);
    for (int r = 0; r < enrb; ++r) init_block(d, d->e_mid[r], "encoder.mid.res_blocks." + std::to_string(r), top, top);
    const int k4 = (cfg.token_size + 3) / 4 * 4;           // stored channel count of z (8-byte stores)
    init_norm(*d, d->e_norm_out, "encoder.norm_out", top);
    init_conv(*d, d->e_conv_out, "encoder.conv_out", top, k4, 1, true, false, false);
    d->e_conv_out.cout_w = cfg.token_size;
    d->has_enc = true;
  }
  for (int i = 0; i < 3; ++i) m.get(&d->buf[i], (size_t)max_batch * max_elems);
  const size_t nlat = (size_t)max_batch * cfg.latent_size * cfg.latent_size;
  m.get(&d->z, nlat * d->conv_in.cin_pad);
  m.get(&d->gn.part, gn_part_elems(max_batch, d->out_res, d->out_res));
  m.get(&d->gn.ss, (size_t)max_batch * 4096);
  d->lookup = vq;
  if (vq) d->vq.alloc(m, codebook_size, cfg.token_size, l2_normalize, nlat);
  if (int rc = m.failed(what)) { delete d; return rc; }
  *out = d;
  return 0;
}

// ConvVQModel.encode with the lookup quantizer: mb_enc_encode_vq, and mb_enc_encode on a lookup handle (`what`)
int encode_vq(const char* what, mb_dec* d, const float* img, int64_t* indices, float* zq, float* zraw, float* row_dist, int B, hipStream_t s) {
  ProfScope p("encode", s);
  if (!d->has_enc) return fail(-1, "%s: this engine was created without the encoder half (mb_dec_cfg.build_encoder)", what);
  if (!d->lookup) return fail(-1, "%s: not a lookup (VQ) handle", what);
  if (!d->vq.loaded) return fail(-1, "%s: the codebook (quantize.embedding.weight) is not loaded", what);
  if (B <= 0 || B > d->max_batch) return fail(-1, "%s: batch outside [1, max_batch]", what);
  int res = 0;
  const int t = encode_to_z(d, img, B, s, &res);
  d->vq.encode_rows(d->buf[t], d->e_conv_out.cout, B * res * res, res * res, indices, zq, zraw, row_dist, s);
  return launched();
}

}  // namespace

extern "C" {

int mb_dec_create(const mb_dec_cfg* cfg, int max_batch, mb_dec** out) {
  if (!cfg || !out || max_batch <= 0) return fail(-1, "mb_dec_create: bad arguments");
  return create_handle("mb_dec_create", *cfg, max_batch, 0, 0, out);
}
int mb_dec_create_vq(const mb_dec_cfg* cfg, int codebook_size, int l2_normalize, int max_batch, mb_dec** out) {
  if (!cfg || !out || max_batch <= 0) return fail(-1, "mb_dec_create_vq: bad arguments");
  if (codebook_size < 2 || codebook_size > 65536) return fail(-1, "mb_dec_create_vq: codebook_size %d outside [2, 65536]", codebook_size);
  return create_handle("mb_dec_create_vq", *cfg, max_batch, codebook_size, l2_normalize, out);
}
void mb_dec_destroy(mb_dec* d) { delete d; }

int mb_dec_load(mb_dec* d, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!d || !name || !data) return fail(-1, "mb_dec_load: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const std::string n(name);
  if (d->lookup && n == "quantize.embedding.weight") {                           // SimpleVectorizer.embedding [C, K]
    if (!d->vq.load_codebook(shape, ndim, data, s)) return fail(-4, "mb_dec_load: %s: expected [codebook_size, token_size]", name);
    return launched();
  }
  if (n.rfind("quantize.", 0) == 0) return 0;                                    // derived buffers
  if (n.rfind("encoder.", 0) == 0 && !d->has_enc) return 0;                       // encode half not built in this engine
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
  return load_param("mb_dec_load", *d, name, data, numel, s);
}

int mb_dec_decode(mb_dec* d, const int64_t* tokens, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream) {
  if (!d || !tokens) return fail(-1, "mb_dec_decode: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("decode", s);
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_dec_decode: batch outside [1, max_batch]");
  const mb_dec_cfg& c = d->c;
  const size_t npix = (size_t)B * c.latent_size * c.latent_size;
  if (d->lookup) {                                    // SimpleVectorizer.get_codebook_entry (quantizer.py:105-119): codebook rows
    if (!d->vq.loaded) return fail(-1, "mb_dec_decode: the codebook (quantize.embedding.weight) is not loaded");
    vq_gather(d->vq.q, tokens, npix, d->z, d->conv_in.cin_pad, d->sat, s);
  } else {
    launch_latent(s, tokens, d->z, npix, c.token_size);
  }
  decode_from_z(d, img_nchw, img_nhwc_u8, B, s);
  return launched();
}
int mb_dec_decode_latent(mb_dec* d, const float* z_nchw, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream) {
  if (!d || !z_nchw) return fail(-1, "mb_dec_decode_latent: null argument");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("decode", s);
  if (!d->lookup) return fail(-1, "mb_dec_decode_latent: decode of a float latent needs a lookup (VQ) handle");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_dec_decode_latent: batch outside [1, max_batch]");
  const int hw = d->c.latent_size * d->c.latent_size;
  vq_pack_latent(z_nchw, B, d->c.token_size, hw, d->z, d->conv_in.cin_pad, d->sat, s);
  decode_from_z(d, img_nchw, img_nhwc_u8, B, s);
  return launched();
}

// synchronises the stream
int mb_dec_saturation_count(mb_dec* d, unsigned* count, int reset, mb_stream stream) {
  if (!d || !count) return fail(-1, "mb_dec_saturation_count: null argument");
  return read_counter("mb_dec_saturation_count", d->sat, count, reset, (hipStream_t)stream);
}

// ConvVQModel.encode (conv_vqgan.py:70-83): image [B,C,H,W] fp32 -> code indices [B, h*w] (+ optional +-1 latent / raw z, fp32 NCHW)
int mb_enc_encode(mb_dec* d, const float* img_nchw, int64_t* indices, float* zq, float* zraw, int B, mb_stream stream) {
  if (!d || !img_nchw || !indices) return fail(-1, "mb_enc_encode: null argument");
  hipStream_t s = (hipStream_t)stream;
  if (d->lookup) return encode_vq("mb_enc_encode", d, img_nchw, indices, zq, zraw, nullptr, B, s);
  ProfScope p("encode", s);
  if (!d->has_enc) return fail(-1, "mb_enc_encode: this engine was created without the encoder half (mb_dec_cfg.build_encoder)");
  if (B <= 0 || B > d->max_batch) return fail(-1, "mb_enc_encode: batch outside [1, max_batch]");
  int res = 0;
  const int t = encode_to_z(d, img_nchw, B, s, &res);
  launch_lfq(s, d->buf[t], indices, zq, zraw, B, res * res, d->c.token_size, d->e_conv_out.cout);
  return launched();
}
int mb_enc_encode_vq(mb_dec* d, const float* img_nchw, int64_t* indices, float* zq, float* zraw, float* row_dist, int B, mb_stream stream) {
  if (!d || !img_nchw || !indices) return fail(-1, "mb_enc_encode_vq: null argument");
  return encode_vq("mb_enc_encode_vq", d, img_nchw, indices, zq, zraw, row_dist, B, (hipStream_t)stream);
}

}  // extern "C"
