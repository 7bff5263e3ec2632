/* libmaskbit_hip.so -- C ABI of the MI355X-native MaskBit sampling engine.
 *
 * The reference (markweberdev/maskbit) has no FFI / plugin layer: its hot path sits behind a
 * Python call surface.  This header is therefore the *new* boundary beneath the Python classes
 * that mirror that surface (maskbit_amd.LFQBert / ConvVQModel / sample); every entry point cites
 * the reference code it replaces (paths relative to the reference root).  Plain pointers and
 * sizes only -- no torch types.  All pointers are DEVICE pointers unless noted; `stream` is a
 * hipStream_t passed as void*.  Calls are stream-ordered, never synchronise the device and never
 * touch the default stream.  Return value: 0 on success, negative on error (message through
 * mb_last_error(), thread-local).  A handle is bound to the device that was current at create
 * time and is not thread-safe (the reference is single-threaded Python on one device,
 * scripts/eval_maskbit.py:65).
 */
#ifndef MASKBIT_HIP_H
#define MASKBIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MB_ABI_VERSION 8
enum { MB_PREC_FP16 = 0, MB_PREC_DIFF = 1, MB_PREC_WCORR = 2, MB_PREC_ALO = 3, MB_PREC_ALO_ALL = 4, MB_PREC_F32 = 5 };

typedef struct mb_gen mb_gen; /* generator engine  (modeling/bert.py LFQBert)            */
typedef struct mb_dec mb_dec; /* tokenizer decoder (modeling/conv_vqgan.py ConvVQModel)  */
typedef struct mb_lpips mb_lpips; /* LPIPS network (modeling/modules/lpips.py LPIPS)        */
typedef void* mb_stream;      /* hipStream_t                                              */

/* LFQBert constructor arguments (modeling/bert.py:345-358). */
typedef struct {
  int bits;    /* K = log2(codebook_size)          */
  int splits;  /* m = codebook_splits              */
  int hidden;  /* hidden_dim (multiple of 64)      */
  int heads;   /* heads; hidden/heads in {32,64}   */
  int depth;   /* transformer layers               */
  int mlp;     /* mlp_dim (multiple of 64)         */
  int seq;     /* (img_size/input_stride)^2 = 256  */
  int nclass;  /* 1000; row nclass = "dropped"     */
  /* Generator variants of modeling/bert.py: prenorm = use_prenorm (LayerNorm before each sub-layer, raw residual,
   * norm_after_transformer; bert.py:49-59,106-123,498-499); embed_tables = the `Bert` class (bert.py:184-340): per-group
   * nn.Embedding(C+1, hidden) inputs summed, output head tied to those tables plus a per-position bias [seq, C].
   * Checkpoint keys then are tok_emb_list.{g}.weight and bias.{g} instead of input_proj.* / prediction_layer.*. */
  int prenorm;
  int embed_tables;
  /* Precision mode of the engine -- ONE knob (no counterpart in the reference, which is fp32; DESIGN.md "Precision").  fp16 operands, fp32 accumulation
   * everywhere; the two head GEMMs always multiply hi + lo inputs by hi + lo weights.
   *   MB_PREC_FP16  0  single fp16 operands, guided forward = plain forward over [cond | uncond] (1.4e-3 token mismatch on configs[2]: a baseline).
   *   MB_PREC_DIFF  1  classifier-free guidance in DIFFERENTIAL form: the unconditional stream's GEMM operands are fp16(x_u - x_c), so the rounding of
   *                    x_c cancels in (c - u); plain forwards carry the LayerNorm outputs as fp16 hi + lo pairs (~1.0e-3: AT the bound).
   *   MB_PREC_WCORR 2  + MX-fp4 mini-tile correction of the fp16 rounding of all four trunk WEIGHTS (gemm_ht.hip XP = 6), guided and plain (5.5e-4).
   *   MB_PREC_ALO   3  + the same kind of pass for the fp16 rounding of the ACTIVATIONS of the guided forward's conditional stream (e2m1 of their lo halves
   *                    against e2m1 of the fp16 weight): attention outputs in out-proj and LayerNorm outputs in FFN-up, every layer (what the 7-bit-per-group
   *                    codebooks need: 3.8e-4 over four 14-bit / 256-step runs, every run <= 5.5e-4; without it one run is at 1.0e-3; rounds 4-5: FFN-up only).
   *   MB_PREC_ALO_ALL 4 + the FFN hiddens in FFN-down (the QKV set buys nothing in any measured configuration), and the zero-scale steps of a guided run
   *                    through the guided forward as well: what heavy-tailed ("trained-like") weights with massive-activation channels need (round 6).
   * Modes 1-4 need seq in {256, 1024}, hidden in {768, 1024}, mlp % 256 == 0 (2-4 also hidden / heads = 64); other shapes run mode 0 with hi + lo
   * LayerNorm outputs.  The host's default is 2, 3 from 7 bits per group on, 4 for heavy-tailed checkpoints (LFQBert.resolved_precision).
   *   MB_PREC_F32   5  the fp32 REFERENCE mode (an addition; no other mode changes): no fp16 operand anywhere.  Accepted for every configuration
   *                    mb_gen_create accepts (any seq / hidden / heads / mlp, prenorm, embed_tables).  The GEMM weights stay the checkpoint's fp32, the
   *                    workspace is fp32, every GEMM output element is one ascending-k fmaf chain on the f32-input MFMA plus one bias add
   *                    (maskbit_amd/csrc/gemm_f32.hip), attention and LayerNorm are fp32; the guided forward is the plain forward over
   *                    [B cond | B dropped].  Deterministic and independent of the batch.  About 1/16 of the fp16 MFMA rate: an instrument for judging the
   *                    other modes on a given checkpoint (maskbit_amd.check_checkpoint), never chosen by the host's auto rule.  mb_gen_forward_attn
   *                    refuses it (-3); mb_gen_saturation_count reports 0. */
  int precision;
} mb_gen_cfg;

/* ConvDecoder configuration (modeling/modules/autoencoder.py:358-397, configs/tokenizer yaml files). */
typedef struct {
  int token_size;      /* K bits per token = conv_in input channels */
  int hidden_channels; /* 128                                       */
  int num_resolutions; /* 5                                         */
  int num_res_blocks;  /* 2                                         */
  int num_channels;    /* 3                                         */
  int channel_mult[8]; /* [1,1,2,2,4]                               */
  int latent_size;     /* token grid side: 16 (=> 256x256 output)   */
  int build_encoder;   /* 1: also build ConvEncoder (autoencoder.py:230-286) for mb_enc_encode */
  int sample_with_conv;/* encoder downsampling by stride-2 conv (every shipped config); 0 = 2x2 average pooling */
  int enc_res_blocks;  /* num_res_blocks of the encoder (num_res_blocks above is the decoder's); 0 = same */
} mb_dec_cfg;

/* Per-step plan of modeling.modules.sample (modeling/modules/sampling.py:81-124), evaluated on the
 * host exactly as the reference does (float32 torch scalars) and handed over as HOST arrays. */
typedef struct {
  int num_steps;
  int use_guidance;            /* guidance_scale != 0 => 2B sequences per step (sampling.py:83-88) */
  const float* scale;          /* [num_steps] guidance_scale * a_i (sampling.py:91-98)            */
  const float* temperature;    /* [num_steps] softmax temperature (sampling.py:103-105)           */
  const int* mask_len;         /* [num_steps] floor(mask_ratio * n*m) (sampling.py:120-123)       */
  /* Step chunk of this call: step_end = 0 -> the whole run; otherwise steps [step_begin, step_end) -- the first chunk (step_begin 0) starts from the
   * all-masked state, later chunks continue from the state the engine kept, the last one (step_end = num_steps) combines and decodes.  The noise and
   * step_tokens pointers of a call hold the steps of ITS chunk (chunk-relative), the arrays above the whole run.  A chunk is accepted only as the
   * exact continuation of the run in progress on that handle (same B, num_steps, use_guidance; step_begin = the previous chunk's step_end): a
   * generator handle is NOT re-entrant while a chunked run is in progress -- two interleaved runs need two handles.
   * Steps whose scale[i] is exactly 0 run the conditional forward alone (c + 0 (c - u) == c: the unconditional forward cannot change the result; at
   * precision 4 they run the guided forward, whose conditional half is the more precise one). */
  int step_begin, step_end;
} mb_sample_plan;

int mb_abi_version(void);
const char* mb_last_error(void);

/* ---- generator: LFQBert.forward, modeling/bert.py:456-508 --------------------------------- */
int mb_gen_create(const mb_gen_cfg* cfg, int max_seqs, mb_gen** out);
void mb_gen_destroy(mb_gen* g);
/* One call per checkpoint entry (key names of SURVEY.md 8b / BaseModel.load_pretrained,
 * modeling/modules/base_model.py:87-141).  `data` is a device fp32 tensor in the checkpoint's
 * own layout; GEMM weights are repacked to fp16 here (plus the e2m1 operands of the correction passes; the two head weights as fp16
 * hi + lo planes; precision MB_PREC_F32: kept as fp32, no repack).  Unknown names return -2. */
int mb_gen_load(mb_gen* g, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream);
/* tokens int64 [nb,seq,m] (value C = masked), labels int64 [nb], drop uint8 [nb] (1 => label
 * replaced by nclass, bert.py:482-484; may be NULL) -> logits fp32 [nb,seq,m,C]. */
int mb_gen_forward(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop,
                   float* logits, int nb, mb_stream stream);
/* The guided forward of sample() (sampling.py:83-88): tokens int64 [B,seq,m], labels int64 [B] -> logits fp32 [2B,seq,m,C], rows [0,B) the
 * conditional and [B,2B) the label-dropped forward of the same tokens.  With cfg.precision >= 1 the two streams run in differential form
 * (see mb_gen_cfg.precision); the precision of the forward does not depend on the guidance scale the caller combines the two halves with. */
int mb_gen_forward_cfg(mb_gen* g, const int64_t* tokens, const int64_t* labels, float* logits, int B, mb_stream stream);
/* The same forward with `return_attn=True` (bert.py:461, 505-508; nn.MultiheadAttention need_weights with head averaging,
 * bert.py:119,137): additionally attn fp32 [depth, nb, seq+1, seq+1], layer l's softmax weights averaged over the heads
 * (class token = last row / column).  Visualisation path, not used by sample(). */
int mb_gen_forward_attn(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop,
                        float* logits, float* attn, int nb, mb_stream stream);

/* ---- one sampling step after the forward: sampling.py:90-131 ------------------------------ *
 * logits_u NULL => no guidance.  `scale` = guidance_scale * a_i (sampling.py:91-98), `temperature`
 * the softmax temperature of this step.  exp_noise [B*n*m, C] is the Exp(1) draw of
 * torch.multinomial; conf_noise [B,n,m] is gumbel*randomize_temperature*(1-progress).
 * k_mask_len = floor(ratio * n*m) (masking.py:41-65, sampling.py:120-123); the clamp to
 * [1, num_masked(sample 0) - 1] happens on the device.  tokens_in / tokens_out [B,n,m] must not
 * alias; pred_out (may be NULL) receives the step's predicted tokens (l_full_tokens entry). */
int mb_sample_step(const float* logits_c, const float* logits_u, float scale, float temperature,
                   const float* exp_noise, const float* conf_noise, int k_mask_len,
                   const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out,
                   int B, int n, int m, int C, mb_stream stream);

/* ---- decoder: ConvVQModel.decode_tokens, modeling/conv_vqgan.py:98-112 --------------------- */
int mb_dec_create(const mb_dec_cfg* cfg, int max_batch, mb_dec** out);
void mb_dec_destroy(mb_dec* d);
int mb_dec_load(mb_dec* d, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream);
/* tokens int64 [B, n] (K-bit codes) -> img_nchw fp32 [B,3,H,W] unclamped (may be NULL) and/or
 * img_nhwc_u8 uint8 [B,H,W,3] = trunc(clamp(x,0,1)*255) (scripts/eval_maskbit.py:134-135; may be NULL). */
int mb_dec_decode(mb_dec* d, const int64_t* tokens, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream);
/* The decoder / encoder keep activations in fp16 (saturating stores).  Number of 4-channel output groups that were clamped at +-65504 since the last
 * reset, over all conv layers (0 for every configuration tested; a trained checkpoint that needs more range shows up here instead of being
 * clipped silently).  Synchronises `stream`. */
int mb_dec_saturation_count(mb_dec* d, unsigned* count, int reset, mb_stream stream);
/* ---- encoder half: ConvVQModel.encode, modeling/conv_vqgan.py:70-83 (ConvEncoder autoencoder.py:264-286 +
 * LookupFreeQuantizer sign/pack lookup_free.py:57-62,113-127).  img fp32 [B,C,H,W] -> indices int64 [B, h*w];
 * zq (+-1 latent, fp32 [B,K,h,w]) and zraw (pre-sign encoder output) may be NULL.  Needs build_encoder = 1. */
int mb_enc_encode(mb_dec* d, const float* img_nchw, int64_t* indices, float* zq, float* zraw, int B, mb_stream stream);

/* ---- lookup (VQ) tokenizer: ConvVQModel with quantizer_type "lookup" (SimpleVectorizer, modeling/quantizer/quantizer.py:10-119) ---------- *
 * A handle with a codebook of codebook_size (2 .. 65 536) entries of token_size (1 .. 256) channels; l2_normalize = use_l2_normalisation
 * (z and the codebook rows through F.normalize).  The codebook is the checkpoint entry quantize.embedding.weight [codebook_size, token_size],
 * loaded through mb_dec_load (which prepares the fp32 rows, normalised if required, and their squared norms); decoding or encoding before it is
 * loaded is an error.  On such a handle mb_dec_decode takes codebook indices (clamped to [0, codebook_size) on the device) and mb_enc_encode
 * behaves as mb_enc_encode_vq with row_dist = NULL. */
int mb_dec_create_vq(const mb_dec_cfg* cfg, int codebook_size, int l2_normalize, int max_batch, mb_dec** out);
/* ConvVQModel.decode (conv_vqgan.py:85-96) of any float latent z_nchw fp32 [B, token_size, h, w]; VQ handles only. */
int mb_dec_decode_latent(mb_dec* d, const float* z_nchw, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream);
/* ConvVQModel.encode with the lookup quantizer: img fp32 [B,C,H,W] -> indices int64 [B, h*w] (nearest entry, ties to the lowest index), and
 * optionally zq fp32 [B,K,h,w] (the selected rows), zraw fp32 [B,K,h,w] (encoder output before normalisation) and row_dist fp32 [B*h*w] =
 * sum_k (z_k - e_idx,k)^2 over the (possibly normalised) vectors. */
int mb_enc_encode_vq(mb_dec* d, const float* img_nchw, int64_t* indices, float* zq, float* zraw, float* row_dist, int B, mb_stream stream);

/* ---- whole loop: modeling.modules.sample, sampling.py:55-136 ------------------------------- *
 * Runs num_steps x (forward [+CFG], step) then combine (factorization.py:7-24) + decode.
 * exp_noise [steps, B*n*m, C] and conf_noise [steps, B, n, m] (= gumbel * randomize_temperature *
 * (1-progress)) are drawn by the caller with the reference's RNG protocol.  step_tokens int64
 * [steps,B,n,m] may be NULL.  tokens_out int64 [B,n] receives the combined K-bit codes (may be
 * NULL).  d may be NULL (then both image pointers must be NULL). */
int mb_sample(mb_gen* g, mb_dec* d, const mb_sample_plan* plan, const int64_t* labels, int B,
              const float* exp_noise, const float* conf_noise, int64_t* step_tokens, int64_t* tokens_out,
              float* img_nchw, uint8_t* img_nhwc_u8, mb_stream stream);

/* ---- image editing: sampling from a partly known token map (inpainting, outpainting, regenerating a region under another label) ------------ *
 * No counterpart in the reference, whose sample() always starts from the all-masked state (sampling.py:65-71).  Per sample b a run starts with
 * num_regen[b] masked slots (the reference's num_maskable, per sample) and each step re-masks per sample: with nm_b = sample b's masked count on
 * entry and mask_len = floor(mask_ratio * num_regen[b]) in fp32 (torch.floor(ratio * num_maskable) with a float32 ratio),
 *   nm_b >= 2: k = min(max(mask_len, 1), nm_b - 1), threshold = the k-th smallest confidence of the sample, every slot at or below it is masked again
 *              (always a masked slot's confidence: a known slot, at +inf, is never re-masked);
 *   nm_b <= 1: nothing is re-masked, tokens_out = pred (the reference's clamp gives k = 0 there, whose sorted[-1] = +inf would mask every token).
 * With every slot masked a run equals mb_sample bit for bit.  The plan of a run: mb_sample_plan with the float32 masking ratios of the steps
 * (get_masking_ratio(progress), masking.py:41-65) in the place of the mask lengths. */
typedef struct {
  int num_steps;
  int use_guidance;
  const float* scale;          /* [num_steps] as in mb_sample_plan */
  const float* temperature;    /* [num_steps] as in mb_sample_plan */
  const float* mask_ratio;     /* [num_steps] float32 masking ratio of the step */
  int step_begin, step_end;    /* step chunk of this call, as in mb_sample_plan; chunk 0 reads init_tokens */
} mb_edit_plan;
/* mb_sample_step with the per-sample rule above: num_regen int32 [B] (device) and the step's mask_ratio in the place of k_mask_len. */
int mb_sample_step_edit(const float* logits_c, const float* logits_u, float scale, float temperature,
                        const float* exp_noise, const float* conf_noise, float mask_ratio, const int32_t* num_regen,
                        const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out,
                        int B, int n, int m, int C, mb_stream stream);
/* mb_sample from the caller's token state: init_tokens int64 [B,n,m] with the value C at the slots to regenerate (values outside [0, C] are clamped
 * on the device); the first chunk copies them into the engine and counts num_regen per sample on the device.  Everything else -- zero-scale steps,
 * precision modes, step chunks and their checks, outputs -- as in mb_sample; a chunk of mb_sample does not continue a run mb_sample_edit began, nor
 * the other way round. */
int mb_sample_edit(mb_gen* g, mb_dec* d, const mb_edit_plan* plan, const int64_t* labels, int B, const int64_t* init_tokens,
                   const float* exp_noise, const float* conf_noise, int64_t* step_tokens, int64_t* tokens_out,
                   float* img_nchw, uint8_t* img_nhwc_u8, mb_stream stream);
/* Stateless helpers around such a run: the caller owns every buffer, nothing is allocated, nothing synchronises.
 * codes int64 [B,n] (what mb_enc_encode gives) + regen_mask uint8 [B,n,m] (non-zero = regenerate) -> tokens int64 [B,n,m] =
 * (code >> g * log2(C)) & (C - 1), or C where the mask is set; num_regen int32 [B] = the number of set slots per sample. */
int mb_edit_init(const int64_t* codes, const uint8_t* regen_mask, int64_t* tokens, int32_t* num_regen, int B, int n, int m, int C, mb_stream stream);
/* pixel_mask uint8 [B,H,W] -> token_mask uint8 [B,H/stride,W/stride]: 1 where any pixel of the stride x stride block is non-zero.  stride = the
 * tokenizer's 2^(num_resolutions - 1): a power of two dividing H and W; pixel_mask aligned to min(stride, 16) bytes. */
int mb_edit_token_mask(const uint8_t* pixel_mask, uint8_t* token_mask, int B, int H, int W, int stride, mb_stream stream);
/* x = pixel_mask ? gen : orig per pixel (fp32 [B,C,H,W], 16-byte aligned; pixel_mask uint8 [B,H,W], 4-byte aligned; C in 1 .. 4, W % 4 == 0), from
 * one read of each: out_nchw fp32 [B,C,H,W] = x (may be NULL; must not alias an input) and / or out_nhwc_u8 uint8 [B,H,W,C] = trunc(clamp(x,0,1)*255),
 * the conversion of mb_dec_decode (may be NULL). */
int mb_edit_composite(const float* gen_nchw, const float* orig_nchw, const uint8_t* pixel_mask, float* out_nchw, uint8_t* out_nhwc_u8,
                      int B, int C, int H, int W, mb_stream stream);

/* ---- per-sample seeded sampling: the step kernel generates its own noise ------------------------------------------------------------------- *
 * No counterpart in the reference, whose noise is drawn by torch outside the loop (sampling.py:107,113-117) and therefore depends on a sample's
 * position in the batch, the batch size and the generators' history.  Here every noise value is a pure function of (the sample's 64-bit seed, the
 * absolute step index of the run, the slot, the class): nothing is drawn, stored, chunked or copied, and a sample's tokens depend only on its seed,
 * its label and the sampling arguments -- not on the batch it runs in, its position there, the step chunks or the number of devices.
 *
 * THE NOISE DEFINITION (all integers unsigned 32-bit, all floating point IEEE binary32 with round-to-nearest, no fused multiply-add):
 *   generator  Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123): ten rounds of
 *                (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  M0 = 0xD2511F53, M1 = 0xCD9E8D57,
 *              hi / lo = the upper / lower 32 bits of the 64-bit product; between rounds k0 += 0x9E3779B9, k1 += 0xBB67AE85 (mod 2^32).
 *   key        (k0, k1) = (low dword, high dword) of the sample's seed (int64 on the device: the bit pattern of an unsigned 64-bit value).
 *   counter    slot = position * m + group within the sample (0 .. n m - 1), step = the absolute step index of the run (a step chunk does not
 *              change it), class c in 0 .. C - 1:
 *                categorical stream: (c0, c1, c2, c3) = (c >> 2, slot, step, 0); class c takes output word c & 3;
 *                confidence stream : (c0, c1, c2, c3) = (0, slot, step, 1); output word 0.
 *              Nothing batch-dependent enters: no row index, batch size or chunk offset.
 *   uniform    of an output word x: u = float((x >> 8) | 1) * 2^-24 -- exact in binary32, in [2^-24, 1 - 2^-24], never 0 or 1.
 *   categorical draw   q = -logf(u) takes the place of exp_noise[row, c] in argmax((p / psum) / q).  u has 2^23 levels: the race is biased by about
 *              1e-7 relative, far below what any test of the distribution resolves.
 *   confidence noise   g = -logf(-logf(u)); the value added to log p[pred] is (g * randomize_temperature) * w_i, two separately rounded products in
 *              the reference's order (sampling.py:117), w_i = float32(1 - (i + 1) / num_steps) evaluated on the host.
 *   logf is the accurate single-precision logarithm (at most 3 ulp, the OpenCL bound; in practice 1), as in the confidence itself.
 *
 * THE THRESHOLD RULE of a seeded step is the per-sample rule of the edit step above; a run that starts all-masked has num_regen[b] = n m.  The
 * reference's rule reads sample 0's masked count for the whole batch -- the one remaining coupling between the samples of a batch.  From an
 * all-masked state every sample has the same masked count as long as no confidence ties at the threshold, so the two rules can differ only on exact
 * confidence ties (a tie re-masks both slots, and that sample's count then differs from sample 0's).
 *
 * mb_sample_step_edit with generated noise: seeds int64 [B] (device), `step` >= 0, conf_weight = w_step.  pred_out may be NULL and must not alias a
 * token buffer. */
int mb_sample_step_seeded(const float* logits_c, const float* logits_u, float scale, float temperature, const int64_t* seeds, int step,
                          float randomize_temperature, float conf_weight, float mask_ratio, const int32_t* num_regen,
                          const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C, mb_stream stream);
/* mb_sample_edit with generated noise, one call for the whole run: init_tokens NULL = every slot masked (then num_regen[b] = n m); seeds int64 [B]
 * (device); conf_weight = HOST array [num_steps] of the w_i above, indexed by the absolute step like the plan's arrays.  Zero-scale steps, precision
 * modes, step chunks and their checks, outputs: as in mb_sample_edit (step_tokens holds the steps of this call's chunk); a chunk continues only a
 * run that a seeded call began. */
int mb_sample_seeded(mb_gen* g, mb_dec* d, const mb_edit_plan* plan, const int64_t* labels, int B, const int64_t* init_tokens, const int64_t* seeds,
                     float randomize_temperature, const float* conf_weight, int64_t* step_tokens, int64_t* tokens_out,
                     float* img_nchw, uint8_t* img_nhwc_u8, mb_stream stream);

/* ---- per-sample sampling arguments: mixed requests in one seeded batch ---------------------------------------------------------------------- *
 * A seeded run whose B samples ("requests") each bring their own num_steps N_b, guidance scale and annealing, temperatures and mask schedule, next
 * to their own seed, label and (optionally) start tokens.  The step kernels read their constants per sample from a device table instead of from
 * kernel arguments; the noise definition and the threshold rule are those of the seeded section above, unchanged.
 *
 * SEMANTICS
 *   - The run lasts S = max_b N_b global steps.  Request b is RIGHT-ALIGNED: it is inactive while t < S - N_b, and at global step t it executes its
 *     own local step i = t - (S - N_b).  All requests finish at t = S - 1; one combine and one decode serve the whole batch.
 *   - Noise counter (step), conf_weight, scale, temperature and mask ratio of request b at global step t are those of local step i of an N_b-step
 *     run.  Consequence: a request's tokens are exactly what it would produce alone.
 *   - The caller orders the requests by N_b descending, so the active set at step t is a prefix [0, active[t]) and active[] is non-decreasing, with
 *     active[S - 1] = B.  At step t the forward, the step kernels and the writes to step_tokens cover that prefix only: inactive samples are
 *     untouched.  Both token buffers of the engine are initialised with the start state (all masked, or init_tokens) at step 0, so an inactive
 *     sample needs no copy while the buffers ping-pong.  Cost: sum_b N_b sequence-forwards instead of B * S.
 *   - use_guidance is ONE flag for the run.  In a guided run EVERY step runs the guided forward, also where all active scales are 0: what a request
 *     sees must not depend on its neighbours' schedules, and at precision 4 the guided forward is not the plain forward bit for bit.  A request
 *     with scale 0 in a guided run gets c + 0 * (c - u).  So a request's result is a function of (its own fields, use_guidance) and nothing else.
 *     THIS DIFFERS from mb_sample_seeded, which runs the plain forward on zero-scale steps below precision 4: a requests run equals a seeded run
 *     of the same settings where both run the same forwards (no zero-scale step in a guided run, or no guidance at all).
 *   - Threshold rule: the per-sample rule of the edit and seeded steps.
 * One record per (global step, position in the batch); an inactive record has step = -1 and is never read. */
typedef struct {
  float scale;                   /* annealed guidance scale of the request's local step */
  float temperature;             /* softmax temperature of that step */
  float mask_ratio;              /* float32 masking ratio of that step */
  float randomize_temperature;
  float conf_weight;             /* float32(1 - (i + 1) / N_b) */
  int32_t step;                  /* local step i = the noise counter; -1: inactive */
} mb_request_step;
typedef struct {
  int num_steps;                 /* S */
  int use_guidance;
  const int* active;             /* HOST [S]: the active prefix per global step */
  const mb_request_step* table;  /* DEVICE [S, B] */
} mb_request_plan;
/* mb_sample_step_seeded with the constants of sample b read from table_row[b] (device [B]: one row of the table). */
int mb_sample_step_requests(const float* logits_c, const float* logits_u, const mb_request_step* table_row, const int64_t* seeds,
                            const int32_t* num_regen, const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out,
                            int B, int n, int m, int C, mb_stream stream);
/* The whole run, one call (no step chunks: there is no noise tensor to bound).  labels, seeds, init_tokens (may be NULL = every slot masked) in the
 * descending-N_b order of the plan.  step_tokens int64 [S, B, n, m] (may be NULL): only the active (t, b) are written.  tokens_out, images: as in
 * mb_sample.  The call ends any run in progress on the handle: a step chunk of another kind does not continue it.  Refused before any launch: null
 * arguments; active[] not non-decreasing or outside [1, B]; active[S - 1] != B; an image without a decoder; 2 B (guided) or B sequences beyond the
 * engine's. */
int mb_sample_requests(mb_gen* g, mb_dec* d, const mb_request_plan* plan, const int64_t* labels, int B, const int64_t* init_tokens,
                       const int64_t* seeds, int64_t* step_tokens, int64_t* tokens_out, float* img_nchw, uint8_t* img_nhwc_u8, mb_stream stream);

/* ---- sampling session: requests join and leave a running batch ------------------------------------------------------------------------------------ *
 * A requests run (above) is closed: planned for a fixed set, right-aligned, the handle busy for max N_b steps.  A SESSION is the open form: a batch of
 * at most max_active rows that requests enter (mb_session_admit) and leave (when their own N steps are done) while it runs, one step per
 * mb_session_tick.  Additions only, MB_ABI_VERSION unchanged.
 *
 * STATE  A session is created for one generator configuration (seq, splits and bits of mb_gen_cfg: n = seq positions of m = splits groups of
 * C = 2^(bits / splits) codes; every tick takes a generator handle of that configuration) with a capacity max_active, a max_steps and ONE
 * use_guidance flag, which follows the mb_sample_requests rule: in a guided session every tick runs the guided forward, and a zero scale gets
 * c + 0 * (c - u).  It owns, on the device, both token buffers and a prediction buffer [max_active, n, m]; per row its label, seed, num_regen,
 * schedule slot, local step and N; a schedule pool of mb_request_step records [max_active, max_steps]; the step's table row, a codes buffer and the
 * plan snapshot -- allocated by the first admit that passes its checks (mb_session_create itself touches no device).  The active requests are the
 * dense row prefix [0, A).
 *
 * ADMIT appends K requests at rows [A, A + K): labels, seeds (device int64 [K]), num_steps (HOST int [K], 1 <= N <= max_steps) and the schedule --
 * request k's N_k records, local step i of an N_k-step run (table[i][0] of build_request_plan([r]): step = i), packed one request after the other in
 * one device array of sum_k N_k records.  init_tokens (device int64 [K, n, m], or NULL = every slot masked) go into the buffer the next tick reads,
 * clamped to [0, C], and num_regen is counted on the device, both as mb_sample_edit does.  tickets (HOST uint64 [K]) receives one ticket per request:
 * they count from 0 in admission order.  A + K > max_active is refused without any launch.
 *
 * TICK runs one step for the rows [0, A), in this order:
 *   1. row table   row[r] = pool[slot[r]][local_step[r]], then local_step[r] += 1 -- a kernel; nothing is uploaded per tick.
 *   2. forward and step over A rows, exactly one global step of mb_sample_requests.  The predictions go to pred_out ([A, n, m]) or, NULL, to the
 *      session's own buffer.
 *   3. retire and compact   F = {r : local_step[r] == N[r]}, k = |F|, A' = A - k.  The predictions of the rows of F are combined
 *      (combine_factorized_tokens) into codes [k, n] IN ASCENDING ROW ORDER (codes_out, or NULL: the session's buffer).  The holes H = F below A' and
 *      the movers M = the unfinished rows at or above A', both ascending, have the same length, and row M[j] moves to H[j]: its tokens in the buffer
 *      the next tick reads, and label, seed, num_regen, slot, local step and N.  Sources lie at or above A', destinations below: the moves are
 *      disjoint and run in parallel in place.  F, H and M are taken ONCE, by a plan kernel into a snapshot; the move kernel acts on the snapshot
 *      alone (it overwrites local_step[dst], from which F was derived).
 *   4. decode   with a decoder the k codes are decoded by mb_dec_decode into img_nchw / img_nhwc_u8 ([k, ...], each may be NULL).
 * The session keeps a host mirror of (ticket, local step, N) per row and applies the same rule to it, so a tick reports without reading the device:
 * *num_finished = k, finished (HOST uint64 [>= mb_session_due()]) = the tickets of the finished requests in output order, ran (HOST uint64 [A], may
 * be NULL) = the ticket of every row that ran this tick, row by row -- what pred_out's rows belong to.  mb_session_due: how many requests the NEXT
 * tick finishes (size the image buffers by it); mb_session_active: A.  A tick with A = 0 does nothing.  Every tick and every admit is enqueue-only:
 * no synchronisation, no host read, and no host-to-device copy.
 *
 * CONSEQUENCES
 *   - A request admitted before tick t runs its local step i at tick t + i and finishes at tick t + N - 1.
 *   - Its tokens, codes and image are bit for bit what mb_sample_requests gives for it alone under the same use_guidance -- whatever else is in the
 *     session and however its row has moved: noise is a function of (seed, local step, slot, class), the threshold rule is per sample, the step
 *     kernels read their constants per sample, the forwards and the decoder do not depend on the batch.
 *   - The guided forward's [labels | labels] / [0 | 1] cache of the handle is keyed by the label pointer, and the session's label buffer keeps its
 *     address while its contents move: the session invalidates the cache whenever membership changed (an admit, a tick that retired a request).
 *   - A tick ends any chunked run in progress on the handle, as mb_sample_requests does.
 *   - The session owns its token state: other calls on the same handle (mb_sample, mb_sample_seeded, ...) may run between two ticks without changing
 *     the session's results, and the handle may be replaced by another of the same configuration.
 * Refused before any launch, the checks that need no handle first: null arguments; max_active, max_steps or K below 1; an N outside [1, max_steps];
 * A + K > max_active; an image without a decoder; a handle of another configuration, or one that holds fewer than 2 A (guided) or A sequences. */
typedef struct mb_session mb_session;
int mb_session_create(int seq, int splits, int bits, int max_active, int max_steps, int use_guidance, mb_session** out);
void mb_session_destroy(mb_session* s);
int mb_session_admit(mb_session* s, int K, const int64_t* labels, const int64_t* seeds, const int* num_steps, const mb_request_step* schedule,
                     const int64_t* init_tokens, uint64_t* tickets, mb_stream stream);
int mb_session_due(const mb_session* s);      /* requests the next tick finishes; -1: null */
int mb_session_active(const mb_session* s);   /* A; -1: null */
int mb_session_tick(mb_session* s, mb_gen* g, mb_dec* d, int64_t* pred_out, int64_t* codes_out, float* img_nchw, uint8_t* img_nhwc_u8,
                    uint64_t* finished, uint64_t* ran, int* num_finished, mb_stream stream);

/* ---- tokenizer evaluation: TokenizerEvaluator.update, evaluator/evaluator.py:262-375 (scripts/eval_tokenizer.py:137-149) ---------------- *
 * Stateless: the caller owns every buffer (and zeroes its running state once); nothing is allocated, nothing synchronises.
 * Bytes of workspace mb_eval_images needs for this shape (one slot of three doubles per 32 x 32 tile of every image plane); 0 for a shape it
 * does not take. */
size_t mb_eval_workspace_bytes(int B, int C, int H, int W);
/* MAE, MSE, PSNR and SSIM of fake against real (fp32 [B,C,H,W], H, W >= 6) from one read of both: replaces the difference / power / mean chains of
 * evaluator.py:282-294 and the clone / reflect-pad / product / cat / depthwise 11 x 11 Gaussian conv2d / SSIM formula chain of evaluator.py:296-334
 * (window gaussian(11, 1.5) of evaluator.py:44-56, k1 / k2 = 0.01 / 0.03, data range 1).  metrics: bit 0 = absolute error, bit 1 = squared error
 * and PSNR, bit 2 = SSIM (needs C == 3, evaluator.py:298).  clamp01 != 0 clamps both inputs to [0, 1] on the load (eval_tokenizer.py:146-147).
 * per_image double [B][3] receives sum |d|, sum d^2, sum SSIM over each image's C*H*W values (0 for a metric not asked for); sums double [4] +=
 * the batch's per-image MAE, MSE, PSNR = 10 log10(1 / (mse + 1e-10)) and mean-SSIM terms, added in image order (what evaluator.py:284,288,292,334
 * add to the four running sums), deterministic: one update of a batch and consecutive updates of its parts leave identical bits. */
int mb_eval_images(const float* real, const float* fake, int B, int C, int H, int W, unsigned metrics, int clamp01, void* workspace,
                   double* per_image, double* sums, mb_stream stream);
/* hist[i] += number of indices equal to i, over n int64 indices of any shape: replaces both torch.unique calls, the .tolist() into a Python set
 * (a host synchronisation per batch) and the index_add_ of evaluator.py:370-375.  Indices outside [0, K) are not counted; *out_of_range += their
 * number. */
int mb_eval_codebook(const int64_t* indices, int64_t n, int K, int64_t* hist, unsigned* out_of_range, mb_stream stream);

/* ---- masked-token validation: the forward half of the training step, scripts/train_maskbit.py:372-381 ------------------------------------ *
 * Stateless like the tokenizer evaluation above: caller-owned buffers, no allocation, no synchronisation.
 * get_mask_tokens (modeling/modules/masking.py:34-37) after its draws: mask uint8 [B,n,m] = uniforms < val_to_mask[b] (fp32 compare; uniforms fp32
 * [B,n,m] and val_to_mask fp32 [B] are the caller's draws and schedule values, masking.py:22-30,35) and masked_tokens int64 [B,n,m] = mask ?
 * mask_token : tokens, in place of the clone / boolean-index / full_like / index_put chain.  tokens is not modified and must not alias
 * masked_tokens. */
int mb_mlm_mask(const int64_t* tokens, const float* uniforms, const float* val_to_mask, int64_t mask_token, int64_t* masked_tokens, uint8_t* mask,
                int B, int n, int m, mb_stream stream);
/* Bytes of workspace mb_mlm_loss needs for this shape (one 48-byte slot per workgroup and per sample); 0 for a shape it does not take. */
size_t mb_mlm_workspace_bytes(int B, int n, int m, int C);
/* Bytes of the pooled state of mb_mlm_loss: 37 words of 8 bytes, zeroed once by the caller --
 *   [0] double sum of the loss over all rows, [1] double sum over the masked rows,
 *   [2..5] int64 rows, masked rows, correct rows, correct masked rows,
 *   [6 + 3 k .. 8 + 3 k], k = 0..9: double masked-loss sum, int64 masked correct, int64 masked rows of the samples whose realised mask fraction
 *   falls in decile k = min(9, 10 * masked / (n * m)) (integer division),
 *   [36] int64 targets outside [0, C). */
size_t mb_mlm_state_bytes(void);
/* MLMLoss.forward (modeling/modules/losses.py:319-326) from one read of logits fp32 [B,n,m,C] (contiguous, any C >= 2): per row the label-smoothed
 * cross entropy of torch.nn.CrossEntropyLoss(label_smoothing) against targets int64 [B,n,m] and whether the first index of the row's maximum
 * (torch.argmax) equals the target, summed over all rows and over the rows with mask uint8 [B,n,m] != 0 -- in place of the reshape / log-softmax /
 * gather / smoothing mean / argmax chain, its boolean-index copy inputs[masks] (a host synchronisation) and the same chain on the copy.
 * sample_sums double [B][2] = sum of the row losses over all / over the masked rows of each sample; sample_counts int64 [B][3] = correct rows,
 * correct masked rows, masked rows (either may be NULL).  state (may be NULL) += the samples in sample order: deterministic, no floating-point
 * atomics; a sample's figures do not depend on B, and consecutive calls on the parts of a batch leave the bits of one call on the whole.  A row
 * whose target lies outside [0, C) enters no figure and is counted in the state's last word; memory is never indexed by a target. */
int mb_mlm_loss(const float* logits, const int64_t* targets, const uint8_t* mask, float label_smoothing, int B, int n, int m, int C,
                void* workspace, double* sample_sums, int64_t* sample_counts, void* state, mb_stream stream);

/* ---- LPIPS: modeling/modules/lpips.py (the metric of evaluator/evaluator.py:336-341) ------------------------------------------------------- *
 * A handle owns the VGG16 `features` weights (fp16, repacked for the MFMA convolutions of the tokenizer), the five 1x1 weight vectors and a
 * workspace for max_pairs image pairs of up to max_h x max_w pixels (two fp16 buffers of 2 max_pairs max_h max_w 64 values).  max_h % 128 == 0,
 * max_w % 256 == 0: the convolution tiles are 8 x 16 pixels and the deepest level runs at 1/16 resolution. */
int mb_lpips_create(int max_pairs, int max_h, int max_w, mb_lpips** out);
void mb_lpips_destroy(mb_lpips* h);
/* One entry of the reference's LPIPS state dict (fp32, device): scaling_layer.shift / .scale, net.slice{1..5}.{0,2,5,7,10,12,14,17,19,21,24,26,28}.weight
 * / .bias (torchvision's VGG16-D `features` indices inside the reference's five slices), lin{0..4}.model.1.weight (model.0 without dropout).  All 33
 * must be given before a forward. */
int mb_lpips_load(mb_lpips* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream);
/* LPIPS.forward (lpips.py:39-52) of B pairs real / fake fp32 [B,3,H,W] in [0, 1] (clamp01 != 0: clamped to it on the load, eval_tokenizer.py:146-147):
 * scaling layer, thirteen 3x3 convolutions + bias + ReLU and four max-pools on both images in one batch of 2B, and per tap one read of the two
 * feature maps for sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 and its spatial mean.  per_image double [B] = the value of each pair;
 * *sum (may be NULL) += those values in image order: deterministic, no floating-point atomics, a pair's value does not depend on B.  Features are
 * stored as fp16 (DESIGN.md "Precision").  1 <= B <= max_pairs, H % 128 == 0, W % 256 == 0, H W <= max_h max_w; anything else is refused before
 * any device work.  No allocation, no synchronisation. */
int mb_lpips_forward(mb_lpips* h, const float* real, const float* fake, int B, int H, int W, int clamp01, double* per_image, double* sum, mb_stream stream);
/* 4-channel activation groups of this handle's convolutions clamped at +-65504 since the last reset.  Synchronises `stream`. */
int mb_lpips_saturation_count(mb_lpips* h, unsigned* count, int reset, mb_stream stream);

/* ---- FID / Inception Score statistics: GeneratorEvaluator.update, evaluator/evaluator.py:549-569 (rFID: :336-364) --------------------------- *
 * Stateless like the tokenizer evaluation above: caller-owned buffers (zeroed once by the caller), no allocation, no synchronisation.  dtype of the
 * input rows: 0 = fp32 (widened exactly), 1 = fp64; row_stride in elements, >= the row length.  A shape outside B, D (C) in [1, 2^20] is refused.
 * total double [D] += sum_n f_n and sigma double [D,D] += F^T F for feats [B, D]: the per-image `total += f; sigma += torch.outer(f, f)` loop of
 * evaluator.py:567-569 as one fp64 MFMA rank-B update.  Every element chains the batch's rows in increasing order onto its loaded value and is
 * written by one wave (no floating-point atomics): bitwise reproducible, and consecutive calls on the parts of a batch split at a multiple of 4 rows
 * leave the bits of one call on the whole.  ONLY the 64 x 64 blocks of sigma on and above the diagonal are updated (elements [i][j] with
 * i / 64 <= j / 64); the blocks below it are never read or written -- mirror the upper triangle before reading the matrix. */
int mb_fid_accumulate(const void* feats, int dtype, int B, int D, int64_t row_stride, double* total, double* sigma, mb_stream stream);
/* Bytes of workspace mb_is_accumulate needs (two doubles per row); 0 for a shape it does not take. */
size_t mb_is_workspace_bytes(int B, int C);
/* p = softmax(logits [B, C]) in fp64 with the row maximum subtracted; prob_total double [C] += sum_n p and kl_total double [C] += sum_n p log(p + 1e-16)
 * (evaluator.py:553-564), each column summed over the batch in a fixed order: deterministic. */
int mb_is_accumulate(const void* logits, int dtype, int B, int C, int64_t row_stride, double* prob_total, double* kl_total, void* workspace,
                     mb_stream stream);

/* ---- precision / recall: the k-NN manifolds of Kynkaanniemi et al. as ADM's evaluator computes them (manifold_radii / evaluate_pr) ----------- *
 * Stateless: caller-owned buffers, no allocation, no synchronisation.  dtype and row_stride as above (0 = fp32 widened exactly, 1 = fp64; elements).
 * For rows a, b of width D:   d2(a, b) = max(0, |a|^2 + |b|^2 - 2 a.b),   the three sums in fp64 (a.b on v_mfma_f64_16x16x4_f64), each in a fixed
 * order over d that does not depend on where the row sits in its matrix, on N or on the launch geometry (csrc/manifold.hip states the orders), the
 * combination as fma(-2, a.b, |a|^2 + |b|^2).  So a pair's value is a function of the two rows alone: results are bitwise reproducible, a row
 * permutation of X permutes radii2 bit for bit, and mb_manifold_cover over any split of the queries leaves the bytes of one call.  The N x N
 * matrix is never stored; no floating-point atomics.
 * Bytes of workspace for N rows in all (mb_knn_radii: N; mb_manifold_cover: Nq + Nb) -- 145 doubles per row: its |a|^2, and for each of up to 16
 * parts the column walk is cut into a list of 9 values (or a flag); 0 for a shape the entries do not take (N outside [1, 2^24], D outside
 * [1, 2^20]). */
size_t mb_manifold_workspace_bytes(int N, int D);
/* radii2 double [N]: radii2[i] = the (k+1)-th smallest of { d2(x_i, x_j) : j = 0..N-1 } counted with multiplicity, d2(x_i, x_i) taken as exactly 0
 * -- the squared distance to the k-th nearest neighbour other than the row itself (ADM's manifold_radii).  X [N, D]; 1 <= k <= 8, k + 1 <= N. */
int mb_knn_radii(const void* x, int dtype, int N, int D, int64_t row_stride, int k, double* radii2, void* workspace, mb_stream stream);
/* inside uint8 [Nq]: 1 iff some j has d2(q, b_j) <= radii2[j] (`<=` as in ADM's evaluate_pr), else 0.  Q [Nq, D] and B [Nb, D] may differ in dtype
 * and stride; radii2 double [Nb] belongs to B. */
int mb_manifold_cover(const void* q, int q_dtype, int Nq, int64_t q_stride, const void* b, int b_dtype, int Nb, int64_t b_stride, int D,
                      const double* radii2, uint8_t* inside, void* workspace, mb_stream stream);

/* ---- FID Inception-v3 (the network behind the reference's metrics.inception.get_inception_model(): pytorch-fid's pt_inception-2015-12-05) ------ *
 * fp16 NHWC activations, one general implicit-GEMM convolution on MFMA with a BatchNorm (eval) + ReLU epilogue (csrc/inception.hip); the graph
 * is the one written out in DESIGN.md "Inception-v3".  The handle holds the packed weights and the activation buffers for max_images images. */
typedef struct mb_inception mb_inception;
int mb_inception_create(int max_images, mb_inception** out);
void mb_inception_destroy(mb_inception* h);
/* One state-dict entry (device fp32): `<layer>.conv.weight` [Cout, Cin, kh, kw], `<layer>.bn.{weight,bias,running_mean,running_var}` [Cout] for the
 * 94 BasicConv2d layers, `fc.weight` [1008, 2048], `fc.bias` [1008]; `<layer>.bn.num_batches_tracked` is accepted and ignored.  -2: unknown name,
 * -4: wrong size. */
int mb_inception_load(mb_inception* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream);
/* u8 uint8 [B, 3, H, W] (H, W >= 2, B <= max_images) -> pool fp32 [B, 2048], logits_unbiased fp32 [B, 1008] = pool @ fc.weight^T, logits = that +
 * fc.bias; a NULL output is skipped.  A row does not depend on B or on the other images (no floating-point atomics).  No synchronisation.
 * Fails (-1) before any launch when the checkpoint is incomplete or the geometry is not taken. */
int mb_inception_forward(mb_inception* h, const uint8_t* u8, int B, int H, int W, float* pool, float* logits_unbiased, float* logits, mb_stream stream);
/* mb_inception_forward plus the spatial tap of sFID: spatial fp32 [B, 2023] (may be NULL) = the first 7 channels of Mixed_6d.branch1x1 after
 * BatchNorm and ReLU on the 17 x 17 map, flattened in (h, w, c) order as ADM's evaluator reshapes `mixed_6/conv:0`[..., :7] of the NHWC tensor
 * (Mixed_6d is the 2015 graph's mixed_6, its first conv the 1 x 1 branch).  Whether that graph tensor is the post-ReLU one could not be checked
 * against TensorFlow; sFID values are therefore NOT claimed to match published ones (DESIGN.md "sFID").  The other outputs keep their bits. */
int mb_inception_forward_spatial(mb_inception* h, const uint8_t* u8, int B, int H, int W, float* spatial, float* pool, float* logits_unbiased,
                                 float* logits, mb_stream stream);
/* 4-channel output groups the convolutions clamped at the fp16 range since the last reset.  Synchronises the stream. */
int mb_inception_saturation_count(mb_inception* h, unsigned* count, int reset, mb_stream stream);

/* ---- ResNet-50 perceptual loss: modeling/modules/perceptual_loss.py PerceptualLoss("resnet50") ------------------------------------------------- *
 * torchvision's resnet50 (v1.5) as written out in DESIGN.md "ResNet-50", inference only, on the convolution of the Inception network with a linear
 * and a residual epilogue (csrc/resnet.hip).  The handle holds the packed weights and the activation buffers for max_pairs pairs (10.7 MiB of fp16
 * per image).  Additions, MB_ABI_VERSION unchanged. */
typedef struct mb_resnet mb_resnet;
int mb_resnet_create(int max_pairs, mb_resnet** out);
void mb_resnet_destroy(mb_resnet* h);
/* One state-dict entry (device fp32) of the reference module: `mean`, `std` (3 values each) and `model.` + torchvision's resnet50 keys (the prefix
 * may be missing): `conv1.weight` [64, 3, 7, 7], `bn1.*`, `layerL.B.conv{1,2,3}.weight`, `layerL.B.bn{1,2,3}.{weight,bias,running_mean,running_var}`,
 * `layerL.0.downsample.0.weight`, `layerL.0.downsample.1.*`, `fc.weight` [1000, 2048], `fc.bias`; `*.num_batches_tracked` is accepted and ignored.
 * -2: unknown name, -4: wrong size. */
int mb_resnet_load(mb_resnet* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream);
/* PerceptualLoss.forward of B pairs real / fake fp32 [B, 3, H, W] (32 <= H, W <= 1024; clamp01 != 0: clamped to [0, 1] on the load): both resized to
 * 224 x 224 (bilinear, antialiased, half-pixel centres), (x - mean) / std, one batch of 2B images through the network.  per_pair double [B] = the
 * mean over the 1000 logits of (a - b)^2; on_logits == 0: plus the mean over the 2048 x 7 x 7 layer4 map of the same.  sum (double, may be NULL)
 * += per_pair[0 .. B) in pair order.  Fixed summation order, no floating-point atomics: a pair's value does not depend on B or on the other pairs.
 * No synchronisation.  Fails (-1) before any launch when the checkpoint is incomplete ("not complete") or the geometry is not taken. */
int mb_resnet_forward(mb_resnet* h, const float* real, const float* fake, int B, int H, int W, int clamp01, int on_logits, double* per_pair, double* sum,
                      mb_stream stream);
/* 4-channel output groups the convolutions clamped at the fp16 range since the last reset.  Synchronises the stream. */
int mb_resnet_saturation_count(mb_resnet* h, unsigned* count, int reset, mb_stream stream);

/* ---- VQGAN+ discriminator: modeling/modules/discriminator.py NLayerDiscriminatorv2 -------------------------------------------------------------- *
 * The graph of DESIGN.md "Discriminator", inference only (csrc/discriminator.hip): block_in (5 x 5 + LeakyReLU 0.1), `stages` stages of 3 x 3
 * convolution, downsample (blur_kernel 3, 4, 5: BlurBlock; 0: AvgPool2d(2)), GroupNorm(32, eps 1e-5) and LeakyReLU, AdaptiveMaxPool2d(16), to_logits.
 * hidden a multiple of 32; 1 .. 4 stages; at most 2048 channels in the last stage.  fp16 NHWC activations, fp32 accumulation.  The workspace holds
 * max_images images of 256 x 256 (at least one of 512 x 512): a batch is walked in chunks of as many images as fit, 4 max_images at the most.
 * Additions, MB_ABI_VERSION unchanged. */
typedef struct mb_disc mb_disc;
int mb_disc_create(int max_images, int hidden, int stages, int blur_kernel, mb_disc** out);
void mb_disc_destroy(mb_disc* h);
/* One state-dict entry (device fp32) of the reference module: `block_in.0.{weight,bias}` [hidden, 3, 5, 5], `blocks.I.0.{weight,bias}`,
 * `blocks.I.2.{weight,bias}` (GroupNorm), `to_logits.0.{weight,bias}`, `to_logits.2.{weight,bias}` [1, c, 5, 5]; with a blur, `blocks.I.1.kernel`
 * [1, 1, k, k] must EQUAL the binomial kernel the handle computes itself (that entry synchronises the stream).  -2: unknown name, -4: wrong
 * size, or a blur kernel that is not the binomial one. */
int mb_disc_load(mb_disc* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream);
/* images fp32 [B, 3, H, W], H and W multiples of 16 in [32, 512] (clamp01 != 0: clamped to [0, 1] on the load).  Each output may be NULL:
 * logits fp32 [B, 256] (the 16 x 16 map, row-major); stats double [B, 5] = per image the sums over its 256 logits l of l, relu(1 - l), relu(1 + l),
 * softplus(-l), softplus(l) (softplus as max(x, 0) + log1p(exp(-|x|)) in double); sum double [5] += those sums in image order.  Fixed summation
 * order, no floating-point atomics: an image's logits and sums do not depend on B, on the chunking or on its place in the batch, bit for bit.
 * No synchronisation.  Fails (-1) before any launch when the checkpoint is incomplete ("not complete") or the geometry is not taken. */
int mb_disc_forward(mb_disc* h, const float* images, int B, int H, int W, int clamp01, float* logits, double* stats, double* sum, mb_stream stream);
/* output groups (4 channels of a convolution, 8 of a GroupNorm) clamped at the fp16 range since the last reset.  Synchronises the stream. */
int mb_disc_saturation_count(mb_disc* h, unsigned* count, int reset, mb_stream stream);

/* ---- Taming VQGAN tokenizer: OriginalVQModel, modeling/taming_vqgan.py:19-69 (Encoder / Decoder of modeling/taming/taming_autoencoder.py) ---- *
 * The fixed network of that class: ch 128, ch_mult (1,1,2,2,4), 2 (decoder: 3) res blocks per level, seven single-head AttnBlocks of 512 channels at
 * the 16-pixel level, quant_conv / post_quant_conv, SimpleVectorizer(1024, 256) without normalisation.  fp16 NHWC activations on the convolution
 * launchers of the other tokenizers (every conv with bias; GroupNorm without SiLU in front of q / k / v), the attention in csrc/spatial_attention.hip,
 * the nearest-codeword search of the lookup tokenizer.  latent_size 16 or 32 = 256 x 256 or 512 x 512 images; additions, MB_ABI_VERSION unchanged. */
typedef struct mb_taming mb_taming;
int mb_taming_create(int max_batch, int latent_size, mb_taming** out);
void mb_taming_destroy(mb_taming* h);
/* One state-dict entry of the reference model (device fp32), by its own key: the 343 entries `encoder.*`, `decoder.*`, `quant_conv.*`,
 * `post_quant_conv.*`, `quantize.embedding.weight`.  q / k / v of an AttnBlock are stacked into one projection; decoder.conv_out takes decode's
 * (y + 1) / 2 (weight x 0.5, bias (b + 1) / 2).  -2: unknown name, -4: wrong size. */
int mb_taming_load(mb_taming* h, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream);
/* OriginalVQModel.encode: img fp32 [B,3,H,W] in [0,1] (scaled x * 2 - 1 on the way in) -> indices int64 [B, h*w] (nearest entry, ties to the lowest
 * index) and optionally zq fp32 [B,256,h,w] (the selected rows), zraw fp32 [B,256,h,w] (the output of quant_conv) and row_dist fp32 [B*h*w] =
 * sum_k (z_k - e_idx,k)^2. */
int mb_taming_encode(mb_taming* h, const float* img_nchw, int64_t* indices, float* zq, float* zraw, float* row_dist, int B, mb_stream stream);
/* OriginalVQModel.decode_tokens: tokens int64 [B, h*w] (clamped to [0, 1024) on the device) -> img_nchw fp32 [B,3,H,W] unclamped and / or
 * img_nhwc_u8 uint8 [B,H,W,3] = trunc(clamp(x,0,1)*255); at least one of the two. */
int mb_taming_decode(mb_taming* h, const int64_t* tokens, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream);
/* OriginalVQModel.decode of any float latent z_nchw fp32 [B,256,h,w]. */
int mb_taming_decode_latent(mb_taming* h, const float* z_nchw, float* img_nchw, uint8_t* img_nhwc_u8, int B, mb_stream stream);
/* 4-channel activation groups (conv outputs incl. q / k / v, attention outputs, latent packs) clamped at the fp16 range since the last reset.
 * Synchronises `stream`; nothing else of this handle does. */
int mb_taming_saturation_count(mb_taming* h, unsigned* count, int reset, mb_stream stream);

/* ---- image transform: the data loader's eval_transform (data/webdataset_reader.py:79-85: torchvision Resize -> CenterCrop -> ToTensor on a PIL
 * image) and guided-diffusion's center_crop_arr (the ADM reference batches), bit for bit what Pillow computes (csrc/image.hip) ------------------- *
 * Stateless: caller-owned buffers, no allocation, no synchronisation; additions, MB_ABI_VERSION unchanged.  One call is one PASS over B jobs:
 * Pillow's antialiased resize (ImagingResample, 8 bits per channel) of each job's whole source to res_h x res_w with one filter -- 0 BOX,
 * 1 BILINEAR, 2 BICUBIC (a = -0.5) --, horizontal pass first into a uint8 intermediate, then vertical, an axis whose size does not change skipped;
 * of the result only the window [win_y, win_y + win_h) x [win_x, win_x + win_w) is computed and written (the crop; every output depends on its own
 * taps alone, so this changes no bit).  The recipes ("reference": one pass; "adm": BOX halvings, each a pass with the window equal to the image,
 * then a BICUBIC pass) are host arithmetic on sizes: maskbit_amd.ImageTransform.plan.
 * A job (72 bytes; the host array and its device copy hold the same records):
 *   src_offset   bytes from `src` to the source's pixel (0, 0); packed RGB, 3 bytes per pixel, rows src_stride bytes apart (any alignment)
 *   dst_offset   PIXELS from the output bases to the job's first output: uint8 HWC [win_h, win_w, 3] at out_u8 + 3 dst_offset, float32 planes
 *                [3, win_h, win_w] = byte / 255 (IEEE float32 division, what ToTensor() gives) at out_f32 + 3 dst_offset
 *   work_offset, kx, ky   the job's slot in the workspace and the taps per output of its two coefficient tables: FILLED IN by
 *                mb_image_workspace_bytes, which is therefore called on the host array before it is copied to the device
 *   src_h, src_w, src_stride, res_h, res_w, win_y, win_x, win_h, win_w   as above; sides in [1, 16384], src_stride in [3 src_w, 2^20] */
typedef struct {
  int64_t src_offset, dst_offset, work_offset;
  int32_t src_h, src_w, src_stride;
  int32_t res_h, res_w;
  int32_t win_y, win_x, win_h, win_w;
  int32_t kx, ky;
  int32_t reserved;
} mb_image_job;
/* Lays the B jobs of one pass out in a workspace (fills work_offset, kx, ky of every job; HOST array) and returns its size in bytes -- per job the
 * two int32 coefficient tables and src_h rows of the intermediate; 0 for a job or a filter the pass does not take. */
size_t mb_image_workspace_bytes(mb_image_job* jobs, int B, int filter);
/* One pass: coefficients, horizontal, vertical + crop + formats, three launches over the whole ragged batch.  jobs_host: the laid-out records (read
 * before returning, for the checks and the grid sizes); jobs_dev: their copy in device memory (8-byte aligned; the upload is the caller's, on this
 * stream).  src .. src + src_bytes: the device buffer the sources lie in.  out_u8 / out_f32: either may be NULL, not both; out_pixels = pixels
 * either holds (a job writes [dst_offset, dst_offset + win_h win_w)).  workspace: 16-byte aligned, workspace_bytes of it.
 * Refused before any launch (-1, message prefixed "mb_image_resample:"): a NULL pointer among jobs, source and workspace; a filter outside 0 .. 2;
 * a source side outside [1, 16384]; a window (the resolution R) below 1 or outside the resized image; a job that reads beyond src_bytes, writes
 * beyond out_pixels, or does not carry the layout of mb_image_workspace_bytes; a workspace too small; B outside [1, 4096]. */
int mb_image_resample(const mb_image_job* jobs_host, const mb_image_job* jobs_dev, int B, int filter, const uint8_t* src, size_t src_bytes,
                      uint8_t* out_u8, float* out_f32, int64_t out_pixels, void* workspace, size_t workspace_bytes, mb_stream stream);

/* ---- measurement hooks used by bench.py (not part of the reference surface) ----------------- */
int mb_prof_enable(int on); /* 0 off; n >= 1: HIP-event timing of every kernel of every n-th generator forward (forwards n/2, n/2 + n, ..) and of all other calls */
int mb_prof_read(char* buf, int buflen); /* host buffer; writes "name calls total_ms\n" lines */
/* fp16 activation stores of the trunk saturate at +-65504 instead of producing infinities.  Number of QKV / FFN-up / attention / LayerNorm output
 * groups of this handle's forwards that were clamped since the last reset (0 for every configuration tested, synthetic heavy-tailed weights
 * included; a checkpoint that needs more range shows up here instead of being clipped silently).  Synchronises `stream`. */
int mb_gen_saturation_count(mb_gen* g, unsigned* count, int reset, mb_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MASKBIT_HIP_H */
