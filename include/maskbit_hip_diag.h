/* libmaskbit_hip.so -- DIAGNOSTIC entry points: single kernels of the engine on caller buffers, for the unit tests (tests/test_hip_gemm.py,
 * test_hip_pair.py, test_hip_conv.py; the row kernels -- mb_layernorm, mb_layernorm_f4_seq, mb_layernorm_pair, mb_pairify, mb_embed_ln, mb_embed_pair --
 * in test_hip_rows.py; the quantizer kernels in test_hip_quantizer.py; the tokenizers' blocks in test_hip_taming_blocks.py; the feature networks' tail in test_hip_convnet_tail.py) and the tools under tools/.  Nothing here is part of the reference's
 * surface and no host binding of the product needs it: include/maskbit_hip.h is the ABI.  Same conventions (device pointers, stream-ordered,
 * 0 / negative return, mb_last_error()).
 */
#ifndef MASKBIT_HIP_DIAG_H
#define MASKBIT_HIP_DIAG_H

#include "maskbit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One GEMM of the trunk family, out[M,N] = A[M,K] . W[N,K]^T + bias with epilogue `epi` (0 fp16 out, 1 gelu->fp16, 2 +residual->fp32, 3 gelu->fp32,
 * 4 logits fp32 with every `period`-th row dropped); A, W, out_h16 are fp16 device buffers.  variant: 0 auto, -1 the 128x128 kernel, 6 / 8 the
 * half-tile kernel with 192 / 256-row tiles, 257 its sequence-aligned tiles (M % 257 == 0). */
int mb_gemm(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32,
            void* out_h16, int M, int N, int K, int period, int variant, mb_stream stream);
/* mb_gemm with the LayerNorm-residual epilogue: ln_stats != NULL: the residual that is added is LayerNorm(residual rows) re-derived from
 * {mean, rstd}[M] (epi 2 only). */
int mb_gemm_ex(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32, void* out_h16,
               int M, int N, int K, const float* ln_stats, const float* ln_g, const float* ln_b, int period, int variant, mb_stream stream);
/* LayerNorm over rows (modeling/bert.py:69-70,137-139): any of x_f32 / x_h16 / x_lo (fp16 lo halves) / stats ({mean, rstd} per row) may be NULL. */
int mb_layernorm(const float* y, const float* gamma, const float* beta, float eps, float* x_f32, void* x_h16, void* x_lo, float* stats,
                 int M, int d, mb_stream stream);
/* Split-activation GEMM (the plain forward's LayerNorm outputs as fp16 hi + lo pairs): out = (A_hi + A_lo) . W^T + bias, both [M, kw]. */
int mb_gemm_act_split(int epi, const void* A_hi, const void* A_lo, const void* W, const float* bias, const float* residual,
                      float* out_f32, void* out_h16, int M, int N, int kw, int variant, mb_stream stream);
/* "CFG pair" GEMM (mb_gen_cfg.precision >= 1): rows [0, pair_rows) of A / out are conditional, [pair_rows, 2 pair_rows) their unconditional twins whose
 * A rows hold the difference operand; out_c = f(A_c.W), out_u = f(A_c.W + A_delta.W) (GELU epilogue: the u rows receive gelu(u) - gelu(c)).
 * mb_gemm_mini: a sequence-aligned GEMM (rows % 257 == 0; pair != 0: a pair GEMM over `rows` conditional rows) with nlo MX-fp4 mini-tile passes:
 * lo = nlo x {A4, a_scale, W4, w_scale} device pointers (operand layouts: mb_kernels.h GemmArgs.lo; w_scale = N K / 128 bytes as mb_w4_from_f32 writes them; the token scales in lane order,
 * index (((blk * nseq + seq) * 4 + (r >> 6)) * 64 + (r & 15) * 4 + ((r >> 4) & 3) for token r of sequence seq).  out4 / out4_scale (GELU epilogue,
 * optional): e2m1 of the (conditional) outputs + their lane-ordered scales. */
int mb_gemm_mini(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32, void* out_h16, void* out4,
                 void* out4_scale, int rows, int pair, int N, int K, int nlo, const void* const* lo, mb_stream stream);
/* ... the pair form for sequences of seq_rows rows incl. the class token (0 = 257; 1 025 = the 512 x 512 models: eight 128-token pair tiles per sequence
 * pair, (seq_rows - 1) / 64 token groups in the lane-ordered scale arrays).  out4l / out4l_scale (GELU epilogue, optional, with out4; precision 4): the same e2m1
 * copy for the fp16 LO HALVES v - fp16(v) of the (conditional) outputs. */
int mb_gemm_mini_seq(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32, void* out_h16, void* out4,
                     void* out4_scale, void* out4l, void* out4l_scale, int rows, int pair, int seq_rows, int N, int K, int nlo, const void* const* lo, mb_stream stream);
/* e2m1 operands of the mini-tile passes: of the fp16 weight values (scales minimising the quantisation error) and of the weight's fp16 rounding error
 * W - fp16(W); dst4 = N K / 2 bytes mini-tile-packed (mb_kernels.h w4_packed_offset), scale_out = N K / 128 bytes -- one E8M0 byte per (weight row, 128
 * K-elements) -- in the kernel's lane order (w4_scale_index: byte ((((n >> 6) * (K / 128) + j) * 16 + (n & 15)) * 4 + ((n >> 4) & 3)); N % 64 == 0, K % 128 == 0. */
int mb_w4_from_f32(const float* W, int N, int K, void* dst4, void* scale_out, mb_stream stream);
int mb_w4lo_from_f32(const float* W, int N, int K, void* dst4, void* scale_out, mb_stream stream);
/* ---- the head path of gemm.hip (tests/test_hip_head.py): the two head GEMMs as the engine's head_gemms fills them, and the two weight-preparation
 * launchers of mb_gen_load.
 * mb_gemm_head: out = ((A_hi + A_lo) . W_hi^T + A_hi . W_lo^T) * *scale + bias -- sweeps (A_hi, W_hi), (A_lo, W_hi), (A_hi, W_lo) of kw columns each in one
 * fp32 accumulator, no lo x lo term; A_* fp16 [M, kw], W_* fp16 [N, kw], scale one device float.  W_lo and scale both NULL: the two-sweep form
 * (A_hi + A_lo) . W_hi^T + bias (Bert's prediction layer).  epi 3: gelu -> out_f32 [M, N], bias [N].  epi 4: row m with m % period == period - 1 is dropped,
 * the others land in row (m / period) * (period - 1) + m % period; bias [N], or with bias_per_pos [period - 1][N], row m % period.
 * Refusals (-1, nothing launched): a NULL required pointer, kw <= 0 or kw % 64, N % 4, an epilogue other than 3 / 4, epilogue 4 with period < 2 or
 * M % period, bias_per_pos outside epilogue 4, W_lo without scale or the reverse.  -3: the launcher refused. */
int mb_gemm_head(int epi, const void* A_hi, const void* A_lo, const void* W_hi, const void* W_lo, const float* scale, const float* bias, int bias_per_pos,
                 float* out_f32, int M, int N, int kw, int period, mb_stream stream);
/* dst fp16 [n] = IEEE round-to-nearest-even of src fp32 [n], what torch's .half() gives: beyond 65520 -> inf, NaN stays NaN (mb::cast_f32_to_h16: the
 * trunk weights at load); src and dst 16- / 8-byte aligned, n >= 0. */
int mb_cast_f32_to_h16(const float* src, void* dst, int64_t n, mb_stream stream);
/* src fp32 [N, K] -> hi = fp16(src * 2^S), lo = fp16(src * 2^S - hi), *scale_out = 2^-S with S = 15 - e for max |src| = f * 2^e, f in [0.5, 1) (0 for an
 * all-zero weight): mb::split_f32_to_h16_planes, the head weights at load.  tmp = one device uint32 of the caller's (scratch).  -1: a NULL pointer, N K <= 0. */
int mb_split_f32_planes(const float* src, void* hi, void* lo, int N, int K, float* scale_out, unsigned* tmp, mb_stream stream);
/* LayerNorm that also writes the e2m1 copies of its output rows: values (x4 / x4_scale) and / or fp16 lo halves (xl4 / xl4_scale); M % 257 == 0,
 * d = 768 / 1024; class-token rows (row % 257 == 256) are skipped. */
/* ... the plain forward's default for QKV / FFN-up (precision >= 2): plain sequence tiles over hi + lo activation halves
 * (A_hi, A_lo [rows, kw]; the fp16 sweep runs twice over W [N, kw]) AND one mini-tile operand set over the kw columns; epi 0 / 1. */
int mb_gemm_mini_split(int epi, const void* A_hi, const void* A_lo, const void* W, const float* bias, void* out_h16, void* out4, void* out4_scale,
                       int rows, int N, int kw, const void* const* lo, mb_stream stream);
/* ... and the residual GEMMs as the engine launches them (epilogue 2): y [rows (pair: 2 rows), N] fp32 holds the PRE-LayerNorm rows on entry; the
 * residual that is added is LayerNorm(y) re-derived from ln_stats = {mean, rstd} per row, ln_g, ln_b, and y is updated in place.  Arguments otherwise
 * as mb_gemm_mini_seq. */
int mb_gemm_mini_ln(const void* A, const void* W, const float* bias, float* y, const float* ln_stats, const float* ln_g, const float* ln_b, int rows, int pair,
                    int seq_rows, int N, int K, int nlo, const void* const* lo, mb_stream stream);
int mb_layernorm_f4(const float* y, const float* gamma, const float* beta, float eps, float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4,
                    void* xl4_scale, int M, int d, mb_stream stream);
/* ... for sequences of seq_rows rows incl. the class token: M % seq_rows == 0, (seq_rows - 1) % 64 == 0; the scale arrays hold
 * (d / 64) * (M / seq_rows) * (seq_rows - 1) bytes in lane order with (seq_rows - 1) / 64 token groups per sequence.  mb_layernorm_f4 = seq_rows 257. */
int mb_layernorm_f4_seq(const float* y, const float* gamma, const float* beta, float eps, float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4,
                        void* xl4_scale, int M, int d, int seq_rows, mb_stream stream);

/* ---- the other row kernels of norm_embed.hip, each through the product's own launcher (tests/test_hip_rows.py).  Common refusals (-1): a NULL
 * required pointer, d > 2048, an e2m1 copy (x4 / xl4) without its scale array or the reverse, e2m1 copies at d other than 768 / 1024 or for sequences
 * whose token count is no multiple of 64.  e2m1 rows have a stride of 2 d bytes (first d / 2 written); class-token rows receive none.
 * mb_layernorm_pair (mb::layernorm_pair): y fp32 [2 P, d], rows r < P conditional, r + P their unconditional twins -> x_h16 [2 P, d] =
 * fp16(LN(y_r)) | fp16(LN(y_{r+P}) - LN(y_r)), stats (optional) {mean, rstd} [2 P], the e2m1 set (optional) of the CONDITIONAL rows' values / lo halves
 * (P % seq_rows == 0 then; seq_rows is not read otherwise).  d = 768 / 1024, anything else returns -3 and writes nothing.
 * mb_pairify (mb::pairify_rows): the same operands from fp32 rows x_f32 [2 P, d] that already exist. */
int mb_layernorm_pair(const float* y, const float* gamma, const float* beta, float eps, void* x_h16, float* stats, void* x4, void* x4_scale, void* xl4,
                      void* xl4_scale, int P, int d, int seq_rows, mb_stream stream);
int mb_pairify(const float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4, void* xl4_scale, int P, int d, int seq_rows, mb_stream stream);
/* mb_embed_ln (mb::embed_ln): tokens int64 [nb, seq, m], labels int64 [nb], drop uint8 [nb] or NULL, w_in = input_proj.weight as the checkpoint holds
 * it, fp32 [d, m * gbits] (transposed inside by the product's kernel, as mb_gen_load does), b_in [d], class_emb [nclass + 1, d], pos [seq + 1, d], gamma /
 * beta [d] of the first LayerNorm (eps 1e-12), tables (optional; then w_in / b_in may be NULL) = the embedding tables [m][2^gbits + 1][d], row 2^gbits the
 * mask token's -> x_f32 and x_h16 [nb (seq + 1), d] (both required), x_lo (optional) the fp16 lo halves, the e2m1 set (optional) of the token rows.
 * Further refusals (-1): m * gbits > 24, more than 8 tables.  The entry trusts the device CONTENTS: the caller passes tokens in [0, 2^gbits] and
 * labels in [0, nclass], nothing else.  Synchronises the stream (the transposed weight is scratch).
 * mb_embed_pair (mb::embed_pair): the guided forward's fused form over nb CONDITIONAL sequences: x_f32 / x_h16 [2 nb (seq + 1), d], what mb_embed_ln
 * over [conditional | label-dropped twins] followed by mb_pairify writes, bit for bit.  Returns -3 and launches nothing where the fused kernel does
 * not serve (tables, m * gbits > 24, d other than 768 / 1024): the engine then runs those two. */
int mb_embed_ln(const int64_t* tokens, const int64_t* labels, const uint8_t* drop, const float* w_in, const float* b_in, const float* class_emb,
                const float* pos, const float* gamma, const float* beta, const float* tables, float* x_f32, void* x_h16, void* x_lo, void* x4,
                void* x4_scale, void* xl4, void* xl4_scale, int nb, int seq, int m, int gbits, int d, int nclass, mb_stream stream);
int mb_embed_pair(const int64_t* tokens, const int64_t* labels, const float* w_in, const float* b_in, const float* class_emb, const float* pos,
                  const float* gamma, const float* beta, const float* tables, float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4,
                  void* xl4_scale, int nb, int seq, int m, int gbits, int d, int nclass, mb_stream stream);
/* Attention of a CFG pair batch (the generator's guided forward, bert.py:84,137 on both streams): qkv [2 pairs N, 3d] fp16 packed in_proj rows, the
 * conditional sequences first, their unconditional twins `pairs` sequences later.  out rows of conditional sequences = softmax(QK^T/sqrt(dh))V in
 * fp16; rows of unconditional sequences = fp16(o_u - o_c), the difference operand of the out-proj pair GEMM (the conditional output tiles stay in
 * registers in between).  Every N >= 1 is computed: 256 <= N <= 288 with one head's K / V in LDS (that kernel masks keys 256 .. 287 only); shorter
 * and longer sequences by the streaming kernel, which masks every key >= N.  Refused (negative return, message): head widths other than 32 / 64. */
int mb_attention_pair(const void* qkv, void* out_h16, int pairs, int N, int d, int heads, mb_stream stream);
/* The same launch as the engine issues it at precision >= 2: + out4 [2 pairs N, 2 d] (first d / 2 bytes of a row used) = e2m1 of the CONDITIONAL outputs, two
 * values per byte, and out4_scale = one E8M0 byte per (row, head) in the lane order of the mini-tile passes (mb_kernels.h fp4_scale_index with (N - 1) / 64
 * token groups per sequence, `pairs` sequences): the token operand of the out-projection's weight-correction pass.  Head width 64, N = 257 or
 * (N - 1) % 64 == 0 beyond 288. */
/* out4l / out4l_scale (optional, both or neither; precision 4): the same for the fp16 lo halves o_c - fp16(o_c) of the conditional outputs. */
int mb_attention_pair_f4(const void* qkv, void* out_h16, void* out4, void* out4_scale, void* out4l, void* out4l_scale, int pairs, int N, int d, int heads, mb_stream stream);
/* The plain forward's attention launch (mb::attention, as the engine issues it): qkv [nb N, 3d] -> out_h16 [nb N, d] = softmax(QK^T/sqrt(dh))V, every
 * N >= 1 (kernel choice as above); head width d / heads = 32 or 64, anything else is refused.  out4 / out4_scale (optional, both or neither): the e2m1
 * copy of the token rows of EVERY sequence, written for head width 64 at N = 257 or (N - 1) % 64 == 0 beyond 288; at other shapes no copy is made. */
int mb_attention(const void* qkv, void* out_h16, void* out4, void* out4_scale, int nb, int N, int d, int heads, mb_stream stream);
/* The head-averaged softmax weights of one layer (mb::attention_probs, return_attn): out_f32 [nb, N, N]; head width 32 / 64, N <= 5120. */
int mb_attention_probs(const void* qkv, float* out_f32, int nb, int N, int d, int heads, mb_stream stream);
/* Which GEMMs of the guided forward carry the ACTIVATION-LO sets of precision >= 3 (1 QKV, 2 out-proj, 4 FFN-up, 8 FFN-down; every layer).  A handle is
 * created with the operands of its precision's own coverage (3: out-proj + FFN-up = 6; 4: + FFN-down = 14) and runs that; this can only narrow it.  The
 * product never calls this. */
int mb_gen_set_alo(mb_gen* g, int gemm_mask);
/* Persistent kernels launch one workgroup per CU.  On a stream created with a CU mask (hipExtStreamCreateWithCUMask) fewer CUs serve the launch:
 * n = the CUs the following launches should size their grids for, 0 = the device's count (default).  Process-wide, not thread-safe. */
int mb_set_cu_count(int n);
/* Walk order.  Every trunk launch takes a direction: 0 visits its tiles / workgroups / rows front to back, 1 is the exact mirror in time (the same work,
 * bit-identical results).  The generator alternates it along the launch chain of a forward so that a kernel starts on what its producer wrote last.
 * mb_gen_set_walk: 1 = alternating (the product's default), 0 = every launch in direction 0 -- for timing both in one process and comparing their logits.
 * mb_diag_set_walk: the direction the per-launch entries of this header (mb_gemm*, mb_attention*, mb_layernorm*, mb_pairify) hand to their kernel from
 * now on (process-wide, not thread-safe; default 0).  C has no default arguments, so this stands in for a trailing parameter of each of those entries.
 * mb_walk_tile / mb_walk_seq / mb_walk_row / mb_walk_group: the order functions themselves, evaluated on the host (no GPU needed; -1 on a bad index):
 * virtual block -> logical tile of the persistent GEMM walk; slot -> sequence (pair) of the grid kernels, `grp` sequences per GEMM super-row; slot -> row
 * of the row kernels over whole sequences of seq_rows (pair: pair tiles); sequences per super-row. */
int mb_gen_set_walk(mb_gen* g, int mode);
int mb_diag_set_walk(int reverse);
int mb_walk_tile(int vb, int ntiles, int reverse);
int mb_walk_seq(int slot, int n, int grp, int reverse);
int mb_walk_row(int slot, int rows, int seq_rows, int pair, int reverse);
int mb_walk_group(int seq_rows, int pair);
/* Host only: 1 if the half-tile kernel (gemm_ht.hip) takes a plain M x N x K GEMM with this epilogue, 0 if the launcher falls back to the 128 x 128
 * kernel -- among other rules, the kernel's 32-bit byte offsets need M * K * 2 and N * K * 2 below 2^32. */
int mb_gemm_ht_supported(int epi, int M, int N, int K);

/* The noise a seeded step (mb_sample_step_seeded) generates for itself, from the step kernel's own device function, in the layout of the explicit
 * path: exp_noise fp32 [B*P, C] = -logf(u) and conf_noise fp32 [B*P] = (-logf(-logf(u)) * randomize_temperature) * conf_weight for samples with seeds
 * int64 [B], slots 0 .. P - 1, at `step`; exp_u / conf_u (optional, same shapes) = the uniforms themselves.  C <= 4096, P <= 8192. */
int mb_seeded_noise(const int64_t* seeds, int step, float randomize_temperature, float conf_weight, float* exp_u, float* exp_noise, float* conf_u,
                    float* conf_noise, int B, int P, int C, mb_stream stream);

/* The lookup quantizer's search on caller buffers (vq.hip): z fp32 [N, K], codebook fp32 [C, K] (K <= 256, 2 <= C <= 65 536), l2 = normalise both;
 * idx int64 [N] = argmin_j ||z - e_j||^2 (ties to the lowest index), dist fp32 [N] (may be NULL) = that squared distance; splits = codebook splits
 * across workgroups (0 = automatic; clamped to [1, min(64, C / 64 rounded up)]). */
int mb_vq_argmin(const float* z, const float* codebook, int N, int C, int K, int l2, int splits, int64_t* idx, float* dist, mb_stream stream);

/* ---- the quantizer kernels one launch sequence at a time (vq.hip; lfq_kernel, latent_kernel, pack_image_kernel of conv.hip), each through the
 * product's own launchers on stream-ordered temporaries (tests/test_hip_quantizer.py).  Refused (-1, nothing launched): a NULL required pointer, a
 * size <= 0, a shape outside what is stated.
 * mb_vq_encode_rows: the lookup encode as mb_enc_encode_vq runs it after the encoder -- vq_prep_codebook, vq_prep_rows, vq_search -- over N = B * HW
 * rows.  Exactly one of z_h16 (fp16 rows of K values at a row stride of stride16 >= K elements; the elements beyond K are never read) and z_f32
 * (fp32 [N, K]) is non-NULL.  codebook fp32 [C, K], 2 <= C <= 65 536, 1 <= K <= 256, N <= 2^24; l2, splits as for mb_vq_argmin.  Outputs, each may be NULL:
 * idx int64 [N], dist fp32 [N], zq_nchw fp32 [B, K, HW] = the chosen (prepared) codebook rows, zraw_nchw fp32 [B, K, HW] = the rows as given. */
int mb_vq_encode_rows(const void* z_h16, int stride16, const float* z_f32, const float* codebook, int B, int HW, int C, int K, int l2, int splits,
                      int64_t* idx, float* zq_nchw, float* zraw_nchw, float* dist, mb_stream stream);
/* vq_prep_codebook + vq_gather: codes int64 [npix] (clamped to [0, C)) -> out_h16 fp16 [npix, cin_pad], channels >= K zero; cin_pad >= K a multiple
 * of 64; *sat (device, required) += stored elements beyond +-65504 (stored as +-65504). */
int mb_vq_gather(const int64_t* codes, const float* codebook, int64_t npix, int C, int K, int l2, int cin_pad, void* out_h16, unsigned* sat,
                 mb_stream stream);
/* vq_pack_latent: z_nchw fp32 [B, K, HW] -> out_h16 fp16 [B * HW, cin_pad], K in [1, 256], cin_pad and *sat as for mb_vq_gather. */
int mb_vq_pack_latent(const float* z_nchw, int B, int K, int HW, int cin_pad, void* out_h16, unsigned* sat, mb_stream stream);
/* launch_lfq: z_h16 fp16 [B * HW, Kp] (Kp >= K; columns >= K are never read), K in [1, 64] -> idx int64 [B * HW] (required), bit j = (z_j > 0), LSB
 * first (K = 64: bit 63 is the sign bit of the int64); zq_nchw / zraw_nchw fp32 [B, K, HW] (each may be NULL) = +-1 / the values as given. */
int mb_lfq_pack(const void* z_h16, int B, int HW, int K, int Kp, int64_t* idx, float* zq_nchw, float* zraw_nchw, mb_stream stream);
/* launch_latent: tokens int64 [npix], K in [1, 64] -> out_h16 fp16 [npix, 64]: channel j < K = +1 if bit j of the token is set, else -1; 0 beyond. */
int mb_lfq_latent(const int64_t* tokens, int64_t npix, int K, void* out_h16, mb_stream stream);
/* launch_pack_image: img_nchw fp32 [B, C, H, W], C in [1, 4] (what the tokenizer handle accepts) -> out_h16 fp16 [B * H * W, 64], channels < C the
 * saturating fp16 of the image, 0 beyond. */
int mb_pack_image(const float* img_nchw, int B, int C, int H, int W, void* out_h16, mb_stream stream);

/* ---- single tokenizer layers (conv.hip) on caller buffers, through the handle's own launch_conv / launch_gn / weight repack on a scratch
 * context.  These four synchronise the stream.
 * mb_conv_layer: one convolution.  in_h16 = fp16 NHWC [B, Hin, Win, Cin] with the TRUE channel count (padded to 64-channel chunks inside);
 * (Hin, Win) = (H, W), or (H / 2, W / 2) with `up` (nearest-2x upsampling fused into the 3x3 conv), or (2 H, 2 W) for ks 2 = the stride-2 3x3 TF-"same"
 * conv (one zero row / column after), run as a 2x2 conv on the space-to-depth input (s2d_kernel; Cin % 16 == 0).  w_oihw = fp32 [Cout, Cin, k, k] with
 * k = 3 for ks 2 and 3, 1 for ks 1, repacked by the product's kernel; bias fp32 [Cout] or NULL; gn_gamma / gn_beta [Cin] or both NULL: the
 * GroupNorm(32 groups, eps 1e-6) + SiLU prologue, statistics by the sweep (Cin % 64 == 0; not with ks 2); residual_h16 [B, H, W, Cout] or NULL.
 * H % 8 == 0, W % 16 == 0.  Outputs: out_h16 [B, H, W, Cout] (Cout % 4 == 0), or with final_layer (ks 3, Cout <= 4) img_nchw fp32 [B, Cout, H, W]
 * and / or img_nhwc_u8 [B, H, W, Cout] = trunc(clamp(v, 0, 1) * 255).  *saturated (host) = 4-channel groups clamped at +-65504.
 * out_gn_part (optional, B * tiles * 64 floats) = the GroupNorm partials [B][tile][32 groups][sum, sumsq] the epilogue wrote for the output and
 * *part_tiles (host) their pixel tiles per image (0: the epilogue wrote none -- Cout % 128 != 0, or channels per group not 4 / 8 / 16).
 * out_scale_shift (optional, with out_gamma / out_beta [Cout], Cout % 32 == 0) = [B, Cout] (scale, shift) of the OUTPUT's GroupNorm as the next
 * layer would get them: from the epilogue's partials when there are any, else by the sweep. */
int mb_conv_layer(const void* in_h16, const float* w_oihw, const float* bias, const float* gn_gamma, const float* gn_beta, const void* residual_h16,
                  void* out_h16, float* img_nchw, uint8_t* img_nhwc_u8, const float* out_gamma, const float* out_beta, float* out_scale_shift,
                  float* out_gn_part, int* part_tiles, unsigned* saturated, int B, int H, int W, int Cin, int Cout, int ks, int up, int final_layer,
                  mb_stream stream);
/* mb_conv_layer (= flags 0) with the two launch_conv switches the handles use and mb_conv_layer never sets.  flags bit 0: the GroupNorm prologue
 * WITHOUT SiLU (the q / k / v projection of the Taming AttnBlock; ks 1 with gn_gamma / gn_beta only).  Bit 1: stats = false -- the epilogue writes no
 * GroupNorm partials and leaves the context without a source: *part_tiles = 0 whatever Cout, and out_scale_shift comes from the sweep.
 * Refused (-1, nothing launched): bit 0 with ks other than 1 or without a prologue, any other bit. */
int mb_conv_layer_ex(const void* in_h16, const float* w_oihw, const float* bias, const float* gn_gamma, const float* gn_beta, const void* residual_h16,
                     void* out_h16, float* img_nchw, uint8_t* img_nhwc_u8, const float* out_gamma, const float* out_beta, float* out_scale_shift,
                     float* out_gn_part, int* part_tiles, unsigned* saturated, int B, int H, int W, int Cin, int Cout, int ks, int up, int final_layer,
                     int flags, mb_stream stream);
/* One ResNet block of the conv-autoencoder scaffold (mb_autoenc.h) on a scratch AutoEnc: built with mb::init_block, loaded with mb::load_param under
 * the checkpoint names norm1 / conv1 / norm2 / conv2 / nin_shortcut (.weight, .bias), run with mb::run_block from buffer 0.  x_h16 fp16
 * [B, H, W, cin]; the parameters fp32 on the device: n1_g / n1_b [cin], c1_w [cout, cin, 3, 3], n2_g / n2_b [cout], c2_w [cout, cout, 3, 3],
 * sc_w [cout, cin, 1, 1] (form 1) or [cout, cout, 1, 1] (form 2), the biases [cout] (read with `bias` only).  form 0: cin == cout, no shortcut;
 * 1: out = nin_shortcut(x) + h (Taming, sc_on_input); 2: out = h + nin_shortcut(h) (conv-VQGAN).  Outputs fp16 NHWC, each required:
 * out_h16 [.., cout]; h1_h16 = conv1's output (through AutoEnc::h1_tap: in form 2 the buffer rotation overwrites it); mid_h16 = the
 * shortcut's output (form 1) / conv2's raw output (form 2), not written in form 0 (may be NULL there).  out_scale_shift (optional, with out_gamma /
 * out_beta [cout]) = [B, cout] (scale, shift) by one further launch_gn on the block's output from whatever the block left in GnCtx.
 * *saturated (host) as for mb_conv_layer.  Refused (-1, nothing launched): a NULL required pointer, cin / cout no multiple of 64 or beyond 2048,
 * H % 8, W % 16, a form that does not go with (cin, cout).  Synchronises the stream. */
int mb_autoenc_block(const void* x_h16, const float* n1_g, const float* n1_b, const float* c1_w, const float* c1_b, const float* n2_g, const float* n2_b,
                     const float* c2_w, const float* c2_b, const float* sc_w, const float* sc_b, int form, int bias, void* out_h16, void* h1_h16,
                     void* mid_h16, const float* out_gamma, const float* out_beta, float* out_scale_shift, unsigned* saturated, int B, int H, int W,
                     int cin, int cout, mb_stream stream);
/* GroupNorm statistics of x fp16 [B, HW, C] by the sweep (gn_partial_kernel + gn_finalize_kernel): scale_shift [B, C] pairs with
 * scale = gamma * rstd, shift = beta - mean * scale; C % 32 == 0, C <= 2048. */
int mb_groupnorm_stats(const void* x_h16, const float* gamma, const float* beta, float* scale_shift, int B, int HW, int C, mb_stream stream);
/* avg_pool2d(2, 2) / space-to-depth of x fp16 [B, H, W, C] -> [B, H/2, W/2, C] / [B, H/2, W/2, 4 C] (channel (py * 2 + px) * C + c); C % 8 == 0. */
int mb_avgpool2(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream);
int mb_s2d(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream);

/* ---- the pieces of the LPIPS forward (lpips.hip, conv.hip) on caller buffers.
 * mb_conv_relu_layer: one convolution + bias + ReLU as the VGG16 stack launches it (no GroupNorm prologue or partials, zero padding 1 for ks 3;
 * ks 1 or 3): in_h16 fp16 NHWC [B, H, W, Cin] with the true channel count, w_oihw fp32 [Cout, Cin, ks, ks], bias fp32 [Cout] or NULL, out_h16
 * [B, H, W, Cout] (Cout % 4 == 0), H % 8 == 0, W % 16 == 0; *saturated (host) as for mb_conv_layer.  Synchronises the stream. */
int mb_conv_relu_layer(const void* in_h16, const float* w_oihw, const float* bias, void* out_h16, unsigned* saturated, int B, int H, int W, int Cin,
                       int Cout, int ks, mb_stream stream);
/* max_pool2d(2, 2) of x fp16 [B, H, W, C] -> [B, H/2, W/2, C]; C % 8 == 0. */
int mb_maxpool2(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream);
/* The input kernel: real / fake fp32 [B,3,H,W] -> out_h16 fp16 [2B, H, W, 64] (real images first), channel ci * 9 + ky * 3 + kx < 27 = the scaled
 * value ((2x - 1) - shift[ci]) / scale[ci] at pixel (y + ky - 1, x + kx - 1), 0 outside the image; channels 27 .. 63 are 0.  shift_scale = fp32
 * {shift[3], scale[3]} on the device.  Any H, W. */
int mb_lpips_input(const float* real, const float* fake, const float* shift_scale, void* out_h16, int B, int H, int W, int clamp01, mb_stream stream);
/* The distance kernel and its finalize alone: feat_a / feat_b fp16 [B, HW, C], C in {64, 128, 256, 512}, w fp32 [C] ->
 * per_image double [B] = mean over the pixels of sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2.  Synchronises the stream. */
int mb_lpips_distance(const void* feat_a, const void* feat_b, const float* w, int B, int HW, int C, double* per_image, mb_stream stream);
/* The five taps of a forward (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) as fp16 NHWC [2B, H / 2^k, W / 2^k, {64, 128, 256, 512, 512}], real
 * images first; arguments as for the forward. */
int mb_lpips_features(mb_lpips* h, const float* real, const float* fake, int B, int H, int W, int clamp01, void* tap0, void* tap1, void* tap2, void* tap3,
                      void* tap4, mb_stream stream);

/* ---- the pieces of the Inception-v3 forward (inception.hip) on caller buffers.
 * mb_convbn_layer: one BasicConv2d as the network launches it -- convolution (kh x kw in 1 .. 7, stride 1 or 2, zero padding ph < kh, pw < kw, no
 * bias), fp32 epilogue scale[c] * acc + shift[c], ReLU, saturating fp16 store.  in_h16 fp16 [B, H, W, in_cs] of which channels
 * [in_off, in_off + Cin) are read (in_off % 8 == 0, in_cs % 8 == 0, in_off + Cin rounded up to 8 <= in_cs); out_h16 [B, Ho, Wo, out_cs] of which
 * channels [out_off, out_off + Cout) are written and nothing else (Cout, out_off, out_cs % 4 == 0); w_oihw fp32 [Cout, Cin, kh, kw], scale / shift
 * fp32 [Cout].  variant: 0 = the launcher's choice, 1 = the 64-pixel x 64-channel wave tile, 2 = the 32 x 32 one (the same bits).
 * *saturated (host) = 4-channel groups clamped at 65504.  Synchronises the stream. */
int mb_convbn_layer(const void* in_h16, const float* w_oihw, const float* scale, const float* shift, void* out_h16, unsigned* saturated, int B, int H,
                    int W, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw, int in_off, int in_cs, int out_off, int out_cs, int variant,
                    mb_stream stream);
/* 3 x 3 pools of x fp16 [B, H, W, in_cs] channels [in_off, in_off + C) -> y [B, Ho, Wo, out_cs] channels [out_off, ..): mode 0 = max, stride 2,
 * no padding (Ho = (H - 3) / 2 + 1); 1 = max, stride 1, padding 1 over the in-image taps only; 2 = average, stride 1, padding 1, fp32 sum of the
 * in-image taps in row-major order divided by their number, one fp16 rounding.  C, offsets and strides % 8 == 0. */
int mb_pool3(const void* x_h16, void* y_h16, int B, int H, int W, int C, int mode, int in_off, int in_cs, int out_off, int out_cs, mb_stream stream);
/* uint8 [B, 3, H, W] -> fp16 [B, 299, 299, 8]: channels 0 .. 2 = (bilinear(x) - 128) / 128 with source coordinate dst * in / 299 (no half-pixel
 * offset), i0 = (dst * in) / 299 and t = ((dst * in) % 299) / 299 from the integers, v = a0 + (a1 - a0) * t along x, then along y, in fp32;
 * channels 3 .. 7 = 0. */
int mb_inception_input(const uint8_t* u8, void* out_h16, int B, int H, int W, mb_stream stream);
/* One forward with every tap; each output may be NULL.  map0 .. map3: the fp16 NHWC maps after MaxPool_2 [B, 35, 35, 192], Mixed_5d [B, 35, 35, 288],
 * Mixed_6e [B, 17, 17, 768], Mixed_7c [B, 8, 8, 2048]; tap64 / tap192 / tap768 fp32 [B, C]: the spatial means after the first pool, the second pool
 * and Mixed_6e; pool, logits_unbiased, logits as in mb_inception_forward. */
int mb_inception_taps(mb_inception* h, const uint8_t* u8, int B, int H, int W, void* map0, void* map1, void* map2, void* map3, float* tap64,
                      float* tap192, float* tap768, float* pool, float* logits_unbiased, float* logits, mb_stream stream);

/* ---- the tail the Conv+BatchNorm networks share (inception.hip; mb_inception and mb_resnet both run it): the BatchNorm fold of the loaders, the
 * spatial mean, the head and the channel tap, each through the product's own launcher on caller buffers (tests/test_hip_convnet_tail.py).  Every
 * refusal is -1 with nothing launched.  No synchronisation.
 * mb_bn_fold (launch_bn_fold): bn fp32 [4][cout] = gamma, beta, running mean, running variance -> scale[c] = gamma / sqrt(var + eps),
 * shift[c] = beta - mean * scale: five fp32 operations, each rounded to nearest.  Refused: a NULL pointer, cout < 1, eps < 0 or NaN.
 * mb_spatial_mean (launch_spatial_mean): x fp16 [B, HW, C] dense -> mean fp32 [B, C]: thread t of 256 adds pixels t, t + 256, .. in sequence from
 * +0, then red[i] += red[i + o] for o = 128 .. 1, then one division by float(HW).  Refused: a NULL pointer, B < 1, HW < 1, C < 8 or C % 8.
 * mb_fc_head (launch_fc_head): pool fp32 [B, D], w fp32 [N, D], bias fp32 [N] or NULL (read as 0) -> unbiased [B, N] = pool . w^T and / or
 * biased = unbiased + bias (one fp32 add); a lane's fma chain over its D / 64 values, then six butterfly levels.  Refused: pool or w NULL, both
 * outputs NULL, D not a multiple of 256 or beyond 2048 (the kernel would drop the tail), B < 1 or beyond 8 * 65535, N < 1.
 * mb_channel_tap (launch_channel_tap): out fp32 [B, HW, C] = channels [off, off + C) of x fp16 [B, HW, cs], widened.  Refused: a NULL pointer, an
 * empty shape, off < 0, off + C > cs.
 * mb_inception_folded_bn / mb_resnet_folded_bn: the handle's folded scale and shift [cout] of the BatchNorm `bn_prefix` (its checkpoint entries
 * without `.weight` ..; resolved as the handle's loader resolves an entry, so ResNet takes it with and without `model.`) copied to the caller's
 * device buffers.  -2: the prefix names no BatchNorm of the handle; -4: cout is not its channel count (the loaders' codes). */
int mb_bn_fold(const float* bn, float* scale, float* shift, int cout, float eps, mb_stream stream);
int mb_spatial_mean(const void* x_h16, float* mean_f32, int B, int HW, int C, mb_stream stream);
int mb_fc_head(const float* pool, const float* w, const float* bias, float* unbiased, float* biased, int B, int D, int N, mb_stream stream);
int mb_channel_tap(const void* x_h16, float* out_f32, int B, int HW, int C, int off, int cs, mb_stream stream);
int mb_inception_folded_bn(mb_inception* h, const char* bn_prefix, float* scale_out, float* shift_out, int cout, mb_stream stream);
int mb_resnet_folded_bn(mb_resnet* h, const char* bn_prefix, float* scale_out, float* shift_out, int cout, mb_stream stream);

/* ---- the pieces of the ResNet-50 perceptual loss (inception.hip, resnet.hip) on caller buffers.
 * mb_convbn_layer_ex: mb_convbn_layer with the epilogue chosen: 0 = fp16(relu(v)), v = fma(acc, scale, shift) (mb_convbn_layer itself, the same
 * bits); 1 = fp16(v), no ReLU, *saturated counts groups with |v| > 65504; 2 = fp16(relu(v + float(identity[p][c]))), the identity read as fp16
 * from channels [idn_off, idn_off + Cout) of identity_h16 [B, Ho, Wo, idn_cs] (idn_off, idn_cs % 4 == 0) and from nowhere else, the add in fp32.
 * mb_pool3_ex: mb_pool3 plus mode 3 = max, stride 2, padding 1 over the in-image taps only (Ho = (H - 1) / 2 + 1); mb_pool3 keeps refusing it. */
int mb_convbn_layer_ex(const void* in_h16, const float* w_oihw, const float* scale, const float* shift, void* out_h16, unsigned* saturated, int B, int H,
                       int W, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw, int in_off, int in_cs, int out_off, int out_cs, int variant,
                       int epilogue, const void* identity_h16, int idn_off, int idn_cs, mb_stream stream);
int mb_pool3_ex(const void* x_h16, void* y_h16, int B, int H, int W, int C, int mode, int in_off, int in_cs, int out_off, int out_cs, mb_stream stream);
/* The input path alone: real / fake fp32 [B, 3, H, W] (32 <= H, W <= 1024) -> image_h16 fp16 [2B, 224, 224, 4], real images first: channels 0 .. 2 =
 * (resize(x) - mean[c]) / std[c], channel 3 = 0; mean_std = fp32 {mean[3], std[3]} on the device.  The resize is F.interpolate(size=224,
 * mode="bilinear", antialias=True, align_corners=False): per axis scale = n / 224, support = max(scale, 1), c = scale (i + 0.5), taps j in
 * [max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n)) with weights max(0, 1 - |(j - c + 0.5) / support|) over their sum, computed in
 * double and stored as fp32; fp32 accumulation rows outer, columns inner, taps ascending, one fma each; IEEE division by std.  cols_h16 (may be
 * NULL) fp16 [2B, 112, 112, 160]: the stem's im2col of that image, channel ci * 49 + ky * 7 + kx < 147 = pixel (2 oy - 3 + ky, 2 ox - 3 + kx) or 0
 * outside the image, channels 147 .. 159 = 0.  Synchronises the stream. */
int mb_resnet_input(const float* real, const float* fake, const float* mean_std, void* image_h16, void* cols_h16, int B, int H, int W, int clamp01,
                    mb_stream stream);
/* The stem's im2col alone, at any side: image_h16 fp16 [B, S, S, 4] -> cols_h16 [B, So, So, 160], So = (S - 1) / 2 + 1, channels as above.  conv1 is
 * then mb_convbn_layer on it with Cin 147, in_cs 160, a 1 x 1 kernel and conv1.weight [64, 3, 7, 7] read as [64, 147, 1, 1].  No synchronisation. */
int mb_resnet_stem_cols(const void* image_h16, void* cols_h16, int B, int S, mb_stream stream);
/* The distance alone: logits fp32 [2B, N] (the first B rows against the last B), feat_h16 fp16 [2B, F] or NULL (F % 8 == 0) -> per_pair double [B] =
 * mean_i (a_i - b_i)^2 over the logits (+ the same over feat); sum (may be NULL) += per_pair in pair order.  No synchronisation. */
int mb_resnet_distance(const float* logits, const void* feat_h16, int B, int N, long long F, double* per_pair, double* sum, mb_stream stream);
/* The trunk on a caller's normalised image fp16 [B, S, S, 4] (channel 3 is not read), S % 8 == 0 in [32, 224], B <= 2 max_pairs -- the network is
 * convolutional up to the spatial mean, so it runs at any side.  Each output may be NULL: layer1 .. layer4 fp16 NHWC [B, s, s, {256, 512, 1024,
 * 2048}] with s = ceil(S / 4), then halved rounding up three times; pool fp32 [B, 2048]; logits fp32 [B, 1000]. */
int mb_resnet_taps(mb_resnet* h, const void* image_h16, int B, int S, void* layer1, void* layer2, void* layer3, void* layer4, float* pool, float* logits,
                   mb_stream stream);

/* ---- the pieces of the VQGAN+ discriminator (discriminator.hip; the LeakyReLU epilogue in inception.hip) on caller buffers, one launcher each.
 * mb_convbn_layer_leaky: mb_convbn_layer_ex plus epilogue 3 = fp16(v >= 0 ? v : v * slope), v = fma(acc, scale, shift), 0 <= slope <= 1,
 * *saturated counts groups with |v| > 65504; mb_convbn_layer_ex keeps refusing 3.  Synchronises the stream.
 * mb_disc_cols: images fp32 [B, 3, H, W] -> block_in's im2col fp16 [B, H, W, 96]: channel ci * 25 + ky * 5 + kx < 75 = pixel (y - 2 + ky,
 * x - 2 + kx) of channel ci or 0 outside the image, channels 75 .. 95 = 0.
 * mb_disc_downsample: x fp16 [B, H, W, C] (C % 8 == 0, C <= 2048; H, W >= 2) -> y fp16 [B, Ho, Wo, C]; K = 3, 4, 5: the binomial blur with stride 2
 * and BlurBlock's padding (per axis pad = max((ceil(n / 2) - 1) 2 + K - n, 0), pad / 2 in front), Ho = ceil(H / 2); K = 0: AvgPool2d(2), Ho =
 * floor(H / 2).  part (may be NULL; needs C % 32 == 0) float [B][nchunk][32][2], nchunk = mb_disc_down_chunks(Ho, Wo, C): per image, chunk of
 * ceil(Ho Wo / nchunk) consecutive output pixels and GroupNorm group the sum and the sum of squares of the fp32 values before rounding.
 * mb_disc_groupnorm: GroupNorm(32, C, eps 1e-5) + affine + LeakyReLU(slope) in place on x fp16 [B, HW, C] (C % 32 == 0, C <= 2048) with the
 * statistics taken from part [B][nchunk][32][2] (1 <= nchunk); *saturated (may be NULL) = the 8-channel groups clamped.  Synchronises the stream.
 * mb_disc_pool: AdaptiveMaxPool2d((16, 16)) x fp16 [B, H, W, C] -> y fp16 [B, 16, 16, C] (C % 8 == 0; any H, W >= 1).
 * mb_disc_logits: x fp16 [B, 16, 16, C] (C % 8 == 0), w_oihw fp32 [1, C, 5, 5], bias fp32 [1] -> logits / stats / sum as mb_disc_forward leaves them
 * (each may be NULL; sum needs stats).  Synchronises the stream. */
int mb_convbn_layer_leaky(const void* in_h16, const float* w_oihw, const float* scale, const float* shift, void* out_h16, unsigned* saturated, int B,
                          int H, int W, int Cin, int Cout, int kh, int kw, int stride, int ph, int pw, int in_off, int in_cs, int out_off, int out_cs,
                          int variant, int epilogue, float slope, const void* identity_h16, int idn_off, int idn_cs, mb_stream stream);
int mb_disc_cols(const float* images, void* cols_h16, int B, int H, int W, int clamp01, mb_stream stream);
int mb_disc_down_chunks(int Ho, int Wo, int C);
int mb_disc_downsample(const void* x_h16, void* y_h16, float* part, int B, int H, int W, int C, int K, mb_stream stream);
int mb_disc_groupnorm(void* x_h16, const float* part, int nchunk, const float* gamma, const float* beta, unsigned* saturated, int B, int HW, int C,
                      float slope, mb_stream stream);
int mb_disc_pool(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream);
int mb_disc_logits(const void* x_h16, const float* w_oihw, const float* bias, float* logits, double* stats, double* sum, int B, int C, mb_stream stream);

/* ---- the Taming tokenizer (spatial_attention.hip, taming.hip).
 * mb_spatial_attention: the AttnBlock's attention as the handle launches it: one head of 512 channels over the N pixels of each of B images,
 * out[b, i] = sum_j softmax_j(q[b, i] . k[b, j] * 512^-0.5) v[b, j].  q, k, v fp16, pixel (b, i) at element (b N + i) * ld of each (ld >= 512,
 * ld % 8 == 0; slices of one [B N, 1536] projection have ld = 1536), out_h16 fp16 rows at stride ldo (>= 512, % 4 == 0); N % 16 == 0,
 * 16 <= N <= 1024.  Scores and P V on MFMA with fp32 accumulation, fp32 streaming softmax over 32-key blocks, probabilities rounded to fp16 for P V.
 * No atomics on data, tiles per image: bitwise deterministic and independent of B.  *sat (device, may be NULL) += output groups of 4 clamped at
 * the fp16 range.  Refused (-1, nothing launched): a NULL pointer, a shape outside the above.
 * mb_taming_set_tap: the next forwards of the handle also copy the output of AttnBlock `block` (0, 1 = encoder.down.4.attn.{0,1}, 2 =
 * encoder.mid.attn_1, 3 = decoder.mid.attn_1, 4 .. 6 = decoder.up.4.attn.{0,1,2}) to out_h16 fp16 [B, N, 512]; NULL removes the tap. */
int mb_spatial_attention(const void* q, const void* k, const void* v, void* out_h16, unsigned* sat, int B, int N, int ld, int ldo, mb_stream stream);
int mb_taming_set_tap(mb_taming* h, int block, void* out_h16);
/* Pieces of the handle's schedule on caller data (tests/test_hip_taming_blocks.py), each through the function the schedule itself calls.
 * mb_taming_attn_block: run_attn of AttnBlock `block` (numbered as for mb_taming_set_tap) -- x fp16 [B, H, W, 512] is copied into buffer 0 and the
 * GroupNorm context cleared of its source, then GroupNorm -> the stacked 512 -> 1536 projection (no SiLU) -> spatial attention on its slices ->
 * proj_out + x.  Outputs fp16, each required: qkv_out [B H W, 1536], attn_out [B H W, 512] (the attention's output), out [B, H, W, 512].
 * out_scale_shift (optional, with out_gamma / out_beta [512]) = [B, 512] (scale, shift) by one further launch_gn on the block's output from the
 * state run_attn left.  H % 8 == 0, W % 16 == 0, H W <= latent^2, 1 <= B <= max_batch.  Only that block's parameters need to be loaded.
 * mb_taming_final: decoder.norm_out + the folded decoder.conv_out as decode runs them, on x fp16 [B, H, W, 128] -> img_nchw fp32 [B, 3, H, W]
 * and / or img_nhwc_u8 [B, H, W, 3]; H % 8 == 0, W % 16 == 0, H W <= the handle's image, 1 <= B <= max_batch.
 * mb_taming_pack_image: the encoder's input kernel alone: img_nchw fp32 [B, 3, H, W] -> out_h16 fp16 [B H W, 64], channels 0 .. 2 the saturating
 * fp16 of x * 2 - 1, 0 beyond; any H, W >= 1, B H W <= 2^24.  No handle.
 * Refused (-1, nothing launched): a NULL required pointer, a block outside [0, 7), a shape outside the above. */
int mb_taming_attn_block(mb_taming* h, int block, const void* x_h16, void* qkv_out, void* attn_out, void* out_h16, const float* out_gamma,
                         const float* out_beta, float* out_scale_shift, int B, int H, int W, mb_stream stream);
int mb_taming_final(mb_taming* h, const void* x_h16, float* img_nchw, uint8_t* img_nhwc_u8, int B, int H, int W, mb_stream stream);
int mb_taming_pack_image(const float* img_nchw, void* out_h16, int B, int H, int W, mb_stream stream);

/* ---- the fp32 reference mode's kernels (gemm_f32.hip; mb_gen_cfg.precision = MB_PREC_F32), everything fp32 in device memory.
 * mb_gemm_f32: out = epi(A[M,K] . W[N,K]^T + bias).  Every output element is acc = 0; for k = 0 .. K-1: acc = fmaf(A[m,k], W[n,k], acc) -- one chain,
 * ascending k --, then one fp32 add of bias[n], then epi: 0 nothing, 1 gelu_erf with an accurate erff, 2 + residual[m,n] (out may alias residual),
 * 3 logits -- row m with m % period == period - 1 is dropped, the others land in row (m / period) * (period - 1) + m % period; bias [N], or with
 * bias_per_pos [period - 1][N], row m % period.  Any M >= 1, N >= 1, K >= 4 with K % 4 == 0; A and W 16-byte aligned.  residual is read by epi 2 only.
 * Refusals, nothing launched: -1 a NULL required pointer or an epilogue outside 0 .. 3; -3 a shape outside the above (also: epi 3 with period < 2 or
 * M % period, bias_per_pos outside epi 3) or a misaligned operand.
 * mb_attention_f32: qkv fp32 [nb, N, 3d] (nn.MultiheadAttention's head split) -> out fp32 [nb, N, d] = softmax(Q K^T / sqrt(d / heads)) V per
 * (sequence, head), fp32 throughout, keys streamed in tiles with a running max and sum.  Any N >= 1; d / heads = 32 or 64 (-3 otherwise). */
int mb_gemm_f32(int epi, const float* A, const float* W, const float* bias, const float* residual, float* out, int M, int N, int K, int period,
                int bias_per_pos, mb_stream stream);
int mb_attention_f32(const float* qkv, float* out, int nb, int N, int d, int heads, mb_stream stream);

/* ---- the sampling session's kernels (session.hip; include/maskbit_hip.h "sampling session") on caller-owned arrays, no generator
 * (tests/test_hip_session.py).  mb_session_rows: the per-row state of a session of max_active rows, all device arrays -- slot a permutation of
 * [0, max_active), pool [max_active, max_steps] records.
 * mb_session_row_table: row_out[r] = pool[slot[r]][local_step[r]], local_step[r] += 1 for r < A.
 * mb_session_admit_rows: what mb_session_admit enqueues for K requests at rows [A, A + K) of tokens [max_active, n, m]: the start tokens (init_tokens
 * [K, n, m] clamped to [0, C], or NULL: all C), num_regen = their masked count, label, seed, N = num_steps[k] (HOST), local step 0 and the request's
 * records (packed in schedule) into pool[slot[A + k]].
 * mb_session_retire: step 3 of a tick -- the plan kernel into plan (int32 [2 + 3 max_active]: k, moves, finished rows, sources, destinations), the
 * finished rows' pred [A, n, m] combined into codes_out [k, n] in ascending row order (codes_all [A, n]: scratch), and the moves in tokens and in
 * every field of rows.  The launches are sized by A (the session sizes them by its host mirror); rows beyond the snapshot's counts do nothing.
 * Refused (-1, nothing launched): a NULL pointer, A or K below 1, rows beyond max_active, an N outside [1, max_steps], n m beyond 8192, C no power of
 * two up to 4096. */
typedef struct {
  int64_t* label; int64_t* seed;
  int32_t* num_regen; int32_t* slot; int32_t* local_step; int32_t* N;
  mb_request_step* pool;
  int max_active, max_steps;
} mb_session_rows;
int mb_session_row_table(const mb_session_rows* rows, mb_request_step* row_out, int A, mb_stream stream);
int mb_session_admit_rows(const mb_session_rows* rows, int64_t* tokens, int A, int K, const int64_t* labels, const int64_t* seeds, const int* num_steps,
                          const mb_request_step* schedule, const int64_t* init_tokens, int n, int m, int C, mb_stream stream);
int mb_session_retire(const mb_session_rows* rows, int64_t* tokens, const int64_t* pred, int64_t* codes_all, int64_t* codes_out, int32_t* plan,
                      int A, int n, int m, int C, mb_stream stream);

/* ---- the image transform's coefficient tables alone (image.hip; include/maskbit_hip.h "image transform"; tests/test_hip_image_transform.py): the
 * coefficient kernel's own device function for outputs [first, first + count) of one axis resized from in_size to out_size, on caller-owned
 * arrays -- xmin int32 [count], n int32 [count], taps int32 [count, ksize] (zero beyond n); ksize must be Pillow's (int)ceil(support) * 2 + 1, or 1
 * for in_size == out_size (the identity table of a skipped axis).  Refused (-1, nothing launched): a NULL pointer, a filter outside 0 .. 2, a
 * size outside [1, 16384], a range outside the axis, another ksize. */
int mb_image_coeffs(int in_size, int out_size, int filter, int first, int count, int ksize, int32_t* xmin, int32_t* n, int32_t* taps, mb_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MASKBIT_HIP_DIAG_H */
