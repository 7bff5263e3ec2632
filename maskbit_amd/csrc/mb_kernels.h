// Internal launcher declarations shared between the kernel translation units, engine.hip, sampler.hip and diag.hip.
#pragma once
#include "mb_common.h"

namespace mb {

// ---- GEMM  out[M,N] = A[M,K] * W[N,K]^T + bias (+ epilogue) ------------------------------------
enum GemmEpi {
  EPI_H16 = 0,         // h16 out = acc + bias                      (QKV projection)
  EPI_GELU_H16 = 1,    // h16 out = gelu_erf(acc + bias)            (FFN up projection)
  EPI_RES_F32 = 2,      // f32 out  = acc + bias + residual           (attention out-proj, FFN down)
  EPI_GELU_F32 = 3,     // f32 out  = gelu_erf(acc + bias)            (last_layer.0)
  EPI_LOGITS_F32 = 4,   // f32 out, rows with (m % period)==period-1 dropped, rest compacted (head)
};
struct GemmArgs {
  const h16* A;        // [M,K] row-major
  const h16* W;        // [N,K] row-major (torch Linear layout)
  const float* bias;    // [N]
  const float* residual;// [M,N] fp32 or null
  float* out_f32;
  h16* out_h16;
  int M, N, K;
  int period;           // EPI_LOGITS_F32 only: tokens per sequence incl. the class row
  // out = acc * (*scale) + bias for weights stored pre-scaled by a power of two (the head GEMMs' hi / lo planes, W2 below); null: 1
  const float* scale = nullptr;
  // EPI_RES_F32 with ln_stats != null: `residual` holds the PRE-LayerNorm rows y; the residual that is added is
  // LayerNorm(y) = (y - mean) * rstd * ln_g + ln_b re-derived from ln_stats[m] = {mean, rstd} (what layernorm_rows
  // wrote) -- bit-identical to the fp32 rows that kernel would have stored.  out_f32 may alias residual (in place).
  const float* ln_stats = nullptr;
  const float* ln_g = nullptr;
  const float* ln_b = nullptr;
  // EPI_LOGITS_F32: bias is [period - 1][N] (one row per position: Bert's per-position output bias, bert.py:262,332) when set
  int bias_per_pos = 0;
  // Split-activation ("fp16 hi+lo") GEMMs: A2 = the lo halves x - fp16(x) of the activations whose fp16 hi halves are A, both
  // [M, kw]; W has kw = K/2 columns and is swept twice (K-tiles below K/2 pair A with W, the others A2 with W), so both
  // products land in the same fp32 accumulator.  A2 = null / kw = 0: plain GEMM.
  const h16* A2 = nullptr;
  int kw = 0;
  // ... with W2 != null as well (128x128 kernel only; the two head GEMMs): THREE sweeps of kw columns, K = 3 kw -- (A, W), (A2, W), (A, W2) with
  // W = fp16(w * 2^S), W2 = fp16(w * 2^S - W) [N, kw] each and *scale = 2^-S: hi + lo inputs against hi + lo weights (the lo x lo term, 2^-22, is dropped)
  const h16* W2 = nullptr;
  // "CFG pair" GEMM (sequence-aligned half-tile kernel only): the M = 2 * pair_rows rows are pair_rows conditional rows followed by their
  // unconditional twins (whole sequences); in A the unconditional rows hold the difference operand fp16(x_u - x_c).  Output
  // rows: out_c = f(A_c . W), out_u = f(A_c . W + A_delta . W) -- with the GELU epilogue the unconditional rows receive gelu(u) - gelu(c),
  // i.e. the next GEMM's difference operand.  See gemm_ht.hip and DESIGN.md "Precision".
  int pair_rows = 0;
  // sequence tiles: rows per sequence incl. the class token (0 = 257).  A pair tile is 128 tokens of one sequence pair, a plain tile 256 tokens of one
  // sequence, so any (seq_rows - 1) / 128 (/ 256) that is a power of two is served: 257 (256 x 256 images) and 1 025 (the 512 x 512 models,
  // scripts/eval_maskbit.py:125,139-144); the LAST tile of a sequence (pair) stores the class row(s).
  int seq_rows = 0;
  // GELU epilogue of sequence-aligned tiles (optional): out4 / out4_scale receive e2m1 of the (conditional) OUTPUT values (row stride 2N bytes) and
  // their lane-ordered scale bytes -- the token operand of the next GEMM's weight-correction pass; class-token rows are left untouched.
  uint8_t* out4 = nullptr;
  uint8_t* out4_scale = nullptr;
  // ... and (optional, with out4; precision 4) out4l / out4l_scale: the same for the fp16 LO HALVES v - fp16(v) of those outputs, the token operand of the
  // next GEMM's activation-lo pass
  uint8_t* out4l = nullptr;
  uint8_t* out4l_scale = nullptr;
  // MX-fp4 MINI-TILE correction passes (sequence-aligned half-tile kernel, K % 128 == 0): mini-tiles of 128 token rows x 256 weight rows x 128
  // K-elements (24 KiB of LDS behind the two K-tile parities), staged while the fp16 K-tiles run and multiplied in a fifth phase between them
  // (16 v_mfma_scale_f32_16x16x128_f8f6f4 per wave).  nlo = number of operand sets:
  //   pair tiles : lo[0] (, lo[1]) on the CONDITIONAL rows: K / 128 mini-tiles per set (one per two fp16 K-tiles with one set, one per K-tile with two);
  //   plain tiles: lo[0] on both 128-row halves of the 256-token sequence tile (nlo = 1): 2 K / 128 mini-tiles, one per fp16 K-tile.
  // Operands: A4 = e2m1 token operand, two values per byte, row stride 2 K bytes (first K / 2 used); W4 = e2m1 weight operand, mini-tile-packed
  // (w4_packed_offset; N K / 2 bytes); w_scale = the weights' E8M0 bytes, ONE PER (weight row, 128 K-elements) = per (row, mini-tile), in the kernel's
  // lane order (w4_scale_index: a lane's dword of mini-tile j holds the bytes of its four n-tiles; N K / 128 bytes -- round 6; rounds 2-5 had one byte
  // per weight row: on heavy-tailed weights a row's largest rounding error then took the resolution of all its other columns); a_scale = the token operand's E8M0 bytes per (row, 64 K-elements) in LANE ORDER (fp4_scale_index: one dword per lane holds the
  // scales of its four m-tiles).  Class-token rows take no part in these passes.
  struct LoSet { const uint8_t* A4; const uint8_t* a_scale; const uint8_t* W4; const uint8_t* w_scale; };
  LoSet lo[2] = {};
  int nlo = 0;
  // fp16 epilogues (optional): lanes that stored a value outside fp16's range (or a NaN) add 1 to *sat (mb_gen_saturation_count)
  unsigned* sat = nullptr;
  // walk order (walk_tile below): 0 = the tile list front to back, 1 = back to front.  The same tiles with the same contents either way; the engine
  // alternates it along the launch chain so that a kernel starts on the rows its producer wrote last.
  int reverse = 0;
};
// Byte offset of element (row n, K-element k) of an e2m1 WEIGHT operand of the mini-tile passes.  The operand is stored MINI-TILE-PACKED:
// [N / 16][K / 128] chunks of 1 KiB = 16 rows x 64 B, the 16-byte pieces of a row swizzled with (row >> 1) & 3 -- the LDS image of one DMA
// instruction, so that every instruction of a weight mini-tile reads 1 KiB of CONTIGUOUS memory (8 full 128-byte lines) instead of 16 half lines
// of a row-major operand (measured: the L2 -> LDS path pays per line, not per byte -- profiles/r04_gemm_minitiles.md).  N % 16 == 0, K % 128 == 0.
__host__ __device__ inline size_t w4_packed_offset(int n, int k, int K) {
  const int r = n & 15, c = (k & 127) >> 5;
  return ((size_t)(n >> 4) * (K >> 7) + (k >> 7)) * 1024 + r * 64 + ((c ^ ((r >> 1) & 3)) << 4) + ((k & 31) >> 1);
}
// byte index of the E8M0 scale of (weight row n, K-elements [128 j, 128 j + 128)) in the lane-ordered weight scale arrays of the mini-tile passes
// (GemmArgs.lo w_scale; K % 128 == 0, N % 64 == 0): dword ((n >> 6) * (K / 128) + j) * 16 + (n & 15) -- what lane (n & 15) of the wave column (n >> 6)
// loads for mini-tile j --, byte (n >> 4) & 3 = its n-tile
__host__ __device__ inline size_t w4_scale_index(int n, int j, int K) {
  return (((size_t)(n >> 6) * (K >> 7) + j) * 16 + (n & 15)) * 4 + ((n >> 4) & 3);
}
// byte index of the scale of (token row r of sequence seq, 64-column block blk) in the lane-ordered scale arrays of the mini-tile passes
// (groups = 64-token groups per sequence: 4 for the 256-token models, 16 for the 1024-token ones of 512 x 512 images)
__host__ __device__ inline size_t fp4_scale_index(int blk, int nseq, int seq, int r, int groups = 4) {
  return (((size_t)blk * nseq + seq) * groups + (r >> 6)) * 64 + (r & 15) * 4 + ((r >> 4) & 3);
}
// ---- walk order: which sequence (pair) a trunk launch visits when -------------------------------------------------------------------------------
// A consumer that streams a hand-off larger than the 256 MiB Infinity Cache in its producer's direction asks first for the bytes written longest ago,
// which are gone.  Each launch therefore takes a direction (`reverse`, 0 or 1) and the engine alternates it along the launch chain: a kernel starts
// with the sequences its producer touched LAST.  Direction 1 is the exact mirror in time of direction 0 -- the same tiles, workgroups and rows,
// visited in the opposite order; no arithmetic changes.  (Measured, profiles/walk_order.md: at 64 pairs the hand-off that large is FFN-up's output,
// and FFN-down is where the time is won; the others fit the cache in either direction.)
//
// The persistent GEMM walk (gemm_ht.hip): virtual block vb -> logical tile; direction 0 is the XCD-contiguous map the kernel always had.
__host__ __device__ inline int walk_tile(int vb, int ntiles, int reverse) { return xcd_remap(reverse ? ntiles - 1 - vb : vb, ntiles); }
__host__ __device__ inline int xcd_chunk_start(int x, int n) { return xcd_remap(x, n); }   // first item of XCD x's chunk (x < 8)
// The grid kernels (attention: workgroup = (sequence, head); LayerNorm: rows of a sequence): slot s of n sequences (pairs) -> the sequence visited s-th.
// A GEMM walk is eight sawteeth, not one ramp: XCD x owns the contiguous sequences [xcd_chunk_start(x, n), xcd_chunk_start(x + 1, n)) and walks them in
// super-rows of `grp` sequences (8 m-tiles), all eight XCDs in step.  Direction 0 lists the sequences in the order such a direction-0 walk completes them
// (super-row t of every chunk before super-row t + 1 of any), direction 1 is its mirror: the sequences a direction-0 GEMM wrote last come first.
__host__ __device__ inline int walk_seq(int slot, int n, int grp, int reverse) {
  if (reverse) slot = n - 1 - slot;
  const int q = n >> 3, r = n & 7;
  for (int lo = 0, before = 0;; lo += grp) {
    const int a = q + 1 - lo < grp ? (q + 1 - lo > 0 ? q + 1 - lo : 0) : grp;   // sequences of this super-row in a long chunk (the first r) ..
    const int b = q - lo < grp ? (q - lo > 0 ? q - lo : 0) : grp;               // .. and in a short one
    const int step = r * a + (8 - r) * b;
    if (slot < before + step) {
      int s = slot - before, x;
      if (s < r * a) { x = s / a; s -= x * a; }
      else { s -= r * a; x = s / b; s -= x * b; x += r; }
      return xcd_chunk_start(x, n) + lo + s;
    }
    before += step;
  }
}
// sequences (pairs) per super-row of the GEMM walk: 8 m-tiles of 128 tokens of a pair / 256 tokens of a plain sequence
inline int walk_group(int seq_rows, bool pair) { const int tps = (seq_rows - 1) / (pair ? 128 : 256); return tps >= 8 ? 1 : tps >= 1 ? 8 / tps : 8; }
// The row kernels (one wave per row or row pair): slot s of `rows` rows = whole sequences of seq_rows -> the row visited s-th.  The sequences follow
// walk_seq, a sequence's rows keep their order (and are mirrored with everything else in direction 1).
struct WalkRows { int seq_rows, grp, reverse; };
__host__ __device__ inline int walk_row(int slot, int rows, const WalkRows& w) {
  if (w.reverse) slot = rows - 1 - slot;
  const int ss = slot / w.seq_rows;
  return walk_seq(ss, rows / w.seq_rows, w.grp, 0) * w.seq_rows + (slot - ss * w.seq_rows);
}
// (rows that are not whole sequences of seq_rows, or seq_rows = 0: one run of rows, front to back or back to front)
inline WalkRows walk_rows(int rows, int seq_rows, bool pair, int reverse) {
  if (seq_rows <= 0 || rows % seq_rows) return WalkRows{rows, 8, reverse ? 1 : 0};
  return WalkRows{seq_rows, walk_group(seq_rows, pair), reverse ? 1 : 0};
}

int gemm_tn(hipStream_t s, GemmEpi epi, const GemmArgs& a, int variant = 0);   // 0, or -1: lo-pass request outside the half-tile kernel's shapes
bool gemm_ht_supported(GemmEpi epi, const GemmArgs& a);
void gemm_ht(hipStream_t s, GemmEpi epi, const GemmArgs& a, int mt);
void set_cu_count(int n);   // persistent grids are sized for n CUs (0 = the device's count): for launches on CU-masked streams

// ---- the fp32 reference mode (gemm_f32.hip; MB_PREC_F32): everything fp32 in global memory -------------------------------------------------------
// gemm_f32: out[M,N] = epi(A[M,K] . W[N,K]^T + bias) on the f32-input MFMA.  NUMERICAL CONTRACT: every output element is
//   acc = 0; for k = 0 .. K-1: acc = fmaf(A[m,k], W[n,k], acc)   -- one chain, ascending k, continued across K-tiles in the same accumulator --,
// then ONE fp32 add of the bias, then the epilogue: no split-K, no reordering, so the result does not depend on tile position, batch size or grid.
// Any M >= 1, N >= 1, K >= 4 with K % 4 == 0 (A, W 16-byte aligned); ragged M / N / K-tile edges are guarded, nothing is read out of bounds.
enum GemmF32Epi {
  F32_EPI_PLAIN = 0,    // out = acc + bias                               (QKV)
  F32_EPI_GELU = 1,     // out = gelu_erf(acc + bias), accurate erff      (FFN-up, last_layer.0)
  F32_EPI_RES = 2,      // out = (acc + bias) + residual[m,n]             (out-proj, FFN-down; out may alias residual)
  F32_EPI_LOGITS = 3,   // EPI_LOGITS_F32's rows: m % period == period - 1 dropped, the rest compacted; bias [N] or, bias_per_pos, [period - 1][N]
};
struct GemmF32Args {
  int epi;
  const float* A; const float* W; const float* bias; const float* residual; float* out;
  int M, N, K;
  int period = 0, bias_per_pos = 0;
};
int gemm_f32(hipStream_t s, const GemmF32Args& a);   // 0, or -1: refused (shape, alignment, a missing pointer), nothing launched
// fp32 qkv [nb, N, 3d] (nn.MultiheadAttention's head split, as `attention` below) -> fp32 out [nb, N, d] = softmax(Q K^T / sqrt(dh)) V per (sequence,
// head); scores, softmax and P V in fp32 on the VALU, keys streamed in tiles with a running max and sum.  Any N >= 1; d / heads = 32 or 64 (-1 otherwise).
int attention_f32(hipStream_t s, const float* qkv, float* out, int nb, int N, int d, int heads);

// e2m1 copy of a weight for the mini-tile passes: e2m1(fp16(W[n][k]) * 2^r) in the mini-tile-packed layout (w4_packed_offset; N K / 2 bytes), r per
// (row, 128 columns) chosen to minimise the block's quantisation error; scale_out [N K / 128] in the kernel's lane order (w4_scale_index).  N % 64 == 0, K % 128 == 0.
void w4_from_f32(hipStream_t s, const float* src, uint8_t* dst4, int N, int K, uint8_t* scale_out);
// the same layout for the weight's fp16 ROUNDING ERROR: e2m1((W - fp16(W)) * 2^r), r from the (row, 128-column) block's largest |error| (no saturation)
void w4lo_from_f32(hipStream_t s, const float* src, uint8_t* dst4, int N, int K, uint8_t* scale_out);

// e2m1 copies written by the row-wise producers for the trunk GEMMs' mini-tile passes (GemmArgs.lo): the rows' VALUES (x4, with the
// lane-ordered per-(row, 64 columns) scale bytes x4s) and / or their fp16 LO HALVES x - fp16(x) (xl4 / xl4s); rows are tokens of nseq sequences of
// 257 (row stride 2d bytes, first d / 2 used; class-token rows are skipped).  hidden = 768 / 1024 only.
struct Fp4Rows { uint8_t* x4 = nullptr; uint8_t* x4s = nullptr; uint8_t* xl4 = nullptr; uint8_t* xl4s = nullptr; int nseq = 0; int seq_rows = 257; };   // seq_rows: tokens per sequence incl. the class token

// ---- LayerNorm over rows of y[M,d] -> x_f32 (optional), x_h16 (optional), stats[M][2] = {mean, rstd} (optional) ---
void layernorm_rows(hipStream_t s, const float* y, const float* gamma, const float* beta, float eps,
                    float* x_f32, h16* x_h16, float* stats, int M, int d, h16* x_lo = nullptr,
                    const Fp4Rows& f4 = Fp4Rows{}, int reverse = 0, int seq_rows = 0);   // x_lo: fp16(x - fp16(x)), optional; reverse / seq_rows: the walk order (walk_row)

// "CFG pair" forms (hidden = 768 / 1024 only; -1 otherwise): rows r < P are conditional, r + P their unconditional twins.  Writes
// x_h16[r] = fp16(x_c), x_h16[r + P] = fp16(x_u - x_c), both rows' {mean, rstd}; optional f4: e2m1 copies of the CONDITIONAL rows.
int layernorm_pair(hipStream_t s, const float* y, const float* gamma, const float* beta, float eps, h16* x_h16, float* stats, int P, int d,
                   const Fp4Rows& f4 = Fp4Rows{}, int reverse = 0, int seq_rows = 0);
int pairify_rows(hipStream_t s, const float* x32, h16* x_h16, int P, int d, const Fp4Rows& f4 = Fp4Rows{}, int reverse = 0, int seq_rows = 0);

// ---- bit-token embed + class token + pos-emb + first LayerNorm (bert.py:440-454, 482-496) -------
struct EmbedArgs {
  const int64_t* tokens;   // [nb, seq, m]
  const int64_t* labels;   // [nb]
  const uint8_t* drop;     // [nb] or null
  const float* w_in;       // [K, d]  (input_proj.weight transposed at load)
  const float* b_in;       // [d]
  const float* class_emb;  // [nclass+1, d]
  const float* pos;        // [seq+1, d]
  const float* gamma; const float* beta;
  float* x_f32; h16* x_h16;   // [nb*(seq+1), d]  (embed_ln: x_h16 may be null)
  int nb, seq, m, gbits, d, nclass;
  // Bert (modeling/bert.py:313-315): per-group embedding tables [m][2^gbits + 1][d] summed instead of the bit projection
  const float* tables = nullptr;
  h16* x_lo = nullptr;     // optional: lo halves of x_h16 (split-activation GEMMs)
  Fp4Rows f4;              // optional: e2m1 copies for the mini-tile passes (embed_pair: of the conditional rows)
};
void embed_ln(hipStream_t s, const EmbedArgs& a);
// guided forward: a.nb = B conditional sequences (tokens [B, seq, m], labels [B]); rows of the label-dropped twins are written B * (seq + 1) rows further
// down; x_h16 receives the pair operands (fp16(x_c) | fp16(x_u - x_c)), a.f4 (optional) the e2m1 copies of the conditional rows.  -1: shape not
// served (embedding tables, widths other than 768 / 1024) -> embed_ln over [cond | twins] + pairify_rows
int embed_pair(hipStream_t s, const EmbedArgs& a);
void transpose_f32(hipStream_t s, const float* src /*[rows,cols]*/, float* dst /*[cols,rows]*/, int rows, int cols);

// ---- multi-head self-attention over packed qkv [nb*N, 3d] -> out [nb*N, d] -----------------------
void attention(hipStream_t s, const h16* qkv, h16* out, int nb, int N, int d, int heads,
               uint8_t* out4 = nullptr, uint8_t* out4s = nullptr, int reverse = 0);   // out4 / out4s (N = 257 or (N - 1) % 64 == 0 beyond the one-block kernel's length; head width 64): e2m1 of the outputs + lane-ordered scale
                                                                      // bytes for the out-proj GEMM's mini-tile pass
// "CFG pair" attention: sequences [0, P) are conditional, [P, 2P) their unconditional twins; one workgroup runs a (pair, head) -- conditional pass,
// then the twin with the conditional output tiles kept in registers -- and writes out[r + P*N] = fp16(att_u - att_c), the difference operand of the
// out-proj pair GEMM.  256 <= N <= 288: K / V of a head in LDS; longer sequences (the 1024 + 1-token models) and shorter ones: the streaming kernel in pair form.
// out4 / out4s (head dimension 64 only): e2m1 of the conditional output values, row stride 2d bytes, + lane-ordered E8M0 scale bytes (GemmArgs.lo)
// out4l / out4ls (optional, with out4; precision 4): the same for the fp16 lo halves o_c - fp16(o_c) of the conditional outputs (the out-proj GEMM's activation-lo pass)
int attention_pair(hipStream_t s, const h16* qkv, h16* out, int P, int N, int d, int heads, uint8_t* out4 = nullptr, uint8_t* out4s = nullptr,
                   uint8_t* out4l = nullptr, uint8_t* out4ls = nullptr, int reverse = 0);   // reverse: the walk order (walk_seq above)
// head-averaged attention weights [nb, N, N] fp32 of one layer (return_attn=True); -1 if the shape is not supported
int attention_probs(hipStream_t s, const h16* qkv, float* out, int nb, int N, int d, int heads);

// ---- fused sampling step (sampling.py:90-131) ----------------------------------------------------
// The constants of one sample at one step of a requests run (mb_request_step of include/maskbit_hip.h, field for field)
struct RequestStep { float scale, temperature, mask_ratio, rand_temp, conf_w; int32_t step; };
struct StepArgs {
  const float* logits_c; const float* logits_u;   // [B, n*m, C]
  float scale, temperature;
  const float* exp_noise;    // [B*n*m, C]
  const float* conf_noise;   // [B, n*m]
  int k_mask_len;
  int64_t* tokens;           // [B, n*m] out (must not alias tokens_in)
  int64_t* pred;             // [B, n*m] out (may be null)
  int B, P /* n*m */, C;
  // seeds != null: the SEEDED step (mb_sample_step_seeded) -- exp_noise / conf_noise are not read; the kernel computes both values from
  // (seeds[b], step, slot, class) as include/maskbit_hip.h defines them: int64 [B] (device) = the samples' 64-bit seeds, step = the absolute step of
  // the run, rand_temp = randomize_temperature, conf_w = float32(1 - (step + 1) / num_steps).  Needs the per-sample threshold rule (num_regen).
  const int64_t* seeds = nullptr;
  int step = 0;
  float rand_temp = 0.f, conf_w = 0.f;
  // req != null (with seeds): the PER-SAMPLE step (mb_sample_step_requests) -- scale, temperature, step, rand_temp, conf_w above and the mask_ratio of
  // sample_step are not read; sample b takes them from req[b] (device [B]).
  const RequestStep* req = nullptr;
};
// num_regen != null: the EDIT step (mb_sample_step_edit) -- per sample b the mask length is floor(mask_ratio * num_regen[b]), the masked count is the
// sample's own, and a sample with fewer than two masked slots is not re-masked; a.k_mask_len is not read.
int sample_step(hipStream_t s, const StepArgs& a, const int64_t* tokens_in, const int* num_regen = nullptr, float mask_ratio = 0.f);
// The noise of a seeded step in the explicit path's layout, from the step kernel's own device function: exp_u / exp_noise [B*P, C], conf_u / conf_noise
// [B*P] (each may be null).  -1: C or P beyond the step kernel's.
int seeded_noise_dump(hipStream_t s, const int64_t* seeds, int step, float rand_temp, float conf_w, float* exp_u, float* exp_noise, float* conf_u,
                      float* conf_noise, int B, int P, int C);

// ---- small integer helpers of the loop (sampling.py:65, factorization.py:7-24) -------------------
void fill_i64(hipStream_t s, int64_t* dst, int64_t value, size_t n);

// ---- image editing (edit.hip): the helpers in front of and behind a sampling run that starts from a partly known token map ----------------------
// One workgroup per sample, deterministic count.  src int64 [B, P] -> dst (may be null) = src clamped to [0, C], num_regen[b] = slots of sample b equal to C
void edit_load_tokens(hipStream_t s, const int64_t* src, int64_t* dst, int* num_regen, int B, int P, int C);
// codes int64 [B, n] + regeneration mask uint8 [B, n, m] -> grouped tokens [B, n, m] ((code >> g * gbits) & (C - 1); C where the mask is set), num_regen[B]
void edit_init(hipStream_t s, const int64_t* codes, const uint8_t* regen, int64_t* tokens, int* num_regen, int B, int n, int m, int gbits);
// pixel mask uint8 [B, H, W] -> token mask uint8 [B, H / st, W / st]: 1 if any pixel of the st x st block is set.  st a power of two, W % st == 0, H % st == 0
void edit_token_mask(hipStream_t s, const uint8_t* pixel_mask, uint8_t* token_mask, int B, int H, int W, int st);
// x = mask ? gen : orig per pixel (fp32 [B, C, H, W], mask uint8 [B, H, W]); out_nchw (may be null) = x, out_u8 (may be null) uint8 [B, H, W, C] =
// trunc(clamp(x, 0, 1) * 255).  C in 1 .. 4, W % 4 == 0; -1 otherwise
int edit_composite(hipStream_t s, const float* gen, const float* orig, const uint8_t* pixel_mask, float* out_nchw, uint8_t* out_u8, int B, int C, int H, int W);
void combine_groups(hipStream_t s, const int64_t* tokens /*[rows,m]*/, int64_t* codes /*[rows]*/, size_t rows, int m, int gbits);

// ---- sampling session (session.hip): the per-row state of the active prefix [0, A) and the kernels that keep it dense ----------------------------
// Device arrays of `cap` rows (mb_session_rows of include/maskbit_hip_diag.h, field for field): slot[] is a permutation of [0, cap) -- rows [0, A) hold
// the pool slots in use --, pool [cap, max_steps] the schedule records of the request in each slot.
struct SessionRows {
  int64_t* label; int64_t* seed;
  int* num_regen; int* slot; int* local_step; int* N;
  RequestStep* pool;
  int cap, max_steps;
};
// What one admit launch carries in its kernel arguments: num_steps of up to MAX requests and where each one's records begin in the packed schedule
struct AdmitBatch { enum { MAX = 64 }; int n[MAX]; int off[MAX]; };
// ints of the plan snapshot of a session of cap rows: {k, moves, finished[cap], src[cap], dst[cap]}
inline size_t session_plan_ints(int cap) { return 2 + 3 * (size_t)cap; }
// row[r] = pool[slot[r]][local_step[r]]; local_step[r] += 1, r < A (A >= 1)
void session_row_table(hipStream_t s, const SessionRows& st, RequestStep* row, int A);
// Rows [A, A + K) of tokens [cap, P]: the start tokens (init_tokens [K, P] clamped to [0, C], or null: all C) and num_regen = their masked count -- both
// edit_load_tokens' --, label, seed, N = num_steps[k] (HOST [K]), local step 0, and request k's num_steps[k] records -- packed one request after the
// other in sched (device) -- into pool[slot[A + k]]
void session_admit(hipStream_t s, const SessionRows& st, int64_t* tokens, const int64_t* init_tokens, const int* num_steps, const int64_t* labels,
                   const int64_t* seeds, const RequestStep* sched, int A, int K, int P, int C);
// Step 3 of a tick.  The snapshot: finished rows F = {r < A : local_step[r] == N[r]} ascending, holes (dst) = F below A' = A - |F| ascending, movers
// (src) = the unfinished rows at or above A' ascending.  Then codes_out [k, n] = combine_groups(pred [A, n, m]) of the rows of F (codes_all [A, n]:
// scratch), and row src[j] -> row dst[j]: the n m tokens of the row in `tokens` [cap, n m], label, seed, num_regen, local step, N; slots swapped.
// k and moves size the two launches: the exact counts (the session's host mirror), or upper bounds (rows beyond the snapshot's counts do nothing)
void session_retire(hipStream_t s, const SessionRows& st, int* plan, int64_t* tokens, const int64_t* pred, int64_t* codes_all, int64_t* codes_out,
                    int A, int n, int m, int gbits, int k, int moves);

// ---- fp32 -> h16 repack ------------------------------------------------------------------------
void cast_f32_to_h16(hipStream_t s, const float* src, h16* dst, size_t n);
// W[N,K] fp32 -> two planes hi[N,K] = fp16(W*2^S), lo[N,K] = fp16(W*2^S - hi) (GemmArgs.W / W2), S chosen from max|W| (tmp: one device uint32 of
// scratch); *scale_out = 2^-S.  Stream-ordered, no host synchronisation.
void split_f32_to_h16_planes(hipStream_t s, const float* src, h16* hi, h16* lo, int N, int K, float* scale_out, unsigned* tmp);

}  // namespace mb
