// The generator handle of libmaskbit_hip.so (include/maskbit_hip.h): checkpoint ingest with h16 repack, the two forward schedules (plain and
// differential CFG), the fused sampling step and the whole sampling loop; and the three ABI-wide entries (mb_abi_version, mb_last_error, mb_prof_*).
// The tokenizer handle's entry points are in decoder.hip, the diagnostic ones (include/maskbit_hip_diag.h) in diag.hip -- all but mb_gen_set_alo,
// which needs struct mb_gen; the error path, the device-allocation arena and the profiling scopes they all share are in mb_abi.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/maskbit_hip_diag.h"
#include "mb_abi.h"
#include "mb_kernels.h"

using mb::fail;
using mb::g_prof;
using mb::launched;
using mb::ProfScope;

// ================================================================================================
// generator
// ================================================================================================
// An e2m1 (MX-fp4) copy of an activation: values at the row stride of the fp16 sibling (2 * width bytes, the first width / 2 used) and their
// block-scale bytes in lane order, [width / 64][sequences][256]
struct F4Buf { uint8_t *v = nullptr, *s = nullptr; };

struct mb_gen {
  mb_gen_cfg c{};
  int max_seqs = 0, chunk_seqs = 0, N = 0, C = 0, gbits = 0, device = 0;   // chunk_seqs: sequences per forward pass (workspace size)
  struct Layer {
    h16 *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;
    float *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
    float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
  };
  std::vector<Layer> layers;
  float *w_in = nullptr, *b_in = nullptr, *class_emb = nullptr, *pos = nullptr, *ln0g = nullptr, *ln0b = nullptr;
  h16 *wl = nullptr, *wp = nullptr;
  float *bl = nullptr, *lnhg = nullptr, *lnhb = nullptr, *bp = nullptr;
  float *lnag = nullptr, *lnab = nullptr;              // norm_after_transformer (pre-norm variant)
  float *tables = nullptr, *bias_pos = nullptr;       // Bert: embedding tables [m][C+1][d]; output bias [seq][m*C]
  unsigned* split_tmp = nullptr;                        // scratch of the head weights' hi / lo split
  // workspace
  float *y_f32 = nullptr, *ln_stats = nullptr;       // fp32 residual stream (pre-LayerNorm rows) and {mean, rstd} per row
  h16 *x_h16 = nullptr, *x_lo = nullptr, *qkv = nullptr, *att = nullptr, *h = nullptr;   // x_lo: lo halves of x_h16 (head GEMMs; precision >= 1: QKV / FFN-up of plain forwards)
  // precision >= 1: differential CFG forward (pair_ok = the shape allows it).  precision >= 2 (mini_ok = the shape allows it): every trunk GEMM carries the
  // MX-fp4 weight-correction mini-tiles (gemm_ht.hip, XP = 6) -- in the guided forward on the conditional rows, in the plain forward (257-token sequences)
  // on every row: x4 / att4 / h4 hold e2m1 of the LayerNorm outputs, attention outputs and FFN hiddens,
  // w4lo / w4los e2m1 of the weights' fp16 rounding errors.  precision 3 additionally corrects the fp16 rounding of the LayerNorm OUTPUTS
  // in the guided forward's FFN-up GEMM: xl4 = e2m1 of their lo halves, w4 / w4s = e2m1 of the (fp16) weight net.0.
  bool pair_ok = false, mini_ok = false;
  F4Buf x4, xl4;
  std::vector<uint8_t*> w4, w4s;                                                         // [4 * layer + {qkv, o, 1, 2}]: the GEMMs of alo_mask_built only
  float* logits_tmp = nullptr;                          // guided forwards over more pairs than one pass holds
  // The two head GEMMs run hi + lo inputs against hi + lo WEIGHTS in every mode (GemmArgs.W2: three sweeps): their rounding reaches the logits
  // un-averaged -- fp16 head weights alone were a quarter of the sampled-logit error variance left after the trunk's weight correction
  // (tests/diag/error_budget.py) -- and the two GEMMs are 0.4 % of a forward.  wl / wp = fp16(w 2^S), wl_lo / wp_lo = the remainders, head_scale = 2^-S.
  // (Bert's tied head, embed_tables: wp holds the tables' first C rows per group as single fp16, no lo plane.)
  h16 *wl_lo = nullptr, *wp_lo = nullptr;
  float* head_scale = nullptr;
  unsigned* sat = nullptr;                              // lanes of the QKV / FFN-up epilogues that clamped a fp16 store (mb_gen_saturation_count)
  std::vector<uint8_t*> w4lo, w4los;                                                     // [4 * layer + {qkv, o, 1, 2}]
  F4Buf att4, h4;                                       // e2m1 of the conditional attention outputs / FFN hiddens
  F4Buf attl4, hl4;                                     // precision 4: e2m1 of their fp16 LO HALVES (activation-lo sets of out-proj / FFN-down)
  // The run the sampling loop is in the middle of (step chunks).  id = what every chunk of one run shares: samples, total steps, guidance flag and
  // kind -- 0 plain, 1 an EDIT run (mb_sample_edit: started from the caller's tokens; num_regen = its initial masked count per sample, [max_seqs]),
  // 2 a SEEDED run (mb_sample_seeded: an edit run whose steps generate their noise); next = the step the next chunk must begin with (-1: no run).
  // cfg_labels / cfg_B: during one call of the loop, gen_forward_cfg's lab_cfg / drop_cfg already hold [labels | labels] / [0 | 1] for this many pairs.
  struct Run {
    struct Id {
      int B = 0, steps = 0, guided = 0, kind = 0;
      bool operator==(const Id& o) const { return B == o.B && steps == o.steps && guided == o.guided && kind == o.kind; }
    } id;
    int next = -1;
    const int64_t* cfg_labels = nullptr;
    int cfg_B = 0;
  } run;
  int* num_regen = nullptr;
  // precision >= 3: which GEMMs carry the activation-lo set (1 QKV, 2 out-proj, 4 FFN-up, 8 FFN-down).  Coverage measured on the reference's own runs in round 6
  // (profiles/r06_coverage.md: four 14-bit / 256-step runs, four 12-bit runs, three trained-like runs; mismatches / guided-forward time of 64 pairs):
  //   none 595 / 263 / 271 at 29.9 ms;  FFN-up of layers >= depth / 2 (round 5's precision 3) 506 / 222 / 276 at 30.5;  out-proj + FFN-up 384 / 186 / 219 at 31.6;
  //   out-proj + FFN-up + FFN-down 241 / 115 / 203 at 33.4;  all four 228 / 116 / 200 at 34.3 -- the QKV set buys nothing (as round 5 found for precision 3).
  // precision 3 = out-proj + FFN-up of every layer (6); precision 4 = + FFN-down (14).  mb_gen_set_alo (diagnostic) narrows within what the handle was created with.
  int alo_mask = 0, alo_mask_built = 0;
  // Walk order of the trunk launches (mb_kernels.h walk_tile / walk_seq): 1 = every launch of a forward walks the batch opposite to the launch in front of
  // it, so that it starts on what its producer wrote last (the product); 0 = every launch front to back (mb_gen_set_walk, diagnostic: the A/B of the two)
  int walk = 1;
  // precision MB_PREC_F32, the fp32 reference mode (gemm_f32.hip): the GEMM weights stay the checkpoint's fp32 (layers32, wl32, wp32 -- Bert's tied
  // head: the tables' first C rows per group), the workspace is fp32 only -- x_f32 = the LayerNorm output rows (GEMM operand AND residual), y_f32 = the
  // pre-LayerNorm sum, qkv32 / att32 / h32 -- and none of the fp16 / e2m1 buffers above exist.  Every forward of such a handle is gen_forward_f32_impl.
  bool f32 = false;
  struct Layer32 { float *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr; };
  std::vector<Layer32> layers32;
  float *wl32 = nullptr, *wp32 = nullptr;
  float *x_f32 = nullptr, *qkv32 = nullptr, *att32 = nullptr, *h32 = nullptr;
  int64_t *tok_a = nullptr, *tok_b = nullptr, *tok_cfg = nullptr, *lab_cfg = nullptr, *pred = nullptr, *codes = nullptr;
  uint8_t* drop_cfg = nullptr;
  float* logits = nullptr;
  mb::DevArena mem;
  int loaded = 0;
};

namespace {

// rows x width e2m1 values and the scale bytes of ntok = sequences x tokens rows, zeroed
void alloc_f4(mb::DevArena& m, F4Buf* b, size_t rows, size_t width, size_t ntok) {
  m.zeroed(&b->v, rows * 2 * width);
  m.zeroed(&b->s, (width / 64) * ntok + 256);
}

// The head (bert.py:411-417, 500-503): last_layer.0 + GELU, LayerNorm, prediction layer, on the hi + lo rows the trunk's last LayerNorm left in
// x_h16 / x_lo -- hi + lo inputs against hi + lo weights in every mode (mb_gen::wl_lo)
int head_gemms(mb_gen* g, float* logits, int M, hipStream_t s) {
  using namespace mb;
  const mb_gen_cfg& c = g->c;
  const int d = c.hidden;
  int rc = 0;
  { ProfScope p("gemm_head", s, true);
    GemmArgs ga{g->x_h16, g->wl, g->bl, nullptr, g->y_f32, nullptr, M, d, 3 * d, 0, g->head_scale};
    ga.A2 = g->x_lo; ga.kw = d; ga.W2 = g->wl_lo;
    rc |= gemm_tn(s, EPI_GELU_F32, ga); }
  { ProfScope p("layernorm", s, true);
    layernorm_rows(s, g->y_f32, g->lnhg, g->lnhb, 1e-12f, nullptr, g->x_h16, nullptr, M, d, g->x_lo); }
  { ProfScope p("gemm_head", s, true);
    GemmArgs ga{g->x_h16, g->wp, c.embed_tables ? g->bias_pos : g->bp, nullptr, logits, nullptr, M, c.splits * g->C, (g->wp_lo ? 3 : 2) * d, g->N,
                g->wp_lo ? g->head_scale + 1 : nullptr};
    ga.A2 = g->x_lo; ga.kw = d; ga.W2 = g->wp_lo;
    ga.bias_per_pos = c.embed_tables;
    rc |= gemm_tn(s, EPI_LOGITS_F32, ga); }
  return rc;
}

int gen_forward_impl(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits,
                     int nb, hipStream_t s, float* attn = nullptr) {
  using namespace mb;
  const mb_gen_cfg& c = g->c;
  const int d = c.hidden, f = c.mlp, N = g->N, M = nb * N;
  // return_attn: layer l's head-averaged attention weights go to attn[l][nb][N][N], computed from the same qkv rows
  auto attn_maps = [&](int l) {
    return attn ? attention_probs(s, g->qkv, attn + (size_t)l * nb * N * N, nb, N, d, c.heads) : 0;
  };
  int attn_rc = 0, gemm_rc = 0;
  // the direction bit of this forward (mb_gen::walk): the embedding starts the chain front to back, every trunk launch after it takes the bit and flips it
  int wdir = 0;
  auto walk_next = [&] { wdir ^= g->walk; return wdir; };
  // The plain forward (mb_gen_forward, sampling without guidance, the zero-scale steps of a guided run), by precision:
  //   >= 1: the LayerNorm output enters FFN-UP as an fp16 hi + lo pair (x_h16 + x_lo: that GEMM sweeps its weight twice, K = 2d).  Rounds 3-4 did the
  //         same in QKV; over configs[1]'s three reference runs + the trained-like one (348 160 positions) the QKV sweep buys nothing -- 153 mismatches
  //         with both, 158 with FFN-up alone, 192 with QKV alone, 195 with neither (profiles/raw/r05/xlo_mask.log) -- and costs 19-69 us per layer;
  //         by layer range (FFN-up sweep; configs[1]'s three runs, 261 120 positions; raw/r05/xlo_layers.log): [0, 24) 144, [6, 24) 140, [12, 24) 147,
  //         [18, 24) 145, [0, 12) 164, none 182 -- the late layers carry all of it, so the sweep runs in layers >= depth / 2 (~80 us per layer saved
  //         in the first half at 64 sequences; the same rule as precision 3's activation-lo set in the guided forward);
  //   >= 2: all four trunk GEMMs also carry the MX-fp4 weight-correction mini-tiles on every row -- the fp16 rounding of the
  //         WEIGHTS is 80 % of the sampled-logit error variance here (tests/diag/error_budget.py: rms 0.0082 single fp16, 0.0073 with hi + lo
  //         activation pairs, 0.0045 with the weight correction alone); both together: 5.3e-4 over configs[1]'s three reference runs.
  const bool xlo = c.precision >= 1;
  const bool wm = g->mini_ok && c.precision >= 2;   // (sequence tiles: 256 + 1 rows, or four tiles per 1024 + 1-row sequence)
  // Both coverage rules above (FFN-up only, late layers only) were measured WITH the weight correction on, on shapes the mini-tiles serve.  Shapes they
  // do not serve (other widths, heads of 32, sequences other than 256 / 1024 tokens) have no weight correction to carry the margin: there the hi + lo
  // LayerNorm outputs enter QKV and FFN-up of EVERY layer, as in rounds 3-4 (round-5 advice: the narrowed rule was a silent regression for them).
  const bool xlo_all = xlo && !wm;
  auto xlo_layer = [&](int l) { return xlo && (xlo_all || 2 * l + 1 >= c.depth); };   // (with the correction: the second half of the layers, see above)
  h16* const xlo_ffn = xlo ? g->x_lo : nullptr;          // the LayerNorm in front of FFN-up writes lo halves (the one in front of QKV only without the correction; the last one feeds the head)
  h16* const xlo_qkv = xlo_all ? g->x_lo : nullptr;
  // the LayerNorms write the MX-fp4 copy (+ scale bytes) only when a GEMM of THIS forward reads it (the buffers also exist for the pair forward)
  Fp4Rows f4x;
  if (wm) { f4x.x4 = g->x4.v; f4x.x4s = g->x4.s; f4x.nseq = nb; f4x.seq_rows = N; }
  auto lo_set = [&](GemmArgs& ga, const uint8_t* a4, const uint8_t* a4s, int widx) {
    if (!wm) return;
    ga.nlo = 1; ga.lo[0] = {a4, a4s, g->w4lo[widx], g->w4los[widx]};
  };
  // QKV / FFN-up: consume the LayerNorm output
  auto xgemm = [&](GemmEpi epi, const h16* W, const float* bias, h16* out, int Nout, int widx) {
    GemmArgs ga{g->x_h16, W, bias, nullptr, nullptr, out, M, Nout, d, 0};
    if (wm) ga.seq_rows = N;
    lo_set(ga, g->x4.v, g->x4.s, widx);
    if (wm && epi == EPI_GELU_H16) { ga.out4 = g->h4.v; ga.out4_scale = g->h4.s; }
    if (((widx & 3) == 2 || xlo_all) && xlo_layer(widx >> 2)) { ga.K = 2 * d; ga.A2 = g->x_lo; ga.kw = d; }   // FFN-up only with the correction (see above)
    ga.sat = g->sat;
    ga.reverse = walk_next();
    gemm_rc |= gemm_tn(s, epi, ga, wm ? 257 : 0);
  };
  // out-proj / FFN-down: + residual (prev: the LayerNorm whose output is the residual, re-derived from the row statistics; null: the buffer's own rows)
  auto rgemm = [&](const h16* A, const h16* W, const float* bias, int K, int widx, const uint8_t* a4, const uint8_t* a4s, const float* ln_g, const float* ln_b) {
    GemmArgs ga{A, W, bias, g->y_f32, g->y_f32, nullptr, M, d, K, 0};
    if (ln_g) { ga.ln_stats = g->ln_stats; ga.ln_g = ln_g; ga.ln_b = ln_b; }
    if (wm) ga.seq_rows = N;
    lo_set(ga, a4, a4s, widx);
    ga.reverse = walk_next();
    gemm_rc |= gemm_tn(s, EPI_RES_F32, ga, wm ? 257 : 0);
  };
  {
    ProfScope p("embed_ln", s, true);
    EmbedArgs e{tokens, labels, drop, g->w_in, g->b_in, g->class_emb, g->pos, g->ln0g, g->ln0b,
                g->y_f32, g->x_h16, nb, c.seq, c.splits, g->gbits, d, c.nclass, g->tables};
    e.x_lo = c.depth ? (c.prenorm ? nullptr : xlo_qkv) : g->x_lo;
    e.f4 = f4x;
    embed_ln(s, e);
  }
  for (int l = 0; l < c.depth; ++l) {
    const mb_gen::Layer& L = g->layers[l];
    // post-norm (every shipped config): the fp32 residual stream lives in ONE buffer, y_f32, holding pre-LayerNorm rows; a LayerNorm writes only the
    // fp16 GEMM operand and {mean, rstd}, the next residual GEMM re-derives the normalised rows in its epilogue and updates y_f32 in place (layer 0's
    // first residual is the embedding LayerNorm output, stored as is by embed_ln).  use_prenorm (bert.py:49-59, 106-123): x = x + Attn(LN(x));
    // x = x + FFN(LN(x)): the buffer holds x itself, every LayerNorm only produces the GEMM operand, the residual GEMMs add the buffer's own rows.
    if (c.prenorm) { ProfScope p("layernorm", s, true); layernorm_rows(s, g->y_f32, L.ln1g, L.ln1b, 1e-12f, nullptr, g->x_h16, nullptr, M, d, xlo_qkv, f4x, walk_next(), N); }
    { ProfScope p("gemm_qkv", s, true); xgemm(EPI_H16, L.wqkv, L.bqkv, g->qkv, 3 * d, 4 * l); }
    { ProfScope p("attention", s, true); attention(s, g->qkv, g->att, nb, N, d, c.heads, wm ? g->att4.v : nullptr, wm ? g->att4.s : nullptr, walk_next()); }
    attn_rc |= attn_maps(l);
    { ProfScope p("gemm_attn_out", s, true);
      const bool re = !c.prenorm && l > 0;
      rgemm(g->att, L.wo, L.bo, d, 4 * l + 1, g->att4.v, g->att4.s, re ? g->layers[l - 1].ln2g : nullptr, re ? g->layers[l - 1].ln2b : nullptr); }
    { ProfScope p("layernorm", s, true);
      layernorm_rows(s, g->y_f32, c.prenorm ? L.ln2g : L.ln1g, c.prenorm ? L.ln2b : L.ln1b, 1e-12f, nullptr, g->x_h16, c.prenorm ? nullptr : g->ln_stats, M, d, xlo_layer(l) ? xlo_ffn : nullptr, f4x, walk_next(), N); }
    { ProfScope p("gemm_ffn_up", s, true); xgemm(EPI_GELU_H16, L.w1, L.b1, g->h, f, 4 * l + 2); }
    { ProfScope p("gemm_ffn_down", s, true);
      rgemm(g->h, L.w2, L.b2, f, 4 * l + 3, g->h4.v, g->h4.s, c.prenorm ? nullptr : L.ln1g, c.prenorm ? nullptr : L.ln1b); }
    if (!c.prenorm) { ProfScope p("layernorm", s, true);
      const bool last = l + 1 == c.depth;                  // the last one feeds the head: plain hi + lo rows
      layernorm_rows(s, g->y_f32, L.ln2g, L.ln2b, 1e-12f, nullptr, g->x_h16, g->ln_stats, M, d, last ? g->x_lo : xlo_qkv, last ? Fp4Rows{} : f4x, walk_next(), N); }
  }
  if (c.prenorm) { ProfScope p("layernorm", s, true); layernorm_rows(s, g->y_f32, g->lnag, g->lnab, 1e-12f, nullptr, g->x_h16, nullptr, M, d, g->x_lo, Fp4Rows{}, walk_next(), N); }   // norm_after_transformer
  gemm_rc |= head_gemms(g, logits, M, s);
  if (int rc = launched()) return rc;
  if (attn_rc) return fail(-3, "attention maps: head dim %d / %d tokens not supported", d / c.heads, N);
  if (gemm_rc) return fail(-3, "a trunk GEMM of this forward (%d sequences x %d tokens, hidden %d, mlp %d; precision %d%s) is outside the half-tile "
                               "kernel's shapes: its correction mini-tiles cannot run", nb, N, d, f, c.precision, wm ? ", weight-correction mini-tiles" : "");
  return 0;
}

// Differential CFG forward (mb_gen_cfg.precision >= 1): nb = 2 * B sequences laid out [B conditional | B label-dropped twins] in every buffer.
// Wherever a fp16 GEMM operand is produced (embedding LayerNorm, the LayerNorms, attention output, GELU output), the conditional rows hold
// fp16(x_c) and the unconditional rows the DIFFERENCE fp16(x_u - x_c); the pair GEMM (gemm_ht.hip, PAIR) adds the two products for the
// unconditional outputs.  The fp32 residual stream, qkv and the logits hold ordinary values for both streams.  wmode: MX-fp4 correction
// pass for the fp16 rounding of the QKV / FFN-up weights (conditional rows; the unconditional outputs inherit it through acc_c).
int gen_forward_pair_impl(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, int B, bool wmode, hipStream_t s) {
  using namespace mb;
  const mb_gen_cfg& c = g->c;
  const int d = c.hidden, f = c.mlp, N = g->N, nb = 2 * B, M = nb * N, P = B * N;
  int rc = 0;
  int wdir = 0;                                         // the direction bit of this forward: see gen_forward_impl
  auto walk_next = [&] { wdir ^= g->walk; return wdir; };
  // measured (profiles/r03_parity.md): the correction pass in layers >= depth / 2 alone buys about 60 % of the gain on the 12-bit runs for half of
  // the cost and next to nothing on the 14-bit one (and per GEMM type no subset is a cheaper "precise": section 5 there) -- so it runs on every GEMM
  // of every layer
  // The activation-lo sets of precision >= 3.  Rounds 4-5 knew the LayerNorm outputs' set only: over FOUR 14-bit / 256-step reference runs (1 002 744
  // positions; profiles/r05_coverage.md) QKV + FFN-up in all layers 496 mismatches, FFN-up alone 491-493, QKV alone 555, neither 625 -- the QKV set buys
  // nothing --, and round 5 ran it in FFN-up of the layers >= depth / 2 (531).
  // Round 6 (DESIGN.md "Precision"): the activation-lo set beyond the LayerNorm outputs -- the lo halves of the attention outputs (out-proj) and of the FFN
  // hiddens (FFN-down), each as e2m1 with per-(row, 64 columns) scales against e2m1 of the fp16 weight, in every layer: precision 3 = out-proj + FFN-up,
  // precision 4 (what heavy-tailed checkpoints need) = + FFN-down.  With exact weights the fp16 rounding of those three operands alone costs 7e-4 of
  // token mismatch on the early steps of a trained-like run (a third each); emulated on that run (tests/diag/error_budget.py EB_STUDY=r6): rms error
  // of the sampled logits' top-2 gap 0.0062 -> 0.0031 with the three sets (and the per-(row, 128 columns) weight-error scales).
  // (which GEMMs: mb_gen::alo_mask -- bit 0 QKV, 1 out-proj, 2 FFN-up, 3 FFN-down)
  auto alo_on = [&](int gemm) { return wmode && c.precision >= 3 && ((g->alo_mask >> gemm) & 1); };
  auto f4_for = [&](bool feeds_ffn = false) {   // what the producer of a LayerNorm operand also writes
    Fp4Rows f;
    if (wmode) {
      f.x4 = g->x4.v; f.x4s = g->x4.s; f.nseq = B; f.seq_rows = N;
      if (alo_on(feeds_ffn ? 2 : 0)) { f.xl4 = g->xl4.v; f.xl4s = g->xl4.s; }   // (the lo halves' e2m1 copy: only the LayerNorm in front of a GEMM that carries the set)
    }
    return f;
  };
  // lo: 0 = fp16 only, 1 = weight-correction mini-tiles (a4 / a4s = e2m1 of the conditional operand values), 2 = + the activation-lo set (al4 / al4s = e2m1
  // of the operand's lo halves, against e2m1 of the fp16 weight)
  auto pgemm = [&](GemmEpi epi, const h16* A, const h16* W, const float* bias, h16* out16, float* res, int Nout, int K, int widx, int lo,
                   const uint8_t* a4 = nullptr, const uint8_t* a4s = nullptr, const uint8_t* al4 = nullptr, const uint8_t* al4s = nullptr) {
    GemmArgs ga{A, W, bias, res, res, out16, M, Nout, K, 0};
    ga.pair_rows = P;
    ga.seq_rows = N;
    if (epi != EPI_RES_F32) ga.sat = g->sat;
    if (lo) {
      ga.nlo = lo; ga.lo[0] = {a4, a4s, g->w4lo[widx], g->w4los[widx]};
      if (lo == 2) ga.lo[1] = {al4, al4s, g->w4[widx], g->w4s[widx]};
    }
    ga.reverse = walk_next();                           // (every pgemm is launched where it is built)
    return ga;
  };
  {
    ProfScope p("embed_ln", s, true);
    // (tokens / labels / drop are laid out [B conditional | B twins]; the twins repeat the conditional tokens and labels with the drop flag set)
    EmbedArgs e{tokens, labels, nullptr, g->w_in, g->b_in, g->class_emb, g->pos, g->ln0g, g->ln0b,
                g->y_f32, g->x_h16, B, c.seq, c.splits, g->gbits, d, c.nclass, g->tables};
    e.f4 = f4_for();
    if (embed_pair(s, e)) {         // shapes the fused kernel does not serve: the two-kernel path
      e.drop = drop; e.nb = nb; e.f4 = Fp4Rows{};
      embed_ln(s, e);
      rc |= pairify_rows(s, g->y_f32, g->x_h16, P, d, f4_for(), walk_next(), N);        // y_f32 holds the embedding LayerNorm's fp32 rows here
    }
  }
  // pre-norm: the first sub-layer normalises the embedding rows again (LayerNorm 1 of layer 0); post-norm: the embedding's own pair operands feed QKV
  if (c.prenorm && c.depth > 0) {
    ProfScope p("layernorm", s, true);
    rc |= layernorm_pair(s, g->y_f32, g->layers[0].ln1g, g->layers[0].ln1b, 1e-12f, g->x_h16, nullptr, P, d, f4_for(), walk_next(), N);
  }
  for (int l = 0; l < c.depth; ++l) {
    const mb_gen::Layer& L = g->layers[l];
    const int xlo_mode = wmode ? (alo_on(2) ? 2 : 1) : 0;
    { ProfScope p("gemm_qkv", s, true);
      GemmArgs ga = pgemm(EPI_H16, g->x_h16, L.wqkv, L.bqkv, g->qkv, nullptr, 3 * d, d, 4 * l, wmode ? (alo_on(0) ? 2 : 1) : 0, g->x4.v, g->x4.s, g->xl4.v, g->xl4.s);
      rc |= gemm_tn(s, EPI_H16, ga, 257); }
    const bool lo_o = alo_on(1), lo_h = alo_on(3);      // the producers also write the lo halves' e2m1 copies for a consumer that carries the set
    { ProfScope p("attention", s, true); rc |= attention_pair(s, g->qkv, g->att, B, N, d, c.heads, wmode ? g->att4.v : nullptr, wmode ? g->att4.s : nullptr,
                                                              lo_o ? g->attl4.v : nullptr, lo_o ? g->attl4.s : nullptr, walk_next()); }
    { ProfScope p("gemm_attn_out", s, true);
      GemmArgs ga = pgemm(EPI_RES_F32, g->att, L.wo, L.bo, nullptr, g->y_f32, d, d, 4 * l + 1, wmode ? (alo_on(1) ? 2 : 1) : 0, g->att4.v, g->att4.s, g->attl4.v, g->attl4.s);
      if (l > 0 && !c.prenorm) { ga.ln_stats = g->ln_stats; ga.ln_g = g->layers[l - 1].ln2g; ga.ln_b = g->layers[l - 1].ln2b; }
      rc |= gemm_tn(s, EPI_RES_F32, ga, 257); }
    // post-norm: LayerNorm 1 follows the attention block; pre-norm: LayerNorm 2 precedes the FFN (same place in the launch order, other parameters;
    // the stream buffer then holds the raw residual and no GEMM re-derives a LayerNorm from the statistics)
    { ProfScope p("layernorm", s, true);
      rc |= layernorm_pair(s, g->y_f32, c.prenorm ? L.ln2g : L.ln1g, c.prenorm ? L.ln2b : L.ln1b, 1e-12f, g->x_h16, c.prenorm ? nullptr : g->ln_stats, P, d, f4_for(true), walk_next(), N); }
    { ProfScope p("gemm_ffn_up", s, true);
      GemmArgs ga = pgemm(EPI_GELU_H16, g->x_h16, L.w1, L.b1, g->h, nullptr, f, d, 4 * l + 2, xlo_mode, g->x4.v, g->x4.s, g->xl4.v, g->xl4.s);
      if (wmode) { ga.out4 = g->h4.v; ga.out4_scale = g->h4.s; }
      if (lo_h) { ga.out4l = g->hl4.v; ga.out4l_scale = g->hl4.s; }
      rc |= gemm_tn(s, EPI_GELU_H16, ga, 257); }
    { ProfScope p("gemm_ffn_down", s, true);
      GemmArgs ga = pgemm(EPI_RES_F32, g->h, L.w2, L.b2, nullptr, g->y_f32, d, f, 4 * l + 3, wmode ? (alo_on(3) ? 2 : 1) : 0, g->h4.v, g->h4.s, g->hl4.v, g->hl4.s);
      if (!c.prenorm) { ga.ln_stats = g->ln_stats; ga.ln_g = L.ln1g; ga.ln_b = L.ln1b; }
      rc |= gemm_tn(s, EPI_RES_F32, ga, 257); }
    { ProfScope p("layernorm", s, true);
      if (c.prenorm) {            // the next layer's LayerNorm 1 (bert.py:49-59, 106-123), or norm_after_transformer in front of the head
        if (l + 1 == c.depth) layernorm_rows(s, g->y_f32, g->lnag, g->lnab, 1e-12f, nullptr, g->x_h16, nullptr, M, d, g->x_lo, Fp4Rows{}, walk_next(), N);
        else rc |= layernorm_pair(s, g->y_f32, g->layers[l + 1].ln1g, g->layers[l + 1].ln1b, 1e-12f, g->x_h16, nullptr, P, d, f4_for(), walk_next(), N);
      }
      else if (l + 1 == c.depth) layernorm_rows(s, g->y_f32, L.ln2g, L.ln2b, 1e-12f, nullptr, g->x_h16, g->ln_stats, M, d, g->x_lo, Fp4Rows{}, walk_next(), N);   // feeds the head: plain hi (+ lo) rows
      else rc |= layernorm_pair(s, g->y_f32, L.ln2g, L.ln2b, 1e-12f, g->x_h16, g->ln_stats, P, d, f4_for(), walk_next(), N); }
  }
  rc |= head_gemms(g, logits, M, s);
  if (int lrc = launched()) return lrc;
  if (rc) return fail(-3, "differential CFG forward: a kernel refused the shape (%d pairs x %d tokens, hidden %d, mlp %d)", B, N, d, f);
  return 0;
}

// The fp32 reference forward (precision MB_PREC_F32): the straight chain embed -> depth x (QKV, attention, out-proj + residual, LayerNorm, FFN-up + GELU,
// FFN-down + residual, LayerNorm) -> head, every operand, product and sum in fp32 (gemm_f32.hip: each GEMM output is one ascending-k fmaf chain).
// Post-norm: x_f32 holds the LayerNorm output -- the next GEMM's operand and the residual that GEMM's successor adds --, y_f32 the pre-LayerNorm sum.
// Pre-norm: y_f32 holds the stream x itself (the residual GEMMs add in place), x_f32 the LayerNorm output that feeds a GEMM.
int gen_forward_f32_impl(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, int nb, hipStream_t s) {
  using namespace mb;
  const mb_gen_cfg& c = g->c;
  const int d = c.hidden, f = c.mlp, N = g->N, M = nb * N;
  int rc = 0;
  auto gemm = [&](int epi, const float* A, const float* W, const float* bias, const float* res, float* out, int Nout, int K) {
    GemmF32Args ga{epi, A, W, bias, res, out, M, Nout, K};
    rc |= gemm_f32(s, ga);
  };
  auto ln = [&](const float* gamma, const float* beta) {
    ProfScope p("layernorm", s, true);
    layernorm_rows(s, g->y_f32, gamma, beta, 1e-12f, g->x_f32, nullptr, nullptr, M, d);
  };
  float* const stream = c.prenorm ? g->y_f32 : g->x_f32;     // what the residual GEMMs add
  {
    ProfScope p("embed_ln", s, true);
    EmbedArgs e{tokens, labels, drop, g->w_in, g->b_in, g->class_emb, g->pos, g->ln0g, g->ln0b,
                stream, nullptr, nb, c.seq, c.splits, g->gbits, d, c.nclass, g->tables};
    embed_ln(s, e);
  }
  for (int l = 0; l < c.depth; ++l) {
    const mb_gen::Layer& L = g->layers[l];
    const mb_gen::Layer32& W = g->layers32[l];
    if (c.prenorm) ln(L.ln1g, L.ln1b);
    { ProfScope p("gemm_qkv", s, true); gemm(F32_EPI_PLAIN, g->x_f32, W.wqkv, L.bqkv, nullptr, g->qkv32, 3 * d, d); }
    { ProfScope p("attention", s, true); rc |= attention_f32(s, g->qkv32, g->att32, nb, N, d, c.heads); }
    { ProfScope p("gemm_attn_out", s, true); gemm(F32_EPI_RES, g->att32, W.wo, L.bo, stream, g->y_f32, d, d); }
    ln(c.prenorm ? L.ln2g : L.ln1g, c.prenorm ? L.ln2b : L.ln1b);
    { ProfScope p("gemm_ffn_up", s, true); gemm(F32_EPI_GELU, g->x_f32, W.w1, L.b1, nullptr, g->h32, f, d); }
    { ProfScope p("gemm_ffn_down", s, true); gemm(F32_EPI_RES, g->h32, W.w2, L.b2, stream, g->y_f32, d, f); }
    if (!c.prenorm) ln(L.ln2g, L.ln2b);
  }
  if (c.prenorm) ln(g->lnag, g->lnab);                       // norm_after_transformer
  // the head (bert.py:411-417, 500-503): last_layer.0 + GELU, LayerNorm, prediction layer
  { ProfScope p("gemm_head", s, true); gemm(F32_EPI_GELU, g->x_f32, g->wl32, g->bl, nullptr, g->y_f32, d, d); }
  ln(g->lnhg, g->lnhb);
  { ProfScope p("gemm_head", s, true);
    GemmF32Args ga{F32_EPI_LOGITS, g->x_f32, g->wp32, c.embed_tables ? g->bias_pos : g->bp, nullptr, logits, M, c.splits * g->C, d, N, c.embed_tables};
    rc |= gemm_f32(s, ga); }
  if (int lrc = launched()) return lrc;
  if (rc) return fail(-3, "fp32 reference forward: a kernel refused the shape (%d sequences x %d tokens, hidden %d, heads %d, mlp %d)", nb, N, d, c.heads, f);
  return 0;
}

// One pass over nb <= chunk_seqs sequences: the fp32 reference chain at precision MB_PREC_F32 -- decided here, in front of every precision >= n test of
// the fp16 schedules --, gen_forward_impl otherwise (attn: that schedule's attention maps; mb_gen_forward_attn refuses the fp32 mode itself)
int gen_forward_pass(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, int nb, hipStream_t s, float* attn = nullptr) {
  if (g->f32) return gen_forward_f32_impl(g, tokens, labels, drop, logits, nb, s);
  return gen_forward_impl(g, tokens, labels, drop, logits, nb, s, attn);
}

// The kernels index with 32-bit element / byte offsets (rows * mlp * 4 < 2^32): forwards over more sequences than that allows run as
// independent chunks (sequences never interact), which also bounds the workspace of very large batches.
int gen_forward(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, int nb, hipStream_t s,
                float* attn = nullptr) {
  const int chunk = g->chunk_seqs;
  g_prof.begin_forward(true);
  if (nb <= chunk) return gen_forward_pass(g, tokens, labels, drop, logits, nb, s, attn);
  if (attn) return fail(-3, "attention maps are limited to %d sequences per call", chunk);
  const size_t P = (size_t)g->c.seq * g->c.splits;
  for (int b0 = 0; b0 < nb; b0 += chunk) {
    const int nc = nb - b0 < chunk ? nb - b0 : chunk;
    int rc = gen_forward_pass(g, tokens + (size_t)b0 * P, labels + b0, drop ? drop + b0 : nullptr, logits + (size_t)b0 * P * g->C, nc, s);
    if (rc) return rc;
  }
  return 0;
}

// Guided forward (sampling.py:83-88) over B samples: logits rows [0, B) conditional, [B, 2B) label-dropped.
int gen_forward_cfg(mb_gen* g, const int64_t* tokens, const int64_t* labels, float* logits, int B, hipStream_t s) {
  const size_t P = (size_t)g->c.seq * g->c.splits;
  const bool pair = !g->f32 && g->pair_ok && g->c.precision >= 1;   // (the fp32 reference mode: the plain forward over [cond | dropped])
  const bool wmode = pair && g->c.precision >= 2;       // weight-rounding correction pass (every step: weight rounding costs parity late in the run too)
  const int chunk = g->chunk_seqs / 2;                  // pairs per pass
  if (chunk < 1) return fail(-1, "engine holds %d sequences: too few for a guided forward", g->chunk_seqs);
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nc = B - b0 < chunk ? B - b0 : chunk;
    HIP_TRY(hipMemcpyAsync(g->tok_cfg, tokens + (size_t)b0 * P, nc * P * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    // (the fused pair embedding reads the conditional tokens only: the twins' copy is needed by the two-kernel path and the plain fallback)
    if (!(pair && !g->c.embed_tables && g->c.bits <= 24))
      HIP_TRY(hipMemcpyAsync(g->tok_cfg + nc * P, tokens + (size_t)b0 * P, nc * P * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (!(nc == B && g->run.cfg_labels == labels && g->run.cfg_B == B)) {       // (the sampling loop marks them ready for the steps of one call)
      g->run.cfg_labels = nullptr;                      // whatever they were marked ready for is overwritten: a session's mark outlives its call
      HIP_TRY(hipMemcpyAsync(g->lab_cfg, labels + b0, nc * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(g->lab_cfg + nc, labels + b0, nc * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemsetAsync(g->drop_cfg, 0, nc, s));
      HIP_TRY(hipMemsetAsync(g->drop_cfg + nc, 1, nc, s));
    }
    float* out = (nc == B) ? logits : g->logits_tmp;    // chunked: through a buffer of the engine's own, then to the two halves of the caller's
    if (b0 == 0) g_prof.begin_forward(false);           // one guided forward = all of its chunks
    int rc = pair ? gen_forward_pair_impl(g, g->tok_cfg, g->lab_cfg, g->drop_cfg, out, nc, wmode, s)
                  : gen_forward_pass(g, g->tok_cfg, g->lab_cfg, g->drop_cfg, out, 2 * nc, s);
    if (rc) return rc;
    if (nc != B) {
      HIP_TRY(hipMemcpyAsync(logits + (size_t)b0 * P * g->C, out, nc * P * g->C * sizeof(float), hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(logits + (size_t)(B + b0) * P * g->C, out + (size_t)nc * P * g->C, nc * P * g->C * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
  }
  return 0;
}

}  // namespace

extern "C" {

int mb_abi_version(void) { return MB_ABI_VERSION; }
const char* mb_last_error(void) { return mb::g_err.c_str(); }

int mb_prof_enable(int on) {
  if (!on) g_prof.drain();
  g_prof.on = on != 0;
  if (on) { g_prof.acc.clear(); g_prof.stride = on; g_prof.tick[0] = g_prof.tick[1] = 0; }
  return 0;
}
int mb_prof_read(char* buf, int buflen) {
  g_prof.drain();
  std::string out;
  char line[256];
  for (auto& kv : g_prof.acc) {
    snprintf(line, sizeof line, "%s %ld %.6f\n", g_prof.names[kv.first].c_str(), kv.second.first, kv.second.second);
    out += line;
  }
  if ((int)out.size() + 1 > buflen) return fail(-3, "mb_prof_read: buffer too small (%zu needed)", out.size() + 1);
  memcpy(buf, out.c_str(), out.size() + 1);
  return (int)out.size();
}

int mb_gen_create(const mb_gen_cfg* cfg, int max_seqs, mb_gen** out) {
  if (!cfg || !out || max_seqs <= 0) return fail(-1, "mb_gen_create: bad arguments");
  const mb_gen_cfg& c = *cfg;
  if (c.splits <= 0 || c.bits % c.splits) return fail(-1, "bits (%d) must be divisible by splits (%d)", c.bits, c.splits);
  if (c.bits > 24) return fail(-1, "bits > 24 is not supported");
  if (c.hidden % 64 || c.mlp % 64) return fail(-1, "hidden (%d) and mlp (%d) must be multiples of 64", c.hidden, c.mlp);
  if (c.hidden > 2048) return fail(-1, "hidden > 2048 is not supported");
  const int dh = c.heads > 0 ? c.hidden / c.heads : 0;
  if (c.heads <= 0 || c.hidden % c.heads || (dh != 32 && dh != 64)) return fail(-1, "hidden/heads must be 32 or 64 (got %d)", dh);
  if (c.seq < 1 || c.seq > 4096) return fail(-1, "seq = %d outside [1, 4096]", c.seq);   // > 287 or < 255 tokens: streaming attention kernel
  if ((size_t)c.seq * c.splits > 8192) return fail(-1, "seq * splits = %zu exceeds the step kernel's 8192 positions", (size_t)c.seq * c.splits);
  const int C = 1 << (c.bits / c.splits);
  if (C > 4096 || (c.splits * C) % 4) return fail(-1, "unsupported group codebook size %d (the fused step kernel holds up to 4096 codes per group)", C);
  if ((c.prenorm != 0 && c.prenorm != 1) || (c.embed_tables != 0 && c.embed_tables != 1)) return fail(-1, "prenorm / embed_tables must be 0 or 1");
  if (c.embed_tables && c.splits > 8) return fail(-1, "embed_tables supports up to 8 token groups");
  if (c.precision < 0 || c.precision > MB_PREC_F32) return fail(-1, "precision must be 0 .. 5 (MB_PREC_FP16 / _DIFF / _WCORR / _ALO / _ALO_ALL / _F32)");
  const bool f32 = c.precision == MB_PREC_F32;          // the fp32 reference mode: every configuration accepted above, fp32 weights and workspace only
  mb_gen* g = new mb_gen();
  g->f32 = f32;
  g->c = c; g->max_seqs = max_seqs; g->N = c.seq + 1; g->gbits = c.bits / c.splits; g->C = C;
  (void)hipGetDevice(&g->device);
  // rows per forward pass: 32-bit byte offsets inside the kernels need rows * max(mlp, 3 * hidden) * 4 < 2^32 (gemm_ht_supported)
  const size_t widest = (size_t)(c.mlp > 3 * c.hidden ? c.mlp : 3 * c.hidden);
  const size_t max_rows = ((1ull << 32) - 1) / (4 * widest);
  g->chunk_seqs = (int)std::min<size_t>((size_t)max_seqs, std::max<size_t>(1, max_rows / g->N));
  const size_t d = c.hidden, f = c.mlp, M = (size_t)g->chunk_seqs * g->N;
  mb::DevArena& m = g->mem;
  g->layers.resize(c.depth);
  if (f32) g->layers32.resize(c.depth);
  else m.get(&g->split_tmp, 1);
  m.zeroed(&g->sat, 1);                                 // (the fp32 mode has no fp16 store to clamp: the count stays 0)
  for (int l = 0; l < c.depth; ++l) {
    mb_gen::Layer& L = g->layers[l];
    if (f32) { mb_gen::Layer32& W = g->layers32[l]; m.get(&W.wqkv, 3 * d * d); m.get(&W.wo, d * d); m.get(&W.w1, f * d); m.get(&W.w2, d * f); }
    else { m.get(&L.wqkv, 3 * d * d); m.get(&L.wo, d * d); m.get(&L.w1, f * d); m.get(&L.w2, d * f); }
    m.get(&L.bqkv, 3 * d); m.get(&L.bo, d); m.get(&L.b1, f); m.get(&L.b2, d);
    m.get(&L.ln1g, d); m.get(&L.ln1b, d); m.get(&L.ln2g, d); m.get(&L.ln2b, d);
  }
  m.get(&g->w_in, d * c.bits); m.get(&g->b_in, d);
  if (c.prenorm) { m.get(&g->lnag, d); m.get(&g->lnab, d); }
  if (c.embed_tables) { m.get(&g->tables, (size_t)c.splits * (C + 1) * d); m.get(&g->bias_pos, (size_t)c.seq * c.splits * C); }
  m.get(&g->class_emb, (size_t)(c.nclass + 1) * d); m.get(&g->pos, (size_t)g->N * d);
  m.get(&g->ln0g, d); m.get(&g->ln0b, d);
  m.get(&g->bl, d); m.get(&g->lnhg, d); m.get(&g->lnhb, d); m.get(&g->bp, (size_t)c.splits * C);
  m.get(&g->y_f32, M * d);
  if (f32) {
    m.get(&g->wl32, d * d); m.get(&g->wp32, (size_t)c.splits * C * d);
    m.get(&g->x_f32, M * d); m.get(&g->qkv32, M * 3 * d); m.get(&g->att32, M * d); m.get(&g->h32, M * f);
  } else {
    m.get(&g->wl, d * d); m.get(&g->wl_lo, d * d);
    m.get(&g->wp, (size_t)c.splits * C * d); m.get(&g->head_scale, 2);
    if (!c.embed_tables) m.get(&g->wp_lo, (size_t)c.splits * C * d);
    m.get(&g->ln_stats, M * 2); m.get(&g->x_h16, M * d);
    m.get(&g->x_lo, M * d);   // lo halves of the LayerNorm outputs: always for the head GEMMs, precision >= 1 for QKV / FFN-up of plain forwards
    m.get(&g->qkv, M * 3 * d); m.get(&g->att, M * d); m.get(&g->h, M * f);
  }
  // MX-fp4 mini-tile passes (precision 2 / 3): 257- / 1025-token sequences, vector LayerNorm widths, heads of 64 (the attention kernels' e2m1 output), whole mini-tiles
  g->mini_ok = !f32 && c.precision >= 2 && (c.seq == 256 || c.seq == 1024) && (c.hidden == 768 || c.hidden == 1024) && c.mlp % 256 == 0 && c.hidden / c.heads == 64;   // (FFN-up's N = mlp: whole 256-column tiles)
  // differential CFG forward: 257-token sequences (pair tiles = 2 x 128 tokens + the class pair), vector LayerNorm widths, plain fp16 operands
  // (round 5: also the 1024 + 1-token models of 512 x 512 images -- a pair tile is 128 tokens of a sequence pair whatever the sequence length)
  if (c.precision == 3) g->alo_mask = g->alo_mask_built = 6;                 // out-proj + FFN-up, every layer
  if (c.precision == 4) g->alo_mask = g->alo_mask_built = 14;                // + FFN-down
  g->pair_ok = !f32 && c.precision >= 1 && (c.seq == 256 || c.seq == 1024) && (c.hidden == 768 || c.hidden == 1024) && c.mlp % 256 == 0 && g->chunk_seqs >= 2 &&
               (c.precision == 1 || g->mini_ok);
  if (g->mini_ok) {
    const size_t ntok = (size_t)g->chunk_seqs * c.seq;
    alloc_f4(m, &g->x4, M, d, ntok);
    alloc_f4(m, &g->att4, M, d, ntok);
    alloc_f4(m, &g->h4, M, f, ntok);
    if (g->alo_mask_built & 5) alloc_f4(m, &g->xl4, M, d, ntok);
    if (g->alo_mask_built & 2) alloc_f4(m, &g->attl4, M, d, ntok);
    if (g->alo_mask_built & 8) alloc_f4(m, &g->hl4, M, f, ntok);
    g->w4lo.assign((size_t)4 * c.depth, nullptr); g->w4los.assign((size_t)4 * c.depth, nullptr);
    g->w4.assign((size_t)4 * c.depth, nullptr); g->w4s.assign((size_t)4 * c.depth, nullptr);
    // mini-tile-packed e2m1 of the four weights of a layer: half a byte per weight, one scale byte per (weight row, 128 columns)
    const size_t wn[4] = {3 * d * d, d * d, f * d, d * f};
    for (int i = 0; i < 4 * c.depth; ++i) {
      const size_t n = wn[i & 3];
      m.get(&g->w4lo[i], n / 2); m.get(&g->w4los[i], n / 128);
      // e2m1 of the fp16 weight VALUES for the GEMMs that carry an activation-lo set (precision >= 3)
      if ((g->alo_mask_built >> (i & 3)) & 1) { m.get(&g->w4[i], n / 2); m.get(&g->w4s[i], n / 128); }
    }
  }
  const size_t P = (size_t)c.seq * c.splits, B = max_seqs;
  m.get(&g->tok_a, B * P); m.get(&g->tok_b, B * P); m.get(&g->tok_cfg, B * P);
  m.get(&g->pred, B * P); m.get(&g->codes, B * c.seq);
  m.get(&g->lab_cfg, B); m.get(&g->drop_cfg, B); m.get(&g->logits, B * P * C);
  m.get(&g->num_regen, B);
  if (g->chunk_seqs < max_seqs) m.get(&g->logits_tmp, (size_t)g->chunk_seqs * P * C);
  if (int rc = m.failed("mb_gen_create")) { delete g; return rc; }
  *out = g;
  return 0;
}

void mb_gen_destroy(mb_gen* g) { delete g; }

int mb_gen_load(mb_gen* g, const char* name, const float* data, const int64_t* shape, int ndim, mb_stream stream) {
  if (!g || !name || !data) return fail(-1, "mb_gen_load: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  const mb_gen_cfg& c = g->c;
  const size_t d = c.hidden, f = c.mlp;
  size_t numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= (size_t)shape[i];
  float* dst_f = nullptr; h16* dst_h = nullptr; size_t want = 0;
  int wrows = 0, wcols = 0, sidx = -1;                 // GEMM weights: [rows, cols] and their output-scale slot
  int l = -1, sub = -1; char rest[96] = {0};
  std::string n(name);
  // the embedding-table generator (Bert) has neither a bit projection nor an untied prediction layer: those keys belong to LFQBert checkpoints
  if (c.embed_tables && (n.rfind("prediction_layer.", 0) == 0 || n.rfind("input_proj.", 0) == 0))
    return fail(-2, "mb_gen_load: unknown checkpoint entry '%s' (embed_tables engine: tok_emb_list.* / bias.* instead)", name);
  if (sscanf(name, "transformer.layers.%d.%d.%95s", &l, &sub, rest) == 3) {
    if (l < 0 || l >= c.depth) return fail(-2, "layer index out of range in '%s'", name);
    mb_gen::Layer& L = g->layers[l];
    std::string r(rest);
    if (sub == 0) {
      if (r == "mha.in_proj_weight") { dst_h = L.wqkv; want = 3 * d * d; wrows = 3 * d; wcols = d; sidx = 4 * l; }
      else if (r == "mha.in_proj_bias") { dst_f = L.bqkv; want = 3 * d; }
      else if (r == "mha.out_proj.weight") { dst_h = L.wo; want = d * d; wrows = d; wcols = d; sidx = 4 * l + 1; }
      else if (r == "mha.out_proj.bias") { dst_f = L.bo; want = d; }
      else if (r == "norm.weight") { dst_f = L.ln1g; want = d; }
      else if (r == "norm.bias") { dst_f = L.ln1b; want = d; }
    } else if (sub == 1) {
      if (r == "net.0.weight") { dst_h = L.w1; want = f * d; wrows = f; wcols = d; sidx = 4 * l + 2; }
      else if (r == "net.0.bias") { dst_f = L.b1; want = f; }
      else if (r == "net.2.weight") { dst_h = L.w2; want = d * f; wrows = d; wcols = f; sidx = 4 * l + 3; }
      else if (r == "net.2.bias") { dst_f = L.b2; want = d; }
      else if (r == "norm.weight") { dst_f = L.ln2g; want = d; }
      else if (r == "norm.bias") { dst_f = L.ln2b; want = d; }
    }
  } else if (n == "pos_emb") { dst_f = g->pos; want = (size_t)g->N * d; }
  else if (n == "class_emb.weight") { dst_f = g->class_emb; want = (size_t)(c.nclass + 1) * d; }
  else if (n == "input_proj.weight") { dst_f = g->w_in; want = d * c.bits; }
  else if (n == "input_proj.bias") { dst_f = g->b_in; want = d; }
  else if (n == "first_layer.0.weight") { dst_f = g->ln0g; want = d; }
  else if (n == "first_layer.0.bias") { dst_f = g->ln0b; want = d; }
  else if (n == "last_layer.0.weight") { dst_h = g->wl; want = d * d; wrows = d; wcols = d; sidx = 4 * c.depth; }
  else if (n == "last_layer.0.bias") { dst_f = g->bl; want = d; }
  else if (n == "last_layer.2.weight") { dst_f = g->lnhg; want = d; }
  else if (n == "last_layer.2.bias") { dst_f = g->lnhb; want = d; }
  else if (n == "prediction_layer.weight") { dst_h = g->wp; want = (size_t)c.splits * g->C * d; wrows = c.splits * g->C; wcols = d; sidx = 4 * c.depth + 1; }
  else if (n == "prediction_layer.bias") { dst_f = g->bp; want = (size_t)c.splits * g->C; }
  else if (n == "bits_to_indices") return 0;   // derived buffer (bert.py:383-384): recomputed on the device
  else if (c.prenorm && n == "norm_after_transformer.weight") { dst_f = g->lnag; want = d; }
  else if (c.prenorm && n == "norm_after_transformer.bias") { dst_f = g->lnab; want = d; }
  else if (c.embed_tables) {
    int q = -1;
    if (sscanf(name, "tok_emb_list.%d.weight", &q) == 1 && n == "tok_emb_list." + std::to_string(q) + ".weight") {
      // Bert (bert.py:224-226, 329-332): the table is the input embedding (fp32, gathered) AND, rows 0..C-1, the output head
      if (q < 0 || q >= c.splits) return fail(-2, "group index out of range in '%s'", name);
      const size_t rows = (size_t)g->C + 1;
      if (numel != rows * d) return fail(-4, "mb_gen_load: '%s' has %zu elements, expected %zu", name, numel, rows * d);
      HIP_TRY(hipMemcpyAsync(g->tables + (size_t)q * rows * d, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
      if (g->f32) HIP_TRY(hipMemcpyAsync(g->wp32 + (size_t)q * g->C * d, data, (size_t)g->C * d * sizeof(float), hipMemcpyDeviceToDevice, s));   // the tied head: fp32 table rows
      else mb::cast_f32_to_h16(s, data, g->wp + (size_t)q * g->C * d, (size_t)g->C * d);
      g->loaded++;
      return 0;
    }
    if (sscanf(name, "bias.%d", &q) == 1 && n == "bias." + std::to_string(q)) {
      if (q < 0 || q >= c.splits) return fail(-2, "group index out of range in '%s'", name);
      if (numel != (size_t)c.seq * g->C) return fail(-4, "mb_gen_load: '%s' has %zu elements, expected %zu", name, numel, (size_t)c.seq * g->C);
      HIP_TRY(hipMemcpy2DAsync(g->bias_pos + (size_t)q * g->C, (size_t)c.splits * g->C * sizeof(float), data, (size_t)g->C * sizeof(float),
                               (size_t)g->C * sizeof(float), (size_t)c.seq, hipMemcpyDeviceToDevice, s));
      g->loaded++;
      return 0;
    }
  }
  if (g->f32 && sidx >= 0) {                           // a GEMM weight in the fp32 reference mode: kept as the checkpoint's fp32, no repack, no hi / lo planes
    if (sidx < 4 * c.depth) { mb_gen::Layer32& W = g->layers32[sidx >> 2]; float* const w4[4] = {W.wqkv, W.wo, W.w1, W.w2}; dst_f = w4[sidx & 3]; }
    else dst_f = sidx == 4 * c.depth ? g->wl32 : g->wp32;
    dst_h = nullptr;
  }
  if (!dst_f && !dst_h) return fail(-2, "mb_gen_load: unknown checkpoint entry '%s'", name);
  if (numel != want) return fail(-4, "mb_gen_load: '%s' has %zu elements, expected %zu", name, numel, want);
  if (dst_f == g->w_in) mb::transpose_f32(s, data, g->w_in, (int)d, c.bits);       // [d,K] -> [K,d] for the embed kernel
  else if (dst_h && dst_h == g->wl) mb::split_f32_to_h16_planes(s, data, g->wl, g->wl_lo, wrows, wcols, g->head_scale, g->split_tmp);
  else if (dst_h && dst_h == g->wp) mb::split_f32_to_h16_planes(s, data, g->wp, g->wp_lo, wrows, wcols, g->head_scale + 1, g->split_tmp);
  else if (dst_h) {
    mb::cast_f32_to_h16(s, data, dst_h, numel);
    if (g->mini_ok && sidx >= 0 && sidx < 4 * c.depth) {
      mb::w4lo_from_f32(s, data, g->w4lo[sidx], wrows, wcols, g->w4los[sidx]);
      if (g->w4[sidx]) mb::w4_from_f32(s, data, g->w4[sidx], wrows, wcols, g->w4s[sidx]);
    }
  }
  else HIP_TRY(hipMemcpyAsync(dst_f, data, numel * sizeof(float), hipMemcpyDeviceToDevice, s));
  g->loaded++;
  return 0;
}

int mb_gen_set_alo(mb_gen* g, int gemm_mask) {
  if (!g || gemm_mask < 0 || gemm_mask > 15) return fail(-1, "mb_gen_set_alo: mask outside [0, 15]");
  if (gemm_mask & ~g->alo_mask_built)
    return fail(-1, "mb_gen_set_alo: the handle was created (precision %d) with the activation-lo operands of GEMM mask %d only", g->c.precision, g->alo_mask_built);
  g->alo_mask = gemm_mask;
  return 0;
}

int mb_gen_set_walk(mb_gen* g, int mode) {
  if (!g || (mode != 0 && mode != 1)) return fail(-1, "mb_gen_set_walk: mode 0 (every launch front to back) or 1 (alternating)");
  g->walk = mode;
  return 0;
}

int mb_gen_saturation_count(mb_gen* g, unsigned* count, int reset, mb_stream stream) {
  if (!g || !count) return fail(-1, "mb_gen_saturation_count: null argument");
  return mb::read_counter("mb_gen_saturation_count", g->sat, count, reset, (hipStream_t)stream);
}

int mb_gen_forward(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits,
                   int nb, mb_stream stream) {
  if (!g || !tokens || !labels || !logits) return fail(-1, "mb_gen_forward: null argument");
  if (nb <= 0 || nb > g->max_seqs) return fail(-1, "mb_gen_forward: nb=%d outside [1, %d]", nb, g->max_seqs);
  return gen_forward(g, tokens, labels, drop, logits, nb, (hipStream_t)stream);
}

int mb_gen_forward_cfg(mb_gen* g, const int64_t* tokens, const int64_t* labels, float* logits, int B, mb_stream stream) {
  if (!g || !tokens || !labels || !logits) return fail(-1, "mb_gen_forward_cfg: null argument");
  if (B <= 0 || 2 * B > g->max_seqs) return fail(-1, "mb_gen_forward_cfg: B=%d needs %d sequences, engine holds %d", B, 2 * B, g->max_seqs);
  return gen_forward_cfg(g, tokens, labels, logits, B, (hipStream_t)stream);
}

int mb_gen_forward_attn(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, float* attn,
                        int nb, mb_stream stream) {
  if (!g || !tokens || !labels || !logits || !attn) return fail(-1, "mb_gen_forward_attn: null argument");
  if (nb <= 0 || nb > g->max_seqs) return fail(-1, "mb_gen_forward_attn: nb=%d outside [1, %d]", nb, g->max_seqs);
  if (g->f32) return fail(-3, "mb_gen_forward_attn: attention maps are not available in the fp32 reference mode (precision %d)", (int)MB_PREC_F32);
  return gen_forward(g, tokens, labels, drop, logits, nb, (hipStream_t)stream, attn);
}

// One step, from the three step entries and from the loop.  who: the entry's name in the messages; num_regen != null: the edit step, which reads
// mask_ratio instead of a.k_mask_len; a.seeds != null: the seeded step, which generates its noise from (seeds, step, rand_temp, conf_w) instead of
// reading a.exp_noise / a.conf_noise.  a.tokens is tokens_out, a.pred pred_out, a.P = n m (0: n or m was not positive).
static int sample_step_checked(const char* who, const mb::StepArgs& a, const int64_t* tokens_in, const int32_t* num_regen, float mask_ratio, hipStream_t s) {
  if (!a.logits_c || (!a.seeds && (!a.exp_noise || !a.conf_noise)) || !tokens_in || !a.tokens) return fail(-1, "%s: null argument", who);
  if (tokens_in == a.tokens) return fail(-1, "%s: tokens_in and tokens_out must not alias", who);
  if (a.B <= 0 || a.P <= 0 || a.C <= 0) return fail(-1, "%s: bad sizes", who);
  ProfScope p(a.req ? "sample_step_requests" : a.seeds ? "sample_step_seeded" : num_regen ? "sample_step_edit" : "sample_step", s);
  if (mb::sample_step(s, a, tokens_in, num_regen, mask_ratio)) return fail(-1, "%s: C=%d or n*m=%d too large", who, a.C, a.P);
  return launched();
}

static int step_slots(int n, int m) { return n > 0 && m > 0 ? n * m : 0; }

int mb_sample_step(const float* logits_c, const float* logits_u, float scale, float temperature,
                   const float* exp_noise, const float* conf_noise, int k_mask_len, const int64_t* tokens_in,
                   int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C, mb_stream stream) {
  mb::StepArgs a{};
  a.logits_c = logits_c; a.logits_u = logits_u; a.scale = scale; a.temperature = temperature;
  a.exp_noise = exp_noise; a.conf_noise = conf_noise; a.k_mask_len = k_mask_len;
  a.tokens = tokens_out; a.pred = pred_out; a.B = B; a.P = step_slots(n, m); a.C = C;
  return sample_step_checked("mb_sample_step", a, tokens_in, nullptr, 0.f, (hipStream_t)stream);
}

int mb_sample_step_edit(const float* logits_c, const float* logits_u, float scale, float temperature, const float* exp_noise, const float* conf_noise,
                        float mask_ratio, const int32_t* num_regen, const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out, int B, int n, int m,
                        int C, mb_stream stream) {
  if (!num_regen) return fail(-1, "mb_sample_step_edit: null argument");
  mb::StepArgs a{};
  a.logits_c = logits_c; a.logits_u = logits_u; a.scale = scale; a.temperature = temperature;
  a.exp_noise = exp_noise; a.conf_noise = conf_noise;
  a.tokens = tokens_out; a.pred = pred_out; a.B = B; a.P = step_slots(n, m); a.C = C;
  return sample_step_checked("mb_sample_step_edit", a, tokens_in, num_regen, mask_ratio, (hipStream_t)stream);
}

int mb_sample_step_seeded(const float* logits_c, const float* logits_u, float scale, float temperature, const int64_t* seeds, int step,
                          float randomize_temperature, float conf_weight, float mask_ratio, const int32_t* num_regen, const int64_t* tokens_in,
                          int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C, mb_stream stream) {
  if (!seeds || !num_regen) return fail(-1, "mb_sample_step_seeded: null argument");
  if (step < 0) return fail(-1, "mb_sample_step_seeded: step = %d is negative", step);
  if (pred_out && (pred_out == tokens_out || pred_out == tokens_in)) return fail(-1, "mb_sample_step_seeded: pred_out must not alias tokens_in or tokens_out");
  mb::StepArgs a{};
  a.logits_c = logits_c; a.logits_u = logits_u; a.scale = scale; a.temperature = temperature;
  a.seeds = seeds; a.step = step; a.rand_temp = randomize_temperature; a.conf_w = conf_weight;
  a.tokens = tokens_out; a.pred = pred_out; a.B = B; a.P = step_slots(n, m); a.C = C;
  return sample_step_checked("mb_sample_step_seeded", a, tokens_in, num_regen, mask_ratio, (hipStream_t)stream);
}

static_assert(sizeof(mb::RequestStep) == sizeof(mb_request_step) && sizeof(mb_request_step) == 24, "mb_request_step is the kernels' RequestStep");

int mb_sample_step_requests(const float* logits_c, const float* logits_u, const mb_request_step* table_row, const int64_t* seeds, const int32_t* num_regen,
                            const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C, mb_stream stream) {
  if (!table_row || !seeds || !num_regen) return fail(-1, "mb_sample_step_requests: null argument");
  if (pred_out && (pred_out == tokens_out || pred_out == tokens_in)) return fail(-1, "mb_sample_step_requests: pred_out must not alias tokens_in or tokens_out");
  mb::StepArgs a{};
  a.logits_c = logits_c; a.logits_u = logits_u;
  a.seeds = seeds; a.req = (const mb::RequestStep*)table_row;
  a.tokens = tokens_out; a.pred = pred_out; a.B = B; a.P = step_slots(n, m); a.C = C;
  return sample_step_checked("mb_sample_step_requests", a, tokens_in, num_regen, 0.f, (hipStream_t)stream);
}

}  // extern "C"

// ================================================================================================
// whole loop (sampling.py:55-136)
// ================================================================================================
namespace {

// Where a run's noise comes from: the caller's tensors of this chunk's steps (mb_sample, mb_sample_edit), or the samples' seeds (mb_sample_seeded: the
// step kernel generates it; conf_weight = host [num_steps], indexed by the absolute step like the plan's arrays)
struct RunNoise {
  const float* exp_noise = nullptr; const float* conf_noise = nullptr;
  const int64_t* seeds = nullptr; float rand_temp = 0.f; const float* conf_weight = nullptr;
};
// What the three run entries differ in.  mask_len (mb_sample: the run starts all-masked) or mask_ratio (an edit run: the step reads the ratio and the
// per-sample counts the first chunk left in g->num_regen); init_tokens: the tokens an edit run starts from (mb_sample_seeded: may be null = all-masked,
// num_regen[b] = n m); noise.seeds != null: a seeded run.
struct RunSpec {
  const char* who = nullptr;                           // the entry's name in the messages
  int num_steps = 0, use_guidance = 0, step_begin = 0, step_end = 0;
  const float* scale = nullptr; const float* temperature = nullptr;
  const int* mask_len = nullptr; const float* mask_ratio = nullptr;
  const int64_t* init_tokens = nullptr;
  RunNoise noise;
};
struct RunOut { int64_t* step_tokens; int64_t* codes; float* img_nchw; uint8_t* img_nhwc_u8; };   // each may be null

const char* const kRunKind[3] = {"plain", "edit", "seeded"};
const char* const kStepEntry[3] = {"mb_sample_step", "mb_sample_step_edit", "mb_sample_step_seeded"};

// (mb_sample_plan and mb_edit_plan differ in their third array alone)
template <class Plan>
RunSpec run_spec(const char* who, const Plan& p) {
  RunSpec r;
  r.who = who; r.num_steps = p.num_steps; r.use_guidance = p.use_guidance; r.step_begin = p.step_begin; r.step_end = p.step_end;
  r.scale = p.scale; r.temperature = p.temperature;
  return r;
}

// The null checks of the caller's own pointers are the entries'; g and labels are theirs too.
int sample_run(mb_gen* g, mb_dec* d, const RunSpec& r, const int64_t* labels, int B, const RunOut& out, hipStream_t s) {
  const char* who = r.who;
  const RunNoise& nz = r.noise;
  const bool edit = r.mask_ratio != nullptr, seeded = nz.seeds != nullptr;
  const int num_steps = r.num_steps;
  if (!r.scale || !r.temperature || !(edit ? (const void*)r.mask_ratio : (const void*)r.mask_len) || num_steps <= 0) return fail(-1, "%s: incomplete plan", who);
  const mb_gen::Run::Id id{B, num_steps, r.use_guidance != 0, seeded ? 2 : edit ? 1 : 0};
  const int nbf = id.guided ? 2 * B : B;
  if (B <= 0 || nbf > g->max_seqs) return fail(-1, "%s: B=%d needs %d sequences, engine holds %d", who, B, nbf, g->max_seqs);
  if (!d && (out.img_nchw || out.img_nhwc_u8)) return fail(-1, "%s: image requested without a decoder", who);
  const mb_gen_cfg& c = g->c;
  const int n = c.seq, m = c.splits, C = g->C;
  const size_t P = (size_t)n * m;
  // state init (sampling.py:65-71): every position masked; CFG batch = [cond | label-dropped]
  // A run may be fed in step chunks (plan->step_begin / step_end: the noise of a whole 256-step run at batch 100 is 6.7 GB): chunk [0, e) starts from
  // the all-masked state, later chunks continue from the token state the engine kept; exp_noise / conf_noise / step_tokens hold THIS chunk's steps.
  const int s0 = r.step_end > 0 ? r.step_begin : 0, s1 = r.step_end > 0 ? r.step_end : num_steps;
  if (s0 < 0 || s1 > num_steps || s0 >= s1) return fail(-1, "%s: step chunk [%d, %d) outside [0, %d)", who, s0, s1, num_steps);
  // A run fed in chunks keeps its token state in the engine: a chunk is accepted only as the exact continuation of the run in progress (same batch,
  // plan length, guidance flag and kind -- plain, edit or seeded --, beginning where the previous chunk ended).  The handle is not re-entrant while a run is in progress.
  mb_gen::Run& run = g->run;
  if (s0 == 0) {
    if (r.init_tokens) mb::edit_load_tokens(s, r.init_tokens, g->tok_a, g->num_regen, B, (int)P, C);   // the caller's tokens; num_regen[b] = sample b's masked count
    else {
      mb::fill_i64(s, g->tok_a, (int64_t)C, (size_t)B * P);
      if (seeded) mb::edit_load_tokens(s, g->tok_a, nullptr, g->num_regen, B, (int)P, C);          // the per-sample rule from the all-masked state: num_regen[b] = n m
    }
    run.id = id;
  }
  else if (!(run.id == id && run.next == s0))
    return fail(-1, "%s: step chunk [%d, %d) of a %d-step %s run with B = %d does not continue the run in progress (next step %d of %d, B = %d, %s %s run)",
                who, s0, s1, num_steps, kRunKind[id.kind], B, run.next, run.id.steps, run.id.B, run.id.kind == 1 ? "an" : "a", kRunKind[run.id.kind]);
  run.next = -1;                                       // (set again below when this chunk has been enqueued and more follow)
  int64_t* cur = (s0 & 1) ? g->tok_b : g->tok_a;
  int64_t* nxt = (s0 & 1) ? g->tok_a : g->tok_b;
  int64_t* last_pred = g->pred;
  // lab_cfg / drop_cfg are marked ready for the steps of this call only: whichever way it returns
  struct CfgReady { mb_gen::Run& run; ~CfgReady() { run.cfg_labels = nullptr; } } cfg_ready{run};
  run.cfg_labels = nullptr;
  mb::StepArgs a{};
  a.logits_c = g->logits; a.B = B; a.P = (int)P; a.C = C;
  a.seeds = nz.seeds; a.rand_temp = nz.rand_temp;
  for (int i = s0; i < s1; ++i) {
    int rc;
    // sampling.py:98-99 combines c + s_i (c - u).  Where the annealed scale s_i is exactly 0 -- the first steps of the cosine schedule: (i / N)^p pi
    // is below float32's cos() resolution -- the unconditional logits do not enter the result (c + 0 (c - u) == c for finite logits), so that
    // forward is not run: the step is the plain conditional forward, bit for bit what the guided expression evaluates to.
    // (precision 4: the guided forward is also the MORE PRECISE conditional forward -- its pair tiles carry the activation-lo sets, the plain tiles do not --
    // and the first, almost fully masked steps are where near-ties flip: the zero-scale steps run it too; its unconditional half is then multiplied by 0)
    if (id.guided && (r.scale[i] != 0.0f || (!g->f32 && g->pair_ok && c.precision >= 4))) {
      rc = gen_forward_cfg(g, cur, labels, g->logits, B, s);
      a.logits_u = g->logits + (size_t)B * P * C;
      if (B <= g->chunk_seqs / 2) { run.cfg_labels = labels; run.cfg_B = B; }   // lab_cfg / drop_cfg stay valid for the rest of this call
    } else {
      rc = gen_forward(g, cur, labels, nullptr, g->logits, B, s);
      a.logits_u = nullptr;
    }
    if (rc) return rc;
    const size_t k = (size_t)(i - s0);                 // the noise / step_tokens buffers hold this chunk's steps
    a.scale = r.scale[i]; a.temperature = r.temperature[i];
    a.tokens = nxt; a.pred = out.step_tokens ? out.step_tokens + k * B * P : g->pred;
    if (seeded) { a.step = i; a.conf_w = nz.conf_weight[i]; }
    else { a.exp_noise = nz.exp_noise + k * B * P * C; a.conf_noise = nz.conf_noise + k * B * P; }
    if (!edit) a.k_mask_len = r.mask_len[i];
    rc = sample_step_checked(kStepEntry[id.kind], a, cur, edit ? g->num_regen : nullptr, edit ? r.mask_ratio[i] : 0.f, s);
    if (rc) return rc;
    last_pred = a.pred;
    int64_t* t = cur; cur = nxt; nxt = t;
  }
  if (s1 < num_steps) {                                // more chunks follow: keep the last predictions only if they are the engine's own buffer
    if (int rc = launched()) return rc;
    run.next = s1;
    return 0;
  }
  // combine_factorized_tokens (factorization.py:7-24) on the LAST step's predictions, kept as integers
  int64_t* codes = out.codes ? out.codes : g->codes;
  mb::combine_groups(s, last_pred, codes, (size_t)B * n, m, g->gbits);
  if (d) {
    int rc = mb_dec_decode(d, codes, out.img_nchw, out.img_nhwc_u8, B, (mb_stream)s);
    if (rc) return rc;
  }
  return launched();
}

// The fourth kind of run, "requests" (include/maskbit_hip.h "per-sample sampling arguments"): a seeded run whose step t covers the prefix
// [0, active[t]) of the batch and whose step kernels read their constants per sample from plan.table.  A sibling of sample_run that shares its pieces --
// the start state, the two forwards, the checked step, combine and decode -- and has none of its step chunks.  Every argument check is in front of the
// first launch, those that need no handle in front of the handle's own (the entry is refused the same way with or without a device).
int sample_requests_run(mb_gen* g, mb_dec* d, const mb_request_plan& plan, const int64_t* labels, int B, const int64_t* init_tokens, const int64_t* seeds,
                        const RunOut& out, hipStream_t s) {
  const char* who = "mb_sample_requests";
  const int S = plan.num_steps;
  if (!plan.active || !plan.table || !labels || !seeds) return fail(-1, "%s: null argument", who);
  if (S <= 0 || B <= 0) return fail(-1, "%s: bad sizes (num_steps = %d, B = %d)", who, S, B);
  for (int t = 0; t < S; ++t) {
    if (plan.active[t] < 1 || plan.active[t] > B) return fail(-1, "%s: active[%d] = %d outside [1, %d]", who, t, plan.active[t], B);
    if (t && plan.active[t] < plan.active[t - 1])
      return fail(-1, "%s: active[] is not non-decreasing (active[%d] = %d after %d): order the requests by num_steps descending", who, t, plan.active[t], plan.active[t - 1]);
  }
  if (plan.active[S - 1] != B) return fail(-1, "%s: active[%d] = %d, but all %d requests run the last step", who, S - 1, plan.active[S - 1], B);
  if (!d && (out.img_nchw || out.img_nhwc_u8)) return fail(-1, "%s: image requested without a decoder", who);
  if (!g) return fail(-1, "%s: null argument (no generator handle)", who);
  const bool guided = plan.use_guidance != 0;
  const int nbf = guided ? 2 * B : B;
  if (nbf > g->max_seqs) return fail(-1, "%s: B=%d needs %d sequences, engine holds %d", who, B, nbf, g->max_seqs);
  const mb_gen_cfg& c = g->c;
  const int n = c.seq, m = c.splits, C = g->C;
  const size_t P = (size_t)n * m;
  mb_gen::Run& run = g->run;
  run.next = -1;                                       // ends any run in progress: no chunk of another kind continues this one
  // The start state in BOTH token buffers: a request that becomes active at step t reads whichever buffer is `cur` then, and nothing has touched its rows
  if (init_tokens) mb::edit_load_tokens(s, init_tokens, g->tok_a, g->num_regen, B, (int)P, C);
  else {
    mb::fill_i64(s, g->tok_a, (int64_t)C, (size_t)B * P);
    mb::edit_load_tokens(s, g->tok_a, nullptr, g->num_regen, B, (int)P, C);
  }
  HIP_TRY(hipMemcpyAsync(g->tok_b, g->tok_a, (size_t)B * P * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  int64_t* cur = g->tok_a;
  int64_t* nxt = g->tok_b;
  int64_t* last_pred = g->pred;
  struct CfgReady { mb_gen::Run& run; ~CfgReady() { run.cfg_labels = nullptr; } } cfg_ready{run};
  run.cfg_labels = nullptr;
  mb::StepArgs a{};
  a.logits_c = g->logits; a.P = (int)P; a.C = C;
  a.seeds = seeds;
  for (int t = 0; t < S; ++t) {
    const int Bt = plan.active[t];
    int rc;
    // The forward is chosen by the run's flag alone, never by the scales of the step: a request with scale 0 gets c + 0 (c - u) from the guided forward
    if (guided) {
      rc = gen_forward_cfg(g, cur, labels, g->logits, Bt, s);
      a.logits_u = g->logits + (size_t)Bt * P * C;
      if (Bt <= g->chunk_seqs / 2) { run.cfg_labels = labels; run.cfg_B = Bt; }   // valid until the prefix grows: gen_forward_cfg then refreshes lab_cfg / drop_cfg
      else run.cfg_labels = nullptr;
    } else {
      rc = gen_forward(g, cur, labels, nullptr, g->logits, Bt, s);
      a.logits_u = nullptr;
    }
    if (rc) return rc;
    a.B = Bt;
    a.req = (const mb::RequestStep*)plan.table + (size_t)t * B;
    a.tokens = nxt; a.pred = out.step_tokens ? out.step_tokens + (size_t)t * B * P : g->pred;
    rc = sample_step_checked(who, a, cur, g->num_regen, 0.f, s);
    if (rc) return rc;
    last_pred = a.pred;                                // (the last step runs all B requests: its predictions are the whole batch's)
    int64_t* tmp = cur; cur = nxt; nxt = tmp;
  }
  int64_t* codes = out.codes ? out.codes : g->codes;
  mb::combine_groups(s, last_pred, codes, (size_t)B * n, m, g->gbits);
  if (d) {
    int rc = mb_dec_decode(d, codes, out.img_nchw, out.img_nhwc_u8, B, (mb_stream)s);
    if (rc) return rc;
  }
  return launched();
}

}  // namespace

extern "C" {

int mb_sample_requests(mb_gen* g, mb_dec* d, const mb_request_plan* plan, const int64_t* labels, int B, const int64_t* init_tokens, const int64_t* seeds,
                       int64_t* step_tokens, int64_t* tokens_out, float* img_nchw, uint8_t* img_nhwc_u8, mb_stream stream) {
  if (!plan) return fail(-1, "mb_sample_requests: null argument");
  return sample_requests_run(g, d, *plan, labels, B, init_tokens, seeds, RunOut{step_tokens, tokens_out, img_nchw, img_nhwc_u8}, (hipStream_t)stream);
}

int mb_sample(mb_gen* g, mb_dec* d, const mb_sample_plan* plan, const int64_t* labels, int B, const float* exp_noise,
              const float* conf_noise, int64_t* step_tokens, int64_t* tokens_out, float* img_nchw,
              uint8_t* img_nhwc_u8, mb_stream stream) {
  if (!plan || !g || !labels || !exp_noise || !conf_noise) return fail(-1, "mb_sample: null argument");
  RunSpec r = run_spec("mb_sample", *plan);
  r.mask_len = plan->mask_len;
  r.noise.exp_noise = exp_noise; r.noise.conf_noise = conf_noise;
  return sample_run(g, d, r, labels, B, RunOut{step_tokens, tokens_out, img_nchw, img_nhwc_u8}, (hipStream_t)stream);
}

int mb_sample_edit(mb_gen* g, mb_dec* d, const mb_edit_plan* plan, const int64_t* labels, int B, const int64_t* init_tokens, const float* exp_noise,
                   const float* conf_noise, int64_t* step_tokens, int64_t* tokens_out, float* img_nchw, uint8_t* img_nhwc_u8, mb_stream stream) {
  if (!plan || !plan->mask_ratio) return fail(-1, "mb_sample_edit: %s", plan ? "incomplete plan" : "null argument");
  if (!g || !labels || !exp_noise || !conf_noise || !init_tokens) return fail(-1, "mb_sample_edit: null argument");
  RunSpec r = run_spec("mb_sample_edit", *plan);
  r.mask_ratio = plan->mask_ratio;
  r.init_tokens = init_tokens;
  r.noise.exp_noise = exp_noise; r.noise.conf_noise = conf_noise;
  return sample_run(g, d, r, labels, B, RunOut{step_tokens, tokens_out, img_nchw, img_nhwc_u8}, (hipStream_t)stream);
}

int mb_sample_seeded(mb_gen* g, mb_dec* d, const mb_edit_plan* plan, const int64_t* labels, int B, const int64_t* init_tokens, const int64_t* seeds,
                     float randomize_temperature, const float* conf_weight, int64_t* step_tokens, int64_t* tokens_out, float* img_nchw,
                     uint8_t* img_nhwc_u8, mb_stream stream) {
  if (!plan || !plan->mask_ratio) return fail(-1, "mb_sample_seeded: %s", plan ? "incomplete plan" : "null argument");
  if (!seeds || !conf_weight || !g || !labels) return fail(-1, "mb_sample_seeded: null argument");
  RunSpec r = run_spec("mb_sample_seeded", *plan);
  r.mask_ratio = plan->mask_ratio;
  r.init_tokens = init_tokens;
  r.noise.seeds = seeds; r.noise.rand_temp = randomize_temperature; r.noise.conf_weight = conf_weight;
  return sample_run(g, d, r, labels, B, RunOut{step_tokens, tokens_out, img_nchw, img_nhwc_u8}, (hipStream_t)stream);
}

}  // extern "C"

// ================================================================================================
// sampling session (include/maskbit_hip.h "sampling session"; kernels: session.hip)
// ================================================================================================
// The session object: the device state of max_active rows (allocated by the first admit that passes its checks) and the HOST MIRROR of the rule the
// kernels apply -- per active row its ticket, local step and N --, from which a tick knows k, the moves and the finished tickets without reading the
// device.  tok[cur] is the buffer the next tick reads.
struct mb_session {
  int n = 0, m = 0, C = 0, gbits = 0, cap = 0, max_steps = 0;
  bool guided = false, allocated = false;
  size_t P = 0;
  struct Row { uint64_t ticket; int local_step, N; };
  std::vector<Row> rows;                                // [A]
  uint64_t next_ticket = 0;
  int64_t* tok[2] = {nullptr, nullptr};
  int cur = 0;
  int64_t *pred = nullptr, *codes_all = nullptr, *codes = nullptr;
  mb::SessionRows st{};
  mb::RequestStep* row = nullptr;                       // [cap]: the step's table row
  int* plan = nullptr;                                  // the snapshot of a tick's retire step (mb::session_plan_ints)
  bool cfg_dirty = true;                                // membership changed since the handle's lab_cfg / drop_cfg were filled from st.label
  mb::DevArena mem;
};

namespace {

int session_allocate(mb_session* s) {
  if (s->allocated) return 0;
  mb::DevArena& m = s->mem;
  const size_t cap = (size_t)s->cap;
  m.get(&s->tok[0], cap * s->P); m.get(&s->tok[1], cap * s->P); m.get(&s->pred, cap * s->P);
  m.get(&s->codes_all, cap * s->n); m.get(&s->codes, cap * s->n);
  m.get(&s->st.label, cap); m.get(&s->st.seed, cap);
  m.get(&s->st.num_regen, cap); m.get(&s->st.slot, cap); m.zeroed(&s->st.local_step, cap); m.zeroed(&s->st.N, cap);
  m.get(&s->st.pool, cap * s->max_steps);
  m.get(&s->row, cap); m.get(&s->plan, mb::session_plan_ints(s->cap));
  if (int rc = m.failed("mb_session_admit")) return rc;
  std::vector<int> iota(cap);
  for (size_t r = 0; r < cap; ++r) iota[r] = (int)r;    // every pool slot free: row r would take slot r
  HIP_TRY(hipMemcpy(s->st.slot, iota.data(), cap * sizeof(int), hipMemcpyHostToDevice));
  s->st.cap = s->cap; s->st.max_steps = s->max_steps;
  s->allocated = true;
  return 0;
}

}  // namespace

extern "C" {

int mb_session_create(int seq, int splits, int bits, int max_active, int max_steps, int use_guidance, mb_session** out) {
  if (!out) return fail(-1, "mb_session_create: null argument");
  if (max_active < 1 || max_steps < 1) return fail(-1, "mb_session_create: bad sizes (max_active = %d, max_steps = %d: both at least 1)", max_active, max_steps);
  if (seq < 1 || splits < 1 || bits < 1 || bits > 24 || bits % splits || (size_t)seq * splits > 8192 || (1 << (bits / splits)) > 4096)
    return fail(-1, "mb_session_create: seq = %d, splits = %d, bits = %d is no generator configuration (mb_gen_create)", seq, splits, bits);
  if ((size_t)max_active * max_steps > ((size_t)1 << 27)) return fail(-1, "mb_session_create: max_active * max_steps = %zu schedule records exceed 2^27", (size_t)max_active * max_steps);
  mb_session* s = new mb_session();
  s->n = seq; s->m = splits; s->gbits = bits / splits; s->C = 1 << s->gbits; s->P = (size_t)seq * splits;
  s->cap = max_active; s->max_steps = max_steps; s->guided = use_guidance != 0;
  s->rows.reserve(max_active);
  *out = s;
  return 0;
}

void mb_session_destroy(mb_session* s) { delete s; }

int mb_session_active(const mb_session* s) { return s ? (int)s->rows.size() : -1; }

int mb_session_due(const mb_session* s) {
  if (!s) return -1;
  int due = 0;
  for (const mb_session::Row& r : s->rows) due += r.local_step + 1 == r.N;
  return due;
}

int mb_session_admit(mb_session* s, int K, const int64_t* labels, const int64_t* seeds, const int* num_steps, const mb_request_step* schedule,
                     const int64_t* init_tokens, uint64_t* tickets, mb_stream stream) {
  const char* who = "mb_session_admit";
  if (K < 1) return fail(-1, "%s: bad sizes (K = %d)", who, K);
  if (!s || !labels || !seeds || !num_steps || !schedule || !tickets) return fail(-1, "%s: null argument", who);
  for (int k = 0; k < K; ++k)
    if (num_steps[k] < 1 || num_steps[k] > s->max_steps) return fail(-1, "%s: num_steps[%d] = %d outside [1, %d]", who, k, num_steps[k], s->max_steps);
  const int A = (int)s->rows.size();
  if (K > s->cap - A) return fail(-1, "%s: %d active + %d new requests exceed max_active = %d", who, A, K, s->cap);
  if (int rc = session_allocate(s)) return rc;
  hipStream_t st = (hipStream_t)stream;
  // the start state goes into the buffer the next tick reads; the other one is written by that tick's step before anything reads it
  mb::session_admit(st, s->st, s->tok[s->cur], init_tokens, num_steps, labels, seeds, (const mb::RequestStep*)schedule, A, K, (int)s->P, s->C);
  for (int k = 0; k < K; ++k) {
    tickets[k] = s->next_ticket;
    s->rows.push_back({s->next_ticket++, 0, num_steps[k]});
  }
  s->cfg_dirty = true;
  return launched();
}

int mb_session_tick(mb_session* s, mb_gen* g, mb_dec* d, int64_t* pred_out, int64_t* codes_out, float* img_nchw, uint8_t* img_nhwc_u8, uint64_t* finished,
                    uint64_t* ran, int* num_finished, mb_stream stream) {
  const char* who = "mb_session_tick";
  if (!s || !num_finished) return fail(-1, "%s: null argument", who);
  *num_finished = 0;
  const int A = (int)s->rows.size();
  if (A == 0) return 0;                                  // an empty session: nothing to run, nothing launched
  if (!finished && mb_session_due(s) > 0) return fail(-1, "%s: null argument (%d requests finish, no ticket array)", who, mb_session_due(s));
  if (!d && (img_nchw || img_nhwc_u8)) return fail(-1, "%s: image requested without a decoder", who);
  if (!g) return fail(-1, "%s: null argument (no generator handle)", who);
  const mb_gen_cfg& c = g->c;
  if (c.seq != s->n || c.splits != s->m || g->C != s->C)
    return fail(-1, "%s: the session was created for %d positions x %d groups of %d codes, the generator has %d x %d of %d", who, s->n, s->m, s->C, c.seq, c.splits, g->C);
  const int nbf = s->guided ? 2 * A : A;
  if (nbf > g->max_seqs) return fail(-1, "%s: %d active requests need %d sequences, engine holds %d", who, A, nbf, g->max_seqs);
  hipStream_t st = (hipStream_t)stream;
  const size_t P = s->P;
  mb_gen::Run& run = g->run;
  run.next = -1;                                         // ends any chunked run in progress, as mb_sample_requests does
  // 1. the step's table row, gathered on the device
  mb::session_row_table(st, s->st, s->row, A);
  // 2. one global step of sample_requests_run over the A rows.  lab_cfg / drop_cfg of the handle stay marked ready ACROSS ticks (nothing else leaves a
  // mark behind, and gen_forward_cfg drops it when it overwrites them), but never across a change of membership: the label buffer keeps its address
  int64_t* cur = s->tok[s->cur];
  int64_t* nxt = s->tok[s->cur ^ 1];
  if (s->cfg_dirty && run.cfg_labels == s->st.label) run.cfg_labels = nullptr;
  mb::StepArgs a{};
  a.logits_c = g->logits; a.B = A; a.P = (int)P; a.C = s->C;
  a.seeds = s->st.seed; a.req = s->row;
  int rc;
  if (s->guided) {
    rc = gen_forward_cfg(g, cur, s->st.label, g->logits, A, st);
    a.logits_u = g->logits + (size_t)A * P * s->C;
    if (A <= g->chunk_seqs / 2) { run.cfg_labels = s->st.label; run.cfg_B = A; }
    else run.cfg_labels = nullptr;
    s->cfg_dirty = false;
  } else {
    rc = gen_forward(g, cur, s->st.label, nullptr, g->logits, A, st);
  }
  if (rc) return rc;
  int64_t* pred = pred_out ? pred_out : s->pred;
  a.tokens = nxt; a.pred = pred;
  rc = sample_step_checked(who, a, cur, s->st.num_regen, 0.f, st);
  if (rc) return rc;
  s->cur ^= 1;
  // 3. retire and compact: the mirror applies the kernels' rule -- F ascending, holes = F below A', movers = the unfinished rows at or above A'
  std::vector<mb_session::Row>& rows = s->rows;
  int k = 0;
  for (int r = 0; r < A; ++r) {
    if (ran) ran[r] = rows[r].ticket;
    if (++rows[r].local_step == rows[r].N) finished[k++] = rows[r].ticket;
  }
  *num_finished = k;
  if (k == 0) return launched();
  const int Ap = A - k;
  int moves = 0;
  for (int hole = 0, mover = Ap; hole < Ap; ++hole) {
    if (rows[hole].local_step != rows[hole].N) continue;
    while (rows[mover].local_step == rows[mover].N) ++mover;   // (as many unfinished rows at or above A' as finished ones below)
    rows[hole] = rows[mover++];
    ++moves;
  }
  rows.resize(Ap);
  s->cfg_dirty = true;
  if (run.cfg_labels == s->st.label) run.cfg_labels = nullptr;
  int64_t* codes = codes_out ? codes_out : s->codes;
  mb::session_retire(st, s->st, s->plan, s->tok[s->cur], pred, s->codes_all, codes, A, s->n, s->m, s->gbits, k, moves);
  // 4. decode the k finished requests
  if (d && (img_nchw || img_nhwc_u8)) {
    rc = mb_dec_decode(d, codes, img_nchw, img_nhwc_u8, k, (mb_stream)st);
    if (rc) return rc;
  }
  return launched();
}

}  // extern "C"
