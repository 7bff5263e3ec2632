// The generator handle of libmaskbit_hip.so (include/maskbit_hip.h; its members: mb_gen.h): create, checkpoint ingest with h16 repack, the three forward
// schedules (plain, differential CFG, fp32 reference) behind gen_forward / gen_forward_cfg; and the three ABI-wide entries (mb_abi_version, mb_last_error,
// mb_prof_*).  What samples with the handle -- the step entries, the whole-run loops, the session -- is in sampler.hip, the tokenizer handle's entry points in
// decoder.hip, the diagnostic ones (include/maskbit_hip_diag.h) in diag.hip; the error path, the device-allocation arena and the profiling scopes they all share are in mb_abi.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "mb_gen.h"

using mb::fail;
using mb::g_prof;
using mb::launched;
using mb::ProfScope;

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

}  // namespace

namespace mb {   // (declared in mb_gen.h: sampler.hip calls the two)

// The kernels index with 32-bit element / byte offsets (rows * mlp * 4 < 2^32): forwards over more sequences than that allows run as
// independent chunks (sequences never interact), which also bounds the workspace of very large batches.
int gen_forward(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, int nb, hipStream_t s, float* attn) {
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
    if (!(nc == B && g->run.cfg_labels == labels && g->run.cfg_B == B)) {       // (the ready mark: sampler.hip forward_and_step sets it and states its contract)
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

}  // namespace mb

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

int mb_gen_saturation_count(mb_gen* g, unsigned* count, int reset, mb_stream stream) {
  if (!g || !count) return fail(-1, "mb_gen_saturation_count: null argument");
  return mb::read_counter("mb_gen_saturation_count", g->sat, count, reset, (hipStream_t)stream);
}

int mb_gen_forward(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits,
                   int nb, mb_stream stream) {
  if (!g || !tokens || !labels || !logits) return fail(-1, "mb_gen_forward: null argument");
  if (nb <= 0 || nb > g->max_seqs) return fail(-1, "mb_gen_forward: nb=%d outside [1, %d]", nb, g->max_seqs);
  return mb::gen_forward(g, tokens, labels, drop, logits, nb, (hipStream_t)stream);
}

int mb_gen_forward_cfg(mb_gen* g, const int64_t* tokens, const int64_t* labels, float* logits, int B, mb_stream stream) {
  if (!g || !tokens || !labels || !logits) return fail(-1, "mb_gen_forward_cfg: null argument");
  if (B <= 0 || 2 * B > g->max_seqs) return fail(-1, "mb_gen_forward_cfg: B=%d needs %d sequences, engine holds %d", B, 2 * B, g->max_seqs);
  return mb::gen_forward_cfg(g, tokens, labels, logits, B, (hipStream_t)stream);
}

int mb_gen_forward_attn(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, float* attn,
                        int nb, mb_stream stream) {
  if (!g || !tokens || !labels || !logits || !attn) return fail(-1, "mb_gen_forward_attn: null argument");
  if (nb <= 0 || nb > g->max_seqs) return fail(-1, "mb_gen_forward_attn: nb=%d outside [1, %d]", nb, g->max_seqs);
  if (g->f32) return fail(-3, "mb_gen_forward_attn: attention maps are not available in the fp32 reference mode (precision %d)", (int)MB_PREC_F32);
  return mb::gen_forward(g, tokens, labels, drop, logits, nb, (hipStream_t)stream, attn);
}

}  // extern "C"
