// The generator handle's members, for the translation units that work on it: engine.hip (create, load, the forward schedules), sampler.hip (the step
// entries, the sampling loops, the session) and diag.hip (the two study knobs); and what sampler.hip calls in engine.hip.  Internal: not part of the ABI.
#pragma once
#include <vector>

#include "../../include/maskbit_hip_diag.h"
#include "mb_abi.h"
#include "mb_kernels.h"

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

namespace mb {

// engine.hip: the plain forward over nb sequences (attn: optional attention maps) and the guided one over B samples, each in passes of at most chunk_seqs sequences
int gen_forward(mb_gen* g, const int64_t* tokens, const int64_t* labels, const uint8_t* drop, float* logits, int nb, hipStream_t s, float* attn = nullptr);
int gen_forward_cfg(mb_gen* g, const int64_t* tokens, const int64_t* labels, float* logits, int B, hipStream_t s);

}  // namespace mb
