// Diagnostic entry points (include/maskbit_hip_diag.h): single kernels and single layers on caller buffers, for the tests and the tools.
// No host binding of the product needs them.  Argument checks, a scratch arena (mb::DevArena) where a layer needs one, and the launchers' own calls
// only: this file holds no kernel of its own (mb_autoenc.h brings the loader's affine_kernel along for mb_autoenc_block).
// (mb_gen_set_alo and mb_gen_set_walk, the entries that set a member of the generator handle, see it through mb_gen.h.)
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/maskbit_hip_diag.h"
#include "mb_abi.h"
#include "mb_autoenc.h"
#include "mb_conv.h"
#include "mb_disc.h"
#include "mb_gen.h"
#include "mb_image.h"
#include "mb_kernels.h"
#include "mb_spattn.h"
#include "mb_vq.h"

using mb::fail;
using mb::launched;
using mb::ProfScope;

namespace {

// The walk direction (mb_kernels.h walk_tile / walk_seq) the per-launch entries below hand to their trunk kernel: mb_diag_set_walk, 0 unless a test sets it.
int g_walk_reverse = 0;

// The common tail of the GEMM entries: the timed launch, the refusal message (`mini`: the entry's name, sequence-aligned tiles), the launch check.
int run_gemm(mb_stream stream, int epi, const mb::GemmArgs& args, int variant, const char* mini = nullptr) {
  mb::GemmArgs a = args;
  a.reverse = g_walk_reverse;
  ProfScope p("gemm_diag", (hipStream_t)stream);
  if (mb::gemm_tn((hipStream_t)stream, (mb::GemmEpi)epi, a, variant))
    return mini ? fail(-3, "%s: shape refused", mini) : fail(-3, "GEMM shape M=%d N=%d K=%d is outside the kernels' shapes", a.M, a.N, a.K);
  return launched();
}

int w4_entry(const char* what, decltype(mb::w4_from_f32)* pack, const float* W, int N, int K, void* dst4, void* scale_out, mb_stream stream) {
  if (!W || !dst4 || !scale_out || N <= 0 || K <= 0 || N % 64 || K % 128) return fail(-1, "%s: bad arguments", what);
  pack((hipStream_t)stream, W, (uint8_t*)dst4, N, K, (uint8_t*)scale_out);
  return launched();
}

int pool_entry(const char* what, decltype(mb::launch_s2d)* launch, const void* x, void* y, int B, int H, int W, int C, mb_stream stream) {
  if (!x || !y) return fail(-1, "%s: null argument", what);
  if (B <= 0 || H <= 0 || W <= 0 || H % 2 || W % 2 || C <= 0 || C % 8) return fail(-1, "%s: H and W must be even, C a multiple of 8", what);
  launch((hipStream_t)stream, (const h16*)x, (h16*)y, B, H, W, C);
  return launched();
}

// The quantizer entries: the shapes mb_dec_create_vq / vq_argmin accept, the codebook descriptor the handle fills, and temporaries that are
// allocated and freed in stream order (no synchronisation: a free waits for the launches queued before it).
bool vq_shape_ok(int C, int K) { return C >= 2 && C <= 65536 && K >= 1 && K <= 256; }
mb::VqCodebook vq_shape(int C, int K, int l2) {
  mb::VqCodebook q;
  q.C = C; q.K = K; q.Kp = mb::vq_kp(K); q.Cpad = mb::vq_cpad(C); q.l2 = l2 ? 1 : 0;
  return q;
}
struct StreamTemps {
  explicit StreamTemps(hipStream_t stream) : s(stream) {}
  StreamTemps(const StreamTemps&) = delete;
  StreamTemps& operator=(const StreamTemps&) = delete;
  ~StreamTemps() { for (void* p : owned) (void)hipFreeAsync(p, s); }
  template <class T>
  void get(T** out, size_t n) {
    void* p = nullptr;
    *out = nullptr;
    if (ok && hipMallocAsync(&p, n * sizeof(T), s) == hipSuccess) { owned.push_back(p); *out = (T*)p; }
    else ok = false;
  }
  hipStream_t s;
  std::vector<void*> owned;
  bool ok = true;
};

// The optional e2m1 outputs of a row kernel (values x4 / x4_scale, fp16 lo halves xl4 / xl4_scale) over `rows` rows of `seq_rows` each, the class
// token last: the vector kernels alone write them (d = 768 / 1024), and the lane-ordered scale arrays hold whole 64-token groups.
int f4_rows(const char* who, mb::Fp4Rows& f4, void* x4, void* x4_scale, void* xl4, void* xl4_scale, int rows, int d, int seq_rows) {
  f4 = mb::Fp4Rows{};
  if ((x4 != nullptr) != (x4_scale != nullptr) || (xl4 != nullptr) != (xl4_scale != nullptr)) return fail(-1, "%s: an e2m1 copy and its scale array go together", who);
  if (!x4 && !xl4) return 0;
  if (d != 768 && d != 1024) return fail(-1, "%s: e2m1 copies are written at d = 768 / 1024 only, not %d", who, d);
  if (seq_rows < 65 || (seq_rows - 1) % 64 || rows % seq_rows)
    return fail(-1, "%s: e2m1 copies: sequences of 64 k tokens + the class token, whole sequences (%d rows of %d)", who, rows, seq_rows);
  f4 = mb::Fp4Rows{(uint8_t*)x4, (uint8_t*)x4_scale, (uint8_t*)xl4, (uint8_t*)xl4_scale, rows / seq_rows, seq_rows};
  return 0;
}

// The argument checks of the two embedding entries (the kernels check nothing).  Device CONTENTS are trusted: tokens in [0, 2^gbits], labels in [0, nclass].
int embed_args(const char* who, mb::EmbedArgs& e, const int64_t* tokens, const int64_t* labels, const float* w_in, const float* b_in, const float* class_emb,
               const float* pos, const float* gamma, const float* beta, const float* tables, float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4,
               void* xl4_scale, int nb, int seq, int m, int gbits, int d, int nclass) {
  if (!tokens || !labels || !class_emb || !pos || !gamma || !beta || !x_f32 || !x_h16 || (!tables && (!w_in || !b_in))) return fail(-1, "%s: null argument", who);
  if (nb <= 0 || seq <= 0 || m <= 0 || gbits <= 0 || d <= 0 || nclass < 0) return fail(-1, "%s: bad sizes", who);
  if (d > 2048) return fail(-1, "%s: d = %d is beyond the row kernels (2048)", who, d);
  if ((int64_t)m * gbits > 24) return fail(-1, "%s: %d groups of %d bits are beyond the embed kernels (24 bits)", who, m, gbits);
  if (tables && m > 8) return fail(-1, "%s: %d embedding tables are beyond the embed kernel (8)", who, m);
  mb::Fp4Rows f4;
  if (int rc = f4_rows(who, f4, x4, x4_scale, xl4, xl4_scale, nb * (seq + 1), d, seq + 1)) return rc;
  e = mb::EmbedArgs{tokens, labels, nullptr, nullptr, b_in, class_emb, pos, gamma, beta, x_f32, (h16*)x_h16, nb, seq, m, gbits, d, nclass, tables};
  e.f4 = f4;
  return 0;
}
// input_proj.weight as the checkpoint holds it, [d, K] -> e.w_in = [K, d] in the arena, by the product's transpose as mb_gen_load runs it
int embed_weight(const char* who, mb::DevArena& arena, mb::EmbedArgs& e, const float* w_in, hipStream_t s) {
  if (e.tables) return 0;
  const int K = e.m * e.gbits;
  float* wt = nullptr;
  arena.get(&wt, (size_t)K * e.d);
  if (int rc = arena.failed(who)) return rc;
  mb::transpose_f32(s, w_in, wt, e.d, K);
  e.w_in = wt;
  return 0;
}

}  // namespace

extern "C" {

int mb_set_cu_count(int n) { mb::set_cu_count(n); return 0; }

// the two study knobs of the generator handle (mb_gen.h: alo_mask, walk)
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

int mb_diag_set_walk(int reverse) {
  if (reverse != 0 && reverse != 1) return fail(-1, "mb_diag_set_walk: direction 0 or 1");
  g_walk_reverse = reverse;
  return 0;
}
int mb_walk_tile(int vb, int ntiles, int reverse) { return vb < 0 || vb >= ntiles ? -1 : mb::walk_tile(vb, ntiles, reverse ? 1 : 0); }
int mb_walk_seq(int slot, int n, int grp, int reverse) { return slot < 0 || slot >= n || grp < 1 ? -1 : mb::walk_seq(slot, n, grp, reverse ? 1 : 0); }
int mb_walk_row(int slot, int rows, int seq_rows, int pair, int reverse) {
  return slot < 0 || slot >= rows ? -1 : mb::walk_row(slot, rows, mb::walk_rows(rows, seq_rows, pair != 0, reverse));
}
int mb_walk_group(int seq_rows, int pair) { return seq_rows < 2 ? -1 : mb::walk_group(seq_rows, pair != 0); }
int mb_gemm_ht_supported(int epi, int M, int N, int K) {
  mb::GemmArgs a{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, M, N, K, 0};
  return mb::gemm_ht_supported((mb::GemmEpi)epi, a) ? 1 : 0;
}

// ---- one GEMM of the trunk family on caller buffers (tests and tools/gemm_bench.py) ----
int mb_gemm(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32, void* out_h16,
            int M, int N, int K, int period, int variant, mb_stream stream) {
  if (!A || !W || !bias || epi < 0 || epi > 4) return fail(-1, "mb_gemm: bad arguments");
  if (K % 64) return fail(-1, "mb_gemm: K must be a multiple of 64");
  mb::GemmArgs a{(const h16*)A, (const h16*)W, bias, residual, out_f32, (h16*)out_h16, M, N, K, period};
  return run_gemm(stream, epi, a, variant);
}
int mb_gemm_ex(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32, void* out_h16,
               int M, int N, int K, const float* ln_stats, const float* ln_g, const float* ln_b, int period, int variant, mb_stream stream) {
  if (!A || !W || !bias || epi < 0 || epi > 4) return fail(-1, "mb_gemm_ex: bad arguments");
  if (K % 64) return fail(-1, "mb_gemm_ex: K must be a multiple of 64");
  if (ln_stats && (!ln_g || !ln_b || epi != mb::EPI_RES_F32)) return fail(-1, "mb_gemm_ex: LayerNorm residual needs gamma, beta and the fp32+residual epilogue");
  mb::GemmArgs a{(const h16*)A, (const h16*)W, bias, residual, out_f32, (h16*)out_h16, M, N, K, period, nullptr, ln_stats, ln_g, ln_b};
  return run_gemm(stream, epi, a, variant);
}
int mb_gemm_act_split(int epi, const void* A_hi, const void* A_lo, const void* W, const float* bias, const float* residual, float* out_f32,
                      void* out_h16, int M, int N, int kw, int variant, mb_stream stream) {
  if (!A_hi || !A_lo || !W || !bias || epi < 0 || epi > 3 || kw <= 0 || kw % 64) return fail(-1, "mb_gemm_act_split: bad arguments");
  mb::GemmArgs a{(const h16*)A_hi, (const h16*)W, bias, residual, out_f32, (h16*)out_h16, M, N, 2 * kw, 0};
  a.A2 = (const h16*)A_lo; a.kw = kw;
  return run_gemm(stream, epi, a, variant);
}
int mb_gemm_mini(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32, void* out_h16, void* out4,
                 void* out4_scale, int rows, int pair, int N, int K, int nlo, const void* const* lo /* nlo x {A4, a_scale, W4, w_scale} */, mb_stream stream) {
  return mb_gemm_mini_seq(epi, A, W, bias, residual, out_f32, out_h16, out4, out4_scale, nullptr, nullptr, rows, pair, 0, N, K, nlo, lo, stream);
}
int mb_gemm_mini_seq(int epi, const void* A, const void* W, const float* bias, const float* residual, float* out_f32, void* out_h16, void* out4,
                     void* out4_scale, void* out4l, void* out4l_scale, int rows, int pair, int seq_rows, int N, int K, int nlo, const void* const* lo, mb_stream stream) {
  if ((out4l || out4l_scale) && (!out4l || !out4l_scale || !out4 || !out4_scale)) return fail(-1, "mb_gemm_mini_seq: the lo copy (out4l / out4l_scale) rides with the value copy (out4 / out4_scale)");
  if (!A || !W || !bias || epi < 0 || epi > 2 || rows <= 0 || K <= 0 || K % 64 || nlo < 0 || nlo > 2 || (nlo && !lo)) return fail(-1, "mb_gemm_mini: bad arguments");
  mb::GemmArgs a{(const h16*)A, (const h16*)W, bias, residual, out_f32, (h16*)out_h16, pair ? 2 * rows : rows, N, K, 0};
  if (pair) a.pair_rows = rows;
  a.seq_rows = seq_rows;
  a.nlo = nlo;
  for (int i = 0; i < nlo; ++i) a.lo[i] = {(const uint8_t*)lo[4 * i], (const uint8_t*)lo[4 * i + 1], (const uint8_t*)lo[4 * i + 2], (const uint8_t*)lo[4 * i + 3]};
  a.out4 = (uint8_t*)out4; a.out4_scale = (uint8_t*)out4_scale;
  a.out4l = (uint8_t*)out4l; a.out4l_scale = (uint8_t*)out4l_scale;
  if ((!seq_rows && a.M % 257) || !mb::gemm_ht_supported((mb::GemmEpi)epi, a)) return fail(-3, "mb_gemm_mini: shape not supported by the sequence-aligned tiles");
  return run_gemm(stream, epi, a, 257, "mb_gemm_mini");
}
int mb_gemm_mini_ln(const void* A, const void* W, const float* bias, float* y, const float* ln_stats, const float* ln_g, const float* ln_b, int rows, int pair,
                    int seq_rows, int N, int K, int nlo, const void* const* lo, mb_stream stream) {
  if (!A || !W || !bias || !y || !ln_stats || !ln_g || !ln_b || rows <= 0 || K <= 0 || K % 64 || nlo < 0 || nlo > 2 || (nlo && !lo))
    return fail(-1, "mb_gemm_mini_ln: bad arguments");
  mb::GemmArgs a{(const h16*)A, (const h16*)W, bias, y, y, nullptr, pair ? 2 * rows : rows, N, K, 0, nullptr, ln_stats, ln_g, ln_b};
  if (pair) a.pair_rows = rows;
  a.seq_rows = seq_rows;
  a.nlo = nlo;
  for (int i = 0; i < nlo; ++i) a.lo[i] = {(const uint8_t*)lo[4 * i], (const uint8_t*)lo[4 * i + 1], (const uint8_t*)lo[4 * i + 2], (const uint8_t*)lo[4 * i + 3]};
  if ((!seq_rows && a.M % 257) || !mb::gemm_ht_supported(mb::EPI_RES_F32, a)) return fail(-3, "mb_gemm_mini_ln: shape not supported by the sequence-aligned tiles");
  return run_gemm(stream, mb::EPI_RES_F32, a, 257, "mb_gemm_mini_ln");
}
int mb_gemm_mini_split(int epi, const void* A_hi, const void* A_lo, const void* W, const float* bias, void* out_h16, void* out4, void* out4_scale,
                       int rows, int N, int kw, const void* const* lo /* {A4, a_scale, W4, w_scale} */, mb_stream stream) {
  if (!A_hi || !A_lo || !W || !bias || !out_h16 || !lo || epi < 0 || epi > 1 || rows <= 0 || rows % 257 || kw <= 0 || kw % 128)
    return fail(-1, "mb_gemm_mini_split: bad arguments");
  mb::GemmArgs a{(const h16*)A_hi, (const h16*)W, bias, nullptr, nullptr, (h16*)out_h16, rows, N, 2 * kw, 0};
  a.A2 = (const h16*)A_lo; a.kw = kw;
  a.nlo = 1;
  a.lo[0] = {(const uint8_t*)lo[0], (const uint8_t*)lo[1], (const uint8_t*)lo[2], (const uint8_t*)lo[3]};
  a.out4 = (uint8_t*)out4; a.out4_scale = (uint8_t*)out4_scale;
  if (!mb::gemm_ht_supported((mb::GemmEpi)epi, a)) return fail(-3, "mb_gemm_mini_split: shape not supported by the sequence-aligned tiles");
  return run_gemm(stream, epi, a, 257, "mb_gemm_mini_split");
}

// ---- the head GEMMs as head_gemms (engine.hip) fills them, and the two weight-preparation launchers of mb_gen_load that had no entry ----
int mb_gemm_head(int epi, const void* A_hi, const void* A_lo, const void* W_hi, const void* W_lo, const float* scale, const float* bias, int bias_per_pos,
                 float* out_f32, int M, int N, int kw, int period, mb_stream stream) {
  if (!A_hi || !A_lo || !W_hi || !bias || !out_f32) return fail(-1, "mb_gemm_head: null argument");
  if ((W_lo != nullptr) != (scale != nullptr)) return fail(-1, "mb_gemm_head: the weights' lo plane and the scale go together");
  if (epi != mb::EPI_GELU_F32 && epi != mb::EPI_LOGITS_F32) return fail(-1, "mb_gemm_head: epilogue 3 or 4");
  if (M <= 0 || N <= 0 || N % 4 || kw <= 0 || kw % 64) return fail(-1, "mb_gemm_head: M > 0, N a multiple of 4, kw a multiple of 64");
  if (epi == mb::EPI_LOGITS_F32 && (period < 2 || M % period)) return fail(-1, "mb_gemm_head: epilogue 4: whole sequences of period >= 2 rows");
  if (bias_per_pos && epi != mb::EPI_LOGITS_F32) return fail(-1, "mb_gemm_head: a per-position bias goes with epilogue 4");
  mb::GemmArgs a{(const h16*)A_hi, (const h16*)W_hi, bias, nullptr, out_f32, nullptr, M, N, (W_lo ? 3 : 2) * kw, period, scale};
  a.A2 = (const h16*)A_lo; a.kw = kw; a.W2 = (const h16*)W_lo;
  a.bias_per_pos = bias_per_pos;
  return run_gemm(stream, epi, a, 0, "mb_gemm_head");
}
int mb_cast_f32_to_h16(const float* src, void* dst, int64_t n, mb_stream stream) {
  if (!src || !dst || n < 0) return fail(-1, "mb_cast_f32_to_h16: bad arguments");
  mb::cast_f32_to_h16((hipStream_t)stream, src, (h16*)dst, (size_t)n);
  return launched();
}
int mb_split_f32_planes(const float* src, void* hi, void* lo, int N, int K, float* scale_out, unsigned* tmp, mb_stream stream) {
  if (!src || !hi || !lo || !scale_out || !tmp || N <= 0 || K <= 0) return fail(-1, "mb_split_f32_planes: bad arguments");
  mb::split_f32_to_h16_planes((hipStream_t)stream, src, (h16*)hi, (h16*)lo, N, K, scale_out, tmp);
  return launched();
}

int mb_w4_from_f32(const float* W, int N, int K, void* dst4, void* scale_out, mb_stream stream) {
  return w4_entry("mb_w4_from_f32", mb::w4_from_f32, W, N, K, dst4, scale_out, stream);
}
int mb_w4lo_from_f32(const float* W, int N, int K, void* dst4, void* scale_out, mb_stream stream) {
  return w4_entry("mb_w4lo_from_f32", mb::w4lo_from_f32, W, N, K, dst4, scale_out, stream);
}

int mb_layernorm(const float* y, const float* gamma, const float* beta, float eps, float* x_f32, void* x_h16, void* x_lo, float* stats, int M,
                 int d, mb_stream stream) {
  if (!y || !gamma || !beta || M <= 0 || d <= 0 || d > 2048) return fail(-1, "mb_layernorm: bad arguments");
  mb::layernorm_rows((hipStream_t)stream, y, gamma, beta, eps, x_f32, (h16*)x_h16, stats, M, d, (h16*)x_lo, mb::Fp4Rows{}, g_walk_reverse, 0);
  return launched();
}
int mb_layernorm_f4_seq(const float* y, const float* gamma, const float* beta, float eps, float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4,
                        void* xl4_scale, int M, int d, int seq_rows, mb_stream stream) {
  if (!y || !gamma || !beta || (!x4 && !xl4) || M <= 0) return fail(-1, "mb_layernorm_f4: bad arguments (an e2m1 output is required)");
  mb::Fp4Rows f4;
  if (int rc = f4_rows("mb_layernorm_f4", f4, x4, x4_scale, xl4, xl4_scale, M, d, seq_rows)) return rc;
  mb::layernorm_rows((hipStream_t)stream, y, gamma, beta, eps, x_f32, (h16*)x_h16, nullptr, M, d, nullptr, f4, g_walk_reverse, seq_rows);
  return launched();
}
int mb_layernorm_f4(const float* y, const float* gamma, const float* beta, float eps, float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4,
                    void* xl4_scale, int M, int d, mb_stream stream) {
  return mb_layernorm_f4_seq(y, gamma, beta, eps, x_f32, x_h16, x4, x4_scale, xl4, xl4_scale, M, d, 257, stream);
}

// ---- the pair forms and the embedding kernels of norm_embed.hip on caller buffers ----
int mb_layernorm_pair(const float* y, const float* gamma, const float* beta, float eps, void* x_h16, float* stats, void* x4, void* x4_scale, void* xl4,
                      void* xl4_scale, int P, int d, int seq_rows, mb_stream stream) {
  if (!y || !gamma || !beta || !x_h16 || P <= 0 || d <= 0 || d > 2048) return fail(-1, "mb_layernorm_pair: bad arguments");
  mb::Fp4Rows f4;
  if (int rc = f4_rows("mb_layernorm_pair", f4, x4, x4_scale, xl4, xl4_scale, P, d, seq_rows)) return rc;
  if (mb::layernorm_pair((hipStream_t)stream, y, gamma, beta, eps, (h16*)x_h16, stats, P, d, f4, g_walk_reverse, seq_rows))
    return fail(-3, "mb_layernorm_pair: width %d is outside the pair kernels (768 or 1024)", d);
  return launched();
}
int mb_pairify(const float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4, void* xl4_scale, int P, int d, int seq_rows, mb_stream stream) {
  if (!x_f32 || !x_h16 || P <= 0 || d <= 0 || d > 2048) return fail(-1, "mb_pairify: bad arguments");
  mb::Fp4Rows f4;
  if (int rc = f4_rows("mb_pairify", f4, x4, x4_scale, xl4, xl4_scale, P, d, seq_rows)) return rc;
  if (mb::pairify_rows((hipStream_t)stream, x_f32, (h16*)x_h16, P, d, f4, g_walk_reverse, seq_rows))
    return fail(-3, "mb_pairify: width %d is outside the pair kernels (768 or 1024)", d);
  return launched();
}
int mb_embed_ln(const int64_t* tokens, const int64_t* labels, const uint8_t* drop, const float* w_in, const float* b_in, const float* class_emb,
                const float* pos, const float* gamma, const float* beta, const float* tables, float* x_f32, void* x_h16, void* x_lo, void* x4,
                void* x4_scale, void* xl4, void* xl4_scale, int nb, int seq, int m, int gbits, int d, int nclass, mb_stream stream) {
  mb::EmbedArgs e;
  if (int rc = embed_args("mb_embed_ln", e, tokens, labels, w_in, b_in, class_emb, pos, gamma, beta, tables, x_f32, x_h16, x4, x4_scale, xl4, xl4_scale,
                          nb, seq, m, gbits, d, nclass)) return rc;
  e.drop = drop; e.x_lo = (h16*)x_lo;
  mb::DevArena arena;
  if (int rc = embed_weight("mb_embed_ln", arena, e, w_in, (hipStream_t)stream)) return rc;
  mb::embed_ln((hipStream_t)stream, e);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(-10, "mb_embed_ln: the launch failed");   // the arena goes on return
  return launched();
}
int mb_embed_pair(const int64_t* tokens, const int64_t* labels, const float* w_in, const float* b_in, const float* class_emb, const float* pos,
                  const float* gamma, const float* beta, const float* tables, float* x_f32, void* x_h16, void* x4, void* x4_scale, void* xl4,
                  void* xl4_scale, int nb, int seq, int m, int gbits, int d, int nclass, mb_stream stream) {
  // what mb::embed_pair itself refuses (-1 there) is refused here in front of the weight transpose, so that nothing at all is launched
  // (an e2m1 request at a scalar-path width, or a width beyond 2048, is a bad argument: -1 from embed_args)
  const bool f4 = x4 || x4_scale || xl4 || xl4_scale;
  if (tables || (m > 0 && gbits > 0 && (int64_t)m * gbits > 24) || (!f4 && d > 0 && d <= 2048 && d != 768 && d != 1024))
    return fail(-3, "mb_embed_pair: not served by the fused kernel (embedding tables, more than 24 bits, widths other than 768 / 1024): embed_ln + pairify");
  mb::EmbedArgs e;
  if (int rc = embed_args("mb_embed_pair", e, tokens, labels, w_in, b_in, class_emb, pos, gamma, beta, tables, x_f32, x_h16, x4, x4_scale, xl4, xl4_scale,
                          nb, seq, m, gbits, d, nclass)) return rc;
  mb::DevArena arena;
  if (int rc = embed_weight("mb_embed_pair", arena, e, w_in, (hipStream_t)stream)) return rc;
  const int refused = mb::embed_pair((hipStream_t)stream, e);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return fail(-10, "mb_embed_pair: the launch failed");
  if (refused) return fail(-3, "mb_embed_pair: not served by the fused kernel");
  return launched();
}

int mb_attention(const void* qkv, void* out_h16, void* out4, void* out4_scale, int nb, int N, int d, int heads, mb_stream stream) {
  if (!qkv || !out_h16 || (!out4) != (!out4_scale) || nb <= 0 || N <= 0 || d <= 0 || heads <= 0 || d % heads) return fail(-1, "mb_attention: bad arguments");
  if (d / heads != 32 && d / heads != 64) return fail(-3, "mb_attention: head width %d is outside the attention kernels (32 or 64)", d / heads);
  ProfScope p("attention", (hipStream_t)stream);
  mb::attention((hipStream_t)stream, (const h16*)qkv, (h16*)out_h16, nb, N, d, heads, (uint8_t*)out4, (uint8_t*)out4_scale, g_walk_reverse);
  return launched();
}
int mb_attention_probs(const void* qkv, float* out_f32, int nb, int N, int d, int heads, mb_stream stream) {
  if (!qkv || !out_f32 || nb <= 0 || N <= 0 || d <= 0 || heads <= 0 || d % heads) return fail(-1, "mb_attention_probs: bad arguments");
  if (mb::attention_probs((hipStream_t)stream, (const h16*)qkv, out_f32, nb, N, d, heads))
    return fail(-3, "mb_attention_probs: head width %d / N = %d tokens is outside the probabilities kernel (32 or 64; N <= 5120)", d / heads, N);
  return launched();
}
int mb_attention_pair(const void* qkv, void* out_h16, int pairs, int N, int d, int heads, mb_stream stream) {
  if (!qkv || !out_h16 || pairs <= 0 || N <= 0 || heads <= 0 || d % heads) return fail(-1, "mb_attention_pair: bad arguments");
  ProfScope p("attention", (hipStream_t)stream);
  if (mb::attention_pair((hipStream_t)stream, (const h16*)qkv, (h16*)out_h16, pairs, N, d, heads, nullptr, nullptr, nullptr, nullptr, g_walk_reverse))
    return fail(-3, "mb_attention_pair: head width %d (N = %d tokens) is outside the attention kernels", d / heads, N);
  return launched();
}
int mb_attention_pair_f4(const void* qkv, void* out_h16, void* out4, void* out4_scale, void* out4l, void* out4l_scale, int pairs, int N, int d, int heads, mb_stream stream) {
  if (!qkv || !out_h16 || !out4 || !out4_scale || (!out4l) != (!out4l_scale) || pairs <= 0 || N <= 0 || heads <= 0 || d % heads) return fail(-1, "mb_attention_pair_f4: bad arguments");
  ProfScope p("attention", (hipStream_t)stream);
  if (mb::attention_pair((hipStream_t)stream, (const h16*)qkv, (h16*)out_h16, pairs, N, d, heads, (uint8_t*)out4, (uint8_t*)out4_scale, (uint8_t*)out4l, (uint8_t*)out4l_scale, g_walk_reverse))
    return fail(-3, "mb_attention_pair_f4: head width %d / N = %d tokens: no e2m1 copy for this shape", d / heads, N);
  return launched();
}

int mb_seeded_noise(const int64_t* seeds, int step, float randomize_temperature, float conf_weight, float* exp_u, float* exp_noise, float* conf_u,
                    float* conf_noise, int B, int P, int C, mb_stream stream) {
  if (!seeds || !exp_noise || !conf_noise) return fail(-1, "mb_seeded_noise: null argument");
  if (B <= 0 || P <= 0 || C <= 0 || step < 0) return fail(-1, "mb_seeded_noise: bad sizes");
  if (exp_u == exp_noise || conf_u == conf_noise) return fail(-1, "mb_seeded_noise: the uniforms and the noise must not alias");
  if (mb::seeded_noise_dump((hipStream_t)stream, seeds, step, randomize_temperature, conf_weight, exp_u, exp_noise, conf_u, conf_noise, B, P, C))
    return fail(-1, "mb_seeded_noise: C=%d or P=%d too large", C, P);
  return launched();
}

int mb_vq_argmin(const float* z, const float* codebook, int N, int C, int K, int l2, int splits, int64_t* idx, float* dist, mb_stream stream) {
  if (!z || !codebook || !idx) return fail(-1, "mb_vq_argmin: null argument");
  if (int rc = mb::vq_argmin(z, codebook, N, C, K, l2, splits, idx, dist, (hipStream_t)stream)) return rc;
  return launched();
}

// ---- the quantizer kernels (vq.hip; lfq / latent / pack_image of conv.hip) through the launchers the tokenizer handle calls, in its order ----
int mb_vq_encode_rows(const void* z_h16, int stride16, const float* z_f32, const float* codebook, int B, int HW, int C, int K, int l2, int splits,
                      int64_t* idx, float* zq_nchw, float* zraw_nchw, float* dist, mb_stream stream) {
  using namespace mb;
  hipStream_t s = (hipStream_t)stream;
  if (!codebook || (z_h16 != nullptr) == (z_f32 != nullptr)) return fail(-1, "mb_vq_encode_rows: a codebook and exactly one of z_h16 / z_f32 required");
  if (!vq_shape_ok(C, K)) return fail(-1, "mb_vq_encode_rows: C in [2, 65536], K in [1, 256] required");
  if (B < 1 || HW < 1 || (int64_t)B * HW > (1 << 24)) return fail(-1, "mb_vq_encode_rows: B >= 1, HW >= 1, B * HW <= 2^24 required");
  if (z_h16 && stride16 < K) return fail(-1, "mb_vq_encode_rows: stride16 = %d is below K = %d", stride16, K);
  const int N = B * HW, Npad = vq_npad(N);
  VqCodebook q = vq_shape(C, K, l2);
  splits = vq_splits(q, N, splits);
  StreamTemps t(s);
  float *zT = nullptr, *ps = nullptr;
  int* pi = nullptr;
  t.get(&q.cb, (size_t)C * K); t.get(&q.cbT, (size_t)q.Kp * q.Cpad); t.get(&q.cbn, (size_t)q.Cpad);
  t.get(&zT, (size_t)q.Kp * Npad); t.get(&ps, (size_t)splits * Npad); t.get(&pi, (size_t)splits * Npad);
  if (!t.ok) return fail(-10, "mb_vq_encode_rows: device allocation failed");
  vq_prep_codebook(q, codebook, s);
  vq_prep_rows(q, (const h16*)z_h16, stride16, z_f32, N, HW, zT, zraw_nchw, s);
  vq_search(q, zT, N, HW, splits, ps, pi, idx, zq_nchw, dist, s);
  return launched();
}
int mb_vq_gather(const int64_t* codes, const float* codebook, int64_t npix, int C, int K, int l2, int cin_pad, void* out_h16, unsigned* sat,
                 mb_stream stream) {
  using namespace mb;
  hipStream_t s = (hipStream_t)stream;
  if (!codes || !codebook || !out_h16 || !sat) return fail(-1, "mb_vq_gather: null argument");
  if (!vq_shape_ok(C, K)) return fail(-1, "mb_vq_gather: C in [2, 65536], K in [1, 256] required");
  if (npix < 1 || npix > (1 << 24)) return fail(-1, "mb_vq_gather: npix in [1, 2^24] required");
  if (cin_pad < K || cin_pad % CK) return fail(-1, "mb_vq_gather: cin_pad = %d must be a multiple of 64 and at least K = %d", cin_pad, K);
  VqCodebook q = vq_shape(C, K, l2);
  StreamTemps t(s);
  t.get(&q.cb, (size_t)C * K); t.get(&q.cbT, (size_t)q.Kp * q.Cpad); t.get(&q.cbn, (size_t)q.Cpad);
  if (!t.ok) return fail(-10, "mb_vq_gather: device allocation failed");
  vq_prep_codebook(q, codebook, s);
  vq_gather(q, codes, (size_t)npix, (h16*)out_h16, cin_pad, sat, s);
  return launched();
}
int mb_vq_pack_latent(const float* z_nchw, int B, int K, int HW, int cin_pad, void* out_h16, unsigned* sat, mb_stream stream) {
  if (!z_nchw || !out_h16 || !sat) return fail(-1, "mb_vq_pack_latent: null argument");
  if (B < 1 || HW < 1 || (int64_t)B * HW > (1 << 24) || K < 1 || K > 256) return fail(-1, "mb_vq_pack_latent: B >= 1, HW >= 1, B * HW <= 2^24, K in [1, 256] required");
  if (cin_pad < K || cin_pad % mb::CK) return fail(-1, "mb_vq_pack_latent: cin_pad = %d must be a multiple of 64 and at least K = %d", cin_pad, K);
  mb::vq_pack_latent(z_nchw, B, K, HW, (h16*)out_h16, cin_pad, sat, (hipStream_t)stream);
  return launched();
}
int mb_lfq_pack(const void* z_h16, int B, int HW, int K, int Kp, int64_t* idx, float* zq_nchw, float* zraw_nchw, mb_stream stream) {
  if (!z_h16 || !idx) return fail(-1, "mb_lfq_pack: null argument");
  if (B < 1 || HW < 1 || (int64_t)B * HW > (1 << 24)) return fail(-1, "mb_lfq_pack: B >= 1, HW >= 1, B * HW <= 2^24 required");
  if (K < 1 || K > mb::CK || Kp < K) return fail(-1, "mb_lfq_pack: K in [1, 64] and Kp >= K required");
  mb::launch_lfq((hipStream_t)stream, (const h16*)z_h16, idx, zq_nchw, zraw_nchw, B, HW, K, Kp);
  return launched();
}
int mb_lfq_latent(const int64_t* tokens, int64_t npix, int K, void* out_h16, mb_stream stream) {
  if (!tokens || !out_h16) return fail(-1, "mb_lfq_latent: null argument");
  if (npix < 1 || npix > (1 << 24) || K < 1 || K > mb::CK) return fail(-1, "mb_lfq_latent: npix in [1, 2^24] and K in [1, 64] required");
  mb::launch_latent((hipStream_t)stream, tokens, (h16*)out_h16, (size_t)npix, K);
  return launched();
}
int mb_pack_image(const float* img_nchw, int B, int C, int H, int W, void* out_h16, mb_stream stream) {
  if (!img_nchw || !out_h16) return fail(-1, "mb_pack_image: null argument");
  if (B < 1 || H < 1 || W < 1 || (int64_t)B * H * W > (1 << 24) || C < 1 || C > 4) return fail(-1, "mb_pack_image: B, H, W >= 1, B * H * W <= 2^24, C in [1, 4] required");
  mb::launch_pack_image((hipStream_t)stream, img_nchw, (h16*)out_h16, B, C, H, W);
  return launched();
}

// ---- single tokenizer layers on caller buffers: the handle's own launchers (mb_conv.h) on a scratch arena instead of a handle.  The ones that
// allocate synchronise the stream before they return (the scratch is freed on return); where a later allocation fails after work was queued, it is
// the arena's hipFree that waits for that work, as hipFree does. ----
int mb_conv_layer(const void* in_h16, const float* w_oihw, const float* bias, const float* gn_gamma, const float* gn_beta, const void* residual_h16,
                  void* out_h16, float* img_nchw, uint8_t* img_nhwc_u8, const float* out_gamma, const float* out_beta, float* out_scale_shift,
                  float* out_gn_part, int* part_tiles, unsigned* saturated, int B, int H, int W, int Cin, int Cout, int ks, int up_, int final_layer,
                  mb_stream stream) {
  return mb_conv_layer_ex(in_h16, w_oihw, bias, gn_gamma, gn_beta, residual_h16, out_h16, img_nchw, img_nhwc_u8, out_gamma, out_beta, out_scale_shift,
                          out_gn_part, part_tiles, saturated, B, H, W, Cin, Cout, ks, up_, final_layer, 0, stream);
}
// flags: 1 = the prologue without SiLU, 2 = stats off (launch_conv's gn_silu = false / stats = false, which the handles' schedules use)
int mb_conv_layer_ex(const void* in_h16, const float* w_oihw, const float* bias, const float* gn_gamma, const float* gn_beta, const void* residual_h16,
                     void* out_h16, float* img_nchw, uint8_t* img_nhwc_u8, const float* out_gamma, const float* out_beta, float* out_scale_shift,
                     float* out_gn_part, int* part_tiles, unsigned* saturated, int B, int H, int W, int Cin, int Cout, int ks, int up_, int final_layer,
                     int flags, mb_stream stream) {
  using namespace mb;
  hipStream_t s = (hipStream_t)stream;
  const bool fin = final_layer != 0, up = up_ != 0, no_silu = (flags & 1) != 0, stats = (flags & 2) == 0;
  if (flags & ~3) return fail(-1, "mb_conv_layer: unknown flag bits");
  if (no_silu && (ks != 1 || !gn_gamma)) return fail(-1, "mb_conv_layer: the prologue without SiLU goes with ks 1 and gamma / beta");
  if (!in_h16 || !w_oihw || B <= 0 || Cin <= 0 || Cout <= 0) return fail(-1, "mb_conv_layer: null or empty argument");
  if (ks < 1 || ks > 3) return fail(-1, "mb_conv_layer: ks must be 1, 2 or 3");
  if (H <= 0 || W <= 0 || H % TH8 || W % TW) return fail(-1, "mb_conv_layer: the output must be whole 8 x 16 pixel tiles");
  if (fin && (ks != 3 || up || Cout > 4 || residual_h16 || !(img_nchw || img_nhwc_u8))) return fail(-1, "mb_conv_layer: final layer: ks 3, at most 4 channels, no residual, an image output");
  if (!fin && (!out_h16 || Cout % 4)) return fail(-1, "mb_conv_layer: fp16 output: Cout must be a multiple of 4");
  if (up && ks != 3) return fail(-1, "mb_conv_layer: upsampling goes with ks 3");
  if (ks == 2 && (Cin % 16 || gn_gamma)) return fail(-1, "mb_conv_layer: ks 2 (stride-2 conv): Cin must be a multiple of 16, no prologue");
  if ((gn_gamma != nullptr) != (gn_beta != nullptr) || (gn_gamma && (Cin % CK || Cin > 2048))) return fail(-1, "mb_conv_layer: prologue: gamma and beta, Cin a multiple of 64 up to 2048");
  if (out_scale_shift && (fin || !out_gamma || !out_beta || Cout % 32 || Cout > 2048)) return fail(-1, "mb_conv_layer: output statistics: gamma and beta, Cout a multiple of 32 up to 2048");
  Conv c;
  if (ks == 2) shape_down_conv(c, Cin); else shape_conv(c, Cin, Cout, ks, bias != nullptr, up, fin);
  if (ks == 2) { c.cout = Cout; c.cout_w = Cout; c.cout_pad = (Cout + 127) / 128 * 128; c.has_bias = bias != nullptr; }
  DevArena m;
  GnCtx gc;
  const int Hin = ks == 2 ? 2 * H : (up ? H / 2 : H), Win = ks == 2 ? 2 * W : (up ? W / 2 : W);   // the caller's input tensor
  if (up && (H % 2 || W % 2)) return fail(-1, "mb_conv_layer: upsampling needs even H and W");
  const size_t npix_in = (size_t)B * Hin * Win;
  h16* staged = nullptr;
  m.get(&c.w, conv_weight_elems(c)); m.get(&c.b, (size_t)c.cout_pad); m.get(&c.sat, 1);
  m.get(&gc.part, gn_part_elems(B, std::max(H, Hin), std::max(W, Win))); m.get(&gc.ss, (size_t)B * std::max(c.cin_pad, std::max(Cout, 1)));
  if (int rc = m.failed("mb_conv_layer")) return rc;
  bool ok = hipMemsetAsync(c.b, 0, c.cout_pad * sizeof(float), s) == hipSuccess && hipMemsetAsync(c.sat, 0, sizeof(unsigned), s) == hipSuccess;
  if (ok && bias) ok = hipMemcpyAsync(c.b, bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess;
  launch_repack_conv(s, c, w_oihw);
  const h16* in = (const h16*)in_h16;
  if (ks == 2) {                                    // [B, 2H, 2W, Cin] -> [B, H, W, 4 Cin]
    if (!m.get(&staged, npix_in * Cin)) return m.failed("mb_conv_layer");
    launch_s2d(s, in, staged, B, Hin, Win, Cin);
    in = staged;
  } else if (c.cin_pad != Cin) {                    // channels padded with zeros to a whole chunk, as pack_image_kernel / latent_kernel leave them
    if (!m.get(&staged, npix_in * c.cin_pad)) return m.failed("mb_conv_layer");
    ok = ok && hipMemsetAsync(staged, 0, npix_in * c.cin_pad * sizeof(h16), s) == hipSuccess &&
         hipMemcpy2DAsync(staged, c.cin_pad * sizeof(h16), in, Cin * sizeof(h16), Cin * sizeof(h16), npix_in, hipMemcpyDeviceToDevice, s) == hipSuccess;
    in = staged;
  }
  if (!ok) return fail(-10, "mb_conv_layer: copy failed");
  const float2* gn = nullptr;
  if (gn_gamma) {
    Norm n; n.c = Cin; n.g = const_cast<float*>(gn_gamma); n.b = const_cast<float*>(gn_beta);
    launch_gn(s, &gc, n, in, B, Hin * Win);
    gn = gc.ss;
  }
  launch_conv(s, &gc, c, in, gn, (const h16*)residual_h16, (h16*)out_h16, img_nchw, img_nhwc_u8, B, H, W, fin, stats, !no_silu);
  const int tiles = gc.of == (const void*)out_h16 && !fin ? gc.ntile : 0;      // the epilogue wrote GroupNorm partials of the output
  if (part_tiles) *part_tiles = tiles;
  if (out_gn_part && tiles) ok = hipMemcpyAsync(out_gn_part, gc.part, (size_t)B * tiles * 64 * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess;
  if (ok && out_scale_shift) {
    Norm n; n.c = Cout; n.g = const_cast<float*>(out_gamma); n.b = const_cast<float*>(out_beta);
    launch_gn(s, &gc, n, (const h16*)out_h16, B, H * W);                      // from the epilogue's partials when there are any, else the sweep
    ok = hipMemcpyAsync(out_scale_shift, gc.ss, (size_t)B * Cout * sizeof(float2), hipMemcpyDeviceToDevice, s) == hipSuccess;
  }
  unsigned nsat = 0;
  ok = ok && hipMemcpyAsync(&nsat, c.sat, sizeof(unsigned), hipMemcpyDeviceToHost, s) == hipSuccess;
  if (hipStreamSynchronize(s) != hipSuccess || !ok) return fail(-10, "mb_conv_layer: copy failed");
  if (saturated) *saturated = nsat;
  return launched();
}
int mb_groupnorm_stats(const void* x_h16, const float* gamma, const float* beta, float* scale_shift, int B, int HW, int C, mb_stream stream) {
  using namespace mb;
  hipStream_t s = (hipStream_t)stream;
  if (!x_h16 || !gamma || !beta || !scale_shift) return fail(-1, "mb_groupnorm_stats: null argument");
  if (B <= 0 || HW <= 0 || C < 32 || C > 2048 || C % 32 || (C / 8) > 256) return fail(-1, "mb_groupnorm_stats: C must be a multiple of 32 in [32, 2048]");
  DevArena m;
  GnCtx gc;
  m.get(&gc.part, gn_part_elems(B, 0, 0)); m.get(&gc.ss, (size_t)B * C);
  if (int rc = m.failed("mb_groupnorm_stats")) return rc;
  Norm n; n.c = C; n.g = const_cast<float*>(gamma); n.b = const_cast<float*>(beta);
  launch_gn(s, &gc, n, (const h16*)x_h16, B, HW);   // gc.of is null: the sweep (gn_partial_kernel) + gn_finalize_kernel
  if (hipMemcpyAsync(scale_shift, gc.ss, (size_t)B * C * sizeof(float2), hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) return fail(-10, "mb_groupnorm_stats: copy failed");
  return launched();
}
// One ResNet block of the handles' scaffold (mb_autoenc.h) on a scratch AutoEnc: init_block, load_param under checkpoint names, run_block
int mb_autoenc_block(const void* x_h16, const float* n1_g, const float* n1_b, const float* c1_w, const float* c1_b, const float* n2_g, const float* n2_b,
                     const float* c2_w, const float* c2_b, const float* sc_w, const float* sc_b, int form, int bias_, void* out_h16, void* h1_h16,
                     void* mid_h16, const float* out_gamma, const float* out_beta, float* out_scale_shift, unsigned* saturated, int B, int H, int W,
                     int cin, int cout, mb_stream stream) {
  using namespace mb;
  hipStream_t s = (hipStream_t)stream;
  const bool bias = bias_ != 0;
  if (!x_h16 || !n1_g || !n1_b || !c1_w || !n2_g || !n2_b || !c2_w || !out_h16 || !h1_h16) return fail(-1, "mb_autoenc_block: null argument");
  if (form < 0 || form > 2 || (form == 0) != (cin == cout)) return fail(-1, "mb_autoenc_block: form 0 goes with cin == cout, forms 1 and 2 with cin != cout");
  if (form != 0 && (!sc_w || !mid_h16)) return fail(-1, "mb_autoenc_block: the shortcut's weight and the mid output are required with a shortcut");
  if (bias && (!c1_b || !c2_b || (form != 0 && !sc_b))) return fail(-1, "mb_autoenc_block: bias on needs every bias");
  if (B <= 0 || H <= 0 || W <= 0 || H % TH8 || W % TW) return fail(-1, "mb_autoenc_block: whole 8 x 16 pixel tiles required");
  if (cin <= 0 || cout <= 0 || cin % CK || cout % CK || cin > 2048 || cout > 2048) return fail(-1, "mb_autoenc_block: cin and cout must be multiples of 64 up to 2048");
  if (out_scale_shift && (!out_gamma || !out_beta)) return fail(-1, "mb_autoenc_block: output statistics need gamma and beta");
  AutoEnc a;
  ResBlock rb;
  const size_t npix = (size_t)B * H * W;
  a.mem.zeroed(&a.sat, 1);
  init_block(a, rb, "b", cin, cout, bias, form == 1);
  for (int i = 0; i < 3; ++i) a.mem.get(&a.buf[i], npix * std::max(cin, cout));
  a.mem.get(&a.gn.part, gn_part_elems(B, H, W));
  a.mem.get(&a.gn.ss, (size_t)B * std::max(cin, cout));
  if (int rc = a.mem.failed("mb_autoenc_block")) return rc;
  const size_t sc_in = form == 1 ? cin : cout;
  struct { const char* name; const float* data; size_t numel; } entries[] = {
      {"b.norm1.weight", n1_g, (size_t)cin}, {"b.norm1.bias", n1_b, (size_t)cin}, {"b.conv1.weight", c1_w, (size_t)cout * cin * 9},
      {"b.conv1.bias", bias ? c1_b : nullptr, (size_t)cout}, {"b.norm2.weight", n2_g, (size_t)cout}, {"b.norm2.bias", n2_b, (size_t)cout},
      {"b.conv2.weight", c2_w, (size_t)cout * cout * 9}, {"b.conv2.bias", bias ? c2_b : nullptr, (size_t)cout},
      {"b.nin_shortcut.weight", form ? sc_w : nullptr, (size_t)cout * sc_in}, {"b.nin_shortcut.bias", form && bias ? sc_b : nullptr, (size_t)cout}};
  for (const auto& e : entries)
    if (e.data)
      if (int rc = load_param("mb_autoenc_block", a, e.name, e.data, e.numel, s)) return rc;
  HIP_TRY(hipMemcpyAsync(a.buf[0], x_h16, npix * cin * sizeof(h16), hipMemcpyDeviceToDevice, s));
  a.h1_tap = (h16*)h1_h16;
  const int oi = run_block(s, a, rb, 0, B, H, W);
  // where run_block's rotation leaves the middle tensor: buffer 2 in both forms (the shortcut's output / conv2's raw output)
  if (form) HIP_TRY(hipMemcpyAsync(mid_h16, a.buf[2], npix * cout * sizeof(h16), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipMemcpyAsync(out_h16, a.buf[oi], npix * cout * sizeof(h16), hipMemcpyDeviceToDevice, s));
  if (out_scale_shift) {
    Norm n; n.c = cout; n.g = const_cast<float*>(out_gamma); n.b = const_cast<float*>(out_beta);
    launch_gn(s, &a.gn, n, a.buf[oi], B, H * W);                               // from whatever state the block left in the context
    HIP_TRY(hipMemcpyAsync(out_scale_shift, a.gn.ss, (size_t)B * cout * sizeof(float2), hipMemcpyDeviceToDevice, s));
  }
  unsigned nsat = 0;
  HIP_TRY(hipMemcpyAsync(&nsat, a.sat, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (saturated) *saturated = nsat;
  return launched();
}
int mb_avgpool2(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream) { return pool_entry("mb_avgpool2", mb::launch_avgpool2, x_h16, y_h16, B, H, W, C, stream); }
int mb_s2d(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream) { return pool_entry("mb_s2d", mb::launch_s2d, x_h16, y_h16, B, H, W, C, stream); }

// ---- the pieces of the LPIPS forward (mb_lpips_input / _distance / _features need lpips.hip's kernels and handle and are defined there) ----
// w fp32 OIHW, bias fp32 [Cout] or null, in / out fp16 NHWC with the true channel counts
int mb_conv_relu_layer(const void* in_h16, const float* w_oihw, const float* bias, void* out_h16, unsigned* saturated, int B, int H, int W, int Cin,
                       int Cout, int ks, mb_stream stream) {
  using namespace mb;
  hipStream_t s = (hipStream_t)stream;
  if (!in_h16 || !w_oihw || !out_h16 || B <= 0 || Cin <= 0 || Cout <= 0) return fail(-1, "mb_conv_relu_layer: null or empty argument");
  if (ks != 1 && ks != 3) return fail(-1, "mb_conv_relu_layer: ks must be 1 or 3");
  if (H <= 0 || W <= 0 || H % TH8 || W % TW) return fail(-1, "mb_conv_relu_layer: the output must be whole 8 x 16 pixel tiles");
  if (Cout % 4) return fail(-1, "mb_conv_relu_layer: Cout must be a multiple of 4");
  Conv c;
  shape_conv(c, Cin, Cout, ks, true, false, false);
  DevArena m;
  const size_t npix = (size_t)B * H * W;
  const h16* in = (const h16*)in_h16;
  h16* staged = nullptr;
  m.get(&c.w, conv_weight_elems(c)); m.get(&c.b, (size_t)c.cout_pad); m.get(&c.sat, 1);
  if (int rc = m.failed("mb_conv_relu_layer")) return rc;
  bool ok = hipMemsetAsync(c.b, 0, c.cout_pad * sizeof(float), s) == hipSuccess && hipMemsetAsync(c.sat, 0, sizeof(unsigned), s) == hipSuccess;
  if (ok && bias) ok = hipMemcpyAsync(c.b, bias, (size_t)Cout * sizeof(float), hipMemcpyDeviceToDevice, s) == hipSuccess;
  launch_repack_conv(s, c, w_oihw);
  if (c.cin_pad != Cin) {                           // channels padded with zeros to a whole chunk
    if (!m.get(&staged, npix * c.cin_pad)) return m.failed("mb_conv_relu_layer");
    ok = ok && hipMemsetAsync(staged, 0, npix * c.cin_pad * sizeof(h16), s) == hipSuccess &&
         hipMemcpy2DAsync(staged, c.cin_pad * sizeof(h16), in, Cin * sizeof(h16), Cin * sizeof(h16), npix, hipMemcpyDeviceToDevice, s) == hipSuccess;
    in = staged;
  }
  if (!ok) return fail(-10, "mb_conv_relu_layer: copy failed");
  launch_conv_relu(s, ConvRelu{in, c.w, c.b, (h16*)out_h16, c.sat, B, H, W, c.cin_pad, c.cout, c.cout_pad, ks});
  unsigned nsat = 0;
  ok = hipMemcpyAsync(&nsat, c.sat, sizeof(unsigned), hipMemcpyDeviceToHost, s) == hipSuccess;
  if (hipStreamSynchronize(s) != hipSuccess || !ok) return fail(-10, "mb_conv_relu_layer: copy failed");
  if (saturated) *saturated = nsat;
  return launched();
}
// the spatial self-attention launch of the Taming tokenizer's AttnBlock (spatial_attention.hip), as the handle issues it
int mb_spatial_attention(const void* q, const void* k, const void* v, void* out_h16, unsigned* sat, int B, int N, int ld, int ldo, mb_stream stream) {
  using namespace mb;
  if (!q || !k || !v || !out_h16) return fail(-1, "mb_spatial_attention: null argument");
  if (!launch_spatial_attention((hipStream_t)stream, SpAttn{(const h16*)q, (const h16*)k, (const h16*)v, (h16*)out_h16, sat, B, N, ld, ldo}))
    return fail(-1, "mb_spatial_attention: B >= 1, N a multiple of 16 in [16, 1024], ld >= 512 a multiple of 8, ldo >= 512 a multiple of 4");
  return launched();
}
int mb_maxpool2(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream) { return pool_entry("mb_maxpool2", mb::launch_maxpool2, x_h16, y_h16, B, H, W, C, stream); }

// ---- the fp32 reference mode's two kernels on caller buffers (tests/test_hip_gemm_f32.py, test_hip_attention_f32.py) ----
int mb_gemm_f32(int epi, const float* A, const float* W, const float* bias, const float* residual, float* out, int M, int N, int K, int period,
                int bias_per_pos, mb_stream stream) {
  if (!A || !W || !bias || !out || epi < 0 || epi > 3 || (epi == mb::F32_EPI_RES && !residual)) return fail(-1, "mb_gemm_f32: bad arguments");
  mb::GemmF32Args a{epi, A, W, bias, residual, out, M, N, K, period, bias_per_pos};
  ProfScope p("gemm_f32_diag", (hipStream_t)stream);
  if (mb::gemm_f32((hipStream_t)stream, a))
    return fail(-3, "mb_gemm_f32: M=%d N=%d K=%d (period %d) is outside the kernel's shapes: M, N >= 1, K >= 4 and K %% 4 == 0, 16-byte aligned A and W, "
                    "logits rows in whole periods", M, N, K, period);
  return launched();
}
int mb_attention_f32(const float* qkv, float* out, int nb, int N, int d, int heads, mb_stream stream) {
  if (!qkv || !out) return fail(-1, "mb_attention_f32: null argument");
  ProfScope p("attention_f32_diag", (hipStream_t)stream);
  if (mb::attention_f32((hipStream_t)stream, qkv, out, nb, N, d, heads))
    return fail(-3, "mb_attention_f32: nb=%d N=%d d=%d heads=%d is outside the kernel's shapes (d / heads = 32 or 64)", nb, N, d, heads);
  return launched();
}

// ---- the sampling session's kernels on caller-owned arrays (tests/test_hip_session.py) ----
static_assert(sizeof(mb_session_rows) == sizeof(mb::SessionRows), "mb_session_rows is the kernels' SessionRows");
static const char* session_rows_check(const mb_session_rows* r, int rows_used, int n, int m, int C, int* gbits) {
  if (!r || !r->label || !r->seed || !r->num_regen || !r->slot || !r->local_step || !r->N || !r->pool) return "null argument";
  if (r->max_active < 1 || r->max_steps < 1 || rows_used < 1 || rows_used > r->max_active) return "rows outside [1, max_active]";
  if (n < 1 || m < 1 || (size_t)n * m > 8192) return "n * m outside [1, 8192]";
  if (C < 2 || C > 4096 || (C & (C - 1))) return "C must be a power of two up to 4096";
  *gbits = 0;
  while ((1 << *gbits) < C) ++*gbits;
  return nullptr;
}
static mb::SessionRows session_rows(const mb_session_rows* r) {
  return mb::SessionRows{r->label, r->seed, r->num_regen, r->slot, r->local_step, r->N, (mb::RequestStep*)r->pool, r->max_active, r->max_steps};
}
int mb_session_row_table(const mb_session_rows* rows, mb_request_step* row_out, int A, mb_stream stream) {
  int gbits;
  if (const char* why = session_rows_check(rows, A, 1, 1, 2, &gbits)) return fail(-1, "mb_session_row_table: %s", why);
  if (!row_out) return fail(-1, "mb_session_row_table: null argument");
  mb::session_row_table((hipStream_t)stream, session_rows(rows), (mb::RequestStep*)row_out, A);
  return launched();
}
int mb_session_admit_rows(const mb_session_rows* rows, int64_t* tokens, int A, int K, const int64_t* labels, const int64_t* seeds, const int* num_steps,
                          const mb_request_step* schedule, const int64_t* init_tokens, int n, int m, int C, mb_stream stream) {
  int gbits;
  if (A < 0 || K < 1) return fail(-1, "mb_session_admit_rows: bad sizes (A = %d, K = %d)", A, K);
  if (const char* why = session_rows_check(rows, A + K, n, m, C, &gbits)) return fail(-1, "mb_session_admit_rows: %s", why);
  if (!tokens || !labels || !seeds || !num_steps || !schedule) return fail(-1, "mb_session_admit_rows: null argument");
  for (int k = 0; k < K; ++k)
    if (num_steps[k] < 1 || num_steps[k] > rows->max_steps) return fail(-1, "mb_session_admit_rows: num_steps[%d] = %d outside [1, %d]", k, num_steps[k], rows->max_steps);
  mb::session_admit((hipStream_t)stream, session_rows(rows), tokens, init_tokens, num_steps, labels, seeds, (const mb::RequestStep*)schedule, A, K, n * m, C);
  return launched();
}
int mb_session_retire(const mb_session_rows* rows, int64_t* tokens, const int64_t* pred, int64_t* codes_all, int64_t* codes_out, int32_t* plan,
                      int A, int n, int m, int C, mb_stream stream) {
  int gbits;
  if (const char* why = session_rows_check(rows, A, n, m, C, &gbits)) return fail(-1, "mb_session_retire: %s", why);
  if (!tokens || !pred || !codes_all || !codes_out || !plan) return fail(-1, "mb_session_retire: null argument");
  mb::session_retire((hipStream_t)stream, session_rows(rows), plan, tokens, pred, codes_all, codes_out, A, n, m, gbits, A, A / 2);   // (at most min(k, A - k) moves)
  return launched();
}

// ---- the image transform's coefficient tables (image.hip) on caller-owned arrays
int mb_image_coeffs(int in_size, int out_size, int filter, int first, int count, int ksize, int32_t* xmin, int32_t* n, int32_t* taps, mb_stream stream) {
  if (!xmin || !n || !taps) return fail(-1, "mb_image_coeffs: null argument");
  if (filter < 0 || filter > 2) return fail(-1, "mb_image_coeffs: filter is 0 (box), 1 (bilinear) or 2 (bicubic), got %d", filter);
  if (in_size < 1 || in_size > mb::IMG_MAX_SIDE || out_size < 1 || out_size > mb::IMG_MAX_SIDE)
    return fail(-1, "mb_image_coeffs: sizes in [1, %d] required (got %d -> %d)", mb::IMG_MAX_SIDE, in_size, out_size);
  if (first < 0 || count < 1 || first > out_size - count) return fail(-1, "mb_image_coeffs: outputs [%d, %d + %d) outside [0, %d)", first, first, count, out_size);
  if (ksize != mb::image_ksize(in_size, out_size, filter)) return fail(-1, "mb_image_coeffs: ksize %d, the axis has %d", ksize, mb::image_ksize(in_size, out_size, filter));
  mb::image_coeffs_launch(in_size, out_size, filter, first, count, ksize, xmin, n, taps, (hipStream_t)stream);
  return launched();
}

// ---- the discriminator's kernels (discriminator.hip), each through the launcher the handle calls
int mb_disc_cols(const float* images, void* cols_h16, int B, int H, int W, int clamp01, mb_stream stream) {
  if (!images || !cols_h16 || B < 1 || H < 1 || W < 1 || (size_t)B * H * W >= (1u << 30)) return fail(-1, "mb_disc_cols: bad arguments");
  mb::launch_disc_cols((hipStream_t)stream, images, (h16*)cols_h16, B, H, W, clamp01);
  return launched();
}
int mb_disc_down_chunks(int Ho, int Wo, int C) { return Ho < 1 || Wo < 1 || C < 8 || C % 8 ? -1 : mb::disc_down_chunks(Ho, Wo, C); }
int mb_disc_downsample(const void* x_h16, void* y_h16, float* part, int B, int H, int W, int C, int K, mb_stream stream) {
  if (!x_h16 || !y_h16) return fail(-1, "mb_disc_downsample: null argument");
  if (K != 0 && (K < 3 || K > 5)) return fail(-1, "mb_disc_downsample: K %d: 3, 4, 5, or 0 for the average pool", K);
  if (B < 1 || B > 65535 || H < 2 || W < 2 || C < 8 || C % 8 || C > 2048 || (size_t)B * H * W >= (1u << 30))
    return fail(-1, "mb_disc_downsample: [%d, %d, %d, %d]: 1 <= B <= 65535, H and W >= 2, C a multiple of 8 up to 2048", B, H, W, C);
  if (part && C % 32) return fail(-1, "mb_disc_downsample: the GroupNorm partials need C %% 32 == 0, got %d", C);
  mb::launch_disc_down((hipStream_t)stream, (const h16*)x_h16, (h16*)y_h16, part, B, H, W, C, K);
  return launched();
}
int mb_disc_groupnorm(void* x_h16, const float* part, int nchunk, const float* gamma, const float* beta, unsigned* saturated, int B, int HW, int C,
                      float slope, mb_stream stream) {
  if (!x_h16 || !part || !gamma || !beta) return fail(-1, "mb_disc_groupnorm: null argument");
  if (B < 1 || B > 65535 || HW < 1 || nchunk < 1 || C < 32 || C % 32 || C > 2048 || !(slope >= 0.f && slope <= 1.f))
    return fail(-1, "mb_disc_groupnorm: B %d, HW %d, C %d, %d chunks, slope %g: C a multiple of 32 up to 2048, slope in [0, 1]", B, HW, C, nchunk, (double)slope);
  hipStream_t s = (hipStream_t)stream;
  mb::DevArena m;
  float2* ss = nullptr;
  unsigned* sat = nullptr;
  m.get(&ss, (size_t)B * C); m.zeroed(&sat, 1);
  if (int rc = m.failed("mb_disc_groupnorm")) return rc;
  mb::launch_disc_gn(s, (h16*)x_h16, part, nchunk, gamma, beta, ss, sat, B, HW, C, mb::DISC_GN_EPS, slope);
  const int rc = launched();
  unsigned nsat = 0;
  const bool ok = hipMemcpyAsync(&nsat, sat, sizeof(unsigned), hipMemcpyDeviceToHost, s) == hipSuccess;
  if (hipStreamSynchronize(s) != hipSuccess || !ok) return fail(-10, "mb_disc_groupnorm: copy failed");     // the scratch is freed on return
  if (saturated) *saturated = nsat;
  return rc;
}
int mb_disc_pool(const void* x_h16, void* y_h16, int B, int H, int W, int C, mb_stream stream) {
  if (!x_h16 || !y_h16) return fail(-1, "mb_disc_pool: null argument");
  if (B < 1 || H < 1 || W < 1 || H > 16384 || W > 16384 || C < 8 || C % 8 || (size_t)B * H * W >= (1u << 30))
    return fail(-1, "mb_disc_pool: [%d, %d, %d, %d]: C a multiple of 8", B, H, W, C);
  mb::launch_disc_pool((hipStream_t)stream, (const h16*)x_h16, (h16*)y_h16, B, H, W, C);
  return launched();
}
int mb_disc_logits(const void* x_h16, const float* w_oihw, const float* bias, float* logits, double* stats, double* sum, int B, int C, mb_stream stream) {
  if (!x_h16 || !w_oihw || !bias) return fail(-1, "mb_disc_logits: null argument");
  if (B < 1 || B > 65535 || C < 8 || C % 8 || C > (1 << 16)) return fail(-1, "mb_disc_logits: B %d, C %d: C a multiple of 8", B, C);
  if (sum && !stats) return fail(-1, "mb_disc_logits: the running sum needs the per-image sums");
  hipStream_t s = (hipStream_t)stream;
  mb::DevArena m;
  float* w = nullptr;
  m.get(&w, (size_t)25 * C);
  if (int rc = m.failed("mb_disc_logits")) return rc;
  mb::launch_disc_logits_weight(s, w_oihw, w, C);
  mb::launch_disc_logits(s, (const h16*)x_h16, w, bias, logits, stats, sum, B, C);
  const int rc = launched();
  if (hipStreamSynchronize(s) != hipSuccess) return fail(-10, "mb_disc_logits: synchronise failed");        // the weights are freed on return
  return rc;
}

}  // extern "C"
