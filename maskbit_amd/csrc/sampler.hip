// What samples with the generator handle (include/maskbit_hip.h): the checked sampling step and its four mb_sample_step* entries, the whole-run loops
// (mb_sample, mb_sample_edit, mb_sample_seeded, mb_sample_requests) and the sampling session (mb_session_*).  Host code only: the kernels are in
// sampling.hip, edit.hip and session.hip, the two forwards (mb::gen_forward, mb::gen_forward_cfg) in engine.hip, the handle's members in mb_gen.h.
#include <hip/hip_runtime.h>

#include "mb_gen.h"

using mb::fail;
using mb::launched;
using mb::ProfScope;

namespace {

// One step, from the four step entries and from the loops.  who: the entry's name in the messages; num_regen != null: the edit step, which reads
// mask_ratio instead of a.k_mask_len; a.seeds != null: the seeded step, which generates its noise from (seeds, step, rand_temp, conf_w) instead of
// reading a.exp_noise / a.conf_noise.  a.tokens is tokens_out, a.pred pred_out, a.P = n m (0: n or m was not positive).
int sample_step_checked(const char* who, const mb::StepArgs& a, const int64_t* tokens_in, const int32_t* num_regen, float mask_ratio, hipStream_t s) {
  if (!a.logits_c || (!a.seeds && (!a.exp_noise || !a.conf_noise)) || !tokens_in || !a.tokens) return fail(-1, "%s: null argument", who);
  if (tokens_in == a.tokens) return fail(-1, "%s: tokens_in and tokens_out must not alias", who);
  if (a.B <= 0 || a.P <= 0 || a.C <= 0) return fail(-1, "%s: bad sizes", who);
  ProfScope p(a.req ? "sample_step_requests" : a.seeds ? "sample_step_seeded" : num_regen ? "sample_step_edit" : "sample_step", s);
  if (mb::sample_step(s, a, tokens_in, num_regen, mask_ratio)) return fail(-1, "%s: C=%d or n*m=%d too large", who, a.C, a.P);
  return launched();
}

int step_slots(int n, int m) { return n > 0 && m > 0 ? n * m : 0; }

// What all four step entries fill alike; each adds its own fields, and its own null and alias checks under its own name
mb::StepArgs step_args(const float* logits_c, const float* logits_u, int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C) {
  mb::StepArgs a{};
  a.logits_c = logits_c; a.logits_u = logits_u; a.tokens = tokens_out; a.pred = pred_out; a.B = B; a.P = step_slots(n, m); a.C = C;
  return a;
}

}  // namespace

extern "C" {

int mb_sample_step(const float* logits_c, const float* logits_u, float scale, float temperature,
                   const float* exp_noise, const float* conf_noise, int k_mask_len, const int64_t* tokens_in,
                   int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C, mb_stream stream) {
  mb::StepArgs a = step_args(logits_c, logits_u, tokens_out, pred_out, B, n, m, C);
  a.scale = scale; a.temperature = temperature; a.exp_noise = exp_noise; a.conf_noise = conf_noise; a.k_mask_len = k_mask_len;
  return sample_step_checked("mb_sample_step", a, tokens_in, nullptr, 0.f, (hipStream_t)stream);
}

int mb_sample_step_edit(const float* logits_c, const float* logits_u, float scale, float temperature, const float* exp_noise, const float* conf_noise,
                        float mask_ratio, const int32_t* num_regen, const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out, int B, int n, int m,
                        int C, mb_stream stream) {
  if (!num_regen) return fail(-1, "mb_sample_step_edit: null argument");
  mb::StepArgs a = step_args(logits_c, logits_u, tokens_out, pred_out, B, n, m, C);
  a.scale = scale; a.temperature = temperature; a.exp_noise = exp_noise; a.conf_noise = conf_noise;
  return sample_step_checked("mb_sample_step_edit", a, tokens_in, num_regen, mask_ratio, (hipStream_t)stream);
}

int mb_sample_step_seeded(const float* logits_c, const float* logits_u, float scale, float temperature, const int64_t* seeds, int step,
                          float randomize_temperature, float conf_weight, float mask_ratio, const int32_t* num_regen, const int64_t* tokens_in,
                          int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C, mb_stream stream) {
  if (!seeds || !num_regen) return fail(-1, "mb_sample_step_seeded: null argument");
  if (step < 0) return fail(-1, "mb_sample_step_seeded: step = %d is negative", step);
  if (pred_out && (pred_out == tokens_out || pred_out == tokens_in)) return fail(-1, "mb_sample_step_seeded: pred_out must not alias tokens_in or tokens_out");
  mb::StepArgs a = step_args(logits_c, logits_u, tokens_out, pred_out, B, n, m, C);
  a.scale = scale; a.temperature = temperature; a.seeds = seeds; a.step = step; a.rand_temp = randomize_temperature; a.conf_w = conf_weight;
  return sample_step_checked("mb_sample_step_seeded", a, tokens_in, num_regen, mask_ratio, (hipStream_t)stream);
}

static_assert(sizeof(mb::RequestStep) == sizeof(mb_request_step) && sizeof(mb_request_step) == 24, "mb_request_step is the kernels' RequestStep");

int mb_sample_step_requests(const float* logits_c, const float* logits_u, const mb_request_step* table_row, const int64_t* seeds, const int32_t* num_regen,
                            const int64_t* tokens_in, int64_t* tokens_out, int64_t* pred_out, int B, int n, int m, int C, mb_stream stream) {
  if (!table_row || !seeds || !num_regen) return fail(-1, "mb_sample_step_requests: null argument");
  if (pred_out && (pred_out == tokens_out || pred_out == tokens_in)) return fail(-1, "mb_sample_step_requests: pred_out must not alias tokens_in or tokens_out");
  mb::StepArgs a = step_args(logits_c, logits_u, tokens_out, pred_out, B, n, m, C);
  a.seeds = seeds; a.req = (const mb::RequestStep*)table_row;
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

// The READY MARK, mb_gen::Run::cfg_labels / cfg_B: the one piece of hidden state of the sampling path.  cfg_labels == L and cfg_B == B say that the
// handle's lab_cfg / drop_cfg hold [L | L] / [0 | 1] for B pairs, so a gen_forward_cfg over (L, B) does not write them again.  Its contract:
//  - forward_and_step alone sets it, after a guided forward that returned 0;
//  - gen_forward_cfg clears it whenever it overwrites lab_cfg, whoever called (mb_gen_forward_cfg, a larger prefix, a batch of several passes);
//  - sample_run and sample_requests_run hold a CfgReady: their labels are the caller's buffer, which may be gone or refilled by the next call, so the
//    mark is clear when their loop begins and on every return path of their call;
//  - a session's labels are its own buffer at a fixed address, so its mark outlives a tick (nothing in between leaves a mark behind), but never a
//    change of membership, which changes what that address holds: session_drop_mark, on the tick after an admit and with every retire.
struct CfgReady {
  mb_gen::Run& run;
  explicit CfgReady(mb_gen::Run& r) : run(r) { clear(); }
  ~CfgReady() { clear(); }
  void clear() { run.cfg_labels = nullptr; }
};

// One global step of sampling, for all three loops: the guided or the plain forward over the B sequences of cur, then the checked step on g->logits.
// a holds the step's arguments but logits_u, which depends on the forward alone.  The mark: ready for (labels, B) where one pass held the B pairs,
// clear where not -- what each loop did by itself (sample_run without the clear: gen_forward_cfg has cleared it in that case, so one rule changes
// nothing); after a forward that FAILED the mark stays as gen_forward_cfg left it, which is never ready for rows it did not finish writing.
int forward_and_step(mb_gen* g, const char* who, mb::StepArgs& a, const int64_t* cur, const int64_t* labels, int B, bool guided_forward, const int32_t* num_regen, float mask_ratio, hipStream_t s) {
  a.logits_u = guided_forward ? g->logits + (size_t)B * a.P * a.C : nullptr;
  if (int rc = guided_forward ? mb::gen_forward_cfg(g, cur, labels, g->logits, B, s) : mb::gen_forward(g, cur, labels, nullptr, g->logits, B, s)) return rc;
  if (guided_forward) { g->run.cfg_labels = B <= g->chunk_seqs / 2 ? labels : nullptr; g->run.cfg_B = B; }
  return sample_step_checked(who, a, cur, num_regen, mask_ratio, s);
}

// The start state of a run, in tok_a (sampling.py:65-71): the caller's tokens, num_regen[b] = sample b's masked count; or every position masked and, where
// the run's steps read the counts (`counts`), the per-sample rule from that state: num_regen[b] = n m
void load_start_state(mb_gen* g, const int64_t* init_tokens, bool counts, int B, hipStream_t s) {
  const int P = g->c.seq * g->c.splits, C = g->C;
  if (init_tokens) { mb::edit_load_tokens(s, init_tokens, g->tok_a, g->num_regen, B, P, C); return; }
  mb::fill_i64(s, g->tok_a, (int64_t)C, (size_t)B * P);
  if (counts) mb::edit_load_tokens(s, g->tok_a, nullptr, g->num_regen, B, P, C);
}

// The end of a run: combine_factorized_tokens (factorization.py:7-24) on the LAST step's predictions, kept as integers; the decoder, if there is one
int finish_run(mb_gen* g, mb_dec* d, const int64_t* last_pred, int B, const RunOut& out, hipStream_t s) {
  int64_t* codes = out.codes ? out.codes : g->codes;
  mb::combine_groups(s, last_pred, codes, (size_t)B * g->c.seq, g->c.splits, g->gbits);
  if (int rc = d ? mb_dec_decode(d, codes, out.img_nchw, out.img_nhwc_u8, B, (mb_stream)s) : 0) return rc;
  return launched();
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
  const size_t P = (size_t)c.seq * c.splits;
  // A run may be fed in step chunks (plan->step_begin / step_end: the noise of a whole 256-step run at batch 100 is 6.7 GB): chunk [0, e) starts from
  // the start state (every position masked, or the caller's tokens), later chunks continue from the token state the engine kept; exp_noise /
  // conf_noise / step_tokens hold THIS chunk's steps.
  const int s0 = r.step_end > 0 ? r.step_begin : 0, s1 = r.step_end > 0 ? r.step_end : num_steps;
  if (s0 < 0 || s1 > num_steps || s0 >= s1) return fail(-1, "%s: step chunk [%d, %d) outside [0, %d)", who, s0, s1, num_steps);
  // A run fed in chunks keeps its token state in the engine: a chunk is accepted only as the exact continuation of the run in progress (same batch,
  // plan length, guidance flag and kind -- plain, edit or seeded --, beginning where the previous chunk ended).  The handle is not re-entrant while a run is in progress.
  mb_gen::Run& run = g->run;
  if (s0 == 0) {
    load_start_state(g, r.init_tokens, seeded, B, s);
    run.id = id;
  }
  else if (!(run.id == id && run.next == s0))
    return fail(-1, "%s: step chunk [%d, %d) of a %d-step %s run with B = %d does not continue the run in progress (next step %d of %d, B = %d, %s %s run)",
                who, s0, s1, num_steps, kRunKind[id.kind], B, run.next, run.id.steps, run.id.B, run.id.kind == 1 ? "an" : "a", kRunKind[run.id.kind]);
  run.next = -1;                                       // (set again below when this chunk has been enqueued and more follow)
  int64_t* cur = (s0 & 1) ? g->tok_b : g->tok_a;
  int64_t* nxt = (s0 & 1) ? g->tok_a : g->tok_b;
  int64_t* last_pred = g->pred;
  CfgReady cfg_ready(run);
  mb::StepArgs a{};
  a.logits_c = g->logits; a.B = B; a.P = (int)P; a.C = g->C;
  a.seeds = nz.seeds; a.rand_temp = nz.rand_temp;
  for (int i = s0; i < s1; ++i) {
    // sampling.py:98-99 combines c + s_i (c - u).  Where the annealed scale s_i is exactly 0 -- the first steps of the cosine schedule: (i / N)^p pi
    // is below float32's cos() resolution -- the unconditional logits do not enter the result (c + 0 (c - u) == c for finite logits), so that
    // forward is not run: the step is the plain conditional forward, bit for bit what the guided expression evaluates to.
    // (precision 4: the guided forward is also the MORE PRECISE conditional forward -- its pair tiles carry the activation-lo sets, the plain tiles do not --
    // and the first, almost fully masked steps are where near-ties flip: the zero-scale steps run it too; its unconditional half is then multiplied by 0)
    const bool guided_forward = id.guided && (r.scale[i] != 0.0f || (!g->f32 && g->pair_ok && c.precision >= 4));
    const size_t k = (size_t)(i - s0);                 // the noise / step_tokens buffers hold this chunk's steps
    a.scale = r.scale[i]; a.temperature = r.temperature[i];
    a.tokens = nxt; a.pred = out.step_tokens ? out.step_tokens + k * B * P : g->pred;
    if (seeded) { a.step = i; a.conf_w = nz.conf_weight[i]; }
    else { a.exp_noise = nz.exp_noise + k * B * P * a.C; a.conf_noise = nz.conf_noise + k * B * P; }
    if (!edit) a.k_mask_len = r.mask_len[i];
    if (int rc = forward_and_step(g, kStepEntry[id.kind], a, cur, labels, B, guided_forward, edit ? g->num_regen : nullptr, edit ? r.mask_ratio[i] : 0.f, s)) return rc;
    last_pred = a.pred;
    int64_t* t = cur; cur = nxt; nxt = t;
  }
  if (s1 < num_steps) {                                // more chunks follow: keep the last predictions only if they are the engine's own buffer
    if (int rc = launched()) return rc;
    run.next = s1;
    return 0;
  }
  return finish_run(g, d, last_pred, B, out, s);
}

// The fourth kind of run, "requests" (include/maskbit_hip.h "per-sample sampling arguments"): a seeded run whose step t covers the prefix
// [0, active[t]) of the batch and whose step kernels read their constants per sample from plan.table.  A sibling of sample_run on the same pieces --
// load_start_state, forward_and_step, finish_run -- with none of its step chunks.  Every argument check is in front of the
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
  const size_t P = (size_t)g->c.seq * g->c.splits;
  mb_gen::Run& run = g->run;
  run.next = -1;                                       // ends any run in progress: no chunk of another kind continues this one
  // The start state in BOTH token buffers: a request that becomes active at step t reads whichever buffer is `cur` then, and nothing has touched its rows
  load_start_state(g, init_tokens, true, B, s);
  HIP_TRY(hipMemcpyAsync(g->tok_b, g->tok_a, (size_t)B * P * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  int64_t* cur = g->tok_a;
  int64_t* nxt = g->tok_b;
  int64_t* last_pred = g->pred;
  CfgReady cfg_ready(run);
  mb::StepArgs a{};
  a.logits_c = g->logits; a.P = (int)P; a.C = g->C;
  a.seeds = seeds;
  for (int t = 0; t < S; ++t) {
    // The forward is chosen by the run's flag alone, never by the scales of the step: a request with scale 0 gets c + 0 (c - u) from the guided forward.
    // (A mark stays valid until the prefix grows: gen_forward_cfg then refreshes lab_cfg / drop_cfg.)
    a.B = plan.active[t];
    a.req = (const mb::RequestStep*)plan.table + (size_t)t * B;
    a.tokens = nxt; a.pred = out.step_tokens ? out.step_tokens + (size_t)t * B * P : g->pred;
    if (int rc = forward_and_step(g, who, a, cur, labels, a.B, guided, g->num_regen, 0.f, s)) return rc;
    last_pred = a.pred;                                // (the last step runs all B requests: its predictions are the whole batch's)
    int64_t* tmp = cur; cur = nxt; nxt = tmp;
  }
  return finish_run(g, d, last_pred, B, out, s);
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

// The session's membership changed: the handle's ready mark, if it is this session's, ends (the contract: CfgReady)
void session_drop_mark(const mb_session* s, mb_gen* g) { if (g->run.cfg_labels == s->st.label) g->run.cfg_labels = nullptr; }

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
  s->cfg_dirty = true;                                   // (no handle here: the next tick drops the mark)
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
  g->run.next = -1;                                      // ends any chunked run in progress, as mb_sample_requests does
  // 1. the step's table row, gathered on the device
  mb::session_row_table(st, s->st, s->row, A);
  // 2. one global step of sample_requests_run over the A rows, on the mark the last tick left unless the membership changed since
  int64_t* cur = s->tok[s->cur];
  if (s->cfg_dirty) session_drop_mark(s, g);
  if (s->guided) s->cfg_dirty = false;                   // (the guided forward below fills lab_cfg / drop_cfg from the members of now)
  mb::StepArgs a{};
  a.logits_c = g->logits; a.B = A; a.P = (int)s->P; a.C = s->C;
  a.seeds = s->st.seed; a.req = s->row;
  int64_t* pred = pred_out ? pred_out : s->pred;
  a.tokens = s->tok[s->cur ^ 1]; a.pred = pred;
  if (int rc = forward_and_step(g, who, a, cur, s->st.label, A, s->guided, s->st.num_regen, 0.f, st)) return rc;
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
  session_drop_mark(s, g);
  int64_t* codes = codes_out ? codes_out : s->codes;
  mb::session_retire(st, s->st, s->plan, s->tok[s->cur], pred, s->codes_all, codes, A, s->n, s->m, s->gbits, k, moves);
  // 4. decode the k finished requests
  if (d && (img_nchw || img_nhwc_u8)) {
    int rc = mb_dec_decode(d, codes, img_nchw, img_nhwc_u8, k, (mb_stream)st);
    if (rc) return rc;
  }
  return launched();
}

}  // extern "C"
