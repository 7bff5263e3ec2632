// The device-side bookkeeping of a sampling session (include/maskbit_hip.h "sampling session"; the host side is mb_session_* in sampler.hip): the
// active requests are the dense row prefix [0, A) of the session's buffers, and membership changes at every tick without a host round trip.
//   session_row_table_kernel -- row[r] = pool[slot[r]][local_step[r]], local_step[r] += 1: the step's table row, gathered from the schedule pool.
//   session_admit_kernel     -- K new rows at [A, A + K): label, seed, N, local step 0, and the request's N schedule records into the row's pool slot
//                               (the tokens and their masked count are edit.hip's edit_load_tokens).
//   session_plan_kernel      -- ONE workgroup reads local_step / N once and writes the snapshot every later kernel of the tick acts on: the finished
//                               rows F (ascending), the holes H = F below A' = A - |F| and the movers M = the unfinished rows at or above A'.
//   session_gather_kernel    -- codes_out[j] = codes_all[F[j]]: the finished rows' combined codes, in ascending row order.
//   session_move_kernel      -- row M[j] -> row H[j]: tokens and every per-row field; one workgroup per (move, 4 KiB chunk of the token row).
// The move kernel never looks at local_step / N to decide anything -- it overwrites local_step[dst] while other workgroups are still running --: the
// snapshot is the decision.  Sources lie at or above A', destinations below: the moves are disjoint and run in parallel in place.
// slot[] is a permutation of [0, max_active): rows [0, A) hold the pool slots in use, the rows above the free ones.  A move SWAPS the two rows'
// slots, so the finished row's slot ends up above A' and is free again.
// No atomics, nothing allocated, nothing synchronises.
#include <algorithm>

#include "mb_abi.h"
#include "mb_kernels.h"

namespace mb {

namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_CHUNK = 512;   // int64 of a token row per move workgroup: 256 lanes x 16 bytes

static_assert(sizeof(RequestStep) == 24, "a schedule record is three 8-byte words");

__device__ __forceinline__ void copy_record(RequestStep* __restrict__ dst, const RequestStep* __restrict__ src) {
  const uint2* s = (const uint2*)src;                  // (records are 24 bytes from a 256-byte aligned base: 8-byte aligned)
  uint2* d = (uint2*)dst;
  const uint2 a = s[0], b = s[1], c = s[2];
  d[0] = a; d[1] = b; d[2] = c;
}

__global__ __launch_bounds__(SE_THREADS) void session_row_table_kernel(SessionRows st, RequestStep* __restrict__ row, int A) {
  const int r = blockIdx.x * SE_THREADS + threadIdx.x;
  if (r >= A) return;
  // (slot and local step are the session's own values; clamped all the same, so that a damaged state cannot index outside the pool)
  const int slot = min(max(st.slot[r], 0), st.cap - 1);
  const int ls = st.local_step[r];
  copy_record(row + r, st.pool + (size_t)slot * st.max_steps + min(max(ls, 0), st.max_steps - 1));
  st.local_step[r] = ls + 1;
}

__global__ __launch_bounds__(SE_THREADS) void session_admit_kernel(SessionRows st, AdmitBatch b, const int64_t* __restrict__ labels,
                                                                   const int64_t* __restrict__ seeds, const RequestStep* __restrict__ sched, int A) {
  const int k = blockIdx.x, r = A + k;
  if (r >= st.cap) return;
  const int N = min(b.n[k], st.max_steps);
  const int slot = min(max(st.slot[r], 0), st.cap - 1);
  for (int i = threadIdx.x; i < N; i += SE_THREADS) copy_record(st.pool + (size_t)slot * st.max_steps + i, sched + (size_t)b.off[k] + i);
  if (threadIdx.x == 0) {
    st.label[r] = labels[k];
    st.seed[r] = seeds[k];
    st.N[r] = N;
    st.local_step[r] = 0;
  }
}

// Exclusive rank of `flag` among the workgroup's threads in thread order, and the workgroup's total: ballot per wave, the waves' totals through LDS.
// part: LDS [SE_THREADS / 64]; the caller separates two uses of the same part[] by a barrier.
__device__ __forceinline__ int block_rank(bool flag, int* part, int* total) {
  const unsigned long long bal = __ballot(flag);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = __popcll(bal);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < SE_THREADS / 64; ++w) { before += w < wave ? part[w] : 0; all += part[w]; }
  *total = all;
  return before + __popcll(bal & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(SE_THREADS) void session_plan_kernel(SessionRows st, int* __restrict__ plan, int A) {
  __shared__ int part[3][SE_THREADS / 64];
  const int cap = st.cap;
  int* fin = plan + 2; int* src = fin + cap; int* dst = src + cap;
  // pass 1: k = |F|, hence A'
  int k = 0;
  for (int base = 0; base < A; base += SE_THREADS) {
    const int r = base + threadIdx.x;
    int total;
    block_rank(r < A && st.local_step[r] == st.N[r], part[0], &total);
    k += total;
    __syncthreads();
  }
  const int Ap = A - k;
  // pass 2: the three lists, each ascending: chunks of SE_THREADS rows in row order, the ranks of the chunks before in nf / nh / nm
  int nf = 0, nh = 0, nm = 0;
  for (int base = 0; base < A; base += SE_THREADS) {
    const int r = base + threadIdx.x;
    const bool in = r < A, done = in && st.local_step[r] == st.N[r];
    const bool hole = done && r < Ap, mover = in && !done && r >= Ap;
    int tf, th, tm;
    const int rf = block_rank(done, part[0], &tf), rh = block_rank(hole, part[1], &th), rm = block_rank(mover, part[2], &tm);
    if (done) fin[nf + rf] = r;
    if (hole) dst[nh + rh] = r;
    if (mover) src[nm + rm] = r;
    nf += tf; nh += th; nm += tm;
    __syncthreads();
  }
  if (threadIdx.x == 0) { plan[0] = k; plan[1] = nh; }   // (|H| = |M|: both count the rows that change sides of A')
}

__global__ __launch_bounds__(SE_THREADS) void session_gather_kernel(const int* __restrict__ plan, int cap, const int64_t* __restrict__ codes_all,
                                                                    int64_t* __restrict__ codes_out, int n) {
  const int j = blockIdx.x;
  if (j >= plan[0]) return;
  const int r = plan[2 + j];
  if (r < 0 || r >= cap) return;
  const int i = blockIdx.y * SE_THREADS + threadIdx.x;
  if (i < n) codes_out[(size_t)j * n + i] = codes_all[(size_t)r * n + i];
}

// VEC: token rows of an even number of int64 start 16-byte aligned (the base is): one 16-byte load and store per lane; odd P: two 8-byte ones.
template <bool VEC>
__global__ __launch_bounds__(SE_THREADS) void session_move_kernel(SessionRows st, const int* __restrict__ plan, int64_t* __restrict__ tokens, int P) {
  const int j = blockIdx.x, cap = st.cap;
  if (j >= plan[1]) return;
  const int s = plan[2 + cap + j], d = plan[2 + 2 * cap + j];
  if (s < 0 || s >= cap || d < 0 || d >= cap || s == d) return;
  const int64_t* from = tokens + (size_t)s * P;
  int64_t* to = tokens + (size_t)d * P;
  if (VEC) {
    const int i = blockIdx.y * SE_THREADS + threadIdx.x;
    if (i < P / 2) ((uint4*)to)[i] = ((const uint4*)from)[i];
  } else {
    for (int i = blockIdx.y * SE_CHUNK + threadIdx.x; i < min(P, (int)(blockIdx.y + 1) * SE_CHUNK); i += SE_THREADS) to[i] = from[i];
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    st.label[d] = st.label[s];
    st.seed[d] = st.seed[s];
    st.num_regen[d] = st.num_regen[s];
    st.local_step[d] = st.local_step[s];
    st.N[d] = st.N[s];
    const int freed = st.slot[d];                      // the finished row's pool slot goes where the mover was: above A', free again
    st.slot[d] = st.slot[s];
    st.slot[s] = freed;
  }
}

}  // namespace

void session_row_table(hipStream_t s, const SessionRows& st, RequestStep* row, int A) {
  ProfScope p("session_row_table", s);
  hipLaunchKernelGGL(session_row_table_kernel, dim3((A + SE_THREADS - 1) / SE_THREADS), dim3(SE_THREADS), 0, s, st, row, A);
}

void session_admit(hipStream_t s, const SessionRows& st, int64_t* tokens, const int64_t* init_tokens, const int* num_steps, const int64_t* labels,
                   const int64_t* seeds, const RequestStep* sched, int A, int K, int P, int C) {
  ProfScope p("session_admit", s);
  int64_t* dst = tokens + (size_t)A * P;
  if (init_tokens) edit_load_tokens(s, init_tokens, dst, st.num_regen + A, K, P, C);   // the caller's tokens, clamped; num_regen = the row's masked count
  else {
    fill_i64(s, dst, (int64_t)C, (size_t)K * P);
    edit_load_tokens(s, dst, nullptr, st.num_regen + A, K, P, C);                     // the per-sample rule from the all-masked state: num_regen = P
  }
  int off = 0;
  for (int k0 = 0; k0 < K; k0 += AdmitBatch::MAX) {
    const int kc = std::min(K - k0, (int)AdmitBatch::MAX);
    AdmitBatch b{};
    for (int k = 0; k < kc; ++k) { b.n[k] = num_steps[k0 + k]; b.off[k] = off; off += num_steps[k0 + k]; }
    hipLaunchKernelGGL(session_admit_kernel, dim3(kc), dim3(SE_THREADS), 0, s, st, b, labels + k0, seeds + k0, sched, A + k0);
  }
}

void session_retire(hipStream_t s, const SessionRows& st, int* plan, int64_t* tokens, const int64_t* pred, int64_t* codes_all, int64_t* codes_out,
                    int A, int n, int m, int gbits, int k, int moves) {
  { ProfScope p("session_plan", s);
    hipLaunchKernelGGL(session_plan_kernel, dim3(1), dim3(SE_THREADS), 0, s, st, plan, A); }
  if (k > 0) {
    ProfScope p("session_codes", s);
    combine_groups(s, pred, codes_all, (size_t)A * n, m, gbits);
    hipLaunchKernelGGL(session_gather_kernel, dim3(k, (n + SE_THREADS - 1) / SE_THREADS), dim3(SE_THREADS), 0, s, plan, st.cap, codes_all, codes_out, n);
  }
  if (moves > 0) {
    ProfScope p("session_move", s);
    const int P = n * m;
    const dim3 grid(moves, (P + SE_CHUNK - 1) / SE_CHUNK), block(SE_THREADS);
    if (P % 2 == 0 && (uintptr_t)tokens % 16 == 0) hipLaunchKernelGGL(session_move_kernel<true>, grid, block, 0, s, st, plan, tokens, P);
    else hipLaunchKernelGGL(session_move_kernel<false>, grid, block, 0, s, st, plan, tokens, P);
  }
}

}  // namespace mb
