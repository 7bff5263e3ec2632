// The k-NN manifolds behind the improved precision / recall of Kynkaanniemi et al. (ADM's evaluator: manifold_radii / evaluate_pr, k = 3 on pool
// features) on gfx950: all pairwise squared distances of two sets of rows, reduced per row on the fly, in fp64 on v_mfma_f64_16x16x4_f64.  The
// N x N matrix is never in memory.
//
// Definition.  For rows a, b of width D (fp32 widened exactly, or fp64):  d2(a, b) = max(0, fma(-2, a.b, |a|^2 + |b|^2)).
//   |a|^2 (row_norms_kernel, once per row into the workspace): lane l of a wave chains d = l, l + 64, ... by fma from 0, then the 64 partial sums
//     are added by an xor butterfly (32, 16, .. 1) -- addition commutes, so every lane ends with the same bits.
//   a.b: the MFMA accumulator starts at 0 and takes, for s = 0, 1, .. and e = 0..7 in that order, the four products at
//     d = 32 s + 8 q + e, q = 0..3 (one instruction).  Lane (row l & 15, q = l >> 4) reads 8 CONSECUTIVE values d = 32 s + 8 q .. + 7 of its row
//     (32 or 64 bytes: a wave's load takes whole 128-byte lines of fp32 rows) and instruction e contracts element e of every lane: a fixed
//     bijection of d, the same for both operands.  Columns past D load as exact zeros.
//   Neither order depends on where a row sits in its matrix, on N, or on the launch geometry, so the value a row sees for another row is a
//   function of the two rows alone (which one is the A operand is fixed too: the row that owns the list / the query).
//
// A workgroup of four waves owns 128 rows and one of up to 16 parts of the column walk (parts_for: more workgroups than row blocks, so that the
// last round of them is short); a wave owns 32 rows (two strips of 16) and walks the part's column tiles of 64 rows of the other set, eight 16 x 16
// accumulators at a time, straight from global memory (the four waves read the same column tile: L1).  f64 C/D layout: col = lane & 15,
// row = (lane >> 4) + 4 * reg -- a lane keeps, for each of its 8 rows, the smallest values of ITS column residue as a sorted list in registers
// (knn_lists_kernel: 4 values for k <= 3, else 9) or one flag (cover_flags_kernel); the 16 lanes of a row are merged once, after the walk, by an
// xor butterfly over lanes 1, 2, 4, 8 (disjoint column sets, so multiplicity is kept), and a second small kernel merges the parts
// (knn_merge_kernel takes the (k+1)-th smallest, cover_merge_kernel the OR).  Rows and columns past the edge load a clamped row and are never looked at: a phantom column enters no list and no
// OR, a phantom row is not stored.  The diagonal of mb_knn_radii is forced to 0.  No floating-point atomics: every output is written by one
// thread, bitwise reproducible.  The N x N matrix never exists; the workspace holds a norm and the parts' lists or flags per row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/maskbit_hip.h"
#include "mb_abi.h"

namespace mb {

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int MF_MAX_N = 1 << 24;        // rows of one call (mb_manifold_cover: queries + base)
constexpr int MF_MAX_D = 1 << 20;
constexpr int MF_MAX_K = 8;
constexpr int MF_SLOTS = MF_MAX_K + 1;   // list length: the k + 1 smallest, k <= 8 (k <= 3 runs with lists of 4)
constexpr int MF_TILE = 64;              // columns per step of the walk
constexpr int MF_SLAB = 32;              // contraction values per step of a tile: 8 instructions
constexpr int MF_MAX_SPLITS = 16;        // parts the column walk of a row block is cut into, for more workgroups than row blocks
constexpr int MF_MR = 2;                 // 16-row strips per wave: a wave's tile is 32 x 64, a workgroup's 128 x 64
constexpr int MF_BLOCK = 4 * 16 * MF_MR; // rows per workgroup

// 8 consecutive values d .. d + 7 of a row, as stored; past D exact zeros
template <class T>
__device__ __forceinline__ void load8_guarded(const T* __restrict__ row, int d, int D, T (&v)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = d + e < D ? row[d + e] : T(0);
}
// the same for a slab that lies inside D, of a row whose base and stride allow 16-byte loads
template <class T>
__device__ __forceinline__ void load8_whole(const T* __restrict__ row, int d, T (&v)[8]) {
  typedef T vec4 __attribute__((ext_vector_type(4), aligned(16)));
  const vec4 lo = *(const vec4*)(row + d), hi = *(const vec4*)(row + d + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
}

// grid (ceil(N / 4)), 256 threads: a wave per row
template <class T>
__global__ __launch_bounds__(256) void row_norms_kernel(const T* __restrict__ x, int N, int D, int64_t row_stride, double* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                      // wave-uniform
  const T* __restrict__ p = x + (int64_t)n * row_stride;
  double s = 0.0;
  for (int d = lane; d < D; d += 64) {
    const double v = (double)p[d];
    s = __fma_rn(v, v, s);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) norms[n] = s;
}

// One slab (contraction values d0 .. d0 + 31) of a wave's operands: 8 values of each of its 2 + 4 rows per lane.  `vec` and the test against D
// are wave-uniform, so the walk has ONE branch around its twelve 16-byte loads and none of them waits for another.
template <class TA, class TB>
__device__ __forceinline__ void load_slab(const TA* const (&pa)[MF_MR], const TB* const (&pb)[4], int d, int d0, int D, bool vec, TA (&ua)[MF_MR][8],
                                          TB (&ub)[4][8]) {
  if (vec && d0 + MF_SLAB <= D) {
#pragma unroll
    for (int m = 0; m < MF_MR; ++m) load8_whole(pa[m], d, ua[m]);
#pragma unroll
    for (int t = 0; t < 4; ++t) load8_whole(pb[t], d, ub[t]);
  } else {
#pragma unroll
    for (int m = 0; m < MF_MR; ++m) load8_guarded(pa[m], d, D, ua[m]);
#pragma unroll
    for (int t = 0; t < 4; ++t) load8_guarded(pb[t], d, D, ub[t]);
  }
  __builtin_amdgcn_sched_barrier(0);                       // issued before the instructions that follow: they run under these loads
}

template <class TA, class TB>
__device__ __forceinline__ void mma_slab(const TA (&ua)[MF_MR][8], const TB (&ub)[4][8], f64x4 (&acc)[MF_MR][4]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const double bv = (double)ub[t][e];
#pragma unroll
      for (int m = 0; m < MF_MR; ++m) acc[m][t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)ua[m][e], bv, acc[m][t], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);                     // widen step by step: all 48 values widened ahead would not fit the registers
  }
}

// The 32 x 64 tile of dot products of a wave: rows i0 .. i0 + 31 of a (clamped to Na - 1) against rows j0 .. j0 + 63 of b (clamped to Nb - 1),
// acc[m][t] = strip m (16 rows) x 16 columns.  Two sets of load registers take the slabs in turn: the loads of one slab fly under the 64
// instructions of the other, and no value is copied.
template <class TA, class TB>
__device__ __forceinline__ void dot_tile(const TA* __restrict__ a, int64_t a_stride, int Na, const TB* __restrict__ b, int64_t b_stride, int Nb,
                                         bool vec, int D, int i0, int j0, int lane, f64x4 (&acc)[MF_MR][4]) {
  const int lc = lane & 15, dq = 8 * (lane >> 4);
  const TA* pa[MF_MR];
  const TB* pb[4];
#pragma unroll
  for (int m = 0; m < MF_MR; ++m) pa[m] = a + (int64_t)min(i0 + 16 * m + lc, Na - 1) * a_stride;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    pb[t] = b + (int64_t)min(j0 + 16 * t + lc, Nb - 1) * b_stride;
#pragma unroll
    for (int m = 0; m < MF_MR; ++m) acc[m][t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  TA xa[MF_MR][8], ya[MF_MR][8];
  TB xb[4][8], yb[4][8];
  load_slab(pa, pb, dq, 0, D, vec, xa, xb);
  for (int d0 = 0; d0 < D; d0 += 2 * MF_SLAB) {
    const bool second = d0 + MF_SLAB < D;
    if (second) load_slab(pa, pb, d0 + MF_SLAB + dq, d0 + MF_SLAB, D, vec, ya, yb);
    mma_slab(xa, xb, acc);
    if (d0 + 2 * MF_SLAB < D) load_slab(pa, pb, d0 + 2 * MF_SLAB + dq, d0 + 2 * MF_SLAB, D, vec, xa, xb);
    if (second) mma_slab(ya, yb, acc);
  }
}

__device__ __forceinline__ double dist2(double na, double nb, double dot) { return fmax(0.0, __fma_rn(-2.0, dot, na + nb)); }

// sorted ascending list, keeps the SLOTS smallest with multiplicity
template <int SLOTS>
__device__ __forceinline__ void list_insert(double (&list)[SLOTS], double v) {
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const double lo = fmin(list[s], v);
    v = fmax(list[s], v);
    list[s] = lo;
  }
}

// the column tiles [first, last) of part y of `parts`
__device__ __forceinline__ void tile_range(int n_cols, int y, int parts, int& first, int& last) {
  const int tiles = (n_cols + MF_TILE - 1) / MF_TILE, per = (tiles + parts - 1) / parts;
  first = min(tiles, y * per);
  last = min(tiles, first + per);
}

// grid (ceil(N / 128), parts), 256 threads; part [parts][N][SLOTS]: per row the SLOTS smallest values of the part's columns
template <class T, int SLOTS>
__global__ __launch_bounds__(256) void knn_lists_kernel(const T* __restrict__ x, int N, int D, int64_t row_stride, bool vec, const double* __restrict__ norms,
                                              double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = (blockIdx.x * 4 + wave) * 16 * MF_MR;
  if (i0 >= N) return;                                     // wave-uniform; no barrier in this kernel
  const int lc = lane & 15, lr = lane >> 4;
  double list[MF_MR][4][SLOTS], na[MF_MR][4];
#pragma unroll
  for (int m = 0; m < MF_MR; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      na[m][r] = norms[min(i0 + 16 * m + lr + 4 * r, N - 1)];
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) list[m][r][s] = INFINITY;
    }
  }
  int first, last;
  tile_range(N, blockIdx.y, gridDim.y, first, last);
  for (int j0 = first * MF_TILE; j0 < last * MF_TILE; j0 += MF_TILE) {
    f64x4 acc[MF_MR][4];
    dot_tile(x, row_stride, N, x, row_stride, N, vec, D, i0, j0, lane, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = j0 + 16 * t + lc;
      if (col < N) {
        const double nb = norms[col];
#pragma unroll
        for (int m = 0; m < MF_MR; ++m) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double v = (col == i0 + 16 * m + lr + 4 * r) ? 0.0 : dist2(na[m][r], nb, acc[m][t][r]);
            if (v < list[m][r][SLOTS - 1]) list_insert(list[m][r], v);
          }
        }
      }
    }
  }
  // the 16 lanes of a row hold disjoint column sets: after the four exchanges every one of them holds the smallest SLOTS of the row's part
#pragma unroll
  for (int m = 0; m < MF_MR; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) {
        double other[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) other[s] = __shfl_xor(list[m][r][s], o);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) list_insert(list[m][r], other[s]);
      }
      const int row = i0 + 16 * m + lr + 4 * r;
      if (lc == 0 && row < N) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) part[((size_t)blockIdx.y * N + row) * SLOTS + s] = list[m][r][s];
      }
    }
  }
}

// grid (ceil(N / 256)): a thread per row merges the parts (disjoint column sets) and takes the (k+1)-th smallest
template <int SLOTS>
__global__ __launch_bounds__(256) void knn_merge_kernel(const double* __restrict__ part, int N, int parts, int k, double* __restrict__ radii2) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  double list[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) list[s] = INFINITY;
  for (int y = 0; y < parts; ++y) {
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) list_insert(list, part[((size_t)y * N + row) * SLOTS + s]);
  }
  double v = list[0];
#pragma unroll
  for (int s = 1; s < SLOTS; ++s) v = (s == k) ? list[s] : v;
  radii2[row] = v;
}

// grid (ceil(Nq / 128), parts), 256 threads; part uint8 [parts][Nq]
template <class TQ, class TB>
__global__ __launch_bounds__(256)
void cover_flags_kernel(const TQ* __restrict__ q, int Nq, int64_t q_stride, const TB* __restrict__ b, int Nb, int64_t b_stride, bool vec, int D,
                        const double* __restrict__ q_norms, const double* __restrict__ b_norms, const double* __restrict__ radii2,
                        uint8_t* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i0 = (blockIdx.x * 4 + wave) * 16 * MF_MR;
  if (i0 >= Nq) return;
  const int lc = lane & 15, lr = lane >> 4;
  double na[MF_MR][4];
  int hit[MF_MR][4];
#pragma unroll
  for (int m = 0; m < MF_MR; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      na[m][r] = q_norms[min(i0 + 16 * m + lr + 4 * r, Nq - 1)];
      hit[m][r] = 0;
    }
  }
  int first, last;
  tile_range(Nb, blockIdx.y, gridDim.y, first, last);
  for (int j0 = first * MF_TILE; j0 < last * MF_TILE; j0 += MF_TILE) {
    f64x4 acc[MF_MR][4];
    dot_tile(q, q_stride, Nq, b, b_stride, Nb, vec, D, i0, j0, lane, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int col = j0 + 16 * t + lc;
      if (col < Nb) {
        const double nb = b_norms[col], r2 = radii2[col];
#pragma unroll
        for (int m = 0; m < MF_MR; ++m) {
#pragma unroll
          for (int r = 0; r < 4; ++r) hit[m][r] |= dist2(na[m][r], nb, acc[m][t][r]) <= r2 ? 1 : 0;
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MF_MR; ++m) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) hit[m][r] |= __shfl_xor(hit[m][r], o);
      const int row = i0 + 16 * m + lr + 4 * r;
      if (lc == 0 && row < Nq) part[(size_t)blockIdx.y * Nq + row] = (uint8_t)hit[m][r];
    }
  }
}

// grid (ceil(Nq / 256)): the OR over the parts
__global__ __launch_bounds__(256) void cover_merge_kernel(const uint8_t* __restrict__ part, int Nq, int parts, uint8_t* __restrict__ inside) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= Nq) return;
  uint8_t hit = 0;
  for (int y = 0; y < parts; ++y) hit |= part[(size_t)y * Nq + row];
  inside[row] = hit;
}

bool set_ok(int N, int D, int64_t row_stride) { return N >= 1 && N <= MF_MAX_N && D >= 1 && D <= MF_MAX_D && row_stride >= D; }

// 16-byte loads need the base and every row start on a 16-byte boundary
bool vec_ok(const void* p, int dtype, int64_t row_stride) { return (uintptr_t)p % 16 == 0 && (row_stride * (dtype ? 8 : 4)) % 16 == 0; }

// Parts of the column walk: enough workgroups (about 16 per compute unit) that the last round of them is a small share of the run, never more
// than there are column tiles.  The values a row sees do not depend on it.
int parts_for(int rows, int cols) {
  const int blocks = (rows + MF_BLOCK - 1) / MF_BLOCK, tiles = (cols + MF_TILE - 1) / MF_TILE;
  return std::max(1, std::min({MF_MAX_SPLITS, tiles, (4096 + blocks - 1) / blocks}));
}

template <class T>
void launch_norms(const void* x, int N, int D, int64_t row_stride, double* norms, hipStream_t s) {
  hipLaunchKernelGGL(row_norms_kernel<T>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (const T*)x, N, D, row_stride, norms);
}

template <class T, int SLOTS>
void launch_knn(const void* x, int N, int D, int64_t row_stride, bool vec, int k, double* norms, double* part, double* radii2, hipStream_t s) {
  const int parts = parts_for(N, N);
  launch_norms<T>(x, N, D, row_stride, norms, s);
  hipLaunchKernelGGL((knn_lists_kernel<T, SLOTS>), dim3((unsigned)((N + MF_BLOCK - 1) / MF_BLOCK), parts), dim3(256), 0, s, (const T*)x, N, D, row_stride, vec, norms, part);
  hipLaunchKernelGGL(knn_merge_kernel<SLOTS>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, part, N, parts, k, radii2);
}

template <class TQ, class TB>
void launch_cover(const void* q, int Nq, int64_t q_stride, const void* b, int Nb, int64_t b_stride, bool vec, int D,
                  const double* q_norms, const double* b_norms, const double* radii2, uint8_t* part, uint8_t* inside, hipStream_t s) {
  const int parts = parts_for(Nq, Nb);
  hipLaunchKernelGGL((cover_flags_kernel<TQ, TB>), dim3((unsigned)((Nq + MF_BLOCK - 1) / MF_BLOCK), parts), dim3(256), 0, s, (const TQ*)q, Nq, q_stride,
                     (const TB*)b, Nb, b_stride, vec, D, q_norms, b_norms, radii2, part);
  hipLaunchKernelGGL(cover_merge_kernel, dim3((unsigned)((Nq + 255) / 256)), dim3(256), 0, s, part, Nq, parts, inside);
}

}  // namespace

}  // namespace mb

using namespace mb;

extern "C" {

// per row its norm and, for every part of the column walk, a list of MF_SLOTS doubles (mb_knn_radii) or a flag (mb_manifold_cover)
size_t mb_manifold_workspace_bytes(int N, int D) {
  if (N < 1 || N > MF_MAX_N || D < 1 || D > MF_MAX_D) return 0;
  return (size_t)N * (1 + MF_MAX_SPLITS * MF_SLOTS) * sizeof(double);
}

int mb_knn_radii(const void* x, int dtype, int N, int D, int64_t row_stride, int k, double* radii2, void* workspace, mb_stream stream) {
  if (!x || !radii2 || !workspace) return fail(-1, "mb_knn_radii: null argument");
  if (dtype != 0 && dtype != 1) return fail(-1, "mb_knn_radii: dtype is 0 (fp32) or 1 (fp64), got %d", dtype);
  if (!set_ok(N, D, row_stride))
    return fail(-1, "mb_knn_radii: N in [1, %d], D in [1, %d] and row_stride >= D required (got N %d, D %d, row_stride %lld)", MF_MAX_N, MF_MAX_D, N,
                D, (long long)row_stride);
  if (k < 1 || k > MF_MAX_K || k + 1 > N) return fail(-1, "mb_knn_radii: 1 <= k <= %d and k + 1 <= N required (got k %d, N %d)", MF_MAX_K, k, N);
  if ((uintptr_t)x % (dtype ? 8 : 4) || (uintptr_t)radii2 % 8 || (uintptr_t)workspace % 8) return fail(-1, "mb_knn_radii: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("knn_radii", s);
  double* norms = (double*)workspace;
  double* part = norms + N;
  const bool vec = vec_ok(x, dtype, row_stride);
  if (k <= 3) {                                            // lists of 4 (ADM's k = 3) leave the registers for a second wave per SIMD
    if (dtype) launch_knn<double, 4>(x, N, D, row_stride, vec, k, norms, part, radii2, s);
    else launch_knn<float, 4>(x, N, D, row_stride, vec, k, norms, part, radii2, s);
  } else {
    if (dtype) launch_knn<double, MF_SLOTS>(x, N, D, row_stride, vec, k, norms, part, radii2, s);
    else launch_knn<float, MF_SLOTS>(x, N, D, row_stride, vec, k, norms, part, radii2, s);
  }
  return launched();
}

int mb_manifold_cover(const void* q, int q_dtype, int Nq, int64_t q_stride, const void* b, int b_dtype, int Nb, int64_t b_stride, int D,
                      const double* radii2, uint8_t* inside, void* workspace, mb_stream stream) {
  if (!q || !b || !radii2 || !inside || !workspace) return fail(-1, "mb_manifold_cover: null argument");
  if ((q_dtype != 0 && q_dtype != 1) || (b_dtype != 0 && b_dtype != 1))
    return fail(-1, "mb_manifold_cover: dtype is 0 (fp32) or 1 (fp64), got %d and %d", q_dtype, b_dtype);
  if (!set_ok(Nq, D, q_stride) || !set_ok(Nb, D, b_stride) || (int64_t)Nq + Nb > MF_MAX_N)
    return fail(-1, "mb_manifold_cover: Nq, Nb >= 1 with Nq + Nb <= %d, D in [1, %d] and strides >= D required (got Nq %d, Nb %d, D %d, strides %lld, %lld)",
                MF_MAX_N, MF_MAX_D, Nq, Nb, D, (long long)q_stride, (long long)b_stride);
  if ((uintptr_t)q % (q_dtype ? 8 : 4) || (uintptr_t)b % (b_dtype ? 8 : 4) || (uintptr_t)radii2 % 8 || (uintptr_t)workspace % 8)
    return fail(-1, "mb_manifold_cover: misaligned pointer");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("manifold_cover", s);
  double* q_norms = (double*)workspace;
  double* b_norms = q_norms + Nq;
  uint8_t* part = (uint8_t*)(b_norms + Nb);
  const bool vec = vec_ok(q, q_dtype, q_stride) && vec_ok(b, b_dtype, b_stride);
  if (q_dtype) launch_norms<double>(q, Nq, D, q_stride, q_norms, s);
  else launch_norms<float>(q, Nq, D, q_stride, q_norms, s);
  if (b_dtype) launch_norms<double>(b, Nb, D, b_stride, b_norms, s);
  else launch_norms<float>(b, Nb, D, b_stride, b_norms, s);
  if (q_dtype && b_dtype) launch_cover<double, double>(q, Nq, q_stride, b, Nb, b_stride, vec, D, q_norms, b_norms, radii2, part, inside, s);
  else if (q_dtype) launch_cover<double, float>(q, Nq, q_stride, b, Nb, b_stride, vec, D, q_norms, b_norms, radii2, part, inside, s);
  else if (b_dtype) launch_cover<float, double>(q, Nq, q_stride, b, Nb, b_stride, vec, D, q_norms, b_norms, radii2, part, inside, s);
  else launch_cover<float, float>(q, Nq, q_stride, b, Nb, b_stride, vec, D, q_norms, b_norms, radii2, part, inside, s);
  return launched();
}

}  // extern "C"
