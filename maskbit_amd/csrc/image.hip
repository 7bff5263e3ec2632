// The data loader's image transform on gfx950, bit for bit what Pillow computes: the antialiased resize of ImagingResample (8 bits per channel;
// BOX / BILINEAR / BICUBIC), the centre crop, and ToTensor().  The reference's eval_transform (data/webdataset_reader.py:79-85) is
// Resize -> CenterCrop -> ToTensor on a PIL image; guided-diffusion's center_crop_arr (the ADM reference batches) is BOX halvings + one BICUBIC
// resize + a crop.  Both are one or more PASSES of the same three launches over a ragged batch of jobs (include/maskbit_hip.h "image transform"):
//
//   coeff_kernel   per (job, axis, output index in the window): xmin, n and the int32 taps k[] of that output, in IEEE double exactly as Pillow's
//                  precompute_coeffs + normalize_coeffs_8bpc -- scale = in / out, fs = max(scale, 1), support = s fs, center = (xx + 0.5) scale,
//                  xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), in) - xmin,
//                  w[x] = f((x + xmin - center + 0.5) (1 / fs)) / sum (ascending x), k = (int)(w 2^22 +- 0.5).  An axis whose size does not change
//                  is skipped by Pillow; here it gets the identity table (one tap of 2^22: (2^21 + p 2^22) >> 22 = p), so that every job runs
//                  the same two passes.
//   hpass_kernel   HORIZONTAL first, as Pillow: packed uint8 RGB source rows -> the uint8 intermediate (rounded and clipped) in the job's workspace
//                  slot, only for the window's columns and the source rows the window's vertical taps read.  A block takes 4 rows x 256 outputs
//                  and stages the row segments its taps read through LDS with whole-dword loads (rows are not 4-byte aligned in general: the
//                  segment starts at the dword below and keeps its shift); a segment beyond the LDS tile (scale above ~5) reads global bytes.
//   vpass_kernel   vertical over the intermediate, fused with the crop and both output formats: uint8 HWC at out_u8 and / or float32 planes at
//                  out_f32 (v / 255 by a 256-entry table of correctly rounded quotients -- a reciprocal multiply differs for 126 byte values).
//                  A thread owns 4 consecutive outputs of a row: 3 dwords per tap row in, 3 dwords / three float4 out.
//
// Each output depends on its own taps alone, so computing only the window changes no bit.  sum |k| < 1.3 2^22, so the sums fit int32.  No atomics,
// no allocation, no synchronisation; grids come from the host-known maxima of the jobs, blocks beyond a job's sizes leave at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/maskbit_hip.h"
#include "mb_abi.h"
#include "mb_image.h"

// The coefficient arithmetic must round after every operation: Pillow's build does not fuse a multiply into an add, and one wrong bit in a
// coefficient is a wrong output byte -- this is not a tolerance question.  hipcc contracts by default (-ffp-contract=fast-honor-pragmas), so it
// is turned off here for the whole file (host arithmetic on sizes included; nothing else in it is floating point except one division).
#pragma clang fp contract(off)

namespace mb {

namespace {

constexpr int PREC_BITS = 22;
constexpr int HP_ROWS = 4;               // source rows per block of the horizontal pass
constexpr int HP_TX = 256;               // outputs along x per block: 64 lanes x 4
constexpr int HP_SEG = 4096;             // LDS bytes per staged row segment

__host__ __device__ inline double filter_support(int f) { return f == IMG_BOX ? 0.5 : f == IMG_BILINEAR ? 1.0 : 2.0; }

// Pillow's box_filter / bilinear_filter / bicubic_filter (a = -0.5), operation for operation
__device__ inline double filter_value(int f, double x) {
  if (f == IMG_BOX) return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
  if (x < 0.0) x = -x;
  if (f == IMG_BILINEAR) return x < 1.0 ? 1.0 - x : 0.0;
  const double a = -0.5;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// one output of one axis; K = the table's taps per output (identity: the axis is skipped)
__device__ inline void coeff_entry(int in, int out, int f, int xx, int K, bool identity, int32_t* e_xmin, int32_t* e_n, int32_t* taps) {
  if (identity) {
    *e_xmin = xx; *e_n = 1; taps[0] = 1 << PREC_BITS;
    for (int x = 1; x < K; ++x) taps[x] = 0;
    return;
  }
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(f) * fs;
  const double ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  if (xmax > K) xmax = K;                                  // never: ksize bounds it, as Pillow's own allocation relies on
  if (xmax < 0) xmax = 0;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += filter_value(f, (x + xmin - center + 0.5) * ss);
  for (int x = 0; x < xmax; ++x) {
    double w = filter_value(f, (x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    taps[x] = w < 0 ? (int)(-0.5 + w * (1 << PREC_BITS)) : (int)(0.5 + w * (1 << PREC_BITS));
  }
  for (int x = xmax; x < K; ++x) taps[x] = 0;
  *e_xmin = xmin; *e_n = xmax;
}

// a job's slot: int32 x table [win_w][2 + kx], y table [win_h][2 + ky], then (16-byte aligned) the intermediate [src_h][pitch] bytes
__host__ __device__ inline int64_t tmp_pitch(int win_w) { return 12 * (int64_t)((win_w + 3) / 4); }
__host__ __device__ inline int64_t coef_bytes(const mb_image_job& j) {
  const int64_t ints = (int64_t)j.win_w * (2 + j.kx) + (int64_t)j.win_h * (2 + j.ky);
  return (ints * 4 + 15) / 16 * 16;
}
__host__ __device__ inline int64_t slot_bytes(const mb_image_job& j) { return coef_bytes(j) + (tmp_pitch(j.win_w) * j.src_h + 15) / 16 * 16; }

__device__ inline uint8_t clip8(int v) { return (uint8_t)min(max(v >> PREC_BITS, 0), 255); }

// grid (ceil(max(win_w + win_h) / 256), B)
__global__ __launch_bounds__(256) void coeff_kernel(const mb_image_job* __restrict__ jobs, int filter, uint8_t* __restrict__ work) {
  const mb_image_job j = jobs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= j.win_w + j.win_h) return;
  int32_t* cx = (int32_t*)(work + j.work_offset);
  if (i < j.win_w) {
    int32_t* e = cx + (int64_t)i * (2 + j.kx);
    coeff_entry(j.src_w, j.res_w, filter, j.win_x + i, j.kx, j.res_w == j.src_w, e, e + 1, e + 2);
  } else {
    const int y = i - j.win_w;
    int32_t* e = cx + (int64_t)j.win_w * (2 + j.kx) + (int64_t)y * (2 + j.ky);
    coeff_entry(j.src_h, j.res_h, filter, j.win_y + y, j.ky, j.res_h == j.src_h, e, e + 1, e + 2);
  }
}

// grid (ceil(count / 256)): the diagnostic form on caller-owned arrays
__global__ __launch_bounds__(256) void coeff_table_kernel(int in, int out, int filter, int first, int count, int K, int32_t* __restrict__ xmin,
                                                          int32_t* __restrict__ n, int32_t* __restrict__ taps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  coeff_entry(in, out, filter, first + i, K, in == out, xmin + i, n + i, taps + (int64_t)i * K);
}

// grid (ceil(max win_w / 256), ceil(max src_h / 4), B), 256 threads = 64 x-quads x 4 rows
__global__ __launch_bounds__(256) void hpass_kernel(const mb_image_job* __restrict__ jobs, const uint8_t* __restrict__ src, const uint8_t* src_end,
                                                    uint8_t* __restrict__ work) {
  __shared__ uint32_t seg[HP_ROWS][HP_SEG / 4];
  const mb_image_job j = jobs[blockIdx.z];
  const int x0 = blockIdx.x * HP_TX;
  if (x0 >= j.win_w) return;                               // block-uniform, as every return before the barrier
  const int32_t* cx = (const int32_t*)(work + j.work_offset);
  const int32_t* cy = cx + (int64_t)j.win_w * (2 + j.kx);
  const int32_t* cy_last = cy + (int64_t)(j.win_h - 1) * (2 + j.ky);
  // the source rows the window's vertical taps read: xmin and xmin + n both grow with the output index
  const int row_end = min(cy_last[0] + cy_last[1], j.src_h);
  const int row0 = cy[0] + blockIdx.y * HP_ROWS;
  if (row0 >= row_end) return;
  const int nrows = min(HP_ROWS, row_end - row0);
  const int x_last = min(x0 + HP_TX, j.win_w) - 1;
  const int32_t* e_first = cx + (int64_t)x0 * (2 + j.kx);
  const int32_t* e_last = cx + (int64_t)x_last * (2 + j.kx);
  const int seg_lo = e_first[0], seg_hi = min(e_last[0] + e_last[1], j.src_w);          // source columns [seg_lo, seg_hi)
  const int seg_len = 3 * (seg_hi - seg_lo);
  const uint8_t* base = src + j.src_offset + 3 * (int64_t)seg_lo;
  const bool staged = seg_len + 3 <= HP_SEG;
  if (staged) {
    for (int r = 0; r < nrows; ++r) {
      const uint8_t* g = base + (int64_t)(row0 + r) * j.src_stride;
      const int sh = (int)((uintptr_t)g & 3);
      const uint8_t* a0 = g - sh;
      const int ndw = (sh + seg_len + 3) >> 2;
      for (int i = threadIdx.x; i < ndw; i += 256) {
        const uint8_t* a = a0 + 4 * i;
        uint32_t v;
        if (a >= src && a + 4 <= src_end) {
          v = *(const uint32_t*)a;
        } else {                                           // the dword straddles an end of the source buffer: its bytes inside
          v = 0;
          for (int b = 0; b < 4; ++b)
            if (a + b >= src && a + b < src_end) v |= (uint32_t)a[b] << (8 * b);
        }
        seg[r][i] = v;
      }
    }
    __syncthreads();
  }
  const int tx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  if (ry >= nrows) return;
  const int row = row0 + ry;
  const int xq = x0 + 4 * tx;
  if (xq >= j.win_w) return;
  const uint8_t* g = base + (int64_t)row * j.src_stride;
  const uint8_t* p0 = staged ? (const uint8_t*)seg[ry] + ((uintptr_t)g & 3) : g;        // byte 0 = channel 0 of source column seg_lo
  uint32_t packed[3] = {0, 0, 0};
  const int nv = min(4, j.win_w - xq);
  for (int q = 0; q < nv; ++q) {
    const int32_t* e = cx + (int64_t)(xq + q) * (2 + j.kx);
    const int xmin = e[0], n = e[1];
    const uint8_t* p = p0 + 3 * (xmin - seg_lo);
    int a0 = 1 << (PREC_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
      const int k = e[2 + t];
      a0 += p[3 * t] * k; a1 += p[3 * t + 1] * k; a2 += p[3 * t + 2] * k;
    }
    const uint32_t px[3] = {clip8(a0), clip8(a1), clip8(a2)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int b = 3 * q + c;
      packed[b >> 2] |= px[c] << (8 * (b & 3));
    }
  }
  uint8_t* tmp = work + j.work_offset + coef_bytes(j) + tmp_pitch(j.win_w) * row + 3 * (int64_t)(xq);   // 4-byte aligned: pitch and 3 xq are multiples of 4
  uint32_t* t32 = (uint32_t*)tmp;
  t32[0] = packed[0]; t32[1] = packed[1]; t32[2] = packed[2];                            // a short last quad writes zeros into the row's padding
}

// grid (ceil(max win_w / 256), ceil(max win_h / 4), B), 256 threads = 64 x-quads x 4 rows
__global__ __launch_bounds__(256) void vpass_kernel(const mb_image_job* __restrict__ jobs, const uint8_t* __restrict__ work, uint8_t* __restrict__ out_u8,
                                                    float* __restrict__ out_f32) {
  __shared__ float to_float[256];
  // ToTensor(): uint8 -> float32, then .div(255): the correctly rounded float quotient.  The double quotient rounded to float is the same float
  // for all 256 values (the double's error is far below the distance of any v / 255 to a float rounding boundary; tests/test_image_transform_cpu.py).
  to_float[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
  __syncthreads();
  const mb_image_job j = jobs[blockIdx.z];
  const int tx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int x = blockIdx.x * 256 + 4 * tx, y = blockIdx.y * 4 + ry;
  if (x >= j.win_w || y >= j.win_h) return;
  const int32_t* cx = (const int32_t*)(work + j.work_offset);
  const int32_t* e = cx + (int64_t)j.win_w * (2 + j.kx) + (int64_t)y * (2 + j.ky);
  const int ymin = e[0], n = e[1];
  const int64_t pitch = tmp_pitch(j.win_w);
  const uint8_t* tmp = work + j.work_offset + coef_bytes(j) + pitch * ymin + 3 * (int64_t)x;
  int acc[12];
#pragma unroll
  for (int b = 0; b < 12; ++b) acc[b] = 1 << (PREC_BITS - 1);
  for (int t = 0; t < n; ++t) {
    const int k = e[2 + t];
    const uint32_t* r = (const uint32_t*)(tmp + pitch * t);
    const uint32_t d[3] = {r[0], r[1], r[2]};
#pragma unroll
    for (int b = 0; b < 12; ++b) acc[b] += (int)((d[b >> 2] >> (8 * (b & 3))) & 255u) * k;
  }
  uint8_t v[12];
#pragma unroll
  for (int b = 0; b < 12; ++b) v[b] = clip8(acc[b]);
  const int nv = min(4, j.win_w - x);
  const int64_t pix = j.dst_offset + (int64_t)y * j.win_w + x;
  if (out_u8) {
    uint8_t* d = out_u8 + 3 * pix;
    if (nv == 4 && ((uintptr_t)d & 3) == 0) {
      uint32_t* d32 = (uint32_t*)d;
#pragma unroll
      for (int w = 0; w < 3; ++w) d32[w] = v[4 * w] | (v[4 * w + 1] << 8) | (v[4 * w + 2] << 16) | ((uint32_t)v[4 * w + 3] << 24);
    } else {
      for (int b = 0; b < 3 * nv; ++b) d[b] = v[b];
    }
  }
  if (out_f32) {
    const int64_t plane = (int64_t)j.win_h * j.win_w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* d = out_f32 + 3 * j.dst_offset + c * plane + (int64_t)y * j.win_w + x;
      if (nv == 4 && ((uintptr_t)d & 15) == 0) {
        *(float4*)d = make_float4(to_float[v[c]], to_float[v[3 + c]], to_float[v[6 + c]], to_float[v[9 + c]]);
      } else {
        for (int q = 0; q < nv; ++q) d[q] = to_float[v[3 * q + c]];
      }
    }
  }
}

bool filter_ok(int f) { return f == IMG_BOX || f == IMG_BILINEAR || f == IMG_BICUBIC; }

// what is wrong with a job's geometry, or null
const char* job_fault(const mb_image_job& j) {
  if (j.src_h < 1 || j.src_h > IMG_MAX_SIDE || j.src_w < 1 || j.src_w > IMG_MAX_SIDE) return "a source side outside [1, 16384]";
  if (j.res_h < 1 || j.res_h > IMG_MAX_SIDE || j.res_w < 1 || j.res_w > IMG_MAX_SIDE) return "a resized side outside [1, 16384]";
  if (j.win_h < 1 || j.win_w < 1) return "a window (the resolution R) below 1";
  if (j.win_y < 0 || j.win_x < 0 || (int64_t)j.win_y + j.win_h > j.res_h || (int64_t)j.win_x + j.win_w > j.res_w) return "a window outside the resized image";
  if (j.src_stride < 3 * j.src_w || j.src_stride > (1 << 20)) return "a row stride below 3 * src_w (or above 2^20)";
  if (j.src_offset < 0 || j.dst_offset < 0) return "a negative offset";
  return nullptr;
}

}  // namespace

int image_ksize(int in_size, int out_size, int filter) {
  if (in_size == out_size) return 1;
  const double scale = (double)in_size / (double)out_size;
  const double fs = scale < 1.0 ? 1.0 : scale;
  return (int)std::ceil(filter_support(filter) * fs) * 2 + 1;
}

void image_coeffs_launch(int in_size, int out_size, int filter, int first, int count, int ksize, int32_t* xmin, int32_t* n, int32_t* taps, hipStream_t s) {
  hipLaunchKernelGGL(coeff_table_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, in_size, out_size, filter, first, count, ksize, xmin, n, taps);
}

}  // namespace mb

using namespace mb;

extern "C" {

size_t mb_image_workspace_bytes(mb_image_job* jobs, int B, int filter) {
  if (!jobs || B < 1 || B > IMG_MAX_JOBS || !filter_ok(filter)) return 0;
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    mb_image_job& j = jobs[b];
    if (job_fault(j)) return 0;
    j.kx = image_ksize(j.src_w, j.res_w, filter);
    j.ky = image_ksize(j.src_h, j.res_h, filter);
    j.work_offset = total;
    total += slot_bytes(j);
  }
  return (size_t)total;
}

int mb_image_resample(const mb_image_job* jobs_host, const mb_image_job* jobs_dev, int B, int filter, const uint8_t* src, size_t src_bytes,
                      uint8_t* out_u8, float* out_f32, int64_t out_pixels, void* workspace, size_t workspace_bytes, mb_stream stream) {
  if (!jobs_host || !jobs_dev || !src || !workspace) return fail(-1, "mb_image_resample: null argument (jobs, source or workspace)");
  if (!out_u8 && !out_f32) return fail(-1, "mb_image_resample: neither output is given");
  if (!filter_ok(filter)) return fail(-1, "mb_image_resample: filter is 0 (box), 1 (bilinear) or 2 (bicubic), got %d", filter);
  if (B < 1 || B > IMG_MAX_JOBS) return fail(-1, "mb_image_resample: 1 <= B <= %d required, got %d", IMG_MAX_JOBS, B);
  if ((uintptr_t)jobs_dev % 8 || (uintptr_t)workspace % 16 || (uintptr_t)out_f32 % 4) return fail(-1, "mb_image_resample: misaligned pointer");
  int64_t total = 0;
  int max_w = 0, max_h = 0, max_src_h = 0, max_wh = 0;
  for (int b = 0; b < B; ++b) {
    const mb_image_job& j = jobs_host[b];
    if (const char* what = job_fault(j)) return fail(-1, "mb_image_resample: job %d has %s", b, what);
    if ((uint64_t)j.src_offset + (uint64_t)(j.src_h - 1) * j.src_stride + 3ull * j.src_w > src_bytes)
      return fail(-1, "mb_image_resample: job %d reads beyond the %zu source bytes", b, src_bytes);
    if (j.dst_offset + (int64_t)j.win_h * j.win_w > out_pixels) return fail(-1, "mb_image_resample: job %d writes beyond the %lld output pixels", b, (long long)out_pixels);
    if (j.kx != image_ksize(j.src_w, j.res_w, filter) || j.ky != image_ksize(j.src_h, j.res_h, filter) || j.work_offset != total)
      return fail(-1, "mb_image_resample: job %d does not carry the layout of mb_image_workspace_bytes for this filter", b);
    total += slot_bytes(j);
    max_w = std::max(max_w, j.win_w); max_h = std::max(max_h, j.win_h);
    max_src_h = std::max(max_src_h, j.src_h); max_wh = std::max(max_wh, j.win_w + j.win_h);
  }
  if ((uint64_t)total > workspace_bytes) return fail(-1, "mb_image_resample: the workspace holds %zu bytes, %lld are needed", workspace_bytes, (long long)total);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("image_resample", s);
  uint8_t* work = (uint8_t*)workspace;
  {
    ProfScope q("image_coeffs", s);
    hipLaunchKernelGGL(coeff_kernel, dim3((unsigned)((max_wh + 255) / 256), (unsigned)B), dim3(256), 0, s, jobs_dev, filter, work);
  }
  {
    ProfScope q("image_hpass", s);
    hipLaunchKernelGGL(hpass_kernel, dim3((unsigned)((max_w + HP_TX - 1) / HP_TX), (unsigned)((max_src_h + HP_ROWS - 1) / HP_ROWS), (unsigned)B), dim3(256), 0, s,
                       jobs_dev, src, src + src_bytes, work);
  }
  {
    ProfScope q("image_vpass", s);
    hipLaunchKernelGGL(vpass_kernel, dim3((unsigned)((max_w + 255) / 256), (unsigned)((max_h + 3) / 4), (unsigned)B), dim3(256), 0, s, jobs_dev, work, out_u8, out_f32);
  }
  return launched();
}

}  // extern "C"
