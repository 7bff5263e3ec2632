// The convolution, GroupNorm, pool and repack kernels of the conv-VQGAN tokenizer (ConvDecoder.forward, modeling/modules/autoencoder.py:399-423;
// ConvEncoder, :230-286) and their launchers (mb_conv.h): NHWC h16 implicit-GEMM convolutions on MFMA.  No handle and no allocation here: the
// tokenizer handle is decoder.hip, the VGG16 stack of LPIPS (lpips.hip) and the single-layer diagnostics (diag.hip) run the same launchers.
//
// Layout: every activation is [B, H, W, C] h16 (channels contiguous = the MFMA k order), weights
// are repacked once to [tap][Cout_pad][Cin_pad] h16.  One workgroup computes an 8x16-pixel output
// tile for 128 (or 16) output channels; for each 64-channel input chunk the (8+2)x(16+2) halo tile
// is staged ONCE into LDS and re-used by all 9 taps (a tap is just a shifted LDS row index), while
// the per-tap weight tiles stream in by LDS-DMA, double-buffered, exactly like the GEMM's W tile.
// Fusions:  GroupNorm-apply + SiLU happen on the way into LDS (per-(image,channel) scale/shift
// from the stats pass), nearest-2x upsampling is an index shift (>>1) of the source pixel, bias /
// residual add live in the epilogue, and the last conv writes fp32 NCHW and/or clamp*255 uint8 NHWC.
// GroupNorm statistics (32 groups, eps 1e-6, autoencoder.py:39-43) are a deterministic two-level
// reduction (no float atomics), so outputs are bit-stable run to run.  Level one lives in the epilogue of the conv that PRODUCES the tensor
// (one (sum, sumsq) pair per 8x16-pixel tile and group, written next to the tile), level two in gn_finalize_kernel before the consuming conv;
// only tensors that no conv of this file produced (the encoder's average-pooled ones) still take the separate sweep (gn_partial_kernel).
#include <algorithm>
#include <cassert>
#include <type_traits>

#include "mb_conv.h"

namespace mb {

struct ConvArgs {
  const h16* in;        // [B, Hin, Win, Cin] (Hin = H/2 when UP)
  const float2* gn;      // [B, Cin] (scale, shift) or null
  const h16* w;         // [taps][Cout_pad][Cin]
  const float* bias;     // [Cout_pad] or null
  const h16* residual;  // [B, H, W, Cout] or null
  h16* out;             // [B, H, W, Cout]
  float* img_nchw;       // final conv only
  uint8_t* img_u8;       // final conv only
  int B, H, W, Cin, Cout, Cout_pad;
  unsigned* sat;         // counts output groups of 4 whose value left the fp16 range and was clamped (mb_dec_saturation_count)
  float* gn_part;        // or null: GroupNorm partial statistics of the OUTPUT, [B][pixel tiles per image][32 groups][sum, sumsq] -- the consumer's
                         // GroupNorm then needs no sweep over the tensor (its fp16-stored values are what is summed, as that sweep did)
};

__device__ __forceinline__ float silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

// TH = 16 (round 3): the 8 x 16 tile ran two 4-wave workgroups per CU (LDS-bound) = two waves per SIMD, each tap step (32 MFMAs per wave) behind
// a barrier and the LDS-DMA of its weight tile: per step 3 500 clocks for 512 clocks of matrix work.  A 16 x 16 tile on 8 waves keeps two
// workgroups per CU (74 KiB each) but FOUR waves per SIMD at the same 125 VGPRs, stages each weight tile for twice the pixels and shrinks the
// halo overhead from 1.41 to 1.27 pixels read per pixel written.
// RELU (the VGG16 stack of lpips.hip): max(v, 0) after bias, before the fp16 store.  Off by default: every instantiation without it compiles to the code it had.
// SILU = false (the q / k / v projection of the Taming AttnBlock, whose `norm` has no nonlinearity behind it): the prologue applies (scale, shift) only.
template <int NI, int WN, int KS, bool UP, bool FINAL, int TH = 8, bool RELU = false, bool SILU = true>
__global__ __launch_bounds__(32 * TH, TH / 4) void conv_kernel(ConvArgs a) {
  constexpr int NTHR = 32 * TH, NWAVE = NTHR / 64;
  constexpr int WM = NWAVE / WN, MJ = TH / WM, BN = WN * NI * 16;
  // KS = 3: symmetric pad 1.  KS = 2 (the stride-2 Conv2dSame of the encoder, run on a space-to-depth input): no pad before,
  // one zero row/column after (autoencoder.py:18,31-36: TF "SAME" puts the odd pixel at the bottom/right).
  constexpr int PAD = (KS - 1) / 2, HW_ = TW + KS - 1, HALO = (TH + KS - 1) * HW_, NTAP = KS * KS;
  constexpr int WT_BYTES = BN * 128;
  constexpr int HALO_BYTES = (HALO + 7) / 8 * 1024;   // whole 8-pixel DMA groups
  __shared__ __attribute__((aligned(16))) char smem[HALO_BYTES + 2 * WT_BYTES];
  char* halo = smem;
  char* wt = smem + HALO_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l15 = lane & 15, g = lane >> 4;

  const int ntn = a.Cout_pad / BN, ntx = a.W / TW, nty = a.H / TH;
  int bid = blockIdx.x;
  const int tn = bid % ntn; bid /= ntn;
  const int tx = bid % ntx; bid /= ntx;
  const int ty = bid % nty; const int b = bid / nty;
  const int n0 = tn * BN, y0 = ty * TH, x0 = tx * TW;
  const int Cin = a.Cin;
  const int Hin = UP ? a.H / 2 : a.H, Win = UP ? a.W / 2 : a.W;

  // ---- weight-tile DMA: BN rows of 128 B; a wave instruction covers 8 rows
  constexpr int WROWS_PER_WAVE = BN / NWAVE;        // 32 / 16 (BN = 128 on 4 / 8 waves) or 4 (BN = 16)
  constexpr int WINST = (WROWS_PER_WAVE + 7) / 8;   // 4 / 2 or 1
  const h16* wsrc[WINST];
#pragma unroll
  for (int j = 0; j < WINST; ++j) {
    int row = wave * WROWS_PER_WAVE + j * 8 + (lane >> 3);
    if (WROWS_PER_WAVE < 8) row = min(row, BN - 1);
    wsrc[j] = a.w + (size_t)(n0 + row) * Cin + ((lane & 7) ^ ((row >> 1) & 7)) * 8;
  }
  auto stage_w = [&](int t, int buf) {
    const int chunk = t / NTAP, tap = t - chunk * NTAP;
    const size_t off = (size_t)tap * a.Cout_pad * Cin + chunk * CK;
    if (WROWS_PER_WAVE >= 8) {
#pragma unroll
      for (int j = 0; j < WINST; ++j)
        MB_GLDS16(wsrc[j] + off, wt + buf * WT_BYTES + (wave * WROWS_PER_WAVE + j * 8) * 128);
    } else if (wave < 2) {                           // BN = 16: two 8-row instructions in total
      const int row = wave * 8 + (lane >> 3);
      const h16* src = a.w + (size_t)(n0 + row) * Cin + ((lane & 7) ^ ((row >> 1) & 7)) * 8;
      MB_GLDS16(src + off, wt + buf * WT_BYTES + wave * 8 * 128);
    }
  };

  // ---- halo staging (GN-apply + SiLU + zero padding).  The raw rows come in by LDS-DMA, 8 pixels x 128 B per wave instruction, from clamped
  // coordinates; every lane then normalises the 16 bytes IT brought in, in place (no barrier in between: a lane re-reads only its own slot after
  // its own vmcnt wait).  All of a wave's 5-6 instructions are in flight together and hold no registers.  (Round 3, before: a
  // load -> SiLU -> ds_write loop through registers, which the compiler left rolled -- six trips to memory per thread one after the other,
  // ~1.5 us each under load, twice per tile of a 128-channel conv whose workgroup lived 47 us; unrolled with the loads batched it spilled.)
  // Wave w takes pixel groups j = w, w + NWAVE, ..: j keeps its parity, so the 16-byte slot swizzle ((pixel >> 1) & 7 = (4j + lane/16) & 7)
  // maps a lane to ONE logical channel slot for all its groups and the GroupNorm scale / shift of its 8 channels stay in registers.
  constexpr int NGRP = (HALO + 7) / 8, NGW = (NGRP + NWAVE - 1) / NWAVE;
  const int myslot = (lane & 7) ^ (lane >> 4) ^ ((wave & 1) << 2);
  auto stage_halo = [&](int chunk) {
    const int c0 = chunk * CK + myslot * 8;
#pragma unroll
    for (int jj = 0; jj < NGW; ++jj) {
      const int j = wave + jj * NWAVE;
      if (j < NGRP) {
        const int hp = min(j * 8 + (lane >> 3), HALO - 1);
        const int hy = hp / HW_, hx = hp - hy * HW_;
        const int Y = min(max(y0 - PAD + hy, 0), a.H - 1), X = min(max(x0 - PAD + hx, 0), a.W - 1);
        const int sy = UP ? (Y >> 1) : Y, sx = UP ? (X >> 1) : X;
        MB_GLDS16(a.in + (((size_t)b * Hin + sy) * Win + sx) * Cin + c0, halo + j * 1024);
      }
    }
    float sc[8], sh[8];
    if (a.gn) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float2 v = a.gn[(size_t)b * Cin + c0 + e]; sc[e] = v.x; sh[e] = v.y; }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int jj = 0; jj < NGW; ++jj) {
      const int j = wave + jj * NWAVE;
      const int hp = j * 8 + (lane >> 3);
      if (j < NGRP && hp < HALO) {
        const int hy = hp / HW_, hx = hp - hy * HW_;
        const int Y = y0 - PAD + hy, X = x0 - PAD + hx;
        h16x8* slot = (h16x8*)(halo + j * 1024 + lane * 16);
        if (Y >= 0 && Y < a.H && X >= 0 && X < a.W) {
          if (a.gn) {
            h16x8 v = *slot;
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float f = fmaf((float)v[e], sc[e], sh[e]); v[e] = to_h(SILU ? silu(f) : f); }
            *slot = v;
          }
        } else {
          *slot = h16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
      }
    }
  };

  int wfoff[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) wfoff[kk] = l15 * 128 + (((kk * 4 + g) ^ (l15 >> 1)) * 16);

  f32x4 acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int T = (Cin / CK) * NTAP;
  stage_w(0, 0);
  for (int t = 0; t < T; ++t) {
    const int chunk = t / NTAP, tap = t - chunk * NTAP;
    if (tap == 0) {
      __syncthreads();                      // all waves are done with the previous chunk's halo
      stage_halo(chunk);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                        // weight tile t landed, halo visible
    if (t + 1 < T) stage_w(t + 1, (t + 1) & 1);
    const int dy = tap / KS, dx = tap - dy * KS;
    const char* wb = wt + (t & 1) * WT_BYTES + wn * NI * 16 * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      h16x8 wf[NI], xf[MJ];
#pragma unroll
      for (int i = 0; i < NI; ++i) wf[i] = *(const h16x8*)(wb + i * 16 * 128 + wfoff[kk]);
#pragma unroll
      for (int j = 0; j < MJ; ++j) {
        const int hp = (wm * MJ + j + dy) * HW_ + l15 + dx;
        xf[j] = *(const h16x8*)(halo + hp * 128 + (((kk * 4 + g) ^ ((hp >> 1) & 7)) * 16));
      }
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MJ; ++j)
          acc[i][j] = MB_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
    }
  }

  // ---- epilogue: lane holds out[pixel (y = wm*MJ+j, x = l15)][cout = ..+g*4 .. +3]
  // The bias of a lane's channels is fetched once; the residual values of pixel row j + 1 are requested before row j is stored, and the
  // saturation count is one atomic per lane at the end.  (Round 3, before: bias and residual loaded inside the (row, channel tile) loop behind
  // run-time branches -- the compiler waited vmcnt(0) after each of the 32 loads, i.e. also for the previous store: 14.5 us of a 50 us workgroup.)
  float gs[NI], gq[NI];                     // GroupNorm partials of this lane's 4 channels of n-tile i over its MJ pixels
  float4 bv[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    gs[i] = 0.f; gq[i] = 0.f;
    bv[i] = a.bias ? *(const float4*)(a.bias + n0 + wn * NI * 16 + i * 16 + g * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if constexpr (FINAL) {
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const int Y = y0 + wm * MJ + j, X = x0 + l15;
      const size_t pix = ((size_t)b * a.H + Y) * a.W + X;
      const float v[4] = {acc[0][j][0] + bv[0].x, acc[0][j][1] + bv[0].y, acc[0][j][2] + bv[0].z, acc[0][j][3] + bv[0].w};
      if (g == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (r < a.Cout) {
            if (a.img_nchw) a.img_nchw[(((size_t)b * a.Cout + r) * a.H + Y) * a.W + X] = v[r];
            if (a.img_u8) a.img_u8[pix * a.Cout + r] = (uint8_t)(fminf(fmaxf(v[r], 0.f), 1.f) * 255.0f);
          }
        }
      }
    }
  } else {
    const size_t pix0 = ((size_t)b * a.H + y0 + wm * MJ) * a.W + x0 + l15;        // pixel row j: + j * W
    const int nl = n0 + wn * NI * 16 + g * 4;                                       // channel of n-tile i: + i * 16
    unsigned nsat = 0;
    // straight-line per variant (residual or not; every channel of the tile stored or not): with the run-time tests inside the loop the
    // compiler's wait-count pass fell back to vmcnt(0) in front of every store
    auto body = [&](auto res_c, auto full_c) {
      constexpr bool RES = decltype(res_c)::value, FULL = decltype(full_c)::value;
      h16x4 rv[2][NI];
      auto fetch = [&](int j, h16x4 (&r)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          r[i] = h16x4{0, 0, 0, 0};
          if (RES && (FULL || nl + i * 16 < a.Cout)) r[i] = *(const h16x4*)(a.residual + (pix0 + (size_t)j * a.W) * a.Cout + nl + i * 16);
        }
      };
      fetch(0, rv[0]);
#pragma unroll
      for (int j = 0; j < MJ; ++j) {
        if (j + 1 < MJ) fetch(j + 1, rv[(j + 1) & 1]);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          if (FULL || nl + i * 16 < a.Cout) {
            float v[4] = {acc[i][j][0] + bv[i].x, acc[i][j][1] + bv[i].y, acc[i][j][2] + bv[i].z, acc[i][j][3] + bv[i].w};
            if (RES) {
              const h16x4 r = rv[j & 1][i];
              v[0] += (float)r[0]; v[1] += (float)r[1]; v[2] += (float)r[2]; v[3] += (float)r[3];
            }
            if constexpr (RELU) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
            // activations are stored as fp16: values beyond +-65504 are clamped by to_h -- counted, so that a checkpoint whose decoder needs a
            // wider residual stream is noticed instead of silently clipped (random-init weights stay far inside the range)
            nsat += fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) > MB_H16_MAX ? 1u : 0u;
            const h16x4 hv = {to_h(v[0]), to_h(v[1]), to_h(v[2]), to_h(v[3])};
            *(h16x4*)(a.out + (pix0 + (size_t)j * a.W) * a.Cout + nl + i * 16) = hv;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float f = (float)hv[r]; gs[i] += f; gq[i] = fmaf(f, f, gq[i]); }
          }
        }
      }
    };
    const bool full = n0 + BN <= a.Cout;
    if (a.residual) { if (full) body(std::true_type{}, std::true_type{}); else body(std::true_type{}, std::false_type{}); }
    else { if (full) body(std::false_type{}, std::true_type{}); else body(std::false_type{}, std::false_type{}); }
    if (nsat) atomicAdd(a.sat, nsat);
  }
  if constexpr (!FINAL) {
    if (a.gn_part) {                        // uniform; requires Cout % 128 == 0 and 4 | 8 | 16 channels per group (launch_conv)
      // 16 pixel columns (lanes of a lane group), then the lane groups that share a GroupNorm group, then the WM wave rows through LDS
      const int cpg = a.Cout >> 5;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { gs[i] += __shfl_xor(gs[i], o); gq[i] += __shfl_xor(gq[i], o); }
        if (cpg >= 8) { gs[i] += __shfl_xor(gs[i], 16); gq[i] += __shfl_xor(gq[i], 16); }
        if (cpg >= 16) { gs[i] += __shfl_xor(gs[i], 32); gq[i] += __shfl_xor(gq[i], 32); }
      }
      __syncthreads();                      // everyone is done with the halo / weight tiles: smem is free
      float* red = (float*)smem;            // [wave][i][g][2]
      if (l15 == 0) {
#pragma unroll
        for (int i = 0; i < NI; ++i) { red[((wave * NI + i) * 4 + g) * 2] = gs[i]; red[((wave * NI + i) * 4 + g) * 2 + 1] = gq[i]; }
      }
      __syncthreads();
      // one thread per GroupNorm group of this workgroup's BN channels: channel c0 = first channel of the group inside the tile
      const int ngrp = BN / cpg;
      if (tid < ngrp) {
        const int c0 = tid * cpg, wn_ = c0 / (NI * 16), i_ = (c0 % (NI * 16)) / 16, g_ = (c0 % 16) / 4;
        float ts = 0.f, tq = 0.f;
#pragma unroll
        for (int m = 0; m < WM; ++m) {      // fixed order over the wave rows
          const int w = m * WN + wn_;
          ts += red[((w * NI + i_) * 4 + g_) * 2]; tq += red[((w * NI + i_) * 4 + g_) * 2 + 1];
        }
        const int ntile = nty * ntx, tile = ty * ntx + tx;
        float* o = a.gn_part + (((size_t)b * ntile + tile) * 32 + (n0 / cpg + tid)) * 2;
        o[0] = ts; o[1] = tq;
      }
    }
  }
}

// ---- GroupNorm statistics: partial (sum, sumsq) per (image, pixel chunk, group) -----------------
__global__ __launch_bounds__(256) void gn_partial_kernel(const h16* __restrict__ x, float* __restrict__ part, int HW,
                                                         int C, int nchunk) {
  __shared__ float red[2][256 * 8];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int nslot = C / 8, npl = 256 / nslot;       // 8-channel slots per pixel, pixel lanes
  const int slot = tid % nslot, pl = tid / nslot;
  const int per = (HW + nchunk - 1) / nchunk;
  const int p0 = chunk * per, p1 = min(HW, p0 + per);
  float s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
  for (int p = p0 + pl; p < p1; p += npl) {
    const h16x8 v = *(const h16x8*)(x + ((size_t)b * HW + p) * C + slot * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) { const float f = (float)v[e]; s[e] += f; q[e] = fmaf(f, f, q[e]); }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[0][pl * C + slot * 8 + e] = s[e]; red[1][pl * C + slot * 8 + e] = q[e]; }
  __syncthreads();
  // The upper levels of the reduction add few, large, same-signed terms: in fp32 each of those additions costs up to half an ulp of the TOTAL, and
  // var = E[x^2] - mean^2 magnifies that by mean^2 / var (4 096 for a group whose |mean| is 64 x its std).  They run in fp64 (a handful of
  // additions per thread); only the many leaf sums above stay fp32, where the errors are small against the total and average out.
  for (int c = tid; c < C; c += 256) {               // fixed-order sum over pixel lanes
    double ts = 0.0, tq = 0.0;
    for (int l = 0; l < npl; ++l) { ts += (double)red[0][l * C + c]; tq += (double)red[1][l * C + c]; }
    red[0][c] = (float)ts; red[1][c] = (float)tq;    // row 0 of the scratch is only read by thread c here
  }
  __syncthreads();
  if (tid < 32) {
    const int cpg = C / 32;
    double ts = 0.0, tq = 0.0;
    for (int e = 0; e < cpg; ++e) { ts += (double)red[0][tid * cpg + e]; tq += (double)red[1][tid * cpg + e]; }
    float* o = part + (((size_t)b * nchunk + chunk) * 32 + tid) * 2;
    o[0] = (float)ts; o[1] = (float)tq;
  }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float2* __restrict__ out, int HW, int C, int nchunk) {
  // 256 threads = 32 groups x 8 chunk lanes: lane l sums chunks l, l+8, ... in order, then the 8 lanes are summed in order (fixed association:
  // bit-stable run to run whatever produced the partials)
  // The per-tile partials are combined, and the variance formed, in fp64: E[x^2] - mean^2 cancels mean^2 / var leading digits (12 bits for a group whose
  // |mean| is 64 x its std -- trained decoders show such groups), and fp32 sums of up to 256 same-signed partials alone lose 2 - 3 bits of the 24.
  __shared__ double red[2][8][32];
  __shared__ float2 ms[32];
  const int b = blockIdx.x, grp = threadIdx.x & 31, l = threadIdx.x >> 5;
  const int cpg = C / 32;
  double ts = 0.0, tq = 0.0;
  for (int k = l; k < nchunk; k += 8) {
    const float* o = part + (((size_t)b * nchunk + k) * 32 + grp) * 2;
    ts += (double)o[0]; tq += (double)o[1];
  }
  red[0][l][grp] = ts; red[1][l][grp] = tq;
  __syncthreads();
  if (threadIdx.x < 32) {
    ts = 0.0; tq = 0.0;
    for (int k = 0; k < 8; ++k) { ts += red[0][k][grp]; tq += red[1][k][grp]; }
    const double n = (double)HW * (double)cpg;
    const double mean = ts / n;
    const double var = fmax(tq / n - mean * mean, 0.0);
    ms[grp] = make_float2((float)mean, (float)(1.0 / sqrt(var + 1e-6)));
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    const float2 m = ms[c / cpg];
    const float sc = m.y * gamma[c];
    out[(size_t)b * C + c] = make_float2(sc, beta[c] - m.x * sc);
  }
}

// ---- tokens -> +-1 latent, NHWC padded to 64 channels (lookup_free.py:96-111, conv_vqgan.py:107-110)
__global__ void latent_kernel(const int64_t* __restrict__ tokens, h16* __restrict__ z, size_t npix, int K) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix * CK; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i / CK; const int c = (int)(i - p * CK);
    float v = 0.f;
    if (c < K) v = ((tokens[p] >> c) & 1) ? 1.f : -1.f;
    z[i] = to_h(v);
  }
}

// ---- OIHW fp32 -> [tap][Cout_pad][Cin_pad] h16 ---------------------------------------------------
__global__ void repack_conv_kernel(const float* __restrict__ w, h16* __restrict__ out, int Cout, int Cin, int ks,
                                   int Cout_pad, int Cin_pad) {
  const size_t total = (size_t)ks * ks * Cout_pad * Cin_pad;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin_pad); size_t r = i / Cin_pad;
    const int co = (int)(r % Cout_pad); const int tap = (int)(r / Cout_pad);
    float v = 0.f;
    if (ci < Cin && co < Cout) v = w[((size_t)co * Cin + ci) * ks * ks + tap];
    out[i] = to_h(v);
  }
}

// ---- encoder half (ConvEncoder, autoencoder.py:230-286; LFQ sign/pack, lookup_free.py:57-62,113-127) -------------
// image fp32 NCHW -> fp16 NHWC padded to 64 channels
__global__ void pack_image_kernel(const float* __restrict__ img, h16* __restrict__ out, int B, int C, int H, int W) {
  const size_t npix = (size_t)B * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix * 8; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i >> 3; const int slot = (int)(i & 7);
    const size_t b = p / ((size_t)H * W), yx = p - b * (size_t)H * W;
    h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (slot == 0)
      for (int c = 0; c < C && c < 8; ++c) v[c] = to_h(img[(b * C + c) * (size_t)H * W + yx]);
    *(h16x8*)(out + p * CK + slot * 8) = v;
  }
}
// space-to-depth: x[B,H,W,C] -> y[B,H/2,W/2,4C], channel (py*2+px)*C + c <- pixel (2Y+py, 2X+px)
__global__ void s2d_kernel(const h16* __restrict__ x, h16* __restrict__ y, int B, int H, int W, int C) {
  const int c8 = C / 8;
  const size_t total = (size_t)B * H * W * c8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int sl = (int)(i % c8); size_t p = i / c8;
    const int X = (int)(p % W); p /= W; const int Y = (int)(p % H); const size_t b = p / H;
    const h16x8 v = *(const h16x8*)(x + ((b * H + Y) * W + X) * C + sl * 8);
    *(h16x8*)(y + (((b * (H / 2) + (Y >> 1)) * (W / 2) + (X >> 1)) * 4 + ((Y & 1) * 2 + (X & 1))) * C + sl * 8) = v;
  }
}
// F.avg_pool2d(kernel 2, stride 2) (autoencoder.py:182): x[B,H,W,C] -> y[B,H/2,W/2,C], fp32 mean of the four fp16 inputs
__global__ void avgpool2_kernel(const h16* __restrict__ x, h16* __restrict__ y, int B, int H, int W, int C) {
  const int c8 = C / 8, Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)B * Ho * Wo * c8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int sl = (int)(i % c8); size_t p = i / c8;
    const int X = (int)(p % Wo); p /= Wo; const int Y = (int)(p % Ho); const size_t b = p / Ho;
    const h16* src = x + ((b * H + 2 * Y) * W + 2 * X) * C + sl * 8;
    const h16x8 v00 = *(const h16x8*)src, v01 = *(const h16x8*)(src + C), v10 = *(const h16x8*)(src + (size_t)W * C),
                v11 = *(const h16x8*)(src + (size_t)W * C + C);
    h16x8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = to_h(((float)v00[c] + (float)v01[c] + (float)v10[c] + (float)v11[c]) * 0.25f);
    *(h16x8*)(y + ((b * Ho + Y) * Wo + X) * C + sl * 8) = o;
  }
}
// F.max_pool2d(kernel 2, stride 2) (the VGG16 stack of lpips.hip): x[B,H,W,C] -> y[B,H/2,W/2,C]; the maximum of fp16 values is exact
__global__ void maxpool2_kernel(const h16* __restrict__ x, h16* __restrict__ y, int B, int H, int W, int C) {
  const int c8 = C / 8, Ho = H / 2, Wo = W / 2;
  const size_t total = (size_t)B * Ho * Wo * c8;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int sl = (int)(i % c8); size_t p = i / c8;
    const int X = (int)(p % Wo); p /= Wo; const int Y = (int)(p % Ho); const size_t b = p / Ho;
    const h16* src = x + ((b * H + 2 * Y) * W + 2 * X) * C + sl * 8;
    const h16x8 v00 = *(const h16x8*)src, v01 = *(const h16x8*)(src + C), v10 = *(const h16x8*)(src + (size_t)W * C),
                v11 = *(const h16x8*)(src + (size_t)W * C + C);
    h16x8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (h16)fmaxf(fmaxf((float)v00[c], (float)v01[c]), fmaxf((float)v10[c], (float)v11[c]));
    *(h16x8*)(y + ((b * Ho + Y) * Wo + X) * C + sl * 8) = o;
  }
}
// OIHW 3x3 stride-2 weights -> [tap (by,bx)][Cout_pad][4*Cin] for the 2x2 conv on the space-to-depth input:
// tap (by,bx), channel (py*2+px)*Cin + ci  <-  w[co][ci][2by+py][2bx+px] (zero where that index is 3)
__global__ void repack_down_kernel(const float* __restrict__ w, h16* __restrict__ out, int Cout, int Cin, int Cout_pad) {
  const size_t total = (size_t)4 * Cout_pad * 4 * Cin;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % (4 * Cin)); size_t r = i / (4 * Cin);
    const int co = (int)(r % Cout_pad); const int tap = (int)(r / Cout_pad);
    const int ci = ch % Cin, pp = ch / Cin, py = pp >> 1, px = pp & 1, by = tap >> 1, bx = tap & 1;
    const int dy = 2 * by + py, dx = 2 * bx + px;
    float v = 0.f;
    if (co < Cout && dy < 3 && dx < 3) v = w[(((size_t)co * Cin + ci) * 3 + dy) * 3 + dx];
    out[i] = to_h(v);
  }
}
// z[B*h*w, Kp] (fp16 NHWC) -> indices (bit j = z_j > 0, LSB first), optional +-1 latent and raw z as fp32 NCHW
__global__ void lfq_kernel(const h16* __restrict__ z, int64_t* __restrict__ idx, float* __restrict__ zq, float* __restrict__ zraw,
                           int B, int HW, int K, int Kp) {
  const size_t npix = (size_t)B * HW;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (size_t)gridDim.x * blockDim.x) {
    const size_t b = p / HW, yx = p - b * HW;
    int64_t code = 0;
    for (int j = 0; j < K; ++j) {
      const float v = (float)z[p * Kp + j];
      const bool pos = v > 0.0f;
      code |= (int64_t)pos << j;
      if (zq) zq[(b * K + j) * HW + yx] = pos ? 1.0f : -1.0f;
      if (zraw) zraw[(b * K + j) * HW + yx] = v;
    }
    idx[p] = code;
  }
}


// ================================================================================================
namespace {
constexpr int GN_MAXCHUNK = 64;

// 16-row tiles (8 waves) for the 3x3 convolutions from 32 x 32 maps on; 8-row tiles below (a 16 x 16 map would be one tile per image).  The choice
// must not depend on the batch: the GroupNorm partial sums are per tile, and results are bit-identical across batch sizes.
bool tile16(int ks, int H) { return ks == 3 && H % 16 == 0 && H >= 32; }
}  // namespace

void shape_conv(Conv& c, int cin, int cout, int ks, bool bias, bool up, bool final_) {
  c.cin = cin; c.cout = cout; c.cout_w = cout; c.ks = ks; c.has_bias = bias; c.up = up;
  c.cin_pad = (cin + CK - 1) / CK * CK;
  c.cout_pad = final_ ? 16 : (cout + 127) / 128 * 128;
}
void shape_down_conv(Conv& c, int ch) {
  c.cin = ch; c.cout = ch; c.cout_w = ch; c.ks = 2; c.has_bias = true; c.down = true;
  c.cin_pad = 4 * ch; c.cout_pad = (ch + 127) / 128 * 128;
}
size_t conv_weight_elems(const Conv& c) { return (size_t)c.ks * c.ks * c.cout_pad * c.cin_pad; }
size_t gn_part_elems(int B, int H, int W) { return (size_t)B * std::max(GN_MAXCHUNK, (H / TH8) * (W / TW)) * 64; }

void launch_repack_conv(hipStream_t s, const float* w_oihw, h16* out, int cout, int cin, int ks, int cout_pad, int cin_pad, bool down) {
  if (down) hipLaunchKernelGGL(repack_down_kernel, dim3(512), dim3(256), 0, s, w_oihw, out, cout, cin, cout_pad);
  else hipLaunchKernelGGL(repack_conv_kernel, dim3(512), dim3(256), 0, s, w_oihw, out, cout, cin, ks, cout_pad, cin_pad);
}
void launch_s2d(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C) {
  const size_t n8 = (size_t)B * H * W * (C / 8);
  hipLaunchKernelGGL(s2d_kernel, dim3((unsigned)std::min<size_t>(4096, (n8 + 255) / 256)), dim3(256), 0, s, x, y, B, H, W, C);
}
void launch_avgpool2(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C) {
  const size_t n8 = (size_t)B * H * W * (C / 8);
  hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)std::min<size_t>(4096, (n8 / 4 + 255) / 256)), dim3(256), 0, s, x, y, B, H, W, C);
}
void launch_maxpool2(hipStream_t s, const h16* x, h16* y, int B, int H, int W, int C) {
  const size_t n8 = (size_t)B * H * W * (C / 8);
  hipLaunchKernelGGL(maxpool2_kernel, dim3((unsigned)std::min<size_t>(4096, (n8 / 4 + 255) / 256)), dim3(256), 0, s, x, y, B, H, W, C);
}
void launch_latent(hipStream_t s, const int64_t* tokens, h16* z, size_t npix, int K) {
  hipLaunchKernelGGL(latent_kernel, dim3((unsigned)std::min<size_t>(2048, (npix * CK + 255) / 256)), dim3(256), 0, s, tokens, z, npix, K);
}
void launch_pack_image(hipStream_t s, const float* img, h16* out, int B, int C, int H, int W) {
  const size_t npix = (size_t)B * H * W;
  hipLaunchKernelGGL(pack_image_kernel, dim3((unsigned)std::min<size_t>(4096, (npix * 8 + 255) / 256)), dim3(256), 0, s, img, out, B, C, H, W);
}
void launch_lfq(hipStream_t s, const h16* z, int64_t* idx, float* zq, float* zraw, int B, int HW, int K, int Kp) {
  const size_t np = (size_t)B * HW;
  hipLaunchKernelGGL(lfq_kernel, dim3((unsigned)std::min<size_t>(1024, (np + 255) / 256)), dim3(256), 0, s, z, idx, zq, zraw, B, HW, K, Kp);
}

void launch_conv(hipStream_t s, GnCtx* gc, const Conv& c, const h16* in, const float2* gn, const h16* residual, h16* out,
                 float* img, uint8_t* u8, int B, int H, int W, bool final_, bool stats, bool gn_silu) {
  assert((gn_silu || !gn || (c.ks == 1 && !final_)) && "the GroupNorm prologue without SiLU is built for 1x1 convolutions only");
  // GroupNorm partials of the output ride in the epilogue when a GroupNorm will read it (stats) and its groups are whole lane groups of a tile
  const int cpg = c.cout / 32;
  const bool part = !final_ && stats && c.cout % 128 == 0 && (cpg == 4 || cpg == 8 || cpg == 16);
  ConvArgs a{in, gn, c.w, c.has_bias ? c.b : nullptr, residual, out, img, u8, B, H, W, c.cin_pad, c.cout, c.cout_pad, c.sat, part ? gc->part : nullptr};
  gc->of = part ? (const void*)out : nullptr;
  const int bn = final_ ? 16 : 128;
  const bool th16 = !final_ && tile16(c.ks, H);
  const int th = th16 ? 16 : TH8;
  gc->ntile = (H / th) * (W / TW);
  dim3 grid((unsigned)((size_t)B * (H / th) * (W / TW) * (c.cout_pad / bn))), block(32 * th);
  if (final_) hipLaunchKernelGGL((conv_kernel<1, 1, 3, false, true>), grid, block, 0, s, a);
  else if (c.ks == 1 && gn && !gn_silu) hipLaunchKernelGGL((conv_kernel<4, 2, 1, false, false, 8, false, false>), grid, block, 0, s, a);
  else if (c.ks == 1) hipLaunchKernelGGL((conv_kernel<4, 2, 1, false, false>), grid, block, 0, s, a);
  else if (c.ks == 2) hipLaunchKernelGGL((conv_kernel<4, 2, 2, false, false>), grid, block, 0, s, a);
  else if (c.up && th16) hipLaunchKernelGGL((conv_kernel<4, 2, 3, true, false, 16>), grid, block, 0, s, a);
  else if (c.up) hipLaunchKernelGGL((conv_kernel<4, 2, 3, true, false>), grid, block, 0, s, a);
  else if (th16) hipLaunchKernelGGL((conv_kernel<4, 2, 3, false, false, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv_kernel<4, 2, 3, false, false>), grid, block, 0, s, a);
}

void launch_conv_relu(hipStream_t s, const ConvRelu& q) {
  ConvArgs a{q.in, nullptr, q.w, q.bias, nullptr, q.out, nullptr, nullptr, q.B, q.H, q.W, q.cin_pad, q.cout, q.cout_pad, q.sat, nullptr};
  const bool th16 = tile16(q.ks, q.H);
  const int th = th16 ? 16 : TH8;
  dim3 grid((unsigned)((size_t)q.B * (q.H / th) * (q.W / TW) * (q.cout_pad / 128))), block(32 * th);
  if (q.ks == 1) hipLaunchKernelGGL((conv_kernel<4, 2, 1, false, false, 8, true>), grid, block, 0, s, a);
  else if (th16) hipLaunchKernelGGL((conv_kernel<4, 2, 3, false, false, 16, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((conv_kernel<4, 2, 3, false, false, 8, true>), grid, block, 0, s, a);
}

void launch_gn(hipStream_t s, GnCtx* gc, const Norm& n, const h16* x, int B, int HW) {
  int nchunk = gc->ntile;
  if (gc->of != (const void*)x) {                   // not the tensor the last conv summed (average-pooled tensors of the encoder): sweep it
    nchunk = HW / 256; if (nchunk < 1) nchunk = 1; if (nchunk > GN_MAXCHUNK) nchunk = GN_MAXCHUNK;
    hipLaunchKernelGGL(gn_partial_kernel, dim3(nchunk, B), dim3(256), 0, s, x, gc->part, HW, n.c, nchunk);
  }
  gc->of = nullptr;
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(256), 0, s, gc->part, n.g, n.b, gc->ss, HW, n.c, nchunk);
}

}  // namespace mb
