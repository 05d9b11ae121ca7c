// Device-side clip transforms (datasets/transforms.py:47-168 of the reference: hflip, resize, crop, normalize as float
// tensor ops on a loader worker): ONE launch resizes a window of the source clip to a window of a virtual output and
// applies a per-channel affine, out = a[c] * interp + b[c].
//
//   source   uint8 [n,h,w,3] (decoder layout) or fp32 [n,3,h,w]; taps clamp at the edges of the clamp window
//            (win_y, win_x, win_h, win_w); with `flip`, column j of the window is source column win_w - 1 - j
//   output   fp32 [n,3,oh,ow], the part (oy0, ox0, oh, ow) of the virtual (OH, OW) image whose size sets the scales
//   filter   antialias off: torch's upsample_bilinear2d, align_corners=False (two taps per axis);
//            antialias on : torch's separable triangle filter (support max(scale, 1) per axis)
//
// One 256-thread workgroup owns a TH x TW tile of one frame, all three channels, in four steps with LDS between them:
//   1. per-axis tap tables (first tap, count, weights) of the tile's rows and columns
//   2. the source rows x columns those taps touch -> LDS as floats, in WINDOW coordinates (the flip is applied here);
//      uint8 rows are read as aligned 32-bit words.  Halo rows shared with the neighbour tiles come from L2.
//   3. width pass : mid[c][source row][x]   = sum_k wx[x][k] * src[c][row][x0[x] + k]       (LDS -> LDS)
//   4. height pass: out[c][y][x]            = a[c] * sum_k wy[y][k] * mid[c][y0[y] + k][x] + b[c]
//      every lane owns four consecutive x of one row, cut at 16-byte boundaries of the OUTPUT ADDRESS (not of the row),
//      so rows that start unaligned (ow % 4 != 0) still store float4 everywhere but at their two ends.
// Tiles are 2^i rows x 4 * 2^j - 4 columns (16 x 60 unless a strong down-scale needs more LDS than 64 KiB): a tile row
// is then 2^j lanes wide in step 4 whatever its phase, a wave owns a whole row in steps 2 and 3, and no loop divides.
// The width-then-height order is torch's, for both filters.  Every sum is one product followed by explicit fmaf steps, so
// the vector path, the scalar row ends and every tiling give the same bits for the same output element.  No atomics: the result does not depend on the mode.
#pragma once

#include <cstdint>

#include "stcat_platform.h"

struct ClipResizeParams {
  const void* src;
  float* out;
  const float* a;
  const float* b;
  long src_bytes;                        // extent of the whole source (the aligned word reads stay inside it)
  int n, h, w;                           // source dims
  int win_y, win_x, win_h, win_w, flip;  // clamp window
  int OH, OW;                            // virtual output size
  float sy, sx;                          // scales (float)win_h / OH, (float)win_w / OW, as torch forms them
  int oy0, ox0, oh, ow;                  // output window = the tensor written
  int antialias;
  int TH, TW, lgTH, lgG;                 // tile: TH = 1 << lgTH rows, TW = 4 G - 4 <= 60 columns, G = 1 << lgG (step 4)
  int rcap, ccap;                        // staged source rows / columns per tile (upper bounds, clip_span_cap)
  int mty, mtx;                          // taps per output row / column (upper bounds, clip_tap_cap)
};

// host and device agree on these bounds; the kernel additionally clamps every LDS index it forms
static inline int clip_tap_cap(int in, int out, int aa) {
  if (!aa) return 2;
  const float s = (float)in / (float)out;
  return 2 * (int)ceilf(s >= 1.f ? s : 1.f) + 2;
}
// source rows (columns) touched by `tile` consecutive outputs: the first taps of two outputs t apart differ by at most
// s t + 1, the last output adds its own taps
static inline int clip_span_cap(int in, int out, int aa, int tile) {
  const float s = (float)in / (float)out;
  const long cap = (long)(s * (float)(tile - 1)) + 2 + clip_tap_cap(in, out, aa);
  return (int)(cap < in ? cap : in);
}
static __host__ __device__ inline int clip_round4(int v) { return (v + 3) & ~3; }
// LDS floats of one tile: mid | src | wx | wy | x0 nx y0 ny   (each part a multiple of 4 floats: mid stays 16-byte aligned)
static inline long clip_lds_floats(const ClipResizeParams& p) {
  return (long)3 * p.rcap * (p.TW + 4) + clip_round4(3 * p.rcap * p.ccap) + (long)p.TW * p.mtx +
         clip_round4(p.TH * p.mty) + 2 * p.TW + clip_round4(2 * p.TH);
}

// taps of output index d of an axis resized in -> out: first tap t0, count nt (<= maxt), weights w[0 .. nt)
static __device__ __forceinline__ void clip_axis_taps(int d, int in, float s, bool aa, int maxt, int& t0, int& nt,
                                                      float* w) {
  if (!aa) {
    float src = s * ((float)d + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    int i0 = (int)src;
    i0 = i0 > in - 1 ? in - 1 : i0;
    const float l1 = src - (float)i0;
    t0 = i0;
    nt = 2;  // the second tap is i0 + 1 clamped to in - 1 where it is read
    w[0] = 1.f - l1;
    w[1] = l1;
    return;
  }
  const float sup = s >= 1.f ? s : 1.f, inv = s >= 1.f ? 1.f / s : 1.f;
  const float center = s * ((float)d + 0.5f);
  int lo = (int)(center - sup + 0.5f), hi = (int)(center + sup + 0.5f);
  lo = lo < 0 ? 0 : (lo > in - 1 ? in - 1 : lo);
  hi = hi > in ? in : hi;
  int cnt = hi - lo;
  cnt = cnt < 1 ? 1 : (cnt > maxt ? maxt : cnt);
  float total = 0.f;
  for (int j = 0; j < cnt; ++j) {
    const float t = fabsf(((float)(j + lo) - center + 0.5f) * inv);
    const float v = t < 1.f ? 1.f - t : 0.f;
    w[j] = v;
    total += v;
  }
  if (total != 0.f)
    for (int j = 0; j < cnt; ++j) w[j] /= total;
  t0 = lo;
  nt = cnt;
}

template <bool U8, bool AA>
__global__ __launch_bounds__(256) void clip_resize_kernel(ClipResizeParams p) {
  STCAT_DYN_SHARED(float, sm);
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * p.TW, ty0 = blockIdx.y * p.TH, frame = blockIdx.z;
  const int tw = min(p.TW, p.ow - tx0), th = min(p.TH, p.oh - ty0);
  const int MP = p.TW + 4;
  float* mid = sm;
  float* srcl = mid + 3 * p.rcap * MP;
  float* wx = srcl + clip_round4(3 * p.rcap * p.ccap);
  float* wy = wx + p.TW * p.mtx;
  int* x0 = reinterpret_cast<int*>(wy + clip_round4(p.TH * p.mty));
  int* nx = x0 + p.TW;
  int* y0 = nx + p.TW;
  int* ny = y0 + p.TH;

  // 1. tap tables
  for (int t = tid; t < tw + th; t += 256) {
    if (t < tw)
      clip_axis_taps(p.ox0 + tx0 + t, p.win_w, p.sx, AA, p.mtx, x0[t], nx[t], wx + t * p.mtx);
    else
      clip_axis_taps(p.oy0 + ty0 + (t - tw), p.win_h, p.sy, AA, p.mty, y0[t - tw], ny[t - tw], wy + (t - tw) * p.mty);
  }
  __syncthreads();
  const int rlo = y0[0], clo = x0[0];
  const int R = min(min(y0[th - 1] + ny[th - 1], p.win_h) - rlo, p.rcap);
  const int C = min(min(x0[tw - 1] + nx[tw - 1], p.win_w) - clo, p.ccap);

  // 2. stage rows [rlo, rlo + R) x columns [clo, clo + C) of the window; sc0 = the first SOURCE column of that range
  const int sc0 = p.win_x + (p.flip ? p.win_w - clo - C : clo);
  if (U8) {
    const unsigned char* base = static_cast<const unsigned char*>(p.src);
    const uintptr_t lo_ok = (reinterpret_cast<uintptr_t>(base) + 3) & ~uintptr_t(3);
    const uintptr_t hi_ok = reinterpret_cast<uintptr_t>(base) + (uintptr_t)p.src_bytes;
    const int nw = (3 * C + 3) / 4 + 1;  // 32-bit words that cover a row segment starting anywhere in a word
    for (int i = tid; i < R * 64; i += 256) {  // one wave per source row
      const int r = i >> 6;
      const unsigned char* row = base + (((long)frame * p.h + p.win_y + rlo + r) * p.w + sc0) * 3;
      const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
      for (int k = i & 63; k < nw; k += 64) {
        const int b0 = 4 * k - mis;  // byte of the row segment at which this word starts
        if (b0 >= 3 * C) continue;
        const uintptr_t wa = reinterpret_cast<uintptr_t>(row + b0);
        unsigned word = 0;
        if (wa >= lo_ok && wa + 4 <= hi_ok) {
          word = *reinterpret_cast<const unsigned*>(row + b0);
        } else {
          for (int e = 0; e < 4; ++e)
            if (b0 + e >= 0 && b0 + e < 3 * C) word |= (unsigned)row[b0 + e] << (8 * e);
        }
        int sc = (b0 + 3) / 3 - 1, ch = b0 - 3 * sc;  // pixel and channel of the word's first byte (b0 >= -3)
        STCAT_UNROLL
        for (int e = 0; e < 4; ++e) {
          const int bp = b0 + e;
          if (bp >= 0 && bp < 3 * C)
            srcl[(ch * R + r) * p.ccap + (p.flip ? C - 1 - sc : sc)] = (float)((word >> (8 * e)) & 255u);
          if (++ch == 3) {
            ch = 0;
            ++sc;
          }
        }
      }
    }
  } else {
    const float* base = static_cast<const float*>(p.src);
    for (int i = tid; i < 3 * R * 64; i += 256) {  // one wave per (channel, source row)
      const int cr = i >> 6;
      const int ch = cr / R, r = cr - ch * R;
      const float* row = base + (((long)frame * 3 + ch) * p.h + p.win_y + rlo + r) * p.w + sc0;
      for (int sc = i & 63; sc < C; sc += 64) srcl[cr * p.ccap + (p.flip ? C - 1 - sc : sc)] = row[sc];
    }
  }
  __syncthreads();

  // 3. width pass.  mid columns are shifted by M so that the rows of the tile whose output address has the phase of
  // its first row (all of them when ow % 4 == 0) read their four values as one aligned float4
  const int out_phase = (int)((reinterpret_cast<uintptr_t>(p.out) >> 2) & 3);
  const int M = (int)((out_phase + ((long)frame * 3 * p.oh + ty0) * p.ow + tx0) & 3);
  if ((tid & 63) < tw) {  // one wave per (channel, source row), a lane per column (TW <= 60): its taps stay in registers
    const int x = tid & 63;
    const float* w = wx + x * p.mtx;
    const int j0 = x0[x] - clo, cnt = AA ? nx[x] : 2;
    const int ja = min(j0, C - 1), jb = min(j0 + 1, C - 1);
    const float w0 = w[0], w1 = cnt > 1 ? w[1] : 0.f;
    for (int cr = tid >> 6; cr < 3 * R; cr += 4) {
      const float* row = srcl + cr * p.ccap;
      float acc = w0 * row[ja];
      if (cnt > 1) acc = fmaf(w1, row[jb], acc);
      if (AA)
        for (int k = 2; k < cnt; ++k) acc = fmaf(w[k], row[min(j0 + k, C - 1)], acc);
      mid[cr * MP + x + M] = acc;
    }
  }
  __syncthreads();

  // 4. height pass + affine + store
  for (int i = tid; i < ((3 << p.lgTH) << p.lgG); i += 256) {
    const int cy = i >> p.lgG, q = i & ((1 << p.lgG) - 1);
    const int ch = cy >> p.lgTH, y = cy & (p.TH - 1);
    if (y >= th) continue;
    const long off = (((long)frame * 3 + ch) * p.oh + ty0 + y) * p.ow + tx0;
    const int g = (int)((out_phase + off) & 3);
    const int xl = 4 * q - g;  // first of this lane's four columns: out + off + xl is 16-byte aligned
    if (xl >= tw) continue;
    const float* w = wy + y * p.mty;
    const int r0 = y0[y] - rlo, cnt = AA ? ny[y] : 2;
    const float sa = p.a[ch], sb = p.b[ch];
    const float* mrow = mid + ch * R * MP;
    if (xl >= 0 && xl + 4 <= tw) {
      float4 acc;
      if (g == M) {
        const float4 v = stcat_ld4(mrow + min(r0, R - 1) * MP + 4 * q);
        acc = make_float4(w[0] * v.x, w[0] * v.y, w[0] * v.z, w[0] * v.w);
        for (int k = 1; k < cnt; ++k) {
          const float4 u = stcat_ld4(mrow + min(r0 + k, R - 1) * MP + 4 * q);
          acc = make_float4(fmaf(w[k], u.x, acc.x), fmaf(w[k], u.y, acc.y), fmaf(w[k], u.z, acc.z),
                            fmaf(w[k], u.w, acc.w));
        }
      } else {
        const float* v = mrow + min(r0, R - 1) * MP + xl + M;
        acc = make_float4(w[0] * v[0], w[0] * v[1], w[0] * v[2], w[0] * v[3]);
        for (int k = 1; k < cnt; ++k) {
          const float* u = mrow + min(r0 + k, R - 1) * MP + xl + M;
          acc = make_float4(fmaf(w[k], u[0], acc.x), fmaf(w[k], u[1], acc.y), fmaf(w[k], u[2], acc.z),
                            fmaf(w[k], u[3], acc.w));
        }
      }
      stcat_st4(p.out + off + xl,
                make_float4(fmaf(sa, acc.x, sb), fmaf(sa, acc.y, sb), fmaf(sa, acc.z, sb), fmaf(sa, acc.w, sb)));
    } else {
      for (int e = 0; e < 4; ++e) {
        const int x = xl + e;
        if (x < 0 || x >= tw) continue;
        float acc = w[0] * mrow[min(r0, R - 1) * MP + x + M];
        for (int k = 1; k < cnt; ++k) acc = fmaf(w[k], mrow[min(r0 + k, R - 1) * MP + x + M], acc);
        p.out[off + x] = fmaf(sa, acc, sb);
      }
    }
  }
}
