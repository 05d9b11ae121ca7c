// The two sums of the canonical window (stcat_amd.set_canonical_window(N)): the mean gradient of an
// optimizer step as ONE fp32 expression over its N clips, whatever the split of the clips over ranks and micro-steps —
//   ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)),  times fp32(1 / N) once after the last add
// — a balanced binary tree over the clips in index order.  Clip c = m * world + r runs on rank r at micro-step m, so the
// lower log2(world) levels of the tree add the ranks of one micro-step (rank_tree_kernel, from the ordered exchange of
// stcat_amd/dist.py), the upper log2(k) levels add the micro-steps (grad_tree_fold_kernel, from AdamW.accumulate / step).
// Both are pure HBM streams modelled on rank_sum.h: one float4 per lane (a scalar tail), non-temporal loads, every load of
// an element issued before its first add, one owner per element — no atomics, no LDS, no cross-lane operation.  The
// order of the adds is the order written here: fp32 adds are not reassociated without a fast-math flag (the build line
// has none), and a multiply AFTER an add cannot contract into an fma.
#pragma once

#include "optim.h"
#include "stcat_platform.h"

constexpr int RANK_TREE_MAX = 8;       // ranks of one tree (powers of two up to here)
constexpr int GRAD_TREE_LEVELS = 4;    // level buffers per table row: k = 2^q micro-steps need q of them, so k <= 16

// element (group) of NR slices: all loads, then the adjacent-pair tree in rank order — width 1 adds (0,1) (2,3) ...,
// width 2 adds (01,23) (45,67), width 4 adds (0123, 4567) — then the one multiply.  NR = 1: slice 0 itself (a -0.0f
// with scale 1 stays a -0.0f: nothing is added to it).
template <typename T, int NR>
static __device__ __forceinline__ T rank_tree(const T* src, long stride, float scale) {
  T v[NR];
  STCAT_UNROLL
  for (int j = 0; j < NR; ++j) v[j] = STCAT_LOAD_STREAM(src + j * stride);
  STCAT_UNROLL
  for (int w = 1; w < NR; w *= 2) {
    STCAT_UNROLL
    for (int j = 0; j + w < NR; j += 2 * w) v[j] = v[j] + v[j + w];
  }
  return v[0] * scale;
}

// out, in 16-byte aligned, stride % 4 == 0 (the entry point refuses anything else): n / 4 float4 groups grid-strided over
// the workgroups, the n % 4 tail elements by the first lanes of workgroup 0.  An element is read (every rank) and written
// by one thread, which reads before it writes: out may be one of the slices.
template <int NR>
__global__ void __launch_bounds__(256) rank_tree_kernel(float* out, const float* in, long n, long stride, float scale) {
  const long step = (long)gridDim.x * blockDim.x;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n4 = n >> 2, stride4 = stride >> 2;
  const f32x4* in4 = reinterpret_cast<const f32x4*>(in);
  f32x4* out4 = reinterpret_cast<f32x4*>(out);
  for (long g = t; g < n4; g += step) out4[g] = rank_tree<f32x4, NR>(in4 + g, stride4, scale);
  const long i = (n4 << 2) + t;
  if (t < 4 && i < n) out[i] = rank_tree<float, NR>(in + i, stride, scale);
}

// The fold of micro-step m into the level buffers of one table row (a binary counter: level j holds the sum of 2^j
// consecutive clips' worth of micro-steps, or nothing).  NC = the number of trailing one bits of m = the levels that
// are full and are consumed now:
//   carry = g;  carry = L_j + carry  for j = 0 .. NC - 1   (the level is the LEFT operand: it holds the earlier clips)
//   last ? carry *= scale : nothing
// `dst` is level NC, or — on the window's last micro-step, where every level is consumed — the top level consumed.
// The level pointers of a row sit in the columns the fold has no other use for: p, m, v, ema = levels 0, 1, 2, 3.
static __device__ __forceinline__ const float* grad_tree_level(const OptTensor& t, int j) {
  return j == 0 ? t.p : j == 1 ? t.m : j == 2 ? t.v : t.ema;
}

template <typename T, int NC>
static __device__ __forceinline__ T grad_tree_carry(const float* g, const OptTensor& t, long i, bool last, float scale) {
  T lv[NC > 0 ? NC : 1];
  T carry = STCAT_LOAD_STREAM(reinterpret_cast<const T*>(g + i));
  STCAT_UNROLL
  for (int j = 0; j < NC; ++j) lv[j] = STCAT_LOAD_STREAM(reinterpret_cast<const T*>(grad_tree_level(t, j) + i));
  STCAT_UNROLL
  for (int j = 0; j < NC; ++j) carry = lv[j] + carry;
  if (last) carry = carry * scale;
  return carry;
}

template <int NC>
__global__ void __launch_bounds__(256) grad_tree_fold_kernel(const OptTensor* tab, const int* chunk_tensor,
                                                             const long* chunk_off, int chunk, int last, float scale) {
  const OptTensor t = tab[chunk_tensor[blockIdx.x]];
  const long lo = chunk_off[blockIdx.x];
  const long hi = lo + chunk < t.n ? lo + chunk : t.n;
  const float* g = t.g;
  float* dst = const_cast<float*>(grad_tree_level(t, last ? NC - 1 : NC));
  unsigned long bits = (unsigned long)(g + lo) | (unsigned long)(dst + lo);
  STCAT_UNROLL
  for (int j = 0; j < NC; ++j) bits |= (unsigned long)(grad_tree_level(t, j) + lo);
  if ((bits & 15u) == 0) {
    const long nv = lo + ((hi - lo) / 4) * 4;
    for (long i = lo + (long)threadIdx.x * 4; i < nv; i += 256 * 4)
      *reinterpret_cast<f32x4*>(dst + i) = grad_tree_carry<f32x4, NC>(g, t, i, last != 0, scale);
    const long j = nv + threadIdx.x;    // ragged tail (< 4 elements), one lane each
    if (j < hi) dst[j] = grad_tree_carry<float, NC>(g, t, j, last != 0, scale);
  } else {
    for (long i = lo + threadIdx.x; i < hi; i += 256) dst[i] = grad_tree_carry<float, NC>(g, t, i, last != 0, scale);
  }
}
