// The cross-rank gradient sum of the ordered data-parallel exchange (stcat_amd/dist.py): `in` holds n_ranks slices of n
// floats, slice k at in + k * stride (what all_to_all_single delivered: every rank's copy of this rank's shard), and
//   out[i] = (((in[i] + in[stride + i]) + in[2 stride + i]) + ...) * scale
// — fp32, round to nearest, rank 0 first, ONE multiply after the last add.  The order is the whole point: a collective's
// own reduction order changes with its algorithm, the topology and the channel count, this chain never does.  One form,
// in and out of deterministic mode: no atomics, no LDS, no cross-lane operation — an element is read and written by one
// thread, which reads every rank's value before it writes, so `out` may be one of the slices.
//
// A pure HBM stream (n_ranks * n * 4 bytes read once, n * 4 written): one float4 per lane per rank, the loads of up to
// RANK_SUM_BATCH ranks in flight before the first add, further ranks in batches that continue the same chain.  The loads
// are non-temporal (every byte is read once); the stores are plain (the all-gather reads `out` next).
#pragma once

#include "stcat_platform.h"

constexpr int RANK_SUM_BATCH = 8;

// NB slices starting at src: all loads first, then the chain (FIRST: the chain starts with slice 0 itself, not 0 + it —
// a -0.0f stays a -0.0f)
template <typename T, int NB, bool FIRST>
static __device__ __forceinline__ T rank_sum_batch(T acc, const T* src, long stride) {
  T v[NB];
  STCAT_UNROLL
  for (int j = 0; j < NB; ++j) v[j] = STCAT_LOAD_STREAM(src + j * stride);
  if (FIRST) acc = v[0];
  STCAT_UNROLL
  for (int j = FIRST ? 1 : 0; j < NB; ++j) acc = acc + v[j];
  return acc;
}

template <typename T, bool FIRST>
static __device__ __forceinline__ T rank_sum_some(T acc, int nb, const T* src, long stride) {
  switch (nb) {
    case 1: return rank_sum_batch<T, 1, FIRST>(acc, src, stride);
    case 2: return rank_sum_batch<T, 2, FIRST>(acc, src, stride);
    case 3: return rank_sum_batch<T, 3, FIRST>(acc, src, stride);
    case 4: return rank_sum_batch<T, 4, FIRST>(acc, src, stride);
    case 5: return rank_sum_batch<T, 5, FIRST>(acc, src, stride);
    case 6: return rank_sum_batch<T, 6, FIRST>(acc, src, stride);
    case 7: return rank_sum_batch<T, 7, FIRST>(acc, src, stride);
    default: return rank_sum_batch<T, RANK_SUM_BATCH, FIRST>(acc, src, stride);
  }
}

// element (group) g of every slice, T = float4-wide vector or float; stride in units of T
template <typename T>
static __device__ __forceinline__ T rank_sum_chain(const T* src, int n_ranks, long stride, float scale) {
  int left = n_ranks;
  int nb = left < RANK_SUM_BATCH ? left : RANK_SUM_BATCH;
  T acc = rank_sum_some<T, true>(T{}, nb, src, stride);
  for (left -= nb; left > 0; left -= nb) {
    src += (long)nb * stride;
    nb = left < RANK_SUM_BATCH ? left : RANK_SUM_BATCH;
    acc = rank_sum_some<T, false>(acc, nb, src, stride);
  }
  return acc * scale;
}

// VEC: out, in 16-byte aligned and stride % 4 == 0 — n / 4 float4 groups grid-strided over the workgroups, the n % 4
// tail elements by the first lanes of workgroup 0.  !VEC: one float per lane, any alignment.
template <bool VEC>
__global__ void __launch_bounds__(256) rank_sum_kernel(float* out, const float* in, int n_ranks, long n, long stride,
                                                      float scale) {
  const long step = (long)gridDim.x * blockDim.x;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    const long n4 = n >> 2, stride4 = stride >> 2;
    const f32x4* in4 = reinterpret_cast<const f32x4*>(in);
    f32x4* out4 = reinterpret_cast<f32x4*>(out);
    for (long g = t; g < n4; g += step) out4[g] = rank_sum_chain<f32x4>(in4 + g, n_ranks, stride4, scale);
    const long i = (n4 << 2) + t;
    if (t < 4 && i < n) out[i] = rank_sum_chain<float>(in + i, n_ranks, stride, scale);
  } else {
    for (long i = t; i < n; i += step) out[i] = rank_sum_chain<float>(in + i, n_ranks, stride, scale);
  }
}
