// Kernels of the text encoder (RoBERTa-base geometry: hidden 768, 12 heads of 64, at most 128 tokens): the embedding
// gather fused with its LayerNorm, its backward with the three table gradients, softmax attention at head dimension 64
// and erf-GELU.  LayerNorm at D = 768 is the D / 256 = 3 instantiation of the kernels of pointwise.h.
// All are wave64 kernels.  None uses a float atomic: every output element has ONE owner and a summation order fixed by
// the shapes alone, so the same kernels serve the deterministic mode.
#pragma once
#include "pointwise.h"
#include "stcat_platform.h"
#include "stcat_rng.h"

#define STCAT_TXT_D 768
#define STCAT_TXT_NAN __builtin_nanf("")

// ---------------------------------------------------------------------------------
// y = dropout(LayerNorm(word[ids[t]] + pos[pos_ids[t]] + type[0]))     (one wave per token, three float4 per lane)
// ---------------------------------------------------------------------------------
struct EmbedRow { float4 v[3]; };

// the summed embedding row of token t; ok = false (nothing read) when an index is outside its table
static __device__ __forceinline__ bool embed_row(const long* ids, const long* pos_ids, const float* word, const float* pos,
                                                 const float* type, int t, int lane, int V, int P, EmbedRow& e) {
  const long id = ids[t], pid = pos_ids[t];
  if (id < 0 || id >= V || pid < 0 || pid >= P) return false;
  STCAT_UNROLL
  for (int j = 0; j < 3; ++j) {
    const int c = j * 256 + lane * 4;
    const float4 a = stcat_ld4(word + id * STCAT_TXT_D + c), b = stcat_ld4(pos + pid * STCAT_TXT_D + c);
    const float4 ty = stcat_ld4(type + c);
    e.v[j] = make_float4(a.x + b.x + ty.x, a.y + b.y + ty.y, a.z + b.z + ty.z, a.w + b.w + ty.w);
  }
  return true;
}

__global__ void __launch_bounds__(256) embed_ln_fwd_kernel(const long* ids, const long* pos_ids, const float* word,
                                                          const float* pos, const float* type, const float* gamma,
                                                          const float* beta, float* y, float* mean, float* rstd, int L,
                                                          int V, int P, float eps, DropParams drop) {
  drop = stcat_drop_resolve(drop);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int t = blockIdx.x * 4 + w; t < L; t += gridDim.x * 4) {
    EmbedRow e;
    const bool ok = embed_row(ids, pos_ids, word, pos, type, t, lane, V, P, e);   // (wave-uniform)
    if (!ok) {   // an index outside its table: nothing was read; the row is poisoned (the host wrapper refuses such ids)
      for (int j = 0; j < 3; ++j)
        stcat_st4(y + (long)t * STCAT_TXT_D + j * 256 + lane * 4,
                  make_float4(STCAT_TXT_NAN, STCAT_TXT_NAN, STCAT_TXT_NAN, STCAT_TXT_NAN));
      if (lane == 0) { mean[t] = STCAT_TXT_NAN; rstd[t] = STCAT_TXT_NAN; }
      continue;
    }
    float s = 0.f;
    for (int j = 0; j < 3; ++j) s += e.v[j].x + e.v[j].y + e.v[j].z + e.v[j].w;
    const float mu = stcat_wave_sum(s) * (1.f / STCAT_TXT_D);
    float q = 0.f;
    for (int j = 0; j < 3; ++j) {
      e.v[j].x -= mu; e.v[j].y -= mu; e.v[j].z -= mu; e.v[j].w -= mu;
      q += e.v[j].x * e.v[j].x + e.v[j].y * e.v[j].y + e.v[j].z * e.v[j].z + e.v[j].w * e.v[j].w;
    }
    const float rs = 1.f / sqrtf(stcat_wave_sum(q) * (1.f / STCAT_TXT_D) + eps);
    for (int j = 0; j < 3; ++j) {
      const int c = j * 256 + lane * 4;
      const float4 g = stcat_ld4(gamma + c), bt = stcat_ld4(beta + c);
      float4 o = make_float4(e.v[j].x * rs * g.x + bt.x, e.v[j].y * rs * g.y + bt.y, e.v[j].z * rs * g.z + bt.z,
                             e.v[j].w * rs * g.w + bt.w);
      if (drop.thresh) {
        const unsigned long long c0 = (unsigned long long)t * STCAT_TXT_D + c;
        o.x *= stcat_drop_mul(drop, c0); o.y *= stcat_drop_mul(drop, c0 + 1);
        o.z *= stcat_drop_mul(drop, c0 + 2); o.w *= stcat_drop_mul(drop, c0 + 3);
      }
      stcat_st4(y + (long)t * STCAT_TXT_D + c, o);
    }
    if (lane == 0) { mean[t] = mu; rstd[t] = rs; }
  }
}

// de[t] = LayerNorm backward of (mask * dy[t]) with xhat rebuilt from the tables: the gradient of the summed embedding row
__global__ void __launch_bounds__(256) embed_ln_bwd_rows_kernel(const float* dy, const long* ids, const long* pos_ids,
                                                               const float* word, const float* pos, const float* type,
                                                               const float* gamma, const float* mean, const float* rstd,
                                                               float* de, int L, int V, int P, DropParams drop) {
  drop = stcat_drop_resolve(drop);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int t = blockIdx.x * 4 + w; t < L; t += gridDim.x * 4) {
    EmbedRow e;
    const bool ok = embed_row(ids, pos_ids, word, pos, type, t, lane, V, P, e);
    if (!ok) {
      for (int j = 0; j < 3; ++j)
        stcat_st4(de + (long)t * STCAT_TXT_D + j * 256 + lane * 4, make_float4(0.f, 0.f, 0.f, 0.f));
      continue;
    }
    const float mu = mean[t], rs = rstd[t];
    float4 gv[3];
    float s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < 3; ++j) {
      const int c = j * 256 + lane * 4;
      float4 d = stcat_ld4(dy + (long)t * STCAT_TXT_D + c);
      if (drop.thresh) {
        const unsigned long long c0 = (unsigned long long)t * STCAT_TXT_D + c;
        d.x *= stcat_drop_mul(drop, c0); d.y *= stcat_drop_mul(drop, c0 + 1);
        d.z *= stcat_drop_mul(drop, c0 + 2); d.w *= stcat_drop_mul(drop, c0 + 3);
      }
      const float4 g = stcat_ld4(gamma + c);
      e.v[j] = make_float4((e.v[j].x - mu) * rs, (e.v[j].y - mu) * rs, (e.v[j].z - mu) * rs, (e.v[j].w - mu) * rs);
      gv[j] = make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w);
      s1 += gv[j].x + gv[j].y + gv[j].z + gv[j].w;
      s2 += gv[j].x * e.v[j].x + gv[j].y * e.v[j].y + gv[j].z * e.v[j].z + gv[j].w * e.v[j].w;
    }
    const float c1 = stcat_wave_sum(s1) * (1.f / STCAT_TXT_D), c2 = stcat_wave_sum(s2) * (1.f / STCAT_TXT_D);
    for (int j = 0; j < 3; ++j)
      stcat_st4(de + (long)t * STCAT_TXT_D + j * 256 + lane * 4,
                make_float4(rs * (gv[j].x - c1 - e.v[j].x * c2), rs * (gv[j].y - c1 - e.v[j].y * c2),
                            rs * (gv[j].z - c1 - e.v[j].z * c2), rs * (gv[j].w - c1 - e.v[j].w * c2)));
  }
}

// The table rows are written by a GATHER: the workgroup of token t owns row ids[t] of the word table iff no earlier token
// holds the same id, and then sums de over every position with that id in ascending position order (a scatter-add would
// make "the ... the" order-dependent).  The same rule serves the position table.  Row `pad` of either table (RoBERTa's
// padding_idx, -1 = none) is never written, as nn.Embedding(padding_idx=) keeps its gradient at zero.
__global__ void __launch_bounds__(256) embed_ln_bwd_tables_kernel(const float* de, const long* ids, const long* pos_ids,
                                                                 float* dword, float* dpos, int L, int V, int P,
                                                                 int pad) {
  const int t = blockIdx.x;
  for (int table = 0; table < 2; ++table) {
    const long* ix = table ? pos_ids : ids;
    float* out = table ? dpos : dword;
    const long id = ix[t];
    if (id < 0 || id >= (table ? P : V) || id == pad) continue;   // nn.Embedding(padding_idx): that row's gradient stays zero
    bool first = true;
    for (int u = 0; u < t; ++u) first = first && ix[u] != id;
    if (!first) continue;
    for (int c = threadIdx.x; c < STCAT_TXT_D; c += 256) {
      float acc = de[(long)t * STCAT_TXT_D + c];
      for (int u = t + 1; u < L; ++u)
        if (ix[u] == id) acc += de[(long)u * STCAT_TXT_D + c];
      out[id * STCAT_TXT_D + c] = acc;
    }
  }
}

// dgamma[c] += sum_t mask dy xhat, dbeta[c] += sum_t mask dy, dtype[c] += sum_t de: the fixed tree of
// layernorm_bwd_affine_det_kernel (a workgroup per 32 columns, 16 row lanes)
__global__ void __launch_bounds__(STCAT_DET_COLS * STCAT_DET_LANES)
    embed_ln_bwd_cols_kernel(const float* dy, const float* de, const long* ids, const long* pos_ids, const float* word,
                             const float* pos, const float* type, const float* mean, const float* rstd, float* dtype,
                             float* dgamma, float* dbeta, int L, int V, int P, DropParams drop) {
  drop = stcat_drop_resolve(drop);
  __shared__ float red[STCAT_DET_LANES][STCAT_DET_COLS + 1];
  const int cl = threadIdx.x % STCAT_DET_COLS, rl = threadIdx.x / STCAT_DET_COLS, c = blockIdx.x * STCAT_DET_COLS + cl;
  float ag = 0.f, ab = 0.f, at = 0.f;
  for (int t = rl; t < L; t += STCAT_DET_LANES) {
    const long id = ids[t], pid = pos_ids[t];
    if (id < 0 || id >= V || pid < 0 || pid >= P) continue;
    const long i = (long)t * STCAT_TXT_D + c;
    const float x = word[id * STCAT_TXT_D + c] + pos[pid * STCAT_TXT_D + c] + type[c];
    float d = dy[i];
    if (drop.thresh) d *= stcat_drop_mul(drop, (unsigned long long)i);
    ag += d * ((x - mean[t]) * rstd[t]);
    ab += d;
    at += de[i];
  }
  ag = stcat_det_lane_tree(ag, red, rl, cl);
  __syncthreads();
  ab = stcat_det_lane_tree(ab, red, rl, cl);
  __syncthreads();
  at = stcat_det_lane_tree(at, red, rl, cl);
  if (rl == 0) {
    dgamma[c] += ag;
    dbeta[c] += ab;
    dtype[c] += at;
  }
}

// ---------------------------------------------------------------------------------
// softmax attention, head dimension 64, 1 <= S <= 128 (fp32 FMA in every mma mode: a whole layer is 50 MFLOP).
// One workgroup per (batch, head, 32-row tile); a wave owns 8 rows of the tile, a lane two keys of a score row and one
// of the 64 output columns.  The probabilities P [B,H,S,S] (after the softmax, before dropout) are kept for the backward
// pass; the dropout decision of (query, key) is counter ((b H + h) Sp + key) Sp + query, Sp = 32 ceil(S / 32): the layout
// of the head-dimension-32 kernels (attention.h).
// ---------------------------------------------------------------------------------
struct MhaD64Params {
  const float *Q, *K, *V, *dO, *P, *delta_in;
  const unsigned char* kpm;
  float *O, *Pout, *delta, *dQ, *dK, *dV;
  int B, H, S, ldq, ldk, ldv, ldo, ldg, ldgv;
  float scale;
  DropParams drop;
};

// rows [0, n) x 64 columns of a head's slice into LDS with row stride `stride` floats
static __device__ __forceinline__ void d64_stage(float* dst, int stride, const float* src, long ld, int n) {
  for (int i = threadIdx.x; i < n * 16; i += 256) {
    const int r = i >> 4, c = (i & 15) * 4;
    const float4 v = stcat_ld4(src + r * ld + c);
    float* d = dst + r * stride + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
}

static inline int mha_d64_fwd_lds(int S) { const int sp = (S + 31) & ~31; return (S * 64 + 32 * 64 + S * 65 + 32 * (sp + 1)) * 4; }
static inline int mha_d64_dq_lds(int S) { return mha_d64_fwd_lds(S); }
static inline int mha_d64_dkv_lds(int S) { const int sp = (S + 31) & ~31; return (S * 65 + S * 64 + 32 * 64 + 2 * 32 * (sp + 1)) * 4; }

__global__ void __launch_bounds__(256) mha_d64_fwd_kernel(MhaD64Params a) {
  STCAT_DYN_SHARED(float, sm);
  const DropParams drop = stcat_drop_resolve(a.drop);
  const int S = a.S, SP = (S + 31) & ~31, PS = SP + 1;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H, q0 = blockIdx.y * 32;
  const int nq = min(32, S - q0);
  float* Vs = sm;                 // [S][64]
  float* Qs = Vs + S * 64;        // [32][64]
  float* Ks = Qs + 32 * 64;       // [S][65]
  float* Ps = Ks + S * 65;        // [32][SP + 1]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  d64_stage(Vs, 64, a.V + (long)b * S * a.ldv + h * 64, a.ldv, S);
  d64_stage(Ks, 65, a.K + (long)b * S * a.ldk + h * 64, a.ldk, S);
  d64_stage(Qs, 64, a.Q + ((long)b * S + q0) * a.ldq + h * 64, a.ldq, nq);
  __syncthreads();
  for (int rr = 0; rr < 8; ++rr) {
    const int r = w * 8 + rr, q = q0 + r;
    if (q >= S) break;            // (wave-uniform; no workgroup barrier follows)
    float s[2];
    for (int j = 0; j < 2; ++j) {
      const int kk = lane + j * 64;
      s[j] = STCAT_NEG_INF;
      if (kk < S && !(a.kpm && a.kpm[(long)b * S + kk])) {
        float acc = 0.f;
        for (int d = 0; d < 64; ++d) acc = fmaf(Qs[r * 64 + d], Ks[kk * 65 + d], acc);
        s[j] = acc * a.scale;
      }
    }
    const float m = stcat_wave_max(fmaxf(s[0], s[1]));
    float e[2];
    for (int j = 0; j < 2; ++j) e[j] = s[j] == STCAT_NEG_INF ? 0.f : expf(s[j] - m);
    const float sum = stcat_wave_sum(e[0] + e[1]);
    const float inv = sum > 0.f ? 1.f / sum : 0.f;     // (a row whose keys are all padded gives zeros)
    for (int j = 0; j < 2; ++j) {
      const int kk = lane + j * 64;
      if (kk < S) {
        float p = e[j] * inv;
        if (a.Pout) a.Pout[((long)bh * S + q) * S + kk] = p;
        p *= stcat_drop_mul(drop, ((unsigned long long)bh * SP + kk) * SP + q);
        Ps[r * PS + kk] = p;
      }
    }
    STCAT_WAVE_LDS_FENCE();
    float o = 0.f;
    for (int kk = 0; kk < S; ++kk) o = fmaf(Ps[r * PS + kk], Vs[kk * 64 + lane], o);
    a.O[((long)b * S + q) * a.ldo + h * 64 + lane] = o;
  }
}

// dQ of a 32-row query tile and delta[q] = sum_k P mask dP (the row term of the softmax backward, kept for the dK / dV kernel)
__global__ void __launch_bounds__(256) mha_d64_bwd_dq_kernel(MhaD64Params a) {
  STCAT_DYN_SHARED(float, sm);
  const DropParams drop = stcat_drop_resolve(a.drop);
  const int S = a.S, SP = (S + 31) & ~31, PS = SP + 1;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H, q0 = blockIdx.y * 32;
  const int nq = min(32, S - q0);
  float* Ks = sm;                 // [S][64]
  float* Gs = Ks + S * 64;        // [32][64]  dO of the tile
  float* Vs = Gs + 32 * 64;       // [S][65]
  float* Ds = Vs + S * 65;        // [32][SP + 1]  dS of the tile
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  d64_stage(Ks, 64, a.K + (long)b * S * a.ldk + h * 64, a.ldk, S);
  d64_stage(Vs, 65, a.V + (long)b * S * a.ldv + h * 64, a.ldv, S);
  d64_stage(Gs, 64, a.dO + ((long)b * S + q0) * a.ldo + h * 64, a.ldo, nq);
  __syncthreads();
  for (int rr = 0; rr < 8; ++rr) {
    const int r = w * 8 + rr, q = q0 + r;
    if (q >= S) break;
    float p[2], g[2];
    float part = 0.f;
    for (int j = 0; j < 2; ++j) {
      const int kk = lane + j * 64;
      p[j] = 0.f; g[j] = 0.f;
      if (kk < S) {
        float acc = 0.f;
        for (int d = 0; d < 64; ++d) acc = fmaf(Gs[r * 64 + d], Vs[kk * 65 + d], acc);
        p[j] = a.P[((long)bh * S + q) * S + kk];
        g[j] = acc * stcat_drop_mul(drop, ((unsigned long long)bh * SP + kk) * SP + q);
        part += p[j] * g[j];
      }
    }
    const float delta = stcat_wave_sum(part);
    if (lane == 0) a.delta[(long)bh * S + q] = delta;
    for (int j = 0; j < 2; ++j) {
      const int kk = lane + j * 64;
      if (kk < S) Ds[r * PS + kk] = p[j] * (g[j] - delta);
    }
    STCAT_WAVE_LDS_FENCE();
    float o = 0.f;
    for (int kk = 0; kk < S; ++kk) o = fmaf(Ds[r * PS + kk], Ks[kk * 64 + lane], o);
    a.dQ[((long)b * S + q) * a.ldg + h * 64 + lane] = o * a.scale;
  }
}

// dK and dV of a 32-row key tile: the tile's workgroup is the only writer of its rows and walks the queries in order
__global__ void __launch_bounds__(256) mha_d64_bwd_dkv_kernel(MhaD64Params a) {
  STCAT_DYN_SHARED(float, sm);
  const DropParams drop = stcat_drop_resolve(a.drop);
  const int S = a.S, SP = (S + 31) & ~31, PS = SP + 1;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H, k0 = blockIdx.y * 32;
  const int nk = min(32, S - k0);
  float* Qs = sm;                 // [S][64]
  float* Vt = Qs + S * 64;        // [32][64]  V of the tile
  float* Gs = Vt + 32 * 64;       // [S][65]   dO
  float* Ds = Gs + S * 65;        // [32][SP + 1]  dS^T
  float* Pm = Ds + 32 * PS;       // [32][SP + 1]  (P mask)^T
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  d64_stage(Qs, 64, a.Q + (long)b * S * a.ldq + h * 64, a.ldq, S);
  d64_stage(Gs, 65, a.dO + (long)b * S * a.ldo + h * 64, a.ldo, S);
  d64_stage(Vt, 64, a.V + ((long)b * S + k0) * a.ldv + h * 64, a.ldv, nk);
  __syncthreads();
  for (int rr = 0; rr < 8; ++rr) {
    const int r = w * 8 + rr, kk = k0 + r;
    if (kk >= S) break;
    for (int j = 0; j < 2; ++j) {
      const int q = lane + j * 64;
      if (q < S) {
        float acc = 0.f;
        for (int d = 0; d < 64; ++d) acc = fmaf(Gs[q * 65 + d], Vt[r * 64 + d], acc);
        const float p = a.P[((long)bh * S + q) * S + kk];
        const float mk = stcat_drop_mul(drop, ((unsigned long long)bh * SP + kk) * SP + q);
        Ds[r * PS + q] = p * (acc * mk - a.delta_in[(long)bh * S + q]);
        Pm[r * PS + q] = p * mk;
      }
    }
    STCAT_WAVE_LDS_FENCE();
    float dk = 0.f, dv = 0.f;
    for (int q = 0; q < S; ++q) {
      dk = fmaf(Ds[r * PS + q], Qs[q * 64 + lane], dk);
      dv = fmaf(Pm[r * PS + q], Gs[q * 65 + lane], dv);
    }
    a.dK[((long)b * S + kk) * a.ldg + h * 64 + lane] = dk * a.scale;
    a.dV[((long)b * S + kk) * a.ldgv + h * 64 + lane] = dv;
  }
}

// ---------------------------------------------------------------------------------
// erf-GELU (RoBERTa's hidden_act "gelu"): y = x / 2 (1 + erf(x / sqrt 2)); backward takes dy and x.
// Four elements per thread through 16-byte accesses; the last n % 4 elements go through the scalar tail.
// ---------------------------------------------------------------------------------
static __device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }
static __device__ __forceinline__ float gelu_b(float dy, float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * expf(-0.5f * x * x);
  return dy * (cdf + x * pdf);
}

// a = x (forward) or dy (backward, then b = x)
__global__ void __launch_bounds__(256) gelu_kernel(int bwd, const float* a, const float* b, float* out, long n) {
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const float4 x = stcat_ld4(a + i * 4);
    float4 r;
    if (bwd) {
      const float4 xx = stcat_ld4(b + i * 4);
      r = make_float4(gelu_b(x.x, xx.x), gelu_b(x.y, xx.y), gelu_b(x.z, xx.z), gelu_b(x.w, xx.w));
    } else {
      r = make_float4(gelu_f(x.x), gelu_f(x.y), gelu_f(x.z), gelu_f(x.w));
    }
    stcat_st4(out + i * 4, r);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = n4 * 4 + threadIdx.x;
    out[i] = bwd ? gelu_b(a[i], b[i]) : gelu_f(a[i]);
  }
}
