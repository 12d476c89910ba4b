// apa_clip_stages.h -- the stages of frame pooling and its backward, written once for the one-block-per-clip kernels
// (apa_cliploss.hip: clip_xent_kernel / clip_finish_kernel, apa_clipscores.hip: clip_scores_kernel) and the module path
// (apa_framepool.hip: one launch per stage), so that all give the same bits:
//   a[r]        = x[r,:] . w + b0                  one wave per frame row, wave_sum's tree          clip_tatt_row
//   pooled[b,k] = (1/F) sum_f x[b,f,k] a[b,f]      one thread per column, frames in increasing f    clip_pool_col
//   d[r], G[r,:]                                   one wave per frame row                           clip_grad_row
//   dw[k]       = sum_r d[r] x[r,k]                one thread per column, rows in increasing r      clip_dw_col
// clip_pool_col starts from x * a where fp_pool_kernel starts from fma(x, a, 0): the same bits but for the sign of a
// zero sum, so that kernel keeps its own loop.  The *_stage forms are called by every thread of a 256-thread block.
#pragma once

#include "apa_device.h"

namespace apa {

constexpr int CLIP_LDS_K = 4096;   // the pooled row (and the gradient row) in LDS up to this K
constexpr int CLIP_LDS_F = 64;     // a[b, :] in LDS up to this F (else re-read from tatt)

// a of one frame row xr, by ONE wave (wave-uniform)
__device__ __forceinline__ float clip_tatt_row(const float* __restrict__ xr, const float* __restrict__ w,
                                               const float* __restrict__ b0, int K, int lane) {
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc = fmaf(xr[k], w[k], acc);
  return wave_sum(acc) + b0[0];
}

// Temporal attention of the clip whose first frame row is rb: tatt[rb + f] = a (tatt == nullptr: not stored) and, with
// a_lds, sa[f] = a.  Returns where the pooling stage reads a[b, :] -- sa, or the rows just written to tatt.  Ends with
// a block barrier.
__device__ __forceinline__ const float* clip_tatt_stage(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b0, float* __restrict__ tatt,
                                                        float* sa, bool a_lds, size_t rb, int F, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int f = wave; f < F; f += 4) {
    const float a = clip_tatt_row(x + (rb + f) * K, w, b0, K, lane);
    if (lane == 0) {
      if (tatt) tatt[rb + f] = a;
      if (a_lds) sa[f] = a;
    }
  }
  __syncthreads();
  return a_lds ? sa : tatt + rb;
}

// One column of the pooled row; xc = &x[rb, k] (F == 1 without attention: x * 1)
template <bool TEMPORAL>
__device__ __forceinline__ float clip_pool_col(const float* __restrict__ xc, const float* ap, int F, int K) {
  float acc = TEMPORAL ? xc[0] * ap[0] : xc[0];
  int f = 1;
  for (; f + 8 <= F; f += 8) {   // eight loads in flight, added in frame order (HMDB-51 tests on 25 frames a clip)
    float xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) xv[u] = xc[(size_t)(f + u) * K];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = TEMPORAL ? fmaf(xv[u], ap[f + u], acc) : acc + xv[u];
  }
  for (; f < F; ++f) {
    const float xv = xc[(size_t)f * K];
    acc = TEMPORAL ? fmaf(xv, ap[f], acc) : acc + xv;
  }
  return acc * (1.0f / (float)F);
}

// The pooled row of the clip: prow[k] (where the block goes on reading it) and, when given, out[k] as well.  No
// barrier: the caller places one before it reads prow.
template <bool TEMPORAL>
__device__ __forceinline__ void clip_pool_stage(const float* __restrict__ x, const float* ap, float* prow, float* out,
                                                size_t rb, int F, int K) {
  for (int k = threadIdx.x; k < K; k += 256) {
    const float p = clip_pool_col<TEMPORAL>(x + rb * K + k, ap, F, K);
    prow[k] = p;
    if (out) out[k] = p;
  }
}

// The gradient at the logits of frame row r, by ONE wave: g = the gradient row of the row's clip at the pooled logits.
//   plain:     G[r,k] = (1/F) g[k]
//   temporal:  d = (1/F) sum_k g[k] x[r,k] -> dws[r];  G[r,k] = (1/F) g[k] a[r] + d w[k]   (a_r: where a[r] is read)
template <bool TEMPORAL>
__device__ __forceinline__ void clip_grad_row(const float* __restrict__ x, const float* __restrict__ w, const float* g,
                                              const float* a_r, float* __restrict__ G, float* __restrict__ dws, size_t r,
                                              int K, float invF, int lane) {
  if (!TEMPORAL) {
    for (int k = lane; k < K; k += 64) G[r * K + k] = g[k] * invF;
  } else {
    const float* xr = x + r * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(g[k], xr[k], acc);
    const float d = wave_sum(acc) * invF;
    const float a = a_r[0];
    for (int k = lane; k < K; k += 64) G[r * K + k] = fmaf(g[k] * invF, a, d * w[k]);
    if (lane == 0) dws[r] = d;
  }
}

// dw[k] = sum_r dws[r] x[r,k] by one thread, rows in increasing r
__device__ __forceinline__ float clip_dw_col(const float* __restrict__ x, const float* __restrict__ dws, int rows, int K,
                                             int k) {
  float acc = 0.f;
  int r = 0;
  for (; r + 8 <= rows; r += 8) {   // eight loads in flight, added in row order
    float xv[8], dv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { xv[u] = x[(size_t)(r + u) * K + k]; dv[u] = dws[r + u]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fmaf(dv[u], xv[u], acc);
  }
  for (; r < rows; ++r) acc = fmaf(dws[r], x[(size_t)r * K + k], acc);
  return acc;
}

}  // namespace apa
