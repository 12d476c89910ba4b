// apa_clip_stages.h -- the two stages every one-block-per-clip kernel starts with (apa_cliploss.hip: clip_xent_kernel,
// apa_clipscores.hip: clip_scores_kernel), written once so that both give the same bits -- which are also
// apa_frame_pool_fwd's: fma(x, a, 0) = x * a and fma(x, 1, acc) = acc + x.
//   a[r]        = x[r,:] . w + b0                  one wave per frame row, wave_sum's tree
//   pooled[b,k] = (1/F) sum_f x[b,f,k] a[b,f]      one thread per column, frames in increasing f
// Both are called by every thread of a 256-thread block (4 waves).
#pragma once

#include "apa_device.h"

namespace apa {

constexpr int CLIP_LDS_K = 4096;   // the pooled row (and the gradient row) in LDS up to this K
constexpr int CLIP_LDS_F = 64;     // a[b, :] in LDS up to this F (else re-read from tatt)

// Temporal attention of the clip whose first frame row is rb: tatt[rb + f] = a (tatt == nullptr: not stored) and, with
// a_lds, sa[f] = a.  Returns where the pooling stage reads a[b, :] -- sa, or the rows just written to tatt.  Ends with
// a block barrier.
__device__ __forceinline__ const float* clip_tatt_stage(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ b0, float* __restrict__ tatt,
                                                        float* sa, bool a_lds, size_t rb, int F, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int f = wave; f < F; f += 4) {
    const float* xr = x + (rb + f) * K;
    float acc = 0.f;
    for (int k = lane; k < K; k += 64) acc = fmaf(xr[k], w[k], acc);
    const float a = wave_sum(acc) + b0[0];
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

}  // namespace apa
