// apa_multihead.hip -- H independent class-agnostic heads (M == 1, Xatt == X) fed from ONE streaming pass over the
// cached features per direction (include/apa_multihead.h).
//
// The shape of apa_m1_rank.hip, in its independent form, built from the same row routines (apa_rowpass.h: ownership,
// loader, dot, keep bits, merges).  The forward pass keeps the H rows of Wa in LDS and H accumulator sets in registers;
// the backward pass keeps the image's H rows of dz in LDS and H sets of dWa accumulators in registers, and walks each
// block's pixels in the direction opposite to the forward pass (the rows the forward pass of the same block read last
// are the likeliest to still sit in that XCD's L2).  The keep bits of a row are drawn once and serve all heads.  The
// small products and the loss carry the head as a grid dimension, so a step has the same number of launches whatever H
// is.  The three products are exact fp32 on v_mfma_f32_16x16x4_f32 (mfma16) with operands straight from global memory,
// as in apa_m1_small.hip.  Nothing is accumulated with floating-point atomics, every run repeats bit for bit.
#include <math.h>

#include "../../include/apa_multihead.h"
#include "apa_device.h"
#include "apa_internal.h"
#include "apa_rowpass.h"

namespace apa {
namespace {
constexpr int HMAX = APA_HEADS_MAX;

// --------------------------------------------------------------------------------------------
// Forward pass.  grid N * S blocks of 256 threads; block (n, s) owns pixels [p_begin, p_end) of batch image n = cache
// image clamp(index[n]), wave w the pixels p_begin + w, + 4, ...  Outputs: att [H,N,P], and per block
// pacc [blk][H][C] = sum_p A_h Xt, pstat [blk][4] = sum_p A_h.
// --------------------------------------------------------------------------------------------
template <typename T, int NVL, bool TRAIN>
__global__ __launch_bounds__(256, 2) void mh_pool_fwd_kernel(const T* __restrict__ X, const float* __restrict__ Wa,
                                                             const float* __restrict__ ba, float* __restrict__ att,
                                                             float* __restrict__ pacc, float* __restrict__ pstat, int N,
                                                             int P, int S, int C, int H, int act, float inv_keep,
                                                             uint32_t thresh, uint64_t seed, uint64_t offset, M1Gather g) {
  constexpr int EPV = Vec<T>::EPV, EL = NVL * EPV, CP = 64 * EL;
  __shared__ float sm[3 * EL * 64];
  __shared__ __attribute__((aligned(16))) float sm_wa[HMAX * CP];
  __shared__ float sm_stat[4][HMAX];
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset, k0, k1);
  const int blk = blockIdx.x, n = blk / S, s = blk % S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int p_begin, p_end;
  m1_pix_range(s, P, S, p_begin, p_end);
  const int nvec = C / EPV;
  m1_gather_note(n, s == 0 && threadIdx.x == 0, g);
  float bias[HMAX];
#pragma unroll
  for (int h = 0; h < HMAX; ++h) bias[h] = h < H ? ba[h] : 0.f;
  float acc[HMAX][EL];
#pragma unroll
  for (int h = 0; h < HMAX; ++h)
#pragma unroll
    for (int i = 0; i < EL; ++i) acc[h][i] = 0.f;
  float asum[HMAX] = {0.f, 0.f, 0.f, 0.f};
  const T* xim = X + (size_t)m1_src_image(n, g) * P * C;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);   // the loader and the dot, inline:
  uint4 nxt[NVL];                                  // profiles/rowpass_summary.md (timing)
  if (p_begin + wave < p_end) {
#pragma unroll
    for (int j = 0; j < NVL; ++j) {
      const int v = j * 64 + lane;
      nxt[j] = v < nvec ? ld16(xim + (size_t)(p_begin + wave) * C + (size_t)v * EPV) : zero4;
    }
  }
  // the H rows of attention weights wait in LDS (zero beyond C and beyond H): the registers belong to the H accumulator
  // sets.  Staged behind the first row's loads, which travel meanwhile
  for (int i = threadIdx.x; i < HMAX * CP; i += 256) {
    const int h = i / CP, c = i - h * CP;
    sm_wa[i] = (h < H && c < C) ? Wa[(size_t)h * C + c] : 0.f;
  }
  __syncthreads();
  for (int p = p_begin + wave; p < p_end; p += 4) {
    float x[EL];
#pragma unroll
    for (int j = 0; j < NVL; ++j) Vec<T>::unpack(nxt[j], x + j * EPV);
    if (p + 4 < p_end) {   // the next row travels while this one is consumed
#pragma unroll
      for (int j = 0; j < NVL; ++j) {
        const int v = j * 64 + lane;
        nxt[j] = v < nvec ? ld16(xim + (size_t)(p + 4) * C + (size_t)v * EPV) : zero4;
      }
    }
    float A[HMAX];
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
      A[h] = 0.f;
      if (h < H) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < NVL; ++j) {
#pragma unroll
          for (int e = 0; e < EPV; e += 4) {
            const float4 w4 = *reinterpret_cast<const float4*>(sm_wa + h * CP + (j * 64 + lane) * EPV + e);
            const int i = j * EPV + e;
            d = fmaf(x[i], w4.x, d); d = fmaf(x[i + 1], w4.y, d);
            d = fmaf(x[i + 2], w4.z, d); d = fmaf(x[i + 3], w4.w, d);
          }
        }
        const float z = wave_sum(d) + bias[h];
        A[h] = act == M1_ACT_RELU ? fmaxf(z, 0.f) : z;
      }
    }
    if (lane < H)
      att[((size_t)lane * N + n) * P + p] = lane == 0 ? A[0] : (lane == 1 ? A[1] : (lane == 2 ? A[2] : A[3]));
    if (TRAIN) {
      const uint32_t bits = row_keep_bits<RngLib, NVL, EPV>(((uint64_t)n * P + p) * C, lane, nvec, k0, k1, thresh);
#pragma unroll
      for (int i = 0; i < EL; ++i) x[i] = (bits >> i) & 1u ? x[i] : 0.f;
    }
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
      if (h < H) {
        asum[h] += A[h];
        const float ak = TRAIN ? A[h] * inv_keep : A[h];
#pragma unroll
        for (int i = 0; i < EL; ++i) acc[h][i] = fmaf(ak, x[i], acc[h][i]);
      }
    }
  }
  // ---- combine the 4 waves (fixed order), one head at a time ----
  float* pa = pacc + (size_t)blk * H * C;
#pragma unroll
  for (int h = 0; h < HMAX; ++h)
    if (h < H) row_merge4<NVL, EPV>(acc[h], sm, pa + (size_t)h * C, wave, lane, nvec);
  if (lane == 0) {
#pragma unroll
    for (int h = 0; h < HMAX; ++h) sm_stat[wave][h] = asum[h];
  }
  __syncthreads();
  if (threadIdx.x < HMAX) {
    const int h = threadIdx.x;
    pstat[(size_t)blk * 4 + h] = row_stat_merge4(sm_stat, h);
  }
}

// Merge of the S block partials of each image (fixed order): zsave [H,N,C] and abar [H,N].  grid (N, ceil(C / 1024), H).
__global__ __launch_bounds__(256) void mh_finalize_fwd_kernel(const float* __restrict__ pacc,
                                                              const float* __restrict__ pstat, int N, int P, int S, int C,
                                                              int H, float* __restrict__ zsave, float* __restrict__ abar) {
  const int n = blockIdx.x, h = blockIdx.z;
  const float invP = 1.0f / (float)P;
  const int i = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (i < C) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const float4 v = *reinterpret_cast<const float4*>(pacc + (((size_t)n * S + s) * H + h) * C + i);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    a.x *= invP; a.y *= invP; a.z *= invP; a.w *= invP;
    *reinterpret_cast<float4*>(zsave + ((size_t)h * N + n) * C + i) = a;
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) {
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += pstat[((size_t)n * S + s) * 4 + h];
    abar[(size_t)h * N + n] = a * invP;
  }
}

// ---- the small products: exact fp32 on v_mfma_f32_16x16x4_f32, operands straight from global memory, the head as
// grid.z (the forms of apa_m1_small.hip: lane (r, kq) = (lane & 15, lane >> 4) supplies A[row r][k = kq] and
// B[k = kq][column r] of a 16 x 4 by 4 x 16 step and holds D[row 4 kq + reg][column r]; fixed summation order).  A wave
// owns MT 16-row tiles that share its B operand.
//
// logits[h,n,k] = sum_c z[h,n,c] Wt[h,c,k] + abar[h,n] bt[h,k].  grid (ceil(K / 16), ceil(N / (16 MT)), H), LW waves per
// block: wave w multiplies the 4-channel groups [w (C/4) / LW, (w + 1) (C/4) / LW) of MT image tiles by one 16-column
// tile of Wt, wave 0 adds the LW partial tiles in wave order and the bias term.  hs: rows between two heads of `logits`
// (N in a step, the epoch's count in an evaluation epoch).
constexpr int LW = 16;
template <int MT>
__global__ __launch_bounds__(64 * LW) void mh_logits_kernel(const float* __restrict__ z, const float* __restrict__ Wt,
                                                            const float* __restrict__ abar, const float* __restrict__ bt,
                                                            float* __restrict__ logits, int N, int C, int K, size_t hs) {
  __shared__ float sm[LW - 1][MT][4][64];
  const int h = blockIdx.z, n0 = blockIdx.y * 16 * MT, k0 = blockIdx.x * 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  const int ngrp = C / 4;
  const int g0 = (int)(((long)wave * ngrp) / LW), g1 = (int)(((long)(wave + 1) * ngrp) / LW);
  const float* zr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) zr[t] = z + ((size_t)h * N + min(n0 + t * 16 + r, N - 1)) * C + kq;
  const float* w = Wt + (size_t)h * C * K + (size_t)kq * K + min(k0 + r, K - 1);
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int g = g0;
  for (; g + 4 <= g1; g += 4) {   // four steps' operands in flight
    float b[4], a[4][MT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      b[u] = w[(size_t)(g + u) * 4 * K];
#pragma unroll
      for (int t = 0; t < MT; ++t) a[u][t] = zr[t][(g + u) * 4];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = mfma16(a[u][t], b[u], acc[t]);
  }
  for (; g < g1; ++g) {
    const float b = w[(size_t)g * 4 * K];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = mfma16(zr[t][g * 4], b, acc[t]);
  }
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) sm[wave - 1][t][e][lane] = acc[t][e];
  }
  __syncthreads();
  const int k = k0 + r;
  if (wave == 0 && k < K) {
#pragma unroll
    for (int t = 0; t < MT; ++t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + t * 16 + kq * 4 + e;
        if (n < N) {
          float s = acc[t][e];
          for (int q = 0; q < LW - 1; ++q) s += sm[q][t][e][lane];
          logits[((size_t)h * hs + n) * K + k] = fmaf(abar[(size_t)h * N + n], bt[(size_t)h * K + k], s);
        }
      }
    }
  }
}

// One logits row's softmax (half-wave forms for 4 <= K <= 1024, the stream form otherwise: apa_xent_row.h) on ONE whole
// wave.  probs / G: the row's K floats or nullptr.  Returns the row's loss; *cand: the first maximal index.
__device__ __forceinline__ float mh_softmax_row(const float* __restrict__ row, int K, int lab, float* __restrict__ probs,
                                                float* __restrict__ G, float gscale, int* cand) {
  if (xent_row_half_wave(K)) {
    return xent_row_3pass(row, K, lab, probs != nullptr || G != nullptr, [&](int c, float p) {
      if (probs) probs[c] = p;
      if (G) G[c] = xent_grad(p, gscale, c == lab);
    }, cand);
  }
  return xent_row_stream([&](int k) { return row[k]; }, K, lab, probs != nullptr, probs, G != nullptr, G, gscale, cand);
}

// The cross-entropy rows of all heads: one wave per row (h, n).  grid ceil(H N / 4).
__global__ __launch_bounds__(256) void mh_xent_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      float* __restrict__ loss, float* __restrict__ G, int H, int N, int K,
                                                      float gscale) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= H * N) return;
  const int h = r / N, n = r - h * N;
  const float lv = mh_softmax_row(logits + (size_t)r * K, K, (int)labels[n], nullptr, G + (size_t)r * K, gscale, nullptr);
  if ((threadIdx.x & 63) == 0) loss[(size_t)h * (1 + N) + 1 + n] = lv;
}

// loss[h,0] = lscale * sum_n loss[h,1+n]: thread t adds rows t, t + 256, ..., wave_sum, (w0 + w1) + (w2 + w3).  grid H.
__global__ __launch_bounds__(256) void mh_loss_mean_kernel(float* __restrict__ loss, int N, float lscale) {
  __shared__ float red[4];
  float* l = loss + (size_t)blockIdx.x * (1 + N);
  const float t = block_sum256(xent_mean256_load(l + 1, N), red);
  if (threadIdx.x == 0) l[0] = t * lscale;
}

// dz[h,n,c] = sum_k G[h,n,k] Wt[h,c,k], and sn[h,n] = G[h,n,:] . bt[h,:] (the bias' share of dA, handed to the backward
// pass).  grid (ceil(C / 64), ceil(N / (16 MT)), H), four waves: wave w owns the 16 channels c0 + 16 w .. of MT image
// tiles.  Both operands are contiguous along the contraction: a lane takes columns kb + 4 kq .. + 3 of a 16-column chunk
// with one 16-byte load per operand (rows of K floats are 4-byte aligned: unaligned dwordx4) and step e of the chunk
// contracts the columns kb + 4 kq' + e; the last, partial chunk is loaded column by column, zero past K.
template <int MT>
__global__ __launch_bounds__(256) void mh_dz_kernel(const float* __restrict__ G, const float* __restrict__ Wt,
                                                    const float* __restrict__ bt, float* __restrict__ dz,
                                                    float* __restrict__ sn, int N, int C, int K) {
  const int h = blockIdx.z, n0 = blockIdx.y * 16 * MT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  const int c0 = blockIdx.x * 64 + wave * 16;
  if (blockIdx.x == 0) {   // sn of this block's images: one wave per image, lanes stride the columns
    for (int i = wave; i < 16 * MT && n0 + i < N; i += 4) {
      const float* g = G + ((size_t)h * N + n0 + i) * K;
      float a = 0.f;
      for (int k = lane; k < K; k += 64) a = fmaf(g[k], bt[(size_t)h * K + k], a);
      a = wave_sum(a);
      if (lane == 0) sn[(size_t)h * N + n0 + i] = a;
    }
  }
  if (c0 >= C) return;
  const float* gr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) gr[t] = G + ((size_t)h * N + min(n0 + t * 16 + r, N - 1)) * K + 4 * kq;
  const float* w = Wt + ((size_t)h * C + min(c0 + r, C - 1)) * K + 4 * kq;
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  int kb = 0;
  for (; kb + 16 <= K; kb += 16) {
    const f4u b = *reinterpret_cast<const f4u*>(w + kb);
    f4u a[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const f4u*>(gr[t] + kb);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = mfma16(a[t][e], b[e], acc[t]);
  }
  if (kb < K) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = kb + 4 * kq + e < K;
      const float b = in ? w[kb + e] : 0.f;
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = mfma16(in ? gr[t][kb + e] : 0.f, b, acc[t]);
    }
  }
  const int c = c0 + r;
  if (c < C) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + t * 16 + kq * 4 + e;
        if (n < N) dz[((size_t)h * N + n) * C + c] = acc[t][e];
      }
  }
}

// dWt[h,c,k] = sum_n z[h,n,c] G[h,n,k], and as row c == C: dbt[h,k] = sum_n abar[h,n] G[h,n,k]; images in ascending
// groups of four.  grid (ceil(K / 16), ceil(ceil((C + 1) / 16) / (4 WT)), H), four waves: wave w owns the WT 16-row
// tiles of channels from (4 blockIdx.y + w) WT on and one 16-column tile of G.
constexpr int WT = 4;
__global__ __launch_bounds__(256) void mh_dwt_kernel(const float* __restrict__ z, const float* __restrict__ abar,
                                                     const float* __restrict__ G, float* __restrict__ dWt,
                                                     float* __restrict__ dbt, int N, int C, int K) {
  const int h = blockIdx.z, k0 = blockIdx.x * 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  const int ct0 = (blockIdx.y * 4 + wave) * WT;
  if (ct0 * 16 > C) return;
  const float* zb = z + (size_t)h * N * C;
  const float* ab = abar + (size_t)h * N;
  const float* gb = G + (size_t)h * N * K + min(k0 + r, K - 1);
  f32x4 acc[WT];
#pragma unroll
  for (int t = 0; t < WT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto step = [&](int nb) {
    const int n = nb + kq;
    const bool in = n < N;
    const int nc = min(n, N - 1);
    const float b = in ? gb[(size_t)nc * K] : 0.f;
    float a[WT];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
      const int c = (ct0 + t) * 16 + r;
      const float v = c < C ? zb[(size_t)nc * C + c] : (c == C ? ab[nc] : 0.f);
      a[t] = in ? v : 0.f;
    }
#pragma unroll
    for (int t = 0; t < WT; ++t) acc[t] = mfma16(a[t], b, acc[t]);
  };
  int nb = 0;
  for (; nb + 16 <= N; nb += 16) {
    step(nb); step(nb + 4); step(nb + 8); step(nb + 12);
  }
  for (; nb < N; nb += 4) step(nb);
  const int k = k0 + r;
  if (k < K) {
#pragma unroll
    for (int t = 0; t < WT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = (ct0 + t) * 16 + kq * 4 + e;
        if (c < C) dWt[((size_t)h * C + c) * K + k] = acc[t][e];
        else if (c == C) dbt[(size_t)h * K + k] = acc[t][e];
      }
  }
}

// --------------------------------------------------------------------------------------------
// Backward pass (frozen features: no dX), same ownership as the forward pass, pixels in the opposite order.
// dz [H][N][C], sn [H][N].  Per block: pgrad [blk][ld]: H rows of C dWa partials, then H dba partials (ld = H C + 4).
// --------------------------------------------------------------------------------------------
template <typename T, int NVL, bool TRAIN>
__global__ __launch_bounds__(256, 2) void mh_bwd_main_kernel(const T* __restrict__ X, const float* __restrict__ att,
                                                             const float* __restrict__ dz, const float* __restrict__ snp,
                                                             float* __restrict__ pgrad,
                                                             int N, int P, int S, int C, int H, int act,
                                                             float inv_keep, uint32_t thresh, uint64_t seed,
                                                             uint64_t offset, M1Gather g) {
  constexpr int EPV = Vec<T>::EPV, EL = NVL * EPV, CP = 64 * EL;
  // the image's H rows of dz wait in LDS (zero beyond C and H); the merge of the dWa rows reuses the space after the loop
  __shared__ __attribute__((aligned(16))) float sm_dz[HMAX * CP];
  __shared__ float sm_stat[4][HMAX];
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset, k0, k1);
  const int blk = blockIdx.x, n = blk / S, s = blk % S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int p_begin, p_end;
  m1_pix_range(s, P, S, p_begin, p_end);
  const int nvec = C / EPV;
  const float invP = 1.0f / (float)P;
  // this wave's pixels p_begin + wave + 4 i, i = cnt - 1 .. 0
  const int cnt = p_begin + wave < p_end ? (p_end - p_begin - wave + 3) / 4 : 0;
  const T* xim = X + (size_t)m1_src_image(n, g) * P * C;
  uint4 nxt[NVL];
  if (cnt > 0) {
    const int p = p_begin + wave + 4 * (cnt - 1);
    row_load<T, NVL>(nxt, xim + (size_t)p * C, lane, nvec);
  }
  float sn[HMAX];   // G[h,n,:] . bt[h,:], the bias' share of dA (mh_dz_kernel)
#pragma unroll
  for (int h = 0; h < HMAX; ++h) sn[h] = h < H ? snp[(size_t)h * N + n] : 0.f;
  for (int i = threadIdx.x; i < HMAX * CP; i += 256) {
    const int h = i / CP, c = i - h * CP;
    sm_dz[i] = (h < H && c < C) ? dz[((size_t)h * N + n) * C + c] : 0.f;
  }
  __syncthreads();
  float dwa[HMAX][EL];
#pragma unroll
  for (int h = 0; h < HMAX; ++h)
#pragma unroll
    for (int i = 0; i < EL; ++i) dwa[h][i] = 0.f;
  float dba[HMAX] = {0.f, 0.f, 0.f, 0.f};
  for (int it = cnt - 1; it >= 0; --it) {
    const int p = p_begin + wave + 4 * it;
    float x[EL];
#pragma unroll
    for (int j = 0; j < NVL; ++j) Vec<T>::unpack(nxt[j], x + j * EPV);
    if (it > 0) {   // the next row travels while this one is consumed
      row_load<T, NVL>(nxt, xim + (size_t)(p - 4) * C, lane, nvec);
    }
    uint32_t bits = 0xFFFFFFFFu;
    if (TRAIN) bits = row_keep_bits<RngLib, NVL, EPV>(((uint64_t)n * P + p) * C, lane, nvec, k0, k1, thresh);
#pragma unroll
    for (int h = 0; h < HMAX; ++h) {
      if (h < H) {
        float d = 0.f;   // row_dot over the kept elements, inline: as a routine it spills (profiles/rowpass_summary.md)
#pragma unroll
        for (int j = 0; j < NVL; ++j) {
#pragma unroll
          for (int e = 0; e < EPV; e += 4) {
            const float4 g4 = *reinterpret_cast<const float4*>(sm_dz + h * CP + (j * 64 + lane) * EPV + e);
            const int i = j * EPV + e;
            d = fmaf((bits >> i) & 1u ? x[i] : 0.f, g4.x, d);
            d = fmaf((bits >> (i + 1)) & 1u ? x[i + 1] : 0.f, g4.y, d);
            d = fmaf((bits >> (i + 2)) & 1u ? x[i + 2] : 0.f, g4.z, d);
            d = fmaf((bits >> (i + 3)) & 1u ? x[i + 3] : 0.f, g4.w, d);
          }
        }
        float tot = wave_sum(d);
        if (TRAIN) tot *= inv_keep;
        const float dA = (tot + sn[h]) * invP;
        // the relu gate from the saved map: A = max(Z, 0) > 0 exactly where Z > 0
        const float gz = (act == M1_ACT_RELU && !(att[((size_t)h * N + n) * P + p] > 0.f)) ? 0.f : dA;
        dba[h] += gz;
#pragma unroll
        for (int i = 0; i < EL; ++i) dwa[h][i] = fmaf(gz, x[i], dwa[h][i]);
      }
    }
  }
  const size_t ld = (size_t)H * C + 4;
  float* pg = pgrad + (size_t)blk * ld;
#pragma unroll
  for (int h = 0; h < HMAX; ++h)
    if (h < H) row_merge4<NVL, EPV>(dwa[h], sm_dz, pg + (size_t)h * C, wave, lane, nvec);
  if (lane == 0) {
#pragma unroll
    for (int h = 0; h < HMAX; ++h) sm_stat[wave][h] = dba[h];
  }
  __syncthreads();
  if ((int)threadIdx.x < HMAX) {
    const int h = threadIdx.x;
    pg[(size_t)H * C + h] = row_stat_merge4(sm_stat, h);   // (h >= H: zeros)
  }
}

// --------------------------------------------------------------------------------------------
// Evaluation scores.  grid N blocks of 256 threads; wave h < H takes row (h, n): probs, pred and, with labels, the
// row's loss; then the block forms the late-fusion row ((p_0 + p_1) + p_2 ...) / H and wave 0 its first maximal index.
// hs: rows between two heads of logits / probs / pred.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mh_scores_kernel(const float* __restrict__ logits,
                                                        const int64_t* __restrict__ labels, float* __restrict__ loss,
                                                        float* __restrict__ probs, int64_t* __restrict__ pred,
                                                        float* __restrict__ fused_probs, int64_t* __restrict__ fused_pred,
                                                        int H, int N, int K, size_t hs, int kind) {
  const int n = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < H) {
    const int h = wave;
    const float* row = logits + ((size_t)h * hs + n) * K;
    float* prow = probs + ((size_t)h * hs + n) * K;
    int cand = 0;
    if (kind == APA_SCORES_SOFTMAX) {
      const float lv = mh_softmax_row(row, K, labels ? (int)labels[n] : -1, prow, nullptr, 0.f, &cand);
      if (lane == 0 && loss) loss[(size_t)h * (1 + N) + 1 + n] = lv;
    } else {
      cand = wave_first_max<true>(row, K, lane, prow);
    }
    if (lane == 0) pred[(size_t)h * hs + n] = cand;
  }
  if (!fused_probs) return;
  __syncthreads();   // the block's own global stores are visible to it behind the barrier
  const float invH = 1.0f / (float)H;
  for (int k = threadIdx.x; k < K; k += 256) {
    float a = probs[((size_t)0 * hs + n) * K + k];
    for (int h = 1; h < H; ++h) a += probs[((size_t)h * hs + n) * K + k];
    fused_probs[(size_t)n * K + k] = a * invH;
  }
  if (!fused_pred) return;
  __syncthreads();
  if (wave == 0) {
    const int cand = wave_first_max<false>(fused_probs + (size_t)n * K, K, lane, nullptr);
    if (lane == 0) fused_pred[n] = cand;
  }
}

// apa_momentum_sgd_step's update (apa_optim.hip: momentum_sgd_kernel), head as grid.z: segment sg of head h is row h of
// the stacked tensor w[sg], its gradient and accumulator sit at flat offset off[sg] + h * n.
struct HeadSegs {
  float* w[APA_SGD_MAX_SEGMENTS];
  unsigned long long off[APA_SGD_MAX_SEGMENTS + 1];
  float wd[APA_SGD_MAX_SEGMENTS][HMAX];
  float lr[HMAX], momentum[HMAX];
};
__global__ __launch_bounds__(256) void mh_momentum_sgd_kernel(HeadSegs s, const float* __restrict__ grad,
                                                              float* __restrict__ acc, int H, float gscale) {
  const int sg = blockIdx.y, h = blockIdx.z;
  const size_t n = (s.off[sg + 1] - s.off[sg]) / (size_t)H, o = s.off[sg] + (size_t)h * n;
  float* __restrict__ w = s.w[sg] + (size_t)h * n;
  const float* __restrict__ g = grad + o;
  float* __restrict__ a = acc + o;
  const float wd = s.wd[sg][h], lr = s.lr[h], momentum = s.momentum[h];
  const size_t nv = n / 4;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (size_t)gridDim.x * 256) {
    f4u wv = *reinterpret_cast<const f4u*>(w + v * 4);
    const f4u gv = *reinterpret_cast<const f4u*>(g + v * 4);
    f4u av = *reinterpret_cast<const f4u*>(a + v * 4);
    momentum_sgd_update4(av, wv, gv, wd, lr, momentum, gscale);
    *reinterpret_cast<f4u*>(a + v * 4) = av;
    *reinterpret_cast<f4u*>(w + v * 4) = wv;
  }
  if (blockIdx.x == 0) {
    for (size_t i = nv * 4 + threadIdx.x; i < n; i += 256) {
      momentum_sgd_update(a[i], w[i], g[i], wd, lr, momentum, gscale);
    }
  }
}

// ============================================================================================
// host
// ============================================================================================
struct MhPlan {
  int S, nblk;
  size_t off_pacc, off_pstat, off_pgrad, off_dz, off_labels, off_sn, total;
};
MhPlan mh_plan(int H, int N, int P, int C) {
  MhPlan pl;
  int S = (512 + N / 2) / N;
  if (S < 1) S = 1;
  int maxS = P >= 8 ? P / 4 : 1;
  if (maxS > 256) maxS = 256;
  if (S > maxS) S = maxS;
  pl.S = S;
  pl.nblk = N * S;
  size_t off = 0;
  pl.off_pacc = off;   off += align_up((size_t)pl.nblk * H * C * 4, 256);
  pl.off_pstat = off;  off += align_up((size_t)pl.nblk * 4 * 4, 256);
  pl.off_pgrad = off;  off += align_up((size_t)pl.nblk * ((size_t)H * C + 4) * 4, 256);
  pl.off_dz = off;     off += align_up((size_t)H * N * C * 4, 256);
  pl.off_labels = off; off += align_up((size_t)N * 8, 256);
  pl.off_sn = off;     off += align_up((size_t)H * N * 4, 256);
  pl.total = off;
  return pl;
}

// One step's arguments, as both steps and both epoch drivers describe them
struct MhStep {
  const char* who;
  const apa_feature_cache* cache; const apa_multihead* heads;
  const void* X; const int64_t* labels;
  float *logits, *att, *zsave, *abar, *loss, *G, *dWa, *dba, *dWt, *dbt;   // train: all; eval: the first five
  float* probs; int64_t* pred; float* fused_probs; int64_t* fused_pred;    // eval
  void* ws; size_t ws_bytes;
  int N, P, C, K; unsigned flags; float keep_prob; uint64_t seed, offset; int dtype;
  bool train; int scores_kind; float loss_wt, grad_scale;
  size_t hs;   // rows between two heads of the per-row outputs
  Hooks hk;
};

#define MH_REFUSE(code, ...) do { set_error(__VA_ARGS__); return code; } while (0)

int mh_check_heads(const char* who, int H) {
  if (H < 1 || H > APA_HEADS_MAX)
    MH_REFUSE(APA_ERR_INVALID_ARG, "%s: H = %d outside 1 .. APA_HEADS_MAX (%d)", who, H, APA_HEADS_MAX);
  return APA_OK;
}

// rules 1 .. 8 of the header, in its order; `index`: the index (a step) or the order (an epoch).  epoch_rule(need): what
// an epoch checks behind rules 1 and 2 and in front of the rest (H, its count rule, the optimiser's checks), with cache,
// heads and index at hand; need: workspace bytes it asks for beyond the step's own plan.  A step has none.
template <typename Rule>
int mh_check(const MhStep& a, const int32_t* index, const char* index_name, Rule&& epoch_rule) {
  const char* who = a.who;
  if (!a.cache) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: cache is NULL", who);
  if (!a.heads) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: heads is NULL", who);
  if (!index) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: %s is NULL", who, index_name);
  const apa_multihead& hd = *a.heads;
  size_t ws_need_extra = 0;
  if (const int rc = epoch_rule(ws_need_extra)) return rc;
  const struct { const void* p; const char* name; bool need; } ptrs[] = {
      {hd.Wa, "heads->Wa", true}, {hd.ba, "heads->ba", true}, {hd.Wt, "heads->Wt", true}, {hd.bt, "heads->bt", true},
      {a.X, "X", true}, {a.labels, "labels", a.train || a.loss != nullptr}, {a.logits, "logits", true},
      {a.att, "att", true}, {a.zsave, "zsave", true}, {a.abar, "abar", true}, {a.loss, "loss", a.train || a.labels != nullptr},
      {a.G, "G", a.train}, {a.dWa, "dWa", a.train}, {a.dba, "dba", a.train}, {a.dWt, "dWt", a.train},
      {a.dbt, "dbt", a.train}, {a.probs, "probs", !a.train}, {a.pred, "pred", !a.train},
      {a.fused_probs, "fused_probs", !a.train && a.fused_pred != nullptr}, {a.ws, "ws", true}};
  for (const auto& q : ptrs)
    if (q.need && !q.p) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: %s is NULL", who, q.name);
  if (const int rc = mh_check_heads(who, hd.H)) return rc;
  if (a.N < 1 || a.P < 1 || a.C < 1 || a.K < 1 || a.cache->cache_images < 1)
    MH_REFUSE(APA_ERR_INVALID_ARG, "%s: non-positive size (N=%d P=%d C=%d K=%d cache_images=%d)", who, a.N, a.P, a.C, a.K,
              a.cache->cache_images);
  if (!a.train && a.scores_kind != APA_SCORES_SOFTMAX && a.scores_kind != APA_SCORES_SIGMOID)
    MH_REFUSE(APA_ERR_INVALID_ARG, "%s: unknown scores_kind %d", who, a.scores_kind);
  if (!a.train && a.scores_kind == APA_SCORES_SIGMOID && a.labels)
    MH_REFUSE(APA_ERR_INVALID_ARG, "%s: the sigmoid scores take no labels / loss", who);
  {
    const int dt = a.dtype == APA_DTYPE_BF16 ? APA_DTYPE_BF16 : APA_DTYPE_F32;   // (the dtype rule comes sixth)
    if (m1r_vectors_per_lane(a.C, dt) == 0)
      MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: C = %d is not served (whole 16-byte vectors, C <= 2048)", who, a.C);
  }
  const MhPlan pl = mh_plan(hd.H, a.N, a.P, a.C);
  if (!m1_pix_range_ok(a.P, pl.S) || (size_t)a.N * a.P >= (1ull << 31))
    MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: N * P = %zu pixels are not served", who, (size_t)a.N * a.P);
  if (a.train && !(a.flags & APA_FLAG_FROZEN_INPUT))
    MH_REFUSE(APA_ERR_INVALID_ARG, "%s: a cache has no gradient: training needs APA_FLAG_FROZEN_INPUT", who);
  if (a.flags & APA_FLAG_SOFTMAX_ATT) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: APA_FLAG_SOFTMAX_ATT is not served", who);
  if (a.flags & APA_FLAG_RELU_INPUT) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: APA_FLAG_RELU_INPUT is not served", who);
  if (a.flags & APA_FLAG_RNG_EXTERNAL) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: APA_FLAG_RNG_EXTERNAL is not served", who);
  if (a.flags & APA_FLAG_RNG_DEVICE) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: APA_FLAG_RNG_DEVICE is not served", who);
  if (a.dtype == APA_DTYPE_FP8_E4M3)
    MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: FP8 caches are not served (the FP8 arm hashes per pair of elements)", who);
  if (a.dtype != APA_DTYPE_F32 && a.dtype != APA_DTYPE_BF16) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: unknown dtype %d", who, a.dtype);
  if (a.train && (a.flags & APA_FLAG_TRAIN) && !(a.keep_prob > 0.f && a.keep_prob <= 1.f))
    MH_REFUSE(APA_ERR_INVALID_ARG, "%s: keep_prob %g outside (0, 1]", who, (double)a.keep_prob);
  const size_t need = pl.total > ws_need_extra ? pl.total : ws_need_extra;
  if (a.ws_bytes < need) MH_REFUSE(APA_ERR_WORKSPACE, "%s: ws_bytes %zu < %zu", who, a.ws_bytes, need);
  const auto mis = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) != 0; };
  if (mis(a.X, 16)) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: X must be 16-byte aligned", who);
  if (mis(a.ws, 16)) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: ws must be 16-byte aligned", who);
  if (mis(a.zsave, 16)) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: zsave must be 16-byte aligned", who);
  if (mis(index, 4)) MH_REFUSE(APA_ERR_UNSUPPORTED, "%s: %s must be 4-byte aligned", who, index_name);
  return APA_OK;
}

// what both streaming passes of a step are launched with
struct MhPass { bool drop; int act; float inv_keep; uint32_t thresh; M1Gather g; };

template <typename T, int NVL>
void mh_launch_fwd(const MhStep& a, const MhPlan& pl, const MhPass& ps, hipStream_t st) {
  char* w = static_cast<char*>(a.ws);
  float* pacc = reinterpret_cast<float*>(w + pl.off_pacc);
  float* pstat = reinterpret_cast<float*>(w + pl.off_pstat);
  auto go = [&](auto kernel) {
    launch_ev(kernel, dim3(pl.nblk), dim3(256), 0, st, a.hk.fwd0, a.hk.fwd1, static_cast<const T*>(a.X), a.heads->Wa,
              a.heads->ba, a.att, pacc, pstat, a.N, a.P, pl.S, a.C, a.heads->H, ps.act, ps.inv_keep, ps.thresh, a.seed,
              a.offset, ps.g);
  };
  if (ps.drop) go(mh_pool_fwd_kernel<T, NVL, true>); else go(mh_pool_fwd_kernel<T, NVL, false>);
}

template <typename T, int NVL>
void mh_launch_bwd(const MhStep& a, const MhPlan& pl, const MhPass& ps, hipStream_t st) {
  char* w = static_cast<char*>(a.ws);
  auto go = [&](auto kernel) {
    launch_ev(kernel, dim3(pl.nblk), dim3(256), 0, st, a.hk.bwd0, a.hk.bwd1, static_cast<const T*>(a.X),
              static_cast<const float*>(a.att), reinterpret_cast<const float*>(w + pl.off_dz),
              reinterpret_cast<const float*>(w + pl.off_sn), reinterpret_cast<float*>(w + pl.off_pgrad), a.N, a.P, pl.S, a.C,
              a.heads->H, ps.act, ps.inv_keep, ps.thresh, a.seed, a.offset, ps.g);
  };
  if (ps.drop) go(mh_bwd_main_kernel<T, NVL, true>); else go(mh_bwd_main_kernel<T, NVL, false>);
}

// the launches of one step; everything was checked
int mh_run(const MhStep& a, const int32_t* index, hipStream_t st) {
  const apa_multihead& hd = *a.heads;
  const int H = hd.H, N = a.N, P = a.P, C = a.C, K = a.K;
  const MhPlan pl = mh_plan(H, N, P, C);
  char* w = static_cast<char*>(a.ws);
  MhPass ps;
  ps.drop = a.train && (a.flags & APA_FLAG_TRAIN);
  ps.act = (a.flags & APA_FLAG_RELU_ATT) ? M1_ACT_RELU : M1_ACT_ID;
  ps.inv_keep = ps.drop ? 1.0f / a.keep_prob : 1.0f;
  ps.thresh = ps.drop ? keep_thresh(a.keep_prob) : 0u;
  ps.g.index = index; ps.g.T = a.cache->cache_images; ps.g.status = a.cache->status;
  const int64_t* labels = a.labels;
  ps.g.labels = nullptr; ps.g.labels_out = nullptr;
  if (a.cache->labels_cached && a.labels) {
    ps.g.labels = a.labels;
    ps.g.labels_out = reinterpret_cast<int64_t*>(w + pl.off_labels);
    labels = ps.g.labels_out;
  }
  row_instance(C, a.dtype, [&](auto t, auto nvl) { mh_launch_fwd<decltype(t), decltype(nvl)::value>(a, pl, ps, st); });
  APA_LAUNCH_CHECK("mh_pool_fwd_kernel");
  hipLaunchKernelGGL(mh_finalize_fwd_kernel, dim3(N, (C / 4 + 255) / 256, H), dim3(256), 0, st,
                     reinterpret_cast<const float*>(w + pl.off_pacc), reinterpret_cast<const float*>(w + pl.off_pstat), N, P,
                     pl.S, C, H, a.zsave, a.abar);
  APA_LAUNCH_CHECK("mh_finalize_fwd_kernel");
  {   // image tiles per wave: two up to 32 images, four beyond (Wt is re-read once per group of tiles)
    const float* zs = a.zsave; const float* ab = a.abar;
    if (N <= 32)
      hipLaunchKernelGGL(mh_logits_kernel<2>, dim3((K + 15) / 16, (N + 31) / 32, H), dim3(64 * LW), 0, st, zs, hd.Wt, ab,
                         hd.bt, a.logits, N, C, K, a.hs);
    else
      hipLaunchKernelGGL(mh_logits_kernel<4>, dim3((K + 15) / 16, (N + 63) / 64, H), dim3(64 * LW), 0, st, zs, hd.Wt, ab,
                         hd.bt, a.logits, N, C, K, a.hs);
  }
  APA_LAUNCH_CHECK("mh_logits_kernel");
  if (!a.train) {
    hipLaunchKernelGGL(mh_scores_kernel, dim3(N), dim3(256), 0, st, static_cast<const float*>(a.logits), labels, a.loss,
                       a.probs, a.pred, a.fused_probs, a.fused_pred, H, N, K, a.hs, a.scores_kind);
    APA_LAUNCH_CHECK("mh_scores_kernel");
    if (a.loss) {
      hipLaunchKernelGGL(mh_loss_mean_kernel, dim3(H), dim3(256), 0, st, a.loss, N, 1.0f / (float)N);
      APA_LAUNCH_CHECK("mh_loss_mean_kernel");
    }
    return APA_OK;
  }
  const float lscale = a.loss_wt / (float)N, gscale = a.loss_wt * a.grad_scale / (float)N;
  hipLaunchKernelGGL(mh_xent_kernel, dim3((H * N + 3) / 4), dim3(256), 0, st, static_cast<const float*>(a.logits), labels,
                     a.loss, a.G, H, N, K, gscale);
  APA_LAUNCH_CHECK("mh_xent_kernel");
  hipLaunchKernelGGL(mh_loss_mean_kernel, dim3(H), dim3(256), 0, st, a.loss, N, lscale);
  APA_LAUNCH_CHECK("mh_loss_mean_kernel");
  {
    const float* Gc = a.G;
    float* dzp = reinterpret_cast<float*>(w + pl.off_dz);
    float* snp = reinterpret_cast<float*>(w + pl.off_sn);
    if (N <= 32)
      hipLaunchKernelGGL(mh_dz_kernel<2>, dim3((C + 63) / 64, (N + 31) / 32, H), dim3(256), 0, st, Gc, hd.Wt, hd.bt, dzp,
                         snp, N, C, K);
    else
      hipLaunchKernelGGL(mh_dz_kernel<4>, dim3((C + 63) / 64, (N + 63) / 64, H), dim3(256), 0, st, Gc, hd.Wt, hd.bt, dzp,
                         snp, N, C, K);
  }
  APA_LAUNCH_CHECK("mh_dz_kernel");
  hipLaunchKernelGGL(mh_dwt_kernel, dim3((K + 15) / 16, (C / 16 + 1 + 4 * WT - 1) / (4 * WT), H), dim3(256), 0, st,
                     static_cast<const float*>(a.zsave), static_cast<const float*>(a.abar), static_cast<const float*>(a.G),
                     a.dWt, a.dbt, N, C, K);
  APA_LAUNCH_CHECK("mh_dwt_kernel");
  row_instance(C, a.dtype, [&](auto t, auto nvl) { mh_launch_bwd<decltype(t), decltype(nvl)::value>(a, pl, ps, st); });
  APA_LAUNCH_CHECK("mh_bwd_main_kernel");
  ColsumArgs cs;   // [nblk][H C + 4]: the H dWa rows, then the H dba partials as a second section
  cs.pdwa = reinterpret_cast<const float*>(w + pl.off_pgrad);
  cs.nblk = pl.nblk; cs.C = H * C + H; cs.ld = H * C + 4;
  cs.dwa = a.dWa; cs.dwa2 = a.dba; cs.C1 = H * C;
  return m1_colsum(cs, st);
}

int sgd_heads_check(const char* who, int H, int nseg, float* const* weights, const size_t* sizes, const float* weight_decay,
                    const float* grad_flat, float* acc_flat, const float* lr, const float* momentum) {
  if (const int rc = mh_check_heads(who, H)) return rc;
  if (nseg <= 0 || nseg > APA_SGD_MAX_SEGMENTS || !weights || !sizes || !weight_decay || !grad_flat || !acc_flat || !lr ||
      !momentum)
    MH_REFUSE(APA_ERR_INVALID_ARG, "%s: bad arguments (nseg=%d, max %d)", who, nseg, APA_SGD_MAX_SEGMENTS);
  for (int i = 0; i < nseg; ++i)
    if (!weights[i]) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: weights[%d] is NULL", who, i);
  return APA_OK;
}

int sgd_heads_run(int H, int nseg, float* const* weights, const size_t* sizes, const float* weight_decay,
                  const float* grad_flat, float* acc_flat, const float* lr, const float* momentum, float grad_scale,
                  hipStream_t st) {
  HeadSegs s;
  size_t o = 0, biggest = 0;
  for (int i = 0; i < nseg; ++i) {
    s.w[i] = weights[i];
    s.off[i] = o;
    for (int h = 0; h < HMAX; ++h) s.wd[i][h] = h < H ? weight_decay[(size_t)i * H + h] : 0.f;
    o += sizes[i] * (size_t)H;
    if (sizes[i] > biggest) biggest = sizes[i];
  }
  for (int i = nseg; i <= APA_SGD_MAX_SEGMENTS; ++i) s.off[i] = o;
  for (int i = nseg; i < APA_SGD_MAX_SEGMENTS; ++i) {
    s.w[i] = nullptr;
    for (int h = 0; h < HMAX; ++h) s.wd[i][h] = 0.f;
  }
  for (int h = 0; h < HMAX; ++h) {
    s.lr[h] = h < H ? lr[h] : 0.f;
    s.momentum[h] = h < H ? momentum[h] : 0.f;
  }
  if (o == 0) return APA_OK;
  size_t nbx = (biggest / 4 + 255) / 256;
  if (nbx < 1) nbx = 1;
  if (nbx > 1024) nbx = 1024;
  hipLaunchKernelGGL(mh_momentum_sgd_kernel, dim3((unsigned)nbx, (unsigned)nseg, (unsigned)H), dim3(256), 0, st, s,
                     grad_flat, acc_flat, H, grad_scale);
  APA_LAUNCH_CHECK("mh_momentum_sgd_kernel");
  return APA_OK;
}

}  // namespace
}  // namespace apa

using namespace apa;

extern "C" size_t apa_multihead_workspace_bytes(int H, int N, int P, int C, int K) {
  if (H < 1 || H > APA_HEADS_MAX || N < 1 || P < 1 || C < 1 || K < 1) return 0;
  return mh_plan(H, N, P, C).total;
}

namespace {
// A direction's flat argument list as the step it describes (hs = N: an evaluation epoch spaces its heads wider)
MhStep mh_train_args(const char* who, const apa_feature_cache* cache, const apa_hooks* hooks, const apa_multihead*
                     heads, const void* X, const int64_t* labels, float loss_wt, float grad_scale, float* logits, float*
                     att, float* zsave, float* abar, float* loss, float* G, float* dWa, float* dba, float* dWt, float*
                     dbt, void* ws, size_t ws_bytes, int N, int P, int C, int K, unsigned flags, float keep_prob,
                     uint64_t seed, uint64_t offset, int dtype) {
  MhStep a = {};
  a.who = who;
  a.cache = cache; a.heads = heads; a.X = X; a.labels = labels;
  a.logits = logits; a.att = att; a.zsave = zsave; a.abar = abar; a.loss = loss; a.G = G;
  a.dWa = dWa; a.dba = dba; a.dWt = dWt; a.dbt = dbt; a.ws = ws; a.ws_bytes = ws_bytes;
  a.N = N; a.P = P; a.C = C; a.K = K; a.flags = flags; a.keep_prob = keep_prob; a.seed = seed; a.offset = offset;
  a.dtype = dtype; a.train = true; a.loss_wt = loss_wt; a.grad_scale = grad_scale; a.hs = (size_t)(N > 0 ? N : 0);
  a.hk = Hooks(hooks);
  return a;
}

MhStep mh_eval_args(const char* who, const apa_feature_cache* cache, const apa_multihead* heads, int scores_kind, const
                    void* X, const int64_t* labels, float* logits, float* att, float* zsave, float* abar, float* loss,
                    float* probs, int64_t* pred, float* fused_probs, int64_t* fused_pred, void* ws, size_t ws_bytes, int
                    N, int P, int C, int K, unsigned flags, int dtype) {
  MhStep a = {};
  a.who = who;
  a.cache = cache; a.heads = heads; a.X = X; a.labels = labels;
  a.logits = logits; a.att = att; a.zsave = zsave; a.abar = abar; a.loss = loss;
  a.probs = probs; a.pred = pred; a.fused_probs = fused_probs; a.fused_pred = fused_pred;
  a.ws = ws; a.ws_bytes = ws_bytes; a.N = N; a.P = P; a.C = C; a.K = K; a.flags = flags & ~APA_FLAG_TRAIN;
  a.keep_prob = 1.f; a.dtype = dtype; a.train = false; a.scores_kind = scores_kind; a.hs = (size_t)(N > 0 ? N : 0);
  return a;
}

int mh_step(const MhStep& a, void* stream) {
  const int32_t* index = a.cache ? a.cache->index : nullptr;
  const int rc = mh_check(a, index, "cache->index", [](size_t&) { return APA_OK; });
  return rc != APA_OK ? rc : mh_run(a, index, static_cast<hipStream_t>(stream));
}
}  // namespace

extern "C" int apa_multihead_train_step_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const
                                               apa_multihead* heads, const void* X, const int64_t* labels, float
                                               loss_wt, float grad_scale, float* logits, float* att, float* zsave,
                                               float* abar, float* loss, float* G, float* dWa, float* dba, float* dWt,
                                               float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int K,
                                               unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int
                                               dtype, void* stream) {
  return mh_step(mh_train_args("apa_multihead_train_step_cached", cache, hooks, heads, X, labels, loss_wt, grad_scale,
                               logits, att, zsave, abar, loss, G, dWa, dba, dWt, dbt, ws, ws_bytes, N, P, C, K, flags,
                               keep_prob, seed, offset, dtype), stream);
}

extern "C" int apa_multihead_eval_step_cached(const apa_feature_cache* cache, const apa_multihead* heads, int
                                              scores_kind, const void* X, const int64_t* labels, float* logits, float*
                                              att, float* zsave, float* abar, float* loss, float* probs, int64_t* pred,
                                              float* fused_probs, int64_t* fused_pred, void* ws, size_t ws_bytes, int N,
                                              int P, int C, int K, unsigned flags, int dtype, void* stream) {
  return mh_step(mh_eval_args("apa_multihead_eval_step_cached", cache, heads, scores_kind, X, labels, logits, att,
                              zsave, abar, loss, probs, pred, fused_probs, fused_pred, ws, ws_bytes, N, P, C, K, flags,
                              dtype), stream);
}

extern "C" int apa_momentum_sgd_step_heads(int H, int nseg, float* const* weights, const size_t* sizes,
                                           const float* weight_decay, const float* grad_flat, float* acc_flat,
                                           const float* lr, const float* momentum, float grad_scale, void* stream) {
  const int rc = sgd_heads_check("apa_momentum_sgd_step_heads", H, nseg, weights, sizes, weight_decay, grad_flat, acc_flat,
                                 lr, momentum);
  if (rc != APA_OK) return rc;
  return sgd_heads_run(H, nseg, weights, sizes, weight_decay, grad_flat, acc_flat, lr, momentum, grad_scale,
                       static_cast<hipStream_t>(stream));
}

extern "C" int apa_multihead_train_epoch_cached(const apa_epoch* ep, const apa_multihead_sgd* opt, const
                                                apa_feature_cache* cache, const apa_hooks* hooks, const apa_multihead*
                                                heads, const void* X, const int64_t* labels, float loss_wt, float
                                                grad_scale, float* logits, float* att, float* zsave, float* abar, float*
                                                loss, float* G, float* dWa, float* dba, float* dWt, float* dbt, void*
                                                ws, size_t ws_bytes, int N, int P, int C, int K, unsigned flags, float
                                                keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  const char* who = "apa_multihead_train_epoch_cached";
  if (!ep) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: ep is NULL", who);
  if (!opt) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: opt is NULL", who);
  if (!opt->lr) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: opt->lr is NULL", who);
  const MhStep a = mh_train_args(who, cache, hooks, heads, X, labels, loss_wt, grad_scale, logits, att, zsave, abar,
                                 loss, G, dWa, dba, dWt, dbt, ws, ws_bytes, N, P, C, K, flags, keep_prob, seed, offset,
                                 dtype);
  // rules 1 and 2, then the count rule in the place of rule 3's sizes and the optimiser's checks, then the rest
  int rc = mh_check(a, ep->order, "ep->order", [&](size_t&) -> int {
    if (const int r = mh_check_heads(who, heads->H)) return r;
    if (N < 1 || ep->count < N || ep->count % N != 0)
      MH_REFUSE(APA_ERR_INVALID_ARG, "%s: count = %d is not a positive multiple of N = %d", who, ep->count, N);
    return sgd_heads_check(who, heads->H, opt->nseg, opt->weights, opt->sizes, opt->weight_decay, opt->grad_flat,
                           opt->acc_flat, opt->lr, opt->momentum);
  });
  if (rc != APA_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int steps = ep->count / N, H = heads->H;
  for (int s = 0; s < steps; ++s) {
    MhStep b = a;
    b.offset = offset + (uint64_t)s;
    b.loss = loss + (size_t)s * H * (1 + N);
    if (!cache->labels_cached) b.labels = labels + (size_t)s * N;
    if ((rc = mh_run(b, ep->order + (size_t)s * N, st)) != APA_OK) return rc;
    if ((rc = sgd_heads_run(H, opt->nseg, opt->weights, opt->sizes, opt->weight_decay, opt->grad_flat, opt->acc_flat,
                            opt->lr + (size_t)s * H, opt->momentum, opt->grad_scale, st)) != APA_OK)
      return rc;
  }
  return APA_OK;
}

extern "C" int apa_multihead_eval_epoch_cached(const apa_epoch* ep, const apa_feature_cache* cache, const apa_multihead*
                                               heads, int scores_kind, const void* X, const int64_t* labels, float*
                                               logits, float* att, float* zsave, float* abar, float* loss, float* probs,
                                               int64_t* pred, float* fused_probs, int64_t* fused_pred, void* ws, size_t
                                               ws_bytes, int N, int P, int C, int K, unsigned flags, int dtype, void*
                                               stream) {
  const char* who = "apa_multihead_eval_epoch_cached";
  if (!ep) MH_REFUSE(APA_ERR_INVALID_ARG, "%s: ep is NULL", who);
  MhStep a = mh_eval_args(who, cache, heads, scores_kind, X, labels, logits, att, zsave, abar, loss, probs, pred,
                          fused_probs, fused_pred, ws, ws_bytes, N, P, C, K, flags, dtype);
  int steps = 0, last = 0;
  int rc = mh_check(a, ep->order, "ep->order", [&](size_t& need) -> int {
    if (const int r = mh_check_heads(who, heads->H)) return r;
    if (N < 1 || ep->count < 1)
      MH_REFUSE(APA_ERR_INVALID_ARG, "%s: count = %d, N = %d: both must be positive", who, ep->count, N);
    steps = (ep->count + N - 1) / N;
    last = ep->count - (steps - 1) * N;
    // the smaller last batch runs in the same workspace: its plan is checked with the full batch's
    need = (P >= 1 && C >= 1) ? mh_plan(heads->H, last, P, C).total : 0;
    return APA_OK;
  });
  if (rc != APA_OK) return rc;
  a.hs = (size_t)ep->count;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int H = heads->H;
  for (int s = 0; s < steps; ++s) {
    MhStep b = a;
    const size_t r0 = (size_t)s * N;
    b.N = s == steps - 1 ? last : N;
    b.logits = logits + r0 * K;
    b.probs = probs + r0 * K;
    b.pred = pred + r0;
    if (fused_probs) b.fused_probs = fused_probs + r0 * K;
    if (fused_pred) b.fused_pred = fused_pred + r0;
    if (loss) b.loss = loss + (size_t)s * H * (1 + N);
    if (labels && !cache->labels_cached) b.labels = labels + r0;
    if ((rc = mh_run(b, ep->order + r0, st)) != APA_OK) return rc;
  }
  return APA_OK;
}
