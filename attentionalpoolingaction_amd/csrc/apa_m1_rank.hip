// apa_m1_rank.hip -- rank-R attentional pooling (NET.USE_POSE_PRELOGITS_BASED_ATTENTION_RANK > 1) with one bottom-up
// map, in ONE streaming pass over the features per direction.
//
// Reference semantics: models/slim/nets/nets_factory.py:247-328 with RANK = R.  Every further attention conv is a
// 1x1 conv on a ONE-channel map, i.e. a scalar affine map of the one before it:
//
//   Z_0 = Xatt . Wa + ba                Z_r = w_r Z_{r-1} + b_r   (r = 1 .. R-1)          A_r = f(Z_r), f = id | relu
//   z_r[n,:] = (1/P) sum_p A_r[n,p] Xt[n,p,:]      abar_r[n] = (1/P) sum_p A_r[n,p]       Xt = X * mask / keep
//   logits   = sum_r ( z_r . Wt_r + abar_r (x) bt_r )
//
//   dz_r = G . Wt_r^T        dA_r[n,p] = (Xt[n,p,:] . dz_r[n,:] + G[n,:] . bt_r) / P       dZ_r = dA_r [* (Z_r > 0)]
//   dZ~_r = dZ_r + w_{r+1} dZ~_{r+1}                dw_r = sum dZ~_r Z_{r-1}     db_r = sum dZ~_r   (r >= 1)
//   dX = (1/P) sum_r A_r dz_r * mask/keep + dZ~_0 (x) Wa        dWa = Xatt^T dZ~_0         dba = sum dZ~_0
//
// so a pixel's row of X is loaded once forward (Z_0, then R accumulator sets) and once backward (R dot products with
// dz_r, the gates from the saved Z_0, one dX row).  The per-block partials are merged in a fixed order by small
// kernels; nothing is accumulated with atomics, every run repeats bit for bit.  The chain gradients dw_r / db_r are
// summed directly (the kernel has Z_{r-1} and dZ~_r of its pixel at hand): 2 (R - 1) partials per block.
//
// One wave owns a pixel and keeps its row in registers (apa_rowpass.h: ownership, loader, dot, keep bits, merges):
// NVL * EPV = 8 elements per lane serve C <= 512, 32 elements C <= 2048 (the ResNet conv5 map: every lane busy).
// The forward pass keeps its R accumulator sets in registers and the attention weights in LDS; the backward pass keeps
// the image's R rows of dz and the attention weights in LDS, its dwa accumulators in registers: two blocks per CU.
// The small products (z_r . Wt_r, G . Wt_r^T, z_r^T . G) run through the existing M == 1 kernels, one launch per rank,
// on rank-major copies of z / dz in the workspace.
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"
#include "apa_rowpass.h"

namespace apa {

namespace {
constexpr int RMAX = APA_RANK_MAX;

struct ChainPtrs {   // by value to the kernels: the chain scalars live in separate one-float tensors
  const float* w[RMAX - 1];
  const float* b[RMAX - 1];
};
struct BtPtrs { const float* bt[RMAX]; };

// Z_r and A_r of one pixel from its Z_0: the ONE definition both passes use, so that the backward pass's relu gates
// are the forward pass's, bit for bit
__device__ __forceinline__ void rank_chain(float z0, const float* cw, const float* cb, int R, int act, float* Z,
                                           float* A) {
  Z[0] = z0;
#pragma unroll
  for (int r = 1; r < RMAX; ++r) Z[r] = r < R ? fmaf(cw[r - 1], Z[r - 1], cb[r - 1]) : 0.f;
#pragma unroll
  for (int r = 0; r < RMAX; ++r) A[r] = r < R ? (act == M1_ACT_RELU ? fmaxf(Z[r], 0.f) : Z[r]) : 0.f;
}

// --------------------------------------------------------------------------------------------
// Forward pass.  grid N * S blocks of 256 threads (m1_plan); block (n, s) owns pixels [p_begin, p_end) of image n,
// wave w the pixels p_begin + w, + 4, ...  Outputs: z0 [N,P] (FUSED; else it is an input), att [N,P,R], and per block
// pacc [blk][R][C] = sum_p A_r Xt, pstat [blk][4] = sum_p A_r.
// --------------------------------------------------------------------------------------------
template <typename T, int NVL, bool FUSED, bool TRAIN>
__global__ __launch_bounds__(256, 2) void m1r_pool_fwd_kernel(
    const T* __restrict__ X, const float* __restrict__ Wa, const float* __restrict__ ba, ChainPtrs ch,
    float* __restrict__ z0, float* __restrict__ att, float* __restrict__ pacc, float* __restrict__ pstat, int P, int S,
    int C, int R, int act, float inv_keep, uint32_t thresh, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev) {
  constexpr int EPV = Vec<T>::EPV, EL = NVL * EPV;
  __shared__ float sm[3 * EL * 64];
  __shared__ __attribute__((aligned(16))) float sm_wa[FUSED ? 64 * EL : 4];
  __shared__ float sm_stat[4][RMAX];
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev_x(seed, offset_dev ? *offset_dev : offset, thresh, k0, k1);
  const int blk = blockIdx.x, n = blk / S, s = blk % S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // 64-bit quotients: nothing on this path checks m1_pix_range_ok, which m1_pix_range's 32-bit form needs
  const int p_begin = (int)(((long)s * P) / S), p_end = (int)(((long)(s + 1) * P) / S);
  const int nvec = C / EPV;
  float cw[RMAX - 1], cb[RMAX - 1];
#pragma unroll
  for (int r = 0; r < RMAX - 1; ++r) {
    cw[r] = r < R - 1 ? ch.w[r][0] : 0.f;
    cb[r] = r < R - 1 ? ch.b[r][0] : 0.f;
  }
  const float bias = FUSED ? ba[0] : 0.f;
  float acc[RMAX][EL];
#pragma unroll
  for (int r = 0; r < RMAX; ++r)
#pragma unroll
    for (int i = 0; i < EL; ++i) acc[r][i] = 0.f;
  float asum[RMAX] = {0.f, 0.f, 0.f, 0.f};
  const T* xim = X + (size_t)n * P * C;
  uint4 nxt[NVL];
  if (p_begin + wave < p_end) {
    row_load<T, NVL>(nxt, xim + (size_t)(p_begin + wave) * C, lane, nvec);
  }
  // the attention weights wait in LDS (zero beyond C): the registers belong to the R accumulator sets.  Staged behind
  // the first row's loads, which travel meanwhile
  if (FUSED) {
    for (int c = threadIdx.x; c < 64 * EL; c += 256) sm_wa[c] = c < C ? Wa[c] : 0.f;
    __syncthreads();
  }
  for (int p = p_begin + wave; p < p_end; p += 4) {
    float x[EL];
#pragma unroll
    for (int j = 0; j < NVL; ++j) Vec<T>::unpack(nxt[j], x + j * EPV);
    if (p + 4 < p_end) {   // the next row travels while this one is consumed
      row_load<T, NVL>(nxt, xim + (size_t)(p + 4) * C, lane, nvec);
    }
    const size_t px = (size_t)n * P + p;
    float zl;
    if (FUSED) {
      const float d = row_dot<NVL, EPV>(x, sm_wa, lane);
      zl = wave_sum(d) + bias;
      if (lane == 0) z0[px] = zl;
    } else {
      zl = z0[px];
    }
    float Z[RMAX], A[RMAX];
    rank_chain(zl, cw, cb, R, act, Z, A);
    if (lane < R) att[px * R + lane] = lane == 0 ? A[0] : (lane == 1 ? A[1] : (lane == 2 ? A[2] : A[3]));
    if (TRAIN) {
      const uint32_t bits = row_keep_bits<RngAny, NVL, EPV>((uint64_t)px * C, lane, nvec, k0, k1, thresh);
#pragma unroll
      for (int i = 0; i < EL; ++i) x[i] = (bits >> i) & 1u ? x[i] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      if (r < R) {
        asum[r] += A[r];
        const float ak = TRAIN ? A[r] * inv_keep : A[r];
#pragma unroll
        for (int i = 0; i < EL; ++i) acc[r][i] = fmaf(ak, x[i], acc[r][i]);
      }
    }
  }
  // ---- combine the 4 waves (fixed order), one rank at a time ----
  float* pa = pacc + (size_t)blk * R * C;
#pragma unroll
  for (int r = 0; r < RMAX; ++r)
    if (r < R) row_merge4<NVL, EPV>(acc[r], sm, pa + (size_t)r * C, wave, lane, nvec);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RMAX; ++r) sm_stat[wave][r] = asum[r];
  }
  __syncthreads();
  if (threadIdx.x < RMAX) {
    const int r = threadIdx.x;
    pstat[blk * 4 + r] = row_stat_merge4(sm_stat, r);
  }
}

// --------------------------------------------------------------------------------------------
// Backward pass, same ownership.  dz [R][N][C] and sn [R][N] (or null: G . bt_r is formed here) are rank-major.
// Outputs: dX; FUSED: pdwa [blk][C], pdba [blk]; else dzatt [N,P] = dZ~_0 for the attention GEMV backward; and
// pchain [blk][8] = {dw_1, db_1, dw_2, db_2, dw_3, db_3, 0, 0}.
// --------------------------------------------------------------------------------------------
template <typename T, int NVL, bool FUSED, bool TRAIN>
__global__ __launch_bounds__(256) void m1r_bwd_main_kernel(
    const T* __restrict__ X, const float* __restrict__ Wa, ChainPtrs ch, const float* __restrict__ z0,
    const float* __restrict__ dz, const float* __restrict__ sn_pre, const float* __restrict__ G, BtPtrs btp,
    T* __restrict__ dX, float* __restrict__ dzatt, float* __restrict__ pdwa, float* __restrict__ pdba,
    float* __restrict__ pchain, int N, int P, int S, int C, int K, int R, int act, float inv_keep, uint32_t thresh,
    uint64_t seed, uint64_t offset, const uint64_t* __restrict__ offset_dev) {
  constexpr int EPV = Vec<T>::EPV, EL = NVL * EPV, CP = 64 * EL;   // CP: the channel count the instance pads to
  // the image's R rows of dz and the attention weights wait in LDS (zero beyond C), so that two blocks fit a CU;
  // the merge of the dwa rows reuses the dz rows' space after the loop
  __shared__ __attribute__((aligned(16))) float sm_dz[RMAX * CP];
  __shared__ __attribute__((aligned(16))) float sm_wa[FUSED ? CP : 4];
  float* const sm = sm_dz;
  __shared__ float sm_stat[4][8];
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev_x(seed, offset_dev ? *offset_dev : offset, thresh, k0, k1);
  const int blk = blockIdx.x, n = blk / S, s = blk % S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p_begin = (int)(((long)s * P) / S), p_end = (int)(((long)(s + 1) * P) / S);
  const int nvec = C / EPV;
  const float invP = 1.0f / (float)P;
  float cw[RMAX - 1], cb[RMAX - 1];
#pragma unroll
  for (int r = 0; r < RMAX - 1; ++r) {
    cw[r] = r < R - 1 ? ch.w[r][0] : 0.f;
    cb[r] = r < R - 1 ? ch.b[r][0] : 0.f;
  }
  float sn[RMAX];
#pragma unroll
  for (int r = 0; r < RMAX; ++r) {
    sn[r] = 0.f;
    if (r < R) {
      if (sn_pre) {
        sn[r] = sn_pre[(size_t)r * N + n];
      } else {
        float a = 0.f;
        for (int k = lane; k < K; k += 64) a = fmaf(G[(size_t)n * K + k], btp.bt[r][k], a);
        sn[r] = wave_sum(a);
      }
    }
  }
  float dwa[EL];
#pragma unroll
  for (int i = 0; i < EL; ++i) dwa[i] = 0.f;
  float cdw[RMAX - 1] = {0.f, 0.f, 0.f}, cdb[RMAX - 1] = {0.f, 0.f, 0.f}, dba = 0.f;
  const T* xim = X + (size_t)n * P * C;
  T* dxim = dX + (size_t)n * P * C;
  uint4 nxt[NVL];
  float z0n = 0.f;
  if (p_begin + wave < p_end) {
    row_load<T, NVL>(nxt, xim + (size_t)(p_begin + wave) * C, lane, nvec);
    z0n = z0[(size_t)n * P + p_begin + wave];
  }
  // staged behind the first row's loads, which travel meanwhile
  for (int i = threadIdx.x; i < RMAX * CP; i += 256) {
    const int r = i / CP, c = i - r * CP;
    sm_dz[i] = (r < R && c < C) ? dz[((size_t)r * N + n) * C + c] : 0.f;
  }
  if (FUSED)
    for (int c = threadIdx.x; c < CP; c += 256) sm_wa[c] = c < C ? Wa[c] : 0.f;
  __syncthreads();
  for (int p = p_begin + wave; p < p_end; p += 4) {
    float x[EL];
#pragma unroll
    for (int j = 0; j < NVL; ++j) Vec<T>::unpack(nxt[j], x + j * EPV);
    const float z0p = z0n;
    if (p + 4 < p_end) {   // the next row travels while this one is consumed
      row_load<T, NVL>(nxt, xim + (size_t)(p + 4) * C, lane, nvec);
      z0n = z0[(size_t)n * P + p + 4];
    }
    const size_t px = (size_t)n * P + p;
    float Z[RMAX], A[RMAX];
    rank_chain(z0p, cw, cb, R, act, Z, A);
    uint32_t bits = 0xFFFFFFFFu;
    if (TRAIN) bits = row_keep_bits<RngAny, NVL, EPV>((uint64_t)px * C, lane, nvec, k0, k1, thresh);
    float dZ[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
      dZ[r] = 0.f;
      if (r < R) {
        float d = 0.f;   // row_dot over the kept elements, inline: as a routine it spills (profiles/rowpass_summary.md)
#pragma unroll
        for (int j = 0; j < NVL; ++j) {
#pragma unroll
          for (int e = 0; e < EPV; e += 4) {
            const float4 g4 = *reinterpret_cast<const float4*>(sm_dz + r * CP + (j * 64 + lane) * EPV + e);
            const int i = j * EPV + e;
            d = fmaf((bits >> i) & 1u ? x[i] : 0.f, g4.x, d);
            d = fmaf((bits >> (i + 1)) & 1u ? x[i + 1] : 0.f, g4.y, d);
            d = fmaf((bits >> (i + 2)) & 1u ? x[i + 2] : 0.f, g4.z, d);
            d = fmaf((bits >> (i + 3)) & 1u ? x[i + 3] : 0.f, g4.w, d);
          }
        }
        float tot = wave_sum(d);
        if (TRAIN) tot *= inv_keep;
        const float dA = (tot + sn[r]) * invP;
        dZ[r] = (act == M1_ACT_RELU && !(Z[r] > 0.f)) ? 0.f : dA;
      }
    }
    // dZ~_r = dZ_r + w_{r+1} dZ~_{r+1}: the total gradient arriving at Z_r
#pragma unroll
    for (int r = RMAX - 2; r >= 0; --r)
      if (r + 1 < R) dZ[r] = fmaf(cw[r], dZ[r + 1], dZ[r]);
#pragma unroll
    for (int r = 1; r < RMAX; ++r) {
      if (r < R) {
        cdw[r - 1] = fmaf(dZ[r], Z[r - 1], cdw[r - 1]);
        cdb[r - 1] += dZ[r];
      }
    }
    const float g0 = dZ[0];
    float ap[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) ap[r] = A[r] * invP * (TRAIN ? inv_keep : 1.f);
#pragma unroll
    for (int j = 0; j < NVL; ++j) {
      const int v = j * 64 + lane;
      float o[EPV];
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] = 0.f;
#pragma unroll
      for (int r = 0; r < RMAX; ++r) {
        if (r < R) {
#pragma unroll
          for (int e = 0; e < EPV; e += 4) {
            const float4 g4 = *reinterpret_cast<const float4*>(sm_dz + r * CP + (j * 64 + lane) * EPV + e);
            o[e] = fmaf(ap[r], g4.x, o[e]);
            o[e + 1] = fmaf(ap[r], g4.y, o[e + 1]);
            o[e + 2] = fmaf(ap[r], g4.z, o[e + 2]);
            o[e + 3] = fmaf(ap[r], g4.w, o[e + 3]);
          }
        }
      }
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int i = j * EPV + e;
        o[e] = (bits >> i) & 1u ? o[e] : 0.f;
        if (FUSED) {
          o[e] = fmaf(g0, sm_wa[(j * 64 + lane) * EPV + e], o[e]);
          dwa[i] = fmaf(g0, x[i], dwa[i]);
        }
      }
      if (v < nvec) st16(dxim + (size_t)p * C + (size_t)v * EPV, Vec<T>::pack(o));
    }
    if (FUSED) dba += g0;
    else if (lane == 0) dzatt[px] = g0;
  }
  if (FUSED) row_merge4<NVL, EPV>(dwa, sm, pdwa + (size_t)blk * C, wave, lane, nvec);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < RMAX - 1; ++r) {
      sm_stat[wave][2 * r] = cdw[r];
      sm_stat[wave][2 * r + 1] = cdb[r];
    }
    sm_stat[wave][6] = dba;
    sm_stat[wave][7] = 0.f;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int j = threadIdx.x;
    const float t = row_stat_merge4(sm_stat, j);
    if (j < 6) pchain[(size_t)blk * 8 + j] = t;
    else if (j == 6) { if (FUSED) pdba[blk] = t; pchain[(size_t)blk * 8 + 6] = 0.f; }
    else pchain[(size_t)blk * 8 + 7] = 0.f;
  }
}

// --------------------------------------------------------------------------------------------
// Merge of the S block partials of each image (fixed order): zsave [N,R,C] and abar [N,R] as the caller keeps them,
// and the rank-major copies zr [R][N][C] / abar_r [R][N] the per-rank products read.  grid (N, ceil(R C / 1024)).
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m1r_finalize_fwd_kernel(const float* __restrict__ pacc,
                                                               const float* __restrict__ pstat, int N, int P, int S,
                                                               int C, int R, float* __restrict__ zsave,
                                                               float* __restrict__ abar, float* __restrict__ zr,
                                                               float* __restrict__ abar_r) {
  const int n = blockIdx.x;
  const int RC = R * C;
  const float invP = 1.0f / (float)P;
  const int i = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (i < RC) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const float4 v = *reinterpret_cast<const float4*>(pacc + ((size_t)n * S + s) * RC + i);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    a.x *= invP; a.y *= invP; a.z *= invP; a.w *= invP;
    const int r = i / C, c = i - r * C;
    *reinterpret_cast<float4*>(zsave + (size_t)n * RC + i) = a;
    *reinterpret_cast<float4*>(zr + ((size_t)r * N + n) * C + c) = a;
  }
  if (blockIdx.y == 0 && (int)threadIdx.x < R) {
    const int r = threadIdx.x;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += pstat[((size_t)n * S + s) * 4 + r];
    a *= invP;
    abar[(size_t)n * R + r] = a;
    abar_r[(size_t)r * N + n] = a;
  }
}

// logits = ((l_0 + l_1) + l_2) + l_3 over the per-rank products lpart [R][N K]
__global__ __launch_bounds__(256) void m1r_logits_sum_kernel(const float* __restrict__ lpart, float* __restrict__ logits,
                                                             long NK, int R) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= NK) return;
  float a = lpart[i];
  for (int r = 1; r < R; ++r) a += lpart[(size_t)r * NK + i];
  logits[i] = a;
}

// backward: the caller's zsave [N,R,C] / abar [N,R] into the rank-major copies
__global__ __launch_bounds__(256) void m1r_unstack_kernel(const float* __restrict__ zsave, const float* __restrict__ abar,
                                                          float* __restrict__ zr, float* __restrict__ abar_r, int N, int C,
                                                          int R) {
  const long tot = (long)N * R * C / 4;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < tot) {
    const long i = t * 4;
    const int n = (int)(i / ((long)R * C));
    const int rem = (int)(i - (long)n * R * C);
    const int r = rem / C, c = rem - r * C;
    *reinterpret_cast<float4*>(zr + ((size_t)r * N + n) * C + c) = *reinterpret_cast<const float4*>(zsave + i);
  }
  if (t < (long)N * R) {
    const int n = (int)(t / R), r = (int)(t % R);
    abar_r[(size_t)r * N + n] = abar[t];
  }
}

// The finishing step of the backward call: the chain gradients from the per-block partials (fixed order), and, off
// the small-K head route, dbt_r = sum_n abar_r[n] G[n,:].  One block of 256 threads.
struct FinishArgs {
  float* dcw[RMAX - 1]; float* dcb[RMAX - 1];
  float* dbt[RMAX];   // null: the head kernels wrote dbt_r
};
__global__ __launch_bounds__(256) void m1r_finish_bwd_kernel(const float* __restrict__ pchain, int nblk, int R,
                                                             FinishArgs fa, const float* __restrict__ abar_r,
                                                             const float* __restrict__ G, int N, int K) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = 0; j < 2 * (R - 1); ++j) {
    float a = 0.f;
    for (int b = threadIdx.x; b < nblk; b += 256) a += pchain[(size_t)b * 8 + j];
    a = wave_sum(a);
    __syncthreads();
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float t = (red[0] + red[1]) + (red[2] + red[3]);
      if (j & 1) fa.dcb[j >> 1][0] = t; else fa.dcw[j >> 1][0] = t;
    }
  }
  for (int r = 0; r < R; ++r) {
    if (!fa.dbt[r]) continue;
    for (int k = threadIdx.x; k < K; k += 256) {
      float a = 0.f;
      for (int n = 0; n < N; ++n) a = fmaf(abar_r[(size_t)r * N + n], G[(size_t)n * K + k], a);
      fa.dbt[r][k] = a;
    }
  }
}

// the rank region of the workspace, behind m1_plan's (byte offsets from the workspace's start)
struct RankPlan {
  M1Plan pl;
  size_t off_pacc, off_pstat, off_zr, off_abar, off_dz, off_sn, off_lpart, off_pchain, total;
};
RankPlan rank_plan(int N, int P, int C, int Ca, int K, int R) {
  RankPlan rp;
  rp.pl = m1_plan(N, P, C, Ca, K);
  size_t off = align_up(rp.pl.total, 256);
  rp.off_pacc = off;   off += align_up((size_t)rp.pl.nblk * R * C * 4, 256);
  rp.off_pstat = off;  off += align_up((size_t)rp.pl.nblk * 4 * 4, 256);
  rp.off_zr = off;     off += align_up((size_t)R * N * C * 4, 256);
  rp.off_abar = off;   off += align_up((size_t)R * N * 4, 256);
  rp.off_dz = off;     off += align_up((size_t)R * N * C * 4, 256);
  rp.off_sn = off;     off += align_up((size_t)R * N * 4, 256);
  rp.off_lpart = off;  off += align_up((size_t)R * N * K * 4, 256);
  rp.off_pchain = off; off += align_up((size_t)rp.pl.nblk * 8 * 4, 256);
  rp.total = off;
  return rp;
}

template <typename T, int NVL>
int launch_fwd(const M1Call& c, const RankCall& rk, const RankPlan& rp, const M1Fwd& io, const ChainPtrs& ch) {
  char* w = static_cast<char*>(rk.ws);
  float* pacc = reinterpret_cast<float*>(w + rp.off_pacc);
  float* pstat = reinterpret_cast<float*>(w + rp.off_pstat);
  return m1_fused_train(c.fused, c.train, [&](auto F, auto TR) -> int {
    launch_ev(m1r_pool_fwd_kernel<T, NVL, decltype(F)::value, decltype(TR)::value>, dim3(c.pl.nblk), dim3(256), 0, c.st,
              nullptr, nullptr, static_cast<const T*>(io.X), io.Wa, io.ba, ch, rk.z0, io.att, pacc, pstat, c.P, c.pl.S,
              c.C, rk.R, c.act, c.inv_keep, c.key.thresh, c.key.seed, c.key.offset, c.key.offset_dev);
    return APA_OK;
  });
}

template <typename T, int NVL>
int launch_bwd(const M1Call& c, const RankCall& rk, const RankPlan& rp, const M1Bwd& io, const ChainPtrs& ch,
               const float* sn) {
  char* w = static_cast<char*>(rk.ws);
  BtPtrs btp;
  for (int r = 0; r < RMAX; ++r) btp.bt[r] = r < rk.R ? rk.bt[r] : nullptr;
  return m1_fused_train(c.fused, c.train, [&](auto F, auto TR) -> int {
    launch_ev(m1r_bwd_main_kernel<T, NVL, decltype(F)::value, decltype(TR)::value>, dim3(c.pl.nblk), dim3(256), 0, c.st,
              nullptr, nullptr, static_cast<const T*>(io.X), io.Wa, ch, rk.z0,
              reinterpret_cast<const float*>(w + rp.off_dz), sn, io.G, btp, static_cast<T*>(io.dX), c.dzatt, c.pdwa,
              c.pdba, reinterpret_cast<float*>(w + rp.off_pchain), c.N, c.P, c.pl.S, c.C, c.K, rk.R, c.act, c.inv_keep,
              c.key.thresh, c.key.seed, c.key.offset, c.key.offset_dev);
    return APA_OK;
  });
}

ChainPtrs chain_ptrs(const RankCall& rk) {
  ChainPtrs ch;
  for (int r = 0; r < RMAX - 1; ++r) {
    ch.w[r] = r < rk.R - 1 ? rk.cw[r] : nullptr;
    ch.b[r] = r < rk.R - 1 ? rk.cb[r] : nullptr;
  }
  return ch;
}
}  // namespace

// NVL of the instance that serves C (0: none): 8 elements per lane up to C = 512, 32 up to C = 2048, in 16-byte
// vectors of 4 (f32) or 8 (bf16) elements
int m1r_vectors_per_lane(int C, int dtype) {
  const int epv = dtype == APA_DTYPE_BF16 ? 8 : 4;
  if (C < epv || C % epv != 0) return 0;
  return C <= 512 ? 8 / epv : (C <= 2048 ? 32 / epv : 0);
}

bool m1r_supported(int C, int Ca, int dtype, bool fused) {
  const int epv = dtype == APA_DTYPE_BF16 ? 8 : 4;
  if (!fused && (Ca < epv || Ca % epv != 0)) return false;
  return m1r_vectors_per_lane(C, dtype) != 0;
}

size_t m1r_workspace_bytes(int N, int P, int C, int Ca, int K, int R) { return rank_plan(N, P, C, Ca, K, R).total; }

int m1r_forward(const M1Call& c, const RankCall& rk, const M1Fwd& io) {
  const int N = c.N, C = c.C, K = c.K, R = rk.R;
  const RankPlan rp = rank_plan(N, c.P, C, c.Ca, K, R);
  char* w = static_cast<char*>(rk.ws);
  float* zr = reinterpret_cast<float*>(w + rp.off_zr);
  float* abar_r = reinterpret_cast<float*>(w + rp.off_abar);
  float* lpart = reinterpret_cast<float*>(w + rp.off_lpart);
  const ChainPtrs ch = chain_ptrs(rk);
  int rc;
  if (!c.fused) {   // Z_0 = Xatt . Wa + ba by the attention GEMV, no activation: the chain starts from it
    M1Call c0 = c;
    c0.act = M1_ACT_ID;
    M1Fwd f0 = io;
    f0.att = rk.z0;
    if ((rc = m1_att_gemv_forward(c0, f0)) != APA_OK) return rc;
  }
  rc = row_instance(C, c.dtype, [&](auto t, auto nvl) {
    return launch_fwd<decltype(t), decltype(nvl)::value>(c, rk, rp, io, ch);
  });
  if (rc != APA_OK) return rc;
  APA_LAUNCH_CHECK("m1r_pool_fwd_kernel");
  hipLaunchKernelGGL(m1r_finalize_fwd_kernel, dim3(N, (R * C / 4 + 255) / 256), dim3(256), 0, c.st,
                     reinterpret_cast<const float*>(w + rp.off_pacc), reinterpret_cast<const float*>(w + rp.off_pstat), N,
                     c.P, c.pl.S, C, R, io.zsave, io.abar, zr, abar_r);
  APA_LAUNCH_CHECK("m1r_finalize_fwd_kernel");
  // logits = sum_r z_r . Wt_r + abar_r (x) bt_r: one product per rank with the M == 1 kernels, then the fixed-order sum
  for (int r = 0; r < R; ++r) {
    float* z = zr + (size_t)r * N * C;
    float* lp = lpart + (size_t)r * N * K;
    if (m1_logits2_supported(C, K))
      rc = m1_logits2(z, rk.Wt[r], abar_r + (size_t)r * N, rk.bt[r], lp, c.gemm_ws, N, C, K, c.st);
    else
      rc = sgemm_small(z, C, 1, rk.Wt[r], K, 1, lp, K, N, K, C, c.pl.lsplits, abar_r + (size_t)r * N, rk.bt[r],
                       c.gemm_ws, c.st);
    if (rc != APA_OK) return rc;
  }
  const long NK = (long)N * K;
  hipLaunchKernelGGL(m1r_logits_sum_kernel, dim3((unsigned)((NK + 255) / 256)), dim3(256), 0, c.st, lpart, io.logits, NK,
                     R);
  APA_LAUNCH_CHECK("m1r_logits_sum_kernel");
  return APA_OK;
}

int m1r_backward(const M1Call& c, const RankCall& rk, const M1Bwd& io) {
  const int N = c.N, C = c.C, K = c.K, R = rk.R;
  hipStream_t st = c.st;
  const RankPlan rp = rank_plan(N, c.P, C, c.Ca, K, R);
  char* w = static_cast<char*>(rk.ws);
  float* zr = reinterpret_cast<float*>(w + rp.off_zr);
  float* abar_r = reinterpret_cast<float*>(w + rp.off_abar);
  float* dz = reinterpret_cast<float*>(w + rp.off_dz);
  float* sn = reinterpret_cast<float*>(w + rp.off_sn);
  const ChainPtrs ch = chain_ptrs(rk);
  int rc;
  {
    const long nt = (long)N * R * C / 4;
    hipLaunchKernelGGL(m1r_unstack_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, io.zsave, io.abar, zr,
                       abar_r, N, C, R);
    APA_LAUNCH_CHECK("m1r_unstack_kernel");
  }
  // dz_r = G . Wt_r^T, dWt_r = z_r^T . G (and on the small-K route dbt_r, sn_r = G . bt_r): per rank
  bool small = true;
  for (int r = 0; r < R; ++r) small = small && m1_small_route_ok(C, K, io.G, rk.Wt[r], zr + (size_t)r * N * C);
  for (int r = 0; r < R; ++r) {
    const float* z = zr + (size_t)r * N * C;
    float* dzr = dz + (size_t)r * N * C;
    if (small) {
      rc = m1_bwd_head_supported(N, C, K)
               ? m1_bwd_head(io.G, rk.Wt[r], z, abar_r + (size_t)r * N, rk.bt[r], dzr, rk.dWt[r], rk.dbt[r],
                             sn + (size_t)r * N, N, C, K, st)
               : m1_bwd_small(io.G, rk.Wt[r], z, abar_r + (size_t)r * N, rk.bt[r], dzr, rk.dWt[r], rk.dbt[r],
                              sn + (size_t)r * N, N, C, K, st);
      if (rc != APA_OK) return rc;
    } else {
      rc = sgemm_small(io.G, K, 1, rk.Wt[r], 1, K, dzr, C, N, C, K, 1, nullptr, nullptr, c.gemm_ws, st);
      if (rc != APA_OK) return rc;
      rc = sgemm_small(z, 1, C, io.G, K, 1, rk.dWt[r], K, C, K, N, 1, nullptr, nullptr, c.gemm_ws, st);
      if (rc != APA_OK) return rc;
    }
  }
  rc = row_instance(C, c.dtype, [&](auto t, auto nvl) {
    return launch_bwd<decltype(t), decltype(nvl)::value>(c, rk, rp, io, ch, small ? sn : nullptr);
  });
  if (rc != APA_OK) return rc;
  APA_LAUNCH_CHECK("m1r_bwd_main_kernel");
  FinishArgs fa;
  for (int r = 0; r < RMAX - 1; ++r) {
    fa.dcw[r] = r < R - 1 ? rk.dcw[r] : nullptr;
    fa.dcb[r] = r < R - 1 ? rk.dcb[r] : nullptr;
  }
  for (int r = 0; r < RMAX; ++r) fa.dbt[r] = (!small && r < R) ? rk.dbt[r] : nullptr;
  hipLaunchKernelGGL(m1r_finish_bwd_kernel, dim3(1), dim3(256), 0, st,
                     reinterpret_cast<const float*>(w + rp.off_pchain), c.pl.nblk, R, fa, abar_r, io.G, N, K);
  APA_LAUNCH_CHECK("m1r_finish_bwd_kernel");
  // dWa / dba (and the device-side dropout counter): the attention GEMV backward for a separate input, then the
  // fixed-order column sum, as the rank-1 call ends
  int nred = c.pl.nblk, cred = C;
  if (!c.fused) {
    if ((rc = m1_att_gemv_backward(c, io, &nred)) != APA_OK) return rc;
    cred = c.Ca;
  }
  ColsumArgs cs;
  cs.pdwa = c.pdwa; cs.pdba = c.pdba; cs.nblk = nred; cs.C = cred; cs.ld = cred; cs.dwa = io.dWa; cs.dba = io.dba;
  cs.rng_bump = c.bump;
  return m1_colsum(cs, st);
}

}  // namespace apa
