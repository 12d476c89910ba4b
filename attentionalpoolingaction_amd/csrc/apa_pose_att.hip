// apa_pose_att.hip -- the pose-heatmap attention head (cfg.NET.USE_POSE_ATTENTION_LOGITS, nets_factory.py:162-189):
// the J PoseLogits maps (a selection of them), their mean and a constant map act as M attention maps on last_conv;
// the M attention-weighted spatial means are concatenated on the channel axis, dropped out and classified.
//
//   A[n,p,m]       = Pl[n,p,sel[m]] (m < n_sel) | mean_j Pl[n,p,j] (avged) | 1 (last map)
//   F[n, m*C + c]  = (1/P) sum_p A[n,p,m] X[n,p,c]                        pal_pool_fwd_kernel   (one read of X)
//   logits         = (F * mask / keep) . W + b,  W [M*C, K]                pal_cls_fwd_kernel    (one read of W, f32 MFMA)
//                                                                          + pal_cls_reduce_kernel (fixed-order slab sum)
//   dF = (G . W^T) * mask / keep, dW = Fd^T . G, db = colsum G             pal_cls_bwd_kernel    (one read of W, f32 MFMA)
//   dX (=|+=) (1/P) sum_m A dF,  dA = (1/P) sum_c X dF                     pal_pool_bwd_kernel   (one read of X)
//   dPl += fold of dA onto the parts (selection, mean; constant map dropped) pal_fold_kernel
//
// Every split reduction is summed in a fixed order (LDS in wave order, per-slab partials summed slab by slab): no
// float atomics, two identical calls give bit-identical results.  The dropout mask is the library's counter hash over
// the flat index n*(M*C) + m*C + c of F, i.e. apa_dropout_mask(N*M*C, ...), or a replayed bit image
// (APA_FLAG_RNG_EXTERNAL).
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {
namespace {

constexpr int PAL_MAXM = 32;      // maps (n_sel + avged + 1)
constexpr int PAL_SLAB = 256;     // channels per pooling block: 64 lanes x 4
constexpr int PAL_WAVES = 8;      // pooling: the waves of a block split the pixels
constexpr int PAL_PCHUNK = 64;    // pixels whose attention rows are staged in LDS at a time
constexpr int CLS_ROWS = 256;     // classifier forward: rows of W per block
constexpr int CLS_WAVES = 8;
constexpr int CLS_NT = 4;         // classifier forward: 16-column tiles of K per wave and pass
constexpr int CB_WAVES = 4;       // classifier backward: 16 rows of W per wave
constexpr int PAL_MAXK = 480;     // classifier backward: a 32 x K tile of G in LDS (<= 64 KB)

struct PalMaps {
  int M, nsel, avged, J;
  int sel[PAL_MAXM];
};
struct PalRng {
  uint32_t thresh;
  uint64_t seed, offset;
  float inv_keep;
  int train;
};

template <typename T> struct Ld4;
template <> struct Ld4<float> {
  static __device__ __forceinline__ void load(const float* p, float* o) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  static __device__ __forceinline__ void store(float* p, const float* o) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
  }
};
template <> struct Ld4<bf16_t> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* o) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    o[0] = bf16_lo(v.x); o[1] = bf16_hi(v.x); o[2] = bf16_lo(v.y); o[3] = bf16_hi(v.y);
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* o) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
  }
};

__device__ __forceinline__ void copy_sel(const PalMaps& mp, int* s_sel) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < PAL_MAXM; ++i) s_sel[i] = mp.sel[i];
  }
}

// A[n, p0 .. p0+np-1, 0 .. M-1] -> s_att[pp * PAL_MAXM + m]
__device__ __forceinline__ void stage_att(const float* __restrict__ Pl, const PalMaps& mp, const int* s_sel, int n,
                                          int P, int p0, int np, float* s_att) {
  const int M = mp.M, J = mp.J;
  const float invJ = 1.0f / (float)J;
  for (int i = threadIdx.x; i < np * M; i += blockDim.x) {
    const int pp = i / M, m = i - pp * M;
    const float* row = Pl + ((size_t)n * P + p0 + pp) * J;
    float a = 1.0f;
    if (m < mp.nsel) {
      a = row[s_sel[m]];
    } else if (m < mp.nsel + mp.avged) {
      float s = 0.f;
      for (int j = 0; j < J; ++j) s += row[j];
      a = s * invJ;
    }
    s_att[pp * PAL_MAXM + m] = a;
  }
}

__device__ __forceinline__ float keep_scale(const PalRng& rng, uint32_t k0, uint32_t k1, uint64_t e) {
  if (!rng.train) return 1.0f;
  float m0, m1;
  rng_keep2_x(e & ~1ull, k0, k1, rng.thresh, m0, m1);
  return ((e & 1) ? m1 : m0) * rng.inv_keep;
}

// ------------------------------------------------------------------------------------------------------------------
// Pooling forward.  Block (slab, n): 256 channels of one image; each lane owns 4 channels, the 8 waves split the
// pixels (wave w takes pixels w, w + 8, ... of every chunk, ascending); the wave partials are summed in LDS in wave
// order.  X is read once.
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int MT>
__global__ __launch_bounds__(64 * PAL_WAVES) void pal_pool_fwd_kernel(const T* __restrict__ X,
                                                                      const float* __restrict__ Pl,
                                                                      float* __restrict__ F, PalMaps mp, int P,
                                                                      int C, float invP) {
  __shared__ float s_att[PAL_PCHUNK * PAL_MAXM];
  __shared__ float s_red[MT * PAL_SLAB];
  __shared__ int s_sel[PAL_MAXM];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = slab * PAL_SLAB + lane * 4;
  const bool active = c0 < C;
  const int M = mp.M;
  copy_sel(mp, s_sel);
  float acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[m][i] = 0.f;
  for (int p0 = 0; p0 < P; p0 += PAL_PCHUNK) {
    const int np = min(PAL_PCHUNK, P - p0);
    __syncthreads();
    stage_att(Pl, mp, s_sel, n, P, p0, np, s_att);
    __syncthreads();
    if (active) {
      for (int pp = wave; pp < np; pp += PAL_WAVES) {
        float x[4];
        Ld4<T>::load(X + ((size_t)n * P + p0 + pp) * C + c0, x);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (m < M) {
            const float a = s_att[pp * PAL_MAXM + m];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[m][i] = fmaf(a, x[i], acc[m][i]);
          }
        }
      }
    }
  }
  for (int w = 0; w < PAL_WAVES; ++w) {
    __syncthreads();
    if (wave == w && active) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        if (m < M) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float* d = &s_red[m * PAL_SLAB + lane * 4 + i];
            *d = w == 0 ? acc[m][i] : *d + acc[m][i];
          }
        }
      }
    }
  }
  __syncthreads();
  const size_t R = (size_t)M * C;
  for (int i = threadIdx.x; i < M * PAL_SLAB; i += blockDim.x) {
    const int m = i / PAL_SLAB, c = slab * PAL_SLAB + (i - m * PAL_SLAB);
    if (c < C) F[(size_t)n * R + (size_t)m * C + c] = s_red[i] * invP;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Pooling backward.  Same blocks as the forward pass (same (slab, n) -> same hardware block index -> same XCD), pixels
// walked the other way round: descending.  dF arrives masked and scaled (pal_cls_bwd_kernel).
// dX is written (or added to) per pixel; dA over the block's 256 channels is a wave sum per pixel and map, stored as a
// per-slab partial that pal_fold_kernel sums slab by slab.
// ------------------------------------------------------------------------------------------------------------------
template <typename T, int MT, bool ACC>
__global__ __launch_bounds__(64 * PAL_WAVES) void pal_pool_bwd_kernel(const T* __restrict__ X,
                                                                      const float* __restrict__ Pl,
                                                                      const float* __restrict__ dF, T* dX,
                                                                      float* __restrict__ dApart, PalMaps mp, int N,
                                                                      int P, int C, float invP) {
  __shared__ float s_att[PAL_PCHUNK * PAL_MAXM];
  __shared__ int s_sel[PAL_MAXM];
  const int n = blockIdx.y, slab = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = slab * PAL_SLAB + lane * 4;
  const bool active = c0 < C;
  const int M = mp.M;
  const size_t R = (size_t)M * C;
  copy_sel(mp, s_sel);
  float g[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (m < M && active) Ld4<float>::load(dF + (size_t)n * R + (size_t)m * C + c0, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) g[m][i] = v[i] * invP;
  }
  const int nchunk = (P + PAL_PCHUNK - 1) / PAL_PCHUNK;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int p0 = ch * PAL_PCHUNK, np = min(PAL_PCHUNK, P - p0);
    __syncthreads();
    stage_att(Pl, mp, s_sel, n, P, p0, np, s_att);
    __syncthreads();
    for (int pp = np - 1 - wave; pp >= 0; pp -= PAL_WAVES) {
      const size_t pix = (size_t)n * P + p0 + pp;
      float x[4] = {0.f, 0.f, 0.f, 0.f}, dx[4] = {0.f, 0.f, 0.f, 0.f};
      if (active) Ld4<T>::load(X + pix * C + c0, x);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        if (m < M) {
          const float a = s_att[pp * PAL_MAXM + m];
#pragma unroll
          for (int i = 0; i < 4; ++i) dx[i] = fmaf(a, g[m][i], dx[i]);
        }
      }
      if (active) {
        if (ACC) {
          float o[4];
          Ld4<T>::load(dX + pix * C + c0, o);
#pragma unroll
          for (int i = 0; i < 4; ++i) dx[i] += o[i];
        }
        Ld4<T>::store(dX + pix * C + c0, dx);
      }
      float* dst = dApart + ((size_t)slab * N * P + pix) * M;
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        if (m < M) {
          float s = x[0] * g[m][0];
#pragma unroll
          for (int i = 1; i < 4; ++i) s = fmaf(x[i], g[m][i], s);
          s = wave_sum(s);            // all 64 lanes take part (idle lanes add 0)
          if (lane == 0) dst[m] = s;
        }
      }
    }
  }
}

// dPl[n,p,j] += sum_{m < nsel, sel[m] == j} dA[n,p,m] + avged * dA[n,p,nsel] / J, dA = sum over slabs (in order)
__global__ __launch_bounds__(256) void pal_fold_kernel(const float* __restrict__ dApart, float* __restrict__ dPl,
                                                       PalMaps mp, int NP, int nslab) {
  __shared__ int s_sel[PAL_MAXM];
  copy_sel(mp, s_sel);
  __syncthreads();
  const int J = mp.J, M = mp.M;
  const size_t total = (size_t)NP * J;
  const float invJ = 1.0f / (float)J;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pix = i / J;
    const int j = (int)(i - pix * J);
    float add = 0.f;
    for (int m = 0; m < mp.nsel + mp.avged; ++m) {
      const bool hit = m < mp.nsel ? s_sel[m] == j : true;
      if (!hit) continue;
      float d = 0.f;
      for (int s = 0; s < nslab; ++s) d += dApart[((size_t)s * NP + pix) * M + m];
      add += m < mp.nsel ? d : d * invJ;
    }
    dPl[i] += add;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Classifier forward on the f32 MFMA (v_mfma_f32_16x16x4_f32: bitwise an fmaf chain).  Block = a slab of 256 rows of
// W; the dropped-out slab of F (32 images at a time) sits in LDS; wave w takes the 16-column tiles w, w + 8, ... of K.
// Each element of W is read once (per 32 images).  Per-slab partial logits -> pal_cls_reduce_kernel.
//   A[i = n][kk = r] = Fd[n][r] (lane: n = l & 15, r = l >> 4),  B[kk = r][j = k] = W[r][k] (lane: r = l >> 4,
//   k = l & 15),  D: k = l & 15, n = 4 (l >> 4) + reg
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * CLS_WAVES) void pal_cls_fwd_kernel(const float* __restrict__ F,
                                                                     const float* __restrict__ W,
                                                                     float* __restrict__ part, PalRng rng, int N,
                                                                     int R, int K) {
  constexpr int LDF = CLS_ROWS + 1;
  __shared__ float s_f[32 * LDF];
  const int slab = blockIdx.x, r0 = slab * CLS_ROWS;
  const int nrows = min(CLS_ROWS, R - r0);             // a multiple of 4 (R = M*C, C % 4 == 0)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int KT = (K + 15) / 16;
  uint32_t k0 = 0, k1 = 0;
  if (rng.train) rng_key_dev_x(rng.seed, rng.offset, rng.thresh, k0, k1);
  for (int nb = 0; nb < N; nb += 32) {
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * (CLS_ROWS / 2); i += blockDim.x) {
      const int nn = i / (CLS_ROWS / 2), rr = 2 * (i - nn * (CLS_ROWS / 2));
      const int n = nb + nn;
      float v0 = 0.f, v1 = 0.f;
      if (n < N && rr < nrows) {
        const size_t e = (size_t)n * R + r0 + rr;     // even: R and r0 + rr are
        v0 = F[e]; v1 = F[e + 1];
        if (rng.train) {
          float m0, m1;
          rng_keep2_x(e, k0, k1, rng.thresh, m0, m1);
          v0 *= m0 * rng.inv_keep;
          v1 *= m1 * rng.inv_keep;
        }
      }
      s_f[nn * LDF + rr] = v0;
      s_f[nn * LDF + rr + 1] = v1;
    }
    __syncthreads();
    for (int kt0 = wave; kt0 < KT; kt0 += CLS_WAVES * CLS_NT) {
      f32x4 acc[CLS_NT][2];
#pragma unroll
      for (int t = 0; t < CLS_NT; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int rr = 0; rr < nrows; rr += 4) {
        const int kr = rr + (lane >> 4);
        const float a0 = s_f[(lane & 15) * LDF + kr];
        const float a1 = s_f[(16 + (lane & 15)) * LDF + kr];
        const float* wrow = W + (size_t)(r0 + kr) * K;
#pragma unroll
        for (int t = 0; t < CLS_NT; ++t) {
          const int kt = kt0 + t * CLS_WAVES;
          if (kt < KT) {                                   // wave-uniform
            const int k = kt * 16 + (lane & 15);
            const float b = k < K ? wrow[k] : 0.f;
            acc[t][0] = mfma16(a0, b, acc[t][0]);
            acc[t][1] = mfma16(a1, b, acc[t][1]);
          }
        }
      }
#pragma unroll
      for (int t = 0; t < CLS_NT; ++t) {
        const int kt = kt0 + t * CLS_WAVES;
        const int k = kt * 16 + (lane & 15);
        if (kt >= KT || k >= K) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int n = nb + 16 * h + 4 * (lane >> 4) + q;
            if (n < N) part[((size_t)slab * N + n) * K + k] = acc[t][h][q];
          }
      }
    }
  }
}

// logits[n,k] = b[k] + sum_s part[s][n][k], s ascending
__global__ __launch_bounds__(256) void pal_cls_reduce_kernel(const float* __restrict__ part,
                                                             const float* __restrict__ b,
                                                             float* __restrict__ logits, int N, int K, int nslab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * K) return;
  float s = 0.f;
  for (int t = 0; t < nslab; ++t) s += part[(size_t)t * N * K + i];
  logits[i] = s + b[i % K];
}

// ------------------------------------------------------------------------------------------------------------------
// Classifier backward in one pass over W.  Wave = 16 rows of W; G (32 images at a time, zero-padded to 16-column
// tiles) sits in LDS.  dFd[n][r] = sum_k G[n][k] W[r][k] and dW[r][k] = sum_n Fd[n][r] G[n][k] on the f32 MFMA; the
// row of W is read once (per 32 images).  dF = dFd * mask / keep goes to the workspace for the pooling backward.
// db = colsum G (block 0, n ascending).
//   dFd:  A[i = n][kk = k] = G[n][k],  B[kk = k][j = r] = W[r][k];  D: r = l & 15, n = 4 (l >> 4) + reg
//   dW:   A[i = r][kk = n] = Fd[n][r], B[kk = n][j = k] = G[n][k];  D: k = l & 15, r = 4 (l >> 4) + reg
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * CB_WAVES) void pal_cls_bwd_kernel(const float* __restrict__ F,
                                                                    const float* __restrict__ W,
                                                                    const float* __restrict__ G,
                                                                    float* __restrict__ dF, float* __restrict__ dW,
                                                                    float* __restrict__ db, PalRng rng, int N, int R,
                                                                    int K) {
  extern __shared__ float s_g[];                       // [32][ldg]
  const int KT = (K + 15) / 16, ldg = KT * 16 + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = (blockIdx.x * CB_WAVES + wave) * 16;
  uint32_t k0 = 0, k1 = 0;
  if (rng.train) rng_key_dev_x(rng.seed, rng.offset, rng.thresh, k0, k1);
  if (blockIdx.x == 0) {
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
      float s = 0.f;
      for (int n = 0; n < N; ++n) s += G[(size_t)n * K + k];
      db[k] = s;
    }
  }
  for (int nb = 0; nb < N; nb += 32) {
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * ldg; i += blockDim.x) {
      const int nn = i / ldg, k = i - nn * ldg;
      const int n = nb + nn;
      s_g[i] = (n < N && k < K) ? G[(size_t)n * K + k] : 0.f;
    }
    __syncthreads();
    if (r0 >= R) continue;                             // wave-uniform; no barrier below
    // dFd for 32 images x 16 rows
    {
      f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
      const int r = r0 + (lane & 15);
      const float* wrow = W + (size_t)(r < R ? r : 0) * K;
      for (int kb = 0; kb < KT * 16; kb += 4) {
        const int k = kb + (lane >> 4);
        const float a0 = s_g[(lane & 15) * ldg + k];
        const float a1 = s_g[(16 + (lane & 15)) * ldg + k];
        const float b = (r < R && k < K) ? wrow[k] : 0.f;
        d0 = mfma16(a0, b, d0);
        d1 = mfma16(a1, b, d1);
      }
      if (r < R) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int na = nb + 4 * (lane >> 4) + q, nb2 = na + 16;
          if (na < N) dF[(size_t)na * R + r] = d0[q] * keep_scale(rng, k0, k1, (uint64_t)na * R + r);
          if (nb2 < N) dF[(size_t)nb2 * R + r] = d1[q] * keep_scale(rng, k0, k1, (uint64_t)nb2 * R + r);
        }
      }
    }
    // dW for 16 rows x K
    {
      float fa[8];
      const int r = r0 + (lane & 15);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int n = nb + 4 * s + (lane >> 4);
        fa[s] = (n < N && r < R) ? F[(size_t)n * R + r] * keep_scale(rng, k0, k1, (uint64_t)n * R + r) : 0.f;
      }
      for (int kt = 0; kt < KT; ++kt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const float b = s_g[(4 * s + (lane >> 4)) * ldg + kt * 16 + (lane & 15)];
          acc = mfma16(fa[s], b, acc);
        }
        const int k = kt * 16 + (lane & 15);
        if (k < K) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rw = r0 + 4 * (lane >> 4) + q;
            if (rw < R) {
              float* d = dW + (size_t)rw * K + k;
              *d = nb == 0 ? acc[q] : *d + acc[q];
            }
          }
        }
      }
    }
  }
}

template <typename T, int MT>
void launch_pool_fwd(dim3 grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* X, const float* Pl,
                     float* F, const PalMaps& mp, int P, int C) {
  launch_ev(pal_pool_fwd_kernel<T, MT>, grid, dim3(64 * PAL_WAVES), 0, st, e0, e1, static_cast<const T*>(X), Pl, F,
            mp, P, C, 1.0f / (float)P);
}
template <typename T, int MT, bool ACC>
void launch_pool_bwd(dim3 grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* X, const float* Pl,
                     const float* dF, void* dX, float* dApart, const PalMaps& mp, int N, int P, int C) {
  launch_ev(pal_pool_bwd_kernel<T, MT, ACC>, grid, dim3(64 * PAL_WAVES), 0, st, e0, e1, static_cast<const T*>(X),
            Pl, dF, static_cast<T*>(dX), dApart, mp, N, P, C, 1.0f / (float)P);
}

template <typename T>
void dispatch_pool_fwd(dim3 grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* X, const float* Pl,
                       float* F, const PalMaps& mp, int P, int C) {
  if (mp.M <= 4) launch_pool_fwd<T, 4>(grid, st, e0, e1, X, Pl, F, mp, P, C);
  else if (mp.M <= 8) launch_pool_fwd<T, 8>(grid, st, e0, e1, X, Pl, F, mp, P, C);
  else if (mp.M <= 17) launch_pool_fwd<T, 17>(grid, st, e0, e1, X, Pl, F, mp, P, C);
  else launch_pool_fwd<T, PAL_MAXM>(grid, st, e0, e1, X, Pl, F, mp, P, C);
}
template <typename T, bool ACC>
void dispatch_pool_bwd(dim3 grid, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* X, const float* Pl,
                       const float* dF, void* dX, float* dApart, const PalMaps& mp, int N, int P, int C) {
  if (mp.M <= 4) launch_pool_bwd<T, 4, ACC>(grid, st, e0, e1, X, Pl, dF, dX, dApart, mp, N, P, C);
  else if (mp.M <= 8) launch_pool_bwd<T, 8, ACC>(grid, st, e0, e1, X, Pl, dF, dX, dApart, mp, N, P, C);
  else if (mp.M <= 17) launch_pool_bwd<T, 17, ACC>(grid, st, e0, e1, X, Pl, dF, dX, dApart, mp, N, P, C);
  else launch_pool_bwd<T, PAL_MAXM, ACC>(grid, st, e0, e1, X, Pl, dF, dX, dApart, mp, N, P, C);
}

// workspace: forward = per-slab partial logits [nslab][N][K] at 0; backward = dF [N][M*C] at 0, then the per-slab
// dA partials [C/256][N][P][M] at dA_off.  The two calls may share one buffer.
struct PalPlan {
  size_t dA_off, total;
};
PalPlan pal_plan(int N, int P, int C, int M, int K) {
  PalPlan p;
  const size_t R = (size_t)M * C;
  const size_t nslab_cls = (R + CLS_ROWS - 1) / CLS_ROWS, nslab_pool = (size_t)(C + PAL_SLAB - 1) / PAL_SLAB;
  const size_t fwd = align_up(nslab_cls * N * K * sizeof(float), 256);
  p.dA_off = align_up((size_t)N * R * sizeof(float), 256);
  const size_t bwd = p.dA_off + align_up(nslab_pool * N * P * M * sizeof(float), 256);
  p.total = fwd > bwd ? fwd : bwd;
  return p;
}

// dX: the backward call's gradient buffer (stored with X's vector width); NULL in the forward call
int pal_check(const char* fn, const void* X, const void* dX, const float* Pl, const int32_t* sel, int n_sel,
              int avged, const float* W, const void* ws, int N, int P, int C, int J, int K, unsigned flags,
              float keep_prob, uint64_t seed, int dtype, PalMaps* mp) {
  if (!X || !Pl || !W || !ws || (n_sel > 0 && !sel)) {
    set_error("%s: null pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (N <= 0 || P <= 0 || C <= 0 || J <= 0 || K <= 0 || n_sel < 0) {
    set_error("%s: non-positive dimension N=%d P=%d C=%d J=%d K=%d n_sel=%d", fn, N, P, C, J, K, n_sel);
    return APA_ERR_INVALID_ARG;
  }
  if (dtype != APA_DTYPE_F32 && dtype != APA_DTYPE_BF16) {
    set_error("%s: unknown dtype %d", fn, dtype);
    return APA_ERR_INVALID_ARG;
  }
  if ((flags & APA_FLAG_TRAIN) && !(keep_prob > 0.f && keep_prob <= 1.f)) {
    set_error("%s: keep_prob=%g outside (0,1]", fn, (double)keep_prob);
    return APA_ERR_INVALID_ARG;
  }
  if ((flags & APA_FLAG_TRAIN) && (flags & APA_FLAG_RNG_EXTERNAL) && seed == 0) {
    set_error("%s: APA_FLAG_RNG_EXTERNAL with a null keep-bit image (seed == 0)", fn);
    return APA_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_sel; ++i) {
    if (sel[i] < 0 || sel[i] >= J) {
      set_error("%s: sel[%d]=%d outside [0, J=%d)", fn, i, sel[i], J);
      return APA_ERR_INVALID_ARG;
    }
  }
  const int M = n_sel + (avged ? 1 : 0) + 1;
  if (M > PAL_MAXM || C % 4 != 0 || K > PAL_MAXK || (flags & (APA_FLAG_RNG_DEVICE | APA_FLAG_RELU_INPUT))) {
    set_error("%s: built for M <= %d maps, C a multiple of 4, K <= %d, without APA_FLAG_RNG_DEVICE / "
              "APA_FLAG_RELU_INPUT (M=%d C=%d K=%d flags=%u)", fn, PAL_MAXM, PAL_MAXK, M, C, K, flags);
    return APA_ERR_UNSUPPORTED;
  }
  if (flags & APA_FLAG_FROZEN_INPUT) {   // the pose-heatmap attention head has no arm without the dX stores
    set_error("%s: APA_FLAG_FROZEN_INPUT is not served by the pose-heatmap attention head: run without the flag", fn);
    return APA_ERR_UNSUPPORTED;
  }
  const uintptr_t align = dtype == APA_DTYPE_F32 ? 15 : 7;
  if (reinterpret_cast<uintptr_t>(X) & align) {
    set_error("%s: X must be %d-byte aligned", fn, (int)align + 1);
    return APA_ERR_UNSUPPORTED;
  }
  if (dX && (reinterpret_cast<uintptr_t>(dX) & align)) {
    set_error("%s: dX must be %d-byte aligned, like X", fn, (int)align + 1);
    return APA_ERR_UNSUPPORTED;
  }
  if (reinterpret_cast<uintptr_t>(ws) & 15) {             // dF is read from it as float4
    set_error("%s: the workspace must be 16-byte aligned", fn);
    return APA_ERR_UNSUPPORTED;
  }
  mp->M = M; mp->nsel = n_sel; mp->avged = avged ? 1 : 0; mp->J = J;
  for (int i = 0; i < PAL_MAXM; ++i) mp->sel[i] = i < n_sel ? sel[i] : 0;
  return APA_OK;
}

PalRng pal_rng(unsigned flags, float keep_prob, uint64_t seed, uint64_t offset) {
  PalRng r;
  const RngKeyArgs k = rng_resolve(flags, keep_prob, seed, offset);
  r.thresh = k.thresh; r.seed = k.seed; r.offset = k.offset;
  r.train = (flags & APA_FLAG_TRAIN) ? 1 : 0;
  r.inv_keep = r.train ? 1.0f / keep_prob : 1.0f;
  return r;
}

}  // namespace
}  // namespace apa

using namespace apa;

extern "C" size_t apa_pose_att_logits_workspace_bytes(int N, int P, int C, int M, int K) {
  if (N <= 0 || P <= 0 || C <= 0 || M <= 0 || K <= 0) return 0;
  return pal_plan(N, P, C, M, K).total;
}

extern "C" int apa_pose_att_logits_fwd_ex(const apa_hooks* hooks, const void* X, const float* Pl, const int32_t* sel, int n_sel, int avged,
                                          const float* W, const float* b, float* F, float* logits, void* ws,
                                          size_t ws_bytes, int N, int P, int C, int J, int K, unsigned flags,
                                          float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  const char* fn = "apa_pose_att_logits_fwd";
  if (!b || !F || !logits) {
    set_error("%s: null pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  PalMaps mp;
  int rc = pal_check(fn, X, nullptr, Pl, sel, n_sel, avged, W, ws, N, P, C, J, K, flags, keep_prob, seed, dtype,
                     &mp);
  if (rc != APA_OK) return rc;
  const PalPlan plan = pal_plan(N, P, C, mp.M, K);
  if (ws_bytes < plan.total) {
    set_error("%s: workspace too small (%zu < %zu)", fn, ws_bytes, plan.total);
    return APA_ERR_WORKSPACE;
  }
  const Hooks hk(hooks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int R = mp.M * C;
  const dim3 pgrid((C + PAL_SLAB - 1) / PAL_SLAB, N);
  if (dtype == APA_DTYPE_BF16) dispatch_pool_fwd<bf16_t>(pgrid, st, hk.fwd0, hk.fwd1, X, Pl, F, mp, P, C);
  else dispatch_pool_fwd<float>(pgrid, st, hk.fwd0, hk.fwd1, X, Pl, F, mp, P, C);
  APA_LAUNCH_CHECK("pal_pool_fwd_kernel");
  const int nslab = (R + CLS_ROWS - 1) / CLS_ROWS;
  float* part = static_cast<float*>(ws);
  launch_ev(pal_cls_fwd_kernel, dim3(nslab), dim3(64 * CLS_WAVES), 0, st, hk.bwd0, nullptr, F, W, part,
            pal_rng(flags, keep_prob, seed, offset), N, R, K);
  APA_LAUNCH_CHECK("pal_cls_fwd_kernel");
  launch_ev(pal_cls_reduce_kernel, dim3((N * K + 255) / 256), dim3(256), 0, st, nullptr, hk.bwd1, part, b, logits,
            N, K, nslab);
  APA_LAUNCH_CHECK("pal_cls_reduce_kernel");
  return APA_OK;
}

extern "C" int apa_pose_att_logits_fwd(const void* X, const float* Pl, const int32_t* sel, int n_sel, int avged,
                                       const float* W, const float* b, float* F, float* logits, void* ws,
                                       size_t ws_bytes, int N, int P, int C, int J, int K, unsigned flags,
                                       float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  return apa_pose_att_logits_fwd_ex(nullptr, X, Pl, sel, n_sel, avged, W, b, F, logits, ws, ws_bytes, N, P, C, J, K, flags,
                                    keep_prob, seed, offset, dtype, stream);
}

extern "C" int apa_pose_att_logits_bwd_ex(const apa_hooks* hooks, const void* X, const float* Pl, const int32_t* sel, int n_sel, int avged,
                                          const float* W, const float* F, const float* G, void* dX,
                                          int accumulate_dX, float* dPl, float* dW, float* db, void* ws,
                                          size_t ws_bytes, int N, int P, int C, int J, int K, unsigned flags,
                                          float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  const char* fn = "apa_pose_att_logits_bwd";
  if (!F || !G || !dX || !dPl || !dW || !db) {
    set_error("%s: null pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  PalMaps mp;
  int rc = pal_check(fn, X, dX, Pl, sel, n_sel, avged, W, ws, N, P, C, J, K, flags, keep_prob, seed, dtype, &mp);
  if (rc != APA_OK) return rc;
  const PalPlan plan = pal_plan(N, P, C, mp.M, K);
  if (ws_bytes < plan.total) {
    set_error("%s: workspace too small (%zu < %zu)", fn, ws_bytes, plan.total);
    return APA_ERR_WORKSPACE;
  }
  const Hooks hk(hooks);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int R = mp.M * C;
  float* dF = static_cast<float*>(ws);
  float* dA = reinterpret_cast<float*>(static_cast<char*>(ws) + plan.dA_off);
  const int KT = (K + 15) / 16;
  const size_t shm = (size_t)32 * (KT * 16 + 1) * sizeof(float);
  const int rows_per_block = 16 * CB_WAVES;
  launch_ev(pal_cls_bwd_kernel, dim3((R + rows_per_block - 1) / rows_per_block), dim3(64 * CB_WAVES), shm, st,
            hk.bwd0, hk.bwd1, F, W, G, dF, dW, db, pal_rng(flags, keep_prob, seed, offset), N, R, K);
  APA_LAUNCH_CHECK("pal_cls_bwd_kernel");
  const dim3 pgrid((C + PAL_SLAB - 1) / PAL_SLAB, N);
  if (dtype == APA_DTYPE_BF16) {
    if (accumulate_dX) dispatch_pool_bwd<bf16_t, true>(pgrid, st, hk.fwd0, nullptr, X, Pl, dF, dX, dA, mp, N, P, C);
    else dispatch_pool_bwd<bf16_t, false>(pgrid, st, hk.fwd0, nullptr, X, Pl, dF, dX, dA, mp, N, P, C);
  } else {
    if (accumulate_dX) dispatch_pool_bwd<float, true>(pgrid, st, hk.fwd0, nullptr, X, Pl, dF, dX, dA, mp, N, P, C);
    else dispatch_pool_bwd<float, false>(pgrid, st, hk.fwd0, nullptr, X, Pl, dF, dX, dA, mp, N, P, C);
  }
  APA_LAUNCH_CHECK("pal_pool_bwd_kernel");
  const size_t NP = (size_t)N * P;
  size_t nb = (NP * J + 255) / 256;
  if (nb > 4096) nb = 4096;
  launch_ev(pal_fold_kernel, dim3((unsigned)nb), dim3(256), 0, st, nullptr, hk.fwd1, dA, dPl, mp, (int)NP, (int)pgrid.x);
  APA_LAUNCH_CHECK("pal_fold_kernel");
  return APA_OK;
}

extern "C" int apa_pose_att_logits_bwd(const void* X, const float* Pl, const int32_t* sel, int n_sel, int avged,
                                       const float* W, const float* F, const float* G, void* dX, int accumulate_dX,
                                       float* dPl, float* dW, float* db, void* ws, size_t ws_bytes, int N, int P,
                                       int C, int J, int K, unsigned flags, float keep_prob, uint64_t seed,
                                       uint64_t offset, int dtype, void* stream) {
  return apa_pose_att_logits_bwd_ex(nullptr, X, Pl, sel, n_sel, avged, W, F, G, dX, accumulate_dX, dPl, dW, db, ws, ws_bytes,
                                    N, P, C, J, K, flags, keep_prob, seed, offset, dtype, stream);
}
