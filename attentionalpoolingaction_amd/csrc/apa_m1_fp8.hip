// apa_m1_fp8.hip -- the two streaming passes of the factorised (M == 1) head over an FP8 feature cache
// (apa.h: APA_DTYPE_FP8_E4M3; M1_POOL_FP8), the fourth pooling family beside apa_m1_stream / _vec / _generic.hip.
//
// A cache is frozen by construction: fused attention (Xatt == X), identity or ReLU, no dX.  Both passes read the codes
// once, 16 per lane and load (a 2048-channel pixel row is two wave loads), decode them with v_cvt_pk_f32_fp8 and work
// on the UNSCALED values q; the image's scale s_n enters once per pixel or once per block:
//   forward   Z_p = s_n (q_p . wa) + ba     pacc[blk] = s_n sum_p A_p mask/keep q_p     pstat[blk] = sum_p A_p
//   backward  dA_p = (s_n/keep (q_p mask . dz) + G . bt) / P     pdwa[blk] = s_n sum_p dZ_p q_p     pdba[blk] = sum_p dZ_p
// Same block / pixel ownership and the same per-block partials as the other families (M1Plan), so the partial merge,
// the logits product with its fused losses, the head kernel, the column sum and the counter bump behind them run
// unchanged.  The dropout mask is the counter hash over the flat [N,P,C] index (apa_dropout_mask); the backward pass
// hashes again.
//
// One wave owns a pixel (no block barrier per pixel); the four waves of a block take the block's pixels interleaved
// and are merged through LDS once, in wave order.  A lane owns the vectors lane + 64 j, j < NV, of every row; NV is a
// template parameter so that the C channel accumulators and the operand row (wa / dz) stay in registers.
#include <math.h>

#include "apa_device.h"
#include "apa_fp8.h"
#include "apa_internal.h"

namespace apa {

namespace {
// hides the pointer's provenance from alias analysis, so that a chunk's loads stay where the source puts them: in
// front of the arithmetic of the chunk before it (apa_m1_stream.hip)
__device__ __forceinline__ const uint8_t* opaque_codes(const uint8_t* p) {
  typedef const uint8_t __attribute__((address_space(1))) * gp;
  gp g = (gp)p;
  asm volatile("" : "+s"(g));
  return (const uint8_t*)g;
}

// pixels per chunk and blocks per CU: up to 2048 channels two blocks (eight waves) share a CU's registers
constexpr int pix_per_chunk(int NV) { return NV == 1 ? 4 : (NV == 2 ? 2 : 1); }
constexpr int blocks_per_cu(int NV) { return NV <= 2 ? 2 : 1; }

// This wave's pixels: p_begin + wave + 4 i.  Chunk ch holds i = ch PIX .. ch PIX + PIX - 1; a slot past the block's
// end re-reads the block's last pixel (an L1 hit) and carries weight 0.
template <int NV, int PIX>
__device__ __forceinline__ void load_chunk(uint4 (&xr)[PIX][NV], const uint8_t* xim, int p0, int p_last, int C,
                                           const int (&voff)[NV]) {
#pragma unroll
  for (int i = 0; i < PIX; ++i) {
    const uint8_t* row = xim + (size_t)min(p0 + 4 * i, p_last) * C;
#pragma unroll
    for (int j = 0; j < NV; ++j) xr[i][j] = ld16(row + voff[j]);
  }
}

// the block's per-wave channel rows summed in wave order, ((w0 + w1) + w2) + w3, and scaled stores into dst: one [C]
// row of LDS, three barriers.  acc is scaled by `s` first.
template <int NV>
__device__ __forceinline__ void merge_waves(float (&acc)[NV * 16], float s, float* sm, float* dst, const int (&voff)[NV],
                                            const bool (&active)[NV], int wave) {
#pragma unroll
  for (int i = 0; i < NV * 16; ++i) acc[i] *= s;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        if (!active[j]) continue;
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
          float4 r = make_float4(acc[j * 16 + e], acc[j * 16 + e + 1], acc[j * 16 + e + 2], acc[j * 16 + e + 3]);
          float* at = (w == 3 ? dst : sm) + voff[j] + e;
          if (w > 0) {
            const float4 o = *reinterpret_cast<const float4*>(sm + voff[j] + e);
            r.x = o.x + r.x; r.y = o.y + r.y; r.z = o.z + r.z; r.w = o.w + r.w;
          }
          *reinterpret_cast<float4*>(at) = r;
        }
      }
    }
    if (w < 3) __syncthreads();
  }
}

// GATHER: the gathered instances (apa_device.h: M1Gather; the plain ones take an empty M1NoGather) read the codes and
// the scale of cache image index[n]; the launchers below name every instance from m1_train_gather's tags
template <int NV, bool TRAIN, bool GATHER = false>
__global__ __launch_bounds__(256, blocks_per_cu(NV)) void m1f_pool_fwd_kernel(
    const uint8_t* __restrict__ X, const float* __restrict__ scale, const float* __restrict__ Wa,
    const float* __restrict__ ba, float* __restrict__ att, float* __restrict__ pacc, float* __restrict__ pstat, int P,
    int S, int C, int act, float inv_keep, uint32_t thresh, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, M1GatherArg<GATHER> g) {
  constexpr int PIX = pix_per_chunk(NV);
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [C] merge row, then 4 per-wave sums
  const int blk = blockIdx.x, n = blk / S, s = blk % S;
  const int src = GATHER ? m1_src_image(n, g) : n;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p_begin = (int)(((long)s * P) / S), p_end = (int)(((long)(s + 1) * P) / S);
  const int p_last = p_end - 1;
  const int nvec = C / 16;
  int voff[NV];
  bool active[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    active[j] = lane + 64 * j < nvec;
    voff[j] = min(lane + 64 * j, nvec - 1) * 16;   // idle lanes shadow the last vector, operand 0
  }
  const int npw = p_begin + wave < p_end ? (p_end - p_begin - wave + 3) / 4 : 0;
  const int nchunk = (npw + PIX - 1) / PIX;
  const int pw0 = p_begin + wave;

  const uint8_t* xim = opaque_codes(X + (size_t)src * P * C);
  uint4 xr[2][PIX][NV];
  load_chunk<NV, PIX>(xr[0], xim, pw0, p_last, C, voff);
  // L2 hits, issued in the shadow of the first chunk's loads
  float wa[NV * 16], acc[NV * 16];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int e = 0; e < 16; e += 4) {
      const float4 w = *reinterpret_cast<const float4*>(Wa + voff[j] + e);
      wa[j * 16 + e] = active[j] ? w.x : 0.f; wa[j * 16 + e + 1] = active[j] ? w.y : 0.f;
      wa[j * 16 + e + 2] = active[j] ? w.z : 0.f; wa[j * 16 + e + 3] = active[j] ? w.w : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < NV * 16; ++i) acc[i] = 0.f;
  const float bias = ba[0], sn = scale[src];
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset_dev ? *offset_dev : offset, k0, k1);
  float a_sum = 0.f;
  float* att_im = att + (size_t)n * P;

  for (int ch = 0; ch < nchunk; ch += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u > 0 && ch + u >= nchunk) break;
      load_chunk<NV, PIX>(xr[u ^ 1], xim, pw0 + 4 * PIX * (ch + u + 1), p_last, C, voff);
#pragma unroll
      for (int i = 0; i < PIX; ++i) {
        const int p = pw0 + 4 * (PIX * (ch + u) + i);
        const bool valid = p < p_end;
        float q[NV * 16];
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          fp8x16_decode(xr[u][i][j], q + j * 16);
#pragma unroll
          for (int e = 0; e < 16; e += 2) {
            d0 = fmaf(q[j * 16 + e], wa[j * 16 + e], d0);
            d1 = fmaf(q[j * 16 + e + 1], wa[j * 16 + e + 1], d1);
          }
        }
        const float zl = fmaf(sn, wave_sum(d0 + d1), bias);
        float a = act == M1_ACT_RELU ? fmaxf(zl, 0.f) : zl;
        if (valid && lane == 0) att_im[p] = a;
        a = valid ? a : 0.f;
        a_sum += a;
        const float ak = TRAIN ? a * inv_keep : a;
        const uint64_t ebase = ((uint64_t)n * P + min(p, p_last)) * C;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
#pragma unroll
          for (int e = 0; e < 16; e += 2) {
            float m0 = 1.f, m1 = 1.f;
            if (TRAIN) rng_keep2(ebase + voff[j] + e, k0, k1, thresh, m0, m1);
            acc[j * 16 + e] = fmaf(ak * m0, q[j * 16 + e], acc[j * 16 + e]);
            acc[j * 16 + e + 1] = fmaf(ak * m1, q[j * 16 + e + 1], acc[j * 16 + e + 1]);
          }
        }
      }
    }
  }

  float* sm_stat = sm + C;
  if (lane == 0) sm_stat[wave] = a_sum;
  merge_waves<NV>(acc, sn, sm, pacc + (size_t)blk * C, voff, active, wave);   // (its barriers publish sm_stat)
  m1_gather_note(n, s == 0 && threadIdx.x == 0, g);
  if (threadIdx.x == 192) {
    pstat[blk * 4 + 0] = 0.f;
    pstat[blk * 4 + 1] = 0.f;
    pstat[blk * 4 + 2] = (sm_stat[0] + sm_stat[1]) + (sm_stat[2] + a_sum);
    pstat[blk * 4 + 3] = 0.f;
  }
}

template <int NV, bool TRAIN, bool GATHER = false>
__global__ __launch_bounds__(256, blocks_per_cu(NV)) void m1f_bwd_main_kernel(
    const uint8_t* __restrict__ X, const float* __restrict__ scale, const float* __restrict__ att,
    const float* __restrict__ dz, const float* __restrict__ G, const float* __restrict__ bt,
    const float* __restrict__ sn_pre, float* __restrict__ pdwa, float* __restrict__ pdba, int P, int S, int C, int K,
    int act, float inv_keep, uint32_t thresh, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, M1GatherArg<GATHER> g) {
  constexpr int PIX = pix_per_chunk(NV);
  extern __shared__ __attribute__((aligned(16))) float sm[];   // [C] merge row, then 4 per-wave sums
  const int blk = blockIdx.x, n = blk / S, s = blk % S;
  const int src = GATHER ? m1_src_image(n, g) : n;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p_begin = (int)(((long)s * P) / S), p_end = (int)(((long)(s + 1) * P) / S);
  const int p_last = p_end - 1;
  const int nvec = C / 16;
  int voff[NV];
  bool active[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    active[j] = lane + 64 * j < nvec;
    voff[j] = min(lane + 64 * j, nvec - 1) * 16;
  }
  const int npw = p_begin + wave < p_end ? (p_end - p_begin - wave + 3) / 4 : 0;
  const int nchunk = (npw + PIX - 1) / PIX;
  const int pw0 = p_begin + wave;

  const uint8_t* xim = opaque_codes(X + (size_t)src * P * C);
  uint4 xr[2][PIX][NV];
  load_chunk<NV, PIX>(xr[0], xim, pw0, p_last, C, voff);
  float dzr[NV * 16], dwa[NV * 16];
  const float* dzn = dz + (size_t)n * C;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
#pragma unroll
    for (int e = 0; e < 16; e += 4) {
      const float4 w = *reinterpret_cast<const float4*>(dzn + voff[j] + e);
      dzr[j * 16 + e] = active[j] ? w.x : 0.f; dzr[j * 16 + e + 1] = active[j] ? w.y : 0.f;
      dzr[j * 16 + e + 2] = active[j] ? w.z : 0.f; dzr[j * 16 + e + 3] = active[j] ? w.w : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < NV * 16; ++i) dwa[i] = 0.f;
  const float sc = scale[src];
  float gb;   // G[n,:] . bt
  if (sn_pre) {
    gb = sn_pre[n];
  } else {
    gb = 0.f;
    for (int k = lane; k < K; k += 64) gb = fmaf(G[(size_t)n * K + k], bt[k], gb);
    gb = wave_sum(gb);
  }
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset_dev ? *offset_dev : offset, k0, k1);
  const float invP = 1.0f / (float)P;
  const float ts = TRAIN ? sc * inv_keep : sc;
  const float* att_im = att + (size_t)n * P;
  float dba = 0.f;

  for (int ch = 0; ch < nchunk; ch += 2) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (u > 0 && ch + u >= nchunk) break;
      load_chunk<NV, PIX>(xr[u ^ 1], xim, pw0 + 4 * PIX * (ch + u + 1), p_last, C, voff);
#pragma unroll
      for (int i = 0; i < PIX; ++i) {
        const int p = pw0 + 4 * (PIX * (ch + u) + i);
        const bool valid = p < p_end;
        const float a = att_im[min(p, p_last)];
        const uint64_t ebase = ((uint64_t)n * P + min(p, p_last)) * C;
        float q[NV * 16];
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          fp8x16_decode(xr[u][i][j], q + j * 16);
#pragma unroll
          for (int e = 0; e < 16; e += 2) {
            float m0 = 1.f, m1 = 1.f;
            if (TRAIN) rng_keep2(ebase + voff[j] + e, k0, k1, thresh, m0, m1);
            d0 = fmaf(q[j * 16 + e] * m0, dzr[j * 16 + e], d0);
            d1 = fmaf(q[j * 16 + e + 1] * m1, dzr[j * 16 + e + 1], d1);
          }
        }
        const float dA = (wave_sum(d0 + d1) * ts + gb) * invP;
        float dZ = act == M1_ACT_RELU ? (a > 0.f ? dA : 0.f) : dA;
        dZ = valid ? dZ : 0.f;
        dba += dZ;
#pragma unroll
        for (int i2 = 0; i2 < NV * 16; ++i2) dwa[i2] = fmaf(dZ, q[i2], dwa[i2]);
      }
    }
  }

  float* sm_stat = sm + C;
  if (lane == 0) sm_stat[wave] = dba;
  merge_waves<NV>(dwa, sc, sm, pdwa + (size_t)blk * C, voff, active, wave);
  if (threadIdx.x == 192) pdba[blk] = (sm_stat[0] + sm_stat[1]) + (sm_stat[2] + dba);
}

template <typename F> int by_nv(int C, F&& go) {
  switch (m1f_vectors_per_lane(C)) {
    case 1: return go(std::integral_constant<int, 1>{});
    case 2: return go(std::integral_constant<int, 2>{});
    case 4: return go(std::integral_constant<int, 4>{});
    default: return go(std::integral_constant<int, 8>{});
  }
}
}  // namespace

// NV of the instance that serves C: the 16-code vectors of a row over the 64 lanes, rounded up to 1 / 2 / 4 / 8
int m1f_vectors_per_lane(int C) {
  const int nv = (C / 16 + 63) / 64;
  return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : 8));
}

// C a whole number of 16-code vectors, at most eight per lane of the wave that owns a pixel row
bool m1f_supported(int C) { return C >= 16 && C % 16 == 0 && C <= M1F_MAX_C; }

int m1f_launch_pool_fwd(const M1Call& c, const M1Fwd& io) {
  if (M1Trace* t = m1_trace()) t->pool_fwd = M1_POOL_FP8;
  const uint8_t* X = static_cast<const uint8_t*>(io.X);
  // (a gathered call: the scales lie behind the codes of all c.T images of the cache)
  const float* scale = reinterpret_cast<const float*>(X + fp8_scale_offset(c.T, c.P, c.C));
  const size_t shm = (size_t)c.C * 4 + 16;
  by_nv(c.C, [&](auto NV) -> int {
    return m1_train_gather(c, [&](auto TR, auto G) {
      constexpr bool g = decltype(G)::value;
      launch_ev(m1f_pool_fwd_kernel<decltype(NV)::value, decltype(TR)::value, g>, dim3(c.pl.nblk), dim3(256), shm, c.st,
                c.ev0, c.ev1, X, scale, io.Wa, io.ba, io.att, c.pacc, c.pstat, c.P, c.pl.S, c.C, c.pool_act, c.inv_keep,
                c.key.thresh, c.key.seed, c.key.offset, c.key.offset_dev, m1_gather_arg<g>(c));
      return APA_OK;
    });
  });
  APA_LAUNCH_CHECK("m1f_pool_fwd_kernel");
  return APA_OK;
}

int m1f_launch_bwd_main(const M1Call& c, const M1Bwd& io) {
  if (M1Trace* t = m1_trace()) t->pool_bwd = M1_POOL_FP8;
  const uint8_t* X = static_cast<const uint8_t*>(io.X);
  const float* scale = reinterpret_cast<const float*>(X + fp8_scale_offset(c.T, c.P, c.C));
  const size_t shm = (size_t)c.C * 4 + 16;
  by_nv(c.C, [&](auto NV) -> int {
    return m1_train_gather(c, [&](auto TR, auto G) {
      constexpr bool g = decltype(G)::value;
      launch_ev(m1f_bwd_main_kernel<decltype(NV)::value, decltype(TR)::value, g>, dim3(c.pl.nblk), dim3(256), shm, c.st,
                c.ev0, c.ev1, X, scale, io.att, c.dz, io.G, io.bt, c.sn, c.pdwa, c.pdba, c.P, c.pl.S, c.C, c.K, c.act,
                c.inv_keep, c.key.thresh, c.key.seed, c.key.offset, c.key.offset_dev, m1_gather_arg<g>(c));
      return APA_OK;
    });
  });
  APA_LAUNCH_CHECK("m1f_bwd_main_kernel");
  return APA_OK;
}

}  // namespace apa
