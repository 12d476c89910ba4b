// apa_m1_vec.hip -- the two streaming passes of the factorised (M == 1) head for the narrow powers of two
// (C = 256 / 512 fp32, 512 / 1024 bf16), register-resident per-pixel shape.
//
// Reference semantics and closed forms: the top of apa_m1.hip.
//
// Kernel shape: one wave owns whole pixels.  A pixel's C channels live in the wave's registers
// (C/64 per lane, loaded as 16-byte vectors -> 1 KiB per wave-instruction, fully coalesced), so
// the C-long dot product is a DPP wave reduction and the accumulation into z / dX / dwa needs no
// second look at memory.  The next pixel's loads are issued before the current one is consumed.
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

// --------------------------------------------------------------------------------------------
// F1: pooling pass.  grid = N*S blocks of 256 threads; block (n,s) owns pixels
// [s*ppb, min(P,(s+1)*ppb)) of image n, wave w takes every 4th pixel.
//   FUSED  : Z = x.wa + ba computed in-line (Xatt == X, cfg 002); softmax handled on-line
//            (running max / sum, flash-style) so X is still read once.
//   !FUSED : A[n,p] given (already activated / soft-maxed) in att.
// Outputs: att (FUSED: id/relu -> final A, softmax -> raw Z, normalised in F2),
//          pacc[blk][C] partial sum_p A*Xt, pstat[blk][4] = {m, l, asum, -}.
// --------------------------------------------------------------------------------------------
// GATHER: the gathered instances (apa_device.h: M1Gather; the plain ones take an empty M1NoGather), FUSED or -- the cfg
// 003 cached steps, whose attention map has the batch shape -- not; the launchers below name every instance from
// m1_pool_form's tags
template <typename T, int VEC, bool FUSED, bool TRAIN, bool GATHER = false>
__global__ __launch_bounds__(256) void m1_pool_fwd_kernel(
    const T* __restrict__ X, const float* __restrict__ Wa, const float* __restrict__ ba,
    float* __restrict__ att, float* __restrict__ pacc, float* __restrict__ pstat, int P, int S,
    int act, float inv_keep, uint32_t thresh, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, M1GatherArg<GATHER> g) {
  constexpr int EPV = Vec<T>::EPV;
  constexpr int EPL = VEC * EPV;
  constexpr int C = EPL * 64;
  __shared__ __attribute__((aligned(16))) float sm_acc[4 * C];
  __shared__ float sm_stat[4 * 4];
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset_dev ? *offset_dev : offset, k0, k1);

  const int nblk = gridDim.x;
  const int blk = xcd_remap(blockIdx.x, nblk);
  const int n = blk / S, s = blk % S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p_begin = (int)(((long)s * P) / S);        // balanced split: sizes differ by <= 1
  const int p_end = (int)(((long)(s + 1) * P) / S);

  float wa[FUSED ? EPL : 1];
  float bias = 0.f;
  if (FUSED) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int c0 = j * 64 * EPV + lane * EPV;
#pragma unroll
      for (int e = 0; e < EPV; e += 4) {
        const float4 w = *reinterpret_cast<const float4*>(Wa + c0 + e);
        wa[j * EPV + e + 0] = w.x; wa[j * EPV + e + 1] = w.y;
        wa[j * EPV + e + 2] = w.z; wa[j * EPV + e + 3] = w.w;
      }
    }
    bias = ba[0];
  }

  float acc[EPL];
#pragma unroll
  for (int i = 0; i < EPL; ++i) acc[i] = 0.f;
  float m_run = -INFINITY, l_run = 0.f, a_sum = 0.f;

  const T* xim = X + (size_t)(GATHER ? m1_src_image(n, g) : n) * P * C;
  float* att_im = att + (size_t)n * P;

  uint4 cur[VEC], nxt[VEC];
  int p = p_begin + wave;
  if (p < p_end) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) cur[j] = ld16(xim + (size_t)p * C + j * 64 * EPV + lane * EPV);
  }
  for (; p < p_end; p += 4) {
    const int pn = p + 4;
    if (pn < p_end) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) nxt[j] = ld16(xim + (size_t)pn * C + j * 64 * EPV + lane * EPV);
    }
    float x[EPL];
#pragma unroll
    for (int j = 0; j < VEC; ++j) Vec<T>::unpack(cur[j], x + j * EPV);

    float a;       // weight applied to this pixel's features
    float scale = 1.f;
    if (FUSED) {
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int i = 0; i < EPL; i += 2) {
        d0 = fmaf(x[i], wa[i], d0);
        d1 = fmaf(x[i + 1], wa[i + 1], d1);
      }
      const float zl = wave_sum(d0 + d1) + bias;
      if (act == M1_ACT_SOFTMAX) {
        const float m_new = fmaxf(m_run, zl);
        scale = expf(m_run - m_new);  // exp(-inf) = 0 on the first pixel
        a = expf(zl - m_new);
        l_run = l_run * scale + a;
        m_run = m_new;
        if (lane == 0) att_im[p] = zl;  // raw logit; normalised by the finalize kernel
      } else {
        a = (act == M1_ACT_RELU) ? fmaxf(zl, 0.f) : zl;
        if (lane == 0) att_im[p] = a;
      }
    } else {
      a = att_im[p];
    }
    a_sum += a;

    if (TRAIN) {
      const uint64_t ebase = ((uint64_t)n * P + p) * C;
      const float ak = a * inv_keep;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const uint64_t e0 = ebase + j * 64 * EPV + lane * EPV;
#pragma unroll
        for (int e = 0; e < EPV; e += 2) {
          float m0, m1;
          rng_keep2(e0 + e, k0, k1, thresh, m0, m1);
          const int i = j * EPV + e;
          acc[i] = fmaf(acc[i], scale, ak * m0 * x[i]);
          acc[i + 1] = fmaf(acc[i + 1], scale, ak * m1 * x[i + 1]);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < EPL; ++i) acc[i] = fmaf(acc[i], scale, a * x[i]);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) cur[j] = nxt[j];
  }

  // ---- combine the 4 waves of the block (fixed order -> deterministic) ----
  if (lane == 0) {
    sm_stat[wave * 4 + 0] = m_run;
    sm_stat[wave * 4 + 1] = l_run;
    sm_stat[wave * 4 + 2] = a_sum;
  }
  __syncthreads();
  float wscale = 1.f, m_blk = 0.f, l_blk = 0.f;
  if (act == M1_ACT_SOFTMAX && FUSED) {
    m_blk = fmaxf(fmaxf(sm_stat[0], sm_stat[4]), fmaxf(sm_stat[8], sm_stat[12]));
    wscale = (m_run == -INFINITY) ? 0.f : expf(m_run - m_blk);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float mw = sm_stat[w * 4];
      l_blk += (mw == -INFINITY) ? 0.f : sm_stat[w * 4 + 1] * expf(mw - m_blk);
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
#pragma unroll
    for (int e = 0; e < EPV; e += 4) {
      const int c0 = j * 64 * EPV + lane * EPV + e;
      const int i = j * EPV + e;
      *reinterpret_cast<float4*>(&sm_acc[wave * C + c0]) =
          make_float4(acc[i] * wscale, acc[i + 1] * wscale, acc[i + 2] * wscale, acc[i + 3] * wscale);
    }
  }
  __syncthreads();
  float* pa = pacc + (size_t)blk * C;
  for (int v = threadIdx.x; v < C / 4; v += 256) {
    const float4 a0 = *reinterpret_cast<const float4*>(&sm_acc[0 * C + v * 4]);
    const float4 a1 = *reinterpret_cast<const float4*>(&sm_acc[1 * C + v * 4]);
    const float4 a2 = *reinterpret_cast<const float4*>(&sm_acc[2 * C + v * 4]);
    const float4 a3 = *reinterpret_cast<const float4*>(&sm_acc[3 * C + v * 4]);
    float4 r;
    r.x = (a0.x + a1.x) + (a2.x + a3.x);
    r.y = (a0.y + a1.y) + (a2.y + a3.y);
    r.z = (a0.z + a1.z) + (a2.z + a3.z);
    r.w = (a0.w + a1.w) + (a2.w + a3.w);
    *reinterpret_cast<float4*>(pa + v * 4) = r;
  }
  m1_gather_note(n, s == 0 && threadIdx.x == 0, g);
  if (threadIdx.x == 0) {
    pstat[blk * 4 + 0] = m_blk;
    pstat[blk * 4 + 1] = l_blk;
    pstat[blk * 4 + 2] = (sm_stat[2] + sm_stat[6]) + (sm_stat[10] + sm_stat[14]);
    pstat[blk * 4 + 3] = 0.f;
  }
}

// --------------------------------------------------------------------------------------------
// B3: backward streaming pass (the dominant kernel: reads X once, writes dX once).
// grid = N*S blocks of 256 threads, same pixel ownership as F1.
// NODX (APA_FLAG_FROZEN_INPUT): nothing is stored through dX (it may be NULL); dZout / pdwa / pdba are formed by the
// same operations in the same order as in the writing arm.
// --------------------------------------------------------------------------------------------
template <typename T, int VEC, bool FUSED, bool TRAIN, bool NODX, bool GATHER = false>
__global__ __launch_bounds__(256) void m1_bwd_main_kernel(
    const T* __restrict__ X, const float* __restrict__ Wa, const float* __restrict__ att,
    const float* __restrict__ dz, const float* __restrict__ zsave, const float* __restrict__ abar,
    const float* __restrict__ G, const float* __restrict__ bt,
    const float* __restrict__ sn_pre, T* __restrict__ dX,
    float* __restrict__ dZout, float* __restrict__ pdwa, float* __restrict__ pdba, int P, int S,
    int K, int act, float inv_keep, uint32_t thresh, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, const float* __restrict__ dA_extra, float extra_scale,
    M1GatherArg<GATHER> g) {
  constexpr int EPV = Vec<T>::EPV;
  constexpr int EPL = VEC * EPV;
  constexpr int C = EPL * 64;
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset_dev ? *offset_dev : offset, k0, k1);
  __shared__ __attribute__((aligned(16))) float sm_acc[FUSED ? 4 * C : 4];
  __shared__ float sm_dba[4];

  const int nblk = gridDim.x;
  const int blk = xcd_remap(blockIdx.x, nblk);
  const int n = blk / S, s = blk % S;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p_begin = (int)(((long)s * P) / S);        // balanced split: sizes differ by <= 1
  const int p_end = (int)(((long)(s + 1) * P) / S);
  const float invP = 1.0f / (float)P;

  // the first pixel's HBM loads go out before anything else; the per-image constants below
  // (L2 hits) are fetched in their shadow
  const T* xim = X + (size_t)(GATHER ? m1_src_image(n, g) : n) * P * C;
  T* dxim = NODX ? nullptr : dX + (size_t)n * P * C;
  const float* att_im = att + (size_t)n * P;
  uint4 cur[VEC], nxt[VEC];
  int p = p_begin + wave;
  if (p < p_end) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) cur[j] = ld16(xim + (size_t)p * C + j * 64 * EPV + lane * EPV);
  }

  // per-image constants, every wave computes them redundantly (a few KB from L2)
  float dzr[EPL];
  float wa[FUSED ? EPL : 1];
  float zdz = 0.f;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int c0 = j * 64 * EPV + lane * EPV;
#pragma unroll
    for (int e = 0; e < EPV; e += 4) {
      const int i = j * EPV + e;
      const float4 d = *reinterpret_cast<const float4*>(dz + (size_t)n * C + c0 + e);
      dzr[i] = d.x; dzr[i + 1] = d.y; dzr[i + 2] = d.z; dzr[i + 3] = d.w;
      if (FUSED) {
        const float4 w = *reinterpret_cast<const float4*>(Wa + c0 + e);
        wa[i] = w.x; wa[i + 1] = w.y; wa[i + 2] = w.z; wa[i + 3] = w.w;
      }
      if (act == M1_ACT_SOFTMAX) {
        const float4 zz = *reinterpret_cast<const float4*>(zsave + (size_t)n * C + c0 + e);
        zdz = fmaf(zz.x, d.x, zdz); zdz = fmaf(zz.y, d.y, zdz);
        zdz = fmaf(zz.z, d.z, zdz); zdz = fmaf(zz.w, d.w, zdz);
      }
    }
  }
  float sn;  // G[n,:] . bt: precomputed by the dz kernel (one load), else a K-long dot here
  if (sn_pre) {
    sn = sn_pre[n];
  } else {
    sn = 0.f;
    for (int k = lane; k < K; k += 64) sn = fmaf(G[(size_t)n * K + k], bt[k], sn);
    sn = wave_sum(sn);
  }
  float corr = 0.f;
  if (act == M1_ACT_SOFTMAX) corr = wave_sum(zdz) + sn * abar[n];

  float dwa[FUSED ? EPL : 1];
  if (FUSED) {
#pragma unroll
    for (int i = 0; i < EPL; ++i) dwa[i] = 0.f;
  }
  float dba_acc = 0.f;

  for (; p < p_end; p += 4) {
    const int pn = p + 4;
    if (pn < p_end) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) nxt[j] = ld16(xim + (size_t)pn * C + j * 64 * EPV + lane * EPV);
    }
    const float a = att_im[p];
    float x[EPL];
#pragma unroll
    for (int j = 0; j < VEC; ++j) Vec<T>::unpack(cur[j], x + j * EPV);

    float mk[TRAIN ? EPL : 1];  // mask / keep
    if (TRAIN) {
      const uint64_t ebase = ((uint64_t)n * P + p) * C;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const uint64_t e0 = ebase + j * 64 * EPV + lane * EPV;
#pragma unroll
        for (int e = 0; e < EPV; e += 2) {
          float m0, m1;
          rng_keep2(e0 + e, k0, k1, thresh, m0, m1);
          mk[j * EPV + e] = m0 * inv_keep;
          mk[j * EPV + e + 1] = m1 * inv_keep;
        }
      }
    }
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; i += 2) {
      if (TRAIN) {
        d0 = fmaf(x[i] * mk[i], dzr[i], d0);
        d1 = fmaf(x[i + 1] * mk[i + 1], dzr[i + 1], d1);
      } else {
        d0 = fmaf(x[i], dzr[i], d0);
        d1 = fmaf(x[i + 1], dzr[i + 1], d1);
      }
    }
    // + the concatenated pose channels' share (apa_m1_cat.hip); callers without them pass att, scale 0
    const float dA = (wave_sum(d0 + d1) + sn + dA_extra[(size_t)n * P + p] * extra_scale) * invP;
    float dZ;
    if (act == M1_ACT_SOFTMAX) dZ = a * (dA - corr);
    else if (act == M1_ACT_RELU) dZ = a > 0.f ? dA : 0.f;
    else dZ = dA;

    if constexpr (NODX) {
      if (FUSED) {
#pragma unroll
        for (int i = 0; i < EPL; ++i) dwa[i] = fmaf(dZ, x[i], dwa[i]);
      }
    } else {
      const float ap = a * invP;
      float o[EPL];
#pragma unroll
      for (int i = 0; i < EPL; ++i) {
        const float t = TRAIN ? ap * mk[i] : ap;
        if (FUSED) {
          o[i] = fmaf(t, dzr[i], dZ * wa[i]);
          dwa[i] = fmaf(dZ, x[i], dwa[i]);
        } else {
          o[i] = t * dzr[i];
        }
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        st16(dxim + (size_t)p * C + j * 64 * EPV + lane * EPV, Vec<T>::pack(o + j * EPV));
    }
    if (FUSED) dba_acc += dZ;
    else if (lane == 0) dZout[(size_t)n * P + p] = dZ;
#pragma unroll
    for (int j = 0; j < VEC; ++j) cur[j] = nxt[j];
  }

  if (FUSED) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
#pragma unroll
      for (int e = 0; e < EPV; e += 4) {
        const int c0 = j * 64 * EPV + lane * EPV + e;
        const int i = j * EPV + e;
        *reinterpret_cast<float4*>(&sm_acc[wave * C + c0]) =
            make_float4(dwa[i], dwa[i + 1], dwa[i + 2], dwa[i + 3]);
      }
    }
    if (lane == 0) sm_dba[wave] = dba_acc;
    __syncthreads();
    float* pa = pdwa + (size_t)blk * C;
    for (int v = threadIdx.x; v < C / 4; v += 256) {
      const float4 a0 = *reinterpret_cast<const float4*>(&sm_acc[0 * C + v * 4]);
      const float4 a1 = *reinterpret_cast<const float4*>(&sm_acc[1 * C + v * 4]);
      const float4 a2 = *reinterpret_cast<const float4*>(&sm_acc[2 * C + v * 4]);
      const float4 a3 = *reinterpret_cast<const float4*>(&sm_acc[3 * C + v * 4]);
      float4 r;
      r.x = (a0.x + a1.x) + (a2.x + a3.x);
      r.y = (a0.y + a1.y) + (a2.y + a3.y);
      r.z = (a0.z + a1.z) + (a2.z + a3.z);
      r.w = (a0.w + a1.w) + (a2.w + a3.w);
      *reinterpret_cast<float4*>(pa + v * 4) = r;
    }
    if (threadIdx.x == 0) pdba[blk] = (sm_dba[0] + sm_dba[1]) + (sm_dba[2] + sm_dba[3]);
  }
}

// ============================================================================================
// host side
// ============================================================================================
// the register-resident per-pixel kernels of this file: C = 64 * EPV * {1, 2}; the wider powers of two are
// streaming C's (m1s_supported)
bool m1v_supported(int C, int dtype) {
  const int epv = dtype == APA_DTYPE_BF16 ? 8 : 4;
  return C == 64 * epv || C == 128 * epv;
}

template <typename T, int VEC>
static int launch_fwd_t(const M1Call& c, const M1Fwd& io) {
  if (M1Trace* t = m1_trace()) { t->pool_fwd = M1_POOL_VEC; t->fwd_w = VEC; t->fwd_pix = 0; }
  m1_pool_form(c, [&](auto F, auto TR, auto G) {
    constexpr bool g = decltype(G)::value;
    launch_ev(m1_pool_fwd_kernel<T, VEC, decltype(F)::value, decltype(TR)::value, g>, dim3(c.pl.nblk), dim3(256), 0,
              c.st, c.ev0, c.ev1, static_cast<const T*>(io.X), io.Wa, io.ba, io.att, c.pacc, c.pstat, c.P, c.pl.S,
              c.pool_act, c.inv_keep, c.key.thresh, c.key.seed, c.key.offset, c.key.offset_dev, m1_gather_arg<g>(c));
    return APA_OK;
  });
  APA_LAUNCH_CHECK("m1_pool_fwd_kernel");
  return APA_OK;
}

template <typename T, int VEC>
static int launch_bwd_t(const M1Call& c, const M1Bwd& io) {
  if (M1Trace* t = m1_trace()) { t->pool_bwd = M1_POOL_VEC; t->bwd_w = VEC; t->bwd_pix = 0; }
  m1_pool_form(c, [&](auto F, auto TR, auto G) {
    constexpr bool f = decltype(F)::value, t = decltype(TR)::value, g = decltype(G)::value;
    // the arm without the dX stores (c.no_dx) is a gathered call's only one, fused or not; a plain call has both
    auto kernel = m1_bwd_main_kernel<T, VEC, f, t, true, g>;
    if constexpr (!g) {
      if (!c.no_dx) kernel = m1_bwd_main_kernel<T, VEC, f, t, false>;
    }
    launch_ev(kernel, dim3(c.pl.nblk), dim3(256), 0, c.st, c.ev0, c.ev1, static_cast<const T*>(io.X), io.Wa, io.att,
              c.dz, io.zsave, io.abar, io.G, io.bt, c.sn, g ? nullptr : static_cast<T*>(io.dX), c.dzatt, c.pdwa, c.pdba,
              c.P, c.pl.S, c.K, c.act, c.inv_keep, c.key.thresh, c.key.seed, c.key.offset, c.key.offset_dev, c.ex, c.exs,
              m1_gather_arg<g>(c));
    return APA_OK;
  });
  APA_LAUNCH_CHECK("m1_bwd_main_kernel");
  return APA_OK;
}

#define APA_V_DISPATCH(FN)                                                               \
  if (c.dtype == APA_DTYPE_F32) {                                                        \
    switch (c.C / 256) {                                                                 \
      case 1: return FN<float, 1>(c, io);                                                \
      case 2: return FN<float, 2>(c, io);                                                \
    }                                                                                    \
  } else {                                                                               \
    switch (c.C / 512) {                                                                 \
      case 1: return FN<bf16_t, 1>(c, io);                                               \
      case 2: return FN<bf16_t, 2>(c, io);                                               \
    }                                                                                    \
  }                                                                                      \
  set_error("attn_pool M=1: unsupported C=%d for dtype %d", c.C, c.dtype);               \
  return APA_ERR_UNSUPPORTED

int m1v_launch_pool_fwd(const M1Call& c, const M1Fwd& io) { APA_V_DISPATCH(launch_fwd_t); }
int m1v_launch_bwd_main(const M1Call& c, const M1Bwd& io) { APA_V_DISPATCH(launch_bwd_t); }
#undef APA_V_DISPATCH

}  // namespace apa
