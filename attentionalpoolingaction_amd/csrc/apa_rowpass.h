// apa_rowpass.h -- the row-in-registers toolkit of the streaming passes that keep a pixel's whole row in one wave
// (apa_m1_rank.hip, apa_multihead.hip): one wave owns a pixel, a lane owns NVL 16-byte vectors of its row (vector
// j * 64 + lane, EPV elements each, nvec = C / EPV of them exist), four waves per block.  The row's EL = NVL * EPV
// floats per lane are element i = j * EPV + e; an LDS row that meets them (weights, dz) is padded to 64 * EL floats,
// zero beyond C.  Every merge adds in a fixed order: (w0 + w1) + (w2 + w3).
#pragma once
#include <type_traits>

#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

// The instance that serves (C, dtype), which the caller found served (m1r_vectors_per_lane != 0):
// go(T{}, std::integral_constant<int, NVL>{}) with (float, 2 | 8) or (bf16_t, 1 | 4); returns what go returns, if anything
template <typename Fn> inline auto row_instance(int C, int dtype, Fn&& go) {
  const int nvl = m1r_vectors_per_lane(C, dtype);
  if (dtype == APA_DTYPE_F32) {
    if (nvl == 2) return go(float{}, std::integral_constant<int, 2>{});
    return go(float{}, std::integral_constant<int, 8>{});
  }
  if (nvl == 1) return go(bf16_t{}, std::integral_constant<int, 1>{});
  return go(bf16_t{}, std::integral_constant<int, 4>{});
}

// Which keep decisions a pass draws: the library stream alone, or also the caller's bit image (apa_device.h)
struct RngLib {
  static __device__ __forceinline__ void keep2(uint64_t e, uint32_t k0, uint32_t k1, uint32_t thresh, float& m0,
                                               float& m1) {
    rng_keep2(e, k0, k1, thresh, m0, m1);
  }
};
struct RngAny {
  static __device__ __forceinline__ void keep2(uint64_t e, uint32_t k0, uint32_t k1, uint32_t thresh, float& m0,
                                               float& m1) {
    rng_keep2_x(e, k0, k1, thresh, m0, m1);
  }
};

// keep decisions of the lane's NVL * EPV elements of the pixel row starting at flat element `ebase`, one bit each
template <typename RNG, int NVL, int EPV>
__device__ __forceinline__ uint32_t row_keep_bits(uint64_t ebase, int lane, int nvec, uint32_t k0, uint32_t k1,
                                                  uint32_t thresh) {
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < NVL; ++j) {
    const int v = j * 64 + lane;
    if (v < nvec) {
#pragma unroll
      for (int e = 0; e < EPV; e += 2) {
        float m0, m1;
        RNG::keep2(ebase + (uint64_t)v * EPV + e, k0, k1, thresh, m0, m1);
        bits |= (m0 != 0.f ? 1u : 0u) << (j * EPV + e);
        bits |= (m1 != 0.f ? 1u : 0u) << (j * EPV + e + 1);
      }
    }
  }
  return bits;
}

// The lane's vectors of the row at `row` (zero past nvec), issued and not waited for: the row travels while the one
// before it is consumed
template <typename T, int NVL>
__device__ __forceinline__ void row_load(uint4 (&nxt)[NVL], const T* row, int lane, int nvec) {
#pragma unroll
  for (int j = 0; j < NVL; ++j) {
    const int v = j * 64 + lane;
    nxt[j] = v < nvec ? ld16(row + (size_t)v * Vec<T>::EPV) : make_uint4(0u, 0u, 0u, 0u);
  }
}

// The lane's share of x . w, w a padded LDS row; wave_sum of it is the dot product
template <int NVL, int EPV>
__device__ __forceinline__ float row_dot(const float* x, const float* w, int lane) {
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < NVL; ++j) {
#pragma unroll
    for (int e = 0; e < EPV; e += 4) {
      const float4 w4 = *reinterpret_cast<const float4*>(w + (j * 64 + lane) * EPV + e);
      const int i = j * EPV + e;
      d = fmaf(x[i], w4.x, d); d = fmaf(x[i + 1], w4.y, d);
      d = fmaf(x[i + 2], w4.z, d); d = fmaf(x[i + 3], w4.w, d);
    }
  }
  return d;
}

// The 4 waves' register rows of EL floats per lane, summed in a fixed order into dst[c]: waves 1..3 pass theirs through
// LDS (3 * EL * 64 floats at sm), wave 0 adds (w0 + w1) + (w2 + w3) and stores.  Every thread of the block calls it.
template <int NVL, int EPV>
__device__ __forceinline__ void row_merge4(const float* row, float* sm, float* dst, int wave, int lane, int nvec) {
  constexpr int EL = NVL * EPV;
  __syncthreads();   // sm may still be read from the previous round
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < EL; ++i) sm[((wave - 1) * EL + i) * 64 + lane] = row[i];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int j = 0; j < NVL; ++j) {
      const int v = j * 64 + lane;
      if (v < nvec) {
        float o[EPV];
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          const int i = j * EPV + e;
          o[e] = (row[i] + sm[(0 * EL + i) * 64 + lane]) + (sm[(1 * EL + i) * 64 + lane] + sm[(2 * EL + i) * 64 + lane]);
        }
#pragma unroll
        for (int e = 0; e < EPV; e += 4)
          *reinterpret_cast<float4*>(dst + (size_t)v * EPV + e) = make_float4(o[e], o[e + 1], o[e + 2], o[e + 3]);
      }
    }
  }
}

// Statistic j of the block from the four waves' sm_stat[wave][j], which lane 0 of each wave stored before a barrier
template <int W>
__device__ __forceinline__ float row_stat_merge4(const float (&sm_stat)[4][W], int j) {
  return (sm_stat[0][j] + sm_stat[1][j]) + (sm_stat[2][j] + sm_stat[3][j]);
}

}  // namespace apa
