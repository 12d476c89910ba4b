// apa_fp8.h -- what the FP8 feature cache's kernels share (apa_fp8.hip, apa_m1_fp8.hip): the layout of the one
// allocation behind an APA_DTYPE_FP8_E4M3 feature pointer and the decode of a 16-byte vector of codes.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace apa {

constexpr float FP8_E4M3_MAX = 448.0f;

// byte offset of the N fp32 scales: the first 256-byte boundary behind the N*P*C codes
__host__ __device__ inline size_t fp8_scale_offset(int N, int P, int C) {
  return ((size_t)N * P * C + 255) / 256 * 256;
}

// 16 OCP E4M3 codes -> fp32, element e of the vector in x[e]: eight v_cvt_pk_f32_fp8
__device__ __forceinline__ void fp8x16_decode(const uint4& r, float* x) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[q], true);
    x[4 * q] = lo.x; x[4 * q + 1] = lo.y; x[4 * q + 2] = hi.x; x[4 * q + 3] = hi.y;
  }
}

}  // namespace apa
