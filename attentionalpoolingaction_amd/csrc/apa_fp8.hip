// apa_fp8.hip -- the FP8 feature cache (apa.h: APA_DTYPE_FP8_E4M3): quantiser and dequantiser.
//
// A cache is OCP E4M3 codes [N,P,C] followed, at the next 256-byte boundary, by one fp32 scale per image.  The rule is
// exact (fp32, IEEE division), so custom_ops_factory.quantize_features restates it on the CPU bit for bit:
//   amax = max |x| over the image;  scale = amax / 448;  inv = 448 / amax (both 0 when amax == 0);  code = rne(x * inv)
// Encode and decode are the gfx950 conversion instructions (v_cvt_pk_fp8_f32 / v_cvt_pk_f32_fp8, OCP e4m3fn).
// Neither kernel is on a step's hot path: a cache is written once.
#include "apa_device.h"
#include "apa_fp8.h"
#include "apa_internal.h"

namespace apa {

namespace {
// 16 consecutive elements of a row as fp32: four (f32) or two (bf16) 16-byte loads
template <typename T>
__device__ __forceinline__ void load16(const T* p, float* x) {
  constexpr int EPV = Vec<T>::EPV;
#pragma unroll
  for (int v = 0; v < 16 / EPV; ++v) Vec<T>::unpack(ld16(p + v * EPV), x + v * EPV);
}

// One block per image: the image's amax and its non-finite flag, then its codes.  max is exact in any order, so the
// block's reduction tree does not matter; two calls are bit-identical.
template <typename T>
__global__ __launch_bounds__(1024) void fp8_quantize_kernel(const T* __restrict__ src, uint8_t* __restrict__ codes,
                                                            float* __restrict__ scale, int32_t* __restrict__ status,
                                                            long nvec) {   // nvec = P * C / 16
  __shared__ float s_max[16];
  __shared__ int s_bad[16];
  const int n = blockIdx.x;
  const T* im = src + (size_t)n * nvec * 16;
  uint8_t* out = codes + (size_t)n * nvec * 16;
  float amax = 0.f;
  int bad = 0;
  for (long v = threadIdx.x; v < nvec; v += 1024) {
    float x[16];
    load16(im + v * 16, x);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      bad |= (__float_as_uint(x[e]) & 0x7f800000u) == 0x7f800000u;
      amax = fmaxf(amax, fabsf(x[e]));
    }
  }
  amax = wave_max(amax);
  bad = __any(bad);
  if ((threadIdx.x & 63) == 0) { s_max[threadIdx.x >> 6] = amax; s_bad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  amax = 0.f; bad = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) { amax = fmaxf(amax, s_max[w]); bad |= s_bad[w]; }
  // a non-finite image is reported, not encoded: zero codes, zero scale
  const bool zero = bad || amax == 0.f;
  const float sc = zero ? 0.f : __fdiv_rn(amax, FP8_E4M3_MAX);
  const float inv = zero ? 0.f : __fdiv_rn(FP8_E4M3_MAX, amax);
  if (threadIdx.x == 0) { scale[n] = sc; status[n] = bad ? 1 : 0; }
  for (long v = threadIdx.x; v < nvec; v += 1024) {
    float x[16];
    uint32_t w[4];
    if (zero) {
      w[0] = w[1] = w[2] = w[3] = 0u;
    } else {
      load16(im + v * 16, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int pk = 0;
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(__fmul_rn(x[4 * q], inv), __fmul_rn(x[4 * q + 1], inv), pk, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(__fmul_rn(x[4 * q + 2], inv), __fmul_rn(x[4 * q + 3], inv), pk, true);
        w[q] = (uint32_t)pk;
      }
    }
    st16(out + v * 16, make_uint4(w[0], w[1], w[2], w[3]));
  }
}

// value = scale[n] * decode(code), 16 codes per thread and round
template <typename T>
__global__ __launch_bounds__(256) void fp8_dequantize_kernel(const uint8_t* __restrict__ codes,
                                                             const float* __restrict__ scale, T* __restrict__ dst,
                                                             long nvec_img, long nvec) {
  constexpr int EPV = Vec<T>::EPV;
  for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (long)gridDim.x * 256) {
    const float s = scale[v / nvec_img];
    float x[16];
    fp8x16_decode(ld16(codes + v * 16), x);
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = __fmul_rn(s, x[e]);
#pragma unroll
    for (int u = 0; u < 16 / EPV; ++u) st16(dst + v * 16 + u * EPV, Vec<T>::pack(x + u * EPV));
  }
}

int fp8_shape_check(const char* fn, const void* a, const void* b, int dtype, int N, int P, int C) {
  if (!a || !b) {
    set_error("%s: null tensor pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (N <= 0 || P <= 0 || C <= 0) {
    set_error("%s: non-positive dimension N=%d P=%d C=%d", fn, N, P, C);
    return APA_ERR_INVALID_ARG;
  }
  if (dtype != APA_DTYPE_F32 && dtype != APA_DTYPE_BF16) {
    set_error("%s: unknown dtype %d", fn, dtype);
    return APA_ERR_INVALID_ARG;
  }
  if (C % 16 != 0) {
    set_error("%s: C=%d is not a multiple of 16 (the codes are read and written 16 at a time)", fn, C);
    return APA_ERR_UNSUPPORTED;
  }
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) {
    set_error("%s: src and dst must be 16-byte aligned", fn);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}
}  // namespace

}  // namespace apa

using namespace apa;

extern "C" size_t apa_fp8_features_bytes(int N, int P, int C) {
  if (N <= 0 || P <= 0 || C <= 0) return 0;
  return fp8_scale_offset(N, P, C) + (size_t)N * 4;
}

// n images of src into slots [first, first + n) of the T-image cache at dst
static int quantize_at(const char* fn, const void* src, int src_dtype, void* dst, int T, int first, int32_t* status,
                       int N, int P, int C, void* stream) {
  const int rc = fp8_shape_check(fn, src, dst, src_dtype, N, P, C);
  if (rc != APA_OK) return rc;
  if (!status) {
    set_error("%s: null status pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (first < 0 || T < 1 || (long)first + N > (long)T) {
    set_error("%s: slots [%d, %d + %d) do not lie inside a cache of %d images", fn, first, first, N, T);
    return APA_ERR_INVALID_ARG;
  }
  uint8_t* codes = static_cast<uint8_t*>(dst) + (size_t)first * P * C;
  float* scale = reinterpret_cast<float*>(static_cast<uint8_t*>(dst) + fp8_scale_offset(T, P, C)) + first;
  const long nvec = (long)P * C / 16;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (src_dtype == APA_DTYPE_F32)
    hipLaunchKernelGGL(fp8_quantize_kernel<float>, dim3(N), dim3(1024), 0, st, static_cast<const float*>(src), codes,
                       scale, status, nvec);
  else
    hipLaunchKernelGGL(fp8_quantize_kernel<bf16_t>, dim3(N), dim3(1024), 0, st, static_cast<const bf16_t*>(src), codes,
                       scale, status, nvec);
  APA_LAUNCH_CHECK("fp8_quantize_kernel");
  return APA_OK;
}

extern "C" int apa_quantize_features_fp8(const void* src, int src_dtype, void* dst, int32_t* status, int N, int P,
                                         int C, void* stream) {
  return quantize_at("apa_quantize_features_fp8", src, src_dtype, dst, N, 0, status, N, P, C, stream);
}

extern "C" int apa_quantize_features_fp8_at(const void* src, int src_dtype, void* cache, int cache_images, int first,
                                            int32_t* status, int n, int P, int C, void* stream) {
  return quantize_at("apa_quantize_features_fp8_at", src, src_dtype, cache, cache_images, first, status, n, P, C,
                     stream);
}

extern "C" int apa_dequantize_features_fp8(const void* src, void* dst, int dst_dtype, int N, int P, int C,
                                           void* stream) {
  const int rc = fp8_shape_check("apa_dequantize_features_fp8", src, dst, dst_dtype, N, P, C);
  if (rc != APA_OK) return rc;
  const uint8_t* codes = static_cast<const uint8_t*>(src);
  const float* scale = reinterpret_cast<const float*>(codes + fp8_scale_offset(N, P, C));
  const long nvec_img = (long)P * C / 16, nvec = nvec_img * N;
  const int nb = (int)((nvec + 255) / 256 < 4096 ? (nvec + 255) / 256 : 4096);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dst_dtype == APA_DTYPE_F32)
    hipLaunchKernelGGL(fp8_dequantize_kernel<float>, dim3(nb), dim3(256), 0, st, codes, scale,
                       static_cast<float*>(dst), nvec_img, nvec);
  else
    hipLaunchKernelGGL(fp8_dequantize_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, codes, scale,
                       static_cast<bf16_t*>(dst), nvec_img, nvec);
  APA_LAUNCH_CHECK("fp8_dequantize_kernel");
  return APA_OK;
}
