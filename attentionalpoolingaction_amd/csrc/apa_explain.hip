// apa_explain.hip -- why an image was given a class: the top-down attention map of T chosen classes, its product with
// the bottom-up map, and the reference's overlaid heat-map, on the device.
//
// Reference semantics.  models/slim/nets/nets_factory.py:247-328: the top-down map of class k is the 1x1 conv
// 'Conv2d_PrePose_TopDownAttn' column k of the last conv map, the class logit the spatial mean of bottom-up * top-down
// (end points 'TopDownAttention' / 'PosePrelogitsBasedAttention').  src/train.py:184-195 (_gen_overlayed_img) lays a
// map over the input image; tf.summary.image (src/train.py:451-460) turns the float overlay into uint8.
//
// apa_attn_explain, at most three launches:
//   1. explain_gather_kernel   the N*T selected columns of the row-major Wt [C,K] become a contiguous [N,T,C] image in
//                              the workspace (a column is a stride-K gather: done once per call, N*T*C loads, never per
//                              pixel), beside the clamped class ids and their biases;
//   2. explain_main_kernel     ONE pass over X with 16-byte loads whatever T is.  Block (n, s) owns pixels
//                              m1_pix_range(s) of image n, as the evaluation step's pooling pass does, stages image n's
//                              T*C weights in LDS once and walks its pixels DOWNWARDS (apa_m1_stream.hip: what the
//                              evaluation step read last is what the caches still hold).  A wave takes PIX pixels at a
//                              time: lanes split the channels, every weight vector read from LDS serves PIX pixels, the
//                              PIX * T dot products are finished inside the wave (16-lane DPP sums, two cross-row
//                              exchanges) in a fixed order;
//   3. explain_finish_kernel   class_logit[n,t] = (1/P) sum_p combined[n,t,p] from the stored map, one wave per (n,t),
//                              fixed order.  No floating-point atomics anywhere: two runs give the same bits.
// apa_attention_overlay, at most two launches: the resized map is never materialised -- every output element blends
// the four map taps itself (as apa_images.hip does); the uint8 form needs the (n,t) image's min / max first, which a
// partials launch computes from the same device function, so both launches see bit-identical values.
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

namespace {

constexpr int EXP_THREADS = 256;
constexpr size_t EXP_LDS_MAX = 64 * 1024;       // T * C * 4 bytes of weights per block
constexpr size_t EXP_LDS_SMALL = 16 * 1024;     // up to here the block count is the evaluation step's

}  // namespace

// (ExplainPlan and ExplainGeom: apa_internal.h)
// S: the pixel splits of the evaluation step's own pooling pass (m1_plan), so that block (n, s) meets the lines the
// same XCD read last; halved while a block's weight image is large -- the image is staged once per block, and at
// T * C * 4 = 64 KiB two blocks fill a CU's LDS anyway
ExplainPlan explain_plan(int N, int P, int C, int K, int T) {
  ExplainPlan pl;
  int S = m1_plan(N, P, C, C, K).S;
  if ((size_t)T * C * 4 > EXP_LDS_SMALL && S > 1) S = (S + 1) / 2;
  pl.S = S;
  pl.nblk = N * S;
  size_t off = 0;
  pl.off_w = off; off += align_up((size_t)N * T * C * 4, 256);
  pl.off_k = off; off += align_up((size_t)N * T * 4, 256);
  pl.off_b = off; off += align_up((size_t)N * T * 4, 256);
  pl.total = off;
  return pl;
}

namespace {

__global__ __launch_bounds__(EXP_THREADS) void explain_gather_kernel(
    const float* __restrict__ Wt, const float* __restrict__ bt, const int32_t* __restrict__ classes,
    float* __restrict__ wsel, int32_t* __restrict__ ksel, float* __restrict__ bsel, int32_t* __restrict__ status,
    int C, int K) {
  const int nt = blockIdx.x;
  const int raw = classes[nt];
  const int k = min(max(raw, 0), K - 1);   // the convention of apa_feature_cache.index: clamped, and counted
  float* dst = wsel + (size_t)nt * C;
  for (int c = threadIdx.x; c < C; c += EXP_THREADS) dst[c] = Wt[(size_t)c * K + k];
  if (threadIdx.x == 0) {
    ksel[nt] = k;
    bsel[nt] = bt[k];
    if (status && raw != k) atomicAdd(status, 1);   // an integer count: order-independent
  }
}

// EPV elements of a pixel row per lane and load: 16 bytes, or 8 for bf16 rows that are no whole number of 16-byte
// vectors (C % 8 == 4)
template <typename T, int EPV> struct XVec;
template <> struct XVec<float, 4> {
  typedef uint4 R;
  static __device__ __forceinline__ R load(const float* p) { return ld16(p); }
  static __device__ __forceinline__ void unpack(const R& r, float* o) { Vec<float>::unpack(r, o); }
};
template <> struct XVec<bf16_t, 8> {
  typedef uint4 R;
  static __device__ __forceinline__ R load(const bf16_t* p) { return ld16(p); }
  static __device__ __forceinline__ void unpack(const R& r, float* o) { Vec<bf16_t>::unpack(r, o); }
};
template <> struct XVec<bf16_t, 4> {
  typedef uint2 R;
  static __device__ __forceinline__ R load(const bf16_t* p) { return *reinterpret_cast<const uint2*>(p); }
  static __device__ __forceinline__ void unpack(const R& r, float* o) {
    o[0] = bf16_lo(r.x); o[1] = bf16_hi(r.x); o[2] = bf16_lo(r.y); o[3] = bf16_hi(r.y);
  }
};

template <typename T, int EPV, int TT>
__global__ __launch_bounds__(EXP_THREADS) void explain_main_kernel(
    const T* __restrict__ X, const float* __restrict__ att, const float* __restrict__ wsel,
    const int32_t* __restrict__ ksel, const float* __restrict__ bsel, float* __restrict__ topdown,
    float* __restrict__ combined, int P, int C, int M, int S, int nblk, int relu_in) {
  constexpr int PIX = ExplainGeom<TT>::PIX, U = ExplainGeom<TT>::U;
  typedef XVec<T, EPV> XV;
  extern __shared__ __attribute__((aligned(16))) float sm_w[];   // [TT][C]

  const unsigned blk = (unsigned)xcd_remap(blockIdx.x, nblk);
  const int n = (int)(blk / (unsigned)S), s = (int)(blk % (unsigned)S);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15;
  int p_begin, p_end;
  m1_pix_range(s, P, S, p_begin, p_end);

  // image n's weights: contiguous in the gathered image, 16 bytes per thread and step
  {
    const float4* src = reinterpret_cast<const float4*>(wsel + (size_t)n * TT * C);
    float4* dst = reinterpret_cast<float4*>(sm_w);
    for (int i = threadIdx.x; i < TT * (C >> 2); i += EXP_THREADS) dst[i] = src[i];
  }
  // slot l16 = i * TT + t of a group: pixel i, class t.  Lanes 0 .. PIX * TT - 1 of the wave own one slot each
  const int si = l16 / TT, st = l16 - si * TT;
  const bool slot_lane = lane < PIX * TT;
  const float bias = bsel[(size_t)n * TT + st];
  const int kk = M == 1 ? 0 : ksel[(size_t)n * TT + st];
  __syncthreads();

  const T* xim = X + (size_t)n * P * C;
  const int ngroups = (p_end - p_begin + PIX - 1) / PIX;
  for (int g = wave; g < ngroups; g += 4) {
    const int ptop = p_end - 1 - g * PIX;        // slot i is pixel ptop - i; below p_begin: not this block's
    const int myp = ptop - si;
    const bool mine = slot_lane && myp >= p_begin;
    const float a = mine ? att[((size_t)n * P + myp) * M + kk] : 0.f;
    float acc[PIX][TT];
#pragma unroll
    for (int i = 0; i < PIX; ++i)
#pragma unroll
      for (int t = 0; t < TT; ++t) acc[i][t] = 0.f;

    for (int cb = 0; cb < C; cb += 64 * EPV * U) {
      typename XV::R xr[U][PIX];
      int cc[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = cb + (u * 64 + lane) * EPV;
        ok[u] = c < C;
        cc[u] = ok[u] ? c : 0;       // lanes past the row's end re-read its head and contribute zeros
#pragma unroll
        for (int i = 0; i < PIX; ++i) {
          const int p = max(ptop - i, p_begin);   // slots below the block's range repeat its first pixel
          xr[u][i] = XV::load(xim + (size_t)p * C + cc[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float x[PIX][EPV];
#pragma unroll
        for (int i = 0; i < PIX; ++i) {
          XV::unpack(xr[u][i], x[i]);
#pragma unroll
          for (int e = 0; e < EPV; ++e) {
            if (relu_in) x[i][e] = fmaxf(x[i][e], 0.f);
            x[i][e] = ok[u] ? x[i][e] : 0.f;
          }
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
          float w[EPV];
#pragma unroll
          for (int e = 0; e < EPV; e += 4) {
            const float4 v = *reinterpret_cast<const float4*>(&sm_w[t * C + cc[u] + e]);
            w[e] = v.x; w[e + 1] = v.y; w[e + 2] = v.z; w[e + 3] = v.w;
          }
#pragma unroll
          for (int i = 0; i < PIX; ++i)
#pragma unroll
            for (int e = 0; e < EPV; ++e) acc[i][t] = fmaf(x[i][e], w[e], acc[i][t]);
        }
      }
    }

    // the PIX * TT channel sums: in-row DPP sums, slot j kept by the lanes with l16 == j, then the four rows
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < PIX; ++i)
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float r = row_sum16(acc[i][t]);
        tot = (l16 == i * TT + t) ? r : tot;
      }
    tot += __shfl_xor(tot, 16);
    tot += __shfl_xor(tot, 32);
    if (mine) {
      const float td = tot + bias;
      const size_t o = ((size_t)n * TT + st) * P + myp;
      topdown[o] = td;
      combined[o] = a * td;
    }
  }
}

__global__ __launch_bounds__(64) void explain_finish_kernel(const float* __restrict__ combined,
                                                            float* __restrict__ class_logit, int P) {
  const int nt = blockIdx.x, lane = threadIdx.x;
  const float* row = combined + (size_t)nt * P;
  float s = 0.f;
  for (int p = lane; p < P; p += 64) s += row[p];
  s = wave_sum(s);
  if (lane == 0) class_logit[nt] = s * (1.0f / (float)P);
}

template <typename XT, int EPV>
int explain_launch_t(const ExplainPlan& pl, const void* X, const float* att, const float* wsel, const int32_t* ksel,
                     const float* bsel, float* topdown, float* combined, int P, int C, int M, int T, int relu_in,
                     hipStream_t st, const Hooks& hk) {
  const size_t lds = (size_t)T * C * 4;
  const dim3 grid(pl.nblk), block(EXP_THREADS);
#define APA_EXPLAIN_CASE(TT)                                                                                        \
  case TT:                                                                                                          \
    launch_ev(explain_main_kernel<XT, EPV, TT>, grid, block, lds, st, hk.fwd0, hk.fwd1, static_cast<const XT*>(X),   \
              att, wsel, ksel, bsel, topdown, combined, P, C, M, pl.S, pl.nblk, relu_in);                           \
    break
  switch (T) {
    APA_EXPLAIN_CASE(1); APA_EXPLAIN_CASE(2); APA_EXPLAIN_CASE(3); APA_EXPLAIN_CASE(4);
    APA_EXPLAIN_CASE(5); APA_EXPLAIN_CASE(6); APA_EXPLAIN_CASE(7); APA_EXPLAIN_CASE(8);
  }
#undef APA_EXPLAIN_CASE
  APA_LAUNCH_CHECK("explain_main_kernel");
  return APA_OK;
}

// every refusal of the shape that needs no pointer (shared by the workspace query): APA_OK, or the status
int explain_shape_check(int N, int P, int C, int K, int T, int dtype, bool say) {
  if (N <= 0 || P <= 0 || C <= 0 || K <= 0) {
    if (say) set_error("apa_attn_explain: non-positive dimension N=%d P=%d C=%d K=%d", N, P, C, K);
    return APA_ERR_INVALID_ARG;
  }
  if (dtype == APA_DTYPE_FP8_E4M3) {
    if (say) set_error("apa_attn_explain: reads dense features; an FP8 cache is not served");
    return APA_ERR_UNSUPPORTED;
  }
  if (dtype != APA_DTYPE_F32 && dtype != APA_DTYPE_BF16) {
    if (say) set_error("apa_attn_explain: unknown dtype %d", dtype);
    return APA_ERR_INVALID_ARG;
  }
  if (T < 1 || T > APA_EXPLAIN_MAX_CLASSES) {
    if (say) set_error("apa_attn_explain: T=%d classes per image, served 1..%d", T, APA_EXPLAIN_MAX_CLASSES);
    return APA_ERR_UNSUPPORTED;
  }
  if (C % 4 != 0) {
    if (say) set_error("apa_attn_explain: C=%d is not a multiple of 4", C);
    return APA_ERR_UNSUPPORTED;
  }
  if ((size_t)T * C * 4 > EXP_LDS_MAX) {
    if (say) set_error("apa_attn_explain: T*C=%d*%d weights exceed the %zu-byte LDS image of a block", T, C, EXP_LDS_MAX);
    return APA_ERR_UNSUPPORTED;
  }
  const ExplainPlan pl = explain_plan(N, P, C, K, T);
  if (!m1_pix_range_ok(P, pl.S) || (long long)N * pl.S >= (1ll << 31) || (long long)N * T >= (1ll << 31)) {
    if (say) set_error("apa_attn_explain: N=%d P=%d exceed the 31-bit block / pixel arithmetic", N, P);
    return APA_ERR_UNSUPPORTED;
  }
  return APA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// overlay
// ---------------------------------------------------------------------------------------------------------------
constexpr int OVL_THREADS = 256;
constexpr int OVL_BLOCKS = 64;   // blocks per (n,t) image: one partial per lane of the wave that merges them

// one axis of the TF 1.1 legacy bilinear resize (align_corners = false): the rule of apa_resize_bilinear_tf1
struct OvlTap { int lo, hi; float t; };
__device__ __forceinline__ OvlTap ovl_tap(int i, float scale, int in_size) {
#pragma clang fp contract(off)
  const float f = (float)i * scale;
  OvlTap r;
  int lo = (int)floorf(f);
  r.t = f - (float)lo;
  lo = min(lo, in_size - 1);   // never taken for i < out_size; keeps the read inside the map
  r.lo = lo;
  r.hi = min(lo + 1, in_size - 1);
  return r;
}

// train.py:184-195 for one pixel: out = 0.5 * [gray, gray, gray] + 0.5 * [255 m, 0 m, 0 m].  Every operation rounded
// on its own (contraction off): both launches, and the float32 reference execution, see the same values
__device__ __forceinline__ void ovl_pixel(const float* __restrict__ map, int w, const OvlTap& ty, const OvlTap& tx,
                                          const float* __restrict__ px, float (&out)[3]) {
#pragma clang fp contract(off)
  const float tl = map[(size_t)ty.lo * w + tx.lo], tr = map[(size_t)ty.lo * w + tx.hi];
  const float bl = map[(size_t)ty.hi * w + tx.lo], br = map[(size_t)ty.hi * w + tx.hi];
  const float top = tl + (tr - tl) * tx.t;
  const float bot = bl + (br - bl) * tx.t;
  const float m = top + (bot - top) * ty.t;
  const float gray = (0.2989f * px[0] + 0.5870f * px[1]) + 0.1140f * px[2];
  const float hg = 0.5f * gray;
  out[0] = hg + 0.5f * (m * 255.0f);
  out[1] = hg + 0.5f * (m * 0.0f);
  out[2] = out[1];
}

struct OvlArgs {
  const float* maps; const float* images; int T, h, w, H, W; float sy, sx;
};

// pixel q (= y * W + x) of (n,t) image nt
__device__ __forceinline__ void ovl_value(const OvlArgs& a, int nt, int q, float (&out)[3]) {
  const int y = q / a.W, x = q - y * a.W;
  const OvlTap ty = ovl_tap(y, a.sy, a.h), tx = ovl_tap(x, a.sx, a.w);
  const int n = nt / a.T;
  ovl_pixel(a.maps + (size_t)nt * a.h * a.w, a.w, ty, tx, a.images + ((size_t)n * a.H * a.W + q) * 3, out);
}

__global__ __launch_bounds__(OVL_THREADS) void overlay_minmax_kernel(OvlArgs a, float* __restrict__ part) {
  __shared__ float red[2][4];
  const int nt = blockIdx.x / OVL_BLOCKS, b = blockIdx.x - nt * OVL_BLOCKS;
  const int npix = a.H * a.W;
  float lo = INFINITY, hi = -INFINITY;
  for (int q = b * OVL_THREADS + threadIdx.x; q < npix; q += OVL_BLOCKS * OVL_THREADS) {
    float v[3];
    ovl_value(a, nt, q, v);
    lo = fminf(lo, fminf(v[0], fminf(v[1], v[2])));
    hi = fmaxf(hi, fmaxf(v[0], fmaxf(v[1], v[2])));
  }
  lo = -wave_max(-lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[(size_t)blockIdx.x * 2 + 0] = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    part[(size_t)blockIdx.x * 2 + 1] = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
  }
}

__global__ __launch_bounds__(OVL_THREADS) void overlay_write_kernel(OvlArgs a, const float* __restrict__ part,
                                                                    float* __restrict__ out_f32,
                                                                    uint8_t* __restrict__ out_u8) {
#pragma clang fp contract(off)
  const int nt = blockIdx.x / OVL_BLOCKS, b = blockIdx.x - nt * OVL_BLOCKS;
  const int npix = a.H * a.W;
  float s = 0.f, o = 0.f;
  if (out_u8) {   // tf.summary.image's rule from the image's min / max (every wave merges the partials itself)
    const int lane = threadIdx.x & 63;
    const float lo = -wave_max(-part[((size_t)nt * OVL_BLOCKS + lane) * 2 + 0]);
    const float hi = wave_max(part[((size_t)nt * OVL_BLOCKS + lane) * 2 + 1]);
    const float mx = fmaxf(fabsf(lo), fabsf(hi));
    if (lo < 0.f) { s = __fdiv_rn(127.0f, mx); o = 128.0f; }
    else { s = mx == 0.f ? 0.f : __fdiv_rn(255.0f, hi); o = 0.f; }
  }
  const size_t base = (size_t)nt * npix * 3;
  for (int q = b * OVL_THREADS + threadIdx.x; q < npix; q += OVL_BLOCKS * OVL_THREADS) {
    float v[3];
    ovl_value(a, nt, q, v);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t i = base + (size_t)q * 3 + c;
      if (out_f32) out_f32[i] = v[c];
      if (out_u8) {
        const float z = truncf(v[c] * s + o);
        out_u8[i] = (uint8_t)(int)fminf(255.0f, fmaxf(0.0f, z));
      }
    }
  }
}

}  // namespace

}  // namespace apa

using namespace apa;

extern "C" size_t apa_attn_explain_workspace_bytes(int N, int P, int C, int K, int T, int dtype) {
  if (explain_shape_check(N, P, C, K, T, dtype, false) != APA_OK) return 0;
  return explain_plan(N, P, C, K, T).total;
}

extern "C" int apa_attn_explain(const apa_hooks* hooks, const void* X, const float* att, const float* Wt, const float* bt,
                                const int32_t* classes, float* topdown, float* combined, float* class_logit,
                                int32_t* status, void* ws, size_t ws_bytes, int N, int P, int C, int K, int M, int T,
                                unsigned flags, int dtype, void* stream) {
  if (!X || !att || !Wt || !bt || !classes || !topdown || !combined || !class_logit) {
    set_error("apa_attn_explain: null pointer");
    return APA_ERR_INVALID_ARG;
  }
  if (N <= 0 || P <= 0 || C <= 0 || K <= 0 || M <= 0) {
    set_error("apa_attn_explain: non-positive dimension N=%d P=%d C=%d K=%d M=%d", N, P, C, K, M);
    return APA_ERR_INVALID_ARG;
  }
  if (M != 1 && M != K) {
    set_error("apa_attn_explain: M=%d must be 1 or K=%d", M, K);
    return APA_ERR_INVALID_ARG;
  }
  if (flags & ~APA_FLAG_RELU_INPUT) {
    set_error("apa_attn_explain: flags 0x%x: only APA_FLAG_RELU_INPUT is understood (evaluation semantics)", flags);
    return APA_ERR_INVALID_ARG;
  }
  const int rc = explain_shape_check(N, P, C, K, T, dtype, true);
  if (rc != APA_OK) return rc;
  const ExplainPlan pl = explain_plan(N, P, C, K, T);
  if (!ws || ws_bytes < pl.total) {
    set_error("apa_attn_explain: workspace of %zu bytes, %zu needed (apa_attn_explain_workspace_bytes)", ws_bytes,
              pl.total);
    return APA_ERR_WORKSPACE;
  }
  const bool bf16 = dtype == APA_DTYPE_BF16;
  const int epv = bf16 ? (C % 8 == 0 ? 8 : 4) : 4;
  const uintptr_t xalign = (uintptr_t)(epv * (bf16 ? 2 : 4)) - 1;
  if (((uintptr_t)X & xalign) || ((uintptr_t)ws & 15)) {
    set_error("apa_attn_explain: X must be %zu-byte and the workspace 16-byte aligned", (size_t)xalign + 1);
    return APA_ERR_INVALID_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Hooks hk(hooks);   // prof_fwd_start / prof_fwd_stop bracket the dispatch of explain_main_kernel
  char* base = static_cast<char*>(ws);
  float* wsel = reinterpret_cast<float*>(base + pl.off_w);
  int32_t* ksel = reinterpret_cast<int32_t*>(base + pl.off_k);
  float* bsel = reinterpret_cast<float*>(base + pl.off_b);
  hipLaunchKernelGGL(explain_gather_kernel, dim3(N * T), dim3(EXP_THREADS), 0, st, Wt, bt, classes, wsel, ksel, bsel,
                     status, C, K);
  APA_LAUNCH_CHECK("explain_gather_kernel");
  const int relu_in = (flags & APA_FLAG_RELU_INPUT) ? 1 : 0;
  int lrc;
  if (!bf16) lrc = explain_launch_t<float, 4>(pl, X, att, wsel, ksel, bsel, topdown, combined, P, C, M, T, relu_in, st, hk);
  else if (epv == 8) lrc = explain_launch_t<bf16_t, 8>(pl, X, att, wsel, ksel, bsel, topdown, combined, P, C, M, T, relu_in, st, hk);
  else lrc = explain_launch_t<bf16_t, 4>(pl, X, att, wsel, ksel, bsel, topdown, combined, P, C, M, T, relu_in, st, hk);
  if (lrc != APA_OK) return lrc;
  hipLaunchKernelGGL(explain_finish_kernel, dim3(N * T), dim3(64), 0, st, combined, class_logit, P);
  APA_LAUNCH_CHECK("explain_finish_kernel");
  return APA_OK;
}

static bool overlay_dims_ok(int N, int T, int H, int W) {
  return (long long)N * T * OVL_BLOCKS < (1ll << 31) && (long long)H * W < (1ll << 30);
}

extern "C" size_t apa_attention_overlay_workspace_bytes(int N, int T) {
  if (N <= 0 || T <= 0 || (long long)N * T * OVL_BLOCKS >= (1ll << 31)) return 0;
  return (size_t)N * T * OVL_BLOCKS * 2 * sizeof(float);
}

extern "C" int apa_attention_overlay(const float* maps, const float* images, float* overlay_f32, uint8_t* overlay_u8,
                                     void* ws, size_t ws_bytes, int N, int T, int h, int w, int H, int W,
                                     void* stream) {
  if (!maps || !images || (!overlay_f32 && !overlay_u8)) {
    set_error("apa_attention_overlay: null maps / images, or no output");
    return APA_ERR_INVALID_ARG;
  }
  if (N <= 0 || T <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) {
    set_error("apa_attention_overlay: non-positive size N=%d T=%d map %dx%d image %dx%d", N, T, h, w, H, W);
    return APA_ERR_INVALID_ARG;
  }
  if (!overlay_dims_ok(N, T, H, W)) {
    set_error("apa_attention_overlay: N*T=%d*%d images of %dx%d exceed the 31-bit block / pixel arithmetic", N, T, H, W);
    return APA_ERR_UNSUPPORTED;
  }
  if (overlay_u8 && (!ws || ws_bytes < apa_attention_overlay_workspace_bytes(N, T))) {
    set_error("apa_attention_overlay: workspace of %zu bytes, %zu needed for the uint8 form", ws_bytes,
              apa_attention_overlay_workspace_bytes(N, T));
    return APA_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  OvlArgs a;
  a.maps = maps; a.images = images; a.T = T; a.h = h; a.w = w; a.H = H; a.W = W;
  a.sy = (float)h / (float)H; a.sx = (float)w / (float)W;
  const dim3 grid((unsigned)(N * T * OVL_BLOCKS)), block(OVL_THREADS);
  float* part = static_cast<float*>(ws);
  if (overlay_u8) {
    hipLaunchKernelGGL(overlay_minmax_kernel, grid, block, 0, st, a, part);
    APA_LAUNCH_CHECK("overlay_minmax_kernel");
  }
  hipLaunchKernelGGL(overlay_write_kernel, grid, block, 0, st, a, static_cast<const float*>(part), overlay_f32,
                     overlay_u8);
  APA_LAUNCH_CHECK("overlay_write_kernel");
  return APA_OK;
}
