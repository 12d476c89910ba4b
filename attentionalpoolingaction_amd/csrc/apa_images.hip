// apa_images.hip -- the image half of the input pipeline on the device.
//
// The reference prepares each training image on the CPU with TF image ops -- the author names the stage
// the bottleneck of the training system (src/preprocess_pipeline.py:171-179):
//   _resize_if_needed (src/preprocess_pipeline.py:5-18): wider than cfg.MAX_INPUT_IMAGE_SIZE -> legacy
//     bilinear resize to [lh, max_wd], truncated to uint8 (image L)
//   -> vgg_preprocessing.preprocess_image (models/slim/preprocessing/vgg_preprocessing.py):
//     _aspect_preserving_resize (:241-294) to [ah, aw] in float32 (image A), crop (:52-205), flip (:329-332),
//     - _MEAN (:45, :352, :372)
// Here pass 1 writes L (uint8, workspace) for the samples that need the limit and pass 2 produces the
// final [T, crop_h, crop_w, 3] block per sample straight from L (or from the source): an output element is the
// bilinear blend of four L pixels at the A coordinate the crop / flip maps it to, so A is never built.
// The frames of a sample share one geometry (:182-194: they are concatenated on the channel axis).
// The numpy restatement tests/_image_reference.py, pinned to the reference's own code by
// tests/golden/ref_images.npz, is the bit-exact oracle of these kernels: every a + b * c stays two roundings
// (mul_2r, see apa_labels.hip) and every division is IEEE.
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

// opaque product: keeps hipcc from contracting a * b + c into one fma (apa_labels.hip:22-30)
__device__ __forceinline__ float img_mul_2r(float a, float b) {
  float p = a * b;
  asm volatile("" : "+v"(p));
  return p;
}

__host__ __device__ inline float img_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

// _resize_if_needed (src/preprocess_pipeline.py:7-11): the size after the limit, float32 as the graph
__host__ __device__ inline void img_limit_size(int sh, int sw, int max_wd, long long* lh, int* lw) {
  if (sw > max_wd) {
    *lw = max_wd;
    *lh = (long long)((float)sh * img_div((float)max_wd, (float)sw));
  } else {
    *lw = sw;
    *lh = sh;
  }
}

// _smallest_size_at_least (vgg_preprocessing.py:257-268)
__host__ __device__ inline void img_aug_size(int lh, int lw, int side, int* ah, int* aw) {
  const float h = (float)lh, w = (float)lw, s = (float)side;
  const float scale = lh > lw ? img_div(s, w) : img_div(s, h);
  *ah = (int)(h * scale);
  *aw = (int)(w * scale);
}

constexpr int IMG_THREADS = 256;
constexpr int IMG_ROW_BLOCKS = 512;   // blocks per sample; each strides over the (frame, row) pairs
constexpr size_t IMG_WS_ALIGN = 16;

// What both passes derive for sample n (wave-uniform: every lane computes the same values).
struct ImgPlan {
  bool bad;        // status 1: the reference would have failed, or the sample does not fit its buffers
  bool limited;    // L lives in the workspace slot
  int sh, sw;      // source frame
  int lh, lw;      // L
  const uint8_t* src;   // first frame of the sample
};

__device__ __forceinline__ ImgPlan img_plan(const uint8_t* __restrict__ src, size_t src_bytes,
                                            const int64_t* __restrict__ src_off,
                                            const int32_t* __restrict__ src_hw, const int32_t* __restrict__ geom,
                                            int n, int T, int max_wd, size_t ws_slot) {
  ImgPlan p;
  p.bad = true;
  p.limited = false;
  p.sh = src_hw[2 * n];
  p.sw = src_hw[2 * n + 1];
  p.lh = p.lw = 0;
  p.src = src;
  const int32_t* g = geom + (size_t)n * 9;
  const int aug_ht = g[2], aug_wd = g[3];
  const long long crop_y = g[4], crop_x = g[5], crop_h = g[6], crop_w = g[7];
  if (p.sh <= 0 || p.sw <= 0 || g[0] <= 0 || g[1] <= 0 || aug_ht <= 0 || aug_wd <= 0) return p;
  // the sample's frames lie inside the packed buffer (no product here can overflow: each is checked first)
  const long long off = src_off[n];
  const unsigned long long px = (unsigned long long)p.sh * (unsigned long long)p.sw;
  if (off < 0 || (unsigned long long)off > src_bytes) return p;
  const unsigned long long room = src_bytes - (unsigned long long)off;
  if (px > room / 3 || px * 3 > room / (unsigned long long)T) return p;
  p.src = src + off;
  long long lh;
  img_limit_size(p.sh, p.sw, max_wd, &lh, &p.lw);
  if (lh <= 0 || lh > p.sh) return p;
  p.lh = (int)lh;
  p.limited = p.sw > max_wd;
  if (p.limited && (unsigned long long)T * p.lh * p.lw * 3 > ws_slot) return p;
  // aug size: the recorded one must be what the float32 rule gives for SOME resize side; the rule lands
  // on the side or one short of it (37x53, side 24 -> 23x34), so those two are the candidates
  const int shorter = p.lh > p.lw ? aug_wd : aug_ht;
  bool ok = false;
  for (int side = shorter; side <= shorter + 1 && side > 0; ++side) {
    int ah, aw;
    img_aug_size(p.lh, p.lw, side, &ah, &aw);
    ok = ok || (ah == aug_ht && aw == aug_wd);
  }
  if (!ok) return p;
  // the crop lies inside A (tf.slice / the size assertion would fail) and has the size of the output block
  if (crop_y < 0 || crop_x < 0 || crop_h <= 0 || crop_w <= 0 || crop_y + crop_h > aug_ht || crop_x + crop_w > aug_wd)
    return p;
  if (crop_h != geom[6] || crop_w != geom[7]) return p;
  p.bad = false;
  return p;
}

// one axis of ResizeBilinear, align_corners = false: scale = in / out, src = i * scale in float32
struct ImgTap { int lo, hi; float t; };
__device__ __forceinline__ ImgTap img_tap(int i, float scale, int in_size) {
  const float f = img_mul_2r((float)i, scale);
  ImgTap r;
  int lo = (int)floorf(f);
  r.t = f - (float)lo;
  lo = lo < in_size - 1 ? lo : in_size - 1;     // never taken for i < out_size; keeps the read inside the image
  r.lo = lo;
  r.hi = lo + 1 < in_size ? lo + 1 : in_size - 1;
  return r;
}

__device__ __forceinline__ float img_blend(const uint8_t* __restrict__ img, long long row_bytes, const ImgTap& y,
                                           const ImgTap& x, int c) {
  const uint8_t* r0 = img + (long long)y.lo * row_bytes + c;
  const uint8_t* r1 = img + (long long)y.hi * row_bytes + c;
  const float tl = (float)r0[(long long)x.lo * 3], tr = (float)r0[(long long)x.hi * 3];
  const float bl = (float)r1[(long long)x.lo * 3], br = (float)r1[(long long)x.hi * 3];
  const float top = tl + img_mul_2r(tr - tl, x.t);
  const float bot = bl + img_mul_2r(br - bl, x.t);
  return top + img_mul_2r(bot - top, y.t);
}

// pass 1: L = uint8(resize_bilinear(src, [lh, lw])) of the samples wider than max_wd, into their workspace slot
__global__ __launch_bounds__(IMG_THREADS) void image_limit_kernel(
    const uint8_t* __restrict__ src, size_t src_bytes, const int64_t* __restrict__ src_off,
    const int32_t* __restrict__ src_hw, const int32_t* __restrict__ geom, int T, int max_wd,
    uint8_t* __restrict__ ws, size_t ws_slot) {
  const int n = blockIdx.y;
  const ImgPlan p = img_plan(src, src_bytes, src_off, src_hw, geom, n, T, max_wd, ws_slot);
  if (p.bad || !p.limited) return;
  uint8_t* L = ws + (size_t)n * ws_slot;
  const float sy = img_div((float)p.sh, (float)p.lh), sx = img_div((float)p.sw, (float)p.lw);
  const long long src_row = (long long)p.sw * 3, src_frame = src_row * p.sh;
  const int row_elems = p.lw * 3;
  for (long long r = blockIdx.x; r < (long long)T * p.lh; r += gridDim.x) {
    const int t = (int)(r / p.lh), yo = (int)(r - (long long)t * p.lh);
    const ImgTap ty = img_tap(yo, sy, p.sh);
    const uint8_t* frame = p.src + (long long)t * src_frame;
    uint8_t* dst = L + (size_t)r * row_elems;
    for (int e = threadIdx.x; e < row_elems; e += IMG_THREADS) {
      const int xo = e / 3, c = e - xo * 3;
      const ImgTap tx = img_tap(xo, sx, p.sw);
      dst[e] = (uint8_t)(int)img_blend(frame, src_row, ty, tx, c);   // tf.cast(float -> uint8): truncation
    }
  }
}

__device__ __forceinline__ void img_store(float* out, size_t i, float v) { out[i] = v; }
__device__ __forceinline__ void img_store(bf16_t* out, size_t i, float v) { out[i].v = (uint16_t)f32_to_bf16_bits(v); }

// pass 2: out[n, t, y, x, c] = A[crop_y + y, crop_x + (flip ? crop_w - 1 - x : x), c] - mean, A taken from L on the fly
template <typename OutT>
__global__ __launch_bounds__(IMG_THREADS) void image_crop_kernel(
    const uint8_t* __restrict__ src, size_t src_bytes, const int64_t* __restrict__ src_off,
    const int32_t* __restrict__ src_hw, const int32_t* __restrict__ geom, int T, int max_wd, float mean,
    OutT* __restrict__ out, int32_t* __restrict__ status, const uint8_t* __restrict__ ws, size_t ws_slot) {
  const int n = blockIdx.y;
  const ImgPlan p = img_plan(src, src_bytes, src_off, src_hw, geom, n, T, max_wd, ws_slot);
  if (blockIdx.x == 0 && threadIdx.x == 0) status[n] = p.bad ? 1 : 0;
  // the block every sample owns in `out` has the crop size of sample 0 (img_plan refuses any other)
  const int out_h = geom[6], out_w = geom[7];
  if (out_h <= 0 || out_w <= 0) return;          // no output shape: nothing can be written (every status is 1)
  const int row_elems = out_w * 3;
  const long long rows = (long long)T * out_h;
  OutT* o = out + (size_t)n * rows * row_elems;
  if (p.bad) {
    for (long long r = blockIdx.x; r < rows; r += gridDim.x)
      for (int e = threadIdx.x; e < row_elems; e += IMG_THREADS) img_store(o, (size_t)r * row_elems + e, 0.f);
    return;
  }
  const int32_t* g = geom + (size_t)n * 9;
  const int aug_ht = g[2], aug_wd = g[3], crop_y = g[4], crop_x = g[5], flip = g[8];
  const uint8_t* L = p.limited ? ws + (size_t)n * ws_slot : p.src;
  const float sy = img_div((float)p.lh, (float)aug_ht), sx = img_div((float)p.lw, (float)aug_wd);
  const long long l_row = (long long)p.lw * 3, l_frame = l_row * p.lh;
  for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
    const int t = (int)(r / out_h), y = (int)(r - (long long)t * out_h);
    const ImgTap ty = img_tap(crop_y + y, sy, p.lh);
    const uint8_t* frame = L + (long long)t * l_frame;
    for (int e = threadIdx.x; e < row_elems; e += IMG_THREADS) {
      const int x = e / 3, c = e - x * 3;
      const ImgTap tx = img_tap(crop_x + (flip ? out_w - 1 - x : x), sx, p.lw);
      img_store(o, (size_t)r * row_elems + e, img_blend(frame, l_row, ty, tx, c) - mean);
    }
  }
}

}  // namespace apa

using namespace apa;

extern "C" int apa_image_aug_size(int src_ht, int src_wd, int max_wd, int resize_side, int32_t out[4]) {
  if (!out || src_ht <= 0 || src_wd <= 0 || max_wd <= 0 || resize_side <= 0) {
    set_error("apa_image_aug_size: null pointer or non-positive size");
    return APA_ERR_INVALID_ARG;
  }
  long long lh;
  int lw, ah = 0, aw = 0;
  img_limit_size(src_ht, src_wd, max_wd, &lh, &lw);
  if (lh > 0) img_aug_size((int)lh, lw, resize_side, &ah, &aw);
  if (lh <= 0 || ah <= 0 || aw <= 0) {
    set_error("apa_image_aug_size: %dx%d (limit %d, side %d) resizes to an empty image", src_ht, src_wd, max_wd,
              resize_side);
    return APA_ERR_INVALID_ARG;
  }
  out[0] = (int32_t)lh; out[1] = lw; out[2] = ah; out[3] = aw;
  return APA_OK;
}

// one slot per sample, as large as the largest L of the batch (the launcher divides the workspace evenly: it
// sees the sizes on the device only)
extern "C" size_t apa_preprocess_images_workspace_bytes(int N, int T, const int32_t* src_hw_host, int max_wd) {
  if (N <= 0 || T <= 0 || !src_hw_host || max_wd <= 0) return 0;
  size_t slot = IMG_WS_ALIGN;
  for (int n = 0; n < N; ++n) {
    const int sh = src_hw_host[2 * n], sw = src_hw_host[2 * n + 1];
    if (sh <= 0 || sw <= 0 || sw <= max_wd) continue;
    long long lh;
    int lw;
    img_limit_size(sh, sw, max_wd, &lh, &lw);
    if (lh <= 0) continue;
    const size_t need = (size_t)T * (size_t)lh * (size_t)lw * 3;
    if (need > slot) slot = need;
  }
  return (size_t)N * align_up(slot, IMG_WS_ALIGN);
}

extern "C" int apa_preprocess_images(const uint8_t* src, size_t src_bytes, const int64_t* src_off,
                                     const int32_t* src_hw, const int32_t* geom, int N, int T, int max_wd,
                                     float mean, void* out, int out_dtype, int32_t* status, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (!src || !src_off || !src_hw || !geom || !out || !status || N <= 0 || T <= 0 || max_wd <= 0 ||
      src_bytes == 0) {
    set_error("apa_preprocess_images: null pointer or non-positive size");
    return APA_ERR_INVALID_ARG;
  }
  if (out_dtype != APA_DTYPE_F32 && out_dtype != APA_DTYPE_BF16) {
    set_error("apa_preprocess_images: out_dtype %d", out_dtype);
    return APA_ERR_INVALID_ARG;
  }
  if (N > 65535) {
    set_error("apa_preprocess_images: N=%d > 65535", N);
    return APA_ERR_UNSUPPORTED;
  }
  const size_t ws_slot = (ws_bytes / (size_t)N) / IMG_WS_ALIGN * IMG_WS_ALIGN;
  if (!ws || ws_slot < IMG_WS_ALIGN) {
    set_error("apa_preprocess_images: workspace of %zu bytes for %d samples (see apa_preprocess_images_workspace_bytes)",
              ws_bytes, N);
    return APA_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(IMG_ROW_BLOCKS, N), block(IMG_THREADS);
  hipLaunchKernelGGL(image_limit_kernel, grid, block, 0, st, src, src_bytes, src_off, src_hw, geom, T, max_wd,
                     static_cast<uint8_t*>(ws), ws_slot);
  APA_LAUNCH_CHECK("image_limit_kernel");
  if (out_dtype == APA_DTYPE_F32)
    hipLaunchKernelGGL(image_crop_kernel<float>, grid, block, 0, st, src, src_bytes, src_off, src_hw, geom, T,
                       max_wd, mean, static_cast<float*>(out), status, static_cast<const uint8_t*>(ws), ws_slot);
  else
    hipLaunchKernelGGL(image_crop_kernel<bf16_t>, grid, block, 0, st, src, src_bytes, src_off, src_hw, geom, T,
                       max_wd, mean, static_cast<bf16_t*>(out), status, static_cast<const uint8_t*>(ws), ws_slot);
  APA_LAUNCH_CHECK("image_crop_kernel");
  return APA_OK;
}
