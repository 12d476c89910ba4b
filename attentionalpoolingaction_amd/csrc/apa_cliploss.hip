// apa_cliploss.hip -- the action loss of a video clip, value + gradient, in two launches:
//   frame pooling / temporal attention   models/slim/nets/nets_factory.py:354-374 (reference)
//   softmax cross-entropy on the POOLED logits                     src/loss.py:74-80
//   and the whole backward down to the frame logits (tf.gradients in the reference).
// x = frame logits [B*F, K] (row b*F + f), labels [B]:
//   a[r]        = x[r,:] . w + b0                       (temporal attention; 1 without)     -> tatt
//   pooled[b,k] = (1/F) sum_f x[b,f,k] a[b,f]                                                -> pooled
//   loss[1+b]   = -log softmax(pooled[b])[labels[b]];   loss[0] = wt/B sum_b loss[1+b]
//   g[b,k]      = wt grad_scale / B (softmax(pooled[b])[k] - [k == labels[b]])
//   d[r]        = (1/F) sum_k g[b,k] x[r,k]
//   G[r,k]      = (1/F) g[b,k] a[r] + d[r] w[k]         (the d / w terms vanish without temporal attention)
//   dw[k]       = sum_r d[r] x[r,k];   db0 = sum_r d[r]                    (fixed order over the rows)
// It replaces the module path's five launches (fp_att, fp_pool, softmax_xent, fp_bwd, fp_bwd_w) and the four
// round trips through memory between them.  These tensors are tiny ([B*F, K] with K = 51, F <= 25): the launches
// are latency chains, so the first one keeps a whole clip in one block -- a[], the pooled row and the gradient row
// never leave the CU between the stages -- and the second one only does what needs every clip.
//
//   launch 1  clip_xent_kernel     one 4-wave block per clip: a (one wave per frame row), pooled (one thread per
//                                  column), the row's cross-entropy (wave 0), G and d (one wave per frame row)
//   launch 2  clip_finish_kernel   block 0: the batch mean loss[0] and db0; blocks 1..: 256 columns of dw each
//                                  (temporal attention only)
//
// Which K takes which code:
//   4 <= K <= 1024   the cross-entropy is pc_row_xent_any (apa_xent_row.h): softmax_xent_kernel<NV4>'s row routine in
//                    its three-pass form, on the pooled row in LDS
//   K < 4, K > 1024  xent_row_stream, softmax_xent_stream_kernel's row routine (one wave, three passes, expf)
//   loss[0]          the order xent_mean_slots32(B, K) picks, as there
//   K <= 4096        the pooled row and the gradient row live in LDS (32 KB at most)
//   K >  4096        they live in memory: the pooled row in its output, the gradient row in the workspace
// so that with F == 1 and no temporal attention (pooled = x * 1, G = g * 1) loss and G carry the very bits
// apa_softmax_xent_fwd_bwd gives.  No atomics; every sum has one order: identical calls give identical bits.
//
// ML (apa_clip_multilabel_fwd_bwd): the sigmoid losses of src/loss.py:88-101 in place of the softmax row -- labels are
// f32 multi-hot [B,K], loss[1+b] = (1/K) sum_k l(pooled[b,k], t[b,k]), g[b,k] = wt grad_scale/(B K) l' -- by ml_row
// (apa_device.h) on the whole block, for every K; pooling, tatt, G, d, dw / db, the row placement and launch 2 are the
// softmax form's.  With F == 1 and no temporal attention: apa_multilabel_loss_fwd_bwd's bits.
#include <math.h>

#include "apa_clip_stages.h"
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

// dynamic LDS: [row_floats] pooled row | [row_floats] gradient row | [CLIP_LDS_F] a | [4] xent scratch
template <bool TEMPORAL, bool ML>
__global__ __launch_bounds__(256) void clip_xent_kernel(
    const float* __restrict__ x, const void* __restrict__ labels_any, const float* __restrict__ w,
    const float* __restrict__ b0, float* __restrict__ pooled, float* __restrict__ tatt,
    float* __restrict__ loss, float* __restrict__ G, float* __restrict__ dws, float* __restrict__ gws,
    int F, int K, int row_floats, float gscale, int kind, float pw) {
  const int64_t* __restrict__ labels = static_cast<const int64_t*>(labels_any);
  extern __shared__ __attribute__((aligned(16))) float clip_sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const size_t rb = (size_t)b * F;                 // first frame row of the clip
  const bool rows_lds = row_floats > 0;
  float* prow = rows_lds ? clip_sm : pooled + (size_t)b * K;
  float* grow = rows_lds ? clip_sm + row_floats : gws + (size_t)b * K;
  float* sa = clip_sm + 2 * row_floats;
  float* sx = sa + CLIP_LDS_F;
  const float invF = 1.0f / (float)F;
  const float* ap = nullptr;

  // a[r] = x[r,:] . w + b0, then pooled[b,k]: the stages clip_scores_kernel shares (apa_clip_stages.h)
  if (TEMPORAL) ap = clip_tatt_stage(x, w, b0, tatt, sa, F <= CLIP_LDS_F, rb, F, K);
  clip_pool_stage<TEMPORAL>(x, ap, prow, rows_lds ? pooled + (size_t)b * K : nullptr, rb, F, K);
  __syncthreads();

  if (ML) {   // the pooled row's sigmoid loss, on the whole block: loss[1+b] and the gradient row
    const float s = ml_row<0>([&](int, int k) { return prow[k]; }, static_cast<const float*>(labels_any) + (size_t)b * K,
                              grow, K, kind, pw, gscale, sx);
    if (threadIdx.x == 0) loss[1 + b] = s;
  } else if (wave == 0) {   // the pooled row's cross-entropy: loss[1+b] and the gradient row
    if (xent_row_half_wave(K)) {
      // a one-row problem for the shared row routine: row 0 of (labels + b, sx, grow)
      const PcXent xe = {labels + b, sx, grow, gscale};
      pc_row_xent_any(prow, 0, K, xe, true, grow);
      if (lane == 0) loss[1 + b] = sx[1];
    } else {
      const float lv =
          xent_row_stream([&](int k) { return prow[k]; }, K, (int)labels[b], false, nullptr, true, grow, gscale, nullptr);
      if (lane == 0) loss[1 + b] = lv;
    }
  }
  __syncthreads();

  // the gradient at the frame logits, one wave per frame row
  for (int f = wave; f < F; f += 4)
    clip_grad_row<TEMPORAL>(x, w, grow, TEMPORAL ? ap + f : nullptr, G, dws, rb + f, K, invF, lane);
}

// block 0: loss[0] (in apa_softmax_xent_fwd_bwd's summation order for this (B, K), apa_xent_row.h) and db0; block 1 + j:
// dw[256 j ..]
__global__ __launch_bounds__(256) void clip_finish_kernel(const float* __restrict__ x, const float* __restrict__ dws,
                                                          float* __restrict__ loss, float* __restrict__ dw,
                                                          float* __restrict__ db, int B, int rows, int K,
                                                          float lscale) {
  __shared__ float red[32];
  if (blockIdx.x == 0) {
    if (xent_mean_slots32(B, K)) {
      if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const float t = xent_mean32_finish(xent_mean32_load(loss + 1, B, lane), red, lane);
        if (lane == 0) loss[0] = t * lscale;
      }
    } else {
      const float t = block_sum256(xent_mean256_load(loss + 1, B), red);
      if (threadIdx.x == 0) loss[0] = t * lscale;
    }
    if (dws) {   // db0 in the 256-thread order
      __syncthreads();   // (red is still read by the loss sum)
      const float s = block_sum256(xent_mean256_load(dws, rows), red);
      if (threadIdx.x == 0) db[0] = s;
    }
    return;
  }
  const int k = (blockIdx.x - 1) * 256 + threadIdx.x;
  if (k >= K) return;
  dw[k] = clip_dw_col(x, dws, rows, K, k);
}

// d [B*F] (temporal attention) | gradient rows [B, K] (K > CLIP_LDS_K), in floats
static size_t clip_ws_floats(int B, int F, int K, bool temporal, size_t* off_g) {
  const size_t nd = temporal ? align_up((size_t)B * F, 4) : 0;
  if (off_g) *off_g = nd;
  return nd + (K > CLIP_LDS_K ? (size_t)B * K : 0);
}

int clip_loss_finish(const float* x, const float* dws, float* loss, float* dw, float* db, int B, int rows, int K,
                     float lscale, hipStream_t st) {
  const int nb = 1 + (dws ? (K + 255) / 256 : 0);
  hipLaunchKernelGGL(clip_finish_kernel, dim3(nb), dim3(256), 0, st, x, dws, loss, dw, db, B, rows, K, lscale);
  APA_LAUNCH_CHECK("clip_finish_kernel");
  return APA_OK;
}

}  // namespace apa

using namespace apa;

// both launches; ml: the sigmoid form (labels f32 [B,K]), null: the softmax cross-entropy (labels int64 [B])
static int clip_loss_launch(const char* fn, const apa_multilabel* ml, const float* logits, const void* labels,
                            const float* w, const float* b, float* pooled, float* tatt, float* loss, float* G,
                            float* dw, float* db, void* ws, size_t ws_bytes, int B, int F, int K, float wt,
                            float grad_scale, void* stream) {
  if (B <= 0 || F <= 0 || K <= 0 || (int64_t)B * F > INT32_MAX) {
    set_error("%s: non-positive size or B*F past 2^31 (B=%d F=%d K=%d)", fn, B, F, K);
    return APA_ERR_INVALID_ARG;
  }
  if (!logits || !labels || !pooled || !loss || !G || (w && (!b || !tatt || !dw || !db))) {
    set_error("%s: null pointer (temporal attention needs b, tatt, dw and db)", fn);
    return APA_ERR_INVALID_ARG;
  }
  const bool temporal = w != nullptr;
  size_t off_g = 0;
  const size_t need = clip_ws_floats(B, F, K, temporal, &off_g) * sizeof(float);
  if (need && (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 3))) {
    set_error("%s: workspace too small or misaligned (%zu < %zu)", fn, ws_bytes, need);
    return APA_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* dws = temporal ? static_cast<float*>(ws) : nullptr;
  float* gws = K > CLIP_LDS_K ? static_cast<float*>(ws) + off_g : nullptr;
  const int row_floats = K > CLIP_LDS_K ? 0 : (K + 3) / 4 * 4;
  const size_t shm = (size_t)(2 * row_floats + CLIP_LDS_F + 4) * sizeof(float);
  // the same two factors as apa_softmax_xent_fwd_bwd (ml: apa_multilabel_loss_fwd_bwd), over the B clips
  float lscale = wt / (float)B;
  float gscale = wt * grad_scale / (float)B;
  const int kind = ml ? ml->kind : 0;
  const float pw = ml ? ml->pos_weight : 1.f;
  if (ml) ml_scales(kind, wt, grad_scale, B, K, &lscale, &gscale);
#define APA_CX(T, M)                                                                                                 \
  hipLaunchKernelGGL((clip_xent_kernel<T, M>), dim3(B), dim3(256), shm, st, logits, labels, w, b, pooled, tatt, loss, \
                     G, dws, gws, F, K, row_floats, gscale, kind, pw)
  if (ml) {
    if (temporal) APA_CX(true, true); else APA_CX(false, true);
  } else {
    if (temporal) APA_CX(true, false); else APA_CX(false, false);
  }
#undef APA_CX
  APA_LAUNCH_CHECK("clip_xent_kernel");
  return clip_loss_finish(logits, dws, loss, dw, db, B, B * F, K, lscale, st);
}

extern "C" size_t apa_clip_xent_workspace_bytes(int B, int F, int K) {
  if (B <= 0 || F <= 0 || K <= 0 || (int64_t)B * F > INT32_MAX) return 0;
  const size_t n = clip_ws_floats(B, F, K, true, nullptr) * sizeof(float);
  return n < 16 ? 16 : n;
}

extern "C" int apa_clip_xent_fwd_bwd(const float* logits, const int64_t* labels, const float* w, const float* b,
                                     float* pooled, float* tatt, float* loss, float* G, float* dw, float* db,
                                     void* ws, size_t ws_bytes, int B, int F, int K, float wt, float grad_scale,
                                     void* stream) {
  return clip_loss_launch("apa_clip_xent_fwd_bwd", nullptr, logits, labels, w, b, pooled, tatt, loss, G, dw, db, ws,
                          ws_bytes, B, F, K, wt, grad_scale, stream);
}

extern "C" int apa_clip_multilabel_fwd_bwd(const apa_multilabel* ml, const float* logits, const float* w,
                                           const float* b, float* pooled, float* tatt, float* loss, float* G,
                                           float* dw, float* db, void* ws, size_t ws_bytes, int B, int F, int K,
                                           float wt, float grad_scale, void* stream) {
  const int rc = check_multilabel("apa_clip_multilabel_fwd_bwd", ml);
  if (rc != APA_OK) return rc;
  return clip_loss_launch("apa_clip_multilabel_fwd_bwd", ml, logits, ml->labels, w, b, pooled, tatt, loss, G, dw, db,
                          ws, ws_bytes, B, F, K, wt, grad_scale, stream);
}
