// apa_clipscores.hip -- what an evaluation step does behind the frame logits, in ONE launch:
//   frame pooling / temporal attention   models/slim/nets/nets_factory.py:354-374 (reference)
//   scores and prediction                src/eval.py:193-197
// the forward-only sibling of clip_xent_kernel (apa_cliploss.hip).  x = frame logits [B*F, K] (row b*F + f):
//   a[r]        = x[r,:] . w + b0                       (temporal attention; 1 without)     -> tatt
//   pooled[b,k] = (1/F) sum_f x[b,f,k] a[b,f]                                                -> pooled
//   softmax:  scores[b,:] = softmax(pooled[b,:]);  pred[b] = first maximal index;
//             labels given: loss[1+b] = -log softmax(pooled[b])[labels[b]], loss[0] = (1/B) sum_b loss[1+b]
//   sigmoid:  scores[b,k] = 1 / (1 + expf(-pooled[b,k]))   (ml_term's expression, contraction off)
//             pred[b] = first maximal index of pooled[b,:]  (argmax of the LOGITS, eval.py:193)
// It replaces fp_att + fp_pool + the softmax launch (and, without ground truth, the zero-label scratch and its memset)
// or, for the sigmoid scores, the tensor expressions of eval_utils.predict.  One 4-wave block per clip: a[] and the
// pooled row stay on the CU.  a[] and pooled come from the stages clip_xent_kernel runs (apa_clip_stages.h), so they
// carry apa_clip_xent_fwd_bwd's and apa_frame_pool_fwd's bits; the softmax row carries apa_softmax_xent_fwd_bwd's:
//   4 <= K <= 1024   pc_row_softmax_any (apa_xent_row.h): softmax_xent_kernel<NV4>'s row routine in its three-pass
//                    form, on the row in LDS
//   K < 4, K > 1024  xent_row_stream, softmax_xent_stream_kernel's row routine (one wave, three passes, expf)
//   K <= 4096        the pooled row lives in LDS; beyond that in its output
//   F <= 64          a[b, :] lives in LDS; beyond that it is re-read from tatt
// loss[0] needs every clip and a launch has no order between its blocks, so with labels ONE MORE block walks all B
// clips again -- the same stages on the same inputs, hence the same bits, nothing stored but loss[0] -- and adds the
// rows' losses in apa_softmax_xent_fwd_bwd's order for (B, K): thread n mod 32 takes row n and the 32 slots are added
// in order (4 <= K <= 1024 and B <= 64), else sum_scale_kernel's order (thread n mod 256, wave trees, (w0 + w1) + (w2 +
// w3)).  That block reads nothing another block writes: its a[] is always in LDS (the host sizes the region), and a
// pooled row too long for LDS is formed again per pass instead of being read back.  It is B clips of latency on one
// CU, the price of one launch without atomics; evaluation with ground truth runs it on a handful of clips.
// labels == NULL: no loss, no extra block, no scratch.  No atomics; identical calls give identical bits.
#include <math.h>

#include "apa_clip_stages.h"
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

constexpr int CLIP_SCORES_MAX_F_LABELS = 8192;   // the loss block keeps a[b, :] in LDS (32 KB)

// dynamic LDS: [row_floats] pooled row | [4] scratch | [32] loss slots | [CLIP_LDS_F, or F with labels] a
// grid: B blocks, one per clip (+ 1 with labels: the loss block).  pooled == nullptr: F == 1 without attention, the
// logits rows are the pooled rows.
template <bool TEMPORAL, bool SIGMOID>
__global__ __launch_bounds__(256) void clip_scores_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ labels, const float* __restrict__ w,
    const float* __restrict__ b0, float* __restrict__ pooled, float* __restrict__ tatt, float* __restrict__ scores,
    int64_t* __restrict__ pred, float* __restrict__ loss, int B, int F, int K, int row_floats, float lscale) {
  extern __shared__ __attribute__((aligned(16))) float cs_sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool rows_lds = row_floats > 0;
  float* srow = cs_sm;
  float* sx = cs_sm + row_floats;
  float* slot = sx + 4;
  float* sa = slot + 32;
  const bool loss_block = (int)blockIdx.x == B;
  const bool row_routine = xent_row_half_wave(K);
  const bool slots32 = xent_mean_slots32(B, K);
  float own = 0.f;   // loss block: this thread's share of loss[0]
  const int b_lo = loss_block ? 0 : blockIdx.x, b_hi = loss_block ? B : blockIdx.x + 1;

  for (int b = b_lo; b < b_hi; ++b) {
    const size_t rb = (size_t)b * F;   // first frame row of the clip
    const float* ap = nullptr;
    if (TEMPORAL)
      ap = clip_tatt_stage(x, w, b0, loss_block ? nullptr : tatt, sa, loss_block || F <= CLIP_LDS_F, rb, F, K);
    // where the pooled row is read from: LDS, its output, the logits themselves -- or (loss block, K > CLIP_LDS_K)
    // nowhere: formed again in each pass
    const float* prow = nullptr;
    if (rows_lds) {
      clip_pool_stage<TEMPORAL>(x, ap, srow, (pooled && !loss_block) ? pooled + (size_t)b * K : nullptr, rb, F, K);
      prow = srow;
    } else if (!pooled) {
      prow = x + rb * K;
    } else if (!loss_block) {
      clip_pool_stage<TEMPORAL>(x, ap, pooled + (size_t)b * K, nullptr, rb, F, K);
      prow = pooled + (size_t)b * K;
    }
    __syncthreads();

    if (SIGMOID) {   // the whole block: one thread per column
      float m = -INFINITY;
      int arg = 0x7fffffff;
      for (int k = threadIdx.x; k < K; k += 256) {
#pragma clang fp contract(off)
        const float v = prow[k];
        scores[(size_t)b * K + k] = 1.0f / (1.0f + expf(-v));
        if (v > m) { m = v; arg = k; }   // first maximal index of this thread
      }
      const float mw = wave_max(m);
      const int cw = wave_min_i((m == mw) ? arg : 0x7fffffff);
      if (lane == 0) {
        sx[wave] = mw;
        slot[wave] = __builtin_bit_cast(float, cw);
      }
      __syncthreads();
      if (threadIdx.x == 0) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = 0; v < 4; ++v) {
          const int ci = __builtin_bit_cast(int, slot[v]);
          if (sx[v] > best || (sx[v] == best && ci < bi)) { best = sx[v]; bi = ci; }
        }
        pred[b] = bi;
      }
    } else {
      if (wave == 0) {   // the pooled row's softmax, prediction and loss
        const int lab = labels ? (int)labels[b] : -1;
        float* prb = loss_block ? nullptr : scores + (size_t)b * K;
        float lv;
        int cand;
        if (row_routine) {   // (K <= 1024 < CLIP_LDS_K: the row is in LDS)
          pc_row_softmax_any(prow, K, lab, prb, &lv, &cand);
        } else if (prow) {
          lv = xent_row_stream([&](int k) { return prow[k]; }, K, lab, !loss_block, prb, false, nullptr, 0.f, &cand);
        } else {
          lv = xent_row_stream([&](int k) { return clip_pool_col<TEMPORAL>(x + rb * K + k, ap, F, K); }, K, lab,
                               !loss_block, prb, false, nullptr, 0.f, &cand);
        }
        if (lane == 0) {
          if (loss_block) {
            sx[1] = lv;
          } else {
            pred[b] = cand;
            if (labels) loss[1 + b] = lv;
          }
        }
      }
      if (loss_block) {   // row b joins its thread's sum, rows in increasing b
        __syncthreads();
        if ((int)threadIdx.x == (slots32 ? (b & 31) : (b & 255))) own += sx[1];
      }
    }
  }

  // loss[0]: the thread's share is its slot's sum (32-slot order) or its strided sum (256-thread order); the finish is
  // apa_xent_row.h's
  if (!SIGMOID && loss_block) {
    if (slots32) {
      if (wave == 0) {
        const float t = xent_mean32_slots(own, slot, lane);
        if (lane == 0) loss[0] = t * lscale;
      }
    } else {
      const float t = block_sum256(own, slot);
      if (threadIdx.x == 0) loss[0] = t * lscale;
    }
  }
}

int clip_scores_launch(const char* fn, int kind, const float* logits, const float* w, const float* b,
                       const int64_t* labels, float* pooled, float* tatt, float* scores, int64_t* pred, float* loss,
                       int B, int F, int K, hipStream_t st) {
  const bool temporal = w != nullptr, sigmoid = kind == APA_SCORES_SIGMOID;
  if (labels && F > CLIP_SCORES_MAX_F_LABELS) {
    set_error("%s: the loss of clips of more than %d frames is not served (F=%d): run without labels", fn,
              CLIP_SCORES_MAX_F_LABELS, F);
    return APA_ERR_UNSUPPORTED;
  }
  const int row_floats = K > CLIP_LDS_K ? 0 : (K + 3) / 4 * 4;
  const int a_floats = labels && F > CLIP_LDS_F ? F : CLIP_LDS_F;
  const size_t shm = (size_t)(row_floats + 4 + 32 + a_floats) * sizeof(float);
  const int nb = B + (labels ? 1 : 0);
  const float lscale = 1.0f / (float)B;   // apa_softmax_xent_fwd_bwd's wt / N with wt = 1
#define APA_CS(T, S)                                                                                              \
  hipLaunchKernelGGL((clip_scores_kernel<T, S>), dim3(nb), dim3(256), shm, st, logits, labels, w, b, pooled, tatt, \
                     scores, pred, loss, B, F, K, row_floats, lscale)
  if (sigmoid) {
    if (temporal) APA_CS(true, true); else APA_CS(false, true);
  } else {
    if (temporal) APA_CS(true, false); else APA_CS(false, false);
  }
#undef APA_CS
  APA_LAUNCH_CHECK("clip_scores_kernel");
  return APA_OK;
}

}  // namespace apa

using namespace apa;

extern "C" int apa_clip_scores(int kind, const float* logits, const float* w, const float* b, const int64_t* labels,
                               float* pooled, float* tatt, float* scores, int64_t* pred, float* loss, int B, int F,
                               int K, void* stream) {
  if (kind != APA_SCORES_SOFTMAX && kind != APA_SCORES_SIGMOID) {
    set_error("apa_clip_scores: unknown scores kind %d", kind);
    return APA_ERR_INVALID_ARG;
  }
  if (B <= 0 || F <= 0 || K <= 0 || (int64_t)B * F > INT32_MAX) {
    set_error("apa_clip_scores: non-positive size or B*F past 2^31 (B=%d F=%d K=%d)", B, F, K);
    return APA_ERR_INVALID_ARG;
  }
  if (!logits || !pooled || !scores || !pred || (w && (!b || !tatt))) {
    set_error("apa_clip_scores: null pointer (temporal attention needs b and tatt)");
    return APA_ERR_INVALID_ARG;
  }
  if ((labels == nullptr) != (loss == nullptr)) {
    set_error("apa_clip_scores: labels and loss must be given together");
    return APA_ERR_INVALID_ARG;
  }
  if (kind == APA_SCORES_SIGMOID && labels) {
    set_error("apa_clip_scores: the sigmoid scores take no labels / loss (eval.py computes none)");
    return APA_ERR_INVALID_ARG;
  }
  return clip_scores_launch("apa_clip_scores", kind, logits, w, b, labels, pooled, tatt, scores, pred, loss, B, F, K,
                            static_cast<hipStream_t>(stream));
}
