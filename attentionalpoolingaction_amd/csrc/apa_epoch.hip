// apa_epoch.hip -- the visiting order of one epoch over a resident feature cache, drawn on the device in ONE launch
// (apa.h: apa_epoch_order): order[i] = the image visited at position i, a permutation of [0, T) that every element
// computes on its own from (seed, epoch, i, T).  No atomics, no workspace, no sort, no allocation; capturable.
//
// The rule (apa.h states it for a host restatement; custom_ops_factory._epoch_order_rule_cpu is one):
//   b  = max(2, number of bits of T - 1): the walk's domain is [0, 2^b), the smallest power of two >= max(T, 4)
//   lb = b / 2 bits in the left half, rb = b - lb in the right half: x = (L << rb) | R
//   h  = splitmix64(seed, epoch), key_r = splitmix64(h, r) for r = 0..5 -- rng_key's derivation (apa_internal.h), the
//        low word of key_r is k0, the high word k1
//   round r even: L ^= rng_hash(R, k0, k1) & (2^lb - 1);  r odd: R ^= rng_hash(L, k0, k1) & (2^rb - 1)
//        (rng_hash: the dropout mask's two-round 24-bit multiply-xorshift mix, apa_device.h)
//   six rounds are one bijection of the domain; it is applied to i, and again while the image is >= T (cycle walking:
//   the orbit of i < T returns below T after at most 2^b - T + 1 applications; 2^b < 2 T for T >= 3, so two on average).
// Behind it, host only: the epoch calls that visit such an order (apa.h: apa_epoch; apa_clip_epoch.h), one driver for
// training and one for evaluation, each a loop over the one-call step of apa_capi.h.
#include "../../include/apa_clip_epoch.h"
#include "apa_capi.h"
#include "apa_device.h"

namespace apa {

constexpr int EPOCH_ROUNDS = 6;
struct EpochKeys { uint32_t k0[EPOCH_ROUNDS], k1[EPOCH_ROUNDS]; };

__device__ __forceinline__ uint32_t epoch_feistel(uint32_t x, const EpochKeys& k, int rb, uint32_t mL, uint32_t mR) {
  uint32_t L = x >> rb, R = x & mR;
#pragma unroll
  for (int r = 0; r < EPOCH_ROUNDS; r += 2) {
    L ^= rng_hash(R, k.k0[r], k.k1[r]) & mL;
    R ^= rng_hash(L, k.k0[r + 1], k.k1[r + 1]) & mR;
  }
  return (L << rb) | R;
}

__global__ __launch_bounds__(256) void epoch_order_kernel(int32_t* __restrict__ order, uint32_t T, EpochKeys k, int rb,
                                                          uint32_t mL, uint32_t mR) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  uint32_t x = epoch_feistel((uint32_t)i, k, rb, mL, mR);
  while (x >= T) x = epoch_feistel(x, k, rb, mL, mR);
  order[i] = (int32_t)x;
}

}  // namespace apa

using namespace apa;

extern "C" int apa_epoch_order(int32_t* order, int T, uint64_t seed, uint64_t epoch, void* stream) {
  const char* fn = "apa_epoch_order";
  if (!order || (reinterpret_cast<uintptr_t>(order) & 3)) {
    set_error("%s: order must be a 4-byte aligned device pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (T < 1) {
    set_error("%s: T=%d: an epoch visits at least one image", fn, T);
    return APA_ERR_INVALID_ARG;
  }
  int b = 2;
  while (b < 31 && (1u << b) < (uint32_t)T) ++b;
  const int lb = b / 2, rb = b - lb;
  EpochKeys k;
  uint32_t h0, h1;
  rng_key(seed, epoch, &h0, &h1);
  const uint64_t h = ((uint64_t)h1 << 32) | h0;
  for (int r = 0; r < EPOCH_ROUNDS; ++r) rng_key(h, (uint64_t)r, &k.k0[r], &k.k1[r]);
  const unsigned blocks = (unsigned)(((size_t)T + 255) / 256);
  hipLaunchKernelGGL(epoch_order_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), order,
                     (uint32_t)T, k, rb, (1u << lb) - 1u, (1u << rb) - 1u);
  APA_LAUNCH_CHECK("epoch_order_kernel");
  return APA_OK;
}

// ---- a whole epoch over the cache behind one host call (apa.h: apa_epoch; apa_clip_epoch.h) --------------------------
// One driver per direction.  It IS the loop over the *_cached step it names (and, training, apa_momentum_sgd_step
// behind each step): the same step function (apa_capi.h) on the same request, so the same launches and the same bits.
// What is added is the order of things: every refusal -- the epoch's, the optimiser's, the sampler's, the step's for the
// shape (both halves, and the evaluation pass's shorter last batch) -- is made before the first launch.
// videos: false: `order` holds image ids, a step takes its N rows of it as the index.  true (apa_clip_epoch.h): `order`
// holds video ids, a step takes B = N / F of them and the keyed sampler (apa_clip_epoch.hip), launched in front of it,
// turns them into the step's frame index, labels and targets; ce is then required.

// the epoch's own refusals; *rows: ids per step (N images, or B videos of F frames), *steps: the steps it runs
static int epoch_check(const char* fn, const apa_epoch* ep, const apa_feature_cache* cache, bool videos,
                       const apa_clip_epoch* ce, const apa_clip_pool* clip, int N, bool train, int* rows, int* steps) {
  if (!ep || !ep->order) {
    set_error("%s: null apa_epoch / order pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (!cache) {
    set_error("%s: null apa_feature_cache", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (videos && !ce) {
    set_error("%s: null apa_clip_epoch", fn);
    return APA_ERR_INVALID_ARG;
  }
  const int F = clip ? clip->frames : 1;
  if (!videos && N <= 0) {
    set_error("%s: non-positive batch size N=%d", fn, N);
    return APA_ERR_INVALID_ARG;
  }
  if (N <= 0 || F <= 0 || N % F != 0) {
    set_error("%s: N=%d is not a whole, positive number of clips of %d frames", fn, N, F);
    return APA_ERR_INVALID_ARG;
  }
  const int b = N / F;
  const char* const unit = videos ? "video" : "image";
  const char letter = videos ? 'B' : 'N';
  if (train ? (ep->count < b || ep->count % b != 0) : ep->count < 1) {
    if (train)
      set_error("%s: apa_epoch.count=%d is not a whole, positive number of batches of %c=%d %ss", fn, ep->count, letter,
                b, unit);
    else
      set_error("%s: apa_epoch.count=%d: an evaluation pass visits at least one %s (%c=%d)", fn, ep->count, unit,
                letter, b);
    return APA_ERR_INVALID_ARG;
  }
  const long long s = ((long long)ep->count + b - 1) / b;
  if (s * b > 0x7fffffffLL) {
    set_error("%s: steps * %c = %lld is past 2^31 - 1 (count=%d, %c=%d)", fn, letter, s * b, ep->count, letter, b);
    return APA_ERR_INVALID_ARG;
  }
  *rows = b;
  *steps = (int)s;
  return APA_OK;
}

// what sgd_launch (apa_optim.hip) refuses about apa_momentum_sgd_step's arguments, before the first step
static int epoch_sgd_check(const char* fn, const apa_epoch_sgd* o) {
  if (o->nseg <= 0 || o->nseg > APA_SGD_MAX_SEGMENTS || !o->weights || !o->sizes || !o->weight_decay ||
      !o->grad_flat || !o->acc_flat) {
    set_error("%s: apa_epoch_sgd: bad arguments (nseg=%d, max %d; weights, sizes, weight_decay, grad_flat and acc_flat "
              "must be given)", fn, o->nseg, APA_SGD_MAX_SEGMENTS);
    return APA_ERR_INVALID_ARG;
  }
  for (int i = 0; i < o->nseg; ++i)
    if (!o->weights[i]) {
      set_error("%s: apa_epoch_sgd.weights[%d] is NULL", fn, i);
      return APA_ERR_INVALID_ARG;
    }
  return APA_OK;
}

// the sampler's call of one step: labels / targets are sampled where both the table and the destination are given
static int epoch_sample(const apa_clip_epoch* ce, const int32_t* videos, int64_t* labels, float* targets,
                        int32_t* status, int B, int F, int K, int mode, int step, void* stream) {
  const bool lab = ce->video_labels && labels, tgt = ce->video_targets && targets;
  return apa_sample_clip_frames_keyed(ce->video_first, ce->video_frames, lab ? ce->video_labels : nullptr,
                                      tgt ? ce->video_targets : nullptr, videos, ce->index, lab ? labels : nullptr,
                                      tgt ? targets : nullptr, status, ce->V, B, F, K, mode, ce->seed, ce->epoch,
                                      (uint64_t)step, stream);
}

// what the step will read from the sampler must be sampled; then the sampler's own refusals for the shape
static int epoch_sampler_check(const char* fn, const apa_clip_epoch* ce, const int32_t* videos, bool need_labels,
                               bool need_targets, int B, int F, int K, int mode) {
  if (!ce->index || (reinterpret_cast<uintptr_t>(ce->index) & 3)) {
    set_error("%s: apa_clip_epoch.index must be a 4-byte aligned device pointer (int32 [B*frames] scratch)", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (need_targets && (!ce->video_targets || !ce->targets)) {
    set_error("%s: a sigmoid loss reads the sampled targets: apa_clip_epoch.video_targets and .targets are required", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (need_labels && (!ce->video_labels || !ce->labels)) {
    set_error("%s: the softmax cross-entropy reads the sampled labels: apa_clip_epoch.video_labels and .labels are "
              "required", fn);
    return APA_ERR_INVALID_ARG;
  }
  const bool lab = ce->video_labels && ce->labels, tgt = ce->video_targets && ce->targets;
  return sample_clip_check(fn, ce->video_first, ce->video_frames, lab ? ce->video_labels : nullptr,
                           tgt ? ce->video_targets : nullptr, videos, ce->index, ce->labels, ce->targets, ce->V, B, F, K,
                           mode, false);
}

// r: the step's request as the epoch call was handed it -- r.cache the caller's descriptor, r.loss the log's first row.
// A step-time refusal would carry the step entry point's name, as in the loop this call stands for.
static int train_epoch(const char* fn, const apa_epoch* ep, const apa_epoch_sgd* opt, bool videos,
                       const apa_clip_epoch* ce, HeadTrainStep r) {
  if (!opt || !opt->lr) {
    set_error("%s: null apa_epoch_sgd / lr pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  const int K = r.dims.K;
  int B = 0, steps = 0;
  int rc = epoch_check(fn, ep, r.cache, videos, ce, r.clip, r.dims.N, true, &B, &steps);
  if (rc != APA_OK) return rc;
  if ((rc = epoch_sgd_check(fn, opt)) != APA_OK) return rc;
  const int F = r.dims.N / B;
  apa_feature_cache fc = *r.cache;
  apa_multilabel mls{};
  const int64_t* const labels = r.labels;
  float* const loss = r.loss;
  const uint64_t offset = r.offset;
  r.cache = &fc;
  fc.index = ep->order;
  if (videos) {
    if ((rc = epoch_sampler_check(fn, ce, ep->order, !r.ml, r.ml != nullptr, B, F, K, ce->mode)) != APA_OK) return rc;
    if (r.ml) {   // (its labels are not read: the sampled targets take their place)
      mls = *r.ml;
      mls.labels = ce->targets;
      if ((rc = check_multilabel(fn, &mls)) != APA_OK) return rc;
      r.ml = &mls;
    }
    fc.index = ce->index;
    fc.labels_cached = 0;
    r.labels = ce->labels;
  }
  if ((rc = head_train_check(fn, r)) != APA_OK) return rc;   // the step's checks, once for the shape
  const char* const step_fn = r.sigmoid || r.clips ? "apa_attn_head_train_step_cached_clips"
                                                   : "apa_attn_head_train_step_cached";
  const bool rng_dev = (r.flags & APA_FLAG_RNG_DEVICE) != 0;   // the counter in HBM advances by itself
  for (int s = 0; s < steps; ++s) {
    const size_t row = (size_t)s * B;
    if (videos) {
      rc = epoch_sample(ce, ep->order + row, ce->labels, ce->targets, fc.status, B, F, K, ce->mode, s, r.stream);
      if (rc != APA_OK) return rc;
    } else {
      fc.index = ep->order + row;
      r.labels = (fc.labels_cached || !labels) ? labels : labels + row;
    }
    r.loss = loss + (size_t)s * (1 + B);
    r.offset = rng_dev ? offset : offset + (uint64_t)s;
    if ((rc = head_train_step(step_fn, r)) != APA_OK) return rc;
    rc = apa_momentum_sgd_step(opt->nseg, opt->weights, opt->sizes, opt->weight_decay, opt->grad_flat, opt->acc_flat,
                               opt->lr[s], opt->momentum, opt->grad_scale, r.stream);
    if (rc != APA_OK) return rc;
  }
  return APA_OK;
}

// r: as in train_epoch; the outputs with one row per visited id (probs, pred, loss, the clip's pooled, and logits where
// its rows are per id) advance with the steps.  The last step runs the remaining ids as a smaller batch.
static int eval_epoch(const char* fn, const apa_epoch* ep, bool videos, const apa_clip_epoch* ce, HeadEvalStep r) {
  const int K = r.dims.K;
  int B = 0, steps = 0;
  int rc = epoch_check(fn, ep, r.cache, videos, ce, r.clip, r.dims.N, false, &B, &steps);
  if (rc != APA_OK) return rc;
  const int F = r.dims.N / B;
  const int last = ep->count - (steps - 1) * B;   // ids of the last step, 1..B
  apa_feature_cache fc = *r.cache;
  apa_clip_pool cp{};
  const HeadEvalStep first = r;   // the call's own pointers: step 0's rows
  r.cache = &fc;
  fc.index = ep->order;
  if (videos) {
    rc = epoch_sampler_check(fn, ce, ep->order, r.loss != nullptr, false, B, F, K, APA_CLIP_FRAMES_UNIFORM);
    if (rc != APA_OK) return rc;
    fc.index = ce->index;
    fc.labels_cached = 0;
    r.labels = r.loss ? ce->labels : nullptr;
  }
  for (int b : {B, last}) {   // the step's checks, once for the full batch and once for the last step's shape
    r.dims.N = b * F;
    if ((rc = head_eval_check(fn, r)) != APA_OK) return rc;
  }
  const char* const step_fn = r.clips ? "apa_attn_head_eval_step_cached_clips" : "apa_attn_head_eval_step_cached";
  for (int s = 0; s < steps; ++s) {
    const size_t row = (size_t)s * B;
    const int b = s == steps - 1 ? last : B;
    if (videos) {
      rc = epoch_sample(ce, ep->order + row, ce->labels ? ce->labels + row : nullptr,
                        ce->targets ? ce->targets + row * K : nullptr, fc.status, b, F, K, APA_CLIP_FRAMES_UNIFORM, s,
                        r.stream);
      if (rc != APA_OK) return rc;
      r.labels = first.loss ? ce->labels + row : nullptr;
    } else {
      fc.index = ep->order + row;
      r.labels = (fc.labels_cached || !first.labels) ? first.labels : first.labels + row;
    }
    if (first.clip) {   // frame-level logits stay the last step's; the pooled rows are the per-id rows
      cp = *first.clip;
      cp.pooled = first.clip->pooled + row * K;
      r.clip = &cp;
    } else {
      r.logits = first.logits + row * K;
    }
    r.dims.N = b * F;
    r.loss = first.loss ? first.loss + (size_t)s * (1 + B) : nullptr;
    r.probs = first.probs + row * K;
    r.pred = first.pred + row;
    if ((rc = head_eval_step(step_fn, r)) != APA_OK) return rc;
  }
  return APA_OK;
}

extern "C" int apa_attn_head_train_epoch_cached(const apa_epoch* ep, const apa_epoch_sgd* opt,
                                                const apa_feature_cache* cache, const apa_hooks* hooks, const void* X,
                                                const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                                const float* bt, const int64_t* labels, float loss_wt, float grad_scale,
                                                float* logits, float* att, float* zsave, float* abar, float* loss,
                                                float* G, void* dX, void* dXatt, float* dWa, float* dba, float* dWt,
                                                float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                                                int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                                int dtype, void* stream) {
  HeadTrainStep r{X, Xatt, Wa, ba, Wt, bt, labels, loss_wt, grad_scale, logits, att, zsave, abar, loss, G, dX, dXatt, dWa,
                  dba, dWt, dbt, ws, ws_bytes, {N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, stream, hooks};
  r.cache = cache; r.cached = true;
  return train_epoch("apa_attn_head_train_epoch_cached", ep, opt, false, nullptr, r);
}

extern "C" int apa_attn_head_eval_epoch_cached(const apa_epoch* ep, const apa_feature_cache* cache, int scores_kind,
                                               const void* X, const void* Xatt, const float* Wa, const float* ba,
                                               const float* Wt, const float* bt, const int64_t* labels, float* logits,
                                               float* att, float* zsave, float* abar, float* loss, float* probs,
                                               int64_t* pred, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                                               int K, int M, unsigned flags, int dtype, void* stream) {
  HeadEvalStep r{X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws, ws_bytes,
                 {N, P, C, Ca, K, M, dtype}, flags, stream, scores_kind};
  r.cache = cache; r.cached = true;
  return eval_epoch("apa_attn_head_eval_epoch_cached", ep, false, nullptr, r);
}

// (`labels` of the flat list is not read: the sampler's take its place)
extern "C" int apa_attn_head_train_epoch_cached_clips(
    const apa_epoch* ep, const apa_epoch_sgd* opt, const apa_clip_epoch* ce, const apa_feature_cache* cache,
    const apa_multilabel* ml, const apa_clip_pool* clip, const apa_hooks* hooks, const void* X, const void* Xatt,
    const float* Wa, const float* ba, const float* Wt, const float* bt, const int64_t* labels, float loss_wt,
    float grad_scale, float* logits, float* att, float* zsave, float* abar, float* loss, float* G, void* dX, void* dXatt,
    float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
    unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  HeadTrainStep r{X, Xatt, Wa, ba, Wt, bt, labels, loss_wt, grad_scale, logits, att, zsave, abar, loss, G, dX, dXatt, dWa,
                  dba, dWt, dbt, ws, ws_bytes, {N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, stream, hooks};
  r.cache = cache; r.cached = true;
  r.ml = ml; r.sigmoid = ml != nullptr;
  r.clip = clip; r.clips = clip != nullptr;
  return train_epoch("apa_attn_head_train_epoch_cached_clips", ep, opt, true, ce, r);
}

extern "C" int apa_attn_head_eval_epoch_cached_clips(
    const apa_epoch* ep, const apa_clip_epoch* ce, const apa_feature_cache* cache, const apa_clip_pool* clip,
    int scores_kind, const void* X, const void* Xatt, const float* Wa, const float* ba, const float* Wt, const float* bt,
    const int64_t* labels, float* logits, float* att, float* zsave, float* abar, float* loss, float* probs, int64_t* pred,
    void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags, int dtype, void* stream) {
  HeadEvalStep r{X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws, ws_bytes,
                 {N, P, C, Ca, K, M, dtype}, flags, stream, scores_kind};
  r.cache = cache; r.cached = true;
  r.clip = clip; r.clips = clip != nullptr;
  return eval_epoch("apa_attn_head_eval_epoch_cached_clips", ep, true, ce, r);
}
