/* apa_clip_epoch.h -- a whole CLIP or MULTI-LABEL epoch over a resident frame cache behind ONE host call.
 *
 * The companion of apa.h's epoch calls (apa_attn_head_train_epoch_cached / apa_attn_head_eval_epoch_cached, which serve
 * flat batches under the softmax cross-entropy) for the datasets they leave out: clips (HMDB-51) and the sigmoid losses
 * (HICO, Charades).  Exported by the same library; apa.h itself, its entry points and APA_VERSION are unchanged.
 *
 * Conventions: those of apa.h.  Every function returns APA_OK or an APA_ERR_* code and leaves its reason in
 * apa_last_error(); every launch goes to `stream`, nothing allocates, nothing synchronises, so every entry point here
 * can be captured in a hipGraph; there are no floating-point atomics -- identical calls give identical bits; pointers
 * are device pointers unless a comment says HOST.  What travels BY VALUE and is therefore frozen by a capture:
 * (seed, epoch, step) of the keyed sampler, the learning rates opt->lr[s], an integer dropout offset, every address.
 */
#ifndef APA_CLIP_EPOCH_H_
#define APA_CLIP_EPOCH_H_

#include "apa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * apa_sample_clip_frames with its RANDOM_SEGMENT draws made ON THE DEVICE, keyed by (seed, epoch, step): ONE launch,
 * no workspace, capturable.  It IS apa_sample_clip_frames (same arguments, same frame rule -- apa.h:
 * _get_frame_sublist --, same clamping of a video id into [0,V) and counting in `status`, same labels / targets copy)
 * on these draws, with mix64 and hash exactly as apa.h states them for apa_epoch_order:
 *
 *     h = mix64(mix64(seed, epoch), step);   k0 = low 32 bits of h, k1 = high 32 bits of h
 *     u[j] = (float)(hash(j, k0, k1) >> 8) * 2^-24          j = b * frames + i      (exact in fp32, in [0, 1))
 *
 * Every element is computed on its own; there is no atomic apart from the integer `status` count.  Under
 * APA_CLIP_FRAMES_UNIFORM no draw is taken and (seed, epoch, step) are ignored.  A host restates the rule with
 * apa.h's mix64 / hash (custom_ops/clip_epoch.py: clip_draws_rule_cpu) and gets the same bits from
 * apa_sample_clip_frames fed that u.
 * Refused with APA_ERR_INVALID_ARG before anything is queued -- apa_sample_clip_frames' refusals minus `u`: a null
 * video_first / video_frames / videos / index, video_labels without labels or video_targets without targets,
 * non-positive V / B / frames (K with video_targets), an unknown mode, B * frames past 2^31 - 1. */
int apa_sample_clip_frames_keyed(const int32_t* video_first, const int32_t* video_frames,
                                 const int64_t* video_labels /* NULL */, const float* video_targets /* NULL */,
                                 const int32_t* videos, int32_t* index, int64_t* labels, float* targets,
                                 int32_t* status /* NULL */, int V, int B, int frames, int K, int mode, uint64_t seed,
                                 uint64_t epoch, uint64_t step, void* stream);

/* ------------------------------------------------------------------------------------------
 * What an epoch of clips visits besides apa_epoch: the video tables of apa_sample_clip_frames, the sampler's key and
 * the device scratch the sampler writes and the step reads.  With F = clip->frames (1 without a clip) and B = N / F: */
typedef struct apa_clip_epoch {
  const int32_t* video_first;    /* int32 [V]: cache slot of each video's frame 0                                    */
  const int32_t* video_frames;   /* int32 [V]: its frame count                                                        */
  const int64_t* video_labels;   /* int64 [V], nullable: required where the softmax cross-entropy reads labels        */
  const float* video_targets;    /* f32 [V,K], nullable: required with an apa_multilabel                              */
  int V;
  int mode;                      /* training: APA_CLIP_FRAMES_*; the evaluation pass always samples UNIFORM           */
  uint64_t seed, epoch;          /* the sampler's key; step s of the call draws with (seed, epoch, s)                 */
  int32_t* index;                /* caller-owned scratch, int32 [B*F], 4-byte aligned: the step's frame index         */
  int64_t* labels;               /* training: scratch int64 [B]; evaluation: OUTPUT int64 [count], row-aligned        */
  float* targets;                /* training: scratch f32 [B,K]; evaluation: OUTPUT f32 [count,K], row-aligned        */
} apa_clip_epoch;

/* apa_attn_head_train_epoch_cached_clips(ep, opt, ce, cache, ml, clip, hooks, <the arguments of
 * apa_attn_head_train_step_cached_clips from X on>) IS, bit for bit in every output, weight and accumulator, this loop
 * of steps = ep->count / B passes (ep->order holds VIDEO ids; apa_epoch_order on V gives such an order):
 *   for s in 0 .. steps-1:
 *     apa_sample_clip_frames_keyed(ce->video_*, videos = ep->order + s*B, ce->index, ce->labels, ce->targets,
 *                                  cache->status, ce->V, B, F, K, ce->mode, ce->seed, ce->epoch, step = s)
 *     apa_attn_head_train_step_cached_clips(cache{index = ce->index, labels_cached = 0}, ml{labels = ce->targets},
 *                                           clip, hooks, ..., labels = ce->labels, dropout offset + s,
 *                                           loss + s*(1+B))
 *     apa_momentum_sgd_step(opt->nseg .. opt->acc_flat, opt->lr[s], opt->momentum, opt->grad_scale, stream)
 * ml == NULL: the softmax cross-entropy on the sampled labels (ce->video_labels and ce->labels required); ml given:
 * its sigmoid loss on the sampled targets -- ml->labels is NOT read, ce->targets takes its place (ce->video_targets and
 * ce->targets required) and labels are sampled only where ce->video_labels and ce->labels are both given.  clip->w may
 * be NULL (plain frame mean) or the temporal-attention conv, whose dw / db are segments of opt->grad_flat like every
 * other gradient.  clip == NULL, or clip->frames == 1: one-frame videos, the flat multi-label datasets (apa.h promises
 * that form is bit-identical to the flat multi-label step).  The `labels` argument of the flat list is not read (it may
 * be NULL).  cache->index and cache->labels_cached are ignored; cache->status counts clamped VIDEO ids (the sampler's)
 * and clamped frame ids (the step's; none unless the tables name slots outside the cache).  Under APA_FLAG_RNG_DEVICE
 * the counter in HBM advances by itself and `offset` is passed unchanged.  loss is the epoch's log [steps][1+B]; logits,
 * att, zsave, abar, G, clip->pooled and clip->tatt hold the last step's values.  opt->lr is a HOST array read during
 * the call.  No allocation, no synchronisation; workspace: the step's (apa_clip_step_workspace_bytes with a clip,
 * apa_attn_pool_workspace_bytes without).
 * Served: the class-agnostic head (M == 1) on fp32, bf16 and FP8 caches.  Refused before the first launch, in this
 * order:
 *   1. APA_ERR_INVALID_ARG: a NULL opt / lr; a NULL ep / order; a NULL cache; a NULL ce; N < 1 or N not a whole number
 *      of clips of clip->frames frames; count < B or count % B != 0; steps * B past 2^31 - 1;
 *   2. what apa_momentum_sgd_step refuses (nseg, NULL arrays, a NULL weight);
 *   3. APA_ERR_INVALID_ARG: a NULL or misaligned ce->index, ml without ce->video_targets / ce->targets, no ml without
 *      ce->video_labels / ce->labels; what apa_sample_clip_frames_keyed refuses for (V, B, F, K, mode); an unknown
 *      ml->kind;
 *   4. everything apa_attn_head_train_step_cached_clips refuses for the shape, both halves' checks run once --
 *      per-class maps (M != 1) among them, by name, although the step serves them: this call's update rewrites no
 *      weight images. */
int apa_attn_head_train_epoch_cached_clips(const apa_epoch* ep, const apa_epoch_sgd* opt, const apa_clip_epoch* ce,
                                           const apa_feature_cache* cache, const apa_multilabel* ml /* NULL: softmax */,
                                           const apa_clip_pool* clip /* NULL: one-frame videos */,
                                           const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                                           const float* ba, const float* Wt, const float* bt, const int64_t* labels,
                                           float loss_wt, float grad_scale, float* logits, float* att, float* zsave,
                                           float* abar, float* loss, float* G, void* dX, void* dXatt, float* dWa,
                                           float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P,
                                           int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                                           uint64_t offset, int dtype, void* stream);

/* apa_attn_head_eval_epoch_cached_clips(ep, ce, cache, clip, scores_kind, <the arguments of
 * apa_attn_head_eval_step_cached_clips from X on>) IS the loop of steps = ceil(ep->count / B) passes, the reference's
 * test protocol (uniform frames):
 *   for s in 0 .. steps-1, with b = the step's videos (B, the last step: count - (steps-1)*B) and row = s*B:
 *     apa_sample_clip_frames_keyed(videos = ep->order + row, ce->index, ce->labels + row, ce->targets + row*K, ..., b,
 *                                  F, K, APA_CLIP_FRAMES_UNIFORM, ce->seed, ce->epoch, step = s)
 *     apa_attn_head_eval_step_cached_clips(cache{index = ce->index}, clip{pooled + row*K}, scores_kind, ...,
 *                                          labels = loss ? ce->labels + row : NULL, loss + s*(1+B), probs + row*K,
 *                                          pred + row, N = b*F)
 * Per-VIDEO outputs advance by s*B rows: clip->pooled and probs [count,K], pred [count]; the sampled labels [count]
 * (where ce->video_labels and ce->labels are given) and targets [count,K] (ce->video_targets and ce->targets) are
 * written row-aligned beside them, so that an evaluation meter is filled with no host step.  loss (APA_SCORES_SOFTMAX
 * only; needs the sampled labels) is logged [steps][1+B].  Frame-level outputs -- logits [N,K], att, zsave, abar,
 * clip->tatt -- are the last step's.  The last step runs the remaining videos as a smaller batch in the same workspace,
 * its shape checked before the first launch too; nothing is written past row count.  clip == NULL: one-frame videos
 * without pooling -- the step is apa_attn_head_eval_step_cached, its logits rows ARE the per-video rows: logits is then
 * [count,K] and advances with the others, and no pooled is written.  The `labels` argument of the flat list is not read.
 * Refused before the first launch, in this order: a NULL ep / order, cache or ce; N < 1 or N % clip->frames != 0;
 * count < 1; steps * B past 2^31 - 1; a NULL or misaligned ce->index, loss without ce->video_labels / ce->labels; what
 * apa_sample_clip_frames_keyed refuses; then everything apa_attn_head_eval_step_cached_clips refuses for the full and
 * for the last batch (M != 1 by name, as in the training call). */
int apa_attn_head_eval_epoch_cached_clips(const apa_epoch* ep, const apa_clip_epoch* ce, const apa_feature_cache* cache,
                                          const apa_clip_pool* clip /* NULL: one-frame videos, no pooling */, int scores_kind, const void* X,
                                          const void* Xatt, const float* Wa, const float* ba, const float* Wt, const float* bt,
                                          const int64_t* labels, float* logits, float* att, float* zsave, float* abar,
                                          float* loss, float* probs, int64_t* pred, void* ws, size_t ws_bytes, int N,
                                          int P, int C, int Ca, int K, int M, unsigned flags, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* APA_CLIP_EPOCH_H_ */
