/* apa_pose_cache.h -- the pose-regularised head (cfg 003, 003_MPII_ResNet_withPoseAttention.yaml) trained and
 * evaluated from a resident feature cache read by image index.
 *
 * The companion of apa.h's *_cached entry points (apa_feature_cache: the class-agnostic head with attention from the
 * map itself, and per-class maps on the fused route) for the head they leave out: PoseLogits 2048 -> 768 -> 16 with
 * bottom-up attention from pose_pre_logits, the pose L2 loss and the cross-entropy.  Exported by the same library;
 * apa.h itself, its entry points and APA_VERSION are unchanged, and every *_cached entry point of apa.h answers what it
 * answered ("a separate attention input (Xatt != X)" stays refused there).
 *
 * Conventions: those of apa.h.  Every function returns APA_OK or an APA_ERR_* code and leaves its reason in
 * apa_last_error(); every launch goes to `stream`, nothing allocates, nothing synchronises; the index is read on the
 * device and no address depends on its contents, so both calls can be captured in a hipGraph and replayed with the
 * index rewritten in place; there are no floating-point atomics -- identical calls give identical bits.
 *
 * The contract is the one of apa.h's cached calls: a cached step IS the plain step (apa_pose_attn_train_step under
 * APA_FLAG_FROZEN_INPUT, apa_pose_attn_eval_step) on a gathered copy X[index] of the same images, bit for bit in every
 * output and with the same launches -- whichever route the plain call takes on that copy (training: fast or composed;
 * evaluation: fused or composed).  io->X addresses the WHOLE cache, T = cache->cache_images maps [T,P,C] in bf16, and
 * image n of the batch is cache image index[n].  Everything else in io has the BATCH shape -- pose_labels [N,P,J] and
 * pose_valid [N,J] included: pose labels are not read through the index (0.4 MB per step against 25.7 MB of features;
 * a caller gathers them with two index_select launches, custom_ops/pose_cache.py: PoseLabelTable) -- and so have both
 * workspaces, whose sizes and carve offsets are the plain calls'.  Three kernel families read X and follow the index:
 *   the product Ppre = relu(X . W1 + b1)     the MAP instances of the bf16 GEMM kernels, row map on the M rows
 *   both M == 1 pooling passes               their (FUSED = false, GATHER) instances: only the image's base address moves
 *   the product dW1 = X^T . dPpre            MAP instances again, row map on the contraction rows
 * att, dZ, the keep bits (keyed by batch position), zsave, the partials and every epilogue keep the batch position.
 * An index entry outside [0, T) is clamped into the cache -- nothing outside it is ever addressed -- and, with
 * cache->status given, counted there ONCE per step, by the forward pooling pass (the products clamp silently).
 * cache->labels_cached = 1: io->labels is [T] and image n's label is labels[index[n]], read by the forward pooling pass
 * into the pooling workspace where apa_attn_head_train_step_cached keeps its [N] copy; with 0, io->labels is [N].
 *
 * Refused before anything is queued, in this order, each with its own sentence:
 *   APA_ERR_INVALID_ARG   a NULL io, a NULL descriptor or index (or one that is not 4-byte aligned), cache_images < 1,
 *                         a non-NULL io->dX, training without APA_FLAG_FROZEN_INPUT;
 *   APA_ERR_UNSUPPORTED   dtype != APA_DTYPE_BF16;
 *   APA_ERR_UNSUPPORTED   a cache base that is not 16-byte aligned, or C % 8 != 0;
 *   APA_ERR_UNSUPPORTED   a product the MAP instances do not serve (what the dispatcher would send to the
 *                         fp32-unpacking kernels);
 *   APA_ERR_UNSUPPORTED   APA_FLAG_SOFTMAX_ATT: the forward pass would pool a map that is already final, but the backward
 *                         pooling pass forms dZ under the softmax and has no gathered instance of that arm; evaluation
 *                         refuses it with training;
 * then whatever the plain call refuses.
 *
 * Out of scope: cfg 003 on clips or under the sigmoid losses from a cache; the epoch calls for cfg 003; fp32 and FP8
 * caches for this head; pose labels through the index inside a kernel; the concatenated pose channels
 * (_WITH_POSE_FEAT); rank > 1.
 */
#ifndef APA_POSE_CACHE_H_
#define APA_POSE_CACHE_H_

#include "apa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* apa_pose_attn_train_step on the images cache[index]; flags must carry APA_FLAG_FROZEN_INPUT, io->dX must be NULL. */
int apa_pose_attn_train_step_cached(const apa_feature_cache* cache, const apa_pose_attn_step_io* io, int N, int P,
                                    int C, int Cp, int J, int K, unsigned flags, float keep_prob, uint64_t seed,
                                    uint64_t offset, int dtype, void* stream);

/* apa_pose_attn_eval_step on the images cache[index]; io->route reports the route as there. */
int apa_pose_attn_eval_step_cached(const apa_feature_cache* cache, const apa_pose_attn_eval_io* io, int N, int P, int C,
                                   int Cp, int J, int K, unsigned flags, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* APA_POSE_CACHE_H_ */
