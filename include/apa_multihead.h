/* apa_multihead.h -- H independent class-agnostic heads (cfg 002: M == 1, Xatt == X) trained and evaluated from ONE pass
 * over a resident feature cache per direction.
 *
 * A frozen-feature run trains the small head many times on the same cached conv5 maps: learning-rate and weight-decay
 * sweeps, several initialisations, seed ensembles whose scores are averaged at test time ("late fusion").  Each of
 * those runs streams the same N x P x C rows out of HBM, forward and backward.  Here a pixel's row is read once per
 * direction and serves H heads, each with its own weights, logits, loss, gradients and optimiser state.  The companion
 * of apa.h's *_cached entry points; exported by the same library; apa.h itself, its entry points and APA_VERSION are
 * unchanged, and every refusal of apa.h's entry points stays what it was.
 *
 * Semantics, per head h = 0 .. H-1 (1 <= H <= APA_HEADS_MAX), those of apa_attn_head_train_step_cached under
 * APA_FLAG_FROZEN_INPUT on head h's weights (the M = 1 factorisation):
 *   Z_h = X . Wa_h + ba_h          A_h = f(Z_h), f = id | relu (APA_FLAG_RELU_ATT: ONE flag word for all heads)
 *   Xt = X * mask / keep_prob      (APA_FLAG_TRAIN; else X)
 *   z_h[n,:] = (1/P) sum_p A_h[n,p] Xt[n,p,:]         abar_h[n] = (1/P) sum_p A_h[n,p]
 *   logits_h = z_h . Wt_h + abar_h (x) bt_h
 *   loss_h, G_h: apa_softmax_xent_fwd_bwd of logits_h     (loss [1+N] per head, G = loss_wt * grad_scale / N (p - 1hot))
 *   dz_h = G_h . Wt_h^T      dWt_h = z_h^T . G_h      dbt_h = abar_h^T . G_h
 *   dA_h[n,p] = (Xt[n,p,:] . dz_h[n,:] + G_h[n,:] . bt_h) / P       dZ_h = dA_h [* (A_h > 0)]
 *   dWa_h = X^T dZ_h        dba_h = sum dZ_h                          (no dX: the features are frozen)
 * Parameters are stacked contiguously, fp32: Wa [H,C], ba [H], Wt [H,C,K], bt [H,K]; so are the outputs: logits
 * [H,N,K], att [H,N,P], zsave [H,N,C], abar [H,N], loss [H,1+N], G [H,N,K], dWa [H,C], dba [H], dWt [H,C,K], dbt [H,K].
 *
 * All heads see the same batch through apa_feature_cache (X addresses the WHOLE cache [T,P,C], fp32 or bf16; image n is
 * cache image index[n]; an id outside [0, T) is clamped and, with `status`, counted ONCE per call, not once per head;
 * labels_cached as in apa.h), the same labels, and THE SAME DROPOUT MASK: one (seed, offset, keep_prob), the stream
 * apa_dropout_mask gives over the flat [N,P,C] batch index, so X * mask / keep is formed once per element.  Heads that
 * need different keep probabilities or mask streams are out of scope: run them as separate calls.
 *
 * FP8 caches (APA_DTYPE_FP8_E4M3) are refused by name: the FP8 arm hashes per pair of elements and would need a
 * streaming pass of its own.  Also not built: APA_FLAG_RNG_DEVICE (the epoch call advances the offset on the host),
 * clips, the sigmoid training losses, a separate attention input, per-class maps.
 *
 * Conventions: those of apa.h.  Every function returns APA_OK or an APA_ERR_* code and leaves its reason in
 * apa_last_error(); every launch goes to `stream`, nothing allocates, nothing synchronises; the index is read on the
 * device and no address depends on its contents, so every call can be captured in a hipGraph; there are no
 * floating-point atomics -- identical calls give identical bits.  The head is a grid dimension of every kernel: a step
 * has the same number of launches for H = 1 and H = 4 (training 9, evaluation 4 or, with labels and loss, 5).
 *
 * Refused before anything is queued, in this order, the argument named in apa_last_error:
 *   1. APA_ERR_INVALID_ARG   a NULL cache / heads / cache->index (epochs: ep / ep->order / opt / opt->lr), then any
 *                            other NULL required pointer;
 *   2. APA_ERR_INVALID_ARG   heads->H < 1 or > APA_HEADS_MAX ("H");
 *   3. APA_ERR_INVALID_ARG   N, P, C, K or cache_images < 1 (epochs: the count rules of apa.h's epoch calls);
 *      APA_ERR_INVALID_ARG   evaluation: a scores_kind that is neither APA_SCORES_SOFTMAX nor APA_SCORES_SIGMOID
 *                            ("scores_kind"); the sigmoid scores with labels / loss ("sigmoid");
 *      APA_ERR_UNSUPPORTED   a C the rank kernels' instances do not serve (whole 16-byte vectors, C <= 2048) ("C");
 *      APA_ERR_UNSUPPORTED   N * P >= 2^31 pixels, or (S + 1) * P past 31 bits for the plan's S splits ("pixels");
 *   4. APA_ERR_INVALID_ARG   training without APA_FLAG_FROZEN_INPUT ("APA_FLAG_FROZEN_INPUT");
 *   5. APA_ERR_UNSUPPORTED   APA_FLAG_SOFTMAX_ATT, APA_FLAG_RELU_INPUT, APA_FLAG_RNG_EXTERNAL, APA_FLAG_RNG_DEVICE,
 *                            each by its name;
 *   6. APA_ERR_UNSUPPORTED   dtype APA_DTYPE_FP8_E4M3 ("FP8"); APA_ERR_INVALID_ARG any other unknown dtype;
 *      APA_ERR_INVALID_ARG   training with APA_FLAG_TRAIN and a keep_prob outside (0, 1] ("keep_prob");
 *   7. APA_ERR_WORKSPACE     ws_bytes < apa_multihead_workspace_bytes(H, N, P, C, K) ("ws_bytes");
 *   8. APA_ERR_UNSUPPORTED   X, ws or zsave not 16-byte aligned, index (order) not 4-byte aligned ("aligned").
 */
#ifndef APA_MULTIHEAD_H_
#define APA_MULTIHEAD_H_

#include "apa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of accumulator sets the streaming kernels hold in registers at C = 2048 with two blocks per CU. */
#define APA_HEADS_MAX 4

typedef struct apa_multihead {
  int H;             /* 1 .. APA_HEADS_MAX */
  const float* Wa;   /* [H,C]   */
  const float* ba;   /* [H]     */
  const float* Wt;   /* [H,C,K] */
  const float* bt;   /* [H,K]   */
} apa_multihead;

/* Bytes of workspace both steps need (0 for arguments refused by rules 2 and 3).  The plan, regions in this order,
 * each rounded up to 256 bytes, S = the pixel splits of an image (apa.h's M == 1 plan: S = (512 + N/2) / N, at least
 * 1, at most P/4 for P >= 8 else 1, at most 256), nblk = N * S:
 *   pacc f32 [nblk][H][C] | pstat f32 [nblk][4] | pgrad f32 [nblk][H*C + 4] | dz f32 [H][N][C] | labels i64 [N] |
 *   sn f32 [H][N] */
size_t apa_multihead_workspace_bytes(int H, int N, int P, int C, int K);

/* One training step of all heads.  labels int64 [N] ([T] with cache->labels_cached).  hooks (nullable): prof_fwd_* /
 * prof_bwd_* bracket the two streaming passes. */
int apa_multihead_train_step_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const apa_multihead* heads,
                                    const void* X, const int64_t* labels, float loss_wt, float grad_scale,
                                    float* logits, float* att, float* zsave, float* abar, float* loss, float* G,
                                    float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N,
                                    int P, int C, int K, unsigned flags, float keep_prob, uint64_t seed,
                                    uint64_t offset, int dtype, void* stream);

/* One evaluation step of all heads: the forward pass without dropout (APA_FLAG_TRAIN is cleared), then the scores:
 * probs [H,N,K] (scores_kind APA_SCORES_SOFTMAX or APA_SCORES_SIGMOID) and pred int64 [H,N], the first maximal index.
 * fused_probs f32 [N,K] (nullable): the late-fusion scores, ((p_0 + p_1) + p_2 ...) / H in head order; fused_pred
 * int64 [N] (nullable, needs fused_probs): their first maximal index.  labels / loss [H,1+N] may both be NULL; with
 * the sigmoid scores they must be. */
int apa_multihead_eval_step_cached(const apa_feature_cache* cache, const apa_multihead* heads, int scores_kind,
                                   const void* X, const int64_t* labels, float* logits, float* att, float* zsave,
                                   float* abar, float* loss, float* probs, int64_t* pred, float* fused_probs,
                                   int64_t* fused_pred, void* ws, size_t ws_bytes, int N, int P, int C, int K,
                                   unsigned flags, int dtype, void* stream);

/* apa_momentum_sgd_step for H heads in ONE launch.  Segment i is a stacked tensor [H][sizes[i]] at weights[i] (HOST
 * array of nseg device pointers, sizes HOST [nseg]); grad_flat / acc_flat hold the stacked segments back to back,
 * [H][sizes[0]] | [H][sizes[1]] | ... -- the layout of dWa | dba | dWt | dbt above when they share one allocation.
 * weight_decay HOST [nseg][H], lr HOST [H], momentum HOST [H], all read during the call.  Elementwise, the arithmetic of
 * apa_momentum_sgd_step: bit-identical to H calls of it on the heads' rows.  nseg <= APA_SGD_MAX_SEGMENTS. */
int apa_momentum_sgd_step_heads(int H, int nseg, float* const* weights, const size_t* sizes, const float* weight_decay,
                                const float* grad_flat, float* acc_flat, const float* lr, const float* momentum,
                                float grad_scale, void* stream);

typedef struct apa_multihead_sgd {   /* the update behind every step of an epoch: apa_momentum_sgd_step_heads' arguments */
  int nseg; float* const* weights; const size_t* sizes; const float* weight_decay;
  const float* grad_flat; float* acc_flat;
  const float* lr;                  /* HOST, [steps][H]: the learning rates of update s */
  const float* momentum;            /* HOST, [H] */
  float grad_scale;
} apa_multihead_sgd;

/* apa_multihead_train_epoch_cached IS, bit for bit, this loop of steps = ep->count / N passes:
 *   apa_multihead_train_step_cached with cache.index = ep->order + s*N, dropout offset + s, loss + s*H*(1+N)
 *   apa_momentum_sgd_step_heads(H, opt->nseg .. opt->acc_flat, opt->lr + s*H, opt->momentum, opt->grad_scale, stream)
 * loss is the epoch's log [steps][H][1+N]; the other outputs hold the last step's values.  cache->index is ignored;
 * with labels_cached = 0 labels is [count] in visiting order.  ep and the order rule are apa.h's. */
int apa_multihead_train_epoch_cached(const apa_epoch* ep, const apa_multihead_sgd* opt, const apa_feature_cache* cache,
                                     const apa_hooks* hooks, const apa_multihead* heads, const void* X,
                                     const int64_t* labels, float loss_wt, float grad_scale, float* logits, float* att,
                                     float* zsave, float* abar, float* loss, float* G, float* dWa, float* dba,
                                     float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int K,
                                     unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                                     void* stream);

/* apa_multihead_eval_epoch_cached IS the loop of steps = ceil(ep->count / N) evaluation steps on order + s*N, the last
 * one on the remaining rows as a smaller batch in the same workspace (as apa_attn_head_eval_epoch_cached): logits and
 * probs are [H,count,K], pred [H,count], fused_probs [count,K], fused_pred [count], labels [count] unless
 * labels_cached, loss, where asked for, the log [steps][H][1+N] (the slot of a smaller last batch of n rows holds
 * [H][1+n] at its start); att, zsave and abar are the last step's, stacked for ITS batch size.  Nothing is written past
 * row count.  Workspace: the larger of apa_multihead_workspace_bytes for N and for the last batch's size (the pixel
 * splits of the plan grow as the batch shrinks). */
int apa_multihead_eval_epoch_cached(const apa_epoch* ep, const apa_feature_cache* cache, const apa_multihead* heads,
                                    int scores_kind, const void* X, const int64_t* labels, float* logits, float* att,
                                    float* zsave, float* abar, float* loss, float* probs, int64_t* pred,
                                    float* fused_probs, int64_t* fused_pred, void* ws, size_t ws_bytes, int N, int P,
                                    int C, int K, unsigned flags, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* APA_MULTIHEAD_H_ */
