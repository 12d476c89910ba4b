/*
 * apa.h -- C ABI of libapa_hip.so, the MI355X (gfx950) attentional-pooling library.
 *
 * This is the drop-in boundary for the attentional-pooling hot path of
 * rohitgirdhar/AttentionalPoolingAction.  The reference has no native implementation of the
 * head (it is ~10 TF-slim graph ops, models/slim/nets/nets_factory.py:242-328); its only native
 * plugin mechanism is the set of TF custom ops in src/custom_ops/ (REGISTER_OP + OpKernel::Compute,
 * loaded by src/custom_ops/custom_ops_factory.py:11-18 via tf.load_op_library).  Each entry point
 * below names the reference code it replaces.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 (APA_OK) or a negative apa_status.
 *     Nothing throws across the boundary (the reference signals errors with OP_REQUIRES_OK /
 *     assert, src/custom_ops/pose_to_heatmap.cc:27-32,49).
 *   - all tensor pointers are DEVICE pointers (HBM) unless the name ends in _host.
 *   - the caller owns every buffer, including workspaces; the library is stateless and
 *     re-entrant (the reference ops run concurrently on TF inter-op threads,
 *     src/custom_ops/pose_utils.hpp:7-14).
 *   - every launch goes to the hipStream_t passed as `void* stream`; no implicit
 *     synchronisation, no allocation -> all entry points are hipGraph-capturable
 *     (tests/test_graph_replay_gpu.py replays each of them), with two exceptions that are meant for bind time
 *     and for measurement: apa_clip_by_norm_prepare (marshals a host table and waits for its own copies) and
 *     apa_prof_event_record (records a HIP event).  A capture freezes what travels by value: a dropout offset
 *     without APA_FLAG_RNG_DEVICE, the lr array of apa_epoch_sgd, the (seed, epoch) of apa_epoch_order and the
 *     members of the descriptor structs; what a replay re-reads is what lies in HBM behind the pointers.
 *   - layouts are the reference's: feature maps NHWC flattened to [N, P=H*W, C]; 1x1-conv
 *     weights [Cin, Cout] (TF HWIO [1,1,Cin,Cout] squeezed); float32 unless stated.
 *
 * Symbols: N batch, P = H*W pixels, C feature channels (2048), Ca channels of the attention
 * input (C for cfg 002, 768 for cfg 003), K classes, M bottom-up maps (1, or K for per-class),
 * J pose keypoints (16), Cp pose pre-logit channels (768).
 */
#ifndef APA_H_
#define APA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APA_VERSION 314 /* major*10000 + minor*100 + patch */

typedef enum apa_status {
  APA_OK = 0,
  APA_ERR_INVALID_ARG = -1,   /* null pointer, non-positive dimension, bad enum           */
  APA_ERR_UNSUPPORTED = -2,   /* shape/dtype combination the kernels are not built for    */
  APA_ERR_WORKSPACE = -3,     /* ws_bytes smaller than apa_*_workspace_bytes()            */
  APA_ERR_HIP = -4            /* a HIP runtime call / launch failed (see apa_last_error)  */
} apa_status;

/* dtype of the feature-map tensors (X, Xatt, dX, dXatt, TopDown); parameters are always f32 */
#define APA_DTYPE_F32 0
#define APA_DTYPE_BF16 1
/* A CACHED feature map in OCP FP8 E4M3 with one fp32 scale per image (see "FP8 feature cache" below).  Served by the
 * class-agnostic head on frozen features only: apa_attn_pool_fwd[_ex], apa_attn_pool_bwd[_ex], apa_attn_head_train_step*
 * and apa_attn_head_eval_step*; every other entry point answers "unknown dtype". */
#define APA_DTYPE_FP8_E4M3 2

/* flags (mirror cfg.NET.USE_POSE_PRELOGITS_BASED_ATTENTION_*, src/config.py:194-203)      */
#define APA_FLAG_SOFTMAX_ATT 1u /* _SOFTMAX_ATT: spatial softmax of the bottom-up map       */
#define APA_FLAG_RELU_ATT 2u    /* _RELU_ATT                                                 */
#define APA_FLAG_TRAIN 4u       /* is_training: dropout on the top-down input is active      */
#define APA_FLAG_RNG_DEVICE 8u  /* `offset` is the ADDRESS of a uint64 step counter in HBM: the   */
                                /* kernels read it at run time and apa_attn_pool_bwd adds 1 to it */
                                /* when it is done, so a captured hipGraph draws a fresh dropout  */
                                /* mask on every replay                                           */
#define APA_FLAG_RELU_INPUT 16u /* X in memory is the backbone's PRE-activation (block4's residual */
                                /* sum, resnet_v1.py:108-109): the op applies X = max(X, 0) on the  */
                                /* fly in both passes and returns dX already multiplied by [X > 0], */
                                /* so the ReLU's own read+write of the map and its backward pass    */
                                /* (2 + 3 streams of P*C*s bytes) disappear.    */
                                /* M == 1, Xatt == X, C in {1024,2048,4096} (f32) / 2048 (bf16)     */
#define APA_FLAG_DXATT_RANK1 32u /* apa_attn_pool_bwd, M == 1 with a separate attention input (cfg   */
                                /* 003): the gradient w.r.t. Xatt is rank-1, dXatt = dZ (x) Wa; with  */
                                /* this flag `dXatt` is an fp32 [N*P] buffer that receives dZ and the  */
                                /* [N,P,Ca] tensor is never written (its consumer,                     */
                                /* apa_pose_head_bwd_rank1ext, re-forms it in registers)              */

#define APA_FLAG_WS_FROM_FWD 64u /* RESERVED for the library: apa_attn_head_train_step sets it on its own     */
                                /* backward half (same workspace, nothing in between: operands the forward */
                                /* pass prepared there are reused).  The public apa_attn_pool_bwd* entry    */
                                /* points clear it -- a caller cannot vouch for a workspace's history.      */
#define APA_FLAG_RNG_EXTERNAL 128u /* replay a dropout mask drawn ELSEWHERE (the reference's tf.nn.dropout:   */
                                /* binary = floor(keep_prob + uniform), nets_factory.py:143-146,296): `seed` */
                                /* is the ADDRESS of the keep decisions in HBM, bit-packed -- bit (e & 7) of */
                                /* byte e >> 3 belongs to flat element e of the [N,P,C] map (the *_cat entry */
                                /* points: elements N*P*C .. continue into the [N,P,J] extra channels), the   */
                                /* image is ceil(n/8) bytes rounded up to a multiple of 8; `offset` is        */
                                /* ignored; kept elements are scaled by 1/keep_prob.  Pass the same image to  */
                                /* the backward call.  Excludes APA_FLAG_RNG_DEVICE / APA_FLAG_RELU_INPUT.    */
                                /* A replayed mask is read by the library's run-time-loop kernels (any C that */
                                /* is a whole number of 16-byte vectors; per-class maps take the GEMM route), */
                                /* not by the hash-fused streaming kernels: a parity facility, not a fast path */

#define APA_FLAG_WEIGHT_IMAGES 256u /* per-class maps (M == K): the caller vouches that the padded / concatenated   */
                                /* operand images of Wa, ba, Wt, bt in `ws` are CURRENT -- built there by          */
                                /* apa_per_class_weight_images() and rewritten after every weight change (by that  */
                                /* function again, or by the optimiser's own launch, apa_momentum_sgd_step_images) */
                                /* with nothing else using the workspace in between.  The per-step preparation     */
                                /* launch then produces only what changes per step (the dropout decisions), or     */
                                /* does not run at all (evaluation).  Needs 16-byte aligned features (else         */
                                /* APA_ERR_INVALID_ARG); ignored for M == 1.  A stale image is the caller's bug,   */
                                /* like a stale apa_pose_attn_step_io.W1_bf16.                                    */

#define APA_FLAG_FROZEN_INPUT 512u /* the features are FROZEN (conv5 precomputed, or nothing upstream of it trains --  */
                                /* TRAIN.TRAINABLE_SCOPES without a backbone scope): the backward half writes NO     */
                                /* gradient for X.  The `dX` argument is ignored and may be NULL; every other output */
                                /* is, bit for bit, what the same call produces without the flag.  Accepted by       */
                                /* apa_attn_pool_bwd[_ex] and every apa_*_train_step* entry point (apa_pose_head_bwd  */
                                /* has no flags word: APA_POSE_NO_DX).  Served for M == 1 by every kernel family and  */
                                /* for per-class maps on the fused K <= 64 route; the dense per-class route, the      */
                                /* *_cat entry points and a forward call that also asks for the TopDownAttention dump */
                                /* refuse it with APA_ERR_UNSUPPORTED before anything is queued (run without it).     */
                                /* A forward call otherwise ignores it.                                               */

int apa_version(void);
/* Thread-local, never NULL; describes the last failure on the calling thread. */
const char* apa_last_error(void);
const char* apa_status_string(int status);

/* ------------------------------------------------------------------------------------------
 * Attentional pooling, forward.   Replaces nets_factory.py:247-328 + the squeeze at :350-351.
 *
 *   Z = Xatt . Wa + ba                      [N,P,M]     'Conv2d_PrePose_Attn'   (:259-270)
 *   A = f(Z), f = id | softmax over P | relu                                     (:276-287)
 *   Xt = X * mask / keep_prob  (APA_FLAG_TRAIN) else X             slim.dropout  (:296)
 *   T = Xt . Wt + bt                        [N,P,K]     'Conv'                  (:298-309)
 *   logits[n,k] = (1/P) sum_p A[n,p,m(k)] * T[n,p,k],  m(k) = 0 if M==1 else k   (:322-325)
 *
 * X     [N,P,C]   dtype            Xatt  [N,P,Ca]  dtype; pass Xatt == X (Ca == C) for cfg 002
 * Wa    [Ca,M] f32, ba [M] f32     Wt    [C,K] f32, bt [K] f32
 * logits[N,K] f32 (out)            att   [N,P,M] f32 (out) = end_points['PosePrelogitsBasedAttention']
 * zsave (out, saved for backward)  M==1: [N,C] f32 = (1/P) sum_p A[n,p] Xt[n,p,:]
 *                                  M==K: [N,P,K] f32 = the top-down map T
 * abar  [N]   f32 (out, M==1 only) = (1/P) sum_p A[n,p]             -- saved for backward
 * topdown [N,P,K] dtype or NULL    = end_points['TopDownAttention']; only materialised on request
 *                                    (the reference needs it for eval.py --ept dumps only)
 * ws / ws_bytes: scratch of at least apa_attn_pool_workspace_bytes(...) bytes.
 * seed/offset: counter-based dropout RNG key (APA_FLAG_TRAIN); the same pair must be passed to
 *              the backward call.  apa_dropout_mask() materialises the identical mask.  With
 *              APA_FLAG_RNG_EXTERNAL the mask is the caller's own (see the flag).
 * M == 1 runs the factorised HBM-bound path (T is never formed); M == K the dense MFMA path.
 */
size_t apa_attn_pool_workspace_bytes(int N, int P, int C, int Ca, int K, int M, unsigned flags);

int apa_attn_pool_fwd(const void* X, const void* Xatt, const float* Wa, const float* ba,
                      const float* Wt, const float* bt, float* logits, float* att, float* zsave,
                      float* abar, void* topdown, void* ws, size_t ws_bytes, int N, int P, int C,
                      int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                      uint64_t offset, int dtype, void* stream);

/* Attentional pooling, backward (the reference has none: TF autodiff of the ops above,
 * model_deploy.py:263).  G = dLoss/dlogits [N,K] f32.  Outputs (all written, not accumulated):
 *   dX [N,P,C] dtype; dXatt [N,P,Ca] dtype or NULL when Xatt == X (its term is folded into dX);
 *   dWa [Ca,M], dba [M], dWt [C,K], dbt [K]  f32.
 * att/zsave/abar are the tensors the forward call produced.
 * APA_FLAG_FROZEN_INPUT: dX is not written (NULL allowed); M == 1: the streaming pass becomes read-only like the
 * forward one (cfg 002 fp32, 32 x 14x14x2048: 51.4 MB of the call's 102.8 MB go, 17.5 -> 12.0 us); per-class maps
 * K <= 64: the dX kernel keeps its row work ([dT | dZ], the dbt | dba partials) and loses the product and the stores.
 */
int apa_attn_pool_bwd(const void* X, const void* Xatt, const float* Wa, const float* ba,
                      const float* Wt, const float* bt, const float* att, const float* zsave,
                      const float* abar, const float* G, void* dX, void* dXatt, float* dWa,
                      float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P,
                      int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                      uint64_t offset, int dtype, void* stream);

/* Writes the {0,1} keep-mask that APA_FLAG_TRAIN applies to X (uint8 [N*P*C]); used by the
 * parity tests to hand the oracle the exact mask (TF's own RNG stream is not reproducible). */
int apa_dropout_mask(uint8_t* mask, size_t n_elems, float keep_prob, uint64_t seed, uint64_t offset,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * FP8 feature cache (APA_DTYPE_FP8_E4M3).  A conv5 map that is computed once and read for a whole training run is
 * kept as OCP E4M3 codes (torch.float8_e4m3fn: code 56 = 1.0, 126 = 448, 0x7F / 0xFF = NaN) with one scale per image.
 * The feature pointer X of such a call addresses ONE allocation of apa_fp8_features_bytes(N, P, C) bytes:
 *   N*P*C bytes of codes in [N,P,C] order, 16-byte aligned, then -- at the next 256-byte boundary -- N fp32 scales;
 *   element value = scale[n] * decode(code).
 * Quantisation (fp32 arithmetic, IEEE division, so a CPU restatement is bit-exact):
 *   amax_n = max |x| over image n;  scale_n = amax_n / 448;  inv_n = 448 / amax_n  (both 0 when amax_n == 0);
 *   code = rne_e4m3(x * inv_n).
 * status int32 [N]: 0 = ok, 1 = image n holds a non-finite value (its codes and scale are then zero).
 * src_dtype / dst_dtype: APA_DTYPE_F32 or APA_DTYPE_BF16; src / dst 16-byte aligned, C a multiple of 16.
 * The pooling calls take such an X with Xatt == X, M == 1, C a multiple of 16 up to 8192, identity or ReLU attention;
 * APA_FLAG_SOFTMAX_ATT, APA_FLAG_RELU_INPUT, APA_FLAG_RNG_EXTERNAL, a separate attention input, per-class maps and the
 * TopDownAttention dump are refused with APA_ERR_UNSUPPORTED.  A cache has no gradient: a backward call or a training
 * step without APA_FLAG_FROZEN_INPUT, or with a non-NULL dX, is refused with APA_ERR_INVALID_ARG.  The workspace is
 * apa_attn_pool_workspace_bytes; the dropout mask is apa_dropout_mask's over the flat [N,P,C] index.
 */
size_t apa_fp8_features_bytes(int N, int P, int C);
int apa_quantize_features_fp8(const void* src, int src_dtype, void* dst, int32_t* status, int N, int P, int C,
                              void* stream);
int apa_dequantize_features_fp8(const void* src, void* dst, int dst_dtype, int N, int P, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * PoseLogits head.  Replaces nets_factory.py:147-160:
 *   Ppre = relu(X . W1 + b1)   [N,P,Cp]  dtype    'PoseLogits/ExtraConv2d_1x1'  (Cp = 768)
 *   Pl   = Ppre . W2 + b2      [N,P,J]   f32      'PoseLogits/Conv2d_1c_1x1'    (J = 16)
 * W1 [C,Cp], b1 [Cp], W2 [Cp,J], b2 [J] f32.  Dense: bf16 features run on the bf16 MFMA with
 * fp32 accumulation, fp32 features on the exact f32 MFMA.
 * Backward (TF autodiff in the reference):  dPl [N,P,J] f32 = gradient of the pose loss (or NULL);
 * dPpre_ext [N,P,Cp] dtype = gradient arriving at Ppre from the attention branch of cfg 003 (the
 * dXatt of apa_attn_pool_bwd) or NULL.  Outputs dW1 [C,Cp], db1 [Cp], dW2 [Cp,J], db2 [J] f32 and
 * dX [N,P,C] dtype, overwritten or (accumulate_dX & 1) added to what the buffer already holds.
 * accumulate_dX & APA_POSE_WS_FROM_FWD: `ws` is the workspace of the matching apa_pose_head_fwd call and has
 * not been written since -- the bf16 copy of W1 the forward call left there is reused, not rebuilt.
 * accumulate_dX & APA_POSE_NO_DX: the features are frozen (as APA_FLAG_FROZEN_INPUT for the entry points that have a
 * flags word): the dX product dPpre . W1^T is not launched, `dX` is ignored and may be NULL; dW1, db1, dW2, db2 are
 * what the call produces without the bit, bit for bit.
 */
#define APA_POSE_WS_FROM_FWD 2
#define APA_POSE_NO_DX 4
size_t apa_pose_head_workspace_bytes(int N, int P, int C, int Cp, int J, int dtype);
int apa_pose_head_fwd(const void* X, const float* W1, const float* b1, const float* W2,
                      const float* b2, void* Ppre, float* Pl, void* ws, size_t ws_bytes, int N, int P,
                      int C, int Cp, int J, int dtype, void* stream);
int apa_pose_head_bwd(const void* X, const float* W1, const float* W2, const void* Ppre,
                      const float* dPl, const void* dPpre_ext, void* dX, int accumulate_dX, float* dW1,
                      float* db1, float* dW2, float* db2, void* ws, size_t ws_bytes, int N, int P, int C,
                      int Cp, int J, int dtype, void* stream);
/* Same, with the external gradient in rank-1 form: dPpre_ext[r,j] = ext_row[r] * ext_col[j]
 * (ext_row f32 [N*P] = the dZ that apa_attn_pool_bwd returns under APA_FLAG_DXATT_RANK1, ext_col f32
 * [Cp] = the attention weights Wa): one write and one read of an [N,P,Cp] tensor less per step. */
int apa_pose_head_bwd_rank1ext(const void* X, const float* W1, const float* W2, const void* Ppre,
                               const float* dPl, const float* ext_row, const float* ext_col, void* dX,
                               int accumulate_dX, float* dW1, float* db1, float* dW2, float* db2,
                               void* ws, size_t ws_bytes, int N, int P, int C, int Cp, int J, int dtype,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Pose-heatmap attention head, cfg.NET.USE_POSE_ATTENTION_LOGITS.  Replaces nets_factory.py:162-189 (after the
 * PoseLogits head of :147-160, apa_pose_head_fwd):
 *   A[n,p,m] = Pl[n,p,sel[m]]  (m < n_sel)              the selected parts, USE_POSE_ATTENTION_LOGITS_DIMS (:168-172)
 *            = mean_j Pl[n,p,j] (m == n_sel, avged)     ..._AVGED_HMAP, over all J parts      (:176-179)
 *            = 1                (m == M - 1)            the plain spatial mean                 (:180-181)
 *   F[n, m*C + c] = (1/P) sum_p A[n,p,m] X[n,p,c]        tf.concat(part_logits, axis=-1)       (:173-182)
 *   Fd = F * mask / keep_prob (APA_FLAG_TRAIN) else F    slim.dropout                          (:183)
 *   logits = Fd . W + b                                  'PoseAttention/Conv'                  (:184-188)
 * M = n_sel + avged + 1.  X [N,P,C] dtype; Pl [N,P,J] f32 = raw PoseLogits (no activation: negative weights are
 * fine); W [M*C, K] f32, b [K] f32; F [N, M*C] f32 (out: saved for backward); logits [N,K] f32 (out).
 * sel: HOST int32 [n_sel], already normalised to [0, J) (numpy indexing of the reference: negative indices wrapped,
 * repeats allowed; NULL when n_sel == 0); avged: 0 / 1.
 * flags: APA_FLAG_TRAIN, APA_FLAG_RNG_EXTERNAL (a bit image over the flat index of F).  The hashed mask is the one
 * apa_dropout_mask(N*M*C, keep_prob, seed, offset) returns: element n*(M*C) + m*C + c of F.
 * ws: apa_pose_att_logits_workspace_bytes(N, P, C, M, K) bytes; one buffer may serve both calls.
 * Built for M <= 32, C a multiple of 4, K <= 480 (else APA_ERR_UNSUPPORTED).  Alignment, refused with
 * APA_ERR_UNSUPPORTED before anything is launched: X -- and, in the backward call, dX, which is read and stored with
 * the same vector width -- 16-byte (f32) / 8-byte (bf16) aligned; ws 16-byte aligned in both calls (dF is read from it
 * four floats at a time).  Every other operand (Pl, W, b, F, G, logits, dPl, dW, db) needs its element's alignment only.
 * Every reduction is summed in a fixed order: identical calls give bit-identical results.
 *
 * Backward (TF autodiff in the reference).  G = dLoss/dlogits [N,K] f32.
 *   dW [M*C,K], db [K] f32                       overwritten
 *   dX [N,P,C] dtype                             overwritten, or (accumulate_dX) added to
 *   dPl [N,P,J] f32                              ACCUMULATED: dPl[n,p,j] += sum_{m: sel[m]=j} dA[n,p,m]
 *                                                + avged * dA[n,p,n_sel] / J, dA = (1/P) sum_c X dFd-scaled; the
 *                                                constant map's share is dropped.  Pass the pose-loss gradient
 *                                                (or zeros) and hand the sum to apa_pose_head_bwd.
 * F is the forward call's output; seed / offset / flags as in the forward call.
 * The _ex forms take apa_hooks: prof_fwd_start / stop bracket the pooling kernel(s) of the call, prof_bwd_start /
 * stop its classifier kernel(s) (per-kernel HIP-event times for tools/bench_dense.py).
 */
size_t apa_pose_att_logits_workspace_bytes(int N, int P, int C, int M, int K);
int apa_pose_att_logits_fwd(const void* X, const float* Pl, const int32_t* sel, int n_sel, int avged,
                            const float* W, const float* b, float* F, float* logits, void* ws, size_t ws_bytes,
                            int N, int P, int C, int J, int K, unsigned flags, float keep_prob, uint64_t seed,
                            uint64_t offset, int dtype, void* stream);
int apa_pose_att_logits_bwd(const void* X, const float* Pl, const int32_t* sel, int n_sel, int avged,
                            const float* W, const float* F, const float* G, void* dX, int accumulate_dX,
                            float* dPl, float* dW, float* db, void* ws, size_t ws_bytes, int N, int P, int C,
                            int J, int K, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                            int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Action loss: tf.losses.softmax_cross_entropy(one_hot(labels,K), logits, weights=wt)
 * (src/loss.py:74-80) fused with its gradient.
 *   loss[0] = wt/N * sum_n -log_softmax(logits[n])[labels[n]];  G = wt/N * (softmax - onehot)
 * `grad_scale` multiplies G only (1/num_clones of model_deploy.py:223-225 goes here).
 * labels int64 [N]; loss f32 [1+N]: loss[0] = weighted batch-mean loss, loss[1+n] = unweighted
 * per-example cross-entropy; G f32 [N,K] or NULL; probs f32 [N,K] or NULL (eval.py:196);
 * pred int64 [N] or NULL (argmax, first maximal index -- eval.py:193).
 */
int apa_softmax_xent_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* G,
                             float* probs, int64_t* pred, int N, int K, float wt, float grad_scale,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * One training step of the head as ONE host call: apa_attn_pool_fwd -> apa_softmax_xent_fwd_bwd ->
 * apa_attn_pool_bwd with the same arguments, on the same stream, launching the same kernels (the
 * three entry points above are called back to back; results are bit-identical to calling them
 * separately).  The reference runs this sequence inside one `sess.run(train_op)` (src/train.py:
 * 529-566) in TensorFlow's C++ executor, with no per-op interpreter cost; at ~55 us per step on
 * MI355X three separately marshalled foreign calls would make the HOST the bottleneck, so the
 * native sequence is part of the boundary.  All buffers are caller-owned (see the three functions
 * for shapes); loss f32 [1+N], G f32 [N,K].
 * Every output -- logits, loss and G included -- is valid only when the WHOLE call returns APA_OK: inside the
 * call launches are shared between the three ops (for the per-class maps with K <= 64 the cross-entropy is taken
 * by the first backward kernel, which is what writes logits / loss / G), so an error return from the second half
 * (e.g. APA_ERR_WORKSPACE) leaves them undefined.
 * APA_FLAG_FROZEN_INPUT (also the _ex, _clips and _multilabel forms): the backward half writes no dX (NULL allowed);
 * a route without that arm is refused before the forward half is queued.  Measured against the same step with dX,
 * alternating in one process, 32 x 14x14x2048: cfg 002 fp32 45.6 -> 40.1 us, HMDB-51 per-class bf16 50.6 -> 42.7 us.
 */
int apa_attn_head_train_step(const void* X, const void* Xatt, const float* Wa, const float* ba,
                             const float* Wt, const float* bt, const int64_t* labels, float loss_wt,
                             float grad_scale, float* logits, float* att, float* zsave, float* abar,
                             float* loss, float* G, void* dX, void* dXatt, float* dWa, float* dba,
                             float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C,
                             int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                             uint64_t offset, int dtype, void* stream);

/* One evaluation step of the head as ONE host call (eval.py:181-197: network_fn, then
 * tf.argmax(logits,1) and tf.nn.softmax(logits,-1) in the same sess.run): apa_attn_pool_fwd followed
 * by apa_softmax_xent_fwd_bwd without the gradient.  probs f32 [N,K]; pred int64 [N] (first maximal
 * index); labels / loss ([1+N], see above) may both be NULL when no ground truth is at hand.  */
int apa_attn_head_eval_step(const void* X, const void* Xatt, const float* Wa, const float* ba,
                            const float* Wt, const float* bt, const int64_t* labels, float* logits,
                            float* att, float* zsave, float* abar, float* loss, float* probs,
                            int64_t* pred, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                            int M, unsigned flags, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * One host call for the whole cfg 003 head step (003_MPII_ResNet_withPoseAttention.yaml): what the reference
 * runs as one sess.run of   PoseLogits head (nets_factory.py:147-160) -> attention from pose_pre_logits
 * (:247-270, M = 1) -> dropout + top-down conv + attention-weighted mean (:296-328) -> pose L2 +
 * softmax cross-entropy (src/loss.py:11-80) -> tf.gradients of both w.r.t. every head variable and conv5.
 * Same results as the sequence apa_pose_head_fwd, apa_pose_l2_loss_fwd_bwd, apa_attn_head_train_step
 * (APA_FLAG_DXATT_RANK1), apa_pose_head_bwd_rank1ext -- which is what it runs when the fused kernels do not
 * serve the shape -- but inside one call neighbouring ops share launches (bf16 features, J = 16,
 * Cp in {256,512,768,1024}, K <= 512): the Pl product also emits the attention logits and the pose loss
 * gradient; the pose head's backward rows pass also emits dWa / dba; its column-sum launch also finishes the
 * pose loss and advances the dropout counter: 18 -> 13 launches at the benchmark shape.
 * io->W1_bf16 (optional): a bf16 copy of W1 [C,Cp] the caller keeps current (apa_momentum_sgd_step_shadow
 * rewrites it in the optimizer's own launch); NULL = converted inside the call.
 * io->W2T_bf16 (optional, round 5): W2 TRANSPOSED and rounded to bf16, [16][Cp + 16] (rows J..15 and the 16 pad
 * columns zero), 16-byte aligned, kept current the same way (apa_momentum_sgd_step_images with the map "element
 * (c, j) of W2 -> dst[j * (Cp + 16) + c]": a = 1, d = Cp + 16, c_shift = b = e = 0): the Pl product copies this
 * 24.5 KB image verbatim into LDS (LDS-DMA) instead of converting and transposing the fp32 W2 in every block;
 * NULL = as before.  Same values.
 * All pointers device memory; X/Ppre/dX of `dtype`, everything else f32 (labels int64, pose_valid uint8).
 * flags: APA_FLAG_SOFTMAX_ATT / RELU_ATT / TRAIN / RNG_DEVICE as for apa_attn_pool_fwd.
 * APA_FLAG_FROZEN_INPUT (also the _clips and _multilabel forms): io->dX is ignored and may be NULL -- the pooling pass
 * stores nothing and the pose head's dX product dPpre . W1^T (with the pooling share in its epilogue) is not launched;
 * every other output is unchanged bit for bit.  32 x 14x14x2048 bf16, K = 393: 139.1 -> 113.5 us.
 */
typedef struct apa_pose_attn_step_io {
  const void* X;            /* [N,P,C]                                                   */
  const float* W1;          /* [C,Cp]   PoseLogits/ExtraConv2d_1x1                       */
  const float* b1;          /* [Cp]                                                      */
  const float* W2;          /* [Cp,J]   PoseLogits/Conv2d_1c_1x1                         */
  const float* b2;          /* [J]                                                       */
  const void* W1_bf16;      /* optional bf16 [C,Cp] copy of W1, or NULL                  */
  const void* W2T_bf16;     /* optional bf16 [16,Cp+16] transposed copy of W2, or NULL   */
  const float* Wa;          /* [Cp,1]   Conv2d_PrePose_Attn                              */
  const float* ba;          /* [1]                                                       */
  const float* Wt;          /* [C,K]    top-down conv                                    */
  const float* bt;          /* [K]                                                       */
  const int64_t* labels;    /* [N]                                                       */
  const float* pose_labels; /* [N,P,J]                                                   */
  const uint8_t* pose_valid;/* [N,J]                                                     */
  float action_wt, pose_wt, grad_scale;
  /* activations (outputs) */
  void* Ppre;               /* [N,P,Cp] dtype                                            */
  float* Pl;                /* [N,P,J]                                                   */
  float* att;               /* [N,P]                                                     */
  float* logits;            /* [N,K]                                                     */
  float* zsave;             /* [N,C]                                                     */
  float* abar;              /* [N]                                                       */
  float* loss_action;       /* [1+N]  (as apa_attn_head_train_step)                      */
  float* loss_pose;         /* [1]                                                       */
  /* gradients (outputs) */
  float* G;                 /* [N,K]   d loss / d logits                                 */
  float* dPl;               /* [N,P,J]                                                   */
  float* dZ;                /* [N*P]   gradient at the attention logits (rank-1 factor)  */
  void* dX;                 /* [N,P,C] dtype                                             */
  float *dW1, *db1, *dW2, *db2, *dWa, *dba, *dWt, *dbt;
  /* scratch */
  void* ws_pool;  size_t ws_pool_bytes;   /* apa_attn_pool_workspace_bytes(N,P,C,Cp,K,1,flags) */
  void* ws_pose;  size_t ws_pose_bytes;   /* apa_pose_head_workspace_bytes(N,P,C,Cp,J,dtype)   */
} apa_pose_attn_step_io;
int apa_pose_attn_train_step(const apa_pose_attn_step_io* io, int N, int P, int C, int Cp, int J, int K,
                             unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * One host call for the cfg 003 head at EVALUATION time (eval.py:181-197 on the model of
 * 003_MPII_ResNet_withPoseAttention.yaml): apa_pose_head_fwd followed by apa_attn_head_eval_step(X, Xatt = Ppre, ...).
 * APA_FLAG_TRAIN is cleared (is_training=False); APA_FLAG_SOFTMAX_ATT / RELU_ATT are honoured.
 * Two routes, reported in *io->route when that (host) pointer is given:
 *   1  fused     io->Pl == NULL, dtype bf16, Cp % 128 == 0, C % 64 == 0, X 16-byte aligned, b1 and Wa 16-byte
 *                aligned, and ceil(N*P / 256) * (Cp / 128) no larger than the number of compute units (the pose-head
 *                product then runs as one resident round of the DMA-ring GEMM).  The product's epilogue applies bias
 *                and relu, rounds to bf16 -- the values apa_pose_attn_train_step's attention was trained on --
 *                contracts each 128-column tile with the fp32 Wa and writes one fp32 partial per row and tile; a
 *                second launch adds the Cp / 128 partials in tile order (no atomics: two runs agree bit for bit),
 *                then ba and identity / relu.  pose_pre_logits never exists in memory.
 *   0  composed  every other case (fp32 features, other Cp, Pl requested, ...): the existing kernels back to back
 *                inside the call, pose_pre_logits in the workspace.  With Pl requested and Cp in {256,512,768,1024},
 *                J <= 16, bf16, the Pl product's pass over pose_pre_logits also emits att (as in the training step).
 * (Both routes also need what apa_attn_pool_fwd needs for M == 1: C and Cp whole 16-byte vectors.)
 * Outputs as apa_attn_head_eval_step; att holds the attention map (softmax applied under APA_FLAG_SOFTMAX_ATT).
 * labels / loss ([1+N]) may both be NULL.  Null required pointers: APA_ERR_INVALID_ARG before anything touches the
 * GPU; ws_bytes below apa_pose_attn_eval_workspace_bytes(): APA_ERR_WORKSPACE.
 * want_pose_logits: whether io->Pl will be given (the size covers both routes today and does not depend on it).
 */
typedef struct apa_pose_attn_eval_io {
  const void* X;            /* [N,P,C] dtype                                             */
  const float* W1;          /* [C,Cp]                                                    */
  const float* b1;          /* [Cp]                                                      */
  const void* W1_bf16;      /* optional bf16 [C,Cp] copy of W1 (as in the train step)    */
  const float* W2;          /* [Cp,J]                                                    */
  const float* b2;          /* [J]                                                       */
  const float* Wa;          /* [Cp,1]                                                    */
  const float* ba;          /* [1]                                                       */
  const float* Wt;          /* [C,K]                                                     */
  const float* bt;          /* [K]                                                       */
  const int64_t* labels;    /* [N] or NULL                                               */
  /* outputs */
  float* att;               /* [N,P]                                                     */
  float* logits;            /* [N,K]                                                     */
  float* zsave;             /* [N,C]                                                     */
  float* abar;              /* [N]                                                       */
  float* probs;             /* [N,K]                                                     */
  int64_t* pred;            /* [N]                                                       */
  float* loss;              /* [1+N] or NULL (with labels)                               */
  float* Pl;                /* [N,P,J] or NULL: PoseLogits on request (composed route)   */
  /* scratch */
  void* ws;  size_t ws_bytes;
  int* route;               /* optional, HOST memory: 1 fused, 0 composed                */
} apa_pose_attn_eval_io;
size_t apa_pose_attn_eval_workspace_bytes(int N, int P, int C, int Cp, int J, int K, unsigned flags, int dtype,
                                          int want_pose_logits);
int apa_pose_attn_eval_step(const apa_pose_attn_eval_io* io, int N, int P, int C, int Cp, int J, int K,
                            unsigned flags, int dtype, void* stream);

/* Pose loss: src/loss.py:29-70 ('l2', LOSS_FN_POSE_SAMPLED off) fused with its gradient.
 *   loss[0] = wt * sum_j mean_n( valid[n,j] ? 0.5*sum_p (Pl-lbl)^2 / (N*P) : 0 )
 *   dPl = grad_scale * wt * valid[n,j] * (Pl - lbl) / (N*N*P)
 * Pl, lbl [N,P,J] f32; valid uint8 [N,J]; dPl [N,P,J] f32 or NULL; loss f32 [1];
 * ws: at least apa_pose_l2_workspace_bytes(N,P,J) bytes of device scratch. */
size_t apa_pose_l2_workspace_bytes(int N, int P, int J);
int apa_pose_l2_loss_fwd_bwd(const float* Pl, const float* lbl, const uint8_t* valid, float* loss,
                             float* dPl, void* ws, size_t ws_bytes, int N, int P, int J, float wt,
                             float grad_scale, void* stream);

/* The other action losses gen_losses accepts (src/loss.py:81-101), value + gradient in one launch:
 *   APA_ACTION_LOSS_L2             tf.losses.mean_squared_error(one_hot(labels,K), logits, weights=wt):
 *                                  loss = wt * mean_{n,k} (logits - onehot)^2;  labels int64 [N]
 *   APA_ACTION_LOSS_MULTI_LABEL    mean(tf.nn.weighted_cross_entropy_with_logits(targets, logits,
 *                                  pos_weight)) added with tf.losses.add_loss -- action_loss_wt is NOT
 *                                  applied by the reference (loss.py:93-97), so `wt` is ignored;
 *                                  labels f32 [N,K] multi-hot; the reference passes pos_weight = 10
 *   APA_ACTION_LOSS_MULTI_LABEL_2  tf.losses.sigmoid_cross_entropy(labels, logits) * wt; labels f32 [N,K]
 * loss f32 [1]; G f32 [N,K] or NULL = grad_scale * dloss/dlogits. */
#define APA_ACTION_LOSS_L2 1
#define APA_ACTION_LOSS_MULTI_LABEL 2
#define APA_ACTION_LOSS_MULTI_LABEL_2 3
int apa_action_loss_fwd_bwd(int kind, const float* logits, const void* labels, float* loss, float* G,
                            int N, int K, float wt, float grad_scale, float pos_weight, void* stream);

/* Pose loss with cfg.TRAIN.LOSS_FN_POSE_SAMPLED (src/loss.py:36-52), literally -- including the
 * loop header's swapped names, by which "keep all positive pixels" tests the LOGITS:
 *   ratio_j = #(lbl[..,j] > 0) / (N*P);  sel = (uniform < ratio_j) * (lbl == 0)
 *   mask = (sel + (Pl > 0)) > 0;         loss = wt * sum_j mean_n( valid ? 0.5 * mean_p (mask*(Pl-lbl))^2 : 0 )
 * uniform f32 [N,P,J]: the caller's tf.random_uniform draws in [0,1) (passed in like a dropout mask:
 * TF's stream cannot be reproduced); mask_out f32 [N,P,J] or NULL = end_points['PoseLossMask'];
 * dPl [N,P,J] or NULL (the mask is a constant of the differentiation, as in TF). */
int apa_pose_sampled_loss_fwd_bwd(const float* Pl, const float* lbl, const uint8_t* valid,
                                  const float* uniform, float* loss, float* dPl, float* mask_out, int N,
                                  int P, int J, float wt, float grad_scale, void* stream);

/* tf.image.resize_images(BILINEAR) as of TF 1.1 (legacy rule: src = dst * in/out, no half-pixel
 * offset; src/loss.py:14-22 on the label map, device tensors): in f32 [N,h,w,C] -> out [N,oh,ow,C]. */
int apa_resize_bilinear_tf1(const float* in, float* out, int N, int h, int w, int C, int out_h, int out_w,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Label generator: PoseToHeatmapOp::Compute, src/custom_ops/pose_to_heatmap.cc:35-96.
 * HOST function (the reference op is DEVICE_CPU and runs inside the input pipeline).
 * pose_host int64 [n_vals], n_vals % (3*out_channels) == 0, triples (x, y, is_visible);
 * heatmap_host f32 [out_ht, out_wd, out_channels] with out_ht = (int)(im_ht*out_wd*1.0/im_wd)
 * (query it with apa_pose_to_heatmap_out_ht); valid_host uint8 [out_channels].
 */
int64_t apa_pose_to_heatmap_out_ht(int64_t im_ht, int64_t im_wd, int64_t out_wd);
int apa_pose_to_heatmap(const int64_t* pose_host, int64_t n_vals, int64_t im_ht, int64_t im_wd,
                        int64_t out_wd, int out_channels, float marker_wd_ratio, int do_gauss_blur,
                        float* heatmap_host, uint8_t* valid_host);

/* Label post-processing: _replay_augmentation (src/preprocess_pipeline.py:21-45) + :195-214.
 * HOST function.  hm_host uint8 [h,w,J] (the python wrapper's *255 heat-map); the crop
 * (crop_y, crop_x, crop_h, crop_w) is given in the coordinates of the orig_h x orig_w image it was
 * recorded on and is rescaled to the heat-map with the reference's float32 ratios and truncation;
 * flip != 0 mirrors left-right after the crop; values become float (x/255), are min-max
 * normalised ((x - min) / (max(x - min) + eps), eps = cfg.EPS = 1e-14) and resized with the TF1
 * legacy bilinear rule to out_side x out_side.  out_host f32 [out_side, out_side, J]. */
int apa_pose_label_replay_resize(const uint8_t* hm_host, int h, int w, int J, int orig_h, int orig_w,
                                 int crop_y, int crop_x, int crop_h, int crop_w, int flip,
                                 int out_side, float eps, float* out_host);

/* The same label path on the DEVICE for a whole batch, canvas-free (training call: no blur,
 * src/preprocess_pipeline.py:162): apa_pose_to_heatmap -> *255 -> apa_pose_label_replay_resize fused,
 * one block per image; bit-identical to the two host functions above (eps: any value << 1, e.g.
 * cfg.EPS = 1e-14, gives the same result on a binary canvas).
 *   pose    int64 [N][max_vals]  (x, y, is_visible) triples, n_vals[n] of them used (multiple of 3*J,
 *           at most 32 people)
 *   geom    int32 [N][9] = im_ht, im_wd, aug_ht, aug_wd, crop_y, crop_x, crop_h, crop_w, flip.
 *           TWO frames, as in the reference: the keypoints are scaled onto the canvas with the size
 *           of the ORIGINAL image (im_ht x im_wd, preprocess_pipeline.py:155-157), while the crop
 *           was recorded on the image AFTER the aspect-preserving resize to RESIZE_SIDE (aug_ht x
 *           aug_wd = preproc_info['image_shape'], vgg_preprocessing.py:325) and is rescaled to the
 *           canvas with ratio = canvas / aug size (_replay_augmentation, :29-36) -- the orig_h x
 *           orig_w of apa_pose_label_replay_resize
 *   labels  f32 [N, out_side, out_side, J];  valid uint8 [N, J];  status int32 [N]: 0 = ok, 1 = the
 *           host path would have failed for this image (bad crop / sizes): its label is all zero. */
int apa_pose_labels_device(const int64_t* pose, const int32_t* n_vals, const int32_t* geom, int N,
                           int max_vals, int out_wd, int J, float marker_wd_ratio, int out_side,
                           float* labels, uint8_t* valid, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * The IMAGE half of the input pipeline (src/preprocess_pipeline.py:5-18 `_resize_if_needed` +
 * models/slim/preprocessing/vgg_preprocessing.py `preprocess_image`, the preprocessing of resnet_v1_*,
 * vgg_* and inception_v2_tsn), all arithmetic in float32 as the reference's graph:
 *   1. limit   src wider than max_wd (cfg.MAX_INPUT_IMAGE_SIZE): lw = max_wd, lh = (int64)(f32(sh) *
 *              (f32(max_wd) / f32(sw))), L = uint8(trunc(legacy bilinear resize of src to [lh, lw])); else L = src
 *   2. resize  scale = f32(side) / f32(lh > lw ? lw : lh), ah = (int32)(f32(lh) * scale), aw likewise;
 *              A = legacy bilinear resize of L to [ah, aw], float32 (ah / aw may land one short of side)
 *   3. crop    [crop_y, crop_y + crop_h) x [crop_x, crop_x + crop_w) of A   4. flip left-right   5. - mean
 * The legacy bilinear rule is the one of apa_resize_bilinear_tf1.
 *
 * HOST function: lh, lw, ah, aw of steps 1-2 -> out[0..3].  APA_ERR_INVALID_ARG for non-positive arguments or
 * an empty result. */
int apa_image_aug_size(int src_ht, int src_wd, int max_wd, int resize_side, int32_t out[4]);

/* Workspace of apa_preprocess_images for N samples of T frames whose sizes are src_hw_host int32 [N][2]
 * (HOST memory): N equal slots, each holding the largest L image of the batch.  0 for invalid arguments. */
size_t apa_preprocess_images_workspace_bytes(int N, int T, const int32_t* src_hw_host, int max_wd);

/* Steps 1-5 for a whole batch on the device: two launches on `stream`, no synchronisation.
 *   src      uint8, ONE packed device buffer of src_bytes bytes; the T frames [T, sh, sw, 3] of sample n start
 *            at byte src_off[n] (int64 [N], any byte offset) and share one geometry (:182-194)
 *   src_hw   int32 [N][2] = sh, sw (device)
 *   geom     int32 [N][9], the record apa_pose_labels_device consumes (device): im_ht, im_wd = the ORIGINAL
 *            size stored with the sample (the keypoint frame; never the limited size; only checked > 0 here),
 *            aug_ht, aug_wd = ah, aw, then crop_y, crop_x, crop_h, crop_w, flip
 *   out      [N, T, crop_h, crop_w, 3] f32 or bf16 (out_dtype; bf16 = the f32 result rounded to nearest even).
 *            Every sample must carry the crop_h x crop_w of sample 0: `out` has N * T * crop_h * crop_w * 3
 *            elements of THAT size, and nothing outside it is written whatever geom holds.
 *   status   int32 [N]: 0 = ok; 1 = the reference would have failed or the sample cannot be served, and its
 *            output is all zero: crop outside A or of another size than sample 0's, non-positive sizes, aug_ht x
 *            aug_wd not what step 2 gives for any resize side, frames reaching past src_bytes, L larger than a
 *            workspace slot.  (Sample 0 without a positive crop size: every status is 1, `out` is untouched.)
 *   ws       apa_preprocess_images_workspace_bytes() bytes (at least 16 * N, else APA_ERR_WORKSPACE) */
int apa_preprocess_images(const uint8_t* src, size_t src_bytes, const int64_t* src_off, const int32_t* src_hw,
                          const int32_t* geom, int N, int T, int max_wd, float mean, void* out, int out_dtype,
                          int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Video frame pooling of per-frame logits, nets_factory.py:354-374.  logits f32 [B*F, K] (F
 * consecutive rows per video) -> pooled f32 [B, K].
 *   w == NULL : pooled = mean over the F frames                                   (:374)
 *   w != NULL : temporal attention (cfg.NET.USE_TEMPORAL_ATT, :362-372): tatt[b,f] =
 *               logits[b,f,:] . w + b[0]; pooled = mean_f(logits * tatt); tatt f32 [B*F] is an
 *               output (end_points['TemporalAttention']) and is needed by the backward call.
 * Backward: dpooled [B,K] -> dlogits [B*F,K], dw [K], db [1]; dlda_ws: B*F floats of scratch. */
int apa_frame_pool_fwd(const float* logits, const float* w, const float* b, float* pooled, float* tatt,
                       int B, int F, int K, void* stream);
int apa_frame_pool_bwd(const float* logits, const float* w, const float* tatt, const float* dpooled,
                       float* dlogits, float* dw, float* db, float* dlda_ws, int B, int F, int K,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * The action loss of a video clip: frame pooling / temporal attention (nets_factory.py:354-374), the softmax
 * cross-entropy on the POOLED logits (src/loss.py:74-80) and the backward of both down to the frame logits (TF
 * autodiff in the reference), value + gradient in two launches.
 *   a[r]        = logits[r,:] . w + b[0]   (w == NULL: 1)                       -> tatt [B*F]
 *   pooled[b,k] = (1/F) sum_f logits[b*F+f, k] a[b*F+f]                         -> pooled [B,K]
 *   loss[1+b]   = -log softmax(pooled[b])[labels[b]];   loss[0] = wt/B sum_b loss[1+b]
 *   G[r,k]      = (1/F) g[b,k] a[r] + d[r] w[k],  g = wt grad_scale/B (softmax(pooled) - onehot),
 *                 d[r] = (1/F) sum_k g[b,k] logits[r,k]                         -> G [B*F,K]
 *   dw[k]       = sum_r d[r] logits[r,k];  db[0] = sum_r d[r]                   (temporal attention only)
 * logits f32 [B*F,K] (F consecutive rows per clip); labels int64 [B]; loss f32 [1+B]; w [K], b [1] both NULL for plain
 * averaging (then tatt, dw, db may be NULL and the d / w terms vanish).  Any B, F, K >= 1 with B*F < 2^31.
 * ws: apa_clip_xent_workspace_bytes(B, F, K) bytes of scratch, 4-byte aligned (d [B*F]; K > 4096: the gradient rows).
 * No atomics, every sum in a fixed order: identical calls give bit-identical results; with F == 1 and w == NULL loss and
 * G are bit-identical to apa_softmax_xent_fwd_bwd(logits, labels, ..., N = B).
 * Null required pointers, non-positive sizes, B*F overflow: APA_ERR_INVALID_ARG before anything touches the GPU. */
size_t apa_clip_xent_workspace_bytes(int B, int F, int K);
int apa_clip_xent_fwd_bwd(const float* logits, const int64_t* labels, const float* w, const float* b, float* pooled,
                          float* tatt, float* loss, float* G, float* dw, float* db, void* ws, size_t ws_bytes, int B,
                          int F, int K, float wt, float grad_scale, void* stream);

/* Backward of the global average pool of the attention-free head (cfg 001, resnet_v1.py:206-208
 * `tf.reduce_mean(net, [1, 2])`):  dX[n,p,c] = dz[n,c] / P.   dz f32 [N,C]; dX dtype [N,P,C].
 * (The forward pool is apa_attn_pool_fwd with a constant attention map: its zsave output.) */
int apa_spatial_mean_bwd(const float* dz, void* dX, int N, int P, int C, int dtype, void* stream);

/* zero_out_channels.cc:18-51:  out[n,h,w,c] = channels[c] ? in[n,h,w,c] : 0   (f32, device). */
int apa_zero_out_channels(const float* in, const uint8_t* channels, float* out, size_t n_outer,
                          int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-call hooks (communication / compute overlap, measurement).  The library keeps NO state
 * between calls and none per thread: a caller that wants one of the aids below passes this struct
 * to the *_ex form of an entry point; NULL (or the plain entry points) means "no hooks".  Every
 * member is a hipEvent_t created by the caller (or NULL).  Purely ordering / timing aids: results
 * are unaffected.
 *
 *   grad_ready_event        recorded on the call's stream as soon as the classifier gradients
 *                           dWt / dbt -- 99.7 % of the all-reduce payload -- are final, i.e. after the
 *                           FIRST kernel of the backward pass, before the streaming pass starts: a
 *                           data-parallel trainer starts the RCCL all-reduce of that part of the
 *                           bucket on a second stream while dX / dWa are still being produced
 *                           (deploy.OverlappedGradientSum, bench.py --gpus N).
 *   td_weights_ready_event  the mirror image on the forward side: the stream waits for it
 *                           (hipStreamWaitEvent) immediately before the first kernel that reads
 *                           td_weights / td_biases -- on the M == 1 path that is the logits product,
 *                           AFTER the pooling pass, which only needs the attention weights.  The
 *                           trainer records it on its communication stream once the all-reduce (and
 *                           optimizer update) of td_weights of the previous step is done, so that
 *                           collective hides under the streaming backward pass of step k AND the
 *                           pooling pass of step k+1.
 *   prof_fwd_start/stop     the M == 1 streaming kernels (m1s_pool_fwd_kernel / m1s_bwd_main_kernel) are
 *   prof_bwd_start/stop     launched with hipExtLaunchKernel(start, stop), which brackets exactly that
 *                           dispatch on its stream; hipEventElapsedTime(start, stop) measured ~1.2 us
 *                           above rocprofv3's begin -> end of the same kernel on MI355X (profiles/), a
 *                           constant the caller may keep in mind but bench.py does not subtract.
 */
typedef struct apa_hooks {
  void* grad_ready_event;
  void* td_weights_ready_event;
  void* prof_fwd_start;
  void* prof_fwd_stop;
  void* prof_bwd_start;
  void* prof_bwd_stop;
} apa_hooks;

int apa_attn_pool_fwd_ex(const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                         const float* ba, const float* Wt, const float* bt, float* logits, float* att,
                         float* zsave, float* abar, void* topdown, void* ws, size_t ws_bytes, int N,
                         int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob,
                         uint64_t seed, uint64_t offset, int dtype, void* stream);
int apa_attn_pool_bwd_ex(const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                         const float* ba, const float* Wt, const float* bt, const float* att,
                         const float* zsave, const float* abar, const float* G, void* dX, void* dXatt,
                         float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes,
                         int N, int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob,
                         uint64_t seed, uint64_t offset, int dtype, void* stream);
int apa_pose_att_logits_fwd_ex(const apa_hooks* hooks, const void* X, const float* Pl, const int32_t* sel,
                               int n_sel, int avged, const float* W, const float* b, float* F, float* logits,
                               void* ws, size_t ws_bytes, int N, int P, int C, int J, int K, unsigned flags,
                               float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream);
int apa_pose_att_logits_bwd_ex(const apa_hooks* hooks, const void* X, const float* Pl, const int32_t* sel,
                               int n_sel, int avged, const float* W, const float* F, const float* G, void* dX,
                               int accumulate_dX, float* dPl, float* dW, float* db, void* ws, size_t ws_bytes,
                               int N, int P, int C, int J, int K, unsigned flags, float keep_prob, uint64_t seed,
                               uint64_t offset, int dtype, void* stream);
int apa_attn_head_train_step_ex(const apa_hooks* hooks, const void* X, const void* Xatt,
                                const float* Wa, const float* ba, const float* Wt, const float* bt,
                                const int64_t* labels, float loss_wt, float grad_scale, float* logits,
                                float* att, float* zsave, float* abar, float* loss, float* G, void* dX,
                                void* dXatt, float* dWa, float* dba, float* dWt, float* dbt, void* ws,
                                size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * The one-call training steps on a batch of CLIPS: the N = B * frames feature maps are the folded frames of B clips
 * (nets_factory.py:121-125), the head runs per frame, and the action loss is taken on the pooled logits.  Inside the
 * call: the forward half of the step WITHOUT its folded per-image cross-entropy, apa_clip_xent_fwd_bwd, then the
 * backward half reading G from memory (same workspace: APA_FLAG_WS_FROM_FWD).  Bit-identical to calling
 * apa_attn_pool_fwd, apa_clip_xent_fwd_bwd, apa_attn_pool_bwd back to back with the same arguments (cfg 003: to
 * apa_pose_head_fwd, apa_pose_l2_loss_fwd_bwd, apa_attn_head_train_step_clips under APA_FLAG_DXATT_RANK1,
 * apa_pose_head_bwd_rank1ext -- which is what the cfg 003 form runs for every shape: the launches
 * apa_pose_attn_train_step shares between neighbouring ops on its fast bf16 route sum in other orders, so they are not
 * used here, and io->W1_bf16 / io->W2T_bf16 are not read).
 *   labels int64 [B], loss / io->loss_action f32 [1+B]; logits [N,K] holds the FRAME logits
 *   (end_points['logits_beforePool']); G [N,K] is the gradient at the frame logits.  Pose labels, the pose loss and
 *   dropout stay per frame, over the flat N.  N % frames != 0, a null clip / pooled pointer, temporal attention
 *   without b / tatt / dw / db: APA_ERR_INVALID_ARG before anything touches the GPU.
 *   ws (io->ws_pool for the cfg 003 form): apa_clip_step_workspace_bytes(N, frames, P, C, Ca, K, M, flags) bytes --
 *   the pooling workspace followed by the clip loss's scratch; less: APA_ERR_WORKSPACE.
 */
typedef struct apa_clip_pool {
  int frames;       /* F = num_frames of the [B,F,H,W,C] input, nets_factory.py:121-125 (the fold) and :356-358    */
  const float* w;   /* [K]  TemporalAttention/Conv/weights ([1,1,K,1] squeezed), :362-368; NULL: plain mean (:374) */
  const float* b;   /* [1]  TemporalAttention/Conv/biases (initialised to 1/F, :366-367); NULL with w               */
  float* pooled;    /* [B,K]   end_points['Logits'], the reduce_mean over the frames (:371-374)                      */
  float* tatt;      /* [B*F]   end_points['TemporalAttention'] (:369), [B,F,1,1] flattened; NULL with w              */
  float* dw;        /* [K]     gradient of the temporal conv's weights (tf.gradients); NULL with w                   */
  float* db;        /* [1]     gradient of its bias; NULL with w                                                      */
} apa_clip_pool;
size_t apa_clip_step_workspace_bytes(int N, int frames, int P, int C, int Ca, int K, int M, unsigned flags);
int apa_attn_head_train_step_clips(const apa_clip_pool* clip, const apa_hooks* hooks, const void* X, const void* Xatt,
                                   const float* Wa, const float* ba, const float* Wt, const float* bt,
                                   const int64_t* labels, float loss_wt, float grad_scale, float* logits,
                                   float* att, float* zsave, float* abar, float* loss, float* G, void* dX,
                                   void* dXatt, float* dWa, float* dba, float* dWt, float* dbt, void* ws,
                                   size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                   unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                   int dtype, void* stream);
int apa_pose_attn_train_step_clips(const apa_clip_pool* clip, const apa_pose_attn_step_io* io, int N, int P, int C,
                                   int Cp, int J, int K, unsigned flags, float keep_prob, uint64_t seed,
                                   uint64_t offset, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * The sigmoid ("multi-label") action losses of HICO and Charades, row-parallel, and the one-call training steps
 * under them.  TRAIN.LOSS_FN_ACTION 'multi-label' (src/loss.py:88-97: the mean of
 * tf.nn.weighted_cross_entropy_with_logits(targets, logits, pos_weight=10); the action-loss weight is NOT applied,
 * :93-97 adds the bare mean) and 'multi-label-2' (src/loss.py:98-101: tf.losses.sigmoid_cross_entropy(labels, logits)
 * times the weight); labels are the f32 multi-hot rows of read_sparse_label.  With x a logits row and t its label row:
 *   multi-label:    l_k = (1-t_k) x_k + w_k softplus(-x_k),  l'_k = (1-t_k) - w_k (1 - sigmoid(x_k)),
 *                   w_k = 1 + (pos_weight-1) t_k,  softplus(-x) = log1p(exp(-|x|)) + max(-x, 0)
 *   multi-label-2:  l_k = max(x_k, 0) - x_k t_k + log1p(exp(-|x_k|)),  l'_k = sigmoid(x_k) - t_k
 *   loss[1+n] = (1/K) sum_k l_k;   loss[0] = wt/n_loss sum_n loss[1+n];   G[n,k] = wt grad_scale/(n_loss K) l'_k
 * (wt = 1 for multi-label) -- apa_action_loss_fwd_bwd's arithmetic, which one block walks serially; here one block
 * per row, every sum in a fixed order, no atomics: identical calls give identical bits, and every entry point below
 * runs the same row routine, so they give each other's bits too.  loss[0] sums the rows in the order the softmax
 * entry points use for the same (n_loss, K).
 */
typedef struct apa_multilabel {
  int kind;            /* APA_ACTION_LOSS_MULTI_LABEL | APA_ACTION_LOSS_MULTI_LABEL_2                         */
  const float* labels; /* f32 multi-hot [n_loss, K]; n_loss = N (flat) or N / frames (clips)                  */
  float pos_weight;    /* loss.py:96 passes 10; ignored by multi-label-2                                      */
} apa_multilabel;

/* src/loss.py:88-101 on finished logits f32 [N,K]: loss f32 [1+N], G f32 [N,K].  Two launches, any N, K >= 1.
 * ml / ml->labels NULL, an unknown kind, null pointers, non-positive sizes: APA_ERR_INVALID_ARG before anything
 * touches the GPU. */
int apa_multilabel_loss_fwd_bwd(const apa_multilabel* ml, const float* logits, float* loss /*[1+N]*/, float* G,
                                int N, int K, float wt, float grad_scale, void* stream);

/* apa_clip_xent_fwd_bwd with the sigmoid loss on the POOLED logits in place of the softmax cross-entropy
 * (nets_factory.py:354-374, then src/loss.py:88-101): ml->labels f32 [B,K], loss f32 [1+B]; every other argument,
 * the workspace (apa_clip_xent_workspace_bytes) and the refusals are apa_clip_xent_fwd_bwd's.  With F == 1 and
 * w == NULL loss and G are bit-identical to apa_multilabel_loss_fwd_bwd(ml, logits, ..., N = B). */
int apa_clip_multilabel_fwd_bwd(const apa_multilabel* ml, const float* logits, const float* w, const float* b,
                                float* pooled, float* tatt, float* loss, float* G, float* dw, float* db, void* ws,
                                size_t ws_bytes, int B, int F, int K, float wt, float grad_scale, void* stream);

/* apa_attn_head_train_step_ex (clip == NULL) / apa_attn_head_train_step_clips under a sigmoid action loss: the
 * arguments of those entry points without `labels`.  Bit-identical to apa_attn_pool_fwd, apa_multilabel_loss_fwd_bwd
 * (clips: apa_clip_multilabel_fwd_bwd), apa_attn_pool_bwd back to back.  Flat, M == 1, 4 <= K <= 832 on the small-K
 * route: the rows' loss rides in the logits reducer, and the batch sum in the backward head kernel where that serves
 * the shape (else it is one small launch); else the stand-alone rows kernel runs on the finished logits.  clip: ws holds apa_clip_step_workspace_bytes.
 * ml / ml->labels NULL, an unknown kind, N % frames != 0: APA_ERR_INVALID_ARG before anything touches the GPU. */
int apa_attn_head_train_step_multilabel(const apa_multilabel* ml, const apa_clip_pool* clip /* NULL: flat */,
                                        const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                                        const float* ba, const float* Wt, const float* bt, float loss_wt,
                                        float grad_scale, float* logits, float* att, float* zsave, float* abar,
                                        float* loss, float* G, void* dX, void* dXatt, float* dWa, float* dba,
                                        float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                                        int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                        int dtype, void* stream);

/* apa_pose_attn_train_step (clip == NULL) / apa_pose_attn_train_step_clips under a sigmoid action loss; the pose L2
 * loss stays.  Bit-identical to apa_pose_head_fwd, apa_pose_l2_loss_fwd_bwd, apa_attn_head_train_step_multilabel under
 * APA_FLAG_DXATT_RANK1, apa_pose_head_bwd_rank1ext back to back -- which is what it runs for every shape, flat and on
 * clips: the launches apa_pose_attn_train_step shares between neighbouring ops on its fast bf16 route sum in other
 * orders than the per-op kernels, so they are not used here and io->W1_bf16 / io->W2T_bf16 are not read.  io->labels
 * is unused and may be NULL; io->loss_action is f32 [1+n_loss].  Refusals as above. */
int apa_pose_attn_train_step_multilabel(const apa_multilabel* ml, const apa_clip_pool* clip /* NULL: flat */,
                                        const apa_pose_attn_step_io* io /* io->labels unused, may be NULL */, int N,
                                        int P, int C, int Cp, int J, int K, unsigned flags, float keep_prob,
                                        uint64_t seed, uint64_t offset, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation of clips and of the sigmoid ("multi-label") datasets: what src/eval.py does behind the frame logits --
 * frame pooling / temporal attention (nets_factory.py:354-374), then the scores and the prediction (eval.py:193-197)
 * -- in ONE launch, one block per clip, and the one-call evaluation steps that end in it.
 *   a[r]        = logits[r,:] . w + b[0]   (w == NULL: 1)                       -> tatt [B*F]
 *   pooled[b,k] = (1/F) sum_f logits[b*F+f, k] a[b*F+f]                         -> pooled [B,K]
 *   APA_SCORES_SOFTMAX  scores[b,:] = softmax(pooled[b,:]), pred[b] = its first maximal index; with labels int64 [B]
 *                       loss[1+b] = -log softmax(pooled[b])[labels[b]], loss[0] = (1/B) sum_b loss[1+b]
 *   APA_SCORES_SIGMOID  scores[b,k] = 1 / (1 + exp(-pooled[b,k])), pred[b] = first maximal index of pooled[b,:] (the
 *                       argmax of the LOGITS, eval.py:193); labels and loss must be NULL (eval.py takes no loss)
 * pooled and tatt carry apa_frame_pool_fwd's and apa_clip_xent_fwd_bwd's bits; the softmax scores, pred and loss carry
 * apa_softmax_xent_fwd_bwd's on the same pooled rows (loss[0] in its summation order for (B, K)).  labels == NULL is
 * served by the kernel: no scratch, no memset.  No workspace, no atomics, every sum in a fixed order: identical calls
 * give identical bits.  With labels one extra block recomputes the B rows' losses for loss[0] (B clips of latency on
 * one compute unit; clips of more than 8192 frames: APA_ERR_UNSUPPORTED with labels).
 * Null required pointers (logits, pooled, scores, pred; b and tatt with w), non-positive sizes, B*F past 2^31, an
 * unknown kind, labels without loss or loss without labels, either of them under APA_SCORES_SIGMOID:
 * APA_ERR_INVALID_ARG before anything touches the GPU. */
#define APA_SCORES_SOFTMAX 0   /* eval.py:197 */
#define APA_SCORES_SIGMOID 1   /* eval.py:194-195, TRAIN.LOSS_FN_ACTION starts with 'multi-label' */

/* frame logits f32 [B*F,K] -> pooled [B,K], tatt [B*F] (w != NULL), scores [B,K], pred int64 [B], loss [1+B] */
int apa_clip_scores(int kind, const float* logits, const float* w, const float* b, const int64_t* labels,
                    float* pooled, float* tatt, float* scores, int64_t* pred, float* loss, int B, int F, int K,
                    void* stream);

/* apa_attn_head_eval_step / apa_pose_attn_eval_step on a batch of CLIPS and / or with the sigmoid scores: N = B *
 * clip->frames folded frames, logits [N,K] holds the FRAME logits (end_points['logits_beforePool']), probs [B,K]
 * (io->probs), pred [B], labels [B], loss [1+B].  clip->pooled is required, clip->tatt exactly when clip->w is given
 * (and clip->b with it); clip->dw / clip->db are not read.  clip == NULL: F = 1 without temporal attention -- the
 * logits rows are the pooled rows and no `pooled` is written; with APA_SCORES_SOFTMAX that call IS
 * apa_attn_head_eval_step (apa_pose_attn_eval_step), same launches, same bits.
 * Otherwise the forward half runs WITHOUT the softmax that rides in (or trails) its logits reduction, and the launch
 * of apa_clip_scores is the only one behind the logits: bit-identical to apa_attn_pool_fwd without APA_FLAG_TRAIN
 * (the pose form: preceded by apa_pose_head_fwd, or apa_pose_attn_eval_step up to its logits -- both of its routes
 * are kept) followed by apa_clip_scores.  Workspace: apa_attn_pool_workspace_bytes /
 * apa_pose_attn_eval_workspace_bytes for the flat N; the scores launch needs none.  No allocation, no
 * synchronisation, no memset: capturable like every other entry point.
 * Refused with APA_ERR_INVALID_ARG before anything touches the GPU: what apa_clip_scores refuses, N % frames != 0,
 * and what the flat evaluation steps refuse. */
int apa_attn_head_eval_step_clips(const apa_clip_pool* clip /* NULL: flat */, int scores_kind, const void* X,
                                  const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                  const float* bt, const int64_t* labels, float* logits, float* att, float* zsave,
                                  float* abar, float* loss, float* probs, int64_t* pred, void* ws, size_t ws_bytes,
                                  int N, int P, int C, int Ca, int K, int M, unsigned flags, int dtype, void* stream);
int apa_pose_attn_eval_step_clips(const apa_clip_pool* clip /* NULL: flat */, int scores_kind,
                                  const apa_pose_attn_eval_io* io, int N, int P, int C, int Cp, int J, int K,
                                  unsigned flags, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * ..._WITH_POSE_FEAT (nets_factory.py:289-295): `last_conv = tf.concat([last_conv, pose_logits], -1)`
 * before the dropout and the top-down conv, i.e. J extra fp32 channels Xext [N,P,J] (the PoseLogits
 * output, after the optional ..._2LAYER conv) next to the C channels of X.  The concatenated tensor is
 * never formed: the *_cat entry points take the two parts separately.  With `cat` given
 *   Wt / dWt are the full td_weights [C+J, K] (rows C.. belong to the extra channels),
 *   the dropout mask of the extra channels continues X's flat element stream at index N*P*C
 *   (apa_dropout_mask over N*P*C + N*P*J elements returns both parts),
 *   zext [N,J] is written by the forward call and must be passed unchanged to the backward call,
 *   dXext [N,P,J] receives the gradient w.r.t. Xext (backward call only).
 * M == 1 only, no APA_FLAG_RELU_INPUT, no TopDownAttention dump; cat == NULL is the plain call.
 */
typedef struct apa_concat_feat {
  const float* Xext;
  int J;
  float* zext;
  float* dXext;
} apa_concat_feat;

int apa_attn_pool_fwd_cat(const apa_concat_feat* cat, const apa_hooks* hooks, const void* X,
                          const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                          const float* bt, float* logits, float* att, float* zsave, float* abar,
                          void* topdown, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                          int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                          int dtype, void* stream);
int apa_attn_pool_bwd_cat(const apa_concat_feat* cat, const apa_hooks* hooks, const void* X,
                          const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                          const float* bt, const float* att, const float* zsave, const float* abar,
                          const float* G, void* dX, void* dXatt, float* dWa, float* dba, float* dWt,
                          float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                          int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                          int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * A resident feature cache read by image index.  A frozen-features run reads one tensor epoch after epoch, the cached
 * conv5 map; with the *_cached entry points X addresses the WHOLE cache -- T = cache_images maps [T,P,C] in fp32, bf16
 * or FP8 (APA_DTYPE_FP8_E4M3: the one allocation of apa_fp8_features_bytes(T, P, C) bytes, scales behind all T
 * images' codes) -- and image n of the batch is cache image index[n]: a shuffled mini-batch, or a slice of the cache,
 * without a gathered copy.  Only the feature rows (FP8: and the scale) are fetched through the index; every output,
 * the workspace and the dropout mask (apa_dropout_mask over the flat [N,P,C] index of the BATCH) keep the batch
 * position, so a cached call is bit-identical to the plain call on a gathered copy of the same images, with the same
 * launches.  An index entry outside [0, T) is clamped into the cache -- nothing outside it is ever addressed -- and,
 * with `status` given, counted there by the forward pass (the caller zeroes the word; a training step counts once).
 * labels_cached (the steps): `labels` is [T] and image n's label is labels[index[n]], read by the forward pooling
 * pass; else `labels` is [N] as in the plain steps.
 * Served: the class-agnostic head (M == 1) with attention from the map itself (Xatt == X), identity or ReLU attention,
 * evaluation or training on frozen features; and per-class maps (M == K) from a bf16 cache where the plain entry point
 * takes the fused per-class route -- Ca == C, K <= 64, C % 256 == 0, C <= 8192, Xatt == X, a 16-byte aligned cache --
 * with identity, ReLU or spatial-softmax attention, APA_FLAG_WEIGHT_IMAGES and the tagged keep-bit hand-off of the
 * one-call train step included (the bits are keyed by batch position).  Of that route only the two kernels that read X
 * (the Z | T product and the dW product) have gathered instances; labels_cached leaves its [N] copy in the workspace's
 * materialised-dropout region, which that route never writes.
 * Refused before anything is queued --
 *   APA_ERR_INVALID_ARG: a NULL descriptor or index, cache_images < 1, a non-NULL dX, a backward call or a training
 *                        step without APA_FLAG_FROZEN_INPUT, per-class maps on a cache that is not 16-byte aligned;
 *   APA_ERR_UNSUPPORTED: M != 1 outside the shapes above (fp32 or FP8 caches, K > 64, other C), a separate attention
 *                        input, APA_FLAG_SOFTMAX_ATT with M == 1, APA_FLAG_RELU_INPUT, APA_FLAG_RNG_EXTERNAL, the
 *                        TopDownAttention dump, clips (eval: clip must be NULL);
 * then whatever the plain entry point refuses (for FP8: what the FP8 arm refuses).  Clips and the sigmoid training
 * losses: the *_cached_clips steps below.  Not built: rank > 1, per-class maps from fp32 or FP8 caches, with K > 64 or
 * on the generic route, M == 1 spatial-softmax attention, the concatenated pose channels, the pose head and the
 * cfg 003 steps, clips or sigmoid losses with labels_cached; the epoch calls (apa_attn_head_train_epoch_cached /
 * apa_attn_head_eval_epoch_cached) keep refusing M != 1.
 * Workspace: apa_attn_pool_workspace_bytes of the BATCH shape.  The signatures are those of apa_attn_pool_fwd_ex /
 * apa_attn_pool_bwd_ex / apa_attn_head_train_step_ex / apa_attn_head_eval_step_clips with the descriptor in front.
 */
typedef struct apa_feature_cache {
  const int32_t* index;   /* device, [N], 4-byte aligned: batch image n is cache image index[n] */
  int cache_images;       /* T: images behind X (FP8: the scales sit at the offset of a T-image buffer) */
  int labels_cached;      /* 1: labels is [T], read through index; 0: labels is [N] as ever */
  int32_t* status;        /* device, nullable: number of index entries outside [0, T), which were clamped */
} apa_feature_cache;

int apa_attn_pool_fwd_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const void* X, const void* Xatt,
                             const float* Wa, const float* ba, const float* Wt, const float* bt, float* logits,
                             float* att, float* zsave, float* abar, void* topdown, void* ws, size_t ws_bytes, int N,
                             int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                             uint64_t offset, int dtype, void* stream);
int apa_attn_pool_bwd_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const void* X, const void* Xatt,
                             const float* Wa, const float* ba, const float* Wt, const float* bt, const float* att,
                             const float* zsave, const float* abar, const float* G, void* dX, void* dXatt, float* dWa,
                             float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                             int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                             void* stream);
int apa_attn_head_train_step_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const void* X,
                                    const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                    const float* bt, const int64_t* labels, float loss_wt, float grad_scale,
                                    float* logits, float* att, float* zsave, float* abar, float* loss, float* G,
                                    void* dX, void* dXatt, float* dWa, float* dba, float* dWt, float* dbt, void* ws,
                                    size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags,
                                    float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream);
int apa_attn_head_eval_step_cached(const apa_feature_cache* cache, const apa_clip_pool* clip /* NULL */,
                                   int scores_kind, const void* X, const void* Xatt, const float* Wa, const float* ba,
                                   const float* Wt, const float* bt, const int64_t* labels, float* logits, float* att,
                                   float* zsave, float* abar, float* loss, float* probs, int64_t* pred, void* ws,
                                   size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags,
                                   int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Clips and the sigmoid ("multi-label") losses from a resident FRAME cache: the one-call steps of
 * apa_attn_head_train_step_clips / apa_attn_head_train_step_multilabel / apa_attn_head_eval_step_clips with the cache
 * descriptor in front.  The N = B * clip->frames batch images are the frames index[] names (apa_sample_clip_frames
 * writes such an index, and the clips' labels, on the device); the clip loss, the sigmoid reducers and the scores
 * launch never see X, so nothing but the pooling passes' gathered instances differs from the plain steps.
 * Contract: bit-identical to the same clip / multi-label step on a gathered copy of the B * frames frames, with the
 * same launches -- for fp32, bf16 and FP8 caches, FP8 keeping its own limits.
 *   apa_attn_head_train_step_cached_clips(cache, ml, clip, hooks, <the arguments of apa_attn_head_train_step_cached
 *   from X on>): ml == NULL: the softmax cross-entropy on `labels` (int64 [N], or [B] with a clip); ml given: the
 *   sigmoid loss on ml->labels ([N,K], or [B,K] with a clip) and `labels` is not read (it may be NULL).  clip == NULL:
 *   flat.  loss is [1 + N] flat, [1 + B] on clips.  ml == NULL && clip == NULL: the call IS
 *   apa_attn_head_train_step_cached, same launches, same bits (labels_cached included).
 *   apa_attn_head_eval_step_cached_clips(cache, clip, scores_kind, <the arguments of apa_attn_head_eval_step_clips from
 *   X on>): clip == NULL is apa_attn_head_eval_step_cached with a NULL clip.
 * Workspace: apa_clip_step_workspace_bytes of the batch shape for a training step with a clip,
 * apa_attn_pool_workspace_bytes otherwise (every evaluation step: the scores launch needs none).
 * Refused before anything is queued, in this order --
 *   1. what apa_attn_head_train_step_cached / apa_attn_head_eval_step_cached refuse about the descriptor, the
 *      dimensions, dX, APA_FLAG_FROZEN_INPUT and the forms a cache cannot have, with the same text;
 *   2. training: an invalid ml (apa_attn_head_train_step_multilabel's refusals);
 *   3. APA_ERR_INVALID_ARG: labels_cached = 1 together with a clip or an ml ("labels_cached"): such labels are per clip
 *      or per row and come from the sampler, not from a per-frame table behind the index;
 *   4. what the plain clip / multi-label / evaluation entry points refuse (N % frames != 0, the clip's pointers, the
 *      scores kind, labels and loss; then the pooling call's own checks and the workspace), with their text.
 * apa_attn_head_eval_step_cached keeps refusing any clip as it always did.
 */
int apa_attn_head_train_step_cached_clips(const apa_feature_cache* cache, const apa_multilabel* ml /* NULL: softmax */,
                                          const apa_clip_pool* clip /* NULL: flat */, const apa_hooks* hooks,
                                          const void* X, const void* Xatt, const float* Wa, const float* ba,
                                          const float* Wt, const float* bt, const int64_t* labels, float loss_wt,
                                          float grad_scale, float* logits, float* att, float* zsave, float* abar,
                                          float* loss, float* G, void* dX, void* dXatt, float* dWa, float* dba,
                                          float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C,
                                          int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                                          uint64_t offset, int dtype, void* stream);
int apa_attn_head_eval_step_cached_clips(const apa_feature_cache* cache, const apa_clip_pool* clip /* NULL: flat */,
                                         int scores_kind, const void* X, const void* Xatt, const float* Wa,
                                         const float* ba, const float* Wt, const float* bt, const int64_t* labels,
                                         float* logits, float* att, float* zsave, float* abar, float* loss,
                                         float* probs, int64_t* pred, void* ws, size_t ws_bytes, int N, int P, int C,
                                         int Ca, int K, int M, unsigned flags, int dtype, void* stream);

/* "These B videos, F frames each" -> the index a *_cached call reads, and the clips' labels, in ONE launch on the
 * device: no workspace, no host synchronisation, capturable; identical calls give identical bits.
 *   video_first  int32 [V]   cache slot of each video's frame 0
 *   video_frames int32 [V]   its frame count n >= 1 (a smaller value is read as 1)
 *   videos       int32 [B]   the batch's video ids; an id outside [0,V) is clamped and, with `status` given, counted
 *                            there (the caller zeroes the word; the convention of apa_feature_cache.status)
 *   u            f32 [B*F]   the caller's uniform draws in [0,1) (as apa_pose_sampled_loss_fwd_bwd's `uniform`;
 *                            TensorFlow's random stream is not reproduced); read by RANDOM_SEGMENT only -- under
 *                            UNIFORM it is ignored, NULL or not
 *   index        int32 [B*F] = video_first[v] + frame_i, clip b's frames at [b*F, (b+1)*F)
 *   video_labels int64 [V] (nullable) -> labels int64 [B];  video_targets f32 [V,K] (nullable) -> targets f32 [B,K]
 * The frame rule is _get_frame_sublist (src/datasets/image_read_utils.py:12-44) as video_data_utils.py:79-81 calls it
 * (num_consec_frames = 1, start_frame = 0), with its int32 `/` read as floor division (TF 1.1 under Python 2: our
 * reading, TensorFlow is absent):
 *   step = max((n - 1) / F, 1)
 *   APA_CLIP_FRAMES_UNIFORM         frame_i = min(step * i, n - 1)
 *   APA_CLIP_FRAMES_RANDOM_SEGMENT  lo = min(step * i, n - 2), hi = min(step * (i + 1), n - 1),
 *                                   frame_i = lo + min((int)(u[b*F+i] * (float)(hi - lo)), hi - lo - 1) in fp32,
 *                                   clamped to [0, n - 1]; hi <= lo (n = 1): lo clamped
 * Refused with APA_ERR_INVALID_ARG before anything is queued: a null video_first / video_frames / videos / index,
 * video_labels without labels or video_targets without targets, non-positive V / B / frames (K with video_targets),
 * an unknown mode, RANDOM_SEGMENT without u, B * frames past 2^31 - 1. */
#define APA_CLIP_FRAMES_UNIFORM 0
#define APA_CLIP_FRAMES_RANDOM_SEGMENT 1
int apa_sample_clip_frames(const int32_t* video_first, const int32_t* video_frames,
                           const int64_t* video_labels /* NULL */, const float* video_targets /* NULL */,
                           const int32_t* videos, const float* u /* NULL */, int32_t* index, int64_t* labels,
                           float* targets, int32_t* status /* NULL */, int V, int B, int frames, int K, int mode,
                           void* stream);

/* apa_quantize_features_fp8 into place: the n images of src become images [first, first + n) of the T-image FP8 cache
 * at `cache` (same rule, same kernel; status int32 [n]).  Slots outside the cache: APA_ERR_INVALID_ARG. */
int apa_quantize_features_fp8_at(const void* src, int src_dtype, void* cache, int cache_images, int first,
                                 int32_t* status, int n, int P, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Class attention maps (nets_factory.py:247-328: end points 'TopDownAttention' / 'PosePrelogitsBasedAttention') of T
 * chosen classes per image, in one pass over the map the top-down conv reads -- the K-map [N,P,K] dump is never built:
 *     topdown[n,t,p]   = sum_c x[n,p,c] * Wt[c,k] + bt[k]            k = classes[n,t],  x = X (APA_FLAG_RELU_INPUT: max(X,0))
 *     combined[n,t,p]  = att[n,p, M == 1 ? 0 : k] * topdown[n,t,p]
 *     class_logit[n,t] = (1/P) * sum_p combined[n,t,p]               (the evaluation step's logits[n,k])
 * X [N,P,C] f32 / bf16; att [N,P,M] f32, M == 1 or K: the `att` output of an evaluation step (softmax / relu already
 * applied); Wt [C,K], bt [K] f32; classes [N,T] int32 on the device; the three outputs f32, [N,T,P] / [N,T,P] / [N,T].
 * A class id outside [0,K) is clamped and, with `status` given, counted there (the caller zeroes the word; the
 * convention of apa_feature_cache.index).  Evaluation semantics only: no dropout.  fp32 accumulation in a fixed order,
 * no floating-point atomics: two calls give the same bits.  At most three launches.  hooks (may be NULL): only
 * prof_fwd_start / prof_fwd_stop are read; they bracket the dispatch of the pass over X.
 * Refused before anything touches the GPU, in this order --
 *   APA_ERR_INVALID_ARG   a null pointer (status may be NULL), a non-positive N / P / C / K / M, M not 1 or K, a flag
 *                         bit other than APA_FLAG_RELU_INPUT, an unknown dtype
 *   APA_ERR_UNSUPPORTED   APA_DTYPE_FP8_E4M3, T outside 1 .. APA_EXPLAIN_MAX_CLASSES, C % 4 != 0, T * C > 16384 (the
 *                         weights of an image's classes are staged in 64 KiB of LDS)
 *   APA_ERR_WORKSPACE     ws_bytes < apa_attn_explain_workspace_bytes(...) (which is 0 for arguments refused above)
 *   APA_ERR_INVALID_ARG   X not aligned to its load width (16 bytes; 8 for bf16 with C % 8 == 4), ws not to 16 bytes
 */
#define APA_EXPLAIN_MAX_CLASSES 8
size_t apa_attn_explain_workspace_bytes(int N, int P, int C, int K, int T, int dtype);
int apa_attn_explain(const apa_hooks* hooks /* NULL */, const void* X, const float* att, const float* Wt, const float* bt, const int32_t* classes,
                     float* topdown, float* combined, float* class_logit, int32_t* status, void* ws, size_t ws_bytes,
                     int N, int P, int C, int K, int M, int T, unsigned flags, int dtype, void* stream);

/* The reference's overlaid heat-map (src/train.py:184-195, _gen_overlayed_img) at image size:
 *     m    = tf.image.resize_images(map, [H,W])          TF 1.1 legacy bilinear, the rule of apa_resize_bilinear_tf1
 *     gray = 0.2989 r + 0.5870 g + 0.1140 b               float32, summed in that order
 *     out  = 0.5 * [gray, gray, gray] + 0.5 * [255 m, 0, 0]
 * maps [N,T,h,w] f32 (any of att / topdown / combined); images [N,H,W,3] f32, the network's input (mean-subtracted);
 * overlay_f32 [N,T,H,W,3] f32 and overlay_u8 [N,T,H,W,3] uint8, either may be NULL but not both.  The uint8 form is
 * the rule tf.summary.image documents, per (n,t) image with lo / hi the min / max of its H*W*3 float values:
 *     lo <  0: s = 127 / max(|lo|,|hi|), o = 128;     lo >= 0: s = 255 / hi, o = 0;     max(|lo|,|hi|) == 0: s = 0
 *     u8 = (uint8) min(255, max(0, trunc(v * s + o)))
 * The resized map is never materialised.  One launch, two with overlay_u8 (which needs a workspace of
 * apa_attention_overlay_workspace_bytes(N, T) bytes, else APA_ERR_WORKSPACE; 0 for non-positive arguments).
 * Null maps / images, no output, non-positive sizes: APA_ERR_INVALID_ARG before anything touches the GPU. */
size_t apa_attention_overlay_workspace_bytes(int N, int T);
int apa_attention_overlay(const float* maps, const float* images, float* overlay_f32, uint8_t* overlay_u8, void* ws,
                          size_t ws_bytes, int N, int T, int h, int w, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * The metric an evaluation reports (src/eval.py:303-306): per-class average precision, their mean and the accuracy of
 * T accumulated score rows, on the device -- src/eval/utils.py:4-16 (compute_map) over
 * src/eval/cap_eval_utils.py:55-109 (calc_pr_ovr_noref + voc_ap), in float64.
 *     scores  [T,K] f32 row-major, contiguous
 *     labels  [T] int64, or NULL        class k's positives are labels == k (compute_map)
 *     targets [T,K] f32 multi-hot, or NULL        class k's positives are targets[:,k] > 0 (calc_pr_ovr_noref's counts > 0)
 *     ap      [K] f64     npos [K] int32: the positives of each class
 *     summary [3] f64     mAP, accuracy, the number of classes with positives
 *     status  [2] int32   NaN scores seen, labels outside [0,K)         (written, not accumulated)
 * Exactly one of labels / targets is given.  The accuracy -- the share of rows whose FIRST maximum (np.argmax) is the
 * label -- exists with labels only; with targets summary[1] is NaN.
 *
 * THE RANKING RULE.  A class's scores are ranked in descending order; equal scores are ordered by DESCENDING sample
 * index (what np.argsort(out, kind='stable')[::-1] gives).  -0.0 and +0.0 are equal; +-inf are ordinary values; a NaN
 * is counted in status[0] and ranked behind every number; a label outside [0,K) is counted in status[1] and is no
 * class's positive.  (The reference ranks with np.argsort(out)[::-1], whose order under ties is that of an unstable
 * introsort and cannot be stated; on tie-free scores the two rankings are the same.)
 *
 * THE VALUE.  With ctp_i the positives among ranks 0 .. i:  P_i = ctp_i / (i + 1),  R_i = ctp_i / npos, both correctly
 * rounded float64 quotients;  E_i = max(P_i, P_{i+1}, ...);  ap = sum over the positives i of (R_i - R_{i-1}) * E_i,
 * the difference taken between the two rounded quotients.  The counts are integers and the maximum is exact; the sum
 * runs in rank order, as voc_ap's loop adds its terms, so on tie-free scores ap has the host routine's rounding (a class
 * whose samples are all positives gets exactly 1.0), and two calls on the same input give the same bits.  mAP adds the
 * classes' values in one fixed order of its own (np.mean's pairwise order is not restated: the values lie in [0,1], the
 * two means differ by at most K * 2^-52).  A class without positives has npos = 0, ap = 0 and is left out of the mean;
 * mAP is the mean of the others' ap, NaN if there are none.
 *
 * Three launches on `stream`, no floating-point atomics, no synchronisation.  A class's keys are sorted in ONE block's
 * LDS, which bounds T: APA_AP_MAX_SAMPLES (128 KiB of keys).  Larger evaluations are not served (no multi-pass sort).
 * Refused before anything touches the GPU, in this order --
 *   APA_ERR_INVALID_ARG   a null scores / ap / npos / summary / status; both or neither of labels / targets;
 *                         T < 1 or K < 1
 *   APA_ERR_UNSUPPORTED   T > APA_AP_MAX_SAMPLES
 *   APA_ERR_WORKSPACE     ws NULL or ws_bytes < apa_average_precision_workspace_bytes(T, K) (0 for arguments refused
 *                         above)
 *   APA_ERR_INVALID_ARG   ws not 16-byte aligned
 */
#define APA_AP_MAX_SAMPLES 16384
size_t apa_average_precision_workspace_bytes(int T, int K);
int apa_average_precision(const float* scores, const int64_t* labels, const float* targets, int T, int K, double* ap,
                          int32_t* npos, double* summary, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * NET.USE_POSE_PRELOGITS_BASED_ATTENTION_RANK = R > 1 (nets_factory.py:247-328) with ONE bottom-up map: R attention
 * maps, each with top-down weights of its own, pooled in one streaming pass over X per direction.  Every further
 * attention conv ('Conv2d_PrePose_Attn<r>', a 1x1 conv on a one-channel map) is a scalar affine map of the map
 * before it:
 *     Z_0 = Xatt . Wa + ba        Z_r = chain_w[r-1] * Z_{r-1} + chain_b[r-1]  (r = 1 .. R-1)       A_r = f(Z_r)
 *     z_r[n,:] = (1/P) sum_p A_r[n,p] Xt[n,p,:]       abar_r[n] = (1/P) sum_p A_r[n,p]       Xt = X * mask / keep
 *     logits   = sum_r ( z_r . Wt_r + abar_r (x) bt_r )
 * f is the identity or, with APA_FLAG_RELU_ATT, relu; ONE dropout mask serves all ranks (the reference drops
 * last_conv once).  The flat argument list carries rank 0 (Wt, bt, dWt, dbt); the descriptor in front of it carries
 * ranks 1 .. R-1, entry r-1 for rank r.  Buffers of the rank calls:
 *     att [N,P,R] (end point 'PosePrelogitsBasedAttention'), zsave [N,R,C], abar [N,R], logits [N,K],
 *     rank.z0 [N,P]: Z_0, written by the forward call, read by the backward call (the relu gates of every rank
 *     follow from it).
 * The backward call adds dchain_w / dchain_b (one float each) and dWt / dbt of ranks 1 .. R-1; dX, dXatt, dWa, dba as
 * apa_attn_pool_bwd.  Results repeat bit for bit (no atomics).  apa_attn_head_train_step_rank is forward, softmax
 * cross-entropy (apa_softmax_xent_fwd_bwd: loss [1+N], G [N,K]) and backward in one host call, bit-identical to
 * the three calls made separately.
 *
 * Served: M == 1; fp32 / bf16 features with C a whole number of 16-byte vectors up to 2048 channels (a separate
 * attention input: any such Ca); all three sources of the dropout mask.  Refused before anything is launched:
 *   APA_ERR_INVALID_ARG   rank == NULL, rank->extra outside 1 .. APA_RANK_MAX-1, M not 1 or K, a null pointer among
 *                         the first `extra` entries (or z0), any refusal of apa_attn_pool_fwd / _bwd's arguments
 *   APA_ERR_UNSUPPORTED   M != 1, APA_FLAG_SOFTMAX_ATT (not a valid reference configuration with rank > 1),
 *                         APA_FLAG_RELU_INPUT, APA_FLAG_FROZEN_INPUT, C > 2048
 *   APA_ERR_WORKSPACE     ws_bytes < apa_attn_pool_rank_workspace_bytes(...)
 */
#define APA_RANK_MAX 4
typedef struct apa_rank_maps {
  int extra;                              /* R - 1, 1 .. APA_RANK_MAX-1 */
  const float* chain_w[APA_RANK_MAX - 1]; /* device, one float each */
  const float* chain_b[APA_RANK_MAX - 1];
  const float* Wt[APA_RANK_MAX - 1];      /* [C,K] each */
  const float* bt[APA_RANK_MAX - 1];      /* [K] each */
  float* dchain_w[APA_RANK_MAX - 1];      /* backward only */
  float* dchain_b[APA_RANK_MAX - 1];
  float* dWt[APA_RANK_MAX - 1];
  float* dbt[APA_RANK_MAX - 1];
  float* z0;                              /* [N,P] saved by forward, read by backward */
} apa_rank_maps;

/* 0 for a shape or rank (R = extra + 1) that is not served */
size_t apa_attn_pool_rank_workspace_bytes(int N, int P, int C, int Ca, int K, int extra);
int apa_attn_pool_rank_fwd(const apa_rank_maps* rank, const void* X, const void* Xatt, const float* Wa,
                           const float* ba, const float* Wt, const float* bt, float* logits, float* att,
                           float* zsave, float* abar, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                           int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                           int dtype, void* stream);
int apa_attn_pool_rank_bwd(const apa_rank_maps* rank, const void* X, const void* Xatt, const float* Wa,
                           const float* ba, const float* Wt, const float* bt, const float* att,
                           const float* zsave, const float* abar, const float* G, void* dX, void* dXatt,
                           float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N,
                           int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                           uint64_t offset, int dtype, void* stream);
int apa_attn_head_train_step_rank(const apa_rank_maps* rank, const void* X, const void* Xatt, const float* Wa,
                                  const float* ba, const float* Wt, const float* bt, const int64_t* labels,
                                  float loss_wt, float grad_scale, float* logits, float* att, float* zsave,
                                  float* abar, float* loss, float* G, void* dX, void* dXatt, float* dWa,
                                  float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P,
                                  int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                                  uint64_t offset, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused optimizer step (src/train.py:90-94 tf.train.MomentumOptimizer + the slim L2 regulariser of
 * models/slim/nets/resnet_utils.py:241 on conv weights):  for every parameter segment i
 *     g   = grad_scale * grad_flat[off_i ...] + weight_decay[i] * w_i
 *     acc = momentum * acc + g ;   w_i -= lr * acc
 * weights[i]: device pointers (fp32) to the nseg parameter tensors, sizes[i] their element counts
 * (host arrays); grad_flat / acc_flat: the flat all-reduce bucket and the momentum accumulators in
 * the same concatenated order.  weight_decay[i] is 0 for biases.  One launch, any alignment.
 */
#define APA_SGD_MAX_SEGMENTS 16
int apa_momentum_sgd_step(int nseg, float* const* weights, const size_t* sizes,
                          const float* weight_decay, const float* grad_flat, float* acc_flat,
                          float lr, float momentum, float grad_scale, void* stream);
/* The same update; bf16_shadow[i] (HOST array of nseg device pointers, entries may be NULL) additionally receives
 * the UPDATED weights of segment i rounded to bf16 (round-to-nearest-even) -- the operand copy the bf16 MFMA
 * products read (apa_pose_attn_step_io.W1_bf16), kept current by the optimizer's own launch instead of a
 * conversion kernel in every step. */
int apa_momentum_sgd_step_shadow(int nseg, float* const* weights, const size_t* sizes,
                                 const float* weight_decay, const float* grad_flat, float* acc_flat,
                                 float lr, float momentum, float grad_scale, void* const* bf16_shadow,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * A whole epoch over a resident feature cache behind ONE host call: the visiting order drawn on the device, the step
 * and update loop in C, a validation pass that writes every row's scores where the caller wants them.
 *
 * apa_epoch_order: order[i] (int32 [T], device, 4-byte aligned) = the image visited at position i of epoch `epoch`
 * of the run keyed by `seed`; a permutation of [0, T) for every 1 <= T < 2^31.  Counter-based -- every element is
 * computed on its own from (seed, epoch, i, T) -- in one launch: no atomics, no workspace, no sort, no allocation,
 * capturable; identical calls give identical bits.  The rule, for a host restatement (all arithmetic unsigned):
 *   mix64(s, o):   z = s + 0x9E3779B97F4A7C15 * (o + 1);  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31          (mod 2^64: the dropout key's)
 *   hash(x, k0, k1), 32 bits: x ^= k0;  x ^= x >> 16;  x = (x & 0xFFFFFF) * 0xB5297B;  x ^= x >> 13;  x ^= k1;
 *                  x ^= x >> 17;  x = (x & 0xFFFFFF) * 0x68E31D;  x ^= x >> 15          (mod 2^32: the dropout mask's)
 *   b = max(2, bits of T - 1), lb = b / 2, rb = b - lb;  h = mix64(seed, epoch);  key_r = mix64(h, r), r = 0..5,
 *   k0 = its low and k1 = its high 32 bits
 *   perm(x): L = x >> rb, R = x & (2^rb - 1);  for r = 0..5: r even: L ^= hash(R, k0_r, k1_r) & (2^lb - 1),
 *            r odd: R ^= hash(L, k0_r, k1_r) & (2^rb - 1);  return L << rb | R          (a bijection of [0, 2^b))
 *   order[i] = perm applied to i, and again while the image is >= T (cycle walking; two applications on average)
 * Refused with APA_ERR_INVALID_ARG: a NULL or misaligned order, T < 1.
 *
 * apa_attn_head_train_epoch_cached(ep, opt, cache, hooks, <apa_attn_head_train_step_cached's arguments from X on>) IS,
 * bit for bit in every output, weight and accumulator, this loop of steps = ep->count / N passes:
 *   for s in 0 .. steps-1:
 *     apa_attn_head_train_step_cached with cache.index = ep->order + s*N, dropout offset + s, loss + s*(1+N)
 *     apa_momentum_sgd_step(opt->nseg .. opt->acc_flat, opt->lr[s], opt->momentum, opt->grad_scale, stream)
 * Under APA_FLAG_RNG_DEVICE the counter in HBM advances by itself and `offset` is passed unchanged.  loss is the
 * epoch's log [steps][1+N]; logits, att, zsave, abar and G hold the last step's values; dWa..dbt are opt->grad_flat's
 * segments where the update is to see them.  cache->index is ignored; cache_images, labels_cached and status mean what
 * they mean in the step: with labels_cached = 0 `labels` is [count] in visiting order, status counts a clamped id once
 * per visit.  opt->lr is a HOST array read during the call.  No allocation, no synchronisation; workspace: the step's.
 * Refused before the first launch, in this order: a NULL opt / lr; a NULL ep / order; a NULL cache; N < 1; count < N or
 * count % N != 0; steps * N past 2^31 - 1; what apa_momentum_sgd_step refuses (nseg, NULL arrays, a NULL weight); then
 * everything apa_attn_head_train_step_cached refuses, both halves' checks run once for the shape.
 *
 * apa_attn_head_eval_epoch_cached(ep, cache, scores_kind, <apa_attn_head_eval_step_cached's arguments from X on>) IS
 * the loop of steps = ceil(ep->count / N) evaluation steps on order + s*N: the per-row outputs advance by s*N rows
 * (logits, probs [count,K], pred [count]; labels [count] unless labels_cached), loss, where asked for, is logged
 * [steps][1+N]; att, zsave and abar are the last step's.  The last step runs the remaining count - (steps-1)*N rows
 * as a smaller batch in the same workspace, its shape checked before the first launch too; nothing is written past
 * row count.  Refusals as above (count < 1 in place of the batch rule), then the evaluation step's.
 */
typedef struct apa_epoch {          /* what is visited */
  const int32_t* order;             /* device, [count], 4-byte aligned: image ids in visiting order            */
  int count;                        /* train: steps = count / N, count % N == 0; eval: steps = ceil(count / N) */
} apa_epoch;

typedef struct apa_epoch_sgd {      /* the update behind every step: apa_momentum_sgd_step's arguments         */
  int nseg; float* const* weights; const size_t* sizes; const float* weight_decay;
  const float* grad_flat; float* acc_flat;
  const float* lr;                  /* HOST, [steps]: the learning rate of update s                            */
  float momentum, grad_scale;
} apa_epoch_sgd;

int apa_epoch_order(int32_t* order, int T, uint64_t seed, uint64_t epoch, void* stream);
int apa_attn_head_train_epoch_cached(const apa_epoch* ep, const apa_epoch_sgd* opt, const apa_feature_cache* cache,
                                     const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                                     const float* ba, const float* Wt, const float* bt, const int64_t* labels,
                                     float loss_wt, float grad_scale, float* logits, float* att, float* zsave,
                                     float* abar, float* loss, float* G, void* dX, void* dXatt, float* dWa, float* dba,
                                     float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                                     int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                     int dtype, void* stream);
int apa_attn_head_eval_epoch_cached(const apa_epoch* ep, const apa_feature_cache* cache, int scores_kind,
                                    const void* X, const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                    const float* bt, const int64_t* labels, float* logits, float* att, float* zsave,
                                    float* abar, float* loss, float* probs, int64_t* pred, void* ws, size_t ws_bytes,
                                    int N, int P, int C, int Ca, int K, int M, unsigned flags, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight images of the per-class head (M == K) kept current at WEIGHT-UPDATE time instead of being rebuilt by
 * every step.  The per-class products read Wa | Wt (and ba | bt) as padded, concatenated bf16 images inside the
 * workspace (K <= 64: `[C/64][128][64]` k-tile-major for the forward product and `[C][Wt | Wa]` for dX, biases as
 * one f32 [128] row; any K: `[C][Wt (Kp) | Wa (Kp)]`, ba padded to f32 [Kp]); without APA_FLAG_WEIGHT_IMAGES each
 * forward / train-step call rebuilds them from the fp32 parameters (5-6 us of a 58 us HMDB-51 step).
 *
 * apa_per_class_weight_images: builds every image the shape (N,P,C,Ca,K,dtype) can need in `ws` (>= apa_attn_pool_
 *   workspace_bytes(..., M = K)) -- one or two launches, for initialisation and after a checkpoint restore -- and, when
 *   `maps` is given, describes them: maps[i] says "element (c, k) of parameter `role` goes to
 *   dst[(c >> c_shift) * a + (c & ((1 << c_shift) - 1)) * b + k * d + e]" (bf16, or f32 when is_f32).  *nmaps
 *   receives the count (<= APA_WIMG_MAX; 0: this shape keeps no images and the flag changes nothing).
 * apa_momentum_sgd_step_images: apa_momentum_sgd_step_shadow that ALSO rewrites those images from the updated
 *   weights in the same launch: images[i] belongs to parameter segment image_segment[i].
 */
#define APA_WIMG_ROLE_WA 0
#define APA_WIMG_ROLE_BA 1
#define APA_WIMG_ROLE_WT 2
#define APA_WIMG_ROLE_BT 3
#define APA_WIMG_MAX 12
#define APA_WIMG_PER_SEGMENT 3
typedef struct apa_weight_image {
  void* dst;          /* device pointer INTO the workspace                                   */
  int role;           /* APA_WIMG_ROLE_*: the parameter this image is made from              */
  int is_f32;         /* destination element type: 0 = bf16 (round to nearest even), 1 = f32 */
  int cols;           /* columns of the parameter matrix: flat element i is (c, k) = (i / cols, i % cols) */
  int c_shift;
  int a, b, d, e;
} apa_weight_image;
int apa_per_class_weight_images(const float* Wa, const float* ba, const float* Wt, const float* bt, void* ws,
                                size_t ws_bytes, int N, int P, int C, int Ca, int K, int dtype,
                                apa_weight_image* maps, int* nmaps, void* stream);
int apa_momentum_sgd_step_images(int nseg, float* const* weights, const size_t* sizes, const float* weight_decay,
                                 const float* grad_flat, float* acc_flat, float lr, float momentum,
                                 float grad_scale, void* const* bf16_shadow, const apa_weight_image* images,
                                 const int* image_segment, int nimages, void* stream);

/* The other two optimisers src/train.py:84-100 can select (TRAIN.OPTIMIZER 'adam' / 'rmsprop'; no shipped YAML
 * does), same flat layout, two slot buffers, one launch, optional bf16 shadows (may be NULL) as above:
 *   apa_adam_step     tf.train.AdamOptimizer(lr, beta1, beta2, epsilon):  m += (g - m)(1 - beta1);
 *                     v += (g^2 - v)(1 - beta2);  w -= lr_t m / (sqrt(v) + epsilon), where the CALLER passes
 *                     lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) for update number t = 1, 2, ...; slots start at 0.
 *   apa_rmsprop_step  tf.train.RMSPropOptimizer(lr, decay, momentum, epsilon):  ms += (g^2 - ms)(1 - decay);
 *                     mom = momentum mom + lr g / sqrt(ms + epsilon);  w -= mom;  `ms` starts at ONE, `mom` at 0.
 * g = grad_scale * grad_flat[...] + weight_decay[i] * w_i in both. */
int apa_adam_step(int nseg, float* const* weights, const size_t* sizes, const float* weight_decay,
                  const float* grad_flat, float* m_flat, float* v_flat, float lr_t, float beta1, float beta2,
                  float epsilon, float grad_scale, void* const* bf16_shadow, void* stream);
int apa_rmsprop_step(int nseg, float* const* weights, const size_t* sizes, const float* weight_decay,
                     const float* grad_flat, float* ms_flat, float* mom_flat, float lr, float decay, float momentum,
                     float epsilon, float grad_scale, void* const* bf16_shadow, void* stream);

/* ------------------------------------------------------------------------------------------
 * TRAIN.ITER_SIZE accumulation (src/train.py:529-566: `ref = grad` on the first micro-step, `ref += grad` on the
 * following ones, `apply_gradients(ref / ITER_SIZE)` on the last) for micro-batches whose gradients were written
 * into separate flat buckets (deploy.OverlappedMicroBatches runs them on separate streams):
 *     out[i] = ((parts[0][i] + parts[1][i]) + ...) * scale           same summation order as the reference
 * parts: HOST array of nparts device pointers (f32 [n] each; out may alias parts[0]); one launch, any alignment.
 */
#define APA_ACC_MAX_PARTS 8
int apa_accumulate_gradients(float* out, const float* const* parts, int nparts, size_t n, float scale,
                             void* stream);
/* The same sum DIVIDED by `divisor` (IEEE fp32 division), i.e. literally `ref_grad / float(ITER_SIZE)`
 * (src/train.py:560-563): bit-identical to the reference's arithmetic for every ITER_SIZE, where the scale form
 * differs by an ulp unless ITER_SIZE is a power of two.  divisor == 0 is rejected. */
int apa_accumulate_gradients_div(float* out, const float* const* parts, int nparts, size_t n, float divisor,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-variable gradient clipping by L2 norm (TRAIN.CLIP_GRADIENTS; models/slim/deployment/model_deploy.py:297-304:
 * slim.learning.clip_gradient_norms -> tf.clip_by_norm on every variable separately), over any number of fp32
 * segments, in place:
 *     t   = grads[i] + weight_decay[i] * weights[i]         (the regulariser's gradient, clone 0 only)
 *     out = (t * clip) * min(rsqrt(sum(t * t)), 1 / clip)   (TF 1.x clip_by_norm, that order)
 * grad_absent[i] != 0 (optional, may be NULL): the producer never writes segment i (tf.gradients -> None); its
 * gradient is taken as zero and grads[i] is only written.  grads[i] / weights[i]: device pointers, 4-byte aligned
 * (views of a flat bucket at any offset); weights / weight_decay may be NULL when no segment is regularised.
 *   apa_clip_by_norm_workspace_bytes  device workspace (16-byte aligned) for this segment list
 *   apa_clip_by_norm_prepare          writes the segment / chunk table into `ws` (once per binding; waits for its
 *                                     own copies on `stream`, so it must not be captured) and returns the chunk
 *                                     count the run needs
 *   apa_clip_by_norm_run              two launches on `stream`, no host sync, no allocation: capturable in a
 *                                     hipGraph; clip <= 0 is "off" (no launch).  Deterministic: the chunking
 *                                     depends on the sizes only and the partial sums are combined in a fixed order.
 *                                     `ws` must have been prepared and (nseg, nchunks) must be what prepare took /
 *                                     returned, else APA_ERR_INVALID_ARG; the kernels also check a header that
 *                                     prepare writes into `ws` and do nothing if it does not match.
 */
size_t apa_clip_by_norm_workspace_bytes(int nseg, const size_t* sizes);
int apa_clip_by_norm_prepare(int nseg, float* const* grads, const size_t* sizes, const float* const* weights,
                             const float* weight_decay, const unsigned char* grad_absent, void* ws, size_t ws_bytes,
                             int* nchunks, void* stream);
int apa_clip_by_norm_run(void* ws, int nseg, int nchunks, float clip, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement helpers (bench.py): HIP events owned by the library's HIP runtime, for the prof_*
 * members of apa_hooks.
 */
int apa_prof_event_create(void** event);
int apa_prof_event_destroy(void* event);
int apa_prof_event_record(void* event, void* stream);
int apa_prof_event_elapsed_ms(void* start, void* stop, float* ms); /* both must have completed */

#ifdef __cplusplus
}
#endif
#endif /* APA_H_ */
