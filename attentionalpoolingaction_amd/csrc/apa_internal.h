// apa_internal.h -- host-side declarations shared by the translation units of libapa_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "../../include/apa.h"
#include "apa_colsum.h"
#include "apa_gather.h"

namespace apa {

// Thread-local error text behind apa_last_error().
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
// Zero `bytes` (whole 4-byte words) at `p` with a kernel launch on `st`.  Not hipMemsetAsync: a memset node of a captured
// graph is not a launch, and the replays of such graphs did not reproduce the eager calls (tests/test_graph_replay_gpu.py);
// with this, every node a capture of the library records is a kernel.
int zero_fill(void* p, size_t bytes, hipStream_t st);

// Per-device memo slots.  A host thread may hipSetDevice between two calls, so whatever a launcher remembers
// about "the device" (CU count, LDS limit, "hipFuncSetAttribute already done for this kernel") is keyed by the
// CURRENT device id, not just by the thread.
constexpr int APA_MAX_DEVICES = 64;
inline int current_device_slot() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0) d = 0;
  return d % APA_MAX_DEVICES;
}
template <typename T> struct PerDevice {
  T v[APA_MAX_DEVICES] = {};
  T& here() { return v[current_device_slot()]; }
};

#define APA_HIP_CHECK(expr)                                   \
  do {                                                        \
    hipError_t _e = (expr);                                   \
    if (_e != hipSuccess) return ::apa::hip_fail(_e, #expr);  \
  } while (0)

#define APA_LAUNCH_CHECK(name)                                      \
  do {                                                              \
    hipError_t _e = hipGetLastError();                              \
    if (_e != hipSuccess) return ::apa::hip_fail(_e, "launch " name); \
  } while (0)

// apa_hooks members as typed events (all nullptr when the caller passed no hooks)
struct Hooks {
  hipEvent_t grad_ready = nullptr, td_ready = nullptr;
  hipEvent_t fwd0 = nullptr, fwd1 = nullptr, bwd0 = nullptr, bwd1 = nullptr;
  Hooks() {}
  explicit Hooks(const apa_hooks* h) {
    if (!h) return;
    grad_ready = static_cast<hipEvent_t>(h->grad_ready_event);
    td_ready = static_cast<hipEvent_t>(h->td_weights_ready_event);
    fwd0 = static_cast<hipEvent_t>(h->prof_fwd_start); fwd1 = static_cast<hipEvent_t>(h->prof_fwd_stop);
    bwd0 = static_cast<hipEvent_t>(h->prof_bwd_start); bwd1 = static_cast<hipEvent_t>(h->prof_bwd_stop);
  }
};

// Launch `kernel`; with a start / stop event the launch goes through hipExtLaunchKernel, which brackets
// exactly this dispatch with the two events.
template <typename... KArgs, typename... Args>
inline void launch_ev(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t shm, hipStream_t st,
                      hipEvent_t e0, hipEvent_t e1, Args... args) {
  if (e0 || e1)
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)shm, st, e0, e1, 0u, static_cast<KArgs>(args)...);
  else
    hipLaunchKernelGGL(kernel, grid, block, shm, st, static_cast<KArgs>(args)...);
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// element type of a feature map as the GEMM descriptors (0 f32, 1 bf16) and the workspace carves (bytes) take it
inline int dt_code(int dtype) { return dtype == APA_DTYPE_BF16 ? 1 : 0; }
inline size_t dt_size(int dtype) { return dtype == APA_DTYPE_BF16 ? 2 : 4; }

// splitmix64-derived 2x32-bit dropout key (shared by fwd, bwd and apa_dropout_mask).
inline void rng_key(uint64_t seed, uint64_t offset, uint32_t* k0, uint32_t* k1) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (offset + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  *k0 = (uint32_t)z;
  *k1 = (uint32_t)(z >> 32);
}
inline uint32_t keep_thresh(float keep_prob) {
  double t = (double)keep_prob * 65536.0 + 0.5;
  if (t < 0) t = 0;
  if (t > 65536.0) t = 65536.0;
  return (uint32_t)t;
}
// The dropout key as the kernels take it, for the three sources of the mask (apa.h):
//   default               (thresh, seed, offset, nullptr)   counter hash keyed by splitmix64(seed, offset)
//   APA_FLAG_RNG_DEVICE   (thresh, seed, 0, offset_dev)     `offset` is the address of the step counter
//   APA_FLAG_RNG_EXTERNAL (RNG_THRESH_EXTERNAL, bits, 0, nullptr)   `seed` is the address of the caller's
//                         packed keep bits; understood by the rng_*_x device helpers only (apa_device.h)
constexpr uint32_t RNG_THRESH_EXTERNAL_HOST = 0xFFFFFFFFu;
struct RngKeyArgs {
  uint32_t thresh; uint64_t seed, offset; const uint64_t* offset_dev;
};
inline bool rng_external(unsigned flags) { return (flags & 128u /* APA_FLAG_RNG_EXTERNAL */) != 0; }
inline RngKeyArgs rng_resolve(unsigned flags, float keep_prob, uint64_t seed, uint64_t offset) {
  RngKeyArgs k;
  if (rng_external(flags)) {
    k.thresh = RNG_THRESH_EXTERNAL_HOST; k.seed = seed; k.offset = 0; k.offset_dev = nullptr;
  } else if (flags & 8u /* APA_FLAG_RNG_DEVICE */) {
    k.thresh = keep_thresh(keep_prob); k.seed = seed; k.offset = 0;
    k.offset_dev = reinterpret_cast<const uint64_t*>(static_cast<uintptr_t>(offset));
  } else {
    k.thresh = keep_thresh(keep_prob); k.seed = seed; k.offset = offset; k.offset_dev = nullptr;
  }
  return k;
}

// ------------------------------------------------------------------------------------------
// apa_gemm_small.hip: small fp32 GEMM on the f32 MFMA (exact fp32 FMA chain, deterministic):
//   D[i][j] = sum_k A(i,k) * B(k,j) (+ rank-1 term u[i]*v[j]),  i < m, j < n, k < kdim
//   A(i,k) = A[i*a_si + k*a_sk],  B(k,j) = B[k*b_sk + j*b_sj],  D[i*ldd + j]
// splits > 1 runs split-K into `ws` ([splits][m][n] floats) followed by a fixed-order reduce.
// ------------------------------------------------------------------------------------------
size_t sgemm_ws_bytes(int m, int n, int splits);
int sgemm_small(const float* A, long a_si, long a_sk, const float* B, long b_sk, long b_sj,
                float* D, long ldd, int m, int n, int kdim, int splits, const float* u,
                const float* v, float* ws, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// Dense MFMA GEMM (apa_gemm.hip): C = act(A.B + bias) [* dropout] + beta*C, 128x128x32 tiles.
//   a_kc: A stored [M][K] (k contiguous) else [K][M];  b_kc: B stored [N][K] else [K][N].
//   ta/tb/tc: 0 = f32, 1 = bf16.  f32 x f32 runs on the exact f32 MFMA, anything else on bf16 MFMA.
// ------------------------------------------------------------------------------------------
// The fixed-order column sum (ColsumArgs, apa_colsum.h) as a job that may ride on the tail blocks of a split-K reduce
// launch (GemmDesc::tail, round 6): the reduce is memory-bound on its partial tiles, the column sum is a handful of blocks
// that nothing behind the product waits for -- as a launch of its own it cost 4.9 us of the cfg 003 step.  `done` is
// set by gemm_launch when the job was taken; otherwise the caller launches m1_colsum(a) itself.
struct ColsumJob {
  ColsumArgs a;
  bool done = false;
};
// What gemm_launch actually ran (GemmDesc::trace: filled on the host only, read by the kernel-level tests).
enum GemmKind { GEMM_KIND_NONE = 0, GEMM_KIND_GENERIC, GEMM_KIND_BF16, GEMM_KIND_WIDE, GEMM_KIND_RING,
                GEMM_KIND_GLDS64, GEMM_KIND_GLDS128 };
enum GemmReduce { GEMM_REDUCE_NONE = 0, GEMM_REDUCE_VEC, GEMM_REDUCE_SCALAR, GEMM_REDUCE_TAIL };
enum GemmTwin { GEMM_TWIN_NONE = 0, GEMM_TWIN_FUSED, GEMM_TWIN_SERIAL };
struct GemmTrace {
  int kind = GEMM_KIND_NONE;   // GEMM_KIND_GENERIC: gemm128_kernel; GEMM_KIND_BF16: gemm_bf16_kernel
  int splits = 0, k_per_split = 0;
  int mt = 0;                  // ring / wide: MFMA row tiles per wave row (block rows = 32 mt)
  int twin = GEMM_TWIN_NONE;
  int reduce = GEMM_REDUCE_NONE;
};
struct GemmDesc {
  const void* A = nullptr; long lda = 0; int ta = 0; bool a_kc = true;
  const void* B = nullptr; long ldb = 0; int tb = 0; bool b_kc = false;
  void* C = nullptr; long ldc = 0; int tc = 0;
  int M = 0, N = 0, K = 0;
  int n_valid = 0;   // > 0: B (and ldb) cover N zero-padded columns, only the first n_valid are stored
  const float* bias = nullptr;
  float beta = 0.f;
  int act = 0;
  int splits = 1;
  float* ws = nullptr;  // split-K partials, gemm_ws_bytes(M, N, splits)
  int drop_a = 0, drop_c = 0;
  float inv_keep = 1.f; uint32_t thresh = 0; uint64_t seed = 0, offset = 0;
  const uint64_t* offset_dev = nullptr;
  // rank-1 addend of the epilogue (the fused cfg 003 step): C[m,n] += (r1_row[m] * r1_invP * r1_inv_keep) *
  // r1_col[(m / r1_P) * N + n] * bit(m, n) -- the attentional pooling's own dX share A/P . dz . mask/keep, formed here
  // instead of being written by the streaming kernel and read back (beta = 1).  Wide kernel only.
  const float* r1_row = nullptr; const float* r1_col = nullptr; const uint8_t* r1_bits = nullptr;
  int r1_P = 0; float r1_invP = 0.f, r1_inv_keep = 1.f;
  // a second product of the SAME shape, layouts, dtypes, beta, act and split count, served by the same launch
  // (blockIdx.y selects the problem) when the kernel that takes the first one can (DMA ring / 128 x 64 tiles of the bf16
  // path, and the split-K reduce); else the two are launched one after the other.  Only A, B, C, ldc, n_valid, bias
  // and ws differ.  Used by the per-class maps (Z | T, dWt | dWa): bit-identical to two launches.
  const GemmDesc* twin = nullptr;
  // C is a final output of the step that no later launch reads (a 25.7 MB dX): bf16 vector stores carry the
  // non-temporal hint (measured on the HMDB-51 dX kernel: 15.0 -> 13.8 us)
  bool stream_out = false;
  // mid-contraction mask (wide kernel only, bf16 C): C = (A[:, :mid_k] . B[:, :mid_k]^T) * keepbit / keep + the rest of
  // the contraction; mid_bits = keep bits of C's elements, natural layout (bit (e & 7) of byte e >> 3, e = m * N + n)
  const uint8_t* mid_bits = nullptr; int mid_k = 0; float mid_inv_keep = 1.f;
  // contracted epilogue (ring kernel only, opt-in; gemm_bf16_zp_serves says whether a product can have it): C is NOT
  // stored.  Each 128-column tile applies bias / act, rounds to bf16 as a stored C would be, contracts the rounded
  // values with the fp32 zp_w[n0 : n0 + 128] and writes one fp32 partial per row, zp_out[(n0 / 128) * M + row] --
  // N / 128 partials per row, summed in a fixed order by the consumer (the cfg 003 evaluation step: attention logits
  // out of the pose-head product, pre-logit map never written)
  const float* zp_w = nullptr; float* zp_out = nullptr;
  // a column sum to run on the tail blocks of this product's split-K reduce launch (taken only if there is one)
  ColsumJob* tail = nullptr;
  // optional: where to record the kernel kind / split / reduce that served this product (null at product call sites)
  GemmTrace* trace = nullptr;
  // A is a T-image feature cache read by image index (apa_gather.h: GemmRowMap): with a_kc the map applies to the M rows
  // (Ppre = X . W1), else to the contraction rows (dW1 = X^T . dPpre).  B, C, bias, the partials, the dropout element
  // index and every epilogue keep the batch position.  Served by the MAP instances of the bf16 kernels only
  // (gemm_rowmap_check); the plain instances never see it
  GemmRowMap rmap;
};
size_t gemm_ws_bytes(int M, int N, int splits);
int gemm_pick_splits(int M, int N, int K);
// the split gemm_launch runs for a requested one: whole GEMM_GK-deep k chunks (the k tile of apa_gemm.hip's kernels),
// then -- on the bf16 path -- whole 64-deep ones
constexpr int GEMM_GK = 32;
inline void gemm_split(int K, int want, int unit, int* splits, int* k_per_split) {
  int s = want < 1 ? 1 : want;
  int kps = (K + s - 1) / s;
  kps = (kps + unit - 1) / unit * unit;
  *splits = (K + kps - 1) / kps;
  *k_per_split = kps;
}
int gemm_launch(const GemmDesc& d, hipStream_t st);
// The admission rule of a mapped product (d.rmap.index != nullptr), asked by gemm_launch first and by the entry points
// before anything is queued: APA_OK, or APA_ERR_UNSUPPORTED with its sentence -- a product gemm_launch would send to
// the fp32-unpacking kernels (fp32 features, anything gemm_bf16_eligible refuses), a form without a MAP instance, or a
// batch that is not whole images.  `what`: the product's name in the sentence
int gemm_rowmap_check(const GemmDesc& d, const char* what);
// apa_gemm_bf16.hip: the fast bf16 path (128x128x64, transposing LDS reads for k-major operands)
bool gemm_bf16_eligible(const GemmDesc& d);
int gemm_bf16_launch(const GemmDesc& d, int splits, int k_per_split, hipStream_t st);
bool gemm_bf16_twin_ok(const GemmDesc& d, int splits, int k_per_split);   // can d and d.twin share one launch?
bool gemm_bf16_zp_serves(const GemmDesc& d);   // can this product take the contracted epilogue (GemmDesc::zp_*)?
bool gemm_bf16_wide_serves(int M, int N, int K);   // would this all-bf16, k-contiguous, unsplit product take the wide kernel?
int gemm_bf16_wide_tile_rows(int M, int N, int K);  // ... and with how many rows per tile (0 = not served)
// apa_gemm_bf16.hip: C = (A[:, :64] . B[:, :64]^T) * mask/keep + A[:, 64:] . B[:, 64:]^T  (all bf16, k contiguous)
int gemm_bf16_mid_dropout(const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N,
                          int K, float inv_keep, const uint8_t* maskbits, hipStream_t st);

// ------------------------------------------------------------------------------------------
// M == 1 factorised path (apa_m1.hip)
// ------------------------------------------------------------------------------------------
// Fused train step (apa_attn_head_train_step): softmax cross-entropy folded into the logits
// reduction (forward sets `done` when it ran), batch-mean loss written by the backward head kernel.
// Library-internal flag bits (never accepted from a caller: pool_call, apa_capi.hip, masks with APA_PUBLIC_FLAGS)
constexpr unsigned APA_PUBLIC_FLAGS = 0x3FFu;
constexpr unsigned APA_IFLAG_ATT_READY = 1u << 24;      // M == 1, Xatt != X: `att` already holds Z (id / relu applied)
constexpr unsigned APA_IFLAG_NO_ATT_WGRAD = 1u << 25;   // M == 1 + DXATT_RANK1: dWa / dba / RNG bump done by the caller
constexpr unsigned APA_IFLAG_NO_DX = 1u << 26;          // M == 1, Xatt != X: dX is NOT written -- the caller forms the
                                                        // pooling share A/P . dz . mask/keep in its own product's epilogue
constexpr unsigned APA_IFLAG_FINALIZE_LAUNCH = 1u << 27;   // M == 1 forward: m1_finalize_fwd_kernel stays a launch of its
                                                           // own where the logits kernel could merge the partials itself
constexpr unsigned APA_IFLAG_FOLD_TILE16 = 1u << 28;   // M == 1 folded forward: the 16-image geometry at any shape (read from
                                                       // g_m1_iflags only: the probe library's tests)
constexpr unsigned APA_IFLAG_UNPAIRED = 1u << 29;      // M == 1 forward streaming pass: one 256-thread block and one partial row per
                                                       // logical block at any S (read from g_m1_iflags only, by m1_call_fill)

struct M1Xent {
  const int64_t* labels = nullptr;
  float* loss = nullptr;   // [1+N]
  float* G = nullptr;      // [N,K]
  float gscale = 0.f, lscale = 0.f;
  bool done = false;
  bool deferred = false;   // per-class fused path: logits + cross-entropy are finished by the backward activation pass
  float* logits = nullptr; // (deferred: where that pass writes the logits)
  // evaluation form (apa_attn_head_eval_step without ground truth): probabilities + argmax instead
  float* probs = nullptr;     // [N,K]
  int64_t* pred = nullptr;    // [N]
  // sigmoid ("multi-label") action loss instead (apa_*_train_step_multilabel): kind = APA_ACTION_LOSS_MULTI_LABEL[_2],
  // 0 = the softmax cross-entropy above; then `labels` is unused, gscale carries the 1/K of the mean over the classes
  int kind = 0;
  const float* mlabels = nullptr;   // f32 multi-hot [N,K]
  float pos_weight = 1.f;
  bool finished = false;   // (with done) loss[0] is final too: the backward head kernel has nothing to finish
};
// The two factors of a sigmoid action loss over n_loss rows of K classes: loss[0] = lscale * sum of the row means,
// G = gscale * l'.  'multi-label' ignores the action-loss weight (loss.py:93-97 adds the bare mean).
inline void ml_scales(int kind, float wt, float grad_scale, int n_loss, int K, float* lscale, float* gscale) {
  const float w = kind == APA_ACTION_LOSS_MULTI_LABEL ? 1.0f : wt;
  *lscale = w / (float)n_loss;
  *gscale = w * grad_scale / ((float)n_loss * (float)K);
}
// apa_capi.hip: a valid apa_multilabel (non-null, labels given, a sigmoid loss kind), or the refusal in fn's name
int check_multilabel(const char* fn, const apa_multilabel* ml);
// what apa_sample_clip_frames and apa_sample_clip_frames_keyed refuse (apa_clipcache.hip); nothing has touched the GPU
int sample_clip_check(const char* fn, const void* video_first, const void* video_frames, const void* video_labels,
                      const void* video_targets, const void* videos, const void* index, const void* labels,
                      const void* targets, int V, int B, int frames, int K, int mode, bool u_missing);

// ..._WITH_POSE_FEAT (nets_factory.py:289-295): J extra top-down channels (apa_m1_cat.hip), as the caller describes
// them (apa.h): Xext [N,P,J] f32, zext [N,J] f32 (forward output, backward input), dXext [N,P,J] f32 (backward)
using CatFeat = apa_concat_feat;

// Everything a pooling call carries besides its tensors.  The extern "C" wrappers fill it once (pool_call,
// apa_capi.hip: the one place a caller's flags are masked); the one-call steps hand the same descriptor to both
// halves and change only `flags` (and, on clips, `ws_bytes`) in between.
struct PoolDims { int N, P, C, Ca, K, M, dtype; };
struct PoolCall : PoolDims {
  unsigned flags = 0; float keep_prob = 1.f; uint64_t seed = 0, offset = 0;
  void* ws = nullptr; size_t ws_bytes = 0; hipStream_t st = nullptr; Hooks hk;
  const apa_concat_feat* cat = nullptr;   // checked by the entry point (check_cat) before either path sees it
  bool fp8_ok = false;   // the entry point serves APA_DTYPE_FP8_E4M3 (apa_capi.hip: fp8_served); else "unknown dtype"
  // the *_cached entry points (apa.h: apa_feature_cache), checked by cache_check (apa_capi.hip) before either path sees
  // it: X is a T-image cache, batch image n is its image index[n].  fc_labels: the [T] labels to read through the
  // index (labels_cached), which the forward pooling pass drops into the workspace (m1_gathered_labels)
  const apa_feature_cache* fc = nullptr;
  const int64_t* fc_labels = nullptr;
  // set by the cfg 003 cached steps alone (apa_pose_cache.h): the gathered call may carry a separate attention input --
  // batch-shaped, never read through the index (m1_call_fill: the pose form)
  bool fc_pose = false;
};

struct M1Plan {
  int S;        // pixel splits per image
  int ppb;      // pixels per block
  int nblk;     // N * S
  int lsplits;  // split-K factor of the logits GEMM
  // workspace carve (byte offsets)
  size_t off_pacc, off_pstat, off_pdwa, off_pdba, off_dz, off_gemm, off_dzatt, off_cat_e, off_maskbits, total;
};
M1Plan m1_plan(int N, int P, int C, int Ca, int K);

// What the M == 1 path ran (filled on the host only, read by the kernel-level tests through the test-only probe
// library).  The product never sets the pointer: m1_trace() is null there and nothing is recorded.
enum M1Pool { M1_POOL_NONE = 0, M1_POOL_STREAM, M1_POOL_VEC, M1_POOL_GENERIC, M1_POOL_FP8 };
// (4 was the retired partial-logits form; the values are part of the probe interface and stay put)
enum M1Logits { M1_LOGITS_NONE = 0, M1_LOGITS_XENT, M1_LOGITS_XENT_PROBS, M1_LOGITS2, M1_LOGITS_SGEMM = 5,
                M1_LOGITS_ML = 6 };
enum M1Head { M1_HEAD_NONE = 0, M1_HEAD_TILES, M1_HEAD_ROWS, M1_HEAD_SMALL, M1_HEAD_SGEMM };
enum M1Gemv { M1_GEMV_NONE = 0, M1_GEMV_BWD2, M1_GEMV_BWD2_RANK1, M1_GEMV_BWD };
enum M1Reduce { M1_REDUCE_NONE = 0, M1_REDUCE_COLSUM, M1_REDUCE_BWD_REDUCE };
struct M1Trace {
  int pool_fwd, fwd_w, fwd_pix;    // M1Pool; stream: VW and PIX, per-pixel vec: VEC (pix 0)
  int pool_bwd, bwd_w, bwd_pix;
  int fused, keep_bits, relu_input;   // keep_bits: the backward read the forward call's keep bits
  int S, ppb, nblk, cw;            // plan; cw: channels per thread column of m1_finalize_fwd_kernel (on the folded
                                   // route: of the launch it replaces)
  int logits, logits_nv4, logits_nsub;
  int head, head_ug, head_mv;
  int gemv, reduce, rng_bump, cat_fwd, cat_bwd;
};
extern thread_local M1Trace* g_m1_trace;
inline M1Trace* m1_trace() { return g_m1_trace; }
// Beside the trace, and like it reached through the test-only probe library alone: internal flag bits added to every
// m1_forward of this thread (the extern "C" entries mask the caller's own), and what the last traced m1_forward did
// with the finalize step -- M1Trace's layout is part of the probe interface and stays put.
struct M1FwdRoute {
  int folded;     // 1: the partial merge ran in the logits kernel's prologue, 0: m1_finalize_fwd_kernel
  int launches;   // launches behind the pooling pass: finalize (or none), partial logits, reduce
};
extern thread_local unsigned g_m1_iflags;
extern thread_local M1FwdRoute g_m1_fwd_route;
// ... and the partial rows (M1Call::nrows) of the last traced forward / backward m1_call_fill
struct M1Rows { int fwd, bwd; };
extern thread_local M1Rows g_m1_rows;

enum M1Act { M1_ACT_ID = 0, M1_ACT_RELU = 1, M1_ACT_SOFTMAX = 2 };   // passed to the kernels as int
// A forward / backward call: the caller's tensors (M1Fwd / M1Bwd) and, in M1Call, everything the call resolves before
// its first launch, filled by m1_call_fill (which also holds every refusal of the path).  All on the caller's stack.
// (the per-class path takes the same two bundles; zsave is its fp32 [N,P,K] top-down map, abar unused.  topdown: the
// optional TopDownAttention dump of the forward call, feature type)
struct M1Fwd {
  const void *X, *Xatt; const float *Wa, *ba, *Wt, *bt; float *logits, *att, *zsave, *abar; void* topdown = nullptr;
};
struct M1Bwd {
  const void *X, *Xatt; const float *Wa, *Wt, *bt, *att, *zsave, *abar, *G; void *dX, *dXatt; float *dWa, *dba, *dWt, *dbt;
};
struct M1Call {
  int N, P, C, Ca, K, dtype; unsigned flags; hipStream_t st; const CatFeat* cat;
  int act, pool_act;       // M1Act; pool_act: what the pooling kernel applies (id when att is already final, Xatt != X)
  // fused: Xatt == X; train: dropout active; rank1 (APA_FLAG_DXATT_RANK1): the caller's dXatt buffer is fp32 [N*P] and
  // receives dZ itself; ext (APA_FLAG_RNG_EXTERNAL): the caller's keep bits are read by the run-time-loop kernels only;
  // no_dx (APA_FLAG_FROZEN_INPUT / APA_IFLAG_NO_DX): backward: no kernel stores through dX; small: the backward takes the
  // small-K route (m1_small_route_ok); gemv2: Ca is served by the register-resident attention GEMV backward
  bool fused, train, rank1, ext, relu_input, no_dx, small, gemv2;
  M1Pool pool; M1Plan pl;  // the pooling family of both streaming passes; the plan and what is carved from it:
  // partial rows of pacc the forward streaming pass of this call writes: pl.nblk, or pl.nblk / 2 where two logical
  // blocks share one 512-thread block and add their rows before they leave the CU (apa_m1_stream.hip: the paired
  // form -- fp32, stream family, even S, no softmax).  A backward call always has pl.nblk (pdwa / pdba: one row per
  // logical block).  pstat keeps one entry per logical block
  // (the rank-R route fills the same descriptor but runs its own m1r_* kernels, one row per logical block: its two
  // entry points reset the count with m1_call_full_rows)
  int nrows;
  bool paired() const { return nrows != pl.nblk; }
  float *pacc, *pstat, *pdwa, *pdba, *dz, *dzatt, *gemm_ws, *cat_e;   // (dzatt: the caller's dXatt under rank1)
  float* sn;               // [N] G . bt behind pdba (the region is sized nblk + N): null off the small-K route
  uint8_t* maskbits;       // forward (training): where the keep-bits go
  const uint8_t* maskbits_in;   // backward: the forward call's keep-bits, or nullptr (hash again)
  RngKeyArgs key; float inv_keep; uint64_t* bump;   // the dropout key; backward: the device step counter to advance, or null
  const float* ex; float exs;   // backward: per-pixel addend of dA and its scale (the concat channels' share, else att, 0)
  hipEvent_t ev0, ev1, td_ready, grad_ready;   // ev0 / ev1: apa_hooks prof_*, dispatch begin / end of the streaming pass
  // a gathered call (PoolCall::fc): both streaming passes run their gathered instances on `ga`; T: the images behind X
  bool gather; int T; M1Gather ga;
};
// A call whose streaming kernels are not apa_m1_stream.hip's whatever c.pool says (apa_capi.hip: rank_fwd_run /
// rank_bwd_run): one partial row per logical block
inline void m1_call_full_rows(M1Call& c, bool bwd) {
  c.nrows = c.pl.nblk;
  if (m1_trace()) (bwd ? g_m1_rows.bwd : g_m1_rows.fwd) = c.nrows;
}
// where a gathered forward pass leaves labels[index[n]] for the loss reducers behind it: the head of the pdwa region,
// which nothing writes before the backward pass (nblk * C * 4 >= N * 8 bytes for every served C)
inline int64_t* m1_gathered_labels(void* ws, const M1Plan& pl) {
  return reinterpret_cast<int64_t*>(static_cast<char*>(ws) + pl.off_pdwa);
}
// f: a forward call's tensors, or b: a backward call's (the other null); xf: what the forward half of a one-call step
// folded (M1Xent::done: the backward half needs the head kernel), or null
int m1_call_fill(M1Call& c, const PoolCall& d, const M1Fwd* f, const M1Bwd* b, const M1Xent* xf = nullptr);
int m1_forward(const M1Call& c, const M1Fwd& io, M1Xent* xf = nullptr);
int m1_backward(const M1Call& c, const M1Bwd& io, const M1Xent* xf = nullptr);
bool m1_supported(int C, int Ca, int dtype, bool fused);
bool m1_no_dx_supported(int C, int dtype, bool train);   // APA_IFLAG_NO_DX: can the caller form the dX share from the keep bits?
// the FUSED x TRAIN instances of a kernel template: go(std::bool_constant<FUSED>, std::bool_constant<TRAIN>)
template <typename F> inline int m1_fused_train(bool fused, bool train, F&& go) {
  if (fused) return train ? go(std::true_type{}, std::true_type{}) : go(std::true_type{}, std::false_type{});
  return train ? go(std::false_type{}, std::true_type{}) : go(std::false_type{}, std::false_type{});
}
// the FUSED x TRAIN x GATHER instances of a streaming kernel: go(F, TR, G), std::bool_constant tags.  A gathered call
// is fused (m1_call_fill: the cache form) or carries the cfg 003 steps' batch-shaped attention map (the pose form), so
// it has the four instances of m1_fused_train as a plain call has.  The arms that exist for plain calls only (relu on
// the input, softmax, the dX stores) are the launcher's, chosen under `if constexpr (!G)`: no gathered instance of them
// is ever named.
template <typename Fn> inline int m1_pool_form(const M1Call& c, Fn&& go) {
  if (c.gather) return m1_fused_train(c.fused, c.train, [&](auto F, auto TR) { return go(F, TR, std::true_type{}); });
  return m1_fused_train(c.fused, c.train, [&](auto F, auto TR) { return go(F, TR, std::false_type{}); });
}
// ... of an FP8 kernel, which has no FUSED parameter (m1_call_fill: an FP8 call is fused): go(TR, G)
template <typename Fn> inline int m1_train_gather(const M1Call& c, Fn&& go) {
  if (c.gather) return c.train ? go(std::true_type{}, std::true_type{}) : go(std::false_type{}, std::true_type{});
  return c.train ? go(std::true_type{}, std::false_type{}) : go(std::false_type{}, std::false_type{});
}
// the trailing kernel argument of the instance: c.ga, or the empty M1NoGather
template <bool G> inline M1GatherArg<G> m1_gather_arg(const M1Call& c) {
  if constexpr (G) return c.ga; else return M1NoGather{};
}
bool m1s_supported(int C, int dtype);   // apa_m1_stream.hip: "pixel tile x channel split" for wide maps
int m1s_launch_pool_fwd(const M1Call& c, const M1Fwd& io);
int m1s_launch_bwd_main(const M1Call& c, const M1Bwd& io);
bool m1v_supported(int C, int dtype);   // apa_m1_vec.hip: register-resident per-pixel kernels, narrow powers of two
int m1v_launch_pool_fwd(const M1Call& c, const M1Fwd& io);
int m1v_launch_bwd_main(const M1Call& c, const M1Bwd& io);
bool m1g_supported(int C, int dtype);   // apa_m1_generic.hip: any C (run-time channel loop, LDS accumulators)
int m1g_launch_pool_fwd(const M1Call& c, const M1Fwd& io);
int m1g_launch_bwd_main(const M1Call& c, const M1Bwd& io);
// apa_m1_fp8.hip: an FP8 feature cache (APA_DTYPE_FP8_E4M3; io.X: codes, then the per-image scales): fused attention,
// identity / relu, no dX -- pool_check (apa_capi.hip) refuses everything else before a call gets here
constexpr int M1F_MAX_C = 8192;
bool m1f_supported(int C);
int m1f_vectors_per_lane(int C);   // NV of the instance both launchers pick for a supported C: 1 / 2 / 4 / 8
int m1f_launch_pool_fwd(const M1Call& c, const M1Fwd& io);
int m1f_launch_bwd_main(const M1Call& c, const M1Bwd& io);
// the attention GEMV of a separate attention input as launches of their own (apa_m1.hip; m1_forward / m1_backward run
// the same): Z = Xatt . Wa + ba with c.act into io.att; dXatt / the dWa, dba partials from c.dzatt over *nred blocks
int m1_att_gemv_forward(const M1Call& c, const M1Fwd& io);
int m1_att_gemv_backward(const M1Call& c, const M1Bwd& io, int* nred);
// apa_m1_rank.hip: R = 2 .. APA_RANK_MAX attention maps chained from one bottom-up map (apa.h: apa_rank_maps), one
// streaming pass per direction.  RankCall: rank 0 first, then the descriptor's entries; ws: the call's workspace
// (m1_plan's carve in front, the rank region behind it).  M1Fwd / M1Bwd carry rank 0's Wt / bt / dWt / dbt too;
// att is [N,P,R], zsave [N,R,C], abar [N,R].
struct RankCall {
  int R;
  const float* cw[APA_RANK_MAX - 1]; const float* cb[APA_RANK_MAX - 1];
  const float* Wt[APA_RANK_MAX]; const float* bt[APA_RANK_MAX];
  float* dcw[APA_RANK_MAX - 1]; float* dcb[APA_RANK_MAX - 1];
  float* dWt[APA_RANK_MAX]; float* dbt[APA_RANK_MAX];
  float* z0; void* ws;
};
bool m1r_supported(int C, int Ca, int dtype, bool fused);
int m1r_vectors_per_lane(int C, int dtype);   // NVL of the instance both passes pick: f32 2 / 8, bf16 1 / 4; 0: none serves C
size_t m1r_workspace_bytes(int N, int P, int C, int Ca, int K, int R);
int m1r_forward(const M1Call& c, const RankCall& rk, const M1Fwd& io);
int m1r_backward(const M1Call& c, const RankCall& rk, const M1Bwd& io);
bool m1_cat_supported(int J);   // apa_m1_cat.hip: the J extra top-down channels of CatFeat (c.cat)
int m1_cat_forward(const M1Call& c, const M1Fwd& io);
int m1_cat_backward(const M1Call& c, const M1Bwd& io);   // dWt rows C.., dXext, and c.cat_e

// apa_m1_small.hip: LDS-tiled f32-MFMA kernels for the small products of the M == 1 path
bool m1_small_supported(int C, int K);
// Are the small-K head kernels usable?  They read G / Wt / z with 16-byte loads.  The forward's fused loss (any_ck:
// its evaluation form has shape limits of its own), m1_backward and the fused cfg 003 step must agree.
inline bool m1_small_route_ok(int C, int K, const float* G, const float* Wt, const float* zsave, bool any_ck = false) {
  return (any_ck || m1_small_supported(C, K)) && (((uintptr_t)G | (uintptr_t)Wt | (uintptr_t)zsave) & 15) == 0;
}
int m1_bwd_small(const float* G, const float* Wt, const float* zsave, const float* abar,
                 const float* bt, float* dz, float* dWt, float* dbt, float* sn, int N, int C, int K,
                 hipStream_t st);
bool m1_logits2_supported(int C, int K);
size_t m1_logits2_ws_bytes(int N, int C, int K);
// The folded forward: the partial logits kernel merges the pooling pass's S per-block partials in its prologue
// (z, stored too) and the reduce kernel forms abar from the per-block statistics, both with m1_finalize_fwd_kernel's
// own summation chains -- z and abar are outputs then.  null: z and abar are in memory already.
// rows: partial rows per image in pacc (S, or S / 2 behind a paired pooling pass); pstat has S entries per image
struct M1Fold { const float* pacc; const float* pstat; int S, P, rows; };
bool m1_logits2_fold_supported(int N, int C, int rows);
int m1_logits2(float* z, const float* Wt, float* abar, const float* bt, float* logits,
               float* part_ws, int N, int C, int K, hipStream_t st, const M1Fold* fold = nullptr);
int m1_logits2_partials(float* z, const float* Wt, float* part_ws, int N, int C, int K, hipStream_t st,
                        const M1Fold* fold, int* nparts);
// apa_mlloss.hip: the sigmoid action losses.  The fold: partial logits, then reduce + the row's loss per image
// (logits bit-identical to m1_logits2's; loss[0] is left to the backward head kernel, or to clip_loss_finish where
// that kernel does not serve the shape -- m1_forward)
bool m1_logits_ml_supported(int N, int C, int K);
int m1_logits2_ml(float* z, const float* Wt, float* abar, const float* bt, const M1Xent& xf, float* logits,
                  float* part_ws, int N, int C, int K, hipStream_t st, const M1Fold* fold);
// the stand-alone form on finished logits: one block per row, then the batch sum (apa_multilabel_loss_fwd_bwd)
int ml_loss_rows(int kind, const float* labels, float pos_weight, const float* logits, float* loss, float* G, int N,
                 int K, float wt, float grad_scale, hipStream_t st);
// apa_cliploss.hip: clip_finish_kernel -- loss[0] = lscale * sum_b loss[1+b] in the softmax step's order for (B, K);
// with dws also db = sum dws and dw = dws^T x
int clip_loss_finish(const float* x, const float* dws, float* loss, float* dw, float* db, int B, int rows, int K,
                     float lscale, hipStream_t st);
// apa_clipscores.hip: clip_scores_kernel, the one launch behind the logits of an evaluation step -- frame pooling,
// then the scores (kind: APA_SCORES_*), the prediction and, with labels, the loss of the pooled rows.  pooled ==
// nullptr (F == 1, no temporal attention only): the logits rows are the pooled rows.  Arguments checked by the caller
// but for what the launch itself cannot serve.
int clip_scores_launch(const char* fn, int kind, const float* logits, const float* w, const float* b,
                       const int64_t* labels, float* pooled, float* tatt, float* scores, int64_t* pred, float* loss,
                       int B, int F, int K, hipStream_t st);
bool m1_bwd_head_supported(int N, int C, int K);
int m1_bwd_head(const float* G, const float* Wt, const float* zsave, const float* abar,
                const float* bt, float* dz, float* dWt, float* dbt, float* sn, int N, int C, int K,
                hipStream_t st, float* loss = nullptr, float lscale = 0.f);
bool m1_logits_xent_supported(int N, int C, int K, bool eval);
int m1_logits2_xent(float* z, const float* Wt, float* abar, const float* bt,
                    const int64_t* labels, float* logits, float* loss, float* G, float gscale,
                    float* probs, int64_t* pred, float* part_ws, int N, int C, int K, hipStream_t st,
                    const M1Fold* fold = nullptr);
// the fixed-order column sum of ColsumArgs (apa_colsum.h) as a launch of its own: ceil(C / 32) blocks of 1024 threads
int m1_colsum(const ColsumArgs& a, hipStream_t st);

// apa_pose_head.hip.  A pose-head call, described once: its shape, its stream, its workspace and the carve of it
// (pose_call fills it; pose_check holds every refusal, in the order the entry points promise).  fn / ws_name: what the
// refusals call the entry point and its workspace -- a one-call step has two of them and says "pose workspace".
struct PosePlan {
  long R;
  int nchunks;
  size_t off_dppre, off_partial, off_gemm, off_w1b, off_lpart, total;
};
struct PoseCall {
  const char* fn; const char* ws_name;
  int N, P, C, Cp, J, dtype; hipStream_t st;
  void* ws; size_t ws_bytes; PosePlan pl;   // pl: all zero while a dimension is non-positive (pose_check refuses those)
  // the cfg 003 cached steps (apa_pose_cache.h): X is a T-image cache, the two products that read it (Ppre, dW1) take
  // the row map.  index == nullptr on every other call
  GemmRowMap rmap = {};
  char* at(size_t off) const { return static_cast<char*>(ws) + off; }
};
PoseCall pose_call(const char* fn, int N, int P, int C, int Cp, int J, int dtype, void* ws, size_t ws_bytes,
                   void* stream);
// The caller's tensors of a forward / backward call (as M1Fwd / M1Bwd).  The external gradient of dPpre is a map
// (dPpre_ext), rank-1 (ext_row (x) ext_col) or absent; accumulate: dX += dPpre . W1^T; ws_from_fwd: the workspace still
// holds what the forward call on it left there (APA_POSE_WS_FROM_FWD); no_dx (APA_POSE_NO_DX / APA_FLAG_FROZEN_INPUT): the
// dX product is not launched and dX may be null.
struct PoseFwd {
  const void* X; const float *W1, *b1, *W2, *b2; void* Ppre; float* Pl;
};
struct PoseBwd {
  const void* X; const float *W1, *W2; const void* Ppre; const float* dPl; const void* dPpre_ext;
  const float *ext_row, *ext_col; void* dX; float *dW1, *db1, *dW2, *db2; bool accumulate, ws_from_fwd;
  bool no_dx = false;
};
// What the one-call cfg 003 steps add to the two bundles (apa_pose_attn_train_step; the evaluation step reads W1_bf16
// and the attention conv only)
struct PoseStepArgs {
  const void* W1_bf16 = nullptr;        // caller-maintained bf16 copy of W1 (nullptr: converted per call)
  const void* W2T_bf16 = nullptr;       // caller-maintained bf16 [16][Cp] transposed copy of W2 (nullptr: staged per block)
  const float* wa = nullptr; const float* ba = nullptr; float* att = nullptr; bool relu_att = false;
  const float* pose_labels = nullptr; const uint8_t* pose_valid = nullptr; float* dPl = nullptr;
  float pose_wt = 1.f, grad_scale = 1.f;
  // backward half: the attention conv's gradients (they leave with the rows pass, whose external gradient is
  // dZ (x) wa), the pose loss its column sum finishes and the device-side dropout counter it advances
  float* dWa = nullptr; float* dba = nullptr; float* loss_pose = nullptr; uint64_t* rng_bump = nullptr;
  // ... and the attentional pooling's own dX share, formed in the dX product's epilogue (APA_IFLAG_NO_DX on the pooling
  // side): dX = dPpre . W1^T + att/P . dz . mask/keep -- att [R], dz [N, C], keep bits [R * C / 8] (nullptr: all kept).
  // pool_att == nullptr: dX already holds the share
  const float* pool_att = nullptr; const float* pool_dz = nullptr; const uint8_t* pool_bits = nullptr;
  float pool_inv_keep = 1.f;
};
bool pose_step_fast_ok(const PoseCall& c, const PoseFwd& f, const PoseBwd& b);
// apa_pose_head_fwd / apa_pose_head_bwd[_rank1ext] on a call the caller built (the composed route of the cfg 003 steps:
// c.rmap travels with it)
int pose_head_fwd_run(const PoseCall& c, const PoseFwd& f);
int pose_head_bwd_run(const PoseCall& c, const PoseBwd& b);
// c.rmap set: would gemm_rowmap_check admit the two products that read X?  Launches nothing.  w1_shadow: the caller's
// bf16 copy of W1, or null
int pose_rowmap_check(const PoseCall& c, const void* X, const float* W1, const void* w1_shadow, bool backward);
// What the pose head ran (filled on the host only, as M1Trace: the product never sets the pointer; the test-only
// probe library does, around one call, and tests/test_pose_paths_gpu.py reads it back).  0 = not decided by this call.
enum PoseW1 { POSE_W1_NONE = 0, POSE_W1_BF16_COPY, POSE_W1_F32, POSE_W1_REUSED, POSE_W1_SHADOW };
enum PosePl { POSE_PL_NONE = 0, POSE_PL_FAST, POSE_PL_GEMM };
enum PoseRows { POSE_ROWS_NONE = 0, POSE_ROWS_MFMA, POSE_ROWS_VALU, POSE_ROWS_DPPRE };
enum PoseForm { POSE_FORM_NONE = 0, POSE_FORM_PLAIN, POSE_FORM_EXT, POSE_FORM_RANK1 };
enum PoseDw2 { POSE_DW2_NONE = 0, POSE_DW2_ROWS, POSE_DW2_GEMM, POSE_DW2_MEMSET };
enum PoseColsum { POSE_COLSUM_NONE = 0, POSE_COLSUM_TAIL, POSE_COLSUM_OWN };
struct PoseTrace {
  int w1_fwd, pl, pl_ks, pl_fused, pl_w2t;        // forward: PoseW1 of the Ppre product, PosePl, pose_pl_kernel instance
  int rows, wpb, ngrp, G, rpb, form, wa, jm;      // backward: PoseRows; mfma: wpb / ngrp / G; valu: rpb; dppre: jm
  int dw2, colsum, dw1_splits, w1_bwd, dx_beta;   // PoseDw2, PoseColsum, split-K of dW1, PoseW1 of the dX product
};
extern thread_local PoseTrace* g_pose_trace;
inline PoseTrace* pose_trace() { return g_pose_trace; }
// the workspace carve of the pose head: out[0..7] = R, nchunks, off_dppre, off_partial, off_gemm, off_w1b, off_lpart, total
void pose_plan_offsets(int N, int P, int C, int Cp, int J, int dtype, size_t* out);
void* pose_ws_loss_scratch(const PoseCall& c);   // >= apa_pose_l2_workspace_bytes
int pose_fwd_fused(const PoseCall& c, const PoseFwd& f, const PoseStepArgs& a);
int pose_bwd_fused(const PoseCall& c, const PoseBwd& b, const PoseStepArgs& a);
// the pose-head half of apa_pose_attn_eval_step (apa_pose_head.hip) and the size of its column-tile partials.
// f.Ppre is not read (the map stays in the workspace, or is never stored); f.Pl may be null
struct PoseEvalOut { int route; const void* ppre; bool att_ready; };
size_t pose_eval_zpart_bytes(int N, int P, int Cp);
int pose_eval_fwd(const PoseCall& c, const PoseFwd& f, const PoseStepArgs& a, float* zpart, PoseEvalOut* out);

// Per-class maps (apa_pc_fused.hip, apa_pc.hip).  What they ran (filled on the host only, as M1Trace / PoseTrace: the
// product never sets the pointer; the test-only probe library does, around one call, and tests/test_pc_paths_gpu.py
// reads it back).  0 = not decided by this call.  `phase` says whose fields the apa_pc_fused.hip host functions fill:
// 1 pc_forward, 2 pc_backward, 3 pc_weight_images.
enum PcPath { PC_PATH_NONE = 0, PC_PATH_FUSED, PC_PATH_GENERIC };
enum PcPrep { PC_PREP_NONE = 0, PC_PREP_WEIGHTS, PC_PREP_BITS, PC_PREP_BOTH };
enum PcLogitsAt { PC_LOGITS_NONE = 0, PC_LOGITS_FINISH, PC_LOGITS_DX, PC_LOGITS_FWD_ACT };
enum PcXentAt { PC_XENT_NONE = 0, PC_XENT_FWD_ACT, PC_XENT_DX, PC_XENT_BWD_ACT, PC_XENT_OWN };
enum PcAct { PC_ACT_NONE = 0, PC_ACT_F32, PC_ACT_BF16, PC_ACT_FOLDED };   // element type of pc_fwd_act / pc_bwd_act, or
                                                                         // folded into the product / dX kernel
enum PcDx { PC_DX_NONE = 0, PC_DX_FUSED, PC_DX_MID_GEMM, PC_DX_PLAIN_GEMM, PC_DX_WIDE, PC_DX_TWO };
enum PcWaTo { PC_WA_NONE = 0, PC_WA_DX_BETA1, PC_WA_DXATT };
enum PcDw { PC_DW_NONE = 0, PC_DW_FUSED, PC_DW_TWIN_GEMM };
enum PcTailAt { PC_TAIL_NONE = 0, PC_TAIL_DW, PC_TAIL_COLSUM };
struct PcTrace {
  int phase;
  int path_fwd, path_bwd;                               // PcPath
  int prep_fwd, prep_bwd, prep_wimg;                    // PcPrep: what pc_prep_kernel was launched for
  int pad_fwd, pad_segs_fwd, pad_drop_fwd;              // pc_pad_kernel launched; its segments; dropout blocks or not
                                                        // (pc_weight_images, phase 3, records its pad launch here too)
  int pad_bwd, pad_segs_bwd, pad_drop_bwd;
  int cat, fast, reuse_fwd;
  int zt, zt_train, zt_fold, check_tag;                 // pc_fwd_zt_dma_kernel<TRAIN, FOLD> and its tag argument
  int fwd_act, fwd_act_xe, topdown;                     // PcAct of the forward activation pass; PcXent given; topdown given
  int logits, xent;                                     // PcLogitsAt, PcXentAt
  int t_drop_a;                                         // drop_a of the T product (scalar staging)
  int bwd_act, ps, ldg;                                 // PcAct; pixel splits; row stride of dT / dZ
  int dx, upb, dx_splits, rbs, mid_bits, dx_drop_c, wa_to;   // PcDx, fused-dx geometry, PcWaTo
  int dw, dw_S, dw_rows, dw_ctiles, dw_drop_a;          // PcDw, fused-dw geometry; drop_a of the dWt product
  int tail, tail_nrows, next_bits, rng_bump, aux;       // PcTailAt; partial rows; next step's bits; counter bump; loss mean
  int wimg_cat, wimg_fused, wimg_maps;                  // pc_weight_images: [Wt | Wa] concatenated; fused images built; maps
  GemmTrace g_z, g_t, g_dwt, g_dwa, g_dx, g_dxa;        // the gemm_launch calls (g_dx: the wide or the first dX product)
};
extern thread_local PcTrace* g_pc_trace;
inline PcTrace* pc_trace() { return g_pc_trace; }

// apa_pc_fused.hip: per-class maps with K <= 64 (HMDB-51), bf16, Xatt == X: the HBM-bound form
constexpr int PC_DW_MAX_SPLITS = 32;
struct PcFusedWs {
  void* WcatT;      // bf16 [C/64][128][64]: Wa | Wt transposed (zero padded to 64 columns each), k-tile-major
  void* Wcat2;      // bf16 [C][128]: Wt | Wa
  float* bcat;      // f32 [128]: ba | bt
  void* dTdZ;       // bf16 [R][128]: dT | dZ
  float* partial;   // f32 [splits][C][128]
  uint8_t* maskbits;  // [R*C/8]: keep decisions of the dropout mask, bit (e & 7) of byte e >> 3
  float* lpart;       // f32 [ceil(R/32)][2][64]: per-block partial rows of sum_p A * T (folded activation pass)
  uint64_t* bits_tag; // which mask `maskbits` holds: {seed, offset, thresh, n8} + the running step's offset (apa_pc_fused.hip)
};
// fused dx / dw geometry as pc_fused_dx / pc_fused_dw pick it: out[0..5] = upb, splits, rbs, S, rows_per_split, ctiles
void pc_fused_geometry(int R, int C, int* out);

bool pc_fused_supported(int N, int P, int C, int Ca, int K, int dtype, const void* X, const void* Xatt);
// ... its shape half: what a per-class call on a feature cache is admitted by (apa_capi.hip: cache_form_why)
bool pc_fused_shape_supported(int C, int Ca, int K, int dtype);
size_t pc_fused_ws_bytes(int N, int P, int C);
PcFusedWs pc_fused_carve(void* base, int N, int P, int C);
struct PcPrepBits {   // the step's keep bits, written by the weight-preparation launch's extra blocks
  size_t n_elems; float keep_prob; uint64_t seed, offset; const uint64_t* offset_dev;
};
struct PcDwTail {     // what the dW reduce launch's tail blocks also do (see pc_dw_reduce_kernel)
  ColsumArgs cs;      // dbt | dba from the [nblk][2K] block partials (+ the counter bump and the batch-mean aux)
  bool next_bits = false; uint64_t next_seed = 0;                     // also prepare the NEXT step's keep bits (tagged)
};
// weights == false (APA_FLAG_WEIGHT_IMAGES: the images are the caller's business): the keep bits only
int pc_fused_prep(const PcFusedWs& f, const float* Wa, const float* Wt, const float* ba, const float* bt, int C,
                  int K, hipStream_t st, const PcPrepBits* bits = nullptr, bool weights = true);
struct PcFwdFold { float* att; int act; int P; };   // identity (0) / relu (1) attention folded into the product's epilogue
// ga (here and in pc_fused_dw, the two kernels that read X): a gathered call -- X is the cache -- or null
int pc_fused_forward(const PcFusedWs& f, const void* X, float* Z, float* T, int R, int C, int K, bool train,
                     float keep_prob, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, hipStream_t st,
                     bool prebits = false, const PcFwdFold* fold = nullptr, bool check_tag = false,
                     const PcGather* ga = nullptr);
bool pc_fused_dx_supported(int P, int act);
int pc_fused_dx_rows(int R);
int pc_fused_dx(const PcFusedWs& f, const float* G, const float* att, const float* Tm, void* dX, float* pd, int R,
                int C, int K, int P, int act, bool train, float keep_prob, const M1Xent* defer, hipStream_t st);
int pc_fused_logits_finish(const PcFusedWs& f, float* logits, int N, int P, int K, hipStream_t st);
int pc_fused_dw(const PcFusedWs& f, const void* X, float* dWt, float* dWa, int R, int C, int K, bool train,
                float keep_prob, hipStream_t st, const PcDwTail* tail = nullptr, const PcGather* ga = nullptr);

// apa_pc.hip: per-class bottom-up maps (M == K); Tsave = fp32 [N,P,K] top-down map saved for bwd
size_t pc_workspace_bytes(int N, int P, int C, int Ca, int K, int dtype);
// where a gathered forward product leaves labels[index[n]] (labels_cached) for the loss behind it: the head of the
// materialised dropout(X) region, which only the generic route writes -- and a gathered call never takes that route
// (bf16: the region holds N P C 2 >= 8 N bytes)
int64_t* pc_gathered_labels(void* ws, int N, int P, int C, int Ca, int K, int dtype);
// (test-only probe) the carve of pc_plan: out[0..15] = R, Kp, off_wap, off_wtp, off_bap, off_z, off_dt, off_dz, off_pdbt,
// off_pdba, off_gemm, gemm_half, off_xd, off_bits, off_fused, total
void pc_plan_offsets(int N, int P, int C, int Ca, int K, int dtype, size_t* out);
int pc_bwd_act_psplit_host(int N, int kgroups, int P, int act);
// every weight image the shape can need, built in `ws`; maps (optional, APA_WIMG_MAX entries) / nmaps describe them
// (d: shape, dtype, workspace and stream; M = K, no flags)
int pc_weight_images(const PoolCall& d, const float* Wa, const float* ba, const float* Wt, const float* bt,
                     apa_weight_image* maps, int* nmaps);
int pc_forward(const PoolCall& d, const M1Fwd& io, M1Xent* xf = nullptr);
int pc_backward(const PoolCall& d, const M1Bwd& io, const M1Xent* xf = nullptr);

// apa_explain.hip: what apa_attn_explain decides before its launches (read by the test-only probe, apa_explain_probe.hip)
struct ExplainPlan {
  int S, nblk;                          // pixel splits per image, N * S blocks
  size_t off_w, off_k, off_b, total;    // workspace carve (byte offsets)
};
ExplainPlan explain_plan(int N, int P, int C, int K, int T);
// pixels a wave of explain_main_kernel<.., TT> takes at a time: PIX * TT dot products fit the 16 slots of one DPP row
template <int TT> struct ExplainGeom {
  static constexpr int PIX = TT <= 4 ? 4 : (TT == 5 ? 3 : 2);
  static constexpr int U = PIX == 2 ? 4 : 2;   // channel vectors per round: U * PIX (6 or 8) loads in flight per lane
};

}  // namespace apa
