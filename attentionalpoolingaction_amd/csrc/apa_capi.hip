// apa_capi.hip -- the extern "C" surface of libapa_hip.so (see include/apa.h): argument
// validation, dispatch between the factorised (M == 1) and dense (M == K) paths, error text.
#include <stdarg.h>
#include <stdio.h>

#include "../../include/apa_pose_cache.h"
#include "apa_capi.h"

namespace apa {

static thread_local char g_err[512] = "no error";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
  set_error("HIP error %d (%s) at %s", (int)e, hipGetErrorString(e), what);
  return APA_ERR_HIP;
}

__global__ void zero_words_kernel(uint32_t* __restrict__ p, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0u;
}

int zero_fill(void* p, size_t bytes, hipStream_t st) {
  if (!p || (bytes & 3) || (reinterpret_cast<uintptr_t>(p) & 3)) {
    set_error("zero_fill: %zu bytes at %p are not whole 4-byte words (internal)", bytes, p);
    return APA_ERR_INVALID_ARG;
  }
  const size_t n = bytes / 4;
  if (n == 0) return APA_OK;
  const size_t nb = (n + 255) / 256;
  hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, st,
                     static_cast<uint32_t*>(p), n);
  APA_LAUNCH_CHECK("zero_words_kernel");
  return APA_OK;
}

}  // namespace apa

using namespace apa;

extern "C" int apa_prof_event_create(void** event) {
  if (!event) { set_error("apa_prof_event_create: null"); return APA_ERR_INVALID_ARG; }
  // default flags: timing enabled; the events are stamped by hipExtLaunchKernel (dispatch begin / end)
  hipEvent_t e;
  APA_HIP_CHECK(hipEventCreate(&e));
  *event = e;
  return APA_OK;
}
extern "C" int apa_prof_event_destroy(void* event) {
  if (event) APA_HIP_CHECK(hipEventDestroy(static_cast<hipEvent_t>(event)));
  return APA_OK;
}
extern "C" int apa_prof_event_record(void* event, void* stream) {
  if (!event) { set_error("apa_prof_event_record: null"); return APA_ERR_INVALID_ARG; }
  APA_HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(event), static_cast<hipStream_t>(stream)));
  return APA_OK;
}
extern "C" int apa_prof_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!start || !stop || !ms) { set_error("apa_prof_event_elapsed_ms: null"); return APA_ERR_INVALID_ARG; }
  APA_HIP_CHECK(hipEventElapsedTime(ms, static_cast<hipEvent_t>(start), static_cast<hipEvent_t>(stop)));
  return APA_OK;
}
extern "C" int apa_version(void) { return APA_VERSION; }

extern "C" const char* apa_last_error(void) { return g_err; }

extern "C" const char* apa_status_string(int status) {
  switch (status) {
    case APA_OK: return "APA_OK";
    case APA_ERR_INVALID_ARG: return "APA_ERR_INVALID_ARG";
    case APA_ERR_UNSUPPORTED: return "APA_ERR_UNSUPPORTED";
    case APA_ERR_WORKSPACE: return "APA_ERR_WORKSPACE";
    case APA_ERR_HIP: return "APA_ERR_HIP";
    default: return "APA_ERR_UNKNOWN";
  }
}

// fp8_ok: the entry point serves an FP8 feature cache (PoolCall::fp8_ok); every other one answers "unknown dtype"
static int check_common(const char* fn, const PoolDims& d, bool fp8_ok = false) {
  if (d.N <= 0 || d.P <= 0 || d.C <= 0 || d.Ca <= 0 || d.K <= 0) {
    set_error("%s: non-positive dimension N=%d P=%d C=%d Ca=%d K=%d", fn, d.N, d.P, d.C, d.Ca, d.K);
    return APA_ERR_INVALID_ARG;
  }
  if (d.M != 1 && d.M != d.K) {
    set_error("%s: M must be 1 (class-agnostic) or K (per-class), got M=%d K=%d", fn, d.M, d.K);
    return APA_ERR_INVALID_ARG;
  }
  if (d.dtype != APA_DTYPE_F32 && d.dtype != APA_DTYPE_BF16 && !(fp8_ok && d.dtype == APA_DTYPE_FP8_E4M3)) {
    set_error("%s: unknown dtype %d", fn, d.dtype);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

// A form a frozen cache (an FP8 one, apa.h: APA_DTYPE_FP8_E4M3; one read by image index, apa_feature_cache) cannot
// have, by name, or null: the one chain behind fp8_check and cache_check, whose order decides what a call with several
// defects is told.  fp8: the FP8 kernels' channel limits apply.  (An FP8 call never gets to the _cat row: fp8_served.)
// per_class (the *_cached pooling calls and steps, not the epoch calls, never FP8): per-class maps of a shape on the fused
// K <= 64 route are a form a cache has -- the two kernels of that route that read X have gathered instances
// (apa_pc_fused.hip) -- and spatial-softmax attention goes with them: it is served by the same two X readers.
static bool cache_per_class(const PoolCall& d) {
  return d.M != 1 && pc_fused_shape_supported(d.C, d.Ca, d.K, d.dtype);
}
static const char* cache_form_why(const PoolCall& d, const void* X, const void* Xatt, bool topdown, bool fp8,
                                  bool per_class = false) {
  const bool pc = per_class && !fp8 && cache_per_class(d);
  return (d.M != 1 && !pc) ? "per-class maps (M != 1)"
         : (X && Xatt != X) ? "a separate attention input (Xatt != X)"
         : (fp8 && d.C % 16 != 0) ? "a channel count that is not a multiple of 16"
         : (fp8 && d.C > M1F_MAX_C) ? "more than 8192 channels"
         : ((d.flags & APA_FLAG_SOFTMAX_ATT) && !pc) ? "APA_FLAG_SOFTMAX_ATT"
         : (d.flags & APA_FLAG_RELU_INPUT) ? "APA_FLAG_RELU_INPUT"
         : (d.flags & APA_FLAG_RNG_EXTERNAL) ? "APA_FLAG_RNG_EXTERNAL"
         : topdown ? "the TopDownAttention dump"
         : d.cat ? "the concatenated pose channels (_cat)" : nullptr;
}

// What a call on an FP8 feature cache refuses, each reason by name and before anything is launched.  backward: a
// backward call or the backward half of a one-call step -- a cache has no gradient.
static int fp8_check(const char* fn, const PoolCall& d, const void* X, const void* Xatt, bool topdown, bool backward,
                     const void* dX) {
  if (d.dtype != APA_DTYPE_FP8_E4M3) return APA_OK;
  if (const char* why = cache_form_why(d, X, Xatt, topdown, true)) {
    set_error("%s: APA_DTYPE_FP8_E4M3 does not serve %s (M=%d C=%d): the FP8 cache feeds the fused class-agnostic head "
              "with identity or relu attention", fn, why, d.M, d.C);
    return APA_ERR_UNSUPPORTED;
  }
  if (backward && (!(d.flags & APA_FLAG_FROZEN_INPUT) || dX)) {
    set_error("%s: APA_DTYPE_FP8_E4M3 needs APA_FLAG_FROZEN_INPUT and a NULL dX: a feature cache has no gradient", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (reinterpret_cast<uintptr_t>(X) & 15) {
    set_error("%s: APA_DTYPE_FP8_E4M3 features must be 16-byte aligned", fn);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

extern "C" size_t apa_attn_pool_workspace_bytes(int N, int P, int C, int Ca, int K, int M, unsigned flags) {
  (void)flags;
  if (N <= 0 || P <= 0 || C <= 0 || Ca <= 0 || K <= 0) return 0;
  if (M == 1) return m1_plan(N, P, C, Ca, K).total;
  if (M == K) {  // dtype-dependent intermediates: report the larger of the two plans
    const size_t a = pc_workspace_bytes(N, P, C, Ca, K, APA_DTYPE_F32);
    const size_t b = pc_workspace_bytes(N, P, C, Ca, K, APA_DTYPE_BF16);
    return a > b ? a : b;
  }
  return 0;
}

// The call descriptor of an entry point.  The one place a caller's flags are masked: the library's internal bits, and
// APA_FLAG_WS_FROM_FWD, which only the one-call steps set, on their own backward half (no forward pass reads it).
// APA_FLAG_DXATT_RANK1 passes: the cfg 003 steps set it themselves on every backward half, and it too is a backward
// matter only (m1_call_fill), so a caller's bit on such a step changes nothing.
static PoolCall pool_call(const PoolDims& dims, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                          void* ws, size_t ws_bytes, void* stream, const apa_hooks* hooks = nullptr,
                          const apa_concat_feat* cat = nullptr) {
  return PoolCall{dims, flags & APA_PUBLIC_FLAGS & ~APA_FLAG_WS_FROM_FWD, keep_prob, seed, offset, ws, ws_bytes,
                  static_cast<hipStream_t>(stream), Hooks(hooks), cat};
}
// ... of an entry point that serves an FP8 feature cache: the plain pooling calls and the attention head's one-call steps
static PoolCall fp8_served(PoolCall d) {
  d.fp8_ok = d.cat == nullptr;
  return d;
}

// APA_FLAG_RNG_EXTERNAL: `seed` carries the address of the caller's keep bits
static int check_rng_flags(const char* fn, unsigned flags, uint64_t seed) {
  if (!(flags & APA_FLAG_RNG_EXTERNAL) || !(flags & APA_FLAG_TRAIN)) return APA_OK;
  if (flags & (APA_FLAG_RNG_DEVICE | APA_FLAG_RELU_INPUT)) {
    set_error("%s: APA_FLAG_RNG_EXTERNAL excludes APA_FLAG_RNG_DEVICE and APA_FLAG_RELU_INPUT", fn);
    return (flags & APA_FLAG_RNG_DEVICE) ? APA_ERR_INVALID_ARG : APA_ERR_UNSUPPORTED;
  }
  if (seed == 0) {
    set_error("%s: APA_FLAG_RNG_EXTERNAL with a null keep-bit image (seed == 0)", fn);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

static int check_cat(const char* fn, const PoolCall& d, bool topdown, bool backward) {
  const apa_concat_feat* c = d.cat;
  if (!c->Xext || !c->zext || (backward && !c->dXext)) {
    set_error("%s: apa_concat_feat needs Xext, zext%s", fn, backward ? " and dXext" : "");
    return APA_ERR_INVALID_ARG;
  }
  if (d.M != 1 || (d.flags & APA_FLAG_RELU_INPUT) || topdown || !m1_cat_supported(c->J)) {
    set_error("%s: the concatenated pose channels are built for M == 1, 1 <= J <= 64, without "
              "APA_FLAG_RELU_INPUT and without the TopDownAttention dump (J=%d M=%d)", fn, c->J, d.M);
    return APA_ERR_UNSUPPORTED;
  }
  return APA_OK;
}

// APA_FLAG_FROZEN_INPUT on per-class maps: only the fused K <= 64 route has an arm without the dX product.  Asked by
// the backward call and by the one-call steps BEFORE their forward half: nothing has been queued when it refuses.
static int frozen_input_check(const char* fn, const PoolDims& d, unsigned flags, const void* X, const void* Xatt) {
  if (!(flags & APA_FLAG_FROZEN_INPUT) || d.M == 1) return APA_OK;
  if (pc_fused_supported(d.N, d.P, d.C, d.Ca, d.K, d.dtype, X, Xatt) && !rng_external(flags)) return APA_OK;
  set_error("%s: APA_FLAG_FROZEN_INPUT is not served by the dense per-class route (K > 64, fp32 features, a separate "
            "attention input or a replayed mask; K=%d dtype=%d): run without the flag", fn, d.K, d.dtype);
  return APA_ERR_UNSUPPORTED;
}

// Every refusal of a pooling call above the paths' own (m1_call_fill), each written once.  f: the forward call's
// tensors, or b: the backward call's (the other null).
static int pool_check(const PoolCall& d, const M1Fwd* f, const M1Bwd* b) {
  const char* fn = b ? "apa_attn_pool_bwd" : "apa_attn_pool_fwd";
  const void* const X = b ? b->X : f->X;
  const void* const Xatt = b ? b->Xatt : f->Xatt;
  const bool topdown = f && f->topdown;
  int rc = check_common(fn, d, d.fp8_ok);
  if (rc != APA_OK) return rc;
  if (f ? !X || !Xatt || !f->Wa || !f->ba || !f->Wt || !f->bt || !f->logits || !f->att
        : !X || !Xatt || !b->Wa || !b->Wt || !b->bt || !b->att || !b->G ||
              (!b->dX && !(d.flags & APA_FLAG_FROZEN_INPUT)) || !b->dWa || !b->dba || !b->dWt || !b->dbt) {
    set_error("%s: null tensor pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((rc = fp8_check(fn, d, X, Xatt, topdown, b != nullptr, b ? b->dX : nullptr)) != APA_OK) return rc;
  if (f && Xatt == X && d.Ca != d.C) {
    set_error("%s: Xatt aliases X but Ca=%d != C=%d", fn, d.Ca, d.C);
    return APA_ERR_INVALID_ARG;
  }
  if (b && Xatt != X && !b->dXatt) {
    set_error("%s: Xatt is a separate tensor but dXatt is NULL", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((d.flags & APA_FLAG_TRAIN) && !(d.keep_prob > 0.f && d.keep_prob <= 1.f)) {
    set_error("%s: keep_prob=%g outside (0,1]", fn, (double)d.keep_prob);
    return APA_ERR_INVALID_ARG;
  }
  rc = check_rng_flags(fn, d.flags, d.seed);
  if (rc != APA_OK) return rc;
  if (d.cat && (rc = check_cat(fn, d, topdown, b != nullptr)) != APA_OK) return rc;
  if ((d.flags & APA_FLAG_RELU_INPUT) && (d.M != 1 || topdown)) {
    set_error("%s: APA_FLAG_RELU_INPUT is an M == 1 fast path without the TopDownAttention dump", fn);
    return APA_ERR_UNSUPPORTED;
  }
  if ((d.flags & APA_FLAG_FROZEN_INPUT) && topdown) {
    set_error("%s: APA_FLAG_FROZEN_INPUT together with the TopDownAttention dump is not served: run without the flag",
              fn);
    return APA_ERR_UNSUPPORTED;
  }
  if (b && (d.flags & APA_FLAG_FROZEN_INPUT) && d.cat) {
    set_error("%s: APA_FLAG_FROZEN_INPUT is not served by the *_cat entry points (concatenated pose channels): run "
              "without the flag", fn);
    return APA_ERR_UNSUPPORTED;
  }
  if (b && (rc = frozen_input_check(fn, d, d.flags, X, Xatt)) != APA_OK) return rc;
  if (b && (d.flags & APA_FLAG_DXATT_RANK1) && d.M != 1) {
    set_error("%s: APA_FLAG_DXATT_RANK1 needs one bottom-up map (M == 1): with per-class maps the gradient w.r.t. "
              "Xatt has rank K", fn);
    return APA_ERR_UNSUPPORTED;
  }
  // what the forward call saves for the backward call: M == 1 zsave and abar; M == K zsave, the fp32 [N,P,K] top-down map
  const float* const zsave = b ? b->zsave : f->zsave;
  const float* const abar = b ? b->abar : f->abar;
  if (!zsave || (d.M == 1 && !abar)) {
    set_error(d.M == 1 ? "%s: M==1 needs the zsave and abar buffers (backward: from the forward call)"
                       : "%s: M==K needs zsave = fp32 [N,P,K] buffer (the top-down map, saved by forward for backward)",
              fn);
    return APA_ERR_INVALID_ARG;
  }
  if (d.M == 1 && !m1_supported(d.C, d.Ca, d.dtype, Xatt == X)) {
    set_error("%s: M==1 needs C and Ca to be whole 16-byte vectors (multiples of 4 fp32 / 8 bf16 channels, "
              "C <= 9584); got C=%d Ca=%d dtype=%d", fn, d.C, d.Ca, d.dtype);
    return APA_ERR_UNSUPPORTED;
  }
  const size_t need = d.M == 1 ? m1_plan(d.N, d.P, d.C, d.Ca, d.K).total
                               : pc_workspace_bytes(d.N, d.P, d.C, d.Ca, d.K, d.dtype);
  if (!d.ws || d.ws_bytes < need) {
    set_error("%s: workspace too small (%zu < %zu)", fn, d.ws_bytes, need);
    return APA_ERR_WORKSPACE;
  }
  if (d.M != 1 && (d.flags & APA_FLAG_WEIGHT_IMAGES) && (reinterpret_cast<uintptr_t>(X) & 15)) {
    set_error("%s: APA_FLAG_WEIGHT_IMAGES needs 16-byte aligned features (the images are laid out for them)", fn);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

// end_points['TopDownAttention'] = dropout(X).Wt + bt  (nets_factory.py:296-309): the factorised
// path never needs it; it is materialised only on request (eval.py --ept dumps) by one GEMM.
static int topdown_product(const PoolCall& d, const M1Fwd& f) {
  GemmDesc g;
  g.A = f.X; g.lda = d.C; g.ta = dt_code(d.dtype); g.a_kc = true;
  g.B = f.Wt; g.ldb = d.K; g.tb = 0; g.b_kc = false;
  g.C = f.topdown; g.ldc = d.K; g.tc = g.ta;
  g.M = d.N * d.P; g.N = d.K; g.K = d.C; g.bias = f.bt;
  if ((d.flags & APA_FLAG_TRAIN) && d.keep_prob < 1.0f) {
    g.drop_a = 1;
    g.inv_keep = 1.0f / d.keep_prob;
    const RngKeyArgs k = rng_resolve(d.flags, d.keep_prob, d.seed, d.offset);
    g.thresh = k.thresh; g.seed = k.seed; g.offset = k.offset; g.offset_dev = k.offset_dev;
  }
  return gemm_launch(g, d.st);
}

// xf: the loss (or the evaluation outputs) a one-call step asks the forward pass to fold; `done` says whether it did
static int attn_pool_fwd(const PoolCall& d, const M1Fwd& f, M1Xent* xf) {
  int rc = pool_check(d, &f, nullptr);
  if (rc != APA_OK) return rc;
  if (d.M == 1) {
    M1Call c;
    rc = m1_call_fill(c, d, &f, nullptr);
    if (rc != APA_OK) return rc;
    rc = m1_forward(c, f, xf);
    return rc != APA_OK || !f.topdown ? rc : topdown_product(d, f);
  }
  // M == K: per-class maps, dense MFMA path
  if (d.hk.td_ready) APA_HIP_CHECK(hipStreamWaitEvent(d.st, d.hk.td_ready, 0));
  return pc_forward(d, f, f.topdown ? nullptr : xf);
}

// xf: what the forward half of the same step folded and this half has to finish
static int attn_pool_bwd(const PoolCall& d, const M1Bwd& b, const M1Xent* xf) {
  int rc = pool_check(d, nullptr, &b);
  if (rc != APA_OK) return rc;
  if (d.M == 1) {
    M1Call c;
    rc = m1_call_fill(c, d, nullptr, &b, xf);
    return rc != APA_OK ? rc : m1_backward(c, b, xf);
  }
  rc = pc_backward(d, b, xf);
  if (rc == APA_OK && d.hk.grad_ready) APA_HIP_CHECK(hipEventRecord(d.hk.grad_ready, d.st));
  return rc;
}

extern "C" int apa_attn_pool_fwd_cat(const apa_concat_feat* cat, const apa_hooks* hooks, const void* X,
                                     const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                     const float* bt, float* logits, float* att, float* zsave, float* abar,
                                     void* topdown, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                                     int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                                     void* stream) {
  return attn_pool_fwd(fp8_served(pool_call({N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, ws, ws_bytes,
                                            stream, hooks, cat)),
                       M1Fwd{X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown}, nullptr);
}

extern "C" int apa_attn_pool_fwd_ex(const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                                    const float* ba, const float* Wt, const float* bt, float* logits, float* att,
                                    float* zsave, float* abar, void* topdown, void* ws, size_t ws_bytes, int N, int P,
                                    int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                                    uint64_t offset, int dtype, void* stream) {
  return apa_attn_pool_fwd_cat(nullptr, hooks, X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown, ws, ws_bytes,
                               N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

extern "C" int apa_attn_pool_fwd(const void* X, const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                 const float* bt, float* logits, float* att, float* zsave, float* abar, void* topdown,
                                 void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags,
                                 float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  return apa_attn_pool_fwd_cat(nullptr, nullptr, X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown, ws,
                               ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

// (a caller cannot vouch for a workspace's history: pool_call clears APA_FLAG_WS_FROM_FWD)
extern "C" int apa_attn_pool_bwd_cat(const apa_concat_feat* cat, const apa_hooks* hooks, const void* X,
                                     const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                     const float* bt, const float* att, const float* zsave, const float* abar,
                                     const float* G, void* dX, void* dXatt, float* dWa, float* dba, float* dWt,
                                     float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                     unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                                     void* stream) {
  (void)ba;
  return attn_pool_bwd(fp8_served(pool_call({N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, ws, ws_bytes,
                                            stream, hooks, cat)),
                       M1Bwd{X, Xatt, Wa, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt, dbt}, nullptr);
}

extern "C" int apa_attn_pool_bwd_ex(const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                                    const float* ba, const float* Wt, const float* bt, const float* att,
                                    const float* zsave, const float* abar, const float* G, void* dX, void* dXatt,
                                    float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N,
                                    int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                                    uint64_t offset, int dtype, void* stream) {
  return apa_attn_pool_bwd_cat(nullptr, hooks, X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt,
                               dbt, ws, ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

extern "C" int apa_attn_pool_bwd(const void* X, const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                 const float* bt, const float* att, const float* zsave, const float* abar,
                                 const float* G, void* dX, void* dXatt, float* dWa, float* dba, float* dWt, float* dbt,
                                 void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags,
                                 float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  return apa_attn_pool_bwd_cat(nullptr, nullptr, X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba,
                               dWt, dbt, ws, ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype,
                               stream);
}

// ---- rank > 1 with one bottom-up map (apa.h: apa_rank_maps; apa_m1_rank.hip) ----------------------------------------
// Every refusal of a rank call, nothing launched: the rank's own first (in the order apa.h lists them), then what
// the rank-1 call refuses about the same arguments.  rk: rank 0 from the flat list, then the descriptor's entries.
static int rank_check(const char* fn, const apa_rank_maps* rank, const PoolCall& d, const M1Fwd* f, const M1Bwd* b,
                      RankCall* rk) {
  if (!rank) {
    set_error("%s: null apa_rank_maps", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (rank->extra < 1 || rank->extra > APA_RANK_MAX - 1) {
    set_error("%s: apa_rank_maps.extra=%d outside 1..%d (rank 2..%d)", fn, rank->extra, APA_RANK_MAX - 1, APA_RANK_MAX);
    return APA_ERR_INVALID_ARG;
  }
  int rc = check_common(fn, d);
  if (rc != APA_OK) return rc;
  if (d.M != 1) {
    set_error("%s: rank > 1 is built for one bottom-up map (M == 1), got M=%d", fn, d.M);
    return APA_ERR_UNSUPPORTED;
  }
  if (d.flags & (APA_FLAG_SOFTMAX_ATT | APA_FLAG_RELU_INPUT | APA_FLAG_FROZEN_INPUT)) {
    set_error("%s: rank > 1 does not take %s", fn,
              (d.flags & APA_FLAG_SOFTMAX_ATT) ? "APA_FLAG_SOFTMAX_ATT (softmax attention with rank > 1 is not a valid "
                                                 "reference configuration)"
              : (d.flags & APA_FLAG_RELU_INPUT) ? "APA_FLAG_RELU_INPUT" : "APA_FLAG_FROZEN_INPUT");
    return APA_ERR_UNSUPPORTED;
  }
  rk->R = rank->extra + 1;
  rk->Wt[0] = f ? f->Wt : b->Wt; rk->bt[0] = f ? f->bt : b->bt;
  rk->dWt[0] = b ? b->dWt : nullptr; rk->dbt[0] = b ? b->dbt : nullptr;
  rk->z0 = rank->z0; rk->ws = d.ws;
  for (int r = 0; r < rank->extra; ++r) {
    if (!rank->chain_w[r] || !rank->chain_b[r] || !rank->Wt[r] || !rank->bt[r] ||
        (b && (!rank->dchain_w[r] || !rank->dchain_b[r] || !rank->dWt[r] || !rank->dbt[r]))) {
      set_error("%s: null pointer in entry %d of apa_rank_maps (extra=%d)", fn, r, rank->extra);
      return APA_ERR_INVALID_ARG;
    }
    rk->cw[r] = rank->chain_w[r]; rk->cb[r] = rank->chain_b[r];
    rk->Wt[r + 1] = rank->Wt[r]; rk->bt[r + 1] = rank->bt[r];
    rk->dcw[r] = b ? rank->dchain_w[r] : nullptr; rk->dcb[r] = b ? rank->dchain_b[r] : nullptr;
    rk->dWt[r + 1] = b ? rank->dWt[r] : nullptr; rk->dbt[r + 1] = b ? rank->dbt[r] : nullptr;
  }
  if (!rank->z0) {
    set_error("%s: apa_rank_maps.z0 is NULL (the [N,P] map the forward call saves for the backward call)", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((rc = pool_check(d, f, b)) != APA_OK) return rc;
  const void* const X = b ? b->X : f->X;
  const void* const Xatt = b ? b->Xatt : f->Xatt;
  if (!m1r_supported(d.C, d.Ca, d.dtype, Xatt == X)) {
    set_error("%s: rank > 1 needs C a whole number of 16-byte vectors up to 2048 channels; got C=%d Ca=%d dtype=%d", fn,
              d.C, d.Ca, d.dtype);
    return APA_ERR_UNSUPPORTED;
  }
  const size_t need = m1r_workspace_bytes(d.N, d.P, d.C, d.Ca, d.K, rk->R);
  if (d.ws_bytes < need) {
    set_error("%s: workspace too small (%zu < %zu = apa_attn_pool_rank_workspace_bytes)", fn, d.ws_bytes, need);
    return APA_ERR_WORKSPACE;
  }
  return APA_OK;
}

extern "C" size_t apa_attn_pool_rank_workspace_bytes(int N, int P, int C, int Ca, int K, int extra) {
  if (N <= 0 || P <= 0 || C <= 0 || Ca <= 0 || K <= 0 || extra < 1 || extra > APA_RANK_MAX - 1) return 0;
  return m1r_workspace_bytes(N, P, C, Ca, K, extra + 1);
}

static int rank_fwd_run(const PoolCall& d, const RankCall& rk, const M1Fwd& f) {
  M1Call c;
  const int rc = m1_call_fill(c, d, &f, nullptr);
  m1_call_full_rows(c, false);   // m1r_pool_fwd_kernel: its own rows, never the paired form
  return rc != APA_OK ? rc : m1r_forward(c, rk, f);
}
static int rank_bwd_run(const PoolCall& d, const RankCall& rk, const M1Bwd& b) {
  M1Call c;
  const int rc = m1_call_fill(c, d, nullptr, &b);
  m1_call_full_rows(c, true);
  return rc != APA_OK ? rc : m1r_backward(c, rk, b);
}

extern "C" int apa_attn_pool_rank_fwd(const apa_rank_maps* rank, const void* X, const void* Xatt, const float* Wa,
                                      const float* ba, const float* Wt, const float* bt, float* logits, float* att,
                                      float* zsave, float* abar, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                                      int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                      int dtype, void* stream) {
  const PoolCall d = pool_call({N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, ws, ws_bytes, stream);
  const M1Fwd f{X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar};
  RankCall rk = {};
  const int rc = rank_check("apa_attn_pool_rank_fwd", rank, d, &f, nullptr, &rk);
  return rc != APA_OK ? rc : rank_fwd_run(d, rk, f);
}

extern "C" int apa_attn_pool_rank_bwd(const apa_rank_maps* rank, const void* X, const void* Xatt, const float* Wa,
                                      const float* ba, const float* Wt, const float* bt, const float* att,
                                      const float* zsave, const float* abar, const float* G, void* dX, void* dXatt,
                                      float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N,
                                      int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob,
                                      uint64_t seed, uint64_t offset, int dtype, void* stream) {
  (void)ba;
  const PoolCall d = pool_call({N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, ws, ws_bytes, stream);
  const M1Bwd b{X, Xatt, Wa, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt, dbt};
  RankCall rk = {};
  const int rc = rank_check("apa_attn_pool_rank_bwd", rank, d, nullptr, &b, &rk);
  return rc != APA_OK ? rc : rank_bwd_run(d, rk, b);
}

// forward, softmax cross-entropy, backward: the three entry points' own launches in one host call, so bit-identical
// to them; both halves are checked before the first launch
extern "C" int apa_attn_head_train_step_rank(const apa_rank_maps* rank, const void* X, const void* Xatt,
                                             const float* Wa, const float* ba, const float* Wt, const float* bt,
                                             const int64_t* labels, float loss_wt, float grad_scale, float* logits,
                                             float* att, float* zsave, float* abar, float* loss, float* G, void* dX,
                                             void* dXatt, float* dWa, float* dba, float* dWt, float* dbt, void* ws,
                                             size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags,
                                             float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  const char* fn = "apa_attn_head_train_step_rank";
  const PoolCall d = pool_call({N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, ws, ws_bytes, stream);
  const M1Fwd f{X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar};
  const M1Bwd b{X, Xatt, Wa, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt, dbt};
  RankCall rkf = {}, rkb = {};
  int rc = rank_check(fn, rank, d, &f, nullptr, &rkf);
  if (rc != APA_OK) return rc;
  if (!labels || !loss || !G) {
    set_error("%s: null labels / loss / G pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((rc = rank_check(fn, rank, d, nullptr, &b, &rkb)) != APA_OK) return rc;
  if ((rc = rank_fwd_run(d, rkf, f)) != APA_OK) return rc;
  rc = apa_softmax_xent_fwd_bwd(logits, labels, loss, G, nullptr, nullptr, N, K, loss_wt, grad_scale, stream);
  return rc != APA_OK ? rc : rank_bwd_run(d, rkb, b);
}

// ---- a resident feature cache read by image index (apa.h: apa_feature_cache) -----------------------------------------
// What a *_cached call refuses about its descriptor and about the forms a cache cannot have, each reason by name and
// before anything is queued; what remains (pointers, workspace, the FP8 arm's own limits) is pool_check's as ever.
// backward: a backward call or a training step.  per_class: false for the epoch calls, which keep refusing M != 1 (their
// update rewrites no weight images, which the per-class deploy path relies on) while the step they loop over serves it.
static int cache_check(const char* fn, const apa_feature_cache* fc, const PoolCall& d, const void* X, const void* Xatt,
                       bool topdown, bool backward, const void* dX, bool per_class = true) {
  if (!fc || !fc->index) {
    set_error("%s: null apa_feature_cache / index pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (reinterpret_cast<uintptr_t>(fc->index) & 3) {
    set_error("%s: apa_feature_cache.index must be 4-byte aligned", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (fc->cache_images < 1) {
    set_error("%s: apa_feature_cache.cache_images=%d: a cache holds at least one image", fn, fc->cache_images);
    return APA_ERR_INVALID_ARG;
  }
  const int rc = check_common(fn, d, true);
  if (rc != APA_OK) return rc;
  if (dX) {
    set_error("%s: a feature cache has no gradient: dX must be NULL", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (backward && !(d.flags & APA_FLAG_FROZEN_INPUT)) {
    set_error("%s: a feature cache is frozen: a backward call or a training step needs APA_FLAG_FROZEN_INPUT", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (const char* why = cache_form_why(d, X, Xatt, topdown, false, per_class)) {   // (FP8's own limits: pool_check)
    if (per_class && cache_per_class(d))
      set_error("%s: a feature cache does not serve %s: with per-class maps the gathered kernels feed the fused bf16 "
                "route (K <= 64) with attention from the map itself", fn, why);
    else
      set_error("%s: a feature cache does not serve %s: the gathered kernels feed the fused class-agnostic head with "
                "identity or relu attention", fn, why);
    return APA_ERR_UNSUPPORTED;
  }
  if (d.M != 1 && (reinterpret_cast<uintptr_t>(X) & 15)) {
    set_error("%s: a feature cache of per-class maps must be 16-byte aligned (the fused route fetches its rows by "
              "LDS-DMA)", fn);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

// labels_cached: `labels` is [T]; the loss reads the [N] copy the forward pooling pass leaves in the workspace
static const int64_t* cached_labels(PoolCall* d, const apa_feature_cache* fc, const int64_t* labels) {
  if (!fc->labels_cached || !labels || !d->ws) return labels;
  d->fc_labels = labels;
  if (d->M != 1) return pc_gathered_labels(d->ws, d->N, d->P, d->C, d->Ca, d->K, d->dtype);
  return m1_gathered_labels(d->ws, m1_plan(d->N, d->P, d->C, d->Ca, d->K));
}

// labels_cached reads a per-FRAME table through the index; a clip's or a sigmoid row's labels are per clip / per row
static int cached_clip_labels_check(const char* fn, const apa_feature_cache* fc, bool ml, bool clip) {
  if (!fc->labels_cached || (!ml && !clip)) return APA_OK;
  set_error("%s: apa_feature_cache.labels_cached = 1 is not served together with %s: such labels are per clip or per "
            "row and come from the sampler (apa_sample_clip_frames), not through the frame index", fn,
            ml ? "an apa_multilabel" : "an apa_clip_pool");
  return APA_ERR_INVALID_ARG;
}

// ---- the one-call training steps ------------------------------------------------------------------------------------
// The loss of a step.  ml: a sigmoid action loss on ml->labels (checked by check_multilabel; `labels` unused), null:
// the softmax cross-entropy on the integer `labels`.  clips: the loss is taken on the rows pooled over each clip's frames
// (apa.h: apa_clip_pool; `clip` is checked by clip_step_check), loss is [1 + N / frames] then.
struct StepLoss {
  const apa_multilabel* ml = nullptr;
  const int64_t* labels = nullptr;
  bool clips = false;
  const apa_clip_pool* clip = nullptr;
  float wt = 1.f, grad_scale = 1.f;
  float* loss = nullptr;   // [1 + rows]
  float* G = nullptr;      // [N,K]: the gradient at the (frame) logits
};

// a valid apa_multilabel, or the refusal (nothing has touched the GPU); apa_internal.h: the stand-alone losses call it too
int apa::check_multilabel(const char* fn, const apa_multilabel* ml) {
  if (!ml || !ml->labels) {
    set_error("%s: null apa_multilabel / labels pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (ml->kind != APA_ACTION_LOSS_MULTI_LABEL && ml->kind != APA_ACTION_LOSS_MULTI_LABEL_2) {
    set_error("%s: unknown loss kind %d", fn, ml->kind);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

// the pooling workspace, then the clip loss's scratch
static size_t clip_step_pool_bytes(int N, int P, int C, int Ca, int K, int M, unsigned flags) {
  return align_up(apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags), 256);
}

extern "C" size_t apa_clip_step_workspace_bytes(int N, int frames, int P, int C, int Ca, int K, int M, unsigned flags) {
  if (N <= 0 || frames <= 0 || N % frames != 0) return 0;
  const size_t pool = apa_attn_pool_workspace_bytes(N, P, C, Ca, K, M, flags);
  return pool ? clip_step_pool_bytes(N, P, C, Ca, K, M, flags) + apa_clip_xent_workspace_bytes(N / frames, frames, K)
              : 0;
}

// everything the clip loss would refuse, BEFORE the forward half is launched; *pool_bytes: where its scratch begins
static int clip_step_check(const char* fn, const PoolCall& d, const StepLoss& L, const float* logits,
                           size_t* pool_bytes) {
  const apa_clip_pool* clip = L.clip;
  if (!clip || !(L.ml ? static_cast<const void*>(L.ml->labels) : L.labels) || !L.loss || !logits || !L.G) {
    set_error("%s: null clip / labels / loss / logits / G pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  const int rc = check_common(fn, d, d.fp8_ok);
  if (rc != APA_OK) return rc;
  if (clip->frames <= 0 || d.N % clip->frames != 0) {
    set_error("%s: N=%d is not a whole number of clips of %d frames", fn, d.N, clip->frames);
    return APA_ERR_INVALID_ARG;
  }
  if (!clip->pooled || (clip->w && (!clip->b || !clip->tatt || !clip->dw || !clip->db))) {
    set_error("%s: apa_clip_pool needs pooled, and with w also b, tatt, dw and db", fn);
    return APA_ERR_INVALID_ARG;
  }
  *pool_bytes = clip_step_pool_bytes(d.N, d.P, d.C, d.Ca, d.K, d.M, d.flags);
  const size_t need = *pool_bytes + apa_clip_xent_workspace_bytes(d.N / clip->frames, clip->frames, d.K);
  if (!d.ws || d.ws_bytes < need) {
    set_error("%s: workspace too small (%zu < %zu = apa_clip_step_workspace_bytes)", fn, d.ws_bytes, need);
    return APA_ERR_WORKSPACE;
  }
  return APA_OK;
}

// The loss as its neighbours can fold it inside one call (M1Xent; bit-identical results, same reduction trees), or
// false where no fold applies.  The softmax cross-entropy: the logits reduction also does the row's loss and the
// backward head kernel the batch mean (M == 1, K <= 512), the per-class maps take it in their activation passes.  A
// sigmoid loss: M == 1 with the fold's shapes, the logits reducer does the rows' loss (m1_logits_ml_kernel); the
// per-class pc_row_xent folds read integer labels and are not entered.  On clips the loss is taken on the pooled rows:
// both halves run as the per-op entry points do and G travels through memory.
static bool step_xent(const StepLoss& L, const PoolDims& d, M1Xent* xf) {
  if (L.clips || (L.ml && d.M != 1)) return false;
  xf->labels = L.ml ? nullptr : L.labels; xf->loss = L.loss; xf->G = L.G;
  if (L.ml) {
    xf->kind = L.ml->kind; xf->mlabels = L.ml->labels; xf->pos_weight = L.ml->pos_weight;
    if (d.N > 0 && d.K > 0) ml_scales(L.ml->kind, L.wt, L.grad_scale, d.N, d.K, &xf->lscale, &xf->gscale);
  } else if (d.N > 0) {
    xf->lscale = L.wt / (float)d.N;
    xf->gscale = L.wt * L.grad_scale / (float)d.N;
  }
  return true;
}

// the stand-alone loss on the finished logits; clips: its scratch lies pool_bytes into the workspace
static int step_loss_run(const StepLoss& L, const PoolCall& d, const float* logits, size_t pool_bytes) {
  if (PcTrace* t = pc_trace()) if (d.M != 1) t->xent = PC_XENT_OWN;
  if (L.clips) {
    const apa_clip_pool& c = *L.clip;
    const int B = d.N / c.frames;
    void* const lws = static_cast<char*>(d.ws) + pool_bytes;
    const size_t lws_bytes = apa_clip_xent_workspace_bytes(B, c.frames, d.K);
    return L.ml ? apa_clip_multilabel_fwd_bwd(L.ml, logits, c.w, c.b, c.pooled, c.tatt, L.loss, L.G, c.dw, c.db, lws,
                                              lws_bytes, B, c.frames, d.K, L.wt, L.grad_scale, d.st)
                : apa_clip_xent_fwd_bwd(logits, L.labels, c.w, c.b, c.pooled, c.tatt, L.loss, L.G, c.dw, c.db, lws,
                                        lws_bytes, B, c.frames, d.K, L.wt, L.grad_scale, d.st);
  }
  return L.ml ? ml_loss_rows(L.ml->kind, L.ml->labels, L.ml->pos_weight, logits, L.loss, L.G, d.N, d.K, L.wt,
                             L.grad_scale, d.st)
              : apa_softmax_xent_fwd_bwd(logits, L.labels, L.loss, L.G, nullptr, nullptr, d.N, d.K, L.wt, L.grad_scale,
                                         d.st);
}

// What a step refuses about its loss, before anything is launched.  *pool_bytes: the part of the workspace that is the
// pooling call's -- all of it, or on clips what lies in front of the clip loss's scratch.
static int head_step_check(const char* fn, const PoolCall& d, const StepLoss& L, const float* logits,
                           size_t* pool_bytes) {
  *pool_bytes = d.ws_bytes;
  if (L.clips) return clip_step_check(fn, d, L, logits, pool_bytes);
  if ((!L.ml && !L.labels) || !L.loss || !L.G) {
    set_error("%s: null labels / loss / G pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

// The step every one-call entry point runs on the attention head, head_step_check passed: forward (with the loss folded
// where step_xent says so), the stand-alone loss unless the forward half took it, backward on the same workspace with
// nothing in between -- APA_FLAG_WS_FROM_FWD: it may reuse what the forward half prepared there -- and with the M1Xent
// exactly when there is something left to finish.  Bit-identical to the three separate calls.
// fwd_iflags / bwd_iflags: flag bits of one half only (the fast route of apa_pose_attn_train_step).
static int head_step_run(PoolCall d, const StepLoss& L, const M1Fwd& f, const M1Bwd& b, size_t pool_bytes,
                         unsigned fwd_iflags = 0, unsigned bwd_iflags = 0) {
  d.ws_bytes = pool_bytes;
  const unsigned flags = d.flags;
  int rc = APA_OK;
  // what the backward half refuses about an FP8 cache (a training step on one is a frozen step), before the forward half
  if (d.fp8_ok && d.dtype == APA_DTYPE_FP8_E4M3 && f.X && f.Xatt) {
    if ((rc = check_common("apa_attn_head_train_step", d, true)) != APA_OK) return rc;
    if ((rc = fp8_check("apa_attn_head_train_step", d, f.X, f.Xatt, false, true, b.dX)) != APA_OK) return rc;
  }
  if ((flags & APA_FLAG_FROZEN_INPUT) && f.X && f.Xatt) {   // the backward half's refusal of the flag, before the forward half
    if ((rc = check_common("apa_attn_head_train_step", d, d.fp8_ok)) != APA_OK) return rc;
    if ((rc = frozen_input_check("apa_attn_head_train_step", d, flags, f.X, f.Xatt)) != APA_OK) return rc;
  }
  M1Xent xf;
  const bool fold = step_xent(L, d, &xf);
  d.flags = flags | fwd_iflags;
  rc = attn_pool_fwd(d, f, fold ? &xf : nullptr);
  if (rc != APA_OK) return rc;
  if (!xf.done && (rc = step_loss_run(L, d, f.logits, pool_bytes)) != APA_OK) return rc;
  d.flags = flags | APA_FLAG_WS_FROM_FWD | bwd_iflags;
  return attn_pool_bwd(d, b, xf.done && !xf.finished ? &xf : nullptr);
}

// The request (apa_capi.h: HeadTrainStep) as the calls the step is made of
struct HeadTrainCall { PoolCall d; StepLoss L; M1Fwd f; M1Bwd b; size_t pool_bytes = 0; };

// Everything a step refuses above the two pooling halves' own checks, in ONE order for every entry point, in fn's name
// and with nothing launched:
//   1. the cache: its descriptor and the forms it cannot have (cache_check; per_class: its argument);
//   2. the sigmoid loss (check_multilabel);
//   3. a cache's labels_cached beside labels that are per clip or per row (cached_clip_labels_check);
//   4. the loss's pointers -- on clips with the clip itself, the shape and the workspace (head_step_check).
// A part the request does not take is skipped.  (cached_labels: the identity unless labels_cached, which 3. leaves to
// the flat softmax step alone.)
static int head_train_call(const char* fn, const HeadTrainStep& r, bool per_class, HeadTrainCall* c) {
  c->d = fp8_served(pool_call(r.dims, r.flags, r.keep_prob, r.seed, r.offset, r.ws, r.ws_bytes, r.stream, r.hooks));
  c->f = M1Fwd{r.X, r.Xatt, r.Wa, r.ba, r.Wt, r.bt, r.logits, r.att, r.zsave, r.abar};
  c->b = M1Bwd{r.X, r.Xatt, r.Wa, r.Wt, r.bt, r.att, r.zsave, r.abar, r.G, r.dX, r.dXatt, r.dWa, r.dba, r.dWt, r.dbt};
  int rc = APA_OK;
  if (r.cached && (rc = cache_check(fn, r.cache, c->d, r.X, r.Xatt, false, true, r.dX, per_class)) != APA_OK) return rc;
  if (r.sigmoid && (rc = check_multilabel(fn, r.ml)) != APA_OK) return rc;
  const int64_t* labels = r.sigmoid ? nullptr : r.labels;
  if (r.cached) {
    if ((rc = cached_clip_labels_check(fn, r.cache, r.sigmoid, r.clips)) != APA_OK) return rc;
    c->d.fc = r.cache;
    labels = cached_labels(&c->d, r.cache, labels);
  }
  c->L = StepLoss{r.sigmoid ? r.ml : nullptr, labels, r.clips, r.clip, r.loss_wt, r.grad_scale, r.loss, r.G};
  return head_step_check(fn, c->d, c->L, r.logits, &c->pool_bytes);
}

int apa::head_train_step(const char* fn, const HeadTrainStep& r) {
  HeadTrainCall c;
  const int rc = head_train_call(fn, r, true, &c);
  return rc != APA_OK ? rc : head_step_run(c.d, c.L, c.f, c.b, c.pool_bytes);
}

// the pooling call's refusals and the M == 1 paths' own (m1_call_fill) for one half; nothing is launched
static int pool_half_check(const PoolCall& d, const M1Fwd* f, const M1Bwd* b) {
  const int rc = pool_check(d, f, b);
  if (rc != APA_OK) return rc;
  M1Call c;
  return m1_call_fill(c, d, f, b);
}

// (per-class maps on a cache: refused here although the step serves them -- an epoch's update rewrites no weight images)
int apa::head_train_check(const char* fn, const HeadTrainStep& r) {
  HeadTrainCall c;
  int rc = head_train_call(fn, r, false, &c);
  if (rc != APA_OK) return rc;
  c.d.ws_bytes = c.pool_bytes;
  if ((rc = pool_half_check(c.d, &c.f, nullptr)) != APA_OK) return rc;
  c.d.flags |= APA_FLAG_WS_FROM_FWD;
  return pool_half_check(c.d, nullptr, &c.b);
}

// The six entry points: pack the request (the flat list in its order, then the parts the entry point takes), one call.
extern "C" int apa_attn_head_train_step_ex(const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                                           const float* ba, const float* Wt, const float* bt, const int64_t* labels,
                                           float loss_wt, float grad_scale, float* logits, float* att, float* zsave,
                                           float* abar, float* loss, float* G, void* dX, void* dXatt, float* dWa,
                                           float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P,
                                           int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                                           uint64_t offset, int dtype, void* stream) {
  return head_train_step("apa_attn_head_train_step",
                         {X, Xatt, Wa, ba, Wt, bt, labels, loss_wt, grad_scale, logits, att, zsave, abar, loss, G, dX,
                          dXatt, dWa, dba, dWt, dbt, ws, ws_bytes, {N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed,
                          offset, stream, hooks});
}

extern "C" int apa_attn_head_train_step(const void* X, const void* Xatt, const float* Wa, const float* ba,
                                        const float* Wt, const float* bt, const int64_t* labels, float loss_wt,
                                        float grad_scale, float* logits, float* att, float* zsave, float* abar,
                                        float* loss, float* G, void* dX, void* dXatt, float* dWa, float* dba,
                                        float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                                        int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                        int dtype, void* stream) {
  return apa_attn_head_train_step_ex(nullptr, X, Xatt, Wa, ba, Wt, bt, labels, loss_wt, grad_scale, logits,
                                     att, zsave, abar, loss, G, dX, dXatt, dWa, dba, dWt, dbt, ws, ws_bytes,
                                     N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

extern "C" int apa_attn_head_train_step_clips(const apa_clip_pool* clip, const apa_hooks* hooks, const void* X,
                                              const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                              const float* bt, const int64_t* labels, float loss_wt, float grad_scale,
                                              float* logits, float* att, float* zsave, float* abar, float* loss,
                                              float* G, void* dX, void* dXatt, float* dWa, float* dba, float* dWt,
                                              float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                                              int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                              int dtype, void* stream) {
  HeadTrainStep r{X, Xatt, Wa, ba, Wt, bt, labels, loss_wt, grad_scale, logits, att, zsave, abar, loss, G, dX, dXatt, dWa,
                  dba, dWt, dbt, ws, ws_bytes, {N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, stream, hooks};
  r.clip = clip; r.clips = true;   // (a null clip is clip_step_check's to report)
  return head_train_step("apa_attn_head_train_step_clips", r);
}

// clip == NULL: the flat step, apa_attn_head_train_step_ex with the loss exchanged
extern "C" int apa_attn_head_train_step_multilabel(const apa_multilabel* ml, const apa_clip_pool* clip,
                                                   const apa_hooks* hooks, const void* X, const void* Xatt,
                                                   const float* Wa, const float* ba, const float* Wt, const float* bt,
                                                   float loss_wt, float grad_scale, float* logits, float* att,
                                                   float* zsave, float* abar, float* loss, float* G, void* dX,
                                                   void* dXatt, float* dWa, float* dba, float* dWt, float* dbt,
                                                   void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                                   unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                                   int dtype, void* stream) {
  HeadTrainStep r{X, Xatt, Wa, ba, Wt, bt, nullptr, loss_wt, grad_scale, logits, att, zsave, abar, loss, G, dX, dXatt, dWa,
                  dba, dWt, dbt, ws, ws_bytes, {N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, stream, hooks};
  r.ml = ml; r.sigmoid = true;   // (a null ml is check_multilabel's to report)
  r.clip = clip; r.clips = clip != nullptr;
  return head_train_step("apa_attn_head_train_step_multilabel", r);
}

extern "C" int apa_attn_head_train_step_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const void* X,
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
  return head_train_step("apa_attn_head_train_step_cached", r);
}

// clips and the sigmoid losses from a frame cache; ml == NULL && clip == NULL: apa_attn_head_train_step_cached itself,
// by name too
extern "C" int apa_attn_head_train_step_cached_clips(const apa_feature_cache* cache, const apa_multilabel* ml,
                                                     const apa_clip_pool* clip, const apa_hooks* hooks, const void* X,
                                                     const void* Xatt, const float* Wa, const float* ba,
                                                     const float* Wt, const float* bt, const int64_t* labels,
                                                     float loss_wt, float grad_scale, float* logits, float* att,
                                                     float* zsave, float* abar, float* loss, float* G, void* dX,
                                                     void* dXatt, float* dWa, float* dba, float* dWt, float* dbt,
                                                     void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                                                     int M, unsigned flags, float keep_prob, uint64_t seed,
                                                     uint64_t offset, int dtype, void* stream) {
  HeadTrainStep r{X, Xatt, Wa, ba, Wt, bt, labels, loss_wt, grad_scale, logits, att, zsave, abar, loss, G, dX, dXatt, dWa,
                  dba, dWt, dbt, ws, ws_bytes, {N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, stream, hooks};
  r.cache = cache; r.cached = true;
  r.ml = ml; r.sigmoid = ml != nullptr;
  r.clip = clip; r.clips = clip != nullptr;
  return head_train_step(ml || clip ? "apa_attn_head_train_step_cached_clips" : "apa_attn_head_train_step_cached", r);
}

// ---- the one-call steps of the pose-regularised head (cfg 003) ------------------------------------------------------
// d: the pooling call of the step (Ca = Cp, M = 1, io's pooling workspace); L: its action loss.
//
// The composed route is the four calls a caller without these entry points runs, and the clip and the sigmoid forms
// promise the bits of those separate calls (apa.h), so they take it for EVERY shape.  The launches the fast bf16 route
// shares between neighbouring ops (attention logits out of the Pl product's epilogue, dWa / dba on the pose head's
// backward rows pass, the pooling pass's dX share in the dX product's epilogue) sum in other orders than the per-op
// kernels -- att moves by 2.5e-7, logits 4.4e-7, dWa 9.4e-7, dX by a bf16 ulp; the bf16 operand copies in io (W1_bf16,
// W2T_bf16) are not read there.  A sigmoid loss still rides in the logits reducer inside head_step.
// fc (apa_pose_cache.h: the cached step, pose_cache_check passed): io->X is a T-image cache.  The launches that read X
// -- the Ppre product, both pooling passes, the dW1 product -- follow the index; everything else has the batch shape
static int pose_attn_step(const char* fn, const apa_pose_attn_step_io* io, PoolCall d, StepLoss L, int J,
                          const apa_feature_cache* fc = nullptr) {
  if (!io) {
    set_error("%s: null io", fn);
    return APA_ERR_INVALID_ARG;
  }
  const apa_pose_attn_step_io& s = *io;
  if (!s.X || !s.W1 || !s.b1 || !s.W2 || !s.b2 || !s.Wa || !s.ba || !s.Wt || !s.bt || (!L.ml && !s.labels) ||
      !s.pose_labels || !s.pose_valid || !s.Ppre || !s.Pl || !s.att || !s.logits || !s.zsave || !s.abar ||
      !s.loss_action || !s.loss_pose || !s.G || !s.dPl || !s.dZ || (!s.dX && !(d.flags & APA_FLAG_FROZEN_INPUT)) || !s.dW1 || !s.db1 || !s.dW2 || !s.db2 ||
      !s.dWa || !s.dba || !s.dWt || !s.dbt || !s.ws_pool || !s.ws_pose) {
    set_error("%s: null pointer in apa_pose_attn_step_io (only W1_bf16 / W2T_bf16 -- and dX under "
              "APA_FLAG_FROZEN_INPUT -- may be NULL)", fn);
    return APA_ERR_INVALID_ARG;
  }
  // (on clips the shape is checked with the clip itself, in head_step_check below: a null clip is reported first)
  int rc = L.clips ? APA_OK : check_common(fn, d);
  if (rc != APA_OK) return rc;
  if (J <= 0) {
    set_error("%s: J=%d", fn, J);
    return APA_ERR_INVALID_ARG;
  }
  if (d.flags & (APA_FLAG_RELU_INPUT | APA_FLAG_RNG_EXTERNAL)) {
    set_error("%s: APA_FLAG_RELU_INPUT / APA_FLAG_RNG_EXTERNAL are served by the per-op entry points (the attention "
              "input of cfg 003 is pose_pre_logits; a replayed mask takes the generic kernels)", fn);
    return APA_ERR_UNSUPPORTED;
  }
  const int N = d.N, P = d.P, C = d.C, Cp = d.Ca, K = d.K, dtype = d.dtype;
  d.ws = s.ws_pool; d.ws_bytes = s.ws_pool_bytes;
  L.labels = s.labels; L.wt = s.action_wt; L.grad_scale = s.grad_scale; L.loss = s.loss_action; L.G = s.G;
  if (fc) {   // (labels_cached: the [N] copy lives where the class-agnostic cached step keeps it)
    d.fc = fc; d.fc_pose = true;
    L.labels = cached_labels(&d, fc, s.labels);
  }
  size_t pool_bytes = 0;   // everything the loss would refuse, the clip's defects among it, before the first launch
  if ((rc = head_step_check(fn, d, L, s.logits, &pool_bytes)) != APA_OK) return rc;
  const M1Fwd f{s.X, s.Ppre, s.Wa, s.ba, s.Wt, s.bt, s.logits, s.att, s.zsave, s.abar};
  const M1Bwd b{s.X, s.Ppre, s.Wa, s.Wt, s.bt, s.att, s.zsave, s.abar, s.G, s.dX, s.dZ, s.dWa, s.dba, s.dWt, s.dbt};
  const bool train = (d.flags & APA_FLAG_TRAIN) && d.keep_prob < 1.0f;
  // APA_FLAG_FROZEN_INPUT: the pooling pass takes its arm without the dX stores (the flag rides in d.flags) and the
  // pose head's dX product is not launched -- the pooling share its epilogue carries on the fast route goes with it
  const bool frozen = (d.flags & APA_FLAG_FROZEN_INPUT) != 0;
  // the pose head's call on its own workspace, and its two halves: the external gradient of the backward half is
  // rank-1, dZ (x) Wa, added to the dX the pooling pass wrote, on the workspace the forward half prepared
  PoseCall pc = pose_call(fn, N, P, C, Cp, J, dtype, s.ws_pose, s.ws_pose_bytes, d.st);
  pc.ws_name = "pose workspace";
  if (fc) pc.rmap = GemmRowMap{fc->index, fc->cache_images, P};
  const PoseFwd pf = {s.X, s.W1, s.b1, s.W2, s.b2, s.Ppre, s.Pl};
  const PoseBwd pb = {s.X, s.W1, s.W2, s.Ppre, s.dPl, nullptr, s.dZ, s.Wa, s.dX, s.dW1, s.db1, s.dW2, s.db2, true, true,
                      frozen};
  const bool fast = !L.clips && !L.ml && pose_step_fast_ok(pc, pf, pb) && m1_supported(C, Cp, dtype, false) &&
                    m1_small_route_ok(C, K, s.G, s.Wt, s.zsave);
  if (!fast) {
    // (apa_pose_head_fwd and, below, apa_pose_head_bwd_rank1ext, as calls that carry the step's row map)
    PoseCall pcf = pose_call("apa_pose_head_fwd", N, P, C, Cp, J, dtype, s.ws_pose, s.ws_pose_bytes, d.st);
    pcf.rmap = pc.rmap;
    rc = pose_head_fwd_run(pcf, pf);
    if (rc != APA_OK) return rc;
    rc = apa_pose_l2_loss_fwd_bwd(s.Pl, s.pose_labels, s.pose_valid, s.loss_pose, s.dPl, pose_ws_loss_scratch(pc),
                                  apa_pose_l2_workspace_bytes(N, P, J), N, P, J, s.pose_wt, s.grad_scale, d.st);
    if (rc != APA_OK) return rc;
    d.flags |= APA_FLAG_DXATT_RANK1;   // s.dZ receives dZ itself; apa_pose_head_bwd_rank1ext re-forms dXatt from it
    rc = head_step_run(d, L, f, b, pool_bytes);
    if (rc != APA_OK) return rc;
    PoseCall pcb = pose_call("apa_pose_head_bwd", N, P, C, Cp, J, dtype, s.ws_pose, s.ws_pose_bytes, d.st);
    pcb.rmap = pc.rmap;
    return pose_head_bwd_run(pcb, pb);   // accumulate, workspace from the forward call, no dX on frozen features
  }
  PoseStepArgs a;
  // a caller-kept bf16 copy of W1 is an OPTIMISATION: apa_momentum_sgd_step_shadow accepts any 4-byte aligned
  // shadow (e.g. one carved out of a flat bf16 buffer), the DMA-staged products want 16-byte addressable rows -- an
  // operand they cannot read is ignored and W1 is converted inside the call, as if none had been given
  a.W1_bf16 = (reinterpret_cast<uintptr_t>(s.W1_bf16) & 15) == 0 ? s.W1_bf16 : nullptr;
  a.W2T_bf16 = (reinterpret_cast<uintptr_t>(s.W2T_bf16) & 15) == 0 ? s.W2T_bf16 : nullptr;
  a.wa = s.Wa; a.ba = s.ba; a.att = s.att;
  a.relu_att = (d.flags & APA_FLAG_RELU_ATT) && !(d.flags & APA_FLAG_SOFTMAX_ATT);
  a.pose_labels = s.pose_labels; a.pose_valid = s.pose_valid; a.dPl = s.dPl;
  a.pose_wt = s.pose_wt; a.grad_scale = s.grad_scale;
  rc = pose_fwd_fused(pc, pf, a);
  if (rc != APA_OK) return rc;
  // The pooling pass's own dX share (A/P . dz . mask/keep) is not written and read back: the streaming backward
  // kernel becomes read-only (APA_IFLAG_NO_DX) and the pose head's dX product adds the term in its epilogue from att,
  // dz and the forward half's keep bits -- one 25.7 MB write and one 25.7 MB read less at the benchmark shape.
  const int wide_rows = gemm_bf16_wide_tile_rows(N * P, C, Cp);   // (its rank-1 epilogue wants <= 3 images per tile)
  // ... and only if the dX product is certain to take the wide bf16 kernel (the one with the rank-1 epilogue): all-bf16
  // operands with 16-byte addressable rows -- dPpre and the W1 operand are the workspace's (aligned) or the shadow
  // checked above, dX is the caller's
  const bool nodx = !frozen && m1_no_dx_supported(C, dtype, train) && wide_rows > 0 && wide_rows <= 2 * P &&
                    (reinterpret_cast<uintptr_t>(s.dX) & 15) == 0 && C % 8 == 0 && Cp % 8 == 0 &&
                    dtype == APA_DTYPE_BF16;
  // the pose head's Pl kernel left the attention in place; its backward rows pass takes dWa / dba and the RNG bump
  rc = head_step_run(d, L, f, b, pool_bytes, APA_IFLAG_ATT_READY,
                     APA_FLAG_DXATT_RANK1 | APA_IFLAG_NO_ATT_WGRAD | (nodx ? APA_IFLAG_NO_DX : 0u));
  if (rc != APA_OK) return rc;
  if (nodx) {
    const M1Plan mp = m1_plan(N, P, C, Cp, K);
    char* wp = static_cast<char*>(s.ws_pool);
    a.pool_att = s.att;
    a.pool_dz = reinterpret_cast<const float*>(wp + mp.off_dz);
    a.pool_bits = reinterpret_cast<const uint8_t*>(wp + mp.off_maskbits);
    a.pool_inv_keep = 1.0f / d.keep_prob;
  }
  a.dWa = s.dWa; a.dba = s.dba; a.loss_pose = s.loss_pose;
  a.rng_bump = (train && (d.flags & APA_FLAG_RNG_DEVICE))
                   ? reinterpret_cast<uint64_t*>(static_cast<uintptr_t>(d.offset)) : nullptr;
  // (same workspace, same call: the bf16 copy of W1 the forward half built there -- when the caller keeps none -- is reused)
  return pose_bwd_fused(pc, pb, a);
}

extern "C" int apa_pose_attn_train_step(const apa_pose_attn_step_io* io, int N, int P, int C, int Cp, int J, int K,
                                        unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                                        void* stream) {
  return pose_attn_step("apa_pose_attn_train_step", io,
                        pool_call({N, P, C, Cp, K, 1, dtype}, flags, keep_prob, seed, offset, nullptr, 0, stream),
                        StepLoss{}, J);
}

extern "C" int apa_pose_attn_train_step_clips(const apa_clip_pool* clip, const apa_pose_attn_step_io* io, int N, int P,
                                              int C, int Cp, int J, int K, unsigned flags, float keep_prob,
                                              uint64_t seed, uint64_t offset, int dtype, void* stream) {
  return pose_attn_step("apa_pose_attn_train_step_clips", io,
                        pool_call({N, P, C, Cp, K, 1, dtype}, flags, keep_prob, seed, offset, nullptr, 0, stream),
                        StepLoss{nullptr, nullptr, true, clip}, J);
}

extern "C" int apa_pose_attn_train_step_multilabel(const apa_multilabel* ml, const apa_clip_pool* clip,
                                                   const apa_pose_attn_step_io* io, int N, int P, int C, int Cp, int J,
                                                   int K, unsigned flags, float keep_prob, uint64_t seed,
                                                   uint64_t offset, int dtype, void* stream) {
  const int rc = check_multilabel("apa_pose_attn_train_step_multilabel", ml);
  if (rc != APA_OK) return rc;
  return pose_attn_step("apa_pose_attn_train_step_multilabel", io,
                        pool_call({N, P, C, Cp, K, 1, dtype}, flags, keep_prob, seed, offset, nullptr, 0, stream),
                        StepLoss{ml, nullptr, clip != nullptr, clip}, J);
}

extern "C" int apa_per_class_weight_images(const float* Wa, const float* ba, const float* Wt, const float* bt, void* ws,
                                           size_t ws_bytes, int N, int P, int C, int Ca, int K, int dtype,
                                           apa_weight_image* maps, int* nmaps, void* stream) {
  if (nmaps) *nmaps = 0;
  if (!Wa || !ba || !Wt || !bt) {
    set_error("apa_per_class_weight_images: null parameter pointer");
    return APA_ERR_INVALID_ARG;
  }
  const PoolCall d = pool_call({N, P, C, Ca, K, K, dtype}, 0u, 1.0f, 0, 0, ws, ws_bytes, stream);
  const int rc = check_common("apa_per_class_weight_images", d);
  if (rc != APA_OK) return rc;
  const size_t need = pc_workspace_bytes(N, P, C, Ca, K, dtype);
  if (!ws || ws_bytes < need) {
    set_error("apa_per_class_weight_images: workspace too small (%zu < %zu)", ws_bytes, need);
    return APA_ERR_WORKSPACE;
  }
  return pc_weight_images(d, Wa, ba, Wt, bt, maps, nmaps);
}

// the scratch of the label-free evaluation form at the head of the pooling workspace: labels [N] (0 everywhere), then
// the loss slots [1+N]
static size_t eval_scratch_bytes(int N) { return align_up((size_t)N * 8 + (size_t)(1 + N) * 4, 256); }

// d.flags: the caller's, plus internal bits (APA_IFLAG_ATT_READY from apa_pose_attn_eval_step)
static int attn_head_eval(PoolCall d, const M1Fwd& f, const int64_t* labels, float* loss, float* probs,
                          int64_t* pred) {
  if (!probs || !pred) {
    set_error("apa_attn_head_eval_step: null probs / pred pointer");
    return APA_ERR_INVALID_ARG;
  }
  if ((labels == nullptr) != (loss == nullptr)) {
    set_error("apa_attn_head_eval_step: labels and loss must be given together");
    return APA_ERR_INVALID_ARG;
  }
  d.flags &= ~(unsigned)APA_FLAG_TRAIN;   // is_training=False: no dropout
  // without ground truth the softmax / argmax of a row rides on the logits reduction (M == 1, K <= 512)
  M1Xent xf;
  xf.probs = probs; xf.pred = pred;
  int rc = attn_pool_fwd(d, f, (d.M == 1 && !labels) ? &xf : nullptr);
  if (rc != APA_OK || xf.done) return rc;
  if (PcTrace* t = pc_trace()) if (d.M != 1) t->xent = PC_XENT_OWN;
  if (labels)
    return apa_softmax_xent_fwd_bwd(f.logits, labels, loss, nullptr, probs, pred, d.N, d.K, 1.0f, 1.0f, d.st);
  // no ground truth: the loss slots are scratch at the head of the workspace (label 0 everywhere)
  if (d.ws_bytes < eval_scratch_bytes(d.N)) {
    set_error("apa_attn_head_eval_step: workspace too small for the label-free form");
    return APA_ERR_WORKSPACE;
  }
  rc = zero_fill(d.ws, (size_t)d.N * 8, d.st);
  if (rc != APA_OK) return rc;
  float* lscratch = reinterpret_cast<float*>(static_cast<char*>(d.ws) + (size_t)d.N * 8);
  return apa_softmax_xent_fwd_bwd(f.logits, static_cast<const int64_t*>(d.ws), lscratch, nullptr, probs, pred, d.N,
                                  d.K, 1.0f, 1.0f, d.st);
}

// What the *_eval_step_clips entry points refuse about their clip and their scores, before anything is launched.
static int eval_scores_check(const char* fn, const apa_clip_pool* clip, int kind, int N, int K, const float* logits,
                             const int64_t* labels, const float* loss, const float* probs, const int64_t* pred) {
  if (kind != APA_SCORES_SOFTMAX && kind != APA_SCORES_SIGMOID) {
    set_error("%s: unknown scores kind %d", fn, kind);
    return APA_ERR_INVALID_ARG;
  }
  if (!logits || !probs || !pred) {
    set_error("%s: null logits / probs / pred pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((labels == nullptr) != (loss == nullptr)) {
    set_error("%s: labels and loss must be given together", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (kind == APA_SCORES_SIGMOID && labels) {
    set_error("%s: the sigmoid scores take no labels / loss (eval.py computes none)", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (N <= 0 || K <= 0) {
    set_error("%s: non-positive size N=%d K=%d", fn, N, K);
    return APA_ERR_INVALID_ARG;
  }
  if (!clip) return APA_OK;
  if (clip->frames <= 0 || N % clip->frames != 0) {
    set_error("%s: N=%d is not a whole number of clips of %d frames", fn, N, clip->frames);
    return APA_ERR_INVALID_ARG;
  }
  if (!clip->pooled || (clip->w && (!clip->b || !clip->tatt))) {
    set_error("%s: apa_clip_pool needs pooled, and with w also b and tatt", fn);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

// The tail of both *_eval_step_clips entry points, eval_scores_check passed: the flat softmax form is attn_head_eval
// itself; every other form runs the forward half without a folded or trailing softmax, then the one scores launch.
static int attn_head_eval_clips(const char* fn, const apa_clip_pool* clip, int kind, PoolCall d, const M1Fwd& f,
                                const int64_t* labels, float* loss, float* probs, int64_t* pred) {
  if (!clip && kind == APA_SCORES_SOFTMAX) return attn_head_eval(d, f, labels, loss, probs, pred);
  d.flags &= ~(unsigned)APA_FLAG_TRAIN;   // is_training=False: no dropout
  const int rc = attn_pool_fwd(d, f, nullptr);
  if (rc != APA_OK) return rc;
  if (PcTrace* t = pc_trace()) if (d.M != 1) t->xent = PC_XENT_OWN;
  const int F = clip ? clip->frames : 1;
  return clip_scores_launch(fn, kind, f.logits, clip ? clip->w : nullptr, clip ? clip->b : nullptr, labels,
                            clip ? clip->pooled : nullptr, clip ? clip->tatt : nullptr, probs, pred, loss, d.N / F, F,
                            d.K, d.st);
}

// The request (apa_capi.h: HeadEvalStep) as the call the step is made of
struct HeadEvalCall { PoolCall d; M1Fwd f; const int64_t* labels = nullptr; };

// Everything an evaluation step refuses above the pooling call's own checks, in ONE order, in fn's name, nothing
// launched:
//   1. the cache (cache_check; per_class: its argument), a clip handed to a cached step that takes none, labels_cached
//      beside a clip (cached_clip_labels_check);
//   2. the scores, and the clip with them (eval_scores_check).
// The plain step (no cache, no clip pool taken) has none of these: attn_head_eval words its own refusals.
static int head_eval_call(const char* fn, const HeadEvalStep& r, bool per_class, HeadEvalCall* c) {
  c->d = fp8_served(pool_call(r.dims, r.flags, 1.0f, 0, 0, r.ws, r.ws_bytes, r.stream));
  c->f = M1Fwd{r.X, r.Xatt, r.Wa, r.ba, r.Wt, r.bt, r.logits, r.att, r.zsave, r.abar};
  c->labels = r.labels;
  if (!r.cached && !r.clips) return APA_OK;
  int rc = APA_OK;
  if (r.cached) {
    if ((rc = cache_check(fn, r.cache, c->d, r.X, r.Xatt, false, false, nullptr, per_class)) != APA_OK) return rc;
    if (r.clip && !r.clips) {
      set_error("%s: a feature cache does not serve clips: flat batches only (clip must be NULL)", fn);
      return APA_ERR_UNSUPPORTED;
    }
    if ((rc = cached_clip_labels_check(fn, r.cache, false, r.clips)) != APA_OK) return rc;
  }
  rc = eval_scores_check(fn, r.clip, r.scores_kind, r.dims.N, r.dims.K, r.logits, r.labels, r.loss, r.probs, r.pred);
  if (rc != APA_OK || !r.cached) return rc;
  c->d.fc = r.cache;
  c->labels = cached_labels(&c->d, r.cache, r.labels);
  return APA_OK;
}

// (the plain step: scores_kind is the softmax and there is no clip, so attn_head_eval_clips IS attn_head_eval)
int apa::head_eval_step(const char* fn, const HeadEvalStep& r) {
  HeadEvalCall c;
  const int rc = head_eval_call(fn, r, true, &c);
  return rc != APA_OK ? rc
                      : attn_head_eval_clips(fn, r.clip, r.scores_kind, c.d, c.f, c.labels, r.loss, r.probs, r.pred);
}

// (per-class maps on a cache: refused with the training epoch's, so that the pair stays one interface)
int apa::head_eval_check(const char* fn, const HeadEvalStep& r) {
  HeadEvalCall c;
  const int rc = head_eval_call(fn, r, false, &c);
  if (rc != APA_OK) return rc;
  c.d.flags &= ~(unsigned)APA_FLAG_TRAIN;
  return pool_half_check(c.d, &c.f, nullptr);
}

extern "C" int apa_attn_head_eval_step_clips(const apa_clip_pool* clip, int scores_kind, const void* X,
                                             const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                             const float* bt, const int64_t* labels, float* logits, float* att,
                                             float* zsave, float* abar, float* loss, float* probs, int64_t* pred,
                                             void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                             unsigned flags, int dtype, void* stream) {
  HeadEvalStep r{X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws, ws_bytes,
                 {N, P, C, Ca, K, M, dtype}, flags, stream, scores_kind};
  r.clip = clip; r.clips = true;
  return head_eval_step("apa_attn_head_eval_step_clips", r);
}

extern "C" int apa_attn_head_eval_step(const void* X, const void* Xatt, const float* Wa, const float* ba,
                                       const float* Wt, const float* bt, const int64_t* labels, float* logits,
                                       float* att, float* zsave, float* abar, float* loss, float* probs, int64_t* pred,
                                       void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                       unsigned flags, int dtype, void* stream) {
  return head_eval_step("apa_attn_head_eval_step",
                        {X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws, ws_bytes,
                         {N, P, C, Ca, K, M, dtype}, flags, stream});
}

// flat batches, softmax or sigmoid scores: everything behind the pooling pass never sees X.  `clip` is there to be
// refused by name.
extern "C" int apa_attn_head_eval_step_cached(const apa_feature_cache* cache, const apa_clip_pool* clip,
                                              int scores_kind, const void* X, const void* Xatt, const float* Wa,
                                              const float* ba, const float* Wt, const float* bt, const int64_t* labels,
                                              float* logits, float* att, float* zsave, float* abar, float* loss,
                                              float* probs, int64_t* pred, void* ws, size_t ws_bytes, int N, int P,
                                              int C, int Ca, int K, int M, unsigned flags, int dtype, void* stream) {
  HeadEvalStep r{X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws, ws_bytes,
                 {N, P, C, Ca, K, M, dtype}, flags, stream, scores_kind};
  r.cache = cache; r.cached = true;
  r.clip = clip;
  return head_eval_step("apa_attn_head_eval_step_cached", r);
}

// clips from a frame cache; clip == NULL: apa_attn_head_eval_step_cached itself, by name too
extern "C" int apa_attn_head_eval_step_cached_clips(const apa_feature_cache* cache, const apa_clip_pool* clip,
                                                    int scores_kind, const void* X, const void* Xatt, const float* Wa,
                                                    const float* ba, const float* Wt, const float* bt,
                                                    const int64_t* labels, float* logits, float* att, float* zsave,
                                                    float* abar, float* loss, float* probs, int64_t* pred, void* ws,
                                                    size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                                    unsigned flags, int dtype, void* stream) {
  HeadEvalStep r{X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws, ws_bytes,
                 {N, P, C, Ca, K, M, dtype}, flags, stream, scores_kind};
  r.cache = cache; r.cached = true;
  r.clip = clip; r.clips = clip != nullptr;
  return head_eval_step(clip ? "apa_attn_head_eval_step_cached_clips" : "apa_attn_head_eval_step_cached", r);
}

// ---- the pooling calls on a resident feature cache (apa.h: apa_feature_cache; cache_check above) ---------------------
extern "C" int apa_attn_pool_fwd_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const void* X,
                                        const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                        const float* bt, float* logits, float* att, float* zsave, float* abar,
                                        void* topdown, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                                        int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                        int dtype, void* stream) {
  PoolCall d = fp8_served(pool_call({N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, ws, ws_bytes, stream,
                                    hooks));
  const int rc = cache_check("apa_attn_pool_fwd_cached", cache, d, X, Xatt, topdown != nullptr, false, nullptr);
  if (rc != APA_OK) return rc;
  d.fc = cache;
  return attn_pool_fwd(d, M1Fwd{X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown}, nullptr);
}

extern "C" int apa_attn_pool_bwd_cached(const apa_feature_cache* cache, const apa_hooks* hooks, const void* X,
                                        const void* Xatt, const float* Wa, const float* ba, const float* Wt,
                                        const float* bt, const float* att, const float* zsave, const float* abar,
                                        const float* G, void* dX, void* dXatt, float* dWa, float* dba, float* dWt,
                                        float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                                        unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                                        void* stream) {
  (void)ba;
  PoolCall d = fp8_served(pool_call({N, P, C, Ca, K, M, dtype}, flags, keep_prob, seed, offset, ws, ws_bytes, stream,
                                    hooks));
  const int rc = cache_check("apa_attn_pool_bwd_cached", cache, d, X, Xatt, false, true, dX);
  if (rc != APA_OK) return rc;
  d.fc = cache;
  return attn_pool_bwd(d, M1Bwd{X, Xatt, Wa, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt, dbt}, nullptr);
}

// workspace of apa_pose_attn_eval_step: [pose head | pooling (+ the label-free loss scratch) | column-tile partials]
struct PoseEvalCarve { size_t pose, pool, zpart, total; };
static PoseEvalCarve pose_eval_carve(int N, int P, int C, int Cp, int J, int K, unsigned flags, int dtype) {
  PoseEvalCarve c;
  c.pose = align_up(apa_pose_head_workspace_bytes(N, P, C, Cp, J, dtype), 256);
  const size_t lf = eval_scratch_bytes(N);
  const size_t pool = apa_attn_pool_workspace_bytes(N, P, C, Cp, K, 1, flags);
  c.pool = align_up(pool > lf ? pool : lf, 256);
  c.zpart = pose_eval_zpart_bytes(N, P, Cp);
  c.total = c.pose + c.pool + c.zpart;
  return c;
}

extern "C" size_t apa_pose_attn_eval_workspace_bytes(int N, int P, int C, int Cp, int J, int K, unsigned flags,
                                                     int dtype, int want_pose_logits) {
  (void)want_pose_logits;   // both routes fit: the composed route's Ppre lives in the pose head's own dPpre region
  if (N <= 0 || P <= 0 || C <= 0 || Cp <= 0 || J <= 0 || K <= 0) return 0;
  return pose_eval_carve(N, P, C, Cp, J, K, flags, dtype).total;
}

// clips_fn == nullptr: apa_pose_attn_eval_step; else the _clips entry point of that name with its clip and scores kind
// fc (apa_pose_cache.h: the cached step, flat batches; cached_fn its name): as in pose_attn_step
static int pose_attn_eval(const char* clips_fn, const apa_clip_pool* clip, int kind, const apa_pose_attn_eval_io* io,
                          int N, int P, int C, int Cp, int J, int K, unsigned flags, int dtype, void* stream,
                          const apa_feature_cache* fc = nullptr, const char* cached_fn = nullptr) {
  const char* fn = cached_fn ? cached_fn : clips_fn ? clips_fn : "apa_pose_attn_eval_step";
  if (!io) {
    set_error("%s: null io", fn);
    return APA_ERR_INVALID_ARG;
  }
  const apa_pose_attn_eval_io& s = *io;
  if (!s.X || !s.W1 || !s.b1 || !s.W2 || !s.b2 || !s.Wa || !s.ba || !s.Wt || !s.bt || !s.att || !s.logits ||
      !s.zsave || !s.abar || !s.probs || !s.pred) {
    set_error("%s: null pointer in apa_pose_attn_eval_io (only W1_bf16, labels, loss, Pl and route may be NULL)",
              fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((s.labels == nullptr) != (s.loss == nullptr)) {
    set_error("%s: labels and loss must be given together (both null or neither)", fn);
    return APA_ERR_INVALID_ARG;
  }
  int rc = check_common(fn, {N, P, C, Cp, K, 1, dtype});
  if (rc != APA_OK) return rc;
  if (clips_fn && (rc = eval_scores_check(fn, clip, kind, N, K, s.logits, s.labels, s.loss, s.probs, s.pred)) != APA_OK)
    return rc;
  if (J <= 0) {
    set_error("%s: J=%d", fn, J);
    return APA_ERR_INVALID_ARG;
  }
  if (flags & (APA_FLAG_RELU_INPUT | APA_FLAG_RNG_EXTERNAL)) {
    set_error("%s: APA_FLAG_RELU_INPUT / APA_FLAG_RNG_EXTERNAL have no meaning here (the attention input is "
              "pose_pre_logits; evaluation draws no mask)", fn);
    return APA_ERR_UNSUPPORTED;
  }
  flags &= APA_FLAG_SOFTMAX_ATT | APA_FLAG_RELU_ATT;   // is_training=False: everything else is a training matter
  if (!m1_supported(C, Cp, dtype, false)) {
    set_error("%s: C and Cp must be whole 16-byte vectors (multiples of 4 fp32 / 8 bf16 channels, C <= 9584); got "
              "C=%d Cp=%d dtype=%d", fn, C, Cp, dtype);
    return APA_ERR_UNSUPPORTED;
  }
  const PoseEvalCarve cv = pose_eval_carve(N, P, C, Cp, J, K, flags, dtype);
  if (!s.ws || s.ws_bytes < cv.total) {
    set_error("%s: workspace too small (%zu < %zu)", fn, s.ws_bytes, cv.total);
    return APA_ERR_WORKSPACE;
  }
  char* w = static_cast<char*>(s.ws);
  float* zpart = reinterpret_cast<float*>(w + cv.pose + cv.pool);
  const bool relu_att = (flags & APA_FLAG_RELU_ATT) && !(flags & APA_FLAG_SOFTMAX_ATT);
  PoseCall pc = pose_call(fn, N, P, C, Cp, J, dtype, w, cv.pose, stream);
  pc.ws_name = "pose workspace";
  if (fc) pc.rmap = GemmRowMap{fc->index, fc->cache_images, P};
  PoseStepArgs a;
  a.W1_bf16 = s.W1_bf16; a.wa = s.Wa; a.ba = s.ba; a.att = s.att; a.relu_att = relu_att;
  PoseEvalOut o = {0, nullptr, false};
  rc = pose_eval_fwd(pc, PoseFwd{s.X, s.W1, s.b1, s.W2, s.b2, nullptr, s.Pl}, a, zpart, &o);
  if (rc != APA_OK) return rc;
  if (s.route) *s.route = o.route;
  // with att in place the pooling pass never dereferences its attention input (it only must differ from X)
  const void* xatt = o.ppre ? o.ppre : static_cast<const void*>(zpart);
  PoolCall d = pool_call({N, P, C, Cp, K, 1, dtype}, flags, 1.0f, 0, 0, w + cv.pose, cv.pool, stream);
  if (o.att_ready) d.flags |= APA_IFLAG_ATT_READY;
  const int64_t* labels = s.labels;
  if (fc) {
    d.fc = fc; d.fc_pose = true;
    labels = cached_labels(&d, fc, s.labels);
  }
  const M1Fwd f{s.X, xatt, s.Wa, s.ba, s.Wt, s.bt, s.logits, s.att, s.zsave, s.abar};
  return clips_fn ? attn_head_eval_clips(fn, clip, kind, d, f, labels, s.loss, s.probs, s.pred)
                  : attn_head_eval(d, f, labels, s.loss, s.probs, s.pred);
}

extern "C" int apa_pose_attn_eval_step(const apa_pose_attn_eval_io* io, int N, int P, int C, int Cp, int J, int K,
                                       unsigned flags, int dtype, void* stream) {
  return pose_attn_eval(nullptr, nullptr, APA_SCORES_SOFTMAX, io, N, P, C, Cp, J, K, flags, dtype, stream);
}

extern "C" int apa_pose_attn_eval_step_clips(const apa_clip_pool* clip, int scores_kind,
                                             const apa_pose_attn_eval_io* io, int N, int P, int C, int Cp, int J, int K,
                                             unsigned flags, int dtype, void* stream) {
  return pose_attn_eval("apa_pose_attn_eval_step_clips", clip, scores_kind, io, N, P, C, Cp, J, K, flags, dtype,
                        stream);
}

// ---- the cfg 003 steps from a resident feature cache (apa_pose_cache.h) ------------------------------------------------
// What the two cached steps refuse about their descriptor, the cache and the forms it cannot have, each by name and
// before anything is queued, in the order the header promises; what remains is the plain step's.  The admission of the
// two products that read X through the row map is gemm_rowmap_check's (pose_rowmap_check describes them).
static int pose_cache_check(const char* fn, const apa_feature_cache* fc, const void* X, const void* dX, bool train,
                            unsigned flags, int N, int P, int C, int Cp, int J, int dtype, const float* W1,
                            const void* W1_bf16, void* ws_pose, size_t ws_pose_bytes, void* stream) {
  if (!fc || !fc->index) {
    set_error("%s: null apa_feature_cache / index pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (reinterpret_cast<uintptr_t>(fc->index) & 3) {
    set_error("%s: apa_feature_cache.index must be 4-byte aligned", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (fc->cache_images < 1) {
    set_error("%s: apa_feature_cache.cache_images=%d: a cache holds at least one image", fn, fc->cache_images);
    return APA_ERR_INVALID_ARG;
  }
  if (dX) {
    set_error("%s: a feature cache has no gradient: io->dX must be NULL", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (train && !(flags & APA_FLAG_FROZEN_INPUT)) {
    set_error("%s: a feature cache is frozen: a training step needs APA_FLAG_FROZEN_INPUT", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (dtype != APA_DTYPE_BF16) {
    set_error("%s: dtype %d: the pose-regularised head is served from a bf16 cache (fp32 and FP8 caches: gather a "
              "batch and run the plain step)", fn, dtype);
    return APA_ERR_UNSUPPORTED;
  }
  if ((reinterpret_cast<uintptr_t>(X) & 15) || C % 8 != 0) {
    set_error("%s: the cache must be 16-byte aligned with C a multiple of 8 (C=%d): its rows are fetched by 16-byte "
              "vectors and LDS-DMA", fn, C);
    return APA_ERR_UNSUPPORTED;
  }
  if (N > 0 && P > 0 && C > 0 && Cp > 0 && J > 0) {
    PoseCall pc = pose_call(fn, N, P, C, Cp, J, dtype, ws_pose, ws_pose_bytes, stream);
    pc.rmap = GemmRowMap{fc->index, fc->cache_images, P};
    const int rc = pose_rowmap_check(pc, X, W1, W1_bf16, train);
    if (rc != APA_OK) return rc;
  }
  if (flags & APA_FLAG_SOFTMAX_ATT) {
    set_error("%s: a feature cache does not serve APA_FLAG_SOFTMAX_ATT: the gathered pooling passes have no softmax "
              "instance (the backward pass forms dZ under the softmax)", fn);
    return APA_ERR_UNSUPPORTED;
  }
  return APA_OK;
}

extern "C" int apa_pose_attn_train_step_cached(const apa_feature_cache* cache, const apa_pose_attn_step_io* io, int N,
                                               int P, int C, int Cp, int J, int K, unsigned flags, float keep_prob,
                                               uint64_t seed, uint64_t offset, int dtype, void* stream) {
  const char* fn = "apa_pose_attn_train_step_cached";
  if (!io) {
    set_error("%s: null io", fn);
    return APA_ERR_INVALID_ARG;
  }
  const int rc = pose_cache_check(fn, cache, io->X, io->dX, true, flags, N, P, C, Cp, J, dtype, io->W1, io->W1_bf16,
                                  io->ws_pose, io->ws_pose_bytes, stream);
  if (rc != APA_OK) return rc;
  return pose_attn_step(fn, io, pool_call({N, P, C, Cp, K, 1, dtype}, flags, keep_prob, seed, offset, nullptr, 0, stream),
                        StepLoss{}, J, cache);
}

extern "C" int apa_pose_attn_eval_step_cached(const apa_feature_cache* cache, const apa_pose_attn_eval_io* io, int N,
                                              int P, int C, int Cp, int J, int K, unsigned flags, int dtype,
                                              void* stream) {
  const char* fn = "apa_pose_attn_eval_step_cached";
  if (!io) {
    set_error("%s: null io", fn);
    return APA_ERR_INVALID_ARG;
  }
  const int rc = pose_cache_check(fn, cache, io->X, nullptr, false, flags, N, P, C, Cp, J, dtype, io->W1, io->W1_bf16,
                                  io->ws, io->ws_bytes, stream);
  if (rc != APA_OK) return rc;
  return pose_attn_eval(nullptr, nullptr, APA_SCORES_SOFTMAX, io, N, P, C, Cp, J, K, flags, dtype, stream, cache, fn);
}
