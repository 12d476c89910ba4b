// apa_m1_probe.hip -- test-only access to the M == 1 dispatch (tests/test_m1_paths_gpu.py).
//
// Linked with apa_gemm_probe.hip and the product objects into libapa_gemm_probe.so (never into libapa_hip.so).
// Each wrapper runs one of the product's own extern "C" entry points with the same arguments while the calling
// thread's M1Trace pointer (apa_internal.h) is set, so the tests read back which kernel families, template
// instances, plan and reduce forms served the call.  The trace is zeroed first; the pointer is cleared afterwards.
#include "apa_internal.h"

namespace {
constexpr int64_t M1_PROBE_VERSION = 1;   // its own version: the GEMM half (apa_gemm_probe.hip) keeps its ABI

struct TraceScope {
  explicit TraceScope(apa::M1Trace* t) {
    if (t) *t = apa::M1Trace{};
    apa::g_m1_trace = t;
  }
  ~TraceScope() { apa::g_m1_trace = nullptr; }
};
}  // namespace

extern "C" {

int64_t apa_probe_m1_version(void) { return M1_PROBE_VERSION; }
int64_t apa_probe_m1_trace_size(void) { return (int64_t)sizeof(apa::M1Trace); }

// out[0..3] = S, ppb, nblk, lsplits of the plan both passes use
void apa_probe_m1_plan(int N, int P, int C, int Ca, int K, int64_t* out) {
  const apa::M1Plan pl = apa::m1_plan(N, P, C, Ca, K);
  out[0] = pl.S; out[1] = pl.ppb; out[2] = pl.nblk; out[3] = pl.lsplits;
}

// which families have an instance for (C, dtype), and which small-product kernels accept (C, K):
// bit 0 stream, 1 per-pixel vec, 2 generic, 3 m1_logits2, 4 m1_small (bwd_small / head), 5 bwd_head
int apa_probe_m1_support(int N, int C, int K, int dtype) {
  return (apa::m1s_supported(C, dtype) ? 1 : 0) | (apa::m1v_supported(C, dtype) ? 2 : 0) |
         (apa::m1g_supported(C, dtype) ? 4 : 0) | (apa::m1_logits2_supported(C, K) ? 8 : 0) |
         (apa::m1_small_supported(C, K) ? 16 : 0) | (apa::m1_bwd_head_supported(N, C, K) ? 32 : 0);
}

// The template instance the FP8 launchers / the rank-R launchers pick, by the functions they call themselves: NV of
// m1f_pool_fwd_kernel / m1f_bwd_main_kernel (0: m1f_supported refuses C), NVL of m1r_pool_fwd_kernel /
// m1r_bwd_main_kernel (0: no instance serves C).  Host only, nothing is launched.
int apa_probe_m1f_instance(int C) { return apa::m1f_supported(C) ? apa::m1f_vectors_per_lane(C) : 0; }
int apa_probe_m1r_instance(int C, int dtype) { return apa::m1r_vectors_per_lane(C, dtype); }

// Internal flag bits (APA_IFLAG_*, apa_internal.h) added to every m1_forward this thread runs through the wrappers
// below, until set again: APA_IFLAG_FINALIZE_LAUNCH = 1 << 27 puts the two forward sequences side by side
// (tests/test_m1_fold_gpu.py).  The extern "C" entries mask a caller's own internal bits.
void apa_probe_m1_set_iflags(unsigned iflags) { apa::g_m1_iflags = iflags; }

// out[0..1] = folded, launches of the last traced m1_forward (M1FwdRoute; M1Trace keeps its layout)
void apa_probe_m1_fwd_route(int64_t* out) {
  out[0] = apa::g_m1_fwd_route.folded; out[1] = apa::g_m1_fwd_route.launches;
}

// m1_call_fill alone, on the host: nothing is launched and no pointer is read.  A forward call (bwd == 0) or a
// backward call whose tensors all sit at `base` (16-byte aligned); out[0..9] = S, ppb, nblk, lsplits, plan total,
// pool family, small route, train, fused, offset of the partials in the workspace.  Returns m1_call_fill's status.
int apa_probe_m1_call_fill(int bwd, int loss_done, int xatt_is_x, int N, int P, int C, int Ca, int K, unsigned flags,
                           float keep_prob, int dtype, int64_t* out) {
  alignas(16) static char base[64];
  apa::M1Call c;
  apa::M1Bwd b{};
  b.X = base; b.Xatt = xatt_is_x ? base : base + 16;
  b.Wt = reinterpret_cast<const float*>(base); b.zsave = b.Wt; b.G = b.Wt; b.att = b.Wt;
  b.dXatt = base;
  apa::PoolCall d{{N, P, C, Ca, K, 1, dtype}};
  d.flags = flags; d.keep_prob = keep_prob; d.seed = 1; d.offset = 2; d.ws = base;
  const apa::M1Fwd f{b.X, b.Xatt};
  apa::M1Xent xf;
  xf.done = loss_done != 0;
  const int rc = apa::m1_call_fill(c, d, bwd ? nullptr : &f, bwd ? &b : nullptr, &xf);
  out[0] = c.pl.S; out[1] = c.pl.ppb; out[2] = c.pl.nblk; out[3] = c.pl.lsplits; out[4] = (int64_t)c.pl.total;
  out[5] = c.pool; out[6] = c.small; out[7] = c.train; out[8] = c.fused; out[9] = (int64_t)c.pl.off_pacc;
  return rc;
}

// The paired form of the streaming passes (apa_m1_stream.hip; tests/test_m1_paired_rows_*.py).
// out[0..1] = partial rows (M1Call::nrows) of the last traced forward / backward call
void apa_probe_m1_rows(int64_t* out) { out[0] = apa::g_m1_rows.fwd; out[1] = apa::g_m1_rows.bwd; }

// m1_call_fill alone, as apa_probe_m1_call_fill, for the row-count rule: out[0..3] = nrows, nblk, S, plan total.
// unpaired != 0: with APA_IFLAG_UNPAIRED set for the call; unpaired == 2: as the rank-R entry points fill it
// (apa_capi.hip rank_fwd_run / rank_bwd_run: m1_call_full_rows behind m1_call_fill).
int apa_probe_m1_call_rows(int bwd, int xatt_is_x, int unpaired, int N, int P, int C, int Ca, int K, unsigned flags,
                           float keep_prob, int dtype, int64_t* out) {
  alignas(16) static char base[64];
  apa::M1Call c;
  apa::M1Bwd b{};
  b.X = base; b.Xatt = xatt_is_x ? base : base + 16;
  b.Wt = reinterpret_cast<const float*>(base); b.zsave = b.Wt; b.G = b.Wt; b.att = b.Wt;
  b.dXatt = base;
  apa::PoolCall d{{N, P, C, Ca, K, 1, dtype}};
  d.flags = flags; d.keep_prob = keep_prob; d.seed = 1; d.offset = 2; d.ws = base;
  const apa::M1Fwd f{b.X, b.Xatt};
  const unsigned saved = apa::g_m1_iflags;
  if (unpaired == 1) apa::g_m1_iflags |= apa::APA_IFLAG_UNPAIRED;
  const int rc = apa::m1_call_fill(c, d, bwd ? nullptr : &f, bwd ? &b : nullptr, nullptr);
  if (unpaired == 2) apa::m1_call_full_rows(c, bwd != 0);
  apa::g_m1_iflags = saved;
  out[0] = c.nrows; out[1] = c.pl.nblk; out[2] = c.pl.S; out[3] = (int64_t)c.pl.total;
  return rc;
}

// apa_probe_m1_fwd_ex / apa_probe_m1_bwd_ex with pairing forced off: the streaming pass runs one 256-thread block and
// writes one partial row per logical block, at any S.  The workspace then holds the unpaired rows for a test to add up.
namespace {
struct UnpairedScope {
  unsigned saved;
  UnpairedScope() : saved(apa::g_m1_iflags) { apa::g_m1_iflags |= apa::APA_IFLAG_UNPAIRED; }
  ~UnpairedScope() { apa::g_m1_iflags = saved; }
};
}  // namespace
int apa_probe_m1_fwd_unpaired(apa::M1Trace* t, const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                              const float* ba, const float* Wt, const float* bt, float* logits, float* att,
                              float* zsave, float* abar, void* topdown, void* ws, size_t ws_bytes, int N, int P, int C,
                              int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                              int dtype, void* stream) {
  TraceScope s(t);
  UnpairedScope u;
  return apa_attn_pool_fwd_ex(hooks, X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown, ws, ws_bytes, N, P,
                              C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}
int apa_probe_m1_bwd_unpaired(apa::M1Trace* t, const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                              const float* ba, const float* Wt, const float* bt, const float* att, const float* zsave,
                              const float* abar, const float* G, void* dX, void* dXatt, float* dWa, float* dba,
                              float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                              int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                              void* stream) {
  TraceScope s(t);
  UnpairedScope u;
  return apa_attn_pool_bwd_ex(hooks, X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt, dbt,
                              ws, ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_fwd_ex(apa::M1Trace* t, const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                        const float* ba, const float* Wt, const float* bt, float* logits, float* att, float* zsave,
                        float* abar, void* topdown, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                        int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                        void* stream) {
  TraceScope s(t);
  return apa_attn_pool_fwd_ex(hooks, X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown, ws, ws_bytes, N, P,
                              C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_bwd_ex(apa::M1Trace* t, const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                        const float* ba, const float* Wt, const float* bt, const float* att, const float* zsave,
                        const float* abar, const float* G, void* dX, void* dXatt, float* dWa, float* dba,
                        float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K,
                        int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                        void* stream) {
  TraceScope s(t);
  return apa_attn_pool_bwd_ex(hooks, X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt, dbt,
                              ws, ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_fwd_cat(apa::M1Trace* t, const apa_concat_feat* cat, const apa_hooks* hooks, const void* X,
                         const void* Xatt, const float* Wa, const float* ba, const float* Wt, const float* bt,
                         float* logits, float* att, float* zsave, float* abar, void* topdown, void* ws,
                         size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob,
                         uint64_t seed, uint64_t offset, int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_pool_fwd_cat(cat, hooks, X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown, ws, ws_bytes,
                               N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_bwd_cat(apa::M1Trace* t, const apa_concat_feat* cat, const apa_hooks* hooks, const void* X,
                         const void* Xatt, const float* Wa, const float* ba, const float* Wt, const float* bt,
                         const float* att, const float* zsave, const float* abar, const float* G, void* dX,
                         void* dXatt, float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes,
                         int N, int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                         uint64_t offset, int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_pool_bwd_cat(cat, hooks, X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt,
                               dbt, ws, ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_train_step_ex(apa::M1Trace* t, const apa_hooks* hooks, const void* X, const void* Xatt,
                               const float* Wa, const float* ba, const float* Wt, const float* bt,
                               const int64_t* labels, float loss_wt, float grad_scale, float* logits, float* att,
                               float* zsave, float* abar, float* loss, float* G, void* dX, void* dXatt, float* dWa,
                               float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C,
                               int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                               int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_head_train_step_ex(hooks, X, Xatt, Wa, ba, Wt, bt, labels, loss_wt, grad_scale, logits, att, zsave,
                                     abar, loss, G, dX, dXatt, dWa, dba, dWt, dbt, ws, ws_bytes, N, P, C, Ca, K, M,
                                     flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_train_step_multilabel(apa::M1Trace* t, const apa_multilabel* ml, const apa_clip_pool* clip,
                                       const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                                       const float* ba, const float* Wt, const float* bt, float loss_wt,
                                       float grad_scale, float* logits, float* att, float* zsave, float* abar,
                                       float* loss, float* G, void* dX, void* dXatt, float* dWa, float* dba,
                                       float* dWt, float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca,
                                       int K, int M, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                       int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_head_train_step_multilabel(ml, clip, hooks, X, Xatt, Wa, ba, Wt, bt, loss_wt, grad_scale, logits,
                                             att, zsave, abar, loss, G, dX, dXatt, dWa, dba, dWt, dbt, ws, ws_bytes, N,
                                             P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_eval_step(apa::M1Trace* t, const void* X, const void* Xatt, const float* Wa, const float* ba,
                           const float* Wt, const float* bt, const int64_t* labels, float* logits, float* att,
                           float* zsave, float* abar, float* loss, float* probs, int64_t* pred, void* ws,
                           size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags, int dtype,
                           void* stream) {
  TraceScope s(t);
  return apa_attn_head_eval_step(X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws,
                                 ws_bytes, N, P, C, Ca, K, M, flags, dtype, stream);
}

// the *_cached entry points (apa.h: apa_feature_cache; tests/test_feature_cache_gpu.py)
int apa_probe_m1_fwd_cached(apa::M1Trace* t, const apa_feature_cache* cache, const apa_hooks* hooks, const void* X,
                            const void* Xatt, const float* Wa, const float* ba, const float* Wt, const float* bt,
                            float* logits, float* att, float* zsave, float* abar, void* topdown, void* ws,
                            size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob,
                            uint64_t seed, uint64_t offset, int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_pool_fwd_cached(cache, hooks, X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown, ws,
                                  ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_m1_bwd_cached(apa::M1Trace* t, const apa_feature_cache* cache, const apa_hooks* hooks, const void* X,
                            const void* Xatt, const float* Wa, const float* ba, const float* Wt, const float* bt,
                            const float* att, const float* zsave, const float* abar, const float* G, void* dX,
                            void* dXatt, float* dWa, float* dba, float* dWt, float* dbt, void* ws, size_t ws_bytes,
                            int N, int P, int C, int Ca, int K, int M, unsigned flags, float keep_prob, uint64_t seed,
                            uint64_t offset, int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_pool_bwd_cached(cache, hooks, X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt,
                                  dbt, ws, ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

}  // extern "C"
