// apa_pc_probe.hip -- test-only access to the per-class maps' dispatch (tests/test_pc_paths_gpu.py).
//
// Linked with the other probe sources and the product objects into libapa_gemm_probe.so (never into libapa_hip.so).
// Each wrapper runs one of the product's own extern "C" entry points with the same arguments while the calling thread's
// PcTrace pointer (apa_internal.h) is set, so the tests read back which path, kernel instance, operand form and tail
// served the call.  The trace is zeroed first; the pointer is cleared afterwards.
#include "apa_internal.h"

namespace {
constexpr int64_t PC_PROBE_VERSION = 1;

struct TraceScope {
  explicit TraceScope(apa::PcTrace* t) {
    if (t) *t = apa::PcTrace{};
    apa::g_pc_trace = t;
  }
  ~TraceScope() { apa::g_pc_trace = nullptr; }
};
}  // namespace

extern "C" {

int64_t apa_probe_pc_version(void) { return PC_PROBE_VERSION; }
int64_t apa_probe_pc_trace_size(void) { return (int64_t)sizeof(apa::PcTrace); }

// out[0..15]: the PcPlan carve (apa_internal.h pc_plan_offsets); out[16..24]: byte offsets, from the workspace base, of
// the PcFusedWs members WcatT, Wcat2, bcat, dTdZ, partial, maskbits, lpart, bits_tag and the end of the carve
// (meaningful when the plan has a fused part: bf16, K <= 64, Ca == C)
void apa_probe_pc_plan(int N, int P, int C, int Ca, int K, int dtype, int64_t* out) {
  size_t o[16];
  apa::pc_plan_offsets(N, P, C, Ca, K, dtype, o);
  for (int i = 0; i < 16; ++i) out[i] = (int64_t)o[i];
  char* base = reinterpret_cast<char*>(static_cast<uintptr_t>(1) << 20);   // (addresses only: nothing is dereferenced)
  const apa::PcFusedWs f = apa::pc_fused_carve(base + o[14], N, P, C);
  const void* m[8] = {f.WcatT, f.Wcat2, f.bcat, f.dTdZ, f.partial, f.maskbits, f.lpart, f.bits_tag};
  for (int i = 0; i < 8; ++i) out[16 + i] = (int64_t)(static_cast<const char*>(m[i]) - base);
  out[24] = (int64_t)(o[14] + apa::pc_fused_ws_bytes(N, P, C));
}

// bit 0: pc_fused_supported for 16-byte aligned X == Xatt; bit 1: pc_fused_dx_supported(P, act)
int apa_probe_pc_support(int N, int P, int C, int Ca, int K, int dtype, int act) {
  const void* x = reinterpret_cast<const void*>(static_cast<uintptr_t>(1) << 20);
  return (apa::pc_fused_supported(N, P, C, Ca, K, dtype, x, x) ? 1 : 0) | (apa::pc_fused_dx_supported(P, act) ? 2 : 0);
}
int apa_probe_pc_psplit(int N, int kgroups, int P, int act) { return apa::pc_bwd_act_psplit_host(N, kgroups, P, act); }
// out[0..5] = upb, splits, rbs of pc_bwd_dx_kernel; S, rows_per_split, ctiles of pc_bwd_dw_kernel
void apa_probe_pc_geometry(int R, int C, int* out) { apa::pc_fused_geometry(R, C, out); }
// (asks the device for its CU count)
int apa_probe_pc_wide_serves(int M, int N, int K) { return apa::gemm_bf16_wide_serves(M, N, K) ? 1 : 0; }

int apa_probe_pc_fwd_ex(apa::PcTrace* t, const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                        const float* ba, const float* Wt, const float* bt, float* logits, float* att, float* zsave,
                        float* abar, void* topdown, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M,
                        unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_pool_fwd_ex(hooks, X, Xatt, Wa, ba, Wt, bt, logits, att, zsave, abar, topdown, ws, ws_bytes, N, P, C,
                              Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_pc_bwd_ex(apa::PcTrace* t, const apa_hooks* hooks, const void* X, const void* Xatt, const float* Wa,
                        const float* ba, const float* Wt, const float* bt, const float* att, const float* zsave,
                        const float* abar, const float* G, void* dX, void* dXatt, float* dWa, float* dba, float* dWt,
                        float* dbt, void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags,
                        float keep_prob, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  TraceScope s(t);
  return apa_attn_pool_bwd_ex(hooks, X, Xatt, Wa, ba, Wt, bt, att, zsave, abar, G, dX, dXatt, dWa, dba, dWt, dbt, ws,
                              ws_bytes, N, P, C, Ca, K, M, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_pc_train_step_ex(apa::PcTrace* t, const apa_hooks* hooks, const void* X, const void* Xatt,
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

int apa_probe_pc_eval_step(apa::PcTrace* t, const void* X, const void* Xatt, const float* Wa, const float* ba,
                           const float* Wt, const float* bt, const int64_t* labels, float* logits, float* att,
                           float* zsave, float* abar, float* loss, float* probs, int64_t* pred, void* ws,
                           size_t ws_bytes, int N, int P, int C, int Ca, int K, int M, unsigned flags, int dtype,
                           void* stream) {
  TraceScope s(t);
  return apa_attn_head_eval_step(X, Xatt, Wa, ba, Wt, bt, labels, logits, att, zsave, abar, loss, probs, pred, ws,
                                 ws_bytes, N, P, C, Ca, K, M, flags, dtype, stream);
}

// The trace without a wrapper: every entry point of THIS library the calling thread runs between the two calls records
// into *t (zeroed here).  tests/test_cached_perclass_gpu.py brackets the *_cached calls and steps, clips and sigmoid
// losses included, and the plain calls on a gathered copy they must match launch for launch.
void apa_probe_pc_trace_begin(apa::PcTrace* t) {
  if (t) *t = apa::PcTrace{};
  apa::g_pc_trace = t;
}
void apa_probe_pc_trace_end(void) { apa::g_pc_trace = nullptr; }

int apa_probe_pc_weight_images(apa::PcTrace* t, const float* Wa, const float* ba, const float* Wt, const float* bt,
                               void* ws, size_t ws_bytes, int N, int P, int C, int Ca, int K, int dtype,
                               apa_weight_image* maps, int* nmaps, void* stream) {
  TraceScope s(t);
  return apa_per_class_weight_images(Wa, ba, Wt, bt, ws, ws_bytes, N, P, C, Ca, K, dtype, maps, nmaps, stream);
}

}  // extern "C"
