// apa_pose_probe.hip -- test-only access to the pose-head dispatch (tests/test_pose_paths_gpu.py).
//
// Linked with apa_gemm_probe.hip, apa_m1_probe.hip and the product objects into libapa_gemm_probe.so (never into
// libapa_hip.so).  Each wrapper runs one of the product's own extern "C" entry points with the same arguments while
// the calling thread's PoseTrace pointer (apa_internal.h) is set, so the tests read back which kernel family, template
// instance, block shape and reduce form served the call.  The trace is zeroed first; the pointer is cleared afterwards.
#include "../../include/apa_pose_cache.h"
#include "apa_internal.h"

namespace {
constexpr int64_t POSE_PROBE_VERSION = 1;

struct TraceScope {
  explicit TraceScope(apa::PoseTrace* t) {
    if (t) *t = apa::PoseTrace{};
    apa::g_pose_trace = t;
  }
  ~TraceScope() { apa::g_pose_trace = nullptr; }
};
// the pooling half's trace beside it (the cached cfg 003 steps: both are compared with the plain step's)
struct M1TraceScope {
  explicit M1TraceScope(apa::M1Trace* t) {
    if (t) *t = apa::M1Trace{};
    apa::g_m1_trace = t;
  }
  ~M1TraceScope() { apa::g_m1_trace = nullptr; }
};
}  // namespace

extern "C" {

int64_t apa_probe_pose_version(void) { return POSE_PROBE_VERSION; }
int64_t apa_probe_pose_trace_size(void) { return (int64_t)sizeof(apa::PoseTrace); }

// out[0..7] = R, nchunks, off_dppre, off_partial, off_gemm, off_w1b, off_lpart, total (bytes) of the workspace carve
void apa_probe_pose_plan(int N, int P, int C, int Cp, int J, int dtype, int64_t* out) {
  size_t o[8];
  apa::pose_plan_offsets(N, P, C, Cp, J, dtype, o);
  for (int i = 0; i < 8; ++i) out[i] = (int64_t)o[i];
}

// out[0..1] = byte offsets of dz [N,C] f32 and of the keep bits in the POOLING workspace (m1_plan): what the fused step's
// dX product reads for its rank-1 epilogue
void apa_probe_pose_pool_offsets(int N, int P, int C, int Ca, int K, int64_t* out) {
  const apa::M1Plan pl = apa::m1_plan(N, P, C, Ca, K);
  out[0] = (int64_t)pl.off_dz; out[1] = (int64_t)pl.off_maskbits;
}

int apa_probe_pose_head_fwd(apa::PoseTrace* t, const void* X, const float* W1, const float* b1, const float* W2,
                            const float* b2, void* Ppre, float* Pl, void* ws, size_t ws_bytes, int N, int P, int C,
                            int Cp, int J, int dtype, void* stream) {
  TraceScope s(t);
  return apa_pose_head_fwd(X, W1, b1, W2, b2, Ppre, Pl, ws, ws_bytes, N, P, C, Cp, J, dtype, stream);
}

int apa_probe_pose_head_bwd(apa::PoseTrace* t, const void* X, const float* W1, const float* W2, const void* Ppre,
                            const float* dPl, const void* dPpre_ext, void* dX, int accumulate_dX, float* dW1,
                            float* db1, float* dW2, float* db2, void* ws, size_t ws_bytes, int N, int P, int C, int Cp,
                            int J, int dtype, void* stream) {
  TraceScope s(t);
  return apa_pose_head_bwd(X, W1, W2, Ppre, dPl, dPpre_ext, dX, accumulate_dX, dW1, db1, dW2, db2, ws, ws_bytes, N, P,
                           C, Cp, J, dtype, stream);
}

int apa_probe_pose_head_bwd_rank1ext(apa::PoseTrace* t, const void* X, const float* W1, const float* W2,
                                     const void* Ppre, const float* dPl, const float* ext_row, const float* ext_col,
                                     void* dX, int accumulate_dX, float* dW1, float* db1, float* dW2, float* db2,
                                     void* ws, size_t ws_bytes, int N, int P, int C, int Cp, int J, int dtype,
                                     void* stream) {
  TraceScope s(t);
  return apa_pose_head_bwd_rank1ext(X, W1, W2, Ppre, dPl, ext_row, ext_col, dX, accumulate_dX, dW1, db1, dW2, db2, ws,
                                    ws_bytes, N, P, C, Cp, J, dtype, stream);
}

int apa_probe_pose_attn_train_step(apa::PoseTrace* t, const apa_pose_attn_step_io* io, int N, int P, int C, int Cp,
                                   int J, int K, unsigned flags, float keep_prob, uint64_t seed, uint64_t offset,
                                   int dtype, void* stream) {
  TraceScope s(t);
  return apa_pose_attn_train_step(io, N, P, C, Cp, J, K, flags, keep_prob, seed, offset, dtype, stream);
}

// The cfg 003 steps from a feature cache (apa_pose_cache.h) with both traces; cache == NULL: the plain step on io->X,
// traced the same way -- what the cached call is compared with
int apa_probe_pose_attn_train_step_cached(apa::PoseTrace* t, apa::M1Trace* m, const apa_feature_cache* cache,
                                          const apa_pose_attn_step_io* io, int N, int P, int C, int Cp, int J, int K,
                                          unsigned flags, float keep_prob, uint64_t seed, uint64_t offset, int dtype,
                                          void* stream) {
  TraceScope s(t);
  M1TraceScope sm(m);
  if (!cache) return apa_pose_attn_train_step(io, N, P, C, Cp, J, K, flags, keep_prob, seed, offset, dtype, stream);
  return apa_pose_attn_train_step_cached(cache, io, N, P, C, Cp, J, K, flags, keep_prob, seed, offset, dtype, stream);
}

int apa_probe_pose_attn_eval_step_cached(apa::PoseTrace* t, apa::M1Trace* m, const apa_feature_cache* cache,
                                         const apa_pose_attn_eval_io* io, int N, int P, int C, int Cp, int J, int K,
                                         unsigned flags, int dtype, void* stream) {
  TraceScope s(t);
  M1TraceScope sm(m);
  if (!cache) return apa_pose_attn_eval_step(io, N, P, C, Cp, J, K, flags, dtype, stream);
  return apa_pose_attn_eval_step_cached(cache, io, N, P, C, Cp, J, K, flags, dtype, stream);
}

}  // extern "C"
