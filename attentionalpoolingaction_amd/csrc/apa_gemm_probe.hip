// apa_gemm_probe.hip -- test-only access to the dense GEMM dispatcher (tests/test_gemm_paths_gpu.py).
//
// Linked with the product objects into libapa_gemm_probe.so (never into libapa_hip.so): a flat, versioned C struct
// becomes a GemmDesc and goes to the product's gemm_launch, so the tests drive every kernel kind, layout, split and
// epilogue term directly and read back (GemmDesc::trace) which path served the call.  m1_colsum and sgemm_small are
// exposed the same way.  Every field is 8 bytes wide so that the ctypes mirror has no padding to get wrong.
#include "apa_internal.h"

namespace {
constexpr int64_t PROBE_VERSION = 2;

struct ProbeGemm {
  int64_t version;                 // PROBE_VERSION
  const void* A; int64_t lda, ta, a_kc;
  const void* B; int64_t ldb, tb, b_kc;
  void* C; int64_t ldc, tc;
  int64_t M, N, K, n_valid;
  const float* bias; double beta; int64_t act;
  int64_t splits; float* ws;
  int64_t drop_a, drop_c; double inv_keep; int64_t thresh; uint64_t seed, offset;
  const float* r1_row; const float* r1_col; const uint8_t* r1_bits; int64_t r1_P; double r1_invP, r1_inv_keep;
  const uint8_t* mid_bits; int64_t mid_k; double mid_inv_keep;
  int64_t stream_out;
};

struct ProbeColsum {               // the ColsumArgs fields GemmDesc::tail carries (pdba / dba / perm_* excepted)
  const float* pdwa; float* dwa; int64_t nblk, C, ld;
  float* dwa2; int64_t C1; float* dwa3; int64_t C2; float* dwa4; int64_t C3; float* dwa5; int64_t C4;
  const float* aux_src; int64_t aux_n; double aux_scale; float* aux_dst;
  uint64_t* rng_bump;
};

struct ProbeTrace { int64_t kind, splits, k_per_split, mt, twin, reduce; };

apa::GemmDesc to_desc(const ProbeGemm& p) {
  apa::GemmDesc d;
  d.A = p.A; d.lda = p.lda; d.ta = (int)p.ta; d.a_kc = p.a_kc != 0;
  d.B = p.B; d.ldb = p.ldb; d.tb = (int)p.tb; d.b_kc = p.b_kc != 0;
  d.C = p.C; d.ldc = p.ldc; d.tc = (int)p.tc;
  d.M = (int)p.M; d.N = (int)p.N; d.K = (int)p.K; d.n_valid = (int)p.n_valid;
  d.bias = p.bias; d.beta = (float)p.beta; d.act = (int)p.act;
  d.splits = (int)p.splits; d.ws = p.ws;
  d.drop_a = (int)p.drop_a; d.drop_c = (int)p.drop_c; d.inv_keep = (float)p.inv_keep;
  d.thresh = (uint32_t)p.thresh; d.seed = p.seed; d.offset = p.offset;
  d.r1_row = p.r1_row; d.r1_col = p.r1_col; d.r1_bits = p.r1_bits; d.r1_P = (int)p.r1_P;
  d.r1_invP = (float)p.r1_invP; d.r1_inv_keep = (float)p.r1_inv_keep;
  d.mid_bits = p.mid_bits; d.mid_k = (int)p.mid_k; d.mid_inv_keep = (float)p.mid_inv_keep;
  d.stream_out = p.stream_out != 0;
  return d;
}

apa::ColsumArgs to_colsum(const ProbeColsum& c) {
  apa::ColsumArgs a;
  a.pdwa = c.pdwa; a.dwa = c.dwa; a.nblk = (int)c.nblk; a.C = (int)c.C; a.ld = (int)c.ld;
  a.dwa2 = c.dwa2; a.C1 = (int)c.C1; a.dwa3 = c.dwa3; a.C2 = (int)c.C2;
  a.dwa4 = c.dwa4; a.C3 = (int)c.C3; a.dwa5 = c.dwa5; a.C4 = (int)c.C4;
  a.aux_src = c.aux_src; a.aux_n = (int)c.aux_n; a.aux_scale = (float)c.aux_scale; a.aux_dst = c.aux_dst;
  a.rng_bump = c.rng_bump;
  return a;
}

void to_trace(const apa::GemmTrace& t, ProbeTrace* o) {
  if (!o) return;
  o->kind = t.kind; o->splits = t.splits; o->k_per_split = t.k_per_split; o->mt = t.mt; o->twin = t.twin;
  o->reduce = t.reduce;
}
}  // namespace

extern "C" {

int64_t apa_probe_gemm_struct_size(void) { return (int64_t)sizeof(ProbeGemm); }
int64_t apa_probe_gemm_version(void) { return PROBE_VERSION; }
int64_t apa_probe_gemm_ws_bytes(int M, int N, int splits) { return (int64_t)apa::gemm_ws_bytes(M, N, splits); }
int apa_probe_gemm_pick_splits(int M, int N, int K) { return apa::gemm_pick_splits(M, N, K); }
int64_t apa_probe_sgemm_ws_bytes(int m, int n, int splits) { return (int64_t)apa::sgemm_ws_bytes(m, n, splits); }
const char* apa_probe_last_error(void) { return apa_last_error(); }

// twin / tail / traces may be null.  *tail_done (if given): the column sum rode on the split-K reduce launch.
int apa_probe_gemm_launch(const ProbeGemm* p, const ProbeGemm* twin, const ProbeColsum* tail, ProbeTrace* trace,
                          ProbeTrace* twin_trace, int* tail_done, void* stream) {
  if (!p || p->version != PROBE_VERSION || (twin && twin->version != PROBE_VERSION)) {
    apa::set_error("apa_probe_gemm_launch: null descriptor or version mismatch");
    return APA_ERR_INVALID_ARG;
  }
  apa::GemmTrace tr, ttr;
  apa::GemmDesc d = to_desc(*p), t;
  if (twin) { t = to_desc(*twin); t.trace = &ttr; d.twin = &t; }
  apa::ColsumJob job;
  if (tail) { job.a = to_colsum(*tail); d.tail = &job; }
  d.trace = &tr;
  const int rc = apa::gemm_launch(d, static_cast<hipStream_t>(stream));
  to_trace(tr, trace);
  to_trace(ttr, twin_trace);
  if (tail_done) *tail_done = job.done ? 1 : 0;
  return rc;
}

// ... with operand A read through a row map (GemmDesc::rmap): A addresses a [T * P] row buffer, row r of the product's A
// is its row clamp(index[r / P], 0, T - 1) * P + r % P
int apa_probe_gemm_launch_rowmap(const ProbeGemm* p, const int32_t* index, int T, int P, ProbeTrace* trace) {
  if (!p || p->version != PROBE_VERSION) {
    apa::set_error("apa_probe_gemm_launch_rowmap: null descriptor or version mismatch");
    return APA_ERR_INVALID_ARG;
  }
  apa::GemmTrace tr;
  apa::GemmDesc d = to_desc(*p);
  d.rmap.index = index; d.rmap.T = T; d.rmap.P = P;
  d.trace = &tr;
  int rc = APA_OK;
  if (!index) {
    apa::set_error("apa_probe_gemm_launch_rowmap: null index");
    rc = APA_ERR_INVALID_ARG;
  } else {
    rc = apa::gemm_launch(d, nullptr);
  }
  to_trace(tr, trace);
  return rc;
}

int apa_probe_m1_colsum(const ProbeColsum* c, void* stream) {
  if (!c) { apa::set_error("apa_probe_m1_colsum: null"); return APA_ERR_INVALID_ARG; }
  return apa::m1_colsum(to_colsum(*c), static_cast<hipStream_t>(stream));
}

// ... with the scalar sum of block 0 as well: dba[0] = sum of pdba[0 .. nblk) (ProbeColsum keeps its layout)
int apa_probe_m1_colsum_dba(const ProbeColsum* c, const float* pdba, float* dba, void* stream) {
  if (!c) { apa::set_error("apa_probe_m1_colsum_dba: null"); return APA_ERR_INVALID_ARG; }
  apa::ColsumArgs a = to_colsum(*c);
  a.pdba = pdba; a.dba = dba;
  return apa::m1_colsum(a, static_cast<hipStream_t>(stream));
}

int apa_probe_sgemm_small(const float* A, int64_t a_si, int64_t a_sk, const float* B, int64_t b_sk, int64_t b_sj,
                          float* D, int64_t ldd, int m, int n, int kdim, int splits, const float* u, const float* v,
                          float* ws, void* stream) {
  if (splits > 1 && !ws) { apa::set_error("apa_probe_sgemm_small: split-K needs a workspace"); return APA_ERR_WORKSPACE; }
  return apa::sgemm_small(A, a_si, a_sk, B, b_sk, b_sj, D, ldd, m, n, kdim, splits, u, v, ws,
                          static_cast<hipStream_t>(stream));
}

}  // extern "C"
