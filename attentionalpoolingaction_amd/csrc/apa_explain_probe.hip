// apa_explain_probe.hip -- test-only: what apa_attn_explain (apa_explain.hip) decides before its launches
// (tests/test_explain_gpu.py, tests/test_explain_paths_cpu.py).
//
// Linked with the other probe sources and the product objects into libapa_gemm_probe.so (never into libapa_hip.so).
// Host only: nothing is launched and no device is asked for anything.  The split count comes from explain_plan, the
// wave geometry from ExplainGeom<TT> and the pixel ranges from m1_pix_range -- the functions the launch and the kernel
// use themselves; the load form (EPV) restates the three-way choice of apa_attn_explain, which has no function of its own.
#include "apa_device.h"
#include "apa_internal.h"

namespace {
constexpr int64_t EXPLAIN_PROBE_VERSION = 1;

template <int TT> void geom(int64_t* pix, int64_t* u) {
  *pix = apa::ExplainGeom<TT>::PIX;
  *u = apa::ExplainGeom<TT>::U;
}
}  // namespace

extern "C" {

int64_t apa_probe_explain_version(void) { return EXPLAIN_PROBE_VERSION; }

// out[0..10] = S, nblk, EPV, PIX, U, channels per round of the channel loop (64 * EPV * U), its rounds, the largest
// pixel count of a block, the groups of PIX pixels such a block has (its four waves stride over them: wave 0 makes
// ceil(groups / 4) trips of the group loop), S of m1_plan before explain_plan's halving, LDS bytes of a block.
// Returns 1, or 0 for a shape apa_attn_explain refuses (out untouched).
int apa_probe_explain_plan(int N, int P, int C, int K, int T, int dtype, int64_t* out) {
  if (!out || apa_attn_explain_workspace_bytes(N, P, C, K, T, dtype) == 0) return 0;
  const apa::ExplainPlan pl = apa::explain_plan(N, P, C, K, T);
  const int64_t epv = dtype == APA_DTYPE_BF16 ? (C % 8 == 0 ? 8 : 4) : 4;
  int64_t pix = 0, u = 0;
  switch (T) {
    case 1: geom<1>(&pix, &u); break;
    case 2: geom<2>(&pix, &u); break;
    case 3: geom<3>(&pix, &u); break;
    case 4: geom<4>(&pix, &u); break;
    case 5: geom<5>(&pix, &u); break;
    case 6: geom<6>(&pix, &u); break;
    case 7: geom<7>(&pix, &u); break;
    case 8: geom<8>(&pix, &u); break;
    default: return 0;
  }
  int64_t most = 0;
  for (int s = 0; s < pl.S; ++s) {
    int b, e;
    apa::m1_pix_range(s, P, pl.S, b, e);
    if (e - b > most) most = e - b;
  }
  const int64_t per_round = 64 * epv * u;
  const int64_t groups = (most + pix - 1) / pix;
  out[0] = pl.S; out[1] = pl.nblk; out[2] = epv; out[3] = pix; out[4] = u;
  out[5] = per_round; out[6] = (C + per_round - 1) / per_round;
  out[7] = most; out[8] = groups;
  out[9] = apa::m1_plan(N, P, C, C, K).S;
  out[10] = (int64_t)T * C * 4;
  return 1;
}

}  // extern "C"
