// apa_mlloss.hip -- the sigmoid ("multi-label") action losses of HICO and Charades, row-parallel, value + gradient:
//   'multi-label'    mean(tf.nn.weighted_cross_entropy_with_logits(targets, logits, pos_weight))   src/loss.py:88-97
//   'multi-label-2'  tf.losses.sigmoid_cross_entropy(labels, logits) * wt                          src/loss.py:98-101
// x = logits [N,K], t = f32 multi-hot labels [N,K] (read_sparse_label):
//   loss[1+n] = (1/K) sum_k l(x[n,k], t[n,k]);   loss[0] = wt/N sum_n loss[1+n];   G[n,k] = wt grad_scale/(N K) l'
// with l, l' of ml_term (apa_device.h) -- apa_action_loss_fwd_bwd's arithmetic (apa_loss2.hip), whose one block walks
// all N*K elements serially.  Every kernel here runs ml_row (apa_device.h) on a 256-thread block per row, so the
// stand-alone launch, the fold below and the clip loss (apa_cliploss.hip) give each other's bits.
//
//   ml_rows_kernel       the stand-alone loss on finished logits, one block per row; clip_finish_kernel
//                        (apa_cliploss.hip) then sums the rows in the softmax step's order for (N, K)
//   m1_logits_ml_kernel  the fold of the one-call M == 1 step: the reducer of the partial-logits product
//                        (m1_logits_reduce_kernel's sums, apa_m1_small.hip: the logits keep apa_attn_pool_fwd's bits)
//                        applies the row routine to the values it has just formed -- no launch for the loss.  Thread
//                        tid owns the columns tid + 256 e in registers: no LDS row, K <= 1024.  loss[0] is finished by
//                        the backward head kernel, as for the softmax fold; where that kernel does not serve the shape
//                        (more than 4 columns of dbt per block: K = 600 at C = 2048) by clip_finish_kernel, in the same
//                        order -- the launch the stand-alone loss would have spent on its rows.
// No atomics; every sum has one order: identical calls give identical bits.
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

__global__ __launch_bounds__(256) void ml_rows_kernel(const float* __restrict__ logits,
                                                      const float* __restrict__ labels, float* __restrict__ loss,
                                                      float* __restrict__ G, int K, int kind, float pw, float gscale) {
  __shared__ float red[4];
  const size_t r0 = (size_t)blockIdx.x * K;
  const float* xr = logits + r0;
  const float s = ml_row<0>([&](int, int k) { return xr[k]; }, labels + r0, G + r0, K, kind, pw, gscale, red);
  if (threadIdx.x == 0) loss[1 + blockIdx.x] = s;
}

// pstat (the folded route): abar[n] is formed here, by every wave alike, and stored for the backward pass
template <int EPT>   // columns per thread, K <= 256 EPT
__global__ __launch_bounds__(256) void m1_logits_ml_kernel(
    const float* __restrict__ part, float* abar, const float* __restrict__ bt, const float* __restrict__ labels,
    float* __restrict__ logits, float* __restrict__ out_loss, float* __restrict__ G, int N, int K, int nchunks,
    int kind, float pw, float gscale, const float* __restrict__ pstat, int S, int P) {
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x;
  const size_t stride = (size_t)N * K;
  const float* prow = part + (size_t)n * K;
  float ab;
  if (pstat) {
    ab = m1_abar_wave(pstat, n, S, P, tid & 63);
    if (tid == 0) abar[n] = ab;
  } else {
    ab = abar[n];
  }
  float btv[EPT], acc[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    btv[e] = bt[min(tid + 256 * e, K - 1)];
    acc[e] = 0.f;
  }
  for (int c = 0; c < nchunks; c += 32) {   // one round trip for up to 32 partials (m1_logits_reduce_kernel's order)
    float v[EPT][32];
#pragma unroll
    for (int e = 0; e < EPT; ++e)
#pragma unroll
      for (int u = 0; u < 32; ++u)
        v[e][u] = prow[(size_t)min(c + u, nchunks - 1) * stride + min(tid + 256 * e, K - 1)];
#pragma unroll
    for (int e = 0; e < EPT; ++e)
#pragma unroll
      for (int u = 0; u < 32; ++u) acc[e] += (c + u < nchunks) ? v[e][u] : 0.f;
  }
  float lg[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const int j = tid + 256 * e;
    lg[e] = fmaf(ab, btv[e], acc[e]);
    if (j < K) logits[(size_t)n * K + j] = lg[e];
  }
  const size_t r0 = (size_t)n * K;
  const float s = ml_row<EPT>([&](int j, int) { return lg[j]; }, labels + r0, G + r0, K, kind, pw, gscale, red);
  if (tid == 0) out_loss[1 + n] = s;
}

bool m1_logits_ml_supported(int N, int C, int K) {
  return m1_logits2_supported(C, K) && N >= 1 && K >= 4 && K <= 1024;
}

int m1_logits2_ml(float* z, const float* Wt, float* abar, const float* bt, const M1Xent& xf, float* logits,
                  float* part_ws, int N, int C, int K, hipStream_t st, const M1Fold* fold) {
  int nparts = 0;
  const int rc = m1_logits2_partials(z, Wt, part_ws, N, C, K, st, fold, &nparts);
  if (rc != APA_OK) return rc;
  const float* const pstat = fold ? fold->pstat : nullptr;
  const int fS = fold ? fold->S : 0, fP = fold ? fold->P : 1;
#define APA_LM(EPT)                                                                                             \
  hipLaunchKernelGGL((m1_logits_ml_kernel<EPT>), dim3(N), dim3(256), 0, st, part_ws, abar, bt, xf.mlabels,      \
                     logits, xf.loss, xf.G, N, K, nparts, xf.kind, xf.pos_weight, xf.gscale, pstat, fS, fP)
  const int ept = K <= 256 ? 1 : (K <= 512 ? 2 : 4);
  if (M1Trace* t = m1_trace()) t->logits_nv4 = ept;
  if (ept == 1) APA_LM(1);
  else if (ept == 2) APA_LM(2);
  else APA_LM(4);
#undef APA_LM
  APA_LAUNCH_CHECK("m1_logits_ml_kernel");
  return APA_OK;
}

int ml_loss_rows(int kind, const float* labels, float pos_weight, const float* logits, float* loss, float* G, int N,
                 int K, float wt, float grad_scale, hipStream_t st) {
  float lscale, gscale;
  ml_scales(kind, wt, grad_scale, N, K, &lscale, &gscale);
  hipLaunchKernelGGL(ml_rows_kernel, dim3(N), dim3(256), 0, st, logits, labels, loss, G, K, kind, pos_weight, gscale);
  APA_LAUNCH_CHECK("ml_rows_kernel");
  return clip_loss_finish(nullptr, nullptr, loss, nullptr, nullptr, N, N, K, lscale, st);
}

}  // namespace apa

using namespace apa;

extern "C" int apa_multilabel_loss_fwd_bwd(const apa_multilabel* ml, const float* logits, float* loss, float* G, int N,
                                           int K, float wt, float grad_scale, void* stream) {
  const int rc = check_multilabel("apa_multilabel_loss_fwd_bwd", ml);
  if (rc != APA_OK) return rc;
  if (!logits || !loss || !G || N <= 0 || K <= 0) {
    set_error("apa_multilabel_loss_fwd_bwd: null pointer or non-positive N=%d K=%d", N, K);
    return APA_ERR_INVALID_ARG;
  }
  return ml_loss_rows(ml->kind, ml->labels, ml->pos_weight, logits, loss, G, N, K, wt, grad_scale,
                      static_cast<hipStream_t>(stream));
}
