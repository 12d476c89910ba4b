// apa_loss.hip -- loss kernels of the head (fused value + gradient) and small elementwise ops.
//   softmax cross-entropy : /root/reference/src/loss.py:74-80  (+ eval.py:193-197 consumers)
//   masked pose L2        : /root/reference/src/loss.py:29-70
//   zero_out_channels     : /root/reference/src/custom_ops/zero_out_channels.cc:18-51
//   dropout mask dump     : parity helper for slim.dropout (nets_factory.py:296)
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

// Softmax cross-entropy, fused value + gradient (+ probabilities, + first-index argmax).  The row is xent_row_regs
// (apa_xent_row.h: why half a wave per row, why unaligned 16-byte vectors, why code size is time): a 16-wave block
// covers 32 rows in a single pass (no per-row unrolled copies).
// out_loss[1+n] = xent_n (unweighted); out_loss[0] = lscale * sum_n xent_n.
//   mode 1: one block does everything (N <= 64, only the loss is wanted);
//   mode 2: block 0 computes the losses / predictions of ALL rows (the batch mean needs every row
//           anyway), blocks 1.. write G / probs: one CU moving 2 x 50 KB alone is 3 us of queueing;
//   mode 0: N > 64, out_loss[0] is summed by sum_scale_kernel.
template <int NV4>   // 16-byte vectors per lane: xent_row_nv4(K)
__global__ __launch_bounds__(1024) void softmax_xent_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels,
    float* __restrict__ out_loss, float* __restrict__ G, float* __restrict__ probs,
    int64_t* __restrict__ pred, int N, int K, float gscale, float lscale, int mode) {
  __shared__ float red[32];
  const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
  const int wpb = blockDim.x >> 6;
  const bool split = mode == 2;
  const bool loss_role = !split || blockIdx.x == 0;
  if (split && blockIdx.x == 0) { G = nullptr; probs = nullptr; }
  const int wid = (split ? (blockIdx.x == 0 ? 0 : blockIdx.x - 1) : blockIdx.x) * wpb + (threadIdx.x >> 6);
  const int nw = (split ? (blockIdx.x == 0 ? 1 : gridDim.x - 1) : gridDim.x) * wpb;
  float slot_loss = 0.f;
  for (int base = 2 * wid; base < N; base += 2 * nw) {
    const int n = base + half;
    const bool active = n < N;
    const size_t nc = (size_t)min(n, N - 1);   // the idle half of a ragged last pair re-reads row N-1
    const float* row = logits + nc * K;
    int cand;
    const float lv = xent_row_regs<NV4>(
        [&](int colc) { return *reinterpret_cast<const f4u*>(row + colc); }, [&](int c) { return row[c]; }, K,
        (int)labels[nc], gscale, lane, active && (G || probs),
        [&](int colc, int col0, const f4u& p, const f4u& g) {
          xent_store_vec(probs != nullptr, probs + nc * K, G != nullptr, G + nc * K, colc, col0, K, p, g);
        },
        &cand);
    if (active) {
      slot_loss += lv;   // a half-wave's rows are summed in increasing n
      if (hl == 0 && loss_role) {
        out_loss[1 + n] = lv;
        if (pred) pred[n] = cand;
      }
    }
  }
  // The 32-slot order of the batch mean, by definition: the slots are this block's half waves.  A kernel that folds
  // the loss in reproduces it with xent_mean32_* (apa_xent_row.h).
  if (mode != 0 && loss_role) {
    if (hl == 0) red[(threadIdx.x >> 6) * 2 + half] = slot_loss;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = 0.f;
      for (int w = 0; w < 2 * wpb; ++w) t += red[w];
      out_loss[0] = t * lscale;
    }
  }
}

// Generic fallback (K < 4 or K > 1024): one wave per row, xent_row_stream.
__global__ __launch_bounds__(256) void softmax_xent_stream_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ labels,
    float* __restrict__ out_loss, float* __restrict__ G, float* __restrict__ probs,
    int64_t* __restrict__ pred, int N, int K, float gscale) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* row = logits + (size_t)n * K;
  int cand;
  const float lv = xent_row_stream([&](int k) { return row[k]; }, K, (int)labels[n], probs != nullptr,
                                   probs + (size_t)n * K, G != nullptr, G + (size_t)n * K, gscale, &cand);
  if ((threadIdx.x & 63) == 0) {
    out_loss[1 + n] = lv;
    if (pred) pred[n] = cand;
  }
}

// out[0] = scale * sum_{i<count} in[i], fixed order (one block): the 256-thread order of the batch mean, by definition
__global__ __launch_bounds__(256) void sum_scale_kernel(const float* __restrict__ in,
                                                        float* __restrict__ out, int count,
                                                        float scale) {
  __shared__ float red[4];
  const float t = block_sum256(xent_mean256_load(in, count), red);
  if (threadIdx.x == 0) out[0] = t * scale;
}

// Pose L2: block (n, s) handles share s of image n's P*J elements (grid.y shares: N blocks alone were 32 CUs'
// worth of 12-deep load chains).  ws[n * grid.y + s] = sum over the share of valid[n,j] * (Pl-lbl)^2.
constexpr int POSE_L2_MAX_SPLIT = 8;
__global__ __launch_bounds__(256) void pose_l2_kernel(const float* __restrict__ Pl,
                                                      const float* __restrict__ lbl,
                                                      const uint8_t* __restrict__ valid,
                                                      float* __restrict__ dPl,
                                                      float* __restrict__ ws, int P, int J,
                                                      float gcoef) {
  __shared__ float red[4];
  const int n = blockIdx.x;
  const size_t base = (size_t)n * P * J;
  const int chunk = (P * J + gridDim.y - 1) / gridDim.y;
  const int lo = blockIdx.y * chunk, hi = min(P * J, lo + chunk);
  float acc = 0.f;
  for (int idx = lo + threadIdx.x; idx < hi; idx += 256) {
    const int j = idx % J;
    const float d = Pl[base + idx] - lbl[base + idx];
    const float vm = valid[(size_t)n * J + j] ? 1.0f : 0.0f;
    acc = fmaf(vm * d, d, acc);
    if (dPl) dPl[base + idx] = gcoef * vm * d;
  }
  acc = block_sum256(acc, red);
  if (threadIdx.x == 0) ws[(size_t)n * gridDim.y + blockIdx.y] = acc;
}

__global__ __launch_bounds__(256) void zero_out_channels_kernel(const float* __restrict__ in,
                                                                const uint8_t* __restrict__ ch,
                                                                float* __restrict__ out,
                                                                size_t total, int C) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
    out[i] = ch[i % C] ? in[i] : 0.f;
}

// dX[n,p,c..c+3] = dz[n,c..c+3] / P: one 16-byte (fp32) or 8-byte (bf16) store per thread and element group
template <typename T>
__global__ __launch_bounds__(256) void spatial_mean_bwd_kernel(const float* __restrict__ dz, T* __restrict__ dX,
                                                               size_t total4, int P, int C4, float invP) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
    const size_t np = i / C4;
    const int c4 = (int)(i - np * C4);
    const float4 g = *reinterpret_cast<const float4*>(dz + ((np / P) * C4 + c4) * 4);
    const float4 v = make_float4(g.x * invP, g.y * invP, g.z * invP, g.w * invP);
    if constexpr (sizeof(T) == 2)
      *reinterpret_cast<uint2*>(dX + i * 4) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
    else
      *reinterpret_cast<float4*>(dX + i * 4) = v;
  }
}

__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ mask,
                                                           size_t n_elems, uint32_t thresh,
                                                           uint32_t k0, uint32_t k1) {
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q * 2 < n_elems;
       q += (size_t)gridDim.x * 256) {
    float m0, m1;
    rng_keep2(q * 2, k0, k1, thresh, m0, m1);
    mask[q * 2] = m0 != 0.f;
    if (q * 2 + 1 < n_elems) mask[q * 2 + 1] = m1 != 0.f;
  }
}

}  // namespace apa

using namespace apa;

extern "C" int apa_softmax_xent_fwd_bwd(const float* logits, const int64_t* labels, float* loss,
                                        float* G, float* probs, int64_t* pred, int N, int K,
                                        float wt, float grad_scale, void* stream) {
  if (!logits || !labels || !loss || N <= 0 || K <= 0) {
    set_error("apa_softmax_xent_fwd_bwd: null pointer or non-positive N=%d K=%d", N, K);
    return APA_ERR_INVALID_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  // tf.losses.softmax_cross_entropy with a scalar weight: sum(w * l) / (#non-zero weights) = w*mean
  const float lscale = wt / (float)N;
  const float gscale = wt * grad_scale / (float)N;
  if (!xent_row_half_wave(K)) {
    hipLaunchKernelGGL(softmax_xent_stream_kernel, dim3((N + 3) / 4), dim3(256), 0, st, logits,
                       labels, loss, G, probs, pred, N, K, gscale);
    APA_LAUNCH_CHECK("softmax_xent_stream_kernel");
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, st, loss + 1, loss, N, lscale);
    APA_LAUNCH_CHECK("sum_scale_kernel");
    return APA_OK;
  }
  // N <= 64: one launch; block 0 = losses + batch mean, blocks 1.. = gradients (when any are
  // wanted).  A 16-wave block covers 32 rows per pass (half a wave per row).
  const bool wide = G || probs;
  const int mode = xent_mean_slots32(N, K) ? (wide ? 2 : 1) : 0;
  int nb = mode == 1 ? 1 : (N + 31) / 32 + (mode == 2 ? 1 : 0);
  if (nb > 1024) nb = 1024;
#define APA_XENT(NV4)                                                                           \
  hipLaunchKernelGGL(softmax_xent_kernel<NV4>, dim3(nb), dim3(1024), 0, st, logits, labels, loss, \
                     G, probs, pred, N, K, gscale, lscale, mode)
  switch (xent_row_nv4(K)) {
    case 1: APA_XENT(1); break;
    case 2: APA_XENT(2); break;
    case 4: APA_XENT(4); break;
    default: APA_XENT(8);
  }
#undef APA_XENT
  APA_LAUNCH_CHECK("softmax_xent_kernel");
  if (mode == 0) {
    hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, st, loss + 1, loss, N, lscale);
    APA_LAUNCH_CHECK("sum_scale_kernel");
  }
  return APA_OK;
}

extern "C" size_t apa_pose_l2_workspace_bytes(int N, int P, int J) {
  (void)P; (void)J;
  return N > 0 ? (size_t)N * POSE_L2_MAX_SPLIT * sizeof(float) : 0;
}

extern "C" int apa_pose_l2_loss_fwd_bwd(const float* Pl, const float* lbl, const uint8_t* valid,
                                        float* loss, float* dPl, void* ws, size_t ws_bytes, int N,
                                        int P, int J, float wt, float grad_scale, void* stream) {
  if (!Pl || !lbl || !valid || !loss || !ws || N <= 0 || P <= 0 || J <= 0) {
    set_error("apa_pose_l2_loss_fwd_bwd: null pointer or non-positive dims N=%d P=%d J=%d", N, P, J);
    return APA_ERR_INVALID_ARG;
  }
  if (ws_bytes < apa_pose_l2_workspace_bytes(N, P, J)) {
    set_error("apa_pose_l2_loss_fwd_bwd: workspace too small (%zu < %zu)", ws_bytes,
              apa_pose_l2_workspace_bytes(N, P, J));
    return APA_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  // loss.py:53-62: 0.5*sum_hw(.)^2 / (N*H*W), then mean over n of the valid ones, summed over j
  const float denom = (float)N * (float)N * (float)P;
  const float gcoef = grad_scale * wt / denom;
  int split = (256 + N - 1) / N;                         // ~256 blocks
  if (split > POSE_L2_MAX_SPLIT) split = POSE_L2_MAX_SPLIT;
  while (split > 1 && (P * J + split - 1) / split < 256) --split;   // at least one element per thread
  hipLaunchKernelGGL(pose_l2_kernel, dim3(N, split), dim3(256), 0, st, Pl, lbl, valid, dPl,
                     static_cast<float*>(ws), P, J, gcoef);
  APA_LAUNCH_CHECK("pose_l2_kernel");
  hipLaunchKernelGGL(sum_scale_kernel, dim3(1), dim3(256), 0, st, static_cast<const float*>(ws),
                     loss, N * split, 0.5f * wt / denom);
  APA_LAUNCH_CHECK("sum_scale_kernel");
  return APA_OK;
}

extern "C" int apa_zero_out_channels(const float* in, const uint8_t* channels, float* out,
                                     size_t n_outer, int C, void* stream) {
  if (!in || !channels || !out || C <= 0) {
    set_error("apa_zero_out_channels: null pointer or C=%d", C);
    return APA_ERR_INVALID_ARG;
  }
  const size_t total = n_outer * (size_t)C;
  if (total == 0) return APA_OK;
  size_t nb = (total + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(zero_out_channels_kernel, dim3((unsigned)nb), dim3(256), 0,
                     static_cast<hipStream_t>(stream), in, channels, out, total, C);
  APA_LAUNCH_CHECK("zero_out_channels_kernel");
  return APA_OK;
}

extern "C" int apa_spatial_mean_bwd(const float* dz, void* dX, int N, int P, int C, int dtype, void* stream) {
  if (!dz || !dX || N <= 0 || P <= 0 || C <= 0) {
    set_error("apa_spatial_mean_bwd: null pointer or non-positive dimension");
    return APA_ERR_INVALID_ARG;
  }
  if (dtype != APA_DTYPE_F32 && dtype != APA_DTYPE_BF16) {
    set_error("apa_spatial_mean_bwd: unknown dtype %d", dtype);
    return APA_ERR_INVALID_ARG;
  }
  if (C % 4 != 0 || (reinterpret_cast<uintptr_t>(dz) & 15) || (reinterpret_cast<uintptr_t>(dX) & 15)) {
    set_error("apa_spatial_mean_bwd: C=%d must be a multiple of 4 and both buffers 16-byte aligned", C);
    return APA_ERR_UNSUPPORTED;
  }
  const size_t total4 = (size_t)N * P * (C / 4);
  size_t nb = (total4 + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == APA_DTYPE_BF16)
    hipLaunchKernelGGL(spatial_mean_bwd_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, dz,
                       static_cast<bf16_t*>(dX), total4, P, C / 4, 1.0f / (float)P);
  else
    hipLaunchKernelGGL(spatial_mean_bwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, dz,
                       static_cast<float*>(dX), total4, P, C / 4, 1.0f / (float)P);
  APA_LAUNCH_CHECK("spatial_mean_bwd_kernel");
  return APA_OK;
}

extern "C" int apa_dropout_mask(uint8_t* mask, size_t n_elems, float keep_prob, uint64_t seed,
                                uint64_t offset, void* stream) {
  if (!mask) {
    set_error("apa_dropout_mask: null mask");
    return APA_ERR_INVALID_ARG;
  }
  if (n_elems == 0) return APA_OK;
  uint32_t k0, k1;
  rng_key(seed, offset, &k0, &k1);
  size_t nb = (n_elems / 2 + 255) / 256;
  if (nb > 8192) nb = 8192;
  if (nb < 1) nb = 1;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)nb), dim3(256), 0,
                     static_cast<hipStream_t>(stream), mask, n_elems, keep_thresh(keep_prob), k0, k1);
  APA_LAUNCH_CHECK("dropout_mask_kernel");
  return APA_OK;
}
