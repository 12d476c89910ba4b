// apa_pc.hip -- per-class bottom-up maps (cfg.NET..._PER_CLASS, nets_factory.py:257 of the reference model): M == K.
// Z and T are two real GEMMs here ([N*P, C] x [C, K], apa_gemm.hip); the activation / spatial mean and their
// gradients are small fused elementwise-reduction kernels over the [N,P,K] tensors.  K <= 64 (bf16, Xatt == X) takes
// the HBM-bound kernels of apa_pc_fused.hip instead; the host dispatch of both is here.
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

template <typename T> __device__ __forceinline__ void stf(T* p, size_t i, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, size_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void stf<bf16_t>(bf16_t* p, size_t i, float v) {
  p[i].v = (uint16_t)f32_to_bf16_bits(v);
}

// Zero-padded copies of up to three [rows][K] fp32 parameters as [rows][Kp] in ONE launch; a segment
// marked bf16 is also converted, so that the bf16 products take the DMA-staged MFMA kernels (both
// operands bf16, whole 64-wide k tiles).
struct PcPadSegs {
  const float* src[3];
  void* dst[3];
  long end[3];     // cumulative element counts (rows * Kp)
  int bf16[3];
  int ld[3];       // row stride of dst in elements (>= Kp: two parameters can share rows as [Wt | Wa], see PcCall::cat)
  int n;
};
// Xd = X * mask / keep (bf16), the same counter-based mask as everywhere else (flat index r*C + c); block `bid` of `nb`
struct PcDropArgs {
  const bf16_t* X; bf16_t* Xd; size_t n8; float inv_keep; uint32_t thresh; uint64_t seed, offset;
  const uint64_t* offset_dev; unsigned nblocks;     // nblocks == 0: none
  uint8_t* bits;                                    // optional: the keep decisions, bit (e & 7) of byte e >> 3
};
__device__ __forceinline__ void pc_dropout_block(const PcDropArgs& a, unsigned bid, unsigned nb) {
  uint32_t k0, k1;
  rng_key_dev_x(a.seed, a.offset_dev ? *a.offset_dev : a.offset, a.thresh, k0, k1);
  for (size_t v = (size_t)bid * 256 + threadIdx.x; v < a.n8; v += (size_t)nb * 256) {
    float x[8];
    Vec<bf16_t>::unpack(ld16(a.X + v * 8), x);
    uint32_t byte = 0;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      float m0, m1;
      rng_keep2_x(v * 8 + e, k0, k1, a.thresh, m0, m1);
      x[e] *= m0 * a.inv_keep;
      x[e + 1] *= m1 * a.inv_keep;
      byte |= (m0 != 0.f ? 1u : 0u) << e;
      byte |= (m1 != 0.f ? 1u : 0u) << (e + 1);
    }
    st16(a.Xd + v * 8, Vec<bf16_t>::pack(x));
    if (a.bits) a.bits[v] = (uint8_t)byte;
  }
}
// One thread per 8 output columns (Kp is a multiple of 8): 16-byte stores and 8x fewer waves -- the
// one-element-per-thread form was bound by wave dispatch (28 k waves for 1.8 M elements: 8.4 us).
// Round 4: the forward call's dropout(X) materialisation rides on the same launch (blocks past the padding work):
// two launches at the floor (6.1 + 8.8 us at K = 393) become one.
__global__ __launch_bounds__(256) void pc_pad_kernel(PcPadSegs sg, int K, int Kp, PcDropArgs dr) {
  const unsigned npad = gridDim.x - dr.nblocks;
  if (blockIdx.x >= npad) { pc_dropout_block(dr, blockIdx.x - npad, dr.nblocks); return; }
  const unsigned idx = blockIdx.x * 256u + threadIdx.x;       // vector index: 8 elements each
  if (sg.n == 0 || idx >= (unsigned)(sg.end[sg.n - 1] >> 3)) return;
  int s = 0;
  unsigned base = 0;
  if (sg.n > 1 && idx >= (unsigned)(sg.end[0] >> 3)) { s = 1; base = (unsigned)(sg.end[0] >> 3); }
  if (sg.n > 2 && idx >= (unsigned)(sg.end[1] >> 3)) { s = 2; base = (unsigned)(sg.end[1] >> 3); }
  const unsigned j = idx - base;
  const unsigned kp8 = (unsigned)Kp >> 3;
  const unsigned r = j / kp8;
  const int k0 = (int)(j - r * kp8) * 8;
  const float* __restrict__ src = sg.src[s] + (size_t)r * K;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (k0 + e) < K ? src[k0 + e] : 0.f;
  const size_t doff = (size_t)r * sg.ld[s] + k0;
  if (sg.bf16[s]) {
    st16(static_cast<bf16_t*>(sg.dst[s]) + doff, Vec<bf16_t>::pack(v));
  } else {
    float4* d = reinterpret_cast<float4*>(static_cast<float*>(sg.dst[s]) + doff);
    d[0] = make_float4(v[0], v[1], v[2], v[3]);
    d[1] = make_float4(v[4], v[5], v[6], v[7]);
  }
}
struct PcPadList {
  PcPadSegs sg;
  PcPadList() { sg.n = 0; }
  void add(const float* W, void* Wp, int rows, int Kp, bool to_bf16, int ld = 0) {
    const int i = sg.n++;
    sg.src[i] = W; sg.dst[i] = Wp; sg.bf16[i] = to_bf16 ? 1 : 0; sg.ld[i] = ld > 0 ? ld : Kp;
    sg.end[i] = (i ? sg.end[i - 1] : 0) + (long)rows * Kp;
  }
  // (an empty list -- APA_FLAG_WEIGHT_IMAGES: the padded weights are kept by the caller -- launches the dropout
  // blocks alone, or nothing)
  void launch(int K, int Kp, hipStream_t st, const PcDropArgs* drop = nullptr) const {
    PcDropArgs dr = {nullptr, nullptr, 0, 1.f, 0, 0, 0, nullptr, 0, nullptr};
    if (drop) dr = *drop;
    const unsigned npad = sg.n ? (unsigned)(((sg.end[sg.n - 1] >> 3) + 255) / 256) : 0u;
    if (PcTrace* t = pc_trace()) {
      const bool bwd = t->phase == 2;
      (bwd ? t->pad_bwd : t->pad_fwd) = (npad + dr.nblocks) ? 1 : 0;
      (bwd ? t->pad_segs_bwd : t->pad_segs_fwd) = sg.n;
      (bwd ? t->pad_drop_bwd : t->pad_drop_fwd) = dr.nblocks ? 1 : 0;
    }
    if (npad + dr.nblocks == 0) return;
    hipLaunchKernelGGL(pc_pad_kernel, dim3(npad + dr.nblocks), dim3(256), 0, st, sg, K, Kp, dr);
  }
  // the images of this list as apa_weight_image maps: element (c, k) of segment i -> dst[c * ld + k]
  int describe(const int* roles, int K, apa_weight_image* out) const {
    for (int i = 0; i < sg.n; ++i) {
      apa_weight_image& m = out[i];
      m.dst = sg.dst[i]; m.role = roles[i]; m.is_f32 = sg.bf16[i] ? 0 : 1; m.cols = K; m.c_shift = 0;
      m.a = sg.ld[i]; m.b = 0; m.d = 1; m.e = 0;
    }
    return sg.n;
  }
};

constexpr int PC_PG = 16;   // pixel groups per block of the per-class activation passes
constexpr int PC_MAX_PSPLIT = 8;   // pixel splits (grid.z) of the backward activation pass
// pixel splits of pc_bwd_act_kernel: enough blocks to put one on most CUs; the spatial softmax needs the whole image
static int pc_bwd_act_psplit(int N, int kgroups, int P, int act) {
  if (act == 2) return 1;
  int ps = (256 + N * kgroups - 1) / (N * kgroups);   // HMDB-51 shape, N = 32: 7.9 -> 4.9 us
  if (ps > PC_MAX_PSPLIT) ps = PC_MAX_PSPLIT;
  while (ps > 1 && (P + ps - 1) / ps < PC_PG) --ps;      // at least one pixel per pixel group
  return ps < 1 ? 1 : ps;
}
__device__ __forceinline__ float pc_colsum(const float (&red)[PC_PG][64], int kk) {
  float s = 0.f;
#pragma unroll
  for (int g = 0; g < PC_PG; ++g) s += red[g][kk];   // fixed order
  return s;
}
__device__ __forceinline__ float pc_colmax(const float (&red)[PC_PG][64], int kk) {
  float m = red[0][kk];
#pragma unroll
  for (int g = 1; g < PC_PG; ++g) m = fmaxf(m, red[g][kk]);
  return m;
}

// forward activation + spatial mean.  grid (N, ceil(K/64)); 1024 threads = 64 classes x PC_PG pixel
// groups (16 waves per block: these passes are short dependent-load chains, 4 groups measured 27 us
// at K = 51 where 32 blocks of 4 waves cannot hide any latency)
//   A[n,p,k] = f(Z[n,p,k]);  logits[n,k] = (1/P) sum_p A * T;  optional TopDownAttention copy
// xe (one-call train step, K <= 64 so that one block holds the whole row): the row's softmax cross-entropy on the
// logits it has just reduced -- G[n,:] = gscale (softmax - onehot), loss[1 + n] = xent_n (src/loss.py:74-80); the batch
// mean is finished by the tail of the dW reduce launch.  One launch (4.7 us at the latency floor) less per step.
template <typename T>
__global__ __launch_bounds__(1024) void pc_fwd_act_kernel(const float* __restrict__ Z, int ldz,
                                                         const float* __restrict__ Tm,
                                                         float* __restrict__ att,
                                                         float* __restrict__ logits,
                                                         T* __restrict__ topdown, int P, int K,
                                                         int act, PcXent xe) {
  __shared__ float red[PC_PG][64];
  const int n = blockIdx.x;
  const int kk = threadIdx.x & 63, pg = threadIdx.x >> 6;
  const int k = blockIdx.y * 64 + kk;
  const bool ok = k < K;
  const size_t rbase = (size_t)n * P;
  float m = -INFINITY, l = 1.f;
  if (act == 2) {  // spatial softmax over p (tf.nn.softmax: max-subtracted)
    if (ok)
      for (int p = pg; p < P; p += PC_PG) m = fmaxf(m, Z[(rbase + p) * ldz + k]);
    red[pg][kk] = m;
    __syncthreads();
    m = pc_colmax(red, kk);
    __syncthreads();
    float s = 0.f;
    if (ok)
      for (int p = pg; p < P; p += PC_PG) s += expf(Z[(rbase + p) * ldz + k] - m);
    red[pg][kk] = s;
    __syncthreads();
    l = pc_colsum(red, kk);
    __syncthreads();
  }
  const float invl = 1.0f / l;
  float acc = 0.f;
  if (ok) {
    // four pixels per round, their eight loads issued before the first use (a plain loop is one
    // dependent round trip per pixel)
    for (int p0 = pg; p0 < P; p0 += 4 * PC_PG) {
      float z[4], t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t pr = rbase + min(p0 + u * PC_PG, P - 1);   // surplus slots re-read the last pixel
        z[u] = Z[pr * ldz + k];
        t[u] = Tm[pr * K + k];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * PC_PG;
        if (p < P) {
          float a = z[u];
          if (act == 2) a = expf(z[u] - m) * invl;
          else if (act == 1) a = fmaxf(z[u], 0.f);
          att[(rbase + p) * K + k] = a;
          if (topdown) stf<T>(topdown, (rbase + p) * K + k, t[u]);
          acc = fmaf(a, t[u], acc);
        }
      }
    }
  }
  red[pg][kk] = acc;
  __syncthreads();
  __shared__ float lrow[64];
  if (pg == 0) {                       // wave 0: lane kk owns class k
    const float lg = ok ? pc_colsum(red, kk) / (float)P : -INFINITY;
    if (ok) logits[(size_t)n * K + k] = lg;
    lrow[kk] = lg;
  }
  if (xe.labels) {                     // (block-uniform; gridDim.y == 1 and 4 <= K <= 64: lrow holds the whole row)
    __syncthreads();
    if (pg == 0) {
      pc_row_xent(lrow, n, K, xe, true, nullptr);
    }
  }
}

// one-call step, generic K > 64 path: where the gradient row G[n, :] comes from -- memory (row_logits == nullptr) or the
// logits row the forward activation pass left (4 <= K <= 1024).  (The K <= 64 path takes its cross-entropy in
// pc_bwd_dx_kernel, apa_pc_fused.hip.)
struct PcDefer { PcXent xe; const float* row_logits; };
// backward of the same: dT = G*A/P, dA = G*T/P, dZ = act'(dA); column partials for dbt / dba.
// dT/dZ are written with leading dimension Kp (pad columns zeroed) in the intermediate dtype.
template <typename T>
__global__ __launch_bounds__(1024) void pc_bwd_act_kernel(const float* __restrict__ G,
                                                         const float* __restrict__ att,
                                                         const float* __restrict__ Tm,
                                                         T* __restrict__ dT, T* __restrict__ dZ,
                                                         float* __restrict__ pdbt,
                                                         float* __restrict__ pdba, int P, int K,
                                                         int Kp, int act, int ldg, PcDefer df) {
  // dT / dZ: [R][ldg] with Kp written columns each (ldg = Kp, or 2*Kp when the two are interleaved as
  // one [R][dT | dZ] operand for apa_pc_fused.hip)
  __shared__ float red[PC_PG][64];
  __shared__ float red2[PC_PG][64];
  const int n = blockIdx.x;
  const int kk = threadIdx.x & 63, pg = threadIdx.x >> 6;
  const int k = blockIdx.y * 64 + kk;
  const bool ok = k < K;
  const bool pad = !ok && k < Kp;
  const size_t rbase = (size_t)n * P;
  const float invP = 1.0f / (float)P;
  // grid.z > 1 (identity / relu only: no sum over the image's pixels is needed): block z owns a contiguous
  // share of the pixels and its own partial row -- N x 1 blocks of 16 waves were 32 CUs' worth of latency chains
  const int pchunk = (P + gridDim.z - 1) / gridDim.z;
  const int p_lo = blockIdx.z * pchunk, p_hi = min(P, p_lo + pchunk);
  // the first two pixels of every thread are requested before the gradient row is known: with the cross-entropy
  // taken in this launch (df) the two round trips would otherwise be serial (measured 7.4 -> 14.4 us at K = 393)
  constexpr int NPRE = 2;
  float pa[NPRE], pt[NPRE];
#pragma unroll
  for (int u = 0; u < NPRE; ++u) {
    const int p = p_lo + pg + u * PC_PG;
    pa[u] = pt[u] = 0.f;
    if (ok && p < p_hi) { pa[u] = att[(rbase + p) * K + k]; pt[u] = Tm[(rbase + p) * K + k]; }
  }
  float g;
  if (df.row_logits) {
    // K > 64 (generic path), one-call step: every block takes its image's cross-entropy itself from the logits row
    // (softmax_xent_kernel's arithmetic: bit-identical G); block (y, z) = (0, 0) writes G[n, :] and loss[1 + n]
    __shared__ float growf[1024];
    if (pg == 0) pc_row_xent_any(df.row_logits + (size_t)n * K, n, K, df.xe, blockIdx.y == 0 && blockIdx.z == 0, growf);
    __syncthreads();
    g = ok ? growf[k] * invP : 0.f;
  } else {
    g = ok ? G[(size_t)n * K + k] * invP : 0.f;
  }
  float corr = 0.f;
  if (act == 2) {  // sum_p A * dA (host: grid.z == 1)
    float s = 0.f;
    if (ok)
      for (int p = pg; p < P; p += PC_PG) s = fmaf(att[(rbase + p) * K + k], g * Tm[(rbase + p) * K + k], s);
    red[pg][kk] = s;
    __syncthreads();
    corr = pc_colsum(red, kk);
    __syncthreads();
  }
  float sdt = 0.f, sdz = 0.f;
  auto pixel = [&](int p, float a, float tm) {
    if (ok) {
      const float dA = g * tm;
      const float dt = g * a;
      float dz = dA;
      if (act == 2) dz = a * (dA - corr);
      else if (act == 1) dz = a > 0.f ? dA : 0.f;
      stf<T>(dT, (rbase + p) * ldg + k, dt);
      stf<T>(dZ, (rbase + p) * ldg + k, dz);
      sdt += dt;
      sdz += dz;
    } else if (pad) {
      stf<T>(dT, (rbase + p) * ldg + k, 0.f);
      stf<T>(dZ, (rbase + p) * ldg + k, 0.f);
    }
  };
#pragma unroll
  for (int u = 0; u < NPRE; ++u) {
    const int p = p_lo + pg + u * PC_PG;
    if (p < p_hi) pixel(p, pa[u], pt[u]);
  }
  for (int p = p_lo + pg + NPRE * PC_PG; p < p_hi; p += PC_PG) {   // (batching the loads four pixels deep, as in
    float a = 0.f, tm = 0.f;                                        //  the forward pass, measured slower here)
    if (ok) { a = att[(rbase + p) * K + k]; tm = Tm[(rbase + p) * K + k]; }
    pixel(p, a, tm);
  }
  red[pg][kk] = sdt;
  red2[pg][kk] = sdz;
  __syncthreads();
  if (pg == 0 && ok) {
    const size_t prow = (size_t)n * gridDim.z + blockIdx.z;
    pdbt[prow * 2 * K + k] = pc_colsum(red, kk);            // one [N * grid.z][2K] partial matrix: dbt | dba
    pdba[prow * 2 * K + k] = pc_colsum(red2, kk);
  }
}

struct PcPlan {
  long R;
  int Kp;
  size_t off_wap, off_wtp, off_bap, off_z, off_dt, off_dz, off_pdbt, off_pdba, off_gemm, gemm_half, off_xd, off_bits, off_fused, total;
};
static PcPlan pc_plan(int N, int P, int C, int Ca, int K, int dtype) {
  PcPlan pl;
  pl.R = (long)N * P;
  // bf16: whole 64-wide k tiles for the products that contract over the class axis (dX)
  pl.Kp = dtype == APA_DTYPE_BF16 ? (K + 63) / 64 * 64 : (K + 7) / 8 * 8;
  size_t off = 0;
  pl.off_wap = off;  off += align_up((size_t)Ca * pl.Kp * 4, 256);
  pl.off_wtp = off;  off += align_up((size_t)C * pl.Kp * 4, 256);
  pl.off_bap = off;  off += align_up((size_t)pl.Kp * 4, 256);
  pl.off_z = off;    off += align_up((size_t)pl.R * pl.Kp * 4, 256);
  pl.off_dt = off;   off += align_up((size_t)pl.R * pl.Kp * dt_size(dtype), 256);
  pl.off_dz = off;   off += align_up((size_t)pl.R * pl.Kp * dt_size(dtype), 256);
  // [N * splits][2K]: dbt | dba partials ([ceil(R / 128)][2K] from pc_bwd_dx_kernel)
  pl.off_pdbt = off; off += align_up(((size_t)N * PC_MAX_PSPLIT + (size_t)pl.R / 128 + 1) * 2 * K * 4, 256);
  pl.off_pdba = pl.off_pdbt + (size_t)K * 4;
  const int cm = C > Ca ? C : Ca;
  {
    // split-K partials cover the padded width; two buffers: the twin products (Z | T, dWt | dWa) share a launch.
    // Sized by the splits the launches will pick (the same calls as in pc_forward / pc_backward)
    int sdw = gemm_pick_splits(C, K, (int)pl.R);
    const int sdw2 = gemm_pick_splits(Ca, K, (int)pl.R);
    if (sdw2 > sdw) sdw = sdw2;
    int sfw = gemm_pick_splits((int)pl.R, pl.Kp, C);
    const int sfw2 = gemm_pick_splits((int)pl.R, pl.Kp, Ca);
    if (sfw2 > sfw) sfw = sfw2;
    if (sfw > 8) sfw = 8;
    size_t g = gemm_ws_bytes(cm, pl.Kp, sdw);
    const size_t g2 = gemm_ws_bytes((int)pl.R, pl.Kp, sfw);   // split-K of the skinny forward products
    if (g2 > g) g = g2;
    pl.gemm_half = align_up(g, 256);
    pl.off_gemm = off; off += 2 * pl.gemm_half + 256;
  }
  // bf16 training: dropout(X) materialised once per call, so the MFMA GEMMs that consume it can DMA
  // their operands (the generic kernel applies the mask while staging through registers)
  pl.off_xd = off;   off += dtype == APA_DTYPE_BF16 ? align_up((size_t)pl.R * C * 2, 256) : 0;
  // ... and its keep decisions as bits: the one-launch dX product masks its accumulators with them (PcCall::cat)
  pl.off_bits = off; off += dtype == APA_DTYPE_BF16 ? align_up((size_t)pl.R * C / 8 + 16, 256) : 0;
  // K <= 64, bf16: operands of the HBM-bound fused kernels (apa_pc_fused.hip)
  pl.off_fused = off; off += (dtype == APA_DTYPE_BF16 && K <= 64 && Ca == C) ? pc_fused_ws_bytes(N, P, C) : 0;
  pl.total = off;
  return pl;
}

thread_local PcTrace* g_pc_trace = nullptr;
void pc_plan_offsets(int N, int P, int C, int Ca, int K, int dtype, size_t* out) {
  const PcPlan pl = pc_plan(N, P, C, Ca, K, dtype);
  const size_t v[16] = {(size_t)pl.R, (size_t)pl.Kp, pl.off_wap, pl.off_wtp, pl.off_bap, pl.off_z, pl.off_dt, pl.off_dz,
                        pl.off_pdbt, pl.off_pdba, pl.off_gemm, pl.gemm_half, pl.off_xd, pl.off_bits, pl.off_fused,
                        pl.total};
  for (int i = 0; i < 16; ++i) out[i] = v[i];
}
int pc_bwd_act_psplit_host(int N, int kgroups, int P, int act) { return pc_bwd_act_psplit(N, kgroups, P, act); }

size_t pc_workspace_bytes(int N, int P, int C, int Ca, int K, int dtype) {
  return pc_plan(N, P, C, Ca, K, dtype).total;
}

// What pc_weight_images, pc_forward and pc_backward each derive from the call's shape, flags and workspace, once.
struct PcCall {
  int N, P, C, Ca, K, dtype; unsigned flags; float keep_prob;
  PcPlan pl; char* w;                   // the workspace and its carve
  int Kp, R, tdt;
  bool wb16;                            // padded weights stored as bf16
  bool dma;     // the all-bf16 DMA route: 16-byte addressable bf16 features (else scalar staging, masked while staging)
  // ... with attention and top-down weights of the same height (Ca == C): the padded bf16 weights lie as ONE
  // [C][Wt (Kp) | Wa (Kp)] image and [dT | dZ] as one [R][2 Kp] image, so that
  //     dX = (dT . Wt^T) * mask/keep + dZ . Wa^T
  // is ONE product over the concatenated contraction (the wide kernel's mid-contraction mask) instead of a product plus
  // a read-modify-write product over the 25.7 MB result.  The forward / dW products read the halves with ld = 2 Kp.
  bool cat;
  int ldw;                              // row stride of the padded weights and of [dT | dZ]
  void* WtP; void* WaP; float* baP;     // (WtP / WaP: bf16 when they are padded at all)
  float* Z; float* pdbt; float* pdba;   // pdbt / pdba: one [rows][2K] matrix of dbt | dba block partials
  bool train; int act;                  // act: 0 identity, 1 relu, 2 spatial softmax attention
  RngKeyArgs key;                       // the dropout key as the kernels take it (rng_resolve)
  uint64_t* bump;                       // APA_FLAG_RNG_DEVICE: the counter the backward call's LAST launch advances
  // a gathered call (PoolCall::fc): X is the cache, and the two kernels that read it (pc_fwd_zt_dma_kernel,
  // pc_bwd_dw_kernel) run their gathered instances on `ga`.  status / labels: filled by pc_forward alone -- the backward
  // pass reports and copies nothing.  Fused route only: the generic one materialises dropout(X) from a dense X
  bool gather; PcGather ga;
  const PcGather* gather_arg() const { return gather ? &ga : nullptr; }
};
int64_t* pc_gathered_labels(void* ws, int N, int P, int C, int Ca, int K, int dtype) {
  return reinterpret_cast<int64_t*>(static_cast<char*>(ws) + pc_plan(N, P, C, Ca, K, dtype).off_xd);
}
// X == nullptr (pc_weight_images: which features will come is not known): the layout of 16-byte addressable ones
static PcCall pc_call(const PoolCall& d, const void* X) {
  const int N = d.N, P = d.P, C = d.C, Ca = d.Ca, K = d.K, dtype = d.dtype;
  const unsigned flags = d.flags;
  const float keep_prob = d.keep_prob;
  const uint64_t seed = d.seed, offset = d.offset;
  void* const ws = d.ws;
  PcCall c;
  c.N = N; c.P = P; c.C = C; c.Ca = Ca; c.K = K; c.dtype = dtype; c.flags = flags; c.keep_prob = keep_prob;
  c.pl = pc_plan(N, P, C, Ca, K, dtype); c.w = static_cast<char*>(ws);
  c.Kp = c.pl.Kp; c.R = (int)c.pl.R; c.tdt = dt_code(dtype); c.wb16 = dtype == APA_DTYPE_BF16;
  c.dma = c.wb16 && C % 8 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  c.cat = c.dma && Ca == C; c.ldw = c.cat ? 2 * c.Kp : c.Kp;
  c.WtP = c.w + c.pl.off_wtp;
  c.WaP = c.cat ? static_cast<void*>(static_cast<bf16_t*>(c.WtP) + c.Kp) : static_cast<void*>(c.w + c.pl.off_wap);
  c.baP = reinterpret_cast<float*>(c.w + c.pl.off_bap); c.Z = reinterpret_cast<float*>(c.w + c.pl.off_z);
  c.pdbt = reinterpret_cast<float*>(c.w + c.pl.off_pdbt); c.pdba = reinterpret_cast<float*>(c.w + c.pl.off_pdba);
  c.train = (flags & APA_FLAG_TRAIN) && keep_prob < 1.0f;
  c.act = (flags & APA_FLAG_SOFTMAX_ATT) ? 2 : (flags & APA_FLAG_RELU_ATT) ? 1 : 0;
  c.key = rng_resolve(flags, keep_prob, seed, offset);
  c.bump = (c.train && (flags & APA_FLAG_RNG_DEVICE)) ? reinterpret_cast<uint64_t*>(static_cast<uintptr_t>(offset))
                                                       : nullptr;
  c.gather = d.fc != nullptr;
  c.ga = PcGather{M1Gather{nullptr, 0, nullptr, nullptr, nullptr}, P};
  if (c.gather) { c.ga.g.index = d.fc->index; c.ga.g.T = d.fc->cache_images; }
  return c;
}
// A gathered call is the fused route's or nobody's: cache_check (apa_capi.hip) admits exactly what pc_fused_supported
// serves, and a call built inside the library that gets here without it is refused before anything is queued.
static int pc_gather_refuse(const char* who) {
  set_error("%s: a feature cache feeds the fused per-class route only (bf16, Xatt == X, K <= 64, C %% 256 == 0, "
            "C <= 8192, 16-byte aligned, no replayed mask)", who);
  return APA_ERR_UNSUPPORTED;
}

// the padding launch; training on the DMA route: + the materialised dropout(X) and its keep bits, as extra blocks
static int pc_pad_launch(const PcCall& c, const PcPadList& pads, const void* X, hipStream_t st) {
  const size_t n8 = (size_t)c.pl.R * c.C / 8;
  size_t nb = (n8 + 255) / 256;
  if (nb > 4096) nb = 4096;
  const PcDropArgs dr = {static_cast<const bf16_t*>(X), reinterpret_cast<bf16_t*>(c.w + c.pl.off_xd), n8,
                         1.0f / c.keep_prob, c.key.thresh, c.key.seed, c.key.offset, c.key.offset_dev, (unsigned)nb,
                         reinterpret_cast<uint8_t*>(c.w + c.pl.off_bits)};
  pads.launch(c.K, c.Kp, st, c.dma && c.train ? &dr : nullptr);
  APA_LAUNCH_CHECK("pc_pad_kernel");
  return APA_OK;
}

static void set_dropout(GemmDesc& g, bool on_a, bool on_c, const PcCall& c) {
  g.drop_a = on_a; g.drop_c = on_c;
  g.inv_keep = 1.0f / c.keep_prob;
  g.thresh = c.key.thresh; g.seed = c.key.seed; g.offset = c.key.offset; g.offset_dev = c.key.offset_dev;
}

// the activation passes for the feature type of the call (`topdown`, dT / dZ are of that type)
static int pc_fwd_act(const PcCall& c, const float* Tsave, float* att, float* logits, void* topdown, const PcXent& xe,
                      hipStream_t st) {
  const dim3 grid(c.N, (c.K + 63) / 64);
  if (c.dtype == APA_DTYPE_F32)
    hipLaunchKernelGGL(pc_fwd_act_kernel<float>, grid, dim3(64 * PC_PG), 0, st, c.Z, c.Kp, Tsave, att, logits,
                       static_cast<float*>(topdown), c.P, c.K, c.act, xe);
  else
    hipLaunchKernelGGL(pc_fwd_act_kernel<bf16_t>, grid, dim3(64 * PC_PG), 0, st, c.Z, c.Kp, Tsave, att, logits,
                       static_cast<bf16_t*>(topdown), c.P, c.K, c.act, xe);
  APA_LAUNCH_CHECK("pc_fwd_act_kernel");
  return APA_OK;
}
// ps: pixel splits (out); ldg: row stride of dT / dZ
static int pc_bwd_act(const PcCall& c, const float* G, const float* att, const float* Tsave, void* dT, void* dZ,
                      int ldg, const PcDefer& df, int* ps, hipStream_t st) {
  *ps = pc_bwd_act_psplit(c.N, (c.Kp + 63) / 64, c.P, c.act);
  const dim3 grid(c.N, (c.Kp + 63) / 64, *ps);
  if (c.dtype == APA_DTYPE_F32)
    hipLaunchKernelGGL(pc_bwd_act_kernel<float>, grid, dim3(64 * PC_PG), 0, st, G, att, Tsave, static_cast<float*>(dT),
                       static_cast<float*>(dZ), c.pdbt, c.pdba, c.P, c.K, c.Kp, c.act, ldg, df);
  else
    hipLaunchKernelGGL(pc_bwd_act_kernel<bf16_t>, grid, dim3(64 * PC_PG), 0, st, G, att, Tsave,
                       static_cast<bf16_t*>(dT), static_cast<bf16_t*>(dZ), c.pdbt, c.pdba, c.P, c.K, c.Kp, c.act, ldg,
                       df);
  APA_LAUNCH_CHECK("pc_bwd_act_kernel");
  return APA_OK;
}

// APA_FLAG_WEIGHT_IMAGES: every image pc_forward / pc_backward would otherwise prepare per call, built once here
// (for 16-byte aligned features: the [Wt | Wa] concatenation of PcCall::cat) and described for the optimiser's launch.
// K <= 64 (bf16, Ca == C) builds BOTH sets -- the fused kernels' and the padded GEMM operands -- because which path a
// call takes also depends on its Xatt (== X or not) and on its dropout source.
int pc_weight_images(const PoolCall& d, const float* Wa, const float* ba, const float* Wt, const float* bt,
                     apa_weight_image* maps, int* nmaps) {
  const int N = d.N, P = d.P, C = d.C, Ca = d.Ca, K = d.K;
  hipStream_t const st = d.st;
  const PcCall c = pc_call(d, nullptr);
  const int Kp = c.Kp;
  int n = 0;
  PcTrace* tr = pc_trace();
  if (tr) { tr->phase = 3; tr->wimg_cat = c.cat ? 1 : 0; }
  {
    PcPadList pads;
    pads.add(Wa, c.WaP, Ca, Kp, c.wb16, c.ldw);
    pads.add(ba, c.baP, 1, Kp, false);
    pads.add(Wt, c.WtP, C, Kp, c.wb16, c.ldw);
    pads.launch(K, Kp, st);
    APA_LAUNCH_CHECK("pc_pad_kernel");
    if (maps) {
      const int roles[3] = {APA_WIMG_ROLE_WA, APA_WIMG_ROLE_BA, APA_WIMG_ROLE_WT};
      n += pads.describe(roles, K, maps + n);
    }
  }
  if (c.wb16 && Ca == C && K <= 64 && C % 256 == 0) {   // pc_fused_supported, minus X
    const PcFusedWs f = pc_fused_carve(c.w + c.pl.off_fused, N, P, C);
    if (tr) tr->wimg_fused = 1;
    const int rc = pc_fused_prep(f, Wa, Wt, ba, bt, C, K, st, nullptr, true);
    if (rc != APA_OK) return rc;
    const int rcz = zero_fill(f.bits_tag, 64, st);          // whatever the keep-bit map held: nobody may believe it
    if (rcz != APA_OK) return rcz;
    if (maps) {
      auto put = [&](int role, void* dst, int f32, int sh, int a, int b, int d, int e) {
        apa_weight_image& m = maps[n++];
        m.dst = dst; m.role = role; m.is_f32 = f32; m.cols = K; m.c_shift = sh; m.a = a; m.b = b; m.d = d; m.e = e;
      };
      // WcatT [C/64][128][64]: tile c >> 6, row = column (Wa: k, Wt: 64 + k), position c & 63
      put(APA_WIMG_ROLE_WA, f.WcatT, 0, 6, 128 * 64, 1, 64, 0);
      put(APA_WIMG_ROLE_WT, f.WcatT, 0, 6, 128 * 64, 1, 64, 64 * 64);
      // Wcat2 [C][128]: Wt | Wa
      put(APA_WIMG_ROLE_WT, f.Wcat2, 0, 0, 128, 0, 1, 0);
      put(APA_WIMG_ROLE_WA, f.Wcat2, 0, 0, 128, 0, 1, 64);
      // bcat f32 [128]: ba | bt
      put(APA_WIMG_ROLE_BA, f.bcat, 1, 0, 0, 0, 1, 0);
      put(APA_WIMG_ROLE_BT, f.bcat, 1, 0, 0, 0, 1, 64);
    }
  }
  if (nmaps) *nmaps = n;
  if (tr) tr->wimg_maps = n;
  return APA_OK;
}

// K <= 64 (HMDB-51): Z | T in ONE pass over X, dropout applied on the way into LDS (apa_pc_fused.hip)
static int pc_forward_fused(const PcCall& c, const M1Fwd& io, hipStream_t st, M1Xent* xf) {
  const int N = c.N, P = c.P, C = c.C, K = c.K, R = c.R;
  const void* const X = io.X;
  const float *const Wa = io.Wa, *const ba = io.ba, *const Wt = io.Wt, *const bt = io.bt;
  float *const logits = io.logits, *const att = io.att, *const Tsave = io.zsave;
  void* const topdown = io.topdown;
  PcTrace* tr = pc_trace();
  if (tr) tr->path_fwd = PC_PATH_FUSED;
  const PcFusedWs f = pc_fused_carve(c.w + c.pl.off_fused, N, P, C);
  // training: the weight-preparation launch also writes the step's keep bits (its 128 weight blocks leave half
  // the chip idle), and the product kernel DMAs them instead of hashing on its critical chain
  // Round 5, the one-call train step with caller-kept weight images: NO preparation launch -- the keep bits of this
  // step were written by the previous step's last launch (pc_dw_reduce_kernel's extra blocks) and are believed iff
  // their tag says so; else the forward kernel hashes them itself (first step on a workspace, a jump of the offset)
  const bool tagged = c.train && (c.flags & APA_FLAG_WEIGHT_IMAGES) && xf && xf->labels;
  const bool prebits = c.train && !tagged;
  const PcPrepBits pb = {(size_t)R * C, c.keep_prob, c.key.seed, c.key.offset, c.key.offset_dev};
  int rc = APA_OK;
  if (!tagged)
    rc = pc_fused_prep(f, Wa, Wt, ba, bt, C, K, st, prebits ? &pb : nullptr, !(c.flags & APA_FLAG_WEIGHT_IMAGES));
  if (rc != APA_OK) return rc;
  const bool xent_here = xf && xf->labels && xf->G && xf->loss && !xf->probs && K >= 4 && K <= 64;
  // identity / relu attention: the activation pass rides on the product's epilogue (a block's 32 rows touch at most
  // two images when P >= 32); the softmax needs the whole image's Z first and keeps its own launch
  const bool fold = c.act != 2 && !topdown && P >= 32;
  const PcFwdFold ff = {att, c.act, P};
  rc = pc_fused_forward(f, X, c.Z, Tsave, R, C, K, c.train, c.keep_prob, c.key.seed, c.key.offset, c.key.offset_dev, st,
                        prebits, fold ? &ff : nullptr, tagged, c.gather_arg());
  if (rc != APA_OK) return rc;
  if (fold) {
    // one-call train step: pc_backward's first launch (pc_bwd_dx_kernel) finishes logits + cross-entropy
    if (xent_here && pc_fused_dx_supported(P, c.act)) {
      xf->done = true;
      xf->deferred = true;
      xf->logits = logits;
      return APA_OK;
    }
    return pc_fused_logits_finish(f, logits, N, P, K, st);
  }
  PcXent xe = {nullptr, nullptr, nullptr, 0.f};
  if (xent_here) {
    xe.labels = xf->labels; xe.loss = xf->loss; xe.G = xf->G; xe.gscale = xf->gscale;
    xf->done = true;
  }
  if (tr) {
    tr->fwd_act = PC_ACT_BF16; tr->fwd_act_xe = xent_here ? 1 : 0; tr->logits = PC_LOGITS_FWD_ACT;
    if (xent_here) tr->xent = PC_XENT_FWD_ACT;
  }
  return pc_fwd_act(c, Tsave, att, logits, topdown, xe, st);
}

static int pc_forward_generic(const PcCall& c, const M1Fwd& io, hipStream_t st, M1Xent* xf) {
  const int C = c.C, Ca = c.Ca, K = c.K, Kp = c.Kp, R = c.R;
  const void *const X = io.X, *const Xatt = io.Xatt;
  const float *const Wa = io.Wa, *const ba = io.ba, *const Wt = io.Wt, *const bt = io.bt;
  float *const logits = io.logits, *const att = io.att, *const Tsave = io.zsave;
  void* const topdown = io.topdown;
  PcTrace* tr = pc_trace();
  if (tr) { tr->path_fwd = PC_PATH_GENERIC; tr->cat = c.cat ? 1 : 0; tr->fast = c.dma ? 1 : 0; }
  {
    PcPadList pads;
    if (!(c.flags & APA_FLAG_WEIGHT_IMAGES)) {     // else: kept current by the caller (pc_weight_images' layout)
      pads.add(Wa, c.WaP, Ca, Kp, c.wb16, c.ldw);
      pads.add(ba, c.baP, 1, Kp, false);
      if (c.dma) pads.add(Wt, c.WtP, C, Kp, true, c.ldw);
    }
    const int rc = pc_pad_launch(c, pads, X, st);   // (+ dropout(X) of the T product and its keep bits)
    if (rc != APA_OK) return rc;
  }
  GemmDesc gz;  // Z = Xatt . Wa + ba
  gz.A = Xatt; gz.lda = Ca; gz.ta = c.tdt; gz.a_kc = true;
  gz.B = c.WaP; gz.ldb = c.ldw; gz.tb = c.wb16 ? 1 : 0; gz.b_kc = false;
  gz.C = c.Z; gz.ldc = Kp; gz.tc = 0;
  gz.M = R; gz.N = Kp; gz.K = Ca; gz.bias = c.baP;
  // N = Kp is one tile column: R/128 blocks cannot fill 256 CUs, so split the contraction
  float* gws = reinterpret_cast<float*>(c.w + c.pl.off_gemm);
  gz.splits = gemm_pick_splits(R, Kp, Ca); if (gz.splits > 8) gz.splits = 8;
  gz.ws = gws;
  GemmDesc gt;  // T = dropout(X) . Wt + bt
  gt.A = X; gt.lda = C; gt.ta = c.tdt; gt.a_kc = true;
  gt.C = Tsave; gt.ldc = K; gt.tc = 0;
  gt.M = R; gt.K = C; gt.bias = bt;
  if (c.dma) {  // zero-padded weights (16-byte rows) + materialised dropout: the DMA-staged MFMA GEMM
    gt.B = c.WtP; gt.ldb = c.ldw; gt.tb = 1; gt.b_kc = false;
    gt.N = Kp; gt.n_valid = K;
    if (c.train) gt.A = c.w + c.pl.off_xd;     // (written by the padding launch above)
  } else {      // Wt rows are K floats: unaligned -> scalar staging, mask applied while staging
    gt.B = Wt; gt.ldb = K; gt.tb = 0; gt.b_kc = false;
    gt.N = K;
    if (c.train) set_dropout(gt, true, false, c);
  }
  gt.splits = gemm_pick_splits(R, Kp, C); if (gt.splits > 8) gt.splits = 8;
  gt.ws = reinterpret_cast<float*>(reinterpret_cast<char*>(gws) + c.pl.gemm_half);
  // Z | T: same shape when the attention input has C channels too -- one launch (GemmDesc::twin), else one after
  // the other (the dispatcher decides)
  gz.twin = &gt;
  if (tr) { gz.trace = &tr->g_z; gt.trace = &tr->g_t; tr->t_drop_a = gt.drop_a; }
  int rc = gemm_launch(gz, st);
  if (rc != APA_OK) return rc;
  if (tr) { tr->fwd_act = c.dtype == APA_DTYPE_F32 ? PC_ACT_F32 : PC_ACT_BF16; tr->logits = PC_LOGITS_FWD_ACT; }
  rc = pc_fwd_act(c, Tsave, att, logits, topdown, PcXent{nullptr, nullptr, nullptr, 0.f}, st);
  if (rc != APA_OK) return rc;
  // one-call train step: the cross-entropy of the logits row is taken by the backward activation pass (one launch
  // less); the batch mean rides on the column-sum launch that ends the backward half
  if (xf && xf->labels && xf->G && xf->loss && !xf->probs && K >= 4 && K <= 1024) {
    xf->done = true;
    xf->deferred = true;
    xf->logits = logits;
  }
  return APA_OK;   // (PcTrace::xent of a deferred cross-entropy: recorded where it is taken, in pc_backward)
}

int pc_forward(const PoolCall& d, const M1Fwd& io, M1Xent* xf) {
  PcCall c = pc_call(d, io.X);
  if (c.gather) {   // the forward product counts the clamped ids and leaves the labels read through the index
    c.ga.g.status = d.fc->status;
    if (d.fc_labels) {
      c.ga.g.labels = d.fc_labels;
      c.ga.g.labels_out = pc_gathered_labels(d.ws, d.N, d.P, d.C, d.Ca, d.K, d.dtype);
    }
  }
  if (PcTrace* tr = pc_trace()) { tr->phase = 1; tr->topdown = io.topdown ? 1 : 0; }
  if (pc_fused_supported(d.N, d.P, d.C, d.Ca, d.K, d.dtype, io.X, io.Xatt) && !rng_external(d.flags))
    return pc_forward_fused(c, io, d.st, xf);
  if (c.gather) return pc_gather_refuse("attn_pool_fwd M=K");
  return pc_forward_generic(c, io, d.st, xf);
}

// dbt | dba: the fixed-order column sums of the [nrows][2K] block partials.  The call's LAST launch (its own, or
// the tail blocks of the fused dW reduce), so that it can also advance a device-side dropout counter after every kernel
// that keys its mask with it has run, and finish the batch mean of a cross-entropy taken inside this step
// (aux_n < 0: in apa_softmax_xent_fwd_bwd's own summation order -- bit-identical loss[0])
static ColsumArgs pc_tail_colsum(const PcCall& c, int nrows, float* dbt, float* dba, const M1Xent* xf) {
  ColsumArgs a;
  a.pdwa = c.pdbt; a.nblk = nrows; a.C = 2 * c.K; a.ld = 2 * c.K;
  a.dwa = dbt; a.dwa2 = dba; a.C1 = c.K;
  a.rng_bump = c.bump;
  if (xf && xf->done) { a.aux_src = xf->loss + 1; a.aux_n = -c.N; a.aux_scale = xf->lscale; a.aux_dst = xf->loss; }
  return a;
}

static int pc_backward_fused(const PcCall& c, const M1Bwd& io, hipStream_t st, const M1Xent* xf) {
  const int N = c.N, P = c.P, C = c.C, K = c.K, R = c.R;
  const void* const X = io.X;
  const float *const Wa = io.Wa, *const Wt = io.Wt, *const att = io.att, *const Tsave = io.zsave, *const G = io.G;
  // APA_FLAG_FROZEN_INPUT: no launch below is handed the caller's dX
  const bool frozen = (c.flags & APA_FLAG_FROZEN_INPUT) != 0;
  void* const dX = frozen ? nullptr : io.dX;
  float *const dWa = io.dWa, *const dba = io.dba, *const dWt = io.dWt, *const dbt = io.dbt;
  PcTrace* tr = pc_trace();
  if (tr) tr->path_bwd = PC_PATH_FUSED;
  const PcFusedWs f = pc_fused_carve(c.w + c.pl.off_fused, N, P, C);
  int rc = APA_OK;
  if (!(c.flags & APA_FLAG_WS_FROM_FWD)) {   // else the forward call left the operands and the mask bits in place
    // (the mask bits are regenerated at most here: the counter's last reader runs before the launch that advances it)
    const PcPrepBits pb = {(size_t)R * C, c.keep_prob, c.key.seed, c.key.offset, c.key.offset_dev};
    rc = pc_fused_prep(f, Wa, Wt, nullptr, nullptr, C, K, st, c.train ? &pb : nullptr,
                       !(c.flags & APA_FLAG_WEIGHT_IMAGES));
    if (rc != APA_OK) return rc;
  }
  int nrows;   // of the dbt | dba block partials
  if (pc_fused_dx_supported(P, c.act)) {
    // identity / relu attention: ONE write-bound kernel forms [dT | dZ] from att / T / G in registers, writes dX,
    // leaves [dT | dZ] and the dbt | dba block partials behind for the dW launch and its reduce tail
    nrows = pc_fused_dx_rows(R);
    rc = pc_fused_dx(f, G, att, Tsave, dX, c.pdbt, R, C, K, P, c.act, c.train, c.keep_prob,
                     (xf && xf->deferred) ? xf : nullptr, st);
    if (rc != APA_OK) return rc;
  } else {
    bf16_t* dTc = static_cast<bf16_t*>(f.dTdZ);              // [R][dT (64) | dZ (64)]
    const PcDefer df = {{nullptr, nullptr, nullptr, 0.f}, nullptr};   // (a deferred cross-entropy only goes with the dX kernel above)
    int ps;
    rc = pc_bwd_act(c, G, att, Tsave, dTc, dTc + 64, 128, df, &ps, st);
    if (rc != APA_OK) return rc;
    nrows = N * ps;
    if (tr) { tr->bwd_act = PC_ACT_BF16; tr->ps = ps; tr->ldg = 128; tr->dx = c.train ? PC_DX_MID_GEMM : PC_DX_PLAIN_GEMM; }
    // dX = (dT . Wt^T) * mask/keep + dZ . Wa^T: one launch over the concatenated k = 128.  (Round 5: BEFORE the dW
    // launches -- the reduce tail that ends them may overwrite the keep-bit map with the next step's.)
    if (frozen) {   // the product's only output is dX: not launched
      if (tr) tr->dx = PC_DX_NONE;
    } else if (c.train) {
      rc = gemm_bf16_mid_dropout(f.dTdZ, 128, f.Wcat2, 128, dX, C, R, C, 128, 1.0f / c.keep_prob, f.maskbits, st);
    } else {
      GemmDesc g;
      g.A = f.dTdZ; g.lda = 128; g.ta = 1; g.a_kc = true;
      g.B = f.Wcat2; g.ldb = 128; g.tb = 1; g.b_kc = true;
      g.C = dX; g.ldc = C; g.tc = 1;
      g.M = R; g.N = C; g.K = 128;
      if (tr) g.trace = &tr->g_dx;
      rc = gemm_launch(g, st);
    }
    if (rc != APA_OK) return rc;
  }
  // dbt | dba, the batch mean of a folded cross-entropy and the dropout counter ride on the tail blocks of the dW
  // reduce launch
  PcDwTail tail;
  tail.cs = pc_tail_colsum(c, nrows, dbt, dba, xf);
  // the same condition as pc_forward's `tagged` (WS_FROM_FWD is set by the library's own train step only): this
  // launch is the step's last -- it also leaves the NEXT step's keep bits behind, tagged (seed, offset + 1)
  if (c.train && (c.flags & APA_FLAG_WEIGHT_IMAGES) && (c.flags & APA_FLAG_WS_FROM_FWD)) {
    tail.next_bits = true;
    tail.next_seed = c.key.seed;
  }
  return pc_fused_dw(f, X, dWt, dWa, R, C, K, c.train, c.keep_prob, st, &tail, c.gather_arg());
}

static int pc_backward_generic(const PcCall& c, const M1Bwd& io, hipStream_t st, const M1Xent* xf) {
  const void *const X = io.X, *const Xatt = io.Xatt;
  const float *const Wa = io.Wa, *const Wt = io.Wt, *const att = io.att, *const Tsave = io.zsave, *const G = io.G;
  void *const dX = io.dX, *const dXatt = io.dXatt;
  float *const dWa = io.dWa, *const dba = io.dba, *const dWt = io.dWt, *const dbt = io.dbt;
  const int N = c.N, C = c.C, Ca = c.Ca, K = c.K, Kp = c.Kp, R = c.R, ldw = c.ldw, tdt = c.tdt;
  void* dT = c.w + c.pl.off_dt;
  void* dZ = c.cat ? static_cast<void*>(static_cast<bf16_t*>(dT) + Kp) : static_cast<void*>(c.w + c.pl.off_dz);
  float* gws = reinterpret_cast<float*>(c.w + c.pl.off_gemm);
  const bool fused = (Xatt == X);
  PcTrace* tr = pc_trace();
  // APA_FLAG_WS_FROM_FWD (one-call train step): the forward call's padded bf16 weights and its materialised
  // dropout(X) are still in the workspace -- the second pc_pad / pc_dropout launch (7.9 + 8.4 us at K = 393) is
  // skipped.  Only the all-bf16 DMA route prepares both operands in the forward pass.
  const bool reuse_fwd = (c.flags & APA_FLAG_WS_FROM_FWD) && c.dma;
  if (tr) {
    tr->path_bwd = PC_PATH_GENERIC; tr->cat = c.cat ? 1 : 0; tr->fast = c.dma ? 1 : 0; tr->reuse_fwd = reuse_fwd ? 1 : 0;
  }
  int rc = APA_OK;
  if (!reuse_fwd) {
    PcPadList pads;
    if (!(c.flags & APA_FLAG_WEIGHT_IMAGES)) {
      pads.add(Wa, c.WaP, Ca, Kp, c.wb16, ldw);
      pads.add(Wt, c.WtP, C, Kp, c.wb16, ldw);
    }
    rc = pc_pad_launch(c, pads, X, st);   // (+ dropout(X) for the dWt product and its keep bits)
    if (rc != APA_OK) return rc;
  }
  PcDefer df = {{nullptr, nullptr, nullptr, 0.f}, nullptr};
  if (xf && xf->deferred) {
    df.row_logits = xf->logits;
    df.xe.labels = xf->labels; df.xe.loss = xf->loss; df.xe.G = xf->G; df.xe.gscale = xf->gscale;
  }
  const int ldg = c.dtype == APA_DTYPE_F32 ? Kp : ldw;
  int ps;
  rc = pc_bwd_act(c, G, att, Tsave, dT, dZ, ldg, df, &ps, st);
  if (rc != APA_OK) return rc;
  if (tr) {
    tr->bwd_act = c.dtype == APA_DTYPE_F32 ? PC_ACT_F32 : PC_ACT_BF16; tr->ps = ps; tr->ldg = ldg;
    if (df.row_logits) tr->xent = PC_XENT_BWD_ACT;
  }
  {  // dWt[c,k] = sum_r Xt[r,c] dT[r,k]
    GemmDesc g;
    g.A = X; g.lda = C; g.ta = tdt; g.a_kc = false;
    g.B = dT; g.ldb = ldw; g.tb = tdt; g.b_kc = false;
    g.C = dWt; g.ldc = K; g.tc = 0;
    g.M = C; g.N = K; g.K = R;
    g.splits = gemm_pick_splits(C, K, R); g.ws = gws;
    if (c.dma) {
      g.N = Kp; g.n_valid = K;   // dT is [R][Kp] with zero pad columns
      if (c.train) g.A = c.w + c.pl.off_xd;   // (from the forward call, or from the padding launch above)
    } else if (c.train) {
      set_dropout(g, true, false, c);
      // dropout index of A(m=c, k=r) is r*C + c: the stager computes row*Ktot + k with row = m, so
      // the transposed operand needs the swapped form -> handled by drop_a == 2
      g.drop_a = 2;
    }
    // dWa[c,k] = sum_r Xatt[r,c] dZ[r,k]: the twin of the same launch when the shapes agree (Ca == C, bf16)
    GemmDesc h;
    h.A = Xatt; h.lda = Ca; h.ta = tdt; h.a_kc = false;
    h.B = dZ; h.ldb = ldw; h.tb = tdt; h.b_kc = false;
    h.C = dWa; h.ldc = K; h.tc = 0;
    h.M = Ca; h.N = K; h.K = R;
    h.splits = gemm_pick_splits(Ca, K, R);
    h.ws = reinterpret_cast<float*>(reinterpret_cast<char*>(gws) + c.pl.gemm_half);
    if (c.dtype == APA_DTYPE_BF16) { h.N = Kp; h.n_valid = K; }   // dZ is [R][Kp] with zero pad columns
    g.twin = &h;
    if (tr) { g.trace = &tr->g_dwt; h.trace = &tr->g_dwa; tr->dw = PC_DW_TWIN_GEMM; tr->dw_drop_a = g.drop_a; }
    rc = gemm_launch(g, st);
    if (rc != APA_OK) return rc;
  }
  // (the wide kernel's vector epilogue stores 16 bytes at a time: an odd dX address keeps the two-product form)
  if (c.cat && fused && gemm_bf16_wide_serves(R, C, 2 * Kp) && (reinterpret_cast<uintptr_t>(dX) & 15) == 0) {
    // dX = (dT . Wt^T) * mask/keep + dZ . Wa^T as ONE product over [dT | dZ] . [Wt | Wa]^T: the accumulators are
    // masked with the keep bits after the first Kp of the contraction (gemm_bf16_wide_kernel<.., MID>)
    GemmDesc g;
    g.A = dT; g.lda = ldw; g.ta = 1; g.a_kc = true;
    g.B = c.WtP; g.ldb = ldw; g.tb = 1; g.b_kc = true;
    g.C = dX; g.ldc = C; g.tc = 1;
    g.M = R; g.N = C; g.K = 2 * Kp;
    g.stream_out = true;
    if (c.train) {
      g.mid_bits = reinterpret_cast<const uint8_t*>(c.w + c.pl.off_bits); g.mid_k = Kp; g.mid_inv_keep = 1.0f / c.keep_prob;
    }
    if (tr) { g.trace = &tr->g_dx; tr->dx = PC_DX_WIDE; tr->mid_bits = g.mid_bits ? 1 : 0; tr->wa_to = PC_WA_NONE; }
    rc = gemm_launch(g, st);
    if (rc != APA_OK) return rc;
  } else {
    {  // dX = (dT . Wt^T) * mask/keep
      GemmDesc g;
      g.A = dT; g.lda = ldw; g.ta = tdt; g.a_kc = true;
      g.B = c.WtP; g.ldb = ldw; g.tb = c.wb16 ? 1 : 0; g.b_kc = true;
      g.C = dX; g.ldc = C; g.tc = tdt;
      g.M = R; g.N = C; g.K = Kp;
      if (c.train) set_dropout(g, false, true, c);
      if (tr) { g.trace = &tr->g_dx; tr->dx = PC_DX_TWO; tr->dx_drop_c = g.drop_c; }
      rc = gemm_launch(g, st);
      if (rc != APA_OK) return rc;
    }
    {  // + dZ . Wa^T  (into dX when the attention input is X itself, else into dXatt)
      GemmDesc g;
      g.A = dZ; g.lda = ldw; g.ta = tdt; g.a_kc = true;
      g.B = c.WaP; g.ldb = ldw; g.tb = c.wb16 ? 1 : 0; g.b_kc = true;
      g.C = fused ? dX : dXatt; g.ldc = fused ? C : Ca; g.tc = tdt;
      g.M = R; g.N = fused ? C : Ca; g.K = Kp; g.beta = fused ? 1.f : 0.f;
      g.stream_out = true;
      if (tr) { g.trace = &tr->g_dxa; tr->wa_to = fused ? PC_WA_DX_BETA1 : PC_WA_DXATT; }
      rc = gemm_launch(g, st);
      if (rc != APA_OK) return rc;
    }
  }
  const ColsumArgs tail = pc_tail_colsum(c, N * ps, dbt, dba, xf);
  if (tr) {
    tr->tail = PC_TAIL_COLSUM; tr->tail_nrows = tail.nblk; tr->rng_bump = tail.rng_bump ? 1 : 0;
    tr->aux = tail.aux_src ? 1 : 0;
  }
  return m1_colsum(tail, st);
}

int pc_backward(const PoolCall& d, const M1Bwd& io, const M1Xent* xf) {
  const PcCall c = pc_call(d, io.X);
  if (PcTrace* tr = pc_trace()) tr->phase = 2;
  if (pc_fused_supported(d.N, d.P, d.C, d.Ca, d.K, d.dtype, io.X, io.Xatt) && !rng_external(d.flags))
    return pc_backward_fused(c, io, d.st, xf);
  if (c.gather) return pc_gather_refuse("attn_pool_bwd M=K");
  if (d.flags & APA_FLAG_FROZEN_INPUT) {   // (the entry points refuse this before their forward half: frozen_input_check)
    set_error("per-class maps: APA_FLAG_FROZEN_INPUT is not served by the dense per-class route");
    return APA_ERR_UNSUPPORTED;
  }
  return pc_backward_generic(c, io, d.st, xf);
}

}  // namespace apa
