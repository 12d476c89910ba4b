// apa_m1.hip -- class-agnostic (M == 1) attentional pooling, factorised, HBM-bound.
//
// Reference semantics: models/slim/nets/nets_factory.py:247-328 (see include/apa.h).  With a
// single bottom-up map the [N,P,K] top-down tensor never has to exist:
//
//   forward   z[n,:]  = (1/P) sum_p A[n,p] * Xt[n,p,:]        abar[n] = (1/P) sum_p A[n,p]
//             logits  = z . Wt + abar (x) bt
//   backward  dz      = G . Wt^T          dWt = z^T G         dbt = sum_n abar[n] G[n,:]
//             dA[n,p] = (Xt[n,p,:] . dz[n,:] + G[n,:] . bt) / P
//             dZ      = dA | dA*[A>0] | A*(dA - (z.dz + (G.bt)*abar))     (id | relu | softmax)
//             dX      = (A/P) dz (*mask/keep) + dZ * wa              dwa = sum dZ * X
//
// Each feature map is streamed from HBM exactly once per pass: X is read once in forward, and
// read once + dX written once in backward (3*P*C*sizeof(T) algorithmic bytes per image).
//
// This file: the stages every pooling family shares (finalize, the attention GEMV forward / backward for a separate
// Xatt, softmax rows, the fallback reduce) and the host dispatch.  The two streaming passes themselves come in three
// families behind one pair of launchers each: apa_m1_stream.hip (wide maps), apa_m1_vec.hip (narrow powers of two),
// apa_m1_generic.hip (any C); a fourth, apa_m1_fp8.hip, reads an FP8 feature cache.
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

// --------------------------------------------------------------------------------------------
// F2: merge the S block partials of each image.  grid (N, C/(4 cw)), block 256, cw channel threads
// (one float4 each).
//   z[n,c] = (1/P) sum_s pacc[n,s,c] * w_s     w_s = exp(m_s - M)/L (on-line softmax) or 1
//   abar[n] = (1/P) sum_p A[n,p];  softmax: att[n,p] <- exp(Z - M)/L
// R: partial rows per image in pacc -- S, or S / 2 behind a paired pooling pass (apa_m1_stream.hip; never the on-line
// softmax, whose rows carry their own weights); pstat always has S entries per image.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m1_finalize_fwd_kernel(
    const float* __restrict__ pacc, const float* __restrict__ pstat, int P, int S, int R, int C, int online_softmax,
    int cw, float* __restrict__ z, float* __restrict__ abar, float* __restrict__ att) {   // inputs and sizes first: preload
  // cw = threads of the block that carry channels (one float4 each): the grid is (N, ceil(C / 4cw)).  A CU
  // sustains only ~25-30 GB/s of vector loads, so the 4 MB of partials want to be spread over all 256
  // CUs (cw = 64 at N = 32: 256 blocks x 16 KB) rather than 64 blocks x 64 KB (cw = 256).
  __shared__ float s_w[256];   // per-split weight exp(m_s - M) / L / P   (S <= 256)
  __shared__ float s_red[8];
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float invP = 1.0f / (float)P;
  const float* st = pstat + (size_t)n * S * 4;
  // Latency chain: every load is issued before anything is consumed -- the first 16 partial rows
  // (all of them at the benchmark batch) and the per-split statistics travel together.
  constexpr int FB = 16;
  const bool chan = (int)threadIdx.x < cw;
  const int v = chan ? blockIdx.y * cw + threadIdx.x : 0;
  const float* pa = pacc + (size_t)n * R * C + (v * 4 < C ? v * 4 : 0);
  float4 first[FB];
  if (chan) {   // wave-uniform: cw is a multiple of 64
#pragma unroll
    for (int u = 0; u < FB; ++u)
      first[u] = *reinterpret_cast<const float4*>(pa + (size_t)min(u, R - 1) * C);
  }
  // one split per thread: no serial dependent-load chain
  float m_s = -INFINITY, l_s = 0.f, a_s = 0.f;
  if ((int)threadIdx.x < S) {
    m_s = st[threadIdx.x * 4];
    l_s = st[threadIdx.x * 4 + 1];
    a_s = st[threadIdx.x * 4 + 2];
  }
  float M = 0.f, invL = 1.f, asum = 0.f;
  if (online_softmax) {
    float mw = wave_max(m_s);
    if (lane == 0) s_red[wave] = mw;
    __syncthreads();
    M = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    const float e = ((int)threadIdx.x < S) ? expf(m_s - M) : 0.f;
    float lw = wave_sum(l_s * e);
    if (lane == 0) s_red[4 + wave] = lw;
    __syncthreads();
    invL = 1.0f / ((s_red[4] + s_red[5]) + (s_red[6] + s_red[7]));
    s_w[threadIdx.x] = e * invL * invP;
  } else {
    float aw = wave_sum(a_s);
    if (lane == 0) s_red[wave] = aw;
    s_w[threadIdx.x] = invP;
    __syncthreads();
    asum = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  }
  __syncthreads();
  if (chan && v * 4 < C) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < FB; ++u) {
      if (u < R) {
        const float w = s_w[u];
        r.x = fmaf(first[u].x, w, r.x); r.y = fmaf(first[u].y, w, r.y);
        r.z = fmaf(first[u].z, w, r.z); r.w = fmaf(first[u].w, w, r.w);
      }
    }
    for (int s0 = FB; s0 < R; s0 += FB) {   // more than 16 rows (small batches): further rounds of 16
      float4 a[FB];
#pragma unroll
      for (int u = 0; u < FB; ++u)
        a[u] = *reinterpret_cast<const float4*>(pa + (size_t)min(s0 + u, R - 1) * C);
#pragma unroll
      for (int u = 0; u < FB; ++u) {
        const float w = s0 + u < R ? s_w[s0 + u] : 0.f;
        r.x = fmaf(a[u].x, w, r.x); r.y = fmaf(a[u].y, w, r.y);
        r.z = fmaf(a[u].z, w, r.z); r.w = fmaf(a[u].w, w, r.w);
      }
    }
    *reinterpret_cast<float4*>(z + (size_t)n * C + v * 4) = r;
  }
  if (blockIdx.y == 0) {
    if (online_softmax) {
      // sum_p softmax = 1 up to rounding; keep the measured value for backward consistency
      float tot = 0.f;
      for (int p = threadIdx.x; p < P; p += 256) {
        const float a = expf(att[(size_t)n * P + p] - M) * invL;
        att[(size_t)n * P + p] = a;
        tot += a;
      }
      tot = wave_sum(tot);
      __syncthreads();
      if (lane == 0) s_red[wave] = tot;
      __syncthreads();
      if (threadIdx.x == 0) abar[n] = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) * invP;
    } else if (threadIdx.x == 0) {
      abar[n] = asum * invP;
    }
  }
}

// --------------------------------------------------------------------------------------------
// Attention logits from a separate tensor (cfg 003: Xatt = pose_pre_logits, Ca = 768):
//   Z[n,p] = Xatt[n,p,:] . wa + ba, one wave per pixel, generic Ca (multiple of EPV).
// `act`: id / relu applied here; softmax left raw for m1_softmax_rows_kernel.
// --------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void m1_att_gemv_fwd_kernel(const T* __restrict__ Xa,
                                                              const float* __restrict__ Wa,
                                                              const float* __restrict__ ba,
                                                              float* __restrict__ att, long NP,
                                                              int Ca, int act) {
  constexpr int EPV = Vec<T>::EPV;
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nw = (long)gridDim.x * 4;
  const int nvec = Ca / EPV;
  const float bias = ba[0];
  for (long px = wid; px < NP; px += nw) {
    const T* xr = Xa + (size_t)px * Ca;
    float d = 0.f;
    for (int v = lane; v < nvec; v += 64) {
      float x[EPV];
      Vec<T>::unpack(ld16(xr + v * EPV), x);
#pragma unroll
      for (int e = 0; e < EPV; ++e) d = fmaf(x[e], Wa[v * EPV + e], d);
    }
    float zl = wave_sum(d) + bias;
    if (act == M1_ACT_RELU) zl = fmaxf(zl, 0.f);
    if (lane == 0) att[px] = zl;
  }
}

// In-place spatial softmax of att[n, 0:P] (tf.nn.softmax, max-subtracted); one wave per image.
__global__ __launch_bounds__(64) void m1_softmax_rows_kernel(float* __restrict__ att, int P) {
  float* row = att + (size_t)blockIdx.x * P;
  const int lane = threadIdx.x;
  float m = -INFINITY;
  for (int p = lane; p < P; p += 64) m = fmaxf(m, row[p]);
  m = wave_max(m);
  float l = 0.f;
  for (int p = lane; p < P; p += 64) l += expf(row[p] - m);
  l = wave_sum(l);
  const float inv = 1.0f / l;
  for (int p = lane; p < P; p += 64) row[p] = expf(row[p] - m) * inv;
}

// --------------------------------------------------------------------------------------------
// B4: column sums of the per-block partials (fixed order) + dbt.
//   dwa[c] = sum_b pdwa[b][c];  dba = sum_b pdba[b];  dbt[k] = sum_n abar[n] * G[n][k]
// grid = ceil(C/64) + 1 blocks of 256 threads; the last block does dba and dbt.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void m1_bwd_reduce_kernel(
    const float* __restrict__ pdwa, const float* __restrict__ pdba, float* __restrict__ dwa,
    float* __restrict__ dba, const float* __restrict__ abar, const float* __restrict__ G,
    float* __restrict__ dbt, int nblk, int C, int N, int K, int do_dwa,
    uint64_t* __restrict__ rng_bump) {
  __shared__ float red[4][64];
  // this is the last kernel of the backward call: the step's dropout key has been consumed
  if (rng_bump && blockIdx.x == 0 && threadIdx.x == 0) *rng_bump += 1;
  const int ncol_blocks = (C + 63) / 64;
  if ((int)blockIdx.x < ncol_blocks) {
    if (!do_dwa) return;
    const int c = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rg = threadIdx.x >> 6;
    float acc = 0.f;
    if (c < C)
      for (int b = rg; b < nblk; b += 4) acc += pdwa[(size_t)b * C + c];
    red[rg][threadIdx.x & 63] = acc;
    __syncthreads();
    if (rg == 0 && c < C)
      dwa[c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  } else {
    for (int k = threadIdx.x; k < K; k += 256) {
      float acc = 0.f;
      for (int n = 0; n < N; ++n) acc = fmaf(abar[n], G[(size_t)n * K + k], acc);
      dbt[k] = acc;
    }
    if (do_dwa) {
      float acc = 0.f;
      for (int b = threadIdx.x; b < nblk; b += 256) acc += pdba[b];
      acc = wave_sum(acc);
      if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = acc;
      __syncthreads();
      if (threadIdx.x == 0) dba[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    }
  }
}

// --------------------------------------------------------------------------------------------
// Attention-side backward when Xatt != X (cfg 003):
//   dXatt[n,p,:] = dZ[n,p] * wa;   pdwa[b][:] = sum over block pixels dZ * Xatt;  pdba[b]
// grid = nb blocks x 256 threads; wave-strided pixels; generic Ca.
// --------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void m1_att_gemv_bwd_kernel(
    const T* __restrict__ Xa, const float* __restrict__ Wa, const float* __restrict__ dZ,
    T* __restrict__ dXa, float* __restrict__ pdwa, float* __restrict__ pdba, long NP, int Ca) {
  constexpr int EPV = Vec<T>::EPV;
  extern __shared__ __attribute__((aligned(16))) float sm[];  // [4][Ca] + 4
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long wid = (long)blockIdx.x * 4 + wave;
  const long nw = (long)gridDim.x * 4;
  const int nvec = Ca / EPV;
  float* my = sm + (size_t)wave * Ca;
  for (int c = lane; c < Ca; c += 64) my[c] = 0.f;
  float dba = 0.f;
  for (long px = wid; px < NP; px += nw) {
    const float g = dZ[px];
    dba += g;
    const T* xr = Xa + (size_t)px * Ca;
    T* dr = dXa + (size_t)px * Ca;
    for (int v = lane; v < nvec; v += 64) {
      float x[EPV], o[EPV];
      Vec<T>::unpack(ld16(xr + v * EPV), x);
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        o[e] = g * Wa[v * EPV + e];
        my[v * EPV + e] = fmaf(g, x[e], my[v * EPV + e]);
      }
      st16(dr + v * EPV, Vec<T>::pack(o));
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < Ca; c += 256)
    pdwa[(size_t)blockIdx.x * Ca + c] = (sm[c] + sm[Ca + c]) + (sm[2 * Ca + c] + sm[3 * Ca + c]);
  if (lane == 0) sm[4 * Ca + wave] = dba;
  __syncthreads();
  if (threadIdx.x == 0)
    pdba[blockIdx.x] = (sm[4 * Ca] + sm[4 * Ca + 1]) + (sm[4 * Ca + 2] + sm[4 * Ca + 3]);
}

// Same outputs, one thread per 16-byte vector of the row (Ca <= 256 vectors): the attention weights
// and the dwa accumulators of the thread's channels live in registers (the kernel above re-reads Wa
// from memory and read-modify-writes an LDS accumulator per element and pixel), a block owns a
// contiguous pixel range and takes it eight pixels per round with the eight row loads in flight.
// STORE = false (APA_FLAG_DXATT_RANK1): dXa = dZ (x) wa is not materialised, only the dwa / dba partials.
template <typename T, bool STORE>
__global__ __launch_bounds__(256) void m1_att_gemv_bwd2_kernel(
    const T* __restrict__ Xa, const float* __restrict__ Wa, const float* __restrict__ dZ,
    T* __restrict__ dXa, float* __restrict__ pdwa, float* __restrict__ pdba, long NP, int Ca) {
  constexpr int EPV = Vec<T>::EPV;
  constexpr int PR = 8;
  const int nvec = Ca / EPV;
  const int v = threadIdx.x < nvec ? threadIdx.x : nvec - 1;   // idle lanes shadow the last vector
  const bool active = (int)threadIdx.x < nvec;
  const long p_begin = (long)blockIdx.x * NP / gridDim.x, p_end = (long)(blockIdx.x + 1) * NP / gridDim.x;
  float wa[EPV], dwa[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) { wa[e] = Wa[v * EPV + e]; dwa[e] = 0.f; }
  float dba = 0.f;
  for (long p0 = p_begin; p0 < p_end; p0 += PR) {
    uint4 xr[PR];
    float g[PR];
#pragma unroll
    for (int u = 0; u < PR; ++u) {
      const long px = min(p0 + u, p_end - 1);   // surplus slots re-read the last pixel, weight 0
      xr[u] = ld16(Xa + (size_t)px * Ca + v * EPV);
      g[u] = p0 + u < p_end ? dZ[px] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < PR; ++u) {
      float x[EPV], o[EPV];
      Vec<T>::unpack(xr[u], x);
      dba += g[u];
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        o[e] = g[u] * wa[e];
        dwa[e] = fmaf(g[u], x[e], dwa[e]);
      }
      if (STORE && active && p0 + u < p_end) st16(dXa + (size_t)(p0 + u) * Ca + v * EPV, Vec<T>::pack(o));
    }
  }
  if (active) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) pdwa[(size_t)blockIdx.x * Ca + v * EPV + e] = dwa[e];
  }
  if (threadIdx.x == 0) pdba[blockIdx.x] = dba;
}

// ============================================================================================
// host side
// ============================================================================================
thread_local M1Trace* g_m1_trace = nullptr;
thread_local unsigned g_m1_iflags = 0;
thread_local M1FwdRoute g_m1_fwd_route = {0, 0};
thread_local M1Rows g_m1_rows = {0, 0};

// Any channel count that is a whole number of 16-byte vectors is served: the channel-split streaming
// kernels (apa_m1_stream.hip) for the wide benchmark shapes, the per-pixel kernels (apa_m1_vec.hip) for the
// other powers of two, the run-time-loop kernels of apa_m1_generic.hip for everything else.
bool m1_supported(int C, int Ca, int dtype, bool fused) {
  if (dtype == APA_DTYPE_FP8_E4M3) return fused && m1f_supported(C);
  const int epv = dtype == APA_DTYPE_BF16 ? 8 : 4;
  if (!fused && (Ca % epv != 0)) return false;
  return m1s_supported(C, dtype) || m1v_supported(C, dtype) || m1g_supported(C, dtype);
}

// Grid sizing.  The streaming kernels hold 2 blocks (8 waves) per CU at their register budget, so
// 512 blocks is exactly one resident round of the 256 CUs; small batches get S = 512/N pixel
// splits per image (>= 4 pixels per block so every wave owns at least one), large batches
// (N >= 512) one block per image.
M1Plan m1_plan(int N, int P, int C, int Ca, int K) {
  M1Plan pl;
  int S = (512 + N / 2) / N;
  if (S < 1) S = 1;
  int maxS = P >= 8 ? P / 4 : 1;
  if (maxS > 256) maxS = 256;   // m1_finalize_fwd_kernel: one split per thread of a 256-thread block
  if (S > maxS) S = maxS;
  pl.S = S;
  pl.ppb = (P + S - 1) / S;
  pl.nblk = N * pl.S;
  pl.lsplits = C >= 1024 ? 16 : (C >= 256 ? 4 : 1);
  const int cmax = C > Ca ? C : Ca;
  size_t off = 0;
  pl.off_pacc = off;  off += align_up((size_t)pl.nblk * C * 4, 256);
  pl.off_pstat = off; off += align_up((size_t)pl.nblk * 4 * 4, 256);
  pl.off_pdwa = off;  off += align_up((size_t)pl.nblk * cmax * 4, 256);
  pl.off_pdba = off;  off += align_up((size_t)(pl.nblk + N) * 4, 256);  // + sn[N]
  pl.off_dz = off;    off += align_up((size_t)N * C * 4, 256);
  pl.off_dzatt = off; off += align_up((size_t)N * P * 4, 256);
  {
    size_t g = sgemm_ws_bytes(N, K > C ? K : C, 16);
    if (C % 64 == 0 && m1_logits2_ws_bytes(N, C, K) > g) g = m1_logits2_ws_bytes(N, C, K);
    pl.off_gemm = off;  off += align_up(g, 256);
  }
  pl.off_cat_e = off; off += align_up((size_t)N * P * 4, 256);   // e[n,p] of apa_m1_cat.hip
  // keep-bits of the dropout mask, forward -> backward (apa_m1_stream.hip): 256 * ceil(C / 2048) B per pixel
  pl.off_maskbits = off; off += align_up((size_t)N * P * 256 * ((C / 256 + 7) / 8), 256);
  pl.total = off;
  return pl;
}

// Every backward kernel family has an arm without the dX stores (APA_FLAG_FROZEN_INPUT).  APA_IFLAG_NO_DX -- the
// caller re-forms the pooling share of dX itself, from the keep bits -- additionally needs the keep-bits form of the
// streaming kernel: bf16 features in training mode inside a one-call step (the forward half left the bits in the workspace)
bool m1_no_dx_supported(int C, int dtype, bool train) {
  return train && dtype == APA_DTYPE_BF16 && m1s_supported(C, dtype);
}

int m1_call_fill(M1Call& c, const PoolCall& d, const M1Fwd* f, const M1Bwd* b, const M1Xent* xf) {
  const void* const X = b ? b->X : f->X;
  const void* const Xatt = b ? b->Xatt : f->Xatt;
  const bool loss_done = xf && xf->done;
  const int N = d.N, P = d.P, C = d.C, Ca = d.Ca, K = d.K, dtype = d.dtype;
  const unsigned flags = d.flags;
  const float keep_prob = d.keep_prob;
  const uint64_t seed = d.seed, offset = d.offset;
  const CatFeat* const cat = d.cat;
  const Hooks& hk = d.hk;
  void* const ws = d.ws;
  c.N = N; c.P = P; c.C = C; c.Ca = Ca; c.K = K; c.dtype = dtype; c.flags = flags; c.st = d.st; c.cat = cat;
  c.fused = (Xatt == X);
  c.train = (flags & APA_FLAG_TRAIN) && keep_prob < 1.0f;
  c.act = (flags & APA_FLAG_SOFTMAX_ATT) ? M1_ACT_SOFTMAX   // relu(softmax(.)) == softmax(.)
          : (flags & APA_FLAG_RELU_ATT) ? M1_ACT_RELU : M1_ACT_ID;
  c.pool_act = c.fused ? c.act : M1_ACT_ID;
  c.rank1 = b && (flags & APA_FLAG_DXATT_RANK1) != 0 && !c.fused;
  c.ext = c.train && rng_external(flags);
  c.relu_input = (flags & APA_FLAG_RELU_INPUT) != 0;
  c.no_dx = b && (flags & (APA_IFLAG_NO_DX | APA_FLAG_FROZEN_INPUT)) != 0;
  c.small = b && m1_small_route_ok(C, K, b->G, b->Wt, b->zsave);
  const int epv = dtype == APA_DTYPE_F32 ? 4 : 8;
  c.gemv2 = Ca % epv == 0 && Ca / epv <= 256;
  c.pool = dtype == APA_DTYPE_FP8_E4M3 ? M1_POOL_FP8
           : !c.ext && m1s_supported(C, dtype) ? M1_POOL_STREAM
           : !c.ext && m1v_supported(C, dtype) ? M1_POOL_VEC : M1_POOL_GENERIC;
  c.pl = m1_plan(N, P, C, Ca, K);
  // The paired form of the forward streaming pass (apa_m1_stream.hip): the plan is the logical one, the rows are what
  // is written.  fp32 features on the stream family with an even S and no softmax in the pooling kernel; bf16 features,
  // softmax instances, odd S and every backward pass keep one row per logical block (measured:
  // profiles/paired_rows_summary.md)
  const bool paired = f && c.pool == M1_POOL_STREAM && dtype == APA_DTYPE_F32 && c.pl.S % 2 == 0 &&
                      c.pool_act != M1_ACT_SOFTMAX && !(g_m1_iflags & APA_IFLAG_UNPAIRED);
  c.nrows = paired ? c.pl.nblk / 2 : c.pl.nblk;
  char* w = static_cast<char*>(ws);
  c.pacc = reinterpret_cast<float*>(w + c.pl.off_pacc);
  c.pstat = reinterpret_cast<float*>(w + c.pl.off_pstat);
  c.pdwa = reinterpret_cast<float*>(w + c.pl.off_pdwa);
  c.pdba = reinterpret_cast<float*>(w + c.pl.off_pdba);
  c.sn = c.small ? c.pdba + c.pl.nblk : nullptr;
  c.dz = reinterpret_cast<float*>(w + c.pl.off_dz);
  c.dzatt = c.rank1 ? static_cast<float*>(b->dXatt) : reinterpret_cast<float*>(w + c.pl.off_dzatt);
  c.gemm_ws = reinterpret_cast<float*>(w + c.pl.off_gemm);
  c.cat_e = reinterpret_cast<float*>(w + c.pl.off_cat_e);
  c.maskbits = reinterpret_cast<uint8_t*>(w + c.pl.off_maskbits);
  // APA_FLAG_WS_FROM_FWD: same workspace, untouched since the forward call
  c.maskbits_in = b && (flags & APA_FLAG_WS_FROM_FWD) ? c.maskbits : nullptr;
  c.key = rng_resolve(flags, keep_prob, seed, offset);
  c.inv_keep = c.train ? 1.0f / keep_prob : 1.0f;
  c.bump = (b && c.train && (flags & APA_FLAG_RNG_DEVICE)) ? reinterpret_cast<uint64_t*>(static_cast<uintptr_t>(offset))
                                                          : nullptr;
  // + the concatenated pose channels' share of dA (apa_m1_cat.hip); without them att, scale 0
  c.ex = b ? (cat ? c.cat_e : b->att) : nullptr;
  c.exs = cat ? 1.0f : 0.0f;
  c.ev0 = b ? hk.bwd0 : hk.fwd0; c.ev1 = b ? hk.bwd1 : hk.fwd1;
  c.gather = d.fc != nullptr;
  c.T = c.gather ? d.fc->cache_images : N;
  c.ga = M1Gather{nullptr, 0, nullptr, nullptr, nullptr};
  if (c.gather) {   // the backward pass reports and copies nothing: the forward pass did
    c.ga.index = d.fc->index; c.ga.T = c.T;
    if (f) {
      c.ga.status = d.fc->status;
      if (d.fc_labels) { c.ga.labels = d.fc_labels; c.ga.labels_out = m1_gathered_labels(ws, c.pl); }
    }
  }
  c.td_ready = hk.td_ready; c.grad_ready = hk.grad_ready;
  if (M1Trace* tr = m1_trace()) {
    tr->S = c.pl.S; tr->ppb = c.pl.ppb; tr->nblk = c.pl.nblk; tr->fused = c.fused; tr->relu_input = c.relu_input;
    (b ? g_m1_rows.bwd : g_m1_rows.fwd) = c.nrows;
  }

  // ---- every refusal of the path: nothing has been launched yet ----
  // The form a frozen cache feeds, an FP8 one and a gathered one alike: the fused identity / relu head, backward only in
  // the arm without the dX stores.  The entry points (fp8_check, cache_check, apa_capi.hip) name each reason; a call
  // built inside the library that reaches here with one of them is refused all the same, and only this form has FP8
  // kernels and gathered instances (m1_pool_form).
  const bool cache_form = c.fused && c.act != M1_ACT_SOFTMAX && !c.relu_input && !c.ext && !cat && !(b && !c.no_dx) &&
                          !(flags & APA_IFLAG_NO_DX);
  if (c.pool == M1_POOL_FP8 && !(cache_form && m1f_supported(C))) {
    set_error("attn_pool M=1: APA_DTYPE_FP8_E4M3 serves the fused identity / relu head on frozen features only");
    return APA_ERR_UNSUPPORTED;
  }
  // ... and, from the cfg 003 cached steps alone (PoolCall::fc_pose, apa_pose_cache.h), the same head with a separate
  // attention input: that input (pose_pre_logits, or the map already in `att`) has the batch shape and is never read
  // through the index; the pooling passes run their (FUSED = false, GATHER) instances.  No softmax (the backward pass has
  // no gathered softmax instance), no FP8
  const bool pose_form = d.fc_pose && !c.fused && c.pool != M1_POOL_FP8 && c.act != M1_ACT_SOFTMAX && !c.relu_input &&
                         !c.ext && !cat && !(b && !c.no_dx) && !(flags & APA_IFLAG_NO_DX);
  if (c.gather && !cache_form && !pose_form) {
    set_error("attn_pool M=1: a feature cache serves the fused identity / relu head on frozen features only");
    return APA_ERR_UNSUPPORTED;
  }
  // the streaming kernels split an image's pixels in 32-bit arithmetic (m1_pix_range); the other families keep 64 bits
  if (c.pool == M1_POOL_STREAM && !m1_pix_range_ok(P, c.pl.S)) {
    set_error("attn_pool M=1: P=%d pixels per image in S=%d splits: (S + 1) * P does not fit 31 bits", P, c.pl.S);
    return APA_ERR_UNSUPPORTED;
  }
  if (c.no_dx && cat) {   // m1_cat_backward's share of dA is served, its kernels' dX side has no arm
    set_error("attn_pool M=1: APA_FLAG_FROZEN_INPUT is not served by the *_cat entry points (concatenated pose "
              "channels): run without the flag");
    return APA_ERR_UNSUPPORTED;
  }
  if (b && (flags & APA_IFLAG_NO_DX) &&
      (c.fused || !c.maskbits_in || !m1_no_dx_supported(C, dtype, c.train) || rng_external(flags))) {
    set_error("attn_pool M=1: NO_DX needs a separate attention input, the forward half's keep bits and the bf16 "
              "streaming kernels (internal)");
    return APA_ERR_UNSUPPORTED;
  }
  if (c.relu_input && !(c.fused && m1s_supported(C, dtype))) {
    set_error("attn_pool M=1: APA_FLAG_RELU_INPUT needs Xatt == X and C in {1024,2048,4096} (f32) / 2048 (bf16)");
    return APA_ERR_UNSUPPORTED;
  }
  if (loss_done && !(c.small && m1_bwd_head_supported(N, C, K))) {
    set_error("attn_pool M=1: fused loss path without the head kernel (internal)");
    return APA_ERR_UNSUPPORTED;
  }
  if (c.ext && !m1g_supported(C, dtype)) {
    set_error("attn_pool M=1: APA_FLAG_RNG_EXTERNAL: C=%d is not served by the generic M == 1 kernels", C);
    return APA_ERR_UNSUPPORTED;
  }
  if (b && (flags & APA_IFLAG_NO_ATT_WGRAD)) {
    if (!c.rank1 || !c.small) {
      set_error("attn_pool M=1: NO_ATT_WGRAD needs the rank-1 dXatt form and the small-K head kernels (internal)");
      return APA_ERR_UNSUPPORTED;
    }
  } else if (c.rank1 && !c.gemv2) {
    set_error("attn_pool M=1: APA_FLAG_DXATT_RANK1: Ca=%d not served by the register-resident GEMV", Ca);
    return APA_ERR_UNSUPPORTED;
  }
  return APA_OK;
}

static int softmax_rows(const M1Call& c, float* att) {
  hipLaunchKernelGGL(m1_softmax_rows_kernel, dim3(c.N), dim3(64), 0, c.st, att, c.P);
  APA_LAUNCH_CHECK("m1_softmax_rows_kernel");
  return APA_OK;
}

template <typename T>
static void att_gemv_fwd(const M1Call& c, const M1Fwd& io) {
  const long NP = (long)c.N * c.P;
  const int nb = (int)((NP + 3) / 4 < 2048 ? (NP + 3) / 4 : 2048);
  hipLaunchKernelGGL(m1_att_gemv_fwd_kernel<T>, dim3(nb), dim3(256), 0, c.st, static_cast<const T*>(io.Xatt), io.Wa,
                     io.ba, io.att, NP, c.Ca, c.act);
}

int m1_forward(const M1Call& c, const M1Fwd& io, M1Xent* xf) {
  const int N = c.N, C = c.C, K = c.K;
  M1Trace* const tr = m1_trace();
  int rc = APA_OK;
  if (!c.fused) {
    // APA_IFLAG_ATT_READY, the fused cfg 003 step: the pose head's Pl kernel already left Z = Xatt . wa + ba (id / relu
    // applied) in att
    if (!(c.flags & APA_IFLAG_ATT_READY)) {
      if (c.dtype == APA_DTYPE_F32) att_gemv_fwd<float>(c, io); else att_gemv_fwd<bf16_t>(c, io);
      APA_LAUNCH_CHECK("m1_att_gemv_fwd_kernel");
    }
    if (c.act == M1_ACT_SOFTMAX && (rc = softmax_rows(c, io.att)) != APA_OK) return rc;
    // att already final: the pooling kernel applies c.pool_act = id
  }
  switch (c.pool) {
    case M1_POOL_STREAM: rc = m1s_launch_pool_fwd(c, io); break;
    case M1_POOL_VEC: rc = m1v_launch_pool_fwd(c, io); break;
    case M1_POOL_FP8: rc = m1f_launch_pool_fwd(c, io); break;
    default: rc = m1g_launch_pool_fwd(c, io);
  }
  if (rc != APA_OK) return rc;
  const int online = (c.fused && c.act == M1_ACT_SOFTMAX) ? 1 : 0;
  // which kernels form the logits: the partial-logits kernel with the row's cross-entropy in its reducer (one-call
  // steps), with the plain reducer, or the split-K product
  const bool xeval = xf && xf->probs;
  if (c.cat) xf = nullptr;   // the extra channels add to the logits after the reduction: no fused loss
  const bool ml = xf && xf->kind != 0;   // a sigmoid loss: its own reducer (apa_mlloss.hip), K <= 1024
  const bool xroute = xf && (ml ? m1_logits_ml_supported(N, C, K) : m1_logits_xent_supported(N, C, K, xeval)) &&
                      m1_small_route_ok(C, K, xf->G, io.Wt, io.zsave, xeval);
  const bool l2route = m1_logits2_supported(C, K) && (reinterpret_cast<uintptr_t>(io.zsave) & 15) == 0;
  // The merge of the S block partials: in the partial-logits kernel's prologue where that is exact and within its
  // budget of 16 loads per lane (identity / relu attention -- the on-line softmax merge and the normalisation of att
  // stay with the finalize kernel --, S <= 16, N < 128, no concatenated channels, 16-byte rows), else a launch of its own
  const bool fold = (xroute || l2route) && !((c.flags | g_m1_iflags) & APA_IFLAG_FINALIZE_LAUNCH) &&
                    c.act != M1_ACT_SOFTMAX && !c.cat && m1_logits2_fold_supported(N, C, c.nrows / N) &&
                    c.pl.S <= 16 &&   // (the reducers' abar: one pstat entry per logical block, 16 at the most)
                    ((reinterpret_cast<uintptr_t>(io.zsave) | reinterpret_cast<uintptr_t>(c.pacc)) & 15) == 0;
  const M1Fold mf{c.pacc, c.pstat, c.pl.S, c.P, c.nrows / N};
  // enough blocks to put every CU to work (the kernel is bound by the bytes each CU loads)
  int cw = 256;
  while (cw > 64 && (long)N * ((C + 4 * cw - 1) / (4 * cw)) < 256) cw >>= 1;
  if (tr) {
    tr->cw = cw;
    g_m1_fwd_route.folded = fold;
    g_m1_fwd_route.launches = (fold ? 0 : 1) + 2;
  }
  if (!fold) {
    hipLaunchKernelGGL(m1_finalize_fwd_kernel, dim3(N, (C + 4 * cw - 1) / (4 * cw)), dim3(256), 0, c.st, c.pacc,
                       c.pstat, c.P, c.pl.S, c.nrows / N, C, online, cw, io.zsave, io.abar, io.att);
    APA_LAUNCH_CHECK("m1_finalize_fwd_kernel");
  }
  // logits = z . Wt + abar (x) bt -- the first reader of Wt / bt (apa_hooks.td_weights_ready_event)
  if (c.td_ready) APA_HIP_CHECK(hipStreamWaitEvent(c.st, c.td_ready, 0));
  if (xroute) {
    // training: the same conditions under which m1_backward takes the head kernel, which finishes loss[0]
    if (ml) {
      if (tr) tr->logits = M1_LOGITS_ML;
      rc = m1_logits2_ml(io.zsave, io.Wt, io.abar, io.bt, *xf, io.logits, c.gemm_ws, N, C, K, c.st, fold ? &mf : nullptr);
      // loss[0]: the backward head kernel's where m1_backward will take it, else one small launch here (same order)
      xf->finished = !m1_bwd_head_supported(N, C, K);
      if (rc == APA_OK && xf->finished)
        rc = clip_loss_finish(nullptr, nullptr, xf->loss, nullptr, nullptr, N, N, K, xf->lscale, c.st);
      xf->done = rc == APA_OK;
      return rc;
    }
    if (tr) tr->logits = xeval ? M1_LOGITS_XENT_PROBS : M1_LOGITS_XENT;
    rc = m1_logits2_xent(io.zsave, io.Wt, io.abar, io.bt, xf->labels, io.logits, xf->loss, xf->G, xf->gscale,
                         xf->probs, xf->pred, c.gemm_ws, N, C, K, c.st, fold ? &mf : nullptr);
    xf->done = rc == APA_OK;
    return rc;
  }
  if (l2route) {
    if (tr) tr->logits = M1_LOGITS2;
    rc = m1_logits2(io.zsave, io.Wt, io.abar, io.bt, io.logits, c.gemm_ws, N, C, K, c.st, fold ? &mf : nullptr);
  } else {
    if (tr) tr->logits = M1_LOGITS_SGEMM;
    rc = sgemm_small(io.zsave, C, 1, io.Wt, K, 1, io.logits, K, N, K, C, c.pl.lsplits, io.abar, io.bt, c.gemm_ws, c.st);
  }
  if (rc != APA_OK || !c.cat) return rc;
  // ..._WITH_POSE_FEAT: logits += zext . Wt[C:C+J]
  return m1_cat_forward(c, io);
}

// Attention-side backward when Xatt != X, over nb blocks: the register-resident form where it serves Ca
template <typename T>
static void att_gemv_bwd(const M1Call& c, const M1Bwd& io, int nb) {
  const long NP = (long)c.N * c.P;
  const int Ca = c.Ca;
  const T* xa = static_cast<const T*>(io.Xatt);
  M1Trace* const tr = m1_trace();
  if (c.gemv2) {
    const int nvec = Ca / Vec<T>::EPV, nthr = ((nvec + 63) / 64) * 64;
    if (tr) tr->gemv = c.rank1 ? M1_GEMV_BWD2_RANK1 : M1_GEMV_BWD2;
    auto go = [&](auto ST) {
      hipLaunchKernelGGL((m1_att_gemv_bwd2_kernel<T, decltype(ST)::value>), dim3(nb), dim3(nthr), 0, c.st, xa, io.Wa,
                         c.dzatt, decltype(ST)::value ? static_cast<T*>(io.dXatt) : nullptr, c.pdwa, c.pdba, NP, Ca);
    };
    if (c.rank1) go(std::false_type{}); else go(std::true_type{});
  } else {
    if (tr) tr->gemv = M1_GEMV_BWD;
    const size_t shm = ((size_t)4 * Ca + 8) * sizeof(float);
    hipLaunchKernelGGL(m1_att_gemv_bwd_kernel<T>, dim3(nb), dim3(256), shm, c.st, xa, io.Wa, c.dzatt,
                       static_cast<T*>(io.dXatt), c.pdwa, c.pdba, NP, Ca);
  }
}

int m1_att_gemv_forward(const M1Call& c, const M1Fwd& io) {
  if (c.dtype == APA_DTYPE_F32) att_gemv_fwd<float>(c, io); else att_gemv_fwd<bf16_t>(c, io);
  APA_LAUNCH_CHECK("m1_att_gemv_fwd_kernel");
  return APA_OK;
}

int m1_att_gemv_backward(const M1Call& c, const M1Bwd& io, int* nred) {
  const long NP = (long)c.N * c.P;
  int nb = (int)((NP + 15) / 16);
  if (nb > 1024) nb = 1024;
  if (nb < 1) nb = 1;
  if (nb > c.pl.nblk) nb = c.pl.nblk;  // partial buffer is sized for nblk rows
  if (c.dtype == APA_DTYPE_F32) att_gemv_bwd<float>(c, io, nb); else att_gemv_bwd<bf16_t>(c, io, nb);
  APA_LAUNCH_CHECK("m1_att_gemv_bwd_kernel");
  *nred = nb;
  return APA_OK;
}

int m1_backward(const M1Call& c, const M1Bwd& io, const M1Xent* xf) {
  const int N = c.N, C = c.C, K = c.K;
  hipStream_t st = c.st;
  M1Trace* const tr = m1_trace();
  int rc;
  if (c.small) {
    // dz = G . Wt^T, dWt = z^T . G, dbt = abar^T G in one launch
    if (m1_bwd_head_supported(N, C, K)) {
      rc = m1_bwd_head(io.G, io.Wt, io.zsave, io.abar, io.bt, c.dz, io.dWt, io.dbt, c.sn, N, C, K, st,
                       xf && xf->done ? xf->loss : nullptr, xf ? xf->lscale : 0.f);
    } else {
      if (tr) tr->head = M1_HEAD_SMALL;
      rc = m1_bwd_small(io.G, io.Wt, io.zsave, io.abar, io.bt, c.dz, io.dWt, io.dbt, c.sn, N, C, K, st);
    }
    if (rc != APA_OK) return rc;
  } else {
    // generic fallback (very large K): dz[n,c] = sum_k G[n,k] Wt[c,k]; dWt[c,k] = sum_n z[n,c] G[n,k]
    if (tr) tr->head = M1_HEAD_SGEMM;
    rc = sgemm_small(io.G, K, 1, io.Wt, 1, K, c.dz, C, N, C, K, 1, nullptr, nullptr, c.gemm_ws, st);
    if (rc != APA_OK) return rc;
    rc = sgemm_small(io.zsave, 1, C, io.G, K, 1, io.dWt, K, C, K, N, 1, nullptr, nullptr, c.gemm_ws, st);
    if (rc != APA_OK) return rc;
  }

  // dWt rows C..C+J-1, dXext, and the extra channels' per-pixel share of dA (c.ex)
  if (c.cat && (rc = m1_cat_backward(c, io)) != APA_OK) return rc;
  // dWt / dbt are final here (fast path): let a data-parallel caller start their all-reduce now
  if (c.small && c.grad_ready) APA_HIP_CHECK(hipEventRecord(c.grad_ready, st));

  switch (c.pool) {
    case M1_POOL_STREAM: rc = m1s_launch_bwd_main(c, io); break;
    case M1_POOL_VEC: rc = m1v_launch_bwd_main(c, io); break;
    case M1_POOL_FP8: rc = m1f_launch_bwd_main(c, io); break;
    default: rc = m1g_launch_bwd_main(c, io);
  }
  if (rc != APA_OK) return rc;

  // APA_IFLAG_NO_ATT_WGRAD, fused cfg 003 step: dWa = Xatt^T dZ and dba = sum dZ ride on the pose head's backward rows
  // kernel (dZ is a 17th column of dPl there), and its column-sum launch advances the dropout counter
  if (c.flags & APA_IFLAG_NO_ATT_WGRAD) return APA_OK;
  int nred = c.pl.nblk;
  int cred = C;
  if (!c.fused) {
    if ((rc = m1_att_gemv_backward(c, io, &nred)) != APA_OK) return rc;
    cred = c.Ca;
  }
  if (tr) { tr->reduce = c.small ? M1_REDUCE_COLSUM : M1_REDUCE_BWD_REDUCE; tr->rng_bump = c.bump != nullptr; }
  if (c.small) {
    ColsumArgs cs;
    cs.pdwa = c.pdwa; cs.pdba = c.pdba; cs.nblk = nred; cs.C = cred; cs.ld = cred; cs.dwa = io.dWa; cs.dba = io.dba;
    cs.rng_bump = c.bump;
    return m1_colsum(cs, st);
  }
  hipLaunchKernelGGL(m1_bwd_reduce_kernel, dim3((cred + 63) / 64 + 1), dim3(256), 0, st, c.pdwa, c.pdba,
                     io.dWa, io.dba, io.abar, io.G, io.dbt, nred, cred, N, K, 1, c.bump);
  APA_LAUNCH_CHECK("m1_bwd_reduce_kernel");
  if (c.grad_ready) APA_HIP_CHECK(hipEventRecord(c.grad_ready, st));   // dbt comes last here
  return APA_OK;
}

}  // namespace apa
