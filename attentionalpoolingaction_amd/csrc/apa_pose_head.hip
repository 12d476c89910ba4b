// apa_pose_head.hip -- the PoseLogits head, built on apa_gemm.hip (nets_factory.py:147-160 of the reference model):
//        Ppre = relu(X.W1 + b1)   [N,P,768]      'PoseLogits/ExtraConv2d_1x1'
//        Pl   = Ppre.W2 + b2      [N,P,J]        'PoseLogits/Conv2d_1c_1x1'
//      and its backward (the reference relies on TF autodiff); pose_fwd_fused / pose_bwd_fused are its halves of the
//      one-call cfg 003 step, pose_eval_fwd its half of the evaluation step.
//      Host layer: a call is described once (PoseCall: shape, stream, workspace and its carve; PoseFwd / PoseBwd: the
//      caller's tensors; PoseStepArgs: what a one-call step adds), refused in one place (pose_check), and every
//      product has one builder: pose_w1_operand, pose_ppre_product, pose_pl_product forward; pose_rows_route picks
//      one of pose_rows_mfma / pose_rows_valu / pose_rows_dppre backward, pose_head_bwd_big is the tail of all three.
#include <type_traits>
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

constexpr int POSE_RB = 8;   // rows per block of the dPpre kernel

// dPpre[r,j] = (sum_q dPl[r,q] W2[j,q] + ext[r,j]) * [Ppre[r,j] > 0]
// plus per-block column partials for db1 (= sum_r dPpre) and db2 (= sum_r dPl).
// Block b owns rows [8b, 8b+8); thread t owns the 4 consecutive columns 4t..4t+3 of all of them
// (8-byte bf16 / 16-byte fp32 accesses, a wave covers 512 B / 1 KiB of a row), with its 4 x J
// slice of W2 in registers.  All 16 row loads are issued before the first is used.
// R1 (apa_pose_head_bwd_rank1ext): the external gradient is rank-1, ext[r,j] = ext_row[r] * ext_col[j]
// (the attention branch of cfg 003: dZ (x) wa) -- formed in registers, no [R,Cp] tensor is read.
template <typename T, int JMAX, bool R1>
__global__ __launch_bounds__(512) void pose_dppre_kernel(const float* __restrict__ dPl,
                                                         const float* __restrict__ W2,
                                                         const T* __restrict__ ext,
                                                         const float* __restrict__ ext_row,
                                                         const float* __restrict__ ext_col,
                                                         const T* __restrict__ Ppre,
                                                         T* __restrict__ dPpre,
                                                         float* __restrict__ partial, long R,
                                                         int Cp, int J) {
  __shared__ __attribute__((aligned(16))) float s_dpl[POSE_RB * JMAX];
  __shared__ float s_er[POSE_RB];
  const int tid = threadIdx.x;
  const long r0 = (long)blockIdx.x * POSE_RB;
  const int nrows = (int)min((long)POSE_RB, R - r0);
  if (R1 && tid < POSE_RB) s_er[tid] = tid < nrows ? ext_row[r0 + tid] : 0.f;
  for (int i = tid; i < POSE_RB * JMAX; i += blockDim.x) {
    const int rr = i / JMAX, q = i - rr * JMAX;
    s_dpl[i] = (dPl && rr < nrows && q < J) ? dPl[(r0 + rr) * J + q] : 0.f;
  }
  const int j0 = tid * 4;
  const bool active = j0 < Cp;          // Cp % 4 == 0 (checked on the host)
  // Row loads: raw vectors, no branch between them (an `if (ext)` per row made hipcc emit
  // load / branch / load / s_waitcnt vmcnt(0) eight times -- eight serial round trips, 17.7 us);
  // a missing `ext` re-reads Ppre and is multiplied by 0.
  typedef typename std::conditional<sizeof(T) == 2, uint2, float4>::type rowvec_t;
  rowvec_t pv[POSE_RB], ev[R1 ? 1 : POSE_RB];
  const T* extp = ext ? ext : Ppre;
  const float extm = (R1 || ext) ? 1.f : 0.f;
  float ecol[4] = {0.f, 0.f, 0.f, 0.f};
  {
    const int j0c = active ? j0 : 0;   // idle threads (Cp/4 not a multiple of 64) load column 0
#pragma unroll
    for (int rr = 0; rr < POSE_RB; ++rr) {
      const size_t off = (size_t)(r0 + min(rr, nrows - 1)) * Cp + j0c;   // surplus rows re-read the last
      pv[rr] = *reinterpret_cast<const rowvec_t*>(Ppre + off);
      if (!R1) ev[rr] = *reinterpret_cast<const rowvec_t*>(extp + off);
    }
    if (R1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) ecol[c] = ext_col[j0c + c];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // (Two attempts to take W2 off the per-lane path -- more rows per block, and a coalesced read +
  // LDS transposition -- both measured SLOWER (22 / 21 us vs 16 us): they cost occupancy, and this
  // kernel lives on having ~5 blocks per CU in flight.)  Ablation of the rank-1 form (14.1 us): without
  // the W2 slice loads 10.3, also without the FMA loop 8.1, also without the output stores 6.6 us --
  // no single phase dominates; each block runs load -> compute -> store once, unpipelined, and only
  // ~3 blocks per CU exist to overlap them.  A multi-group block with explicit prefetch is the next step.
  float w[4][JMAX];
  if (dPl && active && J == JMAX) {   // the 4 x J slice of W2 is one contiguous, 16-byte aligned span
    const float4* wsrc = reinterpret_cast<const float4*>(W2 + (size_t)j0 * J);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < JMAX; q += 4) {
        const float4 t = wsrc[(c * JMAX + q) >> 2];
        w[c][q] = t.x; w[c][q + 1] = t.y; w[c][q + 2] = t.z; w[c][q + 3] = t.w;
      }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int q = 0; q < JMAX; ++q) w[c][q] = (dPl && active && q < J) ? W2[(size_t)(j0 + c) * J + q] : 0.f;
  }
  __syncthreads();
  float* prow = partial + (size_t)blockIdx.x * (Cp + J);
  if (active) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int rr = 0; rr < POSE_RB; ++rr) {
      float o[4], x[4], pp[4];
      if constexpr (sizeof(T) == 2) {
        pp[0] = bf16_lo(pv[rr].x); pp[1] = bf16_hi(pv[rr].x); pp[2] = bf16_lo(pv[rr].y); pp[3] = bf16_hi(pv[rr].y);
        if constexpr (!R1) {
          x[0] = bf16_lo(ev[rr].x); x[1] = bf16_hi(ev[rr].x); x[2] = bf16_lo(ev[rr].y); x[3] = bf16_hi(ev[rr].y);
        }
      } else {
        pp[0] = pv[rr].x; pp[1] = pv[rr].y; pp[2] = pv[rr].z; pp[3] = pv[rr].w;
        if constexpr (!R1) { x[0] = ev[rr].x; x[1] = ev[rr].y; x[2] = ev[rr].z; x[3] = ev[rr].w; }
      }
      if constexpr (R1) {
        const float er = s_er[rr];
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = er * ecol[c];
      }
      // the row's dPl values: read from LDS ONCE (4 x ds_read_b128) and kept in registers for the four
      // columns -- indexed in place hipcc re-read them per column: 128 dependent LDS reads per thread
      float d[JMAX];
#pragma unroll
      for (int q = 0; q < JMAX; q += 4) {
        const float4 t = *reinterpret_cast<const float4*>(s_dpl + rr * JMAX + q);
        d[q] = t.x; d[q + 1] = t.y; d[q + 2] = t.z; d[q + 3] = t.w;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float sv = x[c] * extm;
        if (dPl) {
#pragma unroll
          for (int q = 0; q < JMAX; ++q) sv = fmaf(d[q], w[c][q], sv);
        }
        o[c] = pp[c] > 0.f ? sv : 0.f;
        acc[c] += rr < nrows ? o[c] : 0.f;
      }
      if (rr < nrows) {
        const size_t off = (size_t)(r0 + rr) * Cp + j0;
        if constexpr (sizeof(T) == 2)
          *reinterpret_cast<uint2*>(dPpre + off) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        else
          *reinterpret_cast<float4*>(dPpre + off) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) prow[j0 + c] = acc[c];   // (Cp + J need not be a multiple of 4)
  }
  if (tid < J) {
    float a = 0.f;
    for (int rr = 0; rr < nrows; ++rr) a += s_dpl[rr * JMAX + tid];
    prow[Cp + tid] = a;
  }
}

// Round 2: the whole "small side" of the pose-head backward in ONE pass over Ppre (J <= 16):
//   dPpre[r,c] = (sum_q dPl[r,q] W2[c,q] + ext[r,c]) * [Ppre[r,c] > 0]          (written, bf16 / fp32)
//   db1[c] = sum_r dPpre[r,c]    db2[q] = sum_r dPl[r,q]    dW2[c,q] = sum_r Ppre[r,c] dPl[r,q]
// The last three leave as ONE partial row per block, [dW2 (Cp*J) | db1 (Cp) | db2 (J)], reduced in fixed
// order by a single m1_colsum launch.  Before: pose_dppre_kernel (13.2 us) + a split-K MFMA GEMM with 16
// useful output columns (11.8 us) + its reduce (5.3 us) + colsum (4.5 us), and Ppre was read twice.
// Block = RPB rows, thread = 2 consecutive columns of every row (its 2 x 16 slice of W2 and its
// 2 x 16 dW2 accumulators in registers; exact fp32 FMAs, dPl is not rounded to bf16 as the MFMA path did).
// Every row load of a block is issued up front (one HBM latency per block); surplus rows of the last block
// re-read row R-1 and meet dPl = 0 / ext_row = 0.
constexpr int POSE_RPB_MIN = 16;   // smallest rows-per-block variant (sizes the partial matrix)
// leading dimension (floats) of the rows kernel's partial matrix: [dW2 | db1 | db2]; with J == 16 the dW2
// part is padded to 32 floats per thread of the block (permuted layout, see the kernel's epilogue)
// ... followed (WA form of the kernel: the fused cfg 003 step) by [dWa (Cp) | dba (1)], padded to 4 floats
__host__ __device__ static inline size_t pose_rows_dw2(int Cp, int J, int nthr) {
  return J == 16 ? (size_t)nthr * 32 : (size_t)Cp * J;
}
__host__ __device__ static inline size_t pose_rows_ld(int Cp, int J, int nthr) {
  return pose_rows_dw2(Cp, J, nthr) + Cp + J + Cp + 4;
}
// WA (with R1: ext_row = dZ, ext_col = wa): the attention conv's own gradients, dWa[c] = sum_r Ppre[r,c] dZ[r] and
// dba = sum_r dZ[r], leave with the same partial row -- dZ is a 17th column of dPl as far as dW2 is concerned --
// so m1_att_gemv_bwd2_kernel's pass over Ppre and its column-sum launch disappear from the cfg 003 step.
template <typename T, bool R1, bool EXT, int RPB, bool WA = false>
__global__ __launch_bounds__(512) void pose_bwd_rows_kernel(
    const float* __restrict__ dPl, const float* __restrict__ W2, const T* __restrict__ ext,
    const float* __restrict__ ext_row, const float* __restrict__ ext_col, const T* __restrict__ Ppre,
    T* __restrict__ dPpre, float* __restrict__ partial, long R, int Cp, int J) {
  // The block's [RPB][Cp] tile of Ppre (and of ext) is parked in LDS, one slot per thread and row, written
  // and read by the same thread: a register file extension that a REAL loop can index.  (With the rows in
  // registers the row loop has to be unrolled, and hipcc then reorders the 32 x 64 FMAs at will -- it sank
  // the dW2 chains below everything else and spilled every row's dPl values, 2 KB of scratch per lane.)
  typedef typename std::conditional<sizeof(T) == 2, uint32_t, float2>::type rowvec_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* s_dpl = reinterpret_cast<float*>(s_raw);                       // [RPB][16]
  float* s_er = s_dpl + RPB * 16;                                       // [RPB]
  rowvec_t* s_pp = reinterpret_cast<rowvec_t*>(s_er + RPB);             // [RPB][nthr]
  rowvec_t* s_ext = s_pp + (EXT ? RPB * blockDim.x : 0);                // [RPB][nthr]
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long r0 = (long)blockIdx.x * RPB;
  const int nrows = (int)min((long)RPB, R - r0);
  const int c0 = tid * 2;
  const bool active = c0 < Cp;
  const int c0c = active ? c0 : 0;   // idle threads (Cp/2 not a multiple of 64) shadow column 0
  {  // every row of the block is requested before anything else happens: one HBM latency per block
    rowvec_t pv[RPB], ev[EXT ? RPB : 1];
#pragma unroll
    for (int u = 0; u < RPB; ++u) {
      const size_t off = (size_t)min(r0 + u, R - 1) * Cp + c0c;   // surplus rows re-read row R-1
      pv[u] = *reinterpret_cast<const rowvec_t*>(Ppre + off);
      if (EXT) ev[u] = *reinterpret_cast<const rowvec_t*>(ext + off);
    }
#pragma unroll 1
    for (int i = tid; i < RPB * 16; i += nthr) {
      const int rr = i >> 4, q = i & 15;
      s_dpl[i] = (rr < nrows && q < J) ? dPl[(r0 + rr) * J + q] : 0.f;
    }
    if (R1 && tid < RPB) s_er[tid] = tid < nrows ? ext_row[r0 + tid] : 0.f;
#pragma unroll
    for (int u = 0; u < RPB; ++u) {
      s_pp[u * nthr + tid] = pv[u];
      if (EXT) s_ext[u * nthr + tid] = ev[u];
    }
  }
  // packed fp32 math (v_pk_fma_f32): wq[q] = (W2[c0][q], W2[c0+1][q]) pairs the thread's two columns, so
  // the dPpre chains are sv2 += d[q] * wq[q]; the dW2 accumulators a[c][q..q+1] += pp[c] * (d[q], d[q+1]).
  typedef float v2f __attribute__((ext_vector_type(2)));
  v2f wq[16];
  if (J == 16) {   // 2 x 16 floats = one contiguous 128-byte span
    const float4* wsrc = reinterpret_cast<const float4*>(W2 + (size_t)c0c * 16);
    float4 t[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) t[v] = wsrc[v];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      wq[v * 4] = v2f{t[v].x, t[v + 4].x}; wq[v * 4 + 1] = v2f{t[v].y, t[v + 4].y};
      wq[v * 4 + 2] = v2f{t[v].z, t[v + 4].z}; wq[v * 4 + 3] = v2f{t[v].w, t[v + 4].w};
    }
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) {   // clamped index + select: no branch between the loads
      const float t0 = W2[(size_t)c0c * J + min(q, J - 1)];
      const float t1 = W2[(size_t)(c0c + 1) * J + min(q, J - 1)];
      wq[q] = q < J ? v2f{t0, t1} : v2f{0.f, 0.f};
    }
  }
  v2f ecol = {0.f, 0.f};
  if (R1) ecol = v2f{ext_col[c0c], ext_col[c0c + 1]};
  v2f acc = {0.f, 0.f}, awa = {0.f, 0.f};
  v2f a[2][8];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int h = 0; h < 8; ++h) a[c][h] = v2f{0.f, 0.f};
  __syncthreads();
  T* orow = dPpre + (size_t)r0 * Cp + c0;
  // one row ahead: the next row's tile slot, ext_row entry and 16 dPl values are read from LDS before the
  // current row's FMAs (slot RPB-1 is re-read past the end; nothing is done with it)
  auto ld_row = [&](int rr, rowvec_t& pr, rowvec_t& xr, float& er, float4 (&d4)[4]) {
    const int r = min(rr, RPB - 1);
    pr = s_pp[r * nthr + tid];
    if (EXT) xr = s_ext[r * nthr + tid];
    if (R1) er = s_er[r];
#pragma unroll
    for (int v = 0; v < 4; ++v) d4[v] = *reinterpret_cast<const float4*>(s_dpl + r * 16 + v * 4);
  };
  rowvec_t prn = rowvec_t(), xrn = rowvec_t();
  float ern = 0.f;
  float4 dn[4];
  ld_row(0, prn, xrn, ern, dn);
#pragma unroll 2
  for (int rr = 0; rr < nrows; ++rr) {
    const rowvec_t pr = prn, xr = xrn;
    const float er = ern;
    v2f d2[8];
#pragma unroll
    for (int v = 0; v < 4; ++v) { d2[2 * v] = v2f{dn[v].x, dn[v].y}; d2[2 * v + 1] = v2f{dn[v].z, dn[v].w}; }
    ld_row(rr + 1, prn, xrn, ern, dn);
    v2f pp, x = {0.f, 0.f};
    if constexpr (sizeof(T) == 2) pp = v2f{bf16_lo(pr), bf16_hi(pr)};
    else pp = v2f{pr.x, pr.y};
    if constexpr (EXT) {
      if constexpr (sizeof(T) == 2) x = v2f{bf16_lo(xr), bf16_hi(xr)};
      else x = v2f{xr.x, xr.y};
    }
    if constexpr (R1) x = ecol * er;
    v2f sv = x, sv_b = {0.f, 0.f};   // two chains of 8
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      sv = __builtin_elementwise_fma(v2f{d2[h].x, d2[h].x}, wq[2 * h], sv);
      sv_b = __builtin_elementwise_fma(v2f{d2[h].y, d2[h].y}, wq[2 * h + 1], sv_b);
    }
    sv += sv_b;
    v2f o = {pp.x > 0.f ? sv.x : 0.f, pp.y > 0.f ? sv.y : 0.f};
    acc += o;
    if constexpr (WA) awa = __builtin_elementwise_fma(pp, v2f{er, er}, awa);
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      a[0][h] = __builtin_elementwise_fma(v2f{pp.x, pp.x}, d2[h], a[0][h]);
      a[1][h] = __builtin_elementwise_fma(v2f{pp.y, pp.y}, d2[h], a[1][h]);
    }
    if (active) {
      if constexpr (sizeof(T) == 2) *reinterpret_cast<uint32_t*>(orow) = pack_bf16x2(o.x, o.y);
      else *reinterpret_cast<float2*>(orow) = make_float2(o.x, o.y);
    }
    orow += Cp;
  }
  // Partial row of the block: [dW2 | db1 | db2].  J == 16: the dW2 part is stored PERMUTED so that every
  // wave-instruction writes 1 KiB of consecutive bytes -- float4 number v of thread t (v = 4c + q/4) goes
  // to float offset (v * nthr + t) * 4; m1_colsum undoes the permutation when it writes dW2.  (In natural
  // [c][q] order each lane's 128 bytes are contiguous and every store touches 64 different lines: 4.3 us.)
  float* prow = partial + (size_t)blockIdx.x * pose_rows_ld(Cp, J, nthr);
  const size_t dw2_cols = pose_rows_dw2(Cp, J, nthr);
  {
    if (J == 16) {
      float4* dst = reinterpret_cast<float4*>(prow) + tid;
#pragma unroll
      for (int v = 0; v < 8; ++v)
        dst[(size_t)v * nthr] = make_float4(a[v >> 2][(v & 3) * 2].x, a[v >> 2][(v & 3) * 2].y,
                                            a[v >> 2][(v & 3) * 2 + 1].x, a[v >> 2][(v & 3) * 2 + 1].y);
    } else if (active) {
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int h = 0; h < 8; ++h) {
          if (2 * h < J) prow[(size_t)(c0 + c) * J + 2 * h] = a[c][h].x;
          if (2 * h + 1 < J) prow[(size_t)(c0 + c) * J + 2 * h + 1] = a[c][h].y;
        }
    }
    if (active) *reinterpret_cast<float2*>(prow + dw2_cols + c0) = make_float2(acc.x, acc.y);
  }
  if (tid < J) {
    float sdb = 0.f;
    for (int rr = 0; rr < nrows; ++rr) sdb += s_dpl[rr * 16 + tid];
    prow[dw2_cols + Cp + tid] = sdb;
  }
  if constexpr (WA) {
    float* wrow = prow + dw2_cols + Cp + J;
    if (active) { wrow[c0] = awa.x; wrow[c0 + 1] = awa.y; }
    if (tid == 0) {
      float sdz = 0.f;
      for (int rr = 0; rr < nrows; ++rr) sdz += s_er[rr];
      wrow[Cp] = sdz;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// MFMA form of the rows pass (round 6; bf16 features, J == 16, Cp a multiple of 128, rank-1 or no external
// gradient).  The VALU form above spends 16 us at the benchmark shape on 2 x 17 fp32 FMAs per element of the
// [6272 x 768] map (SQ: MFMA 0.000, `active` 0.46); both contractions are 16 deep, i.e. ONE k step of the matrix
// pipe each once the fp32 operand is split into a bf16 head and a bf16 remainder (x = hi + lo exactly to 2^-17):
//     dPpre^T tile [16 c x 16 r] = [W2hi | W2hi] . [dPlhi ; dPllo]  +  [W2lo | 0] . [dPlhi ; 0]        (k = 32)
//     dW2^T tile   [16 q x 16 c] = dPlhi^T . Ppre + dPllo^T . Ppre                                     (k = 32 rows)
// so what is dropped is lo x lo (2^-18 relative): the result is the fp32 kernel's to ~1e-5, far inside the bf16
// store of dPpre.  Block = 32 rows x all Cp columns, parked once in LDS ([32][Cp + 8] bf16, 16-byte vectors);
// wave w owns channels [128 w, 128 w + 128):
//   * dW2 / dWa first (the tile is the k-major B operand: ds_read_b64_tr_b16), written TRANSPOSED -- D[q][c] puts a
//     lane's four registers on four consecutive q of one channel: one float4 per lane, 1 KB per wave-store, in the
//     natural [c][q] order (the permuted layout of the VALU form is not needed);
//   * then dPpre, also transposed (M = channels): a lane holds four CONSECUTIVE channels of one row, reads the four
//     Ppre values it gates with (8 bytes of the tile), adds the rank-1 term dZ[r] wa[c] in fp32, writes the bf16
//     result back IN PLACE; db1 leaves through a 16-lane DPP row sum;
//   * the finished tile is streamed out as 16-byte row segments.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void split_bf16x8(const float (&x)[8], short (&hi)[8], short (&lo)[8]) {
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const uint32_t h = pack_bf16x2(x[e], x[e + 1]);
    const uint32_t l = pack_bf16x2(x[e] - bf16_lo(h), x[e + 1] - bf16_hi(h));
    hi[e] = (short)(h & 0xffffu); hi[e + 1] = (short)(h >> 16);
    lo[e] = (short)(l & 0xffffu); lo[e + 1] = (short)(l >> 16);
  }
}

template <bool R1, bool WA>
__global__ __launch_bounds__(512) void pose_bwd_rows_mfma_kernel(
    const float* __restrict__ dPl, const float* __restrict__ W2, const float* __restrict__ ext_row,
    const float* __restrict__ ext_col, const bf16_t* __restrict__ Ppre, bf16_t* __restrict__ dPpre,
    float* __restrict__ partial, long R, int Cp, size_t ldp, int G) {
  typedef short bf16x8 __attribute__((ext_vector_type(8)));
  typedef short bf16x4 __attribute__((ext_vector_type(4)));
  typedef bf16x4 __attribute__((address_space(3))) * lds_v4;
  constexpr int RPB = 32, DLD = 20;
  constexpr int CT = 4;             // 16-channel tiles per wave (8 spilled: 64 + 64 + 32 fragment / accumulator registers)
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  // blockIdx.y = channel group: the block's waves own channels [gbase, gbase + 16 CT blockDim.x / 64).  blockIdx.x = row
  // block of G groups of 32 rows, taken one after the other with the weight-gradient accumulators kept in registers:
  // ONE partial row per 32 G rows (with a partial row per 32 rows -- 55 KB each -- a third of the kernel's traffic was
  // partials, and the column sum behind it read 196 of them).
  const int CB = (blockDim.x >> 6) * (16 * CT), gbase = blockIdx.y * CB;
  const int LDT = CB + 8;
  short* tile = reinterpret_cast<short*>(s_raw);                  // [32][CB + 8] bf16
  float* s_dpl = reinterpret_cast<float*>(tile + RPB * LDT);      // [32][20]
  float* s_er = s_dpl + RPB * DLD;                                // [32]
  const int tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kb = lane >> 4;
  const int vpr = CB / 8;                                         // 16-byte vectors per row; 32 vpr == CT nthr
  const int cbase = wave * (16 * CT), q0 = 8 * (kb & 1);   // cbase: within the tile; + gbase: within the map

  // this lane's W2 rows as MFMA A fragments, once: channel gbase + cbase + 16 ct + l16, k blocks [hi | hi] and [lo | 0]
  bf16x8 a1[CT], a2v[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const float4* wsrc = reinterpret_cast<const float4*>(W2 + (size_t)(gbase + cbase + ct * 16 + l16) * 16 + q0);
    const float4 w0 = wsrc[0], w1 = wsrc[1];
    const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    short hi[8], lo[8];
    split_bf16x8(wv, hi, lo);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      a1[ct][e] = hi[e];
      a2v[ct][e] = kb < 2 ? lo[e] : (short)0;
    }
  }
  f32x4 accw[CT], acca[WA ? CT : 1];
  float osum[CT][4];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    accw[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (WA) acca[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 4; ++g) osum[ct][g] = 0.f;
  }
  float sdb = 0.f, sdz = 0.f;                 // db2 (threads < 16 of channel group 0) / dba (its last thread)

  // one group ahead through registers: group g + 1's rows (and its dPl / dZ values) are requested between the two
  // MFMA phases of group g and parked in LDS when g's finished tile has left
  uint4 buf[CT];
  float4 dplv = make_float4(0.f, 0.f, 0.f, 0.f);
  float erv = 0.f;
  auto request = [&](int grp) {
    const long r0 = ((long)blockIdx.x * G + grp) * RPB;
    const int nrows = (int)max(0L, min((long)RPB, R - r0));
#pragma unroll
    for (int i = 0; i < CT; ++i) {
      const int vi = tid + i * nthr, row = vi / vpr, v = vi - row * vpr;
      buf[i] = ld16(Ppre + (size_t)max(0L, min(r0 + row, R - 1)) * Cp + gbase + v * 8);   // surplus rows re-read row R - 1 (dPl = 0 there)
    }
    dplv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < 128 && (tid >> 2) < nrows) dplv = *reinterpret_cast<const float4*>(dPl + (size_t)(r0 + (tid >> 2)) * 16 + (tid & 3) * 4);
    erv = 0.f;
    if (R1 && tid >= nthr - 32 && tid - (nthr - 32) < nrows) erv = ext_row[r0 + tid - (nthr - 32)];
  };
  request(0);
  for (int grp = 0; grp < G; ++grp) {
    const long r0 = ((long)blockIdx.x * G + grp) * RPB;
    if (r0 >= R) break;                       // (block-uniform)
    const int nrows = (int)min((long)RPB, R - r0);
    // ---- phase 0: park the group's operands in LDS ----
    if (grp > 0) __syncthreads();             // the previous group's tile has been streamed out
    if (tid < 128) *reinterpret_cast<float4*>(s_dpl + (tid >> 2) * DLD + (tid & 3) * 4) = dplv;
    if (tid >= nthr - 32) s_er[tid - (nthr - 32)] = erv;
#pragma unroll
    for (int i = 0; i < CT; ++i) {
      const int vi = tid + i * nthr, row = vi / vpr, v = vi - row * vpr;
      *reinterpret_cast<uint4*>(tile + row * LDT + v * 8) = buf[i];
    }
    __syncthreads();

    // ---- phase 1: dW2^T (and dWa) tiles: A = dPl^T (m = q = l16, k = row 8 kb + i), B = the tile, k-major ----
    {
      float dv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) dv[i] = s_dpl[(8 * kb + i) * DLD + l16];
      short hi[8], lo[8];
      split_bf16x8(dv, hi, lo);
      const bf16x8 ahi = {hi[0], hi[1], hi[2], hi[3], hi[4], hi[5], hi[6], hi[7]};
      const bf16x8 alo = {lo[0], lo[1], lo[2], lo[3], lo[4], lo[5], lo[6], lo[7]};
      bf16x8 az = {0, 0, 0, 0, 0, 0, 0, 0};
      if (WA) {                               // row m = 0: head of dZ, row m = 1: remainder; the two result rows are added
        float ev[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ev[i] = s_er[8 * kb + i];
        short eh[8], el[8];
        split_bf16x8(ev, eh, el);
#pragma unroll
        for (int i = 0; i < 8; ++i) az[i] = l16 == 0 ? eh[i] : (l16 == 1 ? el[i] : (short)0);
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const short* s0 = tile + (kb * 8 + (l16 >> 2)) * LDT + cbase + ct * 16 + 4 * (l16 & 3);
        const bf16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(s0));
        const bf16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(s0 + 4 * LDT));
        const bf16x8 bfr = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
        accw[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ahi, bfr, accw[ct], 0, 0, 0);
        accw[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bfr, accw[ct], 0, 0, 0);
        if (WA) acca[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bfr, acca[ct], 0, 0, 0);
      }
    }
    if (blockIdx.y == 0) {
      if (tid < 16) {                         // db2[q] += sum_r dPl[r][q] (fixed order)
        for (int rr = 0; rr < nrows; ++rr) sdb += s_dpl[rr * DLD + tid];
      } else if (WA && tid == nthr - 1) {     // dba += sum_r dZ[r]
        for (int rr = 0; rr < nrows; ++rr) sdz += s_er[rr];
      }
    }
    __syncthreads();                          // every wave is done reading the tile as an operand
    if (grp + 1 < G) request(grp + 1);        // (flies under phase 2 and the stores of phase 3)

    // ---- phase 2: dPpre^T tiles: A = W2 (m = channel), B = dPl^T (n = row), gate + rank-1 term, in place ----
    {
      bf16x8 b1[2], b2[2];
      float er2[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const float* dsrc = s_dpl + (rt * 16 + l16) * DLD + q0;
        const float4 d0 = *reinterpret_cast<const float4*>(dsrc), d1 = *reinterpret_cast<const float4*>(dsrc + 4);
        const float dv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        short hi[8], lo[8];
        split_bf16x8(dv, hi, lo);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          b1[rt][e] = kb < 2 ? hi[e] : lo[e];
          b2[rt][e] = kb < 2 ? hi[e] : (short)0;
        }
        er2[rt] = s_er[rt * 16 + l16];
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        float4 wa4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (R1) wa4 = *reinterpret_cast<const float4*>(ext_col + gbase + cbase + ct * 16 + 4 * kb);
        const float wa[4] = {wa4.x, wa4.y, wa4.z, wa4.w};
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[ct], b1[rt], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2v[ct], b2[rt], acc, 0, 0, 0);
          // D[channel 4 kb + reg][row l16]
          short* tp = tile + (rt * 16 + l16) * LDT + cbase + ct * 16 + 4 * kb;
          const uint2 pv = *reinterpret_cast<const uint2*>(tp);
          const float pp[4] = {bf16_lo(pv.x), bf16_hi(pv.x), bf16_lo(pv.y), bf16_hi(pv.y)};
          float o[4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const float x = R1 ? fmaf(er2[rt], wa[g], acc[g]) : acc[g];
            o[g] = pp[g] > 0.f ? x : 0.f;
            osum[ct][g] += o[g];
          }
          *reinterpret_cast<uint2*>(tp) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        }
      }
    }
    __syncthreads();
    // ---- phase 3: the finished dPpre tile leaves as 16-byte row segments ----
#pragma unroll
    for (int i = 0; i < CT; ++i) {
      const int vi = tid + i * nthr, row = vi / vpr, v = vi - row * vpr;
      if (row < nrows)
        st16(dPpre + (size_t)(r0 + row) * Cp + gbase + v * 8, *reinterpret_cast<const uint4*>(tile + row * LDT + v * 8));
    }
  }

  // ---- the block's partial row: [dW2 (natural [c][q]) | db1 | db2 (| dWa | dba)] ----
  float* prow = partial + (size_t)blockIdx.x * ldp;
  const size_t dw2_cols = (size_t)Cp * 16;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    // D[q = 4 kb + reg][c = l16]  ->  dW2[c][q]: four consecutive floats per lane, 1 KB per wave-store
    *reinterpret_cast<float4*>(prow + (size_t)(gbase + cbase + ct * 16 + l16) * 16 + 4 * kb) =
        make_float4(accw[ct][0], accw[ct][1], accw[ct][2], accw[ct][3]);
    if (WA && kb == 0) prow[dw2_cols + Cp + 16 + gbase + cbase + ct * 16 + l16] = acca[ct][0] + acca[ct][1];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float s2 = row_sum16(osum[ct][g]);
      if (l16 == 0) prow[dw2_cols + gbase + cbase + ct * 16 + 4 * kb + g] = s2;
    }
  }
  if (blockIdx.y == 0) {
    if (tid < 16) prow[dw2_cols + Cp + tid] = sdb;
    else if (WA && tid == nthr - 1) prow[dw2_cols + Cp + 16 + Cp] = sdz;
  }
}

// ---------------------------------------------------------------------------------------------
// Which rows pass serves a backward call.  The three facts every form turns on -- the block's thread count, the LDS
// bound and the operand alignments -- are stated here and nowhere else.
// ---------------------------------------------------------------------------------------------
// threads of a rows-kernel block: one per 2 columns, whole waves (the MFMA form's Cp % 128 == 0 makes it Cp / 2)
static int pose_rows_nthr(int Cp) { return ((Cp / 2 + 63) / 64) * 64; }

static bool pose_rows_mfma_ok(const PoseCall& c, const PoseBwd& b) {
  const uintptr_t al = reinterpret_cast<uintptr_t>(b.dPl) | reinterpret_cast<uintptr_t>(b.W2) |
                       reinterpret_cast<uintptr_t>(b.Ppre) | reinterpret_cast<uintptr_t>(b.ext_col);
  return c.dtype == APA_DTYPE_BF16 && b.dPl && c.J == 16 && c.Cp % 128 == 0 && c.Cp >= 256 && c.Cp <= 1024 &&
         (al & 15) == 0 && (!b.dPpre_ext || b.ext_row);
}

// LDS bytes of one block: dPl rows + ext_row + the [rpb][nthr] tile(s)
static size_t pose_rows_lds(int rpb, int nthr, int dtype, bool ext) {
  return (size_t)rpb * 17 * 4 + (size_t)rpb * nthr * (dtype == APA_DTYPE_BF16 ? 4 : 8) * (ext ? 2 : 1);
}
// rows per block: 32 (half the partial matrix: its write and the column sum that follows are what the
// choice moves -- cfg 003 at N = 32, 196 blocks of 32 rows against 392 of 16: kernel 16.9 vs 17.5 us, column sum
// 4.6 vs 6.9 us, step -3 us in four interleaved pairs) once that still gives half the CUs a block and the tile
// stays under the 64 KB a launch gets without opting in, else 16
static int pose_rows_per_block(long R, int nthr, int dtype, bool ext) {
  int rpb = (R + 31) / 32 >= 128 ? 32 : 16;
  if (rpb == 32 && pose_rows_lds(32, nthr, dtype, ext) > 65536) rpb = 16;
  return rpb;
}

static bool pose_bwd_rows_ok(const PoseCall& c, const PoseBwd& b) {
  const uintptr_t al = reinterpret_cast<uintptr_t>(b.Ppre) | reinterpret_cast<uintptr_t>(b.dPpre_ext);
  return b.dPl && c.J <= 16 && c.Cp % 4 == 0 && c.Cp <= 1024 && (al & 7) == 0 &&
         (c.J != 16 || (reinterpret_cast<uintptr_t>(b.W2) & 15) == 0) &&
         (c.dtype == APA_DTYPE_BF16 || c.dtype == APA_DTYPE_F32) &&
         pose_rows_lds(16, pose_rows_nthr(c.Cp), c.dtype, b.dPpre_ext != nullptr) <= 65536;
}

// one pass over Ppre on the matrix pipe, the same pass on the VALU, or the chunk kernel plus a dW2 product of its own
static PoseRows pose_rows_route(const PoseCall& c, const PoseBwd& b) {
  if (!pose_bwd_rows_ok(c, b)) return POSE_ROWS_DPPRE;
  return pose_rows_mfma_ok(c, b) ? POSE_ROWS_MFMA : POSE_ROWS_VALU;
}

// Pl = Ppre . W2 + b2 for bf16 features: [R, Cp] x [Cp, J <= 16] -- 16 output columns, so a 128-wide GEMM
// tile wastes 7/8 of its MFMAs and needs split-K plus a reduce launch (11.6 + 5.2 us at R = 6272).  Here
// a wave owns 16 rows: its A fragments come straight from global memory (one 16-byte load per lane and
// k step, all KS of them in flight at once), the whole W2 sits in registers as bf16 B fragments (staged
// once per block through LDS), KS MFMAs later the 16 x 16 result leaves with the bias added.  HBM-bound
// on the 9.6 MB pre-logit map.  (Fewer waves per block to cover more CUs -- 98 blocks at N = 32 -- measured slower:
// 4 / 2 / 1 waves 7.4 / 8.0 / 11.6 us, every block stages the whole of W2.)
// FUSED (the one-call cfg 003 step, apa_pose_attn_train_step): on the same pass over Ppre
//   * the attention logits Z[r] = Ppre[r,:] . wa + ba of the pose-prelogits-based attention (nets_factory.py:
//     247-270, M = 1; id / relu applied, softmax left raw) -- exact fp32 FMAs on the A fragments the lanes already
//     hold (wa is NOT rounded to bf16), the four k-quarters of a row added across lanes: one launch and one
//     read of the 9.6 MB map less than m1_att_gemv_fwd_kernel;
//   * the pose L2 loss of src/loss.py:29-70 on the finished Pl tile: dPl = gcoef * valid * (Pl - lbl) (the
//     expression of pose_l2_kernel, bit for bit) and one partial sum of valid * (Pl - lbl)^2 per block.
// W2 staging: a thread converts the k pair (2kp, 2kp + 1) of four columns and writes four 32-bit words (2-way
// bank aliasing at most, free for ds_write_b32; the 2-byte scatter it replaces showed an LDS conflict ratio of
// 0.50 in the SQ counters), rows padded by 16 so that the ds_read_b128 fragment reads are conflict-free.
// W2T (round 5): the LDS image of W2 -- [16][Cp + 16] bf16, rows padded for conflict-free fragment reads -- is a
// verbatim copy of a caller-kept image of W2^T in the same layout, fetched by LDS-DMA (25 wave-instructions per block):
// half the bytes of the fp32 W2, no conversion, no ds_write pass (the 2-byte-pair scatter had an LDS conflict ratio of
// 0.29).  With the staging that cheap a block is TWO waves (32 rows, 196 blocks at the benchmark shape: every CU
// ingests 49 + 25 KB instead of 98 + 49 KB; with the fp32 staging smaller blocks measured slower).  First try, B
// fragments loaded straight from the global image by every lane: 10.2 us against 8.5 -- 24 KB per WAVE through the
// CU's one memory pipe.
struct PosePlExtra {
  const float* wa; const float* ba; float* att; int act;                                   // wa == nullptr: off
  const float* lbl; const uint8_t* valid; float* dPl; float* lpart; float gcoef; int P;    // lbl == nullptr: off
  const bf16_t* w2t;                                                                        // W2T form only
};
template <int KS, bool FUSED, bool W2T = false>   // k steps of 32: Cp = 32 * KS
__global__ __launch_bounds__(256) void pose_pl_kernel(const bf16_t* __restrict__ Ppre,
                                                      const float* __restrict__ W2,
                                                      const float* __restrict__ b2, float* __restrict__ Pl,
                                                      int R, int J, PosePlExtra x) {
  typedef short bf16x8 __attribute__((ext_vector_type(8)));
  constexpr int Cp = 32 * KS, LDW = Cp + 16;
  constexpr int WPB = W2T ? 2 : 4;                                   // waves per block (blockDim.x = 64 WPB)
  constexpr int NCH = (16 * LDW * 2 + 1023) / 1024;                  // KiB chunks of the image (W2T: DMA instructions)
  __shared__ __attribute__((aligned(16))) short w2s[W2T ? NCH * 512 : 16 * LDW];   // [n][k] bf16, zero rows for n >= J
  __shared__ __attribute__((aligned(16))) float was[FUSED ? Cp : 4];
  __shared__ float lred[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int l16 = lane & 15, kb = lane >> 4;
  const int r0 = (blockIdx.x * WPB + wave) * 16;
  if constexpr (W2T) {   // first of all: the image is on its way while the A fragments are requested
    typedef __attribute__((address_space(1))) const void* gptr;
    typedef __attribute__((address_space(3))) void* lptr;
    const char* img = reinterpret_cast<const char*>(x.w2t);
    for (int ch = wave; ch < NCH; ch += WPB) {
      const int off = min(ch * 1024 + lane * 16, 16 * LDW * 2 - 16);     // (the last chunk is ragged: clamped re-reads)
      __builtin_amdgcn_global_load_lds((gptr)(img + off), (lptr)(w2s + ch * 512), 16, 0, 0);
    }
  }
  // A fragments first: they are the long-latency loads
  bf16x8 af[KS];
  const bf16_t* arow = Ppre + (size_t)min(r0 + l16, R - 1) * Cp + kb * 8;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const uint4 v = ld16(arow + ks * 32);
    af[ks] = __builtin_bit_cast(bf16x8, v);
  }

  // fused loss: this lane's four label values and validity flags are requested now, next to the A fragments (read after
  // the MFMA chain they were a second exposed round trip: the fused launch took 9.9 us against 6.0 us for Pl alone)
  float lblv[4] = {0.f, 0.f, 0.f, 0.f};
  float vmv[4] = {0.f, 0.f, 0.f, 0.f};
  if (FUSED && x.lbl && l16 < J) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = min(r0 + 4 * kb + r, R - 1);
      lblv[r] = x.lbl[(size_t)row * J + l16];
      vmv[r] = x.valid[(size_t)(row / x.P) * J + l16] ? 1.0f : 0.0f;
    }
  }
  if constexpr (W2T) {
    // nothing to stage
  } else if (J == 16) {   // W2 rows are 64 B: task = (k pair, column quad), both float4 loads issued before the first use
    constexpr int NT = Cp * 2 / 256;             // Cp/2 pairs x 4 quads over 256 threads
    float4 w0[NT], w1[NT];
#pragma unroll
    // (the four lanes of a quad write rows n = 0, 4, 8, 12 of one k pair: 4 rows x 1568 B is a multiple of the 128-byte
    //  bank row, a 4-way conflict on 24 ds_write_b32 per thread -- SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.29.  With
    //  kp fastest instead the ratio is 0.00 and the kernel SLOWER, 8.5 -> 9.2 us, cfg 003 step +1 us: every lane then
    //  reads 16 bytes of a different 64-byte row of W2.  Measured in round 4, the coalesced form kept.)
    for (int u = 0; u < NT; ++u) {
      const int t = tid + u * 256, kp = t >> 2, nq = t & 3;
      w0[u] = *reinterpret_cast<const float4*>(W2 + (size_t)(2 * kp) * 16 + nq * 4);
      w1[u] = *reinterpret_cast<const float4*>(W2 + (size_t)(2 * kp + 1) * 16 + nq * 4);
    }
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const int t = tid + u * 256, kp = t >> 2, n = (t & 3) * 4;
      uint32_t* d = reinterpret_cast<uint32_t*>(w2s + n * LDW + 2 * kp);
      d[0] = pack_bf16x2(w0[u].x, w1[u].x);
      d[LDW / 2] = pack_bf16x2(w0[u].y, w1[u].y);
      d[LDW] = pack_bf16x2(w0[u].z, w1[u].z);
      d[3 * (LDW / 2)] = pack_bf16x2(w0[u].w, w1[u].w);
    }
  } else {
    for (int i = tid; i < 16 * Cp; i += 256) {
      const int k = i >> 4, n = i & 15;          // W2 is [Cp][J]: consecutive threads read consecutive n
      const float v = n < J ? W2[(size_t)k * J + n] : 0.f;
      w2s[n * LDW + k] = (short)f32_to_bf16_bits(v);
    }
  }
  if (FUSED && x.wa)
    for (int i = tid; i < Cp / 4; i += 64 * WPB)
      *reinterpret_cast<float4*>(was + i * 4) = *reinterpret_cast<const float4*>(x.wa + i * 4);
  __syncthreads();       // (W2T: the compiler waits for the DMA -- vmcnt(0) -- in front of this barrier)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const bf16x8 bf = *reinterpret_cast<const bf16x8*>(w2s + l16 * LDW + ks * 32 + kb * 8);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], bf, acc, 0, 0, 0);
  }
  if (FUSED && x.wa) {   // Z of row r0 + l16: this lane's k quarter, then the four quarters across lanes
    float d = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4 wlo = *reinterpret_cast<const float4*>(was + ks * 32 + kb * 8);
      const float4 whi = *reinterpret_cast<const float4*>(was + ks * 32 + kb * 8 + 4);
      float xv[8];
      Vec<bf16_t>::unpack(__builtin_bit_cast(uint4, af[ks]), xv);
      d = fmaf(xv[0], wlo.x, d); d = fmaf(xv[1], wlo.y, d); d = fmaf(xv[2], wlo.z, d); d = fmaf(xv[3], wlo.w, d);
      d = fmaf(xv[4], whi.x, d); d = fmaf(xv[5], whi.y, d); d = fmaf(xv[6], whi.z, d); d = fmaf(xv[7], whi.w, d);
    }
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    float z = d + x.ba[0];
    if (x.act == 1) z = fmaxf(z, 0.f);           // 1 = relu attention; a softmax map stays raw here
    if (kb == 0 && r0 + l16 < R) x.att[r0 + l16] = z;
  }
  float lacc = 0.f;
  if (l16 < J) {
    const float bias = b2[l16];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * kb + r;
      if (row < R) {
        const float pl = acc[r] + bias;
        Pl[(size_t)row * J + l16] = pl;
        if (FUSED && x.lbl) {
          const float dd = pl - lblv[r];
          const float vm = vmv[r];
          lacc = fmaf(vm * dd, dd, lacc);
          x.dPl[(size_t)row * J + l16] = x.gcoef * vm * dd;
        }
      }
    }
  }
  if (FUSED && x.lbl) {
    lacc = wave_sum(lacc);
    if (lane == 0) lred[wave] = lacc;
    __syncthreads();
    if (tid == 0) x.lpart[blockIdx.x] = WPB == 4 ? (lred[0] + lred[1]) + (lred[2] + lred[3]) : lred[0] + lred[1];
  }
}

static bool pose_pl_fast(int Cp, int J, int dtype, const void* Ppre) {
  return dtype == APA_DTYPE_BF16 && J <= 16 && (Cp == 256 || Cp == 512 || Cp == 768 || Cp == 1024) &&
         (reinterpret_cast<uintptr_t>(Ppre) & 15) == 0;
}

// the skinny product's launch; `x` != nullptr: the fused form (attention logits column and / or pose L2 loss)
static int pose_pl_launch(const PoseCall& c, const PoseFwd& f, const PosePlExtra* x) {
  const bf16_t* pp = static_cast<const bf16_t*>(f.Ppre);
  const float *W2 = f.W2, *b2 = f.b2;
  float* Pl = f.Pl;
  const int R = (int)c.pl.R, J = c.J;
  hipStream_t st = c.st;
  const bool w2t = x && x->w2t;
  const dim3 grid(w2t ? (R + 31) / 32 : (R + 63) / 64);
  int ks = c.Cp / 32;                                  // k steps of 32: the kernel's instance
  if (ks != 8 && ks != 16 && ks != 24) ks = 32;        // (pose_pl_fast: Cp = 256 / 512 / 768 / 1024)
  if (PoseTrace* t = pose_trace()) {
    t->pl = POSE_PL_FAST; t->pl_fused = x ? 1 : 0; t->pl_w2t = w2t ? 1 : 0; t->pl_ks = ks;
  }
  const PosePlExtra none = {nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0.f, 1, nullptr};
#define APA_PL(KSv)                                                                                              \
  do {                                                                                                           \
    if (w2t)                                                                                                     \
      hipLaunchKernelGGL((pose_pl_kernel<KSv, true, true>), grid, dim3(128), 0, st, pp, W2, b2, Pl, R, J, *x);    \
    else if (x) hipLaunchKernelGGL((pose_pl_kernel<KSv, true>), grid, dim3(256), 0, st, pp, W2, b2, Pl, R, J, *x); \
    else hipLaunchKernelGGL((pose_pl_kernel<KSv, false>), grid, dim3(256), 0, st, pp, W2, b2, Pl, R, J, none);    \
  } while (0)
  switch (ks) {
    case 8: APA_PL(8); break;
    case 16: APA_PL(16); break;
    case 24: APA_PL(24); break;
    default: APA_PL(32); break;
  }
#undef APA_PL
  APA_LAUNCH_CHECK("pose_pl_kernel");
  return APA_OK;
}

static bool pose_dims_ok(int N, int P, int C, int Cp, int J) { return N > 0 && P > 0 && C > 0 && Cp > 0 && J > 0; }

static PosePlan pose_plan(int N, int P, int C, int Cp, int J, int dtype) {
  PosePlan pl;
  pl.R = (long)N * P;
  pl.nchunks = (int)((pl.R + POSE_RB - 1) / POSE_RB);
  size_t off = 0;
  pl.off_dppre = off;   off += align_up((size_t)pl.R * Cp * dt_size(dtype), 256);
  const size_t rows_part = (size_t)((pl.R + POSE_RPB_MIN - 1) / POSE_RPB_MIN) *
                           pose_rows_ld(Cp, J, pose_rows_nthr(Cp)) * 4;
  const size_t chunk_part = (size_t)pl.nchunks * (Cp + J) * 4;
  pl.off_partial = off; off += align_up(rows_part > chunk_part ? rows_part : chunk_part, 256);
  size_t g = gemm_ws_bytes((int)pl.R, J, 32);
  const size_t g2 = gemm_ws_bytes(Cp, J, 32), g3 = gemm_ws_bytes(C, Cp, 32);
  if (g2 > g) g = g2;
  if (g3 > g) g = g3;
  pl.off_gemm = off;    off += align_up(g, 256);
  // bf16 features: a bf16 copy of W1, so the MFMA GEMMs can DMA both operands straight into LDS
  pl.off_w1b = off;     off += align_up((size_t)C * Cp * 2, 256);
  // fused step: one pose-loss partial per block of the Pl kernel, alive from the forward to the last launch
  {                     // (its fallback runs apa_pose_l2_loss_fwd_bwd with the same region as scratch)
    size_t lp = (size_t)((pl.R + 31) / 32) * 4;         // (32-row blocks with the caller-kept W2^T image, else 64)
    const size_t l2 = apa_pose_l2_workspace_bytes(N, P, J);
    if (l2 > lp) lp = l2;
    pl.off_lpart = off; off += align_up(lp, 256);
  }
  pl.total = off;
  return pl;
}

thread_local PoseTrace* g_pose_trace = nullptr;
void pose_plan_offsets(int N, int P, int C, int Cp, int J, int dtype, size_t* out) {
  const PosePlan pl = pose_plan(N, P, C, Cp, J, dtype);
  out[0] = (size_t)pl.R; out[1] = (size_t)pl.nchunks; out[2] = pl.off_dppre; out[3] = pl.off_partial;
  out[4] = pl.off_gemm; out[5] = pl.off_w1b; out[6] = pl.off_lpart; out[7] = pl.total;
}

PoseCall pose_call(const char* fn, int N, int P, int C, int Cp, int J, int dtype, void* ws, size_t ws_bytes,
                   void* stream) {
  PoseCall c = {fn, "workspace", N, P, C, Cp, J, dtype, static_cast<hipStream_t>(stream), ws, ws_bytes, PosePlan{}};
  if (pose_dims_ok(N, P, C, Cp, J)) c.pl = pose_plan(N, P, C, Cp, J, dtype);
  return c;
}

// Every refusal of a pose-head call that an entry point can earn, in the order the entry points have always fired
// them.  operands: the entry point's own null-pointer list came out clean (it shares one text with the dimensions).
// b: a backward call, which adds its own -- and has never refused an unknown dtype, so it still does not.
static int pose_check(const PoseCall& c, bool operands, const PoseBwd* b = nullptr) {
  if (!operands || !pose_dims_ok(c.N, c.P, c.C, c.Cp, c.J)) {
    set_error("%s: null pointer or non-positive dimension", c.fn);
    return APA_ERR_INVALID_ARG;
  }
  if (!b && c.dtype != APA_DTYPE_F32 && c.dtype != APA_DTYPE_BF16) {
    set_error("%s: unknown dtype %d", c.fn, c.dtype);
    return APA_ERR_INVALID_ARG;
  }
  if (b && !b->dPl && !b->dPpre_ext && !b->ext_row) {
    set_error("%s: neither dPl nor dPpre_ext given (no gradient to propagate)", c.fn);
    return APA_ERR_INVALID_ARG;
  }
  if (b && (c.J > 32 || c.Cp > 2048)) {
    set_error("%s: J=%d > 32 or Cp=%d > 2048 not built", c.fn, c.J, c.Cp);
    return APA_ERR_UNSUPPORTED;
  }
  if (!c.ws || c.ws_bytes < c.pl.total) {
    set_error("%s: %s too small (%zu < %zu)", c.fn, c.ws_name, c.ws_bytes, c.pl.total);
    return APA_ERR_WORKSPACE;
  }
  if (b && c.Cp % 4 != 0) {
    set_error("%s: Cp=%d must be a multiple of 4", c.fn, c.Cp);
    return APA_ERR_UNSUPPORTED;
  }
  return APA_OK;
}

__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ in,
                                                          bf16_t* __restrict__ out, size_t n8) {
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n8; v += (size_t)gridDim.x * 256) {
    const float4 a = *reinterpret_cast<const float4*>(in + v * 8);
    const float4 b = *reinterpret_cast<const float4*>(in + v * 8 + 4);
    st16(out + v * 8, make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y),
                                 pack_bf16x2(b.z, b.w)));
  }
}

// W1 as the B operand of the Ppre product (slot = w1_fwd) and of the dX product (w1_bwd), decided here and nowhere
// else.  With bf16 features, so that the MFMA GEMMs can DMA both operands straight into LDS:
//   * the caller's bf16 shadow, if it gave one the products can read (16-byte addressable rows);
//   * else a bf16 copy in the workspace -- the one the forward call on the same workspace left there (reuse), or a fresh
//     conversion -- when W1's size and address allow whole 16-byte vectors;
//   * else, and with fp32 features, W1 itself.
struct PoseW1Op { const void* B; int tb; };
static PoseW1Op pose_w1_operand(const PoseCall& c, const float* W1, const void* shadow, bool reuse,
                                int PoseTrace::*slot) {
  PoseW1Op op = {W1, 0};
  int kind = POSE_W1_F32;
  if (shadow && c.dtype == APA_DTYPE_BF16 && (reinterpret_cast<uintptr_t>(shadow) & 15) == 0) {
    op = {shadow, 1};
    kind = POSE_W1_SHADOW;
  } else if (c.dtype == APA_DTYPE_BF16 && ((size_t)c.C * c.Cp) % 8 == 0 && (reinterpret_cast<uintptr_t>(W1) & 15) == 0) {
    bf16_t* w1b = reinterpret_cast<bf16_t*>(c.at(c.pl.off_w1b));
    op = {w1b, 1};
    kind = reuse ? POSE_W1_REUSED : POSE_W1_BF16_COPY;
    if (!reuse) {
      const size_t n8 = (size_t)c.C * c.Cp / 8;
      size_t nb = (n8 + 255) / 256;
      if (nb > 2048) nb = 2048;
      hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)nb), dim3(256), 0, c.st, W1, w1b, n8);
    }
  }
  if (PoseTrace* t = pose_trace()) t->*slot = kind;
  return op;
}

// Ppre = relu(X.W1 + b1), C = f.Ppre
static GemmDesc pose_ppre_product(const PoseCall& c, const PoseFwd& f, const PoseW1Op& w1) {
  GemmDesc g;
  g.A = f.X; g.lda = c.C; g.ta = dt_code(c.dtype); g.a_kc = true;
  g.B = w1.B; g.ldb = c.Cp; g.tb = w1.tb; g.b_kc = false;
  g.C = f.Ppre; g.ldc = c.Cp; g.tc = dt_code(c.dtype);
  g.M = (int)c.pl.R; g.N = c.Cp; g.K = c.C; g.bias = f.b1; g.act = 1;
  g.rmap = c.rmap;   // (a cached step: X is the cache, the M rows go through the index)
  return g;
}

// Pl = Ppre.W2 + b2: the skinny product, one wave per 16 rows (x: what its fused form adds, or null), where it serves
// the shape; else a split-K GEMM, which takes no extras
static int pose_pl_product(const PoseCall& c, const PoseFwd& f, const PosePlExtra* x) {
  if (pose_pl_fast(c.Cp, c.J, c.dtype, f.Ppre)) return pose_pl_launch(c, f, x);
  if (PoseTrace* t = pose_trace()) t->pl = POSE_PL_GEMM;
  const int R = (int)c.pl.R;
  GemmDesc g;
  g.A = f.Ppre; g.lda = c.Cp; g.ta = dt_code(c.dtype); g.a_kc = true;
  g.B = f.W2; g.ldb = c.J; g.tb = 0; g.b_kc = false;
  g.C = f.Pl; g.ldc = c.J; g.tc = 0;
  g.M = R; g.N = c.J; g.K = c.Cp; g.bias = f.b2;
  g.splits = gemm_pick_splits(R, c.J, c.Cp); g.ws = reinterpret_cast<float*>(c.at(c.pl.off_gemm));
  return gemm_launch(g, c.st);
}

}  // namespace apa

using namespace apa;

extern "C" size_t apa_pose_head_workspace_bytes(int N, int P, int C, int Cp, int J, int dtype) {
  if (!pose_dims_ok(N, P, C, Cp, J)) return 0;
  return pose_plan(N, P, C, Cp, J, dtype).total;
}

int apa::pose_head_fwd_run(const PoseCall& c, const PoseFwd& f) {
  int rc = pose_check(c, f.X && f.W1 && f.b1 && f.W2 && f.b2 && f.Ppre && f.Pl);
  if (rc != APA_OK) return rc;
  rc = gemm_launch(pose_ppre_product(c, f, pose_w1_operand(c, f.W1, nullptr, false, &PoseTrace::w1_fwd)), c.st);
  if (rc != APA_OK) return rc;
  return pose_pl_product(c, f, nullptr);
}

extern "C" int apa_pose_head_fwd(const void* X, const float* W1, const float* b1, const float* W2,
                                 const float* b2, void* Ppre, float* Pl, void* ws, size_t ws_bytes,
                                 int N, int P, int C, int Cp, int J, int dtype, void* stream) {
  return pose_head_fwd_run(pose_call("apa_pose_head_fwd", N, P, C, Cp, J, dtype, ws, ws_bytes, stream),
                           PoseFwd{X, W1, b1, W2, b2, Ppre, Pl});
}

// split-K factor of dW1 = X^T . dPpre.  bf16 features take the 128 x 64 tile kernel, three blocks per CU: the
// split that fills those 768 slots (C = 2048, Cp = 768: 192 tiles x 4) beats the generic "256 tiles of 128 x 128"
// rule (x 3): product 33.2 -> 29.0 us, reduce 6.0 -> 6.5 us, cfg 003 step -3 us (three interleaved pairs)
static int pose_dw1_splits(int C, int Cp, int R, int dtype) {
  int s = gemm_pick_splits(C, Cp, R);
  if (dtype == APA_DTYPE_BF16 && s > 1) {
    const long t64 = (long)((C + 127) / 128) * ((Cp + 63) / 64);
    const long t128 = (long)((C + 127) / 128) * ((Cp + 127) / 128);
    int s2 = (int)((768 + t64 / 2) / t64);
    const int maxs = R / 256 > 0 ? R / 256 : 1;
    if (s2 > maxs) s2 = maxs;
    if (s2 > 32) s2 = 32;
    if (s2 >= 1 && t128 * s2 < 640) s = s2;   // (the 64-wide kernel is chosen below 640 big tiles)
  }
  return s;
}

// dW1[c,j] = sum_r X[r,c] dPpre[r,j]: the one description of the product, launched by pose_head_bwd_big and put to the
// row map's admission rule by pose_rowmap_check before anything is queued (dW1: the caller's, or a stand-in there)
static GemmDesc pose_dw1_product(const PoseCall& c, const void* X, float* dW1, ColsumJob* job) {
  const int tdt = dt_code(c.dtype);
  GemmDesc g;
  g.A = X; g.lda = c.C; g.ta = tdt; g.a_kc = false;
  g.B = c.at(c.pl.off_dppre); g.ldb = c.Cp; g.tb = tdt; g.b_kc = false;
  g.C = dW1; g.ldc = c.Cp; g.tc = 0;
  g.M = c.C; g.N = c.Cp; g.K = (int)c.pl.R;
  g.splits = pose_dw1_splits(c.C, c.Cp, (int)c.pl.R, c.dtype); g.ws = reinterpret_cast<float*>(c.at(c.pl.off_gemm));
  g.tail = job;
  g.rmap = c.rmap;   // (a cached step: the contraction rows go through the index)
  return g;
}

// The tail of every backward route, the two dense products: dW1 = X^T . dPpre and dX (+)= dPpre . W1^T (b.no_dx: the
// first alone -- the second's only output is dX, and the pooling share its epilogue may carry goes with it).
// job: a column sum nothing behind it reads (the MFMA rows pass's) -- it rides on the tail blocks of dW1's split-K
// reduce launch when there is one (round 6), else it is a launch of its own here; null: already launched.
// x: the fused step's extras (the W1 shadow, the pooling's dX share), or null
static int pose_head_bwd_big(const PoseCall& c, const PoseBwd& b, const PoseStepArgs* x, ColsumJob* job) {
  const int tdt = dt_code(c.dtype), R = (int)c.pl.R, C = c.C, Cp = c.Cp;
  const void* dPpre = c.at(c.pl.off_dppre);
  PoseTrace* tr = pose_trace();
  int rc;
  {  // dW1[c,j] = sum_r X[r,c] dPpre[r,j]
    GemmDesc g = pose_dw1_product(c, b.X, b.dW1, job);
    GemmTrace gt;
    if (tr) g.trace = &gt;
    rc = gemm_launch(g, c.st);
    if (rc != APA_OK) return rc;
    if (tr) {
      tr->dw1_splits = gt.splits;
      if (job) tr->colsum = job->done ? POSE_COLSUM_TAIL : POSE_COLSUM_OWN;
    }
    if (job && !job->done) {     // no split-K reduce launch to ride on: the column sum as a launch of its own
      rc = m1_colsum(job->a, c.st);
      if (rc != APA_OK) return rc;
      job->done = true;
    }
  }
  if (b.no_dx) {
    if (tr) tr->dx_beta = 0;
    return rc;
  }
  {  // dX (+)= dPpre . W1^T
    const PoseW1Op w1 = pose_w1_operand(c, b.W1, x ? x->W1_bf16 : nullptr, b.ws_from_fwd, &PoseTrace::w1_bwd);
    GemmDesc g;
    g.A = dPpre; g.lda = Cp; g.ta = tdt; g.a_kc = true;
    g.B = w1.B; g.ldb = Cp; g.tb = w1.tb; g.b_kc = true;   // W1 [C][Cp]: n = c rows, k contiguous
    g.C = b.dX; g.ldc = C; g.tc = tdt;
    g.M = R; g.N = C; g.K = Cp; g.beta = b.accumulate ? 1.f : 0.f;
    g.stream_out = true;      // dX is the step's output: nothing in this call reads it back
    if (x && x->pool_att) {   // nothing was written to dX: its pooling share is formed in this epilogue
      g.beta = 0.f;
      g.r1_row = x->pool_att; g.r1_col = x->pool_dz; g.r1_bits = x->pool_bits; g.r1_P = c.P;
      g.r1_invP = 1.0f / (float)c.P; g.r1_inv_keep = x->pool_inv_keep;
    }
    if (tr) tr->dx_beta = g.beta != 0.f ? 1 : 0;
    rc = gemm_launch(g, c.st);
  }
  return rc;
}

// [dW2 | db1 | db2 (| dWa | dba)] from the [nblk][ld] partial rows of either rows kernel: one fixed-order column sum
// for all of them; in the fused step (x) the same blocks finish the pose loss -- the block partials pose_fwd_fused's Pl
// launch left in the workspace, one per block of it -- and advance the dropout counter.
// c1: width of the dW2 section; perm_nthr > 0: that section is in pose_bwd_rows_kernel's permuted order.
static ColsumArgs pose_rows_colsum(const PoseCall& c, const PoseBwd& b, const PoseStepArgs* x, int nblk, int ld,
                                   int c1, int perm_nthr) {
  ColsumArgs a;
  a.pdwa = reinterpret_cast<const float*>(c.at(c.pl.off_partial)); a.nblk = nblk; a.ld = ld;
  a.dwa = b.dW2; a.perm_nthr = perm_nthr; a.perm_cp = c.Cp;
  a.dwa2 = b.db1; a.C1 = c1; a.dwa3 = b.db2; a.C2 = c1 + c.Cp;
  a.C = c1 + c.Cp + c.J;
  if (!x) return a;
  if (x->dWa) { a.dwa4 = x->dWa; a.C3 = a.C; a.dwa5 = x->dba; a.C4 = a.C + c.Cp; a.C += c.Cp + 1; }
  a.rng_bump = x->rng_bump;
  a.aux_src = reinterpret_cast<const float*>(c.at(c.pl.off_lpart));
  a.aux_n = (int)(x->W2T_bf16 ? (c.pl.R + 31) / 32 : (c.pl.R + 63) / 64);
  a.aux_scale = 0.5f * x->pose_wt / ((float)c.N * (float)c.N * (float)c.P);
  a.aux_dst = x->loss_pose;
  return a;
}

// The three arms of the backward pass.  Each writes dPpre to the workspace with its kernel, records what it ran and
// sees to the column sums (and to dW2, where its kernel does not form it); pose_head_bwd_big follows.

// Round 6: the one-pass rows kernel on the matrix pipe (bf16 features); partial rows in NATURAL
// [dW2 | db1 | db2 (| dWa | dba)] order.  Its column sum is handed on as `job`
static int pose_rows_mfma(const PoseCall& c, const PoseBwd& b, const PoseStepArgs* x, ColsumJob* job) {
  const PosePlan& pl = c.pl;
  const float *dPl = b.dPl, *W2 = b.W2, *ext_row = b.ext_row, *ext_col = b.ext_col;
  const void* Ppre = b.Ppre;
  void* dPpre = c.at(pl.off_dppre);
  float* partial = reinterpret_cast<float*>(c.at(pl.off_partial));
  const int Cp = c.Cp, J = c.J;
  hipStream_t st = c.st;
  // waves per block (a wave owns 64 channels) and 32-row groups per block.  Fewer partial rows mean less traffic
  // here and in the column sum behind (G), small blocks let a CU overlap one block's loads with another's MFMAs
  // and stores (wpb); measured at the benchmark shape (rows kernel + column sum, us): wpb 6 G 1 14.7 + 5.8,
  // 6/2 12.3 + 4.8, 4/2 11.8 + 4.9, 3/2 11.5 + 4.8, 3/4 15.1 + 4.8, 2/4 15.7 + 4.8 (the VALU form: 16.3 + 5.5)
  const int nw = Cp / 64;                           // waves a whole row takes
  const int wpb = nw % 3 == 0 ? 3 : (nw % 4 == 0 ? 4 : 2);
  const int ngrp = nw / wpb;
  const int G = pl.R >= 2048 ? 2 : 1;
  const int nblk = (int)((pl.R + 32L * G - 1) / (32L * G));
  const size_t lds = (size_t)32 * (wpb * 64 + 8) * 2 + 32 * 20 * 4 + 32 * 4;
  const size_t ldp = pose_rows_ld(Cp, J, pose_rows_nthr(Cp));
  const bool want_wa = x && x->dWa;
#define APA_ROWSM(R1v, WAv)                                                                                      \
  hipLaunchKernelGGL((pose_bwd_rows_mfma_kernel<R1v, WAv>), dim3(nblk, ngrp), dim3(64 * wpb), lds, st, dPl, W2, ext_row, \
                     ext_col, static_cast<const bf16_t*>(Ppre), static_cast<bf16_t*>(dPpre), partial, pl.R, Cp, ldp, G)
  if (PoseTrace* t = pose_trace()) {
    t->rows = POSE_ROWS_MFMA; t->wpb = wpb; t->ngrp = ngrp; t->G = G; t->wa = want_wa ? 1 : 0;
    t->form = ext_row ? POSE_FORM_RANK1 : POSE_FORM_PLAIN; t->dw2 = POSE_DW2_ROWS;
  }
  if (ext_row && want_wa) APA_ROWSM(true, true);
  else if (ext_row) APA_ROWSM(true, false);
  else APA_ROWSM(false, false);
#undef APA_ROWSM
  APA_LAUNCH_CHECK("pose_bwd_rows_mfma_kernel");
  job->a = pose_rows_colsum(c, b, x, nblk, (int)ldp, Cp * J, 0);
  return APA_OK;
}

// The same pass on the VALU: dPpre + partial rows [dW2 | db1 | db2], one fixed-order column sum for all three
static int pose_rows_valu(const PoseCall& c, const PoseBwd& b, const PoseStepArgs* x) {
  const PosePlan& pl = c.pl;
  const float *dPl = b.dPl, *W2 = b.W2, *ext_row = b.ext_row, *ext_col = b.ext_col;
  const void *Ppre = b.Ppre, *dPpre_ext = b.dPpre_ext;
  void* dPpre = c.at(pl.off_dppre);
  float* partial = reinterpret_cast<float*>(c.at(pl.off_partial));
  const int Cp = c.Cp, J = c.J;
  hipStream_t st = c.st;
  const int nthr2 = pose_rows_nthr(Cp);
  const bool ext = dPpre_ext != nullptr && !ext_row;
  const int rpb = pose_rows_per_block(pl.R, nthr2, c.dtype, ext);
  const int nblk = (int)((pl.R + rpb - 1) / rpb);
  const size_t lds = pose_rows_lds(rpb, nthr2, c.dtype, ext);
  const bool want_wa = x && x->dWa;
#define APA_ROWS2(T, R1v, EXTv, RPBv, WAv)                                                                      \
  hipLaunchKernelGGL((pose_bwd_rows_kernel<T, R1v, EXTv, RPBv, WAv>), dim3(nblk), dim3(nthr2), lds, st, dPl, W2, \
                     static_cast<const T*>(dPpre_ext), ext_row, ext_col, static_cast<const T*>(Ppre),       \
                     static_cast<T*>(dPpre), partial, pl.R, Cp, J)
#define APA_ROWS(T, R1v, EXTv, WAv)                                                   \
  do {                                                                               \
    if (rpb == 32) APA_ROWS2(T, R1v, EXTv, 32, WAv); else APA_ROWS2(T, R1v, EXTv, 16, WAv); \
  } while (0)
  if (PoseTrace* t = pose_trace()) {
    t->rows = POSE_ROWS_VALU; t->rpb = rpb; t->wa = want_wa ? 1 : 0; t->dw2 = POSE_DW2_ROWS;
    t->form = ext_row ? POSE_FORM_RANK1 : (dPpre_ext ? POSE_FORM_EXT : POSE_FORM_PLAIN);
    t->colsum = POSE_COLSUM_OWN;
  }
  if (c.dtype == APA_DTYPE_F32) {   // (no WA arm: pose_head_bwd_impl refuses the fused outputs with fp32 features)
    if (ext_row) APA_ROWS(float, true, false, false);
    else if (dPpre_ext) APA_ROWS(float, false, true, false);
    else APA_ROWS(float, false, false, false);
  } else {
    if (ext_row && want_wa) APA_ROWS(bf16_t, true, false, true);
    else if (ext_row) APA_ROWS(bf16_t, true, false, false);
    else if (dPpre_ext) APA_ROWS(bf16_t, false, true, false);
    else APA_ROWS(bf16_t, false, false, false);
  }
#undef APA_ROWS2
#undef APA_ROWS
  APA_LAUNCH_CHECK("pose_bwd_rows_kernel");
  const int ldp = (int)pose_rows_ld(Cp, J, nthr2), c1 = (int)pose_rows_dw2(Cp, J, nthr2);
  return m1_colsum(pose_rows_colsum(c, b, x, nblk, ldp, c1, J == 16 ? nthr2 : 0), st);
}

// Every other shape (J <= 32, Cp <= 2048): dPpre by chunks of 8 rows, db1 / db2 from its block partials, dW2 as a
// product of its own (all zero without a pose-loss gradient)
static int pose_rows_dppre(const PoseCall& c, const PoseBwd& b) {
  const PosePlan& pl = c.pl;
  const float *dPl = b.dPl, *W2 = b.W2, *ext_row = b.ext_row, *ext_col = b.ext_col;
  const void *Ppre = b.Ppre, *dPpre_ext = b.dPpre_ext;
  void* dPpre = c.at(pl.off_dppre);
  float* partial = reinterpret_cast<float*>(c.at(pl.off_partial));
  const int Cp = c.Cp, J = c.J, R = (int)pl.R;
  hipStream_t st = c.st;
  const int nthr = ((Cp / 4 + 63) / 64) * 64;   // one thread per 4 columns (<= 512: Cp <= 2048)
#define APA_DPPRE(T, JM)                                                                            \
  do {                                                                                              \
    if (ext_row)                                                                                    \
      hipLaunchKernelGGL((pose_dppre_kernel<T, JM, true>), dim3(pl.nchunks), dim3(nthr), 0, st, dPl,  \
                         W2, static_cast<const T*>(nullptr), ext_row, ext_col,                      \
                         static_cast<const T*>(Ppre), static_cast<T*>(dPpre), partial, pl.R, Cp, J); \
    else                                                                                            \
      hipLaunchKernelGGL((pose_dppre_kernel<T, JM, false>), dim3(pl.nchunks), dim3(nthr), 0, st, dPl, \
                         W2, static_cast<const T*>(dPpre_ext), ext_row, ext_col,                    \
                         static_cast<const T*>(Ppre), static_cast<T*>(dPpre), partial, pl.R, Cp, J); \
  } while (0)
  if (PoseTrace* t = pose_trace()) {
    t->rows = POSE_ROWS_DPPRE; t->jm = J <= 16 ? 16 : 32; t->colsum = POSE_COLSUM_OWN;
    t->form = ext_row ? POSE_FORM_RANK1 : (dPpre_ext ? POSE_FORM_EXT : POSE_FORM_PLAIN);
    t->dw2 = dPl ? POSE_DW2_GEMM : POSE_DW2_MEMSET;
  }
  if (c.dtype == APA_DTYPE_F32) {
    if (J <= 16) APA_DPPRE(float, 16); else APA_DPPRE(float, 32);
  } else {
    if (J <= 16) APA_DPPRE(bf16_t, 16); else APA_DPPRE(bf16_t, 32);
  }
#undef APA_DPPRE
  APA_LAUNCH_CHECK("pose_dppre_kernel");
  // db1 = column sums of dPpre, db2 = column sums of dPl (fixed-order reduce of the block partials)
  ColsumArgs cs;
  cs.pdwa = partial; cs.nblk = pl.nchunks; cs.C = Cp + J; cs.ld = Cp + J; cs.dwa = b.db1; cs.dwa2 = b.db2; cs.C1 = Cp;
  const int rc = m1_colsum(cs, st);
  if (rc != APA_OK) return rc;
  if (!dPl) {
    return zero_fill(b.dW2, (size_t)Cp * J * sizeof(float), st);
  }
  GemmDesc g;  // dW2[j,q] = sum_r Ppre[r,j] dPl[r,q]
  g.A = Ppre; g.lda = Cp; g.ta = dt_code(c.dtype); g.a_kc = false;
  g.B = dPl; g.ldb = J; g.tb = 0; g.b_kc = false;
  g.C = b.dW2; g.ldc = J; g.tc = 0;
  g.M = Cp; g.N = J; g.K = R;
  g.splits = gemm_pick_splits(Cp, J, R); g.ws = reinterpret_cast<float*>(c.at(pl.off_gemm));
  return gemm_launch(g, st);
}

// The backward pass: checks, route, arm, tail.  x: the fused step's extras, or null.  The three refusals under `x`
// can fire from internal callers only (apa_pose_attn_train_step takes this route when pose_step_fast_ok holds)
static int pose_head_bwd_impl(const PoseCall& c, const PoseBwd& b, const PoseStepArgs* x = nullptr) {
  int rc = pose_check(c, b.X && b.W1 && b.W2 && b.Ppre && (b.dX || b.no_dx) && b.dW1 && b.db1 && b.dW2 && b.db2, &b);
  if (rc != APA_OK) return rc;
  const PoseRows rows = pose_rows_route(c, b);
  if (x && rows == POSE_ROWS_DPPRE) {
    set_error("%s: the fused step needs the one-pass rows kernel (J <= 16, Cp <= 1024; internal)", c.fn);
    return APA_ERR_UNSUPPORTED;
  }
  if (x && x->dWa && !b.ext_row) {
    set_error("%s: the fused dWa / dba outputs need the rank-1 external gradient (internal)", c.fn);
    return APA_ERR_INVALID_ARG;
  }
  if (x && x->dWa && c.dtype == APA_DTYPE_F32) {
    set_error("%s: the fused dWa / dba outputs are built for bf16 features (internal)", c.fn);
    return APA_ERR_UNSUPPORTED;
  }
  ColsumJob job;
  switch (rows) {
    case POSE_ROWS_MFMA: rc = pose_rows_mfma(c, b, x, &job); break;
    case POSE_ROWS_VALU: rc = pose_rows_valu(c, b, x); break;
    default: rc = pose_rows_dppre(c, b); break;
  }
  if (rc != APA_OK) return rc;
  return pose_head_bwd_big(c, b, x, rows == POSE_ROWS_MFMA ? &job : nullptr);
}

// ---------------------------------------------------------------------------------------------
// The pose-head halves of the one-call cfg 003 steps (apa_capi.hip)
// ---------------------------------------------------------------------------------------------
namespace apa {

void* pose_ws_loss_scratch(const PoseCall& c) { return c.at(c.pl.off_lpart); }

// The fused halves below serve a step whose forward half can take the skinny Pl product with both extras and whose
// backward half (dPl and the rank-1 gradient dZ (x) wa given) takes a one-pass rows kernel with the WA outputs
bool pose_step_fast_ok(const PoseCall& c, const PoseFwd& f, const PoseBwd& b) {
  return c.dtype == APA_DTYPE_BF16 && c.J == 16 && pose_pl_fast(c.Cp, c.J, c.dtype, f.Ppre) &&
         (reinterpret_cast<uintptr_t>(b.ext_col) & 15) == 0 && pose_rows_route(c, b) != POSE_ROWS_DPPRE &&
         pose_dims_ok(c.N, c.P, c.C, c.Cp, c.J);
}

// Ppre = relu(X.W1 + b1); then ONE launch for Pl = Ppre.W2 + b2, the attention logits Z = Ppre.wa + ba and the
// pose L2 loss (dPl + block partials kept in the workspace until pose_bwd_fused's last launch sums them).
// pose_step_fast_ok held: the skinny product serves the shape
int pose_fwd_fused(const PoseCall& c, const PoseFwd& f, const PoseStepArgs& a) {
  int rc = pose_check(c, true);
  if (rc != APA_OK) return rc;
  rc = gemm_launch(pose_ppre_product(c, f, pose_w1_operand(c, f.W1, a.W1_bf16, false, &PoseTrace::w1_fwd)), c.st);
  if (rc != APA_OK) return rc;
  const float denom = (float)c.N * (float)c.N * (float)c.P;          // loss.py:54-62 (apa_pose_l2_loss_fwd_bwd)
  PosePlExtra x;
  x.wa = a.wa; x.ba = a.ba; x.att = a.att; x.act = a.relu_att ? 1 : 0;
  x.lbl = a.pose_labels; x.valid = a.pose_valid; x.dPl = a.dPl;
  x.lpart = reinterpret_cast<float*>(c.at(c.pl.off_lpart));
  x.gcoef = a.grad_scale * a.pose_wt / denom; x.P = c.P;
  x.w2t = static_cast<const bf16_t*>(a.W2T_bf16);
  return pose_pl_launch(c, f, &x);
}

// att[r] = act(sum_t zp[t][r] + ba): the N / 128 column-tile partials of the contracted epilogue (GemmDesc::zp_*), summed
// in tile order; id / relu applied, a softmax map stays raw (the pooling call's row softmax takes it from here)
__global__ __launch_bounds__(256) void pose_zpart_finish_kernel(const float* __restrict__ zp, int nt, long R,
                                                                const float* __restrict__ ba, int act,
                                                                float* __restrict__ att) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float z = zp[r];
  for (int t = 1; t < nt; ++t) z += zp[(size_t)t * R + r];
  z += ba[0];
  if (act == 1) z = fmaxf(z, 0.f);
  att[r] = z;
}

size_t pose_eval_zpart_bytes(int N, int P, int Cp) {
  return align_up((size_t)((Cp + 127) / 128) * (size_t)N * P * 4, 256);
}

// The pose-head half of apa_pose_attn_eval_step; a: the W1 shadow and the attention conv (wa, ba, att, relu_att).
// Fused route (out->route = 1; no Pl asked for, bf16 operands, the product served by the contracted epilogue):
// Ppre = relu(X.W1 + b1) is formed tile by tile, contracted with wa and never stored; att receives Z = Ppre.wa + ba
// (id / relu).  Composed route (route = 0): Ppre goes to the workspace's dPpre region (out->ppre), Pl -- when asked
// for -- comes from pose_pl_product, whose skinny FUSED form emits att on the same pass where it serves the shape.
// out->att_ready: att holds Z; else the pooling call's own GEMV forms it from out->ppre.
int pose_eval_fwd(const PoseCall& c, const PoseFwd& f, const PoseStepArgs& a, float* zpart, PoseEvalOut* out) {
  int rc = pose_check(c, true);
  if (rc != APA_OK) return rc;
  const int R = (int)c.pl.R;
  PoseFwd fw = f;
  fw.Ppre = nullptr;
  GemmDesc g1 = pose_ppre_product(c, fw, pose_w1_operand(c, f.W1, a.W1_bf16, false, &PoseTrace::w1_fwd));
  if (!f.Pl && zpart) {
    g1.zp_w = a.wa; g1.zp_out = zpart;
    if (gemm_bf16_zp_serves(g1)) {
      if ((rc = gemm_launch(g1, c.st)) != APA_OK) return rc;
      hipLaunchKernelGGL(pose_zpart_finish_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, c.st, zpart,
                         c.Cp / 128, (long)R, a.ba, a.relu_att ? 1 : 0, a.att);
      APA_LAUNCH_CHECK("pose_zpart_finish_kernel");
      *out = {1, nullptr, true};
      return APA_OK;
    }
    g1.zp_w = nullptr; g1.zp_out = nullptr;
  }
  fw.Ppre = c.at(c.pl.off_dppre);
  g1.C = fw.Ppre;
  if ((rc = gemm_launch(g1, c.st)) != APA_OK) return rc;
  *out = {0, fw.Ppre, false};
  if (!f.Pl) return APA_OK;
  // with the skinny product and a 16-byte addressable wa the same pass emits att
  const bool fz = pose_pl_fast(c.Cp, c.J, c.dtype, fw.Ppre) && (reinterpret_cast<uintptr_t>(a.wa) & 15) == 0;
  const PosePlExtra x = {a.wa, a.ba, a.att, a.relu_att ? 1 : 0, nullptr, nullptr, nullptr, nullptr, 0.f, c.P, nullptr};
  out->att_ready = fz;
  return pose_pl_product(c, fw, fz ? &x : nullptr);
}

// dPpre (+ the rank-1 attention-branch gradient dZ (x) wa), dW2, db1, db2, dWa, dba in one pass + one column
// sum that also finishes the pose loss and advances the dropout counter; then dW1 and dX (+)= dPpre.W1^T
int pose_bwd_fused(const PoseCall& c, const PoseBwd& b, const PoseStepArgs& a) { return pose_head_bwd_impl(c, b, &a); }
int pose_head_bwd_run(const PoseCall& c, const PoseBwd& b) { return pose_head_bwd_impl(c, b); }

// The two products of a cached step that read X, as the routes above will describe them, put to gemm_rowmap_check:
// nothing is launched (pose_w1_operand's decision is repeated without its conversion launch).  The operands that live
// in the workspace are 256-byte aligned by the carve
int pose_rowmap_check(const PoseCall& c, const void* X, const float* W1, const void* w1_shadow, bool backward) {
  if (!c.rmap.index) return APA_OK;
  const bool shadow = w1_shadow && c.dtype == APA_DTYPE_BF16 && (reinterpret_cast<uintptr_t>(w1_shadow) & 15) == 0;
  const bool copy = c.dtype == APA_DTYPE_BF16 && ((size_t)c.C * c.Cp) % 8 == 0 && (reinterpret_cast<uintptr_t>(W1) & 15) == 0;
  const PoseFwd f = {X, W1, nullptr, nullptr, nullptr, c.at(c.pl.off_dppre), nullptr};
  GemmDesc g1 = pose_ppre_product(c, f, PoseW1Op{shadow ? w1_shadow : copy ? c.at(c.pl.off_w1b) : static_cast<const void*>(W1),
                                                 shadow || copy ? 1 : 0});
  int rc = gemm_rowmap_check(g1, c.fn);
  if (rc != APA_OK || !backward) return rc;
  // dW1 = X^T . dPpre as pose_head_bwd_big launches it (the workspace stands in for the caller's dW1; no tail job)
  return gemm_rowmap_check(pose_dw1_product(c, X, reinterpret_cast<float*>(c.at(c.pl.off_gemm)), nullptr), c.fn);
}

}  // namespace apa

// (the three bits of the public accumulate_dX are taken apart here and nowhere else)
extern "C" int apa_pose_head_bwd(const void* X, const float* W1, const float* W2, const void* Ppre,
                                 const float* dPl, const void* dPpre_ext, void* dX, int accumulate_dX,
                                 float* dW1, float* db1, float* dW2, float* db2, void* ws,
                                 size_t ws_bytes, int N, int P, int C, int Cp, int J, int dtype,
                                 void* stream) {
  return pose_head_bwd_impl(pose_call("apa_pose_head_bwd", N, P, C, Cp, J, dtype, ws, ws_bytes, stream),
                            PoseBwd{X, W1, W2, Ppre, dPl, dPpre_ext, nullptr, nullptr, dX, dW1, db1, dW2, db2,
                                    (accumulate_dX & 1) != 0, (accumulate_dX & APA_POSE_WS_FROM_FWD) != 0,
                                    (accumulate_dX & APA_POSE_NO_DX) != 0});
}

// (everything behind its own check reports as apa_pose_head_bwd, whose second form it is)
extern "C" int apa_pose_head_bwd_rank1ext(const void* X, const float* W1, const float* W2,
                                          const void* Ppre, const float* dPl, const float* ext_row,
                                          const float* ext_col, void* dX, int accumulate_dX, float* dW1,
                                          float* db1, float* dW2, float* db2, void* ws, size_t ws_bytes,
                                          int N, int P, int C, int Cp, int J, int dtype, void* stream) {
  if (!ext_row || !ext_col) {
    set_error("apa_pose_head_bwd_rank1ext: null ext_row / ext_col");
    return APA_ERR_INVALID_ARG;
  }
  return pose_head_bwd_impl(pose_call("apa_pose_head_bwd", N, P, C, Cp, J, dtype, ws, ws_bytes, stream),
                            PoseBwd{X, W1, W2, Ppre, dPl, nullptr, ext_row, ext_col, dX, dW1, db1, dW2, db2,
                                    (accumulate_dX & 1) != 0, (accumulate_dX & APA_POSE_WS_FROM_FWD) != 0,
                                    (accumulate_dX & APA_POSE_NO_DX) != 0});
}
