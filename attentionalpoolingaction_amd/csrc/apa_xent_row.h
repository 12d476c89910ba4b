// apa_xent_row.h -- the softmax cross-entropy of ONE logits row and the batch mean of the rows' losses, written once
// for every kernel that computes them.  apa_softmax_xent_fwd_bwd (apa_loss.hip) and every step that folds the loss
// into another kernel (the M == 1 logits reduction, the per-class activation passes, the clip loss, the evaluation
// scores) promise each other's BITS; they keep that promise by calling the routines below, not by repeating them.
//
//   row, 4 <= K <= 1024   xent_row_regs<NV4>   half a wave per row, the row in registers
//                         xent_row_3pass       the same operation order, the row re-read in each pass
//   row, any other K      xent_row_stream      one wave per row, three passes, expf
//   loss[0]               xent_mean_slots32(N, K) picks the order: xent_mean32_* (32 slots) or xent_mean256_load +
//                         block_sum256 (256 strided threads)
// Part of apa_device.h, which includes it behind the cross-lane helpers it builds on (wave_* / half_*, exp_fast) and in
// front of colsum_block, a caller: include apa_device.h.
#pragma once

namespace apa {

constexpr int XENT_ROW_MIN_K = 4, XENT_ROW_MAX_K = 1024;   // the half-wave forms; any other K: the stream form
__host__ __device__ inline bool xent_row_half_wave(int K) { return K >= XENT_ROW_MIN_K && K <= XENT_ROW_MAX_K; }
// 16-byte vectors per lane of the half wave: ceil(ceil(K / 4) / 32), rounded up to the instantiated 1 / 2 / 4 / 8
__host__ __device__ inline int xent_row_nv4(int K) { return K <= 128 ? 1 : (K <= 256 ? 2 : (K <= 512 ? 4 : 8)); }

// the gradient of the half-wave forms: gscale * (p - [this is the label's column]), one fma
__device__ __forceinline__ float xent_grad(float p, float gscale, bool hot) {
  return fmaf(p, gscale, hot ? -gscale : 0.f);
}

// The ragged-lane store of the half-wave forms: lane hl's vector belongs at columns col0 .. col0 + 3 and was taken at
// colc = min(col0, K - 4).  A whole vector is one unaligned 16-byte store; the one ragged lane of the row stores its
// own columns only; lanes past the row store nothing.  want_p: p goes to prow; want_g: g goes to grow (the row's K
// floats of each output).
__device__ __forceinline__ void xent_store_vec(bool want_p, float* __restrict__ prow, bool want_g,
                                               float* __restrict__ grow, int colc, int col0, int K, const f4u& p,
                                               const f4u& g) {
  if (colc == col0) {
    if (want_p) *reinterpret_cast<f4u*>(prow + colc) = p;
    if (want_g) *reinterpret_cast<f4u*>(grow + colc) = g;
  } else if (col0 < K) {
    for (int e = col0 - colc; e < 4; ++e) {
      if (want_p) prow[colc + e] = p[e];
      if (want_g) grow[colc + e] = g[e];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Register form.  These rows are pure latency chains, and two things dominate them (in-kernel timestamps,
// tools/kbench.cpp): global round trips and COLD INSTRUCTION FETCH -- a small kernel starts with an empty instruction
// cache and straight-line code streams in at well under 2 bytes per cycle, so code size is time.  Hence:
//   * HALF a wave (32 lanes) owns a row, so one copy of the code reduces two rows at once (lanes 0-31 and 32-63
//     reduce independently; a caller with one row runs it on both halves);
//   * a row is NV4 (<= 8) 16-byte vectors per lane, not predicated dwords: rows of K = 393 floats are only 4-byte
//     aligned, gfx950 services unaligned dwordx4 accesses; the ragged last vector is shifted back to end at K - 1
//     and its already-covered columns are masked out;
//   * every load is issued before anything is consumed, every store after the last reduction.
// loadv(colc): the four values at columns colc .. colc + 3 (global f4u load, or LDS reads); loadx(c): the value at
// column c (the label's logit: one broadcast load).  store (per lane): emit(colc, col0, p, g) once per vector, p =
// the probabilities, g = the gradient -- the caller stores what it wants of them (xent_store_vec, or element by
// element); what it ignores is never computed.  Returns the row's loss (0 for a label outside [0, K)); cand (may be
// nullptr): the first maximal index.  Both are uniform over the half wave.
// ---------------------------------------------------------------------------------------------------------------
template <int NV4, typename LoadV, typename LoadX, typename Emit>
__device__ __forceinline__ float xent_row_regs(LoadV&& loadv, LoadX&& loadx, int K, int lab, float gscale, int lane,
                                               bool store, Emit&& emit, int* cand) {
  const int hl = lane & 31;
  f4u v[NV4];
  int colc[NV4];
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    colc[i] = min(4 * (hl + 32 * i), K - 4);
    v[i] = loadv(colc[i]);
  }
  const bool lab_ok = lab >= 0 && lab < K;
  const float xl = loadx(lab_ok ? lab : 0);
  // columns already covered by the previous lane (ragged last vector) leave the reductions
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
    const int col0 = 4 * (hl + 32 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[i][e] = colc[i] + e >= col0 ? v[i][e] : -INFINITY;
  }
  float m = -INFINITY;
  int arg = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (v[i][e] > m) { m = v[i][e]; arg = colc[i] + e; }   // first maximal index of this lane
  }
  const float mw = half_max(m, lane);
  // argmax: smallest index among the lanes holding the max (np / tf argmax tie rule: first)
  if (cand) *cand = half_min_first((m == mw) ? arg : 0x7fffffff, lane);
  float l = 0.f;
#pragma unroll
  for (int i = 0; i < NV4; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[i][e] = exp_fast(v[i][e] - mw);   // 0 for the excluded columns
      l += v[i][e];
    }
  }
  l = half_sum(l, lane);
  const float inv = 1.0f / l;
  const float lv = lab_ok ? -(xl - mw - logf(l)) : 0.f;
  if (store) {
#pragma unroll
    for (int i = 0; i < NV4; ++i) {
      f4u p, g;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[e] = v[i][e] * inv;
        g[e] = xent_grad(p[e], gscale, colc[i] + e == lab);
      }
      emit(colc[i], 4 * (hl + 32 * i), p, g);
    }
  }
  return lv;
}

// The row in LDS, 4 <= K <= 64 (NV4 = 1), called by ONE whole wave (both halves run the same row): the per-class
// activation passes.  write: G[n, :] and loss[1 + n] go to memory; grow (optional, LDS): the gradient row for the
// caller's own use.
struct PcXent { const int64_t* labels; float* loss; float* G; float gscale; };
__device__ __forceinline__ void pc_row_xent(const float* lrow, int n, int K, const PcXent& xe, bool write, float* grow) {
  const int lane = threadIdx.x & 63;
  const float lv = xent_row_regs<1>(
      [&](int colc) { return f4u{lrow[colc], lrow[colc + 1], lrow[colc + 2], lrow[colc + 3]}; },
      [&](int c) { return lrow[c]; }, K, (int)xe.labels[n], xe.gscale, lane, lane < 32,
      [&](int colc, int col0, const f4u&, const f4u& g) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = colc + e;
          if (c >= col0 && c < K) {
            if (write) xe.G[(size_t)n * K + c] = g[e];
            if (grow) grow[c] = g[e];
          }
        }
      },
      nullptr);
  if (lane == 0 && write) xe.loss[1 + n] = lv;
}

// ---------------------------------------------------------------------------------------------------------------
// Three-pass form, any 4 <= K <= 1024: the register form's arithmetic on one row that lies in memory or LDS, in
// three passes that re-read the row (cache hits) instead of holding 4 * NV4 values per lane: the callers are blocks
// whose occupancy 100+ registers would halve (pc_bwd_act_kernel, a 16-wave block, went 7.4 -> 14.4 us with the
// register form).  The operation order per lane -- vectors in increasing i, elements in increasing e, then the
// half-wave trees -- is the register form's, so the results are bit-identical.  ONE whole wave calls it, both halves
// run the same row.  store: lanes 0-31 call emit(c, p) for each column c of the row, p = its probability.  Returns
// the row's loss (0 for a label outside [0, K)), valid in every lane like *cand (may be nullptr).
// ---------------------------------------------------------------------------------------------------------------
template <typename Emit>
__device__ __forceinline__ float xent_row_3pass(const float* __restrict__ row, int K, int lab, bool store, Emit&& emit,
                                                int* cand) {
  const int nv4 = xent_row_nv4(K);
  const int lane = threadIdx.x & 63, hl = lane & 31;
  const bool lab_ok = lab >= 0 && lab < K;
  const float xl = row[lab_ok ? lab : 0];
  auto vec = [&](int i, int& colc) {       // this lane's i-th vector, columns the previous lane covers masked out
    const int col0 = 4 * (hl + 32 * i);
    colc = min(col0, K - 4);
    f4u v = *reinterpret_cast<const f4u*>(row + colc);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = colc + e >= col0 ? v[e] : -INFINITY;
    return v;
  };
  float m = -INFINITY;
  int arg = 0x7fffffff;
#pragma unroll 1
  for (int i = 0; i < nv4; ++i) {
    int colc;
    const f4u v = vec(i, colc);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (v[e] > m) { m = v[e]; arg = colc + e; }   // first maximal index of this lane
  }
  const float mw = half_max(m, lane);
  if (cand) *cand = half_min_first((m == mw) ? arg : 0x7fffffff, lane);
  float l = 0.f;
#pragma unroll 1
  for (int i = 0; i < nv4; ++i) {
    int colc;
    const f4u v = vec(i, colc);
#pragma unroll
    for (int e = 0; e < 4; ++e) l += exp_fast(v[e] - mw);
  }
  l = half_sum(l, lane);
  const float inv = 1.0f / l;
  if (store && lane < 32) {
#pragma unroll 1
    for (int i = 0; i < nv4; ++i) {
      int colc;
      const f4u v = vec(i, colc);
      const int col0 = 4 * (hl + 32 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = colc + e;
        if (c >= col0 && c < K) emit(c, exp_fast(v[e] - mw) * inv);
      }
    }
  }
  return lab_ok ? -(xl - mw - logf(l)) : 0.f;
}

// value + gradient: grow (LDS, >= K floats) receives the gradient row; write: G[n, :] and loss[1 + n] also go to memory
__device__ __forceinline__ void pc_row_xent_any(const float* __restrict__ row, int n, int K, const PcXent& xe, bool write,
                                                float* grow) {
  const int lab = (int)xe.labels[n];
  const float lv = xent_row_3pass(row, K, lab, true, [&](int c, float p) {
    const float gv = xent_grad(p, xe.gscale, c == lab);
    if (write) xe.G[(size_t)n * K + c] = gv;
    grow[c] = gv;
  }, nullptr);
  if ((threadIdx.x & 63) == 0 && write) xe.loss[1 + n] = lv;
}

// forward only (apa_clipscores.hip): probabilities (probs: K floats of the row's output, or nullptr), first maximal
// index and row loss; lab < 0 (no ground truth): *lv = 0.  *lv and *cand are valid in every lane.
__device__ __forceinline__ void pc_row_softmax_any(const float* __restrict__ row, int K, int lab,
                                                   float* __restrict__ probs, float* lv, int* cand) {
  *lv = xent_row_3pass(row, K, lab, probs != nullptr, [&](int c, float p) { probs[c] = p; }, cand);
}

// ---------------------------------------------------------------------------------------------------------------
// Stream form (K < 4 or K > 1024): one wave per row, three passes, expf.  P(k): the row's k-th value -- a load, or the
// value formed again in each pass where the row is stored nowhere (clip_scores_kernel's loss block).  want_p: probs
// receives the row's K probabilities; want_g: G its gradient, G[k] = gscale (p_k - [k == lab]).  Returns the row's
// loss (0 for a label outside [0, K)); it and *cand (may be nullptr: the first maximal index) are wave-uniform.
// Contraction: p is stored as a probability by some callers and has the gradient as its only use in others, where the
// compiler would contract p - onehot into an fma on the UNROUNDED product.  apa_softmax_xent_fwd_bwd subtracts from
// the rounded p, so that is the definition: contraction is off for the expression, for every caller.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float xent_stream_grad(float e, float inv, bool hot, float gscale, float* p) {
#pragma clang fp contract(off)
  *p = e * inv;
  return (*p - (hot ? 1.0f : 0.0f)) * gscale;
}

template <typename PF>
__device__ __forceinline__ float xent_row_stream(PF&& P, int K, int lab, bool want_p, float* __restrict__ probs,
                                                 bool want_g, float* __restrict__ G, float gscale, int* cand) {
  const int lane = threadIdx.x & 63;
  float m = -INFINITY, xl = 0.f;
  int arg = 0x7fffffff;
  for (int k = lane; k < K; k += 64) {
    const float x = P(k);
    if (x > m) { m = x; arg = k; }
    if (k == lab) xl = x;
  }
  const float mw = wave_max(m);
  if (cand) *cand = wave_min_i((m == mw) ? arg : 0x7fffffff);
  xl = wave_sum(xl);
  float l = 0.f;
  for (int k = lane; k < K; k += 64) l += expf(P(k) - mw);
  l = wave_sum(l);
  const float inv = 1.0f / l;
  if (want_p || want_g) {
    // (not versioned: the compiler's second copy of the loop behind an alias check is 450 bytes of cold code)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int k = lane; k < K; k += 64) {
      float p;
      const float g = xent_stream_grad(expf(P(k) - mw), inv, k == lab, gscale, &p);
      if (want_p) probs[k] = p;
      if (want_g) G[k] = g;
    }
  }
  return (lab >= 0 && lab < K) ? -(xl - mw - logf(l)) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------
// loss[0] = lscale * sum_n loss[1 + n] has two summation orders, chosen by (N, K).  Their native definitions are
// softmax_xent_kernel's own slot sum (modes 1 / 2: its slots are its half waves) and sum_scale_kernel (apa_loss.hip);
// a kernel that folds the loss in reproduces the order for its (N, K) with the routines below.  Each comes as an early
// LOAD and a late FINISH, so that a caller with other work requests the rows first and reduces after that work.
// ---------------------------------------------------------------------------------------------------------------
// true: the 32-slot order; false: the 256-thread order.  (A caller whose K is in the half-wave range by construction
// passes any such K.)
__host__ __device__ inline bool xent_mean_slots32(int N, int K) { return xent_row_half_wave(K) && N <= 64; }

// 32-slot order, N <= 64, on ONE wave: slot s adds rows s and s + 32, the slots are added in increasing s.
// load: lane n < 64 holds row n's loss (0 beyond N).
__device__ __forceinline__ float xent_mean32_load(const float* __restrict__ rows, int N, int lane) {
  return lane < N ? rows[lane] : 0.f;
}
// slot: lane s < 32 holds slot s's sum, (0.f + row s) + row s + 32.  red: 32 floats of LDS nobody else touches
// meanwhile.  The sum is valid in lane 0.
__device__ __forceinline__ float xent_mean32_slots(float slot, float* red, int lane) {
  if (lane < 32) red[lane] = slot;
  __builtin_amdgcn_wave_barrier();
  float t = 0.f;
  if (lane == 0)
    for (int s = 0; s < 32; ++s) t += red[s];
  return t;
}
__device__ __forceinline__ float xent_mean32_finish(float row, float* red, int lane) {
  return xent_mean32_slots((0.f + row) + __shfl_xor(row, 32), red, lane);
}

// 256-thread order: thread t < 256 adds rows t, t + 256, ...; wave_sum; then (w0 + w1) + (w2 + w3) over the four waves.
__device__ __forceinline__ float xent_mean256_load(const float* __restrict__ rows, int N) {
  float acc = 0.f;
  if (threadIdx.x < 256)
    for (int i = threadIdx.x; i < N; i += 256) acc += rows[i];
  return acc;
}
// The finish, and the fixed-order sum of one value per thread of the first four waves in general.  Every thread of the
// block calls it (one block barrier inside); red: 4 floats of LDS, free again after the NEXT block barrier.  The sum is
// valid in every thread.
__device__ __forceinline__ float block_sum256(float acc, float* red) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace apa
