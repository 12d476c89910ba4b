// apa_m1_stream.hip -- the two HBM-bound streaming passes of the factorised (M == 1) head for
// wide feature maps (C >= 1024 fp32 / 2048 bf16), "pixel tile x channel split" shape.
//
// Reference semantics: models/slim/nets/nets_factory.py:247-328 (see include/apa.h and the
// closed forms at the top of apa_m1.hip).
//
// Work decomposition.  Block (n, s) owns a contiguous run of pixels of image n, processed in
// chunks of at most PIX (<= 16) pixels.  Inside a block the four waves split the CHANNELS, not
// the pixels: wave w owns channels [w*C/4, (w+1)*C/4) of every pixel of the chunk.
//   * all loads of a chunk (PIX x VW 16-byte vectors per lane, up to 32 KiB per wave) are issued
//     back to back before anything is consumed -> every CU has its whole share in flight at once;
//   * the four waves always do the same amount of work (no 4-vs-3 pixel imbalance);
//   * the C-long dot products (x.wa, x.dz) are finished with ONE block exchange per chunk:
//     16-lane DPP row sums -> 1 KiB of LDS -> one barrier -> every lane holds the total of pixel
//     (lane & 15), bit-identical in all four waves (fixed summation order);
//   * the channel accumulators (z partials, dwa partials) are private to a wave, so they go from
//     registers straight to the per-block partial row -- no cross-wave LDS reduction.
// X is read once per pass and dX written once, exactly like the per-pixel kernels in apa_m1_vec.hip
// (which stay as the path for narrow maps).
#include <math.h>

#include "apa_device.h"
#include "apa_internal.h"

// Cache policy, measured (bench.py, fp32): dX goes out with NON-TEMPORAL stores -- 307 -> 271 us at
// N = 512 (5.35 -> 6.07 TB/s), 66 -> 61 us at N = 128, neutral at N = 32.  Non-temporal LOADS of X in
// the backward pass lose everywhere (271 -> 293 us at N = 512, 16.0 -> 17.0 us at N = 32, where X is
// still resident in the 256 MiB Infinity Cache from the forward pass), so X uses plain loads.
#ifndef APA_BWD_NT_LOAD
#define APA_BWD_NT_LOAD false
#endif
// Direction of the backward walk (round 6).  Both passes give block b the same pixels of the same image
// (xcd_remap() puts it on the same XCD), and the forward pass walks them upwards: what it read LAST is what this
// XCD's L2 and the Infinity Cache still hold when the backward pass starts.  Walking DOWNWARDS meets those lines
// first, before the pass's own traffic has pushed them out; walking upwards again evicts them unread.  Measured
// on one box, physically contiguous X / dX, fp32 (up / down, us): N = 32: 18.55 / 17.65, N = 64: 32.6 / 32.2,
// N = 256: 164 / 144.5, N = 512: 320 / 298, 512 x 15x15: 384 / 354; bf16 N = 512: 149.5 / 146.5.
// (docs/DESIGN_HISTORY.md, round 6: how the "two kinds of box" of the N = 512 line turned out to be this.)

namespace apa {

namespace {
// Every wave passes its PIX per-lane partial dot products d[i] (pixel slot i, this wave's channel
// share).  Returns, in lane l of every wave, the block total of slot (l & 15).
//   sm: 256 floats, layout [wave][slot][row]; written conflict-free, read back as one float4.
template <int PIX>
__device__ __forceinline__ float block_dots(const float (&d)[PIX], float* sm, int wave, int lane) {
  const int l16 = lane & 15;
  float mine = 0.f;
#pragma unroll
  for (int i = 0; i < PIX; ++i) {
    const float r = row_sum16(d[i]);
    mine = (l16 == i) ? r : mine;
  }
  sm[wave * 64 + l16 * 4 + (lane >> 4)] = mine;
  __syncthreads();
  const float4 v = *reinterpret_cast<const float4*>(&sm[lane * 4]);
  float s = (v.x + v.y) + (v.z + v.w);  // wave (lane >> 4)'s total of slot l16
  s += __shfl_xor(s, 16);               // (w0 + w1) | (w2 + w3)
  s += __shfl_xor(s, 32);               // (w0 + w1) + (w2 + w3): same bits in every row
  return s;
}

// keep decisions of elements e, e+1 (e even) as bits 0 / 1.
__device__ __forceinline__ uint32_t rng_keep2_bits(uint64_t e, uint32_t k0, uint32_t k1,
                                                   uint32_t thresh) {
  const uint64_t q = e >> 1;
  const uint32_t h = rng_hash((uint32_t)q, k0, k1 ^ __umul24((uint32_t)(q >> 32), 0x9E3779u));
  return ((h & 0xffffu) < thresh ? 1u : 0u) | ((h >> 16) < thresh ? 2u : 0u);
}
}  // namespace

// APA_FLAG_RELU_INPUT: the map in memory is the backbone's PRE-activation; X = max(Xin, 0) is
// applied where a vector is unpacked (never on the packed registers: that would wait for the load)
template <bool RIN, int EPV>
__device__ __forceinline__ void relu_in(float (&x)[EPV]) {
  if (RIN) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) x[e] = fmaxf(x[e], 0.f);
  }
}

// --------------------------------------------------------------------------------------------
// Chunk helpers.  A chunk = np (<= PIX) consecutive pixels starting at q0; xr holds this wave's
// channel share of them.  Chunks are double-buffered: the loads of chunk k+1 are in flight while
// chunk k is consumed (and, in backward, while its dX rows are stored), so reads, VALU work and
// writes of different chunks overlap inside one wave.
// --------------------------------------------------------------------------------------------
// Where the prefetch REALLY lands (round 6).  X is a `const __restrict__` kernel argument: alias analysis calls
// that constant memory, and SelectionDAG does not chain loads of constant memory to anything -- not to the
// sched_barrier below, not to the s_barrier of block_dots.  Instruction selection then linearised every chunk's loads
// next to their first use, i.e. AFTER the barrier of the chunk in front of them (all three kernels of this file,
// rounds 1-5: `-mllvm -print-after=amdgpu-isel` shows SCHED_BARRIER, S_BARRIER, GLOBAL_LOAD x4 in that order): a
// chunk's loads flew only during the second half of its predecessor.  The evaluation instantiation of the forward
// pass, whose second half is a handful of FMAs, was 10 % SLOWER than the training one that also hashes a dropout
// mask (VERDICT r05 Weak #8).  `opaque_global` hides the pointer's provenance from alias analysis (an empty asm on
// the SGPR pair, address space kept so the loads stay global_load): the loads are ordinary chained loads again,
// stay in front of the sched_barrier, and the waits in front of a chunk's arithmetic become vmcnt(4 + ...) -- the
// next chunk's four loads are in flight over the WHOLE of this chunk.
#ifndef APA_M1S_OPAQUE_X
#define APA_M1S_OPAQUE_X 1
#endif
#ifndef APA_M1S_NB
#define APA_M1S_NB 2      // depth of the register ring of chunks (chunk in work + NB - 1 in flight)
#endif
template <typename T>
__device__ __forceinline__ const T* opaque_global(const T* p) {
#if APA_M1S_OPAQUE_X
  typedef const T __attribute__((address_space(1))) * gp;
  gp g = (gp)p;
  asm volatile("" : "+s"(g));
  return (const T*)g;
#else
  return p;
#endif
}

template <typename T, int VW, int PIX, bool NT = false>
__device__ __forceinline__ void load_chunk(uint4 (&xr)[PIX][VW], const T* xim, int q0,
                                           int p_last, int C, int cbase) {
  constexpr int EPV = Vec<T>::EPV;
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  typedef const u4 __attribute__((address_space(1))) * gvec_ptr;
#pragma unroll
  for (int i = 0; i < PIX; ++i) {
    const int p = min(q0 + i, p_last);   // slots past the block's last pixel re-read that pixel
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const T* src = xim + (size_t)p * C + cbase + j * 64 * EPV;
#if APA_M1S_OPAQUE_X
      const u4 v = NT ? __builtin_nontemporal_load((gvec_ptr)src) : *(gvec_ptr)src;
      xr[i][j] = make_uint4(v.x, v.y, v.z, v.w);
#else
      xr[i][j] = NT ? ld16_nt(src) : ld16(src);
#endif
    }
  }
  // keep the prefetch ahead of the current chunk's arithmetic and barrier
  __builtin_amdgcn_sched_barrier(0);
}

// Chunk ch of a block covers pixel slots q0 .. q0+PIX-1; only the first np are the block's own
// (np < PIX on the last chunk only).  Every slot is always processed -- straight-line code, so the
// compiler keeps exact s_waitcnt counts and the next chunk's loads stay in flight -- and the
// surplus slots repeat the block's last pixel: their weights are zero in every accumulation and
// their dX stores rewrite the identical bytes.
// --------------------------------------------------------------------------------------------
// The paired form (PAIR) of the FORWARD pass, fp32 features.  The plan puts two logical blocks on every CU; as two
// 256-thread blocks they cannot see each other, and each leaves a partial row of its own for the fold / finalize kernel
// to read.  PAIR runs the two logical blocks
// (n, 2s') and (n, 2s' + 1) of an even S as ONE 512-thread block: waves 0-3 ("quad 0") are the first, waves 4-7 the
// second.  Each quad is a logical block exactly as before -- its pixels, its walk, its chunk order, its own ring,
// its own exchange buffers, block_dots over its own four waves -- so att, the keep bits and pstat keep their
// bits; only at the end quad 1 hands its channel accumulators to quad 0 through LDS and ONE row, acc0 + acc1,
// leaves the CU (row n S/2 + s').  Same waves per CU, half the partial rows for the fold / finalize kernel to merge.
// Measured (profiles/paired_rows_summary.md): the forward pass paired alone is 1.1 - 1.2 us of the fp32 headline step
// and passes the project's rule; the backward pass paired alone does not (43.45 -> 43.22 us, rule 43.19) and adds
// 0.24 us on top of the forward pairing, inside the spread: it keeps its 256-thread form.  bf16 features: the forward
// pass is VALU-bound on the dropout hash and the keep bits, and a barrier shared by eight waves costs it about 1 us
// (N = 32, K = 51): unpaired.
// s_barrier counts the block's eight waves, so both quads have to execute the same number of barriers: a quad whose
// run has fewer chunks than its partner's executes the missing ones behind its loop and nothing else.
// Physical block b of nblk / 2 is pair xcd_remap(b, nblk / 2): with nblk a multiple of 16 (the benchmark batch) every
// logical block stays on the XCD it had.
// --------------------------------------------------------------------------------------------
struct PairId { int blk, quad, wave, tid; };   // logical block, quad (0 / 1), wave and thread within the quad
template <bool PAIR>
__device__ __forceinline__ PairId pair_id(int nblk) {
  PairId r;
  if (PAIR) {
    r.quad = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));   // wave-uniform: keep n, s and the ranges scalar
    r.blk = 2 * xcd_remap(blockIdx.x, nblk >> 1) + r.quad;
  } else {
    r.quad = 0;
    r.blk = xcd_remap(blockIdx.x, nblk);
  }
  r.tid = threadIdx.x & 255;
  r.wave = r.tid >> 6;
  return r;
}
// chunks of the partner quad's run (split s ^ 1 of the same image)
template <int PIX>
__device__ __forceinline__ int partner_chunks(int s, int P, int S) {
  int b, e;
  m1_pix_range(s ^ 1, P, S, b, e);
  return (e - b + PIX - 1) / PIX;
}
// quad 1's EPL accumulators join quad 0's: row[c] = acc0[c] + acc1[c], one add per element, in quad 0's registers.
// sm: C floats.  One barrier, executed by all eight waves.
template <int EPL, int EPV>
__device__ __forceinline__ void pair_merge(float (&acc)[EPL], float* sm, int quad, int cbase) {
#pragma unroll
  for (int j = 0; j < EPL / EPV; ++j) {
#pragma unroll
    for (int e = 0; e < EPV; e += 4) {
      const int i = j * EPV + e;
      if (quad == 1)
        *reinterpret_cast<float4*>(sm + cbase + j * 64 * EPV + e) = make_float4(acc[i], acc[i + 1], acc[i + 2], acc[i + 3]);
    }
  }
  __syncthreads();
  if (quad == 0) {
#pragma unroll
    for (int j = 0; j < EPL / EPV; ++j) {
#pragma unroll
      for (int e = 0; e < EPV; e += 4) {
        const int i = j * EPV + e;
        const float4 o = *reinterpret_cast<const float4*>(sm + cbase + j * 64 * EPV + e);
        acc[i] = acc[i] + o.x; acc[i + 1] = acc[i + 1] + o.y; acc[i + 2] = acc[i + 2] + o.z; acc[i + 3] = acc[i + 3] + o.w;
      }
    }
  }
}

struct ChunkRange { int q0, np; };
template <int PIX>
__device__ __forceinline__ ChunkRange chunk_range(int p_begin, int p_end, int ch) {
  ChunkRange r;
  r.q0 = p_begin + ch * PIX;
  r.np = min(PIX, p_end - r.q0);
  return r;
}

// --------------------------------------------------------------------------------------------
// Forward pooling pass.  Outputs are those of m1_pool_fwd_kernel (apa_m1_vec.hip):
//   att (FUSED: id/relu -> final A, softmax -> raw Z, normalised by the finalize kernel),
//   pacc[blk][C] = sum_p A*Xt over the block's pixels (softmax: relative to pstat m),
//   pstat[blk][4] = {m, l, asum, -}.
// --------------------------------------------------------------------------------------------
template <typename T, int VW, int PIX, bool FUSED, bool TRAIN>
struct FwdState {
  static constexpr int EPV = Vec<T>::EPV;
  static constexpr int EPL = VW * EPV;
  float wa[FUSED ? EPL : 1];
  float acc[EPL];
  float bias, m_run, l_run, a_sum;
};

// Keep-bits hand-off.  The forward pass has to hash every element anyway; it also leaves the decisions
// behind as bits -- byte (n*P + p) * C/8 + (cbase - j-part)/EPL.. : ONE byte (two for EPL = 16) per lane and
// pixel, bit j*EPV + e = channel cbase + j*64*EPV + e, i.e. exactly the lane's own channels -- and a backward
// call that is handed the same workspace (APA_FLAG_WS_FROM_FWD) reads them back instead of hashing again:
// the hash was 2.1 us of VALU work in the dominant kernel (profiles/r01_hot_pmc.md), the bits are 1/32
// of the fp32 map's bytes.  Layout per pixel: [C / EPL] lanes-worth of BPL bytes, lane-major.
// Measured (bench.py, N = 32 / 512): bf16 features, where a lane hashes 8 elements per 16-byte load and the
// backward pass is VALU-bound on it, gain 15.6 -> 13.2 us in the backward kernel for +0.1 us in the
// forward one; fp32 features (4 elements per load, memory-bound either way) gain nothing in backward and
// pay for the extra store instructions in forward (13.9 -> 14.1 us at N = 32, 150 -> 183 us at N = 512:
// memory-instruction issue, not bytes) -- so the hand-off is compiled in for bf16 only.
template <typename T> struct KeepBits { static constexpr bool ON = sizeof(T) == 2; };
template <int EPL> struct MaskBytes {
  static constexpr int BPL = (EPL + 7) / 8;   // bytes per lane and pixel
  static constexpr int BPP = 256 * BPL;       // bytes per pixel (4 waves x 64 lanes)
};

// SM: softmax attention.  A template argument of both passes: as a test of the run-time `act` all three arms stayed in
// the chunk loop (forward: seven conditional branches per chunk, the expf sequence and the accumulators copied around
// the rescale on the identity path; backward: four per chunk, whose merge made the loop's tail a block of its own).
// Identity against relu stays a select on `act`.
template <typename T, int VW, int PIX, bool FUSED, bool TRAIN, bool SM, bool RIN>
__device__ __forceinline__ void fwd_chunk(FwdState<T, VW, PIX, FUSED, TRAIN>& st,
                                          const uint4 (&xr)[PIX][VW], ChunkRange cr, float* sm,
                                          float* __restrict__ att_im, int n, int P, int C, int cbase,
                                          int wave, int lane, int act, float inv_keep,
                                          uint32_t thresh, uint32_t k0, uint32_t k1,
                                          uint8_t* __restrict__ bits_im, float av_pre) {
  constexpr int EPV = Vec<T>::EPV;
  constexpr int EPL = VW * EPV;
  const int l16 = lane & 15;
  const int q0 = cr.q0, np = cr.np;
  float av = 0.f;   // lane l16: weight of pixel slot l16
  if (FUSED) {
    float d[PIX];
#pragma unroll
    for (int i = 0; i < PIX; ++i) {
      float d0 = 0.f, d1 = 0.f;
#pragma unroll
      for (int j = 0; j < VW; ++j) {
        float x[EPV];
        Vec<T>::unpack(xr[i][j], x);
        relu_in<RIN>(x);
#pragma unroll
        for (int e = 0; e < EPV; e += 2) {
          d0 = fmaf(x[e], st.wa[j * EPV + e], d0);
          d1 = fmaf(x[e + 1], st.wa[j * EPV + e + 1], d1);
        }
      }
      d[i] = d0 + d1;
    }
    const float zt = block_dots<PIX>(d, sm, wave, lane) + st.bias;
    if constexpr (SM) {
      const float m_chunk = row_max16(l16 < np ? zt : -INFINITY);
      const float m_new = fmaxf(st.m_run, m_chunk);
      const float scale = expf(st.m_run - m_new);   // exp(-inf) = 0 on the first chunk
      av = l16 < np ? expf(zt - m_new) : 0.f;
      st.l_run = st.l_run * scale + row_sum16(av);
      st.m_run = m_new;
      if (wave == 0 && lane < np) att_im[q0 + lane] = zt;   // raw logit; normalised later
#pragma unroll
      for (int i = 0; i < EPL; ++i) st.acc[i] *= scale;
    } else {
      av = (act == M1_ACT_RELU) ? fmaxf(zt, 0.f) : zt;
      if (l16 >= np) av = 0.f;
      if (wave == 0 && lane < np) att_im[q0 + lane] = av;
    }
  } else {
    // the pre-computed map's values travel with the chunk's prefetch (round 6: loaded here, on the spot, this was the
    // YOUNGEST outstanding load -- its s_waitcnt vmcnt(0) also waited for the next chunk's features, every chunk)
    av = l16 < np ? av_pre : 0.f;
  }
#pragma unroll
  for (int i = 0; i < PIX; ++i) {
    const float a = readlane_f(av, i);   // 0 for surplus slots
    st.a_sum += a;
    const float ak = TRAIN ? a * inv_keep : a;
    // surplus slots repeat the block's last pixel (data, element index and therefore mask bits alike)
    const int pi = min(q0 + i, q0 + np - 1);
    const uint64_t ebase = ((uint64_t)n * P + pi) * C + cbase;
    uint32_t lbits = 0;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      float x[EPV];
      Vec<T>::unpack(xr[i][j], x);
      relu_in<RIN>(x);
      if (TRAIN) {
#pragma unroll
        for (int e = 0; e < EPV; e += 2) {
          const uint32_t b = rng_keep2_bits(ebase + j * 64 * EPV + e, k0, k1, thresh);
          lbits |= b << (j * EPV + e);
          st.acc[j * EPV + e] = fmaf((b & 1u) ? ak : 0.f, x[e], st.acc[j * EPV + e]);
          st.acc[j * EPV + e + 1] = fmaf((b & 2u) ? ak : 0.f, x[e + 1], st.acc[j * EPV + e + 1]);
        }
      } else {
#pragma unroll
        for (int e = 0; e < EPV; ++e) st.acc[j * EPV + e] = fmaf(ak, x[e], st.acc[j * EPV + e]);
      }
    }
    if (TRAIN && KeepBits<T>::ON) {
      // BPL bytes per lane; the bytes of 4 (BPL = 1) / 2 (BPL = 2) neighbouring lanes leave as one dword
      constexpr int BPL = MaskBytes<EPL>::BPL;
      uint8_t* dst = bits_im + (size_t)pi * MaskBytes<EPL>::BPP + (size_t)(wave * 64 + lane) * BPL;
      if (BPL == 1) {
        const uint32_t b1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)lbits, 0x39, 0xf, 0xf, true);   // lane + 1
        const uint32_t b2 = (uint32_t)__builtin_amdgcn_mov_dpp((int)lbits, 0x4E, 0xf, 0xf, true);   // lane + 2
        const uint32_t b3 = (uint32_t)__builtin_amdgcn_mov_dpp((int)lbits, 0x93, 0xf, 0xf, true);   // lane + 3
        const uint32_t w = (lbits & 0xffu) | ((b1 & 0xffu) << 8) | ((b2 & 0xffu) << 16) | (b3 << 24);
        if ((lane & 3) == 0) *reinterpret_cast<uint32_t*>(dst) = w;
      } else {
        const uint32_t b1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)lbits, 0xB1, 0xf, 0xf, true);   // lane ^ 1
        const uint32_t w = (lbits & 0xffffu) | (b1 << 16);
        if ((lane & 1) == 0) *reinterpret_cast<uint32_t*>(dst) = w;
      }
    }
  }
}

// Parameter order (both kernels of this file): the objects of this file are built with kernarg preload, which hands a
// wave the first 14 argument dwords in SGPRs at launch.  Everything the address of the first chunk's loads is made of
// -- X, P, S and the grid size (xcd_remap: gridDim.x is a hidden argument at the far end of the block) -- and the
// pointers of the loads that follow it lie in that window, so no scalar-memory wait stands in front of the first
// global_load; the rest is fetched with s_load under the first chunk.  The dropout key (a dependent read of the
// device counter) is formed behind the issue of the ring's first NB - 1 chunks: chunk 0's arithmetic is its first
// use, behind an HBM wait that is longer.
// GATHER: the gathered instances (apa_device.h: M1Gather; the plain ones take an empty M1NoGather).  The window is full,
// so the descriptor lies behind it: the index read is one scalar load in front of the first chunk's address, which the
// plain instances do not have.  FUSED or not (the cfg 003 cached steps: att / dZ keep the batch position, only xim
// moves), without RIN or SM and (backward) NODX only: the launchers below name every instance from m1_pool_form's tags.
// SM: the softmax instances (fwd_chunk); forward: of the fused forms only, a map that is already final is pooled as it is.
// PAIR: the 512-thread paired form above (fp32 only; never SM: the (m, l, acc) merge of two softmax blocks stays the finalize
// kernel's); nblk is always the LOGICAL block count.
template <typename T, int VW, int PIX, bool FUSED, bool TRAIN, bool SM, bool RIN = false, bool GATHER = false,
          bool PAIR = false>
__global__ __launch_bounds__(PAIR ? 512 : 256, PAIR ? 1 : 2) void m1s_pool_fwd_kernel(
    const T* __restrict__ X, int P, int S, int nblk, int act, const float* __restrict__ Wa,
    const float* __restrict__ ba, float* __restrict__ att, float* __restrict__ pacc,
    // ---- beyond the preload window ----
    float* __restrict__ pstat, float inv_keep, uint32_t thresh, uint64_t seed, uint64_t offset,
    const uint64_t* __restrict__ offset_dev, uint8_t* __restrict__ maskbits, M1GatherArg<GATHER> g) {
  constexpr int EPV = Vec<T>::EPV;
  constexpr int EPL = VW * EPV;   // channels per lane
  constexpr int CW = EPL * 64;    // channels per wave
  constexpr int C = CW * 4;
  static_assert(!(PAIR && SM), "softmax instances keep one block per logical block");
  __shared__ __attribute__((aligned(16))) float sm_xq[PAIR ? 2 : 1][APA_M1S_NB][256];   // per quad: one exchange buffer per ring slot
  __shared__ __attribute__((aligned(16))) float sm_row[PAIR ? C : 4];

  const PairId id = pair_id<PAIR>(nblk);
  const unsigned blk = (unsigned)id.blk;
  const int n = (int)(blk / (unsigned)S), s = (int)(blk % (unsigned)S);
  const int wave = id.wave, lane = threadIdx.x & 63;
  float (*sm_x)[256] = sm_xq[id.quad];
  int p_begin, p_end;
  m1_pix_range(s, P, S, p_begin, p_end);
  const int npt = p_end - p_begin;
  const int nchunk = (npt + PIX - 1) / PIX;
  const int cbase = wave * CW + lane * EPV;   // + j * 64 * EPV

  const T* xim = opaque_global(X + (size_t)(GATHER ? m1_src_image(n, g) : n) * P * C);
  float* att_im = att + (size_t)n * P;
  uint8_t* bits_im = TRAIN ? maskbits + (size_t)n * P * MaskBytes<EPL>::BPP : nullptr;

  const int p_last = p_end - 1;
  constexpr int NB = APA_M1S_NB;                 // register ring: NB - 1 chunks in flight beside the one in work
  uint4 xr[NB][PIX][VW];
  const int l16 = lane & 15;
  const float* att_rd = opaque_global(static_cast<const float*>(att_im));   // (!FUSED: read-only here)
  float av_r[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) av_r[b] = 0.f;
#pragma unroll
  for (int b = 0; b < NB - 1; ++b) {
    if (!FUSED) av_r[b] = att_rd[min(p_begin + b * PIX + l16, p_last)];
    load_chunk<T, VW, PIX>(xr[b], xim, p_begin + b * PIX, p_last, C, cbase);
  }
  FwdState<T, VW, PIX, FUSED, TRAIN> st;
#pragma unroll
  for (int i = 0; i < EPL; ++i) st.acc[i] = 0.f;
  st.bias = 0.f; st.m_run = -INFINITY; st.l_run = 0.f; st.a_sum = 0.f;
  if (FUSED) {   // L2 hits, issued in the shadow of the first chunk's HBM loads
#pragma unroll
    for (int j = 0; j < VW; ++j) {
#pragma unroll
      for (int e = 0; e < EPV; e += 4) {
        const float4 w = *reinterpret_cast<const float4*>(Wa + cbase + j * 64 * EPV + e);
        st.wa[j * EPV + e + 0] = w.x; st.wa[j * EPV + e + 1] = w.y;
        st.wa[j * EPV + e + 2] = w.z; st.wa[j * EPV + e + 3] = w.w;
      }
    }
    st.bias = ba[0];
  }
  __builtin_amdgcn_sched_barrier(0);   // every load through the window's pointers is out: now the first scalar wait
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset_dev ? *offset_dev : offset, k0, k1);

  // chunk k + NB - 1 is always fetched (clamped to the block's last pixel past the end: L1/L2 hits)
  for (int ch = 0; ch < nchunk; ch += NB) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (u > 0 && ch + u >= nchunk) break;
      constexpr int NBm1 = NB - 1;
      const int slot = (u + NBm1) % NB;
      if (!FUSED) av_r[slot] = att_rd[min(p_begin + (ch + u + NBm1) * PIX + l16, p_last)];
      load_chunk<T, VW, PIX>(xr[slot], xim, p_begin + (ch + u + NBm1) * PIX, p_last, C, cbase);
      fwd_chunk<T, VW, PIX, FUSED, TRAIN, SM, RIN>(st, xr[u], chunk_range<PIX>(p_begin, p_end, ch + u), sm_x[u], att_im,
                                                   n, P, C, cbase, wave, lane, act, inv_keep, thresh, k0, k1, bits_im,
                                                   av_r[u]);
    }
  }

  if constexpr (PAIR) {
    // the barriers of the partner's surplus chunks (FUSED: one per chunk, block_dots), then the hand-over
    if (FUSED)
      for (int ch = nchunk, nc = partner_chunks<PIX>(s, P, S); ch < nc; ++ch) __syncthreads();
    pair_merge<EPL, EPV>(st.acc, sm_row, id.quad, cbase);
  }
  if (!PAIR || id.quad == 0) {
    float* pa = pacc + (size_t)(PAIR ? blk >> 1 : blk) * C + cbase;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
#pragma unroll
      for (int e = 0; e < EPV; e += 4) {
        const int i = j * EPV + e;
        *reinterpret_cast<float4*>(pa + j * 64 * EPV + e) =
            make_float4(st.acc[i], st.acc[i + 1], st.acc[i + 2], st.acc[i + 3]);
      }
    }
  }
  m1_gather_note(n, s == 0 && id.tid == 0, g);
  if (id.tid == 0) {
    pstat[blk * 4 + 0] = (FUSED && SM) ? st.m_run : 0.f;
    pstat[blk * 4 + 1] = st.l_run;
    pstat[blk * 4 + 2] = st.a_sum;
    pstat[blk * 4 + 3] = 0.f;
  }
}

// --------------------------------------------------------------------------------------------
// Backward streaming pass (the dominant kernel: reads X once, writes dX once).  Same outputs as
// m1_bwd_main_kernel (apa_m1_vec.hip): dX, dZout (!FUSED), pdwa[blk][C], pdba[blk] (FUSED).
// --------------------------------------------------------------------------------------------
template <typename T, int VW, int PIX, bool FUSED, bool TRAIN>
struct BwdState {
  static constexpr int EPV = Vec<T>::EPV;
  static constexpr int EPL = VW * EPV;
  float dzr[EPL];
  float wa[FUSED ? EPL : 1];
  float dwa[FUSED ? EPL : 1];
  float dba_acc, sn, corr;
};

template <typename T, int VW, int PIX, bool FUSED, bool TRAIN, bool SM, bool RIN, bool BITS, bool NODX = false>
__device__ __forceinline__ void bwd_chunk(BwdState<T, VW, PIX, FUSED, TRAIN>& st,
                                          const uint4 (&xr)[PIX][VW], float a_l, float e_l,
                                          const uint32_t (&kbits)[PIX],
                                          ChunkRange cr, float* sm, T* __restrict__ dxim,
                                          float* __restrict__ dZout_im, int n, int P, int C,
                                          int cbase, int wave, int lane, int act, float invP,
                                          float inv_keep, uint32_t thresh, uint32_t k0,
                                          uint32_t k1) {
  constexpr int EPV = Vec<T>::EPV;
  constexpr int EPL = VW * EPV;
  constexpr int MBW = (PIX * EPL + 31) / 32;   // mask-bit words per lane
  const int q0 = cr.q0, np = cr.np;
  uint32_t mb[TRAIN ? MBW : 1];
  if (TRAIN) {
#pragma unroll
    for (int w = 0; w < MBW; ++w) mb[w] = 0u;
  }
  float d[PIX];
#pragma unroll
  for (int i = 0; i < PIX; ++i) {
    const int pi = min(q0 + i, q0 + np - 1);   // surplus slots repeat the last pixel
    const uint64_t ebase = ((uint64_t)n * P + pi) * C + cbase;
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      float x[EPV];
      Vec<T>::unpack(xr[i][j], x);
      relu_in<RIN>(x);
#pragma unroll
      for (int e = 0; e < EPV; e += 2) {
        const int c = j * EPV + e;
        if (TRAIN) {
          const uint32_t b = BITS ? ((kbits[i] >> c) & 3u)
                                  : rng_keep2_bits(ebase + j * 64 * EPV + e, k0, k1, thresh);
          if constexpr (!NODX) {   // kept for the dX loop below only
            const int bit = i * EPL + c;
            mb[bit >> 5] |= b << (bit & 31);
          }
          d0 = fmaf((b & 1u) ? x[e] : 0.f, st.dzr[c], d0);
          d1 = fmaf((b & 2u) ? x[e + 1] : 0.f, st.dzr[c + 1], d1);
        } else {
          d0 = fmaf(x[e], st.dzr[c], d0);
          d1 = fmaf(x[e + 1], st.dzr[c + 1], d1);
        }
      }
    }
    d[i] = d0 + d1;
  }
  float tot = block_dots<PIX>(d, sm, wave, lane);
  if (TRAIN) tot *= inv_keep;
  const float dA = (tot + st.sn + e_l) * invP;   // e_l: extra channels' share (apa_m1_cat.hip), else 0
  float dZl;
  if constexpr (SM) dZl = a_l * (dA - st.corr);
  else dZl = (act == M1_ACT_RELU && !(a_l > 0.f)) ? 0.f : dA;   // relu gates on att > 0, identity passes dA
  if (!FUSED && wave == 0 && lane < np) dZout_im[q0 + lane] = dZl;
  // NODX: nothing is stored through dX (APA_FLAG_FROZEN_INPUT: nobody reads it; APA_IFLAG_NO_DX, fused cfg 003 step:
  // the dX share A/P . dz . mask/keep is formed by the pose head's dX product in its epilogue).  With Xatt != X the
  // loop below does nothing else; with Xatt == X it still accumulates dwa / dba from the chunk in registers, in the
  // same order as the writing arm -- only o[], the packed mask words and the stores go away
  if constexpr (NODX && !FUSED) return;

#pragma unroll
  for (int i = 0; i < PIX; ++i) {
    // slot i >= np duplicates slot np-1: it stores the same dX row again (identical bytes) and
    // contributes nothing to dwa / dba
    const int src = min(i, np - 1);
    const float dZ = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dZl), src));
    const float ap = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, a_l), src)) * invP;
    const float apk = TRAIN ? ap * inv_keep : ap;
    const float dZa = i < np ? dZ : 0.f;
    if (FUSED) st.dba_acc += dZa;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      float x[EPV], o[EPV];
      if (FUSED) Vec<T>::unpack(xr[i][j], x);
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const int c = j * EPV + e;
        if constexpr (NODX) {   // (FUSED) the weight-gradient half of the arm below, nothing else
          if constexpr (FUSED) st.dwa[c] = fmaf(dZa, RIN ? fmaxf(x[e], 0.f) : x[e], st.dwa[c]);
          continue;
        }
        float t = apk;
        if (TRAIN) {
          const int bit = i * EPL + c;
          t = ((mb[bit >> 5] >> (bit & 31)) & 1u) ? apk : 0.f;
        }
        if (FUSED) {
          o[e] = fmaf(t, st.dzr[c], dZ * st.wa[c]);
          if (RIN) {   // d/dXin of max(Xin, 0): the gradient passes where Xin > 0
            o[e] = x[e] > 0.f ? o[e] : 0.f;
            st.dwa[c] = fmaf(dZa, fmaxf(x[e], 0.f), st.dwa[c]);
          } else {
            st.dwa[c] = fmaf(dZa, x[e], st.dwa[c]);
          }
        } else {
          o[e] = t * st.dzr[c];
        }
      }
      if constexpr (!NODX) st16_nt(dxim + (size_t)(q0 + src) * C + cbase + j * 64 * EPV, Vec<T>::pack(o));
    }
  }
}

template <int BPL> __device__ __forceinline__ uint32_t ld_keep_bits(const uint8_t* p) {
  if (BPL == 1) return *p;
  return *reinterpret_cast<const uint16_t*>(p);
}

template <typename T, int VW, int PIX, bool FUSED, bool TRAIN, bool SM, bool RIN = false, bool BITS = false,
          bool NODX = false, bool GATHER = false>
__global__ __launch_bounds__(256, 2) void m1s_bwd_main_kernel(
    const T* __restrict__ X, int P, int S, int nblk, int K, const float* __restrict__ att,
    const float* __restrict__ dA_extra, const uint8_t* __restrict__ maskbits, const float* __restrict__ dz,
    // ---- beyond the preload window ----
    const float* __restrict__ Wa, const float* __restrict__ zsave, const float* __restrict__ abar,
    const float* __restrict__ G, const float* __restrict__ bt, const float* __restrict__ sn_pre,
    T* __restrict__ dX, float* __restrict__ dZout, float* __restrict__ pdwa,
    float* __restrict__ pdba, int act, float inv_keep, uint32_t thresh,
    uint64_t seed, uint64_t offset, const uint64_t* __restrict__ offset_dev, float extra_scale, M1GatherArg<GATHER> g) {
  // dA_extra [N,P]: per-pixel additive term of dA * P from the concatenated pose channels; callers
  // without them pass `att` and extra_scale = 0, so the load is unconditional (straight-line code)
  constexpr int EPV = Vec<T>::EPV;
  constexpr int EPL = VW * EPV;
  constexpr int CW = EPL * 64;
  constexpr int C = CW * 4;
  __shared__ __attribute__((aligned(16))) float sm_x[APA_M1S_NB][256];
  __shared__ float sm_aux[4];

  const unsigned blk = (unsigned)xcd_remap(blockIdx.x, nblk);
  const int n = (int)(blk / (unsigned)S), s = (int)(blk % (unsigned)S);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15;
  int p_begin, p_end;
  m1_pix_range(s, P, S, p_begin, p_end);
  const int npt = p_end - p_begin;
  const int nchunk = (npt + PIX - 1) / PIX;
  const int cbase = wave * CW + lane * EPV;
  const float invP = 1.0f / (float)P;

  const T* xim = opaque_global(X + (size_t)(GATHER ? m1_src_image(n, g) : n) * P * C);
  T* dxim = NODX ? nullptr : dX + (size_t)n * P * C;   // NODX: dX may be NULL and is never dereferenced
  const float* att_im = opaque_global(att + (size_t)n * P);     // (prefetched with the chunk: keep the loads chained)
  float* dZout_im = FUSED ? nullptr : dZout + (size_t)n * P;

  const int p_last = p_end - 1;
  constexpr int NB = APA_M1S_NB;
  uint4 xr[NB][PIX][VW];
  const float* ex_im = opaque_global(dA_extra + (size_t)n * P);
  // BITS: the forward pass left the keep decisions of this lane's channels behind, BPL bytes per pixel
  constexpr int BPL = MaskBytes<EPL>::BPL;
  constexpr int BPP = MaskBytes<EPL>::BPP;
  const uint8_t* kb_im = BITS ? opaque_global(maskbits + (size_t)n * P * BPP) + (size_t)(wave * 64 + lane) * BPL : nullptr;
  float a_r[NB], e_r[NB];
  uint32_t kb_r[NB][PIX];
  auto fetch = [&](int slot_, int ch_) {      // everything of chunk ch_ that comes from memory, into ring slot slot_
    load_chunk<T, VW, PIX, APA_BWD_NT_LOAD>(xr[slot_], xim, p_begin + ch_ * PIX, p_last, C, cbase);
    a_r[slot_] = att_im[min(p_begin + ch_ * PIX + l16, p_last)];
    e_r[slot_] = ex_im[min(p_begin + ch_ * PIX + l16, p_last)] * extra_scale;
#pragma unroll
    for (int i = 0; i < PIX; ++i)
      kb_r[slot_][i] = BITS ? ld_keep_bits<BPL>(kb_im + (size_t)min(p_begin + ch_ * PIX + i, p_last) * BPP) : 0u;
  };
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    a_r[b] = 0.f; e_r[b] = 0.f;
#pragma unroll
    for (int i = 0; i < PIX; ++i) kb_r[b][i] = 0u;
  }
  // i-th chunk of the walk (slots past the end re-read the walk's last chunk: L1/L2 hits)
  auto walk = [&](int i_) { return max(nchunk - 1 - i_, 0); };
#pragma unroll
  for (int b = 0; b < NB - 1; ++b) fetch(b, walk(b));
  uint32_t k0 = 0, k1 = 0;
  if (TRAIN) rng_key_dev(seed, offset_dev ? *offset_dev : offset, k0, k1);

  // per-image constants: L2 hits issued behind the first chunk's HBM loads
  BwdState<T, VW, PIX, FUSED, TRAIN> st;
  st.dba_acc = 0.f; st.sn = 0.f; st.corr = 0.f;
  {
    float zdz = 0.f;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
#pragma unroll
      for (int e = 0; e < EPV; e += 4) {
        const int i = j * EPV + e;
        const int c = cbase + j * 64 * EPV + e;
        const float4 dd = *reinterpret_cast<const float4*>(dz + (size_t)n * C + c);
        st.dzr[i] = dd.x; st.dzr[i + 1] = dd.y; st.dzr[i + 2] = dd.z; st.dzr[i + 3] = dd.w;
        if (FUSED) {
          const float4 w = *reinterpret_cast<const float4*>(Wa + c);
          st.wa[i] = w.x; st.wa[i + 1] = w.y; st.wa[i + 2] = w.z; st.wa[i + 3] = w.w;
          st.dwa[i] = 0.f; st.dwa[i + 1] = 0.f; st.dwa[i + 2] = 0.f; st.dwa[i + 3] = 0.f;
        }
        if constexpr (SM) {
          const float4 zz = *reinterpret_cast<const float4*>(zsave + (size_t)n * C + c);
          zdz = fmaf(zz.x, dd.x, zdz); zdz = fmaf(zz.y, dd.y, zdz);
          zdz = fmaf(zz.z, dd.z, zdz); zdz = fmaf(zz.w, dd.w, zdz);
        }
      }
    }
    if (sn_pre) {
      st.sn = sn_pre[n];
    } else {   // G[n,:] . bt
      float sn = 0.f;
      for (int k = lane; k < K; k += 64) sn = fmaf(G[(size_t)n * K + k], bt[k], sn);
      st.sn = wave_sum(sn);
    }
    if constexpr (SM) {   // corr = z.dz + (G.bt) * abar, z.dz summed over the 4 waves
      zdz = wave_sum(zdz);
      if (lane == 0) sm_aux[wave] = zdz;
      __syncthreads();
      st.corr = ((sm_aux[0] + sm_aux[1]) + (sm_aux[2] + sm_aux[3])) + st.sn * abar[n];
    }
  }

  for (int ch = 0; ch < nchunk; ch += NB) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (u > 0 && ch + u >= nchunk) break;
      constexpr int NBm1 = NB - 1;
      fetch((u + NBm1) % NB, walk(ch + u + NBm1));
      bwd_chunk<T, VW, PIX, FUSED, TRAIN, SM, RIN, BITS, NODX>(
          st, xr[u], a_r[u], e_r[u], kb_r[u], chunk_range<PIX>(p_begin, p_end, walk(ch + u)), sm_x[u], dxim, dZout_im, n,
          P, C, cbase, wave, lane, act, invP, inv_keep, thresh, k0, k1);
    }
  }

  if (FUSED) {
    float* pa = pdwa + (size_t)blk * C + cbase;
#pragma unroll
    for (int j = 0; j < VW; ++j) {
#pragma unroll
      for (int e = 0; e < EPV; e += 4) {
        const int i = j * EPV + e;
        *reinterpret_cast<float4*>(pa + j * 64 * EPV + e) =
            make_float4(st.dwa[i], st.dwa[i + 1], st.dwa[i + 2], st.dwa[i + 3]);
      }
    }
    if (threadIdx.x == 0) pdba[blk] = st.dba_acc;
  }
}

// ============================================================================================
// host side
// ============================================================================================
bool m1s_supported(int C, int dtype) {
  const int epv = dtype == APA_DTYPE_BF16 ? 8 : 4;
  if (C % (256 * epv) != 0) return false;
  const int vw = C / (256 * epv);
  // bf16 at C >= 4096 would spill (the unpacked chunk does not fit 256 VGPRs): per-pixel kernels
  if (dtype == APA_DTYPE_BF16) return vw == 1;
  return vw == 1 || vw == 2 || vw == 4;
}

// Chunk width (pixels per register buffer).  bf16: 2 (the keep-bits hand-off is built for it).  fp32: 1 since round 6 --
// with the prefetch finally in front of the chunk it overlaps (opaque_global above) the finer grain wins at the
// benchmark batch: the first chunk's arithmetic starts after 8 KB instead of 16 KB per block and less work is left
// behind the last load (A/B on one box, two runs each: step 51.4 -> 50.1 us, backward kernel 19.45 -> 18.65 us by
// events; N = 512 unchanged, 276 us; 4 and 8 lose 3 and 6 us).
// (C = 4096 fp32, VW = 4: 2)
template <typename T, int VW> constexpr int kPix = sizeof(T) == 2 ? 2 : (VW == 4 ? 2 : 1);

template <typename T, int VW>
static int launch_fwd_t(const M1Call& c, const M1Fwd& io) {
  constexpr int PIX = kPix<T, VW>;
  if (M1Trace* t = m1_trace()) { t->pool_fwd = M1_POOL_STREAM; t->fwd_w = VW; t->fwd_pix = PIX; }
  m1_pool_form(c, [&](auto F, auto TR, auto G) {
    constexpr bool f = decltype(F)::value, t = decltype(TR)::value, g = decltype(G)::value;
    auto arm = [&](auto SM, auto PR) {
      constexpr bool sm = decltype(SM)::value, pr = decltype(PR)::value;
      auto k = m1s_pool_fwd_kernel<T, VW, PIX, f, t, sm, false, g, pr>;
      // relu on the input: instantiated for the plain fused map only (m1_call_fill: relu_input is fused, never gathered)
      if constexpr (f && !g) {
        if (c.relu_input) k = m1s_pool_fwd_kernel<T, VW, PIX, true, t, sm, true, false, pr>;
      }
      return k;
    };
    const std::true_type yes; const std::false_type no;
    auto kernel = arm(no, no);
    // the paired form (m1_call_fill: c.nrows): fp32 features, every instance but the softmax ones
    const bool pair = c.paired();
    if constexpr (sizeof(T) == 4) {
      if (pair) kernel = arm(no, yes);
    }
    // softmax: plain fused maps only (m1_call_fill: pool_act is the identity on a map that is already final, and both
    // forms a gathered call can have -- the cache form and the cfg 003 steps' pose form -- exclude softmax)
    if constexpr (f && !g) {
      if (c.pool_act == M1_ACT_SOFTMAX) kernel = arm(yes, no);
    }
    launch_ev(kernel, dim3(c.nrows), dim3(pair ? 512 : 256), 0, c.st, c.ev0, c.ev1, static_cast<const T*>(io.X), c.P, c.pl.S,
              c.pl.nblk, c.pool_act, io.Wa, io.ba, io.att, c.pacc, c.pstat, c.inv_keep, c.key.thresh, c.key.seed,
              c.key.offset, c.key.offset_dev, c.maskbits, m1_gather_arg<g>(c));
    return APA_OK;
  });
  APA_LAUNCH_CHECK("m1s_pool_fwd_kernel");
  return APA_OK;
}

template <typename T, int VW>
static int launch_bwd_t(const M1Call& c, const M1Bwd& io) {
  constexpr int PIX = kPix<T, VW>;
  M1Trace* const tr = m1_trace();
  if (tr) { tr->pool_bwd = M1_POOL_STREAM; tr->bwd_w = VW; tr->bwd_pix = PIX; }
  // non-null: the forward call's keep-bits (APA_FLAG_WS_FROM_FWD)
  const uint8_t* mbits = c.relu_input ? nullptr : c.maskbits_in;
  bool bits = false;   // the keep-bits variant: bf16 features
  if constexpr (KeepBits<T>::ON) bits = c.train && mbits;
  if (tr && !c.relu_input) tr->keep_bits = bits;
  m1_pool_form(c, [&](auto F, auto TR, auto G) {
    constexpr bool f = decltype(F)::value, t = decltype(TR)::value, g = decltype(G)::value;
    // every form has its arm without the dX stores (APA_FLAG_FROZEN_INPUT / APA_IFLAG_NO_DX): c.no_dx never reaches an
    // instance that stores through dX, and a gathered call (m1_call_fill: no dX) has no instance that does
    auto arm = [&](auto RIN, auto BITS) {
      constexpr bool r = decltype(RIN)::value, b = decltype(BITS)::value;
      auto act_arm = [&](auto SM) {
        constexpr bool sm = decltype(SM)::value;
        auto k = m1s_bwd_main_kernel<T, VW, PIX, f, t, sm, r, b, true, g>;
        if constexpr (!g) {
          if (!c.no_dx) k = m1s_bwd_main_kernel<T, VW, PIX, f, t, sm, r, b, false>;
        }
        return k;
      };
      // softmax: every plain form has its instance (dZ is formed in this pass, fused or not); a gathered call has none
      // (m1_call_fill: the cache form and the pose form exclude softmax)
      if constexpr (!g) {
        if (c.act == M1_ACT_SOFTMAX) return act_arm(std::true_type{});
      }
      return act_arm(std::false_type{});
    };
    const std::true_type yes; const std::false_type no;
    auto kernel = arm(no, no);
    // relu on the input: instantiated for the plain fused map only (m1_call_fill: relu_input is fused, never gathered;
    // mbits is null then)
    if constexpr (f && !g) {
      if (c.relu_input) kernel = arm(yes, no);
    }
    // the keep bits: training mode, bf16 features
    if constexpr (KeepBits<T>::ON && t) {
      if (bits) kernel = arm(no, yes);
    }
    launch_ev(kernel, dim3(c.pl.nblk), dim3(256), 0, c.st, c.ev0, c.ev1, static_cast<const T*>(io.X), c.P, c.pl.S,
              c.pl.nblk, c.K, io.att, c.ex, mbits, c.dz, io.Wa, io.zsave, io.abar, io.G, io.bt, c.sn,
              g ? nullptr : static_cast<T*>(io.dX), c.dzatt, c.pdwa, c.pdba, c.act, c.inv_keep, c.key.thresh, c.key.seed,
              c.key.offset, c.key.offset_dev, c.exs, m1_gather_arg<g>(c));
    return APA_OK;
  });
  APA_LAUNCH_CHECK("m1s_bwd_main_kernel");
  return APA_OK;
}

#define APA_S_DISPATCH(FN)                                                  \
  if (c.dtype == APA_DTYPE_F32) {                                           \
    switch (c.C / 1024) {                                                   \
      case 1: return FN<float, 1>(c, io);                                   \
      case 2: return FN<float, 2>(c, io);                                   \
      case 4: return FN<float, 4>(c, io);                                   \
    }                                                                       \
  } else {                                                                  \
    if (c.C == 2048) return FN<bf16_t, 1>(c, io);                           \
  }                                                                         \
  set_error("m1 stream kernels: unsupported C=%d dtype=%d", c.C, c.dtype);  \
  return APA_ERR_UNSUPPORTED

int m1s_launch_pool_fwd(const M1Call& c, const M1Fwd& io) { APA_S_DISPATCH(launch_fwd_t); }
int m1s_launch_bwd_main(const M1Call& c, const M1Bwd& io) { APA_S_DISPATCH(launch_bwd_t); }
#undef APA_S_DISPATCH

}  // namespace apa
