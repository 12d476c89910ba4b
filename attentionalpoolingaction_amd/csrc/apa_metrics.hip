// apa_metrics.hip -- the number an evaluation reports: per-class average precision, their mean and the accuracy of
// T accumulated score rows, on the device.
//
// Reference semantics.  src/eval.py:303-306 (accuracy, compute_map), src/eval/utils.py:4-16 (compute_map: class k's
// positives are labels == k, classes without one are skipped) and src/eval/cap_eval_utils.py:55-109
// (calc_pr_ovr_noref: P = ctp / (ctp + cfp), R = ctp / npos over the descending ranking; voc_ap: the area under the
// right-max envelope of P over the recall steps), all in float64.
//
// The ranking rule (include/apa.h): scores descending, equal scores by DESCENDING sample index, -0.0 == +0.0, a NaN
// last.  One 64-bit key per (class, sample) carries it: the order-preserving image of the score in the high word,
// (index << 1) | positive in the low word; sorted descending, the keys of the T samples are distinct.
//
// apa_average_precision, three launches, no floating-point atomics:
//   1. ap_pack_kernel        block b owns samples [32 b, 32 b + 32) and walks the classes in tiles of 64: rows are
//                            read with coalesced loads (a wave per row, lanes along the classes), turned through an LDS
//                            tile and stored as keys into the class-major [K][Tpad] image of the workspace, lanes
//                            along the samples (256 contiguous bytes per class and half-wave).  Slots T .. Tpad - 1
//                            get the smallest key, 0.  The same walk keeps each row's first maximum (np.argmax) and
//                            counts the NaN scores and the labels outside [0,K): three integers per block, no atomics.
//   2. ap_sort_scan_kernel   one block per class, Tpad / 16 threads, 16 keys per thread.  A bitonic network sorts the
//                            class's Tpad keys descending: every stage of stride < 16 runs on the 16 keys a thread
//                            holds in registers, the stages of stride >= 16 four at a time on 16 keys a thread
//                            gathers from LDS with the lowest stride of the four between them -- one LDS round trip
//                            per four stages.  The image is XOR-swizzled (slot i lives at i ^ ((i >> 4) & 15)) so
//                            that both the contiguous and the strided gathers are bank-conflict free.  Then, on the
//                            sorted registers: the integer scan of the positive bits, P = ctp / (i + 1) at the
//                            positives (float64, correctly rounded), the suffix maximum of P, and the sum of
//                            (R_i - R_{i-1}) * envelope_i over the positives in rank order, as voc_ap's loop adds
//                            them (the terms are compacted into LDS, one lane adds them).
//   3. ap_finish_kernel      one wave: the mean of the APs of the classes with positives, the accuracy quotient and
//                            the two status words from the per-block counts.
// No fast-math on this file: the float64 divisions are IEEE divisions and no product is contracted into a sum.
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

namespace {

typedef unsigned long long u64;

constexpr int APK_TS = 32;          // samples per block of the pack kernel
constexpr int APK_TK = 64;          // classes per tile: one wave's lanes
constexpr int APK_THREADS = 256;
constexpr int APK_ROWS = APK_TS / (APK_THREADS / 64);   // rows a wave reads per tile
constexpr int APS_E = 16;           // keys per thread of the sort kernel
constexpr int APS_MAX_THREADS = APA_AP_MAX_SAMPLES / APS_E;
constexpr int AP_TPAD_MIN = 64 * APS_E;   // one wave's keys

static_assert(APS_MAX_THREADS == 1024, "one block sorts the largest class image");

struct ApPlan {
  int Tpad, ln, nblk;
  size_t off_keys, off_part, total;
};

ApPlan ap_plan(int T, int K) {
  ApPlan pl;
  int tp = AP_TPAD_MIN, ln = 10;
  while (tp < T) { tp <<= 1; ++ln; }
  pl.Tpad = tp;
  pl.ln = ln;
  pl.nblk = tp / APK_TS;
  size_t off = 0;
  pl.off_keys = off; off += align_up((size_t)K * tp * sizeof(u64), 256);
  pl.off_part = off; off += align_up((size_t)pl.nblk * 4 * sizeof(int32_t), 256);
  pl.total = off;
  return pl;
}

// the high word of a key: unsigned order == the ranking's order of the scores.  0 is left to the padding, 1 to NaN
// (the image of -inf is 0x007fffff, the smallest of a number)
__device__ __forceinline__ uint32_t ap_score_image(float v, bool& nan) {
  uint32_t u = __float_as_uint(v);
  if ((u << 1) == 0u) u = 0u;                       // -0.0 ranks as +0.0
  nan = (u & 0x7fffffffu) > 0x7f800000u;
  const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return nan ? 1u : ord;
}

// (value, class) of a row's maximum so far; i < 0: none yet.  `a` replaces `b` when it is larger, or equal and earlier
__device__ __forceinline__ bool ap_argmax_better(float av, int ai, float bv, int bi) {
  return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi));
}

__global__ __launch_bounds__(APK_THREADS) void ap_pack_kernel(
    const float* __restrict__ scores, const int64_t* __restrict__ labels, const float* __restrict__ targets,
    u64* __restrict__ keys, int32_t* __restrict__ partials, int T, int K, int Tpad) {
  __shared__ uint32_t s_hi[APK_TS][APK_TK + 1];
  __shared__ uint8_t s_pos[APK_TS][APK_TK + 4];
  __shared__ int s_part[APK_THREADS / 64][3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int s0 = blockIdx.x * APK_TS;

  float bv[APK_ROWS];
  int bi[APK_ROWS];
  int64_t lab[APK_ROWS];
#pragma unroll
  for (int q = 0; q < APK_ROWS; ++q) {
    const int s = s0 + wave + 4 * q;
    bv[q] = 0.f;
    bi[q] = -1;
    lab[q] = (labels && s < T) ? labels[s] : (int64_t)-1;
  }
  int n_nan = 0;

  for (int k0 = 0; k0 < K; k0 += APK_TK) {
    // rows in: a wave per row, lanes along the classes
    const int k = k0 + lane;
#pragma unroll
    for (int q = 0; q < APK_ROWS; ++q) {
      const int row = wave + 4 * q, s = s0 + row;
      const bool ok = s < T && k < K;
      const size_t at = (size_t)(ok ? s : 0) * K + (ok ? k : 0);
      const float v = scores[at];
      bool nan;
      const uint32_t hi = ap_score_image(v, nan);
      const bool pos = targets ? targets[at] > 0.f : lab[q] == (int64_t)k;
      n_nan += (ok && nan) ? 1 : 0;
      if (ok && (bi[q] < 0 || v > bv[q])) { bv[q] = v; bi[q] = k; }   // lane-local: ascending k, the first stays
      s_hi[row][lane] = ok ? hi : 0u;
      s_pos[row][lane] = (ok && pos) ? 1 : 0;
    }
    __syncthreads();
    // keys out: lanes along the samples, eight classes per step
    const int sl = threadIdx.x & (APK_TS - 1), cg = threadIdx.x >> 5;
    const int s = s0 + sl;
#pragma unroll
    for (int it = 0; it < APK_TK / 8; ++it) {
      const int c = it * 8 + cg, kk = k0 + c;
      if (kk < K) {
        const u64 key = ((u64)s_hi[sl][c] << 32) | (u64)(((uint32_t)s << 1) | s_pos[sl][c]);
        keys[(size_t)kk * Tpad + s] = s < T ? key : 0ull;
      }
    }
    __syncthreads();
  }

  // the row's first maximum over the lanes, then this wave's three counts
  int n_ok = 0, n_bad = 0;
#pragma unroll
  for (int q = 0; q < APK_ROWS; ++q) {
    float v = bv[q];
    int i = bi[q];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float ov = __shfl_xor(v, d);
      const int oi = __shfl_xor(i, d);
      if (ap_argmax_better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    const int s = s0 + wave + 4 * q;
    if (labels && s < T) {
      n_ok += ((int64_t)i == lab[q]) ? 1 : 0;
      n_bad += (lab[q] < 0 || lab[q] >= (int64_t)K) ? 1 : 0;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) n_nan += __shfl_xor(n_nan, d);
  if (lane == 0) { s_part[wave][0] = n_ok; s_part[wave][1] = n_nan; s_part[wave][2] = n_bad; }
  __syncthreads();
  if (threadIdx.x < 3) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < APK_THREADS / 64; ++w) t += s_part[w][threadIdx.x];
    partials[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// sort + scan
// ---------------------------------------------------------------------------------------------------------------
// compare-exchange of the keys at a lower (a) and a higher (b) slot.  Equal keys are padding: either order
__device__ __forceinline__ void ap_cx(u64& a, u64& b, bool desc) {
  const bool sw = (a < b) == desc;
  const u64 x = sw ? b : a, y = sw ? a : b;
  a = x; b = y;
}

// the stages of strides JTOP .. 1 of merge size k on the 16 keys at slots base .. base + 15
template <int JTOP>
__device__ __forceinline__ void ap_reg_stages(u64 (&r)[APS_E], int base, int k) {
#pragma unroll
  for (int j = JTOP; j >= 1; j >>= 1)
#pragma unroll
    for (int m = 0; m < APS_E; ++m)
      if (!(m & j)) ap_cx(r[m], r[m | j], ((base | m) & k) == 0);
}

// one stage of merge size k on 16 keys gathered from slots base | (m << ls): registers m and m | (1 << MM) are partners
template <int MM>
__device__ __forceinline__ void ap_gathered_stage(u64 (&r)[APS_E], int base, int ls, int k) {
#pragma unroll
  for (int m = 0; m < APS_E; ++m)
    if (!(m & (1 << MM))) ap_cx(r[m], r[m | (1 << MM)], ((base | (m << ls)) & k) == 0);
}

__device__ __forceinline__ int ap_phys(int i) { return i ^ ((i >> 4) & 15); }

__global__ __launch_bounds__(APS_MAX_THREADS) void ap_sort_scan_kernel(
    const u64* __restrict__ keys, double* __restrict__ ap, int32_t* __restrict__ npos_out, int Tpad, int ln) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) u64 sm_keys[];   // [Tpad], swizzled
  __shared__ int s_cnt[APS_MAX_THREADS / 64];
  __shared__ double s_max[APS_MAX_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwaves = blockDim.x >> 6;
  const int cbase = t * APS_E;   // the thread's contiguous slots

  u64 r[APS_E];
  {
    const uint4* src = reinterpret_cast<const uint4*>(keys + (size_t)blockIdx.x * Tpad + cbase);
#pragma unroll
    for (int m = 0; m < APS_E / 2; ++m) {
      const uint4 v = src[m];
      r[2 * m] = ((u64)v.y << 32) | v.x;
      r[2 * m + 1] = ((u64)v.w << 32) | v.z;
    }
  }
  ap_reg_stages<1>(r, cbase, 2);
  ap_reg_stages<2>(r, cbase, 4);
  ap_reg_stages<4>(r, cbase, 8);
  ap_reg_stages<8>(r, cbase, 16);

  for (int lk = 5; lk <= ln; ++lk) {
    const int k = 1 << lk;
#pragma unroll
    for (int m = 0; m < APS_E; ++m) sm_keys[ap_phys(cbase | m)] = r[m];
    __syncthreads();
    int ljt = lk - 1;                       // log2 of the largest stride left in this merge
    while (ljt >= 4) {
      const int g = min(4, ljt - 3);        // stages of stride >= 16 taken by this round trip
      const int ls = ljt - g + 1;           // log2 of the lowest of them: the gather's stride
      const int base = (t & ((1 << ls) - 1)) | ((t >> ls) << (ls + 4));
#pragma unroll
      for (int m = 0; m < APS_E; ++m) r[m] = sm_keys[ap_phys(base | (m << ls))];
      if (g >= 4) ap_gathered_stage<3>(r, base, ls, k);
      if (g >= 3) ap_gathered_stage<2>(r, base, ls, k);
      if (g >= 2) ap_gathered_stage<1>(r, base, ls, k);
      ap_gathered_stage<0>(r, base, ls, k);
      int sbase = base;   // the 16 slot addresses are formed again for the stores, not kept across the stages
      asm volatile("" : "+v"(sbase));
#pragma unroll
      for (int m = 0; m < APS_E; ++m) sm_keys[ap_phys(sbase | (m << ls))] = r[m];
      __syncthreads();
      ljt = ls - 1;
    }
#pragma unroll
    for (int m = 0; m < APS_E; ++m) r[m] = sm_keys[ap_phys(cbase | m)];
    ap_reg_stages<8>(r, cbase, k);
  }

  // r[m]: rank cbase + m of the class.  Inclusive count of positives: in the thread, the wave, the block
  unsigned bits = 0;
#pragma unroll
  for (int m = 0; m < APS_E; ++m) bits |= (unsigned)(r[m] & 1ull) << m;
  const int cnt = __popc(bits);
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  if (lane == 63) s_cnt[wave] = incl;
  __syncthreads();
  int before = incl - cnt, npos = 0;
  for (int w = 0; w < nwaves; ++w) {
    const int c = s_cnt[w];
    before += w < wave ? c : 0;
    npos += c;
  }
  if (npos == 0) {   // block-uniform: the class is left out of the mean
    if (t == 0) { ap[blockIdx.x] = 0.0; npos_out[blockIdx.x] = 0; }
    return;
  }

  // P at the positives only: elsewhere it is below the P of the positive in front, so the envelope at a positive is
  // the same without it.  (Formed again in the second walk instead of kept: 32 registers less)
  double tmax = 0.0;
  {
    int c = before;
#pragma unroll
    for (int m = 0; m < APS_E; ++m) {
      const bool pos = (bits >> m) & 1u;
      c += pos ? 1 : 0;
      if (pos) tmax = fmax(tmax, (double)c / (double)(cbase + m + 1));
    }
  }
  // the maximum of P over every thread behind this one (a maximum: exact in any order)
  double sfx = tmax;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_down(sfx, d);
    if (lane + d < 64) sfx = fmax(sfx, o);
  }
  if (lane == 0) s_max[wave] = sfx;
  double behind = __shfl_down(sfx, 1);
  if (lane == 63) behind = 0.0;
  __syncthreads();
  for (int w = wave + 1; w < nwaves; ++w) behind = fmax(behind, s_max[w]);

  // the recall steps.  Term c - 1 of the class -- its c-th positive by rank -- goes to LDS (the sorted keys live in
  // registers by now; every thread is past its last read of the image, two barriers back), and ONE lane adds the npos
  // terms in rank order: voc_ap's own loop, so the sum has its rounding -- and its exact cases: with a flat envelope
  // every partial sum is the representable R_i, and a class whose samples are all positives gets 1.0
  double* terms = reinterpret_cast<double*>(sm_keys);
  const double dn = (double)npos;
  {
    double env = behind;
    int c = before + cnt;
#pragma unroll
    for (int m = APS_E - 1; m >= 0; --m) {
      if ((bits >> m) & 1u) {
        env = fmax(env, (double)c / (double)(cbase + m + 1));
        const double dr = (double)c / dn - (double)(c - 1) / dn;
        terms[c - 1] = dr * env;
        --c;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    double a = 0.0;
    for (int i = 0; i < npos; ++i) a = a + terms[i];
    ap[blockIdx.x] = a;
    npos_out[blockIdx.x] = npos;
  }
}

__global__ __launch_bounds__(64) void ap_finish_kernel(const double* __restrict__ ap, const int32_t* __restrict__ npos,
                                                       const int32_t* __restrict__ partials, double* __restrict__ summary,
                                                       int32_t* __restrict__ status, int T, int K, int nblk,
                                                       int has_labels) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  double s = 0.0;
  int n = 0;
  for (int k = lane; k < K; k += 64)
    if (npos[k] > 0) { s = s + ap[k]; ++n; }
  int ok = 0, nan = 0, bad = 0;
  for (int b = lane; b < nblk; b += 64) {
    ok += partials[(size_t)b * 4 + 0];
    nan += partials[(size_t)b * 4 + 1];
    bad += partials[(size_t)b * 4 + 2];
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    s = s + __shfl_xor(s, d);
    n += __shfl_xor(n, d);
    ok += __shfl_xor(ok, d);
    nan += __shfl_xor(nan, d);
    bad += __shfl_xor(bad, d);
  }
  if (lane == 0) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    summary[0] = n > 0 ? s / (double)n : qnan;
    summary[1] = has_labels ? (double)ok / (double)T : qnan;
    summary[2] = (double)n;
    status[0] = nan;
    status[1] = bad;
  }
}

// every refusal that needs no pointer (shared by the workspace query): APA_OK, or the status
int ap_shape_check(int T, int K, bool say) {
  if (T <= 0 || K <= 0) {
    if (say) set_error("apa_average_precision: non-positive dimension T=%d K=%d", T, K);
    return APA_ERR_INVALID_ARG;
  }
  if (T > APA_AP_MAX_SAMPLES) {
    if (say)
      set_error("apa_average_precision: T=%d samples, served up to APA_AP_MAX_SAMPLES=%d (a class's keys are sorted "
                "in one block's LDS)", T, APA_AP_MAX_SAMPLES);
    return APA_ERR_UNSUPPORTED;
  }
  return APA_OK;
}

}  // namespace

}  // namespace apa

using namespace apa;

extern "C" size_t apa_average_precision_workspace_bytes(int T, int K) {
  if (ap_shape_check(T, K, false) != APA_OK) return 0;
  return ap_plan(T, K).total;
}

extern "C" int apa_average_precision(const float* scores, const int64_t* labels, const float* targets, int T, int K,
                                     double* ap, int32_t* npos, double* summary, int32_t* status, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (!scores || !ap || !npos || !summary || !status) {
    set_error("apa_average_precision: null pointer");
    return APA_ERR_INVALID_ARG;
  }
  if ((labels != nullptr) == (targets != nullptr)) {
    set_error("apa_average_precision: exactly one of labels / targets is given (got %s)", labels ? "both" : "neither");
    return APA_ERR_INVALID_ARG;
  }
  const int rc = ap_shape_check(T, K, true);
  if (rc != APA_OK) return rc;
  const ApPlan pl = ap_plan(T, K);
  if (!ws || ws_bytes < pl.total) {
    set_error("apa_average_precision: workspace of %zu bytes, %zu needed (apa_average_precision_workspace_bytes)",
              ws_bytes, pl.total);
    return APA_ERR_WORKSPACE;
  }
  if ((uintptr_t)ws & 15) {
    set_error("apa_average_precision: the workspace must be 16-byte aligned");
    return APA_ERR_INVALID_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  u64* keys = reinterpret_cast<u64*>(base + pl.off_keys);
  int32_t* partials = reinterpret_cast<int32_t*>(base + pl.off_part);
  const size_t lds = (size_t)pl.Tpad * sizeof(u64);
  {   // once per device: up to 128 KiB of dynamic LDS beside the kernel's static 320 bytes (the default limit is 64 KiB)
    static thread_local PerDevice<bool> attr_dev; bool& attr_set = attr_dev.here();
    if (!attr_set) {
      APA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ap_sort_scan_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)(APA_AP_MAX_SAMPLES * sizeof(u64))));
      attr_set = true;
    }
  }
  hipLaunchKernelGGL(ap_pack_kernel, dim3(pl.nblk), dim3(APK_THREADS), 0, st, scores, labels, targets, keys, partials,
                     T, K, pl.Tpad);
  APA_LAUNCH_CHECK("ap_pack_kernel");
  hipLaunchKernelGGL(ap_sort_scan_kernel, dim3(K), dim3(pl.Tpad / APS_E), lds, st, static_cast<const u64*>(keys), ap,
                     npos, pl.Tpad, pl.ln);
  APA_LAUNCH_CHECK("ap_sort_scan_kernel");
  hipLaunchKernelGGL(ap_finish_kernel, dim3(1), dim3(64), 0, st, static_cast<const double*>(ap),
                     static_cast<const int32_t*>(npos), static_cast<const int32_t*>(partials), summary, status, T, K,
                     pl.nblk, labels ? 1 : 0);
  APA_LAUNCH_CHECK("ap_finish_kernel");
  return APA_OK;
}
