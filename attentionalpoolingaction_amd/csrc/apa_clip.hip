// apa_clip.hip -- per-variable gradient clipping by L2 norm over many fp32 tensors (TRAIN.CLIP_GRADIENTS).
//
// Reference semantics (models/slim/deployment/model_deploy.py:297-304, src/train.py:507-513): each clone's
// gradient list goes through slim.learning.clip_gradient_norms(g, clip), i.e. tf.clip_by_norm on EVERY variable
// separately (not a global norm).  tf.clip_by_norm(t, c) in TF 1.x is written
//     l2norm_inv = rsqrt(reduce_sum(t * t));  intermediate = t * c;  tclip = intermediate * minimum(l2norm_inv, 1/c)
// and that order is kept: out = (t * c) * min(rsqrt(ss), 1/c).  Below the threshold the result is (t*c)*(1/c), an
// all-zero tensor gives rsqrt(0) = inf -> factor 1/c -> exactly 0.  On clone 0 the regulariser's gradient wd * w is
// part of t (the regularisation loss belongs to the first clone's loss) and is added here, before the norm.
//
// Two launches over one flat chunk table (built once by apa_clip_by_norm_prepare, kept in the caller's workspace):
//   1. block b reads chunk b (CLIP_CHUNK elements of one segment, dwordx4 loads, any 4-byte alignment), forms the
//      sum of squares of t = g + wd*w in double precision and writes one partial per chunk;
//   2. block b sums the partials of its segment in chunk order -- the same fixed-order tree in every block of the
//      segment, hence the same factor -- and rewrites its chunk in place.
// The chunking depends on the segment sizes only, never on occupancy; no atomics: repeated calls are bit-identical.
#include "apa_device.h"
#include "apa_internal.h"

#include <mutex>
#include <unordered_map>
#include <vector>

namespace apa {

constexpr unsigned CLIP_CHUNK = 16384;   // elements per block: 64 KB of gradient
constexpr int CLIP_THREADS = 256;

struct ClipSeg {
  float* g;             // gradient, rewritten in place
  const float* w;       // weight (read when wd != 0)
  float wd;             // regulariser coefficient added before the norm (clone 0), 0 elsewhere
  int absent;           // 1: the producer never writes g -- treated as zero (tf.gradients -> None), g not read
  int first_chunk, nchunks;
};
struct ClipChunk {
  int seg;
  unsigned cnt;                // elements in this chunk
  unsigned long long start;    // first element within the segment
};

static size_t clip_align(size_t x, size_t a) { return (x + a - 1) / a * a; }
static size_t chunks_of(size_t n) { return (n + CLIP_CHUNK - 1) / CLIP_CHUNK; }
// the first 256 bytes of the workspace: what prepare wrote.  Both kernels compare it with their launch (nseg, grid
// size) and do nothing on a mismatch -- a workspace overwritten or re-used behind the caller's back is never walked
constexpr unsigned CLIP_MAGIC = 0x434c4950u;   // "CLIP"
struct ClipHeader {
  unsigned magic;
  int nseg, nchunks, pad_;
};
constexpr size_t CLIP_HDR = 256;
struct ClipLayout {
  size_t seg_off, chunk_off, part_off, bytes;
  ClipLayout(int nseg, size_t nchunks) {
    seg_off = CLIP_HDR;
    chunk_off = clip_align(seg_off + (size_t)nseg * sizeof(ClipSeg), 256);
    part_off = clip_align(chunk_off + nchunks * sizeof(ClipChunk), 256);
    bytes = part_off + nchunks * sizeof(double);
  }
};

__device__ __forceinline__ float clip_t(const ClipSeg& s, float g, float w) { return fmaf(s.wd, w, g); }

// block-wide sum of one double per thread: xor-shuffle tree inside each wave, then the waves in index order
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[wave] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int k = 1; k < CLIP_THREADS / 64; ++k) s += sh[k];
  return s;
}

__device__ __forceinline__ bool clip_header_ok(const ClipHeader* h, int nseg) {
  return h->magic == CLIP_MAGIC && h->nseg == nseg && h->nchunks == (int)gridDim.x;
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_sumsq_kernel(const ClipHeader* __restrict__ hdr, int nseg,
                                                                  const ClipSeg* __restrict__ segs,
                                                                  const ClipChunk* __restrict__ chunks,
                                                                  double* __restrict__ partial) {
  __shared__ double sh[CLIP_THREADS / 64];
  if (!clip_header_ok(hdr, nseg)) return;          // uniform per block
  const ClipChunk c = chunks[blockIdx.x];
  if (c.seg < 0 || c.seg >= nseg) return;
  const ClipSeg s = segs[c.seg];
  const float* g = s.g + c.start;
  const float* w = s.w ? s.w + c.start : nullptr;
  const bool use_w = s.wd != 0.f && w;
  const unsigned nv = c.cnt / 4;
  double acc = 0.0;
  for (unsigned v = threadIdx.x; v < nv; v += CLIP_THREADS) {
    f4u gv = s.absent ? f4u{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f4u*>(g + v * 4);
    if (use_w) {
      const f4u wv = *reinterpret_cast<const f4u*>(w + v * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = clip_t(s, gv[e], wv[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = fma((double)gv[e], (double)gv[e], acc);
  }
  for (unsigned i = nv * 4 + threadIdx.x; i < c.cnt; i += CLIP_THREADS) {
    const float t = clip_t(s, s.absent ? 0.f : g[i], use_w ? w[i] : 0.f);
    acc = fma((double)t, (double)t, acc);
  }
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(CLIP_THREADS) void clip_apply_kernel(const ClipHeader* __restrict__ hdr, int nseg,
                                                                  const ClipSeg* __restrict__ segs,
                                                                  const ClipChunk* __restrict__ chunks,
                                                                  const double* __restrict__ partial, float clip) {
  __shared__ double sh[CLIP_THREADS / 64];
  if (!clip_header_ok(hdr, nseg)) return;
  const ClipChunk c = chunks[blockIdx.x];
  if (c.seg < 0 || c.seg >= nseg) return;
  const ClipSeg s = segs[c.seg];
  if (s.first_chunk < 0 || s.nchunks < 0 || s.first_chunk + s.nchunks > (int)gridDim.x) return;
  // the segment's partials, thread k taking chunks k, k + 256, ... in order: identical in every block of the segment
  double acc = 0.0;
  for (int k = threadIdx.x; k < s.nchunks; k += CLIP_THREADS) acc += partial[s.first_chunk + k];
  const double ss = block_sum(acc, sh);
  // min(rsqrt(ss), 1/c): ss == 0 -> inf -> 1/c
  const double inv = ss > 0.0 ? 1.0 / sqrt(ss) : __builtin_inf();
  const float f = (float)fmin(inv, 1.0 / (double)clip);
  float* g = s.g + c.start;
  const float* w = s.w ? s.w + c.start : nullptr;
  const bool use_w = s.wd != 0.f && w;
  const unsigned nv = c.cnt / 4;
  for (unsigned v = threadIdx.x; v < nv; v += CLIP_THREADS) {
    f4u gv = s.absent ? f4u{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f4u*>(g + v * 4);
    if (use_w) {
      const f4u wv = *reinterpret_cast<const f4u*>(w + v * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = clip_t(s, gv[e], wv[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = (gv[e] * clip) * f;
    *reinterpret_cast<f4u*>(g + v * 4) = gv;
  }
  for (unsigned i = nv * 4 + threadIdx.x; i < c.cnt; i += CLIP_THREADS) {
    const float t = clip_t(s, s.absent ? 0.f : g[i], use_w ? w[i] : 0.f);
    g[i] = (t * clip) * f;
  }
}

// The workspaces prepare has filled, with the table they hold: run refuses (APA_ERR_INVALID_ARG) a workspace that was
// not prepared, or (nseg, nchunks) that are not what prepare returned, on the host and without a device sync.
struct ClipPlan {
  int nseg, nchunks;
};
static std::mutex g_clip_mu;
static std::unordered_map<uintptr_t, ClipPlan>& clip_plans() {
  static std::unordered_map<uintptr_t, ClipPlan> m;
  return m;
}

}  // namespace apa

using namespace apa;

extern "C" size_t apa_clip_by_norm_workspace_bytes(int nseg, const size_t* sizes) {
  if (nseg <= 0 || !sizes) return 0;
  size_t nch = 0;
  for (int i = 0; i < nseg; ++i) nch += chunks_of(sizes[i]);
  return ClipLayout(nseg, nch).bytes;
}

extern "C" int apa_clip_by_norm_prepare(int nseg, float* const* grads, const size_t* sizes,
                                        const float* const* weights, const float* weight_decay,
                                        const unsigned char* grad_absent, void* ws, size_t ws_bytes, int* nchunks,
                                        void* stream) {
  const char* who = "apa_clip_by_norm_prepare";
  if (nseg <= 0 || !grads || !sizes || !ws || !nchunks) {
    set_error("%s: bad arguments (nseg=%d; grads, sizes, ws and nchunks are required)", who, nseg);
    return APA_ERR_INVALID_ARG;
  }
  if (reinterpret_cast<uintptr_t>(ws) & 15) {
    set_error("%s: the workspace must be 16-byte aligned", who);
    return APA_ERR_INVALID_ARG;
  }
  std::vector<ClipSeg> segs((size_t)nseg);
  std::vector<ClipChunk> chunks;
  for (int i = 0; i < nseg; ++i) {
    ClipSeg& s = segs[(size_t)i];
    const float wd = weight_decay ? weight_decay[i] : 0.f;
    const float* w = weights ? weights[i] : nullptr;
    if (sizes[i] > 0 && (!grads[i] || (reinterpret_cast<uintptr_t>(grads[i]) & 3))) {
      set_error("%s: grads[%d] is NULL or not 4-byte aligned", who, i);
      return APA_ERR_INVALID_ARG;
    }
    if (sizes[i] > 0 && wd != 0.f && (!w || (reinterpret_cast<uintptr_t>(w) & 3))) {
      set_error("%s: weights[%d] is NULL or not 4-byte aligned while weight_decay[%d] != 0", who, i, i);
      return APA_ERR_INVALID_ARG;
    }
    if (!(wd == wd)) {
      set_error("%s: weight_decay[%d] is NaN", who, i);
      return APA_ERR_INVALID_ARG;
    }
    s.g = grads[i];
    s.w = wd != 0.f ? w : nullptr;
    s.wd = wd;
    s.absent = grad_absent && grad_absent[i] ? 1 : 0;
    s.first_chunk = (int)chunks.size();
    s.nchunks = (int)chunks_of(sizes[i]);
    for (size_t o = 0; o < sizes[i]; o += CLIP_CHUNK) {
      const size_t cnt = sizes[i] - o < CLIP_CHUNK ? sizes[i] - o : CLIP_CHUNK;
      chunks.push_back(ClipChunk{i, (unsigned)cnt, (unsigned long long)o});
    }
    if (chunks.size() > (size_t)0x7fffffff) {
      set_error("%s: too many chunks", who);
      return APA_ERR_UNSUPPORTED;
    }
  }
  const ClipLayout L(nseg, chunks.size());
  if (ws_bytes < L.bytes) {
    set_error("%s: workspace %zu bytes, %zu needed (apa_clip_by_norm_workspace_bytes)", who, ws_bytes, L.bytes);
    return APA_ERR_WORKSPACE;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  // marshalled once per binding: the host vectors die on return, so the copies are waited for here (never inside a
  // captured region -- apa_clip_by_norm_run is the capturable part)
  {
    std::lock_guard<std::mutex> lk(g_clip_mu);
    clip_plans().erase(reinterpret_cast<uintptr_t>(ws));        // invalid until the new table is in place
  }
  const ClipHeader hdr{CLIP_MAGIC, nseg, (int)chunks.size(), 0};
  APA_HIP_CHECK(hipMemcpyAsync(base, &hdr, sizeof(hdr), hipMemcpyHostToDevice, st));
  APA_HIP_CHECK(hipMemcpyAsync(base + L.seg_off, segs.data(), segs.size() * sizeof(ClipSeg), hipMemcpyHostToDevice,
                               st));
  if (!chunks.empty())
    APA_HIP_CHECK(hipMemcpyAsync(base + L.chunk_off, chunks.data(), chunks.size() * sizeof(ClipChunk),
                                 hipMemcpyHostToDevice, st));
  APA_HIP_CHECK(hipStreamSynchronize(st));
  *nchunks = (int)chunks.size();
  std::lock_guard<std::mutex> lk(g_clip_mu);
  clip_plans()[reinterpret_cast<uintptr_t>(ws)] = ClipPlan{nseg, (int)chunks.size()};
  return APA_OK;
}

extern "C" int apa_clip_by_norm_run(void* ws, int nseg, int nchunks, float clip, void* stream) {
  const char* who = "apa_clip_by_norm_run";
  if (!ws || nseg <= 0 || nchunks < 0 || (reinterpret_cast<uintptr_t>(ws) & 15) || !(clip == clip)) {
    set_error("%s: bad arguments (ws=%p, nseg=%d, nchunks=%d)", who, ws, nseg, nchunks);
    return APA_ERR_INVALID_ARG;
  }
  {
    std::lock_guard<std::mutex> lk(g_clip_mu);
    auto it = clip_plans().find(reinterpret_cast<uintptr_t>(ws));
    if (it == clip_plans().end() || it->second.nseg != nseg || it->second.nchunks != nchunks) {
      set_error("%s: ws=%p holds no table of nseg=%d, nchunks=%d (call apa_clip_by_norm_prepare first and pass what "
                "it returned)", who, ws, nseg, nchunks);
      return APA_ERR_INVALID_ARG;
    }
  }
  if (clip <= 0.f || nchunks == 0) return APA_OK;    // clip <= 0: off (model_deploy.py:301 `if clip_gradients > 0`)
  const ClipLayout L(nseg, (size_t)nchunks);
  char* base = static_cast<char*>(ws);
  const ClipHeader* hdr = reinterpret_cast<const ClipHeader*>(base);
  const ClipSeg* segs = reinterpret_cast<const ClipSeg*>(base + L.seg_off);
  const ClipChunk* chunks = reinterpret_cast<const ClipChunk*>(base + L.chunk_off);
  double* partial = reinterpret_cast<double*>(base + L.part_off);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(clip_sumsq_kernel, dim3((unsigned)nchunks), dim3(CLIP_THREADS), 0, st, hdr, nseg, segs, chunks,
                     partial);
  APA_LAUNCH_CHECK("clip_sumsq_kernel");
  hipLaunchKernelGGL(clip_apply_kernel, dim3((unsigned)nchunks), dim3(CLIP_THREADS), 0, st, hdr, nseg, segs, chunks,
                     (const double*)partial, clip);
  APA_LAUNCH_CHECK("clip_apply_kernel");
  return APA_OK;
}
