// apa_clipcache.hip -- "these B videos, F frames each" -> the int32 index the gathered kernels read (apa.h:
// apa_feature_cache.index), plus the clips' labels or multi-hot rows, in ONE launch: an epoch over a resident frame
// cache needs no host work and no synchronisation.
//
// The frame rule restates _get_frame_sublist (reference: src/datasets/image_read_utils.py:12-44) as
// src/datasets/video_data_utils.py:79-81 calls it: num_consec_frames = 1, start_frame = 0, duration = n (the video's
// frame count), num_samples = F.
//   step = max((n - 1) / F, 1)
// The reference writes `tf.cast((duration - 1) / num_samples, 'int32')` on int32 tensors; under TF 1.1 / Python 2 the
// `/` of two int32 tensors is floor division.  That is OUR READING of the reference -- TensorFlow is not available to
// confirm it -- and n - 1 >= 0, so C's truncating division is that floor.
//   APA_CLIP_FRAMES_UNIFORM         frame_i = min(step * i, n - 1)                                    (:40)
//   APA_CLIP_FRAMES_RANDOM_SEGMENT  lo = min(step * i, n - 2), hi = min(step * (i + 1), n - 1)          (:33-38)
//                                   frame_i = lo + min((int)(u[b*F+i] * (float)(hi - lo)), hi - lo - 1), the product
//                                   in fp32, then clamped to [0, n - 1]; hi <= lo: lo clamped (n = 1, where the
//                                   reference's interval is [-1, 0))
// u: the CALLER's uniform draws in [0,1) (the convention of apa_pose_sampled_loss_fwd_bwd's `uniform`); the stream of
// tf.random_uniform is not reproduced.  Under UNIFORM u is ignored (it may be NULL or not).
//
// One block per clip: thread i, i + 256, ... takes frame i; thread 0 clamps and counts a video id outside [0,V) (an
// ordinary vector atomic, as m1_gather_note does) and copies the int64 label; all threads copy the multi-hot row --
// 16-byte vectors over the part of the row where source and destination share their alignment mod 16, scalars in
// front of and behind it, scalars alone where they do not.  A frame count below 1 is read as 1: nothing outside the
// video's own slots [first, first + max(n,1)) is ever named.  No workspace, no LDS, integer and one fp32 product per
// frame: identical calls give identical bits.
#include "apa_device.h"
#include "apa_internal.h"

namespace apa {

__device__ __forceinline__ int clip_frame(int n, int F, int i, int mode, const float* __restrict__ u, size_t ui) {
  const int step = max((n - 1) / F, 1);
  if (mode == APA_CLIP_FRAMES_UNIFORM) return min(step * i, n - 1);
  const int lo = min(step * i, n - 2), hi = min(step * (i + 1), n - 1);
  int f = lo;
  if (hi > lo) f = lo + min((int)(u[ui] * (float)(hi - lo)), hi - lo - 1);
  return min(max(f, 0), n - 1);
}

__global__ __launch_bounds__(256) void sample_clip_frames_kernel(
    const int32_t* __restrict__ video_first, const int32_t* __restrict__ video_frames,
    const int64_t* __restrict__ video_labels, const float* __restrict__ video_targets,
    const int32_t* __restrict__ videos, const float* __restrict__ u, int32_t* __restrict__ index,
    int64_t* __restrict__ labels, float* __restrict__ targets, int32_t* __restrict__ status, int V, int F, int K,
    int mode) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int raw = videos[b], v = min(max(raw, 0), V - 1);
  const int first = video_first[v], n = max(video_frames[v], 1);
  const size_t row = (size_t)b * F;
  for (int i = t; i < F; i += 256) index[row + i] = first + clip_frame(n, F, i, mode, u, row + i);
  if (t == 0) {
    if (status && raw != v) atomicAdd(status, 1);
    if (video_labels) labels[b] = video_labels[v];
  }
  if (!video_targets) return;
  const float* __restrict__ src = video_targets + (size_t)v * K;
  float* __restrict__ dst = targets + (size_t)b * K;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(src), da = reinterpret_cast<uintptr_t>(dst);
  int head = K;   // scalars in front of the vectors; all K where the two rows do not share their alignment
  if (((sa ^ da) & 15) == 0) head = min((int)(((16 - (da & 15)) & 15) >> 2), K);
  const int nvec = (K - head) >> 2, tail = head + 4 * nvec;
  for (int k = t; k < head; k += 256) dst[k] = src[k];
  const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + head);
  float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + head);
  for (int k = t; k < nvec; k += 256) d4[k] = s4[k];
  for (int k = tail + t; k < K; k += 256) dst[k] = src[k];
}

}  // namespace apa

using namespace apa;

extern "C" int apa_sample_clip_frames(const int32_t* video_first, const int32_t* video_frames,
                                      const int64_t* video_labels, const float* video_targets, const int32_t* videos,
                                      const float* u, int32_t* index, int64_t* labels, float* targets, int32_t* status,
                                      int V, int B, int frames, int K, int mode, void* stream) {
  const char* fn = "apa_sample_clip_frames";
  if (!video_first || !video_frames || !videos || !index) {
    set_error("%s: null video_first / video_frames / videos / index pointer", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((video_labels && !labels) || (video_targets && !targets)) {
    set_error("%s: video_labels needs labels and video_targets needs targets", fn);
    return APA_ERR_INVALID_ARG;
  }
  if (V <= 0 || B <= 0 || frames <= 0 || (video_targets && K <= 0)) {
    set_error("%s: non-positive size V=%d B=%d frames=%d K=%d", fn, V, B, frames, K);
    return APA_ERR_INVALID_ARG;
  }
  if (mode != APA_CLIP_FRAMES_UNIFORM && mode != APA_CLIP_FRAMES_RANDOM_SEGMENT) {
    set_error("%s: unknown mode %d", fn, mode);
    return APA_ERR_INVALID_ARG;
  }
  if (mode == APA_CLIP_FRAMES_RANDOM_SEGMENT && !u) {
    set_error("%s: APA_CLIP_FRAMES_RANDOM_SEGMENT needs the uniform draws u [B*frames]", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((long long)B * frames > 0x7fffffffLL) {
    set_error("%s: B * frames = %lld is past 2^31 - 1 (the index is an int32 batch)", fn, (long long)B * frames);
    return APA_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(sample_clip_frames_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), video_first,
                     video_frames, video_labels, video_targets, videos, u, index, labels, targets, status, V, frames, K,
                     mode);
  APA_LAUNCH_CHECK("sample_clip_frames_kernel");
  return APA_OK;
}
