// apa_clip_sample.h -- the device half of "these B videos, F frames each" (apa.h: apa_sample_clip_frames), shared by the
// two kernels that differ only in where a RANDOM_SEGMENT draw comes from: the caller's u[] (apa_clipcache.hip) or the
// counter-based rule of apa_clip_epoch.h (apa_clip_epoch.hip).  ONE copy of the frame rule and of the row copy.
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
//                                   frame_i = lo + min((int)(u * (float)(hi - lo)), hi - lo - 1), the product in fp32,
//                                   then clamped to [0, n - 1]; hi <= lo: lo clamped (n = 1, where the reference's
//                                   interval is [-1, 0)) and no draw is taken
#pragma once
#include "../../include/apa.h"
#include "apa_device.h"

namespace apa {

// draw(): the uniform draw in [0,1) of this frame; called at most once, and only where the segment has a choice
template <class Draw>
__device__ __forceinline__ int clip_frame(int n, int F, int i, int mode, Draw draw) {
  const int step = max((n - 1) / F, 1);
  if (mode == APA_CLIP_FRAMES_UNIFORM) return min(step * i, n - 1);
  const int lo = min(step * i, n - 2), hi = min(step * (i + 1), n - 1);
  int f = lo;
  if (hi > lo) f = lo + min((int)(draw() * (float)(hi - lo)), hi - lo - 1);
  return min(max(f, 0), n - 1);
}

// One block (256 threads) per clip b = blockIdx.x: thread i, i + 256, ... takes frame i; thread 0 clamps and counts a
// video id outside [0,V) (an ordinary vector atomic, as m1_gather_note does) and copies the int64 label; all threads
// copy the multi-hot row -- 16-byte vectors over the part of the row where source and destination share their alignment
// mod 16, scalars in front of and behind it, scalars alone where they do not.  A frame count below 1 is read as 1:
// nothing outside the video's own slots [first, first + max(n,1)) is ever named.
// draw(j): the draw of flat frame j = b * F + i.
template <class Draw>
__device__ __forceinline__ void sample_clip_block(
    const int32_t* __restrict__ video_first, const int32_t* __restrict__ video_frames,
    const int64_t* __restrict__ video_labels, const float* __restrict__ video_targets,
    const int32_t* __restrict__ videos, int32_t* __restrict__ index, int64_t* __restrict__ labels,
    float* __restrict__ targets, int32_t* __restrict__ status, int V, int F, int K, int mode, Draw draw) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int raw = videos[b], v = min(max(raw, 0), V - 1);
  const int first = video_first[v], n = max(video_frames[v], 1);
  const size_t row = (size_t)b * F;
  for (int i = t; i < F; i += 256) {
    const size_t j = row + i;
    index[j] = first + clip_frame(n, F, i, mode, [&] { return draw(j); });
  }
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
