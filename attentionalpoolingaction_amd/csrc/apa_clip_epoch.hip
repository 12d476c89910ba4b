// apa_clip_epoch.hip -- apa_sample_clip_frames with its RANDOM_SEGMENT draws made on the device (apa_clip_epoch.h:
// apa_sample_clip_frames_keyed), so that a C loop over the steps of an epoch of clips needs no torch.rand in front of
// every step.  The block's work and the frame rule are apa_clip_sample.h's, the ones apa_sample_clip_frames runs; only
// the draw differs:
//   h = splitmix64(splitmix64(seed, epoch), step) -- rng_key's derivation (apa_internal.h), taken twice on the host;
//       k0 = its low word, k1 = its high word, passed by value
//   u[j] = (float)(rng_hash(j, k0, k1) >> 8) * 2^-24, j = b * F + i: a 24-bit integer scaled by a power of two, exact in
//       fp32 and below 1 (rng_hash: the dropout mask's two-round 24-bit multiply-xorshift mix, apa_device.h)
// Counter-based: every frame computes its own draw, and only where its segment has a choice.  No workspace, no LDS, no
// atomics but the integer status count: identical calls give identical bits.  The epoch calls that loop over this
// launch, the *_cached_clips step and the update are apa_epoch.hip's (one driver with the flat epoch calls).
#include "../../include/apa_clip_epoch.h"
#include "apa_clip_sample.h"
#include "apa_internal.h"

namespace apa {

__global__ __launch_bounds__(256) void sample_clip_frames_keyed_kernel(
    const int32_t* __restrict__ video_first, const int32_t* __restrict__ video_frames,
    const int64_t* __restrict__ video_labels, const float* __restrict__ video_targets,
    const int32_t* __restrict__ videos, int32_t* __restrict__ index, int64_t* __restrict__ labels,
    float* __restrict__ targets, int32_t* __restrict__ status, int V, int F, int K, int mode, uint32_t k0,
    uint32_t k1) {
  sample_clip_block(video_first, video_frames, video_labels, video_targets, videos, index, labels, targets, status, V, F,
                    K, mode, [k0, k1](size_t j) { return (float)(rng_hash((uint32_t)j, k0, k1) >> 8) * 0x1p-24f; });
}

}  // namespace apa

using namespace apa;

extern "C" int apa_sample_clip_frames_keyed(const int32_t* video_first, const int32_t* video_frames,
                                            const int64_t* video_labels, const float* video_targets,
                                            const int32_t* videos, int32_t* index, int64_t* labels, float* targets,
                                            int32_t* status, int V, int B, int frames, int K, int mode, uint64_t seed,
                                            uint64_t epoch, uint64_t step, void* stream) {
  const int rc = sample_clip_check("apa_sample_clip_frames_keyed", video_first, video_frames, video_labels,
                                   video_targets, videos, index, labels, targets, V, B, frames, K, mode, false);
  if (rc != APA_OK) return rc;
  uint32_t h0, h1, k0, k1;
  rng_key(seed, epoch, &h0, &h1);
  rng_key(((uint64_t)h1 << 32) | h0, step, &k0, &k1);
  hipLaunchKernelGGL(sample_clip_frames_keyed_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     video_first, video_frames, video_labels, video_targets, videos, index, labels, targets, status, V,
                     frames, K, mode, k0, k1);
  APA_LAUNCH_CHECK("sample_clip_frames_keyed_kernel");
  return APA_OK;
}
