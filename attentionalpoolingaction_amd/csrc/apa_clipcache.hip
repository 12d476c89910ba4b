// apa_clipcache.hip -- "these B videos, F frames each" -> the int32 index the gathered kernels read (apa.h:
// apa_feature_cache.index), plus the clips' labels or multi-hot rows, in ONE launch: an epoch over a resident frame
// cache needs no host work and no synchronisation.
//
// The frame rule (_get_frame_sublist) and the block's work -- one block per clip -- are apa_clip_sample.h's, shared with
// the keyed sampler (apa_clip_epoch.hip).
// u: the CALLER's uniform draws in [0,1) (the convention of apa_pose_sampled_loss_fwd_bwd's `uniform`); the stream of
// tf.random_uniform is not reproduced.  Under UNIFORM u is ignored (it may be NULL or not).
// No workspace, no LDS, integer and one fp32 product per frame: identical calls give identical bits.
#include "apa_clip_sample.h"
#include "apa_internal.h"

namespace apa {

__global__ __launch_bounds__(256) void sample_clip_frames_kernel(
    const int32_t* __restrict__ video_first, const int32_t* __restrict__ video_frames,
    const int64_t* __restrict__ video_labels, const float* __restrict__ video_targets,
    const int32_t* __restrict__ videos, const float* __restrict__ u, int32_t* __restrict__ index,
    int64_t* __restrict__ labels, float* __restrict__ targets, int32_t* __restrict__ status, int V, int F, int K,
    int mode) {
  sample_clip_block(video_first, video_frames, video_labels, video_targets, videos, index, labels, targets, status, V, F,
                    K, mode, [u](size_t j) { return u[j]; });
}

}  // namespace apa

using namespace apa;

// What both samplers refuse, before anything is queued (apa_internal.h).  u_missing: the caller's draws are taken and
// were not given (the keyed sampler makes its own: false).
int apa::sample_clip_check(const char* fn, const void* video_first, const void* video_frames, const void* video_labels,
                           const void* video_targets, const void* videos, const void* index, const void* labels,
                           const void* targets, int V, int B, int frames, int K, int mode, bool u_missing) {
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
  if (mode == APA_CLIP_FRAMES_RANDOM_SEGMENT && u_missing) {
    set_error("%s: APA_CLIP_FRAMES_RANDOM_SEGMENT needs the uniform draws u [B*frames]", fn);
    return APA_ERR_INVALID_ARG;
  }
  if ((long long)B * frames > 0x7fffffffLL) {
    set_error("%s: B * frames = %lld is past 2^31 - 1 (the index is an int32 batch)", fn, (long long)B * frames);
    return APA_ERR_INVALID_ARG;
  }
  return APA_OK;
}

extern "C" int apa_sample_clip_frames(const int32_t* video_first, const int32_t* video_frames,
                                      const int64_t* video_labels, const float* video_targets, const int32_t* videos,
                                      const float* u, int32_t* index, int64_t* labels, float* targets, int32_t* status,
                                      int V, int B, int frames, int K, int mode, void* stream) {
  const int rc = sample_clip_check("apa_sample_clip_frames", video_first, video_frames, video_labels, video_targets,
                                   videos, index, labels, targets, V, B, frames, K, mode, u == nullptr);
  if (rc != APA_OK) return rc;
  hipLaunchKernelGGL(sample_clip_frames_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), video_first,
                     video_frames, video_labels, video_targets, videos, u, index, labels, targets, status, V, frames, K,
                     mode);
  APA_LAUNCH_CHECK("sample_clip_frames_kernel");
  return APA_OK;
}
