"""The frame rule of apa_sample_clip_frames (include/apa.h) restated in numpy, in int32 / float32: what the device
sampler must give bit for bit.  The rule is _get_frame_sublist of the reference (src/datasets/image_read_utils.py:12-44)
called with num_consec_frames = 1 and start_frame = 0, its int32 `/` read as floor division."""
import numpy as np

UNIFORM, RANDOM_SEGMENT = 0, 1
I32, F32 = np.int32, np.float32


def step_of(n, F):
    return max(I32(I32(n - 1) // I32(F)), I32(1))


def frames_uniform(n, F):
    """frame i = min(step * i, n - 1), int32 [F]"""
    step = step_of(n, F)
    i = np.arange(F, dtype=I32)
    return np.minimum(step * i, I32(n - 1)).astype(I32)


def frames_random(n, F, u):
    """u float32 [F] in [0,1): lo + min((int)(u * (float)(hi - lo)), hi - lo - 1), clamped to [0, n - 1]; hi <= lo: lo
    clamped.  int32 [F]"""
    step = step_of(n, F)
    i = np.arange(F, dtype=I32)
    lo = np.minimum(step * i, I32(n - 2)).astype(I32)
    hi = np.minimum(step * (i + I32(1)), I32(n - 1)).astype(I32)
    span = (hi - lo).astype(I32)
    prod = np.asarray(u, dtype=F32) * span.astype(F32)          # one fp32 product, then truncation
    draw = np.minimum(prod.astype(I32), span - I32(1))
    f = np.where(hi > lo, lo + draw, lo)
    return np.clip(f, 0, n - 1).astype(I32)


def segments(n, F):
    """the half-open interval [lo, hi) each random frame is drawn from (hi <= lo: the single frame lo clamped)"""
    step = step_of(n, F)
    i = np.arange(F, dtype=I32)
    return np.minimum(step * i, I32(n - 2)).astype(I32), np.minimum(step * (i + I32(1)), I32(n - 1)).astype(I32)


def sample(video_first, video_frames, videos, F, mode, u=None, video_labels=None, video_targets=None):
    """-> (index int32 [B*F], labels int64 [B] or None, targets float32 [B,K] or None, clamped ids)"""
    V, B = len(video_first), len(videos)
    index = np.zeros(B * F, dtype=I32)
    labels = None if video_labels is None else np.zeros(B, dtype=np.int64)
    targets = None if video_targets is None else np.zeros((B, video_targets.shape[1]), dtype=F32)
    bad = 0
    for b, raw in enumerate(videos):
        v = min(max(int(raw), 0), V - 1)
        bad += int(v != int(raw))
        n = max(int(video_frames[v]), 1)
        fr = frames_uniform(n, F) if mode == UNIFORM else frames_random(n, F, np.asarray(u, dtype=F32)[b * F:(b + 1) * F])
        index[b * F:(b + 1) * F] = I32(video_first[v]) + fr
        if labels is not None:
            labels[b] = video_labels[v]
        if targets is not None:
            targets[b] = video_targets[v]
    return index, labels, targets, bad
