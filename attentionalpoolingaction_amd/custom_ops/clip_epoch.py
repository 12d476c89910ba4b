"""A whole clip or multi-label epoch over a resident frame cache as ONE host call (include/apa_clip_epoch.h).

The counterpart of custom_ops_factory's HeadTrainEpoch / HeadEvalEpoch for the datasets those leave out -- clips
(HMDB-51) and the sigmoid losses (HICO, Charades) -- and the keyed clip sampler that makes them possible: the
random-segment draws come from a counter-based rule on (seed, epoch, step) instead of a torch.rand launch per step.

The entry points live in the same libapa_hip.so as everything else; they are declared in a header of their own and
bound here, on first use, with a signature table of their own: `custom_ops_factory._SIGNATURES` stays the mirror of
include/apa.h.  There is NO CPU fallback (clip_draws_rule_cpu is the host RESTATEMENT of the draws, for tests and for a
loop that wants to reproduce them)."""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_size_t, c_uint, c_uint64, c_void_p
from typing import Optional

import numpy as np
import torch

from . import custom_ops_factory as cof
from .custom_ops_factory import ApaError

# every symbol include/apa_clip_epoch.h declares: name -> (restype, argtypes)
_STEP_TAIL = [c_size_t] + [c_int] * 6 + [c_uint]        # ws_bytes, N, P, C, Ca, K, M, flags
_SIGNATURES = {
    # tables (4), videos, index, labels, targets, status; V, B, frames, K, mode; seed, epoch, step; stream
    'apa_sample_clip_frames_keyed': (c_int, [c_void_p] * 9 + [c_int] * 5 + [c_uint64] * 3 + [c_void_p]),
    # ep, opt, ce, cache, ml, clip, hooks; X .. bt, labels; loss_wt, grad_scale; logits .. dbt, ws; ...; stream
    'apa_attn_head_train_epoch_cached_clips': (c_int, [c_void_p] * 7 + [c_void_p] * 7 + [c_float, c_float] +
                                               [c_void_p] * 13 + _STEP_TAIL +
                                               [c_float, c_uint64, c_uint64, c_int, c_void_p]),
    # ep, ce, cache, clip, kind; X .. bt, labels; logits .. pred, ws; ...; dtype, stream
    'apa_attn_head_eval_epoch_cached_clips': (c_int, [c_void_p] * 4 + [c_int] + [c_void_p] * 7 + [c_void_p] * 8 +
                                              _STEP_TAIL + [c_int, c_void_p]),
}

_lib = None


def exported_symbols():
    """Names include/apa_clip_epoch.h declares (the CPU-side ABI test compares the three)."""
    return sorted(_SIGNATURES)


def load_library() -> ctypes.CDLL:
    """custom_ops_factory's libapa_hip.so with this module's entry points bound as well (once)."""
    global _lib
    if _lib is None:
        lib = cof.load_library()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError here == missing export
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class ApaClipEpoch(ctypes.Structure):
    """`apa_clip_epoch` of include/apa_clip_epoch.h (field order is the ABI)."""
    _fields_ = [('video_first', c_void_p), ('video_frames', c_void_p), ('video_labels', c_void_p),
                ('video_targets', c_void_p), ('V', c_int), ('mode', c_int), ('seed', c_uint64), ('epoch', c_uint64),
                ('index', c_void_p), ('labels', c_void_p), ('targets', c_void_p)]


_M64 = (1 << 64) - 1


def _key(who: str, seed, epoch, step=0):
    """(seed, epoch, step) as the uint64 values the C ABI takes (python integers wrap mod 2^64, as cof.epoch_order's)"""
    try:
        return int(seed) & _M64, int(epoch) & _M64, int(step) & _M64
    except (TypeError, ValueError):
        raise ApaError('{}: seed, epoch and step are integers'.format(who))


def clip_draws_rule_cpu(B: int, frames: int, seed: int, epoch: int, step: int) -> torch.Tensor:
    """The draws apa_sample_clip_frames_keyed takes, restated on the host (include/apa_clip_epoch.h), bit for bit:
    float32 [B*frames] on the CPU, u[j] = (hash(j, k0, k1) >> 8) * 2^-24 with (k0, k1) the low and high words of
    mix64(mix64(seed, epoch), step) -- `apa_sample_clip_frames` fed these gives the keyed sampler's index."""
    n = int(B) * int(frames)
    if int(B) < 1 or int(frames) < 1 or n > 2 ** 31 - 1:
        raise ApaError('clip_draws_rule_cpu: B >= 1, frames >= 1 and B * frames <= 2^31 - 1 expected')
    seed, epoch, step = _key('clip_draws_rule_cpu', seed, epoch, step)
    h = cof._mix64(cof._mix64(seed, epoch), step)
    x = cof._epoch_hash(np.arange(n, dtype=np.uint64), h & 0xFFFFFFFF, h >> 32)
    return torch.from_numpy((x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24))


def _video_cache(who: str, cache) -> None:
    if not isinstance(cache, cof.FeatureCache):
        raise ApaError('{}: a FeatureCache expected'.format(who))
    if cache.video_first is None:
        raise ApaError('{}: set_videos first'.format(who))
    if not cache.features.is_cuda:
        raise ApaError('{}: the cache must live in GPU memory; the HIP path has no CPU fallback'.format(who))


def _mode(who: str, mode: str) -> int:
    if mode not in cof.CLIP_FRAME_MODES:
        raise ApaError('{}: mode must be one of {} (got {!r})'.format(who, tuple(cof.CLIP_FRAME_MODES), mode))
    return cof.CLIP_FRAME_MODES[mode]


def sample_clips_keyed(cache, videos, frames: int, mode: str = 'random-segment', seed: int = 0, epoch: int = 0,
                       step: int = 0, out: Optional[cof.CachedClips] = None) -> cof.CachedClips:
    """`FeatureCache.sample_clips` with the random-segment draws made on the device from (seed, epoch, step)
    (apa_sample_clip_frames_keyed): ONE launch, no torch.rand in front of it, capturable -- (seed, epoch, step) travel by
    value and are frozen by a capture.  Equal, bit for bit, to `cache.sample_clips(videos, frames, mode,
    u=clip_draws_rule_cpu(B, frames, seed, epoch, step))`.  `out`: a CachedClips of the same B and `frames`, rewritten
    in place."""
    who = 'sample_clips_keyed'
    code = _mode(who, mode)
    _video_cache(who, cache)
    F = int(frames)
    if F < 1:
        raise ApaError('{}: frames >= 1 expected'.format(who))
    vid = cof._index_tensor(who, videos, cache.device)
    B = int(vid.numel())
    if B * F > 2 ** 31 - 1:
        raise ApaError('{}: B * frames past 2^31 - 1'.format(who))
    if out is not None and (not isinstance(out, cof.CachedClips) or out.cache is not cache or out.frames != F or
                            out.index.numel() != B * F):
        raise ApaError('{}: out must be a CachedClips of this cache with the same B and frames'.format(who))
    seed, epoch, step = _key(who, seed, epoch, step)
    clips = out if out is not None else cof.CachedClips(cache, B, F)
    K = 0 if cache.video_targets is None else int(cache.video_targets.shape[1])
    dp = cof._dev_ptr
    rc = load_library().apa_sample_clip_frames_keyed(
        cache.video_first.data_ptr(), cache.video_frames.data_ptr(), dp(cache.video_labels, 'labels'),
        dp(cache.video_targets, 'targets'), vid.data_ptr(), clips.index.data_ptr(), dp(clips.labels, 'labels'),
        dp(clips.targets, 'targets'), cache.status.data_ptr(), cache.V, B, F, K, code, seed, epoch, step,
        cof._stream_ptr())
    cof._check(rc, 'apa_sample_clip_frames_keyed')
    clips.videos = vid
    return clips


def _clip_shape(who: str, cache, B, frames, Wa, Wt, multi_label: bool):
    """(B, F, N, P, C, K, dtype code) of an epoch of B videos x F frames per step, validated against the cache"""
    _video_cache(who, cache)
    P, C, dt = cof._epoch_cache(who, cache)
    B, F = int(B), int(frames)
    if B < 1 or F < 1:
        raise ApaError('{}: B >= 1 and frames >= 1 expected'.format(who))
    if Wa.shape[1] != 1:
        raise ApaError('{}: a clip epoch feeds the class-agnostic head (M == 1): per-class maps are not served (its '
                       'update rewrites no weight images)'.format(who))
    K = int(Wt.shape[1])
    if cache.video_targets is not None and int(cache.video_targets.shape[1]) != K:
        raise ApaError('{}: the cache\'s video targets have {} classes, the head {}'.format(
            who, int(cache.video_targets.shape[1]), K))
    if multi_label and cache.video_targets is None:
        raise ApaError('{}: a sigmoid loss / sigmoid scores need a cache with video targets (set_videos(targets=))'
                       .format(who))
    return B, F, B * F, P, C, K, dt


def _bind_temporal(who: str, clip, temporal, K: int) -> None:
    w, b = temporal
    if w.numel() != K or b.numel() != 1:
        raise ApaError('{}: temporal = (w [K], b [1]) expected'.format(who))
    clip.w, clip.b = cof._dev_ptr(w, 'temporal w', torch.float32), cof._dev_ptr(b, 'temporal b', torch.float32)


class ClipTrainEpoch:
    """apa_attn_head_train_epoch_cached_clips bound to caller-owned buffers, everything marshalled ONCE: a whole epoch
    of frozen-feature training on a resident FRAME cache (`FeatureCache.set_videos`) -- `steps` times (the keyed clip
    sampler on the next `B` video ids of `order`, the gathered one-call clip / multi-label step on the frames it names,
    the fused momentum-SGD update with that step's learning rate) -- as ONE foreign call, bit-identical in every
    output, weight and accumulator to the loop of `sample_clips_keyed(..., step=s, out=clips)`,
    `HeadTrainStep.rebind(offset=) + run()` on those clips and `BoundMomentumSGD.run(lr[s], ...)`.

    `frames`: F frames per video (1: one-frame videos, the flat multi-label datasets); `temporal = (w [K], b [1])`: the
    TemporalAttention conv (None: plain mean over the frames) with `temporal_grads = (dw [K], db [1])`, views of
    `grad_flat` like `grads = (dWa, dba, dWt, dbt)`; `action_loss`: 'softmax-xentropy' (the cache's video labels),
    'multi-label' | 'multi-label-2' (its video targets; `pos_weight` for the former); `mode`: the sampler's, 'uniform' |
    'random-segment'.  `weights` / `weight_decay` / `grad_flat` / `acc_flat`: BoundMomentumSGD's arguments.  `offset`:
    the dropout offset of the first step (step s uses offset + s), or a 1-element int64 CUDA tensor (the device
    counter).  `steps`: the most steps one `run` may take.
    Outputs: `loss` [steps, 1+B] (the epoch's log), the LAST step's `logits` [B*F,K], `att`, `zsave`, `abar`, `G`,
    `pooled` [B,K] and `tatt` [B*F] (None without them), and the sampler's scratch `index`, `labels`, `targets` (the last
    step's batch); `outputs={name: tensor}` binds caller-owned buffers in place of loss / logits / att / zsave / abar /
    G."""

    def __init__(self, cache, B, frames, Wa, ba, Wt, bt, grads, weights, weight_decay, grad_flat, acc_flat, *, steps,
                 temporal=None, temporal_grads=None, action_loss='softmax-xentropy', pos_weight=10.0,
                 mode='random-segment', momentum=0.9, update_grad_scale=1.0, flags=0, keep_prob=1.0, seed=0, offset=0,
                 loss_wt=1.0, grad_scale=1.0, workspace=None, hooks=None, outputs=None):
        who = 'ClipTrainEpoch'
        self.lib = load_library()
        if action_loss not in cof.STEP_ACTION_LOSSES:
            raise ApaError('{}: action_loss must be one of {} (got {!r})'.format(who, cof.STEP_ACTION_LOSSES,
                                                                                 action_loss))
        multi = action_loss != 'softmax-xentropy'
        B, F, N, P, C, K, dt = _clip_shape(who, cache, B, frames, Wa, Wt, multi)
        steps = int(steps)
        if steps < 1:
            raise ApaError('{}: steps >= 1 expected'.format(who))
        if not multi and cache.video_labels is None:
            raise ApaError('{}: the softmax cross-entropy needs a cache with video labels (set_videos(labels=))'
                           .format(who))
        dev, f32 = cache.device, torch.float32
        self.cache, self.B, self.frames, self.N, self.steps, self.hooks = cache, B, F, N, steps, hooks
        cof._epoch_outputs(who, self, outputs, (('logits', (N, K), f32), ('att', (N, P, 1), f32),
                                                ('zsave', (N, C), f32), ('abar', (N,), f32),
                                                ('loss', (steps, 1 + B), f32), ('G', (N, K), f32)), dev)
        flags |= cof.APA_FLAG_FROZEN_INPUT
        clips = F != 1 or temporal is not None
        self._clip, self.pooled, self.tatt, keep = None, None, None, ()
        if clips:       # the pooling workspace followed by the clip loss's scratch
            self._clip, self.pooled, self.tatt, keep = cof._bind_clip_pool(who, N, K, F, temporal, temporal_grads, dev)
            need = int(self.lib.apa_clip_step_workspace_bytes(N, F, P, C, C, K, 1, flags))
        else:
            need = int(self.lib.apa_attn_pool_workspace_bytes(N, P, C, C, K, 1, flags))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.workspace = workspace
        # the sampler's scratch: what step s reads
        self.index = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.labels = None if cache.video_labels is None else torch.zeros((B,), dtype=torch.int64, device=dev)
        self.targets = None if cache.video_targets is None else torch.zeros((B, K), dtype=f32, device=dev)
        self._ml = None
        if multi:       # (its labels pointer is not read: the sampled targets take its place)
            self._ml = cof.ApaMultilabel()
            self._ml.kind, self._ml.pos_weight = cof.ACTION_LOSS_KINDS[action_loss], float(pos_weight)
            self._ml.labels = self.targets.data_ptr()
        dp = cof._dev_ptr
        self._ce = ApaClipEpoch(cache.video_first.data_ptr(), cache.video_frames.data_ptr(),
                                dp(cache.video_labels, 'labels'), dp(cache.video_targets, 'targets'), cache.V,
                                _mode(who, mode), 0, 0, self.index.data_ptr(), dp(self.labels, 'labels'),
                                dp(self.targets, 'targets'))
        dWa, dba, dWt, dbt = grads
        a = self._opt_args = cof._OptimizerArgs(weights, weight_decay,
                                                (('grad_flat', grad_flat), ('acc_flat', acc_flat)), who=who)
        self._lr = (c_float * steps)()
        nseg, wptr, sizes, wd, gptr, aptr = a.head
        self._sgd = cof.ApaEpochSgd(nseg, ctypes.addressof(wptr), ctypes.addressof(sizes), ctypes.addressof(wd), gptr,
                                    aptr, ctypes.addressof(self._lr), float(momentum), float(update_grad_scale))
        self._ep = cof.ApaEpoch(None, 0)
        self._fc = cof.ApaFeatureCache(None, cache.T, 0, cache.status.data_ptr())
        self._keep = (Wa, ba, Wt, bt, grads, offset, seed, keep, None)
        seed, off, flags = cof._rng_key(seed, offset, flags)     # the pointers below stay valid
        self._off_dev = isinstance(offset, torch.Tensor)
        X = cache.features.data_ptr()
        self._args = [
            X, X, dp(Wa, 'Wa', f32), dp(ba, 'ba', f32), dp(Wt, 'Wt', f32), dp(bt, 'bt', f32), None,
            float(loss_wt), float(grad_scale),
            self.logits.data_ptr(), self.att.data_ptr(), self.zsave.data_ptr(), self.abar.data_ptr(),
            self.loss.data_ptr(), self.G.data_ptr(), None, None, dp(dWa, 'dWa', f32), dp(dba, 'dba', f32),
            dp(dWt, 'dWt', f32), dp(dbt, 'dbt', f32), workspace.data_ptr(), workspace.numel(), N, P, C, C, K, 1,
            flags, float(keep_prob), int(seed), off, dt]
        self._pre = (ctypes.addressof(self._ep), ctypes.addressof(self._sgd), ctypes.addressof(self._ce),
                     ctypes.addressof(self._fc), None if self._ml is None else ctypes.addressof(self._ml),
                     None if self._clip is None else ctypes.addressof(self._clip))

    def run(self, order, lr, seed: int = 0, epoch: int = 0, offset=None, stream: Optional[int] = None,
            hooks=None) -> torch.Tensor:
        """Enqueue the epoch over `order` (int32 VIDEO ids on the cache's device, a whole number of batches of B:
        `cof.epoch_order(cache.V, seed, epoch, device)` or its first steps * B entries) with `lr[s]` the learning rate
        of update s (a sequence of order.numel() / B floats, or one float for all) and the sampler keyed by
        (`seed`, `epoch`, s).  `offset` (int): another dropout offset for the first step.  Returns the loss log
        [steps, 1+B], a view of `self.loss` on the device -- nothing synchronises.
        Under a captured hipGraph: `lr[s]`, (`seed`, `epoch`, s), an int `offset` and the address of `order` are read
        HERE and are frozen in the graph -- every replay draws the same frames for the same videos and trains with the
        captured rates; the contents of `order`, the device dropout counter, weights and accumulators are re-read
        from HBM."""
        who = 'ClipTrainEpoch.run'
        order = cof._epoch_order_arg(who, order, self.cache)
        count = int(order.numel())
        steps = count // self.B
        if steps < 1 or count % self.B or steps > self.steps:
            raise ApaError('{}: {} video ids are not 1..{} whole batches of {}'.format(who, count, self.steps, self.B))
        lrs = [float(lr)] * steps if isinstance(lr, (int, float)) else [float(v) for v in lr]
        if len(lrs) != steps:
            raise ApaError('{}: one learning rate per step expected ({} for {} steps)'.format(who, len(lrs), steps))
        self._lr[:steps] = lrs
        self._ce.seed, self._ce.epoch, _ = _key(who, seed, epoch)
        if offset is not None:
            if self._off_dev:
                raise ApaError('{}: the epoch was bound to a device-side dropout counter'.format(who))
            self._args[-2] = int(offset)
        self._keep = self._keep[:8] + (order,)
        self._ep.order, self._ep.count = order.data_ptr(), count
        h = self.hooks if hooks is None else hooks
        rc = self.lib.apa_attn_head_train_epoch_cached_clips(*self._pre, cof._hooks_ptr(h), *self._args,
                                                             cof._stream_ptr() if stream is None else stream)
        if rc != 0:
            cof._check(rc, 'apa_attn_head_train_epoch_cached_clips')
        return self.loss[:steps]


class ClipEvalEpoch:
    """apa_attn_head_eval_epoch_cached_clips bound once: a validation pass over `count` videos of a resident frame
    cache in batches of `B` videos x `frames` uniformly spaced frames (the reference's test protocol; the last batch
    shorter) as ONE foreign call, bit-identical to the loop of `cache.sample_clips(order[s*B:(s+1)*B], frames,
    'uniform')` + HeadEvalStep on those clips.  `scores`: 'softmax' | 'sigmoid'; `temporal = (w [K], b [1])`: the
    TemporalAttention conv; `capacity`: the most videos one `run` may visit; `want_loss` (softmax scores, a cache with
    video labels): the per-step losses [ceil(capacity / B), 1+B].
    Outputs, per VIDEO (rows [0, count) are written, nothing behind them): `probs`, `pooled` [capacity,K], `pred`
    [capacity], and the truth the sampler hands out, `labels` [capacity] / `targets` [capacity,K] (None where the cache
    has none); per frame, the LAST step's: `logits` [B*F,K], `att`, `zsave`, `abar`, `tatt`.  One-frame videos without
    temporal attention have no pooling: `logits` is then [capacity,K] per video and `pooled` is `logits`.
    `run(..., probs=, labels=, targets=)` writes into the caller's rows instead (eval_utils.DeviceEvaluation.reserve)."""

    def __init__(self, cache, B, frames, Wa, ba, Wt, bt, *, capacity, temporal=None, flags=0, scores='softmax',
                 want_loss=False, workspace=None, outputs=None):
        who = 'ClipEvalEpoch'
        self.lib = load_library()
        if scores not in ('softmax', 'sigmoid'):
            raise ApaError('{}: scores must be \'softmax\' or \'sigmoid\' (got {!r})'.format(who, scores))
        B, F, N, P, C, K, dt = _clip_shape(who, cache, B, frames, Wa, Wt, False)
        capacity = int(capacity)
        if capacity < 1:
            raise ApaError('{}: capacity >= 1 expected'.format(who))
        if want_loss and (scores != 'softmax' or cache.video_labels is None):
            raise ApaError('{}: want_loss needs softmax scores and a cache with video labels'.format(who))
        dev, f32 = cache.device, torch.float32
        self.cache, self.B, self.frames, self.N, self.capacity, self.K = cache, B, F, N, capacity, K
        flags &= ~cof.APA_FLAG_TRAIN
        clips = F != 1 or temporal is not None
        self.loss = self.tatt = None
        cof._epoch_outputs(who, self, outputs,
                           (('logits', (N, K) if clips else (capacity, K), f32), ('probs', (capacity, K), f32),
                            ('pred', (capacity,), torch.int64), ('att', (N, P, 1), f32), ('zsave', (N, C), f32),
                            ('abar', (N,), f32)) +
                           ((('pooled', (capacity, K), f32),) if clips else ()) +
                           ((('tatt', (N,), f32),) if temporal is not None else ()) +
                           ((('loss', ((capacity + B - 1) // B, 1 + B), f32),) if want_loss else ()), dev)
        self._clip = None
        if clips:
            self._clip = cof.ApaClipPool()
            self._clip.frames, self._clip.pooled = F, self.pooled.data_ptr()
            if temporal is not None:
                _bind_temporal(who, self._clip, temporal, K)
                self._clip.tatt = self.tatt.data_ptr()
        else:
            self.pooled = self.logits
        need = int(self.lib.apa_attn_pool_workspace_bytes(N, P, C, C, K, 1, flags))
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.workspace = workspace
        self.index = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.labels = None if cache.video_labels is None else torch.zeros((capacity,), dtype=torch.int64, device=dev)
        self.targets = None if cache.video_targets is None else torch.zeros((capacity, K), dtype=f32, device=dev)
        dp = cof._dev_ptr
        self._ce = ApaClipEpoch(cache.video_first.data_ptr(), cache.video_frames.data_ptr(),
                                dp(cache.video_labels, 'labels'), dp(cache.video_targets, 'targets'), cache.V,
                                cof.APA_CLIP_FRAMES_UNIFORM, 0, 0, self.index.data_ptr(), None, None)
        self._ep = cof.ApaEpoch(None, 0)
        self._fc = cof.ApaFeatureCache(None, cache.T, 0, cache.status.data_ptr())
        self._keep = (Wa, ba, Wt, bt, temporal, None)
        X = cache.features.data_ptr()
        self._args = [
            X, X, dp(Wa, 'Wa', f32), dp(ba, 'ba', f32), dp(Wt, 'Wt', f32), dp(bt, 'bt', f32), None,
            self.logits.data_ptr(), self.att.data_ptr(), self.zsave.data_ptr(), self.abar.data_ptr(),
            dp(self.loss, 'loss'), self.probs.data_ptr(), self.pred.data_ptr(), workspace.data_ptr(), workspace.numel(),
            N, P, C, C, K, 1, flags, dt]
        self._pre = (ctypes.addressof(self._ep), ctypes.addressof(self._ce), ctypes.addressof(self._fc),
                     None if self._clip is None else ctypes.addressof(self._clip),
                     cof.APA_SCORES_SOFTMAX if scores == 'softmax' else cof.APA_SCORES_SIGMOID)

    def _rows(self, who, name, own, given, shape, dtype):
        """the destination of a per-video output: the caller's rows, or this object's"""
        if given is None:
            return own
        if own is None:
            raise ApaError('{}: {}= needs a cache with video {}'.format(who, name, name))
        if tuple(given.shape) != shape or given.device != self.cache.device:
            raise ApaError('{}: {} {} {} on the cache\'s device expected'.format(who, name, dtype, list(shape)))
        cof._dev_ptr(given, name, dtype)
        return given

    def run(self, order, count: Optional[int] = None, probs: Optional[torch.Tensor] = None,
            labels: Optional[torch.Tensor] = None, targets: Optional[torch.Tensor] = None,
            stream: Optional[int] = None) -> int:
        """Enqueue the pass over the first `count` video ids of `order` (default: all of it).  `probs` float32
        [count,K], `labels` int64 [count], `targets` float32 [count,K]: the caller's rows for the scores and the truth.
        Returns the number of steps."""
        who = 'ClipEvalEpoch.run'
        order = cof._epoch_order_arg(who, order, self.cache)
        count = int(order.numel()) if count is None else int(count)
        if not 1 <= count <= min(int(order.numel()), self.capacity):
            raise ApaError('{}: count = {} outside 1..{} (the order\'s length and the capacity)'.format(
                who, count, min(int(order.numel()), self.capacity)))
        p = self._rows(who, 'probs', self.probs, probs, (count, self.K), torch.float32)
        lab = self._rows(who, 'labels', self.labels, labels, (count,), torch.int64)
        tgt = self._rows(who, 'targets', self.targets, targets, (count, self.K), torch.float32)
        self._args[12] = p.data_ptr()
        self._ce.labels = None if lab is None else lab.data_ptr()
        self._ce.targets = None if tgt is None else tgt.data_ptr()
        self._keep = self._keep[:5] + ((order, p, lab, tgt),)
        self._ep.order, self._ep.count = order.data_ptr(), count
        rc = self.lib.apa_attn_head_eval_epoch_cached_clips(*self._pre, *self._args,
                                                            cof._stream_ptr() if stream is None else stream)
        if rc != 0:
            cof._check(rc, 'apa_attn_head_eval_epoch_cached_clips')
        return (count + self.B - 1) // self.B
