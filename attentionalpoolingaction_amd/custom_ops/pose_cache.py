"""The pose-regularised head (cfg 003) trained and evaluated from a resident feature cache (include/apa_pose_cache.h).

The counterpart of custom_ops_factory's HeadTrainStep / HeadEvalStep on a CachedBatch for the head they leave out:
PoseLogits 2048 -> 768 -> 16 with attention from pose_pre_logits, the pose L2 loss and the cross-entropy.  The batch is
the cache plus an int32 index; the three kernel families that read the feature map follow the index on the device and
nothing is gathered.  A cached step equals the plain step (PoseAttnTrainStep with grads[0] = None, PoseAttnEvalStep) on
`cache.gather(index)` bit for bit.

The entry points live in the same libapa_hip.so as everything else; they are declared in a header of their own and
bound here, on first use, with a signature table of their own: `custom_ops_factory._SIGNATURES` stays the mirror of
include/apa.h.  There is NO fallback: a cache has no dX, so a refused frozen step is an error, never a full step."""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_uint, c_uint64, c_void_p
from typing import Optional

import torch

from . import custom_ops_factory as cof
from .custom_ops_factory import ApaError

# every symbol include/apa_pose_cache.h declares: name -> (restype, argtypes)
_SIGNATURES = {
    # cache, io; N, P, C, Cp, J, K; flags, keep_prob, seed, offset, dtype; stream
    'apa_pose_attn_train_step_cached': (c_int, [c_void_p] * 2 + [c_int] * 6 + [c_uint, c_float, c_uint64, c_uint64,
                                                                              c_int, c_void_p]),
    # cache, io; N, P, C, Cp, J, K; flags, dtype; stream
    'apa_pose_attn_eval_step_cached': (c_int, [c_void_p] * 2 + [c_int] * 6 + [c_uint, c_int, c_void_p]),
}

_lib = None


def exported_symbols():
    """Names include/apa_pose_cache.h declares (the CPU-side ABI test compares the three)."""
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


def cached_pose_served(batch, Cp: int, J: int, K: int, train: bool = True) -> bool:
    """Does the library serve the cfg 003 head on this batch?  The C admission rule (apa_capi.hip: pose_cache_check,
    apa_gemm_bf16.hip: gemm_rowmap_check) restated on the host, so that a caller learns it without a GPU error: a flat
    CachedBatch (no clips) on a 16-byte aligned bf16 cache, C and Cp whole 16-byte vectors (the Ppre product on the bf16
    MFMA path; C <= 9584 is the pooling passes' limit), at least 8 batch rows, and for training N * P a multiple of 8 --
    the contraction of dW1 = X^T . dPpre, which the dispatcher otherwise sends to the fp32-unpacking kernel."""
    if not isinstance(batch, cof.CachedBatch) or isinstance(batch, cof.CachedClips):
        return False
    cache = batch.cache
    if cache.fp8 or cache.dtype != torch.bfloat16:
        return False
    C = int(batch.shape[-1])
    N = int(batch.shape[0])
    R = batch.numel() // C
    Cp, J, K = int(Cp), int(J), int(K)
    if N < 1 or J < 1 or K < 1 or Cp < 8 or C < 8 or C % 8 or Cp % 8 or C > 9584 or R < 8:
        return False
    if cache.features.data_ptr() % 16:
        return False
    return not (train and R % 8)


class PoseAttnTrainStepCached(cof.PoseAttnTrainStep):
    """apa_pose_attn_train_step_cached bound to caller-owned buffers: cof.PoseAttnTrainStep with a flat CachedBatch in
    place of `X` (frozen features: `grads[0]` must be None).  `labels=None` (or 'cache', the evaluation step's word, where
    None means the label-free form) reads the cache's labels through the index;
    `pose_labels` [N,P,J] / `pose_valid` [N,J] have the batch shape (PoseLabelTable.gather fills them).  `w1_bf16` and
    `w2t_bf16` work as in the plain step.  Outputs as attributes, as there."""

    def __init__(self, batch, params, labels, pose_labels, pose_valid, grads, *, flags=0, keep_prob=1.0, seed=0,
                 offset=0, action_wt=1.0, pose_wt=1.0, grad_scale=1.0, w1_bf16=None, share_with=None, w2t_bf16=None):
        who = 'PoseAttnTrainStepCached'
        if not isinstance(batch, cof.CachedBatch) or isinstance(batch, cof.CachedClips):
            raise ApaError('{}: a flat CachedBatch expected (clips are not served from a cache by this head)'.format(who))
        if grads[0] is not None:
            raise ApaError('{}: a CachedBatch is frozen (no gradient for X: grads[0] = None)'.format(who))
        cache = batch.cache
        N = int(batch.shape[0])
        self._labels_cached = labels is None or (isinstance(labels, str) and labels == 'cache')
        if self._labels_cached:
            if cache.labels is None:
                raise ApaError('{}: labels=None reads the cache\'s labels, and the cache has none'.format(who))
            bound = torch.empty((N,), dtype=torch.int64, device=cache.device)   # (shape check only; see io.labels below)
        else:
            bound = labels
        load_library()
        cof.PoseAttnTrainStep.__init__(self, batch, params, bound, pose_labels, pose_valid, grads, flags=flags,
                                       keep_prob=keep_prob, seed=seed, offset=offset, action_wt=action_wt,
                                       pose_wt=pose_wt, grad_scale=grad_scale, w1_bf16=w1_bf16, share_with=share_with,
                                       w2t_bf16=w2t_bf16)
        if self._labels_cached:     # the [T] table behind the index (this object keeps it alive)
            self._cache_labels = cache.labels
            self._io.labels = cache.labels.data_ptr()
        self._cached, self._index = batch, batch.index
        self._fc = batch.descriptor(labels_cached=self._labels_cached)
        self._pre = (ctypes.addressof(self._fc),)
        self._fn, self._name = self.lib.apa_pose_attn_train_step_cached, 'apa_pose_attn_train_step_cached'

    def rebind(self, index=None, labels=None, pose_labels=None, pose_valid=None, offset=None) -> None:
        """Another batch of the same cache (`index`: int32 of the same length on the cache's device), other labels /
        pose labels of the same shapes, another dropout offset: each swaps one marshalled pointer (or the integer) and
        nothing else."""
        if index is not None:
            self._index = cof._index_tensor('PoseAttnTrainStepCached.rebind', index, self._cached.cache.device,
                                            self._cached.shape[0])
            self._fc.index = self._index.data_ptr()
        if labels is not None and self._labels_cached:
            raise ApaError('PoseAttnTrainStepCached.rebind: the step reads the cache\'s labels through the index')
        cof.PoseAttnTrainStep.rebind(self, labels=labels, pose_labels=pose_labels, pose_valid=pose_valid, offset=offset)

    def run(self, stream: Optional[int] = None) -> None:
        rc = self._fn(*self._pre, *self._args, cof._stream_ptr() if stream is None else stream)
        if rc != 0:     # (no fallback to a full step: a cache has no dX)
            cof._check(rc, self._name)


class PoseAttnEvalStepCached(cof.PoseAttnEvalStep):
    """apa_pose_attn_eval_step_cached: cof.PoseAttnEvalStep with a flat CachedBatch in place of `X`.  `labels='cache'`
    reads the cache's labels through the index (labels=None stays the label-free form).  Both routes are kept."""

    def __init__(self, batch, params, labels=None, *, flags=0, w1_bf16=None, want_pose_logits=False, workspace=None):
        who = 'PoseAttnEvalStepCached'
        if not isinstance(batch, cof.CachedBatch) or isinstance(batch, cof.CachedClips):
            raise ApaError('{}: a flat CachedBatch expected (clips are not served from a cache by this head)'.format(who))
        cache = batch.cache
        self._labels_cached = isinstance(labels, str)
        if self._labels_cached:
            if labels != 'cache' or cache.labels is None:
                raise ApaError('{}: labels is None, an int64 [N] tensor or \'cache\' (a cache with labels)'.format(who))
            labels = torch.empty((int(batch.shape[0]),), dtype=torch.int64, device=cache.device)
        load_library()
        cof.PoseAttnEvalStep.__init__(self, batch, params, labels, flags=flags, w1_bf16=w1_bf16,
                                      want_pose_logits=want_pose_logits, workspace=workspace)
        if self._labels_cached:     # the [T] table behind the index (this object keeps it alive)
            self._cache_labels = cache.labels
            self._io.labels = cache.labels.data_ptr()
        self._cached, self._index = batch, batch.index
        self._fc = batch.descriptor(labels_cached=self._labels_cached)
        self._args = [ctypes.addressof(self._fc)] + self._args
        self._fn, self._name = self.lib.apa_pose_attn_eval_step_cached, 'apa_pose_attn_eval_step_cached'

    def rebind(self, index=None, labels=None) -> None:
        """Another batch of the same cache and / or other labels of the same shape: one pointer each."""
        if index is not None:
            self._index = cof._index_tensor('PoseAttnEvalStepCached.rebind', index, self._cached.cache.device,
                                            self._cached.shape[0])
            self._fc.index = self._index.data_ptr()
        if labels is not None:
            if self._labels_cached:
                raise ApaError('PoseAttnEvalStepCached.rebind: the step reads the cache\'s labels through the index')
            cof.PoseAttnEvalStep.rebind(self, labels=labels)


class PoseLabelTable(object):
    """The pose labels of every cached image, `pose_labels` float32 [T,H',W',J] and `pose_valid` uint8 / bool [T,J] on
    the cache's device.  `gather(index, out_labels, out_valid)` writes the batch's rows into a bound step's own buffers
    with two torch.index_select(..., out=) launches -- the pose labels are 0.4 MB per step against 25.7 MB of features,
    and an in-kernel lookup would put the index into the Pl kernel and the pose loss as well."""

    def __init__(self, pose_labels: torch.Tensor, pose_valid: torch.Tensor):
        if pose_valid.dtype == torch.bool:
            pose_valid = pose_valid.to(torch.uint8)
        if pose_labels.dtype != torch.float32 or pose_labels.dim() < 2 or pose_valid.dtype != torch.uint8 or \
                pose_valid.dim() != 2 or pose_valid.shape[0] != pose_labels.shape[0] or \
                pose_valid.shape[1] != pose_labels.shape[-1] or pose_valid.device != pose_labels.device:
            raise ApaError('PoseLabelTable: pose_labels float32 [T,...,J] and pose_valid uint8 [T,J] on one device '
                           'expected')
        self.T, self.J = int(pose_labels.shape[0]), int(pose_labels.shape[-1])
        self.pose_labels = pose_labels.contiguous().view(self.T, -1)
        self.pose_valid = pose_valid.contiguous()
        self.device = pose_labels.device

    def new_batch(self, N: int):
        """(pose_labels [N, P*J] float32, pose_valid [N, J] uint8): buffers a step can be bound to"""
        return (torch.zeros((int(N), self.pose_labels.shape[1]), dtype=torch.float32, device=self.device),
                torch.zeros((int(N), self.J), dtype=torch.uint8, device=self.device))

    def gather(self, index, out_labels: torch.Tensor, out_valid: torch.Tensor, clamp: bool = True) -> None:
        """out_labels <- pose_labels[index], out_valid <- pose_valid[index]: two index_select launches, plus -- with
        `clamp`, the default -- one launch in front that clamps the ids into the table as the kernels clamp them into the
        cache (index_select itself stops the device on an id outside [0, T)).  Pass clamp=False for an index known to lie
        in [0, T), e.g. an epoch's permutation: then exactly the two launches run.  `index`: an int32 / int64 tensor on
        the table's device is used as it is; a list or a tensor elsewhere costs a host-to-device copy per call"""
        idx = index if isinstance(index, torch.Tensor) else torch.as_tensor(list(index), dtype=torch.int32)
        if idx.device != self.device or idx.dtype not in (torch.int32, torch.int64):
            idx = idx.to(device=self.device, dtype=torch.int32)
        if clamp:
            idx = idx.clamp(0, self.T - 1)
        n = int(idx.numel())
        if out_labels.numel() != n * self.pose_labels.shape[1] or out_valid.numel() != n * self.J or \
                not out_labels.is_contiguous() or not out_valid.is_contiguous():
            raise ApaError('PoseLabelTable.gather: contiguous out_labels [N,P,J] and out_valid [N,J] expected')
        torch.index_select(self.pose_labels, 0, idx, out=out_labels.view(n, -1))
        torch.index_select(self.pose_valid, 0, idx, out=out_valid.view(n, self.J))
