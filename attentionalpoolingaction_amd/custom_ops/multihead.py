"""H independent class-agnostic heads (cfg 002) trained and evaluated from one pass over a resident feature cache
(include/apa_multihead.h): a learning-rate / weight-decay sweep, several initialisations or a seed ensemble read the
cached conv5 maps once per direction instead of H times.

Parameters are STACKED: Wa [H,C], ba [H], Wt [H,C,K], bt [H,K], float32 on the cache's device; so is every output.  All
heads share the batch, the labels and ONE dropout mask (one (seed, offset, keep_prob)); heads that need different keep
probabilities or mask streams run as separate HeadTrainStep calls.  FP8 caches are refused by the library by name.

The entry points live in libapa_hip.so; they are declared in a header of their own and bound here, on first use, with a
signature table of their own: `custom_ops_factory._SIGNATURES` stays the mirror of include/apa.h.  There is NO fallback:
a refused call raises ApaError."""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_size_t, c_uint, c_uint64, c_void_p
from typing import Optional, Sequence

import torch

from . import custom_ops_factory as cof
from .custom_ops_factory import ApaError

APA_HEADS_MAX = 4

_P = c_void_p
# every symbol include/apa_multihead.h declares: name -> (restype, argtypes)
_SIGNATURES = {
    'apa_multihead_workspace_bytes': (c_size_t, [c_int] * 5),
    # cache, hooks, heads, X, labels; loss_wt, grad_scale; logits, att, zsave, abar, loss, G, dWa, dba, dWt, dbt; ws,
    # ws_bytes; N, P, C, K; flags, keep_prob, seed, offset, dtype; stream
    'apa_multihead_train_step_cached': (c_int, [_P] * 5 + [c_float] * 2 + [_P] * 10 + [_P, c_size_t] + [c_int] * 4 +
                                        [c_uint, c_float, c_uint64, c_uint64, c_int, _P]),
    # cache, heads, scores_kind, X, labels; logits, att, zsave, abar, loss, probs, pred, fused_probs, fused_pred; ws,
    # ws_bytes; N, P, C, K; flags, dtype; stream
    'apa_multihead_eval_step_cached': (c_int, [_P] * 2 + [c_int] + [_P] * 2 + [_P] * 9 + [_P, c_size_t] + [c_int] * 4 +
                                       [c_uint, c_int, _P]),
    # H, nseg, weights, sizes, weight_decay, grad_flat, acc_flat, lr, momentum, grad_scale, stream
    'apa_momentum_sgd_step_heads': (c_int, [c_int] * 2 + [_P] * 7 + [c_float, _P]),
    'apa_multihead_train_epoch_cached': (c_int, [_P] * 2 + [_P] * 5 + [c_float] * 2 + [_P] * 10 + [_P, c_size_t] +
                                         [c_int] * 4 + [c_uint, c_float, c_uint64, c_uint64, c_int, _P]),
    'apa_multihead_eval_epoch_cached': (c_int, [_P] + [_P] * 2 + [c_int] + [_P] * 2 + [_P] * 9 + [_P, c_size_t] +
                                        [c_int] * 4 + [c_uint, c_int, _P]),
}


class ApaMultihead(ctypes.Structure):
    """`apa_multihead` of include/apa_multihead.h (field order is the ABI)."""
    _fields_ = [('H', c_int), ('Wa', _P), ('ba', _P), ('Wt', _P), ('bt', _P)]


class ApaMultiheadSgd(ctypes.Structure):
    """`apa_multihead_sgd` of include/apa_multihead.h (field order is the ABI)."""
    _fields_ = [('nseg', c_int), ('weights', _P), ('sizes', _P), ('weight_decay', _P), ('grad_flat', _P),
                ('acc_flat', _P), ('lr', _P), ('momentum', _P), ('grad_scale', c_float)]


_lib = None


def exported_symbols():
    """Names include/apa_multihead.h declares (the CPU-side ABI test compares the two)."""
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


def workspace_bytes(H: int, N: int, P: int, C: int, K: int) -> int:
    return int(load_library().apa_multihead_workspace_bytes(int(H), int(N), int(P), int(C), int(K)))


def plan_bytes(H: int, N: int, P: int, C: int, K: int) -> int:
    """The workspace plan of include/apa_multihead.h restated on the host (the CPU test compares the two)."""
    if not (1 <= H <= APA_HEADS_MAX) or min(N, P, C, K) < 1:
        return 0
    S = max((512 + N // 2) // N, 1)
    S = min(S, min(P // 4, 256) if P >= 8 else 1)
    nblk = N * S
    up = lambda b: (b + 255) // 256 * 256
    return (up(nblk * H * C * 4) + up(nblk * 16) + up(nblk * (H * C + 4) * 4) + up(H * N * C * 4) + up(N * 8) +
            up(H * N * 4))


def _stacked(who, Wa, ba, Wt, bt):
    """(H, C, K) of four stacked parameter tensors, checked."""
    if Wt.dim() != 3:
        raise ApaError('{}: Wt [H,C,K] expected'.format(who))
    H, C, K = (int(d) for d in Wt.shape)
    for name, t, n in (('Wa', Wa, H * C), ('ba', ba, H), ('Wt', Wt, H * C * K), ('bt', bt, H * K)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n or t.device != Wt.device:
            raise ApaError('{}: {} must be contiguous float32 with {} elements on the heads\' device'.format(who, name, n))
    if not 1 <= H <= APA_HEADS_MAX:
        raise ApaError('{}: H = {} outside 1 .. {}'.format(who, H, APA_HEADS_MAX))
    return H, C, K


def grad_layout(H: int, C: int, K: int):
    """element offsets of dWa | dba | dWt | dbt in one flat gradient (and accumulator) buffer, and its length"""
    sizes = (H * C, H, H * C * K, H * K)
    offs, o = [], 0
    for s in sizes:
        offs.append(o)
        o += s
    return offs, o


class _Step(object):
    """what the two steps share: the batch, the stacked parameters, the per-step outputs and the workspace"""

    def _bind(self, who, batch, Wa, ba, Wt, bt, flags, ws_N=None):
        if not isinstance(batch, cof.CachedBatch) or isinstance(batch, cof.CachedClips):
            raise ApaError('{}: a flat CachedBatch expected'.format(who))
        self.lib = load_library()
        self.H, self.C, self.K = _stacked(who, Wa, ba, Wt, bt)
        cache = batch.cache
        if int(cache.shape[-1]) != self.C:
            raise ApaError('{}: the cache has C = {}, the heads {}'.format(who, cache.shape[-1], self.C))
        self.N = int(batch.shape[0])
        self.P = batch.numel() // (self.N * self.C)
        self.dev = cache.device
        self.params = (Wa, ba, Wt, bt)
        self._heads = ApaMultihead(self.H, Wa.data_ptr(), ba.data_ptr(), Wt.data_ptr(), bt.data_ptr())
        self.flags = int(flags)
        self.dtype = cof._feat_dtype(batch)
        H, N, P, C, K = self.H, self.N, self.P, self.C, self.K
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.att = torch.empty((H, N, P), **f32)
        self.zsave = torch.empty((H, N, C), **f32)
        self.abar = torch.empty((H, N), **f32)
        nb = max(workspace_bytes(H, N, P, C, K), 256)
        self.workspace = torch.empty((nb,), dtype=torch.uint8, device=self.dev)
        self._cached, self._index = batch, batch.index

    def _labels(self, who, labels, n_rows):
        """-> (labels_cached, tensor or None)"""
        cache = self._cached.cache
        if isinstance(labels, str):
            if labels != 'cache' or cache.labels is None:
                raise ApaError('{}: labels is an int64 tensor or \'cache\' (a cache with labels)'.format(who))
            return True, cache.labels
        if labels is None:
            return False, None
        if labels.dtype != torch.int64 or labels.numel() != n_rows or labels.device != self.dev or \
                not labels.is_contiguous():
            raise ApaError('{}: labels int64 [{}] on the cache\'s device expected'.format(who, n_rows))
        return False, labels


class MultiHeadTrainStep(_Step):
    """apa_multihead_train_step_cached bound to its buffers.  `labels`: int64 [N], or 'cache' (the cache's labels through
    the index).  The gradients dWa | dba | dWt | dbt are views of ONE flat buffer `grad_flat` (grad_layout), the layout
    MultiHeadSGD reads.  Outputs as attributes: logits [H,N,K], att, zsave, abar, loss [H,1+N], G, dWa, dba, dWt, dbt."""

    def __init__(self, batch, Wa, ba, Wt, bt, labels, *, relu_att=False, keep_prob=1.0, seed=0, offset=0, loss_wt=1.0,
                 grad_scale=1.0, grad_flat=None, hooks=None):
        who = 'MultiHeadTrainStep'
        flags = cof.APA_FLAG_FROZEN_INPUT | (cof.APA_FLAG_RELU_ATT if relu_att else 0) | \
            (cof.APA_FLAG_TRAIN if keep_prob < 1.0 else 0)
        self._bind(who, batch, Wa, ba, Wt, bt, flags)
        H, N, C, K = self.H, self.N, self.C, self.K
        self._labels_cached, self.labels = self._labels(who, labels, N)
        if self.labels is None:
            raise ApaError('{}: training needs labels'.format(who))
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.logits = torch.empty((H, N, K), **f32)
        self.loss = torch.empty((H, 1 + N), **f32)
        self.G = torch.empty((H, N, K), **f32)
        offs, total = grad_layout(H, C, K)
        if grad_flat is None:
            grad_flat = torch.zeros((total,), **f32)
        if grad_flat.dtype != torch.float32 or grad_flat.numel() != total or not grad_flat.is_contiguous():
            raise ApaError('{}: grad_flat float32 [{}] expected'.format(who, total))
        self.grad_flat = grad_flat
        self.dWa = grad_flat[offs[0]:offs[1]].view(H, C)
        self.dba = grad_flat[offs[1]:offs[2]]
        self.dWt = grad_flat[offs[2]:offs[3]].view(H, C, K)
        self.dbt = grad_flat[offs[3]:].view(H, K)
        self.keep_prob, self.seed, self.offset = float(keep_prob), int(seed), int(offset)
        self.loss_wt, self.grad_scale = float(loss_wt), float(grad_scale)
        self._hooks = hooks
        self._fc = batch.descriptor(labels_cached=self._labels_cached)

    def rebind(self, index=None, offset=None, labels=None) -> None:
        """another batch of the same cache (int32 index of the same length), another dropout offset, other labels"""
        if index is not None:
            self._index = cof._index_tensor('MultiHeadTrainStep.rebind', index, self.dev, self.N)
            self._fc.index = self._index.data_ptr()
        if offset is not None:
            self.offset = int(offset)
        if labels is not None:
            if self._labels_cached:
                raise ApaError('MultiHeadTrainStep.rebind: the step reads the cache\'s labels through the index')
            _, self.labels = self._labels('MultiHeadTrainStep.rebind', labels, self.N)

    def _args(self):
        return [ctypes.addressof(self._heads), self._cached.data_ptr(), self.labels.data_ptr(), self.loss_wt,
                self.grad_scale, self.logits.data_ptr(), self.att.data_ptr(), self.zsave.data_ptr(), self.abar.data_ptr(),
                self.loss.data_ptr(), self.G.data_ptr(), self.dWa.data_ptr(), self.dba.data_ptr(), self.dWt.data_ptr(),
                self.dbt.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), self.N, self.P, self.C, self.K,
                self.flags, self.keep_prob, self.seed, self.offset, self.dtype]

    def run(self, stream: Optional[int] = None) -> None:
        hk = cof._hooks_ptr(self._hooks)
        rc = self.lib.apa_multihead_train_step_cached(ctypes.addressof(self._fc), hk, *self._args(),
                                                      cof._stream_ptr() if stream is None else stream)
        cof._check(rc, 'apa_multihead_train_step_cached')


class MultiHeadEvalStep(_Step):
    """apa_multihead_eval_step_cached bound to its buffers.  `labels`: None (no loss), int64 [N] or 'cache'.  Outputs:
    logits, probs [H,N,K], pred int64 [H,N], att, zsave, abar, loss [H,1+N] (with labels), and with `fused` the
    late-fusion scores fused_probs [N,K] (the mean over heads) and fused_pred int64 [N]."""

    def __init__(self, batch, Wa, ba, Wt, bt, labels=None, *, relu_att=False, scores='softmax', fused=True):
        who = 'MultiHeadEvalStep'
        self._bind(who, batch, Wa, ba, Wt, bt, cof.APA_FLAG_RELU_ATT if relu_att else 0)
        H, N, K = self.H, self.N, self.K
        self.scores_kind = cof._scores_kind(who, scores)
        self._labels_cached, self.labels = self._labels(who, labels, N)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.logits = torch.empty((H, N, K), **f32)
        self.probs = torch.empty((H, N, K), **f32)
        self.pred = torch.empty((H, N), dtype=torch.int64, device=self.dev)
        self.loss = torch.empty((H, 1 + N), **f32) if self.labels is not None else None
        self.fused_probs = torch.empty((N, K), **f32) if fused else None
        self.fused_pred = torch.empty((N,), dtype=torch.int64, device=self.dev) if fused else None
        self._fc = batch.descriptor(labels_cached=self._labels_cached)

    def rebind(self, index=None) -> None:
        if index is not None:
            self._index = cof._index_tensor('MultiHeadEvalStep.rebind', index, self.dev, self.N)
            self._fc.index = self._index.data_ptr()

    def run(self, stream: Optional[int] = None) -> None:
        p = lambda t: None if t is None else t.data_ptr()
        rc = self.lib.apa_multihead_eval_step_cached(
            ctypes.addressof(self._fc), ctypes.addressof(self._heads), self.scores_kind, self._cached.data_ptr(),
            p(self.labels), self.logits.data_ptr(), self.att.data_ptr(), self.zsave.data_ptr(), self.abar.data_ptr(),
            p(self.loss), self.probs.data_ptr(), self.pred.data_ptr(), p(self.fused_probs), p(self.fused_pred),
            self.workspace.data_ptr(), self.workspace.numel(), self.N, self.P, self.C, self.K, self.flags, self.dtype,
            cof._stream_ptr() if stream is None else stream)
        cof._check(rc, 'apa_multihead_eval_step_cached')


class MultiHeadSGD(object):
    """apa_momentum_sgd_step_heads bound to the stacked parameters: one launch updates every head with its own learning
    rate, momentum and per-segment weight decay.  `weights`: the stacked tensors, each [H, ...], in the order of the
    flat buffers; `weight_decay`: per segment one float or H floats; `grad_flat` / `acc_flat`: the stacked segments back
    to back (grad_layout for Wa, ba, Wt, bt)."""

    def __init__(self, weights: Sequence[torch.Tensor], weight_decay, grad_flat, acc_flat, lr, momentum,
                 grad_scale: float = 1.0):
        who = 'MultiHeadSGD'
        self.lib = load_library()
        self.H = H = int(weights[0].shape[0])
        nseg = len(weights)
        total = 0
        for i, w in enumerate(weights):
            if w.dtype != torch.float32 or not w.is_contiguous() or int(w.shape[0]) != H or w.numel() % H:
                raise ApaError('{}: weights[{}] must be contiguous float32 [H, ...]'.format(who, i))
            total += w.numel()
        for name, t in (('grad_flat', grad_flat), ('acc_flat', acc_flat)):
            if t.dtype != torch.float32 or t.numel() != total or not t.is_contiguous():
                raise ApaError('{}: {} float32 [{}] expected'.format(who, name, total))
        self.weights, self.grad_flat, self.acc_flat = list(weights), grad_flat, acc_flat
        self.nseg = nseg
        self._w = (c_void_p * nseg)(*[w.data_ptr() for w in weights])
        self._sizes = (c_size_t * nseg)(*[w.numel() // H for w in weights])
        wd = []
        for d in weight_decay:
            row = [float(d)] * H if not hasattr(d, '__len__') else [float(v) for v in d]
            if len(row) != H:
                raise ApaError('{}: H weight decays per segment expected'.format(who))
            wd += row
        self._wd = (c_float * (nseg * H))(*wd)
        self._lr = (c_float * H)(*self._per_head(who, lr))
        self._mom = (c_float * H)(*self._per_head(who, momentum))
        self.grad_scale = float(grad_scale)

    def _per_head(self, who, v):
        row = [float(v)] * self.H if not hasattr(v, '__len__') else [float(x) for x in v]
        if len(row) != self.H:
            raise ApaError('{}: one value or H values expected'.format(who))
        return row

    def descriptor(self, lr_table) -> ApaMultiheadSgd:
        """apa_multihead_sgd for an epoch; lr_table: a ctypes float array [steps * H] the caller keeps alive"""
        return ApaMultiheadSgd(self.nseg, ctypes.addressof(self._w), ctypes.addressof(self._sizes),
                               ctypes.addressof(self._wd), self.grad_flat.data_ptr(), self.acc_flat.data_ptr(),
                               ctypes.addressof(lr_table), ctypes.addressof(self._mom), self.grad_scale)

    def run(self, lr=None, stream: Optional[int] = None) -> None:
        if lr is not None:
            self._lr = (c_float * self.H)(*self._per_head('MultiHeadSGD.run', lr))
        rc = self.lib.apa_momentum_sgd_step_heads(
            self.H, self.nseg, ctypes.addressof(self._w), ctypes.addressof(self._sizes), ctypes.addressof(self._wd),
            self.grad_flat.data_ptr(), self.acc_flat.data_ptr(), ctypes.addressof(self._lr), ctypes.addressof(self._mom),
            self.grad_scale, cof._stream_ptr() if stream is None else stream)
        cof._check(rc, 'apa_momentum_sgd_step_heads')


class MultiHeadTrainEpoch(object):
    """apa_multihead_train_epoch_cached: `steps` training steps and heads updates behind one host call.  Built on a
    MultiHeadTrainStep (its buffers, flags and dropout key; its index is ignored) and a MultiHeadSGD on the step's
    grad_flat.  `run(order, lr)`: order int32 [steps * N] on the device, lr [steps][H] (or [H], or one float); with
    labels that are not the cache's, `labels` int64 [steps * N] in visiting order.  Returns the loss log [steps,H,1+N]."""

    def __init__(self, step: MultiHeadTrainStep, sgd: MultiHeadSGD, steps: int):
        if sgd.grad_flat.data_ptr() != step.grad_flat.data_ptr() or sgd.H != step.H:
            raise ApaError('MultiHeadTrainEpoch: the optimiser must read the step\'s grad_flat')
        self.step, self.sgd, self.steps = step, sgd, int(steps)
        self.loss = torch.empty((self.steps, step.H, 1 + step.N), dtype=torch.float32, device=step.dev)
        self.epochs_run = 0

    def run(self, order: torch.Tensor, lr, labels=None, offset=None, stream: Optional[int] = None) -> torch.Tensor:
        st, H, steps = self.step, self.step.H, self.steps
        order = cof._index_tensor('MultiHeadTrainEpoch.run', order, st.dev, steps * st.N)
        if st._labels_cached:
            lab = st.labels
        else:
            if labels is None or labels.dtype != torch.int64 or labels.numel() != steps * st.N:
                raise ApaError('MultiHeadTrainEpoch.run: labels int64 [steps * N] in visiting order expected')
            lab = labels
        rows = [[float(lr)] * H] * steps if not hasattr(lr, '__len__') else \
            ([[float(v) for v in lr]] * steps if not hasattr(lr[0], '__len__') else [[float(v) for v in r] for r in lr])
        if len(rows) != steps or any(len(r) != H for r in rows):
            raise ApaError('MultiHeadTrainEpoch.run: lr [steps][H] expected')
        table = (c_float * (steps * H))(*[v for r in rows for v in r])
        opt = self.sgd.descriptor(table)
        ep = cof.ApaEpoch(order.data_ptr(), steps * st.N)
        if offset is not None:
            st.offset = int(offset)
        a = st._args()
        a[2] = lab.data_ptr()
        a[9] = self.loss.data_ptr()
        rc = st.lib.apa_multihead_train_epoch_cached(ctypes.addressof(ep), ctypes.addressof(opt), ctypes.addressof(st._fc),
                                                     cof._hooks_ptr(st._hooks), *a,
                                                     cof._stream_ptr() if stream is None else stream)
        cof._check(rc, 'apa_multihead_train_epoch_cached')
        st.offset += steps       # the dropout counter advances once per step for all heads
        return self.loss


class MultiHeadEvalEpoch(object):
    """apa_multihead_eval_epoch_cached: every row of `order` (up to `capacity`) scored behind one host call, N rows per
    step and a smaller last batch.  Outputs for the first `count` rows: logits / probs [H,count,K], pred [H,count],
    fused_probs [count,K], fused_pred [count] (with `fused`), loss log [steps,H,1+N] (with labels)."""

    def __init__(self, cache, N, Wa, ba, Wt, bt, *, capacity, relu_att=False, scores='softmax', fused=True,
                 labels=None):
        who = 'MultiHeadEvalEpoch'
        self._step = MultiHeadEvalStep(cache.select(torch.zeros((int(N),), dtype=torch.int32, device=cache.device)), Wa,
                                       ba, Wt, bt, 'cache' if labels == 'cache' else None, relu_att=relu_att,
                                       scores=scores, fused=fused)
        st = self._step
        self.capacity, self.N, self.H = int(capacity), int(N), st.H
        self._want_loss = labels is not None
        self._labels_cached = labels == 'cache'
        # the smaller last batch plans its own workspace: size for every batch size up to N
        nb = max(workspace_bytes(st.H, n, st.P, st.C, st.K) for n in range(1, self.N + 1))
        self.workspace = torch.empty((max(nb, 256),), dtype=torch.uint8, device=st.dev)
        self._fused = fused
        self.who = who

    def run(self, order: torch.Tensor, labels=None, stream: Optional[int] = None):
        st = self._step
        H, N, K = st.H, self.N, st.K
        count = int(order.numel())
        if count < 1 or count > self.capacity:
            raise ApaError('{}: 1 .. {} rows expected'.format(self.who, self.capacity))
        order = cof._index_tensor(self.who, order, st.dev, count)
        steps = (count + N - 1) // N
        f32 = dict(dtype=torch.float32, device=st.dev)
        self.logits = torch.empty((H, count, K), **f32)
        self.probs = torch.empty((H, count, K), **f32)
        self.pred = torch.empty((H, count), dtype=torch.int64, device=st.dev)
        self.fused_probs = torch.empty((count, K), **f32) if self._fused else None
        self.fused_pred = torch.empty((count,), dtype=torch.int64, device=st.dev) if self._fused else None
        lab = None
        if self._want_loss:
            lab = st.labels if self._labels_cached else labels
            if lab is None or lab.dtype != torch.int64 or (not self._labels_cached and lab.numel() != count):
                raise ApaError('{}: labels int64 [count] in visiting order expected'.format(self.who))
        self.loss = torch.zeros((steps, H, 1 + N), **f32) if self._want_loss else None
        p = lambda t: None if t is None else t.data_ptr()
        ep = cof.ApaEpoch(order.data_ptr(), count)
        fc = cof.ApaFeatureCache(None, st._cached.cache.T, 1 if self._labels_cached else 0,
                                 st._cached.cache.status.data_ptr())
        rc = st.lib.apa_multihead_eval_epoch_cached(
            ctypes.addressof(ep), ctypes.addressof(fc), ctypes.addressof(st._heads), st.scores_kind,
            st._cached.data_ptr(), p(lab), self.logits.data_ptr(), st.att.data_ptr(), st.zsave.data_ptr(),
            st.abar.data_ptr(), p(self.loss), self.probs.data_ptr(), self.pred.data_ptr(), p(self.fused_probs),
            p(self.fused_pred), self.workspace.data_ptr(), self.workspace.numel(), N, st.P, st.C, K, st.flags, st.dtype,
            cof._stream_ptr() if stream is None else stream)
        cof._check(rc, 'apa_multihead_eval_epoch_cached')
        return self.probs, self.pred, self.fused_probs, self.fused_pred
