"""Data-parallel deployment of the head: one process per GPU, RCCL all-reduce over xGMI.

Reference semantics (/root/reference/models/slim/deployment/model_deploy.py):
  * every clone's loss is divided by num_clones          (_gather_clone_loss, :223-225)
  * per variable, the tower gradients are summed          (_sum_clones_gradients, :421-451)
  * the regularisation loss is added once (clone 0)       (optimize_clones, :294-309)
  * with TRAIN.ITER_SIZE > 1 gradients are accumulated locally and applied on the last
    micro-step                                           (src/train.py:529-566)
The reference does this in ONE process with towers on /gpu:i and the sum on the CPU device.  Here
each rank owns one MI355X and the sum is a single `all_reduce(SUM)` of one flat fp32 bucket
([dWa | dba | dWt | dbt | ...]: 3.2 MB for cfg 002) -- the kernels write their gradients straight
into views of that bucket, so there is no packing copy.  Backend "nccl" is RCCL on ROCm; the same
code runs on "gloo" with CPU tensors (tests/test_deploy_gloo_cpu.py, tests/test_train_reference_cpu.py,
world_size 2).
"""
from __future__ import annotations

import collections
import functools
import weakref
from typing import Callable, Dict, Iterable, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.distributed as dist


class DeploymentConfig:
    """The subset of slim's DeploymentConfig (model_deploy.py:481-683) that survives the move to
    one-process-per-GPU: the clone count and this process's clone index."""

    def __init__(self, num_clones: Optional[int] = None, clone_index: Optional[int] = None,
                 process_group=None):
        if dist.is_available() and dist.is_initialized():
            self.num_clones = dist.get_world_size(process_group) if num_clones is None else num_clones
            self.clone_index = dist.get_rank(process_group) if clone_index is None else clone_index
        else:
            self.num_clones = 1 if num_clones is None else num_clones
            self.clone_index = 0 if clone_index is None else clone_index
        self.process_group = process_group

    @property
    def clone_loss_scale(self) -> float:
        """model_deploy.py:223-225: clone_loss / num_clones (only when num_clones > 1)."""
        return 1.0 / self.num_clones if self.num_clones > 1 else 1.0

    def is_chief(self) -> bool:
        return self.clone_index == 0


def trainable_scopes(cfg) -> list:
    """TRAIN.TRAINABLE_SCOPES as `_get_variables_to_train` reads it (src/train.py:172-175): '' -> [] (every trainable
    variable), otherwise the comma-separated scopes, each stripped."""
    s = cfg.TRAIN.TRAINABLE_SCOPES
    return [scope.strip() for scope in s.split(',')] if s != '' else []


def in_trainable_scopes(tf_name: str, scopes: Sequence[str]) -> bool:
    """`tf.get_collection(TRAINABLE_VARIABLES, scope)` (src/train.py:178-180) is a PREFIX match on the variable name:
    'PosePrelogitsBasedAttention/Conv' also takes 'PosePrelogitsBasedAttention/Conv2d_PrePose_Attn/weights'.  No
    scopes: every variable."""
    return not scopes or any(tf_name.startswith(s) for s in scopes)


def _tf_trainable_variables(network_fn):
    """[(TF name, Parameter)] of every trainable variable in creation order: the backbone's (its batch-norm moving
    statistics are not trainable variables), the head's, 'TemporalAttention/Conv/*'."""
    out = []
    backbone = getattr(network_fn, 'backbone', None)
    if backbone is not None and hasattr(backbone, 'tf_variable_map'):
        for tfn, (mod, attr) in backbone.tf_variable_map().items():
            p = getattr(mod, attr)
            if isinstance(p, torch.nn.Parameter):
                out.append((tfn, p))
    head = network_fn.head
    named = dict(head.named_parameters())
    out += [(tfn, named[attr]) for attr, tfn in head.tf_variable_names().items() if attr in named]
    temporal = getattr(network_fn, 'temporal', None)
    if temporal is not None:
        out += [('TemporalAttention/Conv/weights', temporal['weights']),
                ('TemporalAttention/Conv/biases', temporal['biases'])]
    return out


def variables_to_train(network_fn, cfg) -> list:
    """_get_variables_to_train (src/train.py:166-181): the ordered TF names of the variables the optimiser trains --
    every trainable variable when TRAIN.TRAINABLE_SCOPES is empty, else scope by scope (in the order listed) the
    variables whose name starts with the scope, in creation order; a variable two scopes reach is listed once."""
    names = [tfn for tfn, _ in _tf_trainable_variables(network_fn)]
    scopes = trainable_scopes(cfg)
    if not scopes:
        return names
    return list(dict.fromkeys(n for s in scopes for n in names if n.startswith(s)))


def apply_trainable_scopes(network_fn, cfg) -> list:
    """`requires_grad_(False)` on every parameter outside `variables_to_train` (backbone included) -> that list.  The
    reference hands the list to `optimize_clones(var_list=...)` (src/train.py:504-513): a variable outside it has no
    gradient, no L2 step and no optimiser slot.  With a scope list that reaches no backbone variable the conv5 map
    then needs no gradient either."""
    trained = variables_to_train(network_fn, cfg)
    keep = set(trained)
    for tfn, p in _tf_trainable_variables(network_fn):
        if tfn not in keep:
            p.requires_grad_(False)
    return trained


class GradientBucket:
    """One flat fp32 buffer holding every head gradient; `views[name]` are the per-parameter
    windows the HIP kernels (or autograd) write into."""

    def __init__(self, shapes: Dict[str, Sequence[int]], device, dtype=torch.float32):
        self.names = list(shapes)
        self.shapes = {k: tuple(v) for k, v in shapes.items()}
        sizes = [int(torch.Size(self.shapes[k]).numel()) for k in self.names]
        self.flat = torch.zeros(sum(sizes), dtype=dtype, device=device)
        self.views: Dict[str, torch.Tensor] = {}
        o = 0
        for k, s in zip(self.names, sizes):
            self.views[k] = self.flat[o:o + s].view(self.shapes[k])
            o += s

    @classmethod
    def for_parameters(cls, named_params: Iterable[Tuple[str, torch.Tensor]]):
        named = list(named_params)
        return cls({n: p.shape for n, p in named}, named[0][1].device)

    def zero_(self):
        self.flat.zero_()

    def nbytes(self) -> int:
        return self.flat.numel() * self.flat.element_size()


def sum_clone_gradients(bucket: GradientBucket, config: DeploymentConfig, async_op: bool = False,
                        comm=None):
    """_sum_clones_gradients: one all-reduce(SUM) of the flat bucket.  The gradients must already
    carry the 1/num_clones loss scale (pass DeploymentConfig.clone_loss_scale as `grad_scale` to
    the loss kernel).  `comm`: an `rccl.RcclCommunicator` -> the collective is one in-stream
    ncclAllReduce on the current stream (no torch.distributed call on the step path); otherwise
    torch.distributed (gloo on CPU, "nccl" = RCCL on GPU), which returns the work handle when
    async_op=True (overlap with the next micro-batch's forward; wait before the optimizer step)."""
    if config.num_clones == 1:
        return None
    if comm is not None:
        comm.all_reduce_(bucket.flat)
        return None
    return dist.all_reduce(bucket.flat, op=dist.ReduceOp.SUM, group=config.process_group,
                           async_op=async_op)


class HipRuntime:
    """streams / events / hooks of one GPU as OverlappedGradientSum uses them (torch.cuda + cof.make_hooks)"""

    def __init__(self, device):
        self.device = device

    def current_stream(self):
        return torch.cuda.current_stream(self.device)

    def new_stream(self):
        return torch.cuda.Stream(self.device)

    def new_event(self):
        return torch.cuda.Event()

    def synchronize(self) -> None:
        torch.cuda.synchronize(self.device)

    def stream(self, s):
        return torch.cuda.stream(s)

    def make_hooks(self, grad_ready, td_weights_ready):
        from .custom_ops import custom_ops_factory as cof
        return cof.make_hooks(grad_ready=grad_ready, td_weights_ready=td_weights_ready)


def probe_overlap_schedule(run_two_streams, run_in_stream, barrier, reduce_max, loops: int = 3, steps: int = 30):
    """`--overlap auto`: which gradient-sum schedule is faster on THIS node is measured, not assumed.  `loops` timed
    loops of `steps` steps of each schedule (after one warm loop each), the median loop of each MAX-reduced over the
    ranks -- every rank therefore sees the same two figures and takes the same decision, whatever its own clock
    said.  -> (keep_two_streams, us_two_streams, us_in_stream)."""
    import time

    def probe(fn):
        t = []
        for _ in range(loops):
            barrier()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            barrier()
            t.append((time.perf_counter() - t0) / steps * 1e6)
        return reduce_max(sorted(t)[len(t) // 2])
    probe(run_two_streams), probe(run_in_stream)               # (both warm)
    us_two, us_one = probe(run_two_streams), probe(run_in_stream)
    return us_two < us_one, us_two, us_one


class OverlappedGradientSum:
    """Two-stream gradient sum for the M == 1 head: the classifier part of the bucket (td_weights |
    td_biases, 99.7 % of the bytes) is final after the FIRST kernel of `apa_attn_pool_bwd` and is not
    read again before the logits product of the NEXT forward call, so its all-reduce (and, if given,
    its optimizer update) runs on a communication stream underneath the streaming backward pass of
    step k and the pooling / finalize passes of step k+1.  Only the attention part (att_weights |
    att_biases, 8 KB), produced by the last kernel of the backward call and needed by the first
    kernel of the next forward, is reduced on the compute stream.

        compute stream   fwd(k): pool, finalize, [wait td_done(k-1)] logits ... xent
                         bwd(k): head kernel -> record ready(k); streaming pass; column sums
                         all-reduce(att part)                          <- only exposed collective
        comm stream      [wait ready(k)] all-reduce(td part) -> update -> record td_done(k)

    The two waits are the `grad_ready_event` / `td_weights_ready_event` members of `apa_hooks`
    (include/apa.h): `self.hooks` is that struct and has to be handed to every forward / backward call
    of the head explicitly (`cof.attn_pool_fwd(..., hooks=ogs.hooks)`, `cof.attn_pool_bwd(..., hooks=
    ogs.hooks)`, `cof.HeadTrainStep(..., hooks=ogs.hooks)`; through the nn.Module surface:
    `network_fn.head.hooks = ogs.hooks`) -- nothing is registered per thread, so the
    schedule also holds when autograd runs the backward on its engine thread.  Each stream drives its own communicator: two collectives of one communicator
    must not be in flight at the same time.  Every rank enqueues them in the same order.  Same sums
    as `sum_clone_gradients` (model_deploy.py:421-451), only the schedule differs."""

    def __init__(self, bucket_att: torch.Tensor, bucket_td: torch.Tensor, comm_att, comm_td, device, runtime=None,
                 clip_td=None, clip_att=None):
        """`runtime` (default: HIP through torch.cuda): where streams, events and the `apa_hooks` struct come from --
        injectable so that the schedule's bookkeeping (which communicator on which stream, the two event
        hand-overs, the order of the collectives) runs on two CPU ranks against stand-ins
        (tests/test_multi_rank_dryrun_cpu.py); see HipRuntime for the interface.
        `clip_td` / `clip_att` (TRAIN.CLIP_GRADIENTS > 0): GradientClipper objects over the td part (td_weights,
        td_biases) and the att part of this rank's bucket.  Clipping is per variable and the two parts hold disjoint
        variables, so each part is clipped on its own stream right before its all-reduce: the td part on the
        communication stream after `ready`, the att part on the compute stream."""
        rt = HipRuntime(device) if runtime is None else runtime
        self.clip_td, self.clip_att = clip_td, clip_att
        for c in (clip_td, clip_att):              # marshalled here, not lazily inside the first step
            if c is not None:
                c.bind()
        self.runtime = rt
        self.bucket_att, self.bucket_td = bucket_att, bucket_td
        self.comm_att, self.comm_td = comm_att, comm_td
        self.compute = rt.current_stream()
        self.side = rt.new_stream()
        self.ready, self.td_done = rt.new_event(), rt.new_event()
        self.ready.record(self.compute)          # materialise the handles; both start out signalled
        self.td_done.record(self.compute)
        rt.synchronize()
        self.hooks = rt.make_hooks(grad_ready=self.ready, td_weights_ready=self.td_done)

    def after_backward(self, update_td=None, update_att=None) -> None:
        """Call right after `attn_pool_bwd` was enqueued on the compute stream.  `update_td()` /
        `update_att()`: optional optimizer launches for the two parts; `update_td` runs with the
        communication stream current."""
        self.side.wait_event(self.ready)
        if self.clip_td is not None:
            with self.runtime.stream(self.side):
                self.clip_td.apply()
        self.comm_td.all_reduce_(self.bucket_td, self.side)
        if update_td is not None:
            with self.runtime.stream(self.side):
                update_td()
        self.td_done.record(self.side)
        if self.clip_att is not None:
            self.clip_att.apply()
        self.comm_att.all_reduce_(self.bucket_att, self.compute)
        if update_att is not None:
            update_att()

    def close(self) -> None:
        self.side.synchronize()


def add_regularization_gradient(bucket: GradientBucket, params: Dict[str, torch.Tensor],
                                weight_decay: float, regularized: Sequence[str]) -> None:
    """d/dW [ wd * 0.5 * |W|^2 ] = wd * W, added ONCE after the reduce -- equivalent to the
    reference adding the regularisation loss to clone 0 only (model_deploy.py:294-309).  Not with gradient
    clipping: the clipper adds wd * w on clone 0 BEFORE the norm (GradientClipper)."""
    if weight_decay == 0.0:
        return
    if any(c.active and c.covers(bucket.flat) for c in list(_CLIPPERS)):
        raise ValueError('add_regularization_gradient: TRAIN.CLIP_GRADIENTS > 0 -- the GradientClipper of this bucket '
                         'already adds wd * w on the chief clone, inside the clip')
    for name in regularized:
        bucket.views[name].add_(params[name].detach().to(bucket.flat.dtype), alpha=weight_decay)


class GradientClipper:
    """TRAIN.CLIP_GRADIENTS (src/train.py:507-513 -> model_deploy.py:297-304): every clone's gradient is clipped per
    VARIABLE with tf.clip_by_norm (slim.learning.clip_gradient_norms; not a global norm) before the clones are summed
    and before ITER_SIZE accumulation.  TF 1.x's clip_by_norm, kept in its own order:

        out = (t * c) * min(rsqrt(sum(t * t)), 1 / c)        t = this clone's gradient of the variable

    Clipping is not linear, so the regulariser's gradient wd * w -- part of clone 0's loss in the reference -- has to
    be inside t on the chief clone: the clipper adds it there (for the names in `regularized`), and the optimiser must
    not fold it in again (configure_optimizer drops its weight decay when CLIP_GRADIENTS > 0).  The 1/num_clones
    loss scale must already be in the gradient (pass `grad_scale` to the loss kernels, not to `opt.step`).

    `grads`: a GradientBucket, a dict / list of (name, fp32 tensor), or None = the `.grad` tensors of `params` (the
    backbone under torch autograd, channels-last conv weights included; a parameter whose `.grad` is None is
    skipped).  On a GPU the segment table is marshalled by `bind()` -- one host sync; call it once after the first
    backward, or let the first `apply()` do it -- and `apply()` is then two launches, no sync, capturable.  The table
    names the `.grad` tensors themselves, so keep them resident: `optimizer.zero_grad(set_to_none=False)`.  If they
    were replaced (set_to_none=True), `apply()` re-binds (counted in `self.rebinds`) -- and refuses to do so inside a
    graph capture.  `absent`: names whose gradient the producer never writes (FusedHeadStep's
    pruned PoseLogits convs on cfg 002): taken as zero -- tf.gradients gives None there, so such a variable gets
    clip(wd * w) on the chief clone and 0 elsewhere.  `apply()` works in place on the current stream: on a GPU one
    `cof.BoundClipByNorm` (two launches, no host sync, capturable), on CPU tensors the equivalent torch expressions.
    Order in a micro-step: backward (including FusedHeadStep's upstream rescale) -> apply() -> GradientAccumulator /
    all-reduce -> optimiser step.  With CLIP_GRADIENTS <= 0 `apply()` does nothing."""

    def __init__(self, cfg, config: DeploymentConfig, grads, params: Dict[str, torch.Tensor],
                 regularized: Sequence[str] = (), absent: Sequence[str] = (), clip: Optional[float] = None,
                 weight_decay: Optional[float] = None):
        self.clip = float(cfg.TRAIN.CLIP_GRADIENTS) if clip is None else float(clip)
        wd = float(cfg.TRAIN.WEIGHT_DECAY) if weight_decay is None else float(weight_decay)
        self.config = config
        self.params = params
        reg, ab = set(regularized), set(absent)
        self._from_params = grads is None
        if grads is None:
            named = [(n, None) for n in params]
        elif isinstance(grads, GradientBucket):
            named = [(n, grads.views[n]) for n in grads.names]
        elif isinstance(grads, dict):
            named = list(grads.items())
        else:
            named = list(grads)
        self.names = [n for n, _ in named]
        self._grads = [g for _, g in named]
        self._wd = {n: (wd if (config.is_chief() and n in reg) else 0.0) for n in self.names}
        self._absent = {n: n in ab for n in self.names}
        self._bound = None
        self._key = None
        self.rebinds = 0
        _CLIPPERS.add(self)

    @property
    def active(self) -> bool:
        return self.clip > 0.0

    def covers(self, t: torch.Tensor) -> bool:
        """does this clipper work on (part of) the memory of `t`?  (add_regularization_gradient's guard)"""
        base = t.untyped_storage().data_ptr()
        return any(g is not None and g.untyped_storage().data_ptr() == base for g in self._grads)

    def bind(self) -> None:
        """Marshal the segment table of the current gradient tensors now (GPU only; one host sync).  A no-op when
        clipping is off, on CPU tensors, or while no `.grad` exists yet."""
        if not self.active:
            return
        named = self._current()
        if not named or not named[0][1].is_cuda:
            return
        key = tuple((n, g.data_ptr(), self.params[n].data_ptr()) for n, g in named)    # + the weights of wd * w
        if self._bound is not None and key == self._key:
            return
        if self._bound is not None:
            self.rebinds += 1
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('GradientClipper: the gradient tensors changed (or were never bound) inside a graph '
                               'capture -- bind() before capturing and keep the .grad tensors resident '
                               '(zero_grad(set_to_none=False))')
        from .custom_ops import custom_ops_factory as cof
        self._bound = cof.BoundClipByNorm([g for _, g in named],
                                          weights=[self.params[n].data for n, _ in named],
                                          wd=[self._wd[n] for n, _ in named],
                                          absent=[self._absent[n] for n, _ in named])
        self._key = key

    def weight_decay_of(self, name: str) -> float:
        return self._wd[name]

    def _current(self):
        if not self._from_params:
            return list(zip(self.names, self._grads))
        return [(n, self.params[n].grad) for n in self.names if self.params[n].grad is not None]

    def apply(self) -> None:
        if not self.active:
            return
        named = self._current()
        if not named:
            return
        if named[0][1].is_cuda:
            self.bind()
            self._bound.run(self.clip)
            return
        c = self.clip
        with torch.no_grad():
            for n, g in named:
                t = torch.zeros_like(g) if self._absent[n] else g.clone()
                if self._wd[n] != 0.0:
                    t = t + self._wd[n] * self.params[n].data.reshape(g.shape).to(g.dtype)
                inv = torch.rsqrt((t * t).sum())
                g.copy_((t * c) * torch.minimum(inv, torch.tensor(1.0 / c, dtype=g.dtype)))


_CLIPPERS = weakref.WeakSet()      # every GradientClipper alive (add_regularization_gradient's guard)


class GradientAccumulator:
    """TRAIN.ITER_SIZE semantics (src/train.py:529-566): micro-step gradients are summed into an
    accumulator, and only the last micro-step triggers reduce + apply; the accumulated gradient
    is divided by ITER_SIZE like train.py:556-560."""

    def __init__(self, bucket: GradientBucket, iter_size: int):
        self.bucket = bucket
        self.iter_size = max(1, int(iter_size))
        self.acc = torch.zeros_like(bucket.flat) if self.iter_size > 1 else None
        self._divisor = torch.full((), float(self.iter_size), dtype=bucket.flat.dtype, device=bucket.flat.device)
        self.micro = 0

    def step(self) -> bool:
        """Call after each micro-batch's backward.  Returns True when the bucket now holds the
        gradient to reduce and apply."""
        if self.iter_size == 1:
            return True
        self.acc.add_(self.bucket.flat)
        self.micro += 1
        if self.micro < self.iter_size:
            return False
        # `ref_grad / float(ITER_SIZE)` (src/train.py:560-563) is a true division.  torch divides a GPU tensor by
        # a python scalar as a multiplication by its reciprocal (an ulp off for ITER_SIZE = 3, 5, ...): divide by
        # a 0-dim tensor on the bucket's device instead, which takes the element-wise IEEE path
        torch.div(self.acc, self._divisor, out=self.bucket.flat)
        self.acc.zero_()
        self.micro = 0
        return True


class OverlappedMicroBatches:
    """The TRAIN.ITER_SIZE micro-batches of ONE update in flight side by side (round 3).

    The reference recipe for cfg 002 / 003 is `ITER_SIZE: 2` (experiments/002_MPII_ResNet_withAttention.yaml;
    src/train.py:529-566): two independent micro-batches, their gradients summed, one apply.  At the reference's
    per-GPU batch the head step is two HBM-streaming passes (~31 us) plus a chain of five latency-bound kernels
    (finalize -> logits -> xent -> backward head ... column sums, ~22 us on a handful of CUs: 42 % of the step,
    DESIGN.md section 3.3).  Here micro-batch i runs on its own HIP stream with its own workspace, dropout counter
    and gradient bucket; the compute stream then forms bucket = (g0 + g1 + ...) / ITER_SIZE in one launch.

    What it buys, measured on MI355X (N = 32 per micro-batch, fp32, bench.py extra.cfg002_train_iter_size): the
    lanes run nearly in lockstep -- pooling beside pooling, chain beside chain, backward beside backward (device
    timeline from the dispatch events) -- so what overlaps is one chain with the other:
    99-102 us per update against 109-110 us back to back (-8 %), per-image step fraction 0.354 -> 0.385.  The
    hoped-for pairing "streaming pass of B underneath the chain of A" (forced with a cross-stream event after A's
    pooling pass, eagerly and inside a hipGraph) measured WORSE (110-118 us): the chain kernels are bound by
    memory latency, and beside a kernel that saturates HBM their loads take about twice as long, while two
    event operations per lane cost the host 12 us.  That variant was removed again.  On this chip the way to
    amortise the chain is a larger pass, not concurrency: the same two micro-batches as ONE call over 2N images
    (memory is no constraint with 288 GB) take 80 us, 0.48 of the HBM roofline (bench.py reports it next to these figures).

    Same kernels, same inputs, a fixed summation order: the result is bit-identical to running the micro-batches
    one after the other through `GradientAccumulator` (tests/test_head_gpu.py).  `steppers[i]` is the
    `cof.HeadTrainStep` of lane i (its gradient views must point into `lane_buckets[i]`)."""

    def __init__(self, steppers: Sequence, lane_buckets: Sequence[torch.Tensor], out_bucket: torch.Tensor, device):
        from .custom_ops import custom_ops_factory as cof
        assert len(steppers) == len(lane_buckets) >= 1
        self._cof = cof
        self.steppers = list(steppers)
        self.lane_buckets = list(lane_buckets)
        self.out = out_bucket
        self.main = torch.cuda.current_stream(device)
        self.sides = [torch.cuda.Stream(device) for _ in steppers[1:]]
        self.start = torch.cuda.Event()
        self.done = [torch.cuda.Event() for _ in steppers[1:]]

    def run(self, steppers: Optional[Sequence] = None) -> None:
        """Enqueue one update's worth of micro-batches.  `steppers` overrides the lanes' steppers for this call
        (e.g. rotating input buffers); every lane keeps its own stream."""
        st = self.steppers if steppers is None else steppers
        self.start.record(self.main)                 # the lanes start after whatever precedes on the compute stream
        for side in self.sides:                      # (the optimizer update of the previous iteration)
            side.wait_event(self.start)
        st[0].run(stream=self.main.cuda_stream)
        for s_, side, ev in zip(st[1:], self.sides, self.done):
            s_.run(stream=side.cuda_stream)
            ev.record(side)
        for ev in self.done:
            self.main.wait_event(ev)
        self._cof.accumulate_gradients(self.out, self.lane_buckets, divisor=float(len(st)),
                                       stream=self.main.cuda_stream)

    def run_sequential(self, steppers: Optional[Sequence] = None) -> None:
        """The same update with the micro-batches one after the other on the compute stream (the schedule of
        `GradientAccumulator`): the yardstick the overlapped form is measured and checked against."""
        st = self.steppers if steppers is None else steppers
        for s_ in st:
            s_.run(stream=self.main.cuda_stream)
        self._cof.accumulate_gradients(self.out, self.lane_buckets, divisor=float(len(st)),
                                       stream=self.main.cuda_stream)

    def close(self) -> None:
        for side in self.sides:
            side.synchronize()


class StaleOperandError(RuntimeError):
    """A head parameter was written behind the optimiser's back (load_state_dict, a checkpoint restore, any in-place
    op on the Parameter, a new storage: `p.data = t`, `module.to()`) while a bf16 shadow / operand image of it is in
    use: the next step would run on the OLD weights.  Call `optimizer.refresh_shadows()` (FusedHeadStep:
    `refresh_operands()`), or build the optimiser with `stale='refresh'`."""


class OperandCopy(NamedTuple):
    """One entry of an optimiser's registry of operand copies (`operand_copies()`)."""
    name: str                       # the parameter it copies
    kind: str                       # SHADOW, LAUNCH_IMAGE or OWNER_IMAGE
    target: object                  # the bf16 tensor (SHADOW) or the cof.ApaWeightImage map (the images)
    owner: object                   # what the copy's memory lives in: kept alive until detach_weight_images(owner)
    refresh: Callable[[], None]     # rebuilds the copy from the current weights


SHADOW = 'shadow'                   # bf16 copy of a whole parameter, rewritten by the update launch (CPU: after it)
LAUNCH_IMAGE = 'launch'             # operand image whose map rides in the update launch (momentum, <= 3 per parameter)
OWNER_IMAGE = 'owner'               # operand image rebuilt by its `refresh` after each update


class _FusedOptimizer:
    """What the three fused optimisers share: the parameters and the flat bucket, `wd` (one L2 coefficient per bucket
    segment, the slim regulariser's gradient `wd * w` folded into the update), `clipping`, the registry of operand
    copies, the staleness guard and `step()`.  A subclass supplies its hyper-parameters, slot buffers (`_slots`), the
    GPU launch (`_bind` / `_launch`) and the CPU arithmetic (`_cpu_update`).

    Operand copies: bf16 shadows of whole parameters and "images" (affine scatter maps into a step's workspace,
    `cof.ApaWeightImage`), one `OperandCopy` each.  Every entry carries its OWNER -- the object whose memory it
    writes -- so the block cannot return to the allocator while the launch still scatters into it, and
    `detach_weight_images(owner)` drops it again.

    Freshness: the fused launches write through raw pointers / `.data` and never bump `Parameter._version`; anything
    else that writes a weight does, and a new storage changes `data_ptr()`.  `(p._version, p.data_ptr())` of every
    parameter that has a copy is recorded whenever its copies are (re)written and compared in `check_fresh()` (called
    by `step()` and by `FusedHeadStep` before each head step; a host-side tuple compare): `stale='raise'` (default) ->
    StaleOperandError, `'refresh'` -> the copies are rebuilt on the spot.  The marshalled launch is rebuilt whenever
    the copy set, a weight's `data_ptr()`, the bucket, a slot buffer or `tuple(wd)` changes."""

    fused_images = False        # does the launch carry image maps?  (otherwise every image is an OWNER_IMAGE)
    clipping = False            # TRAIN.CLIP_GRADIENTS > 0 (configure_optimizer): the L2 term is the clipper's, and
                                # the 1/num_clones scale must be inside the gradient before the clip

    def __init__(self, params: Dict[str, torch.Tensor], bucket: GradientBucket, lr: float, weight_decay: float = 0.0,
                 regularized: Sequence[str] = (), bf16_shadows: Optional[Dict[str, torch.Tensor]] = None,
                 stale: str = 'raise', trainable: Optional[Sequence[str]] = None):
        """`bf16_shadows` {name: bf16 tensor}: operand copies the bf16 MFMA products read (the pose head's W1 for
        `cof.PoseAttnTrainStep(w1_bf16=...)`), rewritten from the updated weights by the update's own launch.
        `trainable` (TRAIN.TRAINABLE_SCOPES, configure_optimizer): the bucket names the optimiser trains, default
        all.  A segment outside it is FROZEN: never written, never decayed, no slot (`slot_names()`), whatever its
        gradient window holds.  CPU buckets only -- on a GPU build the bucket over the trained variables
        (FusedHeadStep does), so the fused launch walks nothing it must not touch."""
        if stale not in ('raise', 'refresh'):
            raise ValueError("stale: 'raise' or 'refresh'")
        self.stale = stale
        self.params = params
        self.bucket = bucket
        self.lr = lr
        reg = set(regularized)
        self.frozen = frozenset(bucket.names) - frozenset(bucket.names if trainable is None else trainable)
        if self.frozen and bucket.flat.is_cuda:
            raise ValueError('frozen variables %s in a GPU bucket: build the bucket over the trained variables '
                             '(deploy.variables_to_train)' % ', '.join(sorted(self.frozen)))
        self.wd = [weight_decay if (n in reg and n not in self.frozen) else 0.0 for n in bucket.names]
        self.acc = torch.zeros_like(bucket.flat)
        self._copies = []           # [OperandCopy]
        self._watched = ()          # the names that have copies
        self._seen = {}             # watched name -> (p._version, p.data_ptr()) when its copies were last written
        self._bound = self._bound_key = None        # the marshalled launch and the fingerprint it was built for
        for name, t in (bf16_shadows or {}).items():
            if name not in params or t.dtype != torch.bfloat16 or t.numel() != params[name].numel():
                raise ValueError('bf16 shadow %r: a bfloat16 tensor with the element count of that parameter' % name)
            self._add([OperandCopy(name, SHADOW, t, t, self._shadow_writer(name, t))])
        self.refresh_shadows()          # a shadow is current from the start, not only after the first update

    def _shadow_writer(self, name, t):
        def write():
            with torch.no_grad():
                t.copy_(self.params[name].data.reshape(t.shape))
        return write

    # -- registry of operand copies ------------------------------------------------------------------------------
    def operand_copies(self) -> Tuple[OperandCopy, ...]:
        """every bf16 shadow and operand image this optimiser keeps current (read-only)"""
        return tuple(self._copies)

    def attach_weight_images(self, step, names: Dict[str, str]) -> None:
        """Keep the per-class head's operand images current: `step` is a cof.HeadTrainStep(..., weight_images=True)
        (or anything with `.weight_image_maps` and `.refresh_weight_images()`), `names` maps the roles 'Wa' / 'ba' /
        'Wt' / 'bt' to parameter names of the bucket.  Several steps (micro-batch lanes, rotating buffer sets) may be
        attached; at most three images per parameter fit the fused launch, further ones (and every image of an
        optimiser whose launch carries none) are rebuilt by their step's own refresh launch after the update.  A role
        missing from `names` (a variable frozen by TRAIN.TRAINABLE_SCOPES) keeps the image its step built.  The
        optimiser keeps `step` (hence its workspace) alive until `detach_weight_images(step)`."""
        maps = [(names[role], m) for role, m in step.weight_image_maps if role in names]
        count = collections.Counter(c.name for c in self._copies if c.kind == LAUNCH_IMAGE)
        count.update(n for n, _ in maps)
        kind = LAUNCH_IMAGE if self.fused_images and all(count[n] <= 3 for n, _ in maps) else OWNER_IMAGE
        refresh = step.refresh_weight_images
        self._add([OperandCopy(n, kind, m, step, refresh) for n, m in maps])

    def add_image(self, name: str, image_map, refresh=None, owner=None) -> None:
        """One more operand image of parameter `name` (a cof.ApaWeightImage, e.g. cof.pose_w2t_image_map: the bf16
        transposed copy of the pose head's W2), rewritten by this optimiser's launch where it can.  `refresh()`
        (required) rebuilds it from the weights: after each update where the launch cannot (more than three images
        on one parameter; the adaptive optimisers) and in `refresh_images()`; `owner`: the tensor / object
        `image_map.dst` points into (kept alive here)."""
        if refresh is None:
            raise ValueError('add_image(%r): refresh= is required -- it rebuilds the image after the weights were '
                             'written outside the optimiser' % name)
        fits = self.fused_images and sum(c.kind == LAUNCH_IMAGE and c.name == name for c in self._copies) < 3
        self._add([OperandCopy(name, LAUNCH_IMAGE if fits else OWNER_IMAGE, image_map, owner, refresh)])

    def detach_weight_images(self, owner) -> None:
        """Forget every copy that lives in `owner`'s memory (a step that is dropped or re-bound): the launch stops
        scattering into it, the reference that kept it alive is released, and a name left without copies is no
        longer watched."""
        self._copies = [c for c in self._copies if c.owner is not owner]
        self._changed()

    def _add(self, copies) -> None:
        for c in copies:
            if c.name not in self.bucket.views:
                raise ValueError('%r is not a parameter of the bucket' % c.name)
        self._copies += copies
        self._changed()
        self._note_written({c.name for c in copies})

    def _changed(self) -> None:
        self._bound = None
        self._watched = tuple(dict.fromkeys(c.name for c in self._copies))
        self._seen = {n: self._seen[n] for n in self._watched if n in self._seen}

    def _rewrite(self, kinds) -> None:
        """run the refresh of every copy of `kinds`, each callable once"""
        for r in {id(c.refresh): c.refresh for c in self._copies if c.kind in kinds}.values():
            r()

    def _refresh(self, kinds) -> None:
        self._rewrite(kinds)
        self._note_written(n for n in self._watched if all(c.kind in kinds for c in self._copies if c.name == n))

    def refresh_images(self) -> None:
        """Rebuild EVERY operand image from the current weights (each owner's own refresh launch)."""
        self._refresh((LAUNCH_IMAGE, OWNER_IMAGE))

    def refresh_shadows(self) -> None:
        """Rewrite every bf16 operand copy AND every operand image from its parameter: at construction, and after
        the weights were changed behind the optimiser's back (load_state_dict, a checkpoint restore)."""
        self._refresh((SHADOW, LAUNCH_IMAGE, OWNER_IMAGE))

    # -- staleness guard -----------------------------------------------------------------------------------------
    def _fingerprint(self, name):
        p = self.params[name]
        return p._version, p.data_ptr()

    def _note_written(self, names) -> None:
        for n in names:
            self._seen[n] = self._fingerprint(n)

    def stale_names(self):
        return [n for n in self._watched if self._fingerprint(n) != self._seen.get(n)]

    def check_fresh(self) -> None:
        """Compare `(p._version, p.data_ptr())` of every parameter with a shadow / image against the value recorded
        when the copies were last written (a host-side tuple compare, no device work)."""
        bad = self.stale_names()
        if not bad:
            return
        if self.stale == 'refresh':
            self.refresh_shadows()
            return
        raise StaleOperandError(
            '%s written outside the optimiser since their bf16 shadow / operand images were built: the head would '
            'run on the old weights -- call refresh_shadows() after load_state_dict / a restore' % ', '.join(bad))

    # -- the update ----------------------------------------------------------------------------------------------
    def _slots(self):
        return [self.acc]

    def _launch_key(self):
        p = self.params
        return ([p[n].data_ptr() for n in self.bucket.names], self.bucket.flat.data_ptr(),
                [s.data_ptr() for s in self._slots()], tuple(self.wd))

    def slot_names(self):
        """the bucket names that have optimiser slots: every one but the frozen"""
        return [n for n in self.bucket.names if n not in self.frozen]

    def _segments(self, grad_scale):
        """CPU: (w, g, *slot views) per TRAINED bucket segment, g with the L2 term folded in"""
        o = 0
        slots = self._slots()
        for name, wd in zip(self.bucket.names, self.wd):
            w = self.params[name].data
            n = w.numel()
            if name in self.frozen:
                o += n
                continue
            g = self.bucket.flat[o:o + n].view_as(w) * grad_scale + wd * w
            yield (w, g) + tuple(s[o:o + n].view_as(w) for s in slots)
            o += n

    def step(self, lr: Optional[float] = None, grad_scale: float = 1.0) -> None:
        lr = self.lr if lr is None else lr
        if self.clipping and grad_scale != 1.0:
            raise ValueError('grad_scale %r with TRAIN.CLIP_GRADIENTS > 0: the clone loss scale has to be inside the '
                             'gradient before the clip -- pass it to the loss / head step instead' % grad_scale)
        self.check_fresh()
        if self.bucket.flat.is_cuda:
            key = self._launch_key()
            if self._bound is None or key != self._bound_key:
                ws = [self.params[n].data for n in self.bucket.names]
                shadows = {c.name: c.target for c in self._copies if c.kind == SHADOW}
                sh = [shadows.get(n) for n in self.bucket.names] if shadows else None
                images = [(self.bucket.names.index(c.name), c.target) for c in self._copies if c.kind == LAUNCH_IMAGE]
                self._bound, self._bound_key = self._bind(ws, list(self.wd), sh, images), key
            self._launch(lr, grad_scale)
            self._rewrite((OWNER_IMAGE,))
        else:
            self._cpu_update(lr, grad_scale)
            self._rewrite((SHADOW, OWNER_IMAGE))


class MomentumSGD(_FusedOptimizer):
    """tf.train.MomentumOptimizer(lr, momentum) (src/train.py:90-94): acc = m*acc + g;
    w -= lr*acc (no Nesterov, no dampening) on the flat bucket layout, with the slim L2
    regulariser's gradient `wd * w` folded in for the names in `regularized`
    (resnet_utils.py:241: conv weights only).  On a GPU the whole update is ONE fused HIP launch
    (`cof.BoundMomentumSGD`), which also rewrites the bf16 shadows and up to three operand images per parameter
    from the updated weights; CPU tensors (the gloo tests) take the equivalent torch expressions.

    The operand copies and their freshness rule are _FusedOptimizer's: a weight written behind the optimiser's back
    -- a bumped `Parameter._version` or a new `data_ptr()` -- raises StaleOperandError in the next `check_fresh()` /
    `step()` (or, `stale='refresh'`, rebuilds every copy); the launch is re-marshalled when a weight's storage, the
    bucket, `acc`, `wd` or the copy set changed."""

    fused_images = True

    def __init__(self, params: Dict[str, torch.Tensor], bucket: GradientBucket, lr: float,
                 momentum: float = 0.9, weight_decay: float = 0.0, regularized: Sequence[str] = (),
                 bf16_shadows: Optional[Dict[str, torch.Tensor]] = None, stale: str = 'raise',
                 trainable: Optional[Sequence[str]] = None):
        super().__init__(params, bucket, lr, weight_decay, regularized, bf16_shadows, stale, trainable)
        self.momentum = momentum

    def _bind(self, ws, wd, sh, images):
        from .custom_ops import custom_ops_factory as cof
        return cof.BoundMomentumSGD(ws, wd, self.bucket.flat, self.acc, shadows=sh, images=images or None)

    def _launch(self, lr, grad_scale):
        self._bound.run(lr, self.momentum, grad_scale)

    def _cpu_update(self, lr, grad_scale):
        for w, g, a in self._segments(grad_scale):
            a.mul_(self.momentum).add_(g)
            w.add_(a, alpha=-lr)


class Adam(_FusedOptimizer):
    """tf.train.AdamOptimizer(lr, beta1, beta2, epsilon) (src/train.py:84-89; TF 1.1 training/adam.py):
    lr_t = lr sqrt(1 - b2^t)/(1 - b1^t);  m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2);  w -= lr_t m/(sqrt(v) + eps).
    Note the reference's epsilon: cfg.TRAIN.OPT_EPSILON defaults to 1.0 (src/config.py:94).  One fused HIP launch
    (`apa_adam_step`, which carries no image maps: an attached owner rebuilds its images after each update) on a GPU;
    the torch expressions on CPU tensors.  `acc` is m, `slot2` is v."""

    def __init__(self, params, bucket, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.0, regularized=(),
                 bf16_shadows=None, stale='raise', trainable=None):
        super().__init__(params, bucket, lr, weight_decay, regularized, bf16_shadows, stale, trainable)
        self.slot2 = torch.zeros_like(bucket.flat)
        self.beta1, self.beta2, self.epsilon, self.t = float(beta1), float(beta2), float(epsilon), 0

    def _slots(self):
        return [self.acc, self.slot2]

    def _bind(self, ws, wd, sh, images):
        from .custom_ops import custom_ops_factory as cof
        return functools.partial(cof.adam_step, ws, wd, self.bucket.flat, self.acc, self.slot2, shadows=sh)

    def _launch(self, lr, grad_scale):
        self.t += 1
        self._bound(lr, self.t, self.beta1, self.beta2, self.epsilon, grad_scale)

    def _cpu_update(self, lr, grad_scale):
        self.t += 1
        lr_t = lr * (1.0 - self.beta2 ** self.t) ** 0.5 / (1.0 - self.beta1 ** self.t)
        for w, g, m, v in self._segments(grad_scale):
            m.add_((g - m) * (1.0 - self.beta1))
            v.add_((g * g - v) * (1.0 - self.beta2))
            w.sub_(m * lr_t / (v.sqrt() + self.epsilon))


class RMSProp(_FusedOptimizer):
    """tf.train.RMSPropOptimizer(lr, decay, momentum, epsilon) (src/train.py:95-100; TF 1.1 training/rmsprop.py, not
    centered):  ms += (g^2 - ms)(1 - decay);  mom = momentum mom + lr g / sqrt(ms + eps);  w -= mom;  `ms` starts at
    ONE.  One fused HIP launch (`apa_rmsprop_step`, no image maps) on a GPU.  `acc` is ms, `slot2` is mom."""

    def __init__(self, params, bucket, lr, decay=0.9, momentum=0.0, epsilon=1e-10, weight_decay=0.0, regularized=(),
                 bf16_shadows=None, stale='raise', trainable=None):
        super().__init__(params, bucket, lr, weight_decay, regularized, bf16_shadows, stale, trainable)
        self.slot2 = torch.zeros_like(bucket.flat)
        self.decay, self.momentum, self.epsilon = float(decay), float(momentum), float(epsilon)
        self.acc.fill_(1.0)                                  # rmsprop.py _create_slots: init_rms = ones

    def _slots(self):
        return [self.acc, self.slot2]

    def _bind(self, ws, wd, sh, images):
        from .custom_ops import custom_ops_factory as cof
        return functools.partial(cof.rmsprop_step, ws, wd, self.bucket.flat, self.acc, self.slot2, shadows=sh)

    def _launch(self, lr, grad_scale):
        self._bound(lr, self.decay, self.momentum, self.epsilon, grad_scale)

    def _cpu_update(self, lr, grad_scale):
        for w, g, ms, mom in self._segments(grad_scale):
            ms.add_((g * g - ms) * (1.0 - self.decay))
            mom.mul_(self.momentum).add_(g * lr / (ms + self.epsilon).sqrt())
            w.sub_(mom)


def exponential_decay_lr(base_lr: float, global_step: int, decay_steps: int, decay_rate: float,
                         staircase: bool = True) -> float:
    """tf.train.exponential_decay (src/train.py:50-56): lr * rate^floor(step/decay_steps)."""
    e = global_step / float(decay_steps)
    if staircase:
        e = float(int(e))
    return base_lr * (decay_rate ** e)


def decay_steps(cfg, num_samples_per_epoch: int, num_clones: int) -> int:
    """The step count between two learning-rate drops, src/train.py:42-48: TRAIN.NUM_STEPS_PER_DECAY when it
    is positive, else int(samples / (BATCH_SIZE * clones * ITER_SIZE) * NUM_EPOCHS_PER_DECAY) -- one "step"
    is one parameter update, i.e. ITER_SIZE micro-batches on every clone."""
    if cfg.TRAIN.NUM_STEPS_PER_DECAY > 0:
        return int(cfg.TRAIN.NUM_STEPS_PER_DECAY)
    return int(num_samples_per_epoch / (cfg.TRAIN.BATCH_SIZE * num_clones * cfg.TRAIN.ITER_SIZE)
               * cfg.TRAIN.NUM_EPOCHS_PER_DECAY)


def configure_learning_rate(cfg, num_samples_per_epoch: int, num_clones: int, global_step: int) -> float:
    """_configure_learning_rate (src/train.py:29-69) evaluated at `global_step` (the number of parameter
    updates applied so far).  'exponential' is the staircase decay, 'fixed' the constant rate; the reference's
    'polynomial' branch (power 1, no cycle) is the linear ramp to END_LEARNING_RATE."""
    kind = cfg.TRAIN.LEARNING_RATE_DECAY_TYPE
    if kind == 'exponential':
        return exponential_decay_lr(cfg.TRAIN.LEARNING_RATE, global_step,
                                    decay_steps(cfg, num_samples_per_epoch, num_clones),
                                    cfg.TRAIN.LEARNING_RATE_DECAY_RATE, staircase=True)
    if kind == 'fixed':
        return float(cfg.TRAIN.LEARNING_RATE)
    if kind == 'polynomial':
        n = decay_steps(cfg, num_samples_per_epoch, num_clones)
        t = min(global_step, n) / float(n)
        return (cfg.TRAIN.LEARNING_RATE - cfg.TRAIN.END_LEARNING_RATE) * (1.0 - t) + cfg.TRAIN.END_LEARNING_RATE
    raise ValueError('learning_rate_decay_type [%s] was not recognized' % kind)


def configure_optimizer(cfg, params: Dict[str, torch.Tensor], bucket: GradientBucket, learning_rate: float,
                        regularized: Sequence[str] = (), bf16_shadows: Optional[Dict[str, torch.Tensor]] = None,
                        stale: str = 'raise', tf_names: Optional[Dict[str, str]] = None):
    """_configure_optimizer (src/train.py:72-105): every optimiser the reference can select, each as ONE fused
    launch -- 'momentum' (cfgs 001-003: MomentumOptimizer(lr, TRAIN.MOMENTUM)), 'sgd' (momentum 0), 'adam'
    (TRAIN.ADAM_BETA1 / ADAM_BETA2 / OPT_EPSILON) and 'rmsprop' (TRAIN.RMSPROP_DECAY / MOMENTUM / OPT_EPSILON).  The
    L2 regulariser's gradient (TRAIN.WEIGHT_DECAY on `regularized`) is folded into the same launch.  As in the
    reference, 'rmsprop' reads cfg.TRAIN.RMSPROP_DECAY, a key src/config.py does not define: without it in the
    YAML the reference fails with an AttributeError at this point, and so does this function.
    With TRAIN.CLIP_GRADIENTS > 0 the L2 term is NOT folded in: the GradientClipper adds it on the chief clone, inside
    the clip (model_deploy.py:294-304), and the optimiser refuses a `grad_scale` other than 1 in `step`.
    TRAIN.TRAINABLE_SCOPES (src/train.py:166-181, handed to optimize_clones(var_list=...)): a bucket segment whose TF
    variable name -- `tf_names[name]`, default the bucket name itself -- starts with none of the scopes is frozen:
    no update, no L2 step, no slot (_FusedOptimizer: `trainable`)."""
    scopes = trainable_scopes(cfg)
    tfn = tf_names or {}
    trainable = [n for n in bucket.names if in_trainable_scopes(tfn.get(n, n), scopes)] if scopes else None
    opt = _configure_optimizer(cfg, params, bucket, learning_rate, regularized, bf16_shadows, stale, trainable)
    opt.clipping = float(cfg.TRAIN.CLIP_GRADIENTS) > 0.0
    return opt


def _configure_optimizer(cfg, params, bucket, learning_rate, regularized, bf16_shadows, stale, trainable=None):
    kind = cfg.TRAIN.OPTIMIZER
    wd = 0.0 if float(cfg.TRAIN.CLIP_GRADIENTS) > 0.0 else float(cfg.TRAIN.WEIGHT_DECAY)
    if kind == 'adam':
        return Adam(params, bucket, lr=learning_rate, beta1=float(cfg.TRAIN.ADAM_BETA1),
                    beta2=float(cfg.TRAIN.ADAM_BETA2), epsilon=float(cfg.TRAIN.OPT_EPSILON), weight_decay=wd,
                    regularized=regularized, bf16_shadows=bf16_shadows, stale=stale, trainable=trainable)
    if kind == 'rmsprop':
        if 'RMSPROP_DECAY' not in cfg.TRAIN:
            raise AttributeError('RMSPROP_DECAY')            # src/train.py:98 on the reference's own config table
        return RMSProp(params, bucket, lr=learning_rate, decay=float(cfg.TRAIN.RMSPROP_DECAY),
                       momentum=float(cfg.TRAIN.MOMENTUM), epsilon=float(cfg.TRAIN.OPT_EPSILON), weight_decay=wd,
                       regularized=regularized, bf16_shadows=bf16_shadows, stale=stale, trainable=trainable)
    if kind == 'momentum':
        momentum = float(cfg.TRAIN.MOMENTUM)
    elif kind == 'sgd':
        momentum = 0.0
    else:
        raise ValueError('Optimizer [%s] was not recognized' % kind)
    return MomentumSGD(params, bucket, lr=learning_rate, momentum=momentum,
                       weight_decay=wd, regularized=regularized, bf16_shadows=bf16_shadows,
                       stale=stale, trainable=trainable)


class _FusedHeadFunction(torch.autograd.Function):
    """autograd node of FusedHeadStep: the forward IS the whole head step (forward + losses + backward, one host
    call); the backward hands the stored conv5 gradient on to the backbone.  `anchor` is a 0-dim leaf that requires
    grad: with it the node exists (and scales the bucket by the upstream coefficient) also when nothing upstream of
    conv5 is differentiated -- head-only training takes the same path as the end-to-end step."""

    @staticmethod
    def forward(ctx, last_conv, anchor, owner, labels_action, labels_pose, pose_valid):
        total = owner._run(last_conv, labels_action, labels_pose, pose_valid)
        ctx.owner = owner
        ctx.step = owner._step_obj
        ctx.xshape = last_conv.shape
        return total

    @staticmethod
    def backward(ctx, g_total):
        o = ctx.owner
        dX = ctx.step._dX_buf.view(ctx.xshape) if ctx.needs_input_grad[0] else None
        if not o.assume_unit_upstream:        # total entered the differentiated scalar with some coefficient
            if dX is not None:
                dX = dX * g_total.to(dX.dtype)
            for n in o._written:
                o.bucket.views[n].mul_(g_total)
        return dX, None, None, None, None, None


class FusedHeadStep:
    """The reference's per-clone training graph for the head -- `clone_fn` (network_fn -> gen_losses,
    src/train.py:393-422) plus `optimizer.compute_gradients` on the clone loss (model_deploy.py:263) -- as ONE host
    call on the conv5 map: `apa_pose_attn_train_step` for the cfg 003 form (attention from pose_pre_logits, pose L2 +
    softmax cross-entropy), `apa_attn_head_train_step` for the cfg 002 / per-class (HMDB-51) forms (attention from
    the map itself, softmax cross-entropy), `apa_attn_head_train_step_rank` for rank 2..4 on one bottom-up map from
    conv5 (NET.USE_POSE_PRELOGITS_BASED_ATTENTION_RANK; flat batches, softmax cross-entropy: its per-rank variables
    join `params`, `tf_names`, the bucket, `regularized`, the staleness guard and the TRAINABLE_SCOPES split).  The YAML-driven surface stays the reference's: `get_network_fn(...)`
    builds backbone + head, this object drives them.

        fused = deploy.FusedHeadStep(network_fn, cfg)                 # raises ValueError if the configuration
        opt = fused.make_optimizer(lr)                                #   needs the per-op module path
        total, end_points = fused(images, labels_action, labels_pose, pose_valid)
        total.backward()              # conv5's gradient enters the backbone's autograd graph; the head's gradients
        fused.clip()                  # TRAIN.CLIP_GRADIENTS > 0 only (else a no-op): per-variable clip of the bucket
        opt.step()                    # already lie in fused.bucket (the flat all-reduce payload)

    * TRAIN.CLIP_GRADIENTS > 0: `make_optimizer` also builds `fused.clipper` (a GradientClipper over the bucket,
      with wd * w added on the chief clone and the PoseLogits convs of the cfg 002 forms -- never written by the
      step -- taken as a zero gradient), and the optimiser folds no L2 term.  Call `fused.clip()` after
      `total.backward()` (which applies the upstream coefficient to the bucket) and before any ITER_SIZE
      accumulation or all-reduce of the bucket -- the reference clips each clone's gradient of each micro-step.

    * video input `[B,F,H,W,C]` (nets_factory.py:121-125, :354-374): the frames are folded into the batch, the head
      runs per frame and the action loss is taken on the POOLED logits, all inside the one call
      (`apa_attn_head_train_step_clips` / `apa_pose_attn_train_step_clips`: frame pooling, the TemporalAttention conv
      when NET.USE_TEMPORAL_ATT built one, the clip cross-entropy and the gradient at the frame logits in two
      launches).  `labels_action` is [B]; `labels_pose` / `pose_valid` arrive folded or as [B,F,...]; the temporal
      bias is initialised to 1/F at the first clip, as `network_fn` does.  The conv's two parameters are in `params`,
      the bucket and `_written` (the weights regularised, the bias not), so `make_optimizer`, `clip()` and the staleness
      guard cover them.  End points of a clip step: 'Logits' (pooled [B,K]), 'logits_beforePool' [B*F,K],
      'TemporalAttention' [B,F,1,1], and the per-frame ones below.  One frame per clip, or 4-D input, takes the flat
      entry points (no pooling, as in the reference).
    * `total` = sum of the clone's tf.losses entries (each scaled by `loss_scale` = 1 / num_clones,
      model_deploy.py:223-225); the L2 regulariser is the optimiser's (`weight_decay * w` folded into its launch).
      end_points: 'Logits', 'PosePrelogitsBasedAttention', 'PoseLogits' (cfg 003), 'Losses' (the individual values
      in tf.GraphKeys.LOSSES order, detached COPIES; the other end points are views of the bound step's buffers,
      overwritten by the next step of the same batch shape).
    * the head's gradients are written straight into `bucket` views, in the step's own launches; the bf16 operand
      copy of the pose head's W1 is owned by the optimiser (`make_optimizer`: `bf16_shadows`) and rewritten by its
      update launch, so no conversion kernel runs in the step.
    * `assume_unit_upstream=True`: the caller promises `total` enters the differentiated scalar with coefficient 1
      (`(total + other).backward()`), which saves one pass over the [N,H,W,C] gradient; the default multiplies by
      whatever arrives -- conv5's gradient and the bucket alike, with or without a differentiated backbone.
    * TRAIN.TRAINABLE_SCOPES (src/train.py:166-181): `trained` / `frozen` split the head's variables by the prefix
      rule of `variables_to_train`.  The bucket, the optimiser's parameter set and slots, the L2 term and the clipper
      cover the trained ones only; a frozen variable's gradient -- still computed, its products share launches with
      the others -- goes to private scratch, the variable is never written or decayed, and the bf16 W1 shadow, the
      W2^T image and the per-class images of a frozen variable are built once (`make_optimizer`) and only rebuilt by
      the staleness guard / `refresh_operands()`.  `deploy.apply_trainable_scopes(network_fn, cfg)` freezes the
      parameters themselves, backbone included.
    * frozen features (`frozen_features=True`; the default when TRAIN.TRAINABLE_SCOPES is set): a step whose conv5 map
      does not require grad (precomputed features, or no backbone variable in the scopes) is bound without a
      conv5-gradient buffer and runs with APA_FLAG_FROZEN_INPUT: no dX is computed or stored; losses, end points
      and the bucket are bit-identical to the full step.  Without scopes and without the argument every step fills
      its conv5-gradient buffer (`_dX`), whether or not autograd asks for it.
    * one bound step (outputs, workspace, conv5-gradient buffer) is kept per batch shape / dtype (`max_bound_steps`
      most recent: a smaller last batch of an epoch comes back every epoch).  Only the step that is about to run
      has its operand images attached to the optimiser's launch; switching detaches the previous one (the launch
      must not scatter into a workspace nobody vouches for any more) and rebuilds the images of the incoming one.
    * before every step the optimiser's staleness guard runs (`check_fresh`): a weight written behind its back
      (load_state_dict after make_optimizer, a new storage) raises StaleOperandError -- or, with `stale='refresh'`,
      rebuilds the bf16 shadow and every operand image first.  `refresh_operands()` does that by hand."""

    max_bound_steps = 4

    def __init__(self, network_fn, cfg, loss_scale: float = 1.0, assume_unit_upstream: bool = False,
                 stale: str = 'raise', frozen_features: Optional[bool] = None):
        from . import nets_factory
        head = network_fn.head
        if not isinstance(head, nets_factory.AttentionalPoolingHead):
            raise ValueError('FusedHeadStep: the attentional-pooling head only (cfg 001 has no attention op)')
        why = self.unsupported_reason(head, cfg, network_fn)
        if why:
            raise ValueError('FusedHeadStep: ' + why)
        self.network_fn, self.head, self.cfg = network_fn, head, cfg
        self.loss_scale = float(loss_scale)
        self.assume_unit_upstream = bool(assume_unit_upstream)
        self.stale = stale
        # may a step whose conv5 map needs no gradient skip dX?  Default: when the configuration declares frozen
        # training (TRAIN.TRAINABLE_SCOPES is set); without it a head-only step keeps filling `_dX`, as it always has
        self.frozen_features = bool(trainable_scopes(cfg)) if frozen_features is None else bool(frozen_features)
        self.pose_form = not head.single_layer
        names = ['pose_w1', 'pose_b1', 'pose_w2', 'pose_b2', 'att_weights', 'att_biases', 'td_weights', 'td_biases']
        self.params = {n: getattr(head, n) for n in names}
        # cfg 002 forms: the PoseLogits convs are pruned from the data path -- no gradient, but their weights are
        # regularised and decay (the optimiser's L2 term on a zero gradient), as in the reference (tf.gradients
        # reaches them through REGULARIZATION_LOSSES only)
        written = names if self.pose_form else names[4:]
        # rank > 1 (apa_attn_head_train_step_rank): the chain convs 'Conv2d_PrePose_Attn<r>' and the top-down convs
        # 'Conv_<r>' of ranks 1 .. R-1, under the attribute names head.tf_variable_names() lists them by
        self.rank_names = ['%s.%d' % (a, r) for r in range(head.rank - 1)
                           for a in ('att_weights_r', 'att_biases_r', 'td_weights_r', 'td_biases_r')]
        for n in self.rank_names:
            attr, r = n.split('.')
            self.params[n] = getattr(head, attr)[int(r)]
        names = names + self.rank_names
        written = written + self.rank_names
        reg = {id(w) for w in head.regularized_weights()}
        self.tf_names = {n: head.tf_variable_names()[n] for n in names}
        self.temporal = getattr(network_fn, 'temporal', None)
        if self.temporal is not None:       # 'TemporalAttention/Conv/{weights,biases}' (nets_factory.py:362-370)
            self.params['temporal_weights'] = self.temporal['weights']
            self.params['temporal_biases'] = self.temporal['biases']
            names = names + ['temporal_weights', 'temporal_biases']
            written = written + ['temporal_weights', 'temporal_biases']
            reg.add(id(self.temporal['weights']))                # regularised like every conv weight; the bias is not
            self.tf_names.update(temporal_weights='TemporalAttention/Conv/weights',
                                 temporal_biases='TemporalAttention/Conv/biases')
        # TRAIN.TRAINABLE_SCOPES (src/train.py:166-181): the bucket -- hence the all-reduce, the optimiser's parameter
        # set, its slots, the L2 term and the clipper -- covers the trained variables only.  The step still computes
        # a frozen variable's gradient (its products are part of the shared launches) into a private scratch tensor
        scopes = trainable_scopes(cfg)
        self.trained = [n for n in names if in_trainable_scopes(self.tf_names[n], scopes)]
        self.frozen = [n for n in names if n not in self.trained]
        if not self.trained:
            raise ValueError('FusedHeadStep: TRAIN.TRAINABLE_SCOPES %r reaches no head variable'
                             % cfg.TRAIN.TRAINABLE_SCOPES)
        self.bucket = GradientBucket.for_parameters((n, self.params[n]) for n in self.trained)
        self._grad_out = dict(self.bucket.views)
        for n in self.frozen:
            if n in written:
                self._grad_out[n] = torch.empty_like(self.params[n].data, dtype=self.bucket.flat.dtype)
        self._written = [n for n in written if n in self.trained]
        self._absent = [n for n in self.trained if n not in written]
        self.regularized = [n for n in self.trained if id(self.params[n]) in reg]
        self._frozen_copies = []         # [(name, refresh)]: operand copies of frozen variables, built once
        self._frozen_seen = {}
        self._steps = {}                 # key (shape, dtype, preact) -> bound one-call step, most recent last
        self._pose_rows = {}             # (PoseLabelTable id, N) -> (the table, pose labels [N,P*J], valid [N,J]): the buffers a cached cfg 003 step reads
        self._step_obj = None
        self._key = None
        self.w1_shadow = None
        self.w2t_image = None
        self._optimizer = None
        self.clipper = None
        self._anchor = torch.zeros((), requires_grad=True)
        self._want_dx = True
        self._fp8 = False
        self._cb = False
        self._epoch = self._epoch_key = None     # the bound epoch call of train_epoch
        self._video_epoch = self._video_epoch_key = None     # ... and of train_video_epoch
        self.probe_events = None

    @staticmethod
    def unsupported_reason(head, cfg, network_fn=None) -> str:
        from . import nets_factory
        tr = cfg.TRAIN
        if isinstance(head, nets_factory.PoseAttentionLogitsHead):
            return 'the pose-heatmap attention head (USE_POSE_ATTENTION_LOGITS) trains through network_fn and autograd'
        if not head.is_training:
            return 'a training-mode head is required'
        if head.with_pose_feat or head.want_topdown:
            return '..._WITH_POSE_FEAT and the TopDownAttention dump run through the per-op module'
        if head.rank != 1:
            # rank 2..APA_RANK_MAX on one bottom-up map computed from conv5: apa_attn_head_train_step_rank
            from .custom_ops import custom_ops_factory as cof
            if head.rank > cof.APA_RANK_MAX:
                return 'rank %d > %d runs through the per-op module' % (head.rank, cof.APA_RANK_MAX)
            if not head.single_layer:
                return 'rank > 1 with attention from pose_pre_logits runs through the per-op module'
            if head.per_class:
                return 'rank > 1 with per-class maps runs through the per-op module'
            if tr.LOSS_FN_ACTION != 'softmax-xentropy':
                return 'rank > 1 with LOSS_FN_ACTION %r (the rank step takes the softmax cross-entropy)' % tr.LOSS_FN_ACTION
        # 'multi-label' / 'multi-label-2' (HICO, Charades; loss.py:88-101): the *_train_step_multilabel entry points
        if tr.LOSS_FN_ACTION not in ('softmax-xentropy', 'multi-label', 'multi-label-2'):
            return 'LOSS_FN_ACTION %r (the one-call steps take the softmax cross-entropy)' % tr.LOSS_FN_ACTION
        if head.single_layer:
            if tr.LOSS_FN_POSE and head.with_pose_logits:
                return 'a pose loss on a head whose attention does not come from the pose head'
        else:
            if head.per_class:
                return 'per-class maps from pose_pre_logits'
            if tr.LOSS_FN_POSE != 'l2' or tr.LOSS_FN_POSE_SAMPLED:
                return 'LOSS_FN_POSE %r / sampled (the cfg 003 step takes the plain pose L2 loss)' % tr.LOSS_FN_POSE
        return ''

    @staticmethod
    def fp8_unsupported_reason(head, network_fn=None, training=True) -> str:
        """why an Fp8Features batch (custom_ops_factory: a cached conv5 map in FP8 E4M3) cannot feed this head; '' when
        it can.  The FP8 arm is the single-layer class-agnostic form on frozen features -- about the batch, not the
        head: `unsupported_reason` does not change."""
        if network_fn is not None and getattr(network_fn, 'backbone', None) is not None:
            return 'a network_fn with a backbone (an FP8 batch IS the cached conv5 map: build it with backbone=None)'
        if not head.single_layer:
            return 'attention from pose_pre_logits (the cfg 003 form)'
        if head.per_class:
            return 'per-class attention maps'
        if head.rank != 1:
            return 'rank %d attention' % head.rank
        if head.with_pose_feat:
            return '..._WITH_POSE_FEAT'
        if head.softmax_att:
            return 'spatial-softmax attention'
        return ''

    @staticmethod
    def cache_unsupported_reason(head, network_fn, batch, multi_label: bool = False) -> str:
        """why `batch` -- an Fp8Features batch, a CachedBatch or a CachedClips -- cannot feed this head; '' when it can.
        An Fp8Features batch, and every head but the single-layer per-class one: `fp8_unsupported_reason`.  The per-class
        head (with identity, ReLU or spatial-softmax attention) is served from a bf16 cache on the fused per-class
        route (K <= 64, C % 256 == 0, C <= 8192: cof.cached_per_class_served), flat or on clips.  The cfg 003 form
        (attention from pose_pre_logits, identity or ReLU) is served from a flat CachedBatch on a bf16 cache where
        pose_cache.cached_pose_served holds (a training head also needs N * P to be a multiple of 8) -- under the softmax
        cross-entropy only: `multi_label` (TRAIN.LOSS_FN_ACTION 'multi-label*', which the two callers pass) is refused by
        name, the cached cfg 003 steps have no sigmoid form."""
        from .custom_ops import custom_ops_factory as cof
        why = FusedHeadStep.fp8_unsupported_reason(head, network_fn)
        if why == 'attention from pose_pre_logits (the cfg 003 form)' and isinstance(batch, cof.CachedBatch) and \
                not isinstance(batch, cof.CachedClips) and not batch.cache.fp8 and batch.dtype == torch.bfloat16:
            from .custom_ops import pose_cache
            plain = not (head.per_class or head.rank != 1 or head.with_pose_feat or head.softmax_att)
            if plain and pose_cache.cached_pose_served(batch, head.pose_w1.shape[1], head.pose_w2.shape[1],
                                                       head.num_classes, train=bool(head.is_training)):
                if multi_label:
                    return ('attention from pose_pre_logits (the cfg 003 form) under a sigmoid action loss (a cache '
                            'feeds this head under the softmax cross-entropy only)')
                return ''
        if why != 'per-class attention maps' or not isinstance(batch, cof.CachedBatch):
            return why
        if head.rank != 1:
            return 'rank %d attention' % head.rank
        if head.with_pose_feat:
            return '..._WITH_POSE_FEAT'
        K, C = int(head.num_classes), int(batch.shape[-1])
        if batch.cache.fp8:
            return 'per-class attention maps from an FP8 cache (the gathered per-class kernels read bf16)'
        if batch.dtype != torch.bfloat16:
            return 'per-class attention maps from a %s cache (the gathered per-class kernels read bf16)' % (
                str(batch.dtype).replace('torch.', ''))
        if not cof.cached_per_class_served(batch, K):
            return ('per-class attention maps with K = %d classes on %d channels (a cache feeds the fused per-class '
                    'route: K <= 64, C %% 256 == 0, C <= 8192)' % (K, C))
        return ''

    @property
    def _dX(self):
        return None if self._step_obj is None else self._step_obj._dX_buf

    def _drop_steps(self) -> None:
        if self._optimizer is not None:
            for st in self._steps.values():
                self._optimizer.detach_weight_images(st)
        self._steps.clear()
        self._step_obj = self._key = None
        self._epoch = self._epoch_key = None
        self._video_epoch = self._video_epoch_key = None

    def make_optimizer(self, learning_rate: float, deploy_config: Optional[DeploymentConfig] = None):
        """deploy.configure_optimizer on the head's parameters (the nn.Parameters themselves: their `_version` feeds
        the staleness guard) and this object's bucket, with the bf16 copy of the pose head's W1 as a shadow of the
        update launch when the cfg 003 step will read one (bf16 features).  With TRAIN.CLIP_GRADIENTS > 0 also
        `self.clipper` (`deploy_config`: this process's clone, default from torch.distributed)."""
        trained = {n: self.params[n] for n in self.trained}
        if float(self.cfg.TRAIN.CLIP_GRADIENTS) > 0.0:
            self.clipper = GradientClipper(self.cfg, deploy_config or DeploymentConfig(), self.bucket,
                                           trained, regularized=self.regularized, absent=self._absent)
            self.clipper.bind()
        shadows = None
        self._drop_steps()                           # re-bind with the shadow / the weight images
        self._frozen_copies = []
        if self.pose_form:
            w1 = self.params['pose_w1']
            shadow = self.w1_shadow = torch.empty(w1.shape, dtype=torch.bfloat16, device=w1.device)
            if 'pose_w1' in trained:
                shadows = {'pose_w1': shadow}
            else:                                    # a frozen W1: the shadow is built once and never rewritten
                self._frozen_copies.append(('pose_w1', lambda: shadow.copy_(w1.data)))
        self._optimizer = configure_optimizer(self.cfg, trained, self.bucket, learning_rate,
                                              regularized=self.regularized, bf16_shadows=shadows, stale=self.stale,
                                              tf_names=self.tf_names)
        w2 = self.params['pose_w2'].data
        if self.pose_form and w2.is_cuda and w2.shape[1] <= 16:
            # the Pl product reads W2^T as a ready-made bf16 image, rewritten by the optimiser's launch as well
            from .custom_ops import custom_ops_factory as cof
            self.w2t_image = cof.pose_w2t_image(w2)
            img, p2 = self.w2t_image, self.params['pose_w2']
            refresh = lambda: img[:w2.shape[1], :w2.shape[0]].copy_(p2.data.t())   # noqa: E731
            if 'pose_w2' in trained:
                self._optimizer.add_image('pose_w2', cof.pose_w2t_image_map(img, w2), owner=img, refresh=refresh)
            else:
                self._frozen_copies.append(('pose_w2', refresh))
        if self.head.per_class:                      # the per-class operand images of the bound step (_select)
            self._frozen_copies += [(n, self._refresh_step_images) for n in self._IMAGE_ROLES.values()
                                    if n in self.frozen]
        self._refresh_frozen_copies()
        return self._optimizer

    # -- operand copies of FROZEN variables: no optimiser launch rewrites them, the staleness guard still sees them
    def _refresh_step_images(self) -> None:
        if self._step_obj is not None and getattr(self._step_obj, 'weight_image_maps', None):
            self._step_obj.refresh_weight_images()

    def _refresh_frozen_copies(self) -> None:
        with torch.no_grad():
            for r in {id(r): r for _, r in self._frozen_copies}.values():
                r()
        self._frozen_seen = {n: (self.params[n]._version, self.params[n].data_ptr()) for n, _ in self._frozen_copies}

    def _check_frozen_fresh(self) -> None:
        bad = [n for n, seen in self._frozen_seen.items()
               if (self.params[n]._version, self.params[n].data_ptr()) != seen]
        if not bad:
            return
        if self.stale == 'refresh':
            self._refresh_frozen_copies()
            return
        raise StaleOperandError(
            '%s (frozen by TRAIN.TRAINABLE_SCOPES) written since their bf16 shadow / operand images were built: the '
            'head would run on the old weights -- call refresh_operands() after load_state_dict / a restore'
            % ', '.join(bad))

    def clip(self) -> None:
        """TRAIN.CLIP_GRADIENTS: clip this clone's gradients in the bucket (see the class docstring for the order);
        nothing to do when clipping is off or `make_optimizer` was not called."""
        if self.clipper is not None:
            self.clipper.apply()

    def refresh_operands(self) -> None:
        """Rebuild the bf16 W1 shadow, the W2^T image and the per-class weight images of the bound step from the
        current weights (after load_state_dict / a checkpoint restore that happened after `make_optimizer`)."""
        if self._optimizer is not None:
            self._optimizer.refresh_shadows()
            self._refresh_frozen_copies()
        elif self._step_obj is not None and getattr(self._step_obj, 'weight_image_maps', None):
            self._step_obj.refresh_weight_images()

    _IMAGE_ROLES = {'Wa': 'att_weights', 'ba': 'att_biases', 'Wt': 'td_weights', 'bt': 'td_biases'}

    def _bind(self, X, labels_action, labels_pose, pose_valid, frames=1):
        from .custom_ops import custom_ops_factory as cof
        head, tr, v = self.head, self.cfg.TRAIN, self._grad_out
        flags = cof.attn_flags(head.softmax_att, head.relu_att, True, self._preact)
        # frozen features (conv5 needs no gradient): no [N,P,C] gradient buffer, the step runs with
        # APA_FLAG_FROZEN_INPUT (a route the library has no arm for falls back to the full step on a scratch buffer)
        dX = torch.empty_like(X) if self._want_dx else None
        p = {n: t.data for n, t in self.params.items()}
        action_wt = float(tr.LOSS_FN_ACTION_WT)
        clip = {}
        if tr.LOSS_FN_ACTION != 'softmax-xentropy':     # the sigmoid losses: weight 1, as loss.gen_losses passes it
            action_wt = 1.0                             # (loss.py:93-101); labels float32 multi-hot [n_loss, K]
            clip = dict(action_loss=tr.LOSS_FN_ACTION)
        if frames > 1:      # a clip batch: frame pooling (and the temporal conv) inside the one call
            clip.update(frames=frames)
            if self.temporal is not None:
                clip.update(temporal=(p['temporal_weights'], p['temporal_biases']),
                            temporal_grads=(v['temporal_weights'], v['temporal_biases']))
        if head.rank > 1:
            # all R maps in one pass over conv5 per direction.  The rank step has no arm without the dX stores: with
            # frozen features conv5's gradient goes to a scratch buffer nobody reads
            R = head.rank
            dX_rank = dX if dX is not None else torch.empty_like(X)
            st = cof.RankHeadTrainStep(
                X, X, p['att_weights'], p['att_biases'],
                [p['td_weights']] + [p['td_weights_r.%d' % r] for r in range(R - 1)],
                [p['td_biases']] + [p['td_biases_r.%d' % r] for r in range(R - 1)],
                [p['att_weights_r.%d' % r] for r in range(R - 1)], [p['att_biases_r.%d' % r] for r in range(R - 1)],
                labels_action,
                (dX_rank, None, v['att_weights'], v['att_biases'],
                 [v['td_weights']] + [v['td_weights_r.%d' % r] for r in range(R - 1)],
                 [v['td_biases']] + [v['td_biases_r.%d' % r] for r in range(R - 1)],
                 [v['att_weights_r.%d' % r] for r in range(R - 1)], [v['att_biases_r.%d' % r] for r in range(R - 1)]),
                flags=flags, keep_prob=head.keep_prob, seed=head.seed, offset=head._step, loss_wt=action_wt,
                grad_scale=self.loss_scale)
        elif self.pose_form:
            shadow = self.w1_shadow if X.dtype == torch.bfloat16 else None
            step_cls = cof.PoseAttnTrainStep
            if self._cb:    # a bf16 feature cache read by index (custom_ops/pose_cache.py): flat softmax batches
                from .custom_ops import pose_cache
                if clip:
                    raise ValueError('FusedHeadStep: a CachedBatch feeds the cfg 003 form under the softmax '
                                     'cross-entropy on flat batches only')
                step_cls = pose_cache.PoseAttnTrainStepCached
            st = step_cls(
                X, (p['pose_w1'], p['pose_b1'], p['pose_w2'], p['pose_b2'], p['att_weights'], p['att_biases'],
                    p['td_weights'], p['td_biases']), labels_action, labels_pose, pose_valid,
                (dX, v['pose_w1'], v['pose_b1'], v['pose_w2'], v['pose_b2'], v['att_weights'], v['att_biases'],
                 v['td_weights'], v['td_biases']), flags=flags, keep_prob=head.keep_prob, seed=head.seed,
                offset=head._step, action_wt=action_wt, pose_wt=float(tr.LOSS_FN_POSE_WT),
                grad_scale=self.loss_scale, w1_bf16=shadow,
                w2t_bf16=self.w2t_image if X.dtype == torch.bfloat16 else None, **clip)
        else:
            st = cof.HeadTrainStep(
                X, X, p['att_weights'], p['att_biases'], p['td_weights'], p['td_biases'], labels_action,
                (dX, None, v['att_weights'], v['att_biases'], v['td_weights'], v['td_biases']), flags=flags,
                keep_prob=head.keep_prob, seed=head.seed, offset=head._step, loss_wt=action_wt,
                grad_scale=self.loss_scale, hooks=head.hooks,
                weight_images=bool(head.per_class and self._optimizer is not None), **clip)
        st._dX_buf = dX
        return st

    def _select(self, key, X, labels_action, labels_pose, pose_valid, frames=1):
        """make the bound step of `key` the current one: at most one step has its operand images attached"""
        prev = self._step_obj
        st = self._steps.pop(key, None)
        cached = st is not None
        if st is None:
            st = self._bind(X, labels_action, labels_pose, pose_valid, frames)
        self._steps[key] = st                            # most recent last
        while len(self._steps) > self.max_bound_steps:
            old_key = next(iter(self._steps))
            old = self._steps.pop(old_key)
            if self._optimizer is not None:
                self._optimizer.detach_weight_images(old)
        if st is not prev and self._optimizer is not None:
            if prev is not None:
                self._optimizer.detach_weight_images(prev)
            if getattr(st, 'weight_image_maps', None):   # per-class maps: rewritten by the optimiser's launch
                if cached:
                    st.refresh_weight_images()           # they went stale while another shape was current
                self._optimizer.attach_weight_images(st, {r: n for r, n in self._IMAGE_ROLES.items() if n in self.trained})
        self._step_obj, self._key = st, key
        return st, cached

    def _run(self, last_conv, labels_action, labels_pose, pose_valid):
        head = self.head
        n, c = last_conv.shape[0], last_conv.shape[-1]
        X = last_conv.flat() if (self._fp8 or self._cb) else last_conv.detach().contiguous().view(n, -1, c)
        if self.pose_form and self._cb and hasattr(labels_pose, 'gather') and hasattr(labels_pose, 'new_batch'):
            # a PoseLabelTable (custom_ops/pose_cache.py): the batch's rows land in buffers the bound step keeps reading
            # (the entry holds the table itself: its id cannot be taken by another object while the entry lives)
            table, tkey = labels_pose, (id(labels_pose), n)
            held = self._pose_rows.pop(tkey, None)
            if held is None or held[0] is not table:
                held = (table,) + tuple(table.new_batch(n))
            self._pose_rows[tkey] = held                     # most recent last
            while len(self._pose_rows) > self.max_bound_steps:
                self._pose_rows.pop(next(iter(self._pose_rows)))
            labels_pose, pose_valid = held[1], held[2]
            table.gather(X.index, labels_pose, pose_valid)   # (ids clamped as the kernels clamp them: three launches)
            labels_pose = labels_pose.view(n, -1, table.J)
        elif self.pose_form:
            J = self.params['pose_w2'].shape[1]
            labels_pose = labels_pose.contiguous().float().view(n, -1, J)
            if pose_valid.dtype == torch.bool:
                pose_valid = pose_valid.to(torch.uint8)
            pose_valid = pose_valid.contiguous()
        frames = self._frames
        if self.temporal is not None:
            if frames > 1 and not self.temporal._bias_initialised:     # 1 / F at the first clip, as network_fn does
                with torch.no_grad():
                    self.temporal['biases'].fill_(1.0 / frames)
                self.temporal._bias_initialised = True
            if frames == 1:                                  # no pooling (nets_factory.py:354): the conv gets no gradient
                self._grad_out['temporal_weights'].zero_()
                self._grad_out['temporal_biases'].zero_()
        if self._optimizer is not None:
            self._optimizer.check_fresh()                # weights written behind the optimiser's back?
            self._check_frozen_fresh()
        # a bound step reads the weights through the pointers it was bound to: a new storage binds a new step
        # (a CachedBatch: one bound step per cache and label source; only the index, and per-batch labels, are re-bound)
        key = (tuple(X.shape), frames, X.dtype, self._preact, self._want_dx,
               tuple(p.data_ptr() for p in self.params.values())) + \
              ((id(X.cache), labels_action is None) if self._cb else ())
        st, cached = self._select(key, X, labels_action, labels_pose, pose_valid, frames)
        if cached and self._cb and self.pose_form:
            st.rebind(index=X.index, labels=labels_action, pose_labels=labels_pose, pose_valid=pose_valid,
                      offset=head._step)
        elif cached and self._cb:
            st.rebind(index=X.index, labels=labels_action, offset=head._step)
        elif cached and self.pose_form:
            st.rebind(X=X, labels=labels_action, pose_labels=labels_pose, pose_valid=pose_valid, offset=head._step)
        elif cached:
            st.rebind(X=X, labels=labels_action, offset=head._step)
        if self.probe_events is not None:                # measurement aid (tools/bench_e2e.py): the call's device time
            self.probe_events[0].record()
        st.run()
        if self.probe_events is not None:
            self.probe_events[1].record()
        head._step += 1                                  # a fresh dropout mask per step
        if self.pose_form:                               # loss.py:70 then :75 -- tf.GraphKeys.LOSSES order
            self._losses = [st.loss_pose[0].clone(), st.loss_action[0].clone()]
            total = self._losses[0] + self._losses[1]
        else:
            self._losses = [st.loss[0].clone()]
            total = self._losses[0].clone()
        if self.loss_scale != 1.0:       # the entry points scale the GRADIENT (grad_scale); the value follows here
            total = total * self.loss_scale
        return total

    def __call__(self, images, labels_action, labels_pose=None, pose_valid=None):
        """`images`: the input batch; an Fp8Features batch (a cached conv5 map in FP8); or a CachedBatch (N images of a
        resident FeatureCache named by index, any of its dtypes: `labels_action=None` reads the cache's own labels
        through the index; under LOSS_FN_ACTION 'multi-label*' `labels_action` is [N,K]); or a CachedClips
        (`FeatureCache.sample_clips`: B clips of a frame cache -- `frames` comes from the batch, `labels_action=None`
        means the batch's own labels / targets, and the end points are those of a 5-D clip batch).  The cached forms
        are frozen by construction (frozen_features=True) and are served under the conditions of
        cache_unsupported_reason (an FP8 batch: fp8_unsupported_reason; a bf16 cache also feeds the per-class head);
        one bound step per (cache, B, F, loss kind)."""
        from .custom_ops.custom_ops_factory import CachedBatch, CachedClips, Fp8Features
        self._frames = 1
        self._cb = isinstance(images, CachedBatch)
        self._fp8 = isinstance(images, Fp8Features)
        if self._fp8 or self._cb:   # a cached conv5 map: frozen by construction, no backbone in front of it
            what = 'an Fp8Features batch' if self._fp8 else 'a CachedBatch'
            why = self.cache_unsupported_reason(self.head, self.network_fn, images,
                                                multi_label=self.cfg.TRAIN.LOSS_FN_ACTION != 'softmax-xentropy')
            if not why and not self.frozen_features:
                why = 'frozen_features=False (a cache has no gradient: build the step with frozen_features=True)'
            if why:
                raise ValueError('FusedHeadStep: %s is not served with %s' % (what, why))
            multi_label = self.cfg.TRAIN.LOSS_FN_ACTION != 'softmax-xentropy'
            if isinstance(images, CachedClips):     # clips sampled from a frame cache: F and the labels ride along
                self._frames = int(images.frames)
                if labels_action is None:
                    labels_action = images.targets if multi_label else images.labels
                    if labels_action is None:
                        raise ValueError('FusedHeadStep: labels_action=None needs a CachedClips with %s '
                                         '(FeatureCache.set_videos)' % ('targets' if multi_label else 'labels'))
            elif self._cb and multi_label and labels_action is None:
                raise ValueError('FusedHeadStep: a CachedBatch under LOSS_FN_ACTION %r needs labels_action [N,K] (the '
                                 'cache\'s own labels are class ids)' % self.cfg.TRAIN.LOSS_FN_ACTION)
        elif images.dim() == 5:                                 # nets_factory.py:121-125: frames fold into the batch
            self._frames = int(images.shape[1])
            images = images.reshape(-1, *images.shape[2:])
        last_conv, self._preact = (images, False) if (self._fp8 or self._cb) else self.network_fn.features(images)
        if last_conv.dim() != 4:
            raise ValueError('FusedHeadStep: [N,H,W,C] (or [B,F,H,W,C]; an Fp8Features batch: [N,H,W,C]) feature maps '
                             'expected')
        if self._frames > 1 and self.head.rank > 1:
            raise ValueError('FusedHeadStep: a clip batch [B,F,H,W,C] with rank > 1 is not served by the one-call rank '
                             'step (frame pooling at rank > 1 runs through the per-op module)')
        if self._preact and not self.head.can_fuse_input_relu(last_conv.dtype):
            last_conv, self._preact = torch.relu(last_conv), False
        if self.pose_form and (labels_pose is None or (pose_valid is None and not hasattr(labels_pose, 'new_batch'))):
            raise ValueError('FusedHeadStep: the cfg 003 form needs labels_pose [N,H,W,J] and pose_valid [N,J]')
        if self.cfg.TRAIN.LOSS_FN_ACTION != 'softmax-xentropy':     # multi-hot labels of any dtype -> float32, once
            labels_action = labels_action.to(torch.float32).contiguous()
        # decided per step: a conv5 map that needs no gradient (frozen / precomputed features) gets none
        self._want_dx = not (self._fp8 or self._cb) and (bool(last_conv.requires_grad) or not self.frozen_features)
        # one autograd node either way: with a differentiated backbone it hands conv5's gradient upstream, without
        # one (head-only training) it still scales the bucket by whatever coefficient `total` is given
        total = _FusedHeadFunction.apply(last_conv, self._anchor, self, labels_action, labels_pose, pose_valid)
        st = self._step_obj
        n, h, w = last_conv.shape[:3]
        # rank > 1: the stacked maps [N,H,W,1,R] (nets_factory.py:271-274)
        att = st.att.view(n, h, w, 1, -1) if self.head.rank > 1 else st.att.view(n, h, w, -1)
        ep = {'Logits': st.logits, 'PosePrelogitsBasedAttention': att,
              'Losses': [l.detach() for l in self._losses]}
        if self.pose_form:
            ep['PoseLogits'] = st.Pl.view(n, h, w, -1)
        if self._frames > 1:                                    # nets_factory.py:354-374
            ep['logits_beforePool'] = st.logits
            ep['Logits'] = st.pooled
            if st.tatt is not None:
                ep['TemporalAttention'] = st.tatt.view(-1, self._frames, 1, 1)
        return total, ep

    def epoch_unsupported_reason(self, cache=None) -> str:
        """why `train_epoch` cannot run this configuration (on this cache); '' when it can.  The epoch call is the flat
        CachedBatch step under the softmax cross-entropy with the fused momentum-SGD update behind every step."""
        tr = self.cfg.TRAIN
        why = self.fp8_unsupported_reason(self.head, self.network_fn)
        if why:
            return why
        if not self.frozen_features:
            return 'frozen_features=False (a cache has no gradient: build the step with frozen_features=True)'
        if tr.LOSS_FN_ACTION != 'softmax-xentropy':
            return 'LOSS_FN_ACTION %r (the epoch call takes the softmax cross-entropy)' % tr.LOSS_FN_ACTION
        if tr.OPTIMIZER not in ('momentum', 'sgd'):
            return 'TRAIN.OPTIMIZER %r (the epoch call runs the momentum / sgd update)' % tr.OPTIMIZER
        if int(tr.ITER_SIZE) != 1:
            return 'TRAIN.ITER_SIZE %d (gradient accumulation over micro-steps)' % int(tr.ITER_SIZE)
        if self.clipper is not None and self.clipper.active:
            return 'TRAIN.CLIP_GRADIENTS > 0 (an active gradient clipper between the step and the update)'
        if self.loss_scale != 1.0:
            return ('more than one clone (loss_scale %r: the gradients of an epoch call are not all-reduced)'
                    % self.loss_scale)
        if self.temporal is not None:
            return 'a TemporalAttention conv (clips are not served by the epoch call)'
        if cache is not None and cache.labels is None:
            return 'a FeatureCache without labels (the epoch reads them through the order)'
        return ''

    def train_epoch(self, cache, batch_size: int, order, lr=None):
        """A whole epoch of frozen-feature training on a resident `FeatureCache` as ONE host call
        (`cof.HeadTrainEpoch`: apa_attn_head_train_epoch_cached): steps = order.numel() / batch_size times the step
        `__call__` runs on `cache.select(order[s*N:(s+1)*N])` (the cache's own labels, a fresh dropout mask per step)
        followed by the update `opt.step()` runs, on this object's bucket and the optimiser's accumulators -- the same
        launches, the same bits.  `order`: int32 on the cache's device (`cache.order(seed, epoch)`, or its first
        steps * batch_size ids).  `lr`: one learning rate per step (e.g. `configure_learning_rate` per global step), or
        None for the optimiser's own.  Needs `make_optimizer()` first.  The staleness guards run once, in front; the
        head's step counter advances by `steps`.  Returns the loss log [steps, 1 + batch_size] (row s: the mean and
        the per-example losses of step s) as a device tensor -- nothing synchronises.  Served: what a flat CachedBatch
        is served with, under the softmax cross-entropy, TRAIN.OPTIMIZER momentum / sgd, ITER_SIZE 1, no active
        clipper, one clone; anything else is a ValueError that names the reason."""
        from .custom_ops import custom_ops_factory as cof
        if self._optimizer is None:
            raise ValueError('FusedHeadStep.train_epoch: make_optimizer() first (the epoch call runs its update)')
        why = self.epoch_unsupported_reason(cache)
        if why:
            raise ValueError('FusedHeadStep.train_epoch: an epoch call is not served with %s' % why)
        opt, head = self._optimizer, self.head
        opt.check_fresh()                                # weights written behind the optimiser's back?
        self._check_frozen_fresh()
        if opt.operand_copies():
            raise ValueError('FusedHeadStep.train_epoch: an epoch call is not served with operand copies attached to '
                             'the optimiser (%s): its update rewrites none' % ', '.join(opt._watched))
        N = int(batch_size)
        count = int(order.numel())
        if N < 1 or count < N or count % N:
            raise ValueError('FusedHeadStep.train_epoch: order holds %d ids, not a whole number of batches of %d'
                             % (count, N))
        steps = count // N
        lrs = [float(opt.lr)] * steps if lr is None else [float(v) for v in lr]
        if len(lrs) != steps:
            raise ValueError('FusedHeadStep.train_epoch: one learning rate per step expected (%d for %d steps)'
                             % (len(lrs), steps))
        p, v = {n: t.data for n, t in self.params.items()}, self._grad_out
        key = (id(cache), N, tuple(t.data_ptr() for t in p.values()), self.bucket.flat.data_ptr(), opt.acc.data_ptr(),
               tuple(opt.wd), float(opt.momentum))
        if self._epoch is None or self._epoch_key != key or self._epoch.steps < steps:
            self._epoch = cof.HeadTrainEpoch(
                cache, N, p['att_weights'], p['att_biases'], p['td_weights'], p['td_biases'],
                (v['att_weights'], v['att_biases'], v['td_weights'], v['td_biases']),
                [p[n] for n in self.bucket.names], list(opt.wd), self.bucket.flat, opt.acc, steps=steps,
                momentum=opt.momentum, flags=cof.attn_flags(head.softmax_att, head.relu_att, True, False),
                keep_prob=head.keep_prob, seed=head.seed, offset=head._step,
                loss_wt=float(self.cfg.TRAIN.LOSS_FN_ACTION_WT), grad_scale=self.loss_scale, hooks=head.hooks)
            self._epoch_key = key
        self._epoch.run(order, lrs, offset=head._step)
        head._step += steps                              # a fresh dropout mask per step, as __call__ leaves it
        return self._epoch.loss[:steps]

    def video_epoch_unsupported_reason(self, cache=None) -> str:
        """why `train_video_epoch` cannot run this configuration (on this cache); '' when it can.  The clip epoch call is
        the CachedClips step -- softmax cross-entropy or a sigmoid loss, with or without the TemporalAttention conv --
        with the fused momentum-SGD update behind every step."""
        tr = self.cfg.TRAIN
        why = self.fp8_unsupported_reason(self.head, self.network_fn)
        if why:
            return why
        if not self.frozen_features:
            return 'frozen_features=False (a cache has no gradient: build the step with frozen_features=True)'
        if tr.OPTIMIZER not in ('momentum', 'sgd'):
            return 'TRAIN.OPTIMIZER %r (the epoch call runs the momentum / sgd update)' % tr.OPTIMIZER
        if int(tr.ITER_SIZE) != 1:
            return 'TRAIN.ITER_SIZE %d (gradient accumulation over micro-steps)' % int(tr.ITER_SIZE)
        if self.clipper is not None and self.clipper.active:
            return 'TRAIN.CLIP_GRADIENTS > 0 (an active gradient clipper between the step and the update)'
        if self.loss_scale != 1.0:
            return ('more than one clone (loss_scale %r: the gradients of an epoch call are not all-reduced)'
                    % self.loss_scale)
        if cache is not None:
            multi_label = tr.LOSS_FN_ACTION != 'softmax-xentropy'
            if cache.video_first is None:
                return 'a FeatureCache without videos (FeatureCache.set_videos names them)'
            if multi_label and cache.video_targets is None:
                return 'a FeatureCache without video targets (LOSS_FN_ACTION %r reads them)' % tr.LOSS_FN_ACTION
            if not multi_label and cache.video_labels is None:
                return 'a FeatureCache without video labels (the softmax cross-entropy reads them)'
        return ''

    def train_video_epoch(self, cache, batch_videos: int, frames: int, order, lr=None, mode: str = 'random-segment',
                          seed: int = 0, epoch: int = 0):
        """A whole epoch of frozen-feature training on the VIDEOS of a resident frame cache (`FeatureCache.set_videos`)
        as ONE host call (`clip_epoch.ClipTrainEpoch`: apa_attn_head_train_epoch_cached_clips): steps = order.numel() /
        batch_videos times the step `__call__` runs on `clip_epoch.sample_clips_keyed(cache, order[s*B:(s+1)*B], frames,
        mode, seed, epoch, step=s)` (the clips' own labels / targets, a fresh dropout mask per step) followed by the
        update `opt.step()` runs -- the same launches, the same bits.  Served under the softmax cross-entropy and both
        multi-label losses, with and without NET.USE_TEMPORAL_ATT; `frames=1`: one-frame videos, the flat multi-label
        datasets.  `order`: int32 VIDEO ids on the cache's device (`cof.epoch_order(cache.V, seed, epoch, device)`, or
        its first steps * batch_videos ids).  `lr`: one learning rate per step, or None for the optimiser's own.  Needs
        `make_optimizer()` first.  The staleness guards run once, in front; the head's step counter advances by
        `steps`.  Returns the loss log [steps, 1 + batch_videos] as a device tensor -- nothing synchronises.  Anything
        that is not served (more than one clone, frozen_features=False, per-class maps, the cfg 003 form, another
        optimiser, ITER_SIZE > 1, an active clipper) is a ValueError that names the reason."""
        from .custom_ops import clip_epoch, custom_ops_factory as cof
        who = 'FusedHeadStep.train_video_epoch'
        if self._optimizer is None:
            raise ValueError('%s: make_optimizer() first (the epoch call runs its update)' % who)
        why = self.video_epoch_unsupported_reason(cache)
        if why:
            raise ValueError('%s: a clip epoch call is not served with %s' % (who, why))
        opt, head, tr = self._optimizer, self.head, self.cfg.TRAIN
        opt.check_fresh()                                # weights written behind the optimiser's back?
        self._check_frozen_fresh()
        if opt.operand_copies():
            raise ValueError('%s: an epoch call is not served with operand copies attached to the optimiser (%s): its '
                             'update rewrites none' % (who, ', '.join(opt._watched)))
        B, F = int(batch_videos), int(frames)
        count = int(order.numel())
        if B < 1 or F < 1 or count < B or count % B:
            raise ValueError('%s: order holds %d video ids, not a whole number of batches of %d' % (who, count, B))
        steps = count // B
        lrs = [float(opt.lr)] * steps if lr is None else [float(v) for v in lr]
        if len(lrs) != steps:
            raise ValueError('%s: one learning rate per step expected (%d for %d steps)' % (who, len(lrs), steps))
        p, v = {n: t.data for n, t in self.params.items()}, self._grad_out
        temporal = {}
        if self.temporal is not None:                    # exactly what _run does in front of a step
            if F > 1 and not self.temporal._bias_initialised:
                with torch.no_grad():
                    self.temporal['biases'].fill_(1.0 / F)
                self.temporal._bias_initialised = True
            if F == 1:                                   # no pooling: the conv gets no gradient, its weights still decay
                v['temporal_weights'].zero_()
                v['temporal_biases'].zero_()
            else:
                temporal = dict(temporal=(p['temporal_weights'], p['temporal_biases']),
                                temporal_grads=(v['temporal_weights'], v['temporal_biases']))
        multi_label = tr.LOSS_FN_ACTION != 'softmax-xentropy'
        key = (id(cache), B, F, mode, tuple(t.data_ptr() for t in p.values()), self.bucket.flat.data_ptr(),
               opt.acc.data_ptr(), tuple(opt.wd), float(opt.momentum))
        if self._video_epoch is None or self._video_epoch_key != key or self._video_epoch.steps < steps:
            self._video_epoch = clip_epoch.ClipTrainEpoch(
                cache, B, F, p['att_weights'], p['att_biases'], p['td_weights'], p['td_biases'],
                (v['att_weights'], v['att_biases'], v['td_weights'], v['td_biases']),
                [p[n] for n in self.bucket.names], list(opt.wd), self.bucket.flat, opt.acc, steps=steps,
                action_loss=tr.LOSS_FN_ACTION, mode=mode, momentum=opt.momentum,
                flags=cof.attn_flags(head.softmax_att, head.relu_att, True, False), keep_prob=head.keep_prob,
                seed=head.seed, offset=head._step,
                loss_wt=1.0 if multi_label else float(tr.LOSS_FN_ACTION_WT),   # (loss.py:93-101 passes no weight)
                grad_scale=self.loss_scale, hooks=head.hooks, **temporal)
            self._video_epoch_key = key
        log = self._video_epoch.run(order, lrs, seed=seed, epoch=epoch, offset=head._step)
        head._step += steps                              # a fresh dropout mask per step, as __call__ leaves it
        return log


class FusedHeadEval:
    """The evaluation counterpart of FusedHeadStep: what eval.py:181-197 computes from `network_fn(images)` -- the
    logits, `tf.argmax(logits, 1)` and the scores (`tf.nn.softmax(logits, -1)`, or `tf.sigmoid(logits)` when
    TRAIN.LOSS_FN_ACTION starts with 'multi-label') -- with the head as ONE host call on the conv5 map:
    `apa_pose_attn_eval_step` for the cfg 003 form (attention from pose_pre_logits, which on the served shapes is
    never written: the pose-head product's epilogue emits the attention logits), `apa_attn_head_eval_step` for the
    single-layer forms (cfg 002, per-class maps).

        ev = deploy.FusedHeadEval(network_fn, cfg)          # network_fn built with is_training=False; raises
        scores, predictions, end_points = ev(images, labels_action)      # ValueError if the module path is needed
        meter.update(scores, labels_action)                 # eval_utils.Evaluation: accuracy / mAP at the end

    * end_points: 'Logits', 'PosePrelogitsBasedAttention', 'PoseLogits' (cfg 003 form with want_pose_logits=True;
      eval.py fetches it only under --ept), 'labels' when given, 'TemporalAttention' for video input with
      NET.USE_TEMPORAL_ATT.  Views of the bound step's buffers: overwritten by the next batch of the same shape.
    * one bound step (outputs, workspace) per batch shape / dtype, the `max_bound_steps` most recent.
    * 5-D video input [B,F,H,W,C]: the frames are folded into the batch for the head step; frame pooling (with the
      TemporalAttention conv when configured) and the scores and predictions of the POOLED logits (nets_factory.py:
      354-374, then eval.py:193-197) run inside the same call (`apa_attn_head_eval_step_clips` /
      `apa_pose_attn_eval_step_clips`), as do the sigmoid scores of a multi-label configuration, flat or on clips.
      Nothing runs behind the call: every returned tensor is a view of `ev.step`'s buffers.
    * the weights are read through the pointers a step was bound to: a parameter with a new storage binds a new step.
      No bf16 operand copy of W1 is kept here (there is no optimiser launch to keep it current): the conversion runs
      inside the call."""

    max_bound_steps = 4

    def __init__(self, network_fn, cfg):
        why = self.unsupported_reason(network_fn.head, cfg, network_fn)
        if why:
            raise ValueError('FusedHeadEval: ' + why)
        self.network_fn, self.head, self.cfg = network_fn, network_fn.head, cfg
        self.pose_form = not self.head.single_layer
        self.multi_label = str(cfg.TRAIN.LOSS_FN_ACTION).startswith('multi-label')
        self._steps = collections.OrderedDict()

    @staticmethod
    def unsupported_reason(head, cfg, network_fn=None) -> str:
        from . import nets_factory
        if isinstance(head, nets_factory.PoseAttentionLogitsHead):
            return 'the pose-heatmap attention head (USE_POSE_ATTENTION_LOGITS) evaluates through network_fn'
        if isinstance(head, nets_factory.BaselineHead) or not isinstance(head, nets_factory.AttentionalPoolingHead):
            return 'the baseline head (cfg 001) has no attention op: it evaluates through network_fn'
        if head.is_training:
            return 'a training-mode head: build network_fn with is_training=False (evaluation draws no dropout mask)'
        if head.rank != 1:
            return 'rank > 1 runs through the per-op module'
        if head.with_pose_feat:
            return '..._WITH_POSE_FEAT (pose logits concatenated to the top-down input) runs through the per-op module'
        if head.want_topdown:
            return 'the TopDownAttention dump is materialised by the per-op module only'
        if not head.single_layer:
            if head.per_class:
                return 'per-class maps from pose_pre_logits'
            if head.pose_w1.shape[0] != head.in_channels:
                return 'a separate feature tap for the pose head (NET.LAST_CONV_MAP_FOR_POSE)'
        return ''

    def _bind(self, X, want_pose_logits, frames=1, temporal=None):
        from .custom_ops import custom_ops_factory as cof
        h = self.head
        flags = cof.attn_flags(h.softmax_att, h.relu_att, False, self._preact)
        # flat softmax batches: the defaults, i.e. the steps as they always were; clips and / or sigmoid scores: the
        # *_eval_step_clips entry points (frame pooling, scores and predictions inside the call)
        clips = dict(frames=frames, temporal=temporal, scores='sigmoid' if self.multi_label else 'softmax')
        if self.pose_form and isinstance(X, cof.CachedBatch):   # a bf16 feature cache read by index: flat batches
            from .custom_ops import pose_cache
            return pose_cache.PoseAttnEvalStepCached(
                X, (h.pose_w1.data, h.pose_b1.data, h.pose_w2.data, h.pose_b2.data, h.att_weights.data,
                    h.att_biases.data, h.td_weights.data, h.td_biases.data), flags=flags,
                want_pose_logits=want_pose_logits)
        if self.pose_form:
            return cof.PoseAttnEvalStep(
                X, (h.pose_w1.data, h.pose_b1.data, h.pose_w2.data, h.pose_b2.data, h.att_weights.data,
                    h.att_biases.data, h.td_weights.data, h.td_biases.data), flags=flags,
                want_pose_logits=want_pose_logits, **clips)
        return cof.HeadEvalStep(X, X, h.att_weights.data, h.att_biases.data, h.td_weights.data, h.td_biases.data,
                                flags=flags, **clips)

    def _params(self):
        h = self.head
        names = ('att_weights', 'att_biases', 'td_weights', 'td_biases')
        if self.pose_form:
            names = ('pose_w1', 'pose_b1', 'pose_w2', 'pose_b2') + names
        return [getattr(h, n) for n in names]

    def __call__(self, images, labels_action=None, want_pose_logits: bool = False):
        from .custom_ops.custom_ops_factory import CachedBatch, CachedClips, Fp8Features
        frames = 1
        cb = isinstance(images, CachedBatch)
        fp8 = isinstance(images, Fp8Features) or cb
        if fp8:             # a cached conv5 map: FP8, or a FeatureCache read by index (see FusedHeadStep.cache_unsupported_reason)
            why = FusedHeadStep.cache_unsupported_reason(self.head, self.network_fn, images,
                                                         multi_label=self.multi_label)
            if why:
                raise ValueError('FusedHeadEval: %s is not served with %s' % (
                    'a CachedBatch' if cb else 'an Fp8Features batch', why))
            if isinstance(images, CachedClips):     # clips sampled from a frame cache: F and the labels ride along
                frames = int(images.frames)
                if labels_action is None:
                    labels_action = images.targets if self.multi_label else images.labels
        elif images.dim() == 5:                                 # nets_factory.py:121-125
            frames = images.shape[1]
            images = images.reshape(-1, *images.shape[2:])
        last_conv, self._preact = (images, False) if fp8 else self.network_fn.features(images)
        if last_conv.dim() != 4:
            raise ValueError('FusedHeadEval: [N,H,W,C] (or [B,F,H,W,C]; an Fp8Features batch: [N,H,W,C]) feature maps '
                             'expected')
        if self._preact and not self.head.can_fuse_input_relu(last_conv.dtype):
            last_conv, self._preact = torch.relu(last_conv), False
        n, hh, ww, c = last_conv.shape
        X = last_conv.flat() if fp8 else last_conv.detach().contiguous().view(n, -1, c)
        want_pl = bool(want_pose_logits and self.pose_form)
        tw = tb = None
        temporal = self.network_fn.temporal if frames > 1 else None     # nets_factory.py:354-374
        if temporal is not None:
            if not temporal._bias_initialised:
                with torch.no_grad():
                    temporal['biases'].fill_(1.0 / frames)
                temporal._bias_initialised = True
            tw, tb = temporal['weights'].data.reshape(-1).contiguous(), temporal['biases'].data
        key = (tuple(X.shape), X.dtype, self._preact, want_pl, tuple(p.data_ptr() for p in self._params()), frames,
               None if tw is None else tw.data_ptr(), None if tb is None else tb.data_ptr(),
               id(X.cache) if cb else None)
        st = self._steps.pop(key, None)
        if st is None:
            st = self._bind(X, want_pl, frames, None if tw is None else (tw, tb))
        elif cb:                                                # the same cache: only the index is re-bound
            st.rebind(index=X.index)
        else:
            st.rebind(X=X) if self.pose_form else st.rebind(X)
        self._steps[key] = st                                   # most recent last
        while len(self._steps) > self.max_bound_steps:
            self._steps.popitem(last=False)
        st.run()                                                # everything returned below is a view of st's buffers
        self.step = st
        ep = {'Logits': st.logits, 'PosePrelogitsBasedAttention': st.att.view(n, hh, ww, -1)}
        if want_pl:
            ep['PoseLogits'] = st.Pl.view(n, hh, ww, -1)
        if labels_action is not None:
            ep['labels'] = labels_action.squeeze() if labels_action.dim() > 1 else labels_action   # eval.py:198
        if frames > 1:
            ep['logits_beforePool'] = st.logits
            ep['Logits'] = st.pooled
            if st.tatt is not None:
                ep['TemporalAttention'] = st.tatt.view(-1, frames, 1, 1)
        return st.probs, st.pred, ep

    def new_evaluation(self, capacity: int):
        """An `eval_utils.DeviceEvaluation` for this head's scores: its K, its device, and multi-hot targets when
        TRAIN.LOSS_FN_ACTION starts with 'multi-label' (the configurations whose scores are sigmoids).  Feed it what
        `__call__` returns -- `meter.update(scores, labels_action)` -- and read accuracy / mAP from `meter.result()`:
        nothing touches the host until then."""
        from . import eval_utils
        w = self.head.td_weights
        return eval_utils.DeviceEvaluation(capacity, int(w.shape[1]), w.device, multi_label=self.multi_label)

    def evaluate_cache(self, cache, batch_size: int, meter=None, order=None):
        """A whole validation pass over a resident `FeatureCache` as ONE host call (`cof.HeadEvalEpoch`:
        apa_attn_head_eval_epoch_cached): the images `order` names (int32 on the cache's device; default all T, in
        cache order) in batches of `batch_size`, the last one shorter, with the scores written straight into
        `meter.reserve(count)` -- no copy, no synchronisation -- and the truth taken from `cache.labels[order]`.
        `meter`: an `eval_utils.DeviceEvaluation` (default: `new_evaluation(count)`); it is returned, and
        `meter.result()` equals that of a meter fed by `__call__` batch by batch.  Served: what a flat CachedBatch is
        served with, softmax scores, a cache with labels; anything else is a ValueError that names the reason.
        `self.epoch` is the bound pass (`logits`, `pred`, the last batch's `att`)."""
        import torch
        from .custom_ops import custom_ops_factory as cof
        why = FusedHeadStep.fp8_unsupported_reason(self.head, self.network_fn)
        if not why and self.multi_label:
            why = ('LOSS_FN_ACTION %r (multi-hot targets: the cache\'s labels are class ids)'
                   % self.cfg.TRAIN.LOSS_FN_ACTION)
        if not why and cache.labels is None:
            why = 'a FeatureCache without labels (the truth is cache.labels[order])'
        if why:
            raise ValueError('FusedHeadEval.evaluate_cache: a cache pass is not served with %s' % why)
        N = int(batch_size)
        if N < 1:
            raise ValueError('FusedHeadEval.evaluate_cache: batch_size >= 1 expected')
        if order is None:
            order = torch.arange(cache.T, dtype=torch.int32, device=cache.device)
        count = int(cof._epoch_order_arg('FusedHeadEval.evaluate_cache', order, cache).numel())
        if meter is None:
            meter = self.new_evaluation(count)
        h = self.head
        key = (id(cache), N, tuple(p.data_ptr() for p in self._params()))
        ep = getattr(self, 'epoch', None)
        if ep is None or self._epoch_key != key or ep.capacity < count:
            ep = self.epoch = cof.HeadEvalEpoch(
                cache, N, h.att_weights.data, h.att_biases.data, h.td_weights.data, h.td_biases.data, capacity=count,
                flags=cof.attn_flags(h.softmax_att, h.relu_att, False, False), scores='softmax')
            self._epoch_key = key
        scores, truth = meter.reserve(count)
        truth.copy_(cache.labels[order.long().clamp_(0, cache.T - 1)])       # (an id outside the cache is clamped, as
        ep.run(order, count, probs=scores)                                   # the kernels clamp it)
        return meter

    def evaluate_videos(self, cache, batch_videos: int, frames: int, meter=None, order=None):
        """A whole validation pass over the VIDEOS of a resident frame cache (`FeatureCache.set_videos`) as ONE host
        call (`clip_epoch.ClipEvalEpoch`: apa_attn_head_eval_epoch_cached_clips): the videos `order` names (int32 on the
        cache's device; default all V, in table order) in batches of `batch_videos`, the last one shorter, each as
        `frames` uniformly spaced frames (the reference's test protocol), with the scores AND the truth -- the videos'
        labels, or their multi-hot targets when TRAIN.LOSS_FN_ACTION starts with 'multi-label' -- written straight into
        `meter.reserve(count)`: no copy, no host step.  `meter`: an `eval_utils.DeviceEvaluation` (default:
        `new_evaluation(count)`); it is returned, and equals one fed by `__call__` on
        `cache.sample_clips(order[a:a+B], frames)` batch by batch, bit for bit.  With and without NET.USE_TEMPORAL_ATT
        (which takes part at frames > 1, as in `__call__`).  Anything that is not served (per-class maps, the cfg 003
        form, a cache without videos or without the truth the scores need) is a ValueError that names the reason.
        `self.video_epoch` is the bound pass (`pred`, `pooled`, the last batch's frame logits and `att`)."""
        import torch
        from .custom_ops import clip_epoch, custom_ops_factory as cof
        who = 'FusedHeadEval.evaluate_videos'
        why = FusedHeadStep.fp8_unsupported_reason(self.head, self.network_fn)
        if not why and getattr(cache, 'video_first', None) is None:
            why = 'a FeatureCache without videos (FeatureCache.set_videos names them)'
        if not why and self.multi_label and cache.video_targets is None:
            why = ('a FeatureCache without video targets (LOSS_FN_ACTION %r: the truth is multi-hot)'
                   % self.cfg.TRAIN.LOSS_FN_ACTION)
        if not why and not self.multi_label and cache.video_labels is None:
            why = 'a FeatureCache without video labels (the truth of the softmax scores)'
        if why:
            raise ValueError('%s: a video pass is not served with %s' % (who, why))
        B, F = int(batch_videos), int(frames)
        if B < 1 or F < 1:
            raise ValueError('%s: batch_videos >= 1 and frames >= 1 expected' % who)
        if order is None:
            order = torch.arange(cache.V, dtype=torch.int32, device=cache.device)
        count = int(cof._epoch_order_arg(who, order, cache).numel())
        if meter is None:
            meter = self.new_evaluation(count)
        h = self.head
        tw = tb = None
        temporal = self.network_fn.temporal if F > 1 else None          # nets_factory.py:354-374, as __call__
        if temporal is not None:
            if not temporal._bias_initialised:
                with torch.no_grad():
                    temporal['biases'].fill_(1.0 / F)
                temporal._bias_initialised = True
            tw, tb = temporal['weights'].data.reshape(-1).contiguous(), temporal['biases'].data
        key = (id(cache), B, F, tuple(p.data_ptr() for p in self._params()),
               None if tw is None else tw.data_ptr(), None if tb is None else tb.data_ptr())
        ep = getattr(self, 'video_epoch', None)
        if ep is None or self._video_epoch_key != key or ep.capacity < count:
            ep = self.video_epoch = clip_epoch.ClipEvalEpoch(
                cache, B, F, h.att_weights.data, h.att_biases.data, h.td_weights.data, h.td_biases.data,
                capacity=count, temporal=None if tw is None else (tw, tb),
                flags=cof.attn_flags(h.softmax_att, h.relu_att, False, False),
                scores='sigmoid' if self.multi_label else 'softmax')
            self._video_epoch_key = key
        scores, truth = meter.reserve(count)
        if self.multi_label:
            ep.run(order, count, probs=scores, targets=truth)
        else:
            ep.run(order, count, probs=scores, labels=truth)
        return meter

    def explain(self, images, classes=None, topk: int = 1, overlay: bool = True, input_images=None):
        """Why the batch was given its classes: the bottom-up map, the top-down map of T chosen classes per image and
        their product (the paper's figures; the end points the reference dumps with `eval.py --ept` and summarises in
        train.py:451-460), from ONE extra pass over the conv5 map (`cof.attn_explain`) behind the bound evaluation
        step, which runs exactly as in `__call__`.  The K-map 'TopDownAttention' dump is never built.

        * classes=None: the step's own predictions -- topk == 1 takes `pred` (no host synchronisation), topk > 1
          `torch.topk` of the scores.  Explicit `classes`: integers [N] or [N,T] (clips: [B] or [B,T]), T <= 8.
        * returns a dict: 'bottom_up' [N,H,W], 'top_down' [N,T,H,W], 'combined' [N,T,H,W], 'class_logit' [N,T]
          (== the step's logits[n, class]), 'classes' [N,T] int64, 'scores' (what `__call__` returns), 'status' (int32
          device scalar: class ids outside [0,K), which were clamped); with overlay=True also 'overlay_bottom_up'
          [N,1,Hi,Wi,3] and 'overlay_combined' [N,T,Hi,Wi,3], uint8 (`cof.attention_overlay`: train.py:184-195, then
          tf.summary.image's scaling).  With per-class bottom-up maps 'bottom_up' is [N,T,H,W], the chosen classes'.
        * the overlay is laid over `images` when a backbone is in front, over `input_images` [N,Hi,Wi,3] otherwise.
        * clip batches [B,F,...]: the frames are folded as in `__call__`; a clip's classes are repeated for its F
          frames and every map is per FRAME.  The temporal attention weight of a frame is NOT applied to its maps.
        * dense feature maps only: an Fp8Features or CachedBatch batch raises ValueError."""
        from .custom_ops import custom_ops_factory as cof
        for kind, what in ((cof.CachedBatch, 'a CachedBatch'), (cof.Fp8Features, 'an Fp8Features batch')):
            if isinstance(images, kind):
                raise ValueError('FusedHeadEval.explain: %s is not served: the explain kernel reads dense feature maps'
                                 % what)
        if self.head.is_training:
            raise ValueError('FusedHeadEval.explain: a training-mode head (evaluation semantics only: no dropout)')
        topk = int(topk)
        if classes is None and not 1 <= topk <= cof.APA_EXPLAIN_MAX_CLASSES:
            raise ValueError('FusedHeadEval.explain: topk must be 1..%d' % cof.APA_EXPLAIN_MAX_CLASSES)
        has_backbone = self.network_fn.backbone is not None
        src = None
        if overlay:
            src = images if has_backbone else input_images
            if src is None:
                raise ValueError('FusedHeadEval.explain: overlay=True needs an image source: there is no backbone in '
                                 'front (`images` is the conv5 map) and no input_images were given')
        scores, pred, ep = self(images)
        st = self.step
        frames = images.shape[1] if images.dim() == 5 else 1
        X = st._keep[0]                                         # the dense [N,P,C] map the step was bound to
        n, hh, ww = ep['PosePrelogitsBasedAttention'].shape[:3]
        if classes is None:
            cls = pred.view(-1, 1) if topk == 1 else torch.topk(scores, topk, dim=1).indices
        else:
            cls = classes if classes.dim() > 1 else classes.view(-1, 1)
            if cls.dim() != 2 or cls.dtype.is_floating_point:
                raise ValueError('FusedHeadEval.explain: classes must be integers [N] or [N,T]')
            cls = cls.to(X.device)
        if cls.shape[0] * frames != n:
            raise ValueError('FusedHeadEval.explain: %d rows of classes for %d %s' % (
                cls.shape[0], n // frames, 'clips' if frames > 1 else 'images'))
        if frames > 1:                                          # a clip's classes, for each of its frames
            cls = cls.repeat_interleave(frames, dim=0)
        cls = cls.to(torch.int64)
        t = cls.shape[1]
        flags = cof.APA_FLAG_RELU_INPUT if self._preact else 0
        h = self.head
        td, comb, cl, status = cof.attn_explain(X, st.att, h.td_weights.data, h.td_biases.data, cls, flags=flags)
        if st.att.shape[2] == 1:
            bottom = st.att.view(n, hh, ww)
            bottom_maps = st.att.view(n, 1, hh, ww)
        else:                                                   # per-class maps: the chosen classes' own
            k = st.att.shape[2]
            idx = cls.clamp(0, k - 1).view(n, 1, t).expand(n, st.att.shape[1], t)
            bottom_maps = torch.gather(st.att, 2, idx).permute(0, 2, 1).contiguous().view(n, t, hh, ww)
            bottom = bottom_maps
        out = {'bottom_up': bottom, 'top_down': td.view(n, t, hh, ww), 'combined': comb.view(n, t, hh, ww),
               'class_logit': cl, 'classes': cls, 'scores': scores, 'status': status}
        if overlay:
            if src.dim() == 5:
                src = src.reshape(-1, *src.shape[2:])
            if src.dim() != 4 or src.shape[0] != n or src.shape[-1] != 3:
                raise ValueError('FusedHeadEval.explain: the overlay needs images [N,Hi,Wi,3] for the %d maps (got %s)'
                                 % (n, tuple(src.shape)))
            src = src.detach().to(device=X.device, dtype=torch.float32).contiguous()
            out['overlay_bottom_up'] = cof.attention_overlay(bottom_maps.contiguous(), src)
            out['overlay_combined'] = cof.attention_overlay(out['combined'], src)
        return out


class HeadSweep:
    """H class-agnostic heads (cfg 002) trained and evaluated from ONE pass over a resident `FeatureCache` per direction
    (custom_ops/multihead.py, include/apa_multihead.h): a learning-rate / weight-decay sweep, several initialisations or
    a seed ensemble whose scores are averaged at test time ("late fusion", the reference's eval.py).

        sweep = deploy.HeadSweep([get_network_fn(..., backbone=None) for _ in range(4)], cfg, lrs=[.1, .03, .01, .003])
        log = sweep.train_epoch(cache, 32, cache.order(seed, epoch))          # loss log [steps, H, 1 + 32]
        meters = sweep.evaluate_cache(val_cache, 64)                          # H per-head meters + the fused one
        h = sweep.best('mAP')

    The heads must have identical shapes and flags (a ValueError names the first difference).  Their parameters move
    into stacked storages -- Wa [H,C], ba [H], Wt [H,C,K], bt [H,K] -- and each head's `Parameter.data` becomes a view of
    row h, so every head stays usable on its own and its `state_dict()` still works.  All heads share the batch, the
    labels and ONE dropout mask per step: the mask's step counter advances once per step for the whole sweep (heads that
    need different keep probabilities or mask streams train as separate FusedHeadStep runs).  FP8 caches are refused by
    the library by name.  Momentum SGD (TRAIN.MOMENTUM) with per-head learning rate and weight decay (biases carry
    none); `FusedHeadStep` / `FusedHeadEval` and their reasons are unchanged."""

    NAMES = ('att_weights', 'att_biases', 'td_weights', 'td_biases')

    def __init__(self, network_fns, cfg, lrs, weight_decays=None):
        from . import nets_factory
        from .custom_ops import multihead as mh
        fns = list(network_fns)
        H = len(fns)
        if not 1 <= H <= mh.APA_HEADS_MAX:
            raise ValueError('HeadSweep: 1 .. %d heads expected (got %d)' % (mh.APA_HEADS_MAX, H))
        for i, fn in enumerate(fns):
            why = '' if isinstance(fn.head, nets_factory.AttentionalPoolingHead) else 'a head without the attention op'
            why = why or FusedHeadStep.fp8_unsupported_reason(fn.head, fn)
            if not why and cfg.TRAIN.LOSS_FN_ACTION != 'softmax-xentropy':
                why = 'LOSS_FN_ACTION %r (the multi-head step takes the softmax cross-entropy)' % cfg.TRAIN.LOSS_FN_ACTION
            if why:
                raise ValueError('HeadSweep: head %d is not served with %s' % (i, why))
        h0 = fns[0].head
        for i, fn in enumerate(fns[1:], 1):
            h = fn.head
            for n in self.NAMES:
                a, b = getattr(h0, n), getattr(h, n)
                if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
                    raise ValueError('HeadSweep: head %d differs from head 0 in %s (%s %s on %s against %s %s on %s)' % (
                        i, n, tuple(b.shape), b.dtype, b.device, tuple(a.shape), a.dtype, a.device))
            for n in ('relu_att', 'softmax_att', 'keep_prob', 'is_training', 'seed'):
                if getattr(h0, n) != getattr(h, n):
                    raise ValueError('HeadSweep: head %d differs from head 0 in %s (%r against %r)' % (
                        i, n, getattr(h, n), getattr(h0, n)))
        self.network_fns, self.heads, self.cfg, self.H = fns, [fn.head for fn in fns], cfg, H
        self.lrs = [float(v) for v in lrs]
        if len(self.lrs) != H:
            raise ValueError('HeadSweep: one learning rate per head expected (%d for %d heads)' % (len(self.lrs), H))
        wds = [float(getattr(fn, 'weight_decay', 0.0)) for fn in fns] if weight_decays is None else \
            [float(v) for v in weight_decays]
        if len(wds) != H:
            raise ValueError('HeadSweep: one weight decay per head expected (%d for %d heads)' % (len(wds), H))
        self.weight_decays = wds
        # the stacked storages; each head's parameters become views of its rows
        self.stacked = []
        with torch.no_grad():
            for n in self.NAMES:
                rows = [getattr(h, n).data.reshape(-1) for h in self.heads]
                st = torch.stack(rows).contiguous()
                for i, h in enumerate(self.heads):
                    p = getattr(h, n)
                    p.data = st[i].view(p.shape)
                self.stacked.append(st)
        C, K = (int(d) for d in h0.td_weights.shape)
        self.C, self.K = C, K
        self.Wa, self.ba = self.stacked[0], self.stacked[1].view(H)
        self.Wt, self.bt = self.stacked[2].view(H, C, K), self.stacked[3]
        self._step = int(h0._step)
        self._train = self._train_key = self._eval = self._eval_key = None
        self.acc = None
        self.meters = None

    def _params(self):
        return self.Wa, self.ba, self.Wt, self.bt

    def train_epoch(self, cache, batch_size: int, order, lr=None):
        """steps = order.numel() / batch_size training steps of all heads and their updates as ONE host call
        (apa_multihead_train_epoch_cached), on the cache's own labels.  `lr`: None (the sweep's `lrs` in every step), H
        values, or one row of H values per step.  Returns the loss log [steps, H, 1 + batch_size] on the device."""
        from .custom_ops import multihead as mh
        if cache.labels is None:
            raise ValueError('HeadSweep.train_epoch: a FeatureCache without labels')
        h0 = self.heads[0]
        if not h0.is_training:
            raise ValueError('HeadSweep.train_epoch: evaluation-mode heads (build network_fn with is_training=True)')
        N, count = int(batch_size), int(order.numel())
        if N < 1 or count < N or count % N:
            raise ValueError('HeadSweep.train_epoch: order holds %d ids, not a whole number of batches of %d' % (count, N))
        steps = count // N
        key = (cache, N, steps)                  # (the cache itself: an id could be reused by another cache)
        if self._train is None or self._train_key != key:
            step = mh.MultiHeadTrainStep(
                cache.select(torch.zeros((N,), dtype=torch.int32, device=cache.device)), *self._params(), 'cache',
                relu_att=h0.relu_att, keep_prob=h0.keep_prob, seed=h0.seed, offset=self._step,
                loss_wt=float(self.cfg.TRAIN.LOSS_FN_ACTION_WT))
            if self.acc is None:
                self.acc = torch.zeros_like(step.grad_flat)
            momentum = float(self.cfg.TRAIN.MOMENTUM) if self.cfg.TRAIN.OPTIMIZER == 'momentum' else 0.0
            sgd = mh.MultiHeadSGD(self._params(), [self.weight_decays, 0.0, self.weight_decays, 0.0], step.grad_flat,
                                  self.acc, self.lrs, momentum)
            self._train, self._train_key = mh.MultiHeadTrainEpoch(step, sgd, steps), key
        log = self._train.run(order, self.lrs if lr is None else lr, offset=self._step)
        self._step += steps                      # ONE dropout stream for the whole sweep: once per step
        for h in self.heads:
            h._step = self._step
        return log

    def evaluate_cache(self, cache, batch_size: int, meters=None, order=None):
        """A validation pass of all heads over the cache as ONE host call (apa_multihead_eval_epoch_cached).  Fills and
        returns H + 1 `eval_utils.DeviceEvaluation` meters: one per head and, last, one for the fused scores (the mean
        of the heads' softmax scores).  The truth is `cache.labels[order]`."""
        from . import eval_utils
        from .custom_ops import multihead as mh
        if cache.labels is None:
            raise ValueError('HeadSweep.evaluate_cache: a FeatureCache without labels (the truth is cache.labels[order])')
        N = int(batch_size)
        if N < 1:
            raise ValueError('HeadSweep.evaluate_cache: batch_size >= 1 expected')
        if order is None:
            order = torch.arange(cache.T, dtype=torch.int32, device=cache.device)
        count = int(order.numel())
        key = (cache, N)
        if self._eval is None or self._eval_key != key or self._eval.capacity < count:
            self._eval = mh.MultiHeadEvalEpoch(cache, N, *self._params(), capacity=count,
                                               relu_att=self.heads[0].relu_att, fused=True)
            self._eval_key = key
        probs, pred, fused_probs, fused_pred = self._eval.run(order)
        if meters is None:
            meters = [eval_utils.DeviceEvaluation(count, self.K, cache.device) for _ in range(self.H + 1)]
        if len(meters) != self.H + 1:
            raise ValueError('HeadSweep.evaluate_cache: %d meters expected (one per head and the fused one)' % (self.H + 1))
        truth = cache.labels[order.long().clamp(0, cache.T - 1)]
        for i, m in enumerate(meters):
            scores, t = m.reserve(count)
            scores.copy_(probs[i] if i < self.H else fused_probs)
            t.copy_(truth)
        self.meters = meters
        return meters

    def best(self, metric: str = 'mAP') -> int:
        """the head with the largest `metric` ('mAP' / 'accuracy') of the last `evaluate_cache` (the first of equals)"""
        if self.meters is None:
            raise ValueError('HeadSweep.best: evaluate_cache() first')
        vals = [m.result()[metric] for m in self.meters[:self.H]]
        return max(range(self.H), key=lambda i: (vals[i], -i))
