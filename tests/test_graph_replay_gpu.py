"""Every stream-taking entry point of include/apa.h, replayed from a captured hipGraph.

include/apa.h: "every launch goes to the hipStream_t passed as `void* stream`; no implicit synchronisation, no
allocation -> all entry points are hipGraph-capturable".  Each row of ROWS captures one call (or the short sequence a
training / evaluation loop makes of them) with torch.cuda.graph and holds three replays, with the mutable inputs
rewritten in place in between, to three eager calls: every output and every piece of written state equal by
torch.equal (tests/_graph_replay.py states the protocol).  ROWS is plain data -- tests/test_graph_replay_cpu.py reads
it without a device and asserts that no stream-taking declaration of the header is missing from it.

Comparison rule: bits, in every row.  The rule's one candidate for an exception, apa_pose_head_bwd's dW2 (its path
starts from a hipMemsetAsync), turned out not to be one: the memset IS the result (dW2 = 0 when there is no pose-loss
gradient) and the library has no floating-point atomic anywhere (its three atomicAdd are integer counts), so the row
'pose_head_bwd_no_dpl' holds that path to bits too.
Shapes are the smallest ones the per-path tests of the same family use; their builders are imported, not copied.
"""
import ctypes

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _graph_replay as gr
from tests._graph_replay import Case

pytestmark = pytest.mark.gpu

BITS = 'bits'       # the only rule in use: "identical calls give identical bits"; a replay is an identical call


def row(name, entries, build, *args, frozen=False):
    return dict(id=name, entries=tuple(entries), rule=BITS, build=build, args=args, frozen=frozen)


# `frozen`: the entry point reads nothing from HBM that a round could rewrite (every argument travels by value), so the
# three replays equal the three eager calls AND each other; the rounds-must-differ check does not apply.
ROWS = [
    # ---- the training-loop body on a resident cache: one capture = the cached step + the optimiser's launch
    row('loop_stream_f32_c1024', ['apa_attn_head_train_step_cached', 'apa_momentum_sgd_step'], 'cached_loop', 'stream', 1024),
    row('loop_stream_bf16_c2048', ['apa_attn_head_train_step_cached', 'apa_momentum_sgd_step'], 'cached_loop', 'stream', 2048),
    row('loop_vec_f32_c256', ['apa_attn_head_train_step_cached', 'apa_momentum_sgd_step'], 'cached_loop', 'vec', 256),
    row('loop_generic_f32_c40', ['apa_attn_head_train_step_cached', 'apa_momentum_sgd_step'], 'cached_loop', 'generic', 40),
    row('loop_fp8_c32', ['apa_attn_head_train_step_cached', 'apa_momentum_sgd_step'], 'cached_loop', 'fp8', 32),
    row('loop_per_class_bf16_k51_images', ['apa_attn_head_train_step_cached', 'apa_per_class_weight_images',
                                          'apa_momentum_sgd_step_images'], 'cached_per_class'),
    # ---- clips from the cache: the sampler, the cached clip step with temporal attention, the update
    row('clips_softmax', ['apa_sample_clip_frames', 'apa_attn_head_train_step_cached_clips', 'apa_momentum_sgd_step'],
        'cached_clips', 'softmax-xentropy'),
    row('clips_multi_label', ['apa_sample_clip_frames', 'apa_attn_head_train_step_cached_clips', 'apa_momentum_sgd_step'],
        'cached_clips', 'multi-label'),
    # ---- the epoch calls
    row('train_epoch_3_steps', ['apa_attn_head_train_epoch_cached'], 'train_epoch'),
    row('eval_epoch_softmax_loss', ['apa_attn_head_eval_epoch_cached'], 'eval_epoch', 'softmax'),
    row('eval_epoch_sigmoid', ['apa_attn_head_eval_epoch_cached'], 'eval_epoch', 'sigmoid'),
    # ---- the rank-R step
    row('rank2_step', ['apa_attn_head_train_step_rank'], 'rank_step'),
    # ---- the pose-attention steps, both routes, with their clip and multi-label forms
    row('pose_attn_train_fused_bf16', ['apa_pose_attn_train_step'], 'pose_train', 'fused_softmax', 'plain'),
    row('pose_attn_train_composed_f32', ['apa_pose_attn_train_step'], 'pose_train', 'composed_fp32', 'plain'),
    row('pose_attn_train_clips', ['apa_pose_attn_train_step_clips'], 'pose_train', 'fused_softmax', 'clips'),
    row('pose_attn_train_multilabel', ['apa_pose_attn_train_step_multilabel'], 'pose_train', 'composed_fp32', 'multi-label'),
    row('pose_attn_eval_fused', ['apa_pose_attn_eval_step'], 'pose_eval', 'fused_softmax', 'plain'),
    row('pose_attn_eval_composed', ['apa_pose_attn_eval_step'], 'pose_eval', 'composed_fp32', 'plain'),
    row('pose_attn_eval_clips_sigmoid', ['apa_pose_attn_eval_step_clips'], 'pose_eval', 'fused_softmax', 'clips'),
    # ---- the evaluation steps, each followed by the average-precision call on its score buffer
    row('eval_flat_softmax_t1025', ['apa_attn_head_eval_step', 'apa_average_precision'], 'eval_step', 'flat'),
    row('eval_clips_sigmoid_t5', ['apa_attn_head_eval_step_clips', 'apa_average_precision'], 'eval_step', 'clips'),
    row('eval_cached_softmax_t5', ['apa_attn_head_eval_step_cached', 'apa_average_precision'], 'eval_step', 'cached'),
    row('eval_cached_clips_sigmoid_t3', ['apa_attn_head_eval_step_cached_clips', 'apa_average_precision'], 'eval_step',
        'cached_clips'),
    # per-class maps without labels: the label-free form zeroes its scratch labels at the head of the workspace
    row('eval_per_class_no_labels', ['apa_attn_head_eval_step'], 'eval_per_class'),
    # ---- the one-call steps on a plain batch
    row('train_step_plain', ['apa_attn_head_train_step'], 'train_step', 'plain'),
    row('train_step_ex', ['apa_attn_head_train_step_ex'], 'train_step', 'ex'),
    row('train_step_clips', ['apa_attn_head_train_step_clips'], 'train_step', 'clips'),
    row('train_step_multilabel', ['apa_attn_head_train_step_multilabel'], 'train_step', 'multi-label'),
    # ---- the separate calls: forward / loss / backward
    row('pool_fwd_bwd', ['apa_attn_pool_fwd', 'apa_softmax_xent_fwd_bwd', 'apa_attn_pool_bwd'], 'pool', 'plain'),
    row('pool_fwd_bwd_ex', ['apa_attn_pool_fwd_ex', 'apa_softmax_xent_fwd_bwd', 'apa_attn_pool_bwd_ex'], 'pool', 'ex'),
    row('pool_fwd_bwd_cached', ['apa_attn_pool_fwd_cached', 'apa_attn_pool_bwd_cached'], 'pool', 'cached'),
    row('pool_fwd_bwd_cat', ['apa_attn_pool_fwd_cat', 'apa_attn_pool_bwd_cat'], 'pool_cat'),
    row('pool_fwd_bwd_rank3', ['apa_attn_pool_rank_fwd', 'apa_attn_pool_rank_bwd'], 'pool_rank'),
    row('pose_head_fwd_bwd', ['apa_pose_head_fwd', 'apa_pose_head_bwd'], 'pose_head', 'plain'),
    row('pose_head_bwd_no_dpl', ['apa_pose_head_fwd', 'apa_pose_head_bwd'], 'pose_head', 'no_dpl'),
    row('pose_head_bwd_rank1ext', ['apa_pose_head_fwd', 'apa_pose_head_bwd_rank1ext'], 'pose_head', 'rank1'),
    row('pose_att_logits', ['apa_pose_att_logits_fwd', 'apa_pose_att_logits_bwd'], 'pose_att', False),
    row('pose_att_logits_ex', ['apa_pose_att_logits_fwd_ex', 'apa_pose_att_logits_bwd_ex'], 'pose_att', True),
    # ---- the losses
    row('xent_n7_loss_only', ['apa_softmax_xent_fwd_bwd'], 'xent', 7, 100, False),
    row('xent_n7_grad', ['apa_softmax_xent_fwd_bwd'], 'xent', 7, 100, True),
    row('xent_n65', ['apa_softmax_xent_fwd_bwd'], 'xent', 65, 100, True),
    row('xent_stream_k3', ['apa_softmax_xent_fwd_bwd'], 'xent', 9, 3, True),
    row('action_losses', ['apa_action_loss_fwd_bwd'], 'action_loss'),
    row('multilabel_losses', ['apa_multilabel_loss_fwd_bwd'], 'multilabel_loss'),
    row('clip_xent', ['apa_clip_xent_fwd_bwd'], 'clip_loss', 'softmax-xentropy'),
    row('clip_multilabel', ['apa_clip_multilabel_fwd_bwd'], 'clip_loss', 'multi-label'),
    row('pose_l2', ['apa_pose_l2_loss_fwd_bwd'], 'pose_l2'),
    row('pose_sampled', ['apa_pose_sampled_loss_fwd_bwd'], 'pose_sampled'),
    row('frame_pool', ['apa_frame_pool_fwd', 'apa_frame_pool_bwd'], 'frame_pool'),
    row('clip_scores', ['apa_clip_scores'], 'clip_scores'),
    # ---- the optimisers and elementwise ops
    row('momentum_sgd', ['apa_momentum_sgd_step'], 'optimiser', 'sgd'),
    row('momentum_sgd_shadow', ['apa_momentum_sgd_step_shadow'], 'optimiser', 'shadow'),
    row('momentum_sgd_images', ['apa_momentum_sgd_step_images'], 'optimiser', 'images'),
    row('adam', ['apa_adam_step'], 'optimiser', 'adam'),
    row('rmsprop', ['apa_rmsprop_step'], 'optimiser', 'rmsprop'),
    row('accumulate_gradients', ['apa_accumulate_gradients', 'apa_accumulate_gradients_div'], 'accumulate'),
    row('spatial_mean_bwd', ['apa_spatial_mean_bwd'], 'spatial_mean_bwd'),
    row('zero_out_channels', ['apa_zero_out_channels'], 'zero_out_channels'),
    row('dropout_mask', ['apa_dropout_mask'], 'dropout_mask', frozen=True),
    row('per_class_weight_images', ['apa_per_class_weight_images'], 'weight_images'),
    row('resize_bilinear_tf1', ['apa_resize_bilinear_tf1'], 'resize'),
    # ---- the cache and input kernels
    row('fp8_quantize_dequantize', ['apa_quantize_features_fp8', 'apa_dequantize_features_fp8'], 'fp8_quantize'),
    row('fp8_quantize_at', ['apa_quantize_features_fp8_at'], 'fp8_quantize_at'),
    row('sample_clip_frames_uniform', ['apa_sample_clip_frames'], 'sample_clips'),
    row('epoch_order', ['apa_epoch_order'], 'epoch_order', frozen=True),
    row('pose_labels_device', ['apa_pose_labels_device'], 'pose_labels'),
    row('preprocess_images', ['apa_preprocess_images'], 'preprocess_images'),
    row('attn_explain', ['apa_attn_explain'], 'explain'),
    row('attention_overlay', ['apa_attention_overlay'], 'overlay'),
]


# Stream-taking entry points without a row.  include/apa.h takes each of them out of its "all entry points" sentence.
NOT_CAPTURED = {
    'apa_clip_by_norm_prepare': 'marshals a host table into the workspace and waits for its own copies on the stream, by '
                                'design, once per binding; apa_clip_by_norm_run is the capturable half',
    'apa_prof_event_record': 'records a HIP event for the measurement hooks; events inside a captured region are out of '
                             'scope here (they belong to the overlapped-gradient and timing paths)',
}
# Captured by a test that already exists: named here, not duplicated.
CAPTURED_ELSEWHERE = {
    'apa_clip_by_norm_run': 'tests/test_clip_gradients_gpu.py::test_clip_kernel_against_float64',
}


# ------------------------------------------------------------------------------------------ small tools
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _variants(t, R=3):
    """R different tensors of t's shape and dtype on the host: t, and t rolled along its flat index"""
    return [t if r == 0 else torch.roll(t.reshape(-1), 7 * r + 1).reshape(t.shape).contiguous() for r in range(R)]


def _rounds(**named):
    """{name: host tensor} -> three rounds, each input in three variants"""
    vs = {k: _variants(v) for k, v in named.items()}
    return [{k: v[r] for k, v in vs.items()} for r in range(3)]


def _bucket(tensors, dev):
    """(grad_flat, acc_flat, views of grad_flat shaped like `tensors`)"""
    n = sum(t.numel() for t in tensors)
    grad, acc = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    views, o = [], 0
    for t in tensors:
        views.append(grad[o:o + t.numel()].view(t.shape))
        o += t.numel()
    return grad, acc, views


def _named(prefix, tensors):
    return {'%s%d' % (prefix, i): t for i, t in enumerate(tensors) if t is not None}


def _counter(dev, value=7):
    return torch.tensor([value], dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------ the loop on a cache
def _b_cached_loop(dev, family, C):
    from tests import test_epoch_call_gpu as eg
    case = next(c for c in eg.CASES if c[0] == family and c[2] == C)
    _, dtype, C, P, N, _, T, act, _, _ = case
    K, E = 12, 36
    cache = eg._cache(dtype, T, P, C, dev)
    flags = cof.APA_FLAG_TRAIN | (cof.APA_FLAG_RELU_ATT if act == 'relu' else 0)
    g = _gen(40 + C)
    rounds = []
    for r in range(3):
        idx = torch.randint(0, T, (N,), generator=g).to(torch.int32)
        if r == 1:
            idx[2] = T + 5          # an id outside the cache: clamped, and counted in cache.status by every replay
        rounds.append({'index': idx})

    def make():
        run = eg._Run(C, K, E, dev)
        cache.status.zero_()
        index = torch.zeros(N, dtype=torch.int32, device=dev)
        cb = cache.select(index)
        assert cb.index.data_ptr() == index.data_ptr()
        st = cof.HeadTrainStep(cb, cb, *run.w[:4], None, (None, None) + tuple(run.views), flags=flags,
                               keep_prob=eg.KEEP, seed=eg.SEED, offset=run.ctr)        # labels through the index
        sgd = cof.BoundMomentumSGD(run.segs, run.wd, run.grad, run.acc)

        def call():
            st.run()
            sgd.run(eg.LR0, eg.MOMENTUM, 1.0)
        state = dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, loss=st.loss, G=st.G, grad=run.grad,
                     acc=run.acc, ctr=run.ctr, status=cache.status, **_named('w', run.w))

        def after(r, snap):     # one id outside the cache in round 1; the counter advances by one per step
            assert int(snap['status']) == (0 if r == 0 else 1) and int(snap['ctr']) == eg.OFFSET + r + 1, r
        return Case(call, {'index': index}, state, ('logits', 'att', 'zsave', 'abar', 'loss', 'G'), ('loss', 'status'),
                    after=after)
    return make, rounds


def _b_cached_per_class(dev):
    from tests import test_cached_perclass_gpu as pc
    N, P, C, K = 4, 25, 2048, 51
    cache = pc._cache(P, C, dev)
    p0 = pc._params(C, K, 'id', cache, dev)
    flags = pc._flags('id', True)
    g = _gen(5)
    rounds = []
    for r in range(3):
        idx = torch.randint(0, pc.T, (N,), generator=g).to(torch.int32)
        if r == 1:
            idx[0] = -3
        rounds.append({'index': idx})
    order = ('Wa', 'ba', 'Wt', 'bt')

    def make():
        p = {k: p0[k].clone() for k in order}
        grad, acc, views = _bucket([p[k] for k in order], dev)
        ctr = _counter(dev, pc.OFFSET)
        cache.status.zero_()
        index = torch.zeros(N, dtype=torch.int32, device=dev)
        cb = cache.select(index)
        need = cof.attn_pool_workspace_bytes(N, P, C, C, K, K, flags | cof.APA_FLAG_FROZEN_INPUT)
        ws = torch.zeros(need + 256, dtype=torch.uint8, device=dev)     # kept by the caller: images, keep bits, their tag
        st = cof.HeadTrainStep(cb, cb, *[p[k] for k in order], None, (None, None) + tuple(views), flags=flags,
                               keep_prob=pc.KEEP, seed=pc.SEED, offset=ctr, weight_images=True, workspace=ws)
        assert st.weight_image_maps and st.workspace is ws
        images = [(order.index(role), m) for role, m in st.weight_image_maps]
        sgd = cof.BoundMomentumSGD([p[k] for k in order], [5e-4, 0.0, 5e-4, 0.0], grad, acc, images=images)

        def call():
            st.run()
            sgd.run(0.01, 0.9, 1.0)
        state = dict(logits=st.logits, att=st.att, zsave=st.zsave, loss=st.loss, G=st.G, grad=grad, acc=acc, ctr=ctr,
                     status=cache.status, workspace=ws, **p)

        def after(r, snap):
            assert int(snap['status']) == (0 if r == 0 else 1) and int(snap['ctr']) == pc.OFFSET + r + 1, r
        return Case(call, {'index': index}, state, ('logits', 'att', 'zsave', 'loss', 'G'), ('loss', 'status'),
                    after=after)
    return make, rounds


def _b_cached_clips(dev, loss):
    from tests import test_cached_clips_gpu as ccg
    from tests import test_feature_cache_gpu as fcg
    dtype, C, P, K, F, B, V = torch.float32, 1024, 6, 5, 3, ccg.B_, 3
    base = fcg._cache(dtype, P, C, dev)
    p0 = fcg._params(C, K, 'relu', base, dev)
    t0 = ccg._temporal(K, F, 3, dev)
    flags = fcg._flags('relu', True)
    g = _gen(77)
    rounds = []
    for r in range(3):
        videos = torch.randint(0, V, (B,), generator=g).to(torch.int32)
        if r == 1:
            videos[1] = 7           # outside [0, V): clamped by the sampler, counted
        rounds.append(dict(videos=videos, u=ccg._draws(B * F, seed=20 + r),
                           vlab=torch.randint(0, K, (V,), generator=g),
                           vtar=(torch.rand(V, K, generator=g) < 0.4).float()))
    order = ('Wa', 'ba', 'Wt', 'bt')

    def make():
        cache = cof.FeatureCache(base.features, base.labels)        # the shared frames, video tables of its own
        vlab = torch.zeros(V, dtype=torch.int64, device=dev)
        vtar = torch.zeros((V, K), dtype=torch.float32, device=dev)
        cache.set_videos(ccg.VID_FIRST, ccg.VID_COUNT, labels=vlab, targets=vtar)
        videos = torch.zeros(B, dtype=torch.int32, device=dev)
        u = torch.zeros(B * F, dtype=torch.float32, device=dev)
        clips = cof.CachedClips(cache, B, F)
        w = [p0[k].clone() for k in order] + [t0[0].clone(), t0[1].clone()]
        grad, acc, views = _bucket(w, dev)
        ctr = _counter(dev, ccg.OFFSET)
        st = cof.HeadTrainStep(clips, clips, *w[:4], clips.labels if loss == 'softmax-xentropy' else clips.targets,
                               (None, None) + tuple(views[:4]), flags=flags, keep_prob=ccg.KEEP, seed=ccg.SEED,
                               offset=ctr, loss_wt=1.3, grad_scale=0.5, frames=F, temporal=(w[4], w[5]),
                               temporal_grads=(views[4], views[5]), action_loss=loss)
        sgd = cof.BoundMomentumSGD(w, [4e-3, 0.0, 2e-3, 0.0, 1e-3, 0.0], grad, acc)

        def call():
            assert cache.sample_clips(videos, F, mode='random-segment', u=u, out=clips) is clips
            st.run()
            sgd.run(0.05, 0.9, 1.0)
        state = dict(index=clips.index, labels=clips.labels, targets=clips.targets, logits=st.logits, att=st.att,
                     zsave=st.zsave, abar=st.abar, loss=st.loss, G=st.G, pooled=st.pooled, tatt=st.tatt, grad=grad,
                     acc=acc, ctr=ctr, status=cache.status, **_named('w', w))
        return Case(call, dict(videos=videos, u=u, vlab=vlab, vtar=vtar), state,
                    ('index', 'labels', 'targets', 'logits', 'att', 'zsave', 'abar', 'loss', 'G', 'pooled', 'tatt'), 'loss')
    return make, rounds


# ------------------------------------------------------------------------------------------ the epoch calls
def _epoch_case():
    from tests import test_epoch_call_gpu as eg
    return eg, next(c for c in eg.CASES if c[0] == 'generic')      # f32 C = 40, P = 9, N = 8, 3 steps, T = 29


def _b_train_epoch(dev):
    eg, case = _epoch_case()
    _, dtype, C, P, N, steps, T, act, _, _ = case
    K, E = 12, 36
    cache = eg._cache(dtype, T, P, C, dev)
    flags = cof.APA_FLAG_TRAIN | (cof.APA_FLAG_RELU_ATT if act == 'relu' else 0)
    lr = [eg.LR0 * 0.5 ** s for s in range(steps)]
    rounds = []
    for r in range(3):
        order = cof._epoch_order_rule_cpu(T, 21, r)[:steps * N].clone()
        if r == 0:
            order[N + 2] = T + 3
        rounds.append({'order': order})

    def make():
        run = eg._Run(C, K, E, dev)
        cache.status.zero_()
        order = torch.zeros(steps * N, dtype=torch.int32, device=dev)
        ep = cof.HeadTrainEpoch(cache, N, *run.w[:4], tuple(run.views), run.segs, run.wd, run.grad, run.acc, steps=steps,
                                momentum=eg.MOMENTUM, labels_cached=True, flags=flags, keep_prob=eg.KEEP, seed=eg.SEED,
                                offset=run.ctr)

        def call():
            assert ep.run(order, lr) == steps
        state = dict(logits=ep.logits, att=ep.att, zsave=ep.zsave, abar=ep.abar, loss=ep.loss, G=ep.G, grad=run.grad,
                     acc=run.acc, ctr=run.ctr, status=cache.status, **_named('w', run.w))

        def after(r, snap):     # the device counter advances by `steps` per epoch; one id outside the cache in epoch 0
            assert int(snap['ctr']) == eg.OFFSET + (r + 1) * steps and int(snap['status']) == 1, r
        return Case(call, {'order': order}, state, ('logits', 'att', 'zsave', 'abar', 'loss', 'G'), 'loss', after=after)
    return make, rounds


def _b_eval_epoch(dev, scores):
    eg, _ = _epoch_case()
    T, P, N, K, C, count, cap = 29, 7, 8, 12, 1024, 19, 24         # test_validation_epoch_is_the_loop: count % N != 0
    cache = eg._cache(torch.float32, T, P, C, dev)
    Wa, ba, Wt, bt, _ = eg._weights(C, K, 1, dev)
    want_loss = scores == 'softmax'
    rounds = []
    for r in range(3):
        order = cof._epoch_order_rule_cpu(T, 4, r).clone()
        if r == 1:
            order[5] = T + 1
        rounds.append({'order': order})

    def make():
        cache.status.zero_()
        order = torch.zeros(T, dtype=torch.int32, device=dev)
        ep = cof.HeadEvalEpoch(cache, N, Wa, ba, Wt, bt, capacity=cap, flags=cof.APA_FLAG_RELU_ATT, scores=scores,
                               want_loss=want_loss)
        for t in (ep.logits, ep.probs, ep.pred, ep.att, ep.zsave, ep.abar) + ((ep.loss,) if want_loss else ()):
            t.zero_()               # rows past `count` are not written: the same in both instances

        def call():
            assert ep.run(order, count) == 3
        state = dict(logits=ep.logits, probs=ep.probs, pred=ep.pred, att=ep.att, zsave=ep.zsave, abar=ep.abar,
                     status=cache.status)
        if want_loss:
            state['loss'] = ep.loss
        return Case(call, {'order': order}, state, (), 'probs')
    return make, rounds


# ------------------------------------------------------------------------------------------ the bound steps
def _b_rank_step(dev):
    from tests import _rank_reference as rr
    c = rr.case_by_name('bf16_c2048_p49')                           # R = 2, bf16, training
    assert c['R'] == 2
    inp = rr.inputs(c)
    flags = cof.APA_FLAG_TRAIN | (cof.APA_FLAG_RELU_ATT if c['act'] == 'relu' else 0)
    rounds = _rounds(X=inp['X'], labels=inp['labels'])

    def make():
        d = rr.to_device(inp, dev)
        X = d['X'].clone()
        labels = d['labels'].clone()
        Wa = d['Wa'].view(-1, 1)
        like = lambda ts: [torch.zeros_like(t) for t in ts]
        grads = (torch.zeros_like(X), None, torch.zeros_like(Wa), torch.zeros_like(d['ba']), like(d['Wts']),
                 like(d['bts']), like(d['cw']), like(d['cb']))
        ctr = _counter(dev)
        st = cof.RankHeadTrainStep(X, X, Wa, d['ba'], d['Wts'], d['bts'], d['cw'], d['cb'], labels, grads, flags=flags,
                                   keep_prob=c['keep'], seed=11, offset=ctr)
        state = dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, z0=st.z0, loss=st.loss, G=st.G,
                     dX=grads[0], dWa=grads[2], dba=grads[3], ctr=ctr, **_named('dWt', grads[4]),
                     **_named('dbt', grads[5]), **_named('dcw', grads[6]), **_named('dcb', grads[7]))
        outs = tuple(k for k in state if k != 'ctr')
        return Case(st.run, dict(X=X, labels=labels), state, outs, 'logits')
    return make, rounds


def _pose_inputs(name):
    from tests import _pose_eval_ref as pe
    c = next(c for c in pe.CASES if c['name'] == name)
    return c, pe.make_inputs(c)


PARAMS = ('W1', 'b1', 'W2', 'b2', 'Wa', 'ba', 'Wt', 'bt')


def _b_pose_train(dev, name, form):
    c, inp = _pose_inputs(name)
    N, P, C, Cp, J, K = (c[k] for k in ('N', 'P', 'C', 'Cp', 'J', 'K'))
    g = _gen(N + K)
    F = 2 if form == 'clips' else 1
    B = N // F
    if form == 'multi-label':
        labels0 = (torch.rand(B, K, generator=g) < 0.3).float()
    else:
        labels0 = torch.randint(0, K, (B,), generator=g)
    pose_labels0 = torch.rand(N, P, J, generator=g)
    valid0 = (torch.rand(N, J, generator=g) < 0.7).to(torch.uint8)
    temporal0 = ((torch.randn(K, generator=g) * 0.1), torch.full((1,), 0.5))
    rounds = _rounds(X=inp['X'], labels=labels0, pose_labels=pose_labels0, pose_valid=valid0)
    flags = cof.APA_FLAG_TRAIN | c['flags']

    def make():
        X, labels = inp['X'].to(dev), labels0.to(dev)
        pose_labels, valid = pose_labels0.to(dev), valid0.to(dev)
        params = [inp[k].to(dev).reshape(-1, 1) if k == 'Wa' else inp[k].to(dev) for k in PARAMS]
        grads = [torch.zeros_like(X)] + [torch.zeros_like(t) for t in params]
        ctr = _counter(dev)
        kw = {}
        if form == 'clips':
            temporal = tuple(t.to(dev) for t in temporal0)
            tg = tuple(torch.zeros_like(t) for t in temporal)
            kw = dict(frames=F, temporal=temporal, temporal_grads=tg)
        if form == 'multi-label':
            kw = dict(action_loss='multi-label')
        st = cof.PoseAttnTrainStep(X, tuple(params), labels, pose_labels, valid, tuple(grads), flags=flags, keep_prob=0.5,
                                   seed=9, offset=ctr, **kw)
        state = {k: getattr(st, k) for k in ('Ppre', 'Pl', 'att', 'logits', 'zsave', 'abar', 'loss_action', 'loss_pose',
                                             'G', 'dPl', 'dZ')}
        state.update(_named('grad', grads))
        if form == 'clips':
            state.update(pooled=st.pooled, tatt=st.tatt, dtw=tg[0], dtb=tg[1])
        outs = tuple(state)
        state['ctr'] = ctr
        return Case(st.run, dict(X=X, labels=labels, pose_labels=pose_labels, pose_valid=valid), state, outs, 'logits')
    return make, rounds


def _b_pose_eval(dev, name, form):
    c, inp = _pose_inputs(name)
    N, K = c['N'], c['K']
    clips = form == 'clips'
    F = 2 if clips else 1
    g = _gen(3 * N + K)
    labels0 = torch.randint(0, K, (N // F,), generator=g)
    temporal0 = ((torch.randn(K, generator=g) * 0.1), torch.full((1,), 0.5))
    named = dict(X=inp['X']) if clips else dict(X=inp['X'], labels=labels0)      # the sigmoid scores take no labels
    rounds = _rounds(**named)
    want_route = c['route']

    def make():
        X = inp['X'].to(dev)
        params = tuple(inp[k].to(dev).reshape(-1, 1) if k == 'Wa' else inp[k].to(dev) for k in PARAMS)
        if clips:
            labels = None
            st = cof.PoseAttnEvalStep(X, params, None, flags=c['flags'], frames=F,
                                      temporal=tuple(t.to(dev) for t in temporal0), scores='sigmoid')
        else:
            labels = labels0.to(dev)
            st = cof.PoseAttnEvalStep(X, params, labels, flags=c['flags'])

        def call():
            st.run()
            assert st.route == want_route
        state = {k: getattr(st, k) for k in ('att', 'logits', 'zsave', 'abar', 'probs', 'pred')}
        if clips:
            state.update(pooled=st.pooled, tatt=st.tatt)
        else:
            state['loss'] = st.loss
        inputs = dict(X=X) if clips else dict(X=X, labels=labels)
        return Case(call, inputs, state, tuple(state), 'logits')
    return make, rounds


def _b_eval_step(dev, form):
    """HeadEvalStep, then apa_average_precision reading the step's score buffer, in one capture"""
    from tests import test_cached_clips_gpu as ccg
    from tests import test_feature_cache_gpu as fcg
    cached = form.startswith('cached')
    clips = form.endswith('clips')
    F = 3 if clips else 1
    if cached:
        dtype, C, P, K = torch.float32, 256, 49, 5
        cache = fcg._cache(dtype, P, C, dev)
        p = fcg._params(C, K, 'relu', cache, dev)
        N = (3 if clips else 5) * F
        T = N // F
        g = _gen(31)
        idx = torch.randint(0, fcg.T, (N,), generator=g).to(torch.int32)
        named = dict(index=idx)
    else:
        C, P, K = 64, 2, 7
        T = 5 if clips else 1025                                   # the rows of the score buffer: T <= 64 and T = 1025
        N = T * F
        g = _gen(32)
        X0 = torch.relu(torch.randn(N, P, C, generator=g)) * (0.5 + torch.rand(N, 1, 1, generator=g))
        u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
        p = dict(Wa=(u(C, 1) * (4.0 / C)).to(dev), ba=(u(1) * 0.1).to(dev), Wt=(u(C, K) / C ** 0.5).to(dev),
                 bt=(u(K) * 0.1).to(dev))
        named = dict(X=X0)
    sigmoid = clips
    if sigmoid:
        named['targets'] = (torch.rand(T, K, generator=g) < 0.4).float()
    else:
        named['labels'] = torch.randint(0, K, (T,), generator=g)
    temporal0 = ccg._temporal(K, F, 5, dev) if clips else None
    rounds = _rounds(**named)
    flags = cof.APA_FLAG_RELU_ATT

    def make():
        inputs = {k: v.to(dev) for k, v in named.items()}
        if cached:
            cache.status.zero_()
            X = cof.CachedClips(cache, T, F) if clips else cache.select(inputs['index'])
            if clips:
                inputs['index'] = X.index
        else:
            X = inputs['X']
        labels = inputs.get('labels')
        st = cof.HeadEvalStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, flags=flags, frames=F,
                              temporal=temporal0, scores='sigmoid' if sigmoid else 'softmax')
        out = torch.zeros(cof.average_precision_result_bytes(K), dtype=torch.uint8, device=dev)
        ws = torch.zeros(max(cof.average_precision_workspace_bytes(T, K), 16), dtype=torch.uint8, device=dev)

        def call():
            st.run()
            cof.average_precision(st.probs, labels=labels, targets=inputs.get('targets'), workspace=ws, out=out)
        state = dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, probs=st.probs, pred=st.pred,
                     ap_results=out)
        for k in ('loss', 'pooled', 'tatt'):
            if getattr(st, k, None) is not None:
                state[k] = getattr(st, k)
        outs = tuple(state)
        if cached:
            state['status'] = cache.status
        return Case(call, inputs, state, outs, 'probs')
    return make, rounds


def _b_eval_per_class(dev):
    from tests import test_cached_perclass_gpu as pc
    N, P, C, K = 3, 25, 2048, 51
    cache = pc._cache(P, C, dev)
    p = pc._params(C, K, 'id', cache, dev)
    rounds = _rounds(X=cache.features[:N].reshape(N, P, C).cpu())

    def make():
        X = rounds[0]['X'].to(dev)
        st = cof.HeadEvalStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], None, flags=0)
        state = dict(logits=st.logits, att=st.att, zsave=st.zsave, probs=st.probs, pred=st.pred)
        return Case(st.run, dict(X=X), state, tuple(state), 'probs')
    return make, rounds


def _plain_head(seed, N, P, C, K, dtype=torch.float32):
    g = _gen(seed)
    X = (torch.relu(torch.randn(N, P, C, generator=g)) * (0.5 + torch.rand(N, 1, 1, generator=g))).to(dtype)
    u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
    p = dict(Wa=u(C, 1) * (4.0 / C), ba=u(1) * 0.1, Wt=u(C, K) / C ** 0.5, bt=u(K) * 0.1)
    return g, X, p


def _b_train_step(dev, form):
    """HeadTrainStep on a plain batch: the four entry points behind it (the plain one through its C symbol)"""
    from tests import test_feature_cache_gpu as fcg
    N, P, C, K, F = 6, 49, 256, 12, 1                               # the vec family's smallest width
    g, X0, p0 = _plain_head(17, N, P, C, K)
    kw, B = {}, N
    if form == 'clips':
        F, B = 3, 2
    labels0 = (torch.rand(B, K, generator=g) < 0.3).float() if form == 'multi-label' else \
        torch.randint(0, K, (B,), generator=g)
    temporal0 = (torch.randn(K, generator=g) * 0.1, torch.full((1,), 0.4))
    rounds = _rounds(X=X0, labels=labels0)
    flags = cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT

    def make():
        X, labels = X0.to(dev), labels0.to(dev)
        p = {k: v.to(dev) for k, v in p0.items()}
        grads = (torch.zeros_like(X), None) + tuple(torch.zeros_like(p[k]) for k in ('Wa', 'ba', 'Wt', 'bt'))
        ctr = _counter(dev, fcg.OFFSET)
        kw = {}
        if form == 'clips':
            temporal = tuple(t.to(dev) for t in temporal0)
            kw = dict(frames=F, temporal=temporal, temporal_grads=tuple(torch.zeros_like(t) for t in temporal))
        if form == 'multi-label':
            kw = dict(action_loss='multi-label')
        st = cof.HeadTrainStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, grads, flags=flags, keep_prob=fcg.KEEP,
                               seed=fcg.SEED, offset=ctr, hooks=cof.make_hooks() if form == 'ex' else None, **kw)
        call = st.run
        if form == 'plain':         # the symbol without hooks: apa_attn_head_train_step_ex's arguments minus the first
            assert st._name == 'apa_attn_head_train_step' and st._pre == ()

            def call():
                rc = st.lib.apa_attn_head_train_step(*st._args, cof._stream_ptr())
                assert rc == 0, st.lib.apa_last_error().decode()
        else:
            assert st._name == {'ex': 'apa_attn_head_train_step', 'clips': 'apa_attn_head_train_step_clips',
                                'multi-label': 'apa_attn_head_train_step_multilabel'}[form]
        state = dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, loss=st.loss, G=st.G,
                     **_named('grad', grads))
        if form == 'clips':
            state.update(pooled=st.pooled, tatt=st.tatt, dtw=kw['temporal_grads'][0], dtb=kw['temporal_grads'][1])
        outs = tuple(state)
        state['ctr'] = ctr
        return Case(call, dict(X=X, labels=labels), state, outs, 'loss')
    return make, rounds


# ------------------------------------------------------------------------------------------ the separate calls
def _b_pool(dev, form):
    """forward, cross-entropy, backward as three calls; dropout offset by value"""
    from tests import test_feature_cache_gpu as fcg
    lib = cof.load_library()
    kw = dict(flags=cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT, keep_prob=fcg.KEEP, seed=fcg.SEED, offset=fcg.OFFSET)
    if form == 'cached':
        C, P, K, N = 1024, 49, 20, 5
        cache = fcg._cache(torch.float32, P, C, dev)
        p = fcg._params(C, K, 'relu', cache, dev)
        g = _gen(8)
        named = dict(index=torch.randint(0, fcg.T, (N,), generator=g).to(torch.int32),
                     G=(torch.rand(N, K, generator=g) * 1.25 - 0.25) / N)
    else:
        N, P, C, K = 5, 49, 1024, 20
        g, X0, p0 = _plain_head(23, N, P, C, K)
        p = {k: v.to(dev) for k, v in p0.items()}
        named = dict(X=X0, labels=torch.randint(0, K, (N,), generator=g))
    rounds = _rounds(**named)
    if form == 'cached':
        rounds[1]['index'] = rounds[1]['index'].clone()
        rounds[1]['index'][3] = fcg.T + 2

    def make():
        inputs = {k: v.to(dev) for k, v in named.items()}
        w = (p['Wa'], p['ba'], p['Wt'], p['bt'])
        state = {}
        if form == 'cached':
            cache.status.zero_()
            state['status'] = cache.status
            X = cache.select(inputs['index'])

            def call():
                logits, att, zsave, abar, _, ws = cof.attn_pool_fwd(X, X, *w, **kw)
                _, _, dWa, dba, dWt, dbt = cof.attn_pool_bwd(X, X, *w, att, zsave, abar, inputs['G'], workspace=ws,
                                                             want_dx=False, **kw)
                return dict(logits=logits, att=att, zsave=zsave, abar=abar, dWa=dWa, dba=dba, dWt=dWt, dbt=dbt)
        elif form == 'ex':
            X = inputs['X']

            def call():
                logits, att, zsave, abar, _, ws = cof.attn_pool_fwd(X, X, *w, **kw)
                loss, G, _, _ = cof.softmax_xent_fwd_bwd(logits, inputs['labels'])
                dX, _, dWa, dba, dWt, dbt = cof.attn_pool_bwd(X, X, *w, att, zsave, abar, G, workspace=ws, **kw)
                return dict(logits=logits, att=att, zsave=zsave, abar=abar, loss=loss, G=G, dX=dX, dWa=dWa, dba=dba,
                            dWt=dWt, dbt=dbt)
        else:                       # the symbols without hooks, on caller-owned buffers
            X = inputs['X']
            f32 = torch.float32
            new = lambda *s: torch.zeros(s, dtype=f32, device=dev)
            o = dict(logits=new(N, K), att=new(N, P, 1), zsave=new(N, C), abar=new(N), loss=new(1 + N), G=new(N, K),
                     dX=torch.zeros_like(X), dWa=new(C, 1), dba=new(1), dWt=new(C, K), dbt=new(K))
            state.update(o)
            nb = cof.attn_pool_workspace_bytes(N, P, C, C, K, 1, kw['flags'])
            ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device=dev)
            ptr = lambda t: t.data_ptr()
            tail = (ptr(ws), ws.numel(), N, P, C, C, K, 1, kw['flags'], kw['keep_prob'], kw['seed'], kw['offset'],
                    cof.APA_DTYPE_F32)

            def call():
                assert ws.data_ptr() == tail[0]      # (the workspace lives as long as this closure)
                st = cof._stream_ptr()
                rc = lib.apa_attn_pool_fwd(ptr(X), ptr(X), *[ptr(t) for t in w], ptr(o['logits']), ptr(o['att']),
                                           ptr(o['zsave']), ptr(o['abar']), None, *tail, st)
                assert rc == 0, lib.apa_last_error().decode()
                rc = lib.apa_softmax_xent_fwd_bwd(ptr(o['logits']), ptr(inputs['labels']), ptr(o['loss']), ptr(o['G']),
                                                  None, None, N, K, 1.0, 1.0, st)
                assert rc == 0, lib.apa_last_error().decode()
                rc = lib.apa_attn_pool_bwd(ptr(X), ptr(X), *[ptr(t) for t in w], ptr(o['att']), ptr(o['zsave']),
                                           ptr(o['abar']), ptr(o['G']), ptr(o['dX']), None, ptr(o['dWa']), ptr(o['dba']),
                                           ptr(o['dWt']), ptr(o['dbt']), *tail, st)
                assert rc == 0, lib.apa_last_error().decode()
        outs = tuple(k for k in state if k != 'status')
        return Case(call, inputs, state, outs, 'logits')
    return make, rounds


def _b_pool_cat(dev):
    N, P, C, K, J = 3, 25, 256, 9, 16
    g, X0, p0 = _plain_head(29, N, P, C + J, K)
    Xf, Xe = X0[..., :C].contiguous(), X0[..., C:].contiguous()
    p0['Wa'] = p0['Wa'][:C].contiguous()
    G0 = (torch.rand(N, K, generator=g) * 1.25 - 0.25) / N
    rounds = _rounds(X=Xf, Xext=Xe, G=G0)
    kw = dict(flags=cof.APA_FLAG_TRAIN, keep_prob=0.5, seed=3, offset=2)

    def make():
        X, Xext, G = Xf.to(dev), Xe.to(dev), G0.to(dev)
        w = tuple(p0[k].to(dev) for k in ('Wa', 'ba', 'Wt', 'bt'))

        def call():
            logits, att, zsave, abar, zext, ws = cof.attn_pool_fwd_cat(X, X, Xext, *w, **kw)
            r = cof.attn_pool_bwd_cat(X, X, Xext, zext, *w, att, zsave, abar, G, workspace=ws, **kw)
            out = dict(logits=logits, att=att, zsave=zsave, abar=abar, zext=zext)
            out.update({k: t for k, t in zip(('dX', 'dXatt', 'dXext', 'dWa', 'dba', 'dWt', 'dbt'), r) if t is not None})
            return out
        return Case(call, dict(X=X, Xext=Xext, G=G), {}, (), 'logits')
    return make, rounds


def _b_pool_rank(dev):
    from tests import _rank_reference as rr
    c = rr.case_by_name('f32_c96_p20')                              # R = 3, relu, the library's mask
    inp = rr.inputs(c)
    rounds = _rounds(X=inp['X'], G=inp['G'])
    kw = dict(flags=cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT, keep_prob=c['keep'], seed=11, offset=4)

    def make():
        d = rr.to_device(inp, dev)
        X, G = d['X'].clone(), d['G'].clone()
        a = (d['Wa'].view(-1, 1), d['ba'], d['Wts'], d['bts'], d['cw'], d['cb'])

        def call():
            logits, att, zsave, abar, z0, ws = cof.attn_pool_rank_fwd(X, X, *a, **kw)
            dX, _, dWa, dba, dWts, dbts, dcw, dcb = cof.attn_pool_rank_bwd(X, X, *a, att, zsave, abar, z0, G,
                                                                          workspace=ws, **kw)
            out = dict(logits=logits, att=att, zsave=zsave, abar=abar, z0=z0, dX=dX, dWa=dWa, dba=dba)
            for n, ts in (('dWt', dWts), ('dbt', dbts), ('dcw', dcw), ('dcb', dcb)):
                out.update(_named(n, ts))
            return out
        return Case(call, dict(X=X, G=G), {}, (), 'logits')
    return make, rounds


def _b_pose_head(dev, form):
    c, inp = _pose_inputs('composed_cp200' if form == 'no_dpl' else 'fused_softmax')
    N, P, C, Cp, J = (c[k] for k in ('N', 'P', 'C', 'Cp', 'J'))
    g = _gen(N + Cp)
    dPl0 = torch.rand(N, P, J, generator=g) * 1.25 - 0.25
    ext0 = (torch.rand(N, P, Cp, generator=g) * 1.25 - 0.25).to(inp['X'].dtype)
    row0, col0 = torch.rand(N * P, generator=g), torch.rand(Cp, generator=g) * 1.25 - 0.25
    named = dict(X=inp['X'])
    named.update(dict(plain=dict(dPl=dPl0), no_dpl=dict(ext=ext0), rank1=dict(dPl=dPl0, row=row0, col=col0))[form])
    rounds = _rounds(**named)

    def make():
        i = {k: v.to(dev) for k, v in named.items()}
        W1, b1, W2, b2 = (inp[k].to(dev) for k in ('W1', 'b1', 'W2', 'b2'))

        def call():
            Ppre, Pl, ws = cof.pose_head_fwd(i['X'], W1, b1, W2, b2)
            if form == 'plain':     # the bf16 copy of W1 the forward call left in the workspace is reused
                r = cof.pose_head_bwd(i['X'], W1, W2, Ppre, i['dPl'], None, workspace=ws, ws_from_fwd=True)
            elif form == 'no_dpl':  # dW2 = 0 by hipMemsetAsync
                r = cof.pose_head_bwd(i['X'], W1, W2, Ppre, None, i['ext'])
            else:
                r = cof.pose_head_bwd(i['X'], W1, W2, Ppre, i['dPl'], None, ext_rank1=(i['row'], i['col']))
            out = dict(Ppre=Ppre, Pl=Pl)
            out.update(zip(('dX', 'dW1', 'db1', 'dW2', 'db2'), r))
            return out
        return Case(call, i, {}, (), 'dW1')
    return make, rounds


def _b_pose_att(dev, hooks):
    from tests import _pal_stage as ps
    c = ps.BY_NAME['m4_repeat_c12_acc']                              # training, a repeated part, accumulate_dX
    I = ps.make_inputs(c)
    rounds = _rounds(X=I['X'], Pl=I['Pl'], G=I['G'])
    for r in range(3):              # the two accumulated outputs start from the same values in every round
        rounds[r].update(dPl=I['dPl0'], dX=I['dX0'])
    kw = dict(flags=cof.APA_FLAG_TRAIN, keep_prob=c['keep'], seed=ps.SEED, offset=ps.OFFSET)

    def make():
        i = {k: I[k].to(dev) for k in ('X', 'Pl', 'G')}
        i['dPl'], i['dX'] = I['dPl0'].to(dev), I['dX0'].to(dev)
        W, b = I['W'].to(dev), I['b'].to(dev)
        h = cof.make_hooks() if hooks else None

        def call():
            F, logits, ws = cof.pose_att_logits_fwd(i['X'], i['Pl'], c['sel'], c['avged'], W, b, hooks=h, **kw)
            _, _, dW, db = cof.pose_att_logits_bwd(i['X'], i['Pl'], c['sel'], c['avged'], W, F, i['G'], i['dPl'],
                                                   dX=i['dX'], accumulate_dX=True, workspace=ws, hooks=h, **kw)
            return dict(F=F, logits=logits, dW=dW, db=db)
        return Case(call, i, dict(dPl_acc=i['dPl'], dX_acc=i['dX']), (), 'logits')
    return make, rounds


# ------------------------------------------------------------------------------------------ the losses
def _b_xent(dev, N, K, want_grad):
    g = _gen(N * K)
    rounds = _rounds(logits=torch.randn(N, K, generator=g) * 2.5, labels=torch.randint(0, K, (N,), generator=g))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            loss, G, probs, pred = cof.softmax_xent_fwd_bwd(i['logits'], i['labels'], wt=0.7, grad_scale=3.0,
                                                            want_grad=want_grad, want_probs=want_grad, want_pred=True)
            return {k: t for k, t in dict(loss=loss, G=G, probs=probs, pred=pred).items() if t is not None}
        return Case(call, i, {}, (), 'loss')
    return make, rounds


def _b_action_loss(dev):
    from tests import test_support_paths_gpu as sp
    N, K = sp.ACTION_SHAPES[1]
    r = sp._rng(13, N, K)
    x = torch.from_numpy(sp._action_logits(r, N, K, 'extreme'))
    rounds = _rounds(logits=x, labels=torch.from_numpy(sp._action_labels(r, 'l2', N, K, 'mix')),
                     targets=torch.from_numpy(sp._action_labels(r, 'multi-label', N, K, 'mix')))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            out = {}
            for kind in ('l2', 'multi-label', 'multi-label-2'):
                loss, G = cof.action_loss_fwd_bwd(kind, i['logits'], i['labels' if kind == 'l2' else 'targets'],
                                                  wt=sp.WT, grad_scale=sp.GS, pos_weight=10.0)
                out['loss_' + kind], out['G_' + kind] = loss, G
            return out
        return Case(call, i, {}, (), 'G_l2')
    return make, rounds


def _b_multilabel_loss(dev):
    N, K = 9, 157
    g = _gen(N + K)
    rounds = _rounds(logits=torch.randn(N, K, generator=g) * 2.5, targets=(torch.rand(N, K, generator=g) < 0.3).float())

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            out = {}
            for kind in ('multi-label', 'multi-label-2'):
                out['loss_' + kind], out['G_' + kind] = cof.multilabel_loss_fwd_bwd(kind, i['logits'], i['targets'],
                                                                                    wt=0.7, grad_scale=3.0)
            return out
        return Case(call, i, {}, (), 'loss_multi-label')
    return make, rounds


def _b_clip_loss(dev, loss):
    B, F, K = 3, 3, 157
    g = _gen(B + K)
    labels0 = torch.randint(0, K, (B,), generator=g) if loss == 'softmax-xentropy' else \
        (torch.rand(B, K, generator=g) < 0.3).float()
    rounds = _rounds(logits=torch.randn(B * F, K, generator=g), labels=labels0)
    w0, b0 = torch.randn(K, generator=g) * 0.1, torch.full((1,), 0.4)

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        w, b = w0.to(dev), b0.to(dev)

        def call():
            if loss == 'softmax-xentropy':
                r = cof.clip_xent_fwd_bwd(i['logits'], i['labels'], F, w, b, wt=1.3, grad_scale=0.5)
            else:
                r = cof.clip_multilabel_fwd_bwd(loss, i['logits'], i['labels'], F, w, b, wt=1.3, grad_scale=0.5)
            return dict(zip(('pooled', 'tatt', 'loss', 'G', 'dw', 'db'), r))
        return Case(call, i, {}, (), 'loss')
    return make, rounds


def _b_pose_l2(dev):
    from tests import test_support_paths_gpu as sp
    N, P, J = sp.POSE_L2_SHAPES[0]
    g = _gen(N * P * J)
    rounds = _rounds(Pl=torch.randn(N, P, J, generator=g), lbl=torch.rand(N, P, J, generator=g),
                     valid=(torch.rand(N, J, generator=g) < 0.6).to(torch.uint8))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            return dict(zip(('loss', 'dPl'), cof.pose_l2_loss_fwd_bwd(i['Pl'], i['lbl'], i['valid'], wt=0.7, grad_scale=3.0)))
        return Case(call, i, {}, (), 'loss')
    return make, rounds


def _b_pose_sampled(dev):
    from tests import test_support_paths_gpu as sp
    Pl, lbl, u, valid, _ = sp._sampled_inputs((3, 25, 13))
    t = torch.from_numpy
    rounds = _rounds(Pl=t(Pl), lbl=t(np.ascontiguousarray(lbl)), u=t(np.ascontiguousarray(u)),
                     valid=t(valid.astype(np.uint8)))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            return dict(zip(('loss', 'dPl', 'mask'), cof.pose_sampled_loss_fwd_bwd(i['Pl'], i['lbl'], i['valid'], i['u'],
                                                                                  wt=0.7, grad_scale=3.0)))
        return Case(call, i, {}, (), 'loss')
    return make, rounds


def _b_frame_pool(dev):
    B, F, K = 2, 25, 157
    g = _gen(B * F + K)
    rounds = _rounds(logits=torch.randn(B * F, K, generator=g), dpooled=torch.randn(B, K, generator=g))
    w0, b0 = torch.randn(K, generator=g) * 0.1, torch.full((1,), 0.4)

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        w, b = w0.to(dev), b0.to(dev)

        def call():
            pooled, tatt = cof.frame_pool_fwd(i['logits'], F, w, b)
            dlogits, dw, db = cof.frame_pool_bwd(i['logits'], F, w, tatt, i['dpooled'])
            mean, _ = cof.frame_pool_fwd(i['logits'], F)
            dmean, _, _ = cof.frame_pool_bwd(i['logits'], F, None, None, i['dpooled'])
            return dict(pooled=pooled, tatt=tatt, dlogits=dlogits, dw=dw, db=db, mean=mean, dmean=dmean)
        return Case(call, i, {}, (), 'pooled')
    return make, rounds


def _b_clip_scores(dev):
    B, F, K = 3, 3, 157
    g = _gen(2 * B + K)
    rounds = _rounds(logits=torch.randn(B * F, K, generator=g), labels=torch.randint(0, K, (B,), generator=g))
    w0, b0 = torch.randn(K, generator=g) * 0.1, torch.full((1,), 0.4)

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        w, b = w0.to(dev), b0.to(dev)

        def call():
            a = cof.clip_scores(i['logits'], F, w, b, kind='softmax', labels=i['labels'])
            s = cof.clip_scores(i['logits'], F, kind='sigmoid')
            out = dict(zip(('pooled', 'tatt', 'scores', 'pred', 'loss'), a))
            out.update(sig_pooled=s[0], sig_scores=s[2], sig_pred=s[3])
            return out
        return Case(call, i, {}, (), 'scores')
    return make, rounds


# ------------------------------------------------------------------------------------------ optimisers, elementwise
def _b_optimiser(dev, kind):
    from tests import test_support_paths_gpu as sp
    sizes, wd, images = sp.SIZES, sp.WD, None
    shadows = () if kind == 'sgd' else sp.SHADOW_SEGS
    slots = dict(sgd=(0.0,), shadow=(0.0,), images=(0.0,), adam=(0.0, 0.0), rmsprop=(1.0, 0.0))[kind]
    if kind == 'images':
        sizes, wd, shadows = [3, 12 * 5, 7 * 3], [0.0, sp.f32(5e-4), sp.f32(5e-4)], (2,)
    total = sum(sizes)
    g = _gen(total)
    rounds = _rounds(grad=torch.randn(total, generator=g))

    def make():
        p = sp._Params(dev, 7, sizes=sizes, slots=slots, shadows=shadows)
        state = dict(w=p.wflat, **_named('slot', p.slots), **_named('shadow', p.shadows))
        if kind == 'images':
            dsts = [torch.full((n,), sp.IMG_FILL, dtype=dt, device=dev) for _, dt, n, *_ in sp.IMAGES]
            imgs = [(seg, sp._wimg(dst, dt == torch.float32, *m)) for dst, (seg, dt, n, *m) in zip(dsts, sp.IMAGES)]
            state.update(_named('image', dsts))
        if kind in ('sgd', 'shadow', 'images'):
            opt = cof.BoundMomentumSGD(p.weights, wd, p.grad, p.slots[0], shadows=p.shadows if shadows else None,
                                       images=imgs if kind == 'images' else None)
            assert opt._who == {'sgd': 'apa_momentum_sgd_step', 'shadow': 'apa_momentum_sgd_step_shadow',
                                'images': 'apa_momentum_sgd_step_images'}[kind]
            call = lambda: opt.run(sp.LRS[0], sp.f32(0.9), 0.5)
        elif kind == 'adam':
            call = lambda: cof.adam_step(p.weights, wd, p.grad, p.slots[0], p.slots[1], sp.LRS[0], 2, epsilon=1e-6,
                                         grad_scale=0.5, shadows=p.shadows)
        else:
            call = lambda: cof.rmsprop_step(p.weights, wd, p.grad, p.slots[0], p.slots[1], sp.LRS[0], decay=0.9,
                                            momentum=0.9, epsilon=1e-10, grad_scale=0.5, shadows=p.shadows)
        return Case(call, dict(grad=p.grad), state, (), 'w')
    return make, rounds


def _b_accumulate(dev):
    n, nparts = 1027, 9              # more than APA_ACC_MAX_PARTS parts: folded through `out` in two launches
    g = _gen(n)
    rounds = _rounds(**{'part%d' % i: torch.randn(n, generator=g) for i in range(nparts)})

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        parts = [i['part%d' % q] for q in range(nparts)]
        a, b = torch.zeros(n, device=dev), torch.zeros(n, device=dev)

        def call():
            cof.accumulate_gradients(a, parts, divisor=3.0)
            cof.accumulate_gradients(b, parts, scale=1.0 / 3.0)
        return Case(call, i, dict(div=a, scaled=b), ('div', 'scaled'), 'div')
    return make, rounds


def _b_spatial_mean_bwd(dev):
    N, P, C = 3, 49, 12
    rounds = _rounds(dz=torch.randn(N, C, generator=_gen(N * C)))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            return dict(f32=cof.spatial_mean_bwd(i['dz'], (N, P, C), torch.float32),
                        bf16=cof.spatial_mean_bwd(i['dz'], (N, 7, 7, C), torch.bfloat16))
        return Case(call, i, {}, (), 'f32')
    return make, rounds


def _b_zero_out_channels(dev):
    C = 5
    g = _gen(C)
    rounds = _rounds(x=torch.randn(3, 4, 4, C, generator=g), channels=torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        return Case(lambda: dict(out=cof.zero_out_channels(i['x'], i['channels'])), i, {}, (), 'out')
    return make, rounds


def _b_dropout_mask(dev):
    def make():
        return Case(lambda: dict(mask=cof.dropout_mask((3, 49, 40), 0.2, 1234, 7, device=dev)), {}, {}, (), 'mask')
    return make, [{}, {}, {}]


def _b_weight_images(dev):
    from tests import test_cached_perclass_gpu as pc
    N, P, C, K = 4, 25, 2048, 51
    p0 = pc._params(C, K, 'id', pc._cache(P, C, dev), dev)
    rounds = _rounds(**{k: v.cpu() for k, v in p0.items()})

    def make():
        p = {k: v.clone() for k, v in p0.items()}
        nb = cof.attn_pool_workspace_bytes(N, P, C, C, K, K, cof.APA_FLAG_TRAIN)
        ws = torch.zeros(nb, dtype=torch.uint8, device=dev)

        def call():
            assert cof.per_class_weight_images(p['Wa'], p['ba'], p['Wt'], p['bt'], ws, N, P, torch.bfloat16)
        return Case(call, p, dict(workspace=ws), (), 'workspace')
    return make, rounds


def _b_resize(dev):
    rounds = _rounds(img=torch.rand(2, 7, 9, 3, generator=_gen(4)))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        return Case(lambda: dict(out=cof.resize_bilinear_tf1(i['img'], 7, 9), up=cof.resize_bilinear_tf1(i['img'], 15, 15)),
                    i, {}, (), 'up')
    return make, rounds


# ------------------------------------------------------------------------------------------ cache and input kernels
def _b_fp8_quantize(dev):
    N, P, C = 3, 6, 32
    g = _gen(N + P + C)
    X0 = torch.relu(torch.randn(N, P, C, generator=g)) * torch.tensor([1.0, 37.0, 1e-3]).view(N, 1, 1)
    rounds = _rounds(X=X0)
    rounds[2]['X'] = rounds[2]['X'].clone()
    rounds[2]['X'][1, 2, 3] = float('inf')          # status 1 for image 1: its codes and scale are zero

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            q, status = cof.quantize_features(i['X'])
            qb, _ = cof.quantize_features(i['X'].to(torch.bfloat16))
            return dict(buffer=q.buffer, status=status, buffer_bf16=qb.buffer, back=q.dequantize(),
                        back_bf16=q.dequantize(torch.bfloat16))
        return Case(call, i, {}, (), 'buffer')
    return make, rounds


def _b_fp8_quantize_at(dev):
    T, P, C = 7, 6, 32
    g = _gen(T + P + C)
    rounds = _rounds(X=torch.relu(torch.randn(3, P, 1, C, generator=g)) * 5.0)

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        cache = cof.FeatureCache.empty((T, P, 1, C), torch.float8_e4m3fn, dev)

        def call():
            return dict(status=cache.write(2, i['X']))
        return Case(call, i, dict(buffer=cache.features.buffer), (), 'buffer')
    return make, rounds


def _b_sample_clips(dev):
    """the sampler alone, in its 'uniform' mode (the 'random-segment' mode runs in the clip rows)"""
    from tests import test_cached_clips_gpu as ccg
    F, K, V = 25, 5, len(ccg.V_FIRST)
    g = _gen(F)
    rounds = []
    for r in range(3):
        videos = torch.tensor(ccg.VIDEOS, dtype=torch.int32).roll(r)
        rounds.append(dict(videos=videos, vlab=torch.randint(0, 1 << 40, (V,), generator=g),
                           vtar=(torch.rand(V, K, generator=g) < 0.3).float()))
    B = len(ccg.VIDEOS)

    def make():
        cache = cof.FeatureCache(torch.zeros(ccg.T_FRAMES, 1, 1, 16, device=dev))
        vlab = torch.zeros(V, dtype=torch.int64, device=dev)
        vtar = torch.zeros((V, K), dtype=torch.float32, device=dev)
        cache.set_videos(ccg.V_FIRST.tolist(), ccg.V_COUNT.tolist(), labels=vlab, targets=vtar)
        videos = torch.zeros(B, dtype=torch.int32, device=dev)
        clips = cof.CachedClips(cache, B, F)
        state = dict(index=clips.index, labels=clips.labels, targets=clips.targets, status=cache.status)

        def call():
            assert cache.sample_clips(videos, F, mode='uniform', out=clips) is clips
        return Case(call, dict(videos=videos, vlab=vlab, vtar=vtar), state, ('index', 'labels', 'targets'), 'index')
    return make, rounds


def _b_epoch_order(dev):
    T = 1000

    def make():
        out = torch.zeros(T, dtype=torch.int32, device=dev)

        def call():
            assert cof.epoch_order(T, 11, 5, dev, out=out) is out
        return Case(call, {}, dict(order=out), ('order',), 'order')
    return make, [{}, {}, {}]


def _b_pose_labels(dev):
    """the raw entry point on device-resident inputs (the Python wrapper copies from the host)"""
    from tests import test_label_reference_gpu as lr
    lib = cof.load_library()
    c = lr._case(lr.RASTER[0])
    m = c['meta']
    T, J, side = m['T'], m['J'], m['side']
    pose0 = torch.from_numpy(np.ascontiguousarray(c['in/pose']).astype(np.int64))
    nv0 = torch.from_numpy(np.ascontiguousarray(c['in/n_vals']).astype(np.int32))
    geom0 = torch.tensor([c['in/geom'].tolist()] * T, dtype=torch.int32)
    assert pose0.dim() == 2 and pose0.shape[0] == T and int(nv0.max()) <= pose0.shape[1]
    flipped = geom0.clone()
    flipped[:, 8] = 1 - flipped[:, 8]
    hidden = pose0.clone()
    hidden[:, 2::3] = 0              # no keypoint visible
    rounds = [dict(pose=pose0, geom=geom0), dict(pose=pose0, geom=flipped), dict(pose=hidden, geom=flipped)]
    max_vals = int(pose0.shape[1])

    def make():
        pose, geom, nv = pose0.to(dev), geom0.to(dev), nv0.to(dev)
        labels = torch.zeros((T, side, side, J), dtype=torch.float32, device=dev)
        valid = torch.zeros((T, J), dtype=torch.uint8, device=dev)
        status = torch.zeros((T,), dtype=torch.int32, device=dev)

        def call():
            rc = lib.apa_pose_labels_device(pose.data_ptr(), nv.data_ptr(), geom.data_ptr(), T, max_vals,
                                            max(200, side), J, float(m['marker_wd_ratio_cfg']), side, labels.data_ptr(),
                                            valid.data_ptr(), status.data_ptr(), cof._stream_ptr())
            assert rc == 0, lib.apa_last_error().decode()
        return Case(call, dict(pose=pose, geom=geom), dict(labels=labels, valid=valid, status=status),
                    ('labels', 'valid', 'status'), 'labels')
    return make, rounds


def _b_preprocess_images(dev):
    """the raw entry point on device-resident inputs, as test_other_refusals_of_the_kernel calls it"""
    from tests import test_image_preproc_gpu as ip
    lib = cof.load_library()
    c = ip._case('b_short_by_one')
    good = c['in/geom'].tolist()                     # [37, 53, 23, 34, 0, 0, 16, 16, 0]
    frames = torch.from_numpy(np.ascontiguousarray(c['in/frames']).reshape(-1))
    assert frames.dtype == torch.uint8 and frames.numel() == 37 * 53 * 3
    geom0 = torch.tensor([good], dtype=torch.int32)
    flipped = geom0.clone()
    flipped[0, 8] = 1
    rounds = [dict(src=frames, geom=geom0), dict(src=frames.flip(0).contiguous(), geom=geom0),
              dict(src=frames, geom=flipped)]

    def make():
        src, geom = frames.to(dev), geom0.to(dev)
        off = torch.zeros(1, dtype=torch.int64, device=dev)
        hw = torch.tensor([[37, 53]], dtype=torch.int32, device=dev)
        out = torch.zeros((1, 1, 16, 16, 3), device=dev)
        st = torch.zeros((1,), dtype=torch.int32, device=dev)
        hw_host = (ctypes.c_int32 * 2)(37, 53)
        need = int(lib.apa_preprocess_images_workspace_bytes(1, 1, hw_host, 512))
        ws = torch.zeros(max(need, 64), dtype=torch.uint8, device=dev)

        def call():
            rc = lib.apa_preprocess_images(src.data_ptr(), src.numel(), off.data_ptr(), hw.data_ptr(), geom.data_ptr(), 1,
                                           1, 512, 128.0, out.data_ptr(), 0, st.data_ptr(), ws.data_ptr(), ws.numel(),
                                           cof._stream_ptr())
            assert rc == 0, lib.apa_last_error().decode()
        return Case(call, dict(src=src, geom=geom), dict(out=out, status=st), ('out', 'status'), 'out')
    return make, rounds


def _b_explain(dev):
    from tests import test_explain_gpu as ex
    N, Pn, C, K, T, per_class, kind = ex.CASES[6]                    # class ids -1 and K: clamped, counted in `status`
    X0, Wa, ba, Wt, bt = ex._inputs(N, Pn, C, K, per_class, 3)
    att0 = torch.rand(N, Pn, 1, generator=_gen(6))
    rounds = _rounds(X=X0, att=att0, classes=ex._classes(N, K, T, kind))

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}
        Wtd, btd = Wt.to(dev), bt.to(dev)

        def call():
            return dict(zip(('topdown', 'combined', 'class_logit', 'status'),
                            cof.attn_explain(i['X'], i['att'], Wtd, btd, i['classes'])))
        return Case(call, i, {}, (), 'topdown')
    return make, rounds


def _b_overlay(dev):
    g = _gen(12)
    rounds = _rounds(maps=torch.rand(2, 3, 7, 7, generator=g), images=torch.rand(2, 30, 30, 3, generator=g) * 255 - 128)

    def make():
        i = {k: v.to(dev) for k, v in rounds[0].items()}

        def call():
            u8, f32 = cof.attention_overlay(i['maps'], i['images'], want_f32=True)
            return dict(u8=u8, f32=f32)
        return Case(call, i, {}, (), 'f32')
    return make, rounds


# ------------------------------------------------------------------------------------------ the test
@pytest.mark.parametrize('r', ROWS, ids=[r['id'] for r in ROWS])
def test_replay_equals_eager(gpu, r):
    make, rounds = globals()['_b_' + r['build']](gpu, *r['args'])
    gr.replay_equals_eager(r['id'] + ' (' + ', '.join(r['entries']) + ')', make, rounds, frozen=r['frozen'])


# ------------------------------------------------------------------------------------------ what a capture freezes
def _capture(call):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    torch.cuda.synchronize()
    return graph


def test_what_a_capture_freezes(gpu):
    """Arguments that travel by value are part of the captured launches: the dropout offset given as an int, the epoch's
    `lr[s]` (read from the host array when the call is enqueued) and everything `rebind` / `run` marshal.  Every replay
    then repeats the call AS CAPTURED -- `rebind(offset=...)` or another `lr` afterwards changes nothing in the graph.
    What a replay re-reads lives in HBM: the device dropout counter (the replays advance), the index / order / label
    buffers, the weights."""
    from tests import test_epoch_call_gpu as eg
    _, dtype, C, P, N, steps, T, act, _, _ = next(c for c in eg.CASES if c[0] == 'generic')
    K, E = 12, 36
    cache = eg._cache(dtype, T, P, C, gpu)
    flags = cof.APA_FLAG_TRAIN
    index = torch.arange(N, dtype=torch.int32, device=gpu)

    def step(offset):
        run = eg._Run(C, K, E, gpu)
        cb = cache.select(index)
        st = cof.HeadTrainStep(cb, cb, *run.w[:4], None, (None, None) + tuple(run.views), flags=flags, keep_prob=eg.KEEP,
                               seed=eg.SEED, offset=run.ctr if offset is None else offset)
        return st, run
    eager = {}
    for off in (eg.OFFSET, eg.OFFSET + 1, eg.OFFSET + 2):
        st, _ = step(off)
        st.run()
        torch.cuda.synchronize()
        eager[off] = st.loss.clone()
    assert not torch.equal(eager[eg.OFFSET], eager[eg.OFFSET + 1])
    # by value: every replay is the step at the captured offset, whatever rebind says afterwards
    st, _ = step(eg.OFFSET)
    graph = _capture(st.run)
    for i in range(3):
        if i == 1:
            st.rebind(offset=eg.OFFSET + 1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(st.loss, eager[eg.OFFSET]), i
    st.run()                                                          # the eager call does follow the rebind
    torch.cuda.synchronize()
    assert torch.equal(st.loss, eager[eg.OFFSET + 1])
    # the device counter: the replays advance
    st, run = step(None)
    graph = _capture(st.run)
    run.ctr.fill_(eg.OFFSET)
    for i in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(run.ctr) == eg.OFFSET + i + 1 and torch.equal(st.loss, eager[eg.OFFSET + i]), i

    # ---- the epoch call: lr[s] and an int offset are frozen; the order buffer and the device counter are not
    order = cache.order(21, 3)[:steps * N].clone()
    lr_a, lr_b = [eg.LR0 * 0.5 ** s for s in range(steps)], [eg.LR0 * 3.0] * steps

    def epoch(offset):
        run = eg._Run(C, K, E, gpu)
        ep = cof.HeadTrainEpoch(cache, N, *run.w[:4], tuple(run.views), run.segs, run.wd, run.grad, run.acc, steps=steps,
                                momentum=eg.MOMENTUM, flags=flags, keep_prob=eg.KEEP, seed=eg.SEED,
                                offset=run.ctr if offset is None else offset)
        return ep, run

    def snap(ep, run):
        torch.cuda.synchronize()
        return [ep.loss.clone(), run.acc.clone()] + [w.clone() for w in run.w]
    want = []
    ep, run = epoch(eg.OFFSET)
    for lr in (lr_a, lr_a):                                           # two eager epochs, the same offset and rates
        ep.run(order, lr)
        want.append(snap(ep, run))
    ep, run = epoch(eg.OFFSET)
    init = snap(ep, run)
    graph = _capture(lambda: ep.run(order, lr_a))
    for dst, src in zip([ep.loss, run.acc] + run.w, init):
        dst.copy_(src)
    run.grad.zero_()
    for i in range(2):
        if i == 1:
            ep._lr[:steps] = lr_b                                     # the host array the call read when it was enqueued
        graph.replay()
        for got, w in zip(snap(ep, run), want[i]):
            assert torch.equal(got, w), i
    ep.run(order, lr_b, offset=eg.OFFSET)                             # an eager call does take the new rates
    assert not torch.equal(snap(ep, run)[2], want[1][2])
    # the device counter advances by `steps` per replayed epoch
    ep, run = epoch(None)
    graph = _capture(lambda: ep.run(order, lr_a))
    run.ctr.fill_(eg.OFFSET)
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert int(run.ctr) == eg.OFFSET + (i + 1) * steps
