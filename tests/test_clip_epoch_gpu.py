"""A whole clip / multi-label epoch behind one host call, on the GPU.

The oracle of every new entry point is the sequence it is defined as, run with the entry points that existed before it:
* apa_sample_clip_frames_keyed == apa_sample_clip_frames fed the host restatement of the draws;
* the training epoch == `sample_clips_keyed(step=s, out=clips)` + `HeadTrainStep.rebind(offset=) + run()` +
  `BoundMomentumSGD.run(lr[s])` per step -- every weight, accumulator, output, the whole loss log and `status`;
* the evaluation epoch == `FeatureCache.sample_clips(..., 'uniform')` + `HeadEvalStep` per batch, the last batch shorter;
* on a cache whose videos are its images, both epochs == the flat epoch calls (HeadTrainEpoch / HeadEvalEpoch);
* deploy.FusedHeadStep.train_video_epoch / FusedHeadEval.evaluate_videos == the per-batch deploy loops;
* a captured hipGraph of each entry point replays its eager calls (tests/_graph_replay.py), and freezes the key.
Every comparison is torch.equal: the library has no floating-point atomics.

One fixture: 7 videos of 1, 2, 3, 5, 9, 4 and 6 frames (n = 1, n < F and n = F at F = 3), T = 30 maps of 3x3x64, K = 8;
training runs B = 2 videos x F = 3 frames for 3 steps, evaluation 7 videos at B = 3 (the last batch holds one)."""
import os

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import clip_epoch as ce
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _graph_replay as gr
from tests import _ref_fixture as rf
from tests.test_epoch_call_gpu import _guarded, _guards_untouched      # outputs between sentinel elements
from tests.test_graph_replay_gpu import _capture                       # warm up on a side stream, capture one call

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
DTYPES = [torch.float32, torch.bfloat16, F8]
DTYPE_IDS = ['f32', 'bf16', 'fp8']
LOSSES = ('softmax-xentropy', 'multi-label', 'multi-label-2')
COUNTS = [1, 2, 3, 5, 9, 4, 6]
FIRST = [int(v) for v in np.cumsum([0] + COUNTS[:-1])]
V, T, P, C, K = len(COUNTS), sum(COUNTS), 9, 64, 8
B, F, STEPS = 2, 3, 3
SEED, OFFSET, KEEP = 1234, 7, 0.5
KEY = dict(seed=2 ** 63 + 11, epoch=5)               # the sampler's
MOMENTUM, LR0 = 0.9, 2e-3           # (small: the sigmoid losses must not saturate within three steps)
NAN = float('nan')
assert T == 30
# the training epoch's videos: n = 9 (the one video whose segments have a choice at F = 3) in every step, beside n = 1,
# n = 2 < F and n = 3 = F; ids may repeat
TRAIN_ORDER = [4, 0, 1, 4, 4, 2]
assert len(TRAIN_ORDER) == STEPS * B

# ------------------------------------------------------------------------------------------ inputs
_CACHES = {}


def _cache(dtype, dev):
    """T frames of relu(randn) with a per-frame magnitude, the video tables with labels and multi-hot targets; built
    once per dtype, never written afterwards (status apart)"""
    if dtype not in _CACHES:
        g = torch.Generator().manual_seed(77)
        mag = 0.25 + 4.0 * torch.rand((T, 1, 1, 1), generator=g)
        img = (torch.relu(torch.randn(T, 3, 3, C, generator=g)) * mag).to(dev)
        vlab = torch.randint(0, K, (V,), generator=g).to(dev)
        vtar = (torch.rand(V, K, generator=g) < 0.3).float()
        vtar[2] = 0.0                                                       # a video without a positive
        cache = cof.FeatureCache.empty((T, 3, 3, C), dtype, dev)
        assert cache.write(0, img).tolist() == [0] * T
        cache.set_videos(FIRST, COUNTS, labels=vlab, targets=vtar.to(dev))
        _CACHES[dtype] = cache
    return _CACHES[dtype]


def _weights(dev, temporal):
    """Wa, ba, Wt, bt, an extra segment that only decays, and the temporal conv's (w [K], b [1]) behind them"""
    g = torch.Generator().manual_seed(5)
    u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
    w = [(u(C, 1) * (4.0 / C)).to(dev), (u(1) * 0.1 - 0.3).to(dev), (u(C, K) / C ** 0.5).to(dev), (u(K) * 0.1).to(dev),
         u(36).to(dev)]
    if temporal:
        w += [(torch.randn(K, generator=g) * (0.3 / K ** 0.5)).to(dev),
              (torch.full((1,), 1.0 / F) + 0.1 * torch.randn(1, generator=g)).to(dev)]
    return w


WD = [4e-3, 0.0, 2e-3, 0.0, 1e-2, 3e-3, 0.0]       # (Wa, ba, Wt, bt, extra, tw, tb)
SEGMENTS = [2, 0, 5, 4, 3, 6, 1]                   # the bucket's order: Wt, Wa, tw, extra, bt, tb, ba


class _Run(object):
    """one route's own state: weights, flat gradient bucket (the extra segment's window stays zero), accumulators"""

    def __init__(self, dev, temporal):
        self.w = _weights(dev, temporal)
        seg = [i for i in SEGMENTS if i < len(self.w)]
        n = sum(t.numel() for t in self.w)
        self.grad = torch.zeros((n,), device=dev)
        self.acc = (torch.rand((n,), generator=torch.Generator().manual_seed(3)) * 1e-3).to(dev)
        self.segs, self.wd = [self.w[i] for i in seg], [WD[i] for i in seg]
        o, views = 0, {}
        for i, t in zip(seg, self.segs):
            views[i] = self.grad[o:o + t.numel()].view(t.shape)
            o += t.numel()
        self.views = [views[i] for i in range(4)]                                # dWa, dba, dWt, dbt
        self.temporal = (self.w[5], self.w[6]) if temporal else None
        self.tgrads = (views[5], views[6]) if temporal else None
        self.ctr = torch.tensor([OFFSET], dtype=torch.int64, device=dev)

    def tensors(self):
        return dict(grad=self.grad, acc=self.acc, ctr=self.ctr, **{'w%d' % i: t for i, t in enumerate(self.w)})


def _video_order(seed, epoch, dev, n=None):
    o = cof.epoch_order(V, seed, epoch, dev)
    return o if n is None else o[:n].clone()


# ------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize('frames', [1, 3, 25])
@pytest.mark.parametrize('mode', ['uniform', 'random-segment'])
def test_keyed_sampler_is_the_sampler_on_the_restated_draws(gpu, mode, frames):
    cache = _cache(torch.float32, gpu)
    for videos, bad in (([4, 0, 6, 2, 1, 3, 5, 4], 0), ([4, 9, 6, -3, 1], 2)):          # the second run: two ids outside
        nb = len(videos)
        for step in (0, 1):
            u = ce.clip_draws_rule_cpu(nb, frames, KEY['seed'], KEY['epoch'], step).to(gpu)
            cache.status.zero_()
            want = cache.sample_clips(videos, frames, mode=mode, u=u)
            assert int(cache.status) == bad
            cache.status.zero_()
            got = ce.sample_clips_keyed(cache, videos, frames, mode, step=step, **KEY)
            assert isinstance(got, cof.CachedClips) and got.frames == frames and int(cache.status) == bad
            assert torch.equal(got.index, want.index), (mode, frames, step)
            assert torch.equal(got.labels, want.labels) and torch.equal(got.targets, want.targets)
            assert 0 <= int(got.index.min()) and int(got.index.max()) < T
            # identical calls give identical bits; out= rewrites the same buffers, inside them
            ptr = got.index.data_ptr()
            first = got.index.clone()
            got.index.fill_(-1)
            assert ce.sample_clips_keyed(cache, videos, frames, mode, step=step, out=got, **KEY) is got
            assert got.index.data_ptr() == ptr and torch.equal(got.index, first)
    # the key matters exactly where a segment has a choice: video 4 (9 frames) at F = 3 draws from segments of 2 frames
    if mode == 'random-segment' and frames == 3:
        idx = [ce.sample_clips_keyed(cache, [4] * 16, 3, mode, seed=1, epoch=2, step=s).index.clone() for s in (0, 1)]
        assert not torch.equal(idx[0], idx[1])
        assert not torch.equal(idx[0], ce.sample_clips_keyed(cache, [4] * 16, 3, mode, seed=1, epoch=3, step=0).index)
        assert not torch.equal(idx[0], ce.sample_clips_keyed(cache, [4] * 16, 3, mode, seed=2, epoch=2, step=0).index)
    cache.status.zero_()


# ------------------------------------------------------------------------------------------ the training epoch
def _loop_and_epoch(dev, dtype, loss, temporal, frames, mode='random-segment', rng_dev=False):
    """-> (epoch object, its run, the bound step of the loop, its run, the loop's loss log, (status loop, status epoch),
    a function that runs one more one-step epoch on both routes)"""
    cache = _cache(dtype, dev)
    flags = cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT
    N = B * frames
    order = torch.tensor(TRAIN_ORDER, dtype=torch.int32, device=dev)
    lr = [LR0 * 0.5 ** s for s in range(STEPS)]
    multi = loss != 'softmax-xentropy'
    kw = dict(flags=flags, keep_prob=KEEP, seed=SEED, loss_wt=1.3, grad_scale=0.5, action_loss=loss)

    # ---- the loop, with the entry points the epoch call is defined by
    L = _Run(dev, temporal)
    clips = ce.sample_clips_keyed(cache, order[:B], frames, mode, step=0, **KEY)
    st = cof.HeadTrainStep(clips, clips, *L.w[:4], clips.targets if multi else clips.labels,
                           (None, None) + tuple(L.views), offset=L.ctr if rng_dev else OFFSET, frames=frames,
                           temporal=L.temporal, temporal_grads=L.tgrads, **kw)
    sgd = cof.BoundMomentumSGD(L.segs, L.wd, L.grad, L.acc)

    def loop(order, lrs, first_offset):
        cache.status.zero_()
        log = []
        for s in range(len(lrs)):
            ce.sample_clips_keyed(cache, order[s * B:(s + 1) * B], frames, mode, step=s, out=clips, **KEY)
            if not rng_dev:
                st.rebind(offset=first_offset + s)
            st.run()
            sgd.run(lrs[s], MOMENTUM, 1.0)
            log.append(st.loss.clone())
        return torch.stack(log), int(cache.status)
    log, status_loop = loop(order, lr, OFFSET)
    assert st.frozen_input and st.dX_scratch is None and st._name == (
        'apa_attn_head_train_step_cached' if not multi and frames == 1 and not temporal
        else 'apa_attn_head_train_step_cached_clips')

    # ---- the epoch call, every output inside guards, one spare row in the log
    E = _Run(dev, temporal)
    shapes = dict(logits=(N, K), att=(N, P, 1), zsave=(N, C), abar=(N,), loss=(STEPS + 1, 1 + B), G=(N, K))
    guards = {k: _guarded(s, torch.float32, dev) for k, s in shapes.items()}
    ep = ce.ClipTrainEpoch(cache, B, frames, *E.w[:4], tuple(E.views), E.segs, E.wd, E.grad, E.acc, steps=STEPS + 1,
                           temporal=E.temporal, temporal_grads=E.tgrads, mode=mode, momentum=MOMENTUM,
                           offset=E.ctr if rng_dev else OFFSET, outputs={k: v for k, (_, v) in guards.items()}, **kw)
    cache.status.zero_()
    out = ep.run(order, lr, **KEY)
    torch.cuda.synchronize()
    status_epoch = int(cache.status)
    assert out.data_ptr() == ep.loss.data_ptr() and tuple(out.shape) == (STEPS, 1 + B)
    assert torch.equal(out, log) and bool(torch.isnan(ep.loss[STEPS]).all())
    for k, (whole, view) in guards.items():
        _guards_untouched(whole, view.numel())

    def one_more(order1, lr1, first_offset):
        want, s_loop = loop(order1, [lr1], first_offset)
        cache.status.zero_()
        got = ep.run(order1, lr1, offset=None if rng_dev else first_offset, **KEY)
        torch.cuda.synchronize()
        return got, want, int(cache.status), s_loop
    return ep, E, st, L, clips, log, (status_loop, status_epoch), one_more


def _same_state(ep, E, st, L, clips, temporal, frames):
    for (name, a), b in zip(E.tensors().items(), L.tensors().values()):
        assert torch.equal(a, b), name
    for k in ('logits', 'att', 'zsave', 'abar', 'G'):                       # the last step's
        assert torch.equal(getattr(ep, k), getattr(st, k).view(getattr(ep, k).shape)), k
    if frames != 1 or temporal:
        assert torch.equal(ep.pooled, st.pooled)
    if temporal:
        assert torch.equal(ep.tatt, st.tatt)
    else:
        assert ep.tatt is None
    assert torch.equal(ep.index, clips.index) and torch.equal(ep.labels, clips.labels)
    assert torch.equal(ep.targets, clips.targets)


@pytest.mark.parametrize('temporal', [False, True], ids=['mean', 'temporal'])
@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_training_epoch_is_the_loop(gpu, dtype, loss, temporal):
    ep, E, st, L, clips, log, status, one_more = _loop_and_epoch(gpu, dtype, loss, temporal, F)
    _same_state(ep, E, st, L, clips, temporal, F)
    assert status == (0, 0)
    assert bool(torch.isfinite(log).all()) and float(log[:, 0].min()) > 0
    assert not torch.equal(E.w[4], _weights(gpu, temporal)[4])              # the extra segment did decay
    if temporal:
        assert not torch.equal(E.w[5], _weights(gpu, temporal)[5])          # the temporal conv was trained
    assert float(ep.G.abs().max()) > 0                                      # the last step still had a gradient
    # an off-by-one in the learning rate, the dropout offset, the sampler's step or the batch would show
    assert not torch.equal(log[0], log[1]) and not torch.equal(log[1], log[2])
    # a second run on the bound objects: one step, one video id outside [0, V) -- clamped, and counted once
    bad = torch.tensor([V + 2, 2], dtype=torch.int32, device=gpu)
    got, want, s_epoch, s_loop = one_more(bad, 0.01, OFFSET + STEPS)
    assert torch.equal(got, want) and (s_epoch, s_loop) == (1, 1)
    _same_state(ep, E, st, L, clips, temporal, F)
    assert int(ep.index[:F].min()) >= FIRST[6] and int(ep.index[:F].max()) < T      # clamped to the last video


@pytest.mark.parametrize('loss', LOSSES[1:])
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_flat_multilabel_epoch_is_the_loop_on_one_frame_videos(gpu, dtype, loss):
    """HICO's form: one frame per video (frames = 1, no clip descriptor), under both sigmoid losses"""
    ep, E, st, L, clips, log, status, _ = _loop_and_epoch(gpu, dtype, loss, False, 1)
    assert ep._clip is None and ep.pooled is None
    _same_state(ep, E, st, L, clips, False, 1)
    assert status == (0, 0) and bool(torch.isfinite(log).all())
    i4, i2 = ep.index.tolist()                                              # the last batch: videos 4 and 2
    assert FIRST[4] <= i4 < FIRST[5] and FIRST[2] <= i2 < FIRST[3]


def test_training_epoch_uniform_frames_and_the_device_dropout_counter(gpu):
    ep, E, st, L, clips, log, status, one_more = _loop_and_epoch(gpu, torch.bfloat16, 'softmax-xentropy', True, F,
                                                                 mode='uniform', rng_dev=True)
    _same_state(ep, E, st, L, clips, True, F)
    assert int(E.ctr) == int(L.ctr) == OFFSET + STEPS and status == (0, 0)
    with pytest.raises(cof.ApaError, match='device-side dropout counter'):
        ep.run(_video_order(1, 1, gpu, B), 0.1, offset=3)
    with pytest.raises(cof.ApaError, match='whole batches'):
        ep.run(_video_order(1, 1, gpu, B + 1), 0.1)
    with pytest.raises(cof.ApaError, match='one learning rate per step'):
        ep.run(_video_order(1, 1, gpu, 2 * B), [0.1])


# ------------------------------------------------------------------------------------------ the evaluation epoch
EB, CAP = 3, 9                    # 7 videos at B = 3: steps of 3, 3 and 1 videos; two spare rows


def _eval_loop(cache, w, temporal, scores, order, count, frames, want_loss):
    rows = dict(probs=[], pred=[], pooled=[], loss=[], labels=[], targets=[])
    cache.status.zero_()
    for a in range(0, count, EB):
        clips = cache.sample_clips(order[a:min(a + EB, count)], frames, mode='uniform')
        st = cof.HeadEvalStep(clips, clips, *w[:4], clips.labels if want_loss else None, flags=cof.APA_FLAG_RELU_ATT,
                              frames=frames, temporal=temporal, scores=scores)
        st.run()
        rows['probs'].append(st.probs.clone()), rows['pred'].append(st.pred.clone())
        rows['pooled'].append((st.pooled if st.pooled is not None else st.logits).clone())
        rows['labels'].append(clips.labels.clone()), rows['targets'].append(clips.targets.clone())
        if want_loss:
            rows['loss'].append(st.loss.clone())
    return rows, st, int(cache.status)


@pytest.mark.parametrize('form', ['softmax_loss_temporal', 'softmax_mean', 'sigmoid_temporal', 'sigmoid_one_frame'])
@pytest.mark.parametrize('dtype', DTYPES, ids=DTYPE_IDS)
def test_validation_epoch_is_the_loop(gpu, dtype, form):
    scores = form.split('_')[0]
    want_loss, with_t = 'loss' in form, 'temporal' in form
    frames = 1 if 'one_frame' in form else F
    cache = _cache(dtype, gpu)
    w = _weights(gpu, True)
    temporal = (w[5], w[6]) if with_t else None
    order = _video_order(4, 1, gpu).clone()
    order[5] = V + 4                                                        # one id outside: clamped, counted once
    count, steps, last = V, 3, 1
    rows, st, status_loop = _eval_loop(cache, w, temporal, scores, order, count, frames, want_loss)
    # ---- the epoch call: per-video outputs of CAP rows pre-filled, everything inside guards
    N = EB * frames
    clips_form = frames != 1 or with_t
    shapes = dict(probs=(CAP, K), logits=(N, K) if clips_form else (CAP, K), att=(N, P, 1), zsave=(N, C), abar=(N,))
    if clips_form:
        shapes['pooled'] = (CAP, K)
    if with_t:
        shapes['tatt'] = (N,)
    if want_loss:
        shapes['loss'] = (steps, 1 + EB)
    guards = {k: _guarded(s, torch.float32, gpu) for k, s in shapes.items()}
    guards['pred'] = _guarded((CAP,), torch.int64, gpu)
    ep = ce.ClipEvalEpoch(cache, EB, frames, *w[:4], capacity=CAP, temporal=temporal, flags=cof.APA_FLAG_RELU_ATT,
                          scores=scores, want_loss=want_loss, outputs={k: v for k, (_, v) in guards.items()})
    for k in ('probs', 'pooled') + (('loss',) if want_loss else ()):
        getattr(ep, k).fill_(NAN)
    ep.pred.fill_(-5), ep.labels.fill_(-5), ep.targets.fill_(NAN)
    cache.status.zero_()
    assert ep.run(order, count) == steps
    torch.cuda.synchronize()
    for k in ('probs', 'pred', 'pooled', 'labels', 'targets'):
        got = getattr(ep, k)
        assert torch.equal(got[:count], torch.cat(rows[k])), k
        tail = got[count:]                                                   # nothing is written past row `count`
        assert bool(torch.isnan(tail).all()) if got.dtype.is_floating_point else tail.tolist() == [-5] * (CAP - count)
    assert bool(torch.isfinite(ep.probs[:count]).all())
    assert torch.equal(ep.labels[:count], cache.video_labels[order.long().clamp(0, V - 1)])
    assert torch.equal(ep.targets[:count], cache.video_targets[order.long().clamp(0, V - 1)])
    if want_loss:
        for s in range(steps):
            n = 1 + (last if s == steps - 1 else EB)
            assert torch.equal(ep.loss[s, :n], rows['loss'][s]), s
            assert bool(torch.isnan(ep.loss[s, n:]).all())
    nl = last * frames                                                       # the last step's, in its rows
    for k in ('att', 'zsave', 'abar') + (('logits',) if clips_form else ()) + (('tatt',) if with_t else ()):
        assert torch.equal(getattr(ep, k)[:nl], getattr(st, k)), k
    for k, (whole, view) in guards.items():
        _guards_untouched(whole, view.numel())
    assert int(cache.status) == status_loop == 1
    # ---- a DeviceEvaluation fed by the call == one fed batch by batch
    from attentionalpoolingaction_amd import eval_utils
    multi = scores == 'sigmoid'
    want = eval_utils.DeviceEvaluation(CAP, K, gpu, multi_label=multi)
    for p, t in zip(rows['probs'], rows['targets' if multi else 'labels']):
        want.update(p, t)
    meter = eval_utils.DeviceEvaluation(CAP, K, gpu, multi_label=multi)
    dst, truth = meter.reserve(count)
    ep.run(order, count, probs=dst, **({'targets': truth} if multi else {'labels': truth}))
    assert torch.equal(meter._scores[:count], want._scores[:count]) and torch.equal(meter._truth[:count], want._truth[:count])
    ra, rb = meter.result(), want.result()
    assert ra['aps'] == rb['aps'] and np.array_equal(ra['ap_per_class'], rb['ap_per_class'])
    assert (ra['mAP'] == rb['mAP'] or (np.isnan(ra['mAP']) and np.isnan(rb['mAP']))) and np.array_equal(ra['npos'], rb['npos'])
    cache.status.zero_()


# ------------------------------------------------------------------------------------------ the two epoch interfaces
def test_one_frame_videos_are_the_flat_epoch(gpu):
    """The clip epoch calls and the flat epoch calls of apa.h run one driver; on a cache whose videos are its images
    (one frame each, video labels = image labels) they are the same epoch.  T = 10 maps of 3x3x32 in bf16, K = 5,
    N = B = 4: training visits 8 ids in 2 steps under dropout, evaluation 10 rows in steps of 4, 4 and 2."""
    T1, C1, K1, N1 = 10, 32, 5, 4
    g = torch.Generator().manual_seed(91)
    img = torch.relu(torch.randn(T1, 3, 3, C1, generator=g)) * (0.25 + 4.0 * torch.rand((T1, 1, 1, 1), generator=g))
    labels = torch.randint(0, K1, (T1,), generator=g).to(gpu)
    cache = cof.FeatureCache.empty((T1, 3, 3, C1), torch.bfloat16, gpu, labels=labels)
    assert cache.write(0, img.to(gpu)).tolist() == [0] * T1
    cache.set_videos(torch.arange(T1), torch.ones(T1, dtype=torch.int64), labels=labels)
    w0 = [(torch.rand(C1, 1, generator=g) * (4.0 / C1)), torch.rand(1, generator=g) * 0.1 - 0.3,
          (torch.rand(C1, K1, generator=g) - 0.25) / C1 ** 0.5, torch.rand(K1, generator=g) * 0.1]
    n = sum(t.numel() for t in w0)
    acc0 = torch.rand((n,), generator=g) * 1e-3

    def state():
        w, grad, o, views = [t.clone().to(gpu) for t in w0], torch.zeros((n,), device=gpu), 0, []
        for t in w:
            views.append(grad[o:o + t.numel()].view(t.shape))
            o += t.numel()
        return w, views, grad, acc0.clone().to(gpu)
    # ---- training: 2 steps, ids may repeat
    order = torch.tensor([7, 2, 9, 0, 3, 3, 5, 8], dtype=torch.int32, device=gpu)
    lr = [LR0, LR0 * 0.5]
    kw = dict(steps=2, momentum=MOMENTUM, flags=cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT, keep_prob=KEEP, seed=SEED,
              offset=OFFSET, loss_wt=1.3, grad_scale=0.5)
    wf, vf, gf, af = state()
    flat = cof.HeadTrainEpoch(cache, N1, *wf, tuple(vf), wf, [4e-3, 0.0, 2e-3, 0.0], gf, af, labels_cached=True, **kw)
    assert flat.run(order, lr) == 2
    wc, vc, gc, ac = state()
    clip = ce.ClipTrainEpoch(cache, N1, 1, *wc, tuple(vc), wc, [4e-3, 0.0, 2e-3, 0.0], gc, ac, **kw)
    log = clip.run(order, lr, **KEY)
    torch.cuda.synchronize()
    assert clip._clip is None and tuple(log.shape) == (2, 1 + N1)
    assert torch.equal(log, flat.loss) and bool(torch.isfinite(log).all()) and not torch.equal(log[0], log[1])
    for k, (a, b) in enumerate(zip(wc, wf)):
        assert torch.equal(a, b) and not torch.equal(a, w0[k].to(gpu)), k
    assert torch.equal(gc, gf) and torch.equal(ac, af)
    for k in ('logits', 'G', 'att', 'zsave', 'abar'):                       # the last step's
        assert torch.equal(getattr(clip, k), getattr(flat, k)), k
    assert float(clip.G.abs().max()) > 0
    assert torch.equal(clip.index, order[N1:]) and torch.equal(clip.labels, labels[order[N1:].long()])
    # ---- evaluation: all 10 rows, the last step holds 2
    order = cof.epoch_order(T1, 3, 1, gpu)
    ekw = dict(capacity=T1, flags=cof.APA_FLAG_RELU_ATT, scores='softmax', want_loss=True)
    ef = cof.HeadEvalEpoch(cache, N1, *wf, **ekw)
    ec = ce.ClipEvalEpoch(cache, N1, 1, *wf, **ekw)
    ef.loss.fill_(NAN), ec.loss.fill_(NAN)
    assert ef.run(order, T1) == ec.run(order, T1) == 3
    torch.cuda.synchronize()
    assert ec._clip is None and ec.pooled is ec.logits
    for k in ('probs', 'pred', 'logits'):
        assert torch.equal(getattr(ec, k), getattr(ef, k)), k
    assert torch.equal(ec.loss[:2], ef.loss[:2]) and torch.equal(ec.loss[2, :3], ef.loss[2, :3])
    assert bool(torch.isfinite(ec.loss[2, :3]).all()) and bool(torch.isnan(ec.loss[2, 3:]).all())
    for k in ('att', 'zsave', 'abar'):                                      # the last step's two rows
        assert torch.equal(getattr(ec, k)[:2], getattr(ef, k)[:2]), k
    assert torch.equal(ec.labels, labels[order.long()]) and int(cache.status) == 0


# ------------------------------------------------------------------------------------------ deploy
DEPLOY =[('vstep_temporal_att_train', False), ('vstep_framepool_train', False), ('mlstep_clip_temporal_ml', True),
          ('mlstep_flat002_ml2_c32', True)]
D_COUNTS = [1, 2, 3, 5, 4]


def _load(fx, gpu):
    from tests import test_video_step_gpu as vst
    return vst._load(fx, gpu)[:2]


def _fixture_frame_cache(fx, dtype, gpu):
    """15 frames made of the fixture's (cycled, each with its own magnitude) as 5 videos of 1, 2, 3, 5 and 4 frames, with
    labels inside the head's classes and multi-hot targets"""
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu)
    frames = images.reshape(-1, *images.shape[-3:])
    n, Tn, Kn = frames.shape[0], sum(D_COUNTS), int(fx.meta['num_classes'])
    g = torch.Generator().manual_seed(17)
    mag = (0.5 + torch.rand((Tn, 1, 1, 1), generator=g)).to(gpu)
    cache = cof.FeatureCache.empty((Tn,) + tuple(frames.shape[1:]), dtype, gpu)
    assert cache.write(0, frames[[i % n for i in range(Tn)]] * mag).tolist() == [0] * Tn
    cache.set_videos([int(v) for v in np.cumsum([0] + D_COUNTS[:-1])], D_COUNTS,
                     labels=torch.randint(0, Kn, (len(D_COUNTS),), generator=g).to(gpu),
                     targets=(torch.rand(len(D_COUNTS), Kn, generator=g) < 0.25).float().to(gpu))
    return cache


def _deploy_frames(fx):
    return int(fx.arrays['in/images'].shape[1]) if fx.arrays['in/images'].ndim == 5 else 1


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name,multi', DEPLOY, ids=[d[0] for d in DEPLOY])
def test_train_video_epoch_is_the_deploy_loop(gpu, name, multi, dtype):
    from attentionalpoolingaction_amd import config as apa_config, deploy
    Bv, steps = 2, 2
    try:
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_%s.npz' % name))
        Fv = _deploy_frames(fx)
        cache = _fixture_frame_cache(fx, dtype, gpu)
        order = cof.epoch_order(len(D_COUNTS), 3, 0, gpu)[:steps * Bv].clone()
        lrs = [0.02 * 0.5 ** s for s in range(steps)]
        key = dict(seed=5, epoch=2)

        def state(net, fused, opt):
            out = {n: t.data.clone() for n, t in fused.params.items()}
            out.update(acc=opt.acc.clone(), bucket=fused.bucket.flat.clone())
            return out
        # ---- the deploy loop with the keyed draws
        net_b, cfg_b = _load(fx, gpu)
        net_b.head.seed, net_b.head._step = 99, 5
        fb = deploy.FusedHeadStep(net_b, cfg_b, frozen_features=True)
        ob = fb.make_optimizer(0.02)
        log, clips = [], None
        for s in range(steps):
            clips = ce.sample_clips_keyed(cache, order[s * Bv:(s + 1) * Bv], Fv, 'random-segment', step=s, out=clips, **key)
            total, _ = fb(clips, None)
            total.backward()
            ob.step(lr=lrs[s])
            log.append(fb._step_obj.loss.clone())
        want = state(net_b, fb, ob)
        assert (net_b.temporal is not None) == ('temporal' in name)
        # ---- one call
        net_a, cfg_a = _load(fx, gpu)
        net_a.head.seed, net_a.head._step = 99, 5
        fa = deploy.FusedHeadStep(net_a, cfg_a, frozen_features=True)
        oa = fa.make_optimizer(0.02)
        out = fa.train_video_epoch(cache, Bv, Fv, order, lr=lrs, **key)
        assert tuple(out.shape) == (steps, 1 + Bv) and out.is_cuda and torch.equal(out, torch.stack(log))
        assert net_a.head._step == net_b.head._step == 5 + steps
        got = state(net_a, fa, oa)
        assert set(got) == set(want)
        for k, v in want.items():
            assert torch.equal(got[k], v), k
        assert float(oa.acc.abs().max()) > 0 and int(cache.status) == 0
        # lr=None: the optimiser's own rate, on the bound epoch call
        bound = fa._video_epoch
        fa.train_video_epoch(cache, Bv, Fv, order[:Bv], **key)
        assert fa._video_epoch is bound and net_a.head._step == 5 + steps + 1
    finally:
        apa_config.reset_cfg()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('name,multi', DEPLOY, ids=[d[0] for d in DEPLOY])
def test_evaluate_videos_is_the_deploy_loop(gpu, name, multi, dtype):
    from attentionalpoolingaction_amd import config as apa_config, deploy
    Bv, Vn = 2, len(D_COUNTS)
    try:
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_%s.npz' % name))
        Fv = _deploy_frames(fx)
        net, cfg = _load(fx, gpu)
        net.head.is_training = False                            # evaluation draws no mask: the same weights, no dropout
        cache = _fixture_frame_cache(fx, dtype, gpu)
        ev = deploy.FusedHeadEval(net, cfg)
        assert ev.multi_label == multi
        order = cof.epoch_order(Vn, 8, 2, gpu)
        want = ev.new_evaluation(Vn)
        for a in range(0, Vn, Bv):                              # batches of 2, 2 and 1 videos
            clips = cache.sample_clips(order[a:a + Bv], Fv, mode='uniform')
            scores, _, _ = ev(clips)
            want.update(scores, clips.targets if multi else clips.labels)
        meter = ev.evaluate_videos(cache, Bv, Fv, order=order)
        assert len(meter) == Vn and torch.equal(meter._scores[:Vn], want._scores[:Vn])
        assert torch.equal(meter._truth[:Vn], want._truth[:Vn])
        ra, rb = meter.result(), want.result()
        assert ra['aps'] == rb['aps'] and np.array_equal(ra['ap_per_class'], rb['ap_per_class'])
        assert np.array_equal(ra['npos'], rb['npos'])
        if not multi:
            assert ra['accuracy'] == rb['accuracy']
        # a meter that already holds rows; the default order is the table's own
        m2 = ev.new_evaluation(3 + Vn)
        m2.update(want._scores[:3], want._truth[:3])
        bound = ev.video_epoch
        assert ev.evaluate_videos(cache, Bv, Fv, meter=m2) is m2 and len(m2) == 3 + Vn and ev.video_epoch is bound
        plain = ev.new_evaluation(Vn)
        for a in range(0, Vn, Bv):
            clips = cache.sample_clips(list(range(a, min(a + Bv, Vn))), Fv, mode='uniform')
            plain.update(ev(clips)[0], clips.targets if multi else clips.labels)
        assert torch.equal(m2._scores[3:], plain._scores[:Vn]) and torch.equal(m2._truth[3:], plain._truth[:Vn])
        assert int(cache.status) == 0
    finally:
        apa_config.reset_cfg()


# ------------------------------------------------------------------------------------------ hipGraph replay
def _b_sample_clips_keyed(dev):
    cache = _cache(torch.float32, dev)
    rounds = [{'videos': torch.tensor(v, dtype=torch.int32)} for v in ([4, 0, 6, 2], [3, 11, 4, 4], [1, 5, 2, 4])]

    def make():
        cache.status.zero_()
        videos = torch.zeros(4, dtype=torch.int32, device=dev)
        clips = cof.CachedClips(cache, 4, F)

        def call():
            assert ce.sample_clips_keyed(cache, videos, F, 'random-segment', step=2, out=clips, **KEY) is clips
        state = dict(index=clips.index, labels=clips.labels, targets=clips.targets, status=cache.status)

        def after(r, snap):         # one id outside [0, V) in round 1
            assert int(snap['status']) == (0 if r == 0 else 1), r
        return gr.Case(call, {'videos': videos}, state, ('index', 'labels', 'targets'), 'index', after=after)
    return make, rounds


def _video_rounds(n, bad_round):
    rounds = []
    for r in range(3):
        order = cof._epoch_order_rule_cpu(V, 21, r)[:n].clone()
        if r == bad_round:
            order[1] = V + 3
        rounds.append({'order': order})
    return rounds


def _b_train_epoch_clips(dev, loss):
    cache = _cache(torch.bfloat16, dev)
    lr = [LR0 * 0.5 ** s for s in range(STEPS)]

    def make():
        run = _Run(dev, True)
        cache.status.zero_()
        order = torch.zeros(STEPS * B, dtype=torch.int32, device=dev)
        ep = ce.ClipTrainEpoch(cache, B, F, *run.w[:4], tuple(run.views), run.segs, run.wd, run.grad, run.acc,
                               steps=STEPS, temporal=run.temporal, temporal_grads=run.tgrads, action_loss=loss,
                               momentum=MOMENTUM, flags=cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT, keep_prob=KEEP,
                               seed=SEED, offset=run.ctr)

        def call():
            assert tuple(ep.run(order, lr, **KEY).shape) == (STEPS, 1 + B)
        state = dict(logits=ep.logits, att=ep.att, zsave=ep.zsave, abar=ep.abar, loss=ep.loss, G=ep.G, pooled=ep.pooled,
                     tatt=ep.tatt, index=ep.index, labels=ep.labels, targets=ep.targets, status=cache.status,
                     **run.tensors())

        def after(r, snap):     # the device counter advances by STEPS per epoch; one id outside [0, V) in epoch 0
            assert int(snap['ctr']) == OFFSET + (r + 1) * STEPS and int(snap['status']) == 1, r
        return gr.Case(call, {'order': order}, state,
                       ('logits', 'att', 'zsave', 'abar', 'loss', 'G', 'pooled', 'tatt', 'index', 'labels', 'targets'),
                       'loss', after=after)
    return make, _video_rounds(STEPS * B, 0)


def _b_eval_epoch_clips(dev, scores):
    cache = _cache(torch.float32, dev)
    w = _weights(dev, True)
    want_loss = scores == 'softmax'

    def make():
        cache.status.zero_()
        order = torch.zeros(V, dtype=torch.int32, device=dev)
        ep = ce.ClipEvalEpoch(cache, EB, F, *w[:4], capacity=CAP, temporal=(w[5], w[6]), flags=cof.APA_FLAG_RELU_ATT,
                              scores=scores, want_loss=want_loss)
        outs = dict(logits=ep.logits, probs=ep.probs, pred=ep.pred, pooled=ep.pooled, att=ep.att, zsave=ep.zsave,
                    abar=ep.abar, tatt=ep.tatt, labels=ep.labels, targets=ep.targets)
        if want_loss:
            outs['loss'] = ep.loss
        for t in outs.values():
            t.zero_()               # rows past `count` are not written: the same in both instances

        def call():
            assert ep.run(order, V) == 3
        return gr.Case(call, {'order': order}, dict(outs, index=ep.index, status=cache.status), (), 'probs')
    return make, _video_rounds(V, 1)


ROWS = [('sample_clip_frames_keyed', ['apa_sample_clip_frames_keyed'], _b_sample_clips_keyed, ()),
        ('train_epoch_clips_softmax', ['apa_attn_head_train_epoch_cached_clips'], _b_train_epoch_clips,
         ('softmax-xentropy',)),
        ('train_epoch_clips_multi_label', ['apa_attn_head_train_epoch_cached_clips'], _b_train_epoch_clips,
         ('multi-label',)),
        ('eval_epoch_clips_softmax_loss', ['apa_attn_head_eval_epoch_cached_clips'], _b_eval_epoch_clips, ('softmax',)),
        ('eval_epoch_clips_sigmoid', ['apa_attn_head_eval_epoch_cached_clips'], _b_eval_epoch_clips, ('sigmoid',))]


def test_every_new_stream_taking_entry_point_has_a_row():
    bare = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                             'apa_clip_epoch.h')).read()
    import re
    bare = re.sub(r'/\*.*?\*/', '', bare, flags=re.S)
    taking = set(re.findall(r'\b(apa_[a-z0-9_]+)\s*\([^;]*?void\*\s*stream\s*\)\s*;', bare, flags=re.S))
    assert taking == set(ce.exported_symbols()) == {e for r in ROWS for e in r[1]}


@pytest.mark.parametrize('r', ROWS, ids=[r[0] for r in ROWS])
def test_replay_equals_eager(gpu, r):
    make, rounds = r[2](gpu, *r[3])
    gr.replay_equals_eager(r[0] + ' (' + ', '.join(r[1]) + ')', make, rounds, R=3)


def test_a_capture_freezes_seed_epoch_and_step(gpu):
    """(seed, epoch, step) travel by value: every replay draws with the key the call was captured with, whatever is
    called afterwards; the video ids are re-read from HBM.  The same for an epoch call: `run(seed=, epoch=)` after the
    capture changes nothing in the graph."""
    cache = _cache(torch.float32, gpu)
    videos = torch.tensor([4] * 8, dtype=torch.int32, device=gpu)           # 9 frames: every segment has a choice
    clips = cof.CachedClips(cache, 8, F)

    def sample(step, vid=videos):
        return ce.sample_clips_keyed(cache, vid, F, 'random-segment', seed=1, epoch=2, step=step, out=clips)
    eager = {}
    for step in (3, 4):
        eager[step] = sample(step).index.clone()
    assert not torch.equal(eager[3], eager[4])
    graph = _capture(lambda: sample(3))
    sample(4)                                                               # an eager call does take the new key
    torch.cuda.synchronize()
    assert torch.equal(clips.index, eager[4])
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(clips.index, eager[3])
    videos.copy_(torch.tensor([6, 4, 3, 4, 4, 6, 4, 3], dtype=torch.int32))  # in place: the replay follows
    graph.replay()
    torch.cuda.synchronize()
    got = clips.index.clone()
    other = cof.CachedClips(cache, 8, F)
    want = ce.sample_clips_keyed(cache, videos.clone(), F, 'random-segment', seed=1, epoch=2, step=3, out=other).index
    assert torch.equal(got, want) and not torch.equal(got, eager[3])
    # ---- the training epoch: the captured key stays
    lr = [LR0] * STEPS
    order = torch.tensor([4] * (STEPS * B), dtype=torch.int32, device=gpu)

    def epoch():
        run = _Run(gpu, False)
        ep = ce.ClipTrainEpoch(cache, B, F, *run.w[:4], tuple(run.views), run.segs, run.wd, run.grad, run.acc,
                               steps=STEPS, flags=cof.APA_FLAG_RELU_ATT, offset=OFFSET)
        return ep, run
    want = {}
    for key in ((1, 2), (1, 3)):
        ep, run = epoch()
        ep.run(order, lr, seed=key[0], epoch=key[1])
        torch.cuda.synchronize()
        want[key] = (ep.loss.clone(), ep.index.clone())
    assert not torch.equal(want[(1, 2)][0], want[(1, 3)][0])
    ep, run = epoch()
    init = [t.clone() for t in run.tensors().values()]
    graph = _capture(lambda: ep.run(order, lr, seed=1, epoch=2))
    for dst, src in zip(run.tensors().values(), init):
        dst.copy_(src)
    ep._ce.epoch = 3                                                        # the descriptor the call read when enqueued
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(ep.loss, want[(1, 2)][0]) and torch.equal(ep.index, want[(1, 2)][1])
    cache.status.zero_()
