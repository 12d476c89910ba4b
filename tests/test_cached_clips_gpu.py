"""Clips and the multi-label losses from a resident frame cache, on the GPU.

* the device sampler, bit for bit against the numpy restatement of the frame rule (tests/_clip_sampler_reference.py);
* every output of the cached clip / multi-label steps equals, by torch.equal, the plain entry point on
  `cache.gather(index)`: only the feature address goes through the index, the clip loss, the sigmoid reducers and the
  scores launch never see X -- every M == 1 family with gathered instances (asserted from the dispatch trace of
  tests/test_feature_cache_gpu.py, whose caches and widths these are), fp32 / bf16 / FP8;
* the identities: ml == clip == NULL is apa_attn_head_train_step_cached, an identity index is the plain clip step;
* one case per dtype and loss kind against float64: the pooling half by the error model of tests/_m1_probe.py (as
  test_gathered_training_step_against_float64 holds it), the loss half by the float64 restatements and bounds of
  tests/test_video_step_gpu.py / tests/test_multilabel_step_gpu.py on the step's own frame logits;
* deploy.FusedHeadStep / FusedHeadEval on a CachedClips against the same objects on the 5-D gathered tensor."""
import os

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _clip_sampler_reference as ref
from tests import _ml_probe as ml
from tests import _ref_fixture as rf
from tests import test_feature_cache_gpu as fcg
from tests import test_fp8_features_gpu as f8t
from tests import test_multilabel_step_gpu as mlt
from tests import test_video_step_gpu as vst

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
SEED, OFFSET, KEEP = fcg.SEED, fcg.OFFSET, fcg.KEEP
LOSSES = ('softmax-xentropy', 'multi-label', 'multi-label-2')


# ------------------------------------------------------------------------------------------ the sampler
V_FIRST = np.array([0, 1, 3, 6, 13, 53], dtype=np.int32)        # six videos back to back: n = 1, 2, 3, 7, 40, 400
V_COUNT = np.array([1, 2, 3, 7, 40, 400], dtype=np.int32)
VIDEOS = [4, 5, 5, 9, 2]                                        # a repeated id; 9 is out of range (clamped to 5)
T_FRAMES = int(V_FIRST[-1] + V_COUNT[-1])


def _copy_paths(src, dst, videos, V, K):
    """(head, vectors, tail) of each row of the multi-hot copy, by the kernel's rule on the buffers' addresses: 16-byte
    vectors over the part of a row where source and destination share their alignment mod 16, `head` scalars in front
    of it and `tail` behind; (K, 0, 0): the two rows do not share it, scalars alone"""
    out = []
    for b, raw in enumerate(videos):
        v = min(max(raw, 0), V - 1)
        sa, da = src.data_ptr() + 4 * K * v, dst.data_ptr() + 4 * K * b
        head = K if (sa ^ da) & 15 else min(((16 - (da & 15)) & 15) >> 2, K)
        nvec = (K - head) // 4
        out.append((head, nvec, K - head - 4 * nvec))
    return out


def _draws(n, seed):
    """uniform draws in [0,1) with the edges in: 0, the largest float below 1, 0.5"""
    u = torch.rand(n, generator=torch.Generator().manual_seed(seed))
    edge = [0.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), 0.5]
    for i in range(n):
        if i % 4 != 3:
            u[i] = edge[(i // 4 + i) % 3]
    return u.contiguous()


@pytest.mark.parametrize('K', [5, 157, 8])
@pytest.mark.parametrize('F', [1, 3, 25])
def test_sampler_is_the_numpy_restatement_bit_for_bit(gpu, F, K):
    """K = 5 / 157, no multiple of 4: clips 0 and 1 (videos 4 and 5, v - b = 4) share source and destination alignment
    -- row 0 is vectors and a scalar tail, row 1 starts 4 bytes past a 16-byte boundary and takes a 3-scalar head,
    vectors (K = 157) and a 2-scalar tail -- and the other rows (v - b = 3, 2, -2) do not and are copied by scalars
    alone; K = 8: vectors alone.  Which row takes which path is asserted from the buffers' addresses."""
    g = torch.Generator().manual_seed(100 + K)
    vlab = torch.randint(0, 1 << 40, (6,), generator=g)                            # int64 labels past 2^32
    vtar = (torch.rand(6, K, generator=g) < 0.3).float() * torch.arange(1, K + 1)    # a misplaced element shows
    cache = cof.FeatureCache(torch.zeros(T_FRAMES, 1, 1, 16, device=gpu))
    cache.set_videos(V_FIRST.tolist(), V_COUNT.tolist(), labels=vlab.to(gpu), targets=vtar.to(gpu))
    B = len(VIDEOS)
    for mode, code in (('uniform', ref.UNIFORM), ('random-segment', ref.RANDOM_SEGMENT)):
        u = _draws(B * F, seed=F) if code == ref.RANDOM_SEGMENT else None
        want_i, want_l, want_t, bad = ref.sample(V_FIRST, V_COUNT, VIDEOS, F, code, None if u is None else u.numpy(),
                                                 vlab.numpy(), vtar.numpy())
        assert bad == 1
        cache.status.zero_()
        clips = cache.sample_clips(VIDEOS, F, mode=mode, u=None if u is None else u.to(gpu))
        assert isinstance(clips, cof.CachedClips) and clips.frames == F and clips.shape == (B * F, 1, 1, 16)
        assert clips.index.dtype == torch.int32 and np.array_equal(clips.index.cpu().numpy(), want_i), (mode, F)
        assert clips.labels.dtype == torch.int64 and np.array_equal(clips.labels.cpu().numpy(), want_l)
        assert np.array_equal(clips.targets.cpu().numpy(), want_t)
        paths = _copy_paths(cache.video_targets, clips.targets, VIDEOS, 6, K)
        if K == 8:
            assert paths == [(0, 2, 0)] * B
        else:       # head / vectors / tail, a head without room for a vector, and scalars alone: all in one launch
            assert paths[0] == (0, K // 4, 1) and paths[1] == (3, (K - 3) // 4, 2), paths
            assert paths[2:] == [(K, 0, 0)] * 3, paths
        assert int(cache.status) == 1                           # the id out of range: clamped, and counted once
        assert 0 <= int(clips.index.min()) and int(clips.index.max()) < T_FRAMES
        # the same draws give the same bits; out= rewrites the same buffers
        ptrs = (clips.index.data_ptr(), clips.labels.data_ptr(), clips.targets.data_ptr())
        first = (clips.index.clone(), clips.labels.clone(), clips.targets.clone())
        for t in (clips.index, clips.labels, clips.targets):
            t.zero_()
        again = cache.sample_clips(VIDEOS, F, mode=mode, u=None if u is None else u.to(gpu), out=clips)
        assert again is clips and ptrs == (clips.index.data_ptr(), clips.labels.data_ptr(), clips.targets.data_ptr())
        assert all(torch.equal(a, b) for a, b in zip(first, (clips.index, clips.labels, clips.targets)))
        assert int(cache.status) == 2
    # draws of its own from a generator: inside the videos, the same for the same seed
    gen = torch.Generator(device=gpu)
    a = cache.sample_clips(VIDEOS, F, mode='random-segment', generator=gen.manual_seed(5)).index.clone()
    b = cache.sample_clips(VIDEOS, F, mode='random-segment', generator=gen.manual_seed(5)).index
    assert torch.equal(a, b)
    lo = torch.tensor([13, 53, 53, 53, 3], device=gpu).repeat_interleave(F)
    hi = torch.tensor([53, 453, 453, 453, 6], device=gpu).repeat_interleave(F)
    assert bool(((a >= lo) & (a < hi)).all())
    cache.status.zero_()
    # without labels / targets nothing is handed out; an epoch's views feed the sampler uncopied
    bare = cof.FeatureCache(torch.zeros(T_FRAMES, 1, 1, 16, device=gpu))
    bare.set_videos(V_FIRST, V_COUNT)
    batches = list(bare.video_epoch(3, seed=2))
    assert len(batches) == 2 and all(b.is_cuda and b.dtype == torch.int32 for b in batches)
    c = bare.sample_clips(batches[1], F)
    assert c.labels is None and c.targets is None and c.videos.data_ptr() == batches[1].data_ptr()
    want_i = ref.sample(V_FIRST, V_COUNT, batches[1].tolist(), F, ref.UNIFORM)[0]
    assert np.array_equal(c.index.cpu().numpy(), want_i) and int(bare.status) == 0


# ------------------------------------------------------------------------------------------ gathered == gathered copy
B_ = 3
VID_FIRST, VID_COUNT, VID_BATCH = [0, 1, 3], [1, 2, 4], [2, 0, 1]       # three videos in the T = 7 frame cache


def _clips(cache, F, mode='random-segment'):
    """B_ clips of F frames from fcg's 7-image cache read as three videos of 1, 2 and 4 frames"""
    if cache.video_first is None:
        cache.set_videos(VID_FIRST, VID_COUNT)
    u = _draws(B_ * F, seed=10 + F).to(cache.device)
    clips = cache.sample_clips(VID_BATCH, F, mode=mode, u=u)
    want = ref.sample(np.array(VID_FIRST), np.array(VID_COUNT), VID_BATCH, F,
                      ref.RANDOM_SEGMENT if mode == 'random-segment' else ref.UNIFORM, u.cpu().numpy())[0]
    assert np.array_equal(clips.index.cpu().numpy(), want)
    return clips


def _labels(loss, K, seed, dev, B=B_):
    g = torch.Generator().manual_seed(seed)
    if loss == 'softmax-xentropy':
        return torch.randint(0, K, (B,), generator=g).to(dev)
    t = (torch.rand(B, K, generator=g) < 0.2).float()
    t[0] = 0.0
    return t.to(dev)


def _temporal(K, F, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(K, generator=g) * (0.3 / K ** 0.5)).to(dev),
            (torch.full((1,), 1.0 / F) + 0.1 * torch.randn(1, generator=g)).to(dev))


def _train(X, p, labels, flags, F, temporal, loss, keep=KEEP, offset=OFFSET, run=True, wt=1.3, gs=0.5):
    grads = (None, None) + tuple(torch.empty_like(p[k]) for k in ('Wa', 'ba', 'Wt', 'bt'))
    tg = None if temporal is None else (torch.empty_like(temporal[0]), torch.empty_like(temporal[1]))
    st = cof.HeadTrainStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, grads, flags=flags, keep_prob=keep,
                           seed=SEED, offset=offset, loss_wt=wt, grad_scale=gs, frames=F, temporal=temporal,
                           temporal_grads=tg, action_loss=loss)
    st.grads, st.tgrads = grads, tg
    if run:
        st.run()
        assert st.frozen_input and st.dX_scratch is None
    return st


def _train_outputs(st):
    out = dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, loss=st.loss, G=st.G, dWa=st.grads[2],
               dba=st.grads[3], dWt=st.grads[4], dbt=st.grads[5])
    if getattr(st, 'pooled', None) is not None:
        out['pooled'] = st.pooled
    if getattr(st, 'tatt', None) is not None:
        out.update(tatt=st.tatt, dw=st.tgrads[0], db=st.tgrads[1])
    return out


def _eval(X, p, labels, flags, F, temporal, scores):
    st = cof.HeadEvalStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, flags=flags, frames=F, temporal=temporal,
                          scores=scores)
    st.run()
    out = dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, probs=st.probs, pred=st.pred)
    for k in ('pooled', 'tatt', 'loss'):
        if getattr(st, k, None) is not None:
            out[k] = getattr(st, k)
    return out, st


def _same(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    fcg._same(a, b, what)


@pytest.mark.parametrize('P', [6, 33])
@pytest.mark.parametrize('combo', fcg.COMBOS, ids=fcg._combo_id)
def test_cached_clip_steps_equal_the_steps_on_a_gathered_copy(gpu, combo, P):
    """B = 3 clips of F in {1, 2, 4} frames (N = 3, 6, 12), P = 6 (a short block) and 33 (several chunks), K in {5, 51},
    the three losses, mean and temporal pooling; training with dropout, evaluation with softmax and sigmoid scores"""
    family, dtype, C = combo
    cache = fcg._cache(dtype, P, C, gpu)
    before = (cache.features.buffer if cache.fp8 else cache.features).clone()
    entries = set()
    for F in (1, 2, 4):
        clips = _clips(cache, F)
        copy = cache.gather(clips.index)
        N = B_ * F
        act = 'relu' if F == 2 else 'id'
        for K in (5, 51):
            p = fcg._params(C, K, act, cache, gpu)
            for use_t in (False, True):
                temporal = _temporal(K, F, 3 + K + F, gpu) if use_t else None
                for loss in LOSSES:
                    what = '%s P=%d F=%d K=%d %s %s' % (fcg._combo_id(combo), P, F, K, loss,
                                                        'temporal' if use_t else 'mean')
                    labels = _labels(loss, K, 7 + K + F, gpu)
                    flags = fcg._flags(act, True)
                    a, b = _train(clips, p, labels, flags, F, temporal, loss), _train(copy, p, labels, flags, F,
                                                                                      temporal, loss)
                    _same(_train_outputs(a), _train_outputs(b), what + ' train')
                    entries.add(a._name)
                    want_keys = {'logits', 'att', 'zsave', 'abar', 'loss', 'G', 'dWa', 'dba', 'dWt', 'dbt'} | \
                        ({'pooled'} if F > 1 or use_t else set()) | ({'tatt', 'dw', 'db'} if use_t else set())
                    assert set(_train_outputs(a)) == want_keys, what
                    assert a.loss.numel() == 1 + B_ and tuple(a.G.shape) == (N, K)
                # evaluation: softmax scores with the clips' labels, and without; sigmoid scores
                lab = _labels('softmax-xentropy', K, 9 + K, gpu)
                flags = fcg._flags(act, False)
                for labels, scores in ((lab, 'softmax'), (None, 'softmax'), (None, 'sigmoid')):
                    what = '%s P=%d F=%d K=%d eval %s %s' % (fcg._combo_id(combo), P, F, K, scores,
                                                             'temporal' if use_t else 'mean')
                    ea, sa = _eval(cof.FeatureCache(cache.features).select(clips.index) if labels is None else clips, p,
                                   labels, flags, F, temporal, scores)
                    eb, _ = _eval(copy, p, labels, flags, F, temporal, scores)
                    _same(ea, eb, what)
                    entries.add(sa._name)
                    assert tuple(ea['probs'].shape) == (B_, K) and tuple(ea['logits'].shape) == (N, K)
        if F == 4:      # the family the width is meant to reach, from the library's own trace, at this batch shape
            p = fcg._params(C, 51, 'id', cache, gpu)
            G = ((torch.rand(N, 51, generator=torch.Generator().manual_seed(N)) * 1.25 - 0.25) / N).to(gpu)
            flags = fcg._flags('id', True)
            sep = fcg._separate(copy, p, G, flags)
            assert fcg._traced_families(clips, p, G, flags, sep) == (family, family)
    # every entry point took part: the flat softmax step stays the cached step, the rest is the new pair
    assert entries == {'apa_attn_head_train_step_cached', 'apa_attn_head_train_step_cached_clips',
                       'apa_attn_head_eval_step_cached', 'apa_attn_head_eval_step_cached_clips'}
    torch.cuda.synchronize()
    assert torch.equal(cache.features.buffer if cache.fp8 else cache.features, before)      # a cache is read-only
    assert int(cache.status) == 0


# ------------------------------------------------------------------------------------------ identities, rebinding
DTYPES = [(torch.float32, 1024), (torch.bfloat16, 512), (F8, 1040)]


@pytest.mark.parametrize('dtype,C', DTYPES, ids=['f32', 'bf16', 'fp8'])
def test_without_ml_and_clip_the_new_entry_is_the_cached_step(gpu, dtype, C):
    cache = fcg._cache(dtype, 33, C, gpu)
    p = fcg._params(C, 20, 'relu', cache, gpu)
    flags = fcg._flags('relu', True)
    for labels in (None, cache.labels[torch.tensor(fcg.INDEX, device=gpu)].contiguous()):       # labels_cached or not
        st = fcg._train_step(cache.select(fcg.INDEX), p, labels, flags)
        assert st._name == 'apa_attn_head_train_step_cached'
        want = {k: v.clone() for k, v in fcg._step_outputs(st).items()}
        for v in fcg._step_outputs(st).values():
            v.fill_(float('nan'))
        rc = st.lib.apa_attn_head_train_step_cached_clips(st._pre[0], None, None, None, *st._args,
                                                          torch.cuda.current_stream().cuda_stream)
        assert rc == 0, st.lib.apa_last_error()
        fcg._same(fcg._step_outputs(st), want, 'ml == clip == NULL')


@pytest.mark.parametrize('dtype,C', DTYPES, ids=['f32', 'bf16', 'fp8'])
def test_identity_index_equals_the_plain_clip_step(gpu, dtype, C):
    cache = fcg._cache(dtype, 33, C, gpu)
    F, K = 2, 51
    batch = cache.select(torch.arange(6))
    f = cache.features
    plain = cof.Fp8Features.from_parts(f.codes[:6], f.scale[:6]).flat() if cache.fp8 else f[:6]
    p = fcg._params(C, K, 'id', cache, gpu)
    temporal = _temporal(K, F, 1, gpu)
    for loss in LOSSES:
        labels = _labels(loss, K, 21, gpu)
        flags = fcg._flags('id', True)
        _same(_train_outputs(_train(batch, p, labels, flags, F, temporal, loss)),
              _train_outputs(_train(plain, p, labels, flags, F, temporal, loss)), 'identity ' + loss)
    lab = _labels('softmax-xentropy', K, 22, gpu)
    _same(_eval(batch, p, lab, 0, F, temporal, 'softmax')[0], _eval(plain, p, lab, 0, F, temporal, 'softmax')[0],
          'identity eval')


@pytest.mark.parametrize('loss', LOSSES)
def test_out_resampling_moves_a_bound_step_and_the_counter_advances_once_per_step(gpu, loss):
    """one bound step follows `sample_clips(..., out=clips)` without a rebind; rebind(index=, labels=) moves it to
    another CachedClips; the device dropout counter advances once per step, as in the plain step on the copy"""
    dtype, C, P, F, K = torch.bfloat16, 2048, 33, 2, 51
    cache = fcg._cache(dtype, P, C, gpu)
    clips = _clips(cache, F)
    p = fcg._params(C, K, 'relu', cache, gpu)
    temporal = _temporal(K, F, 2, gpu)
    flags = fcg._flags('relu', True)
    labels = _labels(loss, K, 31, gpu)
    ctr = torch.tensor([OFFSET], dtype=torch.int64, device=gpu)
    st = _train(clips, p, labels, flags, F, temporal, loss, offset=ctr, run=False)
    ev, evs = _eval(clips, p, None, 0, F, temporal, 'sigmoid')
    seen = []
    for i, vids in enumerate(([2, 0, 1], [1, 1, 2], [0, 2, 2])):
        u = _draws(B_ * F, seed=40 + i).to(gpu)
        assert cache.sample_clips(vids, F, mode='random-segment', u=u, out=clips) is clips
        st.run()
        assert int(ctr) == OFFSET + i + 1
        copy = cache.gather(clips.index)
        fresh = _train(copy, p, labels, flags, F, temporal, loss, offset=OFFSET + i)
        _same(_train_outputs(st), _train_outputs(fresh), 'resampled, step %d' % i)
        evs.run()
        _same(ev, _eval(copy, p, None, 0, F, temporal, 'sigmoid')[0], 'resampled eval, step %d' % i)
        seen.append(st.loss.clone())
    assert not torch.equal(seen[0], seen[1])
    # rebind to the buffers of another CachedClips
    other = cache.sample_clips([1, 2, 2], F, mode='uniform')
    labels2 = _labels(loss, K, 32, gpu)
    st.rebind(index=other.index, labels=labels2)
    st.run()
    assert int(ctr) == OFFSET + 4
    fresh = _train(cache.gather(other.index), p, labels2, flags, F, temporal, loss, offset=OFFSET + 3)
    _same(_train_outputs(st), _train_outputs(fresh), 'rebound')
    with pytest.raises(cof.ApaError):
        st.rebind(index=other.index[:4])
    # the evaluation step: index and per-clip labels
    lab = _labels('softmax-xentropy', K, 33, gpu)
    eo, es = _eval(clips, p, lab, 0, F, temporal, 'softmax')
    lab2 = _labels('softmax-xentropy', K, 34, gpu)
    es.rebind(index=other.index, labels=lab2)
    es.run()
    _same(eo, _eval(cache.gather(other.index), p, lab2, 0, F, temporal, 'softmax')[0], 'rebound eval')
    with pytest.raises(cof.ApaError, match='without labels'):
        evs.rebind(labels=lab2)
    # what the CPU cannot reach: the shapes of per-clip labels
    g = (None, None) + tuple(torch.empty_like(p[k]) for k in ('Wa', 'ba', 'Wt', 'bt'))
    args = (clips, clips, p['Wa'], p['ba'], p['Wt'], p['bt'])
    with pytest.raises(cof.ApaError, match='multi-hot labels'):
        cof.HeadTrainStep(*args, torch.zeros(B_ * F, K, device=gpu), g, frames=F, action_loss='multi-label')
    with pytest.raises(cof.ApaError, match='one label per clip'):
        cof.HeadTrainStep(*args, torch.zeros(B_ * F, dtype=torch.int64, device=gpu), g, frames=F)
    with pytest.raises(cof.ApaError, match='whole number of clips'):
        cof.HeadTrainStep(*args, lab, g, frames=4)
    assert int(cache.status) == 0


# ------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize('loss', LOSSES)
@pytest.mark.parametrize('dtype,C', [(torch.float32, 1024), (torch.bfloat16, 2048), (F8, 2048)], ids=['f32', 'bf16', 'fp8'])
def test_cached_clip_training_step_against_float64(gpu, dtype, C, loss):
    """The pooling half: the error model of tests/_m1_probe.py on the gathered (FP8: dequantised) frames, G taken from
    the step -- what test_gathered_training_step_against_float64 asserts, with its keep probability.  The loss half, on
    the step's own frame logits: the float64 restatement of tests/test_video_step_gpu.py with its 2e-5 of max|reference|
    (softmax cross-entropy), of tests/test_multilabel_step_gpu.py with its element bounds (the sigmoid losses)."""
    P, K, F, wt, gs, pw = 49, 51, 2, 1.3, 0.5, 10.0
    N = B_ * F
    cache = fcg._cache(dtype, P, C, gpu)
    clips = _clips(cache, F)
    p = fcg._params(C, K, 'relu', cache, gpu)
    temporal = _temporal(K, F, 4, gpu)
    labels = _labels(loss, K, 41, gpu)
    st = _train(clips, p, labels, fcg._flags('relu', True), F, temporal, loss, keep=fcg.OR_KEEP, wt=wt, gs=gs)
    got = _train_outputs(st)
    # -- pooling
    vals = cache.features.dequantize() if cache.fp8 else cache.features
    X64 = vals[clips.index.long()].double().reshape(N, P, C)
    c = dict(name='cached clips', N=N, P=P, C=C, K=K, J=0, Ca=None, act='relu', train=True, keep=fcg.OR_KEEP,
             rank1=False, relu_in=False, dt=cof._feat_dtype(clips), entry='step')
    inp = dict(X=X64, Xatt=X64, Wa=p['Wa'].reshape(C), ba=p['ba'], Wt=p['Wt'], bt=p['bt'], G=got['G'], labels=labels,
               Xext=None)
    mask = cof.dropout_mask((N * P * C,), fcg.OR_KEEP, SEED, OFFSET)
    f8t._check_against_float64(c, inp, got, mask, cancels=True)
    # -- the loss behind the frame logits
    x = got['logits'].cpu()
    w, b = temporal[0].cpu(), temporal[1].cpu()
    keys = ('pooled', 'tatt', 'loss', 'G', 'dw', 'db')
    if loss == 'softmax-xentropy':
        want = vst._clip_reference(x, labels.cpu(), w, b, F, wt, gs)
        for k in keys:
            e = vst._rel(got[k].cpu().numpy(), want[k].numpy())
            print('%s %s: %.3e' % (loss, k, e))
            assert e <= 2e-5, '%s: %.3e' % (k, e)
    else:
        want = mlt._clip_reference(loss, x, labels.cpu(), w, b, B_, F, K, pw, wt, gs)
        for k in keys:
            r = ml.check(got[k], want[k], '%s %s' % (loss, k))
            print('%s %s: %.3f of the bound' % (loss, k, r))


# ------------------------------------------------------------------------------------------ deploy
def _frame_cache(fx, dtype, gpu, multi_label):
    """the fixture's [B,F,H,W,C] clips as a frame cache: the videos in REVERSED order behind one spare frame, F frames
    each, so that uniform sampling of videos [B-1, ..., 0] is the fixture's batch; labels / targets per video"""
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu)
    B, F = images.shape[:2]
    order = list(range(B - 1, -1, -1))
    frames = images[order].reshape(B * F, *images.shape[2:])
    cache = cof.FeatureCache.empty((1 + B * F,) + tuple(images.shape[2:]), dtype, gpu)
    assert cache.write(0, frames[:1] * 3.0).tolist() == [0]
    assert cache.write(1, frames).tolist() == [0] * (B * F)
    lab = torch.from_numpy(fx.arrays['in/labels_action_multihot' if multi_label else 'in/labels_action']).to(gpu)
    if multi_label:
        cache.set_videos([1 + F * i for i in range(B)], [F] * B, targets=lab.reshape(B, -1).float()[order].contiguous())
    else:
        cache.set_videos([1 + F * i for i in range(B)], [F] * B, labels=lab.reshape(B).long()[order].contiguous())
    return cache, order, B, F, lab


@pytest.mark.parametrize('name,multi_label', [('vstep_temporal_att_train', False), ('mlstep_clip_temporal_ml', True)],
                         ids=['softmax', 'multi-label'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, F8], ids=['f32', 'bf16', 'fp8'])
def test_deploy_fused_step_and_eval_on_cached_clips(gpu, dtype, name, multi_label):
    """FusedHeadStep / FusedHeadEval on a CachedClips (frames and labels from the batch) equal, bit for bit, the same
    objects fed the 5-D gathered tensor; an FP8 cache has no 5-D form: its step equals HeadTrainStep / HeadEvalStep on
    `cache.gather(index)` with the head's parameters."""
    from attentionalpoolingaction_amd import config as apa_config, deploy
    try:
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_%s.npz' % name))
        network_fn, cfg, _ = vst._load(fx, gpu)
        head = network_fn.head
        step0 = head._step
        cache, order, B, F, lab = _frame_cache(fx, dtype, gpu, multi_label)
        clips = cache.sample_clips(order, F)                    # n = F frames: uniform sampling takes them all
        assert clips.index.tolist() == [1 + F * v + i for v in order for i in range(F)]
        fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
        total, ep = fused(clips, None)                          # frames and labels from the batch
        total.backward()
        st = fused._step_obj
        assert st._name == 'apa_attn_head_train_step_cached_clips' and st._dX_buf is None and st.frozen_input
        assert set(ep) == {'Logits', 'logits_beforePool', 'PosePrelogitsBasedAttention', 'Losses', 'TemporalAttention'}
        K = ep['Logits'].shape[1]
        assert tuple(ep['Logits'].shape) == (B, K) and tuple(ep['logits_beforePool'].shape) == (B * F, K)
        assert tuple(ep['TemporalAttention'].shape) == (B, F, 1, 1)
        got = dict(total=total.detach().clone(), pooled=ep['Logits'].clone(), logits=ep['logits_beforePool'].clone(),
                   tatt=ep['TemporalAttention'].reshape(-1).clone(), att=st.att.clone(), loss=st.loss.clone(),
                   bucket=fused.bucket.flat.clone())
        assert float(got['bucket'].abs().max()) > 0
        labels = clips.targets if multi_label else clips.labels
        copy = cache.gather(clips.index)
        if dtype != F8:
            head._step = step0
            other = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
            total5, ep5 = other(copy.reshape(B, F, *copy.shape[1:]), labels)
            total5.backward()
            want = dict(total=total5.detach(), pooled=ep5['Logits'], logits=ep5['logits_beforePool'],
                        tatt=ep5['TemporalAttention'].reshape(-1), att=other._step_obj.att, loss=other._step_obj.loss,
                        bucket=other.bucket.flat)
            _same(got, want, 'deploy, 5-D gathered tensor')
        pm = {n: t.data for n, t in fused.params.items()}
        p = dict(Wa=pm['att_weights'], ba=pm['att_biases'], Wt=pm['td_weights'], bt=pm['td_biases'])
        tw = (pm['temporal_weights'], pm['temporal_biases'])
        flags = cof.attn_flags(head.softmax_att, head.relu_att, True, False)
        wt = 1.0 if multi_label else float(cfg.TRAIN.LOSS_FN_ACTION_WT)
        # the same step bound by hand on the gathered frames, with the head's own seed and step counter
        grads = (None, None) + tuple(torch.empty_like(p[k]) for k in ('Wa', 'ba', 'Wt', 'bt'))
        tg = (torch.empty_like(tw[0]), torch.empty_like(tw[1]))
        Xc = copy.flat() if cache.fp8 else copy.reshape(B * F, -1, copy.shape[-1])
        plain = cof.HeadTrainStep(Xc, Xc, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, grads, flags=flags,
                                  keep_prob=head.keep_prob, seed=head.seed, offset=step0, loss_wt=wt,
                                  grad_scale=fused.loss_scale, frames=F, temporal=tw, temporal_grads=tg,
                                  action_loss=str(cfg.TRAIN.LOSS_FN_ACTION))
        plain.run()
        _same(dict(pooled=got['pooled'], logits=got['logits'], tatt=got['tatt'], att=got['att'], loss=got['loss']),
              dict(pooled=plain.pooled, logits=plain.logits, tatt=plain.tatt, att=plain.att, loss=plain.loss),
              'deploy, the step on gather()')
        # out= resampling: the bound step follows without a new binding; explicit labels of the same kind too
        head._step = step0
        assert cache.sample_clips(order[::-1], F, out=clips) is clips
        fused(clips, None)
        assert fused._step_obj is st and len(fused._steps) == 1 and not torch.equal(st.logits, got['logits'])
        head._step = step0
        cache.sample_clips(order, F, out=clips)
        _, ep2 = fused(clips, labels.clone())
        assert fused._step_obj is st and torch.equal(ep2['Logits'], got['pooled'])
        assert head._step == step0 + 1
        if multi_label:         # a plain CachedBatch under a sigmoid loss: labels_action [N,K]
            head._step = step0
            rows = labels.repeat_interleave(F, dim=0).contiguous()
            _, epf = fused(cache.select(clips.index), rows)
            fl = fused._step_obj
            assert fl is not st and fl._name == 'apa_attn_head_train_step_cached_clips'
            assert torch.equal(epf['Logits'], got['logits']) and 'logits_beforePool' not in epf
        # ---- evaluation
        head.is_training = False                                # evaluation draws no mask: the same weights, no dropout
        try:
            ev = deploy.FusedHeadEval(network_fn, cfg)
            scores, pred, epe = ev(clips)
            assert ev.step._name == 'apa_attn_head_eval_step_cached_clips'
            assert tuple(scores.shape) == (B, K) and tuple(epe['logits_beforePool'].shape) == (B * F, K)
            assert torch.equal(epe['labels'], labels.squeeze() if labels.dim() > 1 else labels)
            gote = dict(scores=scores.clone(), pred=pred.clone(), pooled=epe['Logits'].clone(),
                        logits=epe['logits_beforePool'].clone(), tatt=epe['TemporalAttention'].reshape(-1).clone())
            if dtype != F8:
                s5, p5, e5 = deploy.FusedHeadEval(network_fn, cfg)(copy.reshape(B, F, *copy.shape[1:]))
                _same(gote, dict(scores=s5, pred=p5, pooled=e5['Logits'], logits=e5['logits_beforePool'],
                                 tatt=e5['TemporalAttention'].reshape(-1)), 'deploy eval, 5-D gathered tensor')
            pe, _ = _eval(Xc, p, None, cof.attn_flags(head.softmax_att, head.relu_att, False, False), F,
                          (tw[0].reshape(-1).contiguous(), tw[1]), 'sigmoid' if multi_label else 'softmax')
            _same(gote, dict(scores=pe['probs'], pred=pe['pred'], pooled=pe['pooled'], logits=pe['logits'],
                             tatt=pe['tatt']), 'deploy eval, the step on gather()')
            step_e = ev.step
            cache.sample_clips(order[::-1], F, out=clips)
            ev(clips)
            assert ev.step is step_e and len(ev._steps) == 1
        finally:
            head.is_training = True
        assert int(cache.status) == 0
    finally:
        apa_config.reset_cfg()
