"""Per-class attention maps (M == K) from the resident feature cache, on the GPU.

The oracle is the library itself on a gathered copy, whose per-class kernels tests/test_pc_paths_gpu.py holds to
float64: of the fused per-class route only the two kernels that read X (the Z | T product and the dW product) know about
the index, and only in the address of a feature row, so a call on `cache.select(index)` must equal the same call on
`cache.gather(index)` BIT FOR BIT in every output, and record the same dispatch trace (PcTrace, through the test-only
probe library).  The cache has T = 7 images and the index repeats, is non-monotone and leaves images unused.

Shapes: the smallest that reach each way the two kernels can go wrong --
  3 x 32 x 256,  K = 2    blocks aligned to images; K < 4: the loss is a launch of its own; separate calls, evaluation
  8 x 33 x 768,  K = 3    32-row blocks straddle two images at every offset; chunk swizzle off (6 k tiles); R = 264 is no
                          multiple of 32 (clamped tail rows); ReLU attention
  4 x 25 x 2048, K = 51   P < 32: several images per block, no fold, FK = 64 > P in the dW walk
  3 x 49 x 2048, K = 51   spatial softmax
  1 x 32 x 8192, K = 63   the cache's last image; one k tile in dW
  2 x 225 x 2048, K = 64  P odd; ReLU
 32 x 196 x 2048, K = 51  the shipped shape, once: the one-call step with weight images over two steps (T = 40)"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _pc_probe as pp
from tests import _ref_fixture as rf

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
T = 7
FULL_INDEX = [6, 0, 6, 3, 1, 5, 5, 2]
SEED, OFFSET, KEEP = 4321, 5, 0.5
SIDES = {32: (4, 8), 33: (3, 11), 25: (5, 5), 49: (7, 7), 225: (15, 15), 196: (14, 14)}
ACT_FLAGS = {'id': 0, 'relu': cof.APA_FLAG_RELU_ATT, 'softmax': cof.APA_FLAG_SOFTMAX_ATT}


# ------------------------------------------------------------------------------------------ inputs
_CACHES = {}


def _cache(P, C, dev, images=T):
    """a bf16 cache of relu(randn) maps with a per-image magnitude (a wrong image cannot pass) and labels below 3, built
    once per shape and never written afterwards"""
    key = (P, C, images)
    if key not in _CACHES:
        H, W = SIDES[P]
        g = torch.Generator().manual_seed(91 + P + C + images)
        rows = 0.25 + 1.5 * torch.rand((images, H, W, 1), generator=g)
        mag = torch.tensor([1.0, 7.0, 0.125, 2.0, 0.5, 5.0, 3.0]).repeat(images // 7 + 1)[:images].view(images, 1, 1, 1)
        img = (torch.relu(torch.randn(images, H, W, C, generator=g)) * rows * mag).to(BF).to(dev)
        labels = torch.randint(0, 3, (images,), generator=g).to(dev)
        _CACHES[key] = cof.FeatureCache(img.contiguous(), labels)
    return _CACHES[key]


def _params(C, K, act, cache, dev):
    g = torch.Generator().manual_seed(7 + C + K)
    u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
    Wa = u(C, K) * (4.0 / C)
    if act == 'relu':       # gate both ways around the unit-magnitude image's mean pixel
        x0 = cache.features[0].float().cpu().reshape(-1, C)
        ba = -(x0.mean(dim=0) @ Wa)
    else:
        ba = u(K) * 0.1
    return dict(Wa=Wa.to(dev), ba=ba.contiguous().to(dev), Wt=(u(C, K) / C ** 0.5).to(dev), bt=(u(K) * 0.1).to(dev))


def _flags(act, train):
    return ACT_FLAGS[act] | (cof.APA_FLAG_TRAIN if train else 0)


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in b:
        if b[k] is None:
            assert a[k] is None, '%s: %s' % (what, k)
            continue
        assert a[k] is not None and torch.equal(a[k].reshape(b[k].shape), b[k]), '%s: %s differs' % (what, k)
        assert bool(torch.isfinite(b[k].float()).all()), '%s: %s is not finite' % (what, k)


def _labels(cache, index, K, dev):
    return (cache.labels[torch.as_tensor(index, device=dev).long()] % K).contiguous()


def _grad(N, K, dev):
    g = torch.Generator().manual_seed(N + K)
    return ((torch.rand(N, K, generator=g) * 1.25 - 0.25) / N).to(dev)


# ------------------------------------------------------------------------------------------ the calls
def _separate(X, p, G, flags, offset=OFFSET):
    kw = dict(flags=flags, keep_prob=KEEP, seed=SEED, offset=offset)
    logits, att, zsave, abar, _, ws = cof.attn_pool_fwd(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], **kw)
    assert abar is None
    dX, dXatt, dWa, dba, dWt, dbt = cof.attn_pool_bwd(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], att, zsave, abar, G,
                                                      workspace=ws, want_dx=False, **kw)
    assert dX is None and dXatt is None
    return dict(logits=logits, att=att, zsave=zsave, dWa=dWa, dba=dba, dWt=dWt, dbt=dbt)


def _train_step(X, p, labels, flags, offset=OFFSET, run=True, **kw):
    grads = (None, None) + tuple(torch.empty_like(p[k]) for k in ('Wa', 'ba', 'Wt', 'bt'))
    st = cof.HeadTrainStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, grads, flags=flags, keep_prob=KEEP,
                           seed=SEED, offset=offset, **kw)
    st.grads = grads
    if run:
        st.run()
        assert st.frozen_input and st.dX_scratch is None
    return st


def _step_outputs(st):
    out = dict(logits=st.logits, att=st.att, zsave=st.zsave, loss=st.loss, G=st.G, dWa=st.grads[2], dba=st.grads[3],
               dWt=st.grads[4], dbt=st.grads[5])
    for k in ('pooled', 'tatt'):
        if getattr(st, k, None) is not None:
            out[k] = getattr(st, k)
    return out


def _eval_step(X, p, labels, flags, **kw):
    st = cof.HeadEvalStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, flags=flags, **kw)
    st.run()
    out = dict(logits=st.logits, att=st.att, zsave=st.zsave, probs=st.probs, pred=st.pred)
    for k in ('loss', 'pooled', 'tatt'):
        if getattr(st, k, None) is not None:
            out[k] = getattr(st, k)
    return out


# ------------------------------------------------------------------------------------------ the dispatch trace
@contextlib.contextmanager
def _traced():
    """every library call inside the block goes through the probe library's copy of the product and records into the
    yielded PcTrace (csrc/apa_pc_probe.hip: apa_probe_pc_trace_begin / _end)"""
    probe = pp.load_pc_probe()
    probe.apa_probe_pc_trace_begin.argtypes, probe.apa_probe_pc_trace_begin.restype = [ctypes.c_void_p], None
    probe.apa_probe_pc_trace_end.argtypes, probe.apa_probe_pc_trace_end.restype = [], None
    tr = pp.PcTrace()
    product, cof._lib = cof._lib, probe
    probe.apa_probe_pc_trace_begin(ctypes.addressof(tr))
    try:
        yield tr
    finally:
        probe.apa_probe_pc_trace_end()
        cof._lib = product


def _both(call, cached, plain, what, fused_dw=True):
    """call(X) on the cache and on the gathered copy: equal outputs from the product library, and -- run once more through
    the probe library -- equal outputs and equal traces there; returns the outputs"""
    want = call(plain)
    got = call(cached)
    _same(got, want, what)
    with _traced() as tp:
        want_t = call(plain)
        dp = tp.as_dict()
    with _traced() as tc:
        got_t = call(cached)
        dc = tc.as_dict()
    _same(got_t, want, what + ' (traced)')
    _same(want_t, want, what + ' (traced, plain)')
    assert dc == dp, '%s: traces differ: %s' % (what, {k: (dc[k], dp[k]) for k in dc if dc[k] != dp[k]})
    assert dc['path_fwd'] == 'fused' and dc['zt'] == 1, what
    if fused_dw:
        assert dc['path_bwd'] == 'fused' and dc['dw'] == 'fused' and dc['dx'] == 'none', what
    return got, dc


# ------------------------------------------------------------------------------------------ 1: the shapes
#        N    P     C   K  act        index
CASES = [(3, 32, 256, 2, 'id', None),
         (8, 33, 768, 3, 'relu', None),
         (4, 25, 2048, 51, 'id', None),
         (3, 49, 2048, 51, 'softmax', None),
         (1, 32, 8192, 63, 'id', [T - 1]),
         (2, 225, 2048, 64, 'relu', None)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%dx%d_k%d_%s' % c[:5])
def test_cached_calls_equal_the_calls_on_a_gathered_copy(gpu, case):
    N, P, C, K, act, index = case
    index = FULL_INDEX[:N] if index is None else index
    cache = _cache(P, C, gpu)
    before = cache.features.clone()
    batch, copy = cache.select(index), cache.gather(index)
    p = _params(C, K, act, cache, gpu)
    labels = _labels(cache, index, K, gpu)
    G = _grad(N, K, gpu)
    what = '%dx%dx%d K=%d %s' % (N, P, C, K, act)
    fused, dx_route = pp.support(N, P, C, C, K, cof.APA_DTYPE_BF16, {'id': 0, 'relu': 1, 'softmax': 2}[act])
    assert fused, what
    for train in (True, False):
        fl = _flags(act, train)
        _both(lambda X: _separate(X, p, G, fl), batch, copy, what + ' fwd/bwd train=%d' % train)
    out, tr = _both(lambda X: _step_outputs(_train_step(X, p, labels, _flags(act, True))), batch, copy, what + ' step')
    # where the loss is taken is what the shape says: its own launch (K < 4), the dX kernel (folded), pc_fwd_act
    assert tr['xent'] == ('own' if K < 4 else 'dx' if dx_route else 'fwd_act'), (what, tr['xent'])
    assert tr['zt_fold'] == (1 if act != 'softmax' and P >= 32 else 0), what
    assert float(out['loss'][0]) > 0
    _both(lambda X: _eval_step(X, p, labels, _flags(act, False)), batch, copy, what + ' eval', fused_dw=False)
    _both(lambda X: _eval_step(X, p, None, _flags(act, False)), cof.FeatureCache(cache.features).select(index), copy,
          what + ' eval, no labels', fused_dw=False)
    torch.cuda.synchronize()
    assert torch.equal(cache.features, before) and int(cache.status) == 0


def test_the_shipped_shape_with_weight_images_over_two_steps(gpu):
    """32 x 196 x 2048, K = 51, a 40-image cache: the one-call step with caller-kept weight images.  Step 1 finds no
    tagged keep bits and hashes its own; its last launch leaves step 2's, tagged, which step 2 believes -- on a fresh
    index, the bits being keyed by batch position."""
    N, P, C, K, images = 32, 196, 2048, 51, 40
    cache = _cache(P, C, gpu, images=images)
    p = _params(C, K, 'id', cache, gpu)
    g = torch.Generator().manual_seed(3)
    idx = [torch.randint(0, images, (N,), generator=g).tolist() for _ in range(2)]
    idx[0][:4] = [39, 0, 39, 17]
    fl = _flags('id', True)
    lab = [_labels(cache, i, K, gpu) for i in idx]
    a = _train_step(cache.select(idx[0]), p, lab[0], fl, run=False, weight_images=True)
    b = _train_step(cache.gather(idx[0]), p, lab[0], fl, run=False, weight_images=True)
    assert a.weight_image_maps and b.weight_image_maps
    tag_at = pp.plan(N, P, C, C, K, cof.APA_DTYPE_BF16)['bits_tag']

    def tag(st):
        return st.workspace[tag_at:tag_at + 40].view(torch.int64).tolist()
    n8 = N * P * C // 8
    ws_a = a.workspace.data_ptr()
    for s in range(2):
        if s:
            a.rebind(index=torch.tensor(idx[1], dtype=torch.int32, device=gpu), labels=lab[1], offset=OFFSET + 1)
            b.rebind(X=cache.gather(idx[1]), labels=lab[1], offset=OFFSET + 1)
        with _traced() as ta:
            a._fn = getattr(cof._lib, a._fn.__name__)
            a.run()
            da = ta.as_dict()
        with _traced() as tb:
            b._fn = getattr(cof._lib, b._fn.__name__)
            b.run()
            db = tb.as_dict()
        assert da == db, {k: (da[k], db[k]) for k in da if da[k] != db[k]}
        assert da['check_tag'] == 1 and da['prep_fwd'] == 'none' and da['next_bits'] == 1 and da['xent'] == 'dx'
        _same(_step_outputs(a), _step_outputs(b), 'weight images, step %d' % s)
        # the map is tagged with the NEXT step's mask; tag[4]: the offset this step's forward kernel ran with
        ta_, tb_ = tag(a), tag(b)
        assert ta_ == tb_ and ta_[0] == SEED and ta_[1] == OFFSET + s + 1 and ta_[3] == n8 and ta_[4] == OFFSET + s
    assert a.workspace.data_ptr() == ws_a and int(cache.status) == 0


# ------------------------------------------------------------------------------------------ 2: further cases
def test_device_side_dropout_counter(gpu):
    N, P, C, K = 3, 49, 2048, 51
    cache = _cache(P, C, gpu)
    index = FULL_INDEX[:N]
    p = _params(C, K, 'relu', cache, gpu)
    fl = _flags('relu', True)
    labels = _labels(cache, index, K, gpu)
    ctr_a = torch.tensor([OFFSET], dtype=torch.int64, device=gpu)
    ctr_b = ctr_a.clone()
    a = _train_step(cache.select(index), p, labels, fl, offset=ctr_a, run=False)
    b = _train_step(cache.gather(index), p, labels, fl, offset=ctr_b, run=False)
    first = None
    for i in range(2):
        a.run()
        b.run()
        assert int(ctr_a) == int(ctr_b) == OFFSET + i + 1
        _same(_step_outputs(a), _step_outputs(b), 'device counter, step %d' % i)
        if i == 0:
            first = a.loss.clone()
            _same(_step_outputs(a), _step_outputs(_train_step(cache.select(index), p, labels, fl)), 'offset by value')
    assert not torch.equal(first, a.loss)                   # a fresh mask per step


@pytest.mark.parametrize('P,K,act,where', [(49, 51, 'id', 'dx'), (49, 3, 'id', 'own'), (25, 51, 'id', 'fwd_act'),
                                          (49, 51, 'softmax', 'fwd_act')],
                         ids=['dx_kernel', 'own_launch', 'fwd_act_p25', 'fwd_act_softmax'])
def test_labels_through_the_index(gpu, P, K, act, where):
    """labels_cached = 1: the forward product leaves labels[index[n]] in the workspace, wherever the loss is taken"""
    N, C = 5, 2048
    cache = _cache(P, C, gpu)
    index = FULL_INDEX[:N]
    p = _params(C, K, act, cache, gpu)
    labels = _labels(cache, index, K, gpu)              # (the cache's labels lie below 3)
    want = _step_outputs(_train_step(cache.gather(index), p, labels, _flags(act, True)))
    with _traced() as t:
        got = _step_outputs(_train_step(cache.select(index), p, None, _flags(act, True)))
        assert t.as_dict()['xent'] == where
    _same(got, want, 'cached labels (traced)')
    _same(_step_outputs(_train_step(cache.select(index), p, None, _flags(act, True))), want, 'cached labels')
    _same(_eval_step(cache.select(index), p, None, _flags(act, False)),
          _eval_step(cache.gather(index), p, labels, _flags(act, False)), 'cached labels, eval')


def test_identity_index_equals_the_plain_call(gpu):
    P, C, K = 33, 768, 3
    cache = _cache(P, C, gpu)
    batch, plain = cache.select(torch.arange(T)), cache.features
    p = _params(C, K, 'relu', cache, gpu)
    fl = _flags('relu', True)
    G = _grad(T, K, gpu)
    _same(_separate(batch, p, G, fl), _separate(plain, p, G, fl), 'fwd/bwd')
    _same(_step_outputs(_train_step(batch, p, None, fl)), _step_outputs(_train_step(plain, p, cache.labels, fl)), 'step')
    _same(_eval_step(batch, p, None, 0), _eval_step(plain, p, cache.labels, 0), 'eval')


def test_out_of_range_ids_are_clamped_and_counted(gpu):
    """the cache is a view into a larger allocation whose bytes outside it are NaN: an id outside [0, T) reads the
    cache's first or last image, never a neighbour"""
    P, C, K = 33, 768, 3
    src = _cache(P, C, gpu)
    big = torch.full((T + 2,) + tuple(src.shape[1:]), float('nan'), dtype=BF, device=gpu)
    big[1:T + 1].copy_(src.features)
    cache = cof.FeatureCache(big[1:T + 1], src.labels)
    assert cache.features.data_ptr() == big.data_ptr() + 2 * P * C and cache.features.data_ptr() % 16 == 0
    p = _params(C, K, 'id', src, gpu)
    fl = _flags('id', True)
    G = _grad(3, K, gpu)
    bad, good = cache.select([-1, T + 3, 2]), cache.select([0, T - 1, 2])
    want = _separate(good, p, G, fl)
    assert int(cache.status) == 0
    _same(_separate(bad, p, G, fl), want, 'fwd/bwd')
    assert int(cache.status) == 2                           # the forward product counts, the backward call does not
    cache.status.zero_()
    want = _step_outputs(_train_step(good, p, None, fl))
    assert int(cache.status) == 0
    _same(_step_outputs(_train_step(bad, p, None, fl)), want, 'step')       # (labels through the clamped id too)
    assert int(cache.status) == 2                           # once per step
    _same(want, _step_outputs(_train_step(src.gather([0, T - 1, 2]), p, _labels(src, [0, T - 1, 2], K, gpu), fl)),
          'the clamped batch')
    cache.status.zero_()
    _same(_eval_step(bad, p, None, 0), _eval_step(good, p, None, 0), 'eval')
    assert int(cache.status) == 2


def test_rebind_index_swaps_the_batch(gpu):
    N, P, C, K = 4, 25, 2048, 51
    cache = _cache(P, C, gpu)
    p = _params(C, K, 'id', cache, gpu)
    fl = _flags('id', True)
    st = _train_step(cache.select(FULL_INDEX[:N]), p, None, fl)
    first = {k: v.clone() for k, v in _step_outputs(st).items()}
    ws = st.workspace.data_ptr()
    other = [2, 5, 4, 4]
    st.rebind(index=torch.tensor(other, dtype=torch.int32, device=gpu))
    st.run()
    _same(_step_outputs(st), _step_outputs(_train_step(cache.gather(other), p, _labels(cache, other, K, gpu), fl)),
          'rebound')
    st.rebind(index=FULL_INDEX[:N])
    st.run()
    _same(_step_outputs(st), first, 'bound back')
    assert st.workspace.data_ptr() == ws
    with pytest.raises(cof.ApaError):
        st.rebind(index=[1, 2])
    batch = cache.select(FULL_INDEX[:N])
    e = cof.HeadEvalStep(batch, batch, p['Wa'], p['ba'], p['Wt'], p['bt'], flags=0)
    e.run()
    e.rebind(index=other)
    e.run()
    _same(dict(logits=e.logits, probs=e.probs, pred=e.pred, loss=e.loss),
          {k: v for k, v in _eval_step(cache.gather(other), p, _labels(cache, other, K, gpu), 0).items()
           if k in ('logits', 'probs', 'pred', 'loss')}, 'eval, rebound')


# ------------------------------------------------------------------------------------------ 3: clips
@pytest.mark.parametrize('temporal', [False, True], ids=['mean', 'temporal'])
@pytest.mark.parametrize('loss', ['softmax-xentropy', 'multi-label'])
def test_clips_and_sigmoid_losses(gpu, loss, temporal):
    """2 clips x 2 frames x 7 x 7 x 256, K = 8 (and the flat sigmoid step); evaluation at 2 x 3 frames"""
    P, C, K, B, F = 49, 256, 8, 2, 2
    cache = _cache(P, C, gpu)
    index = [6, 0, 6, 3]
    p = _params(C, K, 'id', cache, gpu)
    fl = _flags('id', True)
    g = torch.Generator().manual_seed(11)
    tw, tb = (torch.rand(K, generator=g) - 0.5).to(gpu), torch.full((1,), 0.5, device=gpu)

    def labels_for(rows):
        if loss == 'softmax-xentropy':
            return torch.randint(0, K, (rows,), generator=torch.Generator().manual_seed(rows)).to(gpu)
        return (torch.rand(rows, K, generator=torch.Generator().manual_seed(rows)) < 0.3).float().to(gpu)

    def step(X, rows, **kw):
        if kw.get('temporal') is not None:
            kw['temporal_grads'] = (torch.empty_like(tw), torch.empty_like(tb))
        st = _train_step(X, p, labels_for(rows), fl, action_loss=loss, pos_weight=10.0, **kw)
        out = _step_outputs(st)
        if kw.get('temporal') is not None:
            out['dtw'], out['dtb'] = kw['temporal_grads']
        return out
    kw = dict(frames=F, temporal=(tw, tb) if temporal else None)
    _both(lambda X: step(X, B, **kw), cache.select(index), cache.gather(index), 'clip step %s' % loss)
    if loss != 'softmax-xentropy' and not temporal:         # the flat sigmoid step rides on the same entry point
        _both(lambda X: step(X, len(index)), cache.select(index), cache.gather(index), 'flat sigmoid step')
    if loss == 'softmax-xentropy':
        idx6 = [6, 0, 6, 3, 1, 5]
        lab = labels_for(2)
        ekw = dict(frames=3, temporal=(tw, tb) if temporal else None)
        _both(lambda X: _eval_step(X, p, lab, 0, **ekw), cache.select(idx6), cache.gather(idx6), 'clip eval',
              fused_dw=False)
        _both(lambda X: _eval_step(X, p, None, 0, scores='sigmoid', **ekw), cache.select(idx6), cache.gather(idx6),
              'clip eval, sigmoid scores', fused_dw=False)


# ------------------------------------------------------------------------------------------ 4: deploy
def _network(fx, gpu, training):
    fx.meta['is_training'] = training
    network_fn, cfg = rf.build_head(fx, device=gpu)
    with torch.no_grad():
        for vn, t in rf.module_tf_names(network_fn).items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).reshape(t.shape).to(gpu))
    seed, step = fx.meta.get('libmask') or (SEED, OFFSET)
    network_fn.head.seed, network_fn.head._step = int(seed), int(step)
    return network_fn, cfg


def test_deploy_fused_step_and_eval_on_a_per_class_cache(gpu):
    """the per-class HMDB-style clip fixture (2 clips x 3 frames x 3 x 3 x 256, K = 51): its frames in a bf16 cache, fed
    flat (a CachedBatch) and as clips (a CachedClips); each equals the same object on the gathered tensor, bit for bit"""
    from attentionalpoolingaction_amd import config as apa_config, deploy
    name = os.path.join(rf.GOLD, 'ref_vstep_perclass_framepool_bf16_c256.npz')
    try:
        fx = rf.HeadFixture(name)
        images = torch.from_numpy(fx.arrays['in/images']).to(gpu).to(BF)          # [B, F, H, W, C]
        B, F = images.shape[:2]
        frames = images.reshape(-1, *images.shape[2:])
        order = list(range(B * F - 1, -1, -1))                                     # the cache holds them reversed
        clip_labels = torch.from_numpy(fx.arrays['in/labels_action']).to(gpu).reshape(B).long()
        frame_labels = clip_labels.repeat_interleave(F)
        cache = cof.FeatureCache(torch.cat([frames[order], frames[:1] * 3.0]).contiguous(),
                                 torch.cat([frame_labels[order], frame_labels[:1]]).contiguous())
        cache.set_videos([B * F - F * (v + 1) for v in range(B)], [F] * B, labels=clip_labels)

        def run_step(batch, labels):
            network_fn, cfg = _network(rf.HeadFixture(name), gpu, True)
            fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
            fused.make_optimizer(0.01)                      # the per-class step then keeps weight images
            total, ep = fused(batch, labels)
            total.backward()
            st = fused._step_obj
            assert st.frozen_input and st.dX_scratch is None and st.weight_image_maps
            out = dict(total=total.detach().reshape(1), logits=ep['Logits'], att=ep['PosePrelogitsBasedAttention'],
                       bucket=fused.bucket.flat.clone())
            if 'logits_beforePool' in ep:
                out['frame_logits'] = ep['logits_beforePool']
            return out
        # flat: six frames as six images, labels through the index on the cache
        want = run_step(frames.contiguous(), frame_labels)
        _same(run_step(cache.select(order), None), want, 'FusedHeadStep, flat')
        assert float(want['bucket'].abs().max()) > 0
        # clips: sampled on the device, F frames of each video, reversed in the cache
        clips = cache.sample_clips(list(range(B)), F, mode='uniform')
        gathered = cache.gather(clips.index).reshape(B, F, *frames.shape[1:])
        want = run_step(gathered, clips.labels)
        assert want['logits'].shape[0] == B
        _same(run_step(clips, None), want, 'FusedHeadStep, clips')

        def run_eval(batch):
            net_e, cfg_e = _network(rf.HeadFixture(name), gpu, False)
            scores, pred, ep = deploy.FusedHeadEval(net_e, cfg_e)(batch)
            return dict(scores=scores, pred=pred, logits=ep['Logits'], att=ep['PosePrelogitsBasedAttention'])
        _same(run_eval(cache.select(order)), run_eval(frames.contiguous()), 'FusedHeadEval, flat')
        _same(run_eval(clips), run_eval(gathered), 'FusedHeadEval, clips')
        assert int(cache.status) == 0
    finally:
        apa_config.reset_cfg()
