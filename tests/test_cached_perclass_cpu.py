"""Per-class attention maps (M == K) from the resident feature cache, without a GPU: which *_cached calls are admitted
(a bf16 cache whose shape is on the fused per-class route) and which keep their refusal, each by name and before any HIP
call; the python wrappers' and the deploy layer's side of the same rule.  (Dummy pointers throughout: a call that got
past its checks would fault -- an admitted call stops at the workspace check, still in front of the first launch.)"""
import ctypes
import os

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
FAKE = 0x10000                       # a 16-byte aligned non-null address: nothing is dereferenced
FROZEN = cof.APA_FLAG_FROZEN_INPUT
BF16, F32, FP8 = 1, 0, 2
ATT = {'identity': 0, 'relu': cof.APA_FLAG_RELU_ATT, 'softmax': cof.APA_FLAG_SOFTMAX_ATT}
CACHE_TEXT = ('%s: a feature cache does not serve %s: the gathered kernels feed the fused class-agnostic head with '
              'identity or relu attention')


def _desc(index=FAKE, T=7, labels_cached=0, status=None):
    return cof.ApaFeatureCache(index, T, labels_cached, status)


def _ptr(s):
    return None if s is None else ctypes.addressof(s)


def _clip(frames=2):
    c = cof.ApaClipPool()
    c.frames, c.w, c.b, c.pooled, c.tatt, c.dw, c.db = frames, None, None, FAKE, None, None, None
    return c


def _ml():
    m = cof.ApaMultilabel()
    m.kind, m.labels, m.pos_weight = cof.ACTION_LOSS_KINDS['multi-label'], FAKE, 10.0
    return m


class _Calls(object):
    """the six entry points on dummy pointers; every call returns (status, message)"""

    def __init__(self):
        self.lib = cof.load_library()
        self.keep = []

    def _done(self, rc):
        return rc, self.lib.apa_last_error().decode()

    def fwd(self, cache, dtype=BF16, N=4, P=9, C=256, K=8, M=8, flags=0, X=FAKE, xatt=None, topdown=None, dX=None):
        xatt = X if xatt is None else xatt
        return self._done(self.lib.apa_attn_pool_fwd_cached(
            _ptr(cache), None, X, xatt, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, topdown, FAKE, 0, N, P, C, C, K,
            M, flags & ~FROZEN, 1.0, 0, 0, dtype, None))

    def bwd(self, cache, dtype=BF16, N=4, P=9, C=256, K=8, M=8, flags=0, X=FAKE, xatt=None, topdown=None, dX=None):
        xatt = X if xatt is None else xatt
        return self._done(self.lib.apa_attn_pool_bwd_cached(
            _ptr(cache), None, X, xatt, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, dX, None if xatt == X else FAKE,
            FAKE, FAKE, FAKE, FAKE, FAKE, 0, N, P, C, C, K, M, flags, 1.0, 0, 0, dtype, None))

    def step(self, cache, dtype=BF16, N=4, P=9, C=256, K=8, M=8, flags=0, X=FAKE, xatt=None, topdown=None, dX=None):
        xatt = X if xatt is None else xatt
        return self._done(self.lib.apa_attn_head_train_step_cached(
            _ptr(cache), None, X, xatt, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, 1.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, dX,
            None if xatt == X else FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, N, P, C, C, K, M, flags, 1.0, 0, 0, dtype,
            None))

    def ev(self, cache, dtype=BF16, N=4, P=9, C=256, K=8, M=8, flags=0, X=FAKE, xatt=None, topdown=None, dX=None):
        xatt = X if xatt is None else xatt
        return self._done(self.lib.apa_attn_head_eval_step_cached(
            _ptr(cache), None, 0, X, xatt, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE,
            0, N, P, C, C, K, M, flags & ~FROZEN, dtype, None))

    def step_clips(self, cache, dtype=BF16, N=4, P=9, C=256, K=8, M=8, flags=0, X=FAKE, xatt=None, topdown=None,
                   dX=None, ml=None):
        xatt = X if xatt is None else xatt
        clip = _clip()
        return self._done(self.lib.apa_attn_head_train_step_cached_clips(
            _ptr(cache), _ptr(ml), _ptr(clip), None, X, xatt, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, 1.0, FAKE, FAKE, FAKE,
            FAKE, FAKE, FAKE, dX, None if xatt == X else FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, N, P, C, C, K, M, flags,
            1.0, 0, 0, dtype, None))

    def ev_clips(self, cache, dtype=BF16, N=4, P=9, C=256, K=8, M=8, flags=0, X=FAKE, xatt=None, topdown=None,
                 dX=None):
        xatt = X if xatt is None else xatt
        clip = _clip()
        return self._done(self.lib.apa_attn_head_eval_step_cached_clips(
            _ptr(cache), _ptr(clip), 0, X, xatt, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE,
            FAKE, 0, N, P, C, C, K, M, flags & ~FROZEN, dtype, None))

    def all(self):
        return (self.fwd, self.bwd, self.step, self.ev, self.step_clips, self.ev_clips)

    def training(self):
        return (self.bwd, self.step, self.step_clips)


# ------------------------------------------------------------------------------------------ admission
@pytest.mark.parametrize('att', sorted(ATT))
def test_every_cached_entry_point_admits_the_fused_per_class_shape(att):
    """M = K = 8, C = 256, bf16: each call stops at the workspace refusal, where it used to stop at 'per-class maps'"""
    c = _Calls()
    for call in c.all():
        rc, err = call(_desc(), flags=ATT[att] | FROZEN)
        assert rc == WORKSPACE and 'workspace' in err, (call.__name__, att, rc, err)
        # ... with dropout on, too (the training calls)
        if call in c.training():
            rc, err = call(_desc(), flags=ATT[att] | FROZEN | cof.APA_FLAG_TRAIN)
            assert rc == WORKSPACE, (call.__name__, att, rc, err)
    # labels through the index on the flat step and on the evaluation step
    for call in (c.step, c.ev):
        rc, err = call(_desc(labels_cached=1, status=FAKE), flags=ATT[att] | FROZEN)
        assert rc == WORKSPACE, (call.__name__, rc, err)
    # the sigmoid loss on clips, and the edges of the rule: K = 64, C = 8192, K = 1 is M == 1
    rc, err = c.step_clips(_desc(), flags=ATT[att] | FROZEN, ml=_ml())
    assert rc == WORKSPACE, err
    for kw in (dict(K=64, M=64), dict(C=8192), dict(C=2048, K=51, M=51, N=32, P=196)):
        rc, err = c.step(_desc(), flags=ATT[att] | FROZEN, **kw)
        assert rc == WORKSPACE, (kw, rc, err)


def test_weight_images_flag_is_admitted():
    c = _Calls()
    rc, err = c.step(_desc(), flags=FROZEN | cof.APA_FLAG_TRAIN | cof.APA_FLAG_WEIGHT_IMAGES)
    assert rc == WORKSPACE, err


# ------------------------------------------------------------------------------------------ refusals that remain
def test_per_class_outside_the_fused_route_keeps_its_sentence():
    """fp32 and FP8 caches, K = 65, C = 384, C = 8448: APA_ERR_UNSUPPORTED with today's sentence, byte for byte"""
    c = _Calls()
    names = {c.fwd: 'apa_attn_pool_fwd_cached', c.bwd: 'apa_attn_pool_bwd_cached',
             c.step: 'apa_attn_head_train_step_cached', c.ev: 'apa_attn_head_eval_step_cached',
             c.step_clips: 'apa_attn_head_train_step_cached_clips', c.ev_clips: 'apa_attn_head_eval_step_cached_clips'}
    for call in c.all():
        for kw in (dict(dtype=F32), dict(dtype=FP8), dict(K=65, M=65), dict(C=384), dict(C=8448), dict(C=32),
                   dict(C=8192 + 256)):
            rc, err = call(_desc(), flags=FROZEN, **kw)
            assert rc == UNSUPPORTED and err == CACHE_TEXT % (names[call], 'per-class maps (M != 1)'), (kw, rc, err)


def test_forms_a_cache_cannot_have_stay_refused_for_per_class_maps():
    c = _Calls()
    other = FAKE + 0x1000
    for call in c.all():
        for kw, word in ((dict(xatt=other), 'separate attention input'),
                         (dict(flags=cof.APA_FLAG_RELU_INPUT), 'APA_FLAG_RELU_INPUT'),
                         (dict(flags=cof.APA_FLAG_RNG_EXTERNAL | cof.APA_FLAG_TRAIN), 'APA_FLAG_RNG_EXTERNAL')):
            kw = dict(kw, flags=kw.get('flags', 0) | FROZEN)
            rc, err = call(_desc(), **kw)
            assert rc == UNSUPPORTED and word in err and 'feature cache' in err, (call.__name__, kw, rc, err)
    rc, err = c.fwd(_desc(), topdown=FAKE)
    assert rc == UNSUPPORTED and 'TopDownAttention' in err and 'feature cache' in err, err
    # a cache has no gradient
    for call in c.training():
        rc, err = call(_desc(), flags=FROZEN, dX=FAKE)
        assert rc == INVALID and 'dX must be NULL' in err, (call.__name__, err)
        rc, err = call(_desc(), flags=0)
        assert rc == INVALID and 'APA_FLAG_FROZEN_INPUT' in err, (call.__name__, err)
    # the fused route fetches the rows by LDS-DMA: a misaligned cache base has a sentence of its own
    for call in c.all():
        rc, err = call(_desc(), flags=FROZEN, X=FAKE + 8)
        assert rc == INVALID and '16-byte aligned' in err and 'per-class' in err, (call.__name__, rc, err)
    # the descriptor is checked as ever
    rc, err = c.step(_desc(T=0), flags=FROZEN)
    assert rc == INVALID and 'cache_images=0' in err
    # labels_cached with a clip: per-clip labels do not come through the frame index
    rc, err = c.step_clips(_desc(labels_cached=1), flags=FROZEN)
    assert rc == INVALID and 'labels_cached' in err


def test_class_agnostic_softmax_is_refused_exactly_as_before():
    c = _Calls()
    for call, fn in ((c.fwd, 'apa_attn_pool_fwd_cached'), (c.step, 'apa_attn_head_train_step_cached')):
        for dtype in (F32, BF16):
            rc, err = call(_desc(), dtype=dtype, M=1, flags=cof.APA_FLAG_SOFTMAX_ATT | FROZEN)
            assert rc == UNSUPPORTED and err == CACHE_TEXT % (fn, 'APA_FLAG_SOFTMAX_ATT'), (fn, dtype, rc, err)
    # and M == 1 without it is served as ever
    rc, err = c.step(_desc(), M=1, flags=FROZEN)
    assert rc == WORKSPACE, err


def test_the_epoch_calls_keep_refusing_per_class_maps():
    lib = cof.load_library()
    ep = cof.ApaEpoch(FAKE, 12)
    k = 2
    w = (ctypes.c_void_p * k)(FAKE, FAKE)
    s = (ctypes.c_size_t * k)(4, 4)
    d = (ctypes.c_float * k)(0.0, 0.0)
    lr = (ctypes.c_float * 8)(*[0.1] * 8)
    a = ctypes.addressof
    sgd = cof.ApaEpochSgd(k, a(w), a(s), a(d), FAKE, FAKE, a(lr), 0.9, 1.0)
    cache = _desc(index=None)
    for flags in (0, cof.APA_FLAG_SOFTMAX_ATT):
        rc = lib.apa_attn_head_train_epoch_cached(
            a(ep), a(sgd), a(cache), None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, 1.0, FAKE, FAKE, FAKE, FAKE,
            FAKE, FAKE, None, None, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 4, 9, 256, 256, 8, 8, flags | FROZEN, 1.0, 0, 0,
            BF16, None)
        err = lib.apa_last_error().decode()
        assert rc == UNSUPPORTED and err == CACHE_TEXT % ('apa_attn_head_train_epoch_cached',
                                                          'per-class maps (M != 1)'), (rc, err)
        rc = lib.apa_attn_head_eval_epoch_cached(
            a(ep), a(cache), 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE,
            FAKE, 0, 4, 9, 256, 256, 8, 8, flags, BF16, None)
        err = lib.apa_last_error().decode()
        assert rc == UNSUPPORTED and err == CACHE_TEXT % ('apa_attn_head_eval_epoch_cached',
                                                          'per-class maps (M != 1)'), (rc, err)


# ------------------------------------------------------------------------------------------ python wrappers
def _head(C, K, M):
    Wa, ba, Wt, bt = torch.zeros(C, M), torch.zeros(M), torch.zeros(C, K), torch.zeros(K)
    g = (None, None, torch.zeros(C, M), torch.zeros(M), torch.zeros(C, K), torch.zeros(K))
    return Wa, ba, Wt, bt, g


def test_cached_per_class_served_mirrors_the_c_rule():
    def batch(dtype, C):
        return cof.FeatureCache(torch.zeros(3, 2, 2, C, dtype=dtype)).select([1, 0])
    bf = torch.bfloat16
    assert cof.cached_per_class_served(batch(bf, 256), 8) and cof.cached_per_class_served(batch(bf, 8192), 64)
    assert cof.cached_per_class_served(batch(bf, 2048), 51)
    assert not cof.cached_per_class_served(batch(torch.float32, 256), 8)
    assert not cof.cached_per_class_served(batch(bf, 256), 65)
    assert not cof.cached_per_class_served(batch(bf, 384), 8)
    assert not cof.cached_per_class_served(batch(bf, 8448), 8)
    fp8 = cof.FeatureCache.empty((3, 2, 2, 256), torch.float8_e4m3fn, 'cpu').select([1, 0])
    assert not cof.cached_per_class_served(fp8, 8)


def test_bound_steps_take_a_per_class_cached_batch_as_far_as_the_device():
    """a CPU cache: a qualifying bf16 batch is refused only for want of a GPU; an fp32 one, K > 64 or another C keep
    the messages they had"""
    C, K = 256, 8
    Wa, ba, Wt, bt, g = _head(C, K, K)
    bf = cof.FeatureCache(torch.zeros(5, 3, 3, C, dtype=torch.bfloat16), torch.zeros(5, dtype=torch.int64))
    b = bf.select([4, 0, 4, 1])
    labels = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(cof.ApaError, match='GPU memory'):
        cof.HeadTrainStep(b, b, Wa, ba, Wt, bt, labels, g)
    with pytest.raises(cof.ApaError, match='GPU memory'):
        cof.HeadTrainStep(b, b, Wa, ba, Wt, bt, None, g, weight_images=True)       # the cache's own labels
    with pytest.raises(cof.ApaError, match='GPU memory'):
        cof.HeadTrainStep(b, b, Wa, ba, Wt, bt, torch.zeros(2, dtype=torch.int64), g, frames=2)
    with pytest.raises(cof.ApaError, match='GPU memory'):
        cof.HeadEvalStep(b, b, Wa, ba, Wt, bt)
    with pytest.raises(cof.ApaError, match='GPU memory'):
        cof.HeadEvalStep(b, b, Wa, ba, Wt, bt, frames=2)
    f32 = cof.FeatureCache(torch.zeros(5, 3, 3, C)).select([4, 0, 4, 1])
    with pytest.raises(cof.ApaError, match='class-agnostic'):
        cof.HeadTrainStep(f32, f32, Wa, ba, Wt, bt, labels, g)
    with pytest.raises(cof.ApaError, match='no per-class maps'):
        cof.HeadEvalStep(f32, f32, Wa, ba, Wt, bt)
    Wa65, ba65, Wt65, bt65, g65 = _head(C, 65, 65)
    with pytest.raises(cof.ApaError, match='class-agnostic'):
        cof.HeadTrainStep(b, b, Wa65, ba65, Wt65, bt65, labels, g65)
    with pytest.raises(cof.ApaError, match='no per-class maps'):
        cof.HeadEvalStep(b, b, Wa65, ba65, Wt65, bt65)
    odd = cof.FeatureCache(torch.zeros(5, 3, 3, 384, dtype=torch.bfloat16)).select([4, 0, 4, 1])
    Wa3, ba3, Wt3, bt3, g3 = _head(384, K, K)
    with pytest.raises(cof.ApaError, match='class-agnostic'):
        cof.HeadTrainStep(odd, odd, Wa3, ba3, Wt3, bt3, labels, g3)
    # weight images stay a per-class matter, dxatt_rank1 a matter of a separate attention input
    Wa1, ba1, Wt1, bt1, g1 = _head(C, K, 1)
    with pytest.raises(cof.ApaError, match='class-agnostic'):
        cof.HeadTrainStep(b, b, Wa1, ba1, Wt1, bt1, labels, g1, weight_images=True)
    # the epochs are unchanged
    with pytest.raises(cof.ApaError):
        cof.HeadEvalEpoch(bf, 2, Wa, ba, Wt, bt, capacity=4)


# ------------------------------------------------------------------------------------------ deploy
def test_deploy_reasons():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    reason = deploy.FusedHeadStep.cache_unsupported_reason
    try:
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_vstep_perclass_framepool_bf16_c256.npz'))
        network_fn, cfg = rf.build_head(fx, device='cpu')
        head = network_fn.head
        assert head.per_class and head.single_layer and int(head.num_classes) == 51
        # about the head alone: what it always answered
        assert deploy.FusedHeadStep.fp8_unsupported_reason(head, network_fn) == 'per-class attention maps'
        bf = cof.FeatureCache(torch.zeros(8, 3, 3, 256, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.int64))
        bf.set_videos([0, 4], [4, 4], labels=torch.tensor([3, 1]))
        assert reason(head, network_fn, bf.select([1, 0])) == ''
        assert reason(head, network_fn, cof.CachedClips(bf, 2, 2)) == ''
        f32 = cof.FeatureCache(torch.zeros(8, 3, 3, 256))
        assert 'float32 cache' in reason(head, network_fn, f32.select([1, 0]))
        f8 = cof.FeatureCache.empty((8, 3, 3, 256), torch.float8_e4m3fn, 'cpu')
        assert 'FP8 cache' in reason(head, network_fn, f8.select([1, 0]))
        assert reason(head, network_fn, f8.features) == 'per-class attention maps'     # an Fp8Features batch
        odd = cof.FeatureCache(torch.zeros(8, 3, 3, 384, dtype=torch.bfloat16))
        assert 'C % 256 == 0' in reason(head, network_fn, odd.select([1, 0]))
        head.num_classes = 65
        assert 'K = 65' in reason(head, network_fn, bf.select([1, 0]))
        head.num_classes = 51
        # the objects raise what the function says; a served batch gets as far as the missing device
        with pytest.raises(ValueError, match='a CachedBatch is not served with per-class attention maps from a float32'):
            deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)(f32.select([1, 0]), None)
        with pytest.raises(ValueError, match='frozen_features=False'):
            deploy.FusedHeadStep(network_fn, cfg, frozen_features=False)(bf.select([1, 0]), None)
        # the epoch forms keep refusing per-class heads
        assert deploy.FusedHeadStep(network_fn, cfg, frozen_features=True).epoch_unsupported_reason(bf) == \
            'per-class attention maps'
        fxe = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_vstep_perclass_framepool_bf16_c256.npz'))
        fxe.meta['is_training'] = False                     # the same head at evaluation time
        net_e, cfg_e = rf.build_head(fxe, device='cpu')
        with pytest.raises(ValueError, match='a CachedBatch is not served with per-class attention maps from a float32'):
            deploy.FusedHeadEval(net_e, cfg_e)(f32.select([1, 0]))
        with pytest.raises(ValueError, match='per-class attention maps'):
            deploy.FusedHeadEval(net_e, cfg_e).evaluate_cache(bf, 2)
        # a class-agnostic head answers what fp8_unsupported_reason answers, whatever the batch
        fx1 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz'))
        net1, cfg1 = rf.build_head(fx1, device='cpu')
        c1 = cof.FeatureCache(torch.zeros(4, 3, 3, 2048))
        assert reason(net1.head, net1, c1.select([1, 0])) == ''
    finally:
        apa_config.reset_cfg()
