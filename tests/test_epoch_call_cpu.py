"""A whole frozen-feature epoch behind one host call, without a GPU: the header, the ctypes table and the library agree
on the new names; every refusal of the two epoch calls and of apa_epoch_order is made, by name, before any HIP call
(dummy pointers: a call that got past its checks would fault); the host restatement of the epoch-order rule is a
bijection and spreads like a uniform permutation; DeviceEvaluation.reserve; the deploy layer's refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
NEW = ('apa_epoch_order', 'apa_attn_head_train_epoch_cached', 'apa_attn_head_eval_epoch_cached')
FAKE = 0x10000                       # a 16-byte aligned non-null address: nothing is dereferenced
FROZEN = cof.APA_FLAG_FROZEN_INPUT


# ------------------------------------------------------------------------------------------ ABI
def test_header_table_and_library_agree_on_the_new_names():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    bare = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(apa_[a-z0-9_]+)\s*\(', bare))
    lib = cof.load_library()
    for name in NEW:
        assert name in declared and name in cof.exported_symbols() and hasattr(lib, name), name
    assert int(re.search(r'#define APA_VERSION (\d+)', header).group(1)) >= 314 and lib.apa_version() >= 314
    # the two descriptors: field order and types are the ABI
    m = re.search(r'typedef struct apa_epoch \{(.*?)\} apa_epoch;', bare, flags=re.S)
    assert [f.strip() for f in m.group(1).split(';') if f.strip()] == ['const int32_t* order', 'int count']
    assert [n for n, _ in cof.ApaEpoch._fields_] == ['order', 'count'] and ctypes.sizeof(cof.ApaEpoch) == 16
    m = re.search(r'typedef struct apa_epoch_sgd \{(.*?)\} apa_epoch_sgd;', bare, flags=re.S)
    fields = [f.strip() for f in m.group(1).split(';') if f.strip()]
    assert fields == ['int nseg', 'float* const* weights', 'const size_t* sizes', 'const float* weight_decay',
                      'const float* grad_flat', 'float* acc_flat', 'const float* lr', 'float momentum, grad_scale']
    assert [n for n, _ in cof.ApaEpochSgd._fields_] == ['nseg', 'weights', 'sizes', 'weight_decay', 'grad_flat',
                                                        'acc_flat', 'lr', 'momentum', 'grad_scale']
    assert ctypes.sizeof(cof.ApaEpochSgd) == 64 and cof.ApaEpochSgd.lr.offset == 48
    assert cof.ApaEpochSgd.momentum.offset == 56 and cof.ApaEpochSgd.grad_scale.offset == 60
    # the epoch signatures are the steps' with the epoch descriptors in front
    sig = cof._SIGNATURES
    step = sig['apa_attn_head_train_step_cached']
    assert sig['apa_attn_head_train_epoch_cached'] == (step[0], [ctypes.c_void_p] * 2 + list(step[1]))
    ev = sig['apa_attn_head_eval_step_cached']             # (cache, clip, kind, X ...) -> (ep, cache, kind, X ...)
    assert sig['apa_attn_head_eval_epoch_cached'] == (ev[0], list(ev[1]))


# ------------------------------------------------------------------------------------------ refusals
class _Sgd(object):
    """an apa_epoch_sgd over host arrays of fake device pointers (kept alive here)"""

    def __init__(self, nseg=2, weights=True, sizes=True, wd=True, grad=FAKE, acc=FAKE, lr=True, null_weight=None, n=8):
        k = max(nseg, 1)
        self.w = (ctypes.c_void_p * k)(*[None if i == null_weight else FAKE for i in range(k)])
        self.s = (ctypes.c_size_t * k)(*[4] * k)
        self.d = (ctypes.c_float * k)(*[0.0] * k)
        self.lr = (ctypes.c_float * n)(*[0.1] * n)
        a = ctypes.addressof
        self.c = cof.ApaEpochSgd(nseg, a(self.w) if weights else None, a(self.s) if sizes else None,
                                 a(self.d) if wd else None, grad, acc, a(self.lr) if lr else None, 0.9, 1.0)


def _desc(T=7, labels_cached=0, status=None, index=None):
    return cof.ApaFeatureCache(index, T, labels_cached, status)          # (the epoch calls ignore `index`)


def _ptr(s):
    return None if s is None else ctypes.addressof(s)


def _train(lib, ep='default', opt='default', cache='default', dtype=0, N=4, P=9, C=32, K=8, M=1, flags=FROZEN, xatt=FAKE,
           dX=None, ws_bytes=0, labels=FAKE, loss=FAKE, order=FAKE, count=12, keep=1.0):
    ep = cof.ApaEpoch(order, count) if ep == 'default' else ep
    sgd = _Sgd() if opt == 'default' else opt
    cache = _desc() if cache == 'default' else cache
    rc = lib.apa_attn_head_train_epoch_cached(
        _ptr(ep), None if sgd is None else _ptr(sgd.c), _ptr(cache), None, FAKE, xatt, FAKE, FAKE, FAKE, FAKE, labels,
        1.0, 1.0, FAKE, FAKE, FAKE, FAKE, loss, FAKE, dX, None if xatt == FAKE else FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
        ws_bytes, N, P, C, C, K, M, flags, keep, 0, 0, dtype, None)
    return rc, lib.apa_last_error()


def _eval(lib, ep='default', cache='default', dtype=0, N=8, P=9, C=32, K=8, M=1, flags=0, xatt=FAKE, ws_bytes=0,
          kind=0, order=FAKE, count=19, labels=None, loss=None, probs=FAKE):
    ep = cof.ApaEpoch(order, count) if ep == 'default' else ep
    cache = _desc() if cache == 'default' else cache
    rc = lib.apa_attn_head_eval_epoch_cached(
        _ptr(ep), _ptr(cache), kind, FAKE, xatt, FAKE, FAKE, FAKE, FAKE, labels, FAKE, FAKE, FAKE, FAKE, loss, probs,
        FAKE, FAKE, ws_bytes, N, P, C, C, K, M, flags, dtype, None)
    return rc, lib.apa_last_error()


@pytest.mark.parametrize('dtype', [0, 1, 2], ids=['f32', 'bf16', 'fp8'])
def test_train_epoch_refusals_name_their_reason_before_any_hip_call(dtype):
    lib = cof.load_library()
    fn = b'apa_attn_head_train_epoch_cached'
    # everything in order: the next refusal is the workspace's, nothing was launched
    rc, err = _train(lib, dtype=dtype)
    assert rc == WORKSPACE and b'workspace' in err, err
    rc, err = _train(lib, dtype=dtype, cache=_desc(labels_cached=1, status=FAKE))
    assert rc == WORKSPACE, err
    # the epoch's own
    for kw, word in ((dict(ep=None), b'null apa_epoch'), (dict(order=None), b'null apa_epoch'),
                     (dict(opt=None), b'null apa_epoch_sgd'), (dict(opt=_Sgd(lr=False)), b'null apa_epoch_sgd / lr'),
                     (dict(cache=None), b'null apa_feature_cache'), (dict(N=0), b'non-positive batch size'),
                     (dict(count=3), b'count=3'), (dict(count=0), b'count=0'), (dict(count=-4), b'count=-4'),
                     (dict(count=13), b'count=13 is not a whole'), (dict(order=FAKE + 2), b'4-byte aligned')):
        rc, err = _train(lib, dtype=dtype, **kw)
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
    # the optimiser's own, as apa_momentum_sgd_step makes them
    for opt, word in ((_Sgd(nseg=0), b'nseg=0'), (_Sgd(nseg=17), b'nseg=17'), (_Sgd(weights=False), b'bad arguments'),
                      (_Sgd(sizes=False), b'bad arguments'), (_Sgd(wd=False), b'bad arguments'),
                      (_Sgd(grad=None), b'bad arguments'), (_Sgd(acc=None), b'bad arguments'),
                      (_Sgd(null_weight=1), b'weights[1] is NULL')):
        rc, err = _train(lib, dtype=dtype, opt=opt)
        assert rc == INVALID and word in err and b'apa_epoch_sgd' in err and fn in err, (word, rc, err)
    # ... in front of the descriptor's and the step's
    rc, err = _train(lib, dtype=dtype, opt=_Sgd(nseg=0), cache=_desc(T=0))
    assert rc == INVALID and b'nseg=0' in err
    # what cache_check refuses
    for kw, word in ((dict(cache=_desc(T=0)), b'cache_images=0'), (dict(dX=FAKE), b'dX must be NULL'),
                     (dict(flags=0), b'APA_FLAG_FROZEN_INPUT'), (dict(P=0), b'non-positive'), (dict(dtype=3), b'unknown dtype')):
        rc, err = _train(lib, **dict(dict(dtype=dtype), **kw))
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
    other = FAKE + 0x1000
    for kw, word in ((dict(M=8), b'per-class maps'), (dict(xatt=other), b'separate attention input'),
                     (dict(flags=FROZEN | cof.APA_FLAG_SOFTMAX_ATT), b'APA_FLAG_SOFTMAX_ATT'),
                     (dict(flags=FROZEN | cof.APA_FLAG_RELU_INPUT), b'APA_FLAG_RELU_INPUT'),
                     (dict(flags=FROZEN | cof.APA_FLAG_RNG_EXTERNAL | cof.APA_FLAG_TRAIN), b'APA_FLAG_RNG_EXTERNAL')):
        rc, err = _train(lib, dtype=dtype, **kw)
        assert rc == UNSUPPORTED and word in err and b'feature cache' in err and fn in err, (kw, rc, err)
    # what the step refuses, once for the shape and still in front of the first launch
    rc, err = _train(lib, dtype=dtype, labels=None)
    assert rc == INVALID and b'null labels / loss / G' in err and fn in err, err
    rc, err = _train(lib, dtype=dtype, loss=None)
    assert rc == INVALID and b'null labels / loss / G' in err, err
    rc, err = _train(lib, dtype=dtype, flags=FROZEN | cof.APA_FLAG_TRAIN, keep=0.0)
    assert rc == INVALID and b'keep_prob' in err, err
    if dtype == 2:
        rc, err = _train(lib, dtype=2, C=24)
        assert rc == UNSUPPORTED and b'multiple of 16' in err and b'APA_DTYPE_FP8_E4M3' in err, err
    else:
        rc, err = _train(lib, dtype=dtype, C=30)
        assert rc == UNSUPPORTED and b'16-byte vectors' in err, err


@pytest.mark.parametrize('dtype', [0, 1, 2], ids=['f32', 'bf16', 'fp8'])
def test_eval_epoch_refusals_name_their_reason_before_any_hip_call(dtype):
    lib = cof.load_library()
    fn = b'apa_attn_head_eval_epoch_cached'
    rc, err = _eval(lib, dtype=dtype)
    assert rc == WORKSPACE and b'workspace' in err, err
    rc, err = _eval(lib, dtype=dtype, kind=cof.APA_SCORES_SIGMOID)
    assert rc == WORKSPACE, err
    rc, err = _eval(lib, dtype=dtype, count=3)                      # fewer rows than one batch: one short step
    assert rc == WORKSPACE, err
    rc, err = _eval(lib, dtype=dtype, cache=_desc(labels_cached=1), labels=FAKE, loss=FAKE)
    assert rc == WORKSPACE, err
    for kw, word in ((dict(ep=None), b'null apa_epoch'), (dict(order=None), b'null apa_epoch'),
                     (dict(cache=None), b'null apa_feature_cache'), (dict(N=0), b'non-positive batch size'),
                     (dict(count=0), b'count=0'), (dict(count=-1), b'count=-1'),
                     (dict(count=2 ** 31 - 1), b'past 2^31 - 1'),      # ceil(count / 8) * 8 = 2^31
                     (dict(order=FAKE + 1), b'4-byte aligned'), (dict(cache=_desc(T=-3)), b'cache_images=-3'),
                     (dict(kind=5), b'scores kind'), (dict(probs=None), b'null logits / probs / pred'),
                     (dict(labels=FAKE), b'labels and loss must be given together'),
                     (dict(kind=cof.APA_SCORES_SIGMOID, labels=FAKE, loss=FAKE), b'sigmoid scores take no labels'),
                     (dict(K=0), b'non-positive')):
        rc, err = _eval(lib, dtype=dtype, **kw)
        assert rc == INVALID and word in err and fn in err, (kw, rc, err)
    for kw, word in ((dict(M=8), b'per-class maps'), (dict(xatt=FAKE + 0x1000), b'separate attention input'),
                     (dict(flags=cof.APA_FLAG_SOFTMAX_ATT), b'APA_FLAG_SOFTMAX_ATT')):
        rc, err = _eval(lib, dtype=dtype, **kw)
        assert rc == UNSUPPORTED and word in err and b'feature cache' in err and fn in err, (kw, rc, err)


def test_epoch_order_refusals():
    lib = cof.load_library()
    for args, word in (((None, 5, 1, 2, None), b'4-byte aligned'), ((FAKE + 2, 5, 1, 2, None), b'4-byte aligned'),
                       ((FAKE, 0, 1, 2, None), b'T=0'), ((FAKE, -7, 1, 2, None), b'T=-7')):
        assert lib.apa_epoch_order(*args) == INVALID and word in lib.apa_last_error(), args
    with pytest.raises(cof.ApaError, match='T < 2\\^31'):
        cof.epoch_order(0, 1, 2, 'cpu')
    with pytest.raises(cof.ApaError, match='T < 2\\^31'):
        cof._epoch_order_rule_cpu(2 ** 31, 1, 2)
    with pytest.raises(cof.ApaError, match='out must be'):
        cof.epoch_order(5, 1, 2, 'cpu', out=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(cof.ApaError, match='out must be'):
        cof.epoch_order(5, 1, 2, 'cpu', out=torch.zeros(6, dtype=torch.int32))


# ------------------------------------------------------------------------------------------ the rule on the host
def _order(T, seed, epoch):
    o = cof._epoch_order_rule_cpu(T, seed, epoch)
    assert o.dtype == torch.int32 and tuple(o.shape) == (T,)
    return o.numpy().astype(np.int64)


@pytest.mark.parametrize('lo,hi', [(1, 101), (101, 201), (201, 301)])
def test_host_rule_is_a_bijection_for_every_small_T(lo, hi):
    for T in range(lo, hi):
        for seed, epoch in ((0, 0), (7, 3), (2 ** 64 - 1, 2 ** 40 + 5)):
            assert np.array_equal(np.sort(_order(T, seed, epoch)), np.arange(T)), (T, seed, epoch)


@pytest.mark.parametrize('T', [1000, 4096, 16385, 100003])
def test_host_rule_is_a_bijection(T):
    a = _order(T, 7, 3)
    assert np.array_equal(np.sort(a), np.arange(T))
    assert np.array_equal(a, _order(T, 7, 3))                               # a pure function of (T, seed, epoch)
    assert not np.array_equal(a, _order(T, 7, 4)) and not np.array_equal(a, _order(T, 8, 3))


def test_cache_order_on_the_cpu_is_the_host_rule():
    cache = cof.FeatureCache(torch.zeros(37, 1, 1, 16))
    o = cache.order(5, 2)
    assert o.dtype == torch.int32 and torch.equal(o, cof._epoch_order_rule_cpu(37, 5, 2))
    buf = torch.full((37,), -1, dtype=torch.int32)
    assert cache.order(5, 3, out=buf) is buf and torch.equal(buf, cof._epoch_order_rule_cpu(37, 5, 3))
    assert not torch.equal(buf, o)


@pytest.mark.parametrize('what', ['epochs', 'seeds'])
def test_host_rule_spreads_like_a_uniform_permutation(what):
    """T = 4096, 16 consecutive epochs of one seed and 16 seeds of one epoch: any two orders agree in fewer than 40
    positions (uniform expectation 1), each has fewer than 40 fixed points, and the mean displacement lies within 10 %
    of T / 3 (the uniform expectation; its standard deviation at this T is about 0.4 %)."""
    T = 4096
    orders = [_order(T, 5, e) for e in range(16)] if what == 'epochs' else [_order(T, s, 2) for s in range(16)]
    pos = np.arange(T)
    for i, a in enumerate(orders):
        assert int((a == pos).sum()) < 40, (what, i)
        assert abs(float(np.abs(a - pos).mean()) / (T / 3.0) - 1.0) < 0.10, (what, i)
        for j in range(i):
            assert int((a == orders[j]).sum()) < 40, (what, i, j)


def test_host_rule_position_value_table_at_T_8():
    """seeds 0..8191, epoch 0: the chi-square statistic of the 8 x 8 position / value table stays below 85.4, the 0.999
    quantile for 49 degrees of freedom"""
    table = np.zeros((8, 8))
    pos = np.arange(8)
    for seed in range(8192):
        table[pos, _order(8, seed, 0)] += 1
    e = 8192 / 8.0
    chi2 = float(((table - e) ** 2 / e).sum())
    print('chi-square', chi2)
    assert chi2 < 85.4, chi2


# ------------------------------------------------------------------------------------------ DeviceEvaluation.reserve
@pytest.mark.parametrize('multi_label', [False, True])
def test_reserve_hands_out_the_meters_own_rows(multi_label):
    from attentionalpoolingaction_amd import eval_utils
    m = eval_utils.DeviceEvaluation(10, 3, 'cpu', multi_label=multi_label)
    m.update(torch.full((2, 3), 0.5), torch.ones(2, 3) if multi_label else torch.tensor([1, 2]))
    scores, truth = m.reserve(5)
    assert len(m) == 7 and tuple(scores.shape) == (5, 3) and scores.is_contiguous()
    assert tuple(truth.shape) == ((5, 3) if multi_label else (5,))
    assert truth.dtype == (torch.float32 if multi_label else torch.int64)
    assert scores.data_ptr() == m._scores.data_ptr() + 2 * 3 * 4            # the rows at the cursor, in place
    assert truth.data_ptr() == m._truth.data_ptr() + 2 * (12 if multi_label else 8)
    scores.fill_(0.25)
    assert torch.equal(m._scores[2:7], torch.full((5, 3), 0.25)) and torch.equal(m._scores[:2], torch.full((2, 3), 0.5))
    s2, _ = m.reserve(3)
    assert len(m) == 10 and s2.data_ptr() == m._scores.data_ptr() + 7 * 3 * 4
    with pytest.raises(ValueError, match='overflow the capacity'):
        m.reserve(1)
    with pytest.raises(ValueError, match='n >= 1'):
        m.reserve(0)
    m.reset()
    assert len(m) == 0 and m.reserve(10)[0].data_ptr() == m._scores.data_ptr()


# ------------------------------------------------------------------------------------------ deploy
def _cfg002(device='cpu', **train):
    from tests import _ref_fixture as rf
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz'))
    fx.meta = dict(fx.meta, train_cfg=dict(fx.meta['train_cfg'], **train))
    return rf.build_head(fx, device=device)


def test_deploy_train_epoch_refusals_name_their_reason():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    cache = cof.FeatureCache(torch.zeros(8, 3, 3, 2048), torch.zeros(8, dtype=torch.int64))
    order = cache.order(1, 0)
    try:
        network_fn, cfg = _cfg002()
        fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
        with pytest.raises(ValueError, match='make_optimizer\\(\\) first'):
            fused.train_epoch(cache, 4, order)
        assert fused.epoch_unsupported_reason(cache) == ''
        fused.make_optimizer(0.01)
        with pytest.raises(ValueError, match='FeatureCache without labels'):
            fused.train_epoch(cof.FeatureCache(torch.zeros(8, 3, 3, 2048)), 4, order)
        with pytest.raises(ValueError, match='not a whole number of batches of 3'):
            fused.train_epoch(cache, 3, order)
        with pytest.raises(ValueError, match='one learning rate per step'):
            fused.train_epoch(cache, 4, order, lr=[0.1])
        with pytest.raises(cof.ApaError, match='GPU memory'):          # no CPU fallback
            fused.train_epoch(cache, 4, order)
        fused.loss_scale = 0.5
        with pytest.raises(ValueError, match='more than one clone'):
            fused.train_epoch(cache, 4, order)
        with pytest.raises(ValueError, match='frozen_features=False'):
            f = deploy.FusedHeadStep(network_fn, cfg, frozen_features=False)
            f.make_optimizer(0.01)
            f.train_epoch(cache, 4, order)
        for train, word in ((dict(OPTIMIZER='adam'), "TRAIN.OPTIMIZER 'adam'"), (dict(ITER_SIZE=2), 'TRAIN.ITER_SIZE 2'),
                            (dict(CLIP_GRADIENTS=1.0), 'TRAIN.CLIP_GRADIENTS > 0'),
                            (dict(LOSS_FN_ACTION='multi-label'), "LOSS_FN_ACTION 'multi-label'")):
            net, c = _cfg002(**train)
            f = deploy.FusedHeadStep(net, c, frozen_features=True)
            f.make_optimizer(0.01)
            with pytest.raises(ValueError, match='train_epoch: an epoch call is not served with ' + re.escape(word)):
                f.train_epoch(cache, 4, order)
        fx3 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_train.npz'))
        net3, cfg3 = rf.build_head(fx3, device='cpu', in_channels=2048)
        f3 = deploy.FusedHeadStep(net3, cfg3, frozen_features=True)
        f3.make_optimizer(0.01)
        with pytest.raises(ValueError, match='not served with attention from pose_pre_logits'):
            f3.train_epoch(cache, 4, order)
    finally:
        apa_config.reset_cfg()


def test_deploy_evaluate_cache_refusals_name_their_reason():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    cache = cof.FeatureCache(torch.zeros(8, 3, 3, 2048), torch.zeros(8, dtype=torch.int64))
    try:
        fxe = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_eval_c2048.npz'))
        net, cfg = rf.build_head(fxe, device='cpu')
        ev = deploy.FusedHeadEval(net, cfg)
        with pytest.raises(ValueError, match='FeatureCache without labels'):
            ev.evaluate_cache(cof.FeatureCache(torch.zeros(8, 3, 3, 2048)), 4)
        with pytest.raises(ValueError, match='batch_size >= 1'):
            ev.evaluate_cache(cache, 0)
        with pytest.raises(cof.ApaError, match='int32 vector'):
            ev.evaluate_cache(cache, 4, order=torch.arange(8))
        meter = ev.new_evaluation(8)
        with pytest.raises(cof.ApaError, match='GPU memory'):          # no CPU fallback; the meter was not advanced
            ev.evaluate_cache(cache, 4, meter=meter)
        assert len(meter) == 0
        ev.multi_label = True
        with pytest.raises(ValueError, match='multi-hot targets'):
            ev.evaluate_cache(cache, 4)
        fx3 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_eval.npz'))
        net3, cfg3 = rf.build_head(fx3, device='cpu', in_channels=2048)
        with pytest.raises(ValueError, match='not served with attention from pose_pre_logits'):
            deploy.FusedHeadEval(net3, cfg3).evaluate_cache(cache, 4)
    finally:
        apa_config.reset_cfg()
