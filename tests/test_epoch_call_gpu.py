"""A whole frozen-feature epoch behind one host call, on the GPU.

The oracle of both epoch calls is the loop they are defined as, run with the entry points that existed before them:
`HeadTrainStep.rebind(index=, offset=, labels=) + run()` and `BoundMomentumSGD.run(lr[s])` per step, `HeadEvalStep` per
batch -- every weight, accumulator, output and the whole loss log must be equal BIT FOR BIT, for one case per M == 1
pooling family at the smallest width it takes.  The device epoch order is compared with its host restatement, and
deploy.FusedHeadStep.train_epoch / FusedHeadEval.evaluate_cache with the per-step deploy loops on the cfg 002 fixtures."""
import os

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _ref_fixture as rf

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
SEED, OFFSET, KEEP = 1234, 7, 0.2
MOMENTUM, LR0 = 0.9, 0.05
NAN = float('nan')


# ------------------------------------------------------------------------------------------ the order
@pytest.mark.parametrize('T', [1, 2, 3, 17, 1000, 16385, 100003])
def test_device_order_is_the_host_rule(gpu, T):
    want = cof._epoch_order_rule_cpu(T, 11, 5)
    a = cof.epoch_order(T, 11, 5, gpu)
    b = cof.epoch_order(T, 11, 5, gpu)
    assert a.dtype == torch.int32 and a.is_cuda and torch.equal(a.cpu(), want) and torch.equal(a, b)
    # out= is rewritten in place, inside guards
    buf = torch.full((T + 8,), -7, dtype=torch.int32, device=gpu)
    out = buf[4:4 + T]
    assert cof.epoch_order(T, 2 ** 63 + 9, 2 ** 40, gpu, out=out) is out
    assert torch.equal(out.cpu(), cof._epoch_order_rule_cpu(T, 2 ** 63 + 9, 2 ** 40))
    assert buf[:4].tolist() == [-7] * 4 and buf[4 + T:].tolist() == [-7] * 4
    cache = cof.FeatureCache(torch.zeros(T, 1, 1, 16, device=gpu))
    assert torch.equal(cache.order(11, 5), a)


# ------------------------------------------------------------------------------------------ inputs
_CACHES = {}


def _cache(dtype, T, P, C, dev, K=12):
    """T images of relu(randn) with a per-image magnitude and their labels; built once, never written afterwards"""
    key = (dtype, T, P, C)
    if key not in _CACHES:
        g = torch.Generator().manual_seed(31 + T + P + C)
        mag = (0.25 + 4.0 * torch.rand((T, 1, 1, 1), generator=g))
        img = (torch.relu(torch.randn(T, P, 1, C, generator=g)) * mag).to(dev)
        labels = torch.randint(0, K, (T,), generator=g).to(dev)
        cache = cof.FeatureCache.empty((T, P, 1, C), dtype, dev, labels=labels)
        assert cache.write(0, img).tolist() == [0] * T
        _CACHES[key] = cache
    return _CACHES[key]


def _weights(C, K, E, dev):
    """Wa, ba, Wt, bt and an extra segment that only decays (cfg 002's pruned PoseLogits weights)"""
    g = torch.Generator().manual_seed(5 + C + K)
    u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
    return [(u(C, 1) * (4.0 / C)).to(dev), (u(1) * 0.1 - 0.3).to(dev), (u(C, K) / C ** 0.5).to(dev),
            (u(K) * 0.1).to(dev), u(E).to(dev)]


WD = [4e-3, 0.0, 2e-3, 0.0, 1e-2]          # (Wa, ba, Wt, bt, extra): non-zero on the weights, zero on the biases
SEGMENTS = [2, 0, 4, 3, 1]                 # the bucket's order: Wt, Wa, extra, bt, ba -- every window 16-byte aligned


def _guarded(shape, dtype, dev):
    """(whole, view): `view` of `shape` sits between 16 sentinel elements on either side"""
    n = int(np.prod(shape))
    whole = torch.full((n + 32,), NAN if dtype.is_floating_point else -77, dtype=dtype, device=dev)
    return whole, whole[16:16 + n].view(shape)


def _guards_untouched(whole, n):
    for part in (whole[:16], whole[16 + n:]):
        assert bool(torch.isnan(part).all()) if whole.dtype.is_floating_point else part.tolist() == [-77] * 16


class _Run(object):
    """one route's own state: weights, flat gradient bucket (the extra segment's window stays zero), accumulators"""

    def __init__(self, C, K, E, dev):
        self.w = _weights(C, K, E, dev)
        n = sum(t.numel() for t in self.w)
        self.grad = torch.zeros((n,), device=dev)
        g = torch.Generator().manual_seed(3)
        self.acc = (torch.rand((n,), generator=g) * 1e-3).to(dev)        # a run that is already under way
        self.segs, self.wd = [self.w[i] for i in SEGMENTS], [WD[i] for i in SEGMENTS]
        o, views = 0, {}
        for i, t in zip(SEGMENTS, self.segs):
            views[i] = self.grad[o:o + t.numel()].view(t.shape)
            o += t.numel()
        self.views = [views[i] for i in range(4)]            # dWa, dba, dWt, dbt
        self.ctr = torch.tensor([OFFSET], dtype=torch.int64, device=dev)


# (family, dtype, C) at the smallest C the family takes (tests/test_feature_cache_gpu.py: COMBOS); P, N, steps, T;
# attention; dropout counter on the device; labels through the order
CASES = [('stream', torch.float32, 1024, 5, 4, 4, 19, 'id', False, True),
         ('stream', torch.bfloat16, 2048, 10, 8, 3, 29, 'relu', True, False),
         ('vec', torch.float32, 256, 7, 4, 5, 23, 'relu', False, False),
         ('generic', torch.float32, 40, 9, 8, 3, 29, 'id', True, True),
         ('fp8', F8, 32, 6, 4, 4, 19, 'relu', True, True)]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s_%s_c%d' % (c[0], str(c[1]).split('.')[-1], c[2]))
def test_training_epoch_is_the_loop(gpu, case):
    _, dtype, C, P, N, steps, T, act, rng_dev, labels_cached = case
    K, E = 12, 36
    assert T % N != 0 and steps * N <= T
    cache = _cache(dtype, T, P, C, gpu)
    flags = cof.APA_FLAG_TRAIN | (cof.APA_FLAG_RELU_ATT if act == 'relu' else 0)
    order = cache.order(21, 3)[:steps * N].clone()
    order[1], order[N + 2] = T + 3, -2                       # two ids outside the cache: clamped, counted once each
    lr = [LR0 * 0.5 ** s for s in range(steps)]
    g = torch.Generator().manual_seed(9)
    labels = None if labels_cached else torch.randint(0, K, (steps * N,), generator=g).to(gpu)

    # ---- the loop, with the entry points the epoch call is defined by
    B = _Run(C, K, E, gpu)
    first = cache.select(order[:N])
    st = cof.HeadTrainStep(first, first, *B.w[:4], None if labels_cached else labels[:N],
                           (None, None) + tuple(B.views), flags=flags, keep_prob=KEEP, seed=SEED,
                           offset=B.ctr if rng_dev else OFFSET)
    sgd = cof.BoundMomentumSGD(B.segs, B.wd, B.grad, B.acc)
    cache.status.zero_()
    log = []
    for s in range(steps):
        st.rebind(index=order[s * N:(s + 1) * N], labels=None if labels_cached else labels[s * N:(s + 1) * N],
                  offset=None if rng_dev else OFFSET + s)
        st.run()
        sgd.run(lr[s], MOMENTUM, 1.0)
        log.append(st.loss.clone())
    status_loop = cache.status.clone()
    assert st.frozen_input and st.dX_scratch is None

    # ---- the epoch call, every output inside guards
    A = _Run(C, K, E, gpu)
    shapes = dict(logits=(N, K), att=(N, P, 1), zsave=(N, C), abar=(N,), loss=(steps + 1, 1 + N), G=(N, K))
    guards = {k: _guarded(s, torch.float32, gpu) for k, s in shapes.items()}
    ep = cof.HeadTrainEpoch(cache, N, *A.w[:4], tuple(A.views), A.segs, A.wd, A.grad, A.acc, steps=steps + 1,
                            momentum=MOMENTUM, labels_cached=labels_cached, flags=flags, keep_prob=KEEP, seed=SEED,
                            offset=A.ctr if rng_dev else OFFSET, outputs={k: v for k, (_, v) in guards.items()})
    cache.status.zero_()
    assert ep.run(order, lr, labels=labels) == steps
    torch.cuda.synchronize()

    for name, a, b in zip(('Wa', 'ba', 'Wt', 'bt', 'extra'), A.w, B.w):
        assert torch.equal(a, b), name
    assert not torch.equal(A.w[4], _weights(C, K, E, gpu)[4])            # the extra segment did decay
    assert torch.equal(A.acc, B.acc) and torch.equal(A.grad, B.grad)
    assert torch.equal(ep.loss[:steps], torch.stack(log)) and bool(torch.isnan(ep.loss[steps]).all())
    assert bool(torch.isfinite(ep.loss[:steps]).all()) and float(ep.loss[:steps, 0].min()) > 0
    for k in ('logits', 'att', 'zsave', 'abar', 'G'):
        assert torch.equal(getattr(ep, k), getattr(st, k).view(shapes[k])), k
    for k, (whole, view) in guards.items():
        _guards_untouched(whole, view.numel())
    assert int(cache.status) == int(status_loop) == 2
    assert int(A.ctr) == int(B.ctr) == (OFFSET + steps if rng_dev else OFFSET)
    # an off-by-one in the learning rate, the dropout offset or the batch would show: the steps differ from one another
    assert not torch.equal(log[0], log[1])


@pytest.mark.parametrize('scores', ['softmax', 'sigmoid'])
@pytest.mark.parametrize('dtype,C', [(torch.float32, 1024), (torch.bfloat16, 512), (F8, 32)], ids=['f32', 'bf16', 'fp8'])
def test_validation_epoch_is_the_loop(gpu, dtype, C, scores):
    T, P, N, K, count, cap = 29, 7, 8, 12, 19, 24
    cache = _cache(dtype, T, P, C, gpu)
    Wa, ba, Wt, bt, _ = _weights(C, K, 1, gpu)
    flags = cof.APA_FLAG_RELU_ATT
    order = cache.order(4, 1).clone()
    order[5] = T + 1
    want_loss = scores == 'softmax'
    steps, last = 3, 3
    # ---- the loop of apa_attn_head_eval_step_cached: two full batches and one of 3 rows
    rows = dict(logits=[], probs=[], pred=[], loss=[])
    cache.status.zero_()
    for s in range(steps):
        b = cache.select(order[s * N:min((s + 1) * N, count)])
        st = cof.HeadEvalStep(b, b, Wa, ba, Wt, bt, flags=flags, scores=scores)      # labels through the index
        st.run()
        for k in ('logits', 'probs', 'pred'):
            rows[k].append(getattr(st, k).clone())
        if want_loss:
            rows['loss'].append(st.loss.clone())
    status_loop = cache.status.clone()
    # ---- the epoch call
    shapes = dict(logits=(cap, K), probs=(cap, K), att=(N, P, 1), zsave=(N, C), abar=(N,))
    guards = {k: _guarded(s, torch.float32, gpu) for k, s in shapes.items()}
    guards['pred'] = _guarded((cap,), torch.int64, gpu)
    if want_loss:
        guards['loss'] = _guarded((steps, 1 + N), torch.float32, gpu)
    outs = {k: v for k, (_, v) in guards.items()}
    outs['logits'].fill_(NAN), outs['probs'].fill_(NAN), outs['pred'].fill_(-5)
    if want_loss:
        outs['loss'].fill_(NAN)
    ep = cof.HeadEvalEpoch(cache, N, Wa, ba, Wt, bt, capacity=cap, flags=flags, scores=scores, want_loss=want_loss,
                           outputs=outs)
    cache.status.zero_()
    assert ep.run(order, count) == steps
    torch.cuda.synchronize()
    for k in ('logits', 'probs', 'pred'):
        got = getattr(ep, k)
        assert torch.equal(got[:count], torch.cat(rows[k])), k
        tail = got[count:]                                                   # rows past `count` are untouched
        assert bool(torch.isnan(tail).all()) if got.dtype.is_floating_point else tail.tolist() == [-5] * (cap - count)
    assert bool(torch.isfinite(ep.probs[:count]).all())
    if want_loss:
        for s in range(steps):
            n = 1 + (last if s == steps - 1 else N)
            assert torch.equal(ep.loss[s, :n], rows['loss'][s]), s
            assert bool(torch.isnan(ep.loss[s, n:]).all())
    for k in ('att', 'zsave', 'abar'):                                       # the last step's, in its 3 rows
        assert torch.equal(getattr(ep, k)[:last], getattr(st, k)), k
    for k, (whole, view) in guards.items():
        _guards_untouched(whole, view.numel())
    assert int(cache.status) == int(status_loop) == 1
    # the scores straight into a meter's rows
    from attentionalpoolingaction_amd import eval_utils
    meter = eval_utils.DeviceEvaluation(cap, K, gpu, multi_label=False)
    dst, _ = meter.reserve(count)
    ep.run(order, count, probs=dst)
    assert torch.equal(meter._scores[:count], torch.cat(rows['probs']))


# ------------------------------------------------------------------------------------------ deploy
def _network(fx, gpu):
    network_fn, cfg = rf.build_head(fx, device=gpu)
    with torch.no_grad():
        for vn, t in rf.module_tf_names(network_fn).items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).reshape(t.shape).to(gpu))
    return network_fn, cfg


def _fixture_cache(fx, T, gpu, dtype=torch.float32):
    """T images made of the fixture's (cycled, each with its own magnitude) and labels inside the head's classes"""
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu)
    n = images.shape[0]
    g = torch.Generator().manual_seed(17)
    mag = (0.5 + torch.rand((T, 1, 1, 1), generator=g)).to(gpu)
    labels = torch.randint(0, int(fx.meta['num_classes']), (T,), generator=g).to(gpu)
    cache = cof.FeatureCache.empty((T,) + tuple(images.shape[1:]), dtype, gpu, labels=labels)
    assert cache.write(0, images[[i % n for i in range(T)]] * mag).tolist() == [0] * T
    return cache


def test_fused_head_step_train_epoch_is_the_deploy_loop(gpu):
    """FusedHeadStep.train_epoch against the same number of `__call__` + `opt.step()` on cache.select(order[s*N:(s+1)*N]):
    the head's state_dict (its step counter included), the accumulators and the losses, bit for bit.  The cfg 002 form
    keeps no operand copy, so its staleness guard watches nothing: the guard is shown on an image attached by hand."""
    from attentionalpoolingaction_amd import config as apa_config, deploy
    T, N, steps = 11, 2, 4
    try:
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz'))
        cache = _fixture_cache(fx, T, gpu)
        order = cache.order(3, 0)[:steps * N]
        lrs = [0.02 * 0.5 ** s for s in range(steps)]
        # ---- the deploy loop
        net_b, cfg_b = _network(fx, gpu)
        net_b.head.seed, net_b.head._step = 99, 5
        fb = deploy.FusedHeadStep(net_b, cfg_b, frozen_features=True)
        ob = fb.make_optimizer(0.02)
        log = []
        for s in range(steps):
            total, _ = fb(cache.select(order[s * N:(s + 1) * N]), None)
            total.backward()
            ob.step(lr=lrs[s])
            log.append(fb._step_obj.loss.clone())
        state_b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in net_b.head.state_dict().items()}
        acc_b, bucket_b = ob.acc.clone(), fb.bucket.flat.clone()
        # ---- one call
        net_a, cfg_a = _network(fx, gpu)
        net_a.head.seed, net_a.head._step = 99, 5
        fa = deploy.FusedHeadStep(net_a, cfg_a, frozen_features=True)
        oa = fa.make_optimizer(0.02)
        out = fa.train_epoch(cache, N, order, lr=lrs)
        assert tuple(out.shape) == (steps, 1 + N) and out.is_cuda and torch.equal(out, torch.stack(log))
        assert net_a.head._step == net_b.head._step == 5 + steps
        state_a = net_a.head.state_dict()
        assert set(state_a) == set(state_b)
        for k, v in state_b.items():
            assert torch.equal(state_a[k], v) if isinstance(v, torch.Tensor) else state_a[k] == v, k
        assert torch.equal(oa.acc, acc_b) and torch.equal(fa.bucket.flat, bucket_b)
        assert float(oa.acc.abs().max()) > 0
        # lr=None: the optimiser's own rate, on the bound epoch call
        bound = fa._epoch
        fa.train_epoch(cache, N, order[:2 * N])
        assert fa._epoch is bound and net_a.head._step == 5 + steps + 2
        # ---- a copy attached to the optimiser: refused by name; written behind its back: StaleOperandError first
        img = torch.zeros((16, 16), dtype=torch.bfloat16, device=gpu)
        m = cof.ApaWeightImage()
        m.dst, m.cols, m.d = img.data_ptr(), 1, 1
        oa.add_image('td_biases', m, refresh=lambda: None, owner=img)
        with pytest.raises(ValueError, match='operand copies'):
            fa.train_epoch(cache, N, order)
        with torch.no_grad():
            net_a.head.td_biases.add_(0.0)
        with pytest.raises(deploy.StaleOperandError):
            fa.train_epoch(cache, N, order)
        assert net_a.head._step == 5 + steps + 2
    finally:
        apa_config.reset_cfg()


def test_fused_head_eval_evaluate_cache_is_the_deploy_loop(gpu):
    from attentionalpoolingaction_amd import config as apa_config, deploy
    T, N = 11, 4
    try:
        fxe = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_eval_c2048.npz'))
        net, cfg = _network(fxe, gpu)
        cache = _fixture_cache(fxe, T, gpu, torch.bfloat16)
        ev = deploy.FusedHeadEval(net, cfg)
        order = cache.order(8, 2)
        want = ev.new_evaluation(T)
        for a in range(0, T, N):
            idx = order[a:a + N]
            scores, _, _ = ev(cache.select(idx))
            want.update(scores, cache.labels[idx.long()])
        meter = ev.evaluate_cache(cache, N, order=order)
        assert len(meter) == T and torch.equal(meter._scores[:T], want._scores[:T])
        assert torch.equal(meter._truth[:T], want._truth[:T])
        ra, rb = meter.result(), want.result()
        assert ra['accuracy'] == rb['accuracy'] and ra['mAP'] == rb['mAP'] and ra['aps'] == rb['aps']
        assert np.array_equal(ra['ap_per_class'], rb['ap_per_class']) and np.array_equal(ra['npos'], rb['npos'])
        # a meter that already holds rows; the default order is the cache's own
        m2 = ev.new_evaluation(2 * T)
        m2.update(want._scores[:3], want._truth[:3])
        assert ev.evaluate_cache(cache, N, meter=m2) is m2 and len(m2) == 3 + T
        plain = ev.new_evaluation(T)
        for a in range(0, T, N):
            idx = torch.arange(a, min(a + N, T), dtype=torch.int32, device=gpu)
            plain.update(ev(cache.select(idx))[0], cache.labels[idx.long()])
        assert torch.equal(m2._scores[3:3 + T], plain._scores[:T]) and torch.equal(m2._truth[3:3 + T], plain._truth[:T])
    finally:
        apa_config.reset_cfg()
