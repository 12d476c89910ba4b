"""deploy.HeadSweep on the GPU: train_epoch == the loop over MultiHeadTrainStep + MultiHeadSGD, evaluate_cache == the loop
over MultiHeadEvalStep, bit for bit; each head's meter against FusedHeadEval.evaluate_cache on that head alone, the
scores inside the sum of the two routes' float64 bounds (tests/_multihead_reference.py, from the inputs alone), the mAP
equal under labels whose every compared pair of scores lies further apart than the bounds (chosen in float64, asserted),
the accuracy apart by no more than the share of images whose best two classes the bounds do not separate."""
import os

import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy
from attentionalpoolingaction_amd.custom_ops import multihead as mh
from tests import _m1_probe as mp
from tests import _multihead_reference as mr
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests.test_epoch_call_gpu import _fixture_cache, _network

pytestmark = pytest.mark.gpu

TRAIN_FX = os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz')
EVAL_FX = os.path.join(rf.GOLD, 'ref_head_cfg002_eval_c2048.npz')
H = 3


def _heads(path, gpu):
    """H heads with the fixture's weights, each scaled differently"""
    fx = rf.HeadFixture(path)
    fns, cfg = [], None
    for i in range(H):
        fn, cfg = _network(fx, gpu)
        with torch.no_grad():
            for n in deploy.HeadSweep.NAMES:
                getattr(fn.head, n).mul_(1.0 + 0.25 * i)
        fn.head.seed, fn.head._step = 99, 5
        fns.append(fn)
    return fx, fns, cfg


def _seeded_cache(fx, T, gpu, dtype, seed):
    """tests/test_epoch_call_gpu.py _fixture_cache with evenly spaced magnitudes -- the cycled copies of one fixture
    image differ by 3 / T and more, which keeps their scores apart -- and labels drawn from `seed`"""
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu)
    n = images.shape[0]
    g = torch.Generator().manual_seed(seed)
    mag = (0.5 + torch.arange(T, dtype=torch.float32) / T).view(T, 1, 1, 1).to(gpu)
    labels = torch.randint(0, int(fx.meta['num_classes']), (T,), generator=g).to(gpu)
    cache = cof.FeatureCache.empty((T,) + tuple(images.shape[1:]), dtype, gpu, labels=labels)
    assert cache.write(0, images[[i % n for i in range(T)]] * mag).tolist() == [0] * T
    return cache


def _score_bounds(cache, order, sweep, relu):
    """float64 scores [H,T,K] of the heads on cache[order] and their bounds from the inputs alone (every stage's error
    carried through: tests/_multihead_reference.py); no relu gate may lie within its bound of zero (asserted)"""
    T, K, C = int(order.numel()), sweep.K, sweep.C
    P = cache.features[0].numel() // C
    c = mr.case('sweep', sweep.H, T, P, C, K, bf16=True, relu=relu)
    Xb = cache.features[order.long()].reshape(T, P, C).double()
    fref, amb = mr.forward_bnd(c, Xb, sweep.Wa, sweep.ba, None)
    assert amb is None or int(amb.sum()) == 0
    lg = mr.logits_bnd(c, fref['zsave'], fref['abar'], sweep.Wt, sweep.bt)
    p = torch.softmax(lg.ref, dim=-1)
    return p, p * (2 * lg.err.amax(dim=-1, keepdim=True) + mp.C_ACC * (K + 16) * mp.EPS32)


def _decided_labels(p, bound):
    """For every image the first class in which its score lies further from EVERY other image's score than twice the sum
    of the two bounds, in every head: with these labels each comparison average precision makes -- a positive image
    against a negative one of the same class -- comes out the same on any two routes that stay inside their bounds
    (the order among positives does not enter an AP).  Chosen in float64 from the inputs; asserted to exist."""
    H, T, K = p.shape
    diff = (p[:, :, None, :] - p[:, None, :, :]).abs()                      # [H, i, j, K]
    need = 2 * (bound[:, :, None, :] + bound[:, None, :, :])
    apart = (diff > need) | torch.eye(T, dtype=torch.bool, device=p.device)[None, :, :, None]
    good = apart.all(dim=2).all(dim=0)                                      # [i, K]
    assert bool(good.any(dim=1).all()), 'an image has no class that separates it from the others beyond the bounds'
    return good.int().argmax(dim=1)                                         # (0 / 1 entries: the first class)


def _undecided_top(p, bound):
    """per head, the number of images whose best class is NOT separated from the second by more than twice the sum of
    the two bounds: two routes inside their bounds may predict differently for these images alone"""
    top = p.topk(2, dim=-1)
    tb = bound.gather(2, top.indices)
    return (top.values[..., 0] - top.values[..., 1] <= 2 * (tb[..., 0] + tb[..., 1])).sum(dim=1)


def test_train_epoch_is_the_loop_of_steps_and_updates(gpu):
    T, N, steps = 11, 2, 3
    lrs, wds = [0.02, 0.01, 0.005], [1e-4, 0.0, 1e-3]
    try:
        fx, fns_a, cfg = _heads(TRAIN_FX, gpu)
        cache = _fixture_cache(fx, T, gpu)
        order = cache.order(3, 0)[:steps * N]
        a = deploy.HeadSweep(fns_a, cfg, lrs, wds)
        log = a.train_epoch(cache, N, order)
        torch.cuda.synchronize()
        assert tuple(log.shape) == (steps, H, 1 + N) and all(fn.head._step == 5 + steps for fn in fns_a)
        # ---- the loop
        _, fns_b, cfg_b = _heads(TRAIN_FX, gpu)
        b = deploy.HeadSweep(fns_b, cfg_b, lrs, wds)
        h0 = fns_b[0].head
        step = mh.MultiHeadTrainStep(cache.select(order[:N]), b.Wa, b.ba, b.Wt, b.bt, 'cache', relu_att=h0.relu_att,
                                     keep_prob=h0.keep_prob, seed=99, offset=5,
                                     loss_wt=float(cfg_b.TRAIN.LOSS_FN_ACTION_WT))
        acc = torch.zeros_like(step.grad_flat)
        mom = float(cfg_b.TRAIN.MOMENTUM) if cfg_b.TRAIN.OPTIMIZER == 'momentum' else 0.0
        sgd = mh.MultiHeadSGD([b.Wa, b.ba, b.Wt, b.bt], [wds, 0.0, wds, 0.0], step.grad_flat, acc, lrs, mom)
        for s in range(steps):
            step.rebind(index=order[s * N:(s + 1) * N], offset=5 + s)
            step.run()
            sgd.run()
            assert torch.equal(step.loss, log[s]), s
        torch.cuda.synchronize()
        for x, y in zip(a.stacked, b.stacked):
            assert torch.equal(x, y)
        assert torch.equal(a.acc, acc) and float(acc.abs().max()) > 0
        for fa, fb in zip(fns_a, fns_b):                # the heads see their rows
            assert torch.equal(fa.head.td_weights, fb.head.td_weights)
        assert not torch.equal(fns_a[0].head.td_weights, fns_a[1].head.td_weights)
    finally:
        apa_config.reset_cfg()


def test_evaluate_cache_is_the_loop_and_agrees_with_each_head_alone(gpu):
    T, N = 11, 4
    try:
        fx, fns, cfg = _heads(EVAL_FX, gpu)
        sweep = deploy.HeadSweep(fns, cfg, [0.1] * H)
        relu = bool(fns[0].head.relu_att)
        cache = _seeded_cache(fx, T, gpu, torch.bfloat16, 17)
        order = cache.order(8, 2)
        with torch.no_grad():
            p, bound = _score_bounds(cache, order, sweep, relu)
            # labels under which every comparison of an average precision is decided beyond the bounds (asserted)
            cache.labels[order.long()] = _decided_labels(p, bound)
            undecided = _undecided_top(p, bound)
        meters = sweep.evaluate_cache(cache, N, order=order)
        torch.cuda.synchronize()
        assert len(meters) == H + 1
        K = sweep.K
        # ---- the loop over MultiHeadEvalStep
        for s in range(0, T, N):
            idx = order[s:s + N]
            st = mh.MultiHeadEvalStep(cache.select(idx), sweep.Wa, sweep.ba, sweep.Wt, sweep.bt,
                                      relu_att=fns[0].head.relu_att)
            st.run()
            torch.cuda.synchronize()
            for h in range(H):
                assert torch.equal(meters[h]._scores[s:s + idx.numel()], st.probs[h]), (s, h)
            assert torch.equal(meters[H]._scores[s:s + idx.numel()], st.fused_probs), s
        mp.check(meters[H]._scores[:T], mr.fused_bnd(torch.stack([m._scores[:T] for m in meters[:H]])), 'fused scores')
        # ---- each head alone: the scores inside the two routes' bounds, from the inputs; the metrics equal
        results = [m.result() for m in meters]
        for h in range(H):
            alone = deploy.FusedHeadEval(fns[h], cfg).evaluate_cache(cache, N, order=order)
            a, m = alone._scores[:T].double(), meters[h]._scores[:T].double()
            assert torch.equal(alone._truth[:T], meters[h]._truth[:T])
            for got in (a, m):
                assert bool(((got - p[h]).abs() <= bound[h]).all()), h
            assert bool(((a - m).abs() <= 2 * bound[h]).all()), h
            ra = alone.result()
            assert ra['mAP'] == results[h]['mAP'], h          # every AP comparison is decided: the same ranking
            # the predictions can differ on the undecided images alone
            assert abs(ra['accuracy'] - results[h]['accuracy']) <= float(undecided[h]) / T + 1e-12, h
        best = sweep.best('mAP')
        assert results[best]['mAP'] == max(r['mAP'] for r in results[:H])
    finally:
        apa_config.reset_cfg()
