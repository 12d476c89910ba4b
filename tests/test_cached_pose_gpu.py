"""The pose-regularised head (cfg 003) trained and evaluated from the resident feature cache
(include/apa_pose_cache.h, custom_ops/pose_cache.py) against the library itself on `cache.gather(index)`: every output
of the cached step is torch.equal to the plain frozen step's, with equal PoseTrace and M1Trace.  (The plain step's
kernels are held to float64 by tests/test_pose_paths_gpu.py and tests/test_pose_attn_eval_gpu.py.)

Caches hold T = 7 images, each with its own magnitude, between NaN rows; the index repeats, is non-monotone and leaves
images unused.

Two shapes of the training list differ from a naive reading of it, by the library's own admission rule (a mapped product
the dispatcher would send to the fp32-unpacking kernel is refused, and dW1 = X^T . dPpre contracts over N * P rows, which
that rule wants in whole 8-element vectors): 3 x 9 (27 rows), 4 x 33 (132 rows) and 2 x 25 (50 rows) are EVALUATED from
the cache and their training step is asserted to be refused before anything is queued; training runs at 8 x 9 (72 rows:
not whole 64-row tiles, the register-staged bf16 kernel), 8 x 33 (264 rows) and 8 x 25 (200 rows) on the same routes.
"""
import ctypes

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from attentionalpoolingaction_amd.custom_ops import pose_cache
from tests import _graph_replay as gr
from tests import _m1_probe as m1p
from tests import _pose_probe as pp

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
T = 7
PATTERN = (5, 1, 5, 0, 6, 1, 3, 3, 0, 6, 5, 1)      # images 2 and 4 are never used
TRAIN_OUT = ('Ppre', 'Pl', 'att', 'logits', 'zsave', 'abar', 'loss_action', 'loss_pose', 'G', 'dPl', 'dZ')
EVAL_OUT = ('att', 'logits', 'zsave', 'abar', 'probs', 'pred')
GRADS = ('dW1', 'db1', 'dW2', 'db2', 'dWa', 'dba', 'dWt', 'dbt')


def _index(n, clamped=False):
    idx = [PATTERN[i % len(PATTERN)] for i in range(n)]
    if clamped:
        idx[1], idx[n - 1] = -3, T + 5
    return idx


class World(object):
    """A guarded cache, its label tables and one set of head parameters."""

    def __init__(self, P, C, Cp, J, K, seed, n_cache=T):
        dev = torch.device('cuda')
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        self.dims = (P, C, Cp, J, K)
        self.T = n_cache
        rn = lambda *s, sc=1.0: torch.randn(*s, generator=g, device=dev) * sc
        # NaN rows in front of and behind the cache: nothing outside it may be addressed
        base = torch.full(((n_cache + 2) * P * C,), float('nan'), dtype=BF, device=dev)
        feats = base[P * C:(n_cache + 1) * P * C].view(n_cache, P, 1, C)
        scale = (1.0 + 0.5 * torch.arange(n_cache, device=dev, dtype=torch.float32)).view(-1, 1, 1, 1)
        feats.copy_((rn(n_cache, P, 1, C).abs() * 0.5 + rn(n_cache, P, 1, C, sc=0.25)) * scale)
        self.base, self.base_bits = base, base.view(torch.int16).clone()
        self.labels = torch.randint(0, K, (n_cache,), generator=g, device=dev)
        self.cache = cof.FeatureCache(feats, self.labels)
        self.table = pose_cache.PoseLabelTable(rn(n_cache, P, 1, J),
                                               torch.rand(n_cache, J, generator=g, device=dev) < 0.7)
        self.params = (rn(C, Cp, sc=C ** -0.5), rn(Cp, sc=0.1), rn(Cp, J, sc=Cp ** -0.5), rn(J, sc=0.1),
                       rn(Cp, 1, sc=Cp ** -0.5), rn(1, sc=0.1) + 0.2, rn(C, K, sc=C ** -0.5), rn(K, sc=0.1))

    def grads(self):
        return [None] + [torch.full_like(p, 7.0) for p in self.params]

    def batch_rows(self, index):
        idx = torch.tensor(index, device='cuda').clamp(0, self.T - 1)
        return self.table.pose_labels[idx].clone(), self.table.pose_valid[idx].clone(), self.labels[idx].clone(), idx

    def cache_untouched(self):
        assert torch.equal(self.base.view(torch.int16), self.base_bits)


def _probe():
    lib = pp.load_pose_probe()
    m1p.load_m1_probe()
    tr = lib.apa_probe_pose_attn_train_step_cached
    tr.restype = ctypes.c_int
    tr.argtypes = [ctypes.c_void_p] * 3 + list(pose_cache._SIGNATURES['apa_pose_attn_train_step_cached'][1][1:])
    ev = lib.apa_probe_pose_attn_eval_step_cached
    ev.restype = ctypes.c_int
    ev.argtypes = [ctypes.c_void_p] * 3 + list(pose_cache._SIGNATURES['apa_pose_attn_eval_step_cached'][1][1:])
    return lib


def _run_traced(step, train):
    """the bound step's own arguments through the probe library's traced wrapper (cache == NULL: the plain step)"""
    lib = _probe()
    pt, mt = pp.PoseTrace(), m1p.M1Trace()
    fc = ctypes.addressof(step._fc) if hasattr(step, '_fc') else None
    fn = lib.apa_probe_pose_attn_train_step_cached if train else lib.apa_probe_pose_attn_eval_step_cached
    args = step._args[1:] if (not train and fc is not None) else step._args
    rc = fn(ctypes.addressof(pt), ctypes.addressof(mt), fc, *args, cof._stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.apa_probe_last_error()
    return pt.as_dict(), mt.as_dict()


def _train_pair(w, N, index, *, flags=0, keep=1.0, offset=0, labels_cached=False, shadows=False, seed=11):
    P, C, Cp, J, K = w.dims
    pl, pv, lab, idx = w.batch_rows(index)
    X = w.cache.features.view(w.T, P, C)[idx].contiguous()
    kw = dict(flags=flags, keep_prob=keep, seed=seed, offset=offset, action_wt=0.75, pose_wt=1.5, grad_scale=2.0)
    if shadows:
        kw.update(w1_bf16=w.params[0].to(BF), w2t_bf16=cof.pose_w2t_image(w.params[2]))
    ga, gb = w.grads(), w.grads()
    plain = cof.PoseAttnTrainStep(X, w.params, lab, pl.view(N, P, J), pv, ga, **kw)
    cached = pose_cache.PoseAttnTrainStepCached(w.cache.select(index), w.params, None if labels_cached else lab,
                                                pl.view(N, P, J), pv, gb, **kw)
    plain.test_grads, cached.test_grads = dict(zip(GRADS, ga[1:])), dict(zip(GRADS, gb[1:]))
    return plain, cached


def _grads_of(step):
    return step.test_grads


def _assert_equal_steps(plain, cached, names, what):
    for n in names:
        a, b = getattr(plain, n), getattr(cached, n)
        assert torch.isfinite(a.float()).all(), '%s: plain %s is not finite' % (what, n)
        assert torch.equal(a, b), '%s: %s differs (%d elements)' % (what, n, int((a != b).sum()))


def _assert_equal_grads(plain, cached, what):
    ga, gb = _grads_of(plain), _grads_of(cached)
    for n in GRADS:
        assert torch.isfinite(ga[n]).all() and torch.equal(ga[n], gb[n]), '%s: %s differs' % (what, n)


# --------------------------------------------------------------------------------------------- training
TRAIN_SHAPES = [
    # name, N, P, C, Cp, J, K, flags, keep, expected pooling family, fast route
    ('vec_8x9x512_fast', 8, 9, 512, 256, 16, 5, 0, 1.0, 'vec', True),
    ('stream_8x33x2048_relu_dropout', 8, 33, 2048, 768, 16, 7, cof.APA_FLAG_RELU_ATT | cof.APA_FLAG_TRAIN, 0.5,
     'stream', True),
    ('generic_8x25x384_composed', 8, 25, 384, 320, 7, 3, cof.APA_FLAG_TRAIN, 0.5, 'generic', False),
]


@pytest.mark.parametrize('case', TRAIN_SHAPES, ids=[c[0] for c in TRAIN_SHAPES])
def test_cached_train_step_equals_the_plain_frozen_step(case):
    name, N, P, C, Cp, J, K, flags, keep, family, fast = case
    w = World(P, C, Cp, J, K, seed=len(name))
    index = _index(N)
    counter = torch.zeros(1, dtype=torch.int64, device='cuda') if keep < 1.0 else None
    counter2 = None if counter is None else counter.clone()
    plain, _ = _train_pair(w, N, index, flags=flags, keep=keep, offset=counter if counter is not None else 0)
    _, cached = _train_pair(w, N, index, flags=flags, keep=keep, offset=counter2 if counter2 is not None else 0)
    for step_no in range(2 if keep < 1.0 else 1):      # two steps with the device-side counter
        plain.run()
        cached.run()
        torch.cuda.synchronize()
        _assert_equal_steps(plain, cached, TRAIN_OUT, '%s step %d' % (name, step_no))
        _assert_equal_grads(plain, cached, '%s step %d' % (name, step_no))
        if counter is not None:
            assert int(counter) == int(counter2) == step_no + 1
    # (a cache has no dX: the entry point refuses a non-NULL one -- tests/test_cached_pose_cpu.py -- and the bound step
    # passes NULL, so what there is to guard is the cache itself and the NaN rows around it)
    assert cached._io.dX is None
    w.cache_untouched()
    before = {n: getattr(cached, n).clone() for n in TRAIN_OUT}
    # the routes and kernel families, plain and cached
    tp, mp = _run_traced(plain, True)
    tc, mc = _run_traced(cached, True)
    assert tp == tc and mp == mc, (tp, tc, mp, mc)
    assert (tc['pl_fused'] == 1) is fast, tc
    assert mc['fused'] == 0 and mc['pool_fwd'] == mc['pool_bwd'] == family, mc
    # two runs give the same bits
    if counter2 is not None:
        counter2.fill_(0)
        cached.run()
        cached.run()
    else:
        cached.run()
    torch.cuda.synchronize()
    for n in TRAIN_OUT:
        assert torch.equal(getattr(cached, n), before[n]), n


@pytest.mark.parametrize('N,P,C,Cp,J,K', [(3, 9, 512, 256, 16, 5), (4, 33, 2048, 768, 16, 7), (2, 25, 384, 320, 7, 3)])
def test_training_rows_outside_the_admission_rule_are_refused_before_anything_is_queued(N, P, C, Cp, J, K):
    w = World(P, C, Cp, J, K, seed=5)
    _, cached = _train_pair(w, N, _index(N))
    for n in TRAIN_OUT:
        getattr(cached, n).fill_(-5.0)
    with pytest.raises(cof.ApaError, match='a feature cache behind operand A needs a product of the bf16 MFMA path'):
        cached.run()
    torch.cuda.synchronize()
    for n in TRAIN_OUT:
        assert bool((getattr(cached, n) == -5.0).all()), n


def test_labels_through_the_index_status_counts_once_and_clamped_ids():
    N, P, C, Cp, J, K = 8, 9, 512, 256, 16, 5
    w = World(P, C, Cp, J, K, seed=21)
    index = _index(N, clamped=True)
    plain, cached = _train_pair(w, N, index, labels_cached=True)
    w.cache.status.zero_()
    plain.run()
    cached.run()
    torch.cuda.synchronize()
    assert int(w.cache.status) == 2                    # two out-of-range entries, counted once per training step
    _assert_equal_steps(plain, cached, TRAIN_OUT, 'labels_cached, clamped ids')
    _assert_equal_grads(plain, cached, 'labels_cached, clamped ids')
    w.cache_untouched()
    cached.run()
    torch.cuda.synchronize()
    assert int(w.cache.status) == 4
    # rebind swaps the index pointer and nothing else
    other = [3, 0, 6, 6, 1, 5, 0, 3]
    pl, pv, lab, idx = w.batch_rows(other)
    cached.rebind(index=other, pose_labels=pl.view(N, P, J), pose_valid=pv)
    plain.rebind(X=w.cache.features.view(T, P, C)[idx].contiguous(), labels=lab, pose_labels=pl.view(N, P, J),
                 pose_valid=pv)
    plain.run()
    cached.run()
    torch.cuda.synchronize()
    _assert_equal_steps(plain, cached, TRAIN_OUT, 'after rebind')
    _assert_equal_grads(plain, cached, 'after rebind')


def test_shipped_shape_two_steps_with_the_optimisers_operand_copies():
    N, P, C, Cp, J, K = 32, 196, 2048, 768, 16, 393
    w = World(P, C, Cp, J, K, seed=3, n_cache=40)
    g = torch.Generator(device='cuda')
    g.manual_seed(9)
    runs = []
    for kind in ('plain', 'cached'):
        params = [p.clone() for p in w.params]
        total = sum(p.numel() for p in params)
        grad_flat, acc_flat = torch.zeros(total, device='cuda'), torch.zeros(total, device='cuda')
        views, o = [], 0
        for p in params:
            views.append(grad_flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        shadow, image = params[0].to(BF), cof.pose_w2t_image(params[2])
        opt = cof.BoundMomentumSGD(params, [1e-4] * 8, grad_flat, acc_flat,
                                   shadows=[shadow] + [None] * 7, images=[(2, cof.pose_w2t_image_map(image, params[2]))])
        outs = []
        step = None
        for s in range(2):
            index = torch.randint(0, 40, (N,), generator=torch.Generator().manual_seed(s)).tolist()
            pl, pv, lab, idx = w.batch_rows(index)
            kw = dict(flags=cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT, keep_prob=0.2, seed=4, offset=s,
                      w1_bf16=shadow, w2t_bf16=image)
            if kind == 'plain':
                X = w.cache.features.view(40, P, C)[idx].contiguous()
                step = cof.PoseAttnTrainStep(X, params, lab, pl.view(N, P, J), pv, [None] + views, **kw)
            elif step is None:
                step = pose_cache.PoseAttnTrainStepCached(w.cache.select(index), params, lab, pl.view(N, P, J), pv,
                                                          [None] + views, **kw)
            else:
                step.rebind(index=index, labels=lab, pose_labels=pl.view(N, P, J), pose_valid=pv, offset=s)
            step.run()
            outs.append({n: getattr(step, n).clone() for n in TRAIN_OUT})
            outs[-1]['grad_flat'] = grad_flat.clone()
            opt.run(0.01, 0.9, 0.5)
            outs[-1]['w1_shadow'], outs[-1]['w2t'] = shadow.clone(), image.clone()
            torch.cuda.synchronize()
        runs.append(outs)
    for s in range(2):
        for n, a in runs[0][s].items():
            assert torch.isfinite(a.float()).all() and torch.equal(a, runs[1][s][n]), 'step %d: %s differs' % (s, n)
    w.cache_untouched()


# --------------------------------------------------------------------------------------------- evaluation
EVAL_SHAPES = [
    # name, N, P, C, Cp, J, K, flags, want_pose_logits, route
    ('vec_3x9x512', 3, 9, 512, 256, 16, 5, 0, False, 1),
    ('vec_3x9x512_pl', 3, 9, 512, 256, 16, 5, 0, True, 0),
    ('stream_4x33x2048_relu', 4, 33, 2048, 768, 16, 7, cof.APA_FLAG_RELU_ATT, False, 1),
    ('generic_2x25x384_composed', 2, 25, 384, 320, 7, 3, 0, False, 0),
    ('native_2x225x2048_fused', 2, 225, 2048, 768, 16, 393, 0, False, 1),
    ('native_2x225x2048_pose_logits', 2, 225, 2048, 768, 16, 393, 0, True, 0),
]


@pytest.mark.parametrize('case', EVAL_SHAPES, ids=[c[0] for c in EVAL_SHAPES])
def test_cached_eval_step_equals_the_plain_step(case):
    name, N, P, C, Cp, J, K, flags, want_pl, route = case
    w = World(P, C, Cp, J, K, seed=len(name))
    index = _index(N, clamped=name.startswith('stream'))
    _, _, lab, idx = w.batch_rows(index)
    X = w.cache.features.view(T, P, C)[idx].contiguous()
    w1b = w.params[0].to(BF)
    plain = cof.PoseAttnEvalStep(X, w.params, lab, flags=flags, w1_bf16=w1b, want_pose_logits=want_pl)
    cached = pose_cache.PoseAttnEvalStepCached(w.cache.select(index), w.params, 'cache', flags=flags, w1_bf16=w1b,
                                               want_pose_logits=want_pl)
    w.cache.status.zero_()
    plain.run()
    cached.run()
    torch.cuda.synchronize()
    assert plain.route == cached.route == route, (plain.route, cached.route)
    _assert_equal_steps(plain, cached, EVAL_OUT + ('loss',) + (('Pl',) if want_pl else ()), name)
    assert int(w.cache.status) == (2 if name.startswith('stream') else 0)
    w.cache_untouched()
    tp, mp = _run_traced(plain, False)
    tc, mc = _run_traced(cached, False)
    assert tp == tc and mp == mc, (tp, tc, mp, mc)
    # the label-free form, and a second run with the same bits
    free = pose_cache.PoseAttnEvalStepCached(w.cache.select(index), w.params, None, flags=flags, w1_bf16=w1b,
                                             want_pose_logits=want_pl)
    free.run()
    torch.cuda.synchronize()
    for n in ('att', 'logits', 'probs', 'pred'):
        assert torch.equal(getattr(free, n), getattr(cached, n)), n


# --------------------------------------------------------------------------------------------- hipGraph
def _graph_rounds(N):
    return [{'index': torch.tensor(ix, dtype=torch.int32, device='cuda')}
            for ix in (_index(N), [6, 6, 0, 3, 1, 5, 0, 3][:N], [1, 3, 5, 0, 6, 5, 1, 0][:N])]


def test_train_step_cached_replays_from_a_captured_graph():
    N, P, C, Cp, J, K = 8, 9, 512, 256, 16, 5

    def make():
        w = World(P, C, Cp, J, K, seed=8)
        index = torch.tensor(_index(N), dtype=torch.int32, device='cuda')
        pl, pv, lab, _ = w.batch_rows(_index(N))
        counter = torch.zeros(1, dtype=torch.int64, device='cuda')
        grads = w.grads()
        step = pose_cache.PoseAttnTrainStepCached(w.cache.select(index), w.params, 'cache', pl.view(N, P, J), pv, grads,
                                                  flags=cof.APA_FLAG_TRAIN, keep_prob=0.5, seed=3, offset=counter)
        state = {n: getattr(step, n) for n in TRAIN_OUT}
        state.update(zip(GRADS, grads[1:]))
        state.update(counter=counter, status=w.cache.status)
        case = gr.Case(step.run, {'index': step._index}, state, outputs=TRAIN_OUT + GRADS, main='logits')
        case.keep = (w, step)
        return case

    gr.replay_equals_eager('apa_pose_attn_train_step_cached', make, _graph_rounds(N))


def test_eval_step_cached_replays_from_a_captured_graph():
    N, P, C, Cp, J, K = 4, 33, 2048, 768, 16, 7

    def make():
        w = World(P, C, Cp, J, K, seed=8)
        index = torch.tensor(_index(N), dtype=torch.int32, device='cuda')
        step = pose_cache.PoseAttnEvalStepCached(w.cache.select(index), w.params, 'cache', w1_bf16=w.params[0].to(BF))
        state = {n: getattr(step, n) for n in EVAL_OUT + ('loss',)}
        state.update(status=w.cache.status)
        case = gr.Case(step.run, {'index': step._index}, state, outputs=EVAL_OUT + ('loss',), main='logits')
        case.keep = (w, step)
        return case

    gr.replay_equals_eager('apa_pose_attn_eval_step_cached', make, _graph_rounds(N))


# --------------------------------------------------------------------------------------------- deploy
SLOTS = [5, 1]          # where the fixture's two images live in the cache of T = 7; the index is non-monotone


def _fixture(name):
    import os
    from tests import _ref_fixture as rf
    fx = rf.HeadFixture(os.path.join(rf.GOLD, name))
    a = fx.arrays
    feats = torch.from_numpy(a['in/images']).cuda().to(BF)
    cache_feats = torch.zeros((T,) + tuple(feats.shape[1:]), dtype=BF, device='cuda')
    cache_feats[SLOTS] = feats
    return (rf, fx, cof.FeatureCache(cache_feats), torch.from_numpy(a['in/labels_action']).cuda(),
            torch.from_numpy(a['in/labels_pose']).cuda(), torch.from_numpy(a['in/labels_pose_valid']).cuda())


@pytest.mark.parametrize('labels_from', ['table', 'tensors'])
def test_deploy_fused_head_step_on_the_reference_fixture(labels_from):
    from attentionalpoolingaction_amd import config as apa_config, deploy
    try:
        results = []
        rf, fx, cache, lab, lp, pv = _fixture('ref_head_cfg003_train.npz')
        net, cfg = rf.build_head(fx, device='cuda')
        fused = deploy.FusedHeadStep(net, cfg, frozen_features=True)
        assert deploy.FusedHeadStep.cache_unsupported_reason(net.head, net, cache.select(SLOTS)) == ''
        for kind in ('gathered', 'cached'):
            net.head.seed, net.head._step = 17, 3          # the same dropout mask in both runs
            fused.bucket.flat.zero_()
            if kind == 'gathered':
                total, ep = fused(cache.gather(SLOTS), lab, lp, pv)
            elif labels_from == 'table':
                t_lp = torch.zeros((T,) + tuple(lp.shape[1:]), device='cuda')
                t_pv = torch.zeros((T, pv.shape[1]), dtype=torch.bool, device='cuda')
                t_lp[SLOTS], t_pv[SLOTS] = lp, pv
                total, ep = fused(cache.select(SLOTS), lab, pose_cache.PoseLabelTable(t_lp, t_pv))
                assert isinstance(fused._step_obj, pose_cache.PoseAttnTrainStepCached)
            else:
                total, ep = fused(cache.select(SLOTS), lab, lp, pv)
                assert isinstance(fused._step_obj, pose_cache.PoseAttnTrainStepCached)
            total.backward()
            torch.cuda.synchronize()
            results.append((total.detach().clone(), {k: v.clone() for k, v in ep.items() if torch.is_tensor(v)},
                            fused.bucket.flat.clone()))
            if kind == 'cached':                                # a second batch re-binds the kept step
                st = fused._step_obj
                fused(cache.select(SLOTS[::-1]), lab.flip(0), lp.flip(0).contiguous(), pv.flip(0).contiguous())
                assert fused._step_obj is st and len(fused._steps) == 2      # (the gathered tensor's step and this one)
        (ta, ea, ba), (tb, eb, bb) = results
        assert torch.isfinite(ta) and torch.equal(ta, tb)
        assert set(ea) == set(eb)
        for k in ea:
            assert torch.equal(ea[k], eb[k]), k
        assert float(ba.abs().max()) > 0 and torch.equal(ba, bb)
    finally:
        apa_config.reset_cfg()


def test_deploy_fused_head_eval_on_the_reference_fixture():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    try:
        rf, fx, cache, lab, lp, pv = _fixture('ref_head_cfg003_eval.npz')
        net, cfg = rf.build_head(fx, device='cuda')
        ev = deploy.FusedHeadEval(net, cfg)
        for want_pl in (False, True):
            sa, pa, ea = ev(cache.gather(SLOTS), want_pose_logits=want_pl)
            sa, pa, ea = sa.clone(), pa.clone(), {k: v.clone() for k, v in ea.items()}
            sb, pb, eb = ev(cache.select(SLOTS), want_pose_logits=want_pl)
            assert isinstance(ev.step, pose_cache.PoseAttnEvalStepCached)
            torch.cuda.synchronize()
            assert torch.equal(sa, sb) and torch.equal(pa, pb) and set(ea) == set(eb)
            for k in ea:
                assert torch.equal(ea[k], eb[k]), k
    finally:
        apa_config.reset_cfg()
