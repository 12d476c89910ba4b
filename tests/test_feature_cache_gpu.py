"""The resident feature cache read by image index, on the GPU.

The oracle of the gathered kernels is the library itself on a gathered copy: only the feature address (FP8: and the
scale) goes through the index, everything else keeps the batch position, so a call on `cache.select(index)` must equal
the same call on `cache.gather(index)` BIT FOR BIT -- every output, every pooling family (asserted from the dispatch
trace), fp32 / bf16 / FP8, identity and ReLU, evaluation and training, both head routes.  Independent of the plain
kernels: one gathered training step per dtype against the float64 error model of tests/test_m1_paths_gpu.py, and
deploy.FusedHeadStep / FusedHeadEval on a CachedBatch against the float64 oracle on the cfg 002 reference fixtures.

Cache: T = 7 images; batches index = [6, 0, 6, 3, 1] (a repeated id, unordered, the cache's last image) and N = 1, whose
blocks hold 4 - 5 pixels; and indices of length 342 and 171 (S = 1 and S = 3: 16 - 33 pixels per block), so that the
long-block loops of the stream / vec / generic kernels run through the index as well."""
import ctypes
import os

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _m1_probe as mp
from tests import _ref_fixture as rf
from tests import test_fp8_features_gpu as f8t
from tests import test_m1_paths_gpu as m1p

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
T = 7
INDEX = [6, 0, 6, 3, 1]
SEED, OFFSET = 1234, 7
KEEP = 0.2                      # the reference's DROPOUT = -1 default (nets_factory.py:143-146)
POOL_STREAM, POOL_VEC, POOL_GENERIC, POOL_FP8 = 1, 2, 3, 4          # M1Pool (csrc/apa_internal.h)
# (family, feature dtype, C): the widths follow from m1s_supported / m1v_supported / m1g_supported (asserted below);
# FP8 with one vector per row and with ragged lanes (1040 / 16 = 65 vectors over 64 lanes)
COMBOS = [(POOL_STREAM, torch.float32, 1024), (POOL_STREAM, torch.bfloat16, 2048),
          (POOL_VEC, torch.float32, 256), (POOL_VEC, torch.bfloat16, 512),
          (POOL_GENERIC, torch.float32, 40), (POOL_GENERIC, torch.bfloat16, 40),
          (POOL_FP8, F8, 32), (POOL_FP8, F8, 1040)]
SIDES = {1: (1, 1), 49: (7, 7), 225: (15, 15)}


def _combo_id(c):
    return '%s_%s_c%d' % ({1: 'stream', 2: 'vec', 3: 'generic', 4: 'fp8'}[c[0]], str(c[1]).split('.')[-1], c[2])


# ------------------------------------------------------------------------------------------ inputs
_CACHES = {}


def _cache(dtype, P, C, dev, labels_K=20):
    """a T-image cache of relu(randn) maps with a per-image magnitude (a wrong image or scale cannot pass), its labels,
    built once per (dtype, P, C) and never written afterwards"""
    key = (dtype, P, C)
    if key not in _CACHES:
        H, W = SIDES.get(P, (P, 1))
        g = torch.Generator().manual_seed(77 + P + C)
        rows = 0.25 + 1.5 * torch.rand((T, H, W, 1), generator=g)
        mag = torch.tensor([1.0, 37.0, 1e-3, 2.0, 0.5, 5.0, 11.0]).view(T, 1, 1, 1)
        img = (torch.relu(torch.randn(T, H, W, C, generator=g)) * rows * mag).to(dev)
        labels = torch.randint(0, labels_K, (T,), generator=g).to(dev)
        cache = cof.FeatureCache.empty((T, H, W, C), dtype, dev, labels=labels)
        st = torch.cat([cache.write(0, img[:4]), cache.write(4, img[4:])])          # (FP8: apa_quantize_features_fp8_at)
        assert st.tolist() == [0] * T
        _CACHES[key] = cache
    return _CACHES[key]


def _params(C, K, act, cache, dev):
    g = torch.Generator().manual_seed(5 + C + K)
    u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
    Wa = u(C, 1) * (4.0 / C)
    if act == 'relu':       # gate both ways around the unit-magnitude image's mean pixel
        f = cache.features
        x0 = (f.dequantize()[0] if cache.fp8 else f[0]).float().cpu().reshape(-1, C)
        ba = -(x0.mean(dim=0) @ Wa[:, 0]).reshape(1)
    else:
        ba = u(1) * 0.1
    return dict(Wa=Wa.to(dev), ba=ba.to(dev), Wt=(u(C, K) / C ** 0.5).to(dev), bt=(u(K) * 0.1).to(dev))


def _flags(act, train):
    return (cof.APA_FLAG_RELU_ATT if act == 'relu' else 0) | (cof.APA_FLAG_TRAIN if train else 0)


def _same(a, b, what):
    for k in b:
        assert a[k] is not None and torch.equal(a[k].reshape(b[k].shape), b[k]), '%s: %s differs' % (what, k)


# ------------------------------------------------------------------------------------------ the four calls
def _separate(X, p, G, flags, keep=KEEP, offset=OFFSET):
    kw = dict(flags=flags, keep_prob=keep, seed=SEED, offset=offset)
    logits, att, zsave, abar, _, ws = cof.attn_pool_fwd(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], **kw)
    dX, dXatt, dWa, dba, dWt, dbt = cof.attn_pool_bwd(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], att, zsave, abar, G,
                                                      workspace=ws, want_dx=False, **kw)
    assert dX is None and dXatt is None
    return dict(logits=logits, att=att, zsave=zsave, abar=abar, dWa=dWa, dba=dba, dWt=dWt, dbt=dbt)


def _train_step(X, p, labels, flags, keep=KEEP, offset=OFFSET, run=True):
    grads = (None, None) + tuple(torch.empty_like(p[k]) for k in ('Wa', 'ba', 'Wt', 'bt'))
    st = cof.HeadTrainStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, grads, flags=flags, keep_prob=keep,
                           seed=SEED, offset=offset)
    st.grads = grads
    if run:
        st.run()
        assert st.frozen_input and st.dX_scratch is None
    return st


def _step_outputs(st):
    return dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, loss=st.loss, G=st.G, dWa=st.grads[2],
                dba=st.grads[3], dWt=st.grads[4], dbt=st.grads[5])


def _eval_step(X, p, labels, flags, scores='softmax'):
    st = cof.HeadEvalStep(X, X, p['Wa'], p['ba'], p['Wt'], p['bt'], labels, flags=flags, scores=scores)
    st.run()
    out = dict(logits=st.logits, att=st.att, zsave=st.zsave, abar=st.abar, probs=st.probs, pred=st.pred)
    if st.loss is not None:
        out['loss'] = st.loss
    return out


# ------------------------------------------------------------------------------------------ the dispatch trace
_PROBE = None


def _probe():
    global _PROBE
    if _PROBE is None:
        lib = mp.load_m1_probe()
        for probe, prod in (('apa_probe_m1_fwd_cached', 'apa_attn_pool_fwd_cached'),
                            ('apa_probe_m1_bwd_cached', 'apa_attn_pool_bwd_cached')):
            fn = getattr(lib, probe)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p] + list(cof._SIGNATURES[prod][1])
        _PROBE = lib
    return _PROBE


def _traced_families(batch, p, G, flags, ref):
    """(pool_fwd, pool_bwd) of the gathered calls as the library's own trace records them; the traced calls' outputs
    are those of the untraced ones"""
    lib = _probe()
    N, C, K = batch.shape[0], batch.shape[-1], p['Wt'].shape[1]
    P = batch.numel() // (N * C)
    dev = batch.device
    need = cof.attn_pool_workspace_bytes(N, P, C, C, K, 1, flags)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = {k: torch.empty_like(v) for k, v in ref.items()}
    desc = batch.descriptor()
    tf, tb = mp.M1Trace(), mp.M1Trace()
    X = batch.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.apa_probe_m1_fwd_cached(ctypes.addressof(tf), ctypes.addressof(desc), None, X, X, p['Wa'].data_ptr(),
                                     p['ba'].data_ptr(), p['Wt'].data_ptr(), p['bt'].data_ptr(), out['logits'].data_ptr(),
                                     out['att'].data_ptr(), out['zsave'].data_ptr(), out['abar'].data_ptr(), None,
                                     ws.data_ptr(), need, N, P, C, C, K, 1, flags, KEEP, SEED, OFFSET,
                                     cof._feat_dtype(batch), st)
    assert rc == 0, lib.apa_last_error()
    rc = lib.apa_probe_m1_bwd_cached(ctypes.addressof(tb), ctypes.addressof(desc), None, X, X, p['Wa'].data_ptr(),
                                     p['ba'].data_ptr(), p['Wt'].data_ptr(), p['bt'].data_ptr(), out['att'].data_ptr(),
                                     out['zsave'].data_ptr(), out['abar'].data_ptr(), G.data_ptr(), None, None,
                                     out['dWa'].data_ptr(), out['dba'].data_ptr(), out['dWt'].data_ptr(),
                                     out['dbt'].data_ptr(), ws.data_ptr(), need, N, P, C, C, K, 1,
                                     flags | cof.APA_FLAG_FROZEN_INPUT, KEEP, SEED, OFFSET, cof._feat_dtype(batch), st)
    assert rc == 0, lib.apa_last_error()
    _same(out, ref, 'traced')
    return tf.pool_fwd, tb.pool_bwd


# ------------------------------------------------------------------------------------------ 1 + 2: families, bit identity
@pytest.mark.parametrize('P', [1, 49, 225])
@pytest.mark.parametrize('combo', COMBOS, ids=_combo_id)
def test_gathered_calls_equal_the_calls_on_a_gathered_copy(gpu, combo, P):
    family, dtype, C = combo
    if family != POOL_FP8:      # the width reaches the family it is meant to reach, by the library's own predicates
        sup = mp.support(5, C, 20, cof.APA_DTYPE_F32 if dtype == torch.float32 else cof.APA_DTYPE_BF16)
        first = POOL_STREAM if sup & mp.SUP_STREAM else POOL_VEC if sup & mp.SUP_VEC else POOL_GENERIC
        assert first == family and sup & mp.SUP_GENERIC
    cache = _cache(dtype, P, C, gpu)
    before = (cache.features.buffer if cache.fp8 else cache.features).clone()
    traced = set()
    for index in (INDEX, [6]):                  # N = 5, N = 1
        batch, copy = cache.select(index), cache.gather(index)
        N = len(index)
        lab_batch = cache.labels[torch.tensor(index, device=gpu)].contiguous()
        for act in ('id', 'relu'):
            for train in (False, True):
                flags = _flags(act, train)
                for K in (20, 393):             # the two head routes behind the pass
                    p = _params(C, K, act, cache, gpu)
                    what = '%s N=%d %s %s K=%d' % (_combo_id(combo), N, act, 'train' if train else 'eval', K)
                    g = torch.Generator().manual_seed(N + K)
                    G = ((torch.rand(N, K, generator=g) * 1.25 - 0.25) / N).to(gpu)
                    ref = _separate(copy, p, G, flags)
                    _same(_separate(batch, p, G, flags), ref, what + ' fwd/bwd')
                    if (act, train) not in traced and N == 5 and K == 20:
                        traced.add((act, train))
                        assert _traced_families(batch, p, G, flags, ref) == (family, family), what
                    if train:
                        labels = lab_batch % K
                        want = _step_outputs(_train_step(copy, p, labels, flags))
                        _same(_step_outputs(_train_step(batch, p, labels, flags)), want, what + ' step, batch labels')
                        if K == 20:             # (the cache's labels were drawn below 20)
                            _same(_step_outputs(_train_step(batch, p, None, flags)), want, what + ' step, cached labels')
                    else:
                        labels = lab_batch % K
                        want = _eval_step(copy, p, labels, flags)
                        _same(_eval_step(batch, p, labels, flags), want, what + ' eval, batch labels')
                        if K == 20:
                            _same(_eval_step(batch, p, None, flags), want, what + ' eval, cached labels')
                        else:
                            free = _eval_step(cof.FeatureCache(cache.features).select(index), p, None, flags)
                            _same(free, _eval_step(copy, p, None, flags), what + ' eval, no labels')
    # sigmoid scores ride behind the same pass
    p = _params(C, 20, 'id', cache, gpu)
    _same(_eval_step(cache.select(INDEX), p, None, 0, scores='sigmoid'),
          _eval_step(cache.gather(INDEX), p, None, 0, scores='sigmoid'), 'sigmoid scores')
    # 4: a cache is read-only -- its bytes are what they were, after every training step above
    torch.cuda.synchronize()
    assert torch.equal(cache.features.buffer if cache.fp8 else cache.features, before)
    assert int(cache.status) == 0


# ------------------------------------------------------------------------------------------ long blocks through the index
LONG = [(342, 33), (171, 49)]       # (N, P): m1_plan's S = 1 (33 pixels per block) and S = 3 (blocks of 16 / 16 / 17)


def _long_index(N):
    """N ids into the T-image cache: INDEX first (a repeated id, unordered, the cache's last image), then seeded draws"""
    g = torch.Generator().manual_seed(31 + N)
    idx = torch.randint(0, T, (N,), generator=g)
    idx[:len(INDEX)] = torch.tensor(INDEX)
    assert set(idx.tolist()) == set(range(T))
    return idx.tolist()


@pytest.mark.parametrize('N,P', LONG, ids=['n342_p33_S1', 'n171_p49_S3'])
@pytest.mark.parametrize('combo', [c for c in COMBOS if c[0] != POOL_FP8], ids=_combo_id)
def test_gathered_long_blocks_equal_the_calls_on_a_gathered_copy(gpu, combo, N, P):
    """The batches above give blocks of 4 - 5 pixels, a wave one or two of them; here a block holds 16 - 33, so the
    pixel loops of the stream / vec / generic kernels run their steady state with the image behind the index (the FP8
    family: tests/test_fp8_instances_gpu.py).  Bit comparison only -- the plain kernels have their float64 tests at
    long blocks in tests/test_m1_paths_gpu.py."""
    family, dtype, C = combo
    K = 20
    S, ppb = mp.plan(N, P, C, C, K)[:2]
    assert (S, ppb) == {33: (1, 33), 49: (3, 17)}[P]
    cache = _cache(dtype, P, C, gpu)
    before = cache.features.clone()
    index = _long_index(N)
    batch, copy = cache.select(index), cache.gather(index)
    G = ((torch.rand(N, K, generator=torch.Generator().manual_seed(N + K)) * 1.25 - 0.25) / N).to(gpu)
    for act in ('id', 'relu'):
        p = _params(C, K, act, cache, gpu)
        for train in (False, True):
            flags = _flags(act, train)
            what = '%s N=%d P=%d %s %s' % (_combo_id(combo), N, P, act, 'train' if train else 'eval')
            ref = _separate(copy, p, G, flags)
            _same(_separate(batch, p, G, flags), ref, what)
            assert _traced_families(batch, p, G, flags, ref) == (family, family), what
    torch.cuda.synchronize()
    assert torch.equal(cache.features, before) and int(cache.status) == 0


def test_device_counter_advances_once_per_step_in_both(gpu):
    cache = _cache(torch.bfloat16, 49, 2048, gpu)
    p = _params(2048, 20, 'relu', cache, gpu)
    flags = _flags('relu', True)
    ctr_a = torch.tensor([OFFSET], dtype=torch.int64, device=gpu)
    ctr_b = ctr_a.clone()
    a = _train_step(cache.select(INDEX), p, None, flags, offset=ctr_a, run=False)
    lab = cache.labels[torch.tensor(INDEX, device=gpu)].contiguous()
    b = _train_step(cache.gather(INDEX), p, lab, flags, offset=ctr_b, run=False)
    first = None
    for i in range(3):
        a.run()
        b.run()
        assert int(ctr_a) == int(ctr_b) == OFFSET + i + 1
        _same(_step_outputs(a), _step_outputs(b), 'device counter, step %d' % i)
        if i == 0:
            first = a.loss.clone()
            # the counter is the host offset of the plain form
            _same(_step_outputs(a), _step_outputs(_train_step(cache.select(INDEX), p, None, flags)), 'offset by value')
    assert not torch.equal(first, a.loss)                   # a fresh mask per step


def test_rebind_index_swaps_the_batch(gpu):
    cache = _cache(F8, 49, 1040, gpu)
    p = _params(1040, 20, 'id', cache, gpu)
    flags = _flags('id', True)
    st = _train_step(cache.select(INDEX), p, None, flags)
    first = {k: v.clone() for k, v in _step_outputs(st).items()}
    other = [2, 5, 4, 4, 0]
    st.rebind(index=torch.tensor(other, dtype=torch.int32, device=gpu))
    st.run()
    lab = cache.labels[torch.tensor(other, device=gpu)].contiguous()
    _same(_step_outputs(st), _step_outputs(_train_step(cache.gather(other), p, lab, flags)), 'rebound')
    st.rebind(index=INDEX)
    st.run()
    _same(_step_outputs(st), first, 'bound back')
    with pytest.raises(cof.ApaError):
        st.rebind(index=[1, 2])                             # another batch size is another step
    with pytest.raises(cof.ApaError):
        st.rebind(X=cache.gather(INDEX))
    with pytest.raises(cof.ApaError, match='same object'):
        cof.HeadEvalStep(cache.select(INDEX), cache.select(INDEX), p['Wa'], p['ba'], p['Wt'], p['bt'])
    # an epoch's views feed the bound step without a copy
    batches = list(cache.epoch(5, seed=3))
    assert len(batches) == 1 and batches[0].is_cuda and batches[0].dtype == torch.int32
    st.rebind(index=batches[0])
    assert st._index.data_ptr() == batches[0].data_ptr()
    st.run()
    lab = cache.labels[batches[0].long()].contiguous()
    _same(_step_outputs(st), _step_outputs(_train_step(cache.gather(batches[0]), p, lab, flags)), 'epoch batch')


# ------------------------------------------------------------------------------------------ 3: the identity index
@pytest.mark.parametrize('dtype,C', [(torch.float32, 1024), (torch.bfloat16, 512), (F8, 1040)],
                         ids=['f32', 'bf16', 'fp8'])
def test_identity_index_equals_the_plain_call(gpu, dtype, C):
    cache = _cache(dtype, 49, C, gpu)
    batch = cache.select(torch.arange(T))
    plain = cache.features.flat() if cache.fp8 else cache.features
    p = _params(C, 20, 'relu', cache, gpu)
    flags = _flags('relu', True)
    G = (torch.rand(T, 20, generator=torch.Generator().manual_seed(1)) / T).to(gpu)
    _same(_separate(batch, p, G, flags), _separate(plain, p, G, flags), 'fwd/bwd')
    _same(_step_outputs(_train_step(batch, p, None, flags)), _step_outputs(_train_step(plain, p, cache.labels, flags)),
          'step')
    _same(_eval_step(batch, p, None, 0), _eval_step(plain, p, cache.labels, 0), 'eval')


# ------------------------------------------------------------------------------------------ 5: out-of-range ids
@pytest.mark.parametrize('dtype,C', [(torch.float32, 256), (torch.bfloat16, 2048), (F8, 32)], ids=['f32', 'bf16', 'fp8'])
def test_out_of_range_ids_are_clamped_and_counted(gpu, dtype, C):
    cache = _cache(dtype, 49, C, gpu)
    p = _params(C, 20, 'id', cache, gpu)
    flags = _flags('id', True)
    G = (torch.rand(3, 20, generator=torch.Generator().manual_seed(2)) / 3).to(gpu)
    try:
        cache.status.zero_()
        bad, good = cache.select([7, -1, 2]), cache.select([6, 0, 2])
        want = _separate(good, p, G, flags)
        assert int(cache.status) == 0
        _same(_separate(bad, p, G, flags), want, 'fwd/bwd')
        assert int(cache.status) == 2                       # the forward pass counts, the backward pass does not
        want = _step_outputs(_train_step(good, p, None, flags))
        assert int(cache.status) == 2
        _same(_step_outputs(_train_step(bad, p, None, flags)), want, 'step')       # (labels through the clamped id too)
        assert int(cache.status) == 4                       # once per step
        _same(_eval_step(bad, p, None, 0), _eval_step(good, p, None, 0), 'eval')
        assert int(cache.status) == 6
    finally:
        cache.status.zero_()


# ------------------------------------------------------------------------------------------ 6: float64, deploy
OR_KEEP = 0.5       # the keep probability of tests/test_fp8_features_gpu.py, whose tolerances these are


@pytest.mark.parametrize('dtype,C', [(torch.float32, 1024), (torch.bfloat16, 2048), (F8, 2048)], ids=['f32', 'bf16', 'fp8'])
def test_gathered_training_step_against_float64(gpu, dtype, C):
    """the error model of tests/_m1_probe.py on the gathered (FP8: dequantised) inputs, as tests/test_fp8_features_gpu.py
    holds the FP8 arm to it: fp32 accumulation of exactly representable inputs"""
    P, K, N = 49, 393, len(INDEX)
    cache = _cache(dtype, P, C, gpu)
    p = _params(C, K, 'relu', cache, gpu)
    idx = torch.tensor(INDEX, device=gpu)
    vals = cache.features.dequantize() if cache.fp8 else cache.features
    X64 = vals[idx].double().reshape(N, P, C)
    labels = (cache.labels[idx] * 19 % K).contiguous()
    c = dict(name='cached', N=N, P=P, C=C, K=K, J=0, Ca=None, act='relu', train=True, keep=OR_KEEP, rank1=False,
             relu_in=False, dt=cof._feat_dtype(cache.select(INDEX)), entry='step')
    st = _train_step(cache.select(INDEX), p, labels, _flags('relu', True), keep=OR_KEEP)
    got = _step_outputs(st)
    inp = dict(X=X64, Xatt=X64, Wa=p['Wa'].reshape(C), ba=p['ba'], Wt=p['Wt'], bt=p['bt'], G=got['G'], labels=labels,
               Xext=None)
    mask = cof.dropout_mask((N * P * C,), OR_KEEP, SEED, OFFSET)
    f8t._check_against_float64(c, inp, got, mask, cancels=True)
    f8t._check_loss(c, got, inp)


def _network(fx, gpu):
    network_fn, cfg = rf.build_head(fx, device=gpu)
    with torch.no_grad():
        for vn, t in rf.module_tf_names(network_fn).items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).reshape(t.shape).to(gpu))
    return network_fn, cfg


def _fixture_cache(fx, dtype, gpu, labels=True):
    """the fixture's images in REVERSED order behind one more image, so that index = [n-1, ..., 0] is the fixture's
    batch; (cache, index, the fixture with the cache's own values for images and no L2 term)"""
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu)
    n = images.shape[0]
    lab = torch.from_numpy(fx.arrays['in/labels_action']).to(gpu).reshape(n).long() if labels else None
    order = list(range(n - 1, -1, -1))
    cache = cof.FeatureCache.empty((n + 1,) + tuple(images.shape[1:]), dtype, gpu,
                                   labels=None if lab is None else torch.cat([lab[order], lab[:1]]).contiguous())
    assert cache.write(0, images[order]).tolist() == [0] * n
    assert cache.write(n, images[:1] * 3.0).tolist() == [0]
    vals = cache.features.dequantize() if cache.fp8 else cache.features
    arrays = {k: v for k, v in fx.arrays.items() if not k.startswith(('inseed/', 'inpatch/', 'insum/'))}
    arrays['in/images'] = vals[order].float().cpu().numpy()
    return cache, order, rf.HeadFixture(arrays=arrays, meta=dict(fx.meta, weight_decay=0.0))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, F8], ids=['f32', 'bf16', 'fp8'])
def test_deploy_fused_step_and_eval_on_a_cached_batch(gpu, dtype):
    from attentionalpoolingaction_amd import config as apa_config, deploy
    rel, tol = f8t._rel, f8t.FP32_VS_F64
    try:
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz'))
        network_fn, cfg = _network(fx, gpu)
        head = network_fn.head
        head.seed, head._step = int(fx.meta['libmask'][0]), int(fx.meta['libmask'][1])
        cache, order, fxq = _fixture_cache(fx, dtype, gpu)
        before = (cache.features.buffer if cache.fp8 else cache.features).clone()
        fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
        total, ep = fused(cache.select(order), None)        # labels through the index
        total.backward()
        st = fused._step_obj
        assert st._dX_buf is None and st.frozen_input and st.dX_scratch is None         # no conv5 gradient exists
        ref = rf.run_oracle(fxq)
        assert rel(total.item(), ref['out/losses'].sum()) < tol
        assert rel(ep['Logits'].cpu(), ref['out/logits']) < tol
        want = np.concatenate([ref['grad/var/' + fused.tf_names[n]].reshape(-1) if n in fused._written
                               else np.zeros(fused.bucket.views[n].numel()) for n in fused.bucket.names])
        assert rel(fused.bucket.flat.cpu(), want) < tol
        for n in fused._written:
            assert float(fused.bucket.views[n].abs().max()) > 0, n
        # the bound step is kept across batches of one cache: only the index is re-bound
        first = ep['Logits'].clone()
        head._step = int(fx.meta['libmask'][1])
        fused(cache.select([0] * len(order)), None)
        assert fused._step_obj is st and len(fused._steps) == 1 and not torch.equal(st.logits, first)
        head._step = int(fx.meta['libmask'][1])
        _, ep2 = fused(cache.select(order), None)
        assert fused._step_obj is st and torch.equal(ep2['Logits'], first)
        # per-batch labels bind a step of their own and give the same step
        head._step = int(fx.meta['libmask'][1])
        lab = torch.from_numpy(fx.arrays['in/labels_action']).to(gpu).reshape(-1).long()
        _, ep3 = fused(cache.select(order), lab)
        assert len(fused._steps) == 2 and torch.equal(ep3['Logits'], first)
        assert torch.equal(cache.features.buffer if cache.fp8 else cache.features, before)
        # evaluation
        fxe = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_eval_c2048.npz'))
        net_e, cfg_e = _network(fxe, gpu)
        cache_e, order_e, fxeq = _fixture_cache(fxe, dtype, gpu, labels=False)
        ev = deploy.FusedHeadEval(net_e, cfg_e)
        scores, pred, epe = ev(cache_e.select(order_e))
        refe = rf.run_oracle(fxeq)
        assert rel(epe['Logits'].cpu(), refe['out/logits']) < tol
        want = torch.softmax(torch.from_numpy(refe['out/logits']), dim=1)
        assert rel(scores.cpu(), want.numpy()) < tol
        assert torch.equal(pred.cpu(), want.argmax(dim=1))
        step_e = ev.step
        ev(cache_e.select([0] * len(order_e)))
        assert ev.step is step_e and len(ev._steps) == 1
    finally:
        apa_config.reset_cfg()


# ------------------------------------------------------------------------------------------ 7: quantise into place
@pytest.mark.parametrize('src', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_quantize_at_in_two_chunks_is_quantize_of_the_whole(gpu, src):
    g = torch.Generator().manual_seed(9)
    X = (torch.randn(T, 3, 5, 48, generator=g) * torch.tensor([1.0, 37.0, 1e-3, 2.0, 0.5, 5.0, 11.0]).view(T, 1, 1, 1))
    X[1] = 0.0
    X[5, 2, 4, 47] = float('nan')               # a non-finite image: reported, zero codes and scale
    X = X.to(src).to(gpu)
    whole, status = cof.quantize_features(X)
    cache = cof.FeatureCache.empty(X.shape, F8, gpu)
    cache.features.buffer.fill_(0xA5)           # (the padding between codes and scales is nobody's)
    s1 = cache.write(3, X[3:])
    s0 = cache.write(0, X[:3])
    f = cache.features
    assert torch.equal(f.codes.view(torch.uint8), whole.codes.view(torch.uint8))
    assert torch.equal(f.scale.view(torch.int32), whole.scale.view(torch.int32))
    assert torch.equal(torch.cat([s0, s1]), status) and status.tolist() == [0, 0, 0, 0, 0, 1, 0]
    off = cof.fp8_scale_offset(T, 15, 48)
    assert bool((f.buffer[T * 15 * 48:off] == 0xA5).all())
    # and the CPU rule
    cpu = cof.FeatureCache.empty(X.shape, F8, 'cpu')
    cpu.write(0, X.cpu())
    assert torch.equal(cpu.features.codes.view(torch.uint8), f.codes.view(torch.uint8).cpu())
    assert torch.equal(cpu.features.scale.view(torch.int32), f.scale.view(torch.int32).cpu())
