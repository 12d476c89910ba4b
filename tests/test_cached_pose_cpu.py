"""The pose-regularised head (cfg 003) from the resident feature cache, without a GPU: the companion header and its
python mirror agree with the library's exports, apa.h and cof._SIGNATURES still agree with each other, every refusal of
the two cached steps fires in the promised order with its sentence (dummy pointers: an admitted call stops at the plain
step's workspace check, in front of the first launch), the existing *_cached entry points answer what they answered,
`cached_pose_served` restates the C rule, and the deploy layer admits exactly the new case."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from attentionalpoolingaction_amd.custom_ops import pose_cache
from tests.test_cached_perclass_cpu import _Calls, _desc, _ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'apa_pose_cache.h')
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
FAKE = 0x10000
FROZEN, TRAIN = cof.APA_FLAG_FROZEN_INPUT, cof.APA_FLAG_TRAIN
BF16, F32, FP8 = 1, 0, 2
TRAIN_FN, EVAL_FN = 'apa_pose_attn_train_step_cached', 'apa_pose_attn_eval_step_cached'


# ------------------------------------------------------------------------------------------ ABI
def test_header_module_and_library_name_the_same_symbols():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r'^int\s+(apa_\w+)\s*\(', text, flags=re.M)))
    assert declared == pose_cache.exported_symbols() == sorted([TRAIN_FN, EVAL_FN])
    lib = pose_cache.load_library()
    for name in declared:
        assert getattr(lib, name).argtypes == pose_cache._SIGNATURES[name][1]
    out = subprocess.run(['nm', '-D', '--defined-only', cof.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(declared) <= exported
    # the companion header adds nothing to apa.h's table, and that table still mirrors apa.h
    assert not set(declared) & set(cof._SIGNATURES)
    apa_h = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    code = re.sub(r'/\*.*?\*/', '', apa_h, flags=re.S)
    in_apa_h = set(re.findall(r'\b(apa_\w+)\s*\(', code))
    assert in_apa_h == set(cof._SIGNATURES), in_apa_h ^ set(cof._SIGNATURES)
    assert not set(declared) & in_apa_h


# ------------------------------------------------------------------------------------------ refusals, in order
def _train_io(dX=None, X=FAKE, ws=0):
    io = cof.ApaPoseAttnStepIO()
    for name, _ in io._fields_:
        if name not in ('action_wt', 'pose_wt', 'grad_scale', 'ws_pool_bytes', 'ws_pose_bytes'):
            setattr(io, name, FAKE)
    io.X, io.dX, io.W1_bf16, io.W2T_bf16 = X, dX, None, None
    io.action_wt = io.pose_wt = io.grad_scale = 1.0
    io.ws_pool_bytes = io.ws_pose_bytes = ws
    return io


def _eval_io(X=FAKE):
    io = cof.ApaPoseAttnEvalIO()
    for name, _ in io._fields_:
        if name not in ('ws_bytes', 'route'):
            setattr(io, name, FAKE)
    io.X, io.W1_bf16, io.labels, io.loss, io.Pl, io.ws_bytes = X, None, None, None, None, 0
    return io


class _Pose(object):
    def __init__(self):
        self.lib = pose_cache.load_library()

    def train(self, cache, io='default', dtype=BF16, N=4, P=8, C=512, Cp=256, J=16, K=5, flags=FROZEN, **io_kw):
        io = _train_io(**io_kw) if io == 'default' else io
        rc = self.lib.apa_pose_attn_train_step_cached(_ptr(cache), _ptr(io), N, P, C, Cp, J, K, flags, 0.5, 0, 0, dtype,
                                                      None)
        return rc, self.lib.apa_last_error().decode()

    def ev(self, cache, io='default', dtype=BF16, N=4, P=8, C=512, Cp=256, J=16, K=5, flags=0, **io_kw):
        io_kw.pop('dX', None)
        io_kw.pop('ws', None)
        io = _eval_io(**io_kw) if io == 'default' else io
        rc = self.lib.apa_pose_attn_eval_step_cached(_ptr(cache), _ptr(io), N, P, C, Cp, J, K, flags, dtype, None)
        return rc, self.lib.apa_last_error().decode()


def test_an_admitted_call_stops_at_the_plain_steps_workspace_check():
    p = _Pose()
    for kw in (dict(), dict(N=32, P=196, C=2048, Cp=768, K=393), dict(N=8, P=25, C=384, Cp=320, J=7, K=3),
               dict(flags=FROZEN | TRAIN | cof.APA_FLAG_RELU_ATT)):
        rc, err = p.train(_desc(), **kw)
        assert rc == WORKSPACE and err.startswith(('apa_pose_head_fwd:', TRAIN_FN + ':')), (kw, rc, err)
    for kw in (dict(), dict(N=2, P=225, C=2048, Cp=768, K=393), dict(N=3, P=9), dict(flags=cof.APA_FLAG_RELU_ATT)):
        rc, err = p.ev(_desc(labels_cached=1, status=FAKE), **kw)
        assert rc == WORKSPACE and err.startswith(EVAL_FN + ': workspace too small'), (kw, rc, err)


def test_refusals_fire_in_the_promised_order_each_with_its_sentence():
    p = _Pose()
    both = ((p.train, TRAIN_FN), (p.ev, EVAL_FN))
    for call, fn in both:
        # 1. the descriptor, dX and the frozen flag: APA_ERR_INVALID_ARG (in front of every later defect)
        later = dict(dtype=F32, X=FAKE + 8, flags=cof.APA_FLAG_SOFTMAX_ATT)
        assert call(_desc(), io=None) == (INVALID, fn + ': null io')
        assert call(None, **later) == (INVALID, fn + ': null apa_feature_cache / index pointer')
        assert call(_desc(index=None), **later) == (INVALID, fn + ': null apa_feature_cache / index pointer')
        rc, err = call(_desc(index=FAKE + 2), **later)
        assert rc == INVALID and '4-byte aligned' in err
        rc, err = call(_desc(T=0), **later)
        assert rc == INVALID and err == fn + ': apa_feature_cache.cache_images=0: a cache holds at least one image'
    rc, err = p.train(_desc(), dX=FAKE, dtype=F32)
    assert rc == INVALID and err == TRAIN_FN + ': a feature cache has no gradient: io->dX must be NULL'
    rc, err = p.train(_desc(), flags=TRAIN, dtype=F32)
    assert rc == INVALID and err == TRAIN_FN + ': a feature cache is frozen: a training step needs APA_FLAG_FROZEN_INPUT'
    for call, fn in both:
        base = FROZEN if call == p.train else 0
        # 2. the dtype, in front of alignment, products and softmax
        for dtype in (F32, FP8):
            rc, err = call(_desc(), dtype=dtype, X=FAKE + 8, flags=base | cof.APA_FLAG_SOFTMAX_ATT)
            assert rc == UNSUPPORTED and err.startswith('%s: dtype %d: the pose-regularised head is served from a bf16 '
                                                        'cache' % (fn, dtype)), err
        # 3. a misaligned cache base, C % 8 != 0
        for kw in (dict(X=FAKE + 8), dict(C=516)):
            rc, err = call(_desc(), flags=base | cof.APA_FLAG_SOFTMAX_ATT, **kw)
            assert rc == UNSUPPORTED and 'the cache must be 16-byte aligned with C a multiple of 8' in err, (kw, err)
        # 5. softmax attention (a served shape)
        rc, err = call(_desc(), flags=base | cof.APA_FLAG_SOFTMAX_ATT)
        assert rc == UNSUPPORTED and err.startswith(fn + ': a feature cache does not serve APA_FLAG_SOFTMAX_ATT'), err
        # 6. then the plain step's refusals, with its text
        rc, err = call(_desc(), J=0)
        assert rc == INVALID and err == fn + ': J=0'
        rc, err = call(_desc(), flags=base | cof.APA_FLAG_RELU_INPUT)
        assert rc == UNSUPPORTED and 'APA_FLAG_RELU_INPUT / APA_FLAG_RNG_EXTERNAL' in err
        rc, err = call(_desc(), N=0)
        assert rc == INVALID and 'non-positive dimension' in err
    # 4. a product outside the admission predicate: the dW1 contraction N * P = 27 is not whole 8-element vectors, the
    # dispatcher would send it to the fp32-unpacking kernel -- in front of softmax; evaluation has no such product
    rc, err = p.train(_desc(), N=3, P=9, flags=FROZEN | cof.APA_FLAG_SOFTMAX_ATT)
    assert rc == UNSUPPORTED and 'a feature cache behind operand A needs a product of the bf16 MFMA path' in err, err
    rc, err = p.train(_desc(), Cp=260)
    assert rc == UNSUPPORTED and 'a feature cache behind operand A' in err, err
    rc, err = p.ev(_desc(), N=3, P=9)
    assert rc == WORKSPACE, err


def test_every_existing_cached_entry_point_still_refuses_a_separate_attention_input():
    c = _Calls()
    other = FAKE + 0x1000
    for call in c.all():
        rc, err = call(_desc(), M=1, K=8, xatt=other, flags=FROZEN)
        assert rc == UNSUPPORTED and 'a separate attention input (Xatt != X)' in err and 'feature cache' in err, (
            call.__name__, rc, err)


# ------------------------------------------------------------------------------------------ python
def _batch(N, P, C, dtype=torch.bfloat16, T=7):
    cache = cof.FeatureCache(torch.zeros(T, P, 1, C, dtype=dtype), torch.zeros(T, dtype=torch.int64))
    return cache.select([i % T for i in range(N)])


@pytest.mark.parametrize('N,P,C,Cp,train,served', [
    (32, 196, 2048, 768, True, True), (32, 196, 2048, 768, False, True),
    (8, 9, 512, 256, True, True),         # N * P = 72: whole vectors, not whole 64-row tiles
    (3, 9, 512, 256, True, False),        # N * P = 27: the dW1 contraction is refused ...
    (3, 9, 512, 256, False, True),        # ... and evaluation has no such product
    (2, 225, 2048, 768, False, True), (2, 225, 2048, 768, True, False),
    (8, 25, 384, 320, True, True), (8, 25, 388, 320, True, False), (8, 25, 384, 324, True, False),
    (1, 4, 512, 256, False, False),       # fewer than 8 batch rows
])
def test_cached_pose_served_restates_the_c_rule(N, P, C, Cp, train, served):
    batch = _batch(N, P, C)
    assert pose_cache.cached_pose_served(batch, Cp, 16, 5, train=train) is served
    # ... as the library answers on dummy pointers (aligned fake cache base)
    p = _Pose()
    call = p.train if train else p.ev
    rc, err = call(_desc(), N=N, P=P, C=C, Cp=Cp)
    assert (rc == WORKSPACE) is served, (rc, err)


def test_cached_pose_served_is_about_flat_bf16_batches():
    assert not pose_cache.cached_pose_served(_batch(4, 8, 512, torch.float32), 256, 16, 5)
    assert not pose_cache.cached_pose_served(torch.zeros(4, 8, 512, dtype=torch.bfloat16), 256, 16, 5)
    cache = cof.FeatureCache(torch.zeros(8, 8, 1, 512, dtype=torch.bfloat16))
    assert not pose_cache.cached_pose_served(cof.CachedClips(cache, 2, 2), 256, 16, 5)
    fp8 = cof.FeatureCache.empty((8, 8, 1, 512), torch.float8_e4m3fn, 'cpu')
    assert not pose_cache.cached_pose_served(fp8.select([0, 1, 2, 3]), 256, 16, 5)


def test_python_steps_refuse_what_they_cannot_bind():
    batch = _batch(4, 8, 512)
    with pytest.raises(cof.ApaError, match='a flat CachedBatch expected'):
        pose_cache.PoseAttnTrainStepCached(torch.zeros(4, 8, 512), None, None, None, None, [None] * 9)
    with pytest.raises(cof.ApaError, match='grads\\[0\\] = None'):
        pose_cache.PoseAttnTrainStepCached(batch, None, None, None, None, [torch.zeros(1)] * 9)
    with pytest.raises(cof.ApaError, match='a flat CachedBatch expected'):
        pose_cache.PoseAttnEvalStepCached(cof.CachedClips(batch.cache, 2, 2), None)
    with pytest.raises(cof.ApaError, match='float32 \\[T,...,J\\]'):
        pose_cache.PoseLabelTable(torch.zeros(7, 3, 3, 16), torch.zeros(7, 15, dtype=torch.uint8))
    table = pose_cache.PoseLabelTable(torch.arange(7 * 2 * 16, dtype=torch.float32).view(7, 2, 1, 16),
                                      torch.arange(7 * 16).view(7, 16) % 2 == 0)
    lab, val = table.new_batch(3)
    table.gather([5, -3, 12], lab, val)           # (CPU tensors: the table itself has no device code)
    assert torch.equal(lab, table.pose_labels[[5, 0, 6]]) and torch.equal(val, table.pose_valid[[5, 0, 6]])


# ------------------------------------------------------------------------------------------ deploy
def test_deploy_admits_the_bf16_flat_batch_and_keeps_every_other_sentence():
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    old = 'attention from pose_pre_logits (the cfg 003 form)'
    try:
        fx3 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_train.npz'))
        net3, cfg3 = rf.build_head(fx3, device='cpu', in_channels=2048)
        fxe = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_eval.npz'))
        net3e, cfg3e = rf.build_head(fxe, device='cpu', in_channels=2048)
        reason = deploy.FusedHeadStep.cache_unsupported_reason
        for net in (net3, net3e):
            assert deploy.FusedHeadStep.fp8_unsupported_reason(net.head, net) == old
            assert reason(net.head, net, _batch(2, 4, 2048)) == ''
            assert reason(net.head, net, _batch(2, 4, 2048, torch.float32)) == old
            fp8 = cof.FeatureCache.empty((4, 2, 2, 2048), torch.float8_e4m3fn, 'cpu')
            assert reason(net.head, net, fp8.select([1, 0])) == old
            assert reason(net.head, net, cof.Fp8Features.empty((2, 2, 2, 2048), 'cpu')) == old
            bf = cof.FeatureCache(torch.zeros(8, 2, 2, 2048, dtype=torch.bfloat16))
            assert reason(net.head, net, cof.CachedClips(bf, 2, 2)) == old
        # a training head needs N * P in whole 8-element vectors (the dW1 contraction); evaluation does not
        assert reason(net3.head, net3, _batch(2, 9, 2048)) == old
        assert reason(net3e.head, net3e, _batch(2, 9, 2048)) == ''
        # the four epoch forms keep refusing the head, bf16 cache or not
        cache = cof.FeatureCache(torch.zeros(8, 2, 2, 2048, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.int64))
        order = torch.arange(8, dtype=torch.int32)
        f3 = deploy.FusedHeadStep(net3, cfg3, frozen_features=True)
        f3.make_optimizer(0.01)
        with pytest.raises(ValueError, match='train_epoch: an epoch call is not served with ' + re.escape(old)):
            f3.train_epoch(cache, 4, order)
        with pytest.raises(ValueError, match='a clip epoch call is not served with ' + re.escape(old)):
            f3.train_video_epoch(cache, 2, 2, order)
        e3 = deploy.FusedHeadEval(net3e, cfg3e)
        with pytest.raises(ValueError, match='evaluate_cache: a cache pass is not served with ' + re.escape(old)):
            e3.evaluate_cache(cache, 4)
        with pytest.raises(ValueError, match='a video pass is not served with ' + re.escape(old)):
            e3.evaluate_videos(cache, 2, 2)
        # an admitted batch on a CPU cache gets as far as the binding: no CPU fallback
        with pytest.raises(cof.ApaError, match='GPU memory'):
            e3(_batch(2, 4, 2048))
    finally:
        apa_config.reset_cfg()


def test_deploy_refuses_the_sigmoid_losses_before_anything_is_bound():
    """a cfg 003 head under LOSS_FN_ACTION 'multi-label*': the cached steps have no sigmoid form, so both deploy objects
    refuse the batch by name -- nothing is bound, no softmax score stands in for a sigmoid one"""
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from tests import _ref_fixture as rf
    word = 'under a sigmoid action loss'
    try:
        for loss in ('multi-label', 'multi-label-2'):
            for name, evaluation in (('ref_head_cfg003_train.npz', False), ('ref_head_cfg003_eval.npz', True)):
                fx = rf.HeadFixture(os.path.join(rf.GOLD, name))
                fx.meta = dict(fx.meta, train_cfg=dict(fx.meta['train_cfg'], LOSS_FN_ACTION=loss))
                net, cfg = rf.build_head(fx, device='cpu', in_channels=2048)
                reason = deploy.FusedHeadStep.cache_unsupported_reason
                batch = _batch(2, 4, 2048)
                assert reason(net.head, net, batch) == ''                       # (the head and the batch alone qualify)
                assert word in reason(net.head, net, batch, multi_label=True)
                # a batch that is refused anyway keeps its old sentence
                assert reason(net.head, net, _batch(2, 4, 2048, torch.float32), multi_label=True) == \
                    'attention from pose_pre_logits (the cfg 003 form)'
                if evaluation:
                    ev = deploy.FusedHeadEval(net, cfg)
                    assert ev.multi_label
                    with pytest.raises(ValueError, match='a CachedBatch is not served with .*' + word):
                        ev(batch)
                    assert len(ev._steps) == 0
                else:
                    fused = deploy.FusedHeadStep(net, cfg, frozen_features=True)
                    with pytest.raises(ValueError, match='a CachedBatch is not served with .*' + word):
                        fused(batch, torch.zeros(2, net.head.num_classes), torch.zeros(2, 2, 2, 16),
                              torch.ones(2, 16, dtype=torch.uint8))
                    assert len(fused._steps) == 0
    finally:
        apa_config.reset_cfg()
