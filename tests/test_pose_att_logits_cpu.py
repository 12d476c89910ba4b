"""The pose-heatmap attention head (cfg.NET.USE_POSE_ATTENTION_LOGITS, nets_factory.py:162-189) without a GPU: routing
in get_network_fn (the reference's if/elif precedence, the refused head branches), the TF variable names and shapes
against the reference-executed fixtures tests/golden/ref_pal_*.npz (make_pose_att_reference.py), the DIMS
normalisation, the float64 restatement (_pal_reference) against every fixture, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import torch

import _pal_reference as pal
import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy, nets_factory
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof

SMALL = pal.small_fixture_paths()
ALL = pal.fixture_paths()
PA = 'USE_POSE_ATTENTION_LOGITS'
P = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
REFUSED = ['USE_POSE_LOGITS_DIRECTLY', 'USE_POSE_LOGITS_DIRECTLY_v2', 'USE_COMPACT_BILINEAR_POOLING']


def _cfg(net=None, train=None):
    apa_config.reset_cfg()
    return apa_config.cfg_from_dict({'NET': dict(net or {}), 'TRAIN': dict(train or {})})


def _build(net, C=32, K=20, **kw):
    return nets_factory.get_network_fn('resnet_v1_101', K, 16, _cfg(net), is_training=True, device='cpu',
                                       in_channels=C, **kw)


def pal_build_head(fx):
    """the product module for a ref_pal_* fixture (construction only)"""
    m = fx.meta
    cfg = apa_config.cfg_from_dict({'MODEL_NAME': m['model'], 'NET': dict(m['net']), 'TRAIN': dict(m['train_cfg'])})
    kw = dict(in_channels=fx.arrays['in/images'].shape[-1])
    if fx.pose_tap is not None:
        kw['pose_in_channels'] = fx.pose_tap.shape[-1]
    return nets_factory.get_network_fn(m['model'], m['num_classes'], m['num_pose_keypoints'], cfg,
                                       weight_decay=m['weight_decay'], is_training=m['is_training'], device='cpu',
                                       **kw), cfg


def test_fixtures_present():
    assert len(SMALL) >= 10 and len(pal.big_fixture_paths()) >= 2


@pytest.mark.parametrize('with_attention', [False, True])
def test_flag_routes_to_the_pose_attention_head(with_attention):
    net = {PA: True}
    if with_attention:
        net[P] = True                      # the reference's chain tests USE_POSE_ATTENTION_LOGITS first
    fn = _build(net)
    assert isinstance(fn.head, nets_factory.PoseAttentionLogitsHead)
    assert fn.head.num_maps == 17 and tuple(fn.head.logits_weights.shape) == (17 * 32, 20)
    assert not isinstance(fn.head, nets_factory.BaselineHead)
    apa_config.reset_cfg()


@pytest.mark.parametrize('with_attention', [False, True])
@pytest.mark.parametrize('flag', REFUSED)
def test_unimplemented_head_branches_are_refused(flag, with_attention):
    net = {flag: True}
    if with_attention:
        net[P] = True
    with pytest.raises(ValueError, match=flag):
        _build(net)
    apa_config.reset_cfg()


def test_pose_attention_flag_wins_over_the_refused_ones():
    fn = _build({PA: True, 'USE_POSE_LOGITS_DIRECTLY': True, 'USE_COMPACT_BILINEAR_POOLING': True})
    assert isinstance(fn.head, nets_factory.PoseAttentionLogitsHead)
    apa_config.reset_cfg()


def test_dims_normalisation():
    f = nets_factory.pose_attention_parts
    assert f([-1], 16) == list(range(16))
    assert f([3, 0, 9], 16) == [3, 0, 9]
    assert f([-2, 4, 4], 16) == [14, 4, 4]
    assert f([], 16) == []
    assert f([-1, 2], 16) == [15, 2]
    for bad in ([16], [-17], [0, 40]):
        with pytest.raises(ValueError):
            f(bad, 16)
    fn = _build({PA: True, PA + '_DIMS': [-2, 4, 4], PA + '_AVGED_HMAP': True}, C=16, K=12)
    assert fn.head.parts == [14, 4, 4] and fn.head.num_maps == 5
    with pytest.raises(ValueError):
        _build({PA: True, PA + '_DIMS': [16]})
    apa_config.reset_cfg()


@pytest.mark.parametrize('path', ALL, ids=pal.case_id)
def test_variable_names_and_shapes_match_the_fixture(path):
    fx = rf.HeadFixture(path)
    fn, _ = pal_build_head(fx)
    table = rf.module_tf_names(fn)
    assert sorted(table) == sorted(fx.meta['var_order'])
    for vn, t in table.items():
        assert tuple(t.shape) == tuple(fx.var(vn).shape), vn
    # the regulariser set is slim's: every conv `weights` variable
    reg = {id(w) for w in fn.regularized_weights()}
    assert {vn for vn, t in table.items() if id(t) in reg} == {vn for vn in table if vn.endswith('/weights')}
    apa_config.reset_cfg()


@pytest.mark.parametrize('path', SMALL, ids=pal.case_id)
def test_restatement_reproduces_the_reference_fixture(path):
    fx = rf.HeadFixture(path)
    got = pal.run_pal_fixture(fx)
    keys = [k for k in fx.output_keys() if not k.startswith('out/update/') and k != 'out/ep/PoseLossMask']
    assert 'out/logits' in keys and 'grad/images' in keys and 'grad/var/' + pal.ATT_W in keys
    for key in keys:
        fx.check(key, got[key], fx.tol(key, 1e-10), key, floor=1e-300)


def test_extra_state_and_replay_mask():
    fn = _build({PA: True})
    head = fn.head
    head._step = 7
    sd = head.state_dict()
    fn2 = _build({PA: True})
    fn2.head.load_state_dict(sd)
    assert fn2.head._step == 7
    head.replay_dropout_mask(torch.ones(2, 1, 1, 17 * 32))
    assert head._replay_mask is not None
    head.replay_dropout_mask(None)
    assert head._replay_mask is None
    apa_config.reset_cfg()


def test_fused_head_step_gives_a_reason():
    fn = _build({PA: True})
    why = deploy.FusedHeadStep.unsupported_reason(fn.head, _cfg({PA: True}), fn)
    assert why and 'USE_POSE_ATTENTION_LOGITS' in why
    apa_config.reset_cfg()


def test_abi_rejects_null_pointers_without_a_gpu():
    lib = cof.load_library()
    sel = (ctypes.c_int32 * 2)(0, 1)
    dummy = 256
    inval = -1
    fwd_ptrs = [dummy] * 8          # X, Pl, W, b, F, logits, ws + one spare
    for i in range(7):
        p = list(fwd_ptrs)
        p[i] = None
        X, Pl, W, b, F, logits, ws = p[:7]
        rc = lib.apa_pose_att_logits_fwd(X, Pl, sel, 2, 0, W, b, F, logits, ws, 1 << 20, 2, 4, 8, 16, 3, 0, 1.0,
                                         0, 0, 0, None)
        assert rc == inval, i
    # a selection list missing although n_sel > 0, a negative n_sel, a part index out of range, zero dimensions
    assert lib.apa_pose_att_logits_fwd(dummy, dummy, None, 2, 0, dummy, dummy, dummy, dummy, dummy, 1 << 20, 2, 4, 8,
                                       16, 3, 0, 1.0, 0, 0, 0, None) == inval
    assert lib.apa_pose_att_logits_fwd(dummy, dummy, sel, -1, 0, dummy, dummy, dummy, dummy, dummy, 1 << 20, 2, 4, 8,
                                       16, 3, 0, 1.0, 0, 0, 0, None) == inval
    bad = (ctypes.c_int32 * 1)(16)
    assert lib.apa_pose_att_logits_fwd(dummy, dummy, bad, 1, 0, dummy, dummy, dummy, dummy, dummy, 1 << 20, 2, 4, 8,
                                       16, 3, 0, 1.0, 0, 0, 0, None) == inval
    for dims in ((0, 4, 8, 16, 3), (2, 0, 8, 16, 3), (2, 4, 0, 16, 3), (2, 4, 8, 0, 3), (2, 4, 8, 16, 0)):
        assert lib.apa_pose_att_logits_fwd(dummy, dummy, sel, 2, 0, dummy, dummy, dummy, dummy, dummy, 1 << 20,
                                           *dims, 0, 1.0, 0, 0, 0, None) == inval
    # shapes the kernels are not built for: M > 32 maps, C not a multiple of 4, K > 480
    many = (ctypes.c_int32 * 40)(*([0] * 40))
    unsup = -2
    assert lib.apa_pose_att_logits_fwd(dummy, dummy, many, 40, 0, dummy, dummy, dummy, dummy, dummy, 1 << 20, 2, 4,
                                       8, 16, 3, 0, 1.0, 0, 0, 0, None) == unsup
    assert lib.apa_pose_att_logits_fwd(dummy, dummy, sel, 2, 0, dummy, dummy, dummy, dummy, dummy, 1 << 20, 2, 4, 6,
                                       16, 3, 0, 1.0, 0, 0, 0, None) == unsup
    assert lib.apa_pose_att_logits_fwd(dummy, dummy, sel, 2, 0, dummy, dummy, dummy, dummy, dummy, 1 << 20, 2, 4, 8,
                                       16, 481, 0, 1.0, 0, 0, 0, None) == unsup
    # backward: X, Pl, W, F, G, dX, dPl, dW, db, ws
    for i in range(10):
        p = [dummy] * 10
        p[i] = None
        X, Pl, W, F, G, dX, dPl, dW, db, ws = p
        rc = lib.apa_pose_att_logits_bwd(X, Pl, sel, 2, 1, W, F, G, dX, 0, dPl, dW, db, ws, 1 << 20, 2, 4, 8, 16, 3,
                                         0, 1.0, 0, 0, 0, None)
        assert rc == inval, i
    assert lib.apa_pose_att_logits_workspace_bytes(0, 4, 8, 3, 3) == 0
    assert lib.apa_pose_att_logits_workspace_bytes(32, 196, 2048, 17, 393) > 0
    assert lib.apa_version() >= 301
