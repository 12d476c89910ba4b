"""Class attention maps and overlays (csrc/apa_explain.hip) without a GPU: the C ABI and every refusal, made before any
HIP call; the float64 restatement of apa_attn_explain (tests/_explain_reference.py) against the reference's own end
points on every evaluation-mode head fixture; the overlay restatement against the reference-executed
tests/golden/ref_overlay.npz; and what deploy.FusedHeadEval.explain refuses."""
import json
import os
import re

import numpy as np
import pytest
import torch
import yaml

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy, nets_factory
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _explain_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NEW = ('apa_attn_explain_workspace_bytes', 'apa_attn_explain', 'apa_attention_overlay')
P = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
EVAL_FIXTURES = ['cfg002_eval', 'cfg002_eval_c2048', 'cfg003_eval', 'relu_eval', 'softmax_eval_c2048',
                 'perclass_softmax_eval']


# ------------------------------------------------------------------------------------------ C ABI
def test_header_declares_library_exports_and_ctypes_binds_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    defs = dict(re.findall(r'#define\s+(APA_[A-Z0-9_]+)\s+(\d+)u?\b', header))
    assert int(defs['APA_VERSION']) >= 311 and int(defs['APA_EXPLAIN_MAX_CLASSES']) == cof.APA_EXPLAIN_MAX_CLASSES == 8
    lib = cof.load_library()
    assert lib.apa_version() >= 311
    for name in NEW + ('apa_attention_overlay_workspace_bytes',):
        assert re.search(r'\b%s\s*\(' % name, header), name + ' is not declared in include/apa.h'
        assert name in cof.exported_symbols() and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == len(cof._SIGNATURES[name][1])
    assert callable(cof.attn_explain) and callable(cof.attention_overlay)
    assert callable(deploy.FusedHeadEval.explain)


FAKE = 0x10000                       # a 16-byte aligned non-null address: nothing is dereferenced


def _explain(lib, N=2, P_=9, C=32, K=8, M=1, T=2, flags=0, dtype=0, ws_bytes=0, null=None, ws=FAKE, x=FAKE):
    ptrs = dict(X=x, att=FAKE, Wt=FAKE, bt=FAKE, classes=FAKE, topdown=FAKE, combined=FAKE, class_logit=FAKE,
                status=None)
    if null:
        ptrs[null] = None
    rc = lib.apa_attn_explain(None, *[ptrs[k] for k in ('X', 'att', 'Wt', 'bt', 'classes', 'topdown', 'combined',
                                                  'class_logit', 'status')], ws, ws_bytes, N, P_, C, K, M, T, flags,
                              dtype, None)
    return rc, lib.apa_last_error().decode()


@pytest.mark.parametrize('field', ['X', 'att', 'Wt', 'bt', 'classes', 'topdown', 'combined', 'class_logit'])
def test_explain_null_required_pointer(field):
    rc, msg = _explain(cof.load_library(), null=field, ws_bytes=1 << 30)
    assert rc == INVALID and 'null' in msg


def test_explain_refusals_come_before_any_hip_call():
    lib = cof.load_library()
    big = 1 << 30
    for kw in (dict(N=0), dict(P_=0), dict(C=0), dict(K=0), dict(M=0), dict(N=-3)):
        rc, msg = _explain(lib, ws_bytes=big, **kw)
        assert rc == INVALID and 'non-positive' in msg, (kw, msg)
    for M in (2, 7, 9):                                          # K = 8
        rc, msg = _explain(lib, ws_bytes=big, M=M)
        assert rc == INVALID and 'must be 1 or K' in msg
    for flags in (cof.APA_FLAG_TRAIN, cof.APA_FLAG_SOFTMAX_ATT, cof.APA_FLAG_RELU_INPUT | cof.APA_FLAG_RELU_ATT, 1 << 20):
        rc, msg = _explain(lib, ws_bytes=big, flags=flags)
        assert rc == INVALID and 'flags' in msg, flags
    for T in (0, -1, 9, 64):
        rc, msg = _explain(lib, ws_bytes=big, T=T)
        assert rc == UNSUPPORTED and 'classes per image' in msg, T
    for C in (30, 2, 33):
        rc, msg = _explain(lib, ws_bytes=big, C=C)
        assert rc == UNSUPPORTED and 'multiple of 4' in msg, C
    rc, msg = _explain(lib, ws_bytes=big, dtype=cof.APA_DTYPE_FP8_E4M3)
    assert rc == UNSUPPORTED and 'FP8' in msg
    rc, msg = _explain(lib, ws_bytes=big, dtype=7)
    assert rc == INVALID and 'dtype' in msg
    rc, msg = _explain(lib, ws_bytes=big, C=4096, T=8)           # 128 KiB of weights per image
    assert rc == UNSUPPORTED and 'LDS' in msg
    # the last accepted call stops at the workspace check, for every served form
    for kw in (dict(), dict(M=8), dict(flags=cof.APA_FLAG_RELU_INPUT), dict(dtype=cof.APA_DTYPE_BF16), dict(T=8),
               dict(T=1, C=36, dtype=cof.APA_DTYPE_BF16), dict(N=32, P_=196, C=2048, K=393, T=8)):
        need = lib.apa_attn_explain_workspace_bytes(kw.get('N', 2), kw.get('P_', 9), kw.get('C', 32), kw.get('K', 8),
                                                    kw.get('T', 2), kw.get('dtype', 0))
        assert need > 0
        rc, msg = _explain(lib, ws_bytes=need - 1, **kw)
        assert rc == WORKSPACE and 'workspace' in msg, (kw, msg)
        rc, msg = _explain(lib, ws_bytes=need, ws=None, **kw)
        assert rc == WORKSPACE
    # ... and, with room, at the alignment of X and of the workspace
    rc, msg = _explain(lib, ws_bytes=big, x=FAKE + 4)
    assert rc == INVALID and 'aligned' in msg
    rc, msg = _explain(lib, ws_bytes=big, ws=FAKE + 8)
    assert rc == INVALID and 'aligned' in msg
    rc, msg = _explain(lib, ws_bytes=big, x=FAKE + 8, C=36, dtype=cof.APA_DTYPE_BF16)    # 8-byte rows: not refused here
    assert rc != INVALID or 'aligned' not in msg


def test_explain_workspace_query():
    lib = cof.load_library()
    q = lib.apa_attn_explain_workspace_bytes
    assert q(32, 196, 2048, 393, 8, 0) >= 32 * 8 * 2048 * 4 + 2 * 32 * 8 * 4
    assert q(32, 196, 2048, 393, 1, 1) >= 32 * 2048 * 4
    for bad in ((0, 9, 32, 8, 2, 0), (2, 0, 32, 8, 2, 0), (2, 9, 0, 8, 2, 0), (2, 9, 32, 0, 2, 0), (2, 9, 32, 8, 0, 0),
                (2, 9, 32, 8, 9, 0), (2, 9, 30, 8, 2, 0), (2, 9, 32, 8, 2, cof.APA_DTYPE_FP8_E4M3), (2, 9, 32, 8, 2, 5),
                (2, 9, 4096, 8, 8, 0)):
        assert q(*bad) == 0, bad


def _overlay(lib, maps=FAKE, images=FAKE, f32=FAKE, u8=FAKE, ws=FAKE, ws_bytes=1 << 30, N=2, T=2, h=3, w=5, H=13, W=17):
    rc = lib.apa_attention_overlay(maps, images, f32, u8, ws, ws_bytes, N, T, h, w, H, W, None)
    return rc, lib.apa_last_error().decode()


def test_overlay_refusals_come_before_any_hip_call():
    lib = cof.load_library()
    for kw in (dict(maps=None), dict(images=None), dict(f32=None, u8=None)):
        rc, msg = _overlay(lib, **kw)
        assert rc == INVALID and 'null' in msg, kw
    for dim in ('N', 'T', 'h', 'w', 'H', 'W'):
        for v in (0, -2):
            rc, msg = _overlay(lib, **{dim: v})
            assert rc == INVALID and 'non-positive' in msg, dim
    need = lib.apa_attention_overlay_workspace_bytes(2, 2)
    assert need > 0 and lib.apa_attention_overlay_workspace_bytes(0, 2) == 0 == lib.apa_attention_overlay_workspace_bytes(2, -1)
    rc, msg = _overlay(lib, ws_bytes=need - 1)
    assert rc == WORKSPACE and 'workspace' in msg
    rc, msg = _overlay(lib, ws=None)
    assert rc == WORKSPACE


# ------------------------------------------------------------------------- the restatement against the reference
def _fixture_inputs(fx):
    """X [N,P,C], att [N,P,M], Wt [C,K], bt [K] of an evaluation-mode head fixture, and its grid"""
    x = torch.from_numpy(fx.arrays['in/images'])
    n, hh, ww, c = x.shape
    att = torch.from_numpy(np.asarray(fx.expected('out/ep/PosePrelogitsBasedAttention'), dtype=np.float64))
    Wt = torch.from_numpy(fx.var(rf.PRE + 'Conv/weights'))
    bt = torch.from_numpy(fx.var(rf.PRE + 'Conv/biases').reshape(-1))
    return x.reshape(n, hh * ww, c).double(), att.reshape(n, hh * ww, -1), Wt, bt, (n, hh, ww)


def fixture_classes(n, K):
    """first, last and a repeated class"""
    return torch.tensor([[0, K - 1, 0]] * n)


@pytest.mark.parametrize('name', EVAL_FIXTURES)
def test_restatement_reproduces_the_reference_end_points(name):
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_%s.npz' % name))
    assert not fx.meta['is_training']
    X, att, Wt, bt, (n, hh, ww) = _fixture_inputs(fx)
    K = Wt.shape[1]
    cls = fixture_classes(n, K)
    td, comb, logit, clamped = er.explain_reference(X, att, Wt, bt, cls)
    assert clamped == 0
    exp_td = np.asarray(fx.expected('out/ep/TopDownAttention'), dtype=np.float64).reshape(n, hh * ww, K)
    exp_lg = np.asarray(fx.expected('out/logits'), dtype=np.float64)
    tol_td, tol_lg = fx.tol('out/ep/TopDownAttention'), fx.tol('out/logits')
    for i in range(n):
        for t in range(cls.shape[1]):
            k = int(cls[i, t])
            e = np.abs(td.ref[i, t].numpy() - exp_td[i, :, k]).max()
            assert e <= tol_td * np.abs(exp_td).max(), (i, t, e)
            assert abs(float(logit.ref[i, t]) - exp_lg[i, k]) <= tol_lg * np.abs(exp_lg).max(), (i, t)
    # the combined map is bottom-up times top-down of the same class, and the bounds are small against the values
    a = att[:, :, 0] if att.shape[2] == 1 else None
    for t in range(cls.shape[1]):
        bu = a if a is not None else att[:, :, int(cls[0, t])]
        assert torch.equal(comb.ref[:, t], bu * td.ref[:, t])
    # (the logit's bound is the worst-case one of a C-long and a P-long sum over untrained, cancelling weights)
    assert float(td.err.max()) < 0.01 * float(td.ref.abs().max())
    assert float(logit.err.max()) < 0.05 * float(logit.ref.abs().max())


def test_restatement_clamps_and_counts_class_ids():
    g = torch.Generator().manual_seed(5)
    X, att = torch.randn(2, 6, 8, generator=g), torch.rand(2, 6, 1, generator=g)
    Wt, bt = torch.randn(8, 5, generator=g), torch.randn(5, generator=g)
    a = er.explain_reference(X, att, Wt, bt, torch.tensor([[-1, 5], [7, -9]]))
    b = er.explain_reference(X, att, Wt, bt, torch.tensor([[0, 4], [4, 0]]))
    assert a[3] == 4 and b[3] == 0
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u.ref, v.ref)
    r = er.explain_reference(X, att, Wt, bt, torch.tensor([[0, 4], [4, 0]]), relu_input=True)
    want = torch.einsum('npc,c->np', X.double().clamp_min(0), Wt.double()[:, 4]) + bt.double()[4]
    assert torch.allclose(r[0].ref[0, 1], want[0], rtol=0, atol=1e-12)


def _overlay_fixture():
    d = np.load(os.path.join(rf.GOLD, 'ref_overlay.npz'))
    return d, json.loads(str(d['meta']))['cases']


def test_overlay_fixture_inputs_regenerate_from_their_seeds():
    d, cases = _overlay_fixture()
    assert [c['name'] for c in cases] == [c['name'] for c in er.OVERLAY_CASES]
    shapes = {(c['h'], c['w'], c['H'], c['W']) for c in cases}
    assert {(3, 5, 13, 17), (15, 15, 45, 45), (14, 14, 64, 64)} <= shapes
    assert {c['branch'] for c in cases} == {'lo<0', 'lo>=0'}
    for c, mine in zip(cases, er.OVERLAY_CASES):
        assert all(c[k] == mine[k] for k in mine)
        maps, images = er.overlay_inputs(c)
        assert er.checksum(maps, images) == c['crc'], c['name']
        assert d['expected/' + c['name']].shape == (c['N'], c['T'], c['H'], c['W'], 3)
    assert os.path.getsize(os.path.join(rf.GOLD, 'ref_overlay.npz')) < 512 * 1024


def test_overlay_restatement_reproduces_the_reference_execution():
    d, cases = _overlay_fixture()
    for c in cases:
        maps, images = er.overlay_inputs(c)
        v, mag = er.overlay_reference(maps, images)
        exp = d['expected/' + c['name']].astype(np.float64)
        over = np.abs(v - exp) - er.overlay_bound(mag)
        assert float(over.max()) <= 0, (c['name'], float(over.max()))
        assert float(er.overlay_bound(mag).max()) < 1e-3 * float(np.abs(exp).max())
        # the uint8 rule: both branches present, the band condition holds on the reference alone
        u8, q = er.overlay_u8_reference(v)
        flat = v.reshape(c['N'], c['T'], -1)
        assert ((flat.min(-1) < 0).all() and c['branch'] == 'lo<0') or ((flat.min(-1) >= 0).all() and c['branch'] == 'lo>=0')
        assert float(er.u8_band(q).reshape(c['N'], c['T'], -1).mean(-1).max()) <= er.BAND_SHARE
        if c['branch'] == 'lo<0':          # 0.0 lands on 128 and the extreme on 1 or 255
            assert int(u8.reshape(c['N'], c['T'], -1).max(-1).max()) <= 255 and (np.abs(q - 128.0).max() <= 127.0 + 1e-9)
        else:
            # the maximum lands on 255, or on 254 where hi * (255 / hi) rounds below it (inside the band)
            assert (u8.reshape(c['N'], c['T'], -1).max(-1) >= 254).all()


def test_overlay_u8_rule_edge_cases():
    z = np.zeros((1, 1, 2, 2, 3))
    u8, q = er.overlay_u8_reference(z)
    assert not u8.any() and not q.any()                                            # s = 0
    v = np.array([-2.0, 0.0, 1.0, 2.0] * 3).reshape(1, 1, 2, 2, 3)
    u8, _ = er.overlay_u8_reference(v)
    assert sorted(set(u8.reshape(-1).tolist())) == [1, 128, 191, 255]              # s = 63.5, o = 128
    v = np.array([0.0, 1.0, 2.0, 4.0] * 3).reshape(1, 1, 2, 2, 3)
    u8, _ = er.overlay_u8_reference(v)
    assert sorted(set(u8.reshape(-1).tolist())) == [0, 63, 127, 255]               # s = 63.75, o = 0


# ------------------------------------------------------------------------------------------ FusedHeadEval.explain
def _cfg(net=None, train=None):
    apa_config.reset_cfg()
    return apa_config.cfg_from_dict({'NET': dict(net or {}), 'TRAIN': dict(train or {})})


def _build(cfg, is_training=False, **kw):
    return nets_factory.get_network_fn('resnet_v1_101', 20, 16, cfg, is_training=is_training, device='cpu',
                                       in_channels=32, **kw)


def _yaml_cfg(name, tmp_path, net_extra=None):
    path = rf.experiment_yaml(name, tmp_path)
    if net_extra:
        tree = yaml.safe_load(open(path))
        tree.setdefault('NET', {}).update(net_extra)
        path = os.path.join(str(tmp_path), 'variant_' + name)
        with open(path, 'w') as f:
            yaml.safe_dump(tree, f, default_flow_style=False)
    apa_config.reset_cfg()
    return apa_config.cfg_from_file(path)


def test_explain_value_errors_on_a_cpu_built_head():
    cfg = _cfg({P: True, P + '_SINGLE_LAYER_ATT': True})
    # a training-mode head never gets as far as explain ...
    with pytest.raises(ValueError, match='training-mode'):
        deploy.FusedHeadEval(_build(cfg, is_training=True), cfg)
    fn = _build(cfg)
    ev = deploy.FusedHeadEval(fn, cfg)
    conv5 = torch.zeros(2, 3, 3, 32)
    # ... and one that is switched to training afterwards is refused by explain itself
    fn.head.is_training = True
    with pytest.raises(ValueError, match='training-mode'):
        ev.explain(conv5, overlay=False)
    fn.head.is_training = False
    with pytest.raises(ValueError, match='Fp8Features.*dense'):
        ev.explain(cof.Fp8Features.empty((2, 3, 3, 32), 'cpu'), overlay=False)
    with pytest.raises(ValueError, match='image source'):
        ev.explain(conv5)                                       # no backbone in front, no input_images
    with pytest.raises(ValueError, match='topk'):
        ev.explain(conv5, topk=9, overlay=False)
    apa_config.reset_cfg()


@pytest.mark.parametrize('name,extra', [
    ('002_MPII_ResNet_withAttention.yaml', None),
    ('003_MPII_ResNet_withPoseAttention.yaml', None),
    ('002_MPII_ResNet_withAttention.yaml', {P + '_PER_CLASS': True}),
], ids=['cfg002', 'cfg003', 'per_class_single_layer'])
def test_unsupported_reason_is_unchanged_for_the_shipped_forms(name, extra, tmp_path):
    cfg = _yaml_cfg(name, tmp_path, extra)
    fn = _build(cfg)
    assert deploy.FusedHeadEval.unsupported_reason(fn.head, cfg, fn) == ''
    assert hasattr(deploy.FusedHeadEval(fn, cfg), 'explain')
    apa_config.reset_cfg()


@pytest.mark.parametrize('net,kw,training,text', [
    ({P: True}, {}, True, 'a training-mode head: build network_fn with is_training=False (evaluation draws no dropout mask)'),
    ({P: True, P + '_RANK': 2}, {}, False, 'rank > 1 runs through the per-op module'),
    ({P: True, P + '_SINGLE_LAYER_ATT': True}, {'want_topdown': True}, False,
     'the TopDownAttention dump is materialised by the per-op module only'),
    ({P: True, P + '_PER_CLASS': True}, {}, False, 'per-class maps from pose_pre_logits'),
], ids=['training', 'rank2', 'topdown', 'per_class_posepre'])
def test_unsupported_reason_still_refuses_what_it_refused(net, kw, training, text):
    cfg = _cfg(net)
    fn = _build(cfg, is_training=training, **kw)
    assert deploy.FusedHeadEval.unsupported_reason(fn.head, cfg, fn) == text
    apa_config.reset_cfg()
