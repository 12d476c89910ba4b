"""The one-call evaluation steps for clips and multi-label scores, the parts that need no GPU: the three entry points
are declared, exported and bound and refuse bad arguments before anything touches a device, the constants mirror the
header, the bound steps keep resolving to the old entry points with their default keywords, deploy.FusedHeadEval
constructs for a multi-label clip configuration, and the float64 restatement of the kernel's contract
(tests/_eval_clips_ref.py) reproduces what the reference computed on the two video evaluation fixtures."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _eval_clips_ref as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['apa_clip_scores', 'apa_attn_head_eval_step_clips', 'apa_pose_attn_eval_step_clips']
INVALID = -1


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    consts = dict(re.findall(r'#define\s+(APA_SCORES_\w+)\s+(\d+)', header))
    assert consts == {'APA_SCORES_SOFTMAX': str(cof.APA_SCORES_SOFTMAX), 'APA_SCORES_SIGMOID': str(cof.APA_SCORES_SIGMOID)}
    assert (cof.APA_SCORES_SOFTMAX, cof.APA_SCORES_SIGMOID) == (0, 1)
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = cof.load_library()
    for name in NEW:
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, header)
        assert m, '%s is not declared in include/apa.h' % name
        nargs = len([a for a in m.group(1).split(',') if a.strip()])
        assert hasattr(lib, name), name
        assert len(cof._SIGNATURES[name][1]) == nargs, (name, nargs)
    # the step forms: the clip, the kind, then exactly the flat entry point's arguments
    for name in ('apa_attn_head_eval_step', 'apa_pose_attn_eval_step'):
        assert cof._SIGNATURES[name + '_clips'][1][2:] == cof._SIGNATURES[name][1]
    assert lib.apa_version() >= 307


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = cof.load_library()
    p = 0x1000                                   # a non-null pointer that is never dereferenced
    err = lambda: lib.apa_last_error()
    SM, SG = cof.APA_SCORES_SOFTMAX, cof.APA_SCORES_SIGMOID

    # ---- apa_clip_scores(kind, logits, w, b, labels, pooled, tatt, scores, pred, loss, B, F, K, stream)
    def cs(kind=SM, logits=p, w=None, b=None, labels=None, pooled=p, tatt=None, scores=p, pred=p, loss=None, B=2, F=3,
           K=5):
        return lib.apa_clip_scores(kind, logits, w, b, labels, pooled, tatt, scores, pred, loss, B, F, K, None)
    for kw in (dict(logits=None), dict(pooled=None), dict(scores=None), dict(pred=None)):
        assert cs(**kw) == INVALID and b'null' in err(), kw
    for kw in (dict(B=0), dict(F=0), dict(K=-1), dict(B=1 << 20, F=1 << 12)):          # the last: B*F past 2^31
        assert cs(**kw) == INVALID and b'non-positive size or B*F' in err(), kw
    for kind in (2, -1, 7):
        assert cs(kind=kind) == INVALID and b'unknown scores kind' in err()
    assert cs(labels=p) == INVALID and b'together' in err()
    assert cs(loss=p) == INVALID and b'together' in err()
    assert cs(kind=SG, labels=p, loss=p) == INVALID and b'sigmoid' in err()
    assert cs(kind=SG, loss=p) == INVALID and cs(kind=SG, labels=p) == INVALID
    assert cs(w=p, tatt=p) == INVALID and b'temporal' in err()                         # w without b
    assert cs(w=p, b=p) == INVALID and b'temporal' in err()                            # w without tatt

    def clip(frames=4, w=None, b=None, pooled=p, tatt=None):
        c = cof.ApaClipPool()
        c.frames, c.w, c.b, c.pooled, c.tatt = frames, w, b, pooled, tatt
        return c
    addr = lambda c: None if c is None else ctypes.addressof(c)

    # ---- apa_attn_head_eval_step_clips(clip, kind, <apa_attn_head_eval_step's arguments>)
    def head(c, kind=SM, N=8, labels=None, loss=None, logits=p, probs=p, pred=p, X=p, K=5, P=4):
        return lib.apa_attn_head_eval_step_clips(addr(c), kind, X, X, p, p, p, p, labels, logits, p, p, p, loss, probs,
                                                 pred, p, 1 << 30, N, P, 256, 256, K, 1, 0, 0, None)
    good = clip()
    for c in (good, None):
        for kw in (dict(logits=None), dict(probs=None), dict(pred=None), dict(X=None)):
            assert head(c, kind=SG, **kw) == INVALID and b'null' in err(), kw
        for kw in (dict(N=0), dict(K=0), dict(P=-2)):
            assert head(c, kind=SG, **kw) == INVALID and b'non-positive' in err(), kw
        for kind in (2, -1):
            assert head(c, kind=kind) == INVALID and b'unknown scores kind' in err()
        assert head(c, kind=SG, labels=p, loss=p) == INVALID and b'sigmoid' in err()
        assert head(c, kind=SG, labels=p) == INVALID and head(c, kind=SG, loss=p) == INVALID
        assert head(c, labels=p) == INVALID and b'together' in err()
    assert head(good, N=6) == INVALID and b'whole number of clips' in err()            # N % frames
    assert head(clip(frames=0)) == INVALID and b'whole number of clips' in err()
    assert head(clip(pooled=None)) == INVALID and b'pooled' in err()
    assert head(clip(w=p, tatt=p)) == INVALID and b'pooled' in err()                   # w without b
    assert head(clip(w=p, b=p)) == INVALID and b'pooled' in err()                      # w without tatt

    # ---- apa_pose_attn_eval_step_clips(clip, kind, io, N, P, C, Cp, J, K, flags, dtype, stream)
    io = cof.ApaPoseAttnEvalIO()
    for name in ('X', 'W1', 'b1', 'W2', 'b2', 'Wa', 'ba', 'Wt', 'bt', 'att', 'logits', 'zsave', 'abar', 'probs', 'pred',
                 'ws'):
        setattr(io, name, p)
    io.ws_bytes = 1 << 30
    ioa = ctypes.addressof(io)
    pose = lambda c, kind=SM, io_ptr=ioa, N=8, J=16, K=5: lib.apa_pose_attn_eval_step_clips(
        addr(c), kind, io_ptr, N, 4, 64, 256, J, K, 0, cof.APA_DTYPE_BF16, None)
    for c in (good, None):
        assert pose(c, io_ptr=None) == INVALID and b'null' in err()
        assert pose(c, kind=SG, N=0) == INVALID and pose(c, kind=SG, K=0) == INVALID and pose(c, kind=SG, J=0) == INVALID
        assert pose(c, kind=3) == INVALID and b'unknown scores kind' in err()
    assert pose(good, N=6) == INVALID and b'whole number of clips' in err()
    assert pose(clip(pooled=None)) == INVALID and b'pooled' in err()
    assert pose(clip(w=p, b=p)) == INVALID and b'pooled' in err()
    io.labels, io.loss = p, p
    assert pose(good, kind=SG) == INVALID and b'sigmoid' in err()
    assert pose(None, kind=SG) == INVALID and b'sigmoid' in err()
    io.loss = None
    assert pose(good) == INVALID and b'together' in err()
    io.labels = None
    io.probs = None
    assert pose(good) == INVALID and b'null' in err()


def test_bound_steps_with_default_keywords_resolve_to_the_old_entry_points(monkeypatch):
    """construction only, on host tensors: the device check of the pointer helper is stood in for, nothing runs"""
    monkeypatch.setattr(cof, '_dev_ptr', lambda t, name, dtype=None: None if t is None else t.data_ptr())
    lib = cof.load_library()
    N, P, C, K, Cp, J = 4, 9, 32, 5, 64, 16
    X = torch.zeros(N, P, C)
    Wa, ba, Wt, bt = torch.zeros(C, 1), torch.zeros(1), torch.zeros(C, K), torch.zeros(K)
    ev = cof.HeadEvalStep(X, X, Wa, ba, Wt, bt)
    assert ev._fn is lib.apa_attn_head_eval_step and ev._pre == () and ev._name == 'apa_attn_head_eval_step'
    assert tuple(ev.probs.shape) == (N, K) and tuple(ev.pred.shape) == (N,) and ev.pooled is None and ev.tatt is None
    assert len(ev._pre) + len(ev._args) + 1 == len(cof._SIGNATURES['apa_attn_head_eval_step'][1])
    params = (torch.zeros(C, Cp), torch.zeros(Cp), torch.zeros(Cp, J), torch.zeros(J), torch.zeros(Cp, 1),
              torch.zeros(1), Wt, bt)
    pv = cof.PoseAttnEvalStep(X, params)
    assert pv._fn is lib.apa_pose_attn_eval_step and pv._name == 'apa_pose_attn_eval_step' and pv.pooled is None
    assert len(pv._args) + 1 == len(cof._SIGNATURES['apa_pose_attn_eval_step'][1])
    # clips and / or sigmoid scores: the _clips entry points, outputs per clip
    w, b = torch.zeros(K), torch.zeros(1)
    ec2 = cof.HeadEvalStep(X, X, Wa, ba, Wt, bt, frames=2, temporal=(w, b), scores='sigmoid')
    assert ec2._fn is lib.apa_attn_head_eval_step_clips and ec2._pre[1] == cof.APA_SCORES_SIGMOID
    assert tuple(ec2.probs.shape) == (2, K) and tuple(ec2.pred.shape) == (2,) and tuple(ec2.logits.shape) == (N, K)
    assert tuple(ec2.pooled.shape) == (2, K) and tuple(ec2.tatt.shape) == (N,)
    assert len(ec2._pre) + len(ec2._args) + 1 == len(cof._SIGNATURES['apa_attn_head_eval_step_clips'][1])
    flat = cof.HeadEvalStep(X, X, Wa, ba, Wt, bt, scores='sigmoid')
    assert flat._fn is lib.apa_attn_head_eval_step_clips and flat._pre == (None, cof.APA_SCORES_SIGMOID)
    pc = cof.PoseAttnEvalStep(X, params, torch.zeros(2, dtype=torch.int64), frames=2)
    assert pc._fn is lib.apa_pose_attn_eval_step_clips and pc.loss.numel() == 3 and pc.tatt is None
    assert len(pc._args) + 1 == len(cof._SIGNATURES['apa_pose_attn_eval_step_clips'][1])
    with pytest.raises(cof.ApaError, match='whole number of clips'):
        cof.HeadEvalStep(X, X, Wa, ba, Wt, bt, frames=3)
    with pytest.raises(cof.ApaError, match='sigmoid scores take no labels'):
        cof.HeadEvalStep(X, X, Wa, ba, Wt, bt, torch.zeros(N, dtype=torch.int64), scores='sigmoid')
    with pytest.raises(cof.ApaError, match="'softmax' or 'sigmoid'"):
        cof.HeadEvalStep(X, X, Wa, ba, Wt, bt, scores='l2')


def test_fused_head_eval_constructs_for_a_multilabel_clip_configuration():
    from attentionalpoolingaction_amd import deploy
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_video_temporal_att_eval.npz'))
    fx.meta['train_cfg'] = dict(fx.meta['train_cfg'], LOSS_FN_ACTION='multi-label')
    try:
        network_fn, cfg = rf.build_head(fx, device='cpu')
        assert network_fn.temporal is not None and cfg.NET.USE_TEMPORAL_ATT
        assert deploy.FusedHeadEval.unsupported_reason(network_fn.head, cfg, network_fn) == ''
        ev = deploy.FusedHeadEval(network_fn, cfg)
        assert ev.multi_label and not ev.pose_form and ev.max_bound_steps == 4
    finally:
        apa_config.reset_cfg()


@pytest.mark.parametrize('name', ['video_temporal_att_eval', 'video_framepool_eval'])
def test_float64_contract_reproduces_the_reference_fixture(name):
    """out/logits (and out/ep/TemporalAttention) from out/ep/logits_beforePool, to 1e-12"""
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_%s.npz' % name))
    x = np.asarray(fx.expected('out/ep/logits_beforePool'), dtype=np.float64)
    exp = np.asarray(fx.expected('out/logits'), dtype=np.float64)
    B = exp.shape[0]
    F = x.shape[0] // B
    assert fx.arrays['in/images'].shape[:2] == (B, F)
    w = b = None
    if name == 'video_temporal_att_eval':
        w = np.asarray(fx.var('TemporalAttention/Conv/weights'), dtype=np.float64).reshape(-1)
        b = np.asarray(fx.var('TemporalAttention/Conv/biases'), dtype=np.float64).reshape(-1)
    got = ec.clip_scores_f64(x, F, w, b)
    scale = max(float(np.abs(exp).max()), 1e-30)
    assert np.abs(got['pooled'] - exp).max() <= 1e-12 * max(scale, 1.0)
    assert np.array_equal(got['pred'], exp.argmax(1))
    if w is not None:
        ta = np.asarray(fx.expected('out/ep/TemporalAttention'), dtype=np.float64).reshape(-1)
        assert np.abs(got['tatt'] - ta).max() <= 1e-12 * max(float(np.abs(ta).max()), 1.0)
    assert np.abs(got['scores'].sum(1) - 1.0).max() <= 1e-12
    sg = ec.clip_scores_f64(x, F, w, b, kind='sigmoid')
    assert np.array_equal(sg['pred'], got['pred']) and np.abs(sg['scores'] - 1 / (1 + np.exp(-exp))).max() <= 1e-12
