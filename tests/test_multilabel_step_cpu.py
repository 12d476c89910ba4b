"""The one-call training steps under the multi-label action losses (HICO, Charades), the parts that need no GPU: the
reference-executed fixtures (tests/golden/make_multilabel_step_reference.py) are present and the float64 oracle
reproduces them, the new entry points are declared, exported, bound and refuse bad arguments before anything touches a
device, deploy.FusedHeadStep accepts the two kinds, and the bound steps check the label tensor."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ['flat002_ml_c512', 'flat002_ml2_c32', 'clip_temporal_ml', 'cfg003_ml2', 'cfg003_clip_ml_bf16_c512']
BIG = ['hico_32x14x14_k600_libmask', 'charades_8x4_k157_libmask']
NEW = ['apa_multilabel_loss_fwd_bwd', 'apa_clip_multilabel_fwd_bwd', 'apa_attn_head_train_step_multilabel',
       'apa_pose_attn_train_step_multilabel']
INVALID = -1


def ml_fixture(name):
    """a ref_mlstep fixture with the multi-hot labels where tests/_ref_fixture.py reads the action labels"""
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_mlstep_%s.npz' % name))
    fx.arrays['in/labels_action'] = fx.arrays['in/labels_action_multihot']
    return fx


def test_the_multilabel_step_fixtures_are_present_and_small():
    got = sorted(os.path.basename(p) for p in glob.glob(os.path.join(rf.GOLD, 'ref_mlstep_*.npz')))
    want = sorted(['ref_mlstep_%s.npz' % n for n in SMALL] + ['ref_mlstep_big_%s.npz' % n for n in BIG])
    assert got == want
    for n in got:
        assert os.path.getsize(os.path.join(rf.GOLD, n)) < (1 << 20), n
    # none of them is picked up by the existing fixture tests' globs
    old = rf.head_fixture_paths() + rf.big_fixture_paths() + rf.train_fixture_paths() + \
        glob.glob(os.path.join(rf.GOLD, 'ref_vstep_*.npz')) + glob.glob(os.path.join(rf.GOLD, 'ref_pal_*.npz')) + \
        glob.glob(os.path.join(rf.GOLD, 'ref_clip_*.npz'))
    assert not [p for p in old if 'mlstep' in p]
    for n in SMALL + ['big_' + b for b in BIG]:
        d = np.load(os.path.join(rf.GOLD, 'ref_mlstep_%s.npz' % n))
        m = json.loads(str(d['meta']))
        assert m['is_training'] and len(m['libmask']) == 2 and len(m['draws']) == 1, n
        assert m['train_cfg']['LOSS_FN_ACTION'] in ('multi-label', 'multi-label-2'), n
        t = d['in/labels_action_multihot']
        assert t.dtype == np.float32 and t.shape[1] == m['num_classes'] and set(np.unique(t)) <= {0.0, 1.0}, n
        assert not t[0].any() and t.any(), n                       # an all-zero row, and positives elsewhere
        assert t[-1].any() and t[1:].mean() < 0.3, n               # each class positive with probability ~0.1
        if n.startswith('big_'):
            assert 0.08 < t[1:].mean() < 0.12, n


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    lib = cof.load_library()
    for name in NEW:
        m = re.search(r'\b%s\s*\(([^)]*)\)' % name, header)
        assert m, '%s is not declared in include/apa.h' % name
        nargs = len([a for a in m.group(1).split(',') if a.strip()])
        assert hasattr(lib, name), name
        assert len(cof._SIGNATURES[name][1]) == nargs, (name, nargs)
    assert re.search(r'typedef\s+struct\s+apa_multilabel\s*\{\s*int\s+kind;\s*const\s+float\*\s+labels;\s*float\s+'
                     r'pos_weight;\s*\}\s*apa_multilabel;', header)
    assert [n for n, _ in cof.ApaMultilabel._fields_] == ['kind', 'labels', 'pos_weight']
    assert lib.apa_version() >= 305


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = cof.load_library()
    p = 0x1000                                   # a non-null pointer that is never dereferenced
    err = lambda: lib.apa_last_error()

    def mls(kind=2, labels=p):
        ml = cof.ApaMultilabel()
        ml.kind, ml.labels, ml.pos_weight = kind, labels, 10.0
        return ml
    good = mls()
    bad_ml = [(None, b'null'), (mls(labels=None), b'null'), (mls(kind=1), b'kind'), (mls(kind=0), b'kind'),
              (mls(kind=7), b'kind')]
    addr = lambda ml: None if ml is None else ctypes.addressof(ml)

    # ---- apa_multilabel_loss_fwd_bwd(ml, logits, loss, G, N, K, wt, grad_scale, stream)
    rows = lambda ml, logits=p, loss=p, G=p, N=4, K=5: lib.apa_multilabel_loss_fwd_bwd(
        addr(ml), logits, loss, G, N, K, 1.0, 1.0, None)
    for ml, word in bad_ml:
        assert rows(ml) == INVALID and word in err(), word
    assert rows(good, logits=None) == INVALID and rows(good, loss=None) == INVALID and rows(good, G=None) == INVALID
    assert rows(good, N=0) == INVALID and rows(good, K=-1) == INVALID

    # ---- apa_clip_multilabel_fwd_bwd(ml, logits, w, b, pooled, tatt, loss, G, dw, db, ws, ws_bytes, B, F, K, ...)
    clip = lambda ml, ptrs, B=2, F=3, K=5: lib.apa_clip_multilabel_fwd_bwd(addr(ml), *ptrs, p, 1 << 20, B, F, K, 1.0,
                                                                            1.0, None)
    ok = [p, None, None, p, None, p, p, None, None]
    for ml, word in bad_ml:
        assert clip(ml, ok) == INVALID and word in err(), word
    for i in (0, 3, 5, 6):                       # logits, pooled, loss, G
        bad = list(ok)
        bad[i] = None
        assert clip(good, bad) == INVALID and b'null' in err(), i
    assert clip(good, [p, p, None, p, p, p, p, p, p]) == INVALID                 # temporal attention without b
    for B, F, K in ((0, 3, 5), (2, 0, 5), (2, 3, 0)):
        assert clip(good, ok, B, F, K) == INVALID and b'non-positive' in err()

    # ---- apa_attn_head_train_step_multilabel(ml, clip, hooks, <apa_attn_head_train_step_ex's arguments, no labels>)
    cp = cof.ApaClipPool()
    cp.frames, cp.pooled = 4, p

    def head(ml, clip_ptr, N, loss=p, G=p, P=4, K=5):
        return lib.apa_attn_head_train_step_multilabel(addr(ml), clip_ptr, None, p, p, p, p, p, p, 1.0, 1.0, p, p, p, p,
                                                       loss, G, p, None, p, p, p, p, p, 1 << 30, N, P, 256, 256, K, 1,
                                                       4, 0.5, 0, 0, 0, None)
    a = ctypes.addressof(cp)
    for ml, word in bad_ml:
        assert head(ml, None, 8) == INVALID and word in err(), word
        assert head(ml, a, 8) == INVALID and word in err(), word
    assert head(good, a, 6) == INVALID and b'whole number of clips' in err()     # N % frames
    assert head(good, None, 8, loss=None) == INVALID and head(good, None, 8, G=None) == INVALID
    assert head(good, a, 8, loss=None) == INVALID and head(good, a, 8, G=None) == INVALID
    assert head(good, None, 0) == INVALID and head(good, None, 8, P=0) == INVALID and head(good, a, 8, K=-3) == INVALID

    # ---- apa_pose_attn_train_step_multilabel(ml, clip, io, N, P, C, Cp, J, K, flags, keep_prob, seed, offset, dtype, stream)
    io = cof.ApaPoseAttnStepIO()
    for name, ct in cof.ApaPoseAttnStepIO._fields_:
        setattr(io, name, p if ct is ctypes.c_void_p else (1 << 30 if ct is ctypes.c_size_t else 1.0))
    io.labels = None                                                             # unused under a multi-label loss
    pose = lambda ml, clip_ptr, io_ptr, N, J=16: lib.apa_pose_attn_train_step_multilabel(
        addr(ml), clip_ptr, io_ptr, N, 4, 256, 256, J, 5, 4, 0.5, 0, 0, 0, None)
    ioa = ctypes.addressof(io)
    for ml, word in bad_ml:
        assert pose(ml, None, ioa, 8) == INVALID and word in err(), word
        assert pose(ml, a, ioa, 8) == INVALID and word in err(), word
    assert pose(good, None, None, 8) == INVALID and pose(good, a, None, 8) == INVALID
    assert pose(good, a, ioa, 6) == INVALID and b'whole number of clips' in err()
    assert pose(good, None, ioa, 0) == INVALID and pose(good, None, ioa, 8, J=0) == INVALID
    io.G = None
    assert pose(good, None, ioa, 8) == INVALID and b'null' in err()


def _close(got, exp, tol, what):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(exp).shape)
    exp = np.asarray(exp, dtype=np.float64)
    scale = max(float(np.abs(exp).max()) if exp.size else 0.0, 1e-3)
    e = float(np.abs(got - exp).max()) if exp.size else 0.0
    assert e <= tol * scale, '%s: max abs err %.3e > %.1e * %.3e' % (what, e, tol, scale)


@pytest.mark.parametrize('name', SMALL)
def test_oracle_matches_the_multilabel_step_fixture(name):
    """oracle.attn_pool_oracle through tests/_ref_fixture.run_oracle -- head, frame pooling, gen_losses on the multi-hot
    labels, the regularisers, autograd -- against what the reference's own code computed: 1e-10, float32-stored tensors
    at storage rounding, digest-stored ones (the C = 512 cfg 003 case) through HeadFixture.check."""
    fx = ml_fixture(name)
    got = rf.run_oracle(fx)
    checked = 0
    for key in fx.output_keys():
        assert key in got, 'the oracle produces no %s' % key
        if 'digest/' + key in fx.arrays:
            fx.check(key, got[key], 1e-6, '%s %s' % (fx.name, key))          # a float32 digest of float64 values
        else:
            _close(got[key], fx.arrays[key], fx.tol(key, 1e-10), '%s %s' % (fx.name, key))
        checked += 1
    assert checked >= 8
    n_loss = fx.arrays['in/labels_action_multihot'].shape[0]
    assert got['out/logits'].shape == (n_loss, fx.meta['num_classes'])


def _network(case, loss_fn, extra_net=None):
    fx = ml_fixture(case)
    fx.meta['net'] = dict(fx.meta['net'], **(extra_net or {}))
    fx.meta['train_cfg'] = dict(fx.meta['train_cfg'], LOSS_FN_ACTION=loss_fn)
    return rf.build_head(fx, device='cpu')


@pytest.mark.parametrize('temporal', [False, True], ids=['flat', 'temporal'])
@pytest.mark.parametrize('kind', ['multi-label', 'multi-label-2'])
@pytest.mark.parametrize('case', ['flat002_ml2_c32', 'cfg003_ml2'], ids=['cfg002', 'cfg003'])
def test_fused_head_step_accepts_the_multilabel_losses(case, kind, temporal):
    from attentionalpoolingaction_amd import deploy
    try:
        network_fn, cfg = _network(case, kind, {'USE_TEMPORAL_ATT': True} if temporal else None)
        assert (network_fn.temporal is not None) == temporal
        assert cfg.TRAIN.LOSS_FN_ACTION == kind
        assert deploy.FusedHeadStep.unsupported_reason(network_fn.head, cfg, network_fn) == ''
        fused = deploy.FusedHeadStep(network_fn, cfg)
        assert fused.pose_form == (case == 'cfg003_ml2')
    finally:
        apa_config.reset_cfg()


@pytest.mark.parametrize('loss_fn', ['l2', ''])
def test_fused_head_step_still_refuses_the_other_action_losses(loss_fn):
    from attentionalpoolingaction_amd import deploy
    try:
        network_fn, cfg = _network('flat002_ml2_c32', loss_fn)
        why = deploy.FusedHeadStep.unsupported_reason(network_fn.head, cfg, network_fn)
        assert why == 'LOSS_FN_ACTION %r (the one-call steps take the softmax cross-entropy)' % loss_fn
        with pytest.raises(ValueError):
            deploy.FusedHeadStep(network_fn, cfg)
    finally:
        apa_config.reset_cfg()


def test_bound_steps_check_the_labels_of_a_multilabel_kind():
    """int64 class indices, a wrong shape or an unknown kind: ApaError before any pointer is taken"""
    N, P, C, K = 4, 9, 32, 5
    X = torch.zeros(N, P, C)
    Wa, ba, Wt, bt = torch.zeros(C, 1), torch.zeros(1), torch.zeros(C, K), torch.zeros(K)
    grads = (torch.zeros_like(X), None, torch.zeros_like(Wa), torch.zeros_like(ba), torch.zeros_like(Wt),
             torch.zeros_like(bt))
    for kind in ('multi-label', 'multi-label-2'):
        with pytest.raises(cof.ApaError, match='float32 multi-hot'):
            cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, torch.zeros(N, dtype=torch.int64), grads, action_loss=kind)
        with pytest.raises(cof.ApaError, match='float32 multi-hot'):
            cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, torch.zeros(N, K, dtype=torch.int64), grads, action_loss=kind)
        with pytest.raises(cof.ApaError, match='float32 multi-hot'):          # clips: one row per CLIP
            cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, torch.zeros(N, K), grads, action_loss=kind, frames=2)
    with pytest.raises(cof.ApaError, match='action_loss must be one of'):
        cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, torch.zeros(N, K), grads, action_loss='l2')
