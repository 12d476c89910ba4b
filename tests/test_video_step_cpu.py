"""The one-call training step on video clips, the parts that need no GPU: the reference-executed fixtures
(tests/golden/make_video_step_reference.py) are present and the float64 oracle reproduces them, the three new entry
points are declared, exported, bound and reject bad arguments before anything touches a device, and
deploy.FusedHeadStep accepts a network_fn with the TemporalAttention conv and owns its two parameters."""
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
SMALL = ['framepool_train', 'temporal_att_train', 'perclass_temporal_train', 'perclass_framepool_bf16_c256',
         'cfg003_temporal_train', 'cfg003_one_clip_f5', 'cfg003_framepool_bf16_c512']
BIG = ['hmdb51_perclass_8x4_libmask', 'cfg003_8x4_libmask']
NEW = ['apa_clip_xent_fwd_bwd', 'apa_attn_head_train_step_clips', 'apa_pose_attn_train_step_clips']
INVALID = -1


def small_path(name):
    return os.path.join(rf.GOLD, 'ref_vstep_%s.npz' % name)


def test_the_video_step_fixtures_are_present_and_small():
    got = sorted(os.path.basename(p) for p in glob.glob(os.path.join(rf.GOLD, 'ref_vstep_*.npz')))
    want = sorted(['ref_vstep_%s.npz' % n for n in SMALL] + ['ref_vstep_big_%s.npz' % n for n in BIG])
    assert got == want
    for n in got:
        assert os.path.getsize(os.path.join(rf.GOLD, n)) < (1 << 20), n
    # none of them is picked up by the existing fixture tests' globs
    assert not [p for p in rf.head_fixture_paths() + rf.big_fixture_paths() if 'vstep' in p]
    for n in SMALL + ['big_' + b for b in BIG]:
        m = json.loads(str(np.load(os.path.join(rf.GOLD, 'ref_vstep_%s.npz' % n))['meta']))
        assert m['is_training'] and len(m['libmask']) == 2 and len(m['draws']) == 1, n
        assert len(m['draws'][0]['shape']) == 4, n                # the dropout draw is over the FOLDED frames


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
    assert re.search(r'typedef\s+struct\s+apa_clip_pool\s*\{\s*int\s+frames;', header)
    fields = [n for n, _ in cof.ApaClipPool._fields_]
    assert fields == ['frames', 'w', 'b', 'pooled', 'tatt', 'dw', 'db']
    assert lib.apa_version() >= 304


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = cof.load_library()
    p = 0x1000                                   # a non-null pointer that is never dereferenced
    err = lambda: lib.apa_last_error()
    # ---- apa_clip_xent_fwd_bwd(logits, labels, w, b, pooled, tatt, loss, G, dw, db, ws, ws_bytes, B, F, K, wt, gs, stream)
    clip = lambda ptrs, B, F, K: lib.apa_clip_xent_fwd_bwd(*ptrs, p, 1 << 20, B, F, K, 1.0, 1.0, None)
    ok = [p, p, None, None, p, None, p, p, None, None]
    for i in (0, 1, 4, 6, 7):                    # logits, labels, pooled, loss, G
        bad = list(ok)
        bad[i] = None
        assert clip(bad, 2, 3, 5) == INVALID and b'null' in err(), i
    assert clip([p, p, p, None, p, p, p, p, p, p], 2, 3, 5) == INVALID          # temporal attention without b
    assert clip([p, p, p, p, p, None, p, p, p, p], 2, 3, 5) == INVALID          # ... without tatt
    for B, F, K in ((0, 3, 5), (2, 0, 5), (2, 3, 0), (-1, 3, 5)):
        assert clip(ok, B, F, K) == INVALID and b'non-positive' in err(), (B, F, K)
    assert clip(ok, 1 << 20, 1 << 12, 5) == INVALID                              # B * F past 2^31
    assert lib.apa_clip_xent_workspace_bytes(1 << 20, 1 << 12, 5) == 0
    assert lib.apa_clip_xent_workspace_bytes(2, 3, 5) >= 4 * 6

    # ---- apa_attn_head_train_step_clips(clip, hooks, <apa_attn_head_train_step_ex's arguments>)
    cp = cof.ApaClipPool()
    cp.frames, cp.pooled = 4, p

    def head(clip_ptr, N, labels=p, loss=p, logits=p, G=p, P=4, K=5):
        return lib.apa_attn_head_train_step_clips(clip_ptr, None, p, p, p, p, p, p, labels, 1.0, 1.0, logits, p, p, p,
                                                  loss, G, p, None, p, p, p, p, p, 1 << 30, N, P, 256, 256, K, 1, 4, 0.5,
                                                  0, 0, 0, None)
    a = ctypes.addressof(cp)
    assert head(None, 8) == INVALID and b'null' in err()
    assert head(a, 8, labels=None) == INVALID and head(a, 8, loss=None) == INVALID and head(a, 8, G=None) == INVALID
    assert head(a, 6) == INVALID and b'whole number of clips' in err()           # N % frames
    assert head(a, 0) == INVALID and head(a, 8, P=0) == INVALID and head(a, 8, K=-3) == INVALID
    cp.frames = 0
    assert head(a, 8) == INVALID
    cp.frames, cp.pooled = 4, None
    assert head(a, 8) == INVALID and b'pooled' in err()
    cp.pooled, cp.w = p, p                                                       # temporal attention without b / tatt
    assert head(a, 8) == INVALID
    assert lib.apa_clip_step_workspace_bytes(6, 4, 4, 256, 256, 5, 1, 0) == 0
    assert lib.apa_clip_step_workspace_bytes(8, 4, 4, 256, 256, 5, 1, 0) > \
        lib.apa_attn_pool_workspace_bytes(8, 4, 256, 256, 5, 1, 0)

    # ---- apa_pose_attn_train_step_clips(clip, io, N, P, C, Cp, J, K, flags, keep_prob, seed, offset, dtype, stream)
    cp = cof.ApaClipPool()
    cp.frames, cp.pooled = 4, p
    a = ctypes.addressof(cp)
    io = cof.ApaPoseAttnStepIO()
    for name, ct in cof.ApaPoseAttnStepIO._fields_:
        setattr(io, name, p if ct is ctypes.c_void_p else (1 << 30 if ct is ctypes.c_size_t else 1.0))
    pose = lambda clip_ptr, io_ptr, N, J=16: lib.apa_pose_attn_train_step_clips(
        clip_ptr, io_ptr, N, 4, 256, 256, J, 5, 4, 0.5, 0, 0, 0, None)
    ioa = ctypes.addressof(io)
    assert pose(a, None, 8) == INVALID and pose(None, ioa, 8) == INVALID
    assert pose(a, ioa, 6) == INVALID and b'whole number of clips' in err()
    assert pose(a, ioa, 0) == INVALID and pose(a, ioa, 8, J=0) == INVALID
    io.labels = None
    assert pose(a, ioa, 8) == INVALID and b'null' in err()


CONFIGS = {
    'SL + temporal': ('framepool_train', {'USE_TEMPORAL_ATT': True}),
    'per-class + temporal': ('perclass_temporal_train', {}),
    '003 yaml + temporal': ('cfg003_temporal_train', {}),
}


def _network(case, extra_net):
    fx = rf.HeadFixture(small_path(case))
    fx.meta['net'] = dict(fx.meta['net'], **extra_net)
    return rf.build_head(fx, device='cpu')


@pytest.mark.parametrize('which', sorted(CONFIGS))
def test_fused_head_step_takes_a_network_with_the_temporal_conv(which):
    from attentionalpoolingaction_amd import deploy
    try:
        network_fn, cfg = _network(*CONFIGS[which])
        assert network_fn.temporal is not None
        assert deploy.FusedHeadStep.unsupported_reason(network_fn.head, cfg, network_fn) == ''
        fused = deploy.FusedHeadStep(network_fn, cfg)
        for n in ('temporal_weights', 'temporal_biases'):
            assert n in fused.params and n in fused.bucket.views and n in fused._written, n
            assert tuple(fused.bucket.views[n].shape) == tuple(fused.params[n].shape)
        assert fused.params['temporal_weights'] is network_fn.temporal['weights']
        assert 'temporal_weights' in fused.regularized and 'temporal_biases' not in fused.regularized
        # the regularised set is network_fn's (regularized_weights()): the conv weights, never a bias
        reg = {id(w) for w in network_fn.regularized_weights()}
        assert {id(fused.params[n]) for n in fused.regularized} == reg
    finally:
        apa_config.reset_cfg()


def test_fused_head_step_without_the_temporal_conv_is_unchanged():
    from attentionalpoolingaction_amd import deploy
    try:
        network_fn, cfg = _network('framepool_train', {})
        fused = deploy.FusedHeadStep(network_fn, cfg)
        assert list(fused.params) == ['pose_w1', 'pose_b1', 'pose_w2', 'pose_b2', 'att_weights', 'att_biases',
                                      'td_weights', 'td_biases']
        assert fused._written == ['att_weights', 'att_biases', 'td_weights', 'td_biases']
    finally:
        apa_config.reset_cfg()


def _close(got, exp, tol, what):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(exp).shape)
    exp = np.asarray(exp, dtype=np.float64)
    scale = max(float(np.abs(exp).max()) if exp.size else 0.0, 1e-3)
    err = float(np.abs(got - exp).max()) if exp.size else 0.0
    assert err <= tol * scale, '%s: max abs err %.3e > %.1e * %.3e' % (what, err, tol, scale)


@pytest.mark.parametrize('name', SMALL)
def test_oracle_matches_the_video_step_fixture(name):
    """oracle.attn_pool_oracle (frame_pooling included) driven by tests/_ref_fixture.run_oracle against what the
    reference's own code computed, at the tolerance of test_reference_fixtures_cpu.py: 1e-12, float32-stored tensors
    at storage rounding, digest-stored ones (the C = 512 case) through HeadFixture.check."""
    fx = rf.HeadFixture(small_path(name))
    assert fx.arrays['in/images'].ndim == 5
    got = rf.run_oracle(fx)
    checked = 0
    for key in fx.output_keys():
        assert key in got, 'the oracle produces no %s' % key
        if 'digest/' + key in fx.arrays:
            fx.check(key, got[key], 1e-6, '%s %s' % (fx.name, key))          # a float32 digest of float64 values
        else:
            _close(got[key], fx.arrays[key], fx.tol(key), '%s %s' % (fx.name, key))
        checked += 1
    assert checked >= 8
    assert got['out/logits'].shape[0] * fx.arrays['in/images'].shape[1] == got['out/ep/logits_beforePool'].shape[0]
    for vn in fx.meta['reg_only_grad']:
        _close(got['grad/var/' + vn], fx.meta['weight_decay'] * fx.variables[vn], 1e-12, vn)
