"""The FP8 (E4M3) feature cache without a GPU: the header constant and the layout rule, the views of Fp8Features, the
CPU restatement of the quantisation rule (custom_ops_factory.quantize_features on a CPU tensor -- the float-for-float
twin the GPU tests compare the device with), and every refusal of the arm, made before any HIP call."""
import os
import re

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
F8 = torch.float8_e4m3fn


def test_header_constant_and_layout_rule():
    header = open(os.path.join(ROOT, 'include', 'apa.h')).read()
    defs = dict(re.findall(r'#define\s+(APA_[A-Z0-9_]+)\s+(\d+)u?\b', header))
    assert int(defs['APA_DTYPE_FP8_E4M3']) == cof.APA_DTYPE_FP8_E4M3 == 2
    assert int(defs['APA_VERSION']) >= 309
    lib = cof.load_library()
    assert lib.apa_version() >= 309
    # the scales start at the first 256-byte boundary behind the codes
    assert cof.fp8_scale_offset(2, 9, 16) == 512
    for N, P, C in [(2, 9, 16), (1, 1, 256), (3, 7, 48), (32, 196, 2048), (5, 4, 2048), (1, 16, 16)]:
        want = (N * P * C + 255) // 256 * 256 + 4 * N
        assert lib.apa_fp8_features_bytes(N, P, C) == want == cof.fp8_features_bytes(N, P, C)
    assert lib.apa_fp8_features_bytes(0, 9, 16) == 0 and lib.apa_fp8_features_bytes(2, -1, 16) == 0
    assert {'apa_fp8_features_bytes', 'apa_quantize_features_fp8', 'apa_dequantize_features_fp8'} <= set(
        cof.exported_symbols())
    # torch's E4M3 is the OCP format the header promises
    bits = torch.tensor([56, 126, 127, 255], dtype=torch.uint8).view(F8).to(torch.float32)
    assert bits[0] == 1.0 and bits[1] == 448.0 and torch.isnan(bits[2]) and torch.isnan(bits[3])


def test_views_alias_one_buffer():
    f = cof.Fp8Features.empty((2, 3, 3, 16), 'cpu')
    assert f.buffer.numel() == 512 + 8 and f.shape == (2, 3, 3, 16) and f.device.type == 'cpu'
    assert f.codes.dtype == F8 and tuple(f.codes.shape) == (2, 3, 3, 16)
    assert f.scale.dtype == torch.float32 and tuple(f.scale.shape) == (2,)
    assert f.codes.data_ptr() == f.buffer.data_ptr() == f.data_ptr()
    assert f.scale.data_ptr() == f.buffer.data_ptr() + 512
    f.buffer[5] = 56
    f.buffer[512:516] = torch.tensor([0, 0, 0x80, 0x3f], dtype=torch.uint8)      # 1.0f, little endian
    assert float(f.codes.reshape(-1)[5].to(torch.float32)) == 1.0 and float(f.scale[0]) == 1.0
    flat = f.flat()
    assert flat.shape == (2, 9, 16) and flat.data_ptr() == f.data_ptr()
    # from_parts: a batch gathered from a cache that keeps codes and scales apart
    codes = torch.arange(3 * 4 * 16, dtype=torch.uint8).remainder(120).view(3, 4, 16)
    scales = torch.tensor([0.5, 2.0, 0.0])
    idx = torch.tensor([2, 0])
    g = cof.Fp8Features.from_parts(codes.view(F8)[idx], scales[idx])
    assert g.shape == (2, 4, 16) and torch.equal(g.codes.view(torch.uint8), codes[idx]) and torch.equal(g.scale, scales[idx])
    want = codes[idx].view(F8).to(torch.float32) * scales[idx][:, None, None]
    assert torch.equal(g.dequantize(), want) and g.dequantize(torch.bfloat16).dtype == torch.bfloat16
    with pytest.raises(cof.ApaError):
        cof.Fp8Features.empty((2, 3, 24), 'cpu')                   # C not a multiple of 16
    with pytest.raises(cof.ApaError):
        cof.Fp8Features(torch.zeros(100, dtype=torch.uint8), (2, 3, 3, 16))


def test_cpu_quantize_rule():
    g = torch.Generator().manual_seed(3)
    X = torch.randn(5, 6, 32, generator=g)
    X[0] = 0.0                                  # an all-zero image
    X[1] = -X[1].abs() * 37.0                   # amax is taken on |x|: a negative extreme
    X[2, 3, 7] = float('inf')                   # non-finite: reported, not encoded
    X[3] = X[3] * 1e-3
    X[4, 0, 0] = float('nan')
    f, status = cof.quantize_features(X)
    assert status.dtype == torch.int32 and status.tolist() == [0, 0, 1, 0, 1]
    assert float(f.scale[0]) == 0.0 and not f.codes[0].view(torch.uint8).any()
    for n in (2, 4):
        assert float(f.scale[n]) == 0.0 and not f.codes[n].view(torch.uint8).any()
    amax = X[1].abs().max()
    assert float(f.scale[1]) == float(amax / torch.tensor(448.0)) > 0
    assert float(f.codes[1].to(torch.float32).min()) == -448.0     # the negative extreme lands on -448
    # round trip: three mantissa bits (2^-4 relative) above the subnormals, half the smallest subnormal 2^-9 below
    for n in (1, 3):
        s = float(f.scale[n])
        dq = f.codes[n].to(torch.float32).double()
        err = (X[n].double() - s * dq).abs()
        bound = s * torch.maximum(2.0 ** -4 * dq.abs(), torch.tensor(2.0 ** -10, dtype=torch.float64))
        assert bool((err <= bound).all()), float((err - bound).max())
    assert torch.equal(f.dequantize()[3], f.codes[3].to(torch.float32) * f.scale[3])
    # a bf16 source follows the same rule on its exact fp32 values
    Xb = X[[1, 3]].to(torch.bfloat16)
    fb, sb = cof.quantize_features(Xb)
    ff, _ = cof.quantize_features(Xb.to(torch.float32))
    assert torch.equal(fb.buffer, ff.buffer) and sb.tolist() == [0, 0]
    with pytest.raises(cof.ApaError):
        cof.quantize_features(X.double())


def _fake_calls(lib):
    fake = 0x10000                       # a 16-byte aligned non-null address: nothing is dereferenced
    FROZEN = cof.APA_FLAG_FROZEN_INPUT

    def fwd(N=2, P=9, C=32, K=8, M=1, flags=0, xatt=fake, topdown=None, x=fake, ws_bytes=1 << 30):
        rc = lib.apa_attn_pool_fwd(x, xatt, fake, fake, fake, fake, fake, fake, fake, fake, topdown, fake, ws_bytes,
                                   N, P, C, C, K, M, flags, 1.0, 0, 0, 2, None)
        return rc, lib.apa_last_error()

    def bwd(dX=None, flags=FROZEN, N=2, P=9, C=32, K=8, M=1, xatt=fake, ws_bytes=1 << 30):
        rc = lib.apa_attn_pool_bwd(fake, xatt, fake, fake, fake, fake, fake, fake, fake, fake, dX,
                                   None if xatt == fake else fake, fake, fake, fake, fake, fake, ws_bytes, N, P, C, C,
                                   K, M, flags, 1.0, 0, 0, 2, None)
        return rc, lib.apa_last_error()

    def step(dX=None, flags=FROZEN, C=32, M=1, xatt=fake, ws_bytes=1 << 30):
        rc = lib.apa_attn_head_train_step(fake, xatt, fake, fake, fake, fake, fake, 1.0, 1.0, fake, fake, fake, fake,
                                          fake, fake, dX, None if xatt == fake else fake, fake, fake, fake, fake, fake,
                                          ws_bytes, 2, 9, C, C, 8, M, flags, 1.0, 0, 0, 2, None)
        return rc, lib.apa_last_error()

    def ev(flags=0, C=32, M=1, xatt=fake, ws_bytes=1 << 30):
        rc = lib.apa_attn_head_eval_step(fake, xatt, fake, fake, fake, fake, None, fake, fake, fake, fake, None, fake,
                                         fake, fake, ws_bytes, 2, 9, C, C, 8, M, flags, 2, None)
        return rc, lib.apa_last_error()
    return fake, fwd, bwd, step, ev


def test_refusals_name_their_reason_before_any_hip_call():
    """(dummy pointers: a call that got past its checks would fault -- the last accepted call below stops at the
    workspace check, still in front of the first launch)"""
    lib = cof.load_library()
    fake, fwd, bwd, step, ev = _fake_calls(lib)
    other = fake + 0x1000
    for call in (fwd, bwd, step, ev):
        # the arm is reached: with everything in order the next refusal is the workspace's, nothing was launched
        rc, err = call(ws_bytes=0)
        assert rc == -3 and b'workspace' in err, err
        for kw, word in ((dict(xatt=other), b'separate attention input'), (dict(M=8), b'per-class maps'),
                         (dict(C=24), b'multiple of 16'), (dict(flags=cof.APA_FLAG_SOFTMAX_ATT), b'APA_FLAG_SOFTMAX_ATT'),
                         (dict(flags=cof.APA_FLAG_RELU_INPUT), b'APA_FLAG_RELU_INPUT')):
            if 'flags' in kw and call in (bwd, step):
                kw = dict(flags=kw['flags'] | cof.APA_FLAG_FROZEN_INPUT)
            rc, err = call(**kw)
            assert rc == UNSUPPORTED and word in err and b'APA_DTYPE_FP8_E4M3' in err, (call.__name__, kw, rc, err)
    # a replayed mask is a training matter: the three calls that can train
    ext = cof.APA_FLAG_RNG_EXTERNAL | cof.APA_FLAG_TRAIN
    for rc, err in (fwd(flags=ext), bwd(flags=ext | cof.APA_FLAG_FROZEN_INPUT), step(flags=ext | cof.APA_FLAG_FROZEN_INPUT)):
        assert rc == UNSUPPORTED and b'APA_FLAG_RNG_EXTERNAL' in err
    rc, err = fwd(topdown=fake)
    assert rc == UNSUPPORTED and b'TopDownAttention' in err
    # a cache has no gradient: without the flag, or with a dX, the backward call and the step are invalid
    for call in (bwd, step):
        rc, err = call(dX=None, flags=0)
        assert rc == INVALID, err                                  # (the pointer check: a null dX without the flag)
        rc, err = call(dX=fake, flags=0)
        assert rc == INVALID and b'APA_FLAG_FROZEN_INPUT' in err and b'no gradient' in err
        rc, err = call(dX=fake, flags=cof.APA_FLAG_FROZEN_INPUT)
        assert rc == INVALID and b'NULL dX' in err
    rc, err = fwd(x=fake + 8, xatt=fake + 8)
    assert rc == INVALID and b'16-byte aligned' in err


def test_entry_points_that_do_not_serve_the_arm_answer_unknown_dtype():
    lib = cof.load_library()
    fake = 0x10000
    rank = cof.ApaRankMaps()
    rank.extra = 1
    import ctypes
    rc = lib.apa_attn_pool_rank_fwd(ctypes.addressof(rank), fake, fake, fake, fake, fake, fake, fake, fake, fake, fake,
                                    fake, 1 << 30, 2, 9, 32, 32, 8, 1, 0, 1.0, 0, 0, 2, None)
    assert rc == INVALID and lib.apa_last_error() == b'apa_attn_pool_rank_fwd: unknown dtype 2'
    cat = cof.ApaConcatFeat(fake, 16, fake, fake)
    rc = lib.apa_attn_pool_fwd_cat(ctypes.addressof(cat), None, fake, fake, fake, fake, fake, fake, fake, fake, fake,
                                   fake, None, fake, 1 << 30, 2, 9, 32, 32, 8, 1, 0, 1.0, 0, 0, 2, None)
    assert rc == INVALID and b'unknown dtype 2' in lib.apa_last_error()
    rc = lib.apa_pose_head_fwd(fake, fake, fake, fake, fake, fake, fake, fake, 1 << 30, 2, 9, 32, 64, 16, 2, None)
    assert rc == INVALID and lib.apa_last_error() == b'apa_pose_head_fwd: unknown dtype 2'
    rc = lib.apa_pose_att_logits_fwd(fake, fake, None, 0, 0, fake, fake, fake, fake, fake, 1 << 30, 2, 9, 32, 16, 8, 0,
                                     1.0, 0, 0, 2, None)
    assert rc == INVALID and b'unknown dtype 2' in lib.apa_last_error()
    rc = lib.apa_per_class_weight_images(fake, fake, fake, fake, fake, 1 << 30, 2, 9, 32, 32, 8, 2, None, None, None)
    assert rc == INVALID and b'unknown dtype 2' in lib.apa_last_error()
    # the quantiser's own argument checks
    q = lib.apa_quantize_features_fp8
    assert q(fake, 2, fake, fake, 2, 9, 32, None) == INVALID and b'unknown dtype 2' in lib.apa_last_error()
    assert q(fake, 0, fake, fake, 2, 9, 24, None) == UNSUPPORTED and b'multiple of 16' in lib.apa_last_error()
    assert q(None, 0, fake, fake, 2, 9, 32, None) == INVALID and q(fake, 0, fake, None, 2, 9, 32, None) == INVALID
    assert q(fake, 0, fake, fake, 0, 9, 32, None) == INVALID
    assert lib.apa_dequantize_features_fp8(fake, fake + 4, 0, 2, 9, 32, None) == INVALID


def test_python_wrappers_refuse_a_gradient_for_a_cache():
    f = cof.Fp8Features.empty((2, 9, 32), 'cpu')
    assert cof._feat_dtype(f) == cof.APA_DTYPE_FP8_E4M3
    w = torch.zeros(32, 1)
    with pytest.raises(cof.ApaError, match='no gradient'):
        cof.attn_pool_bwd(f, f, w, w, w, w, w, w, w, w)            # want_dx defaults to True
