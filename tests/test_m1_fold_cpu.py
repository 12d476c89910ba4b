"""Host side of the folded M == 1 forward (tests/test_m1_fold_gpu.py): the fold is a choice made inside m1_forward,
so for its shapes the workspace plan, what m1_call_fill resolves and what it refuses stay what they were.  Everything
here runs m1_plan / m1_call_fill on the host through the test-only probe library; nothing is launched."""
import ctypes

import pytest

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _m1_probe as mp

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
APA_ERR_UNSUPPORTED = -2    # include/apa.h
POOL = {'stream': 1, 'vec': 2, 'generic': 3}

# N, P, C, K, dtype -> S, ppb, nblk by hand: S = round(512 / N) clamped to [1, min(P / 4, 256)], ppb = ceil(P / S)
SHAPES = [
    (3, 49, 1024, 16, F32, (12, 5, 36), 'stream'),
    (9, 196, 2048, 393, F32, (49, 4, 441), 'stream'),
    (33, 49, 2048, 393, F32, (12, 5, 396), 'stream'),
    (32, 196, 2048, 393, F32, (16, 13, 512), 'stream'),
    (32, 196, 2048, 393, BF16, (16, 13, 512), 'stream'),
    (40, 36, 512, 51, F32, (9, 4, 360), 'vec'),
    (8, 196, 2048, 393, F32, (49, 4, 392), 'stream'),
    (128, 16, 1024, 51, F32, (4, 4, 512), 'stream'),
]


def _up(x):
    return (x + 255) // 256 * 256


def _total_by_hand(N, P, C, K, nblk):
    """The carve of m1_plan (csrc/apa_m1.hip), region by region, Ca == C."""
    gemm = max(16 * N * max(K, C) * 4, (C // 64) * N * K * 4 if C % 64 == 0 else 0)
    regions = [nblk * C * 4, nblk * 16, nblk * C * 4, (nblk + N) * 4, N * C * 4, N * P * 4, gemm, N * P * 4,
               N * P * 256 * ((C // 256 + 7) // 8)]
    return sum(_up(r) for r in regions)


def _fill(bwd, loss_done, same, N, P, C, Ca, K, flags, keep, dt):
    lib = mp.load_m1_probe()
    lib.apa_probe_m1_call_fill.argtypes = [ctypes.c_int] * 8 + [ctypes.c_uint, ctypes.c_float, ctypes.c_int,
                                                               ctypes.c_void_p]
    lib.apa_probe_m1_call_fill.restype = ctypes.c_int
    out = (ctypes.c_int64 * 10)()
    rc = lib.apa_probe_m1_call_fill(bwd, loss_done, same, N, P, C, Ca, K, flags, keep, dt, out)
    return rc, [int(v) for v in out], lib


@pytest.mark.parametrize('N,P,C,K,dt,plan,pool', SHAPES)
def test_plan_and_call_fill_of_the_fold_shapes(N, P, C, K, dt, plan, pool):
    S, ppb, nblk = plan
    assert mp.plan(N, P, C, C, K)[:3] == plan
    total = _total_by_hand(N, P, C, K, nblk)
    prod = cof.load_library()
    assert prod.apa_attn_pool_workspace_bytes(N, P, C, C, K, 1, 0) == total
    for bwd in (0, 1):
        for flags, keep in ((0, 1.0), (cof.APA_FLAG_TRAIN | cof.APA_FLAG_RELU_ATT, 0.2)):
            rc, out, lib = _fill(bwd, 0, 1, N, P, C, C, K, flags, keep, dt)
            assert rc == 0, lib.apa_last_error()
            assert out[:3] == [S, ppb, nblk] and out[4] == total and out[9] == 0
            assert out[5] == POOL[pool]
            assert out[6] == bwd               # the small-K backward route serves every one of these (C, K)
            assert out[7] == int(keep < 1.0) and out[8] == 1
    # the one-call step's backward half (loss folded by the forward half) is served too
    rc, out, lib = _fill(1, 1, 1, N, P, C, C, K, cof.APA_FLAG_TRAIN, 0.2, dt)
    assert rc == 0, lib.apa_last_error()


def test_call_fill_refusals_are_unchanged():
    N, P, C, K = 32, 196, 2048, 393
    # the forward half of a call never carries a folded loss: there is no head kernel behind it
    rc, _, lib = _fill(0, 1, 1, N, P, C, C, K, 0, 1.0, F32)
    assert rc == APA_ERR_UNSUPPORTED
    assert lib.apa_last_error().decode() == 'attn_pool M=1: fused loss path without the head kernel (internal)'
    # relu-on-load exists in the streaming family only
    rc, _, lib = _fill(0, 0, 1, 40, 36, 512, 512, 51, cof.APA_FLAG_RELU_INPUT, 1.0, F32)
    assert rc == APA_ERR_UNSUPPORTED
    assert lib.apa_last_error().decode() == ('attn_pool M=1: APA_FLAG_RELU_INPUT needs Xatt == X and C in '
                                             '{1024,2048,4096} (f32) / 2048 (bf16)')
    # ... and needs Xatt == X
    rc, _, lib = _fill(0, 0, 0, N, P, C, 768, K, cof.APA_FLAG_RELU_INPUT, 1.0, F32)
    assert rc == APA_ERR_UNSUPPORTED
    # rank-1 dXatt past the register-resident GEMV (257 fp32 vectors per attention row)
    rc, _, lib = _fill(1, 0, 0, N, P, C, 1028, K, cof.APA_FLAG_DXATT_RANK1, 1.0, F32)
    assert rc == APA_ERR_UNSUPPORTED
    assert lib.apa_last_error().decode() == ('attn_pool M=1: APA_FLAG_DXATT_RANK1: Ca=1028 not served by the '
                                             'register-resident GEMV')
    # the internal forcing bit of the forward (1 << 27) refuses nothing
    rc, _, lib = _fill(0, 0, 1, N, P, C, C, K, 1 << 27, 1.0, F32)
    assert rc == 0, lib.apa_last_error()
