"""Host side of the paired M == 1 streaming passes (tests/test_m1_paired_rows_gpu.py): the row-count rule of
m1_call_fill (csrc/apa_m1.hip) -- nblk / 2 partial rows for a forward call with fp32 features on the stream family
with an even S and no softmax in the pooling kernel, nblk everywhere else (bf16, every backward call, the other
families) -- and that the plan and the workspace total are what
m1_plan gave before.  Everything runs m1_call_fill on the host through the test-only probe library; nothing is launched."""
import ctypes

import pytest

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _m1_probe as mp
from tests.test_m1_fold_cpu import _total_by_hand

F32, BF16, FP8 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16, cof.APA_DTYPE_FP8_E4M3
# which pass takes the paired form, by feature type (m1_call_fill; measured: profiles/paired_rows_summary.md)
PAIR_FWD = {F32: True, BF16: False}
PAIR_BWD = {F32: False, BF16: False}
RELU, SOFTMAX, TRAIN = cof.APA_FLAG_RELU_ATT, cof.APA_FLAG_SOFTMAX_ATT, cof.APA_FLAG_TRAIN


def _rows(bwd, same, unpaired, N, P, C, Ca, K, flags, keep, dt):
    lib = mp.load_m1_probe()
    lib.apa_probe_m1_call_rows.argtypes = [ctypes.c_int] * 8 + [ctypes.c_uint, ctypes.c_float, ctypes.c_int,
                                                               ctypes.c_void_p]
    lib.apa_probe_m1_call_rows.restype = ctypes.c_int
    out = (ctypes.c_int64 * 4)()
    rc = lib.apa_probe_m1_call_rows(bwd, same, unpaired, N, P, C, Ca, K, flags, keep, dt, out)
    assert rc == 0, lib.apa_last_error()
    return [int(v) for v in out]


# N, P, C, K, dtype -> S, nblk by hand (S = round(512 / N) clamped to [1, min(P / 4, 256)]); paired: even S, stream
SHAPES = [
    (32, 196, 2048, 393, F32, 16, 512, True),
    (32, 196, 2048, 393, BF16, 16, 512, True),
    (2, 9, 2048, 20, F32, 2, 4, True),
    (2, 26, 2048, 20, BF16, 6, 12, True),
    (3, 25, 1024, 20, F32, 6, 18, True),
    (2, 9, 4096, 20, F32, 2, 4, True),
    (2, 12, 2048, 20, F32, 3, 6, False),          # odd S
    (512, 196, 2048, 393, F32, 1, 512, False),    # S = 1: one block per image, as before
    (170, 196, 2048, 100, F32, 3, 510, False),
    (40, 36, 512, 51, F32, 9, 360, False),        # per-pixel family, odd S
    (64, 36, 512, 51, F32, 8, 512, False),        # per-pixel family, even S: its own rows
    (32, 36, 40, 20, F32, 9, 288, False),         # generic family
    (64, 64, 40, 20, F32, 8, 512, False),         # generic family, even S
]


@pytest.mark.parametrize('N,P,C,K,dt,S,nblk,paired', SHAPES)
def test_row_count_rule(N, P, C, K, dt, S, nblk, paired):
    assert mp.plan(N, P, C, C, K)[0::2] == (S, nblk)
    total = _total_by_hand(N, P, C, K, nblk)
    assert cof.load_library().apa_attn_pool_workspace_bytes(N, P, C, C, K, 1, 0) == total
    for bwd in (0, 1):
        half = nblk // 2 if paired and (PAIR_BWD if bwd else PAIR_FWD)[dt] else nblk
        for flags, keep in ((0, 1.0), (TRAIN | RELU, 0.2), (cof.APA_FLAG_FROZEN_INPUT, 1.0)):
            assert _rows(bwd, 1, 0, N, P, C, C, K, flags, keep, dt) == [half, nblk, S, total]
            # forced off (the probe's comparison run): one row per logical block, same plan
            assert _rows(bwd, 1, 1, N, P, C, C, K, flags, keep, dt) == [nblk, nblk, S, total]
        # softmax attention keeps full rows: its (m, l, acc) merge is the finalize kernel's
        assert _rows(bwd, 1, 0, N, P, C, C, K, SOFTMAX | TRAIN, 0.2, dt) == [nblk, nblk, S, total]


def test_row_count_with_a_separate_attention_input():
    """Xatt != X: the forward pooling pass applies no activation (att is final) and is paired whatever the attention
    was, softmax included; the backward streaming pass writes no rows, and the GEMV's partials keep their own count"""
    N, P, C, Ca, K = 32, 196, 2048, 768, 393
    S, _, nblk, _ = mp.plan(N, P, C, Ca, K)
    assert (S, nblk) == (16, 512)
    for flags in (0, RELU, SOFTMAX):
        assert _rows(0, 0, 0, N, P, C, Ca, K, flags, 1.0, BF16)[:3] == [nblk // 2 if PAIR_FWD[BF16] else nblk, nblk, S]
        assert _rows(1, 0, 0, N, P, C, Ca, K, flags, 1.0, BF16)[:3] == [nblk, nblk, S]
        assert _rows(0, 0, 0, N, P, C, Ca, K, flags, 1.0, F32)[:3] == [nblk // 2 if PAIR_FWD[F32] else nblk, nblk, S]
        assert _rows(1, 0, 0, N, P, C, Ca, K, flags, 1.0, F32)[:3] == [nblk, nblk, S]


def test_relu_input_is_paired():
    fl = cof.APA_FLAG_RELU_INPUT | TRAIN
    assert _rows(0, 1, 0, 2, 9, 2048, 2048, 20, fl, 0.5, F32)[:2] == [2 if PAIR_FWD[F32] else 4, 4]
    assert _rows(1, 1, 0, 2, 9, 2048, 2048, 20, fl, 0.5, BF16)[:2] == [2 if PAIR_BWD[BF16] else 4, 4]


def test_fp8_and_rank_calls_keep_one_row_per_logical_block():
    """the FP8 family writes its own rows; the rank-R entry points fill the same descriptor at stream widths (C = 2048,
    even S) but run their own kernels and reset the count (m1_call_full_rows)"""
    N, P, C, K = 32, 196, 2048, 51
    for bwd in (0, 1):
        assert _rows(bwd, 1, 0, N, P, C, C, K, cof.APA_FLAG_FROZEN_INPUT, 1.0, FP8)[:3] == [512, 512, 16]
        for dt in (F32, BF16):
            assert _rows(bwd, 1, 2, N, P, C, C, K, TRAIN, 0.5, dt)[:3] == [512, 512, 16]
