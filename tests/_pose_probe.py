"""ctypes glue for the pose-head part of the test-only probe library (csrc/apa_pose_probe.hip, linked into
libapa_gemm_probe.so): the product's PoseLogits entry points run with a host-side dispatch trace (apa_internal.h
PoseTrace), the workspace carve, and the two error terms tests/test_pose_paths_gpu.py adds to the model of
tests/_m1_probe.py (Bnd, contract, check, C_ACC, EPS32, U_BF16) and the operand rule of tests/_gemm_probe.py.

Error model of the pose head (elementwise, every stage from the tensors its kernel read):
  * operands: bf16 features widen exactly.  A product with one bf16 operand runs on the bf16 MFMA and the staging
    code rounds the fp32 operand to bf16, to nearest even (tests/_gemm_probe.py): with bf16 features W1 enters the
    Ppre and dX products, W2 the Pl product and dPl the dW2 product of the GEMM path as `.to(bfloat16)` values;
    pose_pl_kernel rounds W2 the same way (f32_to_bf16_bits / pack_bf16x2).  fp32 x fp32 is exact fp32 FMA;
  * a contraction of length L accumulated in fp32: C_ACC * (L + 8) * 2^-24 * mag (tests/_m1_probe.py);
  * SPLIT2 / SPLIT1 -- pose_bwd_rows_mfma_kernel.  split_bf16x8 writes an fp32 operand x as hi + lo,
    hi = bf16(x) (|x - hi| <= 2^-9 |x|: bf16 keeps 8 significant bits, round to nearest) and
    lo = bf16(x - hi) (|x - hi - lo| <= 2^-9 |x - hi| <= 2^-18 |x|).  So each split operand carries a relative
    representation error of at most 2^-18.  Phase 2 (dPpre) multiplies [W2hi | W2hi] . [dPlhi ; dPllo] +
    [W2lo | 0] . [dPlhi ; 0] = W2hi dPlhi + W2hi dPllo + W2lo dPlhi: against (W2hi + W2lo)(dPlhi + dPllo) the term
    W2lo dPllo is missing, |W2lo| <= 2^-9 |W2|, |dPllo| <= 2^-9 |dPl|: 2^-18 |W2| |dPl|.  Together with the two
    representation errors: SPLIT2 = 3 * 2^-18 of mag.  Phase 1 (dW2, dWa) multiplies (dPlhi + dPllo) by the bf16 tile of
    Ppre, which is exact: only dPl's (dZ's) representation error remains, SPLIT1 = 2^-18 of mag.  The MFMA products of
    two bf16 values are exact in fp32 and accumulate like any fp32 chain (the C_ACC term);
  * a bf16 store adds U_BF16 * |ref| (`check(..., bf16=True)`).
"""
import ctypes

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp

SPLIT1 = 2.0 ** -18
SPLIT2 = 3 * 2.0 ** -18

POSE_PROBE_VERSION = 1
POSE_SYMBOLS = ('apa_probe_pose_version', 'apa_probe_pose_trace_size', 'apa_probe_pose_plan',
                'apa_probe_pose_pool_offsets', 'apa_probe_pose_head_fwd', 'apa_probe_pose_head_bwd',
                'apa_probe_pose_head_bwd_rank1ext', 'apa_probe_pose_attn_train_step')

# PoseTrace enum values (csrc/apa_internal.h)
W1S = {0: 'none', 1: 'bf16_copy', 2: 'f32', 3: 'reused', 4: 'shadow'}
PLS = {0: 'none', 1: 'fast', 2: 'gemm'}
ROWS = {0: 'none', 1: 'mfma', 2: 'valu', 3: 'dppre'}
FORMS = {0: 'none', 1: 'plain', 2: 'ext', 3: 'rank1'}
DW2S = {0: 'none', 1: 'rows', 2: 'gemm', 3: 'memset'}
COLSUMS = {0: 'none', 1: 'tail', 2: 'own'}
_ENUMS = {'w1_fwd': W1S, 'w1_bwd': W1S, 'pl': PLS, 'rows': ROWS, 'form': FORMS, 'dw2': DW2S, 'colsum': COLSUMS}


class PoseTrace(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        'w1_fwd', 'pl', 'pl_ks', 'pl_fused', 'pl_w2t', 'rows', 'wpb', 'ngrp', 'G', 'rpb', 'form', 'wa', 'jm',
        'dw2', 'colsum', 'dw1_splits', 'w1_bwd', 'dx_beta')]

    def as_dict(self):
        d = {}
        for n, _ in self._fields_:
            v = getattr(self, n)
            d[n] = _ENUMS[n][v] if n in _ENUMS else v
        return d


_lib = None


def load_pose_probe():
    """The probe library with the product entry points bound (cof signatures) and the pose wrappers."""
    global _lib
    if _lib is None:
        gp.load_probe()
        lib = cof.load_library(gp.PROBE_PATH)
        sig = cof._SIGNATURES
        lib.apa_probe_pose_version.restype = ctypes.c_int64
        assert lib.apa_probe_pose_version() == POSE_PROBE_VERSION
        lib.apa_probe_pose_trace_size.restype = ctypes.c_int64
        lib.apa_probe_pose_plan.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
        lib.apa_probe_pose_plan.restype = None
        lib.apa_probe_pose_pool_offsets.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
        lib.apa_probe_pose_pool_offsets.restype = None
        for probe, prod in (('apa_probe_pose_head_fwd', 'apa_pose_head_fwd'),
                            ('apa_probe_pose_head_bwd', 'apa_pose_head_bwd'),
                            ('apa_probe_pose_head_bwd_rank1ext', 'apa_pose_head_bwd_rank1ext'),
                            ('apa_probe_pose_attn_train_step', 'apa_pose_attn_train_step')):
            fn = getattr(lib, probe)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p] + list(sig[prod][1])
        assert lib.apa_probe_pose_trace_size() == ctypes.sizeof(PoseTrace)
        _lib = lib
    return _lib


PLAN_FIELDS = ('R', 'nchunks', 'off_dppre', 'off_partial', 'off_gemm', 'off_w1b', 'off_lpart', 'total')


def plan(N, P, C, Cp, J, dtype):
    """The workspace carve of csrc/apa_pose_head.hip pose_plan (byte offsets)."""
    out = (ctypes.c_int64 * 8)()
    load_pose_probe().apa_probe_pose_plan(N, P, C, Cp, J, dtype, out)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def pool_offsets(N, P, C, Ca, K):
    """(off_dz, off_maskbits) of the pooling workspace (csrc/apa_m1.hip m1_plan)."""
    out = (ctypes.c_int64 * 2)()
    load_pose_probe().apa_probe_pose_pool_offsets(N, P, C, Ca, K, out)
    return int(out[0]), int(out[1])
