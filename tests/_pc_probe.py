"""ctypes glue for the per-class-maps part of the test-only probe library (csrc/apa_pc_probe.hip, linked into
libapa_gemm_probe.so): the product's attentional-pooling entry points run with a host-side dispatch trace
(apa_internal.h PcTrace), the workspace carve (PcPlan and PcFusedWs), the support / geometry helpers, and the error
model tests/test_pc_paths_gpu.py adds to tests/_m1_probe.py (Bnd, contract, check, softmax_p, C_ACC, EPS32, U_BF16)
and to the operand rule of tests/_gemm_probe.py.

Error model of the per-class maps (elementwise, every stage from the tensors its kernel read):
  * operands.  bf16 features widen exactly.  With bf16 features every weight enters its product as its bf16 rounding
    (pc_prep_kernel's f32_to_bf16_bits, pc_pad_kernel's pack, or the GEMM stager: all round to nearest even, as
    torch's .to(bfloat16)); with fp32 features both operands are fp32 and the f32 MFMA is an exact FMA chain.  A
    product of two bf16 values has 16 significant bits: exact in fp32.
  * dropout.  The fused kernels zero the dropped A fragments and scale the fp32 ACCUMULATOR by fl32(1 / keep): one
    rounding of the scale, one of the product -- inside C_ACC (below).  The generic bf16 path materialises
    bf16(fl32(x * fl32(m * fl32(1 / keep)))), which torch reproduces bit for bit in fp32: exact equality is asserted and
    the products downstream take that tensor.  The scalar-staging forms (drop_a 1 / 2) form the same fp32 value and,
    on the bf16 MFMA, round it to bf16: reproduced the same way, no error term.
  * a contraction of length L accumulated in fp32, in any order and with any split: C_ACC * (L + 8) * 2^-24 * mag,
    mag the same expression on absolute values (tests/_m1_probe.py).  The fused forward product sums four k-step
    partials through LDS, pc_bwd_dw_kernel leaves S split partials that pc_dw_reduce_kernel adds in order, the folded
    activation pass leaves two partial rows per 32-row block (lpart) that pc_logit_from_partials adds in block order:
    all of these are fp32 chains over the SAME terms, at most L + S (L + 4, P + P / 32 + 2) additions deep, and
    S <= 32 <= 3 L, so C_ACC = 4 covers them with the stated L: L = C (Ca) for Z / T, P for the logits, R for dW and
    the bias gradients, 2 Kp (the concatenated contraction) or Kp for dX.
  * dT = (G / P) att and dZ = act'((G / P) T) are formed in fp32 from fl32(1 / P): three roundings, 4 * 2^-24 |ref|;
    the softmax form a (dA - sum_p a dA) carries a contraction over P.  They are STORED as bf16 with bf16 features
    (one U_BF16), and it is the stored value that dW and dX are computed from, so the test reads it back from the
    workspace and starts the next stage from it.  dbt / dba are sums of the unrounded fp32 values.
  * dX is a bf16 store with bf16 features (U_BF16 |ref|).  The two-product form stores the first product in dX's dtype
    and the second launch reads it back (beta = 1): one more rounding of the first product's magnitude.
  * a relu gate is taken from the kernel's own att (`att > 0`), so no element is ambiguous.  Where the forward kernel
    does not store Z (FOLD), att is held to the float64 Z under Z's own bound: relu is 1-Lipschitz, so
    |relu(Z_kernel) - relu(Z_ref)| <= |Z_kernel - Z_ref|, and an element whose Z lies within the bound of zero passes
    as 0 or as Z without being left out.
Each output's bound must stay below 1 % of its max |ref| (`_m1_probe.check`; excepted, as there: dba and dWa under the
spatial softmax, whose columns cancel to zero -- there the elementwise bound alone is asserted).
"""
import ctypes

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp

PC_PROBE_VERSION = 1
PC_SYMBOLS = ('apa_probe_pc_version', 'apa_probe_pc_trace_size', 'apa_probe_pc_plan', 'apa_probe_pc_support',
              'apa_probe_pc_psplit', 'apa_probe_pc_geometry', 'apa_probe_pc_wide_serves', 'apa_probe_pc_fwd_ex',
              'apa_probe_pc_bwd_ex', 'apa_probe_pc_train_step_ex', 'apa_probe_pc_eval_step',
              'apa_probe_pc_weight_images')

# PcTrace enum values (csrc/apa_internal.h)
PATHS = {0: 'none', 1: 'fused', 2: 'generic'}
PREPS = {0: 'none', 1: 'weights', 2: 'bits', 3: 'both'}
LOGITS = {0: 'none', 1: 'finish', 2: 'dx', 3: 'fwd_act'}
XENTS = {0: 'none', 1: 'fwd_act', 2: 'dx', 3: 'bwd_act', 4: 'own'}
ACTS = {0: 'none', 1: 'f32', 2: 'bf16', 3: 'folded'}
DXS = {0: 'none', 1: 'fused', 2: 'mid_gemm', 3: 'plain_gemm', 4: 'wide', 5: 'two'}
WAS = {0: 'none', 1: 'dx_beta1', 2: 'dxatt'}
DWS = {0: 'none', 1: 'fused', 2: 'twin_gemm'}
TAILS = {0: 'none', 1: 'dw_tail', 2: 'colsum'}
_ENUMS = {'path_fwd': PATHS, 'path_bwd': PATHS, 'prep_fwd': PREPS, 'prep_bwd': PREPS, 'prep_wimg': PREPS,
          'logits': LOGITS, 'xent': XENTS, 'fwd_act': ACTS, 'bwd_act': ACTS, 'dx': DXS, 'wa_to': WAS, 'dw': DWS,
          'tail': TAILS}
_INTS = ('phase', 'path_fwd', 'path_bwd', 'prep_fwd', 'prep_bwd', 'prep_wimg', 'pad_fwd', 'pad_segs_fwd',
         'pad_drop_fwd', 'pad_bwd', 'pad_segs_bwd', 'pad_drop_bwd', 'cat', 'fast', 'reuse_fwd', 'zt', 'zt_train',
         'zt_fold', 'check_tag', 'fwd_act', 'fwd_act_xe', 'topdown', 'logits', 'xent', 't_drop_a', 'bwd_act', 'ps',
         'ldg', 'dx', 'upb', 'dx_splits', 'rbs', 'mid_bits', 'dx_drop_c', 'wa_to', 'dw', 'dw_S', 'dw_rows',
         'dw_ctiles', 'dw_drop_a', 'tail', 'tail_nrows', 'next_bits', 'rng_bump', 'aux', 'wimg_cat', 'wimg_fused',
         'wimg_maps')
GEMMS = ('g_z', 'g_t', 'g_dwt', 'g_dwa', 'g_dx', 'g_dxa')


class _GemmTrace(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ('kind', 'splits', 'k_per_split', 'mt', 'twin', 'reduce')]


class PcTrace(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in _INTS] + [(n, _GemmTrace) for n in GEMMS]

    def as_dict(self):
        d = {}
        for n in _INTS:
            v = getattr(self, n)
            d[n] = _ENUMS[n][v] if n in _ENUMS else v
        for n in GEMMS:
            g = getattr(self, n)
            d[n + '_kind'], d[n + '_twin'] = gp.KINDS[g.kind], gp.TWINS[g.twin]
            d[n + '_splits'], d[n + '_reduce'] = g.splits, gp.REDUCES[g.reduce]
        return d


def merge(*traces):
    """The fields each call set (a forward and a backward call fill different ones)."""
    out = {}
    for t in traces:
        for k, v in t.as_dict().items():
            if v not in (0, 'none') or k not in out:
                out[k] = v
    del out['phase']
    return out


_lib = None
_WRAPPED = (('apa_probe_pc_fwd_ex', 'apa_attn_pool_fwd_ex'), ('apa_probe_pc_bwd_ex', 'apa_attn_pool_bwd_ex'),
            ('apa_probe_pc_train_step_ex', 'apa_attn_head_train_step_ex'),
            ('apa_probe_pc_eval_step', 'apa_attn_head_eval_step'),
            ('apa_probe_pc_weight_images', 'apa_per_class_weight_images'))


def load_pc_probe():
    """The probe library with the product entry points bound (cof signatures) and the per-class wrappers."""
    global _lib
    if _lib is None:
        gp.load_probe()
        lib = cof.load_library(gp.PROBE_PATH)
        sig = cof._SIGNATURES
        lib.apa_probe_pc_version.restype = ctypes.c_int64
        assert lib.apa_probe_pc_version() == PC_PROBE_VERSION
        lib.apa_probe_pc_trace_size.restype = ctypes.c_int64
        lib.apa_probe_pc_plan.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p]
        lib.apa_probe_pc_plan.restype = None
        lib.apa_probe_pc_support.argtypes = [ctypes.c_int] * 7
        lib.apa_probe_pc_psplit.argtypes = [ctypes.c_int] * 4
        lib.apa_probe_pc_geometry.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        lib.apa_probe_pc_geometry.restype = None
        lib.apa_probe_pc_wide_serves.argtypes = [ctypes.c_int] * 3
        for probe, prod in _WRAPPED:
            fn = getattr(lib, probe)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p] + list(sig[prod][1])
        assert lib.apa_probe_pc_trace_size() == ctypes.sizeof(PcTrace)
        _lib = lib
    return _lib


PLAN_FIELDS = ('R', 'Kp', 'off_wap', 'off_wtp', 'off_bap', 'off_z', 'off_dt', 'off_dz', 'off_pdbt', 'off_pdba',
               'off_gemm', 'gemm_half', 'off_xd', 'off_bits', 'off_fused', 'total',
               'WcatT', 'Wcat2', 'bcat', 'dTdZ', 'partial', 'maskbits', 'lpart', 'bits_tag', 'fused_end')


def plan(N, P, C, Ca, K, dtype):
    """The workspace carve of csrc/apa_pc.hip pc_plan and, for its fused part, of pc_fused_carve (byte offsets from
    the workspace base)."""
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    load_pc_probe().apa_probe_pc_plan(N, P, C, Ca, K, dtype, out)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def support(N, P, C, Ca, K, dtype, act):
    """(pc_fused_supported for aligned X == Xatt, pc_fused_dx_supported(P, act))."""
    v = int(load_pc_probe().apa_probe_pc_support(N, P, C, Ca, K, dtype, act))
    return bool(v & 1), bool(v & 2)


def psplit(N, kgroups, P, act):
    return int(load_pc_probe().apa_probe_pc_psplit(N, kgroups, P, act))


def geometry(R, C):
    """upb, dx_splits, rbs of pc_bwd_dx_kernel; dw_S, dw_rows, dw_ctiles of pc_bwd_dw_kernel."""
    out = (ctypes.c_int * 6)()
    load_pc_probe().apa_probe_pc_geometry(R, C, out)
    return dict(zip(('upb', 'dx_splits', 'rbs', 'dw_S', 'dw_rows', 'dw_ctiles'), (int(v) for v in out)))


def wide_serves(M, N, K):
    """gemm_bf16_wide_serves (asks the device for its CU count)."""
    return bool(load_pc_probe().apa_probe_pc_wide_serves(M, N, K))
