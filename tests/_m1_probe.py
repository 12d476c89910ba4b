"""ctypes glue for the M == 1 half of the test-only probe library (csrc/apa_m1_probe.hip, linked into
libapa_gemm_probe.so): the product's attentional-pooling entry points run with a host-side dispatch trace
(apa_internal.h M1Trace), the plan and support helpers, the template instance the FP8 and the rank-R launchers pick for a
width (fp8_instance / rank_instance: the functions those launchers call), and the float64 error model that
tests/test_m1_paths_gpu.py compares the kernels with.

Error model (elementwise; `Bnd` carries a float64 reference and an absolute bound side by side):
  * every operand the kernels read is exact in float64 (bf16 features widen exactly; fp32 dropout scaling
    x * (1 / keep) is one more rounding, inside C_ACC);
  * a contraction of length L accumulated in fp32 (any order, any split): |err| <= C_ACC * (L + 8) * 2^-24 * mag,
    mag the same expression on absolute values; errors of the inputs propagate through |a| eb + ea |b|;
  * softmax over the P pixels (max-shifted / on-line rescaled exp, fp32 normaliser): |dA| <= A * (2 max|dz| +
    C_ACC * (P + 16) * 2^-24); its backward A (g - sum A g) propagates the same way;
  * relu: a pre-activation within its bound of zero may gate either way -- such pixels are counted, and their
    whole contribution is added to the bound of everything downstream (in effect excluded);
  * a bf16 output adds one rounding: 2^-8 |ref|.
Each output's bound must stay below 1 % of its max |ref| (excepted: dWa and dba under softmax -- dba is identically
zero -- or the cross-entropy G, which cancel; there the elementwise bound alone is asserted): the inputs
have a positive mean and a per-pixel scale, so a dropped pixel, chunk, column or image moves an element by more.
"""
import ctypes

import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp

C_ACC = 4.0
EPS32 = 2.0 ** -24
U_BF16 = 2.0 ** -8

M1_PROBE_VERSION = 1
M1_SYMBOLS = ('apa_probe_m1_version', 'apa_probe_m1_trace_size', 'apa_probe_m1_plan', 'apa_probe_m1_support',
              'apa_probe_m1f_instance', 'apa_probe_m1r_instance', 'apa_probe_m1_fwd_ex',
              'apa_probe_m1_bwd_ex', 'apa_probe_m1_fwd_cat', 'apa_probe_m1_bwd_cat', 'apa_probe_m1_train_step_ex',
              'apa_probe_m1_eval_step')

# M1Trace enum values (csrc/apa_internal.h)
POOLS = {0: 'none', 1: 'stream', 2: 'vec', 3: 'generic', 4: 'fp8'}
LOGITS = {0: 'none', 1: 'xent', 2: 'xent_probs', 3: 'logits2', 5: 'sgemm'}   # (4: the retired partial-logits form)
HEADS = {0: 'none', 1: 'tiles', 2: 'rows', 3: 'small', 4: 'sgemm'}
GEMVS = {0: 'none', 1: 'bwd2', 2: 'bwd2_rank1', 3: 'bwd'}
REDUCES = {0: 'none', 1: 'colsum', 2: 'bwd_reduce'}
_ENUMS = {'pool_fwd': POOLS, 'pool_bwd': POOLS, 'logits': LOGITS, 'head': HEADS, 'gemv': GEMVS,
          'reduce': REDUCES}

# support bits of apa_probe_m1_support
SUP_STREAM, SUP_VEC, SUP_GENERIC, SUP_LOGITS2, SUP_SMALL, SUP_HEAD = 1, 2, 4, 8, 16, 32

class M1Trace(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        'pool_fwd', 'fwd_w', 'fwd_pix', 'pool_bwd', 'bwd_w', 'bwd_pix', 'fused', 'keep_bits', 'relu_input',
        'S', 'ppb', 'nblk', 'cw', 'logits', 'logits_nv4', 'logits_nsub', 'head', 'head_ug', 'head_mv',
        'gemv', 'reduce', 'rng_bump', 'cat_fwd', 'cat_bwd')]

    def as_dict(self):
        d = {}
        for n, _ in self._fields_:
            v = getattr(self, n)
            d[n] = _ENUMS[n][v] if n in _ENUMS else v
        return d


def merge(*traces):
    """The fields each call set (a forward and a backward call fill different ones)."""
    out = {}
    for t in traces:
        for k, v in t.as_dict().items():
            if v not in (0, 'none') or k not in out:
                out[k] = v
    return out


_lib = None


def load_m1_probe():
    """The probe library with every product entry point bound (cof signatures) and the M == 1 wrappers."""
    global _lib
    if _lib is None:
        gp.load_probe()                                   # asserts the GEMM half's version
        lib = cof.load_library(gp.PROBE_PATH)             # its own copy of the product entry points
        sig = cof._SIGNATURES
        lib.apa_probe_m1_version.restype = ctypes.c_int64
        assert lib.apa_probe_m1_version() == M1_PROBE_VERSION
        lib.apa_probe_m1_trace_size.restype = ctypes.c_int64
        lib.apa_probe_m1_plan.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
        lib.apa_probe_m1_plan.restype = None
        lib.apa_probe_m1_support.argtypes = [ctypes.c_int] * 4
        lib.apa_probe_m1f_instance.argtypes = [ctypes.c_int]
        lib.apa_probe_m1r_instance.argtypes = [ctypes.c_int] * 2
        for probe, prod in (('apa_probe_m1_fwd_ex', 'apa_attn_pool_fwd_ex'),
                            ('apa_probe_m1_bwd_ex', 'apa_attn_pool_bwd_ex'),
                            ('apa_probe_m1_fwd_cat', 'apa_attn_pool_fwd_cat'),
                            ('apa_probe_m1_bwd_cat', 'apa_attn_pool_bwd_cat'),
                            ('apa_probe_m1_train_step_ex', 'apa_attn_head_train_step_ex'),
                            ('apa_probe_m1_eval_step', 'apa_attn_head_eval_step')):
            fn = getattr(lib, probe)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p] + list(sig[prod][1])
        assert lib.apa_probe_m1_trace_size() == ctypes.sizeof(M1Trace)
        _lib = lib
    return _lib


def plan(N, P, C, Ca, K):
    """(S, ppb, nblk, lsplits) of csrc/apa_m1.hip m1_plan."""
    out = (ctypes.c_int64 * 4)()
    load_m1_probe().apa_probe_m1_plan(N, P, C, Ca, K, out)
    return tuple(int(v) for v in out)


def support(N, C, K, dtype):
    return int(load_m1_probe().apa_probe_m1_support(N, C, K, dtype))


def fp8_instance(C):
    """NV of the FP8 streaming kernels' instance for C, from the function their launchers call (0: C is refused)."""
    return int(load_m1_probe().apa_probe_m1f_instance(C))


def rank_instance(C, dtype):
    """NVL of the rank-R kernels' instance for (C, dtype), from the function their launchers call (0: none)."""
    return int(load_m1_probe().apa_probe_m1r_instance(C, dtype))


# ------------------------------------------------------------------------------------------ error model
class Bnd:
    """A float64 reference value with an elementwise absolute error bound."""

    def __init__(self, ref, err=None):
        self.ref = ref
        self.err = torch.zeros_like(ref) if err is None else err

    def __add__(self, o):
        return Bnd(self.ref + o.ref, self.err + o.err)

    def scale(self, s):
        return Bnd(self.ref * s, self.err * abs(s))

    def mul(self, o):
        """elementwise product (broadcasting), one fp32 rounding."""
        ref = self.ref * o.ref
        mag = (self.ref.abs() + self.err) * (o.ref.abs() + o.err)
        return Bnd(ref, self.err * o.ref.abs() + self.ref.abs() * o.err + self.err * o.err + EPS32 * mag)

    def rounded(self, n=1):
        return Bnd(self.ref, self.err + n * EPS32 * (self.ref.abs() + self.err))


def contract(eq, a, b, L):
    """torch.einsum(eq) of two Bnd operands, accumulated in fp32 over L terms."""
    ref = torch.einsum(eq, a.ref, b.ref)
    mag = torch.einsum(eq, a.ref.abs() + a.err, b.ref.abs() + b.err)
    prop = torch.einsum(eq, a.err, b.ref.abs()) + torch.einsum(eq, a.ref.abs() + a.err, b.err)
    return Bnd(ref, C_ACC * (L + 8) * EPS32 * mag + prop)


def softmax_p(z):
    """softmax over the last axis (the P pixels of one image)."""
    A = torch.softmax(z.ref, dim=-1)
    P = z.ref.shape[-1]
    ez = z.err.amax(dim=-1, keepdim=True)
    return Bnd(A, A * (2 * ez + C_ACC * (P + 16) * EPS32))


def tolerance(b, bf16=False):
    """the elementwise tolerance `check` asserts: err (+ 2^-8 |ref| for a bf16 output)."""
    return b.err + (U_BF16 * b.ref.abs() if bf16 else 0.0)


def check(got, b, what, *, bf16=False, ambiguous=None, zero_ref=False):
    """|got - ref| <= err (+ 2^-8 |ref| for a bf16 output) elementwise; got finite; the bound below 1 % of
    max |ref| over the elements whose relu gate is certain."""
    got = got.double().reshape(b.ref.shape)
    assert torch.isfinite(got).all(), '{}: non-finite output ({} elements)'.format(
        what, int((~torch.isfinite(got)).sum()))
    tol = tolerance(b, bf16)
    bad = (got - b.ref).abs() > tol
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError('{}: {} of {} elements outside the bound; first flat {}: got {:.9g} ref {:.9g} '
                             'bound {:.3g}'.format(what, n, bad.numel(), i, float(got.reshape(-1)[i]),
                                                   float(b.ref.reshape(-1)[i]), float(tol.reshape(-1)[i])))
    if zero_ref:
        return
    keep = torch.ones_like(bad) if ambiguous is None else ~ambiguous.expand_as(bad)
    scale = float(b.ref.abs()[keep].max())
    worst = float(b.err[keep].max())
    assert worst < 0.01 * scale, '{}: bound {:.3g} is not below 1 % of max |ref| {:.3g}'.format(what, worst, scale)
