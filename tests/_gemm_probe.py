"""ctypes glue for libapa_gemm_probe.so (csrc/apa_gemm_probe.hip): the product's dense GEMM dispatcher
(gemm_launch), m1_colsum and sgemm_small driven directly, plus the guarded buffers and the float64 reference
that tests/test_gemm_paths_gpu.py checks them with.

Error model of the comparison (elementwise, `bound`):
  * every operand value the kernel multiplies is reproduced exactly: bf16 operands are exact in float64; an fp32
    operand on a bf16 MFMA path is rounded to bf16 by the staging code, which rounds to nearest even in every
    kernel (v_cvt_pk_bf16_f32 / f32_to_bf16_bits), as torch's .to(bfloat16) does; a dropout mask on A is applied
    in fp32 before that rounding (fl32(a * keep / p)), as the stager does;
  * fp32 accumulation of K products (MFMA chains, split-K partials, the fixed-order reduce, + bias, + beta C,
    the rank-1 term): |err| <= C_ACC * (K + 8) * 2^-24 * mag, where mag is the same expression evaluated on
    absolute values (|A| |B| + |bias| + |beta C| + |rank-1 term|);
  * a bf16 output adds one rounding to nearest: 2^-8 |ref| (bf16 carries 8 significant bits).
Each case also asserts that its bound stays below 1 % of max |ref| (the operands have a positive mean, so |ref| is
of the order of mag): a dropped K chunk, a wrong bias column or a shifted row moves an element by far more.
"""
import ctypes
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_PATH = os.path.join(ROOT, 'attentionalpoolingaction_amd', 'custom_ops', 'libapa_gemm_probe.so')
PROBE_VERSION = 2
PROBE_SYMBOLS = ('apa_probe_gemm_struct_size', 'apa_probe_gemm_version', 'apa_probe_gemm_ws_bytes',
                 'apa_probe_gemm_pick_splits', 'apa_probe_sgemm_ws_bytes', 'apa_probe_last_error',
                 'apa_probe_gemm_launch', 'apa_probe_m1_colsum', 'apa_probe_sgemm_small')

# GemmTrace values (csrc/apa_internal.h)
KINDS = {0: 'none', 1: 'generic', 2: 'bf16', 3: 'wide', 4: 'ring', 5: 'glds64', 6: 'glds128'}
REDUCES = {0: 'none', 1: 'vec', 2: 'scalar', 3: 'tail'}
TWINS = {0: 'none', 1: 'fused', 2: 'serial'}
APA_OK, APA_ERR_UNSUPPORTED, APA_ERR_WORKSPACE = 0, -2, -3

C_ACC = 4.0
EPS32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
GUARD_ROWS = 8          # sentinel rows after every operand / output of more than one row
GUARD_TAIL = 4096       # sentinel elements after every allocation (workspace included)

_I64, _F64, _P = ctypes.c_int64, ctypes.c_double, ctypes.c_void_p


class ProbeGemm(ctypes.Structure):
    _fields_ = [('version', _I64),
                ('A', _P), ('lda', _I64), ('ta', _I64), ('a_kc', _I64),
                ('B', _P), ('ldb', _I64), ('tb', _I64), ('b_kc', _I64),
                ('C', _P), ('ldc', _I64), ('tc', _I64),
                ('M', _I64), ('N', _I64), ('K', _I64), ('n_valid', _I64),
                ('bias', _P), ('beta', _F64), ('act', _I64),
                ('splits', _I64), ('ws', _P),
                ('drop_a', _I64), ('drop_c', _I64), ('inv_keep', _F64), ('thresh', _I64), ('seed', ctypes.c_uint64),
                ('offset', ctypes.c_uint64),
                ('r1_row', _P), ('r1_col', _P), ('r1_bits', _P), ('r1_P', _I64), ('r1_invP', _F64),
                ('r1_inv_keep', _F64),
                ('mid_bits', _P), ('mid_k', _I64), ('mid_inv_keep', _F64),
                ('stream_out', _I64)]


class ProbeColsum(ctypes.Structure):
    _fields_ = [('pdwa', _P), ('dwa', _P), ('nblk', _I64), ('C', _I64), ('ld', _I64),
                ('dwa2', _P), ('C1', _I64), ('dwa3', _P), ('C2', _I64), ('dwa4', _P), ('C3', _I64), ('dwa5', _P),
                ('C4', _I64), ('aux_src', _P), ('aux_n', _I64), ('aux_scale', _F64), ('aux_dst', _P),
                ('rng_bump', _P)]


class ProbeTrace(ctypes.Structure):
    _fields_ = [('kind', _I64), ('splits', _I64), ('k_per_split', _I64), ('mt', _I64), ('twin', _I64),
                ('reduce', _I64)]

    def as_dict(self):
        return {'kind': KINDS[self.kind], 'splits': self.splits, 'k_per_split': self.k_per_split, 'mt': self.mt,
                'twin': TWINS[self.twin], 'reduce': REDUCES[self.reduce]}


_lib = None


def load_probe():
    """The probe library; missing is an error (build() makes it), never a skip."""
    global _lib
    if _lib is None:
        if not os.path.exists(PROBE_PATH):
            raise FileNotFoundError('{} is missing: run __graft_entry__.build()'.format(PROBE_PATH))
        lib = ctypes.CDLL(PROBE_PATH)
        lib.apa_probe_gemm_struct_size.restype = _I64
        lib.apa_probe_gemm_version.restype = _I64
        lib.apa_probe_gemm_ws_bytes.restype = _I64
        lib.apa_probe_gemm_ws_bytes.argtypes = [ctypes.c_int] * 3
        lib.apa_probe_gemm_pick_splits.argtypes = [ctypes.c_int] * 3
        lib.apa_probe_sgemm_ws_bytes.restype = _I64
        lib.apa_probe_sgemm_ws_bytes.argtypes = [ctypes.c_int] * 3
        lib.apa_probe_last_error.restype = ctypes.c_char_p
        lib.apa_probe_gemm_launch.argtypes = [ctypes.POINTER(ProbeGemm), ctypes.POINTER(ProbeGemm),
                                              ctypes.POINTER(ProbeColsum), ctypes.POINTER(ProbeTrace),
                                              ctypes.POINTER(ProbeTrace), ctypes.POINTER(ctypes.c_int), _P]
        lib.apa_probe_m1_colsum.argtypes = [ctypes.POINTER(ProbeColsum), _P]
        lib.apa_probe_sgemm_small.argtypes = [_P, _I64, _I64, _P, _I64, _I64, _P, _I64, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]
        assert lib.apa_probe_gemm_version() == PROBE_VERSION
        assert lib.apa_probe_gemm_struct_size() == ctypes.sizeof(ProbeGemm)
        _lib = lib
    return _lib


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def keep_thresh(keep):
    """apa_internal.h keep_thresh."""
    return int(min(max(float(keep) * 65536.0 + 0.5, 0.0), 65536.0))


# ------------------------------------------------------------------------------------------ guarded buffers
_NAN_BITS = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0}
_INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


class Guarded:
    """A rows x cols matrix with leading dimension ld at element offset `off` of a larger allocation whose every
    other element (the ld padding, GUARD_ROWS rows after the last one of a matrix, GUARD_TAIL elements after that,
    the `off` elements in front) holds a NaN bit pattern.  A one-row buffer (bias, workspace) has the tail only.  `view` is the matrix; `check_guards()` asserts no sentinel moved."""

    def __init__(self, rows, cols, ld, dtype, dev, off=0, data=None):
        assert ld >= cols
        self.dtype, self.rows, self.cols, self.ld, self.off = dtype, rows, cols, ld, off
        total = off + (rows + (GUARD_ROWS if rows > 1 else 0)) * ld + GUARD_TAIL
        self.base = torch.empty(total, dtype=dtype, device=dev)
        self.base.view(_INT_VIEW[dtype]).fill_(_NAN_BITS[dtype])
        self.view = self.base[off:off + rows * ld].view(rows, ld)[:, :cols]
        self.valid = torch.zeros(total, dtype=torch.bool, device=dev)
        self.valid[off:off + rows * ld].view(rows, ld)[:, :cols] = True
        if data is not None:
            self.view.copy_(data)
        self.snap = None

    @property
    def ptr(self):
        return self.view.data_ptr()

    def snapshot(self):
        self.snap = self.base.view(_INT_VIEW[self.dtype]).clone()

    def restore(self):
        self.base.view(_INT_VIEW[self.dtype]).copy_(self.snap)

    def check_guards(self, what):
        now = self.base.view(_INT_VIEW[self.dtype])
        bad = (now != self.snap) & ~self.valid
        n = int(bad.sum())
        assert n == 0, '{}: {} guard elements changed (first at flat {})'.format(
            what, n, int(bad.nonzero()[0]))

    def bits(self):
        return self.view.contiguous().view(_INT_VIEW[self.dtype]).clone()


def rand_operand(shape, gen, dev):
    """Positive-mean operands (U(-0.25, 1)): |A.B| is of the order of |A|.|B|, so the error bound is a small
    fraction of the result and any dropped or misplaced term shows."""
    return torch.rand(shape, generator=gen, device=dev) * 1.25 - 0.25
