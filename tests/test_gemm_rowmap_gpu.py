"""The row map on operand A of the dense bf16 GEMM kernels (GemmDesc::rmap, csrc/apa_gemm_bf16.hip: the MAP instances),
driven through the probe library's apa_probe_gemm_launch_rowmap.

A is a [T, P, width] feature cache; row r of the product's A is row clamp(index[r / P], 0, T - 1) * P + r % P of it.
Two assertions per case:
  * the mapped product equals the same product on a gathered copy of A BIT FOR BIT, with an equal trace, and the trace
    names the kernel the case exists for;
  * the gathered-copy result satisfies the float64 bound of tests/test_gemm_paths_gpu.py (its Problem.reference and the
    error model of tests/_gemm_probe.py; no new tolerance).
Every buffer is guarded with NaN sentinels: the cache has NaN rows in front of and behind it, every cached image has its
own magnitude (a wrong image cannot pass), the index repeats, is non-monotone and leaves images unused.

The contracted epilogue of the ring kernel (its ZP instance) has no field in ProbeGemm, whose layout is fixed: it is
covered by the fused evaluation route in tests/test_cached_pose_gpu.py.
"""
import ctypes

import pytest
import torch

from tests import _gemm_probe as gp
from tests.test_gemm_paths_gpu import Problem, _check_values, _launch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
T = 7
PATTERN = (5, 1, 5, 0, 6, 1, 3, 3, 0, 6, 5, 1)      # images 2 and 4 are never used


def _index(n, clamped=False):
    idx = [PATTERN[i % len(PATTERN)] for i in range(n)]
    if clamped:
        idx[1], idx[n - 1] = -3, T + 5
    return idx


def _lib():
    lib = gp.load_probe()
    lib.apa_probe_gemm_launch_rowmap.argtypes = [ctypes.POINTER(gp.ProbeGemm), ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_int, ctypes.POINTER(gp.ProbeTrace)]
    lib.apa_probe_gemm_launch_rowmap.restype = ctypes.c_int
    return lib


class Mapped:
    """A Problem whose A is the gathered copy of a guarded cache, and the descriptor of the mapped twin."""

    def __init__(self, c, n_img, P, index, seed):
        dev = torch.device('cuda')
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        self.p = p = Problem(c, dev, gen)
        a_kc = c.get('a_kc', True)
        rows, width = n_img * P, (p.K if a_kc else p.M)
        assert rows == (p.M if a_kc else p.K)
        scale = (1.0 + torch.arange(T, device=dev, dtype=torch.float32)).view(T, 1, 1)
        vals = (gp.rand_operand((T, P, width), gen, dev) * scale).to(p.A.dtype)
        lda = p.A.ld
        # NaN rows in front (16-byte aligned offset) and, Guarded's own, behind
        self.cache = gp.Guarded(T * P, width, lda, p.A.dtype, dev, 8 * lda, vals.view(T * P, width))
        self.index = torch.tensor(index, dtype=torch.int32, device=dev)
        src = self.index.long().clamp(0, T - 1)
        gathered = vals[src].reshape(rows, width)
        p.A.view.copy_(gathered)
        p.Aval = gathered if a_kc else gathered.t()
        p.A.snapshot()
        self.cache.snapshot()
        self.P = P
        self.d = gp.ProbeGemm.from_buffer_copy(p.d)
        self.d.A = self.cache.ptr

    def launch(self):
        tr = gp.ProbeTrace()
        rc = _lib().apa_probe_gemm_launch_rowmap(ctypes.byref(self.d), self.index.data_ptr(), T, self.P,
                                                 ctypes.byref(tr))
        torch.cuda.synchronize()
        return rc, tr.as_dict()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# name, kind, desc, (batch images, P)
CASES = [
    ('generic_rows', 'bf16', dict(M=27, K=72, N=16, tc=1, bias=True, act=1), (3, 9)),
    ('generic_kmajor', 'bf16', dict(M=128, K=72, N=64, a_kc=False, tc=0), (8, 9)),
    ('glds64_rows', 'glds64', dict(M=132, K=128, N=64, tc=1, bias=True, act=1), (4, 33)),
    ('glds64_kmajor_splitk', 'glds64', dict(M=256, K=576, N=128, a_kc=False, tc=0, splits=3), (16, 36)),
    ('ring_bkm', 'ring', dict(M=392, K=256, N=256, tc=1, bias=True, act=1), (2, 196)),
    ('ring_bkc', 'ring', dict(M=392, K=256, N=256, tc=1, b_kc=True, bias=True), (2, 196)),
    ('glds128_rows', 'glds128', dict(M=10368, K=128, N=1024, tc=1, bias=True, act=1), (324, 32)),
    ('glds128_kmajor_splitk', 'glds128', dict(M=1024, K=1280, N=1024, a_kc=False, tc=0, splits=10), (40, 32)),
    ('glds64_rows_clamped', 'glds64', dict(M=132, K=128, N=64, tc=1, bias=True, act=1), (4, 33)),
    ('glds64_kmajor_clamped', 'glds64', dict(M=256, K=576, N=128, a_kc=False, tc=0, splits=3), (16, 36)),
]


@pytest.mark.parametrize('name,kind,c,shape', CASES, ids=[c[0] for c in CASES])
def test_mapped_product_equals_gathered_copy(name, kind, c, shape):
    n_img, P = shape
    m = Mapped(dict(c), n_img, P, _index(n_img, clamped=name.endswith('clamped')), seed=len(name))
    p = m.p
    tr_plain, _, _ = _launch(p)
    assert tr_plain['kind'] == kind, '{}: the plain product ran {} (trace {})'.format(name, tr_plain['kind'], tr_plain)
    if kind == 'ring':
        assert tr_plain['mt'] == 4
    if c.get('splits', 1) > 1:
        assert tr_plain['splits'] == c['splits'] and tr_plain['reduce'] == 'vec'
    _check_values(p, name + ' (gathered copy)')
    want = p.C.bits()
    for g in (p.C, p.ws):
        if g is not None:
            g.restore()
    rc, tr = m.launch()
    assert rc == gp.APA_OK, gp.load_probe().apa_probe_last_error()
    assert tr == tr_plain, '{}: mapped trace {} != plain trace {}'.format(name, tr, tr_plain)
    assert torch.equal(p.C.bits(), want), '{}: {} elements differ from the product on the gathered copy'.format(
        name, int((p.C.bits() != want).sum()))
    for g, what in ((p.C, 'C'), (p.ws, 'workspace'), (m.cache, 'cache'), (p.B, 'B')):
        if g is not None:
            g.check_guards('{} {}'.format(name, what))


@pytest.mark.parametrize('why', ['fp32_A', 'lda_not_16_bytes'])
def test_mapped_product_refused_before_anything_is_queued(why):
    c = dict(M=132, K=128, N=64, tc=1, bias=True, act=1)
    if why == 'fp32_A':
        c.update(ta=0, tb=0)
    else:
        c.update(lda=128 + 4)       # 264-byte rows
    m = Mapped(c, 4, 33, _index(4), seed=3)
    before = m.p.C.base.view(torch.int16).clone()
    rc, tr = m.launch()
    assert rc == gp.APA_ERR_UNSUPPORTED
    assert b'feature cache behind operand A' in gp.load_probe().apa_probe_last_error()
    assert tr['kind'] == 'none'
    assert torch.equal(m.p.C.base.view(torch.int16), before), 'a refused product wrote its output'
