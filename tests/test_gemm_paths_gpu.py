"""Every dense GEMM path of csrc/apa_gemm.hip + csrc/apa_gemm_bf16.hip, driven directly through the product's
gemm_launch (libapa_gemm_probe.so, tests/_gemm_probe.py), against a float64 product of the operands the kernel
consumes (error model: tests/_gemm_probe.py).

Each case asserts the path that served it (GemmDesc::trace: kernel kind, ring / wide MT, split, twin, reduce): a
heuristic change that moves a shape to another kernel fails the case by name instead of losing its coverage.  Every
operand and output sits inside a larger allocation whose guard elements hold NaN: valid outputs must be finite (no
k >= K, no row >= M was read into them) and no guard element of C or of the split-K workspace may change.  The ring
and wide shapes are derived from the device's CU count so that each lands on the tile height in its name.
"""
import ctypes
import zlib

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ring_m(mt, N):
    """M that ring_pick_mt maps to `mt` for an N-wide output (ragged last row tile)."""
    return (_cus() // -(-N // 128)) * 32 * mt - 24


def _wide_m(mt, N):
    return (_cus() // -(-N // 256)) * 32 * mt - 24


def _dt(code):
    return BF if code else F32


def _mask(n, keep, seed, offset):
    return cof.dropout_mask((n,), keep, seed, offset).to(torch.float64)


def _bits_to_bytes(bits):
    """{0,1} flat tensor -> packed keep bits (bit e & 7 of byte e >> 3)."""
    b = bits.to(torch.int32).view(-1, 8)
    w = torch.tensor([1 << i for i in range(8)], dtype=torch.int32, device=bits.device)
    return (b * w).sum(1).to(torch.uint8)


class Problem:
    """One GemmDesc with guarded operands, its float64 reference and error bound."""

    def __init__(self, c, dev, gen, seed_off=0):
        self.c = c
        M, N, K = c['M'], c['N'], c['K']
        nv = c.get('n_valid', 0)
        Nst = nv or N
        ta, tb, tc = c.get('ta', 1), c.get('tb', 1), c.get('tc', 0)
        a_kc, b_kc = c.get('a_kc', True), c.get('b_kc', False)
        pad = c.get('pad', 8)
        self.M, self.N, self.K, self.Nst = M, N, K, Nst
        A = gp.rand_operand((M, K), gen, dev).to(_dt(ta))
        B = gp.rand_operand((N, K), gen, dev).to(_dt(tb))
        if nv:
            B[nv:] = 0    # n_valid: B covers N zero-padded columns
        self.Aval, self.Bval = A, B
        lda = c.get('lda', (K if a_kc else M) + pad)
        ldb = c.get('ldb', (K if b_kc else N) + pad)
        ldc = c.get('ldc', Nst + pad)
        self.A = gp.Guarded(M, K, lda, _dt(ta), dev, c.get('off_a', 0), A) if a_kc else \
            gp.Guarded(K, M, lda, _dt(ta), dev, c.get('off_a', 0), A.t())
        self.B = gp.Guarded(N, K, ldb, _dt(tb), dev, 0, B) if b_kc else gp.Guarded(K, N, ldb, _dt(tb), dev, 0, B.t())
        beta = c.get('beta', 0.0)
        self.C = gp.Guarded(M, Nst, ldc, _dt(tc), dev)   # valid region starts as NaN unless it is accumulated into
        if beta:
            self.C.view.copy_(gp.rand_operand((M, Nst), gen, dev))
        self.Cold = self.C.view.double().clone()
        self.bias = gp.Guarded(1, Nst, Nst, F32, dev, 0, torch.randn(1, Nst, generator=gen, device=dev)) \
            if c.get('bias') else None
        splits = c.get('splits', 1)
        self.ws = None
        nws = gp.load_probe().apa_probe_gemm_ws_bytes(M, N, splits) // 4
        if nws:
            self.ws = gp.Guarded(1, nws, nws, F32, dev)
        d = gp.ProbeGemm()
        d.version = gp.PROBE_VERSION
        d.A, d.lda, d.ta, d.a_kc = self.A.ptr, lda, ta, int(a_kc)
        d.B, d.ldb, d.tb, d.b_kc = self.B.ptr, ldb, tb, int(b_kc)
        d.C, d.ldc, d.tc = self.C.ptr, ldc, tc
        d.M, d.N, d.K, d.n_valid = M, N, K, nv
        d.bias = self.bias.ptr if self.bias else None
        d.beta, d.act, d.splits = beta, c.get('act', 0), splits
        d.ws = self.ws.ptr if self.ws else None
        d.stream_out = int(c.get('stream_out', False))
        self.keep = c.get('keep', 0.75)
        self.inv_keep = float(torch.tensor(1.0 / self.keep, dtype=F32))
        seed, offset = 1234 + seed_off, 77
        if c.get('drop_a') or c.get('drop_c'):
            d.drop_a, d.drop_c = c.get('drop_a', 0), c.get('drop_c', 0)
            d.inv_keep, d.thresh, d.seed, d.offset = self.inv_keep, gp.keep_thresh(self.keep), seed, offset
            n = M * K if d.drop_a else M * Nst
            self.mask = _mask(n, self.keep, seed, offset)
        if c.get('mid_k'):
            self.midbits = (torch.rand(M * N, generator=gen, device=dev) < self.keep)
            self.midbytes = _bits_to_bytes(self.midbits)
            d.mid_bits, d.mid_k, d.mid_inv_keep = self.midbytes.data_ptr(), c['mid_k'], self.inv_keep
        if c.get('r1_P'):
            P = c['r1_P']
            nimg = -(-M // P)
            # att[m] of the order of P K / 8: the rank-1 term weighs as much as the product it is added to, so a
            # wrong scale of it cannot hide under the bf16 rounding of the sum
            self.r1_row = torch.rand(M, generator=gen, device=dev) * (P * K / 8)
            self.r1_col = gp.rand_operand((nimg, N), gen, dev).contiguous()
            self.r1bits = (torch.rand(M * N, generator=gen, device=dev) < self.keep)
            self.r1bytes = _bits_to_bytes(self.r1bits)
            d.r1_row, d.r1_col, d.r1_bits = self.r1_row.data_ptr(), self.r1_col.data_ptr(), self.r1bytes.data_ptr()
            d.r1_P, d.r1_invP = P, float(torch.tensor(1.0 / P, dtype=F32))
            d.r1_inv_keep = self.inv_keep
        self.d = d
        for g in self.buffers():
            g.snapshot()

    def buffers(self):
        return [g for g in (self.A, self.B, self.C, self.bias, self.ws) if g is not None]

    def reference(self):
        c, M, K, Nst = self.c, self.M, self.K, self.Nst
        bf = not (c.get('ta', 1) == 0 and c.get('tb', 1) == 0)
        A = self.Aval.float()
        if c.get('drop_a') == 1:
            A = A * (self.mask.view(M, K).float() * self.inv_keep)
        elif c.get('drop_a') == 2:    # transposed flat index k * M + m (the dWt product of apa_pc.hip)
            A = A * (self.mask.view(K, M).t().float() * self.inv_keep)
        B = self.Bval[:Nst].float()
        if bf:
            A, B = A.to(BF), B.to(BF)
        A, B = A.double(), B.double()
        mk = c.get('mid_k', 0)
        if mk:
            s = self.midbits.view(M, self.N)[:, :Nst].double() * self.inv_keep
            ref = (A[:, :mk] @ B[:, :mk].t()) * s + A[:, mk:] @ B[:, mk:].t()
            mag = (A[:, :mk].abs() @ B[:, :mk].abs().t()) * s + A[:, mk:].abs() @ B[:, mk:].abs().t()
        else:
            ref, mag = A @ B.t(), A.abs() @ B.abs().t()
        if self.bias is not None:
            b = self.bias.view.double()
            ref, mag = ref + b, mag + b.abs()
        if c.get('act'):
            ref = torch.relu(ref)
        if c.get('drop_c'):
            s = self.mask.view(M, Nst) * self.inv_keep
            ref, mag = ref * s, mag * s
        if c.get('r1_P'):
            P = c['r1_P']
            apk = (self.r1_row * (1.0 / P) * self.inv_keep).double()     # (fl32 arithmetic inside the bound)
            rows = torch.arange(M, device=A.device) // P
            t = apk[:, None] * self.r1bits.view(M, self.N).double() * self.r1_col.double()[rows]
            ref, mag = ref + t, mag + t.abs()
        if c.get('beta'):
            ref, mag = ref + self.Cold, mag + self.Cold.abs()
        bound = gp.C_ACC * (K + 8) * gp.EPS32 * mag
        if c.get('tc', 0):   # |fl(x) - ref| <= |x - ref| + 2^-8 |x|,  |x| <= |ref| + |x - ref|
            bound = (1 + gp.U_BF16) * bound + gp.U_BF16 * ref.abs()
        return ref, bound

    def restore(self):
        for g in self.buffers():
            g.restore()


def _launch(p, twin=None, tail=None, stream_out=None):
    lib = gp.load_probe()
    d = p.d
    if stream_out is not None:
        d = gp.ProbeGemm.from_buffer_copy(p.d)
        d.stream_out = int(stream_out)
    tr, ttr, done = gp.ProbeTrace(), gp.ProbeTrace(), ctypes.c_int(0)
    rc = lib.apa_probe_gemm_launch(ctypes.byref(d), ctypes.byref(twin.d) if twin else None,
                                   ctypes.byref(tail) if tail is not None else None, ctypes.byref(tr),
                                   ctypes.byref(ttr), ctypes.byref(done), gp.stream_ptr())
    torch.cuda.synchronize()
    assert rc == gp.APA_OK, lib.apa_probe_last_error()
    return tr.as_dict(), ttr.as_dict(), done.value


def _check_values(p, what):
    out = p.C.view.double()
    assert torch.isfinite(out).all(), '{}: {} non-finite outputs (a sentinel was read)'.format(
        what, int((~torch.isfinite(out)).sum()))
    ref, bound = p.reference()
    rmax = float(ref.abs().max())
    assert float(bound.max()) < 0.01 * rmax, '{}: error bound {} is not below 1 % of max|ref| {}'.format(
        what, float(bound.max()), rmax)
    err = (out - ref).abs()
    bad = err > bound
    if bad.any():
        i = int(bad.nonzero()[0][0]), int(bad.nonzero()[0][1])
        raise AssertionError('{}: {} elements outside the bound; first ({}, {}): got {} want {} bound {}'.format(
            what, int(bad.sum()), i[0], i[1], float(out[i]), float(ref[i]), float(bound[i])))
    for g, name in ((p.C, 'C'), (p.ws, 'workspace')):
        if g is not None:
            g.check_guards('{} {}'.format(what, name))


def _check_trace(tr, expect, what):
    for k, v in expect.items():
        if k == 'split':
            assert (tr['splits'] > 1) == (v > 1), '{}: splits {} (want {})'.format(what, tr['splits'], v)
        else:
            assert tr[k] == v, '{}: traced {} = {!r}, expected {!r} (trace {})'.format(what, k, tr[k], v, tr)


def C(name, expect, **kw):
    kw['name'], kw['expect'] = name, expect
    return kw


def _kinds(kind, mt=None, split=1, reduce='none', twin='none'):
    e = {'kind': kind, 'split': split, 'reduce': reduce, 'twin': twin}
    if mt is not None:
        e['mt'] = mt
    return e


# ------------------------------------------------------------------------------------------ the case table
# Shapes whose kind depends on the CU count are lambdas of it (evaluated at run time).
def _cases():
    L = []
    # --- generic gemm128_kernel: exact f32 MFMA for f32 x f32, bf16 MFMA otherwise
    L += [C('generic_f32_exact_ragged', _kinds('generic'), M=300, N=200, K=333, ta=0, tb=0, bias=1, act=1),
          C('generic_f32_kmajor_a_kc_b', _kinds('generic'), M=130, N=129, K=70, ta=0, tb=0, a_kc=False, b_kc=True),
          C('generic_f32_split_scalar', _kinds('generic', split=4, reduce='scalar'), M=256, N=393, K=4000, ta=0,
            tb=0, splits=4, bias=1),
          C('generic_f32_split_vec_beta', _kinds('generic', split=3, reduce='vec'), M=200, N=256, K=3000, ta=0,
            tb=0, splits=3, beta=1.0),
          # 31 requested -> 16 chunks of 64: the last one is 33 deep (one 32-wide tile + 1)
          C('generic_split_k_past_chunk', _kinds('generic', split=16, reduce='vec'), M=200, N=136, K=993, ta=0,
            tb=0, splits=31, bias=1),
          C('generic_bf16_unaligned_base', _kinds('generic'), M=200, N=136, K=256, off_a=1),
          C('generic_bf16_lda_not_vec', _kinds('generic'), M=150, N=140, K=96, lda=99, tc=1),
          C('generic_bf16_k_not_32', _kinds('generic'), M=129, N=70, K=45, tb=0, tc=1, bias=1),
          C('generic_tiny_k_m_below_8', _kinds('generic'), M=5, N=7, K=5, tb=0),
          C('generic_drop_c_f32', _kinds('generic'), M=588, N=256, K=400, ta=0, tb=0, b_kc=True, drop_c=1),
          # apa_capi.hip TopDownAttention end point: dropout(X) . Wt + bt, bf16 X, f32 Wt, drop_a = 1
          C('capi_topdown_shipped', _kinds('generic'), M=6272, N=393, K=2048, tb=0, tc=1, bias=1, drop_a=1,
            keep=0.5, pad=0),
          C('capi_topdown_ragged', _kinds('generic'), M=245, N=393, K=2048, tb=0, tc=1, bias=1, drop_a=1,
            keep=0.5, pad=0)]
    # --- gemm_bf16_kernel (eligible, but not whole bf16 K tiles)
    L += [C('bf16_fp32_b', _kinds('bf16'), M=1000, N=200, K=256, tb=0, tc=1, bias=1, act=1),
          C('bf16_k_not_64_kmajor_a', _kinds('bf16'), M=296, N=136, K=200, a_kc=False, b_kc=True),
          # 17 chunks of 64, the last one 8 deep
          C('bf16_split_k_past_chunk', _kinds('bf16', split=17, reduce='vec'), M=300, N=128, K=1032, tb=0,
            splits=32),
          C('bf16_drop_c', _kinds('bf16'), M=1000, N=200, K=256, tb=0, tc=1, drop_c=1, bias=1),
          C('bf16_split_scalar_reduce', _kinds('bf16', split=5, reduce='scalar'), M=100, N=18, K=1000, tb=0,
            b_kc=True, splits=5, bias=1),
          # apa_pose_head.hip pose fwd g2: Pl = Ppre . W2 + b2 (N = 16) and pose bwd dW2 = Ppre^T dPl
          C('pose_fwd_g2_shipped', _kinds('bf16', split=6, reduce='vec'), M=6272, N=16, K=768, tb=0, bias=1,
            splits=6, pad=0),
          C('pose_fwd_g2_ragged', _kinds('bf16', split=6, reduce='vec'), M=5983, N=16, K=768, tb=0, bias=1,
            splits=6, pad=0),
          C('pose_bwd_dw2_shipped', _kinds('bf16', split=32, reduce='vec'), M=768, N=16, K=6272, a_kc=False,
            tb=0, splits=32, pad=0),
          # R = 31 x 193 is not a multiple of 8: the product's dW2 leaves the bf16 path
          C('pose_bwd_dw2_ragged', _kinds('generic', split=32, reduce='vec'), M=768, N=16, K=5983, a_kc=False,
            tb=0, splits=32, pad=0)]
    # --- glds64: all four layouts, both output types, one K tile; split-K
    for a_kc in (True, False):
        for b_kc in (True, False):
            for tc in (0, 1):
                L.append(C('glds64_a{}_b{}_c{}'.format('kc' if a_kc else 'km', 'kc' if b_kc else 'km',
                                                       'bf16' if tc else 'f32'),
                           _kinds('glds64'), M=1000, N=200, K=64, a_kc=a_kc, b_kc=b_kc, tc=tc, bias=tc))
    L += [C('glds64_split_k_past_chunk', _kinds('glds64', split=4, reduce='vec'), M=512, N=256, K=832,
            splits=4, bias=1),
          C('glds64_drop_c', _kinds('glds64'), M=1000, N=200, K=64, tc=1, drop_c=1, bias=1),
          C('glds64_n16', _kinds('glds64'), M=1000, N=16, K=128, a_kc=False, b_kc=False),
          # pose bwd dW1 = X^T dPpre (both k-major), split per pose_dw1_splits
          C('pose_bwd_dw1_shipped', _kinds('glds64', split=4, reduce='vec'), M=2048, N=768, K=6272, a_kc=False,
            splits=4, pad=0),
          C('pose_bwd_dw1_ragged', _kinds('glds64', split=4, reduce='vec'), M=2048, N=768, K=5952, a_kc=False,
            splits=4, pad=0)]
    # --- glds128: all four layouts (>= 640 tiles of 128 x 128), both output types; split-K
    for a_kc in (True, False):
        for b_kc in (True, False):
            tc = int(a_kc != b_kc)
            L.append(C('glds128_a{}_b{}_c{}'.format('kc' if a_kc else 'km', 'kc' if b_kc else 'km',
                                                    'bf16' if tc else 'f32'),
                       _kinds('glds128'), M=4000, N=2568, K=64, a_kc=a_kc, b_kc=b_kc, tc=tc, bias=1 - tc))
    L.append(C('glds128_drop_c', _kinds('glds128'), M=4000, N=2568, K=64, drop_c=1))
    # 4 chunks of 256, the last one a single 64-deep tile
    L.append(C('glds128_split_k_past_chunk', _kinds('glds128', split=4, reduce='vec'), M=2048, N=1280, K=832,
               splits=4, bias=1))
    L.append(C('glds128_split_nvalid', _kinds('glds128', split=8, reduce='vec'), M=2048, N=768, K=6272,
               a_kc=False, splits=8, n_valid=760))
    # --- ring MT 4..8, B k-major; B k-contiguous; shortest K loop (4 tiles); ragged N; both output types
    for mt in (4, 5, 6, 7, 8):
        L.append(C('ring_mt{}_b_km'.format(mt), _kinds('ring', mt), M=lambda mt=mt: _ring_m(mt, 768), N=768,
                   K=256, tc=mt % 2, bias=1))
    L += [C('ring_mt5_b_kc', _kinds('ring', 5), M=lambda: _ring_m(5, 768), N=768, K=320, b_kc=True, tc=1),
          C('ring_mt4_ragged_n', _kinds('ring', 4), M=lambda: _ring_m(4, 696), N=696, K=256, act=1, bias=1),
          C('ring_nvalid_393_of_400', _kinds('ring'), M=6272, N=400, n_valid=393, K=2048, bias=1),
          C('ring_drop_c_bf16', _kinds('ring', 4), M=588, N=256, K=448, b_kc=True, tc=1, drop_c=1),
          # pose fwd g1: Ppre = relu(X . W1 + b1), bf16 W1 copy
          C('pose_fwd_g1_shipped', _kinds('ring'), M=6272, N=768, K=2048, tc=1, bias=1, act=1, pad=0),
          C('pose_fwd_g1_ragged', _kinds('ring'), M=5983, N=1096, K=384, tc=1, bias=1, act=1, pad=0)]
    # --- wide MT 4..7: N >= 1024, K of 2 .. 16 tiles, both operands k-contiguous
    for mt, K, N in ((4, 128, 1024), (5, 1024, 1024), (6, 192, 1096), (7, 128, 1024)):
        L.append(C('wide_mt{}_k{}_n{}'.format(mt, K, N), _kinds('wide', mt), M=lambda mt=mt, N=N: _wide_m(mt, N),
                   N=N, K=K, b_kc=True, tc=mt % 2, bias=mt % 2))
    # pose bwd dX (+)= dPpre . W1^T (beta 0 / 1, stream_out), and its rank-1 pooling share
    L += [C('pose_bwd_dx_beta0', _kinds('wide'), M=6272, N=2048, K=768, b_kc=True, tc=1, stream_out=True, pad=0),
          C('pose_bwd_dx_beta1', _kinds('wide'), M=6272, N=2048, K=768, b_kc=True, tc=1, beta=1.0,
            stream_out=True, pad=0),
          C('pose_bwd_dx_r1', _kinds('wide'), M=6272, N=2048, K=768, b_kc=True, tc=1, r1_P=196, keep=0.8,
            stream_out=True, pad=0),
          C('pose_bwd_dx_r1_ragged', _kinds('wide'), M=5983, N=2048, K=768, b_kc=True, tc=1, r1_P=193, keep=0.8,
            stream_out=True, pad=0),
          # per-class dX = (dT . Wt^T) * mask / keep + dZ . Wa^T as one product (mid-contraction mask)
          C('pc_dx_mid_mask', _kinds('wide'), M=6272, N=2048, K=896, mid_k=448, b_kc=True, tc=1, keep=0.8,
            stream_out=True, pad=0),
          C('pc_dx_mid_mask_ragged', _kinds('wide'), M=5983, N=2048, K=896, mid_k=448, b_kc=True, tc=1, keep=0.8,
            stream_out=True, pad=0),
          # per-class dX, two-product form (bf16, Xatt != X): dX = (dT . Wt^T) * mask / keep, then dX += dZ . Wa^T
          C('pc_dx_dt_wt_drop_c_shipped', _kinds('wide'), M=6272, N=2048, K=448, b_kc=True, tc=1, drop_c=1,
            keep=0.8, pad=0),
          C('pc_dx_dt_wt_drop_c_ragged', _kinds('wide'), M=5983, N=2048, K=448, b_kc=True, tc=1, drop_c=1,
            keep=0.8, pad=0),
          C('pc_dx_dz_wat_beta1', _kinds('wide'), M=6272, N=2048, K=448, b_kc=True, tc=1, beta=1.0,
            stream_out=True, pad=0),
          C('pc_dx_dz_wat_beta1_ragged', _kinds('wide'), M=5983, N=2048, K=448, b_kc=True, tc=1, beta=1.0,
            stream_out=True, pad=0)]
    return L


CASES = _cases()


def _resolve(c):
    c = dict(c)
    for k in ('M',):
        if callable(c[k]):
            c[k] = c[k]()
    return c


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_gemm_path_against_float64(gpu, case):
    c = _resolve(case)
    gen = torch.Generator(device=gpu).manual_seed(zlib.crc32(c['name'].encode()))
    p = Problem(c, gpu, gen)
    tr, _, _ = _launch(p)
    _check_trace(tr, c['expect'], c['name'])
    _check_values(p, c['name'])
    first = p.C.bits()
    # repeatable bit for bit (split-K included)
    p.restore()
    _launch(p)
    assert torch.equal(p.C.bits(), first), c['name'] + ': a repeated call differs'
    if c.get('tc') and c['expect']['kind'] != 'generic':   # the non-temporal store hint changes no bit
        p.restore()
        _launch(p, stream_out=not c.get('stream_out', False))
        assert torch.equal(p.C.bits(), first), c['name'] + ': stream_out changed the result'


# ------------------------------------------------------------------------------------------ twin products
TWIN_CASES = [
    # per-class Z | T (fast form: padded bf16 weights, T has n_valid = K): one ring launch
    C('pc_fwd_z_t_twin_shipped', _kinds('ring', twin='fused'), M=6272, N=400, K=2048, bias=1, pad=0,
      twin=dict(n_valid=393, bias=1)),
    # the same at 5 images: split-K, 128 x 64 tiles, twin reduce
    C('pc_fwd_z_t_twin_ragged', _kinds('glds64', split=8, reduce='vec', twin='fused'), M=245, N=400, K=2048,
      bias=1, splits=8, pad=0, twin=dict(n_valid=393, bias=1)),
    # dWt | dWa (fast form): k-major operands, split-K, n_valid
    C('pc_bwd_dwt_dwa_twin_shipped', _kinds('glds64', split=4, reduce='vec', twin='fused'), M=2048, N=400, n_valid=393,
      K=6272, a_kc=False, splits=4, pad=0, twin=dict(n_valid=393)),
    # the same at R = 31 x 196 (not a multiple of 8): not bf16-eligible -> generic kernel, two launches
    C('pc_bwd_dwt_dwa_twin_ragged', _kinds('generic', split=4, reduce='scalar', twin='serial'), M=2048, N=400,
      n_valid=393, K=6076, a_kc=False, splits=4, pad=0, twin=dict(n_valid=393)),
    # bf16-eligible, but R = 4 x 196 is not a whole number of 64-deep k tiles: the generic bf16 kernel, two launches
    C('pc_bwd_dwt_dwa_twin_k_ragged', _kinds('bf16', split=4, reduce='vec', twin='serial'), M=2048, N=448,
      n_valid=393, K=784, a_kc=False, splits=4, pad=0, twin=dict(n_valid=393)),
    # fp32-Wt form of Z | T: T is dropout(X) . Wt with unaligned f32 rows -> two launches
    C('pc_fwd_z_t_twin_fp32_wt', _kinds('ring', twin='serial'), M=6272, N=400, K=2048, bias=1, pad=0,
      twin=dict(N=393, tb=0, drop_a=1, keep=0.5, bias=1)),
    # dWt | dWa fp32 form with drop_a = 2 (transposed mask index): generic kernel, two launches
    C('pc_bwd_dwt_dwa_drop_a2_shipped', _kinds('generic', split=4, reduce='scalar', twin='serial'), M=2048,
      N=393, K=6272, ta=0, tb=0, a_kc=False, splits=4, drop_a=2, keep=0.5, pad=0, twin=dict(drop_a=0)),
    C('pc_bwd_dwt_dwa_drop_a2_ragged', _kinds('generic', split=4, reduce='scalar', twin='serial'), M=256, N=393,
      K=588, ta=0, tb=0, a_kc=False, splits=4, drop_a=2, keep=0.5, twin=dict(drop_a=0)),
    # shapes differ -> serialised even though both are bf16-eligible
    C('twin_shapes_differ', _kinds('glds64', twin='serial'), M=1000, N=200, K=64, twin=dict(N=136)),
]


@pytest.mark.parametrize('case', TWIN_CASES, ids=[c['name'] for c in TWIN_CASES])
def test_gemm_twin_against_float64_and_two_launches(gpu, case):
    c = _resolve(case)
    gen = torch.Generator(device=gpu).manual_seed(zlib.crc32(c['name'].encode()))
    p = Problem(c, gpu, gen)
    tc = dict(c)
    tc.pop('twin'); tc.pop('n_valid', None); tc.pop('bias', None)
    tc.update(c['twin'])
    t = Problem(tc, gpu, gen, seed_off=1)
    tr, ttr, _ = _launch(p, twin=t)
    _check_trace(tr, c['expect'], c['name'])
    _check_values(p, c['name'] + ' (first)')
    _check_values(t, c['name'] + ' (twin)')
    one, two = p.C.bits(), t.C.bits()
    for x in (p, t):
        x.restore()
    _launch(p)
    _launch(t)
    assert torch.equal(p.C.bits(), one) and torch.equal(t.C.bits(), two), \
        c['name'] + ': the twin launch differs from two separate launches'


# ------------------------------------------------------------------------------------------ reduce tail
#   id                          dW1 product (M, N, K)  nblk  aux_n  (pose bwd: Cp = 768, J = 16)
TAIL = [('pose_bwd_dw1_tail_shipped', (2048, 768, 6272), 196, 196),
        ('pose_bwd_dw1_tail_ragged',  (2048, 768, 5952), 31,  -31),    # aux_n < 0: the folded batch-mean form
        ('pose_bwd_dw1_tail_big_aux', (2048, 768, 5952), 600, -100)]


@pytest.mark.parametrize('case', TAIL, ids=[t[0] for t in TAIL])
def test_reduce_tail_colsum_is_m1_colsum_bit_for_bit(gpu, case):
    """Pose bwd dW1 + its tail job as apa_pose_head.hip builds it: [dW2 | db1 | db2 | dWa | dba] partial rows routed to
    five outputs, the aux sum and the RNG counter bump.  The tail blocks of the split-K reduce give the same bits
    as a standalone m1_colsum of the same partials, and the GEMM output equals the plain vector reduce."""
    name, (M, N, K), nblk, aux_n = case
    lib = gp.load_probe()
    gen = torch.Generator(device=gpu).manual_seed(K + nblk)
    p = Problem(dict(name=name, M=M, N=N, K=K, a_kc=False, splits=4, pad=0), gpu, gen)
    Cp, J = N, 16
    c1 = Cp * J
    sec = [c1, Cp, J, Cp, 1]                # dW2, db1, db2, dWa, dba
    Ctot = sum(sec)
    ld = Ctot + 15                          # (ldp: padded partial rows)
    part = torch.randn(nblk, ld, generator=gen, device=gpu)
    aux = torch.rand(abs(aux_n), generator=gen, device=gpu)

    def job():
        outs = [gp.Guarded(1, n, n, F32, gpu) for n in sec] + [gp.Guarded(1, 1, 1, F32, gpu)]   # + aux_dst
        bump = torch.full((2,), 41, dtype=torch.int64, device=gpu)
        for g in outs:
            g.snapshot()
        b = [0]
        for n in sec[:-1]:
            b.append(b[-1] + n)
        j = gp.ProbeColsum(part.data_ptr(), outs[0].ptr, nblk, Ctot, ld, outs[1].ptr, b[1], outs[2].ptr, b[2],
                           outs[3].ptr, b[3], outs[4].ptr, b[4], aux.data_ptr(), aux_n, 1.0 / 7.0, outs[5].ptr,
                           bump.data_ptr())
        return j, outs, bump

    j0, outs0, bump0 = job()
    tr, _, done = _launch(p, tail=j0)
    assert done == 1 and tr['reduce'] == 'tail' and tr['kind'] == 'glds64', tr
    _check_values(p, name + ' GEMM with tail')
    with_tail = p.C.bits()
    j1, outs1, bump1 = job()
    assert lib.apa_probe_m1_colsum(ctypes.byref(j1), gp.stream_ptr()) == gp.APA_OK
    torch.cuda.synchronize()
    names = ['dW2', 'db1', 'db2', 'dWa', 'dba', 'aux']
    for a, b, what in zip(outs0, outs1, names):
        assert torch.equal(a.bits(), b.bits()), name + ': tail ' + what + ' != m1_colsum'
        a.check_guards(name + ' ' + what)
        assert torch.isfinite(a.view).all(), name + ' ' + what
    assert bump0.tolist() == bump1.tolist() == [42, 41], (bump0.tolist(), bump1.tolist())
    # and the sums themselves: the partial rows' column sums, the aux mean
    want = part[:, :Ctot].double().sum(0)
    got = torch.cat([o.view[0] for o in outs0[:5]]).double()
    assert ((got - want).abs() <= 2 * nblk * gp.EPS32 * part[:, :Ctot].double().abs().sum(0)).all(), name
    aw = float(aux.double().sum()) / 7.0
    assert abs(float(outs0[5].view[0, 0]) - aw) <= 4 * abs(aux_n) * gp.EPS32 * abs(aw), name
    p.restore()
    tr, _, _ = _launch(p)
    assert tr['reduce'] == 'vec', tr
    assert torch.equal(p.C.bits(), with_tail), name + ': the tail reduce changed the GEMM output'


# ------------------------------------------------------------------------------------------ error paths
def _err_case(gpu, **kw):
    c = dict(name='err', M=256, N=256, K=2048)
    c.update(kw)
    return Problem(c, gpu, torch.Generator(device=gpu).manual_seed(5))


def _launch_rc(p):
    lib = gp.load_probe()
    tr = gp.ProbeTrace()
    rc = lib.apa_probe_gemm_launch(ctypes.byref(p.d), None, None, ctypes.byref(tr), None, None, gp.stream_ptr())
    torch.cuda.synchronize()
    return rc, tr.as_dict(), lib.apa_probe_last_error()


def test_error_paths_return_before_any_launch(gpu):
    # split-K without a workspace
    p = _err_case(gpu, splits=4)
    p.d.ws = None
    rc, tr, msg = _launch_rc(p)
    assert rc == gp.APA_ERR_WORKSPACE and b'workspace' in msg and tr['kind'] == 'none'
    # output dropout with split-K
    p = _err_case(gpu, splits=4, drop_c=1)
    rc, tr, msg = _launch_rc(p)
    assert rc == gp.APA_ERR_UNSUPPORTED and tr['kind'] == 'none'
    # rank-1 term / mid mask on products the wide kernel does not serve: generic (f32), bf16 kernel (f32 B),
    # glds64 -- each refused, none silently ignored
    for kw in (dict(ta=0, tb=0), dict(tb=0), dict(K=64)):
        for extra in (dict(r1_P=256), dict(mid_k=64, tc=1)):
            q = dict(kw)
            q.update(extra)
            p = _err_case(gpu, **q)
            rc, tr, msg = _launch_rc(p)
            assert rc == gp.APA_ERR_UNSUPPORTED, (q, rc, msg)
            assert tr['kind'] == 'none', (q, tr)
            p.C.check_guards('error path C')
            assert torch.isnan(p.C.view.double()).all(), (q, 'C was written')


# ------------------------------------------------------------------------------------------ sgemm_small
#   name                m    n     k     splits  rank1  A strides        B strides
SMALL = [('logits_form',   32,  393,  2048, 8,      True,  ('kc',), ('kn',)),
         ('dz_form',       32,  2048, 393,  1,      False, ('kc',), ('nk',)),
         ('dwt_form',      2048, 393, 32,   1,      False, ('km',), ('kn',)),
         ('ragged_split',  17,  29,   45,   3,      True,  ('km',), ('nk',)),
         ('ragged_one',    5,   3,    7,    1,      True,  ('kc',), ('kn',))]


@pytest.mark.parametrize('case', SMALL, ids=[s[0] for s in SMALL])
def test_sgemm_small_against_float64(gpu, case):
    name, m, n, k, splits, rank1, (al,), (bl,) = case
    lib = gp.load_probe()
    gen = torch.Generator(device=gpu).manual_seed(m * 7 + n + k)
    A = gp.rand_operand((m, k), gen, gpu)
    B = gp.rand_operand((k, n), gen, gpu)
    if al == 'kc':
        Ag = gp.Guarded(m, k, k + 3, F32, gpu, 0, A); a_si, a_sk = k + 3, 1
    else:
        Ag = gp.Guarded(k, m, m + 5, F32, gpu, 0, A.t()); a_si, a_sk = 1, m + 5
    if bl == 'kn':
        Bg = gp.Guarded(k, n, n + 1, F32, gpu, 0, B); b_sk, b_sj = n + 1, 1
    else:
        Bg = gp.Guarded(n, k, k + 2, F32, gpu, 0, B.t()); b_sk, b_sj = 1, k + 2
    D = gp.Guarded(m, n, n + 4, F32, gpu)
    u = torch.rand(m, generator=gen, device=gpu) if rank1 else None
    v = gp.rand_operand((n,), gen, gpu) if rank1 else None
    nws = lib.apa_probe_sgemm_ws_bytes(m, n, splits) // 4
    ws = gp.Guarded(1, nws, nws, F32, gpu) if nws else None
    for g in (D, ws):
        if g is not None:
            g.snapshot()

    def run():
        rc = lib.apa_probe_sgemm_small(Ag.ptr, a_si, a_sk, Bg.ptr, b_sk, b_sj, D.ptr, n + 4, m, n, k, splits,
                                       u.data_ptr() if rank1 else None, v.data_ptr() if rank1 else None,
                                       ws.ptr if ws else None, gp.stream_ptr())
        torch.cuda.synchronize()
        assert rc == gp.APA_OK, lib.apa_probe_last_error()

    run()
    ref = A.double() @ B.double()
    mag = A.double().abs() @ B.double().abs()
    if rank1:
        t = u.double()[:, None] * v.double()[None, :]
        ref, mag = ref + t, mag + t.abs()
    bound = gp.C_ACC * (k + 8) * gp.EPS32 * mag
    assert float(bound.max()) < 0.01 * float(ref.abs().max())
    out = D.view.double()
    assert torch.isfinite(out).all(), name
    assert ((out - ref).abs() <= bound).all(), (name, float((out - ref).abs().max()))
    D.check_guards(name + ' D')
    if ws is not None:
        ws.check_guards(name + ' workspace')
    first = D.bits()
    D.restore()
    run()
    assert torch.equal(D.bits(), first), name + ': repeated call differs'
