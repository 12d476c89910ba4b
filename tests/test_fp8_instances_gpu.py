"""Every instance, lane occupancy and chunk-loop trip count of the two FP8 streaming kernels (csrc/apa_m1_fp8.hip)
against float64, case by case of tests/_fp8_cases.py (whose reach table tests/test_fp8_instances_cpu.py asserts).

A case runs the forward and the backward entry point twice through the probe library -- apa_probe_m1_fwd_ex / _bwd_ex
for a plain batch, apa_probe_m1_fwd_cached / _bwd_cached for an index into the T = 7 cache, so the trace is that of the
entry point that served the call -- with every output and the workspace in NaN-guarded allocations:
  * the conditions on the inputs (the 1 % rule of every bound, the relu gates) are asserted first, from the float64
    reference alone;
  * the trace names the FP8 family in both passes and the head / logits route the library's predicates predict;
  * the two runs repeat bit for bit, no guard moves, the cache's bytes are what they were;
  * the outputs lie within the error model of tests/_m1_probe.py on the exactly dequantised input
    (tests/test_fp8_features_gpu._check_against_float64), the mask replayed from apa_dropout_mask;
  * a gathered case equals the plain call on cache.gather(index) bit for bit.
Each case prints its largest |got - ref| / bound per output before it asserts (profiles/fp8_rank_instances_summary.md)."""
import ctypes

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _fp8_cases as fc
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests import test_fp8_features_gpu as f8t
from tests import test_m1_paths_gpu as m1p

pytestmark = pytest.mark.gpu

FP8 = cof.APA_DTYPE_FP8_E4M3
OUTPUTS = ('logits', 'att', 'zsave', 'abar', 'dWa', 'dba', 'dWt', 'dbt')

_PROBE = None


def _probe():
    global _PROBE
    if _PROBE is None:
        lib = mp.load_m1_probe()
        for probe, prod in (('apa_probe_m1_fwd_cached', 'apa_attn_pool_fwd_cached'),
                            ('apa_probe_m1_bwd_cached', 'apa_attn_pool_bwd_cached')):
            fn = getattr(lib, probe)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_void_p] + list(cof._SIGNATURES[prod][1])
        _PROBE = lib
    return _PROBE


class _Run:
    """The NaN-guarded buffers of one call pair on `feat` (an Fp8Features) read directly or through `index`."""

    def __init__(self, c, inp, feat, index, dev):
        N, P, C, K = c['N'], c['P'], c['C'], c['K']
        self.c, self.inp, self.feat, self.index = c, inp, feat, index
        f32, Gd = torch.float32, gp.Guarded
        self.out = {'logits': Gd(N, K, K, f32, dev), 'att': Gd(N, P, P, f32, dev), 'zsave': Gd(N, C, C, f32, dev),
                    'abar': Gd(1, N, N, f32, dev), 'dWa': Gd(1, C, C, f32, dev), 'dba': Gd(1, 1, 1, f32, dev),
                    'dWt': Gd(C, K, K, f32, dev), 'dbt': Gd(1, K, K, f32, dev)}
        self.G = Gd(N, K, K, f32, dev, data=inp['G'])
        self.flags = (cof.APA_FLAG_RELU_ATT if c['act'] == 'relu' else 0) | (cof.APA_FLAG_TRAIN if c['train'] else 0)
        self.ws_bytes = int(cof.attn_pool_workspace_bytes(N, P, C, C, K, 1, self.flags))
        self.ws = Gd(1, (self.ws_bytes + 3) // 4, (self.ws_bytes + 3) // 4, f32, dev)
        self.status = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.desc = None if index is None else cof.ApaFeatureCache(index.data_ptr(), feat.shape[0], 0,
                                                                   self.status.data_ptr())
        for b in self._all():
            b.snapshot()

    def _all(self):
        return list(self.out.values()) + [self.G, self.ws]

    def run(self):
        """forward, then backward -> (forward trace, backward trace)"""
        c, inp, lib, o = self.c, self.inp, _probe(), self.out
        X = self.feat.data_ptr()
        par = (None, X, X, inp['Wa'].data_ptr(), inp['ba'].data_ptr(), inp['Wt'].data_ptr(), inp['bt'].data_ptr())
        dims = (c['N'], c['P'], c['C'], c['C'], c['K'], 1)
        tail = (fc.KEEP, fc.SEED, fc.OFFSET, FP8, gp.stream_ptr())
        tf, tb = mp.M1Trace(), mp.M1Trace()
        fwd, bwd = (lib.apa_probe_m1_fwd_ex, lib.apa_probe_m1_bwd_ex) if self.desc is None else \
            (lib.apa_probe_m1_fwd_cached, lib.apa_probe_m1_bwd_cached)
        head = (ctypes.addressof(tf),) if self.desc is None else (ctypes.addressof(tf), ctypes.addressof(self.desc))
        rc = fwd(*head, *par, o['logits'].ptr, o['att'].ptr, o['zsave'].ptr, o['abar'].ptr, None, self.ws.ptr,
                 self.ws_bytes, *dims, self.flags, *tail)
        assert rc == 0, lib.apa_last_error()
        head = (ctypes.addressof(tb),) + head[1:]
        rc = bwd(*head, *par, o['att'].ptr, o['zsave'].ptr, o['abar'].ptr, self.G.ptr, None, None, o['dWa'].ptr,
                 o['dba'].ptr, o['dWt'].ptr, o['dbt'].ptr, self.ws.ptr, self.ws_bytes, *dims,
                 self.flags | cof.APA_FLAG_FROZEN_INPUT, *tail)
        assert rc == 0, lib.apa_last_error()
        torch.cuda.synchronize()
        for k, b in self.out.items():
            b.check_guards(k)
        self.G.check_guards('G')
        self.ws.check_guards('workspace')
        return tf, tb

    def restore(self):
        for b in self._all():
            b.restore()

    def bits(self):
        return {k: b.bits() for k, b in self.out.items()}

    def got(self):
        d = {k: b.view.clone() for k, b in self.out.items()}
        d['G'] = self.G.view.clone()
        return d


def _ratio(got, b):
    """largest |got - ref| / bound over the elements (an element with a zero bound must be exact)"""
    err = (got.double().reshape(b.ref.shape) - b.ref).abs()
    tol = mp.tolerance(b)
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    return float(r.max())


@pytest.mark.parametrize('c', fc.CASES, ids=[c['name'] for c in fc.CASES])
def test_fp8_instance(gpu, c):
    nv = mp.fp8_instance(c['C'])
    inp = fc.inputs(c, gpu)
    N, P, C, K = c['N'], c['P'], c['C'], c['K']
    mask = cof.dropout_mask((N * P * C,), fc.KEEP, fc.SEED, fc.OFFSET) if c['train'] else None
    mc = fc.model_case(c)
    with torch.no_grad():       # the conditions, from the inputs alone, before any kernel output is looked at
        ref_f, amb, figures = fc.check_conditions(c, inp, mask, m1p._forward_ref, m1p._backward_ref)
    print('FP8CASE {} NV={} S={} trips={} conditions={}'.format(
        c['name'], nv, fc.blocks(c)[0], sorted(fc.trip_counts(c)[0]),
        {k: (tuple(None if x is None else round(x, 4) for x in v) if isinstance(v, tuple) else round(v, 5))
         for k, v in figures.items()}))

    f8 = inp['f8']
    before = f8.buffer.clone()
    r = _Run(c, inp, f8, inp['index'], gpu)
    tf, tb = r.run()
    first, got = r.bits(), r.got()
    # the trace of the entry point that served the call
    S, ppb, nblk, _ = mp.plan(N, P, C, C, K)
    logits, head = fc.routes(c)
    tr = mp.merge(tf, tb)
    exp = dict(pool_fwd='fp8', pool_bwd='fp8', S=S, ppb=ppb, nblk=nblk, fused=1, logits=logits, head=head,
               reduce='colsum' if head in ('tiles', 'rows', 'small') else 'bwd_reduce')
    bad = {k: (tr[k], v) for k, v in exp.items() if tr[k] != v}
    assert not bad, 'trace mismatch (got, expected): {} in {}'.format(bad, tr)
    # two runs, bit for bit; the cache is read-only
    r.restore()
    tf2, tb2 = r.run()
    assert mp.merge(tf2, tb2) == tr
    second = r.bits()
    for k in OUTPUTS:
        assert torch.equal(first[k], second[k]), '{} differs between two identical calls'.format(k)
    assert torch.equal(f8.buffer, before), 'the call wrote into the features'
    assert int(r.status) == 0

    # float64: the figures first, then the assertions
    with torch.no_grad():
        ref_b = m1p._backward_ref(mc, inp, got, mask)
        ratios = {k: _ratio(got[k], ref_f[k]) for k in ('zsave', 'abar', 'logits')}
        att_err = (got['att'].double().reshape(N, P) - ref_f['att'].ref).abs()
        att_tol = mp.tolerance(ref_f['att'])
        ratios['att'] = float((att_err / att_tol.clamp_min(1e-300))[att_tol > 0].max())
        ratios.update({k: _ratio(got[k], ref_b[k]) for k in ('dWa', 'dba', 'dWt', 'dbt')})
        print('FP8RATIO {} {}'.format(c['name'], ' '.join('{}={:.4f}'.format(k, ratios[k]) for k in OUTPUTS)))
        f8t._check_against_float64(mc, inp, got, mask)

    # a gathered call equals the plain call on the gathered copy
    if c['gathered']:
        copy = cof.Fp8Features.from_parts(f8.codes[inp['index'].long()], f8.scale[inp['index'].long()])
        p = _Run(c, inp, copy, None, gpu)
        p.run()
        plain = p.bits()
        for k in OUTPUTS:
            assert torch.equal(first[k], plain[k]), '{}: the gathered call differs from the call on the copy'.format(k)
