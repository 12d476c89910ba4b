"""The paired form of the M == 1 forward streaming pass (csrc/apa_m1_stream.hip): with fp32 features, where the plan's
S is even and the attention is not a softmax, the two logical blocks (n, 2s') and (n, 2s' + 1) run as the two quads of
ONE 512-thread block and leave ONE partial row, acc0 + acc1, at row n S/2 + s'.  bf16 features and the backward pass
keep one block and one row per logical block (PAIR_FWD / PAIR_BWD below state the rule by hand; measured:
profiles/paired_rows_summary.md) -- the same cases then hold their rows to the forced form entry for entry.

1. Rows, bit for bit: every case runs the forward and the backward call as the library picks them and, through the probe
   library's apa_probe_m1_fwd_unpaired / apa_probe_m1_bwd_unpaired, with pairing forced off, on the same inputs (the
   backward call's G included: the one-call step's G already follows the merged rows) and the same dropout counter.
   A paired pacc row s' equals unpaired row[2s'] + row[2s' + 1] added in fp32 on the host (quad 0 on the left); an
   unpaired pass gives the rows as before; pdwa, pdba and pstat entry for entry, and att and dX are equal.
2. End to end: the train step and the evaluation step, on every paired shape of CASES, against the float64
   restatement and the bounds of tests/test_m1_paths_gpu.py (imported, not restated), fp32 and bf16.
3. Coverage: each case asserts, from the plan (m1_plan, m1_pix_range restated) and the probe's row counts, that it took
   the form it claims -- paired or not, and which quad of which pair ran short of barriers.

m1_pix_range gives split s the pixels [s P / S, (s + 1) P / S) (floors), so at (N, P) = (2, 9), S = 2, the runs are
4 and 5 pixels: it is quad 0 that runs one chunk short there (fp32: 4 / 5 chunks); quad 1 is the short one in pair 1 of
P = 26, S = 6 (runs 4 4 | 5 4 | 4 5), which holds both kinds and an equal pair at once.
"""
import ctypes

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests import test_feature_cache_gpu as fct
from tests import test_m1_paths_gpu as m1p

pytestmark = pytest.mark.gpu

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
K_SMALL = 20
# which pass takes the paired form, by feature type (m1_call_fill; measured: profiles/paired_rows_summary.md)
PAIR_FWD = {F32: True, BF16: False}
PAIR_BWD = {F32: False, BF16: False}


def _up(x):
    return (x + 255) // 256 * 256


def _carve(N, P, C, K):
    """byte offsets of pacc, pstat, pdwa, pdba in the workspace (m1_plan's carve, fused: Ca == C)"""
    S, ppb, nblk, _ = mp.plan(N, P, C, C, K)
    off, out = 0, {}
    for name, size in (('pacc', nblk * C * 4), ('pstat', nblk * 16), ('pdwa', nblk * C * 4), ('pdba', (nblk + N) * 4)):
        out[name] = off
        off += _up(size)
    return out


def _runs(P, S):
    return [(s + 1) * P // S - s * P // S for s in range(S)]


def _pix(c):
    return 2 if c['dt'] == BF16 or c['C'] == 4096 else 1      # kPix (apa_m1_stream.hip)


def _short_quads(c, S):
    """per pair: 0 / 1 = the quad with fewer chunks, None = equal"""
    pix = _pix(c)
    ch = [(r + pix - 1) // pix for r in _runs(c['P'], S)]
    return [None if ch[2 * i] == ch[2 * i + 1] else (0 if ch[2 * i] < ch[2 * i + 1] else 1) for i in range(S // 2)]


def _lib():
    lib = mp.load_m1_probe()
    for probe, prod in (('apa_probe_m1_fwd_unpaired', 'apa_attn_pool_fwd_ex'),
                        ('apa_probe_m1_bwd_unpaired', 'apa_attn_pool_bwd_ex')):
        fn = getattr(lib, probe)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] + list(cof._SIGNATURES[prod][1])
    lib.apa_probe_m1_rows.argtypes = [ctypes.c_void_p]
    lib.apa_probe_m1_rows.restype = None
    return lib


def _rows(lib):
    out = (ctypes.c_int64 * 2)()
    lib.apa_probe_m1_rows(out)
    return int(out[0]), int(out[1])


def pcase(name, N, P, C, *, K=K_SMALL, S, even, short=None, extra=0, **kw):
    """even: an even S without a softmax in the pooling kernel, the shapes the paired form exists for; `paired`: the
    forward pass of the case takes it (fp32); `short`: per pair, the quad that runs short -- stated for paired cases only"""
    c = m1p.case(name, N, P, C, K, entry='step', **kw)
    c.update(S_expect=S, even=even, paired=even and PAIR_FWD[c['dt']], short=short, extra=extra)
    assert (short is not None) == c['paired']
    return c


# (name, N, P, C; S and the short quads are asserted against the plan, not trusted)
CASES = [
    pcase('unequal_f32', 2, 9, 2048, S=2, even=True, short=[0], train=True),
    pcase('unequal_bf16', 2, 9, 2048, S=2, even=True, train=True, dt=BF16),
    pcase('both_short_f32', 2, 26, 2048, S=6, even=True, short=[None, 1, 0], train=True),
    pcase('both_short_bf16', 2, 26, 2048, S=6, even=True, train=True, dt=BF16, act='relu'),
    pcase('equal_f32', 2, 8, 2048, S=2, even=True, short=[None], train=True),
    pcase('equal_bf16', 2, 8, 2048, S=2, even=True, train=True, dt=BF16),
    pcase('ragged_last_pair_c1024', 3, 25, 1024, S=6, even=True, short=[None, None, 0], train=True, act='relu'),
    pcase('odd_S', 2, 12, 2048, S=3, even=False, train=True),
    pcase('vw4_c4096', 2, 9, 4096, S=2, even=True, short=[0], train=True),
    pcase('vw4_c4096_quad1_short', 2, 26, 4096, S=6, even=True, short=[None, 1, 0], train=True),   # chunks 2 2 | 3 2 | 2 3
    pcase('relu_input', 2, 9, 2048, S=2, even=True, short=[0], train=True, relu_in=True),
    pcase('relu_input_bf16', 2, 26, 2048, S=6, even=True, train=True, relu_in=True, dt=BF16),
    pcase('eval_mode_f32', 2, 26, 2048, S=6, even=True, short=[None, 1, 0]),
    pcase('eval_mode_bf16', 2, 9, 2048, S=2, even=True, dt=BF16),
    pcase('frozen_input_f32', 2, 26, 2048, S=6, even=True, short=[None, 1, 0], train=True,
          extra=cof.APA_FLAG_FROZEN_INPUT),
    pcase('frozen_input_bf16', 2, 9, 2048, S=2, even=True, train=True, dt=BF16,
          extra=cof.APA_FLAG_FROZEN_INPUT),
    pcase('softmax', 2, 26, 2048, S=6, even=False, train=True, act='softmax'),
    pcase('headline', 32, 196, 2048, K=393, S=16, even=True,
          short=[None, 0, None, 0, None, 0, None, 0], train=True),   # runs 12 12 | 12 13 | ...
]


def _sep(r, lib, unpaired):
    """the forward and the backward call of _Run r (G: the case's own), paired or with pairing forced off
    -> (fwd trace, bwd trace, (fwd rows, bwd rows))"""
    c, inp = r.c, r.inp
    X = inp['X'].data_ptr()
    seed, offset, flags = r.key()
    flags |= c['extra']
    fwd = lib.apa_probe_m1_fwd_unpaired if unpaired else lib.apa_probe_m1_fwd_ex
    bwd = lib.apa_probe_m1_bwd_unpaired if unpaired else lib.apa_probe_m1_bwd_ex
    t1, t2 = mp.M1Trace(), mp.M1Trace()
    par = (inp['Wa'].data_ptr(), inp['ba'].data_ptr(), r.Wt.ptr, inp['bt'].data_ptr())
    rc = fwd(ctypes.byref(t1), None, X, X, *par, r.p('logits'), r.p('att'), r.p('zsave'), r.p('abar'), None, r.ws.ptr,
             r.ws_bytes, r.N, r.P, r.C, r.C, r.K, 1, flags, c['keep'], seed, offset, c['dt'], gp.stream_ptr())
    assert rc == 0, lib.apa_last_error()
    rc = bwd(ctypes.byref(t2), None, X, X, *par, r.p('att'), r.p('zsave'), r.p('abar'), r.p('G'), r.p('dX'), None,
             r.p('dWa'), r.p('dba'), r.p('dWt'), r.p('dbt'), r.ws.ptr, r.ws_bytes, r.N, r.P, r.C, r.C, r.K, 1, flags,
             c['keep'], seed, offset, c['dt'], gp.stream_ptr())
    assert rc == 0, lib.apa_last_error()
    torch.cuda.synchronize()
    r.check_guards()
    assert mp.POOLS[t1.pool_fwd] == 'stream' and mp.POOLS[t2.pool_bwd] == 'stream'
    return t1, t2, _rows(lib)


def _ws_rows(r, carve, nblk):
    w = r.ws.view.reshape(-1)
    C, f = r.C, lambda k: carve[k] // 4
    return dict(pacc=w[f('pacc'):f('pacc') + nblk * C].reshape(nblk, C).clone(),
                pstat=w[f('pstat'):f('pstat') + nblk * 4].reshape(nblk, 4).clone(),
                pdwa=w[f('pdwa'):f('pdwa') + nblk * C].reshape(nblk, C).clone(),
                pdba=w[f('pdba'):f('pdba') + nblk].clone())


def _check_backward(c, got, ref):
    """m1p._check_backward; under APA_FLAG_FROZEN_INPUT dX is not written, so the helper is handed the reference in its
    place and checks every other gradient as it does everywhere else (the helper itself cannot change)"""
    if c['extra'] & cof.APA_FLAG_FROZEN_INPUT:
        got = dict(got, dX=ref['dX'].ref.clone())
    m1p._check_backward(c, got, ref)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_paired_rows_and_step(gpu, c):
    lib = _lib()
    N, P, C, K = c['N'], c['P'], c['C'], c['K']
    S, ppb, nblk, _ = mp.plan(N, P, C, C, K)
    # 3. the form the case claims, from the plan
    assert S == c['S_expect'] and nblk == N * S
    assert mp.support(N, C, K, c['dt']) & mp.SUP_STREAM
    assert c['even'] == (S % 2 == 0 and c['act'] != 'softmax')
    if c['paired']:
        assert _short_quads(c, S) == c['short'], (_runs(P, S), _short_quads(c, S))
    inp = m1p._inputs(c, gpu)
    cs = dict(c, entry='sep')
    r = m1p._Run(cs, inp, gpu, lib)
    carve = _carve(N, P, C, K)

    t1, t2, rows = _sep(r, lib, unpaired=False)
    for t in (t1, t2):
        assert (t.S, t.ppb, t.nblk) == (S, ppb, nblk), 'the trace reports the logical plan'
    pf, pb = c['paired'] and PAIR_FWD[c['dt']], c['paired'] and PAIR_BWD[c['dt']]
    want_rows = (nblk // 2 if pf else nblk, nblk // 2 if pb else nblk)
    assert rows == want_rows, 'rows written (fwd, bwd): {} expected {}'.format(rows, want_rows)
    got = {k: b.view.clone() for k, b in r.out.items()}
    wp = _ws_rows(r, carve, nblk)

    r.restore()
    _, _, rows_u = _sep(r, lib, unpaired=True)
    assert rows_u == (nblk, nblk)
    got_u = {k: b.view.clone() for k, b in r.out.items()}
    wu = _ws_rows(r, carve, nblk)

    # 1. rows, bit for bit
    assert torch.equal(wp['pstat'], wu['pstat']), 'pstat'
    assert torch.equal(got['att'], got_u['att']), 'att'
    assert torch.equal(got['dX'].view(torch.uint8), got_u['dX'].view(torch.uint8)), 'dX'
    h = nblk // 2
    for k, pair in (('pacc', pf), ('pdwa', pb), ('pdba', pb)):
        if pair:
            assert torch.equal(wp[k][:h], wu[k][0::2] + wu[k][1::2]), '{}: paired row != row[2s] + row[2s + 1]'.format(k)
        else:
            assert torch.equal(wp[k], wu[k]), '{}: the unpaired form must give the rows as before'.format(k)
    if not pf and not pb:                      # neither pass paired: every output as with the forced form
        for k in got:
            assert torch.equal(got[k].view(torch.uint8), got_u[k].view(torch.uint8)), k

    # 2. end to end against float64: the two calls above (paired), then the one-call train step
    with torch.no_grad():
        fref, amb = m1p._forward_ref(cs, inp, r.mask)
        if amb is not None:
            assert int(amb.sum()) <= max(2, amb.numel() // 100)
        m1p._check_forward(cs, got, fref, amb)
        bref = m1p._backward_ref(cs, inp, got, r.mask)
        _check_backward(cs, got, bref)
    del r, got, got_u, wp, wu, bref

    r = m1p._Run(c, inp, gpu, lib)
    r.flags |= c['extra']
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace['pool_fwd'] == 'stream' and trace['pool_bwd'] == 'stream' and _rows(lib) == want_rows
    assert trace['keep_bits'] == int(c['dt'] == BF16 and c['train'] and not c['relu_in'])
    got = {k: b.view.clone() for k, b in r.out.items()}
    with torch.no_grad():
        m1p._check_forward(c, got, fref, amb)
        bref = m1p._backward_ref(c, inp, got, r.mask)
        _check_backward(c, got, bref)
        m1p._check_loss(c, got, inp)


# the evaluation step on every even-S shape of CASES, fp32 (paired) and bf16 (one block per logical block) (each shape, feature type, attention and input form once)
EVAL_CASES = [m1p.case('eval_step_' + c['name'], c['N'], c['P'], c['C'], c['K'], entry='eval', dt=c['dt'], act=c['act'],
                       relu_in=c['relu_in'])
              for c in CASES if c['even'] and not c['extra'] and not c['name'].startswith('eval_mode')]


@pytest.mark.parametrize('c', EVAL_CASES, ids=[c['name'] for c in EVAL_CASES])
def test_eval_step_paired(gpu, c):
    lib = _lib()
    S, ppb, nblk, _ = mp.plan(c['N'], c['P'], c['C'], c['C'], c['K'])
    assert S % 2 == 0
    inp = m1p._inputs(c, gpu)
    r = m1p._Run(c, inp, gpu, lib)
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace['pool_fwd'] == 'stream' and (trace['S'], trace['nblk']) == (S, nblk)
    assert trace['fwd_w'] == c['C'] // (1024 if c['dt'] == F32 else 2048) and trace['fwd_pix'] == _pix(c)
    assert _rows(lib)[0] == (nblk // 2 if PAIR_FWD[c['dt']] else nblk)
    got = {k: b.view.clone() for k, b in r.out.items()}
    got['pred'] = r.pred.clone()
    with torch.no_grad():
        fref, amb = m1p._forward_ref(c, inp, None)
        if amb is not None:
            assert int(amb.sum()) <= max(2, amb.numel() // 100)
        m1p._check_forward(c, got, fref, amb)
        m1p._check_loss(c, got, inp)


def test_paired_forward_with_a_separate_attention_input(gpu):
    """Xatt != X, fp32: the (FUSED = false) PAIR instance of the forward pass -- no block_dots, so no chunk barrier and
    no surplus-barrier loop, only the merge barrier -- on unequal quads either way round (runs 4 4 | 5 4 | 4 5).  Rows
    against the forced form bit for bit, then both calls against float64.  The backward pass writes no rows of its own."""
    lib = _lib()
    c = m1p.case('separate_att_f32', 2, 26, 2048, K_SMALL, Ca=64, act='relu', train=True)
    N, P, C, K, Ca = c['N'], c['P'], c['C'], c['K'], c['Ca']
    S, ppb, nblk, _ = mp.plan(N, P, C, Ca, K)
    assert S == 6 and _runs(P, S) == [4, 4, 5, 4, 4, 5]
    carve = _carve(N, P, C, K)
    inp = m1p._inputs(c, gpu)
    r = m1p._Run(c, inp, gpu, lib)
    f = lambda k: carve[k] // 4

    def rows_of():
        w = r.ws.view.reshape(-1)
        return (w[f('pacc'):f('pacc') + nblk * C].reshape(nblk, C).clone(),
                w[f('pstat'):f('pstat') + nblk * 4].reshape(nblk, 4).clone())

    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace['pool_fwd'] == 'stream' and trace['fused'] == 0 and _rows(lib) == (nblk // 2, nblk)
    got = {k: b.view.clone() for k, b in r.out.items()}
    pacc, pstat = rows_of()
    r.restore()
    lib.apa_probe_m1_set_iflags.argtypes = [ctypes.c_uint]
    lib.apa_probe_m1_set_iflags(1 << 29)           # APA_IFLAG_UNPAIRED
    try:
        r.run()
    finally:
        lib.apa_probe_m1_set_iflags(0)
    torch.cuda.synchronize()
    r.check_guards()
    assert _rows(lib) == (nblk, nblk)
    pacc_u, pstat_u = rows_of()
    assert torch.equal(pstat, pstat_u) and torch.equal(got['att'], r.out['att'].view)
    assert torch.equal(pacc[:nblk // 2], pacc_u[0::2] + pacc_u[1::2]), 'pacc: paired row != row[2s] + row[2s + 1]'
    assert torch.equal(got['dX'], r.out['dX'].view)
    with torch.no_grad():
        fref, amb = m1p._forward_ref(c, inp, r.mask)
        m1p._check_forward(c, got, fref, amb)
        m1p._check_backward(c, got, m1p._backward_ref(c, inp, got, r.mask))


def test_gathered_call_paired_equals_the_call_on_a_gathered_copy(gpu):
    """one cached (GATHER) call, paired, against the plain call on cache.gather(index), bit for bit"""
    lib = _lib()
    P, C, K = 49, 1024, K_SMALL
    index = fct.INDEX
    N = len(index)
    S, _, nblk, _ = mp.plan(N, P, C, C, K)
    assert S % 2 == 0 and S >= 4
    cache = fct._cache(torch.float32, P, C, gpu)
    p = fct._params(C, K, 'relu', cache, gpu)
    g = torch.Generator().manual_seed(3)
    G = ((torch.rand(N, K, generator=g) * 1.25 - 0.25) / N).to(gpu)
    flags = fct._flags('relu', True)
    ref = fct._separate(cache.gather(index), p, G, flags)
    fam = fct._traced_families(cache.select(index), p, G, flags, ref)      # asserts the outputs equal ref's
    assert fam == (fct.POOL_STREAM, fct.POOL_STREAM)
    assert _rows(lib) == (nblk // 2 if PAIR_FWD[F32] else nblk, nblk // 2 if PAIR_BWD[F32] else nblk)
