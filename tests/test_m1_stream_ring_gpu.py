"""The chunk ring of the two M == 1 streaming passes (csrc/apa_m1_stream.hip) at the smallest shapes that reach every
way through it: whole turns of the two-slot ring, a turn left after its first chunk, a last chunk with surplus slots.

m1_plan turns P = 5 / 9 / 12 into blocks of 5 / 5 and 4 / 4 pixels.  With one-pixel chunks (fp32, C = 1024: VW 1,
C = 2048: VW 2) that is 5 and 4 chunks -- an odd count, which leaves the ring in the middle of a turn, and an even
one; with two-pixel chunks (bf16, C = 2048) 3 and 2 chunks, the third one half empty.  Every case crosses the
attention activation (softmax is an instance of its own, identity and relu share one and differ by a select) with
training at keep 0.2 / 0.5 and evaluation, and runs its backward pass twice: with dX and under APA_FLAG_FROZEN_INPUT
(the instances without the dX stores).  bf16 training also runs through the one-call step, whose backward half reads
the forward half's keep bits.  The concatenated pose channels (csrc/apa_m1_cat.hip) are the only caller that hands
the backward pass a non-zero `extra_scale`: P = 5 and P = 9 put a non-zero extra term into both ring slots.

The harness, the float64 references with their error bounds and the tolerances are those of
tests/test_m1_paths_gpu.py / tests/_m1_probe.py, unchanged.  Every run is repeated and must come back byte for byte.
"""
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests import test_m1_paths_gpu as T

pytestmark = pytest.mark.gpu

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
FROZEN = cof.APA_FLAG_FROZEN_INPUT
K = 5
PPB = {5: 5, 9: 5, 12: 4}                      # pixels of the largest block (m1_plan)
SHAPES = [('f32_c1024', F32, 1024, 1, 1), ('f32_c2048', F32, 2048, 2, 1), ('bf16_c2048', BF16, 2048, 1, 2)]
MODES = [('train_keep02', True, 0.2), ('train_keep05', True, 0.5), ('eval', False, 0.5)]


def _cases():
    out = []
    for sname, dt, C, vw, pix in SHAPES:
        for N in (2, 3):
            for P in (5, 9, 12):
                for act in ('id', 'relu', 'softmax'):
                    for mname, train, keep in MODES:
                        entries = ('sep', 'step') if (dt == BF16 and train) else ('sep',)
                        for entry in entries:
                            name = '{}_n{}_p{}_{}_{}_{}'.format(sname, N, P, act, mname, entry)
                            exp = dict(pool_fwd='stream', pool_bwd='stream', fwd_w=vw, bwd_w=vw, fwd_pix=pix,
                                       bwd_pix=pix, ppb=PPB[P])
                            if train:          # the keep bits: bf16, handed over inside the step only
                                exp['keep_bits'] = int(entry == 'step')
                            out.append(T.case(name, N, P, C, K, dt=dt, act=act, train=train, keep=keep, entry=entry,
                                              **exp))
    return out


CASES = _cases()
# the concatenated channels: fp32 C = 2048, J = 4; an odd chunk count (P = 5) and blocks of 5 and 4 (P = 9)
CAT_CASES = [
    T.case('cat_f32_c2048_n2_p5_id_train', 2, 5, 2048, K, train=True, keep=0.5, J=4, pool_fwd='stream',
           pool_bwd='stream', ppb=5, cat_fwd=4, cat_bwd=4),
    T.case('cat_f32_c2048_n3_p9_softmax_train', 3, 9, 2048, K, act='softmax', train=True, keep=0.2, J=4,
           pool_fwd='stream', pool_bwd='stream', ppb=5, cat_fwd=4, cat_bwd=4),
    T.case('cat_f32_c2048_n2_p9_relu_eval', 2, 9, 2048, K, act='relu', J=4, pool_fwd='stream', pool_bwd='stream',
           ppb=5, cat_fwd=4, cat_bwd=4),
]


def _run_twice(r):
    """-> (trace, outputs as bits) of a run that repeats byte for byte."""
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    first = r.bits()
    r.restore()
    trace2 = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace2 == trace
    second = r.bits()
    for k in first:
        assert torch.equal(first[k], second[k]), '{} differs between two identical calls'.format(k)
    return trace, second


def _check_against_float64(c, r, inp):
    got = {k: b.view.clone() for k, b in r.out.items()}
    with torch.no_grad():
        fref, amb = T._forward_ref(c, inp, r.mask)
        if amb is not None:
            assert int(amb.sum()) <= max(2, amb.numel() // 100), 'too many relu gates at zero: {}'.format(
                int(amb.sum()))
        T._check_forward(c, got, fref, amb)
        T._check_backward(c, got, T._backward_ref(c, inp, got, r.mask))
        if c['entry'] == 'step':
            T._check_loss(c, got, inp)


def _check_trace(c, trace):
    S, ppb, nblk, _ = mp.plan(c['N'], c['P'], c['C'], c['C'], c['K'])
    assert (S, ppb) == (trace['S'], trace['ppb'])
    bad = {k: (trace[k], v) for k, v in c['expect'].items() if trace[k] != v}
    assert not bad, 'trace mismatch (got, expected): {} in {}'.format(bad, trace)


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_ring(gpu, c):
    lib = mp.load_m1_probe()
    torch.manual_seed(0)
    inp = T._inputs(c, gpu)
    r = T._Run(c, inp, gpu, lib)
    trace, full = _run_twice(r)
    _check_trace(c, trace)
    _check_against_float64(c, r, inp)

    # the instances without the dX stores: a sentinel-filled, guard-padded dX stays as it is, the rest is the same bits
    r.restore()
    r.flags |= FROZEN
    trace_f, frozen = _run_twice(r)
    assert trace_f == trace
    dx = r.out['dX']
    assert torch.equal(dx.base.view(gp._INT_VIEW[dx.dtype]), dx.snap), 'the flagged call wrote to dX'
    for k in full:
        if k != 'dX':
            assert torch.equal(full[k], frozen[k]), '{} differs from the unflagged run'.format(k)


@pytest.mark.parametrize('c', CAT_CASES, ids=[c['name'] for c in CAT_CASES])
def test_ring_extra_term(gpu, c):
    """extra_scale != 0: the pose channels' share of dA enters every chunk, in both ring slots."""
    lib = mp.load_m1_probe()
    torch.manual_seed(0)
    inp = T._inputs(c, gpu)
    r = T._Run(c, inp, gpu, lib)
    trace, _ = _run_twice(r)
    _check_trace(c, trace)
    _check_against_float64(c, r, inp)
