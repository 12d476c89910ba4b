"""The folded M == 1 forward (csrc/apa_m1_small.hip m1_logits2_fold_kernel: the partial merge of
m1_finalize_fwd_kernel in the partial-logits kernel's prologue, abar formed by the logits reducer) against the
two-launch sequence it replaces, bit for bit.

Every case runs the same inputs twice through the test-only probe library: once with APA_IFLAG_FINALIZE_LAUNCH
(apa_internal.h) set, which keeps the finalize kernel a launch of its own, once as the product runs it.  Both runs
write NaN-guarded buffers; every output -- zsave, abar, att, logits, and through the one-call steps loss, G, probs,
pred, dX, dWa, dba, dWt, dbt -- must be byte-equal, and the route each run took (apa_probe_m1_fwd_route) is asserted:
folded where m1_forward's conditions hold (identity / relu attention, S <= 16, N < 128, C % 64 == 0), else the two
launches in both runs.  tests/test_m1_paths_gpu.py compares the default route of the shipped shapes with float64.

Shapes: the smallest that reach each edge of the folded kernel (8-image groups, two k-tile groups of KG tiles, at most
16 splits): a ragged single image group with S = 12 from the P / 4 cap and one k-tile; an image group of 1 with a
ragged last k-tile (N = 33, P = 49 -- the N = 9, P = 196 shape has S = 49 by m1_plan and so checks the unfolded route
of a ragged batch); the cfg 002 shape in fp32 and bf16; S = 9 on the per-pixel pooling family.
"""
import ctypes

import pytest
import torch

from tests import _m1_probe as mp
from tests.test_m1_paths_gpu import BF16, F32, _inputs, _Run, case

pytestmark = pytest.mark.gpu

APA_IFLAG_FINALIZE_LAUNCH = 1 << 27      # csrc/apa_internal.h

SHAPES = [
    # name, N, P, C, K, dtype
    ('n3_p49_c1024_k16', 3, 49, 1024, 16, F32),          # S = 12 (P / 4), one ragged image group, one k-tile (KG 1)
    ('n9_p196_c2048_k393', 9, 196, 2048, 393, F32),      # S = 49: not folded
    ('n33_p49_c2048_k393', 33, 49, 2048, 393, F32),      # S = 12, image group of 1, 25 k-tiles = 13 + 12, the last ragged
    ('n32_p196_c2048_k393', 32, 196, 2048, 393, F32),    # cfg 002: S = 16, 256 blocks
    ('n32_p196_c2048_k393_bf16', 32, 196, 2048, 393, BF16),
    ('n40_p36_c512_k51', 40, 36, 512, 51, F32),          # S = 9, per-pixel pooling family, KG 2 x 2 groups
]
# entry, activation, training: the three-call path (plain reducer), the one-call training step (keep 0.2) and the
# one-call evaluation step (reducers with the row's cross-entropy / probabilities)
ENTRIES = [('sep', 'relu', False), ('step', 'id', True), ('eval', 'id', False)]
CASES = [case('fold_{}_{}'.format(name, entry), N, P, C, K, dt=dt, act=act, train=train, keep=0.2, entry=entry)
         for name, N, P, C, K, dt in SHAPES for entry, act, train in ENTRIES]
# the default must still be the two launches: softmax attention, S > 16, N = 128 (S = 4: only the batch size decides)
UNFOLDED = [
    case('unfolded_softmax_step', 32, 196, 2048, 393, act='softmax', train=True, keep=0.2, entry='step'),
    case('unfolded_s49_eval', 8, 196, 2048, 393, entry='eval'),
    case('unfolded_n128_sep', 128, 16, 1024, 51, act='relu'),
]


def _lib():
    lib = mp.load_m1_probe()
    lib.apa_probe_m1_set_iflags.argtypes = [ctypes.c_uint]
    lib.apa_probe_m1_set_iflags.restype = None
    lib.apa_probe_m1_fwd_route.argtypes = [ctypes.c_void_p]
    lib.apa_probe_m1_fwd_route.restype = None
    return lib


def _route(lib):
    out = (ctypes.c_int64 * 2)()
    lib.apa_probe_m1_fwd_route(out)
    return int(out[0]), int(out[1])


def _expect_fold(c):
    S = mp.plan(c['N'], c['P'], c['C'], c['C'], c['K'])[0]
    return int(c['act'] != 'softmax' and S <= 16 and c['N'] < 128 and c['C'] % 64 == 0)


def _run(c, inp, dev, lib, iflags):
    r = _Run(c, inp, dev, lib)
    lib.apa_probe_m1_set_iflags(iflags)
    try:
        trace = r.run()
    finally:
        lib.apa_probe_m1_set_iflags(0)
    route = _route(lib)
    torch.cuda.synchronize()
    r.check_guards()
    return r.bits(), route, trace


def _both(c, gpu):
    lib = _lib()
    torch.manual_seed(0)
    inp = _inputs(c, gpu)
    two, route2, trace2 = _run(c, inp, gpu, lib, APA_IFLAG_FINALIZE_LAUNCH)
    one, route1, trace1 = _run(c, inp, gpu, lib, 0)
    assert trace1 == trace2, 'the flag changed more than the finalize step'
    keys = {'sep': ('zsave', 'abar', 'att', 'logits', 'dX', 'dWa', 'dba', 'dWt', 'dbt'),
            'step': ('zsave', 'abar', 'att', 'logits', 'loss', 'G', 'dX', 'dWa', 'dba', 'dWt', 'dbt'),
            'eval': ('zsave', 'abar', 'att', 'logits', 'probs', 'pred')}[c['entry']]
    for k in keys:
        assert torch.equal(one[k], two[k]), '{}: {} differs between the folded and the two-launch forward'.format(
            c['name'], k)
    return route1, route2


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_folded_forward_equals_the_two_launch_sequence(gpu, c):
    route1, route2 = _both(c, gpu)
    fold = _expect_fold(c)
    assert route2 == (0, 3), route2
    assert route1 == (fold, 3 - fold), (route1, fold)


@pytest.mark.parametrize('c', UNFOLDED, ids=[c['name'] for c in UNFOLDED])
def test_routes_outside_the_fold_keep_the_finalize_launch(gpu, c):
    assert _expect_fold(c) == 0
    route1, route2 = _both(c, gpu)
    assert route1 == route2 == (0, 3), (route1, route2)


def test_the_forcing_flag_adds_exactly_the_finalize_launch(gpu):
    """Same call, same thread: the internal flag takes the forward from two launches behind the pooling pass to
    three, and clearing it brings the folded route back."""
    c = case('flag_n3', 3, 49, 1024, 16, entry='eval')
    lib = _lib()
    inp = _inputs(c, gpu)
    seen = [_run(c, inp, gpu, lib, f)[1] for f in (0, APA_IFLAG_FINALIZE_LAUNCH, 0)]
    assert seen == [(1, 2), (0, 3), (1, 2)], seen
    # a caller cannot reach the bit: the entry points mask it
    r = _Run(c, inp, gpu, lib)
    r.flags |= APA_IFLAG_FINALIZE_LAUNCH
    r.run()
    torch.cuda.synchronize()
    assert _route(lib) == (1, 2)
