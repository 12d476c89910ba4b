"""The geometries of the four small kernels of the M == 1 chain (csrc/apa_m1_small.hip, csrc/apa_device.h), each held
bit for bit to the route it replaces or to a float32 restatement of its documented summation order.

* Fold: m1_logits2_fold_kernel has two geometries, 8 images x KG k-tiles (half MFMA tiles) and 16 images x 7 k-tiles
  (full tiles); launch_logits2_fold picks one by shape.  Every case runs three times through the probe library: with
  APA_IFLAG_FINALIZE_LAUNCH (the finalize kernel + m1_logits2_kernel pair), as the product runs it, and with
  APA_IFLAG_FOLD_TILE16 (full tiles whatever the shape).  All outputs must be byte-equal.
* Cross-entropy reducer: m1_logits_xent_kernel addresses its partial copies as one base plus 32-bit byte offsets; the
  one-call steps are compared with the separate calls at 1, 32, 33 and 34 copies (the last two take the copy loop's
  second trip) and at K on both sides of the NV4 instances' limits.
* Column sum: m1_colsum (32 columns x 32 row groups per block; 16- and 8-column blocks were measured and lost)
  against a numpy float32 walk of the order apa_device.h documents, so that any later block shape is held to it:
  thread (rg, c) adds rows rg, rg + 32, ... one by one, the 32 row groups are added in order; dba = the 1024-slot
  order (slot t adds pdba[t], pdba[t + 1024], ...; wave_sum per 64 slots; 16 waves in order).
  tests/test_gemm_paths_gpu.py holds the tail blocks of the split-K reduce to the same launch bit for bit.

Shapes: the smallest that reach each edge -- N = 1, 15, 16, 17, 33 (ragged and second image groups of both
geometries), S = 4 and 12, one k-tile, a ragged tile, exactly one group of 7 k-tiles and one tile more, the cfg 002
class count; nblk through every batch depth of the column sum (16, 8, 1 rows in flight) and C = 40, a ragged last
block.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests.test_m1_paths_gpu import F32, _inputs, _Run, _separate_equivalent, case

pytestmark = pytest.mark.gpu

APA_IFLAG_FINALIZE_LAUNCH = 1 << 27      # csrc/apa_internal.h
APA_IFLAG_FOLD_TILE16 = 1 << 28


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
    return r, r.bits(), route, trace


# ------------------------------------------------------------------------------------------ fold
FOLD_N = (1, 15, 16, 17, 33)
FOLD_K = (4, 16, 17, 112, 113, 393)
FOLD_C = (64, 2048)
FOLD_P = (16, 49)            # S = 4 and 12
FOLD_ACT = ('id', 'relu')


def _fold_cases():
    """Every (N, K, C) twice: the training step and the evaluation step, with the pixel count and the attention
    activation alternating so that each of their values meets every N, K and C."""
    out = []
    for iN, N in enumerate(FOLD_N):
        for iK, K in enumerate(FOLD_K):
            for iC, C in enumerate(FOLD_C):
                a, b = (iN + iK + iC) % 2, (iN + iK // 2 + iC) % 2
                for entry, P, act in (('step', FOLD_P[a], FOLD_ACT[b]), ('eval', FOLD_P[1 - a], FOLD_ACT[1 - b])):
                    out.append(case('fold_n{}_p{}_c{}_k{}_{}_{}'.format(N, P, C, K, act, entry), N, P, C, K, act=act,
                                    train=entry == 'step', keep=0.2, entry=entry))
    return out


FOLD_CASES = _fold_cases()
FOLD_KEYS = {'step': ('zsave', 'abar', 'att', 'logits', 'loss', 'G', 'dX', 'dWa', 'dba', 'dWt', 'dbt'),
             'eval': ('zsave', 'abar', 'att', 'logits', 'probs', 'pred')}


@pytest.mark.parametrize('c', FOLD_CASES, ids=[c['name'] for c in FOLD_CASES])
def test_fold_geometries_equal_the_two_launch_sequence(gpu, c):
    lib = _lib()
    torch.manual_seed(0)
    inp = _inputs(c, gpu)
    S = mp.plan(c['N'], c['P'], c['C'], c['C'], c['K'])[0]
    assert S == {16: 4, 49: 12}[c['P']]
    _, two, route2, trace2 = _run(c, inp, gpu, lib, APA_IFLAG_FINALIZE_LAUNCH)
    _, one, route1, trace1 = _run(c, inp, gpu, lib, 0)
    _, full, route16, trace16 = _run(c, inp, gpu, lib, APA_IFLAG_FOLD_TILE16)
    assert trace1 == trace2 == trace16, 'a flag changed more than the forward sequence'
    assert route2 == (0, 3) and route1 == route16 == (1, 2), (route2, route1, route16)
    for k in FOLD_KEYS[c['entry']]:
        assert torch.equal(one[k], two[k]), '{}: {} differs between the folded and the two-launch forward'.format(
            c['name'], k)
        assert torch.equal(full[k], two[k]), '{}: {} differs between full tiles and the two-launch forward'.format(
            c['name'], k)


# ------------------------------------------------------------------------------------------ cross-entropy reducer
XENT_CASES = [case('xent_n{}_c{}_k{}_{}'.format(N, C, K, entry), N, 16, C, K, train=entry == 'step', keep=0.2,
                   entry=entry)
              for K in (4, 255, 256, 257, 393, 512) for C in (64, 2048, 2112, 2176) for N in (1, 3)
              for entry in ('step', 'eval')]
# C = 2112 (33 copies) reaches the reducer through the evaluation step only: the training step's small-K route wants
# C % 128 == 0 (m1_small_supported), so C = 2176 (34 copies) is its second trip of the copy loop.


@pytest.mark.parametrize('c', XENT_CASES, ids=[c['name'] for c in XENT_CASES])
def test_xent_reducer_step_equals_the_separate_calls(gpu, c):
    lib = _lib()
    torch.manual_seed(0)
    inp = _inputs(c, gpu)
    r, first, route, trace = _run(c, inp, gpu, lib, 0)
    # the reducer under test serves every evaluation step here and the training steps the head kernels accept
    # (C >= 512: m1_bwd_head_supported; C % 128 == 0: m1_small_supported)
    if c['entry'] == 'eval' or (c['C'] >= 512 and c['C'] % 128 == 0):
        assert trace['logits'] == ('xent_probs' if c['entry'] == 'eval' else 'xent'), trace
        assert trace['logits_nv4'] == (1 if c['K'] <= 128 else (2 if c['K'] <= 256 else 4)), trace
    assert route == (1, 2), route          # folded: C / 64 = 1, 32, 33, 34 partial copies
    sep = _separate_equivalent(c, r, lib)
    torch.cuda.synchronize()
    keys = (('logits', 'G', 'loss', 'abar', 'zsave', 'att', 'dWa', 'dba', 'dWt', 'dbt', 'dX') if c['entry'] == 'step'
            else ('logits', 'probs', 'pred', 'abar', 'zsave', 'att'))
    for k in keys:     # loss: [0] the batch mean, [1:] per example
        assert torch.equal(first[k], sep[k]), '{}: {} of the one-call step differs from the separate calls'.format(
            c['name'], k)


# ------------------------------------------------------------------------------------------ column sum
def _row_sum16(v):
    """apa_device.h row_sum16 on [..., 16] float32: lane ^ 1, lane ^ 2, half mirror, mirror."""
    i = np.arange(16)
    for perm in (i ^ 1, i ^ 2, (i & 8) | (7 - (i & 7)), 15 - i):
        v = (v + v[..., perm]).astype(np.float32)
    return v


def _colsum_walk(part, nblk, C):
    """[C] float32: thread (rg, c) adds rows rg, rg + 32, ... in order from 0.f, then the groups 0 .. 31 in order."""
    acc = np.zeros((32, C), np.float32)
    for b0 in range(0, nblk, 32):
        rows = part[b0:b0 + 32, :C]
        acc[:rows.shape[0]] = (acc[:rows.shape[0]] + rows).astype(np.float32)
    s = np.zeros(C, np.float32)
    for g in range(32):
        s = (s + acc[g]).astype(np.float32)
    return s


def _dba_walk(pdba, nblk):
    a = np.zeros(1024, np.float32)
    for b0 in range(0, nblk, 1024):
        seg = pdba[b0:b0 + 1024]
        a[:seg.shape[0]] = (a[:seg.shape[0]] + seg).astype(np.float32)
    rows = _row_sum16(a.reshape(16, 4, 16))[..., 0]                     # [wave][row]: lanes 0, 16, 32, 48
    w = ((rows[:, 0] + rows[:, 1]).astype(np.float32) + (rows[:, 2] + rows[:, 3]).astype(np.float32)).astype(np.float32)
    s = np.float32(0)
    for x in w:
        s = np.float32(s + x)
    return s


COLSUM_CASES = [(nblk, C) for nblk in (1, 31, 33, 255, 257, 512, 513) for C in (8, 40, 2048)]


@pytest.mark.parametrize('nblk,C', COLSUM_CASES, ids=['nblk{}_c{}'.format(*x) for x in COLSUM_CASES])
def test_colsum_keeps_the_documented_order(gpu, nblk, C):
    lib = gp.load_probe()
    lib.apa_probe_m1_colsum_dba.argtypes = [ctypes.POINTER(gp.ProbeColsum), ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p]
    gen = torch.Generator(device=gpu).manual_seed(1000 * nblk + C)
    ld = C + 3
    part = gp.rand_operand((nblk, ld), gen, gpu)
    pdba = gp.rand_operand((nblk,), gen, gpu)
    C1 = C // 2 if C > 8 else C                        # two sections where there is room: dwa | dwa2
    outs = [gp.Guarded(1, C1, C1, torch.float32, gpu), gp.Guarded(1, max(C - C1, 1), max(C - C1, 1), torch.float32, gpu),
            gp.Guarded(1, 1, 1, torch.float32, gpu)]
    for g in outs:
        g.snapshot()
    bump = torch.full((2,), 41, dtype=torch.int64, device=gpu)
    j = gp.ProbeColsum(part.data_ptr(), outs[0].ptr, nblk, C, ld, outs[1].ptr if C1 < C else None, C1, None, 0, None, 0,
                       None, 0, None, 0, 0.0, None, bump.data_ptr())
    rc = lib.apa_probe_m1_colsum_dba(ctypes.byref(j), pdba.data_ptr(), outs[2].ptr, gp.stream_ptr())
    assert rc == gp.APA_OK, lib.apa_probe_last_error()
    torch.cuda.synchronize()
    for g, what in zip(outs, ('dwa', 'dwa2', 'dba')):
        g.check_guards(what)
    want = _colsum_walk(part.cpu().numpy(), nblk, C)
    got = np.concatenate([outs[0].view[0].cpu().numpy()] + ([outs[1].view[0].cpu().numpy()] if C1 < C else []))
    assert got.view(np.int32).tolist() == want.view(np.int32).tolist(), 'column sums leave the documented order'
    dba = outs[2].view[0, 0].cpu().numpy()
    assert dba.view(np.int32) == _dba_walk(pdba.cpu().numpy(), nblk).view(np.int32), 'dba leaves the 1024-slot order'
    assert bump.tolist() == [42, 41], bump.tolist()    # the dropout counter: advanced once, by block 0 alone
