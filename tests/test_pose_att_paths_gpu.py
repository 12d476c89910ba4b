"""Every kernel path of the pose-heatmap attention head (csrc/apa_pose_att.hip) against float64, stage by stage.

Each case of tests/_pal_stage.py CASES calls apa_pose_att_logits_fwd / _bwd through ctypes on NaN-guarded allocations
(tests/_gemm_probe.py Guarded) and compares every stage -- F, every slab of the partial logits, logits, dF, dW, db, dX,
every slab of the dA partials, dPl -- element by element under the bound derived in tests/_pal_stage.py, with float64
computed from THE TENSORS THAT STAGE'S KERNEL READ (its predecessors' stored outputs).  The kernel instance is a pure
function of (M, dtype, accumulate_dX), which the case fixes, and the intermediate stages are read out of the
workspace, whose layout `layout` transcribes from pal_plan (the total is asserted against
apa_pose_att_logits_workspace_bytes); no probe library is involved.

Conditions: no case, stage or element is skipped or masked.  Every output and the whole workspace holds NaN before the
call; after it every element a call owns is finite (`check`), and every other element of every allocation -- inputs,
the other call's outputs, guard rows, tails, alignment gaps and the part of the workspace the call does not own -- is
unchanged bit for bit.  The backward call runs on the workspace the forward call used.  Every case runs twice and
repeats bit for bit.  dPl and, under accumulate_dX, dX are given non-zero values.  The dropout mask is
cof.dropout_mask (exact, not bounded).

Further: the replayed mask (APA_FLAG_RNG_EXTERNAL) and the _ex entry points with all four hook events give the same
bits; operands at the weakest alignment the header allows give the same bits; everything the header refuses is
refused before anything is launched.

tests/test_pose_att_paths_cpu.py shows without a GPU that this checker admits an fp32 emulation of every stage for the
same inputs and rejects seeded value errors.  Measured figures: profiles/r10_pose_att_paths.md.
"""
import ctypes
import os

import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _pal_stage as ps

pytestmark = pytest.mark.gpu

F32, BF16 = ps.F32, ps.BF16
APA_ERR_INVALID_ARG = -1          # include/apa.h
FP32_OPERANDS = ('Pl', 'W', 'b', 'F', 'G', 'dPl', 'dW', 'db', 'logits')   # addressed with scalar accesses
FWD_WRITES, BWD_WRITES = ('F', 'logits', 'ws'), ('dX', 'dPl', 'dW', 'db', 'ws')

FIGS = []
_REF = {}


def _operands(c):
    """host operands of a case: drawn once, shared by the tests that need them, never written to."""
    if c['name'] not in _REF:
        _REF[c['name']] = ps.make_inputs(c)
    return _REF[c['name']]


def _ibits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class _Run:
    """One case on the device.  mis: {buffer: element offset inside its allocation}."""

    def __init__(self, c, dev, mis=()):
        self.c, self.dev, self.lib = c, dev, cof.load_library()
        N, P, C, J, K, M = c['N'], c['P'], c['C'], c['J'], c['K'], c['M']
        self.lay = lay = ps.layout(N, P, C, M, K)
        self.ws_bytes = int(self.lib.apa_pose_att_logits_workspace_bytes(N, P, C, M, K))
        assert self.ws_bytes == lay['total'], (self.ws_bytes, lay)
        R, tdt, mis = lay['R'], ps.TDT[c['dt']], dict(mis)
        self.I = I = {k: v.to(dev) for k, v in _operands(c).items()}
        self.b = {}

        def buf(name, rows, cols, dtype, data=None):
            self.b[name] = gp.Guarded(rows, cols, cols, dtype, dev, off=mis.get(name, 0), data=data)
            assert self.b[name].base.data_ptr() % 256 == 0

        buf('X', N * P, C, tdt, I['X'].view(N * P, C))
        buf('Pl', N * P, J, torch.float32, I['Pl'].view(N * P, J))
        buf('W', R, K, torch.float32, I['W'])
        buf('b', 1, K, torch.float32, I['b'])
        buf('G', N, K, torch.float32, I['G'])
        buf('F', N, R, torch.float32)
        buf('logits', N, K, torch.float32)
        buf('dX', N * P, C, tdt, I['dX0'].view(N * P, C) if c['acc'] else None)
        buf('dPl', N * P, J, torch.float32, I['dPl0'].view(N * P, J))
        buf('dW', R, K, torch.float32)
        buf('db', 1, K, torch.float32)
        buf('ws', 1, self.ws_bytes // 4, torch.float32)
        self.sel = (ctypes.c_int32 * max(len(c['sel']), 1))(*c['sel'])
        self.mask = cof.dropout_mask((N, R), c['keep'], ps.SEED, ps.OFFSET, device=dev) if c['train'] else None
        self.packed = None
        for g in self.b.values():
            g.snapshot()

    # ---- what a call may write: the valid region of its outputs, and its own stages of the workspace
    def _owned(self, name, call):
        g = self.b[name]
        if name != 'ws':
            return g.valid
        own = torch.zeros_like(g.valid)
        lay = self.lay
        spans = [('part_off', 'part_n')] if call == 'fwd' else [('dF_off', 'dF_n'), ('dA_off', 'dA_n')]
        for o, n in spans:
            own[g.off + lay[o] // 4:g.off + lay[o] // 4 + lay[n]] = True
        return own

    def _settle(self, call, before, writes):
        """after a call: nothing outside what the call owns has changed, in any allocation."""
        torch.cuda.synchronize()
        for name, g in self.b.items():
            now = _ibits(g.base)
            changed = now != before[name]
            if name in writes:
                changed &= ~self._owned(name, call)
            n = int(changed.sum())
            assert n == 0, '{}: {} changed {} elements of {} it does not own (first at flat {})'.format(
                self.c['name'], call, n, name, int(changed.nonzero()[0]))

    def _state(self):
        return {name: _ibits(g.base).clone() for name, g in self.b.items()}

    def _ok(self, rc, what):
        assert rc == 0, '{}: {} returned {} ({})'.format(self.c['name'], what, rc, self.lib.apa_last_error().decode())

    def ws_stage(self, which):
        lay, c = self.lay, self.c
        flat = self.b['ws'].view.view(-1)
        o, n = lay[which + '_off'] // 4, lay[which + '_n']
        shape = {'part': (lay['nslab_cls'], c['N'], c['K']), 'dF': (c['N'], lay['R']),
                 'dA': (lay['nslab_pool'], c['N'], c['P'], c['M'])}[which]
        return flat[o:o + n].view(shape).clone()

    def run(self, external=False, hooks=None):
        """forward, then backward on the same workspace.  -> the stored stages (clones)."""
        c, lib, p = self.c, self.lib, lambda k: self.b[k].ptr
        N, P, C, J, K = c['N'], c['P'], c['C'], c['J'], c['K']
        for g in self.b.values():
            g.restore()
        flags = cof.APA_FLAG_TRAIN if c['train'] else 0
        seed, offset = ps.SEED, ps.OFFSET
        if external:
            if self.packed is None:
                self.packed = cof.pack_keep_mask(self.mask, device=self.dev)
            flags, seed, offset = flags | cof.APA_FLAG_RNG_EXTERNAL, self.packed.bits.data_ptr(), 0
        tail = (self.ws_bytes, N, P, C, J, K, flags, float(c['keep']), seed, offset, c['dt'], gp.stream_ptr())
        head = (p('X'), p('Pl'), self.sel, len(c['sel']), 1 if c['avged'] else 0, p('W'))
        torch.cuda.synchronize()
        before = self._state()
        fa = head + (p('b'), p('F'), p('logits'), p('ws')) + tail
        rc = lib.apa_pose_att_logits_fwd(*fa) if hooks is None else \
            lib.apa_pose_att_logits_fwd_ex(ctypes.addressof(hooks[0]), *fa)
        self._ok(rc, 'fwd')
        self._settle('fwd', before, FWD_WRITES)
        obs = dict(F=self.b['F'].view.clone(), part=self.ws_stage('part'), logits=self.b['logits'].view.clone())
        before = self._state()
        ba = head + (p('F'), p('G'), p('dX'), 1 if c['acc'] else 0, p('dPl'), p('dW'), p('db'), p('ws')) + tail
        rc = lib.apa_pose_att_logits_bwd(*ba) if hooks is None else \
            lib.apa_pose_att_logits_bwd_ex(ctypes.addressof(hooks[1]), *ba)
        self._ok(rc, 'bwd')
        self._settle('bwd', before, BWD_WRITES)
        obs.update(dF=self.ws_stage('dF'), dA=self.ws_stage('dA'), dW=self.b['dW'].view.clone(),
                   db=self.b['db'].view.clone().view(-1), dX=self.b['dX'].view.clone().view(N, P, C),
                   dPl=self.b['dPl'].view.clone().view(N, P, J))
        return obs


def _same_bits(c, a, b, what):
    for k in a:
        assert torch.equal(_ibits(a[k].contiguous()), _ibits(b[k].contiguous())), \
            '{}: {} differs {}'.format(c['name'], k, what)


def _verify(c, r, obs):
    def rec(stage, ratio, bound):
        FIGS.append((c['name'], stage, ratio, bound))
        print('PAL_FIG {} {} err/bound {:.4f} bound/ref {:.3e}'.format(c['name'], stage, ratio, bound))
    with torch.no_grad():
        ps.verify(c, r.I, r.mask, obs, rec=rec)


@pytest.mark.parametrize('c', ps.CASES, ids=[c['name'] for c in ps.CASES])
def test_pose_att_path(gpu, c):
    r = _Run(c, gpu)
    first = r.run()
    _verify(c, r, first)
    _same_bits(c, first, r.run(), 'between two identical calls')


@pytest.mark.parametrize('name', ['m5_c260_p65', 'm18_bf16_keep02_acc'])
def test_replayed_mask_gives_the_hashed_bits(gpu, name):
    """APA_FLAG_RNG_EXTERNAL with the packed bits of cof.dropout_mask: every output and workspace stage bit-identical
    to the hashed run."""
    c = ps.BY_NAME[name]
    r = _Run(c, gpu)
    _same_bits(c, r.run(), r.run(external=True), 'between the hashed and the replayed mask')


def test_hooks_leave_the_results_alone(gpu):
    """the _ex entry points with all four hook events: the same bits, and both event pairs of both calls complete."""
    c = ps.BY_NAME['m17_parts_n33']
    r = _Run(c, gpu)
    plain = r.run()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
    for e in evs:
        e.record()
    hf = cof.make_hooks(prof_fwd=(evs[0], evs[1]), prof_bwd=(evs[2], evs[3]))
    hb = cof.make_hooks(prof_fwd=(evs[4], evs[5]), prof_bwd=(evs[6], evs[7]))
    hooked = r.run(hooks=(hf, hb))
    torch.cuda.synchronize()
    _same_bits(c, plain, hooked, 'between the plain and the _ex entry points')
    for i in range(0, 8, 2):
        assert evs[i].elapsed_time(evs[i + 1]) >= 0.0


@pytest.mark.parametrize('name,mis', [
    # X and dX 8-byte but not 16-byte aligned: all bf16 features ask for
    ('m9_bf16_k129', {'X': 4, 'dX': 4}),
    # every fp32 operand other than X / dX 4-byte aligned only
    ('m5_c260_p65', {k: 1 for k in FP32_OPERANDS}),
], ids=['bf16_x_dx_8byte', 'f32_operands_4byte'])
def test_placement(gpu, name, mis):
    """operands at the weakest alignment include/apa.h allows are served, with the bits of the aligned run."""
    c = ps.BY_NAME[name]
    moved = _Run(c, gpu, mis=mis)
    esz = {'X': 2, 'dX': 2}
    for k, off in mis.items():
        assert moved.b[k].ptr % 16 == (off * esz.get(k, 4)) % 16 != 0
    _same_bits(c, _Run(c, gpu).run(), moved.run(), 'between the aligned and the offset placement')


def test_refusals_launch_nothing(gpu):
    """everything include/apa.h refuses: the status, and no element of any allocation changed."""
    lib = cof.load_library()
    # buffers large enough for every variant below, should one be served by mistake
    N, P, C, J, K = 2, 4, 8, 16, 16
    Cb, Mb, Kb = 12, 33, 481
    dev, f32 = gpu, torch.float32
    b = {}
    for name, n in (('X', N * P * Cb), ('dX', N * P * Cb), ('Pl', N * P * J), ('dPl', N * P * J), ('W', Mb * Cb * Kb),
                    ('dW', Mb * Cb * Kb), ('b', Kb), ('db', Kb), ('G', N * Kb), ('logits', N * Kb), ('F', N * Mb * Cb)):
        b[name] = gp.Guarded(1, n, n, f32, dev, off=4)
    ws_bytes = int(lib.apa_pose_att_logits_workspace_bytes(N, P, Cb, Mb, Kb))
    b['ws'] = gp.Guarded(1, ws_bytes // 4, ws_bytes // 4, f32, dev, off=4)
    for g in b.values():
        assert g.ptr % 16 == 0
    bits = cof.pack_keep_mask(torch.ones(N * Mb * Cb, dtype=torch.uint8), device=dev)
    torch.cuda.synchronize()
    before = {k: _ibits(g.base).clone() for k, g in b.items()}
    p = {k: g.ptr for k, g in b.items()}
    st = gp.stream_ptr()

    def call(which, *, sel=(0, 1), C=C, K=K, flags=0, keep=1.0, seed=0, dt=F32, ws_bytes=ws_bytes, **ptr):
        q = dict(p, **ptr)
        arr = (ctypes.c_int32 * max(len(sel), 1))(*sel)
        head = (q['X'], q['Pl'], arr, len(sel), 1, q['W'])
        tail = (ws_bytes, N, P, C, J, K, flags, keep, seed, 0, dt, st)
        if which == 'fwd':
            return lib.apa_pose_att_logits_fwd(*(head + (q['b'], q['F'], q['logits'], q['ws']) + tail))
        return lib.apa_pose_att_logits_bwd(*(head + (q['F'], q['G'], q['dX'], 0, q['dPl'], q['dW'], q['db'], q['ws'])
                                             + tail))

    U, WS, IA = gp.APA_ERR_UNSUPPORTED, gp.APA_ERR_WORKSPACE, APA_ERR_INVALID_ARG
    for which in ('fwd', 'bwd'):
        assert call(which, X=p['X'] + 8) == U                                 # fp32 X 8-byte aligned
        assert call(which, X=p['X'] + 4, dX=p['dX'] + 4, dt=BF16) == U        # bf16 X 4-byte aligned
        assert call(which, C=6) == U
        assert call(which, sel=tuple(range(16)) + tuple(range(15))) == U      # M = 33
        assert call(which, K=481) == U
        assert call(which, flags=cof.APA_FLAG_TRAIN | cof.APA_FLAG_RNG_DEVICE, keep=0.5, seed=1) == U
        assert call(which, flags=cof.APA_FLAG_RELU_INPUT) == U
        assert call(which, ws_bytes=int(lib.apa_pose_att_logits_workspace_bytes(N, P, C, 4, K)) - 1) == WS
        assert call(which, sel=(0, J)) == IA
        assert call(which, sel=(-1, 0)) == IA
        # the workspace is read as float4 (dF): 16 bytes in both calls, with or without a mask image
        for off in (4, 8):
            assert call(which, ws=p['ws'] + off) == U
        assert call(which, ws=p['ws'] + 4, flags=cof.APA_FLAG_TRAIN | cof.APA_FLAG_RNG_EXTERNAL, keep=0.5,
                    seed=bits.bits.data_ptr()) == U
    # dX is stored with X's vector width: refused in the backward call; the forward call has no dX
    assert call('bwd', dX=p['dX'] + 8) == U and call('bwd', dX=p['dX'] + 4) == U
    assert call('bwd', dX=p['dX'] + 4, dt=BF16) == U and call('bwd', dX=p['dX'] + 2, dt=BF16) == U
    assert b'dX' in lib.apa_last_error()
    torch.cuda.synchronize()
    for k, g in b.items():
        assert torch.equal(_ibits(g.base), before[k]), 'a refused call wrote to {}'.format(k)


def teardown_module(module):
    """With APA_PAL_FIGURES=<path>: the per-stage figures of this run as a table (profiles/r10_pose_att_paths.md)."""
    path = os.environ.get('APA_PAL_FIGURES')
    if path and FIGS:
        with open(path, 'w') as f:
            f.write('| case | stage | max err / bound | bound / max ref |\n|---|---|---|---|\n')
            for name, stage, a, b in FIGS:
                f.write('| {} | {} | {:.3f} | {:.2e} |\n'.format(name, stage, a, b))
    _REF.clear()
