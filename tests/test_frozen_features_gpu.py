"""The frozen-features mode (APA_FLAG_FROZEN_INPUT / APA_POSE_NO_DX, include/apa.h): the backward half of every route
that has an arm without the dX stores, run twice from the same inputs -- once as always, once with the flag.

What each kernel-level case asserts (the harnesses, inputs, float64 references and bounds are those of
tests/test_m1_paths_gpu.py, tests/test_pose_paths_gpu.py and tests/test_pc_paths_gpu.py, imported as they are):
  * the flagged run is handed a sentinel-filled, guard-padded dX buffer, NOT a null pointer: every sentinel byte must
    be unchanged, so an arm that still stores shows as a failure of this test, not as a fault;
  * every other output of the flagged run equals the unflagged run bit for bit (the same arithmetic in the same order);
  * the unflagged dX and all weight gradients lie within the float64 bound of the route's probe module;
  * only then the route is called once more with dX = NULL, and compared again.
Then the Python surface: cof.attn_pool_bwd(want_dx=False), the bound one-call steps with None in the dX slot (and their
fall-back to the full step where the library refuses the flag), the module path with a non-grad X, and
deploy.FusedHeadStep on frozen features -- with TRAIN.TRAINABLE_SCOPES on a reference-executed fixture
(tests/golden/ref_scopes_*.npz) and at the benchmark shape (refbig_cfg002_* / refbig_cfg003_*).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _ref_fixture as rf
import test_m1_paths_gpu as m1t
import test_pc_paths_gpu as pct
import test_pose_paths_gpu as pt
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests import _pc_probe as pc
from tests import _pose_probe as pp

pytestmark = pytest.mark.gpu

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
FROZEN = cof.APA_FLAG_FROZEN_INPUT


def _untouched(g, what):
    """every byte of the guarded allocation (the matrix and its guards) is what the snapshot holds"""
    assert torch.equal(g.base.view(gp._INT_VIEW[g.dtype]), g.snap), '{}: the flagged call wrote to dX'.format(what)


def _same(full, other, what, skip=('dX',)):
    for k in full:
        if k not in skip:
            assert torch.equal(full[k], other[k]), '{}: {} differs from the unflagged run'.format(what, k)


# ------------------------------------------------------------------------------------------ M == 1: one case per arm
def _m1_cases():
    acts = ('id', 'softmax', 'relu')
    out = []

    def add(name, N, P, C, **kw):
        out.append(m1t.case(name, N, P, C, 7, **kw))

    def four(prefix, N, P, C, dt, family):
        """the FUSED x TRAIN instances of one kernel shape (Ca = 64: a separate attention input), activations in turn"""
        for fused in (True, False):
            for train in (True, False):
                act = acts[len(out) % 3]
                add('{}_{}_{}_{}'.format(prefix, 'fused' if fused else 'ca64', 'train' if train else 'eval', act),
                    N, P, C, dt=dt, act=act, train=train, Ca=None if fused else 64, pool_bwd=family)

    # streaming kernels: fp32 VW 1 / 2 (PIX 1), VW 4 (PIX 2: 2 x 9 pixels in 2 splits of 4 / 5 -- a partial last chunk)
    four('stream_f32_c1024', 3, 15, 1024, F32, 'stream')
    four('stream_f32_c2048', 3, 15, 2048, F32, 'stream')
    four('stream_f32_c4096', 2, 9, 4096, F32, 'stream')
    # relu-on-load instances (fused map only)
    for C, dt, train, act in ((1024, F32, True, 'relu'), (1024, F32, False, 'id'), (2048, F32, True, 'softmax'),
                              (4096, F32, False, 'relu'), (2048, BF16, True, 'id'), (2048, BF16, False, 'softmax')):
        add('relu_input_{}_c{}_{}_{}'.format('bf16' if dt == BF16 else 'f32', C, 'train' if train else 'eval', act),
            3, 15, C, dt=dt, act=act, train=train, relu_in=True, pool_bwd='stream', relu_input=1)
    # streaming bf16 through the separate calls (hashed mask) ...
    four('stream_bf16_c2048', 3, 15, 2048, BF16, 'stream')
    # ... and through the one-call step: the keep-bits form, fused and with a separate attention input
    add('stream_bf16_c2048_step_fused_softmax', 3, 15, 2048, dt=BF16, act='softmax', train=True, entry='step',
        pool_bwd='stream', keep_bits=1)
    add('stream_bf16_c2048_step_ca64_id', 3, 15, 2048, dt=BF16, train=True, entry='step', Ca=64, pool_bwd='stream',
        keep_bits=1)
    # per-pixel vec kernels: VEC 1 / 2 of each type
    four('vec_f32_c256', 3, 15, 256, F32, 'vec')
    four('vec_f32_c512', 3, 15, 512, F32, 'vec')
    four('vec_bf16_c512', 3, 15, 512, BF16, 'vec')
    four('vec_bf16_c1024', 3, 15, 1024, BF16, 'vec')
    # run-time-loop kernels: any C; a replayed (external) mask
    four('generic_f32_c96', 3, 15, 96, F32, 'generic')
    four('generic_bf16_c4096', 2, 9, 4096, BF16, 'generic')
    add('generic_external_mask_f32_c2048_fused', 2, 9, 2048, train=True, rng='external', pool_bwd='generic')
    add('generic_external_mask_f32_c2048_ca64', 2, 9, 2048, train=True, rng='external', Ca=64, act='relu',
        pool_bwd='generic')
    return out


M1_CASES = _m1_cases()


@pytest.mark.parametrize('c', M1_CASES, ids=[c['name'] for c in M1_CASES])
def test_m1_frozen_input(gpu, c):
    lib = mp.load_m1_probe()
    torch.manual_seed(0)
    inp = m1t._inputs(c, gpu)
    r = m1t._Run(c, inp, gpu, lib)
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    bad = {k: (trace[k], v) for k, v in c['expect'].items() if trace[k] != v}
    assert not bad, 'trace mismatch (got, expected): {} in {}'.format(bad, trace)
    got = {k: b.view.clone() for k, b in r.out.items()}
    with torch.no_grad():                                  # the unflagged run against float64 (tests/_m1_probe.py Bnd)
        m1t._check_backward(c, got, m1t._backward_ref(c, inp, got, r.mask))
    full = r.bits()

    # the flag, with a sentinel-filled, guard-padded dX
    r.restore()
    r.flags |= FROZEN
    trace2 = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    _untouched(r.out['dX'], c['name'])
    assert trace2 == trace
    _same(full, r.bits(), c['name'])

    # only now: dX = NULL
    r.restore()
    dx = r.out.pop('dX')
    try:
        trace3 = r.run()
        torch.cuda.synchronize()
        r.check_guards()
        null = r.bits()
    finally:
        r.out['dX'] = dx
    assert trace3 == trace
    _same(full, null, c['name'] + ' (dX = NULL)')


def test_m1_refusals_of_the_flag(gpu):
    """the *_cat entry points and a forward call that asks for the TopDownAttention dump refuse the flag with
    APA_ERR_UNSUPPORTED before anything is queued; without the flag a NULL dX stays APA_ERR_INVALID_ARG"""
    lib = mp.load_m1_probe()
    c = m1t.case('cat_refused', 2, 9, 1024, 7, J=4)
    inp = m1t._inputs(c, gpu)
    r = m1t._Run(c, inp, gpu, lib)
    r.run()
    torch.cuda.synchronize()
    bufs = dict(r.out, workspace=r.ws)
    for b in bufs.values():
        b.snapshot()
    N, P, C, K = r.N, r.P, r.C, r.K
    X = inp['X'].data_ptr()
    head = (X, X, inp['Wa'].data_ptr(), inp['ba'].data_ptr(), r.Wt.ptr, inp['bt'].data_ptr())
    tail = (r.p('att'), r.p('zsave'), r.p('abar'), r.p('G'))
    grads = (r.p('dWa'), r.p('dba'), r.p('dWt'), r.p('dbt'), r.ws.ptr, r.ws_bytes, N, P, C, C, K, 1)
    st = gp.stream_ptr()
    cat = cof.ApaConcatFeat(inp['Xext'].data_ptr(), c['J'], r.p('zext'), r.p('dXext'))
    rc = lib.apa_attn_pool_bwd_cat(ctypes.addressof(cat), None, *head, *tail, r.p('dX'), None, *grads, FROZEN, 1.0, 0,
                                   0, F32, st)
    assert rc == cof.APA_ERR_UNSUPPORTED and b'_cat entry points' in lib.apa_last_error()
    rc = lib.apa_attn_pool_fwd_ex(None, *head, r.p('logits'), r.p('att'), r.p('zsave'), r.p('abar'), r.p('dX'), r.ws.ptr,
                                  r.ws_bytes, N, P, C, C, K, 1, FROZEN, 1.0, 0, 0, F32, st)
    assert rc == cof.APA_ERR_UNSUPPORTED and b'TopDownAttention' in lib.apa_last_error()
    rc = lib.apa_attn_pool_bwd_ex(None, *head, *tail, None, None, *grads, 0, 1.0, 0, 0, F32, st)
    assert rc == -1 and b'null' in lib.apa_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert torch.equal(b.base.view(gp._INT_VIEW[b.dtype]), b.snap), 'a refused call changed {}'.format(k)


# ------------------------------------------------------------------------------------------ pose head, cfg 003 step
class _PoseRun(pt._Run):
    """tests/test_pose_paths_gpu.py's harness with APA_POSE_NO_DX in the backward call's accumulate_dX (the separate
    entry points; the one-call step takes APA_FLAG_FROZEN_INPUT in self.flags)."""
    no_dx = False

    def run(self):
        c, lib, p = self.c, self.lib, self.p
        if c['entry'] == 'step' or not self.no_dx:
            return super().run()
        N, P, C, Cp, J, dt = c['N'], c['P'], c['C'], c['Cp'], c['J'], c['dt']
        st = gp.stream_ptr()
        t1, t2 = pp.PoseTrace(), pp.PoseTrace()
        self._ok(lib.apa_probe_pose_head_fwd(ctypes.addressof(t1), p('X'), p('W1'), p('b1'), p('W2'), p('b2'),
                                             p('Ppre'), p('Pl'), p('ws'), self.ws_bytes, N, P, C, Cp, J, dt, st), 'fwd')
        acc = (1 if c['beta'] else 0) | (cof.APA_POSE_WS_FROM_FWD if c['reuse'] else 0) | cof.APA_POSE_NO_DX
        if c['form'] == 'rank1':
            rc = lib.apa_probe_pose_head_bwd_rank1ext(
                ctypes.addressof(t2), p('X'), p('W1'), p('W2'), p('Ppre'), p('dPl'), p('ext_row'), p('ext_col'),
                p('dX'), acc, p('dW1'), p('db1'), p('dW2'), p('db2'), p('ws'), self.ws_bytes, N, P, C, Cp, J, dt, st)
        else:
            rc = lib.apa_probe_pose_head_bwd(
                ctypes.addressof(t2), p('X'), p('W1'), p('W2'), p('Ppre'), p('dPl'), p('ext'), p('dX'), acc,
                p('dW1'), p('db1'), p('dW2'), p('db2'), p('ws'), self.ws_bytes, N, P, C, Cp, J, dt, st)
        self._ok(rc, 'bwd')
        d = t1.as_dict()
        for k, v in t2.as_dict().items():
            if v not in (0, 'none'):
                d[k] = v
        d['dx_beta'] = t2.dx_beta
        return d

    def freeze(self):
        self.no_dx = True
        if self.c['entry'] == 'step':
            self.flags |= FROZEN

    def bits_but_dx(self):
        outs, self.outs = self.outs, [k for k in self.outs if k != 'dX']
        try:
            return self.bits()
        finally:
            self.outs = outs


# the smallest shape test_pose_paths_gpu.py runs for each rows route, fp32 and bf16 (the MFMA rows kernel is bf16 only);
# an accumulating call (beta = 1: the given dX must stay as it is); the one-call step on its fast route (evaluation-mode
# dropout, and training at the shipped batch, where the pooling share rides in the dX product's epilogue) and on the
# four-call route (fp32)
POSE_NAMES = ['mfma_cp256_plain_r100', 'valu_f32_cp200_j16_r301', 'valu_bf16_cp200_j7_r301',
              'valu_bf16_cp320_j16_ext_r95', 'dppre_f32_cp256_nodpl_ext_r100', 'dppre_bf16_cp768_j32_plain_r150',
              'step_bf16_cp256', 'step_bf16_cp512_w2t_train', 'step_f32_cp768_fallback']
POSE_CASES = [c for c in pt.CASES if c['name'] in POSE_NAMES]


@pytest.mark.parametrize('c', POSE_CASES, ids=[c['name'] for c in POSE_CASES])
def test_pose_head_frozen_input(gpu, c):
    assert len(POSE_CASES) == len(POSE_NAMES)
    lib = pp.load_pose_probe()
    r = _PoseRun(c, gpu, lib)
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace['w1_bwd'] != 'none'                       # the dX product ran
    with torch.no_grad():                                  # the unflagged run against float64 (tests/_pose_probe.py)
        pt._check_case(c, r, trace)
    full = r.bits_but_dx()

    r.restore()
    r.freeze()
    t2 = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    _untouched(r.b['dX'], c['name'])
    # no dX product in the launch list: no W1 operand was chosen for it, nothing was accumulated
    assert t2['w1_bwd'] == 'none' and t2['dx_beta'] == 0, t2
    for k in t2:
        if k not in ('w1_bwd', 'dx_beta'):
            assert t2[k] == trace[k], (k, t2[k], trace[k])
    _same(full, r.bits_but_dx(), c['name'])

    r.restore()
    dx = r.b.pop('dX')
    try:
        t3 = r.run()
        torch.cuda.synchronize()
        r.check_guards()
        null = r.bits_but_dx()
    finally:
        r.b['dX'] = dx
    assert t3 == t2
    _same(full, null, c['name'] + ' (dX = NULL)')


# ------------------------------------------------------------------------------------------ per-class maps, K <= 64
# the smallest fused-route shapes of tests/test_pc_paths_gpu.py: the folded dX kernel (identity / relu; separate calls,
# and the one-call step whose logits + cross-entropy that kernel finishes, with and without dropout) and the
# activation pass + dX product (P < 32, and the spatial softmax)
PC_NAMES = ['f_k2_c256_p32_id_eval_sep', 'f_k3_c768_p33_relu_train_step', 'f_k4_c256_p36_relu_step_notrain',
            'f_k51_c2048_p25_id_train_sep', 'f_k2_c256_p25_softmax_step_notrain']
PC_CASES = [c for c in pct.CASES if c['name'] in PC_NAMES]
PC_DX_FIELDS = ('dx', 'upb', 'dx_splits', 'rbs', 'mid_bits', 'dx_drop_c', 'g_dx')


def _pc_bits(r):
    return {k: r.b[k].bits() for k in r.outs if k != 'dX'}


@pytest.mark.parametrize('c', PC_CASES, ids=[c['name'] for c in PC_CASES])
def test_per_class_fused_route_frozen_input(gpu, c):
    assert len(PC_CASES) == len(PC_NAMES)
    lib = pc.load_pc_probe()
    r = pct._Run(c, gpu, lib)
    trace = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    assert trace['path_bwd'] == 'fused' and trace['dx'] != 'none'
    with torch.no_grad():                                  # the unflagged run against float64 (tests/_pc_probe.py)
        pct._check_case(c, r, trace)
    full = _pc_bits(r)

    r.restore()
    r.flags |= FROZEN
    t2 = r.run()
    torch.cuda.synchronize()
    r.check_guards()
    _untouched(r.b['dX'], c['name'])
    assert t2['dx'] == 'none', t2                          # no dX product
    for k in t2:
        if k not in PC_DX_FIELDS and not k.startswith('g_dx_'):       # (g_dx_*: the dX product's GemmTrace)
            assert t2[k] == trace[k], (k, t2[k], trace[k])
    _same(full, _pc_bits(r), c['name'])

    r.restore()
    dx = r.b.pop('dX')
    try:
        t3 = r.run()
        torch.cuda.synchronize()
        r.check_guards()
        null = _pc_bits(r)
    finally:
        r.b['dX'] = dx
    assert t3['dx'] == 'none'
    _same(full, null, c['name'] + ' (dX = NULL)')


def test_dense_per_class_route_refuses_the_flag_and_the_wrappers_fall_back(gpu):
    """K = 65: the dense per-class route.  The library refuses the flag before anything is queued -- the one-call step
    before its forward half --; cof.attn_pool_bwd(want_dx=False) and a bound step with None in the dX slot then run the
    full call on a scratch dX: the same results, bit for bit."""
    lib = pc.load_pc_probe()
    c = next(c for c in pct.CASES if c['name'] == 'g_nb_k65')
    r = pct._Run(c, gpu, lib)
    r.fwd()
    torch.cuda.synchronize()
    for g in r.b.values():
        g.snapshot()
    seed, off, flags = r.key()
    p = r.p
    rc = lib.apa_attn_pool_bwd_ex(None, *r.head(), p('att'), p('Tsave'), None, p('G'), p('dX'), p('dXatt'), p('dWa'),
                                  p('dba'), p('dWt'), p('dbt'), p('ws'), r.ws_bytes, *r.dims(), flags | FROZEN,
                                  c['keep'], seed, off, c['dt'], gp.stream_ptr())
    assert rc == cof.APA_ERR_UNSUPPORTED and b'dense per-class route' in lib.apa_last_error()
    loss = gp.Guarded(1, c['N'] + 1, c['N'] + 1, torch.float32, gpu)
    loss.snapshot()
    rc = lib.apa_attn_head_train_step_ex(None, *r.head(), r.labels.data_ptr(), 1.0, 1.0, p('logits'), p('att'),
                                         p('Tsave'), None, loss.ptr, p('G'), p('dX'), p('dXatt'), p('dWa'), p('dba'),
                                         p('dWt'), p('dbt'), p('ws'), r.ws_bytes, *r.dims(), flags | FROZEN, c['keep'],
                                         seed, off, c['dt'], gp.stream_ptr())
    assert rc == cof.APA_ERR_UNSUPPORTED and b'dense per-class route' in lib.apa_last_error()
    torch.cuda.synchronize()
    for k, g in list(r.b.items()) + [('loss', loss)]:
        assert torch.equal(g.base.view(gp._INT_VIEW[g.dtype]), g.snap), 'a refused call changed {}'.format(k)

    # the wrappers
    X = r.b['X'].view.contiguous()
    Wa, ba, Wt, bt = (r.b[k].view.contiguous() for k in ('Wa', 'ba', 'Wt', 'bt'))
    ba, bt = ba.view(-1), bt.view(-1)
    N, P, K = c['N'], c['P'], c['K']
    X3 = X.view(N, P, -1)
    kw = dict(flags=r.flags, keep_prob=c['keep'], seed=7, offset=3)
    logits, att, zsave, abar, _, ws = cof.attn_pool_fwd(X3, X3, Wa, ba, Wt, bt, **kw)
    G = r.b['G'].view.contiguous()
    want = cof.attn_pool_bwd(X3, X3, Wa, ba, Wt, bt, att, zsave, abar, G, workspace=ws, **kw)
    got = cof.attn_pool_bwd(X3, X3, Wa, ba, Wt, bt, att, zsave, abar, G, workspace=ws, want_dx=False, **kw)
    assert got[0] is None and want[0] is not None
    for a, b in zip(want[2:], got[2:]):
        assert torch.equal(a, b)
    labels = r.labels

    def grads(dx):
        return (dx, None, torch.empty_like(Wa), torch.empty_like(ba), torch.empty_like(Wt), torch.empty_like(bt))
    g_full, g_frozen = grads(torch.empty_like(X3)), grads(None)
    s_full = cof.HeadTrainStep(X3, X3, Wa, ba, Wt, bt, labels, g_full, **kw)
    s_frozen = cof.HeadTrainStep(X3, X3, Wa, ba, Wt, bt, labels, g_frozen, **kw)
    assert s_frozen.frozen_input and s_frozen.dX_scratch is None
    s_full.run()
    s_frozen.run()
    torch.cuda.synchronize()
    assert not s_frozen.frozen_input and s_frozen.dX_scratch is not None       # the stated fall-back: the full step
    assert torch.equal(s_frozen.dX_scratch, g_full[0])
    for a, b in zip(g_full[2:], g_frozen[2:]):
        assert torch.equal(a, b)
    assert torch.equal(s_full.loss, s_frozen.loss) and torch.equal(s_full.logits, s_frozen.logits)


# ------------------------------------------------------------------------------------------ the Python op layer
def _head_inputs(gpu, N, P, C, K, dtype, seed=3):
    g = torch.Generator(device=gpu).manual_seed(seed)
    u = lambda *s: torch.rand(s, generator=g, device=gpu) * 1.25 - 0.25
    X = torch.relu(u(N, P, C)).to(dtype)
    return X, u(C, 1) * (4.0 / C), u(1) * 0.1, u(C, K) / C ** 0.5, u(K) * 0.1, \
        torch.randint(0, K, (N,), generator=g, device=gpu)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_bound_steps_take_none_in_the_dx_slot(gpu, dtype):
    """cof.HeadTrainStep / cof.PoseAttnTrainStep with grads[0] = None set the flag, allocate nothing for dX and leave
    every other output bit-identical to the step that writes dX."""
    N, P, C, K, Cp, J = 4, 49, 2048, 51, 256, 16
    X, Wa, ba, Wt, bt, labels = _head_inputs(gpu, N, P, C, K, dtype)
    kw = dict(flags=cof.attn_flags(False, True, True), keep_prob=0.5, seed=11, offset=2)

    def grads(dx):
        return (dx, None, torch.empty_like(Wa), torch.empty_like(ba), torch.empty_like(Wt), torch.empty_like(bt))
    gf, gz = grads(torch.empty_like(X)), grads(None)
    sf = cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, labels, gf, **kw)
    sz = cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, labels, gz, **kw)
    sf.run()
    sz.run()
    torch.cuda.synchronize()
    assert sz.frozen_input and sz.dX_scratch is None
    for a, b in zip(gf[2:], gz[2:]):
        assert torch.equal(a, b)
    for k in ('logits', 'att', 'zsave', 'abar', 'loss', 'G'):
        assert torch.equal(getattr(sf, k), getattr(sz, k)), k

    g = torch.Generator(device=gpu).manual_seed(5)
    u = lambda *s: torch.rand(s, generator=g, device=gpu) * 1.25 - 0.25
    params = (u(C, Cp) / C, u(Cp) * 0.01, u(Cp, J) / Cp, u(J) * 0.1, u(Cp, 1) / Cp, u(1) * 0.1, Wt, bt)
    pose_labels, pose_valid = u(N, P, J), (u(N, J) > 0).to(torch.uint8)

    def pgrads(dx):
        return (dx,) + tuple(torch.empty_like(t) for t in params)
    pf, pz = pgrads(torch.empty_like(X)), pgrads(None)
    kw = dict(flags=cof.attn_flags(False, False, True), keep_prob=0.5, seed=11, offset=2)
    af = cof.PoseAttnTrainStep(X, params, labels, pose_labels, pose_valid, pf, **kw)
    az = cof.PoseAttnTrainStep(X, params, labels, pose_labels, pose_valid, pz, **kw)
    af.run()
    az.run()
    torch.cuda.synchronize()
    assert az.frozen_input and az.dX_scratch is None
    for a, b in zip(pf[1:], pz[1:]):
        assert torch.equal(a, b)
    for k in ('Ppre', 'Pl', 'att', 'logits', 'zsave', 'abar', 'loss_action', 'loss_pose', 'G', 'dPl', 'dZ'):
        assert torch.equal(getattr(af, k), getattr(az, k)), k


def test_module_path_with_a_non_grad_input(gpu):
    """AttentionalPoolingFunction / PoseHeadFunction with an X that needs no gradient: the same parameter gradients bit
    for bit, and X.grad is None; an X that requires grad behaves as before."""
    from attentionalpoolingaction_amd import nets_factory as nf
    N, P, C, K = 3, 25, 2048, 21
    X, Wa, ba, Wt, bt, labels = _head_inputs(gpu, N, P, C, K, torch.float32)
    X = X.view(N, 5, 5, C)

    def run(x):
        ps = [t.clone().requires_grad_(True) for t in (Wa, ba, Wt, bt)]
        logits = nf.attentional_pooling(x, None, *ps, relu_att=True, is_training=True, keep_prob=0.5, seed=4, offset=9)[0]
        torch.nn.functional.cross_entropy(logits, labels).backward()
        return [p.grad for p in ps]
    xg = X.clone().requires_grad_(True)
    with_dx, without = run(xg), run(X)
    assert xg.grad is not None and X.grad is None
    for a, b in zip(with_dx, without):
        assert torch.equal(a, b)

    Cp, J = 256, 16
    g = torch.Generator(device=gpu).manual_seed(6)
    u = lambda *s: torch.rand(s, generator=g, device=gpu) * 1.25 - 0.25
    W1, b1, W2, b2 = u(C, Cp) / C, u(Cp) * 0.01, u(Cp, J) / Cp, u(J) * 0.1

    def run_pose(x):
        ps = [t.clone().requires_grad_(True) for t in (W1, b1, W2, b2)]
        Ppre, Pl = nf.PoseHeadFunction.apply(x, *ps)
        (Pl.sum() + Ppre.float().sum() * 0.01).backward()
        return [p.grad for p in ps]
    xg = X.clone().requires_grad_(True)
    with_dx, without = run_pose(xg), run_pose(X)
    assert xg.grad is not None and X.grad is None
    for a, b in zip(with_dx, without):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ deploy.FusedHeadStep
def _rel(got, exp, floor=1e-30):
    return float(np.abs(np.asarray(got, dtype=np.float64) - exp).max() / max(np.abs(exp).max(), floor))


def _train_batch(tf_, b, gpu, fused):
    """batch `b` of a training fixture as clone_fn folds it (src/train.py:395-398): frames into the batch axis"""
    a = tf_.arrays
    img = torch.from_numpy(a['batch/%d/images' % b]).to(gpu)
    img = img.reshape(-1, *img.shape[2:])
    la = torch.from_numpy(a['batch/%d/labels_action' % b]).to(gpu)
    lp = pv = None
    if fused.pose_form:
        lp = torch.from_numpy(a['batch/%d/labels_pose' % b]).to(gpu)
        lp = lp.reshape(-1, *lp.shape[2:])
        pv = torch.from_numpy(a['batch/%d/labels_pose_valid' % b]).to(gpu)
        pv = pv.reshape(-1, pv.shape[-1])
    return img, la, lp, pv


def _batch(fx, gpu, fused, dtype=torch.float32):
    img = torch.from_numpy(fx.arrays['in/images']).to(gpu)
    if img.dim() == 5:
        img = img.reshape(-1, *img.shape[2:])
    la = torch.from_numpy(fx.arrays['in/labels_action']).to(gpu)
    lp = pv = None
    if fused.pose_form:
        lp = torch.from_numpy(fx.arrays['in/labels_pose']).to(gpu).reshape(img.shape[0], img.shape[1], img.shape[2], -1)
        pv = torch.from_numpy(fx.arrays['in/labels_pose_valid']).to(gpu).reshape(img.shape[0], -1)
    return img.to(dtype), la, lp, pv


def _frozen_equals_full(fused, batch):
    """one step with a conv5 map that needs no gradient, one (same dropout step) with one that does: losses, end
    points and bucket bit for bit; the frozen bound step holds no [N,P,C] gradient buffer"""
    img, la, lp, pv = batch
    head = fused.head
    step0 = head._step
    total_f, ep_f = fused(img, la, lp, pv)
    total_f.backward()
    st = fused._step_obj                                    # no [N,P,C] gradient buffer: none bound, none allocated
    grads = st._keep[7 if isinstance(st, cof.HeadTrainStep) else 5]
    assert st._dX_buf is None and st.frozen_input and st.dX_scratch is None and grads[0] is None
    frozen = dict(total=total_f.detach().clone(), bucket=fused.bucket.flat.clone(),
                  ep={k: (v.clone() if isinstance(v, torch.Tensor) else [l.clone() for l in v]) for k, v in ep_f.items()})
    head._step = step0
    fused.bucket.zero_()
    ig = img.clone().requires_grad_(True)
    total_g, ep_g = fused(ig, la, lp, pv)
    total_g.backward()
    assert fused._step_obj._dX_buf is not None and ig.grad is not None and len(fused._steps) == 2
    assert torch.equal(total_g.detach(), frozen['total']) and torch.equal(fused.bucket.flat, frozen['bucket'])
    for k, v in ep_g.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, frozen['ep'][k]), k
        else:
            assert all(torch.equal(a, b) for a, b in zip(v, frozen['ep'][k])), k


SCOPE_FUSED = ['cfg002_1clone_iter2_att', 'cfg003_2clones_prefix']


@pytest.mark.parametrize('name', SCOPE_FUSED)
def test_fused_head_step_honours_the_scopes_on_frozen_features(gpu, name):
    """TRAIN.TRAINABLE_SCOPES through deploy.FusedHeadStep on a reference-executed fixture (dropout off): the conv5
    maps need no gradient, the first parameter update reproduces the reference's step/0/var/* for the trained
    variables (fp32 against float64: the 2e-5 of tests/test_train_reference_gpu.py) and leaves the frozen ones bit-equal."""
    from attentionalpoolingaction_amd import config as apa_config, deploy
    from test_train_reference_cpu import product_cfg
    tf_ = rf.TrainFixture(os.path.join(rf.GOLD, 'ref_scopes_%s.npz' % name))
    m = tf_.meta
    assert float(m['net']['DROPOUT']) == 0.0
    nc = m['num_clones']
    try:
        params0 = tf_.initial_variables()
        cfg = product_cfg(tf_)
        from attentionalpoolingaction_amd import nets_factory
        network_fn = nets_factory.get_network_fn(m['model'], m['num_classes'], m['num_pose_keypoints'], cfg,
                                                 weight_decay=m['weight_decay'], is_training=True, device=gpu,
                                                 in_channels=tf_.arrays['batch/0/images'].shape[-1])
        table = rf.module_tf_names(network_fn)
        with torch.no_grad():
            for vn, t in table.items():
                t.copy_(torch.from_numpy(params0[vn]).reshape(t.shape).to(gpu))
        trained = deploy.apply_trainable_scopes(network_fn, cfg)
        dc = deploy.DeploymentConfig(nc, 0)
        fused = deploy.FusedHeadStep(network_fn, cfg, loss_scale=dc.clone_loss_scale)
        assert [fused.tf_names[n] for n in fused.bucket.names] == [vn for vn in m['var_order'] if vn in trained]
        assert fused.frozen_features                           # the scopes declare frozen training
        opt = fused.make_optimizer(cfg.TRAIN.LEARNING_RATE, deploy_config=dc)
        accum = deploy.GradientAccumulator(fused.bucket, cfg.TRAIN.ITER_SIZE)
        run_sum = torch.zeros_like(fused.bucket.flat)
        step = m['steps'][0]
        lr = deploy.configure_learning_rate(cfg, m['num_samples'], nc, 0)
        first = True
        for r in step['runs']:
            run = m['runs'][r]
            run_sum.zero_()
            for b in run['batches']:
                batch = _train_batch(tf_, b, gpu, fused)
                if first:
                    _frozen_equals_full(fused, batch)
                    first = False
                    fused.bucket.zero_()
                total, _ = fused(*batch)
                total.backward()
                assert fused._step_obj._dX_buf is None
                run_sum.add_(fused.bucket.flat)
            fused.bucket.flat.copy_(run_sum)
            if accum.step():
                opt.step(lr=lr)
        for vn, t in table.items():
            got = t.detach().cpu().double().numpy()
            if vn in trained and vn in m['grad_vars']:
                exp = tf_.arrays['step/0/var/' + vn]
                assert _rel(got.reshape(exp.shape), exp) < 2e-5, vn
            elif vn not in trained:
                assert np.array_equal(got.reshape(params0[vn].shape), params0[vn]), vn     # never written, never decayed
        moved = _rel(tf_.arrays['var0/' + ATT_TD].astype(np.float64), tf_.arrays['step/0/var/' + ATT_TD])
        assert moved > 1e-3                                    # the update is far above the tolerance
    finally:
        apa_config.reset_cfg()


ATT_TD = 'PosePrelogitsBasedAttention/Conv/weights'
BIG_FROZEN = ['refbig_cfg002_train_baseline_libmask', 'refbig_cfg003_train_baseline_libmask']


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', BIG_FROZEN)
def test_fused_head_step_on_frozen_features_at_the_benchmark_shape(gpu, name, dtype):
    from attentionalpoolingaction_amd import config as apa_config, deploy
    fx = rf.HeadFixture(os.path.join(rf.GOLD, name + '.npz'))
    network_fn, cfg = rf.build_head(fx, device=gpu)
    try:
        table = rf.module_tf_names(network_fn)
        with torch.no_grad():
            for vn, t in table.items():
                t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).to(gpu))
        head = network_fn.head
        head.seed, head._step = int(fx.meta['libmask'][0]), int(fx.meta['libmask'][1])
        assert not deploy.FusedHeadStep(network_fn, cfg).frozen_features      # no scopes: dX is filled as ever
        fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
        fused.make_optimizer(0.01)
        batch = _batch(fx, gpu, fused, torch.bfloat16 if dtype == 'bf16' else torch.float32)
        _frozen_equals_full(fused, batch)
    finally:
        apa_config.reset_cfg()
