"""Rank > 1 on one bottom-up map in one streaming pass (csrc/apa_m1_rank.hip; include/apa.h: apa_rank_maps) on the GPU.

Every case of tests/_rank_reference.CASES (its reach table -- every instance, product and split of the two kernels --
is asserted by tests/test_rank_maps_cpu.py) runs the forward and the backward entry point twice -- the two runs must
repeat bit for bit -- with every output and the workspace inside NaN-guarded allocations, and is compared with the
float64 formulas in the error model of tests/_m1_probe.py: the forward outputs from the inputs, the logits and the
backward from the kernel's own forward outputs.  Then: the one-call step against the three separate calls (bits) and
float64 (loss, G); the two reference-executed rank fixtures replayed with the reference's dropout mask through the op,
the module (fuse_ranks=True) and deploy.FusedHeadStep; the routed module against the per-op module path."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _gemm_probe as gp
from tests import _m1_probe as mp
from tests import _rank_reference as rr
from tests._m1_probe import Bnd

pytestmark = pytest.mark.gpu

F32, BF16 = cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16
SEED, OFFSET = 1234, 7


def _plan(c):
    S, ppb, nblk, _ = mp.plan(c['N'], c['P'], c['C'], c['Ca'] or c['C'], c['K'])
    return S, ppb, nblk


class _Run:
    """The NaN-guarded buffers of one case and the three entry points on them."""

    def __init__(self, c, inp, dev, lib):
        self.c, self.inp, self.lib = c, inp, lib
        N, P, C, K, R = c['N'], c['P'], c['C'], c['K'], c['R']
        Ca = c['Ca'] or C
        tdt = inp['X'].dtype
        f32 = torch.float32
        Gd = gp.Guarded
        o = {'logits': Gd(N, K, K, f32, dev), 'att': Gd(N * P, R, R, f32, dev), 'zsave': Gd(N * R, C, C, f32, dev),
             'abar': Gd(N, R, R, f32, dev), 'z0': Gd(N, P, P, f32, dev), 'G': Gd(N, K, K, f32, dev),
             'loss': Gd(1, N + 1, N + 1, f32, dev), 'dX': Gd(N * P, C, C, tdt, dev), 'dWa': Gd(1, Ca, Ca, f32, dev),
             'dba': Gd(1, 1, 1, f32, dev)}
        for r in range(R):
            o['dWt%d' % r] = Gd(C, K, K, f32, dev)
            o['dbt%d' % r] = Gd(1, K, K, f32, dev)
        for r in range(R - 1):
            o['dcw%d' % r] = Gd(1, 1, 1, f32, dev)
            o['dcb%d' % r] = Gd(1, 1, 1, f32, dev)
        if c['Ca'] is not None:
            o['dXatt'] = Gd(N * P, Ca, Ca, tdt, dev)
        self.out = o
        self.ws_bytes = int(lib.apa_attn_pool_rank_workspace_bytes(N, P, C, Ca, K, R - 1))
        assert self.ws_bytes > 0
        self.ws = Gd(1, (self.ws_bytes + 3) // 4, (self.ws_bytes + 3) // 4, f32, dev)
        self.flags = (cof.APA_FLAG_RELU_ATT if c['act'] == 'relu' else 0) | (cof.APA_FLAG_TRAIN if c['train'] else 0)
        self.mask = cof.dropout_mask((N * P * C,), rr.KEEP, SEED, OFFSET) if c['train'] else None
        rk = cof.ApaRankMaps()
        rk.extra = R - 1
        for r in range(R - 1):
            rk.chain_w[r], rk.chain_b[r] = inp['cw'][r].data_ptr(), inp['cb'][r].data_ptr()
            rk.Wt[r], rk.bt[r] = inp['Wts'][r + 1].data_ptr(), inp['bts'][r + 1].data_ptr()
            rk.dchain_w[r], rk.dchain_b[r] = o['dcw%d' % r].ptr, o['dcb%d' % r].ptr
            rk.dWt[r], rk.dbt[r] = o['dWt%d' % (r + 1)].ptr, o['dbt%d' % (r + 1)].ptr
        rk.z0 = o['z0'].ptr
        self.rk = rk
        self.dims = (N, P, C, Ca, K, 1)
        for b in list(o.values()) + [self.ws]:
            b.snapshot()

    def restore(self):
        for b in list(self.out.values()) + [self.ws]:
            b.restore()

    def _head(self):
        inp = self.inp
        X = inp['X'].data_ptr()
        Xatt = X if self.c['Ca'] is None else inp['Xatt'].data_ptr()
        return (ctypes.addressof(self.rk), X, Xatt, inp['Wa'].data_ptr(), inp['ba'].data_ptr(),
                inp['Wts'][0].data_ptr(), inp['bts'][0].data_ptr())

    def _tail(self):
        dt = BF16 if self.c['bf16'] else F32
        return (self.ws.ptr, self.ws_bytes, *self.dims, self.flags, rr.KEEP, SEED, OFFSET, dt, gp.stream_ptr())

    def p(self, k):
        return self.out[k].ptr if k in self.out else None

    def fwd(self):
        rc = self.lib.apa_attn_pool_rank_fwd(*self._head(), self.p('logits'), self.p('att'), self.p('zsave'),
                                             self.p('abar'), *self._tail())
        assert rc == 0, self.lib.apa_last_error()

    def bwd(self):
        rc = self.lib.apa_attn_pool_rank_bwd(*self._head(), self.p('att'), self.p('zsave'), self.p('abar'), self.p('G'),
                                             self.p('dX'), self.p('dXatt'), self.p('dWa'), self.p('dba'),
                                             self.p('dWt0'), self.p('dbt0'), *self._tail())
        assert rc == 0, self.lib.apa_last_error()

    def xent(self):
        rc = self.lib.apa_softmax_xent_fwd_bwd(self.p('logits'), self.inp['labels'].data_ptr(), self.p('loss'),
                                               self.p('G'), None, None, self.c['N'], self.c['K'], 1.0, 1.0,
                                               gp.stream_ptr())
        assert rc == 0, self.lib.apa_last_error()

    def step(self):
        rc = self.lib.apa_attn_head_train_step_rank(
            *self._head(), self.inp['labels'].data_ptr(), 1.0, 1.0, self.p('logits'), self.p('att'), self.p('zsave'),
            self.p('abar'), self.p('loss'), self.p('G'), self.p('dX'), self.p('dXatt'), self.p('dWa'), self.p('dba'),
            self.p('dWt0'), self.p('dbt0'), *self._tail())
        assert rc == 0, self.lib.apa_last_error()

    def check_guards(self):
        for k, b in self.out.items():
            b.check_guards(k)
        self.ws.check_guards('workspace')

    def bits(self, skip=()):
        return {k: b.bits() for k, b in self.out.items() if k not in skip}

    def got(self):
        return {k: b.view.clone() for k, b in self.out.items()}


def _same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), '{}: {} differs'.format(what, k)


def _ratio(got, b, bf16=False):
    """largest |got - ref| / tolerance over the elements with a tolerance above zero"""
    err = (got.double().reshape(b.ref.shape) - b.ref).abs()
    tol = mp.tolerance(b, bf16)
    ok = tol > 0
    return float((err[ok] / tol[ok]).max()) if bool(ok.any()) else 0.0


def _print_ratios(c, got, fref, lg, bref):
    """the figures of profiles/fp8_rank_instances_summary.md, printed before anything is asserted"""
    bf, R = c['bf16'], c['R']
    out = {k: _ratio(got[k], fref[k]) for k in ('z0', 'att', 'zsave', 'abar')}
    out['logits'] = _ratio(got['logits'], lg)
    out['dX'] = _ratio(got['dX'], bref['dX'], bf)
    if c['Ca'] is not None:
        out['dXatt'] = _ratio(got['dXatt'], bref['dXatt'], bf)
    out['dWa'], out['dba'] = _ratio(got['dWa'], bref['dWa']), _ratio(got['dba'], bref['dba'])
    out['dWt'] = max(_ratio(got['dWt%d' % r], bref['dWts'][r]) for r in range(R))
    out['dbt'] = max(_ratio(got['dbt%d' % r], bref['dbts'][r]) for r in range(R))
    out['dcw'] = max(_ratio(got['dcw%d' % r], bref['dcw'][r]) for r in range(R - 1))
    out['dcb'] = max(_ratio(got['dcb%d' % r], bref['dcb'][r]) for r in range(R - 1))
    print('RANKRATIO {} {}'.format(c['name'], ' '.join('{}={:.4f}'.format(k, v) for k, v in out.items())))


def _check_backward(c, got, ref):
    bf = c['bf16']
    R = c['R']
    mp.check(got['dX'], ref['dX'], 'dX', bf16=bf)
    if c['Ca'] is not None:
        mp.check(got['dXatt'], ref['dXatt'], 'dXatt', bf16=bf)
    rr.check_cancelling(got['dWa'].double(), ref['dWa'], ref['dWa_mag'], 'dWa')
    rr.check_cancelling(got['dba'].double(), ref['dba'], ref['dba_mag'], 'dba')
    closed = 2 if c['b2'] is not None else None
    for r in range(R):
        mp.check(got['dWt%d' % r], ref['dWts'][r], 'dWt rank %d' % r, zero_ref=r == closed)
        mp.check(got['dbt%d' % r], ref['dbts'][r], 'dbt rank %d' % r, zero_ref=r == closed)
    for r in range(R - 1):
        rr.check_cancelling(got['dcw%d' % r].double(), ref['dcw'][r], ref['dcw_mag'][r], 'dw of rank %d' % (r + 1))
        rr.check_cancelling(got['dcb%d' % r].double(), ref['dcb'][r], ref['dcb_mag'][r], 'db of rank %d' % (r + 1))


@pytest.mark.parametrize('c', rr.CASES, ids=[c['name'] for c in rr.CASES])
def test_rank_case(gpu, c):
    lib = cof.load_library()
    inp = rr.to_device(rr.inputs(c), gpu)
    r = _Run(c, inp, gpu, lib)
    r.out['G'].view.copy_(inp['G'])
    r.out['G'].snapshot()
    skip = ('loss',)
    r.fwd()
    r.bwd()
    torch.cuda.synchronize()
    r.check_guards()
    first, got = r.bits(skip), r.got()
    r.restore()
    r.fwd()
    r.bwd()
    torch.cuda.synchronize()
    r.check_guards()
    _same_bits(first, r.bits(skip), 'second run')

    with torch.no_grad():
        fref, amb, opened = rr.forward_bnd(c, inp, r.mask)
        if amb is not None:
            rr.check_gate_condition(c, amb, opened)
        _print_ratios(c, got, fref, rr.logits_bnd(c, inp, rr.parts_of(c, inp, got)),
                      rr.backward_bnd(c, inp, rr.parts_of(c, inp, got), got['G'], r.mask, _plan(c)))
        mp.check(got['z0'], fref['z0'], 'z0')
        mp.check(got['att'], fref['att'], 'att', ambiguous=amb)
        closed = c['b2'] is not None
        if closed:      # rank 2 is shut everywhere: exactly zero, and the other ranks carry the 1 % rule
            N, P, C, R = c['N'], c['P'], c['C'], c['R']
            assert float(got['att'].reshape(N, P, R)[..., 2].abs().max()) == 0.0
            assert float(got['zsave'].reshape(N, R, C)[:, 2].abs().max()) == 0.0
            assert float(got['abar'].reshape(N, R)[:, 2].abs().max()) == 0.0
        mp.check(got['zsave'], fref['zsave'], 'zsave')
        mp.check(got['abar'], fref['abar'], 'abar')
        parts = rr.parts_of(c, inp, got)
        mp.check(got['logits'], rr.logits_bnd(c, inp, parts), 'logits')
        bref = rr.backward_bnd(c, inp, parts, got['G'], r.mask, _plan(c))
        _check_backward(c, got, bref)
        if closed:      # ... and so are its gradients: exactly zero and finite
            for k in ('dWt2', 'dbt2', 'dcw1', 'dcb1'):
                assert torch.isfinite(got[k]).all() and float(got[k].abs().max()) == 0.0, k


@pytest.mark.parametrize('name', rr.STEP_CASES)
def test_one_call_step_equals_the_separate_calls(gpu, name):
    """apa_attn_head_train_step_rank == apa_attn_pool_rank_fwd, apa_softmax_xent_fwd_bwd, apa_attn_pool_rank_bwd in
    turn, every output bit for bit; loss and G against float64 from the kernel's own logits."""
    c = rr.case_by_name(name)
    lib = cof.load_library()
    inp = rr.to_device(rr.inputs(c), gpu)
    one = _Run(c, inp, gpu, lib)
    one.step()
    torch.cuda.synchronize()
    one.check_guards()
    sep = _Run(c, inp, gpu, lib)
    sep.fwd()
    sep.xent()
    sep.bwd()
    torch.cuda.synchronize()
    sep.check_guards()
    _same_bits(one.bits(), sep.bits(), 'one call against three')
    got = one.got()
    N, K = c['N'], c['K']
    lg = got['logits'].double().reshape(N, K)
    p = torch.softmax(lg, dim=1)
    tol = mp.C_ACC * (K + 16) * mp.EPS32
    lab = inp['labels']
    onehot = torch.nn.functional.one_hot(lab, K).double()
    mp.check(got['G'], Bnd((p - onehot) / N, tol * (p + onehot) / N), 'G')
    lse = torch.logsumexp(lg, dim=1)
    per = lse - lg.gather(1, lab[:, None])[:, 0]
    mag = lse.abs() + lg.abs().amax(dim=1)
    loss = got['loss'].double().reshape(N + 1)
    mp.check(loss[1:], Bnd(per, tol * mag), 'loss per example')
    mp.check(loss[:1], Bnd(per.mean().reshape(1), (tol * mag).mean().reshape(1) + tol * per.abs().mean()), 'loss')
    # the backward half really ran on that G: its own float64 check, from the step's forward outputs
    with torch.no_grad():
        parts = rr.parts_of(c, inp, got)
        ref = rr.backward_bnd(c, inp, parts, got['G'], one.mask, _plan(c))
        mp.check(got['dX'], ref['dX'], 'dX', bf16=c['bf16'])
        for r in range(c['R']):
            mp.check(got['dWt%d' % r], ref['dWts'][r], 'dWt rank %d' % r, zero_ref=True)   # rows of G sum to zero


# ------------------------------------------------------------------------------------------ reference fixtures
def _rel(got, exp, floor=1e-30):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(exp).shape)
    exp = np.asarray(exp, dtype=np.float64)
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), floor))


def _check_fixture(fx, q, logits, att, loss, grads):
    """logits 1e-3 abs (2e-5 rel), loss 2e-5 rel, end points and gradients 5e-5 -- the tolerances
    tests/test_reference_fixtures_gpu.py applies to the module path for the same fixtures.  grads: {tf name or
    'images': gradient of the LOSS (no regulariser)}; the fixture's include weight_decay * w on the conv weights."""
    exp_logits = fx.expected('out/logits')
    got_logits = logits.detach().float().cpu().numpy()
    assert np.abs(got_logits - exp_logits).max() <= 1e-3 and _rel(got_logits, exp_logits) < 2e-5
    assert np.array_equal(got_logits.argmax(1), exp_logits.argmax(1))
    exp_att = fx.expected('out/ep/PosePrelogitsBasedAttention')
    assert tuple(att.shape) == exp_att.shape
    assert _rel(att.detach().float().cpu().numpy(), exp_att, 1e-6) < 5e-5
    exp_loss = float(fx.expected('out/losses')[0])
    assert abs(float(loss.detach()) - exp_loss) <= 2e-5 * max(abs(exp_loss), 1e-3)
    wd = fx.meta['weight_decay']
    for vn, g in grads.items():
        g = g.detach().double().cpu().numpy()
        if vn == 'images':
            assert _rel(g, fx.expected('grad/images')) < 5e-5, vn
            continue
        if vn.endswith('/weights'):
            g = g.reshape(fx.variables[vn].shape) + wd * fx.variables[vn]
        assert _rel(g, fx.expected('grad/var/' + vn)) < 5e-5, vn
    assert len(grads) == 1 + 4 * q['R']


def _xent(logits, labels):
    return torch.nn.functional.cross_entropy(logits.double(), labels)


@pytest.mark.parametrize('name', ['rank2_train', 'rank3_relu_train'])
def test_rank_fixture_through_the_op(gpu, name):
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_%s.npz' % name))
    q = rr.fixture_problem(fx)
    R = q['R']
    dev = lambda t: t.to(gpu).float().contiguous()
    X, Wa, ba = dev(q['X']), dev(q['Wa'])[:, None].contiguous(), dev(q['ba'])
    Wts, bts = [dev(w) for w in q['Wts']], [dev(b) for b in q['bts']]
    cw = [torch.tensor([[w]], device=gpu) for w in q['cw']]
    cb = [torch.tensor([b], device=gpu) for b in q['cb']]
    keep = cof.pack_keep_mask(q['mask'], device=gpu)
    flags = cof.attn_flags(False, q['relu'], True)
    kw = dict(flags=flags, keep_prob=q['keep'], seed=keep)
    logits, att, zsave, abar, z0, ws = cof.attn_pool_rank_fwd(X, X, Wa, ba, Wts, bts, cw, cb, **kw)
    labels = q['labels'].to(gpu)
    loss, G = cof.softmax_xent_fwd_bwd(logits, labels)[:2]
    dX, _, dWa, dba, dWts, dbts, dcw, dcb = cof.attn_pool_rank_bwd(X, X, Wa, ba, Wts, bts, cw, cb, att, zsave, abar,
                                                                    z0, G, workspace=ws, **kw)
    grads = {'images': dX.view(fx.arrays['in/images'].shape), q['att_names'][0] + '/weights': dWa,
             q['att_names'][0] + '/biases': dba}
    for r in range(R):
        grads[q['td_names'][r] + '/weights'], grads[q['td_names'][r] + '/biases'] = dWts[r], dbts[r]
    for r in range(R - 1):
        grads[q['att_names'][r + 1] + '/weights'], grads[q['att_names'][r + 1] + '/biases'] = dcw[r], dcb[r]
    n, h, w = fx.arrays['in/images'].shape[:3]
    _check_fixture(fx, q, logits, att.view(n, h, w, 1, R), loss.reshape(-1)[0], grads)


def _load_fixture_head(fx, gpu, **kw):
    network_fn, cfg = rf.build_head(fx, device=gpu, **kw)
    table = rf.module_tf_names(network_fn)
    with torch.no_grad():
        for vn, t in table.items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).to(gpu))
    return network_fn, cfg, table


@pytest.mark.parametrize('name', ['rank2_train', 'rank3_relu_train'])
def test_rank_fixture_through_the_module(gpu, name):
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_%s.npz' % name))
    q = rr.fixture_problem(fx)
    try:
        network_fn, cfg, table = _load_fixture_head(fx, gpu, fuse_ranks=True)
        head = network_fn.head
        assert head.ranks_fused()
        images = torch.from_numpy(fx.arrays['in/images']).to(gpu).requires_grad_(True)
        head.replay_dropout_mask(torch.from_numpy(fx.dropout_mask()).to(gpu))
        logits, ep = network_fn(images)
        loss = _xent(logits, q['labels'].to(gpu))
        loss.backward()
        grads = {'images': images.grad}
        for vn in q['att_names'] + q['td_names']:
            for s in ('/weights', '/biases'):
                grads[vn + s] = table[vn + s].grad
        _check_fixture(fx, q, logits, ep['PosePrelogitsBasedAttention'], loss, grads)
        assert set(ep.keys()) >= {'Logits', 'PosePrelogitsBasedAttention', 'PoseLogits'}
    finally:
        apa_config.reset_cfg()


def test_pose_prelogits_rank_fixture_through_the_module(gpu):
    """ref_head_rank2_posepre_train: rank 2 with the attention computed from pose_pre_logits and the pose loss on.
    With fuse_ranks=True the existing attention GEMV supplies Z_0 and consumes dZ~_0, the pose head's autograd node
    takes dXatt: logits, end points, the losses and every gradient against the reference-executed fixture, at the
    tolerances tests/test_reference_fixtures_gpu.py applies to the per-op module path."""
    from attentionalpoolingaction_amd import loss as apa_loss
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_rank2_posepre_train.npz'))
    try:
        network_fn, cfg, table = _load_fixture_head(fx, gpu, fuse_ranks=True)
        head = network_fn.head
        assert head.ranks_fused() and not head.single_layer
        images = torch.from_numpy(fx.arrays['in/images']).to(gpu).requires_grad_(True)
        head.replay_dropout_mask(torch.from_numpy(fx.dropout_mask()).to(gpu))
        logits, ep = network_fn(images)
        tc = fx.meta['train_cfg']
        use_pose = bool(tc['LOSS_FN_POSE'])
        losses = apa_loss.gen_losses(
            torch.from_numpy(fx.arrays['in/labels_action']).to(gpu), logits, tc['LOSS_FN_ACTION'],
            fx.meta['num_classes'], tc['LOSS_FN_ACTION_WT'],
            torch.from_numpy(fx.arrays['in/labels_pose']).to(gpu) if use_pose else None,
            ep.get('PoseLogits') if use_pose else None, tc['LOSS_FN_POSE'] if use_pose else '',
            torch.from_numpy(fx.arrays['in/labels_pose_valid']).to(gpu) if use_pose else None, tc['LOSS_FN_POSE_WT'],
            ep, cfg)
        total = sum(losses) + apa_loss.l2_regularization(network_fn.regularized_weights(), network_fn.weight_decay)
        total.backward()
        exp_logits = fx.expected('out/logits')
        got_logits = logits.detach().cpu().numpy()
        assert np.abs(got_logits - exp_logits).max() <= 1e-3 and _rel(got_logits, exp_logits) < 2e-5
        exp_att = fx.expected('out/ep/PosePrelogitsBasedAttention')
        assert tuple(ep['PosePrelogitsBasedAttention'].shape) == exp_att.shape
        assert _rel(ep['PosePrelogitsBasedAttention'].detach().cpu().numpy(), exp_att, 1e-6) < 5e-5
        assert _rel(ep['PoseLogits'].detach().float().cpu().numpy(), fx.expected('out/ep/PoseLogits'), 1e-6) < 5e-5
        exp_losses = fx.expected('out/losses')
        assert len(losses) == len(exp_losses)
        for got, exp in zip(losses, exp_losses):
            assert abs(float(got.detach()) - exp) <= 2e-5 * max(abs(exp), 1e-3)
        assert abs(float(total.detach()) - float(fx.expected('out/total'))) <= 2e-5 * float(fx.expected('out/total'))
        assert _rel(images.grad.cpu().numpy(), fx.expected('grad/images')) < 5e-5
        for vn in fx.meta['trainable']:
            assert table[vn].grad is not None, vn
            assert _rel(table[vn].grad.cpu().numpy(), fx.expected('grad/var/' + vn)) < 5e-5, vn
    finally:
        apa_config.reset_cfg()


@pytest.mark.parametrize('name', ['rank2_train', 'rank3_relu_train'])
def test_rank_fixture_through_fused_head_step(gpu, name):
    from attentionalpoolingaction_amd import deploy
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_%s.npz' % name))
    q = rr.fixture_problem(fx)
    try:
        network_fn, cfg, table = _load_fixture_head(fx, gpu)
        head = network_fn.head
        head.seed = cof.pack_keep_mask(torch.from_numpy(fx.dropout_mask()), device=gpu)   # the reference's mask
        fused = deploy.FusedHeadStep(network_fn, cfg)
        images = torch.from_numpy(fx.arrays['in/images']).to(gpu).requires_grad_(True)
        total, ep = fused(images, q['labels'].to(gpu))
        total.backward()
        names = head.tf_variable_names()
        grads = {'images': images.grad}
        for n in fused._written:
            grads[names[n]] = fused.bucket.views[n]
        assert len(ep['Losses']) == 1
        _check_fixture(fx, q, ep['Logits'], ep['PosePrelogitsBasedAttention'], total, grads)
        # frozen features: the same bucket, conv5's gradient goes to scratch
        before = fused.bucket.flat.clone()
        frozen = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
        head._step = 0
        total2, _ = frozen(images.detach(), q['labels'].to(gpu))
        assert frozen._dX is None and torch.equal(frozen.bucket.flat, before) and float(total2) == float(total)
    finally:
        apa_config.reset_cfg()


# ------------------------------------------------------------------------------------------ routed vs per-op module
def test_fused_ranks_match_the_per_op_module_path(gpu):
    """get_network_fn(..., fuse_ranks=True) against the module as it stands (one pass of the rank-1 op per rank) on a
    random rank-3 relu case, the library's own dropout stream in both: the end points have identical shapes, and
    logits, attention maps and every gradient agree within the sum of the two error bounds.  Either path is an fp32
    evaluation of the same formulas with contractions no longer than the model's, so each lies within the model's
    bound (from the inputs alone) of the float64 value -- asserted for both -- and the sum of the two bounds is twice
    it.  The seed leaves no relu gate within its bound of zero, so both paths take the same gates."""
    c = rr.case('parity_rank3_relu', 3, 20, 96, 20, 3, 'relu', True)
    inp = rr.to_device(rr.inputs(c), gpu)
    H, W = 4, 5
    nets = []
    try:
        for fuse in (False, True):
            network_fn, cfg = rr.network('rank3_relu_train', {'DROPOUT': 1.0 - rr.KEEP}, fuse_ranks=fuse,
                                       in_channels=c['C'])
            head = network_fn.head.to(gpu)
            assert head.num_classes == c['K'] and head.keep_prob == rr.KEEP and head.ranks_fused() == fuse
            with torch.no_grad():
                head.att_weights.copy_(inp['Wa'][:, None])
                head.att_biases.copy_(inp['ba'])
                for r, (wt, bt) in enumerate(zip([head.td_weights] + list(head.td_weights_r),
                                                 [head.td_biases] + list(head.td_biases_r))):
                    wt.copy_(inp['Wts'][r])
                    bt.copy_(inp['bts'][r])
                for r in range(2):
                    head.att_weights_r[r].copy_(inp['cw'][r].reshape(1, 1))
                    head.att_biases_r[r].copy_(inp['cb'][r])
            head.seed, head._step = SEED, OFFSET
            nets.append((network_fn, head))
        K = c['K']
        G = (torch.rand((c['N'], K), device=gpu) * 1.25 - 0.25) / c['N']
        res = []
        for network_fn, head in nets:
            X = inp['X'].view(c['N'], H, W, c['C']).clone().requires_grad_(True)
            logits, ep = network_fn(X)
            (logits * G).sum().backward()
            res.append(dict(logits=logits.detach(), att=ep['PosePrelogitsBasedAttention'].detach(), dX=X.grad,
                            dWa=head.att_weights.grad, dba=head.att_biases.grad,
                            dWts=[head.td_weights.grad] + [p.grad for p in head.td_weights_r],
                            dbts=[head.td_biases.grad] + [p.grad for p in head.td_biases_r],
                            dcw=[p.grad for p in head.att_weights_r], dcb=[p.grad for p in head.att_biases_r]))
        a, b = res
        assert a['att'].shape == b['att'].shape == (c['N'], H, W, 1, 3) and a['logits'].shape == b['logits'].shape
        mask = cof.dropout_mask((c['N'] * c['P'] * c['C'],), rr.KEEP, SEED, OFFSET)
        with torch.no_grad():
            fref, amb, opened = rr.forward_bnd(c, inp, mask)
            assert int(amb.sum()) == 0, 'a relu gate within its bound of zero: the two paths may gate differently'
            rr.check_gate_condition(c, amb, opened)
            lg = rr.logits_bnd(c, inp, fref['parts'])
            bref = rr.backward_bnd(c, inp, fref['parts'], G, mask, _plan(c))

        def both(ka, bnd, what):
            ga, gb = ka(a).double().reshape(bnd.ref.shape), ka(b).double().reshape(bnd.ref.shape)
            for g, path in ((ga, 'per-op'), (gb, 'fused')):
                assert bool(((g - bnd.ref).abs() <= bnd.err).all()), '{} ({} path) outside its bound'.format(what, path)
            assert bool(((ga - gb).abs() <= 2 * bnd.err).all()), what
        both(lambda r: r['logits'], lg, 'logits')
        both(lambda r: r['att'], fref['att'], 'attention maps')
        both(lambda r: r['dX'], bref['dX'], 'dX')
        both(lambda r: r['dWa'], bref['dWa'], 'dWa')
        both(lambda r: r['dba'], bref['dba'], 'dba')
        for r in range(3):
            both(lambda x, r=r: x['dWts'][r], bref['dWts'][r], 'dWt rank %d' % r)
            both(lambda x, r=r: x['dbts'][r], bref['dbts'][r], 'dbt rank %d' % r)
        for r in range(2):
            both(lambda x, r=r: x['dcw'][r], bref['dcw'][r], 'dw of rank %d' % (r + 1))
            both(lambda x, r=r: x['dcb'][r], bref['dcb'][r], 'db of rank %d' % (r + 1))
    finally:
        apa_config.reset_cfg()
