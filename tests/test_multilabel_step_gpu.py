"""The multi-label action losses ('multi-label' / 'multi-label-2', src/loss.py:88-101) and the one-call training steps
under them, on the GPU:
  * apa_multilabel_loss_fwd_bwd (csrc/apa_mlloss.hip: ml_rows_kernel) and apa_clip_multilabel_fwd_bwd
    (csrc/apa_cliploss.hip) against float64 at the fp32 inputs, element bounds of tests/_ml_probe.py; finite; repeatable
    bit for bit; the clip form at F == 1 without temporal attention equals the rows kernel bit for bit
  * apa_attn_head_train_step_multilabel / apa_pose_attn_train_step_multilabel against the separate-call sequence, bit
    for bit, with the dispatch trace saying where the loss rode in the logits reducer (m1_logits_ml_kernel)
  * deploy.FusedHeadStep on the reference-executed fixtures (tests/golden/make_multilabel_step_reference.py), small and
    at the HICO / Charades shapes, and against the module path."""
import numpy as np
import pytest
import torch

import _ref_fixture as rf
from oracle import attn_pool_oracle as orc
from tests import _m1_probe as mp
from tests import _ml_probe as ml
from tests._m1_probe import Bnd, contract
from tests.test_multilabel_step_cpu import BIG, SMALL, ml_fixture

pytestmark = pytest.mark.gpu

EPS32 = mp.EPS32
TEMPORAL_TF = {'temporal_weights': 'TemporalAttention/Conv/weights', 'temporal_biases': 'TemporalAttention/Conv/biases'}


def _rel(got, exp, floor=1e-30):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(exp).shape)
    exp = np.asarray(exp, dtype=np.float64)
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), floor))


# ------------------------------------------------------------------------------------------------- the rows kernel
def _rows_problem(N, K, seed):
    """logits N(0, 2) with +-30 and +-90 planted (softplus and sigmoid saturated either way), multi-hot labels with an
    all-zero and an all-one row"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, K, generator=g) * 2.0
    flat = x.view(-1)
    for i, v in enumerate((30.0, -30.0, 90.0, -90.0)):
        flat[(i * 7919 + seed) % flat.numel()] = v
    t = (torch.rand(N, K, generator=g) < 0.1).float()
    t[0] = 0.0
    t[N - 1] = 1.0 if N > 1 else t[N - 1]
    return x, t


ROWS_K = [1, 3, 4, 157, 255, 256, 257, 600, 1024, 1025]
ROWS_N = [1, 6, 33, 64, 65, 70]


@pytest.mark.parametrize('kind', ml.KINDS)
def test_rows_kernel_matches_float64(gpu, kind):
    """K on either side of one, two and four columns per thread (256, 512 via 600, 1024) and odd; N on either side of the
    batch sum's change of order (64 | 65) and of its 32 slots; pw in {10, 1, 0.5} (one for multi-label-2, which ignores
    it).  G and loss within the element bounds, finite, and a second call gives the same bits."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    wt, gs = 1.3, 0.5
    worst = [0.0, 0.0]
    for pw in ((10.0, 1.0, 0.5) if kind == 'multi-label' else (10.0,)):
        for K in ROWS_K:
            for N in ROWS_N:
                x, t = _rows_problem(N, K, seed=1000 * K + N)
                want_loss, want_G = ml.rows_reference(kind, x.double(), t.double(), pw, wt, gs)
                xg, tg = x.to(gpu), t.to(gpu)
                loss, G = cof.multilabel_loss_fwd_bwd(kind, xg, tg, wt=wt, grad_scale=gs, pos_weight=pw)
                loss2, G2 = cof.multilabel_loss_fwd_bwd(kind, xg, tg, wt=wt, grad_scale=gs, pos_weight=pw)
                torch.cuda.synchronize()
                tag = '%s pw=%g N=%d K=%d' % (kind, pw, N, K)
                worst[0] = max(worst[0], ml.check(G, want_G, tag + ' G'))
                worst[1] = max(worst[1], ml.check(loss, want_loss, tag + ' loss'))
                assert torch.equal(loss, loss2) and torch.equal(G, G2), tag
    print('%s: worst G %.3f, loss %.3f of the bound' % (kind, worst[0], worst[1]))


def test_rows_kernel_agrees_with_the_one_block_kernel(gpu):
    """apa_action_loss_fwd_bwd (one block, the module path's) computes the same loss[0] and G to round-off"""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    for kind in ml.KINDS:
        x, t = _rows_problem(33, 157, seed=5)
        xg, tg = x.to(gpu), t.to(gpu)
        loss, G = cof.multilabel_loss_fwd_bwd(kind, xg, tg, wt=0.7, grad_scale=0.25)
        # (gen_losses passes wt = 1 for these kinds; the old kernel ignores wt for 'multi-label' as the new one does)
        loss1, G1 = cof.action_loss_fwd_bwd(kind, xg, tg, wt=0.7, grad_scale=0.25)
        torch.cuda.synchronize()
        assert abs(float(loss[0]) - float(loss1[0])) <= 2e-6 * abs(float(loss1[0]))
        assert _rel(G.cpu().numpy(), G1.cpu().numpy()) <= 2e-6


# ------------------------------------------------------------------------------------------------- the clip kernel
def _clip_problem(B, F, K, temporal, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * F, K, generator=g) * 2.0
    flat = x.view(-1)
    for i, v in enumerate((30.0, -30.0, 90.0, -90.0)):
        flat[(i * 7919 + seed) % flat.numel()] = v
    t = (torch.rand(B, K, generator=g) < 0.1).float()
    t[0] = 0.0
    if B > 1:
        t[B - 1] = 1.0
    w = torch.randn(K, generator=g) * (0.3 / K ** 0.5) if temporal else None
    b = torch.full((1,), 1.0 / F) + 0.1 * torch.randn(1, generator=g) if temporal else None
    return x, t, w, b


def _clip_reference(kind, x, t, w, b, B, F, K, pw, wt, gs):
    """Every output of apa_clip_multilabel_fwd_bwd as a Bnd: float64 values with the error model of tests/_m1_probe.py
    for the pooling chain (fp32 contractions over K for a, over F for pooled, over K for d, over B F for dw / db) and
    tests/_ml_probe.py's element bounds for the loss, the pooled logits' own error propagated through l' and l''."""
    X = Bnd(x.double().view(B, F, K))
    out = {}
    if w is not None:
        a = (contract('bfk,k->bf', X, Bnd(w.double()), K) + Bnd(b.double().view(1, 1).expand(B, F).clone())).rounded()
        out['tatt'] = Bnd(a.ref.reshape(-1), a.err.reshape(-1))
    else:
        a = Bnd(torch.ones(B, F, dtype=torch.float64))
    pooled = contract('bfk,bf->bk', X, a, F).scale(1.0 / F).rounded()
    out['pooled'] = pooled
    loss, g = ml.rows_reference(kind, pooled.ref, t.double(), pw, wt, gs, x_err=pooled.err)
    out['loss'] = loss
    gF = g.scale(1.0 / F).rounded()
    if w is not None:
        d = contract('bk,bfk->bf', g, X, K).scale(1.0 / F).rounded()
        G = Bnd(gF.ref[:, None, :].expand(B, F, K), gF.err[:, None, :].expand(B, F, K)).mul(
            Bnd(a.ref[:, :, None], a.err[:, :, None])) + \
            Bnd(d.ref[:, :, None], d.err[:, :, None]).mul(Bnd(w.double().view(1, 1, K)))
        out['G'] = G.rounded()
        dr = Bnd(d.ref.reshape(-1), d.err.reshape(-1))
        out['dw'] = contract('r,rk->k', dr, Bnd(x.double()), B * F)
        out['db'] = contract('r,r->', dr, Bnd(torch.ones(B * F, dtype=torch.float64)), B * F)
    else:
        out['G'] = Bnd(gF.ref[:, None, :].expand(B, F, K).clone(), gF.err[:, None, :].expand(B, F, K).clone())
    return out


CLIP_K = [1, 3, 157, 600, 1025, 4100]


@pytest.mark.parametrize('temporal', [False, True], ids=['mean', 'temporal'])
@pytest.mark.parametrize('K', CLIP_K)
def test_clip_loss_kernel_matches_float64(gpu, K, temporal):
    """F in {1, 4, 25, 70} x B in {1, 6, 70}, both kinds (F = 70 > CLIP_LDS_F re-reads tatt; K = 4100 keeps the pooled
    and gradient rows in memory; K = 1025 is past four columns per thread).  K = 4100 runs (B, F) in {(1, 1), (6, 4),
    (1, 25), (70, 1), (6, 70)} -- every F and every B once, the float64 reference of 70 x 70 x 4100 alone would take
    longer than the rest of the file."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    wt, gs, pw = 1.3, 0.5, 10.0
    shapes = [(B, F) for B in (1, 6, 70) for F in (1, 4, 25, 70)] if K < 4100 else \
        [(1, 1), (6, 4), (1, 25), (70, 1), (6, 70)]
    worst = {}
    for i, (B, F) in enumerate(shapes):
        for kind in ml.KINDS if K < 4100 else (ml.KINDS[i % 2],):
            x, t, w, b = _clip_problem(B, F, K, temporal, seed=1000 * K + 10 * B + F)
            want = _clip_reference(kind, x, t, w, b, B, F, K, pw, wt, gs)
            d = lambda v: None if v is None else v.to(gpu)
            pooled, tatt, loss, G, dw, db = cof.clip_multilabel_fwd_bwd(kind, d(x), d(t), F, d(w), d(b), wt=wt,
                                                                        grad_scale=gs, pos_weight=pw)
            torch.cuda.synchronize()
            got = dict(pooled=pooled, loss=loss, G=G)
            if temporal:
                got.update(tatt=tatt, dw=dw, db=db)
            else:
                assert tatt is None and dw is None and db is None
            for k_, v in got.items():
                r = ml.check(v, want[k_], '%s B=%d F=%d K=%d %s' % (kind, B, F, K, k_))
                worst[k_] = max(worst.get(k_, 0.0), r)
    print('K=%d %s: worst fraction of the bound %s' % (K, 'temporal' if temporal else 'mean',
                                                        {k_: round(v, 3) for k_, v in worst.items()}))


@pytest.mark.parametrize('B', [1, 6, 64, 70])
@pytest.mark.parametrize('K', [1, 3, 157, 600, 1025, 4100])
def test_clip_loss_with_one_frame_is_the_rows_kernel_bit_for_bit(gpu, K, B):
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    for kind in ml.KINDS:
        x, t, _, _ = _clip_problem(B, 1, K, False, seed=7 * K + B)
        x, t = x.to(gpu), t.to(gpu)
        pooled, _, loss, G, _, _ = cof.clip_multilabel_fwd_bwd(kind, x, t, 1, wt=0.7, grad_scale=0.25, pos_weight=3.0)
        loss2, G2 = cof.multilabel_loss_fwd_bwd(kind, x, t, wt=0.7, grad_scale=0.25, pos_weight=3.0)
        torch.cuda.synchronize()
        assert torch.equal(pooled, x)
        assert torch.equal(loss, loss2), (loss - loss2).abs().max()
        assert torch.equal(G, G2), (G - G2).abs().max()


def test_clip_loss_repeat_calls_are_bit_identical(gpu):
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    for B, F, K, temporal in ((33, 25, 157, True), (8, 4, 157, True), (5, 3, 1025, True), (33, 3, 600, False)):
        x, t, w, b = _clip_problem(B, F, K, temporal, seed=3)
        d = lambda v: None if v is None else v.to(gpu)
        x, t, w, b = d(x), d(t), d(w), d(b)
        first = cof.clip_multilabel_fwd_bwd('multi-label', x, t, F, w, b, wt=1.3, grad_scale=0.5)
        again = cof.clip_multilabel_fwd_bwd('multi-label', x, t, F, w, b, wt=1.3, grad_scale=0.5)
        torch.cuda.synchronize()
        for a_, b_ in zip(first, again):
            assert (a_ is None and b_ is None) or torch.equal(a_, b_)


# ------------------------------------------------------------------------------ one call == the separate calls
P_ = 9


def _head_problem(gpu, dtype, N, C, K, M, n_loss, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.relu(torch.randn(N, P_, C, generator=g)).to(dtype).to(gpu)
    Wa = (torch.randn(C, M, generator=g) / C ** 0.5).to(gpu)
    ba = (torch.randn(M, generator=g) * 0.1).to(gpu)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(gpu)
    bt = (torch.randn(K, generator=g) * 0.1).to(gpu)
    t = (torch.rand(n_loss, K, generator=g) < 0.1).float()
    t[0] = 0.0
    tw = (torch.randn(K, generator=g) * 0.3).to(gpu)
    return X, Wa, ba, Wt, bt, t.to(gpu), tw


FLAT = [
    # id, dtype, N, C, K, per_class, kind, the loss rides in the logits reducer
    ('fold_fp32_n6_k157', torch.float32, 6, 512, 157, False, 'multi-label', True),
    ('fold_bf16_n33_k600', torch.bfloat16, 33, 512, 600, False, 'multi-label-2', True),
    ('k1025_beyond_the_fold', torch.float32, 6, 512, 1025, False, 'multi-label', False),
    ('generic_c32_k20', torch.float32, 6, 32, 20, False, 'multi-label-2', False),
    ('perclass_c64_k12', torch.float32, 6, 64, 12, True, 'multi-label', False),
]


@pytest.mark.parametrize('case', FLAT, ids=[c[0] for c in FLAT])
def test_flat_step_in_one_call_equals_the_separate_calls(gpu, case):
    """apa_attn_head_train_step_multilabel (cof.HeadTrainStep(action_loss=...)) against apa_attn_pool_fwd,
    apa_multilabel_loss_fwd_bwd, apa_attn_pool_bwd back to back with the same (seed, offset): every output bit for bit.
    The raw trace (tests/_ml_probe.py) says which reducer formed the logits: 6 = m1_logits_ml_kernel where M == 1,
    C % 128 == 0 and 4 <= K <= 832 (the small-K route's range), anything else where the rows kernel ran on finished
    logits -- K = 1025, C = 32 (no small-K route) and the per-class maps."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    _, dtype, N, C, K, per_class, kind, folded = case
    M = K if per_class else 1
    X, Wa, ba, Wt, bt, t, _ = _head_problem(gpu, dtype, N, C, K, M, N, seed=K + C)
    kw = dict(flags=cof.attn_flags(False, per_class, True), keep_prob=0.5, seed=11, offset=4)
    wt, gs, pw = 1.3, 0.5, 10.0
    nan = lambda v: torch.full_like(v, float('nan'))
    ga = (nan(X), None, nan(Wa), nan(ba), nan(Wt), nan(bt))
    gb = (nan(X), None, nan(Wa), nan(ba), nan(Wt), nan(bt))
    st = cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, t, ga, loss_wt=wt, grad_scale=gs, action_loss=kind, pos_weight=pw, **kw)
    tr = ml.run_traced(st)
    logits, att, zs, ab, _, ws = cof.attn_pool_fwd(X, X, Wa, ba, Wt, bt, **kw)
    loss, G = cof.multilabel_loss_fwd_bwd(kind, logits, t, wt=wt, grad_scale=gs, pos_weight=pw)
    cof.attn_pool_bwd(X, X, Wa, ba, Wt, bt, att, zs, ab, G, workspace=ws, out=gb, **kw)
    torch.cuda.synchronize()
    assert (tr.logits == ml.M1_LOGITS_ML) == folded, tr.logits
    assert tuple(st.loss.shape) == (1 + N,)
    pairs = dict(logits=(st.logits, logits), att=(st.att, att), zsave=(st.zsave, zs), loss=(st.loss, loss),
                 G=(st.G, G), dX=(ga[0], gb[0]), dWa=(ga[2], gb[2]), dba=(ga[3], gb[3]), dWt=(ga[4], gb[4]),
                 dbt=(ga[5], gb[5]))
    if not per_class:
        pairs['abar'] = (st.abar, ab)
    for k_, (a_, b_) in pairs.items():
        assert not torch.isnan(a_.float()).any(), k_
        assert torch.equal(a_.view_as(b_), b_), k_
    # ... and through the product's own entry point, the bits of the traced run
    first = [v.clone() for v in (st.logits, st.loss, st.G, ga[0], ga[4])]
    st.run()
    torch.cuda.synchronize()
    for a_, b_ in zip(first, (st.logits, st.loss, st.G, ga[0], ga[4])):
        assert torch.equal(a_, b_)
    # the loss itself against float64 at the step's own logits
    want_loss, want_G = ml.rows_reference(kind, st.logits.double().cpu(), t.double().cpu(), pw, wt, gs)
    ml.check(st.G, want_G, case[0] + ' G')
    ml.check(st.loss, want_loss, case[0] + ' loss')


N_, F_ = 6, 2


@pytest.mark.parametrize('temporal', [False, True], ids=['mean', 'temporal'])
@pytest.mark.parametrize('dtype,C,K,per_class', [(torch.float32, 32, 20, False), (torch.bfloat16, 512, 157, False),
                                                 (torch.float32, 64, 12, True)],
                         ids=['m1_fp32_c32', 'm1_bf16_c512_k157', 'perclass_fp32_c64_k12'])
def test_head_clip_step_in_one_call_equals_the_separate_calls(gpu, dtype, C, K, per_class, temporal):
    """3 clips x 2 frames: apa_attn_head_train_step_multilabel with a clip descriptor against apa_attn_pool_fwd,
    apa_clip_multilabel_fwd_bwd, apa_attn_pool_bwd, bit for bit."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    M = K if per_class else 1
    B = N_ // F_
    X, Wa, ba, Wt, bt, t, tw = _head_problem(gpu, dtype, N_, C, K, M, B, seed=K + C + 1)
    tb = torch.full((1,), 1.0 / F_).to(gpu)
    if not temporal:
        tw = tb = None
    kw = dict(flags=cof.attn_flags(False, per_class, True), keep_prob=0.5, seed=11, offset=4)
    wt, gs, kind = 1.3, 0.5, 'multi-label'
    nan = lambda v: torch.full_like(v, float('nan'))
    ga = (nan(X), None, nan(Wa), nan(ba), nan(Wt), nan(bt))
    gb = (nan(X), None, nan(Wa), nan(ba), nan(Wt), nan(bt))
    tg = (nan(tw), nan(tb)) if temporal else None
    st = cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, t, ga, loss_wt=wt, grad_scale=gs, frames=F_, action_loss=kind,
                           temporal=(tw, tb) if temporal else None, temporal_grads=tg, **kw)
    st.run()
    logits, att, zs, ab, _, ws = cof.attn_pool_fwd(X, X, Wa, ba, Wt, bt, **kw)
    pooled, tatt, loss, G, dw, db = cof.clip_multilabel_fwd_bwd(kind, logits, t, F_, tw, tb, wt=wt, grad_scale=gs)
    cof.attn_pool_bwd(X, X, Wa, ba, Wt, bt, att, zs, ab, G, workspace=ws, out=gb, **kw)
    torch.cuda.synchronize()
    assert tuple(st.loss.shape) == (1 + B,) and tuple(st.pooled.shape) == (B, K)
    pairs = dict(logits=(st.logits, logits), att=(st.att, att), zsave=(st.zsave, zs), pooled=(st.pooled, pooled),
                 loss=(st.loss, loss), G=(st.G, G), dX=(ga[0], gb[0]), dWa=(ga[2], gb[2]), dba=(ga[3], gb[3]),
                 dWt=(ga[4], gb[4]), dbt=(ga[5], gb[5]))
    if not per_class:
        pairs['abar'] = (st.abar, ab)
    if temporal:
        pairs.update(tatt=(st.tatt, tatt), dw=(tg[0], dw), db=(tg[1], db))
    for k_, (a_, b_) in pairs.items():
        assert not torch.isnan(a_.float()).any(), k_
        assert torch.equal(a_.view_as(b_), b_), k_


@pytest.mark.parametrize('form', ['flat', 'clips_mean', 'clips_temporal'])
@pytest.mark.parametrize('dtype,C,K', [(torch.float32, 32, 20), (torch.bfloat16, 512, 20)],
                         ids=['cfg003_fp32_c32', 'cfg003_bf16_c512_k20'])
def test_cfg003_step_in_one_call_equals_the_separate_calls(gpu, dtype, C, K, form):
    """apa_pose_attn_train_step_multilabel (cof.PoseAttnTrainStep(action_loss=...)) against the sequence
    apa_pose_head_fwd, apa_pose_l2_loss_fwd_bwd, apa_attn_pool_fwd, the multi-label loss (rows or clip form),
    apa_attn_pool_bwd (APA_FLAG_DXATT_RANK1), apa_pose_head_bwd_rank1ext: every output bit for bit, flat and on clips,
    fp32 and bf16.  The entry point runs those very calls for every shape.  cfg003_bf16_c512_k20-flat is the shape at
    which the SOFTMAX step takes its fast bf16 route, whose shared launches sum in other orders than the per-op kernels
    (with them under the multi-label loss this comparison measured att 2.5e-7, logits 4.4e-7, zsave 2.9e-7, dWa 9.4e-7,
    dWt 2.4e-7 relative to max |value|); the multi-label step promises the bits of the separate calls and does not use
    them.  What the same kernel computes from the same operands is asserted first (the loss recomputed from the step's
    own logits); then every output, each figure printed before it is asserted."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    Cp, J = 768, 16
    clips = form != 'flat'
    temporal = form == 'clips_temporal'
    F = F_ if clips else 1
    B = N_ // F
    g = torch.Generator().manual_seed(C + K)
    d = lambda v: v.to(gpu).contiguous()
    X = d(torch.relu(torch.randn(N_, P_, C, generator=g)).to(dtype))
    W1, b1 = d(torch.randn(C, Cp, generator=g) / C ** 0.5), d(torch.randn(Cp, generator=g) * 0.1)
    W2, b2 = d(torch.randn(Cp, J, generator=g) / Cp ** 0.5), d(torch.randn(J, generator=g) * 0.1)
    Wa, ba = d(torch.randn(Cp, 1, generator=g) / Cp ** 0.5), d(torch.randn(1, generator=g) * 0.1)
    Wt, bt = d(torch.randn(C, K, generator=g) / C ** 0.5), d(torch.randn(K, generator=g) * 0.1)
    t = (torch.rand(B, K, generator=g) < 0.1).float()
    t[0] = 0.0
    t = d(t)
    lbl, valid = d(torch.rand(N_, P_, J, generator=g)), d(torch.rand(N_, J, generator=g) > 0.3)
    tw, tb = (d(torch.randn(K, generator=g) * 0.3), d(torch.full((1,), 1.0 / F))) if temporal else (None, None)
    kw = dict(flags=cof.attn_flags(False, False, True), keep_prob=0.5, seed=9, offset=7)
    wts = dict(action_wt=1.3, pose_wt=0.7, grad_scale=0.5)
    kind, pw = 'multi-label-2', 10.0

    def action_loss(lg):
        if clips:
            return cof.clip_multilabel_fwd_bwd(kind, lg, t, F, tw, tb, wt=wts['action_wt'],
                                               grad_scale=wts['grad_scale'], pos_weight=pw)
        loss_, G_ = cof.multilabel_loss_fwd_bwd(kind, lg, t, wt=wts['action_wt'], grad_scale=wts['grad_scale'],
                                                pos_weight=pw)
        return None, None, loss_, G_, None, None

    Ppre, Pl, pws = cof.pose_head_fwd(X, W1, b1, W2, b2)
    lossp, dPl = cof.pose_l2_loss_fwd_bwd(Pl, lbl, valid, wt=wts['pose_wt'], grad_scale=wts['grad_scale'])
    logits, att, zs, ab, _, ws = cof.attn_pool_fwd(X, Ppre, Wa, ba, Wt, bt, **kw)
    pooled, tatt, lossx, G, dw, db = action_loss(logits)
    dX, dZ, dWa, dba, dWt, dbt = cof.attn_pool_bwd(X, Ppre, Wa, ba, Wt, bt, att, zs, ab, G, workspace=ws,
                                                   dxatt_rank1=True, **kw)
    dXf, dW1, db1, dW2, db2 = cof.pose_head_bwd(X, W1, W2, Ppre, dPl, None, dX=dX, accumulate_dX=True, workspace=pws,
                                                ext_rank1=(dZ, Wa.view(-1)))
    nan = lambda v: torch.full_like(v, float('nan'))
    prm = (W1, b1, W2, b2, Wa, ba, Wt, bt)
    grads = (nan(X),) + tuple(nan(v) for v in prm)
    tg = (nan(tw), nan(tb)) if temporal else None
    extra = dict(frames=F, temporal=(tw, tb) if temporal else None, temporal_grads=tg) if clips else {}
    st = cof.PoseAttnTrainStep(X, prm, t, lbl, valid, grads, action_loss=kind, pos_weight=pw, **extra, **kw, **wts)
    st.run()
    torch.cuda.synchronize()
    assert tuple(st.loss_action.shape) == (1 + B,)
    # the loss from the step's own logits: the same row routine on the same operands
    again = action_loss(st.logits)
    torch.cuda.synchronize()
    mine = ((st.pooled, st.tatt) if clips else (None, None)) + (st.loss_action, st.G) + \
        ((tg[0], tg[1]) if temporal else (None, None))
    for a_, b_ in zip(mine, again):
        assert (a_ is None and b_ is None) or torch.equal(a_.view_as(b_), b_)
    pairs = dict(Ppre=(st.Ppre, Ppre), Pl=(st.Pl, Pl), dPl=(st.dPl, dPl), att=(st.att, att), loss_pose=(st.loss_pose, lossp),
                 logits=(st.logits, logits), zsave=(st.zsave, zs), abar=(st.abar, ab), loss=(st.loss_action, lossx),
                 G=(st.G, G), dZ=(st.dZ, dZ), dX=(grads[0], dXf), dW1=(grads[1], dW1), db1=(grads[2], db1),
                 dW2=(grads[3], dW2), db2=(grads[4], db2), dWa=(grads[5], dWa), dba=(grads[6], dba),
                 dWt=(grads[7], dWt), dbt=(grads[8], dbt))
    if clips:
        pairs['pooled'] = (st.pooled, pooled)
    if temporal:
        pairs.update(tatt=(st.tatt, tatt), dw=(tg[0], dw), db=(tg[1], db))
    for k_, (a_, b_) in pairs.items():
        print('%-10s rel diff %.3e' % (k_, _rel(a_.float().cpu().numpy(), b_.float().cpu().numpy())))
    for k_, (a_, b_) in pairs.items():
        assert not torch.isnan(a_.float()).any(), k_
        assert torch.equal(a_.view_as(b_), b_), k_


# -------------------------------------------------------------------- deploy.FusedHeadStep on the reference fixtures
_CACHE = {}


def _fixture(name):
    if name not in _CACHE:
        _CACHE[name] = ml_fixture(name)
    return _CACHE[name]


def _load(fx, gpu):
    network_fn, cfg = rf.build_head(fx, device=gpu)
    table = rf.module_tf_names(network_fn)
    with torch.no_grad():
        for vn, v in table.items():
            v.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).to(gpu))
    if network_fn.temporal is not None:
        network_fn.temporal._bias_initialised = True            # the fixture's value, not the 1/F initialiser
    network_fn.head.seed, network_fn.head._step = int(fx.meta['libmask'][0]), int(fx.meta['libmask'][1])
    return network_fn, cfg, table


def _fused_step_against_fixture(fx, gpu, bf, upstream=1.0, label_dtype=torch.float32):
    """tests/test_video_step_gpu.py's check of ref_vstep_*, at its tolerances, for flat and clip input: total, Losses,
    every end point, images.grad and every trainable variable's gradient in the bucket"""
    from attentionalpoolingaction_amd import deploy
    network_fn, cfg, table = _load(fx, gpu)
    head = network_fn.head
    fused = deploy.FusedHeadStep(network_fn, cfg)
    fused.make_optimizer(0.01)
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu).to(torch.bfloat16 if bf else torch.float32)
    clips = images.dim() == 5
    B = images.shape[0]
    F = images.shape[1] if clips else 1
    images.requires_grad_(True)
    use_pose = bool(fx.meta['train_cfg']['LOSS_FN_POSE'])
    lp = torch.from_numpy(fx.arrays['in/labels_pose']).to(gpu) if use_pose else None
    lv = torch.from_numpy(fx.arrays['in/labels_pose_valid']).to(gpu) if use_pose else None
    if use_pose and clips and B > 1:
        lp, lv = lp.view(B, F, *lp.shape[1:]), lv.view(B, F, -1)
    labels = torch.from_numpy(fx.arrays['in/labels_action_multihot']).to(gpu).to(label_dtype)
    total, ep = fused(images, labels, lp, lv)
    (upstream * total).backward()
    assert head._step == int(fx.meta['libmask'][1]) + 1
    tag = fx.name + (' bf16' if bf else ' fp32')
    exp_logits = fx.expected('out/logits').astype(np.float64)
    got_logits = ep['Logits'].float().cpu().numpy().astype(np.float64)
    assert got_logits.shape == (B, fx.meta['num_classes'])
    err = np.abs(got_logits - exp_logits).max()
    print('%s: logits max abs err %.3e (max |logit| %.3f)' % (tag, err, np.abs(exp_logits).max()))
    if bf:
        assert err <= min(3e-3, 0.03 * float(np.abs(exp_logits).max()))
    else:
        assert err <= 1e-3 and _rel(got_logits, exp_logits) < 2e-5
    tol, tolp = (1.2e-2, 8e-3) if bf else (5e-5, 5e-5)
    want_eps = {'Logits', 'PosePrelogitsBasedAttention', 'Losses'}
    if clips:
        want_eps.add('logits_beforePool')
        if network_fn.temporal is not None:
            want_eps.add('TemporalAttention')
    if fused.pose_form:
        want_eps.add('PoseLogits')
    assert set(ep) == want_eps
    for name in sorted(want_eps - {'Logits', 'Losses'}):
        got = ep[name].detach().float().cpu().numpy()
        if not fx.has('out/ep/' + name):        # a benchmark-shape fixture keeps the small end points only
            assert fx.meta.get('big'), name
            continue
        fx.check('out/ep/' + name, got, tol, '%s %s' % (tag, name), floor=1e-6)
    exp_losses = fx.expected('out/losses')
    assert len(ep['Losses']) == len(exp_losses)
    ltol_ = 2e-3 if bf else 2e-5
    for g_, e_ in zip(ep['Losses'], exp_losses):
        print('%s: loss %.8g, fixture %.8g' % (tag, float(g_), e_))
        assert abs(float(g_) - e_) <= ltol_ * max(abs(e_), 1e-3)
    assert abs(float(total) - exp_losses.sum()) <= ltol_ * exp_losses.sum()
    assert images.grad.shape == images.shape
    fx.check('grad/images', images.grad.float().cpu().numpy() / upstream, tol, tag + ' grad/images', tol_proj=tolp)
    wd = fx.meta['weight_decay']
    names = dict(head.tf_variable_names(), **TEMPORAL_TF)
    for n in fused._written:            # the regulariser's wd * w is the optimiser's: added here as the fixture has it
        full = fused.bucket.views[n].double().cpu().numpy() / upstream + \
            (wd * fused.params[n].detach().double().cpu().numpy() if n in fused.regularized else 0.0)
        fx.check('grad/var/' + names[n], full.reshape(fx.variables[names[n]].shape), tol, tag + ' ' + n, tol_proj=tolp)
    return fused


@pytest.mark.parametrize('name', SMALL)
def test_fused_head_step_matches_the_reference_fixture(gpu, name):
    """fp32 cases: logits 1e-3 absolute and 2e-5 relative, gradients 5e-5; the bf16 case (a quant='bf16' fixture run
    with bf16 features): logits 3e-3, gradients 1.2e-2 of max|reference|.  The labels go in as int64 once (any dtype is
    converted to float32)."""
    from attentionalpoolingaction_amd import config as apa_config
    fx = _fixture(name)
    try:
        _fused_step_against_fixture(fx, gpu, bf=fx.quant == 'bf16',
                                    label_dtype=torch.int64 if name == 'flat002_ml2_c32' else torch.float32)
    finally:
        apa_config.reset_cfg()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', BIG)
def test_fused_head_step_matches_the_reference_at_the_hico_and_charades_shapes(gpu, name, dtype):
    """32 x 14 x 14 x 2048 with 600 classes, and 8 clips x 4 frames x 14 x 14 x 2048 with 157 classes and temporal
    attention, at fp32 and bf16 (a non-unit upstream coefficient on top)."""
    from attentionalpoolingaction_amd import config as apa_config
    fx = _fixture('big_' + name)
    assert fx.quant == 'bf16'
    try:
        _fused_step_against_fixture(fx, gpu, bf=dtype == 'bf16', upstream=2.0)
    finally:
        apa_config.reset_cfg()


def test_fused_head_step_on_clips_agrees_with_the_module_path(gpu):
    """A random clip batch on clip_temporal_ml's network: network_fn + gen_losses + autograd (the one-block loss kernel)
    against FusedHeadStep, to fp32 round-off (2e-5): the pooled logits, the total, images.grad and every gradient the
    step writes."""
    from attentionalpoolingaction_amd import config as apa_config, deploy, loss as apa_loss
    fx = _fixture('clip_temporal_ml')
    try:
        g = torch.Generator().manual_seed(17)
        shape = fx.arrays['in/images'].shape
        K = fx.meta['num_classes']
        x = torch.relu(torch.randn(*shape, generator=g))
        labels = (torch.rand(shape[0], K, generator=g) < 0.2).float().to(gpu)
        # module path
        network_fn, cfg, table = _load(fx, gpu)
        images = x.to(gpu).requires_grad_(True)
        logits, ep = network_fn(images)
        tc = fx.meta['train_cfg']
        losses = apa_loss.gen_losses(labels, logits, tc['LOSS_FN_ACTION'], K, tc['LOSS_FN_ACTION_WT'], None, None, '',
                                     None, tc['LOSS_FN_POSE_WT'], ep, cfg)
        total = sum(losses)
        total.backward()
        # one call
        network_fn2, cfg2, table2 = _load(fx, gpu)
        fused = deploy.FusedHeadStep(network_fn2, cfg2)
        images2 = x.to(gpu).requires_grad_(True)
        total2, ep2 = fused(images2, labels)
        total2.backward()
        torch.cuda.synchronize()
        n = lambda v: v.detach().float().cpu().numpy()
        assert _rel(n(ep2['Logits']), n(logits)) <= 2e-5
        assert _rel(n(ep2['logits_beforePool']), n(ep['logits_beforePool'])) <= 2e-5
        assert _rel(n(ep2['TemporalAttention']), n(ep['TemporalAttention'])) <= 2e-5
        assert abs(float(total2) - float(total)) <= 2e-5 * abs(float(total))
        assert _rel(n(images2.grad), n(images.grad)) <= 2e-5
        params = dict(fused.head.tf_variable_names(), **TEMPORAL_TF)
        for name in fused._written:
            assert _rel(n(fused.bucket.views[name]), n(table[params[name]].grad)) <= 2e-5, name
    finally:
        apa_config.reset_cfg()
