"""The one-call training step on video clips, on the GPU:
  * apa_clip_xent_fwd_bwd (csrc/apa_cliploss.hip) against oracle.frame_pooling + a float64 cross-entropy, over every K at
    which its code takes another path; bit-identical to apa_softmax_xent_fwd_bwd at F == 1; repeatable bit for bit
  * apa_attn_head_train_step_clips / apa_pose_attn_train_step_clips against the separate-call sequence, bit for bit
  * deploy.FusedHeadStep on [B,F,H,W,C] input against the reference-executed fixtures
    (tests/golden/make_video_step_reference.py), small and at the benchmark shape, and against the module path."""
import os

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from oracle import attn_pool_oracle as orc

pytestmark = pytest.mark.gpu

SMALL = ['framepool_train', 'temporal_att_train', 'perclass_temporal_train', 'perclass_framepool_bf16_c256',
         'cfg003_temporal_train', 'cfg003_one_clip_f5', 'cfg003_framepool_bf16_c512']
BIG = ['hmdb51_perclass_8x4_libmask', 'cfg003_8x4_libmask']
TEMPORAL_TF = {'temporal_weights': 'TemporalAttention/Conv/weights', 'temporal_biases': 'TemporalAttention/Conv/biases'}


def _rel(got, exp, floor=1e-30):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(exp).shape)
    exp = np.asarray(exp, dtype=np.float64)
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), floor))


# ------------------------------------------------------------------------------------------ the clip loss kernel
def _clip_problem(B, F, K, temporal, seed):
    """Frame logits of the size a trained head gives (|x| < ~2).  The scale matters for what a RELATIVE bound on the
    loss can mean: loss_b = logsumexp(p) - p[label] is a difference of fp32 numbers of size max|p|, so any fp32
    evaluation carries ~2^-24 max|p| of absolute error however small the loss is; with logits of size 5 a clip whose
    label dominates has a loss of 1e-3 and no fp32 code (apa_softmax_xent_fwd_bwd included, to which this kernel is
    bit-identical at F = 1) resolves it to 2e-5 of itself.  At this scale every clip's loss is O(1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * F, K, generator=g) * 0.5
    labels = torch.randint(0, K, (B,), generator=g)
    w = torch.randn(K, generator=g) * 0.3 if temporal else None
    b = torch.full((1,), 1.0 / F) + 0.1 * torch.randn(1, generator=g) if temporal else None
    return x, labels, w, b


def _clip_reference(x, labels, w, b, F, wt, gs):
    """oracle.frame_pooling + a float64 softmax cross-entropy; gradients of grad_scale * loss by autograd"""
    xd = x.double().requires_grad_(True)
    wd = w.double().view(-1, 1).requires_grad_(True) if w is not None else None
    bd = b.double().requires_grad_(True) if b is not None else None
    pooled, ep = orc.frame_pooling(xd, F, wd, bd)
    per = -torch.log_softmax(pooled, dim=1).gather(1, labels.view(-1, 1)).view(-1)
    total = wt * per.mean()
    (gs * total).backward()
    out = dict(pooled=pooled.detach(), loss=torch.cat([total.detach().view(1), per.detach()]), G=xd.grad)
    if w is not None:
        out.update(tatt=ep['TemporalAttention'].detach().reshape(-1), dw=wd.grad.view(-1), db=bd.grad)
    return out


# 1 / 3: the stream arithmetic below the vector width; 4 / 51 / 393 / 600: NV4 = 1, 1, 4, 8 of the half-wave form;
# 1025: the stream arithmetic above it; 4100: pooled and gradient rows in memory instead of LDS
@pytest.mark.parametrize('temporal', [False, True], ids=['mean', 'temporal'])
@pytest.mark.parametrize('K', [1, 3, 4, 51, 393, 600, 1025, 4100])
def test_clip_loss_kernel_matches_float64(gpu, K, temporal):
    """pooled, tatt, loss, G, dw, db within 2e-5 of max|reference| (the figure test_pose_att_logits_gpu.py holds fp32
    arithmetic to), B in {1, 2, 33} x F in {1, 2, 3, 25}, wt = 1.3, grad_scale = 0.5.  (B = 33 with F = 25: 825 rows,
    more than one pass of every loop; K = 4100 runs B in {1, 2} x F in {1, 3} only.)"""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    wt, gs = 1.3, 0.5
    shapes = [(B, F) for B in (1, 2, 33) for F in (1, 2, 3, 25)] if K <= 1025 else [(1, 1), (2, 3), (1, 3), (2, 1)]
    for B, F in shapes:
        x, labels, w, b = _clip_problem(B, F, K, temporal, seed=1000 * K + 10 * B + F)
        want = _clip_reference(x, labels, w, b, F, wt, gs)
        d = lambda t: None if t is None else t.to(gpu)
        pooled, tatt, loss, G, dw, db = cof.clip_xent_fwd_bwd(d(x), d(labels), F, d(w), d(b), wt=wt, grad_scale=gs)
        torch.cuda.synchronize()
        got = dict(pooled=pooled, loss=loss, G=G)
        if temporal:
            got.update(tatt=tatt, dw=dw, db=db)
        else:
            assert tatt is None and dw is None and db is None
        for k_, v in got.items():
            e = _rel(v.cpu().numpy(), want[k_].numpy())
            assert e <= 2e-5, 'B=%d F=%d K=%d %s: %.3e' % (B, F, K, k_, e)


@pytest.mark.parametrize('B', [1, 6, 64, 70])
@pytest.mark.parametrize('K', [3, 51, 393, 1025])
def test_clip_loss_with_one_frame_is_the_softmax_cross_entropy_bit_for_bit(gpu, K, B):
    """F == 1 without temporal attention: pooled == logits and loss, G == apa_softmax_xent_fwd_bwd's, BIT-identical --
    K = 51 / 393 through the shared row routine (pc_row_xent_any), K = 3 / 1025 through the stream arithmetic; B = 64 /
    70 on either side of the batch-mean's change of summation order."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    x, labels, _, _ = _clip_problem(B, 1, K, False, seed=7 * K + B)
    x, labels = x.to(gpu), labels.to(gpu)
    pooled, _, loss, G, _, _ = cof.clip_xent_fwd_bwd(x, labels, 1, wt=0.7, grad_scale=0.25)
    loss2, G2, _, _ = cof.softmax_xent_fwd_bwd(x, labels, wt=0.7, grad_scale=0.25)
    torch.cuda.synchronize()
    assert torch.equal(pooled, x)
    assert torch.equal(loss, loss2), (loss - loss2).abs().max()
    assert torch.equal(G, G2), (G - G2).abs().max()


def test_clip_loss_repeat_calls_are_bit_identical(gpu):
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    for B, F, K, temporal in ((33, 25, 51, True), (8, 4, 51, True), (5, 3, 1025, True), (33, 3, 393, False)):
        x, labels, w, b = _clip_problem(B, F, K, temporal, seed=3)
        d = lambda t: None if t is None else t.to(gpu)
        x, labels, w, b = d(x), d(labels), d(w), d(b)
        first = cof.clip_xent_fwd_bwd(x, labels, F, w, b, wt=1.3, grad_scale=0.5)
        for _ in range(3):
            again = cof.clip_xent_fwd_bwd(x, labels, F, w, b, wt=1.3, grad_scale=0.5)
            torch.cuda.synchronize()
            for a_, b_ in zip(first, again):
                assert (a_ is None and b_ is None) or torch.equal(a_, b_)


# ------------------------------------------------------------------------------ one call == the separate calls
N_, F_, P_ = 6, 3, 9


def _head_problem(gpu, dtype, C, K, M, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.relu(torch.randn(N_, P_, C, generator=g)).to(dtype).to(gpu)
    Wa = (torch.randn(C, M, generator=g) / C ** 0.5).to(gpu)
    ba = (torch.randn(M, generator=g) * 0.1).to(gpu)
    Wt = (torch.randn(C, K, generator=g) / C ** 0.5).to(gpu)
    bt = (torch.randn(K, generator=g) * 0.1).to(gpu)
    labels = torch.randint(0, K, (N_ // F_,), generator=g).to(gpu)
    tw = (torch.randn(K, generator=g) * 0.3).to(gpu)
    tb = torch.full((1,), 1.0 / F_).to(gpu)
    return X, Wa, ba, Wt, bt, labels, tw, tb


@pytest.mark.parametrize('temporal', [False, True], ids=['mean', 'temporal'])
@pytest.mark.parametrize('dtype,C,K,per_class', [(torch.float32, 32, 51, False), (torch.bfloat16, 512, 51, False),
                                                 (torch.bfloat16, 256, 51, True), (torch.float32, 64, 70, True)],
                         ids=['m1_fp32_c32', 'm1_bf16_c512', 'perclass_fused_bf16_c256_k51', 'perclass_generic_fp32_k70'])
def test_head_clip_step_in_one_call_equals_the_separate_calls(gpu, dtype, C, K, per_class, temporal):
    """apa_attn_head_train_step_clips (cof.HeadTrainStep(frames=...)) against apa_attn_pool_fwd, apa_clip_xent_fwd_bwd,
    apa_attn_pool_bwd back to back with the same (seed, offset): every output bit for bit.  N = 6 frames as 2 clips x
    3, P = 9.  Routes, from the host predicates:
      m1_fp32_c32                   M == 1, C = 32 is neither a streaming (C % 1024) nor a vector (C = 256 / 512) width:
                                    the generic run-time-loop kernels (m1g); C % 128 != 0: no small-K head kernels
      m1_bf16_c512                  M == 1, C = 64 * 8: the register-resident vector kernels (m1v); C % 128 == 0 and
                                    16-byte aligned G / Wt / z: the small-K head kernels (m1_small_route_ok)
      perclass_fused_bf16_c256_k51  M == K <= 64, bf16, C % 256 == 0: the fused per-class kernels (pc_fused_supported);
                                    P = 9 < 32, so the activation pass keeps its own launch; the backward half reuses
                                    the prepared slab and the keep bits (APA_FLAG_WS_FROM_FWD)
      perclass_generic_fp32_k70     M == K > 64, fp32: the generic GEMM route"""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    M = K if per_class else 1
    X, Wa, ba, Wt, bt, labels, tw, tb = _head_problem(gpu, dtype, C, K, M, seed=K + C)
    if not temporal:
        tw = tb = None
    kw = dict(flags=cof.attn_flags(False, per_class, True), keep_prob=0.5, seed=11, offset=4)
    wt, gs = 1.3, 0.5
    nan = lambda t: torch.full_like(t, float('nan'))
    ga = (nan(X), None, nan(Wa), nan(ba), nan(Wt), nan(bt))
    gb = (nan(X), None, nan(Wa), nan(ba), nan(Wt), nan(bt))
    tg = (nan(tw), nan(tb)) if temporal else None
    st = cof.HeadTrainStep(X, X, Wa, ba, Wt, bt, labels, ga, loss_wt=wt, grad_scale=gs, frames=F_,
                           temporal=(tw, tb) if temporal else None, temporal_grads=tg, **kw)
    st.run()
    logits, att, zs, ab, _, ws = cof.attn_pool_fwd(X, X, Wa, ba, Wt, bt, **kw)
    pooled, tatt, loss, G, dw, db = cof.clip_xent_fwd_bwd(logits, labels, F_, tw, tb, wt=wt, grad_scale=gs)
    cof.attn_pool_bwd(X, X, Wa, ba, Wt, bt, att, zs, ab, G, workspace=ws, out=gb, **kw)
    torch.cuda.synchronize()
    assert tuple(st.loss.shape) == (1 + N_ // F_,) and tuple(st.pooled.shape) == (N_ // F_, K)
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


@pytest.mark.parametrize('temporal', [False, True], ids=['mean', 'temporal'])
@pytest.mark.parametrize('dtype,C,K', [(torch.float32, 32, 20), (torch.bfloat16, 512, 20)],
                         ids=['cfg003_fp32_c32', 'cfg003_bf16_c512_k20'])
def test_cfg003_clip_step_in_one_call_equals_the_separate_calls(gpu, dtype, C, K, temporal):
    """apa_pose_attn_train_step_clips (cof.PoseAttnTrainStep(frames=...)) against the sequence apa_pose_head_fwd,
    apa_pose_l2_loss_fwd_bwd, apa_attn_pool_fwd, apa_clip_xent_fwd_bwd, apa_attn_pool_bwd (APA_FLAG_DXATT_RANK1),
    apa_pose_head_bwd_rank1ext: every output bit for bit.  Cp = 768, J = 16, N = 6 as 2 x 3, P = 9.  Routes:
      cfg003_fp32_c32        fp32 features fail pose_step_fast_ok (bf16 only): the flat apa_pose_attn_train_step would
                             take its composed route, and so does the clip step -- these very calls inside the entry point
      cfg003_bf16_c512_k20   bf16, J = 16, Cp = 768 in {256, 512, 768, 1024}, Ppre / W2 / Wa 16-byte aligned
                             (pose_step_fast_ok), Cp % 8 == 0 (m1_supported), C % 128 == 0 with aligned G / Wt / z
                             (m1_small_route_ok): the shape at which the FLAT step takes its fast route.  That route's
                             shared launches sum in other orders than the per-op kernels (measured here with them in
                             the clip step: att 2.5e-7, logits 4.4e-7, dX 1.6e-3 in bf16, dW1 6.6e-5 -- the flat step
                             differs from its four calls in the same way, tests/test_dense_gpu.py holds that pair to
                             2e-6 / 2e-4), so the clip step, which promises the bits of the separate calls, runs the
                             four-call sequence at this shape too: the pose head's bf16 MFMA products, the M == 1
                             vector kernels (m1v, C = 64 * 8) and the small-K head kernels.
    What the same kernel computes from the same operands is asserted first (Ppre, Pl, dPl, and the clip loss's six outputs
    recomputed from the step's own frame logits); then every output, each figure printed before it is asserted."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    Cp, J = 768, 16
    g = torch.Generator().manual_seed(C + K)
    d = lambda t: t.to(gpu).contiguous()
    X = d(torch.relu(torch.randn(N_, P_, C, generator=g)).to(dtype))
    W1, b1 = d(torch.randn(C, Cp, generator=g) / C ** 0.5), d(torch.randn(Cp, generator=g) * 0.1)
    W2, b2 = d(torch.randn(Cp, J, generator=g) / Cp ** 0.5), d(torch.randn(J, generator=g) * 0.1)
    Wa, ba = d(torch.randn(Cp, 1, generator=g) / Cp ** 0.5), d(torch.randn(1, generator=g) * 0.1)
    Wt, bt = d(torch.randn(C, K, generator=g) / C ** 0.5), d(torch.randn(K, generator=g) * 0.1)
    labels = d(torch.randint(0, K, (N_ // F_,), generator=g))
    lbl, valid = d(torch.rand(N_, P_, J, generator=g)), d(torch.rand(N_, J, generator=g) > 0.3)
    tw, tb = (d(torch.randn(K, generator=g) * 0.3), d(torch.full((1,), 1.0 / F_))) if temporal else (None, None)
    flags = cof.attn_flags(False, False, True)
    kw = dict(flags=flags, keep_prob=0.5, seed=9, offset=7)
    wts = dict(action_wt=1.3, pose_wt=0.7, grad_scale=0.5)

    Ppre, Pl, pws = cof.pose_head_fwd(X, W1, b1, W2, b2)
    lossp, dPl = cof.pose_l2_loss_fwd_bwd(Pl, lbl, valid, wt=wts['pose_wt'], grad_scale=wts['grad_scale'])
    logits, att, zs, ab, _, ws = cof.attn_pool_fwd(X, Ppre, Wa, ba, Wt, bt, **kw)
    pooled, tatt, lossx, G, dw, db = cof.clip_xent_fwd_bwd(logits, labels, F_, tw, tb, wt=wts['action_wt'],
                                                           grad_scale=wts['grad_scale'])
    dX, dZ, dWa, dba, dWt, dbt = cof.attn_pool_bwd(X, Ppre, Wa, ba, Wt, bt, att, zs, ab, G, workspace=ws,
                                                   dxatt_rank1=True, **kw)
    dXf, dW1, db1, dW2, db2 = cof.pose_head_bwd(X, W1, W2, Ppre, dPl, None, dX=dX, accumulate_dX=True, workspace=pws,
                                                ext_rank1=(dZ, Wa.view(-1)))
    nan = lambda t: torch.full_like(t, float('nan'))
    prm = (W1, b1, W2, b2, Wa, ba, Wt, bt)
    grads = (nan(X),) + tuple(nan(t) for t in prm)
    tg = (nan(tw), nan(tb)) if temporal else None
    st = cof.PoseAttnTrainStep(X, prm, labels, lbl, valid, grads, frames=F_, temporal=(tw, tb) if temporal else None,
                               temporal_grads=tg, **kw, **wts)
    st.run()
    torch.cuda.synchronize()
    assert tuple(st.loss_action.shape) == (1 + N_ // F_,)
    # the same kernels on the same operands
    assert torch.equal(st.Ppre, Ppre) and torch.equal(st.Pl, Pl) and torch.equal(st.dPl.view_as(dPl), dPl)
    again = cof.clip_xent_fwd_bwd(st.logits, labels, F_, tw, tb, wt=wts['action_wt'], grad_scale=wts['grad_scale'])
    torch.cuda.synchronize()
    mine = (st.pooled, st.tatt, st.loss_action, st.G) + ((tg[0], tg[1]) if temporal else (None, None))
    for a_, b_ in zip(mine, again):
        assert (a_ is None and b_ is None) or torch.equal(a_.view_as(b_), b_)
    pairs = dict(att=(st.att, att), loss_pose=(st.loss_pose, lossp), logits=(st.logits, logits), zsave=(st.zsave, zs),
                 abar=(st.abar, ab), pooled=(st.pooled, pooled), loss=(st.loss_action, lossx), G=(st.G, G),
                 dZ=(st.dZ, dZ), dX=(grads[0], dXf), dW1=(grads[1], dW1), db1=(grads[2], db1), dW2=(grads[3], dW2),
                 db2=(grads[4], db2), dWa=(grads[5], dWa), dba=(grads[6], dba), dWt=(grads[7], dWt), dbt=(grads[8], dbt))
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
        _CACHE[name] = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_vstep_%s.npz' % name))
    return _CACHE[name]


def _load(fx, gpu):
    network_fn, cfg = rf.build_head(fx, device=gpu)
    table = rf.module_tf_names(network_fn)
    with torch.no_grad():
        for vn, t in table.items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).to(gpu))
    if network_fn.temporal is not None:
        network_fn.temporal._bias_initialised = True            # the fixture's value, not the 1/F initialiser
    network_fn.head.seed, network_fn.head._step = int(fx.meta['libmask'][0]), int(fx.meta['libmask'][1])
    return network_fn, cfg, table


def _bf16_logit_tol(exp_logits):
    return min(3e-3, 0.03 * float(np.abs(exp_logits).max()))          # test_reference_fixtures_gpu.py's figure


def _grad_floor(fx, vn):
    if fx.flag('_SOFTMAX_ATT') and 'Conv2d_PrePose_Attn' in vn and vn.endswith('biases'):
        return float(np.abs(fx.expected('grad/var/' + vn[:-len('biases')] + 'weights')).max())
    return 1e-30


def _fused_step_against_fixture(fx, gpu, bf, upstream=1.0):
    """-> (fused, optimiser, {param name: full gradient incl. weight decay}, params before); asserts total, Losses,
    every end point, images.grad and every trainable variable's gradient in the bucket"""
    from attentionalpoolingaction_amd import deploy
    network_fn, cfg, table = _load(fx, gpu)
    head = network_fn.head
    fused = deploy.FusedHeadStep(network_fn, cfg)
    opt = fused.make_optimizer(0.01)
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu).to(torch.bfloat16 if bf else torch.float32)
    assert images.dim() == 5
    B, F = images.shape[:2]
    images.requires_grad_(True)
    use_pose = bool(fx.meta['train_cfg']['LOSS_FN_POSE'])
    lp = torch.from_numpy(fx.arrays['in/labels_pose']).to(gpu) if use_pose else None
    lv = torch.from_numpy(fx.arrays['in/labels_pose_valid']).to(gpu) if use_pose else None
    if use_pose and B > 1:                  # labels_pose / pose_valid arrive folded or as [B,F,...]: give the 5-D form
        lp, lv = lp.view(B, F, *lp.shape[1:]), lv.view(B, F, -1)
    total, ep = fused(images, torch.from_numpy(fx.arrays['in/labels_action']).to(gpu), lp, lv)
    (upstream * total).backward()
    assert head._step == int(fx.meta['libmask'][1]) + 1
    tag = fx.name + (' bf16' if bf else ' fp32')
    exp_logits = fx.expected('out/logits').astype(np.float64)
    got_logits = ep['Logits'].float().cpu().numpy().astype(np.float64)
    assert got_logits.shape == (B, fx.meta['num_classes'])
    err = np.abs(got_logits - exp_logits).max()
    print('%s: logits max abs err %.3e (max |logit| %.3f)' % (tag, err, np.abs(exp_logits).max()))
    if bf:
        ltol = _bf16_logit_tol(exp_logits)
        assert err <= ltol
        top2 = np.sort(exp_logits, axis=1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) > 2 * ltol
        assert np.array_equal(got_logits.argmax(1)[sure], exp_logits.argmax(1)[sure])
    else:
        assert err <= 1e-3 and _rel(got_logits, exp_logits) < 2e-5
        assert np.array_equal(got_logits.argmax(1), exp_logits.argmax(1))
    tol, tolp = (1.2e-2, 8e-3) if bf else (5e-5, 5e-5)
    want_eps = {'Logits', 'logits_beforePool', 'PosePrelogitsBasedAttention', 'Losses'}
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
    assert tuple(ep['logits_beforePool'].shape) == (B * F, fx.meta['num_classes'])
    if 'TemporalAttention' in ep:
        assert tuple(ep['TemporalAttention'].shape) == (B, F, 1, 1)
    exp_losses = fx.expected('out/losses')
    assert len(ep['Losses']) == len(exp_losses)
    ltol_ = 2e-3 if bf else 2e-5
    for g_, e_ in zip(ep['Losses'], exp_losses):
        assert abs(float(g_) - e_) <= ltol_ * max(abs(e_), 1e-3)
    assert abs(float(total) - exp_losses.sum()) <= ltol_ * exp_losses.sum()
    assert images.grad.shape == images.shape
    fx.check('grad/images', images.grad.float().cpu().numpy() / upstream, tol, tag + ' grad/images', tol_proj=tolp)
    wd = fx.meta['weight_decay']
    before = {n: p.detach().clone() for n, p in fused.params.items()}
    names = dict(head.tf_variable_names(), **TEMPORAL_TF)
    grads = {}
    for n in fused._written:            # the regulariser's wd * w is the optimiser's: added here as the fixture has it
        full = fused.bucket.views[n].double().cpu().numpy() / upstream + \
            (wd * before[n].double().cpu().numpy() if n in fused.regularized else 0.0)
        fx.check('grad/var/' + names[n], full.reshape(fx.variables[names[n]].shape), tol, tag + ' ' + n, tol_proj=tolp,
                 floor=_grad_floor(fx, names[n]))
        grads[n] = full
    written_tf = {names[n] for n in fused._written}
    for vn in fx.meta['trainable']:     # every other trainable variable: regulariser only (the pruned pose convs)
        if vn not in written_tf:
            assert vn in fx.meta['reg_only_grad'] or float(np.abs(fx.expected('grad/var/' + vn)).max()) == 0.0, vn
    if network_fn.temporal is not None:
        assert {'temporal_weights', 'temporal_biases'} <= set(grads)
    return fused, opt, grads, before


@pytest.mark.parametrize('name', SMALL)
def test_fused_head_step_on_clips_matches_the_reference_fixture(gpu, name):
    """get_network_fn + deploy.FusedHeadStep on the fixture's [B,F,H,W,C] input with head.seed / _step from its
    libmask, then total.backward(): total, Losses, every end point, images.grad and every trainable variable's gradient
    in the bucket.  fp32 cases: logits 1e-3 absolute and 2e-5 relative, argmax exact, gradients 5e-5; the two bf16
    cases (quant='bf16' fixtures run with bf16 features): logits 3e-3, argmax on rows whose top-two margin exceeds
    twice that, gradients 1.2e-2 of max|reference|."""
    from attentionalpoolingaction_amd import config as apa_config
    fx = _fixture(name)
    try:
        _fused_step_against_fixture(fx, gpu, bf=fx.quant == 'bf16')
    finally:
        apa_config.reset_cfg()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', BIG)
def test_fused_head_step_on_clips_matches_the_reference_at_the_benchmark_shape(gpu, name, dtype):
    """8 clips x 4 frames x 14 x 14 x 2048, K = 51, temporal attention on, at fp32 and bf16 the same way (a non-unit
    upstream coefficient on top); then ONE update of the optimiser make_optimizer configures against
    w - lr * (fixture gradient), the TemporalAttention conv included."""
    from attentionalpoolingaction_amd import config as apa_config
    fx = _fixture('big_' + name)
    assert fx.quant == 'bf16'
    try:
        fused, opt, grads, before = _fused_step_against_fixture(fx, gpu, bf=dtype == 'bf16', upstream=2.0)
        lr, wd = 0.01, fx.meta['weight_decay']
        fused.bucket.flat.mul_(0.5)
        opt.step()
        assert {'temporal_weights', 'temporal_biases'} <= set(fused.params)
        for n, p_ in fused.params.items():
            g_ = grads.get(n)
            if g_ is None:                    # pruned from the data path (the single-layer form): the L2 term alone
                g_ = (wd if n in fused.regularized else 0.0) * before[n].double().cpu().numpy()
            want = before[n].double().cpu().numpy() - lr * g_
            assert np.abs(p_.detach().double().cpu().numpy() - want).max() <= 1e-6 * max(np.abs(want).max(), 1e-3), n
    finally:
        apa_config.reset_cfg()


def test_fused_head_step_on_clips_agrees_with_the_module_path(gpu):
    """temporal_att_train: network_fn + gen_losses + autograd (five launches and an autograd hop between the head and
    the loss) against FusedHeadStep, to fp32 round-off (2e-5): the pooled logits, the total, images.grad and every
    gradient the step writes."""
    from attentionalpoolingaction_amd import config as apa_config, deploy, loss as apa_loss
    fx = _fixture('temporal_att_train')
    try:
        labels = torch.from_numpy(fx.arrays['in/labels_action']).to(gpu)
        # module path
        network_fn, cfg, table = _load(fx, gpu)
        images = torch.from_numpy(fx.arrays['in/images']).to(gpu).requires_grad_(True)
        logits, ep = network_fn(images)
        tc = fx.meta['train_cfg']
        losses = apa_loss.gen_losses(labels, logits, tc['LOSS_FN_ACTION'], fx.meta['num_classes'],
                                     tc['LOSS_FN_ACTION_WT'], None, None, '', None, tc['LOSS_FN_POSE_WT'], ep, cfg)
        total = sum(losses)
        total.backward()
        # one call
        network_fn2, cfg2, table2 = _load(fx, gpu)
        fused = deploy.FusedHeadStep(network_fn2, cfg2)
        images2 = torch.from_numpy(fx.arrays['in/images']).to(gpu).requires_grad_(True)
        total2, ep2 = fused(images2, labels)
        total2.backward()
        torch.cuda.synchronize()
        n = lambda t: t.detach().float().cpu().numpy()
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
