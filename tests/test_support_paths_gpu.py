"""Every path of the loss, frame-pooling and optimiser kernels (csrc/apa_loss.hip, apa_loss2.hip, apa_framepool.hip,
apa_optim.hip) against float64, from the kernel's own inputs, through the custom_ops_factory wrappers.

Comparison (tests/_support_ref.py): per element, |got - ref| <= c * u * T + 1e-37 with u = 2^-24 and T the element's
magnitude of terms; c is the number of rounded fp32 operations that form the element, counted from the kernel source
and written next to each case, plus 2 u per ulp of a library function (HIP's published single-precision table:
expf 1 ulp, log1pf 1 ulp, sqrtf 1 ulp).  An n-term fp32 sum in any order gets n.  Bit-exact where the kernel performs
one IEEE operation per element (spatial mean, zero_out_channels, accumulation, bf16 shadows and images).  No
whole-array norm anywhere.

The optimisers are compared STEP BY STEP: each of the four steps is held to the float64 rule applied to the state the
kernel itself read (its fp32 weights and slots before the step), so c counts the operations of one launch and no
error of an earlier step enters the bound.

kernel                         edge                                              case
pose_l2_kernel                 split 1, P*J < 512                                test_pose_l2[3-9-16-*], [2-15-17-*]
                               split 1, N > 256                                  test_pose_l2[257-4-13-*]
                               split 8, chunk 366 does not divide 2925, J = 13   test_pose_l2[2-225-13-*], _sentinel[2-225-13]
                               split cut to 3 by the 256-per-share rule          test_pose_l2[4-49-16-*]
                               share start / end membership, idx % J             test_pose_l2_sentinel[*]
                               valid all / none / mix, dPl = NULL, wt, grad_scale test_pose_l2[*-all|none|mix]
sum_scale_kernel               280 partials > 256 threads                        test_pose_l2[40-225-16-*], _sentinel[40-225-16]
action_loss_kernel (3 kinds)   N*K = 3, 700 < 1024, = 1024, 1413, 38400          test_action_loss[*-1-3] .. [*-64-600]
                               |logit| up to 100 (softplus / sigmoid forms)      test_action_loss ('extreme' configurations)
                               labels all 0 / all 1, pos_weight 1 / 10 / 0.25    test_action_loss
                               flat index 0, 1023, 1024, N*K - 1                 test_action_loss_sentinel[*]
pose_sampled_kernel            N*P*J = 4, 975, 6272; J = 1, 13, 64; ratio 0 / 1  test_pose_sampled[*]
                               J = 65 refused                                    test_pose_sampled_refuses_j_65
resize_bilinear_tf1_kernel     identity, 1x1 source, grid-stride (> 2048 blocks) test_resize_bilinear[*]
fp_att / fp_pool / fp_bwd      K = 1, 63, 64, 65, 157, 256, 257, 600             test_frame_pool[K-*]
fp_bwd_w                       K = 256 / 257 / 600 (second and third block)      test_frame_pool[256|257|600-*]
                               rows % 4 = 0, 1, 2, 3                             test_frame_pool[*-4-2], [*-1-1], [*-2-25], [*-7-1]
                               F = 1 plain is the identity                       test_frame_pool[*-1-1], [*-7-1]
spatial_mean_bwd_kernel        fp32 / bf16 store, C = 4, 12, 2048                test_spatial_mean_bwd[*]
                               grid capped at 8192 blocks (8194 wanted)          test_spatial_mean_bwd[*-17-241-2048]
                               C % 4, misaligned dz                              test_spatial_mean_bwd_refusals
zero_out_channels_kernel       C = 1, 5, 2048; total > 4096 * 256; masks         test_zero_out_channels[*]
momentum_sgd_kernel<false>     vector body on unaligned offsets, scalar tail,    test_momentum_sgd[*]
                               n < 4 (tail only), bf16 shadow pairs + tail
momentum_sgd_kernel<true>      image scatter, c_shift 0 / 1 / 2, e != 0, tail    test_momentum_sgd_weight_images
adaptive_step_kernel<0>        eps 1 / 1e-6, v = 0, shadow                       test_adam[*]
adaptive_step_kernel<1>        momentum 0 / 0.9, ms from 1, g = 0, shadow        test_rmsprop[*]
accumulate_kernel<false/true>  parts 1, 2, 8, 9, 17; n = 1, 3, 4, 1027; aliasing test_accumulate_gradients[*]
"""
import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _support_ref as sr

pytestmark = pytest.mark.gpu


def f32(x):
    """the value a C float argument takes"""
    return float(np.float32(x))


WT, GS = f32(0.7), 3.0


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def _dev(a, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(gpu)


def _host(t):
    return t.detach().cpu().numpy()


def _randn(r, shape):
    return r.standard_normal(shape).astype(np.float32)


def _same_bits(a, b):
    """two device tensors of one dtype, bit for bit"""
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------------ pose L2
POSE_L2_SHAPES = [(3, 9, 16), (2, 15, 17), (257, 4, 13), (2, 225, 13), (4, 49, 16), (40, 225, 16)]


def _valid(r, kind, N, J):
    return {'all': np.ones((N, J), bool), 'none': np.zeros((N, J), bool), 'mix': r.random((N, J)) < 0.6}[kind]


@pytest.mark.parametrize('valid_kind', ['all', 'none', 'mix'])
@pytest.mark.parametrize('shape', POSE_L2_SHAPES, ids=lambda s: '%d-%d-%d' % s)
def test_pose_l2(gpu, shape, valid_kind):
    """loss: c = n + 5 with n = N P J terms in the sum: the difference squared (2), its fma (1), 0.5 wt / denom (1; N N P
    is exact) and the final product (1).  dPl: c = 4: grad_scale * wt (1), / denom (1), Pl - lbl (1), the product (1)."""
    N, P, J = shape
    r = _rng(11, N, P, J)
    Pl, lbl = _randn(r, shape), _randn(r, shape)
    valid = _valid(r, valid_kind, N, J)
    dPl_, dlbl, dvalid = _dev(Pl, gpu), _dev(lbl, gpu), _dev(valid, gpu)
    n = N * P * J
    first = None
    for wt, gs, want in ((1.0, 1.0, True), (WT, GS, True), (WT, 1.0, False), (1.0, 1.0, False)):
        loss, g = cof.pose_l2_loss_fwd_bwd(dPl_, dlbl, dvalid, wt=wt, grad_scale=gs, want_grad=want)
        rl, rg, T_l, T_g = sr.pose_l2(Pl, lbl, valid, wt, gs)
        sr.assert_close(_host(loss)[0], rl, T_l, n + 5, 'loss %s' % ((wt, gs, want),))
        if want:
            got = _host(g)
            sr.assert_close(got, rg, T_g, 4, 'dPl %s' % ((wt, gs),))
            assert (got[~np.broadcast_to(valid[:, None, :], shape)] == 0).all()      # exactly 0 where invalid
        else:
            assert g is None
        if wt == 1.0:                                   # the value does not depend on whether dPl is stored
            first = _host(loss)[0] if first is None else first
            assert _host(loss)[0] == first
    if valid_kind == 'none':
        assert first == 0.0


@pytest.mark.parametrize('shape', [(2, 225, 13), (40, 225, 16)], ids=lambda s: '%d-%d-%d' % s)
def test_pose_l2_sentinel(gpu, shape):
    """Pl - lbl is exactly 1 at ONE flat index and exactly 0 elsewhere: the sum is exactly 1, the loss the launcher's
    own scale 0.5 wt / denom and the gradient one element gcoef, both formed in fp32 as the launcher forms them.  The
    index walks the first / last element of the first, a middle and the last share.  2 ulp allowed; a dropped or
    double-counted boundary element is a factor 0 or 2."""
    N, P, J = shape
    PJ = P * J
    shares = sr.pose_l2_shares(N, P, J)
    assert len(shares) == {(2, 225, 13): 8, (40, 225, 16): 7}[shape]
    r = _rng(12, N, P, J)
    lbl = (r.integers(-64, 64, size=(N, PJ)) / 64.0).astype(np.float32)      # + 1 is exact
    dlbl, dvalid = _dev(lbl.reshape(shape), gpu), _dev(np.ones((N, J), bool), gpu)
    denom = np.float32(N) * np.float32(N) * np.float32(P)
    exp_loss = np.float32(0.5) * np.float32(WT) / denom
    exp_g = np.float32(GS) * np.float32(WT) / denom
    cases = set()
    for k, s in enumerate((0, len(shares) // 2, len(shares) - 1)):
        lo, hi = shares[s]
        assert lo < hi
        for idx in (0, lo - 1, lo, hi - 1, PJ - 1):
            if 0 <= idx < PJ:
                cases.add(((0, N // 2, N - 1)[k], idx))
    assert len(cases) >= 9
    for n, idx in sorted(cases):
        Pl = lbl.copy()
        Pl[n, idx] += np.float32(1.0)
        assert Pl[n, idx] - lbl[n, idx] == 1.0
        loss, g = cof.pose_l2_loss_fwd_bwd(_dev(Pl.reshape(shape), gpu), dlbl, dvalid, wt=WT, grad_scale=GS)
        got_l, got_g = _host(loss)[0], _host(g).reshape(N, PJ)
        assert sr.ulps_apart(got_l, exp_loss) <= 2, (n, idx, got_l, exp_loss)
        assert sr.ulps_apart(got_g[n, idx], exp_g) <= 2, (n, idx, got_g[n, idx], exp_g)
        got_g[n, idx] = 0.0
        assert (got_g == 0).all(), (n, idx, np.argwhere(got_g != 0)[:4])


# ------------------------------------------------------------------------------------------ action losses
ACTION_SHAPES = [(1, 3), (7, 100), (8, 128), (9, 157), (64, 600)]
EXTREME = np.array([0.0, 20.0, -20.0, 60.0, -60.0, 88.8, -88.8, 100.0, -100.0], np.float32)
# loss: n terms in the sum + the element + lscale (1 / NK, w * inv, the final product: 3)
#   l2             x - t (1), squared (1)  -> relative to (|x| + t)^2: 3                                   n + 6
#   multi-label    1 - t, * x (2); w: pw - 1, * t, 1 + (3); softplus: expf 1 ulp (2), carried through log1pf
#                  with condition <= 1, log1pf 1 ulp (2), + max (1); w * (1); the sum (1)  -> <= 11         n + 14
#   multi-label-2  x * t (1), max - (1), log1pf(expf) (4), + (1)                                           n + 10
C_LOSS = {'l2': 6, 'multi-label': 14, 'multi-label-2': 10}
# G: gscale = w * inv * grad_scale with inv = 1 / NK (3), the product with it (1), and
#   l2             x - t (1); 2 * is exact                                                                  5
#   multi-label    sigmoid: expf (2), 1 + (1), 1 / (1) = 4; 1 - sigmoid (1); w (3); w * (1); 1 - t (1); - (1)  15
#   multi-label-2  sigmoid (4), - t (1)                                                                      9
C_GRAD = {'l2': 5, 'multi-label': 15, 'multi-label-2': 9}


def _action_logits(r, N, K, mode):
    x = (2.5 * r.standard_normal((N, K))).astype(np.float32)
    if mode == 'extreme':
        pos = np.unique(np.linspace(0, N * K - 1, min(N * K, 2 * EXTREME.size)).astype(np.int64))
        vals = EXTREME if pos.size >= EXTREME.size else np.array([0.0, 88.8, -100.0], np.float32)
        x.reshape(-1)[pos] = np.resize(vals, pos.size)
    return x


def _action_labels(r, kind, N, K, mode):
    if kind == 'l2':
        return r.integers(0, K, N).astype(np.int64)
    return {'mix': (r.random((N, K)) < 0.3), 'zeros': np.zeros((N, K), bool), 'ones': np.ones((N, K), bool)}[
        mode].astype(np.float32)


def _check_action(gpu, kind, x, labels, wt, gs, pw, want=True, what=''):
    N, K = x.shape
    loss, G = cof.action_loss_fwd_bwd(kind, _dev(x, gpu), _dev(labels, gpu), wt=wt, grad_scale=gs, pos_weight=pw,
                                      want_grad=want)
    rl, rG, T_l, T_G = sr.action_loss(kind, x, labels, wt, gs, pw)
    assert np.isfinite(rl) and np.isfinite(rG).all()
    got_l = _host(loss)[0]
    assert np.isfinite(got_l), (what, got_l)
    sr.assert_close(got_l, rl, T_l, N * K + C_LOSS[kind], 'loss ' + what)
    if want:
        got = _host(G)
        assert np.isfinite(got).all(), what
        sr.assert_close(got, rG, T_G, C_GRAD[kind], 'G ' + what)
    else:
        assert G is None
    return got_l


@pytest.mark.parametrize('shape', ACTION_SHAPES, ids=lambda s: '%d-%d' % s)
@pytest.mark.parametrize('kind', ['l2', 'multi-label', 'multi-label-2'])
def test_action_loss(gpu, kind, shape):
    N, K = shape
    r = _rng(13, N, K)
    configs = [('random', 'mix', 10.0, 1.0, 1.0), ('extreme', 'mix', 10.0, 1.0, 1.0), ('extreme', 'zeros', 1.0, 1.0, 1.0),
               ('extreme', 'ones', 0.25, WT, GS), ('random', 'ones', 10.0, 1.0, 1.0), ('random', 'zeros', 0.25, WT, GS)]
    for lm, labm, pw, wt, gs in configs:
        x, labels = _action_logits(r, N, K, lm), _action_labels(r, kind, N, K, labm)
        what = '%s %s' % (kind, (lm, labm, pw, wt, gs))
        a = _check_action(gpu, kind, x, labels, wt, gs, pw, True, what)
        b = _check_action(gpu, kind, x, labels, wt, gs, pw, False, what + ' no G')
        assert a == b


@pytest.mark.parametrize('shape', [(9, 157), (64, 600)], ids=lambda s: '%d-%d' % s)
@pytest.mark.parametrize('kind', ['l2', 'multi-label', 'multi-label-2'])
def test_action_loss_sentinel(gpu, kind, shape):
    """logits 0 except -4.0 (the side where softplus(-x) keeps its linear term) at one flat index: the first and the
    last element of the first pass of the 1024-thread stride, the first of the second pass and the last of all"""
    N, K = shape
    r = _rng(14, N, K)
    labels = _action_labels(r, kind, N, K, 'mix')
    for idx in (0, 1023, 1024, N * K - 1):
        x = np.zeros((N, K), np.float32)
        x.reshape(-1)[idx] = -4.0
        _check_action(gpu, kind, x, labels, 1.0, 1.0, 10.0, True, '%s sentinel %d' % (kind, idx))


# ------------------------------------------------------------------------------------------ sampled pose loss
def _sampled_inputs(shape):
    N, P, J = shape
    r = _rng(15, N, P, J)
    Pl = _randn(r, shape)
    lbl = np.maximum(_randn(r, shape), np.float32(0))            # about half exactly 0
    if J >= 3:
        lbl[..., 1] = 0.0                                        # no positives: ratio 0
        lbl[..., 2] = np.abs(lbl[..., 2]) + np.float32(0.5)      # all positives: ratio 1
    else:
        lbl.reshape(-1)[:] = [0.0, 0.5, 0.0, 0.0][:lbl.size]
    u = r.random(shape).astype(np.float32)
    ratio = sr.pose_sampled_ratio(lbl)
    # the kernel compares u with ratio in fp32, the reference in float64: keep every draw further from its ratio than
    # any rounding of it (a condition on the inputs; the offending draws are replaced, not left out)
    near = np.abs(u.astype(np.float64) - ratio) <= 1e-6
    repl = np.where(ratio < 0.5, ratio + 0.25, ratio - 0.25).astype(np.float32)
    u = np.where(near, np.broadcast_to(repl, shape), u)
    assert (np.abs(u.astype(np.float64) - ratio) > 1e-6).all() and (u >= 0).all() and (u < 1).all()
    valid = r.random((N, J)) < 0.7
    valid[0, :] = True
    return Pl, lbl, u, valid, ratio


@pytest.mark.parametrize('shape', [(1, 4, 1), (3, 25, 13), (2, 49, 64)], ids=lambda s: '%d-%d-%d' % s)
def test_pose_sampled(gpu, shape):
    """mask: exact.  loss: c = n + 6: a m - b m (1; the products are exact), its square (2 with the fma), lscale (0.5 wt
    exact, / (N P): 1) and the final product (1), + 1 spare for wt != 1.  dPl: c = 4 as for the plain pose loss."""
    N, P, J = shape
    Pl, lbl, u, valid, ratio = _sampled_inputs(shape)
    if J >= 3:
        assert ratio[1] == 0.0 and ratio[2] == 1.0
    d = [_dev(a, gpu) for a in (Pl, lbl, valid, u)]
    n = N * P * J
    for wt, gs, want in ((1.0, 1.0, True), (WT, GS, True), (WT, GS, False)):
        loss, g, mask = cof.pose_sampled_loss_fwd_bwd(*d, wt=wt, grad_scale=gs, want_grad=want)
        rl, rg, rmask, T_l, T_g = sr.pose_sampled(Pl, lbl, valid, u, wt, gs)
        assert (_host(mask) == rmask).all()
        sr.assert_close(_host(loss)[0], rl, T_l, n + 6, 'loss')
        if want:
            got = _host(g)
            sr.assert_close(got, rg, T_g, 4, 'dPl')
            assert (got[~np.broadcast_to(valid[:, None, :], shape)] == 0).all()
        else:
            assert g is None
    if J >= 3:                                                    # ratio 0 selects nothing, ratio 1 has no negatives
        m = _host(mask)
        assert (m[..., 1] == (Pl[..., 1] > 0)).all() and (m[..., 2] == (Pl[..., 2] > 0)).all()


def test_pose_sampled_refuses_j_65(gpu):
    z = torch.zeros((2, 4, 65), device=gpu)
    with pytest.raises(cof.ApaError, match='J=65 > 64'):
        cof.pose_sampled_loss_fwd_bwd(z, z, torch.ones((2, 65), dtype=torch.bool, device=gpu), z)


# ------------------------------------------------------------------------------------------ label resize
@pytest.mark.parametrize('case', [((2, 7, 9, 3), (7, 9)), ((1, 1, 1, 5), (4, 6)), ((2, 8, 8, 64), (66, 65))],
                         ids=['identity', 'one-pixel', 'grid-stride'])
def test_resize_bilinear(gpu, case):
    shape, (oh, ow) = case
    img = _rng(16, *shape).random(shape).astype(np.float32)
    got = cof.resize_bilinear_tf1(_dev(img, gpu), oh, ow)
    if (oh, ow) == shape[1:3]:
        assert _same_bits(got, _dev(img, gpu))
    if case[1] == (66, 65):
        assert got.numel() > 2048 * 256
    ref = sr.resize_bilinear(img, oh, ow)
    assert got.shape == ref.shape
    assert np.abs(_host(got).astype(np.float64) - ref).max() <= 2e-6
    if shape[1:3] == (1, 1):
        assert (_host(got) == img.reshape(1, 1, 1, -1)).all()


# ------------------------------------------------------------------------------------------ frame pooling
@pytest.mark.parametrize('BF', [(1, 1), (1, 5), (2, 25), (3, 3), (4, 2), (7, 1)], ids=lambda s: '%d-%d' % s)
@pytest.mark.parametrize('K', [1, 63, 64, 65, 157, 256, 257, 600])
def test_frame_pool(gpu, K, BF):
    """tatt: K fma terms + b0: c = K + 1.  pooled: F fma terms, 1 / F (1), the product (1): c = F + 2, and in temporal
    mode the error of tatt rides on every term: c = (K + 1) + F + 2.  Backward, fed the fp32 rounding of the float64 tatt
    (the reference reads the same numbers): dLda = K terms, 1 / F, product: K + 2;  dx = fma(g / F, a, dLda w):
    (K + 2) + d w (1) + g / F (2) + fma (1) = K + 6, plain g * (1 / F) = 2;  dw, db: `rows` terms of dLda: rows + K + 2."""
    B, F = BF
    rows = B * F
    r = _rng(17, K, B, F)
    x, g = _randn(r, (rows, K)), _randn(r, (B, K))
    w, b0 = _randn(r, (K,)), np.float32(1.0 / F)
    dx_, dg = _dev(x, gpu), _dev(g, gpu)
    # plain
    pooled, tatt = cof.frame_pool_fwd(dx_, F)
    assert tatt is None
    rp, _, T_p, _ = sr.frame_pool_fwd(x, F)
    sr.assert_close(_host(pooled), rp, T_p, F + 2, 'pooled plain')
    dx, dw, db = cof.frame_pool_bwd(dx_, F, None, None, dg)
    assert dw is None and db is None
    out, mag = sr.frame_pool_bwd(x, F, None, None, g)
    sr.assert_close(_host(dx), out['dx'], mag['dx'], 2, 'dx plain')
    if F == 1:
        assert _same_bits(pooled, dx_) and _same_bits(dx, dg)
    # temporal
    dw_, db_ = _dev(w, gpu), _dev(np.array([b0]), gpu)
    pooled, tatt = cof.frame_pool_fwd(dx_, F, dw_, db_)
    rp, ra, T_p, T_a = sr.frame_pool_fwd(x, F, w, b0)
    sr.assert_close(_host(tatt), ra, T_a, K + 1, 'tatt')
    sr.assert_close(_host(pooled), rp, T_p, K + F + 3, 'pooled temporal')
    a32 = ra.astype(np.float32)
    dx, dw, db = cof.frame_pool_bwd(dx_, F, dw_, _dev(a32, gpu), dg)
    out, mag = sr.frame_pool_bwd(x, F, w, a32, g)
    sr.assert_close(_host(dx), out['dx'], mag['dx'], K + 6, 'dx temporal')
    sr.assert_close(_host(dw), out['dw'], mag['dw'], rows + K + 2, 'dw')
    sr.assert_close(_host(db), out['db'], mag['db'], rows + K + 2, 'db')


# ------------------------------------------------------------------------------------------ spatial-mean backward
# (5, 225, 2048) is 2304000 ELEMENTS but 576000 float4 groups (2250 blocks): it stays as a plain large case.  The grid cap
# is in float4 groups: (17, 241, 2048) has 4097 * 512 = 2097664 > 8192 * 256 of them (8194 blocks wanted), the smallest
# such count with C = 2048 and N > 1.
@pytest.mark.parametrize('shape', [(1, 1, 4), (3, 49, 12), (2, 225, 2048), (5, 225, 2048), (17, 241, 2048)],
                         ids=lambda s: '%d-%d-%d' % s)
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_spatial_mean_bwd(gpu, dtype, shape):
    """fp32: dz * (1 / P), both in fp32, bit for bit; bf16: its round-to-nearest-even.  The expectation is formed on the
    host per (n, c) and only broadcast over p on the device."""
    N, P, C = shape
    if shape == (17, 241, 2048):
        assert (N * P * (C // 4) + 255) // 256 > 8192
    dz = _randn(_rng(18, N, P, C), (N, C))
    row = dz * (np.float32(1.0) / np.float32(P))
    assert row.dtype == np.float32
    sr.assert_close(row, sr.spatial_mean_bwd(dz, P)[:, 0, :], np.abs(dz) / P, 2, 'fp32 expectation')   # 1 / P, product
    got = cof.spatial_mean_bwd(_dev(dz, gpu), (N, P, C), dtype)
    assert got.dtype == dtype and tuple(got.shape) == shape
    exp = _dev(row, gpu, dtype).unsqueeze(1).expand(N, P, C)       # the host's conversion rounds to nearest even
    assert _same_bits(got, exp.contiguous())


def test_spatial_mean_bwd_refusals(gpu):
    with pytest.raises(cof.ApaError, match='multiple of 4'):
        cof.spatial_mean_bwd(torch.zeros((2, 6), device=gpu), (2, 3, 6), torch.float32)
    buf = torch.zeros(2 * 8 + 4, device=gpu)
    for dt in (torch.float32, torch.bfloat16):
        with pytest.raises(cof.ApaError, match='16-byte aligned'):
            cof.spatial_mean_bwd(buf[1:17].view(2, 8), (2, 3, 8), dt)


# ------------------------------------------------------------------------------------------ zero_out_channels
@pytest.mark.parametrize('mask', ['none', 'all', 'random'])
@pytest.mark.parametrize('C', [1, 5, 2048])
def test_zero_out_channels(gpu, C, mask):
    outer = 4096 * 256 // C + 3                                   # total > 4096 * 256: the grid-stride loop runs twice
    assert outer * C > 4096 * 256
    r = _rng(19, C)
    x = _randn(r, (outer, C))
    x.reshape(-1)[::7] = np.float32(-0.0)                         # negative zeros pass through a kept channel as they are
    ch = {'none': np.zeros(C, bool), 'all': np.ones(C, bool), 'random': r.random(C) < 0.5}[mask]
    if mask == 'random' and C > 1:
        ch[0], ch[-1] = True, False
    got = cof.zero_out_channels(_dev(x, gpu), _dev(ch, gpu))
    exp = np.where(ch, x, np.float32(0.0))
    assert exp.dtype == np.float32 and (exp == sr.zero_out_channels(x, ch)).all()
    assert _same_bits(got, _dev(exp, gpu))


# ------------------------------------------------------------------------------------------ optimisers
SIZES = [1, 3, 4, 5, 1024, 1031, 1023, 2048 * 51]                  # flat offsets 0, 1, 4, 8, 13, 1037, 2068, 3091
OFFS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
WD = [f32(v) for v in (0.0, 5e-4, 0.0, 5e-4, 5e-4, 5e-4, 0.0, 5e-4)]
ZERO_GRAD_SEG = 6                                                 # the 1023-element segment: no gradient, no decay
SHADOW_SEGS = (3, 5)                                              # sizes 5 and 1031
LRS = [f32(v) for v in (0.1, 0.05, 0.2, 0.01)]


class _Params:
    """weights as views of one flat device buffer at the bucket's own offsets (so they are as unaligned as the bucket),
    the gradient bucket and `nslots` slot buffers"""

    def __init__(self, gpu, seed, sizes=SIZES, slots=(0.0,), shadows=SHADOW_SEGS):
        self.sizes = list(sizes)
        self.offs = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.total = int(self.offs[-1])
        self.r = _rng(20, seed)
        self.wflat = _dev(_randn(self.r, (self.total,)), gpu)
        self.weights = [self.wflat[self.offs[i]:self.offs[i + 1]] for i in range(len(self.sizes))]
        self.grad = torch.zeros(self.total, device=gpu)
        self.slots = [torch.full((self.total,), v, device=gpu) for v in slots]
        self.shadows = [torch.zeros(s, dtype=torch.bfloat16, device=gpu) if i in shadows else None
                        for i, s in enumerate(self.sizes)]
        self.gpu = gpu

    def per_element(self, per_segment):
        return np.repeat(np.asarray(per_segment, np.float64), self.sizes)

    def draw_grad(self, zero_seg=None):
        g = _randn(self.r, (self.total,))
        if zero_seg is not None:
            g[self.offs[zero_seg]:self.offs[zero_seg + 1]] = 0.0
        self.grad.copy_(_dev(g, self.gpu))
        return g

    def state(self):
        return [_host(self.wflat).copy()] + [_host(s).copy() for s in self.slots]

    def check_shadows(self):
        for w, s in zip(self.weights, self.shadows):
            if s is not None:
                assert _same_bits(s, w.to(torch.bfloat16))


def test_offsets_are_unaligned():
    assert list(OFFS[:5]) == [0, 1, 4, 8, 13] and [int(o) % 4 for o in OFFS[4:8]] == [1, 1, 0, 3]


@pytest.mark.parametrize('decay', ['wd', 'no-wd'])
def test_momentum_sgd(gpu, decay):
    """acc: g * gs (1), fma(wd, w, .) (1), fma(m, acc, .) (1): c = 3.  w = fma(-lr, acc', w): c = 4 against
    T = |w| + lr T_acc (the accumulator's 3 ride on lr T_acc, the fma adds 1)."""
    wd = WD if decay == 'wd' else [0.0] * len(SIZES)
    p = _Params(gpu, 1)
    opt = cof.BoundMomentumSGD(p.weights, wd, p.grad, p.slots[0], shadows=p.shadows)
    m, gs = f32(0.9), 0.5
    for lr in LRS:
        g = p.draw_grad(ZERO_GRAD_SEG)
        w0, a0 = p.state()
        opt.run(lr, m, gs)
        w1, a1 = p.state()
        rw, ra, T_w, T_a = sr.momentum_sgd(w0, a0, g, lr, m, p.per_element(wd), gs)
        sr.assert_close(a1, ra, T_a, 3, 'acc lr=%g' % lr)
        sr.assert_close(w1, rw, T_w, 4, 'w lr=%g' % lr)
        p.check_shadows()
    for i, s in enumerate(p.shadows):                             # the other segments have none; theirs moved
        if s is not None:
            assert bool((s != 0).any())


def test_momentum_refuses_a_shadow_on_a_2_byte_boundary(gpu):
    w = torch.zeros(5, device=gpu)
    buf = torch.zeros(8, dtype=torch.bfloat16, device=gpu)
    opt = cof.BoundMomentumSGD([w], [0.0], torch.ones(5, device=gpu), torch.zeros(5, device=gpu), shadows=[buf[1:6]])
    with pytest.raises(cof.ApaError, match='4-byte aligned'):
        opt.run(0.1)
    torch.cuda.synchronize()
    assert bool((w == 0).all()) and bool((buf == 0).all())


@pytest.mark.parametrize('eps', [1.0, 1e-6])
def test_adam(gpu, eps):
    """g' = fma(wd, w, g * gs): 2.  m: g' (2), g' - m (1), 1 - b1 (1), product (1), sum (1): c = 6.  v: g'^2 (2 * 2 + 1),
    - v, 1 - b2, product, sum: c = 9.  w: the terms |w| (1), lr_t T_m / D (6) and |upd| (1 + T_v / v') with D = sqrt(v') + eps:
    m * lr (1), sqrtf 1 ulp (2) and half the relative error of v' (4.5 T_v / v'), + eps (1), the division (1), w - (1):
    no coefficient above 6.5; c = 10 leaves the second-order terms room."""
    p = _Params(gpu, 2, slots=(0.0, 0.0))
    b1, b2, e = f32(0.9), f32(0.999), f32(eps)
    wdv = p.per_element(WD)
    for t, lr in enumerate(LRS, 1):
        g = p.draw_grad(ZERO_GRAD_SEG)
        w0, m0, v0 = p.state()
        cof.adam_step(p.weights, WD, p.grad, p.slots[0], p.slots[1], lr, t, epsilon=eps, grad_scale=0.5,
                      shadows=p.shadows)
        w1, m1, v1 = p.state()
        lr_t = f32(sr.adam_lr_t(lr, t, 0.9, 0.999))              # formed in double by the wrapper, passed as a float
        rw, rm, rv, T_w, T_m, T_v = sr.adam(w0, m0, v0, g, lr_t, b1, b2, e, wdv, 0.5)
        sr.assert_close(m1, rm, T_m, 6, 'm t=%d' % t)
        sr.assert_close(v1, rv, T_v, 9, 'v t=%d' % t)
        sr.assert_close(w1, rw, T_w, 10, 'w t=%d' % t)
        z = slice(int(OFFS[ZERO_GRAD_SEG]), int(OFFS[ZERO_GRAD_SEG + 1]))      # v = 0: 0 / (0 + eps), nothing moves
        assert (v1[z] == 0).all() and (m1[z] == 0).all() and (w1[z] == w0[z]).all()
        p.check_shadows()


@pytest.mark.parametrize('momentum,eps', [(0.0, 1.0), (0.9, 1e-10)], ids=['mom0-eps1', 'mom0.9-eps1e-10'])
def test_rmsprop(gpu, momentum, eps):
    """ms: as Adam's v: c = 9.  mom = mom * momentum + (g' * lr) / sqrtf(ms' + eps): g' (2), * lr (1), + eps (1), sqrtf 1 ulp
    (2) and half the relative error of ms' + eps (4.5 T_ms / S), the division (1), mom * momentum (1), the sum (1): c = 8
    against T = |momentum mom| + lr T_g / sqrt(S) (1 + T_ms / S).  w = w - mom': c = 9 against |w| + T_mom."""
    ms0, mom0 = sr.rmsprop_slots(1)
    p = _Params(gpu, 3, slots=(float(ms0[0]), float(mom0[0])))
    assert (float(ms0[0]), float(mom0[0])) == (1.0, 0.0)
    rho, mo, e = f32(0.9), f32(momentum), f32(eps)
    wdv = p.per_element(WD)
    for step, lr in enumerate(LRS):
        g = p.draw_grad(ZERO_GRAD_SEG)
        w0, s0, q0 = p.state()
        cof.rmsprop_step(p.weights, WD, p.grad, p.slots[0], p.slots[1], lr, decay=0.9, momentum=momentum, epsilon=eps,
                         grad_scale=0.5, shadows=p.shadows)
        w1, s1, q1 = p.state()
        rw, rs, rq, T_w, T_s, T_q = sr.rmsprop(w0, s0, q0, g, lr, rho, mo, e, wdv, 0.5)
        sr.assert_close(s1, rs, T_s, 9, 'ms step %d' % step)
        sr.assert_close(q1, rq, T_q, 8, 'mom step %d' % step)
        sr.assert_close(w1, rw, T_w, 9, 'w step %d' % step)
        z = slice(int(OFFS[ZERO_GRAD_SEG]), int(OFFS[ZERO_GRAD_SEG + 1]))      # g = 0: ms decays from 1, nothing moves
        assert (q1[z] == 0).all() and (w1[z] == w0[z]).all() and (s1[z] < s0[z]).all() and (s1[z] > 0.6).all()
        p.check_shadows()


def _wimg(dst, is_f32, cols, sh, a, b, d, e):
    m = cof.ApaWeightImage()
    m.dst, m.role, m.is_f32, m.cols, m.c_shift, m.a, m.b, m.d, m.e = dst.data_ptr(), 0, int(is_f32), cols, sh, a, b, d, e
    return m


IMG_FILL = 1536.0                                                 # a bf16 number
#            segment  dtype           size  cols sh a  b  d   e
IMAGES = [(1, torch.float32, 80, 5, 0, 1, 0, 16, 0),               # fp32, c_shift 0: the transpose into [5, 16]
          (1, torch.bfloat16, 72, 5, 2, 1, 3, 13, 0),             # bf16, c_shift 2, interleaved: low bits stride 3, high 1
          (1, torch.bfloat16, 72, 5, 0, 5, 0, 1, 7),              # e != 0: the segment as it lies, 7 elements in
          (2, torch.bfloat16, 32, 3, 1, 2, 1, 9, 2)]              # a 7 x 3 segment (21 = 5 vectors + a scalar tail)


def test_momentum_sgd_weight_images(gpu):
    """apa_momentum_sgd_step_images: after each step every image equals the scatter of the updated weights through
    (c >> sh) a + (c & mask) b + k d + e (fp32 as is, bf16 rounded to nearest even), and the elements the map does not
    name keep their prefill.  The update itself: c = 3 / 4 as in test_momentum_sgd."""
    sizes = [3, 12 * 5, 7 * 3]
    wd = [0.0, f32(5e-4), f32(5e-4)]
    p = _Params(gpu, 4, sizes=sizes, shadows=(2,))
    dsts = [torch.full((n,), IMG_FILL, dtype=dt, device=gpu) for _, dt, n, *_ in IMAGES]
    images = [(seg, _wimg(dst, dt == torch.float32, *m)) for dst, (seg, dt, n, *m) in zip(dsts, IMAGES)]
    opt = cof.BoundMomentumSGD(p.weights, wd, p.grad, p.slots[0], shadows=p.shadows, images=images)
    m_ = f32(0.9)
    for lr in LRS[:2]:
        g = p.draw_grad()
        w0, a0 = p.state()
        opt.run(lr, m_, 0.5)
        w1, a1 = p.state()
        rw, ra, T_w, T_a = sr.momentum_sgd(w0, a0, g, lr, m_, p.per_element(wd), 0.5)
        sr.assert_close(a1, ra, T_a, 3, 'acc')
        sr.assert_close(w1, rw, T_w, 4, 'w')
        p.check_shadows()
        for dst, (seg, dt, n, cols, sh, a, b, d, e) in zip(dsts, IMAGES):
            wseg = w1[p.offs[seg]:p.offs[seg + 1]]
            exp = sr.image_scatter(wseg, cols, sh, a, b, d, e, n, IMG_FILL)
            assert (exp != IMG_FILL).sum() == wseg.size
            assert _same_bits(dst, _dev(exp.astype(np.float32), gpu, dt)), (seg, dt, sh, e)


def test_weight_image_refusals(gpu):
    p = _Params(gpu, 5, sizes=[3, 60], shadows=())
    dst = torch.zeros(96, device=gpu)
    ok = (1, _wimg(dst, True, 5, 0, 1, 0, 16, 0))

    def run(weights, wd, grad, acc, images):
        cof.BoundMomentumSGD(weights, wd, grad, acc, images=images).run(0.1)

    for images in ([ok] * 4, [(1, _wimg(dst, True, 7, 0, 1, 0, 16, 0))]):
        with pytest.raises(cof.ApaError, match='bad weight image'):
            run(p.weights, [0.0, 0.0], p.grad, p.slots[0], images)
    w17 = torch.zeros(17 * 4, device=gpu)
    with pytest.raises(cof.ApaError, match='nseg=17, max 16'):
        run([w17[4 * i:4 * i + 4] for i in range(17)], [0.0] * 17, torch.zeros(68, device=gpu),
            torch.zeros(68, device=gpu), [(0, _wimg(dst, True, 4, 0, 1, 0, 16, 0))])
    torch.cuda.synchronize()
    assert bool((dst == 0).all()) and bool((p.slots[0] == 0).all())


@pytest.mark.parametrize('n', [1, 3, 4, 1027])
@pytest.mark.parametrize('nparts', [1, 2, 8, 9, 17])
def test_accumulate_gradients(gpu, nparts, n):
    """the fp32 sum in the stated order, then ONE IEEE division by 3 or product with fl(1/3): bit for bit (more than 8
    parts fold through `out` with scale 1, which changes no bit); `out` may be parts[0]."""
    r = _rng(21, nparts, n)
    parts = [_randn(r, (n,)) for _ in range(nparts)]
    third = f32(1.0 / 3.0)
    for kw, exp in ((dict(divisor=3.0), sr.accumulate_f32(parts, divisor=3.0)),
                    (dict(scale=third), sr.accumulate_f32(parts, scale=third))):
        assert exp.dtype == np.float32
        ref, T = sr.accumulate(parts, **kw)
        sr.assert_close(exp, ref, T, nparts + 1, 'the fp32 expectation')
        dparts = [_dev(q, gpu) for q in parts]
        out = torch.full((n,), float('nan'), device=gpu)
        cof.accumulate_gradients(out, dparts, **kw)
        assert _same_bits(out, _dev(exp, gpu)), kw
        for q, d in zip(parts, dparts):
            assert _same_bits(d, _dev(q, gpu))                    # the parts are only read
        cof.accumulate_gradients(dparts[0], dparts, **kw)         # out aliases parts[0]
        assert _same_bits(dparts[0], _dev(exp, gpu)), ('alias', kw)
