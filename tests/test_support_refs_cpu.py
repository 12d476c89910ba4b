"""The float64 restatements of tests/_support_ref.py held to something independent, on the CPU: the optimiser rules
to torch.optim in float64 and to hand-stepped scalar cases where TF 1.1 differs from torch, the loss gradients to
torch autograd through the oracle, the frame-pooling backward to autograd, the weight-image map to a double loop --
and the refusals of the support entry points that return before any launch (the library loads without a GPU; the
operand addresses are fakes that nothing dereferences)."""
import ctypes

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from oracle import attn_pool_oracle as orc
from tests import _support_ref as sr

INVALID, UNSUPPORTED = -1, -2
D = torch.float64


def _rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------ optimiser rules
def test_momentum_rule_is_torch_sgd_in_float64():
    """torch.optim.SGD(momentum, weight_decay), dampening 0: buf = m buf + (g + wd w); w -= lr buf -- the same rule;
    lr changes between the steps."""
    r = _rng(1)
    w0 = r.standard_normal(37)
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.SGD([p], lr=0.1, momentum=0.9, weight_decay=5e-4)
    w, acc = w0.copy(), np.zeros(37)
    for lr in (0.1, 0.05, 0.2, 0.01):
        g = r.standard_normal(37)
        for grp in opt.param_groups:
            grp['lr'] = lr
        p.grad = torch.from_numpy(0.5 * g)                     # grad_scale = 0.5 applied by hand on torch's side
        opt.step()
        w, acc, T_w, T_a = sr.momentum_sgd(w, acc, g, lr, 0.9, np.full(37, 5e-4), grad_scale=0.5)
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=0, atol=1e-14)
        assert (T_w >= np.abs(w) - 1e-15).all() and (T_a >= np.abs(acc) - 1e-15).all()
    # no decay where the segment carries none
    w2, a2, _, _ = sr.momentum_sgd(w0, np.zeros(37), np.ones(37), 0.1, 0.9, np.zeros(37))
    np.testing.assert_allclose(w2, w0 - 0.1, rtol=0, atol=1e-15)
    np.testing.assert_allclose(a2, 1.0, rtol=0, atol=0)


def test_adam_rule_is_torch_adam_where_epsilon_vanishes():
    """torch: w -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) = TF's lr_t m / (sqrt(v) + eps sqrt(1 - b2^t)):
    the two agree exactly at eps = 0 (every v > 0 here)."""
    r = _rng(2)
    w0 = r.standard_normal(29)
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=0.0, weight_decay=5e-4)
    w, m, v = w0.copy(), np.zeros(29), np.zeros(29)
    for t in range(1, 5):
        g = r.standard_normal(29)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        w, m, v, T_w, _, _ = sr.adam(w, m, v, g, sr.adam_lr_t(1e-2, t), 0.9, 0.999, 0.0, np.full(29, 5e-4))
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=0, atol=1e-13)
        assert (T_w >= np.abs(w) - 1e-15).all()


def test_adam_epsilon_is_outside_the_root_hand_stepped():
    """one scalar by hand: w = 1, g = 3, b1 = 0.9, b2 = 0.999, eps = 1, lr = 0.1, t = 1:
    m = 0.3, v = 0.009, lr_t = 0.1 sqrt(0.001) / 0.1 = sqrt(0.001); w' = 1 - lr_t 0.3 / (sqrt(0.009) + 1)."""
    lr_t = sr.adam_lr_t(0.1, 1)
    assert abs(lr_t - 0.001 ** 0.5) < 1e-15
    w, m, v, _, _, _ = sr.adam([1.0], [0.0], [0.0], [3.0], lr_t, 0.9, 0.999, 1.0, [0.0])
    assert abs(m[0] - 0.3) < 1e-15 and abs(v[0] - 0.009) < 1e-15
    assert abs(w[0] - (1.0 - 0.001 ** 0.5 * 0.3 / (0.009 ** 0.5 + 1.0))) < 1e-15
    # inside the root it would be 1 - lr_t 0.3 / sqrt(1.009): a different number
    assert abs(w[0] - (1.0 - 0.001 ** 0.5 * 0.3 / (1.009 ** 0.5))) > 1e-4
    # v = 0 and g = 0: the step is 0 / (0 + eps), the weight stays
    w, m, v, T_w, _, _ = sr.adam([2.0], [0.0], [0.0], [0.0], lr_t, 0.9, 0.999, 1e-6, [0.0])
    assert (w[0], m[0], v[0], T_w[0]) == (2.0, 0.0, 0.0, 2.0)
    # the L2 term is part of the gradient: g' = 0.5 * 4 + 0.25 * 2 = 2.5
    _, m, _, _, _, _ = sr.adam([2.0], [0.0], [0.0], [4.0], lr_t, 0.9, 0.999, 1.0, [0.25], grad_scale=0.5)
    assert abs(m[0] - 0.25) < 1e-15


def test_rmsprop_rule_is_torch_rmsprop_where_epsilon_vanishes():
    """torch: sq = a sq + (1 - a) g^2; buf = mom buf + g / (sqrt(sq) + eps); w -= lr buf.  At eps = 0, a constant lr and
    `sq` started at ONE (torch starts at 0: its state is set by hand) TF's mom is lr * buf and the weights agree."""
    r = _rng(3)
    for momentum in (0.0, 0.9):
        w0 = r.standard_normal(23)
        p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
        opt = torch.optim.RMSprop([p], lr=1e-2, alpha=0.9, eps=0.0, momentum=momentum, weight_decay=5e-4)
        w = w0.copy()
        ms, mom = sr.rmsprop_slots(23)
        for step in range(4):
            g = r.standard_normal(23)
            p.grad = torch.from_numpy(g.copy())
            opt.step()
            if step == 0:
                # torch has now created its state from sq = 0: overwrite state and weights with the first step taken
                # from sq = 1, by hand; the later steps are torch's own
                st = opt.state[p]
                sq1 = 0.9 * 1.0 + 0.1 * (g + 5e-4 * w0) ** 2
                st['square_avg'].copy_(torch.from_numpy(sq1))
                buf = (g + 5e-4 * w0) / np.sqrt(sq1)
                if momentum > 0:
                    st['momentum_buffer'].copy_(torch.from_numpy(buf))
                with torch.no_grad():
                    p.copy_(torch.from_numpy(w0 - 1e-2 * buf))
            w, ms, mom, T_w, _, _ = sr.rmsprop(w, ms, mom, g, 1e-2, 0.9, momentum, 0.0, np.full(23, 5e-4))
            np.testing.assert_allclose(w, p.detach().numpy(), rtol=0, atol=1e-13)
            np.testing.assert_allclose(ms, opt.state[p]['square_avg'].numpy(), rtol=0, atol=1e-14)
            assert (T_w >= np.abs(w) - 1e-15).all()


def test_rmsprop_slots_and_epsilon_hand_stepped():
    """w = 1, g = 2, rho = 0.9, lr = 0.1, momentum = 0.5, eps = 1, ms = 1, mom = 0:
    ms' = 1 + (4 - 1) 0.1 = 1.3; mom' = 0.1 * 2 / sqrt(1.3 + 1); w' = 1 - mom'.  Second step with g = 0:
    ms'' = 1.3 * 0.9; mom'' = 0.5 mom'."""
    ms, mom = sr.rmsprop_slots(1)
    assert (ms[0], mom[0]) == (1.0, 0.0)
    w, ms, mom, _, _, _ = sr.rmsprop([1.0], ms, mom, [2.0], 0.1, 0.9, 0.5, 1.0, [0.0])
    assert abs(ms[0] - 1.3) < 1e-15 and abs(mom[0] - 0.2 / 2.3 ** 0.5) < 1e-15 and abs(w[0] - (1 - 0.2 / 2.3 ** 0.5)) < 1e-15
    assert abs(mom[0] - 0.2 / (1.3 ** 0.5 + 1.0)) > 1e-3          # epsilon outside the root is another number
    w2, ms2, mom2, _, _, _ = sr.rmsprop(w, ms, mom, [0.0], 0.1, 0.9, 0.5, 1.0, [0.0])
    assert abs(ms2[0] - 1.17) < 1e-15 and abs(mom2[0] - 0.1 / 2.3 ** 0.5) < 1e-15 and abs(w2[0] - (w[0] - mom2[0])) < 1e-15


# ------------------------------------------------------------------------------------------ losses against autograd
@pytest.mark.parametrize('shape', [(3, 9, 16), (2, 15, 17), (4, 49, 13)])
def test_pose_l2_gradient_is_autograd_of_the_oracle(shape):
    N, P, J = shape
    r = _rng(4)
    Pl, lbl = r.standard_normal(shape), r.standard_normal(shape)
    valid = r.random((N, J)) < 0.6
    loss, dPl, T_loss, T_g = sr.pose_l2(Pl, lbl, valid, wt=0.7, grad_scale=1.0)
    x = torch.from_numpy(Pl).view(N, P, 1, J).requires_grad_(True)
    L = orc.pose_l2_loss(x, torch.from_numpy(lbl).view(N, P, 1, J), torch.from_numpy(valid), 0.7)
    L.backward()
    assert abs(loss - float(L.detach())) == 0.0
    np.testing.assert_allclose(dPl, x.grad.numpy().reshape(shape), rtol=0, atol=1e-15)
    assert (dPl[~np.broadcast_to(valid[:, None, :], shape)] == 0).all()
    assert T_loss >= abs(loss) and (T_g >= np.abs(dPl)).all()
    # grad_scale multiplies the gradient alone
    l2, d2, _, _ = sr.pose_l2(Pl, lbl, valid, wt=0.7, grad_scale=3.0)
    assert l2 == loss
    np.testing.assert_allclose(d2, 3.0 * dPl, rtol=1e-15, atol=0)


@pytest.mark.parametrize('kind', ['l2', 'multi-label', 'multi-label-2'])
@pytest.mark.parametrize('pw', [10.0, 0.25])
def test_action_loss_gradient_is_autograd_of_the_oracle(kind, pw):
    r = _rng(5)
    N, K = 7, 11
    x = np.concatenate([2.5 * r.standard_normal((N - 1, K)), [[0, 20, -20, 60, -60, 88.8, -88.8, 100, -100, 1, -1]]])
    labels = r.integers(0, K, N) if kind == 'l2' else (r.random((N, K)) < 0.3).astype(np.float64)
    loss, G, T_loss, T_G = sr.action_loss(kind, x, labels, wt=0.7, grad_scale=1.0, pos_weight=pw)
    xt = torch.from_numpy(x).requires_grad_(True)
    if kind == 'l2':
        L = orc.action_l2(xt, torch.from_numpy(labels), K, 0.7)
    elif kind == 'multi-label':
        L = orc.action_multi_label(xt, torch.from_numpy(labels), pw)
    else:
        L = orc.action_multi_label_2(xt, torch.from_numpy(labels), 0.7)
    L.backward()
    assert np.isfinite(loss) and np.isfinite(G).all()
    assert loss == float(L.detach())
    # at x = 0 exactly autograd picks a subgradient of max(x, 0) and |x| (multi-label-2), not the derivative: that
    # element is held to the mean of its two neighbours' one-sided values instead
    nz = x != 0
    np.testing.assert_allclose(G[nz], xt.grad.numpy()[nz], rtol=1e-12, atol=1e-16)   # autograd forms 1 - e / (1 + e)
    lo, hi = (sr.action_loss(kind, np.where(nz, x, e), labels, wt=0.7, pos_weight=pw)[1] for e in (-1e-9, 1e-9))
    np.testing.assert_allclose(G[~nz], 0.5 * (lo + hi)[~nz], rtol=1e-12, atol=1e-16)
    assert T_loss >= abs(loss) * (1 - 1e-12) and (T_G >= np.abs(G) * (1 - 1e-12)).all()


def test_pose_sampled_gradient_and_mask():
    r = _rng(6)
    N, P, J = 3, 25, 5
    Pl = r.standard_normal((N, P, J))
    lbl = np.maximum(r.standard_normal((N, P, J)), 0.0)
    lbl[..., 1] = 0.0                                           # no positives: ratio 0
    lbl[..., 2] = np.abs(lbl[..., 2]) + 0.5                      # all positives: ratio 1
    u = r.random((N, P, J))
    valid = r.random((N, J)) < 0.7
    loss, dPl, mask, T_loss, T_g = sr.pose_sampled(Pl, lbl, valid, u, wt=0.7)
    ratio = sr.pose_sampled_ratio(lbl)
    assert ratio[1] == 0.0 and ratio[2] == 1.0
    expect = ((u < ratio) & (lbl == 0)) | (Pl > 0)               # the kernel header's own statement of the mask
    assert (mask == expect).all()
    assert (mask[..., 1] == (Pl[..., 1] > 0)).all() and (mask[..., 2] == (Pl[..., 2] > 0)).all()
    x = torch.from_numpy(Pl).view(N, P, 1, J).requires_grad_(True)
    L, _ = orc.pose_l2_sampled_loss(x, torch.from_numpy(lbl).view(N, P, 1, J), torch.from_numpy(valid),
                                    torch.from_numpy(u).view(N, P, 1, J), 0.7)
    L.backward()
    assert loss == float(L.detach())
    np.testing.assert_allclose(dPl, x.grad.numpy().reshape(N, P, J), rtol=0, atol=1e-15)
    assert T_loss >= abs(loss) and (T_g >= np.abs(dPl)).all()


@pytest.mark.parametrize('BF', [(1, 1), (2, 5), (3, 3)])
def test_frame_pool_backward_is_autograd_of_the_oracle(BF):
    B, F = BF
    K = 13
    r = _rng(7)
    x, g = r.standard_normal((B * F, K)), r.standard_normal((B, K))
    w, b0 = r.standard_normal(K), 1.0 / F
    # temporal
    xt = torch.from_numpy(x).requires_grad_(True)
    wt = torch.from_numpy(w).view(K, 1).requires_grad_(True)
    bt = torch.tensor([b0], dtype=D, requires_grad=True)
    pooled, ep = orc.frame_pooling(xt, F, wt, bt)
    (pooled * torch.from_numpy(g)).sum().backward()
    p2, tatt, T_p, T_a = sr.frame_pool_fwd(x, F, w, b0)
    np.testing.assert_allclose(p2, pooled.detach().numpy(), rtol=0, atol=0)
    assert (T_p >= np.abs(p2) * (1 - 1e-12)).all() and (T_a >= np.abs(tatt)).all()
    out, mag = sr.frame_pool_bwd(x, F, w, tatt, g)
    np.testing.assert_allclose(out['dx'], xt.grad.numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(out['dw'], wt.grad.numpy().reshape(K), rtol=0, atol=1e-13)
    np.testing.assert_allclose(out['db'], bt.grad.numpy(), rtol=0, atol=1e-13)
    for k in ('dx', 'dw', 'db'):
        assert (mag[k] >= np.abs(out[k]) * (1 - 1e-12)).all()
    # plain
    xt = torch.from_numpy(x).requires_grad_(True)
    pooled, _ = orc.frame_pooling(xt, F)
    (pooled * torch.from_numpy(g)).sum().backward()
    out, mag = sr.frame_pool_bwd(x, F, None, None, g)
    np.testing.assert_allclose(out['dx'], xt.grad.numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(sr.frame_pool_fwd(x, F)[0], pooled.detach().numpy(), rtol=0, atol=0)


def test_spatial_mean_backward_and_zero_out_channels():
    r = _rng(8)
    dz = r.standard_normal((3, 8))
    x = torch.from_numpy(r.standard_normal((3, 7, 8))).requires_grad_(True)
    (x.mean(dim=1) * torch.from_numpy(dz)).sum().backward()
    np.testing.assert_allclose(sr.spatial_mean_bwd(dz, 7), x.grad.numpy(), rtol=0, atol=1e-16)
    a = r.standard_normal((2, 3, 5))
    ch = np.array([True, False, True, True, False])
    z = sr.zero_out_channels(a, ch)
    for c in range(5):
        assert (z[..., c] == (a[..., c] if ch[c] else 0.0)).all()


# ------------------------------------------------------------------------------------------ image map, accumulation
@pytest.mark.parametrize('m', [dict(cols=5, sh=0, a=1, b=0, d=16, e=0), dict(cols=5, sh=2, a=1, b=3, d=13, e=0),
                               dict(cols=5, sh=0, a=5, b=0, d=1, e=7), dict(cols=3, sh=1, a=2, b=1, d=9, e=2)])
def test_image_map_is_the_double_loop(m):
    rows = 12 if m['cols'] == 5 else 7
    w = np.arange(rows * m['cols'], dtype=np.float64) + 1.0
    got = sr.image_scatter(w, size=96, fill=-3.0, **m)
    expect = np.full(96, -3.0)
    seen = set()
    for c in range(rows):
        for k in range(m['cols']):
            idx = (c >> m['sh']) * m['a'] + (c & ((1 << m['sh']) - 1)) * m['b'] + k * m['d'] + m['e']
            assert idx not in seen                               # the maps the GPU cases use are one-to-one
            seen.add(idx)
            expect[idx] = w[c * m['cols'] + k]
    assert (got == expect).all()
    assert (got != -3.0).sum() == rows * m['cols']


def test_accumulation_order_and_division():
    r = _rng(9)
    parts = [r.standard_normal(9).astype(np.float32) for _ in range(5)]
    ref, T = sr.accumulate(parts, divisor=3.0)
    np.testing.assert_allclose(ref, (((parts[0].astype(np.float64) + parts[1]) + parts[2]) + parts[3] + parts[4]) / 3.0,
                               rtol=0, atol=1e-16)
    # the fp32 sequence is within its 5 roundings of the float64 value
    sr.assert_close(sr.accumulate_f32(parts, divisor=3.0), ref, T, 5, 'fp32 sequence / 3')
    ref, T = sr.accumulate(parts, scale=1.0 / 3.0)
    sr.assert_close(sr.accumulate_f32(parts, scale=np.float32(1.0 / 3.0)), ref, T, 6, 'fp32 sequence * (1/3)')
    # a third is where division and multiplication by the reciprocal part
    one = [np.arange(1, 200, dtype=np.float32)]
    assert (sr.accumulate_f32(one, divisor=3.0) != sr.accumulate_f32(one, scale=np.float32(1.0 / 3.0))).any()


def test_assert_close_is_per_element():
    ref = np.array([1000.0, 1e-3])
    sr.assert_close(ref.astype(np.float32), ref, np.abs(ref), 1)
    with pytest.raises(AssertionError):                          # 1e-6 of the array's maximum, all of a small element
        sr.assert_close(np.array([1000.0, 0.0]), ref, np.abs(ref), 4, 'small element')
    with pytest.raises(AssertionError):
        sr.assert_close(np.array([1000.0, np.nan]), ref, np.abs(ref), 4)
    sr.assert_close(np.zeros(2), np.zeros(2), np.zeros(2), 1)


def test_pose_l2_share_rule():
    assert [sr.pose_l2_split(*s) for s in ((3, 9, 16), (2, 15, 17), (257, 4, 13), (2, 225, 13), (4, 49, 16),
                                           (40, 225, 16))] == [1, 1, 1, 8, 3, 7]
    sh = sr.pose_l2_shares(2, 225, 13)
    assert sh[0] == (0, 366) and sh[7] == (2562, 2925) and 366 % 13 != 0
    assert sr.pose_l2_shares(4, 49, 16) == [(0, 262), (262, 524), (524, 784)]
    assert len(sr.pose_l2_shares(40, 225, 16)) * 40 == 280


# ------------------------------------------------------------------------------------------ refusals before any launch
FAKE = [0x10000 * (i + 1) for i in range(12)]


def _err(lib):
    return lib.apa_last_error()


def test_pose_sampled_refuses_j_65():
    lib = cof.load_library()
    rc = lib.apa_pose_sampled_loss_fwd_bwd(*FAKE[:7], 2, 4, 65, 1.0, 1.0, None)
    assert (rc, _err(lib)) == (UNSUPPORTED, b'apa_pose_sampled_loss_fwd_bwd: J=65 > 64')
    assert lib.apa_pose_sampled_loss_fwd_bwd(None, *FAKE[:6], 2, 4, 64, 1.0, 1.0, None) == INVALID


def test_spatial_mean_bwd_refusals():
    lib = cof.load_library()
    msg = b'apa_spatial_mean_bwd: C=%d must be a multiple of 4 and both buffers 16-byte aligned'
    assert (lib.apa_spatial_mean_bwd(FAKE[0], FAKE[1], 2, 3, 6, cof.APA_DTYPE_F32, None), _err(lib)) == (
        UNSUPPORTED, msg % 6)
    for dz, dX in ((FAKE[0] + 4, FAKE[1]), (FAKE[0], FAKE[1] + 8)):
        for dt in (cof.APA_DTYPE_F32, cof.APA_DTYPE_BF16):
            assert (lib.apa_spatial_mean_bwd(dz, dX, 2, 3, 8, dt, None), _err(lib)) == (UNSUPPORTED, msg % 8)
    assert (lib.apa_spatial_mean_bwd(FAKE[0], FAKE[1], 2, 3, 8, 7, None), _err(lib)) == (
        INVALID, b'apa_spatial_mean_bwd: unknown dtype 7')
    assert lib.apa_spatial_mean_bwd(FAKE[0], FAKE[1], 0, 3, 8, cof.APA_DTYPE_F32, None) == INVALID


def _sgd_args(sizes, shadow=None):
    n = len(sizes)
    w = (ctypes.c_void_p * n)(*[FAKE[0] + 0x1000 * i for i in range(n)])
    sz = (ctypes.c_size_t * n)(*sizes)
    wd = (ctypes.c_float * n)(*([0.0] * n))
    sh = None if shadow is None else (ctypes.c_void_p * n)(*shadow)
    return n, w, sz, wd, sh


def _image(dst=FAKE[5], cols=5, sh=0, a=1, b=0, d=16, e=0, f32=1):
    m = cof.ApaWeightImage()
    m.dst, m.role, m.is_f32, m.cols, m.c_shift, m.a, m.b, m.d, m.e = dst, 0, f32, cols, sh, a, b, d, e
    return m


def _images_call(sizes, images, segs, shadow=None):
    lib = cof.load_library()
    n, w, sz, wd, sh = _sgd_args(sizes, shadow)
    arr = (cof.ApaWeightImage * max(len(images), 1))(*images)
    seg = (ctypes.c_int * max(len(segs), 1))(*segs)
    rc = lib.apa_momentum_sgd_step_images(n, w, sz, wd, FAKE[1], FAKE[2], 0.1, 0.9, 1.0, sh, ctypes.addressof(arr),
                                          seg, len(images), None)
    return rc, _err(lib)


def test_momentum_refuses_a_shadow_on_a_2_byte_boundary():
    lib = cof.load_library()
    n, w, sz, wd, sh = _sgd_args([5, 1031], [None, FAKE[3] + 2])
    rc = lib.apa_momentum_sgd_step_shadow(n, w, sz, wd, FAKE[1], FAKE[2], 0.1, 0.9, 1.0, sh, None)
    assert (rc, _err(lib)) == (INVALID, b'apa_momentum_sgd_step_shadow: bf16_shadow[1] must be 4-byte aligned')
    assert _images_call([5, 60], [_image()], [1], [FAKE[3] + 6, None]) == (
        INVALID, b'apa_momentum_sgd_step_images: bf16_shadow[0] must be 4-byte aligned')


def test_weight_image_refusals():
    bad = b'apa_momentum_sgd_step_images: bad weight image %d (segment %d, cols %d; at most 3 images per segment, ' \
          b'whole rows)'
    # a fourth image on one segment
    assert _images_call([3, 60], [_image()] * 4, [1, 1, 1, 1]) == (INVALID, bad % (3, 1, 5))
    # cols does not divide the segment
    assert _images_call([3, 60], [_image(cols=7)], [1]) == (INVALID, bad % (0, 1, 7))
    # a segment index outside the call, a null image, a shift beyond 20
    assert _images_call([3, 60], [_image()], [2])[0] == INVALID
    assert _images_call([3, 60], [_image(dst=None)], [1])[0] == INVALID
    assert _images_call([3, 60], [_image(sh=21)], [1])[0] == INVALID
    # 17 segments
    assert _images_call([4] * 17, [_image(cols=4)], [0]) == (
        INVALID, b'apa_momentum_sgd_step_images: bad arguments (nseg=17, max 16)')
    lib = cof.load_library()
    n, w, sz, wd, _ = _sgd_args([4] * 17)
    assert lib.apa_momentum_sgd_step(n, w, sz, wd, FAKE[1], FAKE[2], 0.1, 0.9, 1.0, None) == INVALID
    assert lib.apa_adam_step(n, w, sz, wd, FAKE[1], FAKE[2], FAKE[3], 0.1, 0.9, 0.999, 1.0, 1.0, None, None) == INVALID
    assert lib.apa_rmsprop_step(n, w, sz, wd, FAKE[1], FAKE[2], FAKE[3], 0.1, 0.9, 0.9, 1.0, 1.0, None, None) == INVALID


def test_accumulate_refusals():
    lib = cof.load_library()
    arr9 = (ctypes.c_void_p * 9)(*FAKE[:9])
    assert lib.apa_accumulate_gradients(FAKE[9], arr9, 9, 4, 1.0, None) == INVALID
    assert lib.apa_accumulate_gradients(FAKE[9], arr9, 0, 4, 1.0, None) == INVALID
    assert (lib.apa_accumulate_gradients_div(FAKE[9], arr9, 2, 4, 0.0, None), _err(lib)) == (
        INVALID, b'apa_accumulate_gradients_div: bad arguments (nparts=2, max 8, divisor 0)')
    hole = (ctypes.c_void_p * 2)(FAKE[0], None)
    assert (lib.apa_accumulate_gradients(FAKE[9], hole, 2, 4, 1.0, None), _err(lib)) == (
        INVALID, b'apa_accumulate_gradients: parts[1] is NULL')


def test_loss_entry_points_refuse_null_and_non_positive():
    lib = cof.load_library()
    assert lib.apa_pose_l2_loss_fwd_bwd(*FAKE[:4], None, FAKE[5], 1 << 20, 0, 4, 4, 1.0, 1.0, None) == INVALID
    assert lib.apa_pose_l2_loss_fwd_bwd(*FAKE[:4], None, FAKE[5], 8 * 4 * 3 - 1, 3, 4, 4, 1.0, 1.0, None) == -3
    assert lib.apa_pose_l2_workspace_bytes(3, 4, 4) == 96
    assert (lib.apa_action_loss_fwd_bwd(4, *FAKE[:4], 2, 3, 1.0, 1.0, 10.0, None), _err(lib)) == (
        INVALID, b'apa_action_loss_fwd_bwd: unknown loss kind 4')
    assert lib.apa_action_loss_fwd_bwd(1, *FAKE[:4], 2, 0, 1.0, 1.0, 10.0, None) == INVALID
    assert lib.apa_resize_bilinear_tf1(FAKE[0], FAKE[1], 1, 2, 2, 3, 0, 4, None) == INVALID
    assert lib.apa_zero_out_channels(FAKE[0], FAKE[1], FAKE[2], 4, 0, None) == INVALID
    assert lib.apa_frame_pool_fwd(FAKE[0], FAKE[1], None, FAKE[3], FAKE[4], 2, 3, 5, None) == INVALID
    assert lib.apa_frame_pool_bwd(FAKE[0], FAKE[1], FAKE[2], FAKE[3], FAKE[4], None, FAKE[6], FAKE[7], 2, 3, 5,
                                  None) == INVALID
