"""Float64 references of the loss, frame-pooling and optimiser kernels (csrc/apa_loss.hip, apa_loss2.hip,
apa_framepool.hip, apa_optim.hip), and the per-element comparison the support-path tests use.

Every function takes numpy arrays holding the kernel's own fp32 inputs and returns float64 results together with, per
output element, the MAGNITUDE OF TERMS T: the sum of the absolute values of the terms that form the element.  A kernel
that forms the element with m rounded fp32 operations errs by at most m * u * T (u = 2^-24), to first order, whatever
the cancellation between the terms; `assert_close` holds it to  |got - ref| <= c * u * T + tiny  per element.

Where oracle/attn_pool_oracle.py has the function (pose_l2_loss, pose_l2_sampled_loss, action_l2,
action_multi_label[_2], frame_pooling, tf1_resize_bilinear) it is called, in float64; the gradients and the optimiser
rules are restated here from the formulas in the kernels' header comments and held to torch autograd / torch.optim /
hand-stepped cases in tests/test_support_refs_cpu.py."""
import numpy as np
import torch

from oracle import attn_pool_oracle as orc

U = 2.0 ** -24        # unit roundoff of fp32 (half an ulp): one rounded operation errs by at most u * |result|
TINY = 1e-37          # for the true zeros
ULP = 2               # one ulp of a library function, in units of u


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(f64(a)))


def assert_close(got, ref, T, c, what=''):
    """|got - ref| <= c * u * T + tiny for EVERY element (a NaN or an infinity in `got` fails)."""
    got, ref = f64(got), f64(ref)
    T = np.broadcast_to(f64(T), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bound = c * U * T + TINY
    bad = ~(err <= bound)
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.nan_to_num(err / bound, nan=np.inf, posinf=np.inf), 0))),
                             ref.shape) if ref.shape else ()
        raise AssertionError('%s: %d of %d elements out of bound; worst at %s: got %r ref %r |err| %.3e bound %.3e '
                             '(c = %g)' % (what, int(bad.sum()), bad.size, i, got[i], ref[i], err[i], bound[i], c))


def ulps_apart(a, b):
    """distance of two fp32 numbers of equal sign in units in the last place"""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ------------------------------------------------------------------------------------------ pose L2 (apa_loss.hip)
def pose_l2_split(N, P, J):
    """the launcher's share count: ~256 blocks, at most 8 shares, at least 256 elements per share"""
    split = min((256 + N - 1) // N, 8)
    while split > 1 and (P * J + split - 1) // split < 256:
        split -= 1
    return split


def pose_l2_shares(N, P, J):
    """[(lo, hi)] of every share of one image's P*J elements (an empty last share has lo >= hi)"""
    split = pose_l2_split(N, P, J)
    chunk = (P * J + split - 1) // split
    return [(s * chunk, min(P * J, (s + 1) * chunk)) for s in range(split)]


def pose_l2(Pl, lbl, valid, wt=1.0, grad_scale=1.0):
    """Pl, lbl [N,P,J], valid [N,J] -> loss, dPl, T_loss, T_dPl.
    loss = wt * 0.5 / (N^2 P) * sum valid * (Pl - lbl)^2 (oracle.pose_l2_loss); dPl = grad_scale * wt / (N^2 P) *
    valid * (Pl - lbl)."""
    Pl, lbl = f64(Pl), f64(lbl)
    N, P, J = Pl.shape
    v = np.asarray(valid).astype(bool)
    loss = float(orc.pose_l2_loss(_t(Pl).view(N, P, 1, J), _t(lbl).view(N, P, 1, J), torch.from_numpy(v), wt))
    vm = v[:, None, :].astype(np.float64)
    k = 1.0 / (float(N) * N * P)
    mag = np.abs(Pl) + np.abs(lbl)
    return (loss, grad_scale * wt * k * vm * (Pl - lbl), float(0.5 * abs(wt) * k * (vm * mag * mag).sum()),
            abs(grad_scale * wt) * k * vm * mag)


# ------------------------------------------------------------------------------------------ action losses (apa_loss2.hip)
def sigmoid(x):
    x = f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def softplus(x):
    """log(1 + exp(x)), stable"""
    x = f64(x)
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0.0)


def action_loss(kind, x, labels, wt=1.0, grad_scale=1.0, pos_weight=10.0):
    """x [N,K]; labels int [N] ('l2') or multi-hot [N,K] -> loss, G, T_loss, T_G.  The loss is the oracle's; G:
         l2             2 (x - t) * wt / NK
         multi-label    ((1 - t) - (1 + (pw - 1) t) (1 - sigmoid x)) / NK          (action_loss_wt is not applied)
         multi-label-2  (sigmoid x - t) * wt / NK                                   each times grad_scale."""
    x = f64(x)
    N, K = x.shape
    nk = float(N * K)
    if kind == 'l2':
        lab = np.asarray(labels).astype(np.int64)
        loss = float(orc.action_l2(_t(x), torch.from_numpy(lab), K, wt))
        t = np.zeros((N, K))
        t[np.arange(N), lab] = 1.0
        mag = np.abs(x) + t
        return (loss, 2.0 * (x - t) * wt / nk * grad_scale, float(abs(wt) / nk * (mag * mag).sum()),
                2.0 * mag * abs(wt * grad_scale) / nk)
    t = f64(labels)
    s = sigmoid(x)
    if kind == 'multi-label':
        loss = float(orc.action_multi_label(_t(x), _t(t), pos_weight))
        w = 1.0 + (pos_weight - 1.0) * t
        G = ((1.0 - t) - w * sigmoid(-x)) / nk * grad_scale
        wm = 1.0 + abs(pos_weight - 1.0) * np.abs(t)              # the terms of w = 1 + (pw - 1) t
        T_loss = float((np.abs((1.0 - t) * x) + wm * softplus(-x)).sum() / nk)
        return loss, G, T_loss, (np.abs(1.0 - t) + wm * (1.0 + s)) * abs(grad_scale) / nk
    assert kind == 'multi-label-2'
    loss = float(orc.action_multi_label_2(_t(x), _t(t), wt))
    T_loss = float(abs(wt) / nk * (np.maximum(x, 0.0) + np.abs(x * t) + np.log1p(np.exp(-np.abs(x)))).sum())
    return loss, (s - t) * wt / nk * grad_scale, T_loss, (s + np.abs(t)) * abs(wt * grad_scale) / nk


# ------------------------------------------------------------------------------------------ sampled pose loss
def pose_sampled(Pl, lbl, valid, u, wt=1.0, grad_scale=1.0):
    """Pl, lbl, u [N,P,J], valid [N,J] -> loss, dPl, mask, T_loss, T_dPl (oracle.pose_l2_sampled_loss); the mask is
    a constant of the gradient: dPl = grad_scale * wt / (N P) * valid * mask * (Pl - lbl)."""
    Pl, lbl, u = f64(Pl), f64(lbl), f64(u)
    N, P, J = Pl.shape
    v = np.asarray(valid).astype(bool)
    loss, mask = orc.pose_l2_sampled_loss(_t(Pl).view(N, P, 1, J), _t(lbl).view(N, P, 1, J), torch.from_numpy(v),
                                          _t(u).view(N, P, 1, J), wt)
    mask = mask.numpy().reshape(N, P, J)
    vm = v[:, None, :].astype(np.float64)
    k = 1.0 / (float(N) * P)
    mag = (np.abs(Pl) + np.abs(lbl)) * mask
    return (float(loss), grad_scale * wt * k * vm * mask * (Pl - lbl), mask,
            float(0.5 * abs(wt) * k * (vm * mag * mag).sum()), abs(grad_scale * wt) * k * vm * mag)


def pose_sampled_ratio(lbl):
    """ratio_j = #(label > 0) / (N P), per keypoint channel"""
    lbl = f64(lbl)
    return (lbl > 0).sum(axis=(0, 1)) / float(lbl.shape[0] * lbl.shape[1])


def resize_bilinear(img, oh, ow):
    return orc.tf1_resize_bilinear(_t(img), oh, ow).numpy()


# ------------------------------------------------------------------------------------------ frame pooling
def frame_pool_fwd(x, F, w=None, b0=None):
    """x [B*F,K] -> pooled [B,K], tatt [B*F] or None, T_pooled, T_tatt (oracle.frame_pooling)."""
    x = f64(x)
    BF, K = x.shape
    B = BF // F
    if w is None:
        pooled, _ = orc.frame_pooling(_t(x), F)
        return pooled.numpy(), None, np.abs(x).reshape(B, F, K).sum(axis=1) / F, None
    w, b0 = f64(w).reshape(K), float(np.asarray(b0).reshape(()))
    pooled, ep = orc.frame_pooling(_t(x), F, _t(w).view(K, 1), torch.tensor([b0], dtype=torch.float64))
    T_a = np.abs(x) @ np.abs(w) + abs(b0)
    return (pooled.numpy(), ep['TemporalAttention'].numpy().reshape(BF),
            (np.abs(x) * T_a[:, None]).reshape(B, F, K).sum(axis=1) / F, T_a)


def frame_pool_bwd(x, F, w, tatt, g):
    """the header of fp_bwd_kernel / fp_bwd_w_kernel, `tatt` as given:
         dLda[row] = (1/F) sum_k g[b,k] x[row,k];  dx[row,k] = (1/F) g[b,k] a[row] + dLda[row] w[k]  (plain: g / F)
         dw[k] = sum_rows dLda[row] x[row,k];  db = sum_rows dLda[row]
    -> dict(dx, dw, db) and dict of their magnitudes (+ 'dlda')."""
    x, g = f64(x), f64(g)
    BF, K = x.shape
    gr = np.repeat(g, F, axis=0)                                  # [B*F,K]: row -> its video's gradient
    if w is None:
        return dict(dx=gr / F, dw=None, db=None), dict(dx=np.abs(gr) / F)
    w, a = f64(w).reshape(K), f64(tatt).reshape(BF)
    d = (gr * x).sum(axis=1) / F
    T_d = (np.abs(gr) * np.abs(x)).sum(axis=1) / F
    out = dict(dx=gr / F * a[:, None] + d[:, None] * w[None, :], dw=d @ x, db=np.array([d.sum()]))
    mag = dict(dx=np.abs(gr) / F * np.abs(a)[:, None] + T_d[:, None] * np.abs(w)[None, :], dw=T_d @ np.abs(x),
               db=np.array([T_d.sum()]), dlda=T_d)
    return out, mag


# ------------------------------------------------------------------------------------------ small elementwise ops
def spatial_mean_bwd(dz, P):
    """dX[n,p,c] = dz[n,c] / P"""
    dz = f64(dz)
    return np.broadcast_to((dz / P)[:, None, :], (dz.shape[0], P, dz.shape[1]))


def zero_out_channels(x, ch):
    x = f64(x)
    return np.where(np.asarray(ch).astype(bool), x, 0.0)


# ------------------------------------------------------------------------------------------ optimisers (apa_optim.hip)
def momentum_sgd(w, acc, g, lr, momentum, wd, grad_scale=1.0):
    """tf.train.MomentumOptimizer with the slim L2 term: acc <- m acc + (gs g + wd w);  w <- w - lr acc.
    `wd` per element (0 where the segment carries no regulariser) -> w', acc', T_w, T_acc."""
    w, acc, g, wd = f64(w), f64(acc), f64(g), f64(wd)
    a = momentum * acc + (grad_scale * g + wd * w)
    T_a = np.abs(momentum * acc) + np.abs(grad_scale * g) + np.abs(wd * w)
    return w - lr * a, a, np.abs(w) + abs(lr) * T_a, T_a


def adam_lr_t(lr, t, beta1=0.9, beta2=0.999):
    """TF forms lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) on the host, t counted from 1"""
    return lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)


def adam(w, m, v, g, lr_t, beta1, beta2, eps, wd, grad_scale=1.0):
    """TF 1.1 ApplyAdam on g' = gs g + wd w:  m <- m + (g' - m)(1 - b1);  v <- v + (g'^2 - v)(1 - b2);
    w <- w - lr_t m / (sqrt(v) + eps)   (epsilon OUTSIDE the root) -> w', m', v', T_w, T_m, T_v."""
    w, m, v, g, wd = f64(w), f64(m), f64(v), f64(g), f64(wd)
    gg = grad_scale * g + wd * w
    T_g = np.abs(grad_scale * g) + np.abs(wd * w)
    m1 = m + (gg - m) * (1.0 - beta1)
    v1 = v + (gg * gg - v) * (1.0 - beta2)
    T_m = np.abs(m) + (T_g + np.abs(m)) * (1.0 - beta1)
    T_v = np.abs(v) + (T_g * T_g + np.abs(v)) * (1.0 - beta2)
    D = np.sqrt(v1) + eps
    upd = lr_t * m1 / D
    amp = np.divide(T_v, v1, out=np.zeros_like(v1), where=v1 > 0)       # v' = 0 only when every term of it is 0
    T_w = np.abs(w) + abs(lr_t) * T_m / D + np.abs(upd) * (1.0 + amp)
    return w - upd, m1, v1, T_w, T_m, T_v


def rmsprop(w, ms, mom, g, lr, decay, momentum, eps, wd, grad_scale=1.0):
    """TF 1.1 ApplyRMSProp on g' = gs g + wd w:  ms <- ms + (g'^2 - ms)(1 - rho);  mom <- momentum mom +
    lr g' / sqrt(ms + eps)   (epsilon INSIDE the root);  w <- w - mom.  `ms` starts at ONE, `mom` at zero
    -> w', ms', mom', T_w, T_ms, T_mom."""
    w, ms, mom, g, wd = f64(w), f64(ms), f64(mom), f64(g), f64(wd)
    gg = grad_scale * g + wd * w
    T_g = np.abs(grad_scale * g) + np.abs(wd * w)
    ms1 = ms + (gg * gg - ms) * (1.0 - decay)
    T_ms = np.abs(ms) + (T_g * T_g + np.abs(ms)) * (1.0 - decay)
    S = ms1 + eps
    mom1 = momentum * mom + lr * gg / np.sqrt(S)
    T_mom = np.abs(momentum * mom) + abs(lr) * T_g / np.sqrt(S) * (1.0 + T_ms / S)
    return w - mom1, ms1, mom1, np.abs(w) + T_mom, T_ms, T_mom


def rmsprop_slots(n):
    """rmsprop.py `_create_slots`: ms = 1, mom = 0"""
    return np.ones(n), np.zeros(n)


def image_index(i, cols, sh, a, b, d, e):
    """where the weight image keeps flat element i = (c, k) = (i // cols, i % cols) of its segment"""
    c, k = i // cols, i % cols
    return (c >> sh) * a + (c & ((1 << sh) - 1)) * b + k * d + e


def image_scatter(wseg, cols, sh, a, b, d, e, size, fill):
    """a fresh float64 array of `size` elements, `fill` everywhere but where the map puts the segment's elements"""
    wseg = f64(wseg).reshape(-1)
    out = np.full(size, float(fill))
    out[image_index(np.arange(wseg.size), cols, sh, a, b, d, e)] = wseg
    return out


def accumulate(parts, divisor=None, scale=None):
    """((p0 + p1) + p2 ...) / divisor or ... * scale -> out, T"""
    s = f64(parts[0]).copy()
    T = np.abs(s)
    for p in parts[1:]:
        s = s + f64(p)
        T = T + np.abs(f64(p))
    return (s / divisor, T / abs(divisor)) if divisor is not None else (s * scale, T * abs(scale))


def accumulate_f32(parts, divisor=None, scale=None):
    """the same in fp32, one IEEE operation after the other in the stated order: what the kernel must give bit for
    bit"""
    s = np.asarray(parts[0], np.float32).copy()
    for p in parts[1:]:
        s = s + np.asarray(p, np.float32)
    return s / np.float32(divisor) if divisor is not None else s * np.float32(scale)
