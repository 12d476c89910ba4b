"""float64 restatements of the two ops of csrc/apa_explain.hip (include/apa.h: apa_attn_explain, apa_attention_overlay)
and the seeded inputs of tests/golden/ref_overlay.npz.  Test infrastructure.

apa_attn_explain.  The three outputs come back as `_m1_probe.Bnd` values (float64 reference + elementwise absolute
bound) under the project's forward-error rule C_ACC * L * EPS32 * sum |a| |b|:
  * topdown: a contraction of length L = C (the bias is one more term of the sum);
  * combined: one more fp32 rounding (Bnd.mul with the exact `att`);
  * class_logit: a sum of length L = P over combined.
Nothing is added for bf16 features: the reference reads the bf16 values themselves.

apa_attention_overlay.  `overlay_reference` restates src/train.py:184-195 with the TF 1.1 legacy resize rule (scale, source
coordinate and lerp weight in float32, as tests/golden/tf1_shim.py resize_images forms them; everything else float64;
the grey weights are the float32 constants of a float32 graph) and returns the value with the sum of the magnitudes of
its terms, for the bound C_ACC * 8 * EPS32 * sum |terms| (eight roundings lie between the inputs and an output element).
`overlay_u8_reference` is this project's uint8 rule (apa.h; what tf.summary.image documents) in float64.
"""
import zlib

import numpy as np
import torch

from tests._m1_probe import Bnd, C_ACC, EPS32, contract

OVERLAY_OPS = 8            # roundings between the inputs and one overlay element
BAND = 2.0 ** -10          # uint8: distance of v * s + o from an integer below which a difference of 1 is allowed
BAND_SHARE = 0.01          # at most this share of an image's values may lie in the band (a condition on the inputs)


# ------------------------------------------------------------------------------------------------ apa_attn_explain
def explain_reference(X, att, Wt, bt, classes, relu_input=False):
    """X [N,P,C] (f32 / bf16), att [N,P,M] f32, Wt [C,K], bt [K], classes [N,T] integers (any device).  Returns
    (topdown, combined, class_logit) as Bnd with shapes [N,T,P], [N,T,P], [N,T], and the number of clamped ids."""
    x = X.detach().cpu().double()
    if relu_input:
        x = x.clamp_min(0)
    a = att.detach().cpu().double()
    W, b = Wt.detach().cpu().double(), bt.detach().cpu().double()
    cls = classes.detach().cpu().long()
    if cls.dim() == 1:
        cls = cls.view(-1, 1)
    N, P, C = x.shape
    K = W.shape[1]
    k = cls.clamp(0, K - 1)
    clamped = int((k != cls).sum())
    Wsel = W[:, k]                                                    # [C,N,T]
    ref = torch.einsum('npc,cnt->ntp', x, Wsel) + b[k][:, :, None]
    mag = torch.einsum('npc,cnt->ntp', x.abs(), Wsel.abs()) + b[k].abs()[:, :, None]
    td = Bnd(ref, C_ACC * C * EPS32 * mag)
    if a.shape[2] == 1:
        asel = a[:, :, 0][:, None, :].expand(N, k.shape[1], P)
    else:
        asel = torch.gather(a, 2, k[:, None, :].expand(N, P, k.shape[1])).permute(0, 2, 1)
    comb = Bnd(asel.contiguous()).mul(td)
    cmag = (comb.ref.abs() + comb.err).sum(-1)
    logit = Bnd(comb.ref.sum(-1) / P, comb.err.sum(-1) / P + C_ACC * P * EPS32 * cmag / P)
    return td, comb, logit, clamped


def eval_logits_reference(X, att, Wt, bt, relu_input=False):
    """logits [N,K] of the class-agnostic evaluation step from ITS OWN attention map `att` [N,P,1] (taken as exact):
    z = (1/P) sum_p A x (L = P), logits = z . Wt + abar (x) bt (L = C) -- the bound the step's logits are held to."""
    x = X.detach().cpu().double()
    if relu_input:
        x = x.clamp_min(0)
    P = x.shape[1]
    if att.shape[2] != 1:
        # per-class maps: logits[n,k] = (1/P) sum_p A[n,p,k] T[n,p,k], T = x . Wt + bt (L = C), then L = P
        T = contract('npc,ck->npk', Bnd(x), Bnd(Wt.detach().cpu().double()), x.shape[2]) + \
            Bnd(bt.detach().cpu().double()[None, None, :].expand(x.shape[0], P, -1))
        prod = Bnd(att.detach().cpu().double()).mul(T.rounded())
        mag = (prod.ref.abs() + prod.err).sum(1)
        return Bnd(prod.ref.sum(1) / P, prod.err.sum(1) / P + C_ACC * (P + 8) * EPS32 * mag / P)
    A = Bnd(att.detach().cpu().double()[:, :, 0])
    z = contract('np,npc->nc', A, Bnd(x), P).scale(1.0 / P).rounded()
    abar = Bnd(A.ref.sum(1) / P, C_ACC * (P + 8) * EPS32 * A.ref.abs().sum(1) / P)
    lg = contract('nc,ck->nk', z, Bnd(Wt.detach().cpu().double()), x.shape[2])
    return lg + Bnd(abar.ref[:, None], abar.err[:, None]).mul(Bnd(bt.detach().cpu().double()[None, :]))


# ------------------------------------------------------------------------------------------- apa_attention_overlay
GRAY_W = [float(np.float32(v)) for v in (0.2989, 0.5870, 0.1140)]


def _taps(out_size, in_size):
    """tf.image.resize_images, TF 1.1 (align_corners=False): scale, source coordinate and lerp weight in float32"""
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.arange(out_size, dtype=np.float32) * scale
    lo = np.floor(src).astype(np.int64)
    t = (src - np.floor(src)).astype(np.float32).astype(np.float64)
    lo = np.minimum(lo, in_size - 1)
    hi = np.minimum(lo + 1, in_size - 1)
    return lo, hi, t


def _resize(m, H, W, mag=False):
    """[..., h, w] -> [..., H, W]; mag: the same expression on absolute values (every term's magnitude)"""
    h, w = m.shape[-2:]
    y0, y1, fy = _taps(H, h)
    x0, x1, fx = _taps(W, w)
    fy = fy[:, None]
    tl, tr = m[..., y0, :][..., x0], m[..., y0, :][..., x1]
    bl, br = m[..., y1, :][..., x0], m[..., y1, :][..., x1]
    if mag:
        tl, tr, bl, br = np.abs(tl), np.abs(tr), np.abs(bl), np.abs(br)
        top, bot = tl + (tr + tl) * fx, bl + (br + bl) * fx
        return top + (bot + top) * fy
    top, bot = tl + (tr - tl) * fx, bl + (br - bl) * fx
    return top + (bot - top) * fy


def overlay_reference(maps, images):
    """maps [N,T,h,w], images [N,H,W,3] (numpy, float32 values) -> (overlay [N,T,H,W,3] float64, sum |terms|)"""
    maps = np.asarray(maps, dtype=np.float64)
    images = np.asarray(images, dtype=np.float64)
    N, T = maps.shape[:2]
    H, W = images.shape[1:3]
    m, mm = _resize(maps, H, W), _resize(maps, H, W, mag=True)
    gray = (GRAY_W[0] * images[..., 0] + GRAY_W[1] * images[..., 1]) + GRAY_W[2] * images[..., 2]
    gmag = np.abs(images) @ np.asarray(GRAY_W)
    out = np.empty((N, T, H, W, 3))
    mag = np.empty((N, T, H, W, 3))
    out[..., 0] = 0.5 * gray[:, None] + 0.5 * (m * 255.0)
    out[..., 1] = out[..., 2] = np.broadcast_to(0.5 * gray[:, None], (N, T, H, W))
    mag[..., 0] = 0.5 * gmag[:, None] + 0.5 * 255.0 * mm
    mag[..., 1] = mag[..., 2] = np.broadcast_to(0.5 * gmag[:, None], (N, T, H, W))
    return out, mag


def overlay_bound(mag):
    return C_ACC * OVERLAY_OPS * EPS32 * mag


def overlay_u8_reference(v):
    """v [N,T,H,W,3] float64 -> (uint8 [N,T,H,W,3], q = v * s + o in float64): per (n,t) image, lo / hi its min / max;
    lo < 0: s = 127 / max(|lo|,|hi|), o = 128; lo >= 0: s = 255 / hi, o = 0; max(|lo|,|hi|) == 0: s = 0."""
    N, T = v.shape[:2]
    flat = v.reshape(N, T, -1)
    lo, hi = flat.min(-1), flat.max(-1)
    mx = np.maximum(np.abs(lo), np.abs(hi))
    safe = np.where(mx == 0, 1.0, mx)
    s = np.where(lo < 0, 127.0 / safe, 255.0 / np.where(hi == 0, 1.0, hi))
    s = np.where(mx == 0, 0.0, s)
    o = np.where(lo < 0, 128.0, 0.0)
    q = v * s[:, :, None, None, None] + o[:, :, None, None, None]
    return np.clip(np.trunc(q), 0, 255).astype(np.uint8), q


def u8_band(q):
    """elements whose float64 v * s + o lies within BAND of an integer: there the float32 kernel may truncate to the
    neighbouring value"""
    return np.abs(q - np.rint(q)) <= BAND


def check_u8(got, v, what):
    """uint8 output against the float64 rule: exact outside the band, off by at most one inside it; the band holds at
    most BAND_SHARE of every (n,t) image."""
    want, q = overlay_u8_reference(v)
    band = u8_band(q)
    N, T = v.shape[:2]
    share = band.reshape(N, T, -1).mean(-1)
    print('%s: band share max %.4f' % (what, float(share.max())))
    assert float(share.max()) <= BAND_SHARE, '%s: %.4f of an image within 2^-10 of an integer' % (what, share.max())
    d = np.abs(np.asarray(got).astype(np.int64) - want.astype(np.int64))
    assert int(d[~band].max(initial=0)) == 0, '%s: %d values differ outside the band' % (what, int((d[~band] > 0).sum()))
    assert int(d.max(initial=0)) <= 1, '%s: a value differs by %d' % (what, int(d.max()))


# ------------------------------------------------------------------------------------------- seeded overlay inputs
# name, N, T, map h x w, image H x W, kind, seed.  'nonneg': an image in [0, 255] under a non-negative map (lo >= 0);
# 'meansub': the network's input, pixel - 128, under a signed map (lo < 0).
OVERLAY_CASES = [
    dict(name='m3x5_13x17_nonneg', N=2, T=2, h=3, w=5, H=13, W=17, kind='nonneg', seed=401),
    dict(name='m15x15_45x45_meansub', N=1, T=2, h=15, w=15, H=45, W=45, kind='meansub', seed=102),
    dict(name='m14x14_64x64_meansub', N=2, T=1, h=14, w=14, H=64, W=64, kind='meansub', seed=103),
    dict(name='m14x14_64x64_nonneg', N=1, T=1, h=14, w=14, H=64, W=64, kind='nonneg', seed=104),
]


# The edges of apa_attention_overlay that no fixture holds (tests/test_explain_gpu.py; their conditions are checked on
# the CPU from the float64 reference alone, tests/test_explain_paths_cpu.py).  Further kinds:
#   'mixed'   N = 2, T = 3: image 0 in [0, 255] under a map >= 0 (t = 0, lo >= 0), a map <= -1 (t = 1, lo < 0 and
#             |lo| > hi) and a map == 0 (t = 2, lo >= 0); image 1 mean-subtracted under signed maps -- the (n,t) images of
#             one call take different branches of the uint8 rule, with different extremes;
#   'allneg'  a negative image under a map <= 0: hi < 0, so max(|lo|,|hi|) is |lo|;
#   'lozero'  'nonneg' with a black pixel under a zero map corner: lo == 0 exactly, in float32 and in float64.
# The seeds are chosen so that at most BAND_SHARE of every (n,t) image lies in the uint8 band (the extreme value always
# lands on an integer, which is why the thin images are 301 long).
OVERLAY_EDGE_CASES = [
    dict(name='down_15x20_7x9', N=1, T=2, h=15, w=20, H=7, W=9, kind='meansub', seed=601),
    dict(name='identity_9x11', N=1, T=2, h=9, w=11, H=9, W=11, kind='nonneg', seed=602),
    dict(name='m1x1_13x17', N=2, T=1, h=1, w=1, H=13, W=17, kind='meansub', seed=503),
    dict(name='m1x7_5x40', N=1, T=2, h=1, w=7, H=5, W=40, kind='nonneg', seed=504),
    dict(name='m7x1_40x5', N=1, T=2, h=7, w=1, H=40, W=5, kind='meansub', seed=505),
    dict(name='row_image_1x301', N=1, T=2, h=3, w=5, H=1, W=301, kind='meansub', seed=506),
    dict(name='column_image_301x1', N=1, T=2, h=5, w=3, H=301, W=1, kind='nonneg', seed=507),
    dict(name='mixed_4x6_20x24', N=2, T=3, h=4, w=6, H=20, W=24, kind='mixed', seed=508),
    dict(name='allneg_4x6_20x24', N=1, T=2, h=4, w=6, H=20, W=24, kind='allneg', seed=509),
    dict(name='lozero_4x6_20x24', N=1, T=2, h=4, w=6, H=20, W=24, kind='lozero', seed=510),
    dict(name='m5x5_130x131', N=1, T=1, h=5, w=5, H=130, W=131, kind='meansub', seed=511),   # 17030 pixels
]


def overlay_inputs(case):
    """(maps [N,T,h,w] float32, images [N,H,W,3] float32) of a case, from its seed"""
    rs = np.random.RandomState(case['seed'])
    shape_m = (case['N'], case['T'], case['h'], case['w'])
    shape_i = (case['N'], case['H'], case['W'], 3)
    kind = case['kind']
    if kind in ('nonneg', 'lozero'):
        maps = rs.rand(*shape_m)
        images = np.floor(rs.rand(*shape_i) * 256.0)
        if kind == 'lozero':
            maps[:, :, 0, 0] = 0.0
            images[:, 0, 0, :] = 0.0
    elif kind == 'meansub':
        maps = rs.randn(*shape_m) * 0.5
        images = np.floor(rs.rand(*shape_i) * 256.0) - 128.0
    elif kind == 'mixed':
        assert case['N'] == 2 and case['T'] == 3
        maps = rs.randn(*shape_m) * 0.5
        images = np.floor(rs.rand(*shape_i) * 256.0) - 128.0
        images[0] += 128.0
        maps[0, 0] = rs.rand(case['h'], case['w'])
        maps[0, 1] = -1.0 - rs.rand(case['h'], case['w'])
        maps[0, 2] = 0.0
    elif kind == 'allneg':
        maps = -rs.rand(*shape_m)
        images = -1.0 - np.floor(rs.rand(*shape_i) * 127.0)
    else:
        raise ValueError('overlay_inputs: unknown kind %r' % (kind,))
    return maps.astype(np.float32), images.astype(np.float32)


def checksum(*arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c & 0xffffffff
