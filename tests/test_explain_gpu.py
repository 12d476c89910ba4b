"""Class attention maps and overlays on the GPU (csrc/apa_explain.hip): apa_attn_explain against the float64 bounds of
tests/_explain_reference.py at the smallest shapes at which the kernel can still go wrong, the reference's own end
points through deploy.FusedHeadEval.explain, apa_attention_overlay against the reference-executed ref_overlay.npz and
the float64 uint8 rule, and a clip batch."""
import json
import os

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy, nets_factory
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _explain_reference as er
from tests._m1_probe import check

pytestmark = pytest.mark.gpu

P = 'USE_POSE_PRELOGITS_BASED_ATTENTION'
EVAL_FIXTURES = ['cfg002_eval', 'cfg002_eval_c2048', 'cfg003_eval', 'relu_eval', 'softmax_eval_c2048',
                 'perclass_softmax_eval']


# ------------------------------------------------------------------------------------------------ apa_attn_explain
def _classes(N, K, T, kind):
    """class 0 and class K-1 on every image's first slots, a repeated class, the rest spread over the classes"""
    rows = []
    for n in range(N):
        base = [0, K - 1, 0, (n + 1) % K, (3 * n + 2) % K, K // 2, (n + 5) % K, K - 1]
        if T == 1:
            base = [(0, K - 1, K // 2)[n % 3]]
        rows.append(base[:T])
    cls = torch.tensor(rows, dtype=torch.int64)
    if kind == 'clamp':             # ids -1 and K: clamped to 0 and K-1, counted
        cls[0, 0], cls[N - 1, T - 1] = -1, K
    return cls


def _inputs(N, Pn, C, K, per_class, seed):
    g = torch.Generator().manual_seed(seed)
    # positive mean and a per-pixel scale: a dropped pixel, chunk or image moves an output by more than its bound
    X = (torch.randn(N, Pn, C, generator=g) + 0.5) * (0.5 + torch.rand(N, Pn, 1, generator=g))
    M = K if per_class else 1
    Wa = torch.randn(C, M, generator=g) / C ** 0.5
    ba = torch.randn(M, generator=g) * 0.1
    Wt = torch.randn(C, K, generator=g) * 0.2 / C ** 0.5 + 1.0 / C      # little cancellation: bound << |topdown|
    bt = torch.randn(K, generator=g) * 0.1
    return X, Wa, ba, Wt, bt


CASES = [
    # N, P, C, K, T, per-class maps, kind
    (3, 15, 36, 7, 1, False, 'plain'),       # channel tail (36 = 9 vectors), odd P
    (3, 15, 36, 7, 3, False, 'plain'),       # classes 0 and K-1, a repeated class
    (5, 1, 64, 3, 3, False, 'plain'),        # one pixel
    (2, 9, 32, 20, 2, True, 'plain'),        # M == K
    (2, 196, 2048, 393, 8, False, 'plain'),  # full channel loop, maximum T, several blocks per image
    (3, 15, 36, 7, 3, False, 'relu'),        # APA_FLAG_RELU_INPUT on inputs with negative entries
    (3, 15, 36, 7, 3, False, 'clamp'),       # class ids -1 and K
]


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%dP%dC%dK%dT%d%s_%s' % (c[0], c[1], c[2], c[3], c[4],
                                                                                '_pc' if c[5] else '', c[6]))
def test_attn_explain_against_float64_bounds(gpu, case, dtype):
    N, Pn, C, K, T, per_class, kind = case
    X, Wa, ba, Wt, bt = _inputs(N, Pn, C, K, per_class, seed=11 * C + K + T)
    relu = kind == 'relu'
    if relu:
        assert float((X < 0).float().mean()) > 0.1
    Xd = X.to(gpu).to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
    Xv = Xd.float()                                             # the values the kernel reads, exactly
    Wad, bad, Wtd, btd = (t.to(gpu) for t in (Wa, ba, Wt, bt))
    # the evaluation step on the same values (fp32 copies of them: it serves every C only in fp32)
    Xs = torch.relu(Xv) if relu else Xv
    st = cof.HeadEvalStep(Xs, Xs, Wad, bad, Wtd, btd)
    st.run()
    cls = _classes(N, K, T, kind)
    flags = cof.APA_FLAG_RELU_INPUT if relu else 0
    td, comb, logit, status = cof.attn_explain(Xd, st.att, Wtd, btd, cls.to(gpu), flags=flags)
    td2, comb2, logit2, status2 = cof.attn_explain(Xd, st.att, Wtd, btd, cls.to(gpu), flags=flags)
    torch.cuda.synchronize()
    for a, b, what in ((td, td2, 'topdown'), (comb, comb2, 'combined'), (logit, logit2, 'class_logit')):
        assert torch.equal(a, b), what + ': two runs differ'
    b_td, b_comb, b_logit, clamped = er.explain_reference(Xv, st.att, Wtd, btd, cls, relu_input=relu)
    assert int(status) == int(status2) == clamped == (2 if kind == 'clamp' else 0)
    assert tuple(td.shape) == (N, T, Pn) and tuple(logit.shape) == (N, T)
    check(td.cpu(), b_td, 'topdown')
    check(comb.cpu(), b_comb, 'combined', zero_ref=True)
    check(logit.cpu(), b_logit, 'class_logit', zero_ref=True)
    if kind == 'clamp':             # equal to the clamped ids' outputs, bit for bit
        t3, c3, l3, s3 = cof.attn_explain(Xd, st.att, Wtd, btd, cls.clamp(0, K - 1).to(gpu), flags=flags)
        assert int(s3) == 0 and torch.equal(t3, td) and torch.equal(c3, comb) and torch.equal(l3, logit)
    # class_logit against the evaluation step's own logits[n,k], within the sum of the two bounds
    b_step = er.eval_logits_reference(Xv, st.att, Wtd, btd, relu_input=relu)
    kc = cls.clamp(0, K - 1)
    got_step = torch.gather(st.logits.cpu().double(), 1, kc)
    step_err = torch.gather(b_step.err, 1, kc)
    assert bool(((got_step - torch.gather(b_step.ref, 1, kc)).abs() <= step_err).all()), 'the step leaves its own bound'
    diff = (logit.cpu().double() - got_step).abs()
    room = b_logit.err + step_err + (b_logit.ref - torch.gather(b_step.ref, 1, kc)).abs()
    assert bool((diff <= room).all()), float((diff - room).max())
    assert float((b_logit.ref - torch.gather(b_step.ref, 1, kc)).abs().max()) <= 1e-12 * max(1.0, float(b_logit.ref.abs().max()))


def test_attn_explain_wrapper_refuses_bad_arguments(gpu):
    X = torch.zeros(2, 9, 32, device=gpu)
    att, Wt, bt = torch.zeros(2, 9, 1, device=gpu), torch.zeros(32, 8, device=gpu), torch.zeros(8, device=gpu)
    cls = torch.zeros(2, 2, dtype=torch.int64, device=gpu)
    with pytest.raises(cof.ApaError):
        cof.attn_explain(X, att, Wt, bt, torch.zeros(2, 9, dtype=torch.int64, device=gpu))       # T = 9
    with pytest.raises(cof.ApaError):
        cof.attn_explain(X, att, Wt, bt, cls, flags=cof.APA_FLAG_TRAIN)
    with pytest.raises(cof.ApaError):
        cof.attn_explain(X, torch.zeros(2, 9, 3, device=gpu), Wt, bt, cls)                       # M not 1 or K
    with pytest.raises(cof.ApaError):
        cof.attn_explain(X, att, Wt, bt, cls.float())
    with pytest.raises(cof.ApaError):
        cof.attn_explain(X.cpu(), att, Wt, bt, cls)


# --------------------------------------------------------------------------- the reference's fixtures, via explain
def _rel(got, exp, floor=1e-30):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(exp).shape)
    exp = np.asarray(exp, dtype=np.float64)
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), floor))


def _bf16_logit_tol(exp_logits):
    """tests/test_reference_fixtures_gpu.py: 3e-3 absolute for logits of order one, scaled down with small logits"""
    return min(3e-3, 0.03 * float(np.abs(exp_logits).max()))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', EVAL_FIXTURES)
def test_explain_reproduces_the_reference_end_points(gpu, name, dtype):
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_%s.npz' % name))
    network_fn, cfg = rf.build_head(fx, device=gpu)
    with torch.no_grad():
        for vn, t in rf.module_tf_names(network_fn).items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).to(gpu))
    bf = dtype == 'bf16'
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu).to(torch.bfloat16 if bf else torch.float32)
    n, hh, ww, _ = images.shape
    K = fx.meta['num_classes']
    ev = deploy.FusedHeadEval(network_fn, cfg)
    scores, pred, _ = ev(images)
    scores, pred = scores.clone(), pred.clone()
    cls = torch.tensor([[0, K - 1, 0]] * n)                      # first, last and a repeated class
    g = torch.Generator().manual_seed(7)
    pics = torch.floor(torch.rand(n, 3 * hh + 1, 2 * ww + 3, 3, generator=g) * 256) - 128
    out = ev.explain(images, classes=cls, input_images=pics.to(gpu))
    torch.cuda.synchronize()
    assert torch.equal(out['scores'], scores) and torch.equal(ev.step.pred, pred)      # what __call__ returns, bit for bit
    assert torch.equal(out['classes'].cpu(), cls) and int(out['status']) == 0
    exp_td = np.asarray(fx.expected('out/ep/TopDownAttention'), dtype=np.float64)      # [n,h,w,K]
    exp_att = np.asarray(fx.expected('out/ep/PosePrelogitsBasedAttention'), dtype=np.float64)
    exp_lg = np.asarray(fx.expected('out/logits'), dtype=np.float64)
    tol = 1.2e-2 if bf else 5e-5       # test_reference_fixtures_gpu.py: these end points, fp32 / bf16 storage rounding
    sel = cls.numpy()
    want_td = np.stack([exp_td[i][:, :, sel[i]].transpose(2, 0, 1) for i in range(n)])
    assert tuple(out['top_down'].shape) == (n, 3, hh, ww) == tuple(out['combined'].shape)
    assert _rel(out['top_down'].cpu().numpy(), want_td) < tol, 'top_down'
    if exp_att.shape[-1] == 1:
        assert tuple(out['bottom_up'].shape) == (n, hh, ww)
        assert _rel(out['bottom_up'].cpu().numpy(), exp_att[..., 0], 1e-6) < tol, 'bottom_up'
        want_bu = np.repeat(exp_att[..., 0][:, None], 3, axis=1)
    else:                                                        # per-class maps: the chosen classes' own
        want_bu = np.stack([exp_att[i][:, :, sel[i]].transpose(2, 0, 1) for i in range(n)])
        assert _rel(out['bottom_up'].cpu().numpy(), want_bu, 1e-6) < tol, 'bottom_up'
    want_lg = np.take_along_axis(exp_lg, sel, axis=1)
    got_lg = out['class_logit'].cpu().numpy()
    if bf:
        assert np.abs(got_lg - want_lg).max() <= _bf16_logit_tol(exp_lg)
    else:
        assert np.abs(got_lg - want_lg).max() <= min(1e-3, 2e-5 * np.abs(exp_lg).max())
    # the product of two maps that are each within tol of their own maximum
    err = np.abs(out['combined'].cpu().numpy().astype(np.float64) - want_bu * want_td).max()
    assert err <= 2.1 * tol * np.abs(want_bu).max() * np.abs(want_td).max(), 'combined'
    # the overlays: shapes and types; their values are held to the reference in the overlay tests below
    ob, oc = out['overlay_bottom_up'], out['overlay_combined']
    assert ob.dtype == oc.dtype == torch.uint8
    assert tuple(oc.shape) == (n, 3, 3 * hh + 1, 2 * ww + 3, 3)
    assert tuple(ob.shape) == (n, 1 if exp_att.shape[-1] == 1 else 3, 3 * hh + 1, 2 * ww + 3, 3)
    v, _ = er.overlay_reference(out['combined'].cpu().numpy(), pics.numpy())
    want_u8, q = er.overlay_u8_reference(v)
    d = np.abs(oc.cpu().numpy().astype(np.int64) - want_u8.astype(np.int64))
    assert int(d[~er.u8_band(q)].max(initial=0)) == 0 and int(d.max(initial=0)) <= 1
    # default classes: the step's own prediction / top-k, no overlay
    top1 = ev.explain(images, overlay=False)
    assert torch.equal(top1['classes'].view(-1), pred) and 'overlay_combined' not in top1
    top3 = ev.explain(images, topk=3, overlay=False)
    assert torch.equal(top3['classes'], torch.topk(scores, 3, dim=1).indices)
    apa_config.reset_cfg()


# ------------------------------------------------------------------------------------------- apa_attention_overlay
def _overlay_cases():
    d = np.load(os.path.join(rf.GOLD, 'ref_overlay.npz'))
    return d, json.loads(str(d['meta']))['cases']


def test_overlay_matches_the_reference_execution(gpu):
    d, cases = _overlay_cases()
    assert {c['branch'] for c in cases} == {'lo<0', 'lo>=0'}                    # both branches of the uint8 rule
    for c in cases:
        maps, images = er.overlay_inputs(c)
        assert er.checksum(maps, images) == c['crc']
        u8, f32 = cof.attention_overlay(torch.from_numpy(maps).to(gpu), torch.from_numpy(images).to(gpu), want_f32=True)
        only = cof.attention_overlay(torch.from_numpy(maps).to(gpu), torch.from_numpy(images).to(gpu))
        assert torch.equal(only, u8) and u8.dtype == torch.uint8
        v, mag = er.overlay_reference(maps, images)
        exp = d['expected/' + c['name']].astype(np.float64)
        over = np.abs(f32.cpu().numpy().astype(np.float64) - exp) - er.overlay_bound(mag)
        print('%s: float overlay worst |err| - bound = %.3g' % (c['name'], float(over.max())))
        assert float(over.max()) <= 0, c['name']
        er.check_u8(u8.cpu().numpy(), v, c['name'])


def test_overlay_of_an_all_zero_image_is_zero(gpu):
    maps = torch.zeros(1, 2, 3, 5, device=gpu)
    images = torch.zeros(1, 13, 17, 3, device=gpu)
    u8, f32 = cof.attention_overlay(maps, images, want_f32=True)
    assert not u8.any() and not f32.any()                                        # s = 0
    want, _ = er.overlay_u8_reference(np.zeros((1, 2, 13, 17, 3)))
    assert np.array_equal(u8.cpu().numpy(), want)


def test_overlay_at_full_image_size(gpu):
    """14x14 -> 448x448, N = T = 1: the full-size index arithmetic"""
    c = dict(N=1, T=1, h=14, w=14, H=448, W=448, kind='meansub', seed=7)
    maps, images = er.overlay_inputs(c)
    u8, f32 = cof.attention_overlay(torch.from_numpy(maps).to(gpu), torch.from_numpy(images).to(gpu), want_f32=True)
    v, mag = er.overlay_reference(maps, images)
    assert float((np.abs(f32.cpu().numpy().astype(np.float64) - v) - er.overlay_bound(mag)).max()) <= 0
    er.check_u8(u8.cpu().numpy(), v, '14x14 -> 448x448')


# ------------------------------------------------------------------------------------------------------ clip batch
def test_explain_on_a_clip_batch(gpu):
    apa_config.reset_cfg()
    cfg = apa_config.cfg_from_dict({'NET': {P: True, P + '_SINGLE_LAYER_ATT': True}, 'TRAIN': {}})
    fn = nets_factory.get_network_fn('resnet_v1_101', 20, 16, cfg, is_training=False, device=gpu, in_channels=32)
    ev = deploy.FusedHeadEval(fn, cfg)
    g = torch.Generator().manual_seed(3)
    clips = torch.relu(torch.randn(2, 3, 4, 4, 32, generator=g)).to(gpu)
    pics = (torch.floor(torch.rand(2, 3, 9, 11, 3, generator=g) * 256) - 128).to(gpu)
    cls = torch.tensor([[4, 19], [0, 7]])
    out = ev.explain(clips, classes=cls, input_images=pics)
    scores = out['scores'].clone()
    assert tuple(scores.shape) == (2, 20)                                        # per clip, as __call__ returns them
    assert tuple(out['bottom_up'].shape) == (6, 4, 4) and tuple(out['top_down'].shape) == (6, 2, 4, 4)
    assert tuple(out['combined'].shape) == (6, 2, 4, 4) and tuple(out['class_logit'].shape) == (6, 2)
    assert tuple(out['overlay_bottom_up'].shape) == (6, 1, 9, 11, 3)
    assert tuple(out['overlay_combined'].shape) == (6, 2, 9, 11, 3)
    rep = cls.repeat_interleave(3, dim=0)
    assert torch.equal(out['classes'].cpu(), rep)                                # a clip's classes, for each frame
    keep = {k: out[k].clone() for k in ('bottom_up', 'top_down', 'combined', 'class_logit', 'overlay_combined')}
    flat = ev.explain(clips.reshape(6, 4, 4, 32), classes=rep, input_images=pics.reshape(6, 9, 11, 3))
    for k, v in keep.items():
        assert torch.equal(flat[k], v), k
    # the frame logits of the step are what class_logit restates (fp32 sums of C = 32 and P = 16 terms on both sides:
    # 1e-4 of the largest logit is two orders above their rounding and far below any wrong pixel or class)
    lg = torch.gather(ev.step.logits, 1, rep.to(gpu))
    assert float((flat['class_logit'] - lg).abs().max()) <= 1e-4 * max(1.0, float(lg.abs().max()))
    # default classes on clips: the clip's prediction, for each of its frames
    top1 = ev.explain(clips, overlay=False)
    assert torch.equal(top1['classes'].view(-1), ev.step.pred.repeat_interleave(3))
    with pytest.raises(ValueError, match='rows of classes'):
        ev.explain(clips, classes=rep, overlay=False)
    apa_config.reset_cfg()
