"""Class attention maps and overlays on the GPU (csrc/apa_explain.hip): apa_attn_explain against the float64 bounds of
tests/_explain_reference.py at the smallest shapes at which the kernel can still go wrong, the reference's own end
points through deploy.FusedHeadEval.explain, apa_attention_overlay against the reference-executed ref_overlay.npz and
the float64 uint8 rule, and a clip batch.  CASES launches every instance of explain_main_kernel and every trip of its
loops (asserted from the plan probe, tests/_explain_probe.py); OVERLAY_EDGE_CASES are the overlay's edges.  The checker
itself is held to account without a GPU in tests/test_explain_paths_cpu.py."""
import json
import os

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy, nets_factory
from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from tests import _explain_probe as xp
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


# Per-channel factors (powers of two, by their exponents) on the channels of the last, partial 256-channel stretch of a
# row, for the channel-round cases, by C alone.  A wide row's sum hides one 4- or 8-channel load vector of flat inputs
# inside its bound at some elements (the vector's signed terms cancel there, whatever common factor they carry).  These
# exponents were searched on the float64 reference alone so that losing ANY one vector of that stretch moves EVERY
# output element past its bound, in both dtypes (tests/test_explain_paths_cpu.py asserts it on these very inputs); the
# stretch then carries at most half of a row's magnitude, so the other channels still count.
TAIL_EXPONENTS = {
    264: (5, 2, 3, 7, 6, 5, 6, 2),
    516: (7, 2, 7, 6),
    1028: (7, 3, 7, 5),
    1032: (2, 4, 7, 2, 2, 4, 7, 7),
    2056: (7, 5, 6, 7, 6, 4, 6, 5),
}


def _tail_start(C):
    """first channel of the scaled stretch (None: C has none).  It holds the last, partial round of the channel loop --
    or, where one round covers the row, its last, partly filled vector slot -- in every load form: a round is
    64 * EPV * U = 512, 1024 or 2048 channels, a slot 256 or 512."""
    if C not in TAIL_EXPONENTS:
        return None
    assert C - C // 256 * 256 == len(TAIL_EXPONENTS[C])
    return C // 256 * 256


def _inputs(N, Pn, C, K, per_class, seed):
    g = torch.Generator().manual_seed(seed)
    # positive mean and a per-pixel scale: a dropped pixel, chunk or image moves an output by more than its bound
    X = (torch.randn(N, Pn, C, generator=g) + 0.5) * (0.5 + torch.rand(N, Pn, 1, generator=g))
    if _tail_start(C) is not None:
        X[:, :, _tail_start(C):] *= 2.0 ** torch.tensor(TAIL_EXPONENTS[C], dtype=torch.float32)
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
]                                            # (tests/test_graph_replay_gpu.py reads CASES[6]: append, never reorder)

# Every instance of explain_main_kernel<T, EPV, TT> and every trip of its loops ("Which test
# reaches which instance"; test_cases_reach_every_instance_and_trip below asserts what each line claims, from the plan
# probe).  Both dtypes run every case; the evaluation step serves all of them in fp32, so none skips the comparison
# with the step's logits.
# Instance sweep: C = 36 is fp32 and bf16 / 8-byte loads, C = 40 bf16 / 16-byte loads; S = 3, 5 pixels per block: a short
# last group under every PIX (4, 3 and 2 pixels a wave)
CASES += [(3, 15, C, 9, T, False, 'plain') for C in (36, 40) for T in range(1, 9)]
CASES += [
    # the wave-stride group loop, second and third trip: S = 1 and 19 pixels: 5, 7 and 10 groups per block ...
    (400, 19, 32, 5, 4, False, 'plain'),
    (400, 19, 32, 5, 5, False, 'plain'),
    (400, 19, 32, 5, 8, False, 'plain'),
    # ... S = 5 and unequal ranges of 20 or 21 pixels: 6, 7 and 11 groups; P = 103: the finish kernel's second trip
    (100, 103, 32, 5, 4, False, 'plain'),
    (100, 103, 32, 5, 5, False, 'plain'),
    (100, 103, 32, 5, 8, False, 'plain'),
    # ... and a third trip under PIX = 4 and PIX = 3 as well: S = 1 and 35 pixels: 9 groups (the last of 3 pixels) and
    # 12 groups (the last of 2)
    (400, 35, 8, 5, 4, False, 'plain'),
    (400, 35, 8, 5, 5, False, 'plain'),
    # channel rounds (the channels from _tail_start(C) on are scaled, see _inputs)
    (2, 9, 264, 6, 3, False, 'plain'),       # fp32: the second of U = 2 vector slots partly filled
    (2, 9, 516, 6, 5, False, 'plain'),       # fp32, bf16 / 8 B at U = 2: ragged second round; the gather kernel's C > 256 tail
    (2, 9, 1028, 6, 6, False, 'plain'),      # the same at U = 4: slot 0 of the second round partly filled, slots 1..3 past C
    (2, 9, 1032, 6, 4, False, 'plain'),      # bf16 / 16 B at U = 2 (fp32: a third round)
    (2, 9, 2056, 6, 6, False, 'plain'),      # bf16 / 16 B at U = 4; 48 KiB of LDS
    # the LDS-size halving of S: 3 -> 2, ranges of 7 and 8 pixels, PIX = 3
    (3, 15, 1028, 7, 5, False, 'plain'),
    # per-class maps (M == K) at the other geometries, and with clamped ids: att is read at the clamped class
    (2, 9, 32, 20, 8, True, 'plain'),
    (2, 9, 32, 20, 5, True, 'clamp'),
    # relu input under PIX = 3 and PIX = 2
    (3, 15, 36, 7, 5, False, 'relu'),
    (3, 15, 36, 7, 7, False, 'relu'),
]
assert len(set(CASES)) == len(CASES)


def _ratio(got, b):
    """worst |got - ref| / bound (elements with a zero bound: 0 when equal)"""
    d = (got.double().reshape(b.ref.shape) - b.ref).abs()
    exact = torch.where(d > 0, torch.full_like(d, float('inf')), torch.zeros_like(d))
    return float(torch.where(b.err > 0, d / b.err.clamp_min(1e-300), exact).max())


def coverage():
    """what CASES x dtypes reach, from the plan probe (host only): the (form, TT) instances, per PIX the most trips of the
    group loop, the (form, U) pairs with a ragged second channel round, and the (halved?, S > 1) split forms"""
    inst, trips, ragged, splits = set(), {}, set(), set()
    for N, Pn, C, K, T, _, _ in CASES:
        for dtype in ('fp32', 'bf16'):
            pl = xp.plan(N, Pn, C, K, T, dtype)
            inst.add((xp.form(pl, dtype), T))
            trips[pl.PIX] = max(trips.get(pl.PIX, 0), xp.trips(pl))
            if xp.ragged_second_round(pl, C):
                ragged.add((xp.form(pl, dtype), pl.U))
            if pl.S > 1:
                splits.add('halved' if pl.S < pl.S_m1 else 'unhalved')
    return inst, trips, ragged, splits


def test_cases_reach_every_instance_and_trip():
    """host only (no launch): kept beside the table it speaks about; tests/test_explain_paths_cpu.py runs it without a
    GPU too"""
    inst, trips, ragged, splits = coverage()
    forms = ('fp32', 'bf16/16B', 'bf16/8B')
    assert inst == {(f, t) for f in forms for t in range(1, 9)}, sorted({(f, t) for f in forms for t in range(1, 9)} - inst)
    assert set(trips) == {4, 3, 2} and all(v >= 3 for v in trips.values()), trips
    assert ragged == {(f, u) for f in forms for u in (2, 4)}, ragged
    assert splits == {'halved', 'unhalved'}
    print('instances %d/24, group-loop trips per PIX %s' % (len(inst), trips))


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
    print('worst |err| / bound: topdown %.3f combined %.3f class_logit %.3f' % (
        _ratio(td.cpu(), b_td), _ratio(comb.cpu(), b_comb), _ratio(logit.cpu(), b_logit)))
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


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_explain_topk_5_and_8_through_the_product_layer(gpu, dtype):
    """the documented top-5 use (PIX = 3, the instance tools/bench_dense.py times) and the maximum, with overlays"""
    fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_eval.npz'))
    network_fn, cfg = rf.build_head(fx, device=gpu)
    with torch.no_grad():
        for vn, t in rf.module_tf_names(network_fn).items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).to(gpu))
    bf = dtype == 'bf16'
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu).to(torch.bfloat16 if bf else torch.float32)
    n, hh, ww, _ = images.shape
    exp_lg = np.asarray(fx.expected('out/logits'), dtype=np.float64)
    tol = _bf16_logit_tol(exp_lg) if bf else min(1e-3, 2e-5 * np.abs(exp_lg).max())     # the fixture test's, above
    g = torch.Generator().manual_seed(9)
    pics = torch.floor(torch.rand(n, 2 * hh + 1, 3 * ww + 2, 3, generator=g) * 256) - 128
    ev = deploy.FusedHeadEval(network_fn, cfg)
    for topk in (5, 8):
        out = ev.explain(images, topk=topk, input_images=pics.to(gpu))
        torch.cuda.synchronize()
        assert int(out['status']) == 0
        assert torch.equal(out['classes'], torch.topk(out['scores'], topk, dim=1).indices)
        assert tuple(out['top_down'].shape) == (n, topk, hh, ww) == tuple(out['combined'].shape)
        want = torch.gather(ev.step.logits, 1, out['classes'])
        worst = float((out['class_logit'] - want).abs().max())
        print('topk=%d: class_logit against the step worst %.3g (tolerance %.3g)' % (topk, worst, tol))
        assert worst <= tol
        oc = out['overlay_combined']
        assert oc.dtype == torch.uint8 and tuple(oc.shape) == (n, topk, 2 * hh + 1, 3 * ww + 2, 3)
        assert tuple(out['overlay_bottom_up'].shape) == (n, 1, 2 * hh + 1, 3 * ww + 2, 3)
        v, _ = er.overlay_reference(out['combined'].cpu().numpy(), pics.numpy())
        want_u8, q = er.overlay_u8_reference(v)
        d = np.abs(oc.cpu().numpy().astype(np.int64) - want_u8.astype(np.int64))
        assert int(d[~er.u8_band(q)].max(initial=0)) == 0 and int(d.max(initial=0)) <= 1
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


def _overlay_float_only(maps, images):
    """apa_attention_overlay with overlay_u8 = NULL and no workspace: one launch, no min / max pass"""
    N, T, h, w = maps.shape
    H, W = images.shape[1:3]
    f32 = torch.empty((N, T, H, W, 3), dtype=torch.float32, device=maps.device)
    lib = cof.load_library()
    cof._check(lib.apa_attention_overlay(cof._dev_ptr(maps, 'maps', torch.float32), cof._dev_ptr(images, 'images', torch.float32),
                                         f32.data_ptr(), None, None, 0, N, T, h, w, H, W, cof._stream_ptr()),
               'apa_attention_overlay')
    return f32


@pytest.mark.parametrize('case', er.OVERLAY_EDGE_CASES, ids=lambda c: c['name'])
def test_overlay_edges(gpu, case):
    """downscale, identity, maps and images of one row or column (every tap clamps), (n,t) images of one call on
    different branches of the uint8 rule, hi < 0, lo == 0 exactly, a ragged second trip of the pixel loop -- each as
    test_overlay_at_full_image_size checks its case; and the float-only form, bit-equal to the pair form's float output.
    The conditions on the inputs (band share, branch safety) are tests/test_explain_paths_cpu.py's to assert."""
    maps, images = er.overlay_inputs(case)
    md, im = torch.from_numpy(maps).to(gpu), torch.from_numpy(images).to(gpu)
    u8, f32 = cof.attention_overlay(md, im, want_f32=True)
    v, mag = er.overlay_reference(maps, images)
    assert tuple(f32.shape) == v.shape == tuple(u8.shape)
    err, bound = np.abs(f32.cpu().numpy().astype(np.float64) - v), er.overlay_bound(mag)
    print('%s: float overlay worst |err| / bound %.3f' % (case['name'], float((err / np.maximum(bound, 1e-300)).max())))
    assert float((err - bound).max()) <= 0
    er.check_u8(u8.cpu().numpy(), v, case['name'])
    if case['kind'] == 'mixed':
        lo = v.reshape(case['N'], case['T'], -1).min(-1)
        assert (lo[0] < 0).tolist() == [False, True, False] and bool((lo[1] < 0).all())
    only = _overlay_float_only(md, im)
    torch.cuda.synchronize()
    assert torch.equal(only, f32), 'the float-only form differs from the pair form'


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
