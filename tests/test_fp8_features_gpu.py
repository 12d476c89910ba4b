"""The FP8 (E4M3) feature cache on the GPU: the device's decode and encode bit for bit against torch.float8_e4m3fn and
the CPU restatement of the quantisation rule; the two FP8 streaming kernels (apa_m1_fp8.hip) against float64; the
frozen contract; the one-call steps against their separate calls; deploy.FusedHeadStep / FusedHeadEval on an
Fp8Features batch.

Float64 reference of the kernel tests: oracle.attn_pool_oracle on the DEQUANTISED input (scale[n] * decode(code), exact
in float64) with the dropout mask replayed from apa_dropout_mask.  Tolerance: the error model tests/test_m1_paths_gpu.py
holds the bf16 arms to (tests/_m1_probe.py: fp32 accumulation of exactly representable inputs, C_ACC (L + 8) 2^-24 per
contraction, propagated) -- its reference formulas are first tied to the oracle's own outputs and autograd gradients
in float64, then the kernels' outputs are held to its bounds."""
import os

import numpy as np
import pytest
import torch

from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
from oracle import attn_pool_oracle as orc
from tests import _m1_probe as mp
from tests import _ref_fixture as rf
from tests import test_m1_paths_gpu as m1p

pytestmark = pytest.mark.gpu

F8 = torch.float8_e4m3fn
KEEP, SEED, OFFSET = 0.5, 1234, 7
# (N, H, W, C, K): one vector per row; C no power of two and P prime (the split tail); wide; the fused-loss route
SHAPES = [(2, 3, 3, 16, 8), (3, 1, 7, 48, 5), (5, 2, 2, 2048, 8), (2, 3, 3, 2048, 393)]
MAGNITUDES = (1.0, 37.0, 1e-3)      # per image: a wrong or swapped scale[n] cannot pass


# ------------------------------------------------------------------------------------------ decode / encode
def test_device_decode_is_torch_e4m3fn(gpu):
    codes = torch.arange(256, dtype=torch.uint8)
    f = cof.Fp8Features.from_parts(codes.view(1, 1, 256).to(gpu), torch.ones(1, device=gpu))
    got = f.dequantize(torch.float32).cpu().reshape(256)
    want = codes.view(F8).to(torch.float32)
    finite = torch.ones(256, dtype=torch.bool)
    finite[0x7F] = finite[0xFF] = False
    assert torch.isfinite(want[finite]).all() and int(finite.sum()) == 254
    assert torch.equal(got[finite].view(torch.int32), want[finite].view(torch.int32))       # bit-equal, -0 included
    assert torch.isnan(got[0x7F]) and torch.isnan(got[0xFF])
    # the scale is applied per image, and a bf16 destination rounds once
    g = cof.Fp8Features.from_parts(codes[:112].view(1, 7, 16).repeat(2, 1, 1).to(gpu), torch.tensor([0.75, 3.0], device=gpu))
    w = codes[:112].view(F8).to(torch.float32).view(1, 7, 16) * torch.tensor([0.75, 3.0]).view(2, 1, 1)
    assert torch.equal(g.dequantize().cpu(), w) and torch.equal(g.dequantize(torch.bfloat16).cpu(), w.to(torch.bfloat16))


def _encode_probe_image():
    """448 (so amax = 448 and both scales are exactly 1), every finite E4M3 value, every midpoint between neighbouring
    values (the ties) and the fp32 neighbours of each midpoint on both sides; [1, 4, 256] float32."""
    allc = torch.arange(256, dtype=torch.uint8)
    vals = allc.view(F8).to(torch.float32)
    vals = vals[torch.isfinite(vals)]
    pos = torch.unique(vals[vals >= 0])                     # sorted: 0, 2^-9, ..., 448
    assert pos.numel() == 127 and float(pos[-1]) == 448.0
    mid = ((pos[:-1].double() + pos[1:].double()) / 2).to(torch.float32)
    assert torch.equal(mid.double(), (pos[:-1].double() + pos[1:].double()) / 2)            # exact in fp32
    inf = torch.tensor(float('inf'))
    parts = [vals, mid, -mid, torch.nextafter(mid, inf), torch.nextafter(mid, -inf),
             -torch.nextafter(mid, inf), -torch.nextafter(mid, -inf)]
    x = torch.cat(parts)
    assert x.numel() <= 1024 and float(x.abs().max()) == 448.0
    x = torch.cat([x, torch.full((1024 - x.numel(),), 448.0)])
    return x.view(1, 4, 256)


def _same_cache(dev_f, dev_status, cpu_f, cpu_status):
    assert torch.equal(dev_f.codes.view(torch.uint8).cpu(), cpu_f.codes.view(torch.uint8)), 'codes'
    assert torch.equal(dev_f.scale.cpu().view(torch.int32), cpu_f.scale.view(torch.int32)), 'scales'
    assert torch.equal(dev_status.cpu(), cpu_status), 'status'


def test_device_encode_is_the_cpu_rule(gpu):
    x = _encode_probe_image()
    fd, sd = cof.quantize_features(x.to(gpu))
    fc, sc = cof.quantize_features(x)
    assert float(fc.scale[0]) == 1.0 and sc.tolist() == [0]
    _same_cache(fd, sd, fc, sc)
    # three seeded relu(randn) images, one of them all zero; then one with a non-finite value; then a bf16 source
    g = torch.Generator().manual_seed(11)
    y = torch.relu(torch.randn(3, 5, 32, generator=g)) * torch.tensor(MAGNITUDES).view(3, 1, 1)
    y[1] = 0.0
    _same_cache(*cof.quantize_features(y.to(gpu)), *cof.quantize_features(y))
    z = y.clone()
    z[2, 4, 31] = float('nan')
    fd, sd = cof.quantize_features(z.to(gpu))
    assert sd.tolist() == [0, 0, 1]
    _same_cache(fd, sd, *cof.quantize_features(z))
    yb = (torch.randn(3, 5, 32, generator=g) * torch.tensor(MAGNITUDES).view(3, 1, 1)).to(torch.bfloat16)
    _same_cache(*cof.quantize_features(yb.to(gpu)), *cof.quantize_features(yb))
    # two calls are bit-identical
    assert torch.equal(cof.quantize_features(y.to(gpu))[0].buffer, cof.quantize_features(y.to(gpu))[0].buffer)


# ------------------------------------------------------------------------------------------ kernels against float64
def _case(shape, act, train, entry='sep'):
    N, H, W, C, K = shape
    return dict(name='fp8_%dx%dx%dx%d_k%d_%s_%s' % (N, H, W, C, K, act, 'train' if train else 'eval'), N=N, P=H * W,
                H=H, W=W, C=C, K=K, J=0, Ca=None, act=act, train=train, keep=KEEP, rank1=False, relu_in=False,
                dt=cof.APA_DTYPE_FP8_E4M3, entry=entry)


_INPUTS = {}


def _inputs(c, dev):
    """the quantised batch, its exact float64 dequantisation and the head's parameters (computed once per shape and
    activation, shared, never written)"""
    key = (c['N'], c['H'], c['W'], c['C'], c['K'], c['act'])
    if key in _INPUTS:
        return _INPUTS[key]
    N, H, W, C, K = key[:5]
    g = torch.Generator().manual_seed(1000 + sum(key[:5]) + len(c['act']))
    u = lambda *s: torch.rand(s, generator=g) * 1.25 - 0.25
    mag = torch.tensor([MAGNITUDES[n % 3] for n in range(N)]).view(N, 1, 1, 1)
    rows = 0.25 + 1.5 * torch.rand((N, H, W, 1), generator=g)              # a per-pixel scale (tests/test_m1_paths_gpu.py)
    img = torch.relu(torch.randn(N, H, W, C, generator=g)) * rows * mag
    f8, status = cof.quantize_features(img.to(dev))
    assert status.tolist() == [0] * N
    X64 = (f8.codes.cpu().to(torch.float32).double() * f8.scale.cpu().double().view(N, 1, 1, 1)).to(dev)
    Wa = u(C) * (4.0 / C)
    if c['act'] == 'relu':     # the unit-magnitude images gate both ways around their mean pixel
        unit = [n for n in range(N) if n % 3 == 0]
        ba = -(X64[unit].float().cpu().mean(dim=(0, 1, 2)) @ Wa).reshape(1)
    else:
        ba = u(1) * 0.1
    inp = dict(f8=f8, X=X64.view(N, H * W, C), Wa=Wa.to(dev), ba=ba.to(dev), Wt=(u(C, K) / C ** 0.5).to(dev),
               bt=(u(K) * 0.1).to(dev), G=(u(N, K) / N).to(dev),
               labels=torch.randint(0, K, (N,), generator=g).to(dev), Xext=None)
    inp['Xatt'] = inp['X']
    _INPUTS[key] = inp
    return inp


def _flags(c):
    return (cof.APA_FLAG_RELU_ATT if c['act'] == 'relu' else 0) | (cof.APA_FLAG_TRAIN if c['train'] else 0)


def _run_separate(c, inp, G=None, workspace=None):
    f8 = inp['f8'].flat()
    Wa = inp['Wa'].view(-1, 1)
    kw = dict(flags=_flags(c), keep_prob=KEEP, seed=SEED, offset=OFFSET)
    logits, att, zsave, abar, _, ws = cof.attn_pool_fwd(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], workspace=workspace, **kw)
    got = dict(logits=logits, att=att, zsave=zsave, abar=abar)
    if G is None:
        loss, G, _, _ = cof.softmax_xent_fwd_bwd(logits, inp['labels'])
        got['loss'] = loss
    got['G'] = G
    dX, dXatt, got['dWa'], got['dba'], got['dWt'], got['dbt'] = cof.attn_pool_bwd(
        f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], att, zsave, abar, G, workspace=ws, want_dx=False, **kw)
    assert dX is None and dXatt is None
    return got


def _oracle_ties(c, inp, mask, ref_f):
    """the error model's reference formulas are the oracle's: forward outputs, and -- on the oracle's own att / zsave /
    abar -- the autograd gradients, in float64"""
    N, H, W, C, K = c['N'], c['H'], c['W'], c['C'], c['K']
    leaf = lambda t: t.double().clone().requires_grad_(True)
    Wa, ba, Wt, bt = leaf(inp['Wa'].view(C, 1)), leaf(inp['ba']), leaf(inp['Wt']), leaf(inp['bt'])
    X = inp['X'].view(N, H, W, C)
    m = None if mask is None else mask.view(N, H, W, C)
    logits, ep = orc.attentional_pooling(X, None, None, [Wa], [ba], [Wt], [bt],
                                         orc.AttnFlags(single_layer_att=True, relu_att=c['act'] == 'relu'),
                                         is_training=c['train'], keep_prob=KEEP, dropout_mask=m)
    att = ep['PosePrelogitsBasedAttention'].detach().reshape(N, H * W)
    close = lambda a, b, what: torch.testing.assert_close(a.reshape(b.shape), b, rtol=0, atol=1e-11 * float(b.abs().max()) + 1e-300, msg=what)
    close(logits.detach(), ref_f['logits'].ref, 'oracle logits')
    close(att, ref_f['att'].ref, 'oracle att')
    (logits * inp['G'].double()).sum().backward()
    Xt = X if m is None else X * m.double() / KEEP
    zs = (att.view(N, H, W, 1) * Xt).mean(dim=(1, 2))
    ref_b = m1p._backward_ref(c, inp, dict(att=att, zsave=zs, abar=att.mean(dim=1), G=inp['G']), mask)
    for k, gr in (('dWa', Wa.grad), ('dba', ba.grad), ('dWt', Wt.grad), ('dbt', bt.grad)):
        close(gr, ref_b[k].ref, 'oracle ' + k)


def _check_against_float64(c, inp, got, mask, cancels=False):
    ref_f, amb = m1p._forward_ref(c, inp, mask)
    mp.check(got['att'], ref_f['att'], 'att', ambiguous=amb)
    for k in ('zsave', 'abar', 'logits'):
        mp.check(got[k], ref_f[k], k)
    if 'dWt' not in got:
        return
    ref_b = m1p._backward_ref(c, inp, got, mask)
    mp.check(got['dWa'], ref_b['dWa'], 'dWa', zero_ref=cancels)
    mp.check(got['dba'], ref_b['dba'], 'dba', zero_ref=cancels)
    mp.check(got['dWt'], ref_b['dWt'], 'dWt')
    mp.check(got['dbt'], ref_b['dbt'], 'dbt')


FP32_TINY = 2.0 ** -126     # the smallest normal fp32: a probability below it may be stored as 0


def _check_loss(c, got, inp):
    """loss / G (training step) or probs / pred (evaluation step) from the kernel's own logits: the bounds of
    tests/test_m1_paths_gpu.py _check_loss, plus fp32's underflow threshold on a probability -- the x37 image spreads
    its logits far enough for exp(l - max) to leave the fp32 range, which a relative bound alone does not allow."""
    N, K = c['N'], c['K']
    lg = got['logits'].double().reshape(N, K)
    p = torch.softmax(lg, dim=1)
    tol = mp.C_ACC * (K + 16) * mp.EPS32
    if c['entry'] == 'eval':
        mp.check(got['probs'], mp.Bnd(p, tol * p + FP32_TINY), 'probs')
        assert torch.equal(got['pred'], lg.argmax(dim=1)), 'pred'
        return
    lab = inp['labels']
    onehot = torch.nn.functional.one_hot(lab, K).double()
    mp.check(got['G'], mp.Bnd((p - onehot) / N, (tol * (p + onehot) + FP32_TINY) / N), 'G')
    lse = torch.logsumexp(lg, dim=1)
    per = lse - lg.gather(1, lab[:, None])[:, 0]
    mag = lse.abs() + lg.abs().amax(dim=1)
    loss = got['loss'].double().reshape(N + 1)
    mp.check(loss[1:], mp.Bnd(per, tol * mag), 'loss per example')
    mp.check(loss[:1], mp.Bnd(per.mean().reshape(1), (tol * mag).mean().reshape(1) + tol * per.abs().mean()), 'loss')


def _mask(c, dev):
    if not c['train']:
        return None
    return cof.dropout_mask((c['N'] * c['P'] * c['C'],), KEEP, SEED, OFFSET)


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('act', ['id', 'relu'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fp8_kernels_against_float64(gpu, shape, act, train):
    c = _case(shape, act, train)
    inp = _inputs(c, gpu)
    mask = _mask(c, gpu)
    _oracle_ties(c, inp, mask, m1p._forward_ref(c, inp, mask)[0])
    got = _run_separate(c, inp, G=inp['G'])
    _check_against_float64(c, inp, got, mask)
    if shape[3] == 2048 and shape[4] == 393:
        # the fused-loss route: the one-call step (training) / the evaluation step, whose logits reducer carries the
        # row's cross-entropy / probabilities; loss, G, probs and pred from the kernel's own logits
        cs = dict(c, entry='step' if train else 'eval')
        st = _one_call(cs, inp)
        got = {k: getattr(st, k) for k in ('logits', 'att', 'zsave', 'abar')}
        if train:
            got.update(G=st.G, loss=st.loss, dWa=st.grads[2], dba=st.grads[3], dWt=st.grads[4], dbt=st.grads[5])
        else:
            got.update(probs=st.probs, pred=st.pred)
        _check_against_float64(cs, inp, got, mask, cancels=True)
        _check_loss(cs, got, inp)


# ------------------------------------------------------------------------------------------ frozen contract
def test_frozen_contract(gpu):
    c = _case(SHAPES[2], 'relu', True)
    inp = _inputs(c, gpu)
    N, P, C, K = c['N'], c['P'], c['C'], c['K']
    f8 = inp['f8'].flat()
    Wa = inp['Wa'].view(-1, 1)
    lib = cof.load_library()
    need = cof.attn_pool_workspace_bytes(N, P, C, C, K, 1, _flags(c))
    # a sentinel-filled buffer on either side of the workspace
    pad = 4096
    arena = torch.full((need + 2 * pad,), 0xA5, dtype=torch.uint8, device=gpu)
    ws = arena[pad:pad + need]
    got = _run_separate(c, inp, G=inp['G'], workspace=ws)
    torch.cuda.synchronize()
    assert bool((arena[:pad] == 0xA5).all()) and bool((arena[pad + need:] == 0xA5).all())
    # two identical calls: every output bit for bit
    again = _run_separate(c, inp, G=inp['G'], workspace=ws)
    for k, v in got.items():
        assert torch.equal(v, again[k]), k
    # a backward call with a real dX, or without the flag: a cache has no gradient
    dX = torch.empty((N, P, C), dtype=torch.uint8, device=gpu)
    outs = [torch.empty_like(t) for t in (Wa, inp['ba'], inp['Wt'], inp['bt'])]

    def bwd(dx, flags):
        return lib.apa_attn_pool_bwd(f8.data_ptr(), f8.data_ptr(), Wa.data_ptr(), inp['ba'].data_ptr(),
                                     inp['Wt'].data_ptr(), inp['bt'].data_ptr(), got['att'].data_ptr(),
                                     got['zsave'].data_ptr(), got['abar'].data_ptr(), inp['G'].data_ptr(), dx, None,
                                     *[o.data_ptr() for o in outs], ws.data_ptr(), ws.numel(), N, P, C, C, K, 1,
                                     flags, KEEP, SEED, OFFSET, cof.APA_DTYPE_FP8_E4M3, None)
    assert bwd(dX.data_ptr(), _flags(c) | cof.APA_FLAG_FROZEN_INPUT) == -1 and b'no gradient' in lib.apa_last_error()
    assert bwd(dX.data_ptr(), _flags(c)) == -1 and b'no gradient' in lib.apa_last_error()
    with pytest.raises(cof.ApaError):
        cof.HeadTrainStep(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], inp['labels'], (dX, None, *outs))


# ------------------------------------------------------------------------------------------ one call == separate calls
class _Step(object):
    pass


def _one_call(c, inp, frames=1, temporal=None, action_loss='softmax-xentropy', labels=None):
    f8 = inp['f8'].flat()
    Wa = inp['Wa'].view(-1, 1)
    labels = inp['labels'] if labels is None else labels
    if c['entry'] == 'eval':
        st = cof.HeadEvalStep(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], flags=_flags(c), frames=frames,
                              temporal=temporal)
        st.run()
        return st
    grads = (None, None) + tuple(torch.empty_like(t) for t in (Wa, inp['ba'], inp['Wt'], inp['bt']))
    tg = None if temporal is None else tuple(torch.empty_like(t) for t in temporal)
    st = cof.HeadTrainStep(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], labels, grads, flags=_flags(c), keep_prob=KEEP,
                           seed=SEED, offset=OFFSET, frames=frames, temporal=temporal, temporal_grads=tg,
                           action_loss=action_loss)
    st.run()
    st.grads, st.temporal_grads = grads, tg
    assert st.frozen_input and st.dX_scratch is None
    return st


@pytest.mark.parametrize('shape', [SHAPES[3], SHAPES[1]], ids=lambda s: 'x'.join(map(str, s)))
def test_one_call_steps_equal_separate_calls(gpu, shape):
    c = _case(shape, 'relu', True, entry='step')
    inp = _inputs(c, gpu)
    sep = _run_separate(c, inp)
    st = _one_call(c, inp)
    for k in ('logits', 'att', 'zsave', 'abar', 'loss', 'G'):
        assert torch.equal(getattr(st, k).reshape(sep[k].shape), sep[k]), k
    for k, g in zip(('dWa', 'dba', 'dWt', 'dbt'), st.grads[2:]):
        assert torch.equal(g, sep[k]), k
    # evaluation: scores and predictions
    ce = _case(shape, 'relu', False, entry='eval')
    ev = _one_call(ce, inp)
    f8 = inp['f8'].flat()
    logits, att, _, _, _, _ = cof.attn_pool_fwd(f8, f8, inp['Wa'].view(-1, 1), inp['ba'], inp['Wt'], inp['bt'],
                                                flags=_flags(ce))
    _, _, probs, pred = cof.softmax_xent_fwd_bwd(logits, inp['labels'], want_grad=False, want_probs=True, want_pred=True)
    assert torch.equal(ev.logits, logits) and torch.equal(ev.att, att)
    assert torch.equal(ev.probs, probs) and torch.equal(ev.pred, pred)
    # rebind to another cache of the same shape, and back
    other, _ = cof.quantize_features(inp['f8'].dequantize() * 0.5)
    st.rebind(X=other.flat())
    st.run()
    assert not torch.equal(st.logits, sep['logits'])
    st.rebind(X=f8)
    st.run()
    assert torch.equal(st.logits, sep['logits'])


def test_clip_and_multilabel_steps_equal_separate_calls(gpu):
    """B = 2 clips of F = 2 frames with temporal attention, and one multi-label case (K = 8): the same M1Call serves
    them (apa_attn_head_train_step_clips / _multilabel, apa_attn_head_eval_step_clips)"""
    shape = (4, 2, 2, 2048, 8)
    c = _case(shape, 'id', True, entry='step')
    inp = _inputs(c, gpu)
    K = c['K']
    g = torch.Generator().manual_seed(5)
    tw, tb = (torch.rand(K, generator=g) - 0.5).to(gpu), torch.full((1,), 0.5, device=gpu)
    clip_labels = torch.tensor([3, 6], device=gpu)
    st = _one_call(c, inp, frames=2, temporal=(tw, tb), labels=clip_labels)
    f8 = inp['f8'].flat()
    Wa = inp['Wa'].view(-1, 1)
    kw = dict(flags=_flags(c), keep_prob=KEEP, seed=SEED, offset=OFFSET)
    logits, att, zsave, abar, _, ws = cof.attn_pool_fwd(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], **kw)
    pooled, tatt, loss, G, dw, db = cof.clip_xent_fwd_bwd(logits, clip_labels, 2, tw, tb)
    _, _, dWa, dba, dWt, dbt = cof.attn_pool_bwd(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], att, zsave, abar, G,
                                                 workspace=ws, want_dx=False, **kw)
    for a, b, what in ((st.logits, logits, 'logits'), (st.pooled, pooled, 'pooled'), (st.tatt, tatt, 'tatt'),
                       (st.loss, loss, 'loss'), (st.G, G, 'G'), (st.temporal_grads[0], dw, 'dw'),
                       (st.temporal_grads[1], db, 'db'), (st.grads[2], dWa, 'dWa'), (st.grads[3], dba, 'dba'),
                       (st.grads[4], dWt, 'dWt'), (st.grads[5], dbt, 'dbt')):
        assert torch.equal(a.reshape(b.shape), b), what
    # the clip evaluation step
    ce = _case(shape, 'id', False, entry='eval')
    ev = _one_call(ce, inp, frames=2, temporal=(tw, tb))
    elog = cof.attn_pool_fwd(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], flags=_flags(ce))[0]
    pooled, tatt, scores, pred, _ = cof.clip_scores(elog, 2, tw, tb)
    assert torch.equal(ev.logits, elog) and torch.equal(ev.pooled, pooled) and torch.equal(ev.tatt, tatt)
    assert torch.equal(ev.probs, scores) and torch.equal(ev.pred, pred)
    # multi-label, flat
    ml = (torch.rand(c['N'], K, generator=g) < 0.3).to(torch.float32).to(gpu)
    sm = _one_call(c, inp, action_loss='multi-label', labels=ml)
    loss, G = cof.multilabel_loss_fwd_bwd('multi-label', logits, ml)
    _, _, dWa, dba, dWt, dbt = cof.attn_pool_bwd(f8, f8, Wa, inp['ba'], inp['Wt'], inp['bt'], att, zsave, abar, G,
                                                 workspace=ws, want_dx=False, **kw)
    for a, b, what in ((sm.logits, logits, 'logits'), (sm.loss, loss, 'loss'), (sm.G, G, 'G'), (sm.grads[2], dWa, 'dWa'),
                       (sm.grads[3], dba, 'dba'), (sm.grads[4], dWt, 'dWt'), (sm.grads[5], dbt, 'dbt')):
        assert torch.equal(a.reshape(b.shape), b), what


# ------------------------------------------------------------------------------------------ deploy
FP32_VS_F64 = 2e-5      # fp32 kernels against the float64 oracle, relative to max |reference| (tests/test_train_reference_gpu.py)


def _network(fx, gpu):
    network_fn, cfg = rf.build_head(fx, device=gpu)
    with torch.no_grad():
        for vn, t in rf.module_tf_names(network_fn).items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).reshape(t.shape).to(gpu))
    return network_fn, cfg


def _dequantised_fixture(fx, f8):
    """the fixture with its images replaced by the cache's values and no L2 term: what the float64 oracle is run on"""
    arrays = dict(fx.arrays)
    arrays['in/images'] = f8.dequantize().cpu().numpy()
    arrays = {k: v for k, v in arrays.items() if not k.startswith(('inseed/', 'inpatch/', 'insum/'))}
    return rf.HeadFixture(arrays=arrays, meta=dict(fx.meta, weight_decay=0.0))


def _rel(got, exp):
    exp = np.asarray(exp, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64).reshape(exp.shape)
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), 1e-30))


def test_deploy_fused_step_and_eval_on_an_fp8_batch(gpu):
    from attentionalpoolingaction_amd import config as apa_config, deploy
    try:
        # training: a reference-executed cfg 002 fixture whose dropout mask is the library's own
        fx = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_train_c2048_libmask.npz'))
        network_fn, cfg = _network(fx, gpu)
        head = network_fn.head
        head.seed, head._step = int(fx.meta['libmask'][0]), int(fx.meta['libmask'][1])
        images = torch.from_numpy(fx.arrays['in/images']).to(gpu)
        f8, status = cof.quantize_features(images)
        assert status.tolist() == [0] * images.shape[0]
        labels = torch.from_numpy(fx.arrays['in/labels_action']).to(gpu)
        fused = deploy.FusedHeadStep(network_fn, cfg, frozen_features=True)
        total, ep = fused(f8, labels)
        total.backward()
        st = fused._step_obj
        assert st._dX_buf is None and st.frozen_input and st.dX_scratch is None         # the conv5 gradient is None
        ref = rf.run_oracle(_dequantised_fixture(fx, f8))
        assert _rel(total.item(), ref['out/losses'].sum()) < FP32_VS_F64
        assert _rel(ep['Logits'].cpu(), ref['out/logits']) < FP32_VS_F64
        assert torch.equal(ep['Logits'].argmax(dim=1).cpu(), torch.from_numpy(ref['out/logits']).argmax(dim=1))
        # the bucket (the flat all-reduce payload) as a whole; the PoseLogits convs of cfg 002 get no gradient
        want = np.concatenate([ref['grad/var/' + fused.tf_names[n]].reshape(-1) if n in fused._written
                               else np.zeros(fused.bucket.views[n].numel()) for n in fused.bucket.names])
        assert _rel(fused.bucket.flat.cpu(), want) < FP32_VS_F64
        for n in fused._written:                                        # (and no variable's share is missing)
            assert float(fused.bucket.views[n].abs().max()) > 0, n
        # a second batch of the same shape re-binds the kept step
        total2, _ = fused(f8, labels)
        assert fused._step_obj is st and len(fused._steps) == 1
        with pytest.raises(ValueError, match='frozen_features'):
            deploy.FusedHeadStep(network_fn, cfg, frozen_features=False)(f8, labels)
        # a cfg 003 head with the same batch
        fx3 = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_train.npz'))
        net3, cfg3 = rf.build_head(fx3, device=gpu, in_channels=2048)
        with pytest.raises(ValueError, match='cfg 003'):
            deploy.FusedHeadStep(net3, cfg3, frozen_features=True)(f8, labels, torch.zeros(2, 3, 3, 16, device=gpu),
                                                                   torch.ones(2, 16, device=gpu))
        # evaluation
        fxe = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg002_eval_c2048.npz'))
        net_e, cfg_e = _network(fxe, gpu)
        f8e, _ = cof.quantize_features(torch.from_numpy(fxe.arrays['in/images']).to(gpu))
        scores, pred, epe = deploy.FusedHeadEval(net_e, cfg_e)(f8e)
        refe = rf.run_oracle(_dequantised_fixture(fxe, f8e))
        assert _rel(epe['Logits'].cpu(), refe['out/logits']) < FP32_VS_F64
        want = torch.softmax(torch.from_numpy(refe['out/logits']), dim=1)
        assert _rel(scores.cpu(), want.numpy()) < FP32_VS_F64
        assert torch.equal(pred.cpu(), want.argmax(dim=1))
        fx3e = rf.HeadFixture(os.path.join(rf.GOLD, 'ref_head_cfg003_eval.npz'))
        net3e, cfg3e = rf.build_head(fx3e, device=gpu, in_channels=2048)
        with pytest.raises(ValueError, match='cfg 003'):
            deploy.FusedHeadEval(net3e, cfg3e)(f8e)
    finally:
        apa_config.reset_cfg()
