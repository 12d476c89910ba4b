"""TRAIN.CLIP_GRADIENTS on the GPU: the multi-tensor clip-by-norm HIP kernel (csrc/apa_clip.hip) against float64,
and the reference's clipped training loops (tests/golden/ref_clip_*.npz, make_clip_reference.py) replayed with the
HIP head, deploy.GradientClipper and the fused HIP optimisers.  fp32 against the reference's float64."""
import os

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from test_clip_gradients_cpu import CLIP_PATHS, _id, backbone_clip_case, clip_by_norm64, product_cfg, replay_clipped

pytestmark = pytest.mark.gpu


# a gradient the reference has at exactly zero (the attention bias under a softmax over the pixels) is fp32 rounding
# noise here (~1e-8); clipping only scales down, so the noise stays at that level.  The other gradients are 1e-2 .. 1
GRAD_FLOOR = 1e-3


def _rel(got, exp, floor=1e-30):
    return float(np.abs(np.asarray(got, dtype=np.float64) - exp).max() / max(np.abs(exp).max(), floor))


# --------------------------------------------------------------------------------------------------- kernel
def _segments(gpu, sizes, seed, wd_every=2):
    """one flat fp32 buffer starting 4 bytes past a 16-byte boundary, the segments as consecutive views (odd sizes
    -> arbitrary 4-byte offsets); per-segment scales spread the norms around clip = 1"""
    g = torch.Generator().manual_seed(seed)
    total = sum(sizes)
    host = torch.randn(total, generator=g)
    wts = torch.randn(total, generator=g)
    scales = torch.exp(torch.empty(len(sizes)).uniform_(-3.0, 3.0, generator=g))
    o = 0
    for i, n in enumerate(sizes):
        host[o:o + n] *= float(scales[i]) / max(n, 1) ** 0.5
        o += n
    flat = torch.empty(total + 1, device=gpu)[1:]
    wflat = torch.empty(total + 3, device=gpu)[3:]
    flat.copy_(host)
    wflat.copy_(wts)
    views, wviews, o = [], [], 0
    for n in sizes:
        views.append(flat[o:o + n])
        wviews.append(wflat[o:o + n])
        o += n
    wd = [0.05 if (i % wd_every == 0) else 0.0 for i in range(len(sizes))]
    return flat, host, wflat, wts, views, wviews, wd


def _expected(host, wts, sizes, wd, clip, zero=()):
    out, o = [], 0
    for i, n in enumerate(sizes):
        t = np.zeros(n) if i in zero else host[o:o + n].double().numpy()
        t = t + wd[i] * wts[o:o + n].double().numpy()
        out.append(clip_by_norm64(t, clip))
        o += n
    return out


def _resnet101_sizes():
    from attentionalpoolingaction_amd import resnet_v1
    return [p.numel() for p in resnet_v1.ResNetV1('resnet_v1_101').parameters()]


@pytest.mark.parametrize('case', ['resnet101', 'odd'])
def test_clip_kernel_against_float64(gpu, case):
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    if case == 'resnet101':
        sizes = _resnet101_sizes()
        assert len(sizes) == 312 and sum(sizes) > 42_000_000
    else:
        sizes = [1, 3, 5, 7, 17, 1, 1000, 16383, 16384, 16385, 33333, 4, 9, 2, 1, 70001, 6, 11, 13, 1]
    assert len(sizes) > 16
    clip = 1.0
    flat, host, wflat, wts, views, wviews, wd = _segments(gpu, sizes, seed=7 if case == 'odd' else 11)
    assert flat.data_ptr() % 16 == 4
    zero = {6} if case == 'odd' else set()
    for i in zero:
        views[i].zero_()
        host[sum(sizes[:i]):sum(sizes[:i + 1])] = 0.0
    zero_wd = [0.0 if i in zero else w for i, w in enumerate(wd)]        # an all-zero segment stays all zero
    saved = flat.clone()
    bound = cof.BoundClipByNorm(views, weights=wviews, wd=zero_wd)
    bound.run(clip)
    torch.cuda.synchronize()
    exp = _expected(host, wts, sizes, zero_wd, clip)
    got, o = flat.cpu().double().numpy(), 0
    clipped = unclipped = 0
    for i, n in enumerate(sizes):
        e = exp[i]
        if i in zero:
            assert not np.any(got[o:o + n]), i
        else:
            assert _rel(got[o:o + n], e) <= 2e-6, (i, n, _rel(got[o:o + n], e))
            t_norm = np.linalg.norm(host[o:o + n].double().numpy() + zero_wd[i] * wts[o:o + n].double().numpy())
            clipped += t_norm > clip
            unclipped += t_norm < clip
        o += n
    assert clipped >= 3 and unclipped >= 3
    out1 = flat.clone()
    # bit-identical on a repeated call
    flat.copy_(saved)
    bound.run(clip)
    torch.cuda.synchronize()
    assert torch.equal(flat, out1)
    # wd off: the same segments without the regulariser
    flat.copy_(saved)
    cof.clip_by_norm_(views, clip)
    exp0 = _expected(host, wts, sizes, [0.0] * len(sizes), clip)
    got, o = flat.cpu().double().numpy(), 0
    for i, n in enumerate(sizes):
        if i not in zero:
            assert _rel(got[o:o + n], exp0[i]) <= 2e-6, i
        o += n
    # the same result under hipGraph capture and replay (two launches, no host sync, no allocation)
    flat.copy_(saved)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            bound.run(clip)
    torch.cuda.current_stream().wait_stream(side)
    flat.copy_(saved)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(flat, out1)
    # clip <= 0: off, nothing launched, nothing changed
    flat.copy_(saved)
    bound.run(0.0)
    bound.run(-1.0)
    torch.cuda.synchronize()
    assert torch.equal(flat, saved)


def test_clip_kernel_rejects_bad_inputs(gpu):
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    with pytest.raises(cof.ApaError):
        cof.BoundClipByNorm([torch.zeros(8, device=gpu, dtype=torch.float64)])          # not fp32
    with pytest.raises(cof.ApaError):
        cof.BoundClipByNorm([torch.zeros(8)])                                           # not on the GPU
    with pytest.raises(cof.ApaError):
        cof.BoundClipByNorm([torch.zeros(8, device=gpu)], wd=[0.1])                    # wd without a weight
    lib = cof.load_library()
    assert lib.apa_clip_by_norm_run(None, 1, 1, 1.0, None) == -1                     # APA_ERR_INVALID_ARG
    import ctypes
    ws = torch.empty(4096, dtype=torch.uint8, device=gpu)
    n = 1
    g = torch.zeros(9, device=gpu)
    sizes = (ctypes.c_size_t * 1)(8)
    nch = ctypes.c_int(0)
    mis = (ctypes.c_void_p * 1)(g.data_ptr() + 2)                                   # not 4-byte aligned
    assert lib.apa_clip_by_norm_prepare(n, mis, sizes, None, None, None, ws.data_ptr(), ws.numel(), ctypes.byref(nch),
                                        None) == -1
    ok = (ctypes.c_void_p * 1)(g.data_ptr())
    assert lib.apa_clip_by_norm_prepare(n, ok, sizes, None, None, None, ws.data_ptr(), 8, ctypes.byref(nch),
                                        None) == -3                                 # workspace too small
    assert lib.apa_clip_by_norm_prepare(n, ok, sizes, None, None, None, ws.data_ptr() + 4, ws.numel() - 4,
                                        ctypes.byref(nch), None) == -1              # misaligned workspace


# ------------------------------------------------------------------------------- reference training loops
def _hip_clone_gradients(tf_, gpu, built):
    from attentionalpoolingaction_amd import loss as apa_loss
    m = tf_.meta

    def clone_gradients(params, b, d):
        fx = tf_.clone_fixture({vn: p.detach().cpu().numpy() for vn, p in params.items()}, b, d)
        if not built:
            network_fn, cfg = rf.build_head(fx, device=gpu)
            table = rf.module_tf_names(network_fn)
            with torch.no_grad():
                for vn, t in table.items():
                    t.copy_(params[vn].reshape(t.shape))
                    params[vn] = t
            built.update(network_fn=network_fn, cfg=cfg, table=table)
        network_fn, cfg, table = built['network_fn'], built['cfg'], built['table']
        images = torch.from_numpy(fx.arrays['in/images']).to(gpu)
        network_fn.head.replay_dropout_mask(torch.from_numpy(fx.dropout_mask()).to(gpu))
        logits, ep = network_fn(images)
        tc = m['train_cfg']
        use_pose = bool(tc['LOSS_FN_POSE'])
        losses = apa_loss.gen_losses(
            torch.from_numpy(fx.arrays['in/labels_action']).to(gpu), logits, tc['LOSS_FN_ACTION'], m['num_classes'],
            tc['LOSS_FN_ACTION_WT'],
            torch.from_numpy(fx.arrays['in/labels_pose']).to(gpu) if use_pose else None,
            ep.get('PoseLogits') if use_pose else None, tc['LOSS_FN_POSE'] if use_pose else '',
            torch.from_numpy(fx.arrays['in/labels_pose_valid']).to(gpu) if use_pose else None, tc['LOSS_FN_POSE_WT'],
            ep, cfg)
        ts = [table[vn] for vn in m['var_order']]
        gs = torch.autograd.grad(sum(losses), ts, allow_unused=True)
        return {vn: (torch.zeros_like(t) if g is None else g) for vn, t, g in zip(m['var_order'], ts, gs)}, \
            [float(l.detach()) for l in losses]
    return clone_gradients


def _check_history(tf_, history):
    for s, vars_ in enumerate(history):
        for vn, got in vars_.items():
            key = 'step/%d/var/%s' % (s, vn)
            if key in tf_.arrays:
                exp = tf_.arrays[key]
                assert _rel(got.reshape(exp.shape), exp) < 2e-5, key


@pytest.mark.parametrize('path', CLIP_PATHS, ids=_id)
def test_hip_clipped_training_loop_matches_reference(gpu, path):
    tf_ = rf.TrainFixture(path)
    built = {}
    checked = []

    def on_run(r, params, bucket):
        for vn in tf_.meta['grad_vars']:
            key = 'run/%d/grad/%s' % (r, vn)
            if key in tf_.arrays:
                exp = tf_.arrays[key]
                assert _rel(bucket.views[vn].cpu().numpy().reshape(exp.shape), exp, GRAD_FLOOR) < 5e-5, key
                checked.append(key)

    history = replay_clipped(tf_, _hip_clone_gradients(tf_, gpu, built), dtype=torch.float32, device=gpu,
                             on_run=on_run)
    assert checked
    _check_history(tf_, history)
    # the clip moved the weights by far more than the tolerance: the unclipped loop lands elsewhere
    built.clear()
    unclipped = replay_clipped(tf_, _hip_clone_gradients(tf_, gpu, built), dtype=torch.float32, device=gpu, clip=False)
    last = len(history) - 1
    worst = max(_rel(unclipped[last][vn], tf_.arrays['step/%d/var/%s' % (last, vn)].reshape(unclipped[last][vn].shape))
                for vn in tf_.meta['var_order'] if 'step/%d/var/%s' % (last, vn) in tf_.arrays)
    assert worst > 1e-3


FUSED_CASES = ['cfg002_2clones_iter2', 'cfg003_1clone_iter3', 'cfg002_1clone_iter1_bigwd']


@pytest.mark.parametrize('name', FUSED_CASES)
def test_fused_head_step_clipped_loop_matches_reference(gpu, name):
    """deploy.FusedHeadStep with TRAIN.CLIP_GRADIENTS: per clone `fused(...)`, `total.backward()`, the clone's clip
    (`fused.clip()` on the chief, a GradientClipper of clone 1 over the same bucket), the clones summed and ITER_SIZE
    micro-steps accumulated, then the optimiser `make_optimizer` configured (momentum-SGD, no L2 term of its own)."""
    from attentionalpoolingaction_amd import config as apa_config, deploy
    tf_ = rf.TrainFixture(os.path.join(rf.GOLD, 'ref_clip_%s.npz' % name))
    m = tf_.meta
    assert float(m['net']['DROPOUT']) == 0.0                  # the one-call steps draw their own masks
    nc = m['num_clones']
    try:
        params0 = tf_.initial_variables()
        fx0 = tf_.clone_fixture(params0, m['runs'][0]['batches'][0], m['runs'][0]['draws'][0])
        network_fn, _ = rf.build_head(fx0, device=gpu)
        cfg = product_cfg(tf_)
        table = rf.module_tf_names(network_fn)
        with torch.no_grad():
            for vn, t in table.items():
                t.copy_(torch.from_numpy(params0[vn]).reshape(t.shape).to(gpu))
        dcs = [deploy.DeploymentConfig(nc, ci) for ci in range(nc)]
        fused = deploy.FusedHeadStep(network_fn, cfg, loss_scale=dcs[0].clone_loss_scale)
        opt = fused.make_optimizer(cfg.TRAIN.LEARNING_RATE, deploy_config=dcs[0])
        assert fused.clipper is not None and opt.clipping and all(w == 0.0 for w in opt.wd)
        absent = [n for n in fused.params if n not in fused._written]
        clippers = [fused.clip] + [deploy.GradientClipper(cfg, dc, list(fused.bucket.views.items()), dict(fused.params),
                                                          regularized=fused.regularized, absent=absent).apply
                                   for dc in dcs[1:]]
        accum = deploy.GradientAccumulator(fused.bucket, cfg.TRAIN.ITER_SIZE)
        run_sum = torch.zeros_like(fused.bucket.flat)
        attr_of = {tfn: attr for attr, tfn in network_fn.head.tf_variable_names().items()}
        global_step = 0
        history = []
        for step in m['steps']:
            lr = deploy.configure_learning_rate(cfg, m['num_samples'], nc, global_step)
            for r in step['runs']:
                run = m['runs'][r]
                run_sum.zero_()
                for ci, (b, d) in enumerate(zip(run['batches'], run['draws'])):
                    fx = tf_.clone_fixture({vn: t.detach().cpu().numpy() for vn, t in table.items()}, b, d)
                    img = torch.from_numpy(fx.arrays['in/images']).to(gpu)
                    if img.dim() == 5:
                        img = img.reshape(-1, *img.shape[2:])
                    la = torch.from_numpy(fx.arrays['in/labels_action']).to(gpu)
                    lp = pv = None
                    if fused.pose_form:
                        lp = torch.from_numpy(fx.arrays['in/labels_pose']).to(gpu)
                        lp = lp.reshape(img.shape[0], img.shape[1], img.shape[2], -1)
                        pv = torch.from_numpy(fx.arrays['in/labels_pose_valid']).to(gpu).reshape(img.shape[0], -1)
                    total, _ = fused(img, la, lp, pv)
                    total.backward()
                    clippers[ci]()
                    run_sum.add_(fused.bucket.flat)
                fused.bucket.flat.copy_(run_sum)
                for vn in m['grad_vars']:
                    key = 'run/%d/grad/%s' % (r, vn)
                    if key in tf_.arrays:
                        exp = tf_.arrays[key]
                        got = fused.bucket.views[attr_of[vn]].cpu().numpy().reshape(exp.shape)
                        assert _rel(got, exp, GRAD_FLOOR) < 5e-5, key
                if accum.step():
                    opt.step(lr=lr)
                    global_step += 1
            history.append({vn: t.detach().cpu().double().numpy().copy() for vn, t in table.items()})
        _check_history(tf_, history)
    finally:
        apa_config.reset_cfg()


# ------------------------------------------------------------------------------- the adaptive optimisers
@pytest.mark.parametrize('kind', ['adam', 'rmsprop', 'sgd'])
def test_optimisers_with_clipping_take_the_l2_term_once_inside_the_clip(gpu, kind):
    """A few updates of each optimiser with clipping on against a float64 restatement: t = g + wd * w clipped per
    variable, then the optimiser's rule with NO L2 term of its own.  Folding wd * w again in the launch (or outside
    the clip) lands measurably elsewhere."""
    from attentionalpoolingaction_amd import config as apa_config, deploy
    cfg = apa_config.reset_cfg()
    apa_config.cfg_from_dict({'TRAIN': {'OPTIMIZER': kind, 'CLIP_GRADIENTS': 0.5, 'WEIGHT_DECAY': 0.3,
                                        'OPT_EPSILON': 1e-3, 'MOMENTUM': 0.5}})
    cfg.TRAIN.RMSPROP_DECAY = 0.9
    try:
        shapes = {'a/weights': (33, 7), 'a/biases': (7,), 'b/weights': (5, 3)}
        reg = ['a/weights', 'b/weights']
        g = torch.Generator().manual_seed(5)
        w64 = {n: torch.randn(s, generator=g, dtype=torch.float64) for n, s in shapes.items()}
        params = {n: v.float().to(gpu) for n, v in w64.items()}
        bucket = deploy.GradientBucket(shapes, gpu)
        clipper = deploy.GradientClipper(cfg, deploy.DeploymentConfig(1, 0), bucket, params, regularized=reg)
        opt = deploy.configure_optimizer(cfg, params, bucket, 0.05, regularized=reg)
        slots = {n: [torch.zeros(s, dtype=torch.float64), torch.zeros(s, dtype=torch.float64)] for n, s in shapes.items()}
        if kind == 'rmsprop':
            for n in shapes:
                slots[n][0].fill_(1.0)
        lr, wd, c = 0.05, 0.3, 0.5
        for k in range(4):
            grads = {n: torch.randn(s, generator=g, dtype=torch.float64) * (0.1 if n == 'a/biases' else 1.0)
                     for n, s in shapes.items()}
            for n in shapes:
                bucket.views[n].copy_(grads[n].float())
            clipper.apply()
            opt.step(lr=lr)
            for n in shapes:
                t = grads[n].float().double() + (wd * w64[n] if n in reg else 0.0)
                t = torch.from_numpy(clip_by_norm64(t.numpy(), c))
                a, b = slots[n]
                if kind == 'adam':
                    lr_t = lr * (1 - 0.999 ** (k + 1)) ** 0.5 / (1 - 0.9 ** (k + 1))
                    a += (t - a) * (1 - 0.9)
                    b += (t * t - b) * (1 - 0.999)
                    w64[n] -= a * lr_t / (b.sqrt() + 1e-3)
                elif kind == 'rmsprop':
                    a += (t * t - a) * (1 - 0.9)
                    b.mul_(0.5).add_(t * lr / (a + 1e-3).sqrt())
                    w64[n] -= b
                else:
                    w64[n] -= lr * t
        for n in shapes:
            exp = w64[n].numpy()
            assert _rel(params[n].cpu().numpy(), exp) < 2e-5, (kind, n)
    finally:
        apa_config.reset_cfg()


# ----------------------------------------------------------------- the backbone's .grad tensors (grads=None)
def test_clipper_on_resnet101_grads_against_float64(gpu):
    """GradientClipper(grads=None) on resnet_v1.ResNetV1('resnet_v1_101') after a real backward: 312 parameters, 34
    of them channels-last conv weights whose `.grad` has the same strides, one frozen batch-norm parameter (`.grad`
    None, skipped), the regulariser on the conv weights; every tensor against float64.  Then the binding: resident
    gradients (zero_grad(set_to_none=False)) re-use the table, replaced ones are re-bound once."""
    from attentionalpoolingaction_amd import resnet_v1
    torch.manual_seed(0)
    model = resnet_v1.ResNetV1('resnet_v1_101').to(gpu)
    images = torch.randn(2, 64, 64, 3, device=gpu)
    clipper, exp, frozen = backbone_clip_case(model, images)
    named = dict(model.named_parameters())
    assert len(named) == 312
    clipper.bind()
    clipper.apply()
    torch.cuda.synchronize()
    assert named[frozen].grad is None
    clipped = 0
    for n, e in exp.items():
        got = named[n].grad.double().cpu()
        assert _rel(got.numpy(), e.numpy()) <= 2e-6, n
        clipped += abs(float(e.norm()) - clipper.clip) <= 1e-9 * clipper.clip      # scaled down to norm c
    assert 0.3 * len(exp) < clipped < 0.7 * len(exp)
    assert clipper.rebinds == 0
    # resident .grad tensors (set_to_none=False): the same table, no re-binding
    model.zero_grad(set_to_none=False)
    (model(images).float() ** 2).mean().backward()
    clipper.apply()
    assert clipper.rebinds == 0
    # replaced .grad tensors (set_to_none=True): re-bound once, and the result is still right
    model.zero_grad(set_to_none=True)
    (model(images).float() ** 2).mean().backward()
    g64 = {n: p.grad.double().cpu() for n, p in named.items() if p.grad is not None}
    clipper.apply()
    torch.cuda.synchronize()
    assert clipper.rebinds == 1
    wd, c = clipper.weight_decay_of, clipper.clip
    for n, g in g64.items():
        e = clip_by_norm64((g + wd(n) * named[n].data.double().cpu()).numpy(), c)
        assert _rel(named[n].grad.double().cpu().numpy(), e) <= 2e-6, n


def test_clip_run_refuses_a_workspace_it_did_not_prepare(gpu):
    """apa_clip_by_norm_run with (nseg, nchunks) other than what prepare returned, or on a workspace prepare never
    saw, is an error code -- never a launch over a table read at the wrong offsets."""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    ts = [torch.randn(n, device=gpu) for n in (5, 40000, 7)]
    b = cof.BoundClipByNorm(ts)
    lib = cof.load_library()
    before = [t.clone() for t in ts]
    assert lib.apa_clip_by_norm_run(b.ws.data_ptr(), 3, b.nchunks + 1, 1.0, None) == -1
    assert lib.apa_clip_by_norm_run(b.ws.data_ptr(), 2, b.nchunks, 1.0, None) == -1
    other = torch.empty_like(b.ws)
    assert lib.apa_clip_by_norm_run(other.data_ptr(), 3, b.nchunks, 1.0, None) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(t, u) for t, u in zip(ts, before))
    assert lib.apa_clip_by_norm_run(b.ws.data_ptr(), 3, b.nchunks, 1.0, None) == 0
