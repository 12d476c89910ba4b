"""TRAIN.CLIP_GRADIENTS (model_deploy.py:297-304: per-variable tf.clip_by_norm of every clone's gradient, the
regulariser inside clone 0's gradient) against vectors produced by the reference's own training code
(tests/golden/make_clip_reference.py -> ref_clip_*.npz):

  * the float64 restatement of clip_by_norm and deploy.GradientClipper's CPU path on hand cases
  * the product's deploy pieces -- GradientClipper per clone, the clone sum, GradientAccumulator (ITER_SIZE),
    configure_optimizer (no L2 term folded when clipping) -- driven with the oracle's float64 gradients land on the
    reference's variables after every update, and a replay that only sets the flag does not
  * the same loop on two gloo ranks through deploy.OverlappedGradientSum (td part clipped on the side stream, att
    part on the compute stream) with the CPU runtime stand-in of tests/test_multi_rank_dryrun_cpu.py
The HIP kernel and the GPU loops: tests/test_clip_gradients_gpu.py.
"""
import glob
import json
import os
import socket

import numpy as np
import pytest
import torch

import _ref_fixture as rf
from attentionalpoolingaction_amd import config as apa_config, deploy
from test_multi_rank_dryrun_cpu import FakeRuntime

CLIP_PATHS = sorted(glob.glob(os.path.join(rf.GOLD, 'ref_clip_*.npz')))


def _id(path):
    return os.path.basename(path)[len('ref_clip_'):-4]


def clip_by_norm64(t, c):
    """tf.clip_by_norm in float64, TF 1.x's order: (t * c) * min(rsqrt(sum(t * t)), 1 / c)"""
    t = np.asarray(t, dtype=np.float64)
    ss = float((t * t).sum())
    inv = np.inf if ss == 0.0 else 1.0 / np.sqrt(ss)
    return (t * c) * min(inv, 1.0 / c)


def product_cfg(tf_):
    apa_config.reset_cfg()
    net = {k: v for k, v in tf_.meta['net'].items() if k != 'USE_POSE_ATTENTION_LOGITS_DIMS'}
    return apa_config.cfg_from_dict({'MODEL_NAME': tf_.meta['model'], 'NET': net, 'TRAIN': dict(tf_.meta['train_cfg'])})


def oracle_clone_gradients(tf_, variables, batch, draw):
    fx = tf_.clone_fixture(variables, batch, draw, weight_decay=0.0)
    o = rf.run_oracle(fx)
    return {vn: o['grad/var/' + vn] for vn in tf_.meta['var_order']}, o['out/losses']


def _cfg(clip, wd=0.0):
    cfg = apa_config.reset_cfg()
    apa_config.cfg_from_dict({'TRAIN': {'CLIP_GRADIENTS': clip, 'WEIGHT_DECAY': wd}})
    return cfg


# ------------------------------------------------------------------------------------------------- hand cases
def test_clip_by_norm_restatement_hand_cases():
    t = np.array([3.0, 4.0])                                  # norm 5
    assert np.array_equal(clip_by_norm64(t, 10.0), (t * 10.0) * (1.0 / 10.0))       # below: (t*c)*(1/c), not t
    np.testing.assert_allclose(clip_by_norm64(t, 2.5), t * 0.5, rtol=1e-15)         # above: scaled to norm c
    assert np.linalg.norm(clip_by_norm64(t, 2.5)) == pytest.approx(2.5, rel=1e-15)
    z = clip_by_norm64(np.zeros(7), 1.0)                      # rsqrt(0) = inf -> factor 1/c -> exactly 0
    assert np.array_equal(z, np.zeros(7)) and not np.signbit(z).any()


@pytest.mark.parametrize('clip', [0.0, -1.0])
def test_clipper_is_off_for_non_positive_clip(clip):
    cfg = _cfg(clip, wd=0.5)
    bucket = deploy.GradientBucket({'a/weights': (3,), 'a/biases': (2,)}, 'cpu', dtype=torch.float64)
    bucket.flat.copy_(torch.arange(5, dtype=torch.float64) * 100)
    params = {'a/weights': torch.ones(3, dtype=torch.float64), 'a/biases': torch.ones(2, dtype=torch.float64)}
    before = bucket.flat.clone()
    cl = deploy.GradientClipper(cfg, deploy.DeploymentConfig(1, 0), bucket, params, regularized=['a/weights'])
    assert not cl.active
    cl.apply()
    assert torch.equal(bucket.flat, before)
    opt = deploy.configure_optimizer(cfg, params, bucket, 0.1, regularized=['a/weights'])
    assert not opt.clipping and opt.wd == [0.5, 0.0]                  # unchanged: the optimiser folds the L2 term
    apa_config.reset_cfg()


def test_clipper_cpu_path_per_variable_with_the_regulariser_on_the_chief_only():
    cfg = _cfg(2.5, wd=0.5)
    shapes = {'a/weights': (2,), 'a/biases': (2,), 'p/weights': (3,), 'z/biases': (4,)}
    params = {'a/weights': torch.tensor([2.0, -4.0], dtype=torch.float64),
              'a/biases': torch.tensor([0.3, 0.4], dtype=torch.float64),
              'p/weights': torch.tensor([6.0, 8.0, 0.0], dtype=torch.float64),
              'z/biases': torch.zeros(4, dtype=torch.float64)}
    g = {'a/weights': np.array([2.0, 6.0]), 'a/biases': np.array([0.3, 0.4]), 'p/weights': np.array([9.0, 9.0, 9.0]),
         'z/biases': np.zeros(4)}
    reg = ['a/weights', 'p/weights']
    for ci in (0, 1):
        bucket = deploy.GradientBucket(shapes, 'cpu', dtype=torch.float64)
        for n in shapes:
            bucket.views[n].copy_(torch.from_numpy(g[n]))
        cl = deploy.GradientClipper(cfg, deploy.DeploymentConfig(2, ci), bucket, params, regularized=reg,
                                    absent=['p/weights'])
        cl.apply()
        for n in shapes:
            t = np.zeros(3) if n == 'p/weights' else g[n]               # absent: the producer never wrote it
            if ci == 0 and n in reg:
                t = t + 0.5 * params[n].numpy()
            np.testing.assert_array_equal(bucket.views[n].numpy(), clip_by_norm64(t, 2.5))
    # chief, a/weights: t = [3, 4] -> norm 5 > 2.5 -> halved; p/weights: clip(wd * w) = clip([3, 4, 0]) likewise
    apa_config.reset_cfg()


def test_optimiser_refuses_grad_scale_and_regulariser_on_top_when_clipping():
    cfg = _cfg(1.0, wd=0.1)
    for kind in ('momentum', 'sgd', 'adam', 'rmsprop'):
        cfg.TRAIN.OPTIMIZER = kind
        cfg.TRAIN.RMSPROP_DECAY = 0.9                          # a key only a YAML can add (test_deploy_gloo_cpu.py)
        params = {'w/weights': torch.ones(3, dtype=torch.float64)}
        bucket = deploy.GradientBucket({'w/weights': (3,)}, 'cpu', dtype=torch.float64)
        opt = deploy.configure_optimizer(cfg, params, bucket, 0.1, regularized=['w/weights'])
        assert opt.clipping and opt.wd == [0.0], kind                  # the clipper owns wd * w
        with pytest.raises(ValueError):
            opt.step(grad_scale=0.5)
        opt.step()
        cl = deploy.GradientClipper(cfg, deploy.DeploymentConfig(1, 0), bucket, params, regularized=['w/weights'])
        with pytest.raises(ValueError):
            deploy.add_regularization_gradient(bucket, params, 0.1, ['w/weights'])
        del cl
    # a clipper over a list of views of the bucket (OverlappedGradientSum's clip_td / clip_att) guards it too
    bucket = deploy.GradientBucket({'a/weights': (3,), 'b/weights': (2,)}, 'cpu', dtype=torch.float64)
    params = {'a/weights': torch.ones(3, dtype=torch.float64), 'b/weights': torch.ones(2, dtype=torch.float64)}
    deploy.add_regularization_gradient(bucket, params, 0.1, ['a/weights'])          # no clipper yet: allowed
    cl_td = deploy.GradientClipper(cfg, deploy.DeploymentConfig(1, 0), [('b/weights', bucket.views['b/weights'])],
                                   params, regularized=['b/weights'])
    with pytest.raises(ValueError):
        deploy.add_regularization_gradient(bucket, params, 0.1, ['a/weights'])
    assert cl_td.active
    apa_config.reset_cfg()


# ------------------------------------------------------------------------------------- reference fixtures
def test_fixture_inventory():
    names = [_id(p) for p in CLIP_PATHS]
    assert len(names) >= 4
    metas = [rf.TrainFixture(p).meta for p in CLIP_PATHS]
    assert {m['num_clones'] for m in metas} == {1, 2} and {m['iter_size'] for m in metas} >= {1, 2, 3}
    assert any(float(m['net']['DROPOUT']) > 0 for m in metas)
    assert any(m['train_cfg']['LOSS_FN_POSE'] for m in metas)
    for m in metas:
        clip = m['train_cfg']['CLIP_GRADIENTS']
        assert clip > 0
        for run in m['clip_norms']:                      # every run has clipped and unclipped variables
            norms = [n for cl in run for n in cl.values()]
            assert min(norms) < clip < max(norms)
    # the regulariser-only PoseLogits weights are themselves clipped in the big-weight-decay case
    big = [m for m in metas if m['case'].endswith('bigwd')]
    assert big and all(n > big[0]['train_cfg']['CLIP_GRADIENTS'] for run in big[0]['clip_norms'] for cl in run
                       for vn, n in cl.items() if vn.startswith('PoseLogits') and vn.endswith('/weights'))


def replay_clipped(tf_, clone_gradients, dtype=torch.float64, device='cpu', clip=True, on_run=None):
    """src/train.py + model_deploy.py with the product's deploy pieces and clipping: each clone's gradient (with the
    1/num_clones scale) is clipped by GradientClipper -- wd * w added on clone 0 -- then the clones are summed,
    ITER_SIZE micro-steps accumulated and the optimiser (no L2 term of its own) applies."""
    m = tf_.meta
    cfg = product_cfg(tf_)
    if not clip:
        cfg.TRAIN.CLIP_GRADIENTS = -1.0
    names = m['var_order']
    params = {vn: torch.from_numpy(v).to(dtype).to(device) for vn, v in tf_.initial_variables().items()}
    shapes = {vn: params[vn].shape for vn in names}
    bucket = deploy.GradientBucket(shapes, device, dtype=dtype)
    clone_bucket = deploy.GradientBucket(shapes, device, dtype=dtype)
    regularized = [vn for vn in names if vn.endswith('/weights')]
    clippers = [deploy.GradientClipper(cfg, deploy.DeploymentConfig(m['num_clones'], ci), clone_bucket, params,
                                       regularized=regularized) for ci in range(m['num_clones'])]
    accum = deploy.GradientAccumulator(bucket, cfg.TRAIN.ITER_SIZE)
    opt = deploy.configure_optimizer(cfg, params, bucket, cfg.TRAIN.LEARNING_RATE, regularized=regularized)
    assert opt.clipping == clip
    global_step = 0
    history = []
    for step in m['steps']:
        lr = deploy.configure_learning_rate(cfg, m['num_samples'], m['num_clones'], global_step)
        for r in step['runs']:
            run = m['runs'][r]
            bucket.zero_()
            for ci, (b, d) in enumerate(zip(run['batches'], run['draws'])):
                dc = deploy.DeploymentConfig(num_clones=m['num_clones'], clone_index=ci)
                grads, _ = clone_gradients(params, b, d)
                for vn in names:
                    clone_bucket.views[vn].copy_(torch.as_tensor(grads[vn]).to(dtype).to(device)
                                                 .reshape(params[vn].shape) * dc.clone_loss_scale)
                clippers[ci].apply()
                bucket.flat.add_(clone_bucket.flat)                           # _sum_clones_gradients
            if on_run is not None:
                on_run(r, params, bucket)
            if accum.step():
                opt.step(lr=lr)
                global_step += 1
        assert global_step == step['global_step']
        history.append({vn: params[vn].detach().cpu().double().numpy().copy() for vn in names})
    apa_config.reset_cfg()
    return history


def _tol(tf_, key):
    """1e-10 relative in float64; a tensor the generator stored at float32 precision (meta f32_keys) its storage ulp"""
    return max(1e-10, tf_.tol(key))


def _max_rel_dev(tf_, history):
    worst = 0.0
    for s, vars_ in enumerate(history):
        for vn, got in vars_.items():
            key = 'step/%d/var/%s' % (s, vn)
            if key in tf_.arrays:
                exp = tf_.arrays[key]
                worst = max(worst, float(np.abs(got.reshape(exp.shape) - exp).max() / max(np.abs(exp).max(), 1e-30)))
    return worst


@pytest.mark.parametrize('path', CLIP_PATHS, ids=_id)
def test_product_clipped_loop_with_oracle_gradients_is_the_reference_loop(path):
    tf_ = rf.TrainFixture(path)
    m = tf_.meta

    def clone_gradients(params, b, d):
        return oracle_clone_gradients(tf_, {vn: p.numpy() for vn, p in params.items()}, b, d)

    checked = []

    def on_run(r, params, bucket):
        # the reference's summed CLIPPED clone gradient of this run (kept for the first update's runs)
        for vn in m['grad_vars']:
            key = 'run/%d/grad/%s' % (r, vn)
            if key in tf_.arrays:
                exp = tf_.arrays[key]
                got = bucket.views[vn].numpy().reshape(exp.shape)
                assert np.abs(got - exp).max() <= _tol(tf_, key) * max(np.abs(exp).max(), 1e-30), key
                checked.append(key)

    history = replay_clipped(tf_, clone_gradients, on_run=on_run)
    assert checked
    for s, vars_ in enumerate(history):
        for vn, got in vars_.items():
            key = 'step/%d/var/%s' % (s, vn)
            if key in tf_.arrays:
                exp = tf_.arrays[key]
                assert np.abs(got.reshape(exp.shape) - exp).max() <= _tol(tf_, key) * max(np.abs(exp).max(), 1e-30), key
    # a replay that ignores the flag (today's behaviour: unclipped, L2 folded by the optimiser) lands elsewhere
    unclipped = replay_clipped(tf_, clone_gradients, clip=False)
    assert _max_rel_dev(tf_, unclipped) > 1e-4


@pytest.mark.regen
def test_generator_reproduces_a_committed_clip_fixture():
    import importlib.util
    import sys
    saved, saved_path = dict(sys.modules), list(sys.path)
    try:
        spec = importlib.util.spec_from_file_location('make_clip_reference',
                                                      os.path.join(rf.GOLD, 'make_clip_reference.py'))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        name = 'cfg002_2clones_iter2_dropout'
        out = gen.generate(names=[name])[name]
        d = np.load(os.path.join(rf.GOLD, 'ref_clip_%s.npz' % name))
        assert set(out) == set(d.files)
        for k in d.files:
            if k == 'meta':
                assert json.loads(str(out[k])) == json.loads(str(d[k]))
            else:
                assert np.array_equal(out[k], d[k]), k
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved:
                del sys.modules[k]


# ------------------------------------------------------------------ two gloo ranks, OverlappedGradientSum
class _GlooComm:
    """rccl.RcclCommunicator's `all_reduce_(tensor, stream)` over gloo in float64; remembers its one stream"""

    def __init__(self, rt, log):
        self.rt, self.log, self.stream = rt, log, None

    def all_reduce_(self, t, stream=None):
        import torch.distributed as dist
        s = stream if stream is not None else self.rt.current_stream()
        assert self.stream in (None, s.name), 'one communicator, one stream'
        self.stream = s.name
        dist.all_reduce(t)
        self.log.append(('allreduce', s.name, t.numel()))


def _ogs_worker(rank, world, port, path, out_dir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        tf_ = rf.TrainFixture(path)
        m = tf_.meta
        cfg = product_cfg(tf_)
        dc = deploy.DeploymentConfig()
        assert dc.num_clones == world and dc.clone_index == rank
        # bucket layout [att part | td part]: the classifier (td_weights / td_biases: the 'Conv' of the attention
        # scope) last, so that each part is one contiguous window
        td = [vn for vn in m['var_order'] if vn.startswith('PosePrelogitsBasedAttention/Conv/')]
        att = [vn for vn in m['var_order'] if vn not in td]
        names = att + td
        params = {vn: torch.from_numpy(v) for vn, v in tf_.initial_variables().items()}
        bucket = deploy.GradientBucket({vn: params[vn].shape for vn in names}, 'cpu', dtype=torch.float64)
        n_att = sum(params[vn].numel() for vn in att)
        reg = [vn for vn in names if vn.endswith('/weights')]
        clip_att = deploy.GradientClipper(cfg, dc, [(vn, bucket.views[vn]) for vn in att], params, regularized=reg)
        clip_td = deploy.GradientClipper(cfg, dc, [(vn, bucket.views[vn]) for vn in td], params, regularized=reg)
        rt = FakeRuntime()
        on_stream = []

        def on(name):
            return lambda: on_stream.append((name, rt.current_stream().name))
        clip_att.apply = (lambda f: lambda: (on('att')(), f()))(clip_att.apply)
        clip_td.apply = (lambda f: lambda: (on('td')(), f()))(clip_td.apply)
        comm_att, comm_td = _GlooComm(rt, rt.log), _GlooComm(rt, rt.log)
        ogs = deploy.OverlappedGradientSum(bucket.flat[:n_att], bucket.flat[n_att:], comm_att, comm_td, 'cpu',
                                           runtime=rt, clip_td=clip_td, clip_att=clip_att)
        accum = deploy.GradientAccumulator(bucket, cfg.TRAIN.ITER_SIZE)
        opt = deploy.configure_optimizer(cfg, params, bucket, cfg.TRAIN.LEARNING_RATE, regularized=reg)
        step_no = 0
        for step in m['steps']:
            lr = deploy.configure_learning_rate(cfg, m['num_samples'], world, step_no)
            for r in step['runs']:
                run = m['runs'][r]
                grads, _ = oracle_clone_gradients(tf_, {vn: p.numpy() for vn, p in params.items()},
                                                  run['batches'][rank], run['draws'][rank])
                for vn in names:
                    bucket.views[vn].copy_(torch.from_numpy(np.asarray(grads[vn])).reshape(params[vn].shape)
                                           * dc.clone_loss_scale)
                ogs.ready.record(ogs.compute)                # the head kernel's grad_ready (played by hand)
                del on_stream[:]
                ogs.after_backward()                          # clip + all-reduce each part: the run's clone sum
                assert on_stream == [('td', 'side'), ('att', 'compute')]
                if accum.step():
                    opt.step(lr=lr)
                    step_no += 1
        assert comm_td.stream == 'side' and comm_att.stream == 'compute'
        np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), **{vn: p.numpy() for vn, p in params.items()})
    finally:
        dist.destroy_process_group()
        apa_config.reset_cfg()


@pytest.mark.parametrize('name', ['cfg002_2clones_iter2', 'cfg002_2clones_iter2_dropout'])
def test_two_gloo_ranks_through_the_overlapped_sum_replay_the_clipped_loop(tmp_path, name):
    import torch.multiprocessing as mp
    path = os.path.join(rf.GOLD, 'ref_clip_%s.npz' % name)
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_ogs_worker, args=(2, port, path, str(tmp_path)), nprocs=2, join=True)
    tf_ = rf.TrainFixture(path)
    last = len(tf_.meta['steps']) - 1
    r0, r1 = np.load(tmp_path / 'rank0.npz'), np.load(tmp_path / 'rank1.npz')
    for vn in tf_.meta['var_order']:
        assert np.array_equal(r0[vn], r1[vn]), vn
        key = 'step/%d/var/%s' % (last, vn)
        exp = tf_.arrays[key]
        assert np.abs(r0[vn] - exp).max() <= _tol(tf_, key) * max(np.abs(exp).max(), 1e-30), key


# ----------------------------------------------------------------- the backbone's .grad tensors (grads=None)
def backbone_clip_case(model, images, clip_quantile=0.5, wd=0.01):
    """One backward through a resnet_v1 backbone (channels-last conv weights), one batch-norm parameter frozen (its
    `.grad` stays None).  -> (clipper, {name: float64 expected}, frozen name); the clip sits at the median pre-clip
    norm, so that about half the tensors are clipped."""
    named = dict(model.named_parameters())
    frozen = next(n for n, p in named.items() if p.dim() == 1)
    named[frozen].requires_grad_(False)
    out = model(images)
    (out.float() ** 2).mean().backward()
    assert named[frozen].grad is None
    assert any(not p.grad.is_contiguous() for p in named.values() if p.grad is not None)     # channels-last weights
    reg = [n for n, p in named.items() if p.dim() == 4]
    t64 = {n: p.grad.double().cpu() + (wd * p.data.double().cpu() if n in reg else 0.0)
           for n, p in named.items() if p.grad is not None}
    clip = float(np.quantile([float(t.norm()) for t in t64.values()], clip_quantile))
    cfg = _cfg(clip, wd=wd)
    clipper = deploy.GradientClipper(cfg, deploy.DeploymentConfig(1, 0), None, named, regularized=reg)
    apa_config.reset_cfg()
    exp = {n: torch.from_numpy(clip_by_norm64(t.numpy(), clip)) for n, t in t64.items()}
    return clipper, exp, frozen


def test_clipper_on_backbone_grads_cpu():
    from attentionalpoolingaction_amd import resnet_v1
    torch.manual_seed(0)
    model = resnet_v1.ResNetV1('resnet_v1_101', blocks=[(64, 16, 1), (128, 32, 2)])
    images = torch.randn(2, 32, 32, 3)
    clipper, exp, frozen = backbone_clip_case(model, images)
    clipper.apply()
    named = dict(model.named_parameters())
    assert named[frozen].grad is None
    for n, e in exp.items():
        g = named[n].grad.double()
        assert float((g - e).abs().max()) <= 1e-6 * max(float(e.abs().max()), 1e-30), n
