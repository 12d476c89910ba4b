"""The pose-heatmap attention head (cfg.NET.USE_POSE_ATTENTION_LOGITS) on the GPU.

* Every reference-executed fixture tests/golden/ref_pal_*.npz through network_fn -> loss.gen_losses -> autograd, at
  the tolerances tests/test_reference_fixtures_gpu.py applies to the other heads (fp32 kernels against a float64
  target: logits 1e-3 absolute and 2e-5 relative, argmax exact, end points / gradients 5e-5 relative).  The small
  cases replay the reference's own dropout mask (APA_FLAG_RNG_EXTERNAL); the benchmark-shape cases' mask IS the
  library's hash stream for (seed, offset), so the head runs with its own counter hash.
* bf16 features: the inputs and variables of the bf16 fixtures are bf16-representable, so what is measured is the
  kernels' own rounding: the pose head's bf16 pre-logits store and bf16 MFMA operands (an element error of ~2^-9
  relative, carried into Pl and from there into the attention maps) and the bf16 store of dX.  Held to 3e-3 on the
  logits (test_bf16_parity_gpu.py's LOGIT_TOL_BF16), KAPPA * 2^-8 = 1.2e-2 of max|reference| on every gradient.
  Separately, the new kernels given the pose head's own Pl are held to 2e-5 relative against the float64
  restatement (_pal_reference), which keeps their arithmetic apart from the pose head's bf16 rounding.
* A fixed-seed random-shape sweep (odd P, N = 1, K = 1, M = 1 .. 18, C = 4 .. 2048), bit-identical repeats, and the
  mask the kernels apply against apa_dropout_mask.
Kernel by kernel and stage by stage, workspace stages included: tests/test_pose_att_paths_gpu.py."""
import numpy as np
import pytest
import torch

import _pal_reference as pal
import _ref_fixture as rf

pytestmark = pytest.mark.gpu
SMALL = pal.small_fixture_paths()
BIG = pal.big_fixture_paths()


def _rel(got, exp, floor=1e-30):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(exp).shape)
    exp = np.asarray(exp, dtype=np.float64)
    return float(np.abs(got - exp).max() / max(np.abs(exp).max(), floor))


def _run_product(fx, gpu, in_dtype=torch.float32):
    from attentionalpoolingaction_amd import config as apa_config, loss as apa_loss, nets_factory
    m = fx.meta
    cfg = apa_config.cfg_from_dict({'MODEL_NAME': m['model'], 'NET': dict(m['net']), 'TRAIN': dict(m['train_cfg'])})
    kw = dict(in_channels=fx.arrays['in/images'].shape[-1])
    tap = None
    if fx.pose_tap is not None:                                  # a backbone that returns its end points by name
        kw['pose_in_channels'] = fx.pose_tap.shape[-1]
        tap = torch.from_numpy(fx.arrays['in/pose_tap']).to(gpu).to(in_dtype).requires_grad_(True)
        kw['backbone'] = lambda im: {m['last_conv']: im, m['last_conv_pose']: tap}
    network_fn = nets_factory.get_network_fn(m['model'], m['num_classes'], m['num_pose_keypoints'], cfg,
                                             weight_decay=m['weight_decay'], is_training=m['is_training'],
                                             device=gpu, **kw)
    head = network_fn.head
    assert isinstance(head, nets_factory.PoseAttentionLogitsHead)
    table = rf.module_tf_names(network_fn)
    with torch.no_grad():
        for vn, t in table.items():
            t.copy_(torch.from_numpy(fx.var(vn).astype(np.float32)).to(gpu))
    images = torch.from_numpy(fx.arrays['in/images']).to(gpu).to(in_dtype).requires_grad_(True)
    if m['is_training']:
        if m.get('libmask'):          # the fixture's mask is the library's own stream: the head's counter hash
            head.seed, head._step = int(m['libmask'][0]), int(m['libmask'][1])
        else:
            head.replay_dropout_mask(torch.from_numpy(fx.dropout_mask()).to(gpu))
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
    reg = apa_loss.l2_regularization(network_fn.regularized_weights(), network_fn.weight_decay)
    total = sum(losses) + reg
    total.backward()
    apa_config.reset_cfg()
    return dict(network_fn=network_fn, head=head, table=table, logits=logits, ep=ep, losses=losses, reg=reg,
                total=total, images=images, tap=tap)


def _check_fixture(fx, r, bf):
    exp_logits = fx.expected('out/logits').astype(np.float64)
    got_logits = r['logits'].detach().float().cpu().numpy().astype(np.float64)
    err = np.abs(got_logits - exp_logits).max()
    if bf:
        ltol = 3e-3
        assert err <= ltol, err
        top2 = np.sort(exp_logits, axis=1)[:, -2:]
        sure = (top2[:, 1] - top2[:, 0]) > 2 * ltol
        assert np.array_equal(got_logits.argmax(1)[sure], exp_logits.argmax(1)[sure])
    else:
        assert err <= 1e-3 and _rel(got_logits, exp_logits) < 2e-5, err
        assert np.array_equal(got_logits.argmax(1), exp_logits.argmax(1))
    tol, tolp = (1.2e-2, 8e-3) if bf else (5e-5, 5e-5)
    for key in fx.meta['end_points']:
        name = key[len('out/ep/'):]
        assert name in r['ep'], 'end point %s missing' % name
        fx.check(key, r['ep'][name].detach().float().cpu().numpy(), tol, name, floor=1e-6)
    for got, exp in zip(r['losses'], fx.expected('out/losses')):
        assert abs(float(got.detach()) - exp) <= (2e-3 if bf else 2e-5) * max(abs(exp), 1e-3)
    assert abs(float(r['total']) - float(fx.expected('out/total'))) <= \
        (2e-3 if bf else 2e-5) * float(fx.expected('out/total'))
    fx.check('grad/images', r['images'].grad.float().cpu().numpy(), tol, 'grad/images', tol_proj=tolp)
    if r['tap'] is not None:
        fx.check('grad/pose_tap', r['tap'].grad.float().cpu().numpy(), tol, 'grad/pose_tap', tol_proj=tolp)
    for vn in fx.meta['trainable']:
        t = r['table'][vn]
        if vn in fx.meta['reg_only_grad']:
            assert _rel(t.grad.cpu().numpy(), fx.meta['weight_decay'] * fx.variables[vn]) < 5e-5, vn
            continue
        assert t.grad is not None, vn
        fx.check('grad/var/' + vn, t.grad.float().cpu().numpy(), tol, vn, tol_proj=tolp)


@pytest.mark.parametrize('path', SMALL, ids=pal.case_id)
def test_head_matches_reference_fixture(gpu, path):
    fx = rf.HeadFixture(path)
    bf = fx.quant == 'bf16'
    _check_fixture(fx, _run_product(fx, gpu, torch.bfloat16 if bf else torch.float32), bf)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('path', BIG, ids=pal.case_id)
def test_head_matches_reference_at_the_benchmark_shape(gpu, path, dtype):
    fx = rf.HeadFixture(path)
    assert fx.quant == 'bf16' and fx.meta.get('libmask')
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    seed, offset = fx.meta['libmask']
    dr = fx.meta['draws'][0]
    got = cof.dropout_mask(tuple(dr['shape']), fx.keep_prob, seed, offset, device=gpu).cpu().numpy()
    assert np.array_equal(got, fx.dropout_mask())
    bf = dtype == 'bf16'
    _check_fixture(fx, _run_product(fx, gpu, torch.bfloat16 if bf else torch.float32), bf)


def _kernel_case(gpu, N, H, W_, C, J, K, parts, avged, dtype, train, seed=5, offset=3, keep=0.2, gen_seed=0):
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    g = torch.Generator().manual_seed(gen_seed)
    M = cof.pose_att_num_maps(parts, avged)
    X = torch.relu(torch.randn(N, H, W_, C, generator=g)).to(dtype)
    Pl = torch.randn(N, H, W_, J, generator=g)
    Wt = torch.randn(M * C, K, generator=g) / (M * C) ** 0.5
    b = torch.randn(K, generator=g)
    G = torch.randn(N, K, generator=g)
    dPl0 = torch.zeros(N, H, W_, J)
    dev = dict(X=X.to(gpu), Pl=Pl.to(gpu), W=Wt.to(gpu), b=b.to(gpu), G=G.to(gpu), dPl0=dPl0.to(gpu))
    flags = cof.attn_flags(is_training=train)
    kp = keep if train else 1.0
    F, logits, ws = cof.pose_att_logits_fwd(dev['X'], dev['Pl'], parts, avged, dev['W'], dev['b'], flags=flags,
                                            keep_prob=kp, seed=seed, offset=offset)
    dX, dPl, dW, db = cof.pose_att_logits_bwd(dev['X'], dev['Pl'], parts, avged, dev['W'], F, dev['G'],
                                              dev['dPl0'].clone(), flags=flags, keep_prob=kp, seed=seed,
                                              offset=offset, workspace=ws)
    torch.cuda.synchronize()
    mask = cof.dropout_mask((N, M * C), kp, seed, offset, device=gpu).cpu() if train else None
    Xr = X.double().requires_grad_(True)
    Plr = Pl.double().requires_grad_(True)
    Wr = Wt.double().requires_grad_(True)
    br = b.double().requires_grad_(True)
    Fr = pal.pooled_features(Xr, Plr, parts, avged)
    lr = pal.pose_att_logits(Xr, Plr, parts, avged, Wr, br, mask, kp)
    (lr * G.double()).sum().backward()
    got = dict(F=F, logits=logits, dX=dX, dPl=dPl - dev['dPl0'], dW=dW, db=db)
    exp = dict(F=Fr.detach(), logits=lr.detach(), dX=Xr.grad, dW=Wr.grad, db=br.grad,
               dPl=torch.zeros_like(Plr) if Plr.grad is None else Plr.grad)   # no part selected: Pl unused
    return got, exp


def _assert_close(got, exp, tol, what):
    for k in exp:
        g = got[k].detach().float().cpu().double().numpy()
        e = exp[k].numpy()
        scale = max(float(np.abs(e).max()), 1e-30)
        err = float(np.abs(g.reshape(e.shape) - e).max()) / scale
        assert err <= tol, '%s %s: rel err %.3e > %.1e' % (what, k, err, tol)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_kernels_against_restatement_at_the_benchmark_shape(gpu, dtype):
    """the new kernels alone, given Pl: fp32 arithmetic against float64 (bf16 features are exact in both)"""
    got, exp = _kernel_case(gpu, 32, 14, 14, 2048, 16, 393, list(range(16)), False, dtype, True)
    tol = 2e-5
    for k in ('F', 'logits', 'dPl', 'dW', 'db'):
        _assert_close({k: got[k]}, {k: exp[k]}, tol, str(dtype))
    # dX is stored in the feature dtype: bf16 rounding of the stored value (2^-9 relative) on top
    _assert_close({'dX': got['dX']}, {'dX': exp['dX']}, tol if dtype == torch.float32 else 4e-3, str(dtype))


SWEEP_C = [4, 8, 12, 252, 256, 260, 516, 1024, 2048]


def test_random_shape_sweep(gpu):
    rs = np.random.RandomState(20261015)
    cases = [(1, 3, 3, 4, 16, 1, [], False), (1, 1, 1, 8, 16, 1, [0], True)]
    for M_target in range(1, 19):
        n_sel = rs.randint(0, M_target) if M_target > 1 else 0
        avged = (M_target - 1 - n_sel) == 1
        n_sel = M_target - 1 - (1 if avged else 0)
        J = int(rs.choice([1, 13, 16]))
        parts = [int(j) for j in rs.randint(0, J, size=n_sel)]
        H, W_ = int(rs.choice([1, 3, 5, 7, 9])), int(rs.choice([1, 3, 5, 15]))
        cases.append((int(rs.choice([1, 2, 3, 33, 40])), H, W_, int(SWEEP_C[M_target % len(SWEEP_C)]), J,
                      int(rs.choice([1, 7, 51, 393, 480])), parts, avged))
    for C in SWEEP_C:
        cases.append((1, 3, 5, C, 16, 1, [2, 2], True))
    for i, (N, H, W_, C, J, K, parts, avged) in enumerate(cases):
        for train in (False, True):
            got, exp = _kernel_case(gpu, N, H, W_, C, J, K, parts, avged, torch.float32, train, seed=i,
                                    offset=2 * i, keep=0.5, gen_seed=i)
            _assert_close(got, exp, 2e-5, 'case %d %s train=%s' % (i, (N, H, W_, C, J, K, parts, avged), train))


def test_repeat_calls_are_bit_identical(gpu):
    a, _ = _kernel_case(gpu, 32, 14, 14, 2048, 16, 393, [3, 0, 9], True, torch.float32, True)
    b, _ = _kernel_case(gpu, 32, 14, 14, 2048, 16, 393, [3, 0, 9], True, torch.float32, True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_replayed_mask_equals_hashed_mask(gpu):
    """APA_FLAG_RNG_EXTERNAL with the bits apa_dropout_mask returns gives bit-identical results to the hash"""
    from attentionalpoolingaction_amd.custom_ops import custom_ops_factory as cof
    N, P, C, J, K, parts = 4, 25, 256, 16, 51, [1, 5]
    M = cof.pose_att_num_maps(parts, True)
    g = torch.Generator().manual_seed(3)
    X = torch.relu(torch.randn(N, P, C, generator=g)).to(gpu)
    Pl = torch.randn(N, P, J, generator=g).to(gpu)
    W = torch.randn(M * C, K, generator=g).to(gpu)
    b = torch.zeros(K, device=gpu)
    G = torch.randn(N, K, generator=g).to(gpu)
    flags = cof.attn_flags(is_training=True)
    mask = cof.dropout_mask((N, M * C), 0.2, 11, 4, device=gpu)
    outs = []
    for seed in (11, cof.pack_keep_mask(mask, device=gpu)):
        F, lg, ws = cof.pose_att_logits_fwd(X, Pl, parts, True, W, b, flags=flags, keep_prob=0.2, seed=seed, offset=4)
        dX, dPl, dW, db = cof.pose_att_logits_bwd(X, Pl, parts, True, W, F, G, torch.zeros_like(Pl), flags=flags,
                                                  keep_prob=0.2, seed=seed, offset=4, workspace=ws)
        outs.append((lg, dX, dPl, dW, db))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
