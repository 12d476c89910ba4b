"""A float64 torch restatement of the pose-heatmap attention head (cfg.NET.USE_POSE_ATTENTION_LOGITS, the reference's
nets_factory.py:162-189) and the replay of a tests/golden/ref_pal_*.npz fixture through it.  Test infrastructure:
the random-shape sweeps of the GPU tests hold the kernels against `pose_att_logits`, and the CPU tests hold this
restatement against the reference-executed fixtures."""
import glob
import os

import numpy as np
import torch

import _ref_fixture as rf
from oracle import attn_pool_oracle as orc

PAL = 'USE_POSE_ATTENTION_LOGITS'
POSE_W1, POSE_B1 = 'PoseLogits/ExtraConv2d_1x1/weights', 'PoseLogits/ExtraConv2d_1x1/biases'
POSE_W2, POSE_B2 = 'PoseLogits/Conv2d_1c_1x1/weights', 'PoseLogits/Conv2d_1c_1x1/biases'
ATT_W, ATT_B = 'PoseAttention/Conv/weights', 'PoseAttention/Conv/biases'


def small_fixture_paths():
    return sorted(p for p in glob.glob(os.path.join(rf.GOLD, 'ref_pal_*.npz'))
                  if not os.path.basename(p).startswith('ref_pal_big_'))


def big_fixture_paths():
    return sorted(glob.glob(os.path.join(rf.GOLD, 'ref_pal_big_*.npz')))


def fixture_paths():
    return small_fixture_paths() + big_fixture_paths()


def case_id(path):
    return os.path.basename(path)[len('ref_pal_'):-4]


def parts_of(net, num_parts):
    """np.array(parts)[DIMS] of :168-172, as indices into the J parts"""
    dims = list(net[PAL + '_DIMS'])
    if dims == [-1]:
        return list(range(num_parts))
    return [int(j) for j in np.arange(num_parts)[np.asarray(dims, dtype=np.int64)]]


def attention_maps(Pl, parts, avged):
    """A [N,P,M]: the selected parts, their mean over all J parts (avged), the constant map"""
    n, J = Pl.shape[0], Pl.shape[-1]
    Plf = Pl.reshape(n, -1, J)
    maps = [Plf[..., j] for j in parts]
    if avged:
        maps.append(Plf.mean(dim=-1))
    maps.append(torch.ones_like(Plf[..., 0]))
    return torch.stack(maps, dim=-1)


def pooled_features(X, Pl, parts, avged):
    """F [N, M*C]: F[n, m*C + c] = mean_p A[n,p,m] X[n,p,c] (the tf.concat of :182)"""
    n, C = X.shape[0], X.shape[-1]
    Xf = X.reshape(n, -1, C)
    A = attention_maps(Pl, parts, avged)
    return torch.einsum('npm,npc->nmc', A, Xf).div(Xf.shape[1]).reshape(n, -1)


def pose_att_logits(X, Pl, parts, avged, W, b, keep_mask=None, keep_prob=1.0):
    """logits [N,K] = dropout(F) . W + b; keep_mask: the {0,1} mask over F ([N, M*C] or [N,1,1,M*C])"""
    F = pooled_features(X, Pl, parts, avged)
    if keep_mask is not None:
        F = F * keep_mask.reshape(F.shape).to(F.dtype) / keep_prob
    return F @ W.reshape(F.shape[1], -1) + b


def run_pal_fixture(fx, dtype=torch.float64):
    """Replays a ref_pal_* fixture through the restatement: pose head (oracle), pose-attention head, frame pooling,
    losses, regularisers, autograd.  Returns a dict keyed like the fixture ('out/logits', 'out/ep/<name>',
    'out/losses', 'out/reg_losses', 'out/total', 'grad/images', 'grad/pose_tap', 'grad/var/<tf name>')."""
    m = fx.meta
    K, J = m['num_classes'], m['num_pose_keypoints']
    leaf = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype).requires_grad_(True)
    V = {vn: leaf(fx.var(vn)) for vn in m['var_order']}
    images = leaf(fx.images)
    x = images
    frames = 1
    if x.dim() == 5:                                                   # :121-125
        frames = x.shape[1]
        x = x.reshape(-1, *x.shape[2:])
    pose_tap = leaf(fx.pose_tap) if fx.pose_tap is not None else None
    _, pl = orc.pose_logits_head(x if pose_tap is None else pose_tap, V[POSE_W1], V[POSE_B1], V[POSE_W2], V[POSE_B2])
    mask = fx.dropout_mask() if m['is_training'] else None
    logits = pose_att_logits(x, pl, parts_of(m['net'], J), bool(m['net'][PAL + '_AVGED_HMAP']), V[ATT_W], V[ATT_B],
                             None if mask is None else torch.from_numpy(np.asarray(mask)), fx.keep_prob)
    ep = {'PoseLogits': pl, 'Logits': logits}
    if frames > 1:                                                     # :354-374
        logits, ep2 = orc.frame_pooling(logits, frames, None, None)
        ep.update(ep2)

    class _Cfg(object):
        class TRAIN(object):
            LOSS_FN_POSE_SAMPLED = bool(m['train_cfg']['LOSS_FN_POSE_SAMPLED'])
    tc = m['train_cfg']
    use_pose = bool(tc['LOSS_FN_POSE'])
    losses = orc.gen_losses(
        torch.from_numpy(fx.arrays['in/labels_action']), logits, tc['LOSS_FN_ACTION'], K, tc['LOSS_FN_ACTION_WT'],
        torch.from_numpy(fx.arrays['in/labels_pose'].astype(np.float64)).to(dtype) if use_pose else None,
        pl if use_pose else None, tc['LOSS_FN_POSE'] if use_pose else '',
        torch.from_numpy(fx.arrays['in/labels_pose_valid']) if use_pose else None, tc['LOSS_FN_POSE_WT'], ep, _Cfg)
    regs = [orc.l2_regularizer([V[vn]], m['weight_decay']) for vn in m['var_order'] if vn.endswith('/weights')] \
        if m['weight_decay'] > 0 else []
    total = sum(losses) + (sum(regs) if regs else 0.0)
    total.backward()
    out = {'out/logits': logits, 'out/losses': torch.stack([l.reshape(()) for l in losses]),
           'out/reg_losses': torch.stack(regs) if regs else torch.zeros(0), 'out/total': total,
           'grad/images': images.grad}
    if pose_tap is not None:
        out['grad/pose_tap'] = pose_tap.grad
    for k, v in ep.items():
        out['out/ep/' + k] = v
    for vn in m['trainable']:
        g = V[vn].grad
        out['grad/var/' + vn] = (torch.zeros_like(V[vn]) if g is None else g).reshape(fx.variables[vn].shape)
    return {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
