#!/usr/bin/env python
"""Golden vectors for the TRAINING step under the multi-label action losses of HICO and Charades
(TRAIN.LOSS_FN_ACTION 'multi-label' / 'multi-label-2', src/loss.py:88-101; multi-hot labels as read_sparse_label
builds them), flat batches and video clips, produced by EXECUTING THE REFERENCE'S OWN graph-construction and loss code
through make_head_reference.py -- `load_reference()` and `run_head_case()` exactly as they are.  run_head_case draws
integer labels only, so it is handed a thin stand-in for the loss module whose gen_losses substitutes a seeded multi-hot
[n_loss, K] tensor for its first argument (each class positive with probability ~0.1, row 0 all zero) and calls the
reference's gen_losses with everything else untouched; the tensor is added to the file as in/labels_action_multihot.
Nothing of the reference is copied; only the .npz data is committed.

    tests/golden/ref_mlstep_<case>.npz        small cases: every tensor in full
    tests/golden/ref_mlstep_big_<case>.npz    HICO / Charades shapes: inputs by seed, large tensors as digest + sample

Every case carries libmask=(seed, offset): the dropout mask is the library's own counter stream, so the one-call steps
run these fixtures with their hash.  The prefix keeps the files out of every existing fixture glob.

Run in the build container (the GPU box has no reference tree):
    python tests/golden/make_multilabel_step_reference.py            # the small cases
    python tests/golden/make_multilabel_step_reference.py big        # + the HICO / Charades shapes
"""
import copy
import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_head_reference as mhr          # noqa: E402
import make_pose_att_reference as mpar     # noqa: E402  (digest_large_outputs)
import tf1_shim as tfs                     # noqa: E402

P, SL, NOPOSE = mhr.P, mhr.SL, mhr.NOPOSE
Y003 = '003_MPII_ResNet_withPoseAttention.yaml'
TATT = dict(USE_TEMPORAL_ATT=True)
ML, ML2 = dict(LOSS_FN_ACTION='multi-label'), dict(LOSS_FN_ACTION='multi-label-2')
CASES = [
    # C = 512, K = 24: the shape at which the flat step folds the loss into the logits reducer
    dict(name='flat002_ml_c512', train=True, shape=(2, 3, 3, 512), K=24, train_cfg=dict(NOPOSE, **ML), net=SL,
         libmask=(42, 81)),
    dict(name='flat002_ml2_c32', train=True, shape=(2, 3, 3, 32), K=20, train_cfg=dict(NOPOSE, **ML2), net=SL,
         libmask=(42, 85)),
    dict(name='clip_temporal_ml', train=True, shape=(2, 3, 3, 3, 32), K=20, train_cfg=dict(NOPOSE, **ML),
         net=dict(SL, **TATT), libmask=(42, 89)),
    # cfg 003: the pose L2 loss stays on
    dict(name='cfg003_ml2', yaml=Y003, train=True, shape=(2, 3, 3, 32), K=20, train_cfg=ML2, libmask=(42, 93)),
    # (the compact form of make_video_step_reference.py's cfg003_framepool_bf16_c512)
    dict(name='cfg003_clip_ml_bf16_c512', yaml=Y003, train=True, shape=(2, 2, 3, 3, 512), K=20, train_cfg=ML,
         quant='bf16', gate_safe=True, libmask=(42, 97), big=True, full_limit=1 << 16),
]
BIG_CASES = [
    # HICO: 600 classes on images; Charades: 157 classes on clips with the TemporalAttention conv
    dict(name='hico_32x14x14_k600_libmask', train=True, shape=(32, 14, 14, 2048), K=600, train_cfg=dict(NOPOSE, **ML),
         net=SL, libmask=(42, 101), big=True, quant='bf16', full_limit=1 << 16, benchmark=True),
    dict(name='charades_8x4_k157_libmask', train=True, shape=(8, 4, 14, 14, 2048), K=157,
         train_cfg=dict(NOPOSE, **ML), net=dict(SL, **TATT), libmask=(42, 105), big=True, quant='bf16',
         full_limit=1 << 16, benchmark=True),
]


def multihot(name, n_loss, K):
    """seeded multi-hot labels [n_loss, K], float32: each class positive with probability 0.1, row 0 all zero, and at
    least one positive in the last row (a two-row case would otherwise often have none at all)"""
    r = np.random.RandomState(zlib.crc32(('%s|multihot' % name).encode()) & 0x7fffffff)
    t = (r.rand(n_loss, K) < 0.1).astype(np.float32)
    t[0] = 0.0
    k = r.randint(K)
    if n_loss > 1 and not t[-1].any():
        t[-1, k] = 1.0
    return t


class MultiHotLoss(object):
    """Stands in for the reference's loss module in run_head_case: gen_losses with the labels exchanged."""

    def __init__(self, lossmod, name):
        self.lossmod, self.name, self.labels = lossmod, name, None

    def gen_losses(self, labels_action, logits_action, loss_type_action, num_action_classes, *rest):
        n_loss = int(logits_action.v.shape[0])
        assert tuple(labels_action.v.shape) == (n_loss,)
        self.labels = multihot(self.name, n_loss, num_action_classes)
        return self.lossmod.gen_losses(tfs.Tensor(torch.from_numpy(self.labels)), logits_action, loss_type_action,
                                       num_action_classes, *rest)


def main():
    want_big = 'big' in sys.argv[1:]
    only = set(a for a in sys.argv[1:] if a != 'big')
    cfgmod, nf, lossmod = mhr.load_reference()
    defaults = copy.deepcopy(cfgmod.cfg)
    for case in CASES + (BIG_CASES if want_big else []):
        if only and case['name'] not in only:
            continue
        case = dict(case, name='mlstep_' + case['name'])     # the name keys the seeded draws of the generator
        stand_in = MultiHotLoss(lossmod, case['name'])
        out = mhr.run_head_case(cfgmod, nf, stand_in, defaults, case)
        out['in/labels_action_multihot'] = stand_in.labels
        if case.get('big'):
            mpar.digest_large_outputs(out)
        dst = os.path.join(HERE, ('ref_mlstep_big_%s.npz' if case.get('benchmark') else 'ref_mlstep_%s.npz') %
                           case['name'][len('mlstep_'):])
        np.savez_compressed(dst, **out)
        meta = json.loads(str(out['meta']))
        print('%-44s %8.1f KB  losses: %s' % (case['name'], os.path.getsize(dst) / 1024, out['out/losses']))


if __name__ == '__main__':
    main()
