#!/usr/bin/env python
"""Golden vectors for the TRAINING step on video clips: a [B,F,H,W,C] input folded into B*F frames for the head
(the reference's nets_factory.py:121-125), the frame logits averaged per clip -- optionally weighted by the
TemporalAttention conv (:354-374) -- and the action loss taken on the pooled logits (src/loss.py:74-80), produced by
EXECUTING THE REFERENCE'S OWN graph-construction and loss code through make_head_reference.py -- `load_reference()`
and `run_head_case()` exactly as they are, on the case dicts below.  Nothing of the reference is copied; only the
.npz data is committed.

    tests/golden/ref_vstep_<case>.npz        small cases: every tensor in full
    tests/golden/ref_vstep_big_<case>.npz    benchmark shape (8 clips x 4 frames x 14 x 14 x 2048, K = 51): inputs by
                                             seed, large tensors as digest + sample (run_head_case, big=True)

Every case carries libmask=(seed, offset): the dropout mask is the library's own counter stream over the flat
[B*F,H,W,C] draw, so the one-call steps run these fixtures with their hash and no replayed mask.
The prefix keeps these files out of the globs of the existing fixture tests (ref_head_*, refbig_*, ref_pal_*).

Run in the build container (the GPU box has no reference tree):
    python tests/golden/make_video_step_reference.py            # the small cases
    python tests/golden/make_video_step_reference.py big        # + the benchmark-shape cases
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_head_reference as mhr          # noqa: E402
import make_pose_att_reference as mpar     # noqa: E402  (digest_large_outputs)

P, SL, NOPOSE = mhr.P, mhr.SL, mhr.NOPOSE
Y003 = '003_MPII_ResNet_withPoseAttention.yaml'
TATT = dict(USE_TEMPORAL_ATT=True)
CASES = [
    # plain mean over the frames, single-layer attention from the map itself, no pose loss
    dict(name='framepool_train', train=True, shape=(2, 3, 3, 3, 32), K=51, train_cfg=NOPOSE, net=SL, libmask=(42, 45)),
    # + the TemporalAttention conv (pose L2 loss on the pruned PoseLogits branch stays off: NOPOSE)
    dict(name='temporal_att_train', train=True, shape=(2, 3, 3, 3, 32), K=51, train_cfg=NOPOSE,
         net=dict(SL, **TATT), libmask=(42, 49)),
    dict(name='perclass_temporal_train', train=True, shape=(3, 2, 3, 3, 32), K=12, train_cfg=NOPOSE,
         net=dict(SL, **dict(TATT, **{P + '_PER_CLASS': True})), libmask=(42, 53)),
    # bf16-representable values at C = 256, K <= 64: the fused per-class kernels
    dict(name='perclass_framepool_bf16_c256', train=True, shape=(2, 3, 3, 3, 256), K=51, train_cfg=NOPOSE,
         net=dict(SL, **{P + '_PER_CLASS': True}), quant='bf16', libmask=(42, 57)),
    # cfg 003: attention from pose_pre_logits, pose L2 loss per FRAME
    dict(name='cfg003_temporal_train', yaml=Y003, train=True, shape=(2, 3, 3, 3, 32), K=20, net=TATT,
         libmask=(42, 61)),
    dict(name='cfg003_one_clip_f5', yaml=Y003, train=True, shape=(1, 5, 3, 3, 32), K=20, libmask=(42, 65)),
    # (W1 [512,768] and its gradient would make this file 2.4 MB in full: stored in the benchmark cases' compact form,
    # weights by seed and tensors above 2^16 elements as digest + sample -- a small case all the same)
    dict(name='cfg003_framepool_bf16_c512', yaml=Y003, train=True, shape=(2, 2, 3, 3, 512), K=20, quant='bf16',
         gate_safe=True, libmask=(42, 69), big=True, full_limit=1 << 16),
]
# the benchmark's clip batch: 8 clips x 4 frames of 14 x 14 x 2048, HMDB-51's 51 classes, temporal attention on
BIG_CASES = [
    dict(name='hmdb51_perclass_8x4_libmask', train=True, shape=(8, 4, 14, 14, 2048), K=51, train_cfg=NOPOSE,
         net=dict(SL, **dict(TATT, **{P + '_PER_CLASS': True})), libmask=(42, 73), big=True, quant='bf16',
         full_limit=1 << 16, benchmark=True),
    dict(name='cfg003_8x4_libmask', yaml=Y003, train=True, shape=(8, 4, 14, 14, 2048), K=51, net=TATT,
         libmask=(42, 77), big=True, quant='bf16', gate_safe=True, full_limit=1 << 17, benchmark=True),
]


def main():
    want_big = 'big' in sys.argv[1:]
    only = set(a for a in sys.argv[1:] if a != 'big')
    cfgmod, nf, lossmod = mhr.load_reference()
    defaults = copy.deepcopy(cfgmod.cfg)
    for case in CASES + (BIG_CASES if want_big else []):
        if only and case['name'] not in only:
            continue
        case = dict(case, name='vstep_' + case['name'])     # the name keys the seeded draws of the generator
        out = mhr.run_head_case(cfgmod, nf, lossmod, defaults, case)
        if case.get('big'):
            mpar.digest_large_outputs(out)
        dst = os.path.join(HERE, ('ref_vstep_big_%s.npz' if case.get('benchmark') else 'ref_vstep_%s.npz') %
                           case['name'][len('vstep_'):])
        np.savez_compressed(dst, **out)
        meta = json.loads(str(out['meta']))
        print('%-44s %8.1f KB  vars: %s' % (case['name'], os.path.getsize(dst) / 1024, ', '.join(meta['var_order'])))


if __name__ == '__main__':
    main()
