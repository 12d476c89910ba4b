#!/usr/bin/env python
"""Golden vectors for the pose-heatmap attention head (cfg.NET.USE_POSE_ATTENTION_LOGITS, the reference's
nets_factory.py:162-189), produced by EXECUTING THE REFERENCE'S OWN graph-construction and loss code through
make_head_reference.py -- `load_reference()` and `run_head_case()` exactly as they are, on the case dicts below.
Nothing of the reference is copied; only the .npz data is committed.

    tests/golden/ref_pal_<case>.npz        small cases: every tensor in full, the dropout mask as packed bits
    tests/golden/ref_pal_big_<case>.npz    benchmark shape (32 x 14 x 14 x 2048, K = 393): inputs by seed, the
                                           dropout mask = the library's own stream (libmask), large tensors as
                                           digest + sample (make_head_reference.run_head_case, big=True)

The prefix keeps these files out of the globs of the existing fixture tests (ref_head_*, refbig_*).

Run in the build container (the GPU box has no reference tree):
    python tests/golden/make_pose_att_reference.py            # the small cases
    python tests/golden/make_pose_att_reference.py big        # + the benchmark-shape cases
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import apa_digest                   # noqa: E402
import make_head_reference as mhr   # noqa: E402

PA = 'USE_POSE_ATTENTION_LOGITS'
NOPOSE = mhr.NOPOSE
CASES = [
    # the default: all 16 parts + the constant map (M = 17), pose L2 loss (cfg.TRAIN default), dropout 0.2
    dict(name='train', train=True, shape=(2, 4, 4, 32), K=51, net={PA: True}),
    dict(name='eval', train=False, shape=(2, 3, 4, 32), K=20, net={PA: True}),
    # numpy indexing of the part list: a negative index and a repeat; plus the averaged map (M = 5)
    dict(name='dims_neg_repeat_avged_train', train=True, shape=(2, 3, 3, 16), K=12,
         net={PA: True, PA + '_DIMS': [-2, 4, 4], PA + '_AVGED_HMAP': True}),
    # no part at all: the constant map alone (M = 1)
    dict(name='dims_empty_train', train=True, shape=(2, 3, 3, 16), K=10, net={PA: True, PA + '_DIMS': []}),
    dict(name='dropout_half_train', train=True, shape=(2, 4, 3, 16), K=20, net={PA: True, 'DROPOUT': 0.5}),
    dict(name='no_pose_loss_train', train=True, shape=(2, 3, 3, 16), K=20, train_cfg=NOPOSE, net={PA: True}),
    # the cfg 003 YAML (USE_POSE_PRELOGITS_BASED_ATTENTION) plus the flag: the reference's if/elif takes this head
    dict(name='cfg003_precedence_train', yaml='003_MPII_ResNet_withPoseAttention.yaml', train=True,
         shape=(2, 3, 3, 16), K=51, net={PA: True}),
    # LAST_CONV_MAP_FOR_POSE names another end point (inception_v2_tsn: 5a vs 5b)
    dict(name='separate_pose_tap_train', model='inception_v2_tsn', train=True, shape=(2, 3, 3, 16), K=20,
         pose_tap_channels=24, net={PA: True}),
    # 5-D video input: frames folded into the batch, logits averaged over the frames (:121-125, :354-374)
    dict(name='video_train', train=True, shape=(2, 3, 3, 3, 16), K=20, net={PA: True}),
    # bf16-representable inputs and variables: run through the bf16 kernels
    dict(name='dims_avged_bf16_train', train=True, shape=(2, 3, 4, 32), K=20, quant='bf16',
         net={PA: True, PA + '_DIMS': [3, 0, 9], PA + '_AVGED_HMAP': True}),
]
# the benchmark shape; quant='bf16' makes the one fixture serve the fp32 and the bf16 kernels alike; gate_safe: no
# pixel of the pose head's hidden ReLU sits within 1e-5 of its kink (make_head_reference.gate_safe_inputs)
BIG_CASES = [
    dict(name='train_baseline_libmask', train=True, shape=(32, 14, 14, 2048), K=393, net={PA: True},
         libmask=(42, 37), big=True, quant='bf16', gate_safe=True, full_limit=1 << 17),
    dict(name='train_15x15_libmask', train=True, shape=(32, 15, 15, 2048), K=393, net={PA: True},
         libmask=(42, 41), big=True, quant='bf16', gate_safe=True, full_limit=1 << 17),
]
# full_limit = 2^17 keeps the pose labels (an input the reader needs whole) in full; the PoseLogits end point, an
# output of the same size, is then stored as digest + sample like every other large output, so that a fixture stays
# well under 1 MB
DIGESTED_OUTPUTS = ('out/ep/PoseLogits',)


def digest_large_outputs(out):
    for key in DIGESTED_OUTPUTS:
        if key in out:
            arr = out.pop(key)
            out['digest/' + key] = apa_digest.digest(arr)
            out['sample/' + key] = apa_digest.sample(arr)


def main():
    want_big = 'big' in sys.argv[1:]
    only = set(a for a in sys.argv[1:] if a != 'big')
    cfgmod, nf, lossmod = mhr.load_reference()
    defaults = copy.deepcopy(cfgmod.cfg)
    for case in CASES + (BIG_CASES if want_big else []):
        if only and case['name'] not in only:
            continue
        case = dict(case, name='pal_' + case['name'])     # the name keys the seeded draws of the generator
        out = mhr.run_head_case(cfgmod, nf, lossmod, defaults, case)
        if case.get('big'):
            digest_large_outputs(out)
        dst = os.path.join(HERE, ('ref_pal_big_%s.npz' if case.get('big') else 'ref_pal_%s.npz') %
                           case['name'][len('pal_'):])
        np.savez_compressed(dst, **out)
        meta = json.loads(str(out['meta']))
        print('%-36s %8.1f KB  vars: %s' % (case['name'], os.path.getsize(dst) / 1024, ', '.join(meta['var_order'])))


if __name__ == '__main__':
    main()
