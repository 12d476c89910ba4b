#!/usr/bin/env python
"""Golden vectors for TRAIN.TRAINABLE_SCOPES (src/train.py:166-181 -> optimize_clones(var_list=...), :504-513),
produced by the REFERENCE'S OWN training code through make_train_reference.py -- `load_training_reference()` and
`run_train_case()` exactly as they are, on the case dicts below.  A variable outside the listed scopes gets no
gradient, no L2 step and no optimiser slot; the regularisation VALUE still counts every conv weight.
`tf.get_collection(key, scope)` is a prefix match on the variable name: 'PosePrelogitsBasedAttention/Conv' also takes
'PosePrelogitsBasedAttention/Conv2d_PrePose_Attn/*' (asserted below).

    tests/golden/ref_scopes_<case>.npz    the layout of ref_train_*.npz (tests/_ref_fixture.TrainFixture); the
                                          clipped case also carries meta['clip_norms'] like ref_clip_*.npz

The prefix keeps these files out of the ref_train_* / ref_clip_* globs of the existing training tests.

Run in the build container (the GPU box has no reference tree):
    python tests/golden/make_scopes_reference.py
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_train_reference as mtr   # noqa: E402
import make_clip_reference as mcr    # noqa: E402

Y002 = '002_MPII_ResNet_withAttention.yaml'
Y003 = '003_MPII_ResNet_withPoseAttention.yaml'
ATT = 'PosePrelogitsBasedAttention'
CASES = [
    # cfg 002, one clone: only the attention scope trains, the pruned PoseLogits convs must not decay
    dict(name='cfg002_1clone_iter2_att', yaml=Y002, gpus='0', steps=3, batch=2, shape=(1, 4, 4, 32), K=12,
         net={'DROPOUT': 0.0},
         train_cfg={'ITER_SIZE': 2, 'LEARNING_RATE': 0.05, 'NUM_STEPS_PER_DECAY': 2, 'WEIGHT_DECAY': 0.01,
                    'TRAINABLE_SCOPES': ATT},
         trained=4, frozen=['PoseLogits/ExtraConv2d_1x1/weights', 'PoseLogits/Conv2d_1c_1x1/weights']),
    # cfg 003, two clones, a list with blanks: the prefix rule takes both attention convs; Conv2d_1c_1x1 is frozen
    dict(name='cfg003_2clones_prefix', yaml=Y003, gpus='0,1', steps=2, batch=2, shape=(1, 3, 4, 16), K=10,
         net={'DROPOUT': 0.0},
         train_cfg={'ITER_SIZE': 1, 'LEARNING_RATE': 0.02, 'NUM_STEPS_PER_DECAY': 1, 'WEIGHT_DECAY': 0.005,
                    'TRAINABLE_SCOPES': ATT + '/Conv, PoseLogits/ExtraConv2d_1x1'},
         trained=6, frozen=['PoseLogits/Conv2d_1c_1x1/weights', 'PoseLogits/Conv2d_1c_1x1/biases']),
    # cfg 003 with TRAIN.CLIP_GRADIENTS: the pose head and the attention conv train, the top-down conv is frozen
    dict(name='cfg003_1clone_iter3_clip', yaml=Y003, gpus='0', steps=2, batch=2, shape=(1, 3, 4, 16), K=10,
         net={'DROPOUT': 0.0},
         train_cfg={'ITER_SIZE': 3, 'LEARNING_RATE': 0.02, 'NUM_STEPS_PER_DECAY': 1, 'WEIGHT_DECAY': 0.005,
                    'CLIP_GRADIENTS': 1.0, 'TRAINABLE_SCOPES': 'PoseLogits,' + ATT + '/Conv2d_PrePose_Attn'},
         trained=6, frozen=[ATT + '/Conv/weights', ATT + '/Conv/biases']),
    # video clips with the TemporalAttention conv built but left out of the scope list (dropout on)
    dict(name='cfg002_temporal_frozen', yaml=Y002, gpus='0', steps=2, batch=2, shape=(3, 3, 3, 16), K=7,
         net={'DROPOUT': 0.5, 'USE_TEMPORAL_ATT': True},
         train_cfg={'ITER_SIZE': 1, 'LEARNING_RATE': 0.05, 'NUM_STEPS_PER_DECAY': 1, 'WEIGHT_DECAY': 0.01,
                    'TRAINABLE_SCOPES': ATT + ',PoseLogits'},
         trained=6, frozen=['TemporalAttention/Conv/weights', 'TemporalAttention/Conv/biases']),
]


def generate(names=None):
    loaded = mtr.load_training_reference()
    mcr.attach()                      # slim.learning.clip_gradient_norms for the clipped case
    cfgmod = loaded[0]
    defaults = copy.deepcopy(cfgmod.cfg)
    res = {}
    for case in CASES:
        if names is not None and case['name'] not in names:
            continue
        del mcr.CALLS[:]
        run = {k: v for k, v in case.items() if k not in ('trained', 'frozen')}
        out = mtr.run_train_case(*loaded, defaults, run)
        meta = json.loads(str(out['meta']))
        assert meta['train_cfg']['TRAINABLE_SCOPES'] == case['train_cfg']['TRAINABLE_SCOPES']
        assert len(meta['grad_vars']) == case['trained'], meta['grad_vars']
        last = len(meta['steps']) - 1
        for vn in case['frozen']:
            assert vn in meta['var_order'] and vn not in meta['grad_vars']
            assert 'final/momentum/' + vn not in out
            assert np.array_equal(out['step/%d/var/%s' % (last, vn)], out['var0/' + vn].astype(np.float64)), vn
        for r in meta['runs']:        # the regularisation VALUE still counts every conv weight
            assert len(r['reg_losses']) == sum(vn.endswith('/weights') for vn in meta['var_order'])
        if float(case['train_cfg'].get('CLIP_GRADIENTS', 0)) > 0:
            nc = meta['num_clones']
            calls = mcr.CALLS[nc:]
            assert len(calls) == nc * len(meta['runs'])
            meta['clip_norms'] = [calls[r * nc:(r + 1) * nc] for r in range(len(meta['runs']))]
            clip = float(case['train_cfg']['CLIP_GRADIENTS'])
            norms = [n for run_ in meta['clip_norms'] for cl in run_ for n in cl.values()]
            assert min(norms) < clip < max(norms), (min(norms), max(norms))
            # a file stays under 1 MB: the summed clone gradients of the FIRST update's runs only, as in ref_clip_*
            keep = set(meta['steps'][0]['runs'])
            for k in [k for k in out if k.startswith('run/') and int(k.split('/')[1]) not in keep]:
                del out[k]
            meta['grad_runs'] = sorted(keep)
            out['meta'] = np.array(json.dumps(meta, sort_keys=True, default=str))
        res[case['name']] = out
    return res


if __name__ == '__main__':
    for name, blobs in generate(sys.argv[1:] or None).items():
        path = os.path.join(HERE, 'ref_scopes_%s.npz' % name)
        np.savez_compressed(path, **blobs)
        m = json.loads(str(blobs['meta']))
        print('%-32s %7d bytes  clones %d  iter %d  scopes %r\n    trained: %s' % (
            name, os.path.getsize(path), m['num_clones'], m['iter_size'], m['train_cfg']['TRAINABLE_SCOPES'],
            ', '.join(m['grad_vars'])))
