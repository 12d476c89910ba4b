#!/usr/bin/env python
"""Golden vectors for TRAIN.CLIP_GRADIENTS (per-variable clip-by-norm of every clone's gradient), produced by the
REFERENCE'S OWN training code through make_train_reference.py -- `load_training_reference()` and `run_train_case()`
exactly as they are, on the case dicts below.  model_deploy.optimize_clones (executed from the reference tree) calls

    slim.learning.clip_gradient_norms(clone_grad, clip_gradients)        (model_deploy.py:301-304)

on each clone's (gradient, variable) list when clip_gradients > 0.  That function and tf.clip_by_norm are
TensorFlow's (third-party, not in the reference tree) and are restated here, attached to the shim's modules after
loading; tf1_shim.py and make_train_reference.py are not changed.  TF 1.x's clip_by_norm, in its own order:

    l2norm_inv   = rsqrt(reduce_sum(t * t))          # over the whole tensor
    intermediate = t * c
    tclip        = intermediate * minimum(l2norm_inv, 1.0 / c)

and clip_gradient_norms applies it to every gradient that is not None, leaving the pairs in order.

    tests/golden/ref_clip_<case>.npz      the layout of ref_train_*.npz (tests/_ref_fixture.TrainFixture), plus
                                          meta['clip_norms']: per session.run, per clone, {variable: pre-clip norm};
                                          the summed clone gradients only for the runs of the first update
                                          (meta['grad_runs'])

The prefix keeps these files out of the ref_train_* glob of the existing training tests.

Run in the build container (the GPU box has no reference tree):
    python tests/golden/make_clip_reference.py
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_train_reference as mtr   # noqa: E402
import tf1_shim as tfs               # noqa: E402

_BASE = {c['name']: c for c in mtr.TRAIN_CASES}


def _case(base, name, clip, **train_cfg):
    c = copy.deepcopy(_BASE[base])
    c['name'] = name
    c['train_cfg'] = dict(c['train_cfg'], CLIP_GRADIENTS=clip, **train_cfg)
    return c


# clip values sit between the smallest and the largest per-variable norm of every run (asserted below)
CASES = [
    _case('cfg002_2clones_iter2', 'cfg002_2clones_iter2', 0.1),
    # pose L2 loss on: the pose head's weights and the regulariser are inside the clip
    _case('cfg003_1clone_iter3', 'cfg003_1clone_iter3', 1.0),
    # a weight decay large enough that the regulariser-only PoseLogits weights are themselves clipped
    _case('cfg002_1clone_iter1_epoch_decay', 'cfg002_1clone_iter1_bigwd', 0.5, WEIGHT_DECAY=0.5),
    _case('cfg002_2clones_iter2_dropout', 'cfg002_2clones_iter2_dropout', 0.1),
]

CALLS = []          # one entry per clip_gradient_norms call: {variable: pre-clip norm}


def clip_by_norm(t, clip_norm, axes=None, name=None):
    """tf.clip_by_norm (TF 1.x clip_ops.py), restated: (t * c) * minimum(rsqrt(sum(t * t)), 1 / c)"""
    assert axes is None
    v = tfs._raw(t)
    c = float(clip_norm)
    l2norm_inv = torch.rsqrt((v * v).sum())
    intermediate = v * c
    return tfs.Tensor(intermediate * torch.minimum(l2norm_inv, torch.tensor(1.0 / c, dtype=v.dtype)))


def clip_gradient_norms(gradients_to_variables, max_norm):
    """slim.learning.clip_gradient_norms (TF 1.x contrib/slim/python/slim/learning.py), restated: clip_by_norm on
    every gradient that is not None; the (gradient, variable) pairs keep their order."""
    out, norms = [], {}
    for grad, var in gradients_to_variables:
        if grad is not None:
            norms[var.op.name] = float(torch.sqrt((tfs._raw(grad) ** 2).sum()))
            grad = clip_by_norm(grad, max_norm)
        out.append((grad, var))
    CALLS.append(norms)
    return out


def attach():
    tf = sys.modules['tensorflow']
    slim = sys.modules['tensorflow.contrib.slim']
    tf.clip_by_norm = clip_by_norm
    learning = types.ModuleType('tensorflow.contrib.slim.learning')
    learning.clip_gradient_norms = clip_gradient_norms
    slim.learning = learning
    sys.modules['tensorflow.contrib.slim.learning'] = learning


def generate(names=None):
    loaded = mtr.load_training_reference()
    attach()
    cfgmod = loaded[0]
    defaults = copy.deepcopy(cfgmod.cfg)
    res = {}
    for case in CASES:
        if names is not None and case['name'] not in names:
            continue
        del CALLS[:]
        out = mtr.run_train_case(*loaded, defaults, case)
        meta = json.loads(str(out['meta']))
        nc, clip = meta['num_clones'], float(case['train_cfg']['CLIP_GRADIENTS'])
        assert meta['train_cfg']['CLIP_GRADIENTS'] == clip
        calls = CALLS[nc:]                          # the first nc calls build the graph (make_train_reference)
        assert len(calls) == nc * len(meta['runs'])
        runs = [calls[r * nc:(r + 1) * nc] for r in range(len(meta['runs']))]
        for r, per_clone in enumerate(runs):
            norms = [n for cl in per_clone for n in cl.values()]
            assert min(norms) < clip < max(norms), (case['name'], r, min(norms), max(norms))
        if case['name'].endswith('bigwd'):
            pose = [vn for vn in meta['grad_vars'] if vn.startswith('PoseLogits') and vn.endswith('/weights')]
            assert pose and all(cl[vn] > clip for per_clone in runs for cl in per_clone for vn in pose)
        meta['clip_norms'] = runs
        # a file stays under 1 MB: the summed clone gradients of the FIRST update's runs are kept (the variables after
        # every update are, as in ref_train_*)
        keep = set(meta['steps'][0]['runs'])
        for k in [k for k in out if k.startswith('run/') and int(k.split('/')[1]) not in keep]:
            del out[k]
        meta['grad_runs'] = sorted(keep)
        out['meta'] = np.array(json.dumps(meta, sort_keys=True, default=str))
        res[case['name']] = out
    return res


if __name__ == '__main__':
    for name, blobs in generate(sys.argv[1:] or None).items():
        path = os.path.join(HERE, 'ref_clip_%s.npz' % name)
        np.savez_compressed(path, **blobs)
        m = json.loads(str(blobs['meta']))
        norms = [n for run in m['clip_norms'] for cl in run for n in cl.values()]
        print('%-32s %7d bytes  clones %d  iter %d  clip %g  norms %.3g .. %.3g' % (
            name, os.path.getsize(path), m['num_clones'], m['iter_size'], m['train_cfg']['CLIP_GRADIENTS'],
            min(norms), max(norms)))
