#!/usr/bin/env python
"""Golden vectors for the overlaid heat-map (include/apa.h: apa_attention_overlay), produced by the REFERENCE'S OWN code.

What is executed from /root/reference (behind tests/golden/tf1_shim.py, evaluated in FLOAT32 -- the summary graph is
float32): src/train.py `_gen_overlayed_img` (:184-195), taken out of the file by `ast` (the file cannot be imported:
dataset / queue / session code), as make_train_reference.py does for the training pieces.

What this script supplies itself, because the shim has no stand-in for them (tf1_shim.py is not edited): TensorFlow's
own (third-party) image helpers, restated from TF 1.1's python/ops/image_ops_impl.py --
  * tf.image.rgb_to_grayscale: convert_image_dtype to float32 (the identity for a float32 image), reduce_sum over
    flt_image * [0.2989, 0.5870, 0.1140] on the channel axis with keep_dims, cast back (the identity again);
  * tf.image.grayscale_to_rgb: tile the last axis three times;
  * tf.tile.
tf.image.resize_images, tf.expand_dims, tf.concat, tf.name_scope, the arithmetic and the slicing are the shim's.

Inputs are seeded (tests/_explain_reference.py: OVERLAY_CASES / overlay_inputs) and stored as seed + checksum; the
expected float overlays are stored in full (float32: a float32 execution).  The uint8 form is this project's own rule
and has no expected values here; what is checked here is the condition it puts on the INPUTS: at most 1 % of an image's
values v * s + o (float64) within 2^-10 of an integer.

Run in the build container:   python tests/golden/make_overlay_reference.py
Output: tests/golden/ref_overlay.npz.  Test infrastructure only.
"""
from __future__ import annotations

import ast
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tf1_shim as tfs                                   # noqa: E402
from tests import _explain_reference as er               # noqa: E402

REF = '/root/reference'
TRAIN_PY = os.path.join(REF, 'src', 'train.py')


# ------------------------------------------------------------------ TensorFlow helpers the shim does not have
def rgb_to_grayscale(images, name=None):
    v = tfs._raw(images)
    w = tfs._raw([0.2989, 0.5870, 0.1140], like=v)
    p = v * w
    return tfs.Tensor(((p[..., 0] + p[..., 1]) + p[..., 2]).unsqueeze(-1))      # reduce_sum, keep_dims, in that order


def grayscale_to_rgb(images, name=None):
    return tile(images, [1] * (tfs._raw(images).dim() - 1) + [3])


def tile(t, multiples, name=None):
    return tfs.Tensor(tfs._raw(t).repeat(*[int(m) for m in multiples]))


def load_gen_overlayed_img():
    tree = ast.parse(open(TRAIN_PY).read(), TRAIN_PY)
    node = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == '_gen_overlayed_img']
    assert len(node) == 1
    tf = tfs.build_modules()['tensorflow']
    tf.tile = tile
    tf.image.rgb_to_grayscale = rgb_to_grayscale
    tf.image.grayscale_to_rgb = grayscale_to_rgb
    ns = {'tf': tf, '__name__': 'refoverlay'}
    mod = ast.Module(body=node, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, TRAIN_PY, 'exec'), ns)
    return ns['_gen_overlayed_img']


def generate():
    fn = load_gen_overlayed_img()
    old = tfs.DT
    tfs.set_float_dtype(torch.float32)
    out, meta = {}, []
    try:
        for case in er.OVERLAY_CASES:
            maps, images = er.overlay_inputs(case)
            img = tfs.Tensor(torch.from_numpy(images))
            exp = np.empty((case['N'], case['T'], case['H'], case['W'], 3), dtype=np.float32)
            for t in range(case['T']):                  # train.py:205-211: one [N,h,w] map per call
                r = fn(tfs.Tensor(torch.from_numpy(np.ascontiguousarray(maps[:, t]))), img)
                assert r.v.dtype == torch.float32 and tuple(r.v.shape) == exp[:, t].shape
                exp[:, t] = r.v.numpy()
            # the restatement agrees with the execution, and the inputs meet the uint8 test's condition
            v, mag = er.overlay_reference(maps, images)
            assert (np.abs(exp.astype(np.float64) - v) <= er.overlay_bound(mag)).all(), case['name']
            _, q = er.overlay_u8_reference(v)
            share = er.u8_band(q).reshape(case['N'], case['T'], -1).mean(-1)
            assert float(share.max()) <= er.BAND_SHARE, (case['name'], float(share.max()))
            flat = v.reshape(case['N'], case['T'], -1)
            branch = 'lo<0' if (flat.min(-1) < 0).all() else ('lo>=0' if (flat.min(-1) >= 0).all() else 'mixed')
            out['expected/' + case['name']] = exp
            meta.append(dict(case, crc=er.checksum(maps, images), band_share=float(share.max()), branch=branch))
    finally:
        tfs.set_float_dtype(old)
    out['meta'] = np.array(json.dumps(dict(cases=meta, source='src/train.py:_gen_overlayed_img', dtype='float32'),
                                      sort_keys=True))
    return out


if __name__ == '__main__':
    blobs = generate()
    path = os.path.join(HERE, 'ref_overlay.npz')
    np.savez_compressed(path, **blobs)
    for c in json.loads(str(blobs['meta']))['cases']:
        print('%-24s crc %08x  %s  band share %.4f' % (c['name'], c['crc'], c['branch'], c['band_share']))
    print('%s: %d bytes' % (path, os.path.getsize(path)))
