#!/usr/bin/env python
"""Golden vectors for the IMAGE half of the input pipeline, produced by the REFERENCE'S OWN code.

What is executed, from /root/reference behind the TF1 stand-in (tests/golden/tf1_shim.py, FLOAT32 mode: the
image graph is float32 and its size truncations depend on it):
  * training cases: src/preprocess_pipeline.py `train_preprocess_pipeline` (:135-219) -> `get_input` ->
    `_resize_if_needed` (:5-18), with `image_preprocessing_fn` = the REAL
    models/slim/preprocessing/vgg_preprocessing.py `preprocess_image(..., is_training=True)` -- the function
    preprocessing_factory.py:52-62,75-76 hands out for resnet_v1_*, vgg_* and inception_v2_tsn -- instead of the
    stub tests/golden/make_label_reference.py stands in for it.  The label half is switched off
    (num_pose_keypoints = 0): it has its own fixture.
  * evaluation cases: `_resize_if_needed`, then `preprocess_image(..., is_training=False,
    resize_side_min=cfg.TRAIN.RESIZE_SIDE)` as src/eval.py:135-152 calls it, then the flip-all of :155-158 when
    asked for (restated here in its two stand-in calls: that code sits inside eval.py's main()).
What is supplied: the decoded frames (seeded noise), the dataset `provider`, and the random draws -- TF's random
stream cannot be reproduced, so `tf.random_uniform` returns the numbers of the case, in the order
vgg_preprocessing.py draws them (resize side :321, offset_height :172, offset_width :174, flip :330), checks
each against the bounds the reference passed, and records them.

The stand-in lacks a few symbols vgg_preprocessing.py calls; they are added HERE, not in tf1_shim.py:
tf.Assert / rank / logical_and / greater_equal / convert_to_tensor, control_flow_ops.with_dependencies (the
assertions are evaluated eagerly, a failed one raises like the InvalidArgumentError of a session run),
tf.image.resize_bilinear, an integer `random_uniform`, and forms of tf.reshape / tf.cast / tf.image.resize_images
that take tensor-valued sizes and integer images (ResizeBilinear computes in float32 and returns float32 for a
uint8 input).

Stored per case: the frames, the draws, the integers that landed in `preproc_info` (as the geom record
[im_ht, im_wd, aug_ht, aug_wd, crop_y, crop_x, crop_h, crop_w, flip]), the uint8 image after the limit, the output.
Nothing of the reference's text is stored.

Run in the build container (it reads /root/reference):   python tests/golden/make_image_reference.py
Output: tests/golden/ref_images.npz.  Test infrastructure only.
"""
from __future__ import annotations

import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import tf1_shim as tfs                                   # noqa: E402
import make_head_reference as mhr                        # noqa: E402
import make_label_reference as mlr                       # noqa: E402

REF = mhr.REF

# name, T, source (sh, sw), MAX_INPUT_IMAGE_SIZE, RESIZE_SIDE, IMAGE_SIZE, mode, draws
CASES = [
    # limit stage + its uint8 truncation, the clamp at the last row / column of both resizes (offsets = the maxima), flip
    dict(name='a_limit_flip', T=1, src=(40, 70), max_wd=32, side=24, crop=16, train=True, off=(8, 26), flip=True),
    # to_int32 lands one short of the resize side: A is 23 x 34
    dict(name='b_short_by_one', T=1, src=(37, 53), max_wd=512, side=24, crop=16, train=True, off=(0, 0), flip=False),
    # the portrait branch of the scale
    dict(name='c_portrait', T=1, src=(53, 37), max_wd=512, side=24, crop=16, train=True, off=(9, 3), flip=False),
    # evaluation: central crop
    dict(name='d_eval_central', T=1, src=(64, 64), max_wd=512, side=24, crop=16, train=False, flip=False),
    dict(name='d_eval_central_flipped', T=1, src=(64, 64), max_wd=512, side=24, crop=16, train=False, flip=True),
    # an up-scale after a down-scale; no slack in y
    dict(name='e_up_after_down', T=1, src=(20, 90), max_wd=32, side=16, crop=16, train=True, off=(0, 57), flip=False),
    # A is 15 rows high: the size assertion fails
    dict(name='f_crop_larger_than_image', T=1, src=(41, 60), max_wd=512, side=16, crop=16, train=True, off=(0, 0),
         flip=False),
    # A fits, the offset is one past the last legal one: tf.slice refuses (the draw check is off for this case)
    dict(name='f_offset_past_the_end', T=1, src=(37, 53), max_wd=512, side=24, crop=16, train=True, off=(0, 19),
         flip=False, unchecked_draws=True),
    # one geometry over the frames of a video
    dict(name='g_video_3frames', T=3, src=(40, 70), max_wd=32, side=24, crop=16, train=True, off=(8, 26), flip=True),
    # scale exactly 1: the output is src - 128
    dict(name='i_identity', T=1, src=(64, 64), max_wd=512, side=64, crop=64, train=True, off=(0, 0), flip=False),
]


# ------------------------------------------------------------------------ what the stand-in lacks (see header)
class Draws(object):
    """tf.random_uniform: hands out the numbers of the case, in call order, checked against the bounds given."""

    def __init__(self):
        self.queue, self.log, self.checked = [], [], True

    def __call__(self, shape_, minval=0, maxval=None, dtype=None, seed=None, name=None):
        assert list(shape_) == [] and self.queue, 'unexpected random_uniform call'
        v = self.queue.pop(0)
        lo, hi = _int(minval) if dtype == 'int32' else float(minval), maxval
        if dtype == 'int32':
            hi = _int(hi)
            assert isinstance(v, int) and (not self.checked or lo <= v < hi), (v, lo, hi)
            self.log.append({'dtype': 'int32', 'minval': lo, 'maxval': hi, 'value': v})
            return tfs.Tensor(torch.tensor(v, dtype=torch.int32))
        assert dtype in (None, 'float32') and lo <= v < float(hi), (v, lo, hi)
        self.log.append({'dtype': 'float32', 'minval': lo, 'maxval': float(hi), 'value': float(v)})
        return tfs.Tensor(torch.tensor(v, dtype=tfs.DT))


def _int(x):
    return int(tfs._raw(x).item()) if isinstance(x, (tfs.Tensor, torch.Tensor)) else int(x)


def _ints(x):
    if isinstance(x, (tfs.Tensor, torch.Tensor)):
        return [int(v) for v in tfs._raw(x).reshape(-1).tolist()]
    return [_int(v) for v in x]


def tf_assert(condition, data, summarize=None, name=None):
    if not bool(tfs._raw(condition).item()):
        raise ValueError('assertion failed: ' + str(data[0]))       # InvalidArgumentError at session.run
    return None


def tf_cast(t, dtype, name=None):
    if isinstance(t, (list, tuple)):                                # e.g. tf.cast([new_ht, max_wd], tf.int32)
        t = torch.stack([tfs._raw(e).reshape(()) for e in t])
    return tfs.cast(t, dtype)


def tf_reshape(t, shape, name=None):
    return tfs.Tensor(tfs._raw(t).reshape(_ints(shape)))


def tf_convert_to_tensor(value, dtype=None, name=None):
    return value if isinstance(value, tfs.Tensor) else tfs.cast(value, dtype or 'float32')


def _resize_float(images, size):
    """ResizeBilinear: any real input type, float32 arithmetic and output; the legacy rule of the stand-in."""
    v = tfs._raw(images)
    return tfs.resize_images(tfs.Tensor(v.to(tfs.DT)), _ints(size))


def install(tf, draws):
    tf.Assert = tf_assert
    tf.rank = lambda t, name=None: tfs._raw(t).dim()
    tf.logical_and = lambda a, b, name=None: tfs.Tensor(tfs._raw(a).bool() & tfs._raw(b).bool())
    tf.greater_equal = lambda a, b, name=None: tfs.Tensor(tfs._raw(a) >= tfs._raw(b))
    tf.convert_to_tensor = tf_convert_to_tensor
    tf.cast, tf.reshape, tf.random_uniform = tf_cast, tf_reshape, draws
    tf.image.resize_images = lambda images, size, method=0, align_corners=False: _resize_float(images, size)
    tf.image.resize_bilinear = lambda images, size, align_corners=False, name=None: _resize_float(images, size)
    cfo = types.ModuleType('tensorflow.python.ops.control_flow_ops')
    cfo.with_dependencies = lambda dependencies, output_tensor, name=None: output_tensor
    sys.modules['tensorflow.python.ops'].control_flow_ops = cfo
    sys.modules['tensorflow.python.ops.control_flow_ops'] = cfo


def load():
    """-> (cfg module, preprocess_pipeline module, vgg_preprocessing module, draws, spy state)"""
    cfgmod, pp, _calls, _state = mlr.load_pipeline()
    pp._replay_augmentation = None                                   # the label half is not run here
    tf = sys.modules['tensorflow']
    draws = Draws()
    install(tf, draws)
    vgg = mhr._exec_ref(os.path.join(REF, 'models', 'slim', 'preprocessing', 'vgg_preprocessing.py'),
                        'refvggpreproc')
    spy = {}
    limit, crop, resize = pp._resize_if_needed, vgg._crop, vgg._aspect_preserving_resize

    def limit_spy(image, max_wd):
        out = limit(image, max_wd)
        spy['L'] = tfs._raw(out).numpy().copy()
        assert spy['L'].dtype == np.uint8
        return out

    def resize_spy(image, smallest_side):
        out = resize(image, smallest_side)
        spy['A_shape'] = [int(s) for s in tfs._raw(out).shape]
        assert tfs._raw(out).dtype == torch.float32
        return out

    def crop_spy(image, offset_height, offset_width, crop_height, crop_width):
        spy['crop'] = [offset_height, offset_width, crop_height, crop_width]
        return crop(image, offset_height, offset_width, crop_height, crop_width)

    pp._resize_if_needed, vgg._crop, vgg._aspect_preserving_resize = limit_spy, crop_spy, resize_spy
    return cfgmod, pp, vgg, draws, spy


def run_case(cfgmod, pp, vgg, draws, spy, c):
    cfg = cfgmod.cfg
    T, (sh, sw), crop = c['T'], c['src'], c['crop']
    frames = mlr._rs('image', c['name']).randint(0, 256, size=(T, sh, sw, 3)).astype(np.uint8)
    cfg.MAX_INPUT_IMAGE_SIZE = c['max_wd']
    cfg.TRAIN.IMAGE_SIZE = crop
    cfg.TRAIN.RESIZE_SIDE = c['side']
    cfg.TRAIN.LOSS_FN_POSE = ''
    cfg.INPUT.INPUT_IMAGE_FORMAT = 'image'
    spy.clear()
    draws.log, draws.checked = [], not c.get('unchecked_draws', False)
    image_t = tfs.Tensor(torch.from_numpy(frames if T > 1 else frames[0]))

    class Provider(object):
        def get(self, items):
            vals = {'image': image_t,
                    'pose': [tfs.Tensor(torch.zeros(0, dtype=torch.int64))] * T if T > 1
                    else tfs.Tensor(torch.zeros(0, dtype=torch.int64)),
                    'im_ht': tfs.Tensor(torch.tensor(sh, dtype=torch.int64)),
                    'im_wd': tfs.Tensor(torch.tensor(sw, dtype=torch.int64)),
                    'action_label': tfs.Tensor(torch.tensor(3, dtype=torch.int64))}
            return [vals[i] for i in items]

    info, err, out = {}, None, None
    try:
        if c['train']:
            draws.queue = [c['side'], c['off'][0], c['off'][1], 0.75 if c['flip'] else 0.25]

            def image_preprocessing_fn(image, out_h, out_w, **kwargs):        # preprocessing_factory.py:75-76
                info['preproc_info'] = kwargs['preproc_info']
                return vgg.preprocess_image(image, out_h, out_w, is_training=True, **kwargs)

            image, _hm, _valid, action = pp.train_preprocess_pipeline(
                Provider(), cfg, types.SimpleNamespace(default_image_size=224), 0, image_preprocessing_fn)
            assert int(tfs._raw(action)) == 3 and not draws.queue
            out = tfs._raw(image)
        else:
            draws.queue = []
            [image, _action] = pp.get_input(Provider(), cfg, ['image', 'action_label'])          # eval.py:135-136
            image = vgg.preprocess_image(image, crop, crop, is_training=False,                   # :149-152
                                         resize_side_min=cfg.TRAIN.RESIZE_SIDE,
                                         resize_side_max=cfg.TRAIN.RESIZE_SIDE)
            if c['flip']:                                                                        # :155-158
                image = tfs.flip_left_right(image)
            out = tfs._raw(image).unsqueeze(0)
    except ValueError as e:
        err = str(e)

    blobs = {'in/frames': frames}
    if sw > c['max_wd']:
        blobs['in/L'] = spy['L'] if T > 1 else spy['L'][None]      # uint8 [T, lh, lw, 3]; otherwise L is the source
    else:
        assert np.array_equal(spy['L'], frames if T > 1 else frames[0])
    meta = {'T': T, 'max_wd': c['max_wd'], 'side': c['side'], 'crop': crop, 'train': c['train'],
            'flip_all': bool(c['flip']) and not c['train'], 'draws': list(draws.log), 'raises': err,
            'limited_shape': [int(s) for s in spy['L'].shape[-3:-1]], 'aug_shape': spy.get('A_shape')}
    if c['train'] and 'crop_info' in info.get('preproc_info', {}):
        pi = info['preproc_info']
        assert list(pi['image_shape']) == spy['A_shape'] and spy['A_shape'][2] == 3 * T
        ci = _ints(pi['crop_info'])
        flip = bool(tfs._raw(pi['whether_flip']).item()) if 'whether_flip' in pi else bool(c['flip'])
        geom = [sh, sw] + spy['A_shape'][:2] + ci + [int(flip)]
    elif 'crop' in spy:
        geom = [sh, sw] + spy['A_shape'][:2] + [_int(tfs.to_int32(v)) for v in spy['crop'][:2]] + \
            [_int(v) for v in spy['crop'][2:]] + [int(c['flip'])]
    else:                                               # the size assertion fired before any crop was recorded
        geom = [sh, sw] + spy['A_shape'][:2] + [c['off'][0], c['off'][1], crop, crop, int(c['flip'])]
    blobs['in/geom'] = np.asarray(geom, dtype=np.int32)
    if err is None:
        assert out.dtype == torch.float32 and list(out.shape) == [T, crop, crop, 3], out.shape
        blobs['out/images'] = out.numpy().copy()
    blobs['meta'] = np.asarray(json.dumps(meta, sort_keys=True))
    return blobs


def generate():
    prev = tfs.DT
    tfs.set_float_dtype(torch.float32)
    tfs.set_graph(tfs.Graph(None, None))                # scopes only: no variables; the draws are supplied
    try:
        cfgmod, pp, vgg, draws, spy = load()
        base = copy.deepcopy(cfgmod.cfg)
        blobs = {}
        for c in CASES:
            cfgmod.cfg.clear()
            cfgmod.cfg.update(copy.deepcopy(base))
            for k, v in run_case(cfgmod, pp, vgg, draws, spy, c).items():
                blobs['{}/{}'.format(c['name'], k)] = v
        blobs['cases'] = np.asarray(json.dumps([c['name'] for c in CASES]))
        return blobs
    finally:
        tfs.set_float_dtype(prev)
        tfs.set_graph(None)


if __name__ == '__main__':
    blobs = generate()
    path = os.path.join(HERE, 'ref_images.npz')
    np.savez_compressed(path, **blobs)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(CASES), 'cases')
    for c in CASES:
        m = json.loads(str(blobs[c['name'] + '/meta']))
        print(' ', c['name'], 'L', m['limited_shape'], 'A', m['aug_shape'], 'geom', blobs[c['name'] + '/in/geom'].tolist(),
              'raises' if m['raises'] else '')
