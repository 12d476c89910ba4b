"""The input pipeline of src/preprocess_pipeline.py on the device: one geometry per sample, handed to BOTH halves.

The reference runs `image_preprocessing_fn` (models/slim/preprocessing/vgg_preprocessing.py for resnet_v1_*, vgg_*
and inception_v2_tsn, preprocessing_factory.py:52-62) on the image, records what it did in `preproc_info`, and
replays crop and flip on the pose heat-maps (`_replay_augmentation`, :21-45).  Here the geometry is drawn FIRST, as
the int32 [9] record (im_ht, im_wd, aug_ht, aug_wd, crop_y, crop_x, crop_h, crop_w, flip), and the identical rows go
to `custom_ops_factory.preprocess_images` (limit, resize, crop, flip, - mean: one fused HIP op per batch) and to
`custom_ops_factory.pose_labels_device` (the label path), so the labels cannot drift from the pixels.

TF's random stream cannot be reproduced: the offsets and the flip come from `draws` or from a numpy Generator, and
`info['draws']` returns what was used ((offset_y, offset_x, u) per sample; the image is flipped when u > 0.5,
vgg_preprocessing.py:329-332).
"""
from __future__ import annotations

from typing import Mapping, Optional, Sequence

import numpy as np
import torch

from .custom_ops import custom_ops_factory as cof

# preprocessing_factory.py:52-62: the models whose preprocessing is vgg_preprocessing
VGG_PREPROCESSING_MODELS = ('inception_v2_tsn', 'resnet_v1_50', 'resnet_v1_101', 'resnet_v1_152', 'vgg', 'vgg_a',
                            'vgg_16', 'vgg_19')
MEAN = 128.0                          # vgg_preprocessing.py:45
DEFAULT_IMAGE_SIZE = 224              # network_fn.default_image_size of those models

_default_rngs = {}


def default_rng(cfg) -> np.random.Generator:
    """The generator used when neither `rng` nor `draws` is given: seeded from cfg.RNG_SEED at its first use,
    then continued from call to call."""
    seed = int(cfg.RNG_SEED)
    if seed not in _default_rngs:
        _default_rngs[seed] = np.random.default_rng(seed)
    return _default_rngs[seed]


def check_supported(cfg) -> None:
    """ValueError, naming the key, for the configurations whose input is not `vgg_preprocessing` of an RGB image."""
    if cfg.MODEL_NAME not in VGG_PREPROCESSING_MODELS:
        raise ValueError('cfg.MODEL_NAME = %r: only the vgg_preprocessing models %r are preprocessed here (%s uses '
                         'inception_preprocessing)' % (cfg.MODEL_NAME, VGG_PREPROCESSING_MODELS, cfg.MODEL_NAME))
    if str(cfg.INPUT.VIDEO.MODALITY).startswith('flow'):
        raise ValueError('cfg.INPUT.VIDEO.MODALITY = %r: optical-flow input (vgg_preprocessing.py:333-347) is not '
                         'supported' % (cfg.INPUT.VIDEO.MODALITY,))
    fmt = str(cfg.INPUT.INPUT_IMAGE_FORMAT)
    if fmt.startswith(('rendered-pose', 'pose-glimpse', 'rendered-objects')):
        raise ValueError('cfg.INPUT.INPUT_IMAGE_FORMAT = %r: rendered poses / objects and glimpses '
                         '(preprocess_pipeline.py:70-131) are not supported' % (fmt,))


def _frames(sample) -> np.ndarray:
    a = np.asarray(sample['image'])
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise ValueError("sample['image'] must be uint8 [h,w,3] or [T,h,w,3], got %s %s" % (a.dtype, a.shape))
    return a if a.ndim == 4 else a[None]


def sample_geometry(src_hw, im_hw, cfg, crop: int, draw=None, rng: Optional[np.random.Generator] = None,
                    central: bool = False, flip: bool = False):
    """-> (geom row, draw) for one sample whose frames are src_hw = (h, w) and whose stored size is im_hw.
    Training (central=False): offsets uniform in [0, ah - crop] x [0, aw - crop] and u uniform in [0, 1) from `rng`,
    or all three from `draw`; evaluation: the central crop (vgg_preprocessing.py:200-201 through to_int32) and the
    `flip` asked for.  A crop that does not fit gets offset 0: the device op reports it (status 1)."""
    lh, lw, ah, aw = cof.image_aug_size(src_hw[0], src_hw[1], cfg.MAX_INPUT_IMAGE_SIZE, cfg.TRAIN.RESIZE_SIDE)
    if central:
        oy, ox, u = int((ah - crop) / 2), int((aw - crop) / 2), (1.0 if flip else 0.0)
    elif draw is not None:
        oy, ox, u = int(draw[0]), int(draw[1]), float(draw[2])
    else:
        oy = int(rng.integers(0, ah - crop + 1)) if ah >= crop else 0      # random_uniform([], maxval=h - crop + 1)
        ox = int(rng.integers(0, aw - crop + 1)) if aw >= crop else 0
        u = float(rng.random())
    geom = [int(im_hw[0]), int(im_hw[1]), ah, aw, oy, ox, int(crop), int(crop), int(u > 0.5)]
    return geom, (oy, ox, u)


def _run_images(samples, geoms, cfg, device, out_dtype, on_error):
    frames = [_frames(s) for s in samples]
    images, status = cof.preprocess_images(frames, geoms, cfg.MAX_INPUT_IMAGE_SIZE, out_dtype=out_dtype,
                                           device=device, mean=MEAN)
    return images, status


def _check_status(status_list, names, on_error):
    if on_error == 'zero':
        return
    if on_error != 'raise':
        raise ValueError("on_error must be 'raise' or 'zero'")
    for name, st in zip(names, status_list):
        bad = [i for i, v in enumerate(st.cpu().tolist()) if v]
        if bad:
            raise ValueError('%s preprocessing failed for sample(s) %r (crop outside the resized image, or bad '
                             'sizes); on_error="zero" returns zeros instead' % (name, bad))


def _action_labels(samples, device):
    return torch.as_tensor(np.stack([np.asarray(s['action_label']) for s in samples])).to(device)


def train_preprocess_pipeline(samples: Sequence[Mapping], cfg, num_pose_keypoints: int,
                              rng: Optional[np.random.Generator] = None, draws=None, device='cuda',
                              out_dtype=torch.float32, on_error: str = 'raise'):
    """src/preprocess_pipeline.py:135-219 for a batch.  A sample is a mapping with `image` (uint8 [h,w,3] or
    [T,h,w,3]), `pose` (int64 (x, y, visible) triples; a list of T such arrays for a video), `im_ht`, `im_wd` (the
    size the keypoints refer to) and `action_label`.
    Returns (images [N,T,S,S,3], pose_label_hmap [N,T,s,s,J], pose_label_valid [N,T,J], action_labels, info) with
    S = cfg.TRAIN.IMAGE_SIZE, s = cfg.TRAIN.FINAL_POSE_HMAP_SIDE; the two label tensors are empty when
    num_pose_keypoints == 0 or cfg.TRAIN.LOSS_FN_POSE == '' (:150, :216-217).  info: 'geom' (the rows both ops
    received), 'draws', 'status' (device int32 [N]) and 'label_status' (device int32 [N*T] or None)."""
    check_supported(cfg)
    N = len(samples)
    if draws is not None and len(draws) != N:
        raise ValueError('%d draws for %d samples' % (len(draws), N))
    if draws is None and rng is None:
        rng = default_rng(cfg)
    crop = int(cfg.TRAIN.IMAGE_SIZE or DEFAULT_IMAGE_SIZE)
    geoms, used = [], []
    for i, s in enumerate(samples):
        g, d = sample_geometry(_frames(s).shape[1:3], (s['im_ht'], s['im_wd']), cfg, crop,
                               draw=None if draws is None else draws[i], rng=rng)
        geoms.append(g)
        used.append(d)
    images, status = _run_images(samples, geoms, cfg, device, out_dtype, on_error)
    T = images.shape[1]
    label_status = None
    if num_pose_keypoints > 0 and not cfg.TRAIN.LOSS_FN_POSE == '':          # :150
        side = int(cfg.TRAIN.FINAL_POSE_HMAP_SIDE)
        poses, rows = [], []
        for s, g in zip(samples, geoms):
            pl = s['pose'] if isinstance(s['pose'], (list, tuple)) else [s['pose']]
            if len(pl) != T:
                raise ValueError('a sample with %d frames needs %d pose labels, got %d' % (T, T, len(pl)))
            poses += list(pl)
            rows += [g] * T                                                  # one geometry over the frames (:182-196)
        hmap, valid, label_status = cof.pose_labels_device(
            poses, rows, out_wd=max(200, side), J=num_pose_keypoints,
            marker_wd_ratio=cfg.HEATMAP_MARKER_WD_RATIO, out_side=side, device=device)
        hmap = hmap.view(N, T, side, side, num_pose_keypoints)
        valid = valid.view(N, T, num_pose_keypoints)
    else:
        hmap = torch.zeros((0,), device=device)                              # dummy values, not used (:216-217)
        valid = torch.zeros((0,), device=device)
    _check_status([status] + ([label_status] if label_status is not None else []), ['image', 'label'], on_error)
    info = {'geom': geoms, 'draws': used, 'status': status, 'label_status': label_status}
    return images, hmap, valid, _action_labels(samples, device), info


def eval_preprocess_pipeline(samples: Sequence[Mapping], cfg, flip: bool = False, device='cuda',
                             out_dtype=torch.float32, on_error: str = 'raise'):
    """src/eval.py:135-158 for a batch: limit, resize to cfg.TRAIN.RESIZE_SIDE, CENTRAL crop of cfg.TRAIN.IMAGE_SIZE,
    - mean; `flip=True` mirrors every image (the 'flips' preproc).  Returns (images [N,T,S,S,3], action_labels, info)."""
    check_supported(cfg)
    crop = int(cfg.TRAIN.IMAGE_SIZE or DEFAULT_IMAGE_SIZE)
    geoms = []
    for s in samples:
        f = _frames(s)
        im_hw = (s.get('im_ht', f.shape[1]), s.get('im_wd', f.shape[2]))
        geoms.append(sample_geometry(f.shape[1:3], im_hw, cfg, crop, central=True, flip=flip)[0])
    images, status = _run_images(samples, geoms, cfg, device, out_dtype, on_error)
    _check_status([status], ['image'], on_error)
    return images, _action_labels(samples, device), {'geom': geoms, 'status': status}
