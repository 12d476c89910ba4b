"""Vectorised numpy float32 restatement of the reference's image preprocessing, for shapes beyond the fixture
tests/golden/ref_images.npz (which pins THIS file to the reference's own code, bit for bit:
tests/test_image_preproc_cpu.py::test_restatement_reproduces_every_fixture_output):

  1. limit   src/preprocess_pipeline.py:5-18 `_resize_if_needed`
  2. resize  models/slim/preprocessing/vgg_preprocessing.py:241-294 `_aspect_preserving_resize`
  3. crop    :52-205     4. flip  :329-332 / src/eval.py:155-158     5. mean  :45, :352, :372

Every intermediate is float32 and every `a + b * c` is two roundings (numpy never fuses them).  Test
infrastructure only: the product never imports it."""
import numpy as np

F = np.float32
MEAN = 128.0


def limit_size(sh, sw, max_wd):
    """(lh, lw) of `_resize_if_needed` (:7-11)."""
    if sw > max_wd:
        return int(np.int64(F(sh) * (F(max_wd) / F(sw)))), int(max_wd)
    return int(sh), int(sw)


def aug_size(lh, lw, side):
    """`_smallest_size_at_least` (:257-268)."""
    if lh <= 0 or lw <= 0:
        return 0, 0
    h, w, s = F(lh), F(lw), F(side)
    scale = s / w if lh > lw else s / h
    return int(np.int32(h * scale)), int(np.int32(w * scale))


def image_aug_size(sh, sw, max_wd, side):
    lh, lw = limit_size(sh, sw, max_wd)
    return (lh, lw) + aug_size(lh, lw, side)


def _axis(out_idx, in_size, out_size):
    """lo, hi, t of the legacy bilinear rule for the output indices `out_idx` (any subset of range(out_size))."""
    scale = F(in_size) / F(out_size)
    src = out_idx.astype(F) * scale
    lo = np.floor(src)
    t = (src - lo).astype(F)
    lo = lo.astype(np.int64)
    hi = np.minimum(lo + 1, in_size - 1)
    return lo, hi, t


def resize_window(img, out_hw, ys, xs):
    """Rows `ys` and columns `xs` of resize_bilinear_legacy(f32(img [..., h, w, C]), out_hw), float32."""
    h, w = img.shape[-3], img.shape[-2]
    y0, y1, ty = _axis(np.asarray(ys), h, out_hw[0])
    x0, x1, tx = _axis(np.asarray(xs), w, out_hw[1])
    f = img.astype(F)
    r0, r1 = f[..., y0, :, :], f[..., y1, :, :]
    tl, tr, bl, br = r0[..., x0, :], r0[..., x1, :], r1[..., x0, :], r1[..., x1, :]
    tx = tx.reshape(1, -1, 1)
    ty = ty.reshape(-1, 1, 1)
    top = tl + (tr - tl) * tx
    bot = bl + (br - bl) * tx
    out = top + (bot - top) * ty
    assert out.dtype == F
    return out


def limit(frames, max_wd):
    """Step 1 on uint8 [T, sh, sw, 3] (or [sh, sw, 3]): the uint8 image L."""
    sh, sw = frames.shape[-3], frames.shape[-2]
    lh, lw = limit_size(sh, sw, max_wd)
    if sw <= max_wd:
        return frames
    return resize_window(frames, (lh, lw), np.arange(lh), np.arange(lw)).astype(np.uint8)   # truncation


def central_offsets(ah, aw, ch, cw):
    """`_central_crop` (:200-201, true division) through `to_int32` (:87)."""
    return int(np.int32(F((ah - ch) / 2))), int(np.int32(F((aw - cw) / 2)))


def preprocess(frames, max_wd, side, crop_yx, crop_hw, flip, mean=MEAN):
    """Steps 1-5 on uint8 [T, sh, sw, 3] -> (float32 [T, ch, cw, 3], (lh, lw, ah, aw)).  crop_yx None = central.
    Raises ValueError where the reference's size assertion / tf.slice would fail."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3
    L = limit(frames, max_wd)
    lh, lw = L.shape[1], L.shape[2]
    ah, aw = aug_size(lh, lw, side)
    ch, cw = crop_hw
    if ah < ch or aw < cw:
        raise ValueError('Crop size greater than the image size.')
    oy, ox = central_offsets(ah, aw, ch, cw) if crop_yx is None else crop_yx
    if oy < 0 or ox < 0 or oy + ch > ah or ox + cw > aw:
        raise ValueError('slice outside the resized image')
    xs = ox + np.arange(cw)
    if flip:
        xs = xs[::-1]
    out = resize_window(L, (ah, aw), oy + np.arange(ch), xs) - F(mean)
    return np.ascontiguousarray(out), (lh, lw, ah, aw)


def geom_row(im_ht, im_wd, sizes, crop_yx, crop_hw, flip):
    """The int32 [9] record both device ops consume."""
    return [int(im_ht), int(im_wd), int(sizes[2]), int(sizes[3]), int(crop_yx[0]), int(crop_yx[1]),
            int(crop_hw[0]), int(crop_hw[1]), int(bool(flip))]
