"""The augmentation pipeline on the device -- mirror of /root/reference/tf2/data_util.py.

* `batch_random_blur` -> `random_blur` -> `gaussian_blur`: what `Model.__call__` runs on the accelerator
  (tf2/model.py:255-258, tf2/data_util.py:323-440).
* `preprocess_for_train_batch` / `two_view_batch` / `preprocess_for_eval_batch`: the per-image part of the input
  pipeline (random-resized-crop with bicubic resize, flip, colour jitter in random order, random grayscale;
  tf2/data_util.py:53-320, :362-390, :443-499 and the two-views concat of tf2/data.py:52-62) for a whole batch of
  decoded images at once -- at >6 000 images/s per GPU a host tf.data-style pipeline is the limiter.
  Each has a `_ragged` form that reads a batch as packed variable-size records `(packed, table)` instead of a dense
  canvas: what the input pipeline (simclr_amd/data.py) feeds from the on-disk array format.  tfds / TFRecord readers and
  JPEG decode at training time stay outside (out of scope); tools/make_array_dataset.py converts once.

Random draws (crop boxes, coins, op order, factors; sigma and selectors of the blur) come from numpy / torch
generators: parity with the reference is distributional for the draws and exact (tested against the oracle,
oracle/augment.py and oracle/blur.py) for the arithmetic given the draws.
"""
import numpy as np
import torch

from . import ops

_gen = {}


def _generator(device):
    """One generator per device, seeded with the replica id: every replica draws its own sigma / selectors, like the
    per-replica random ops of the reference (tf2/data_util.py:405, :425-430).  A device generator: the draws never touch
    the host, so the hot path has no host-to-device copy or sync."""
    from .comm import replica_id
    from .resnet import RT
    key = str(device)
    g = _gen.get(key)
    if g is None:
        g = torch.Generator(device=device)
        g.manual_seed(0x51C1 + 7919 * replica_id(RT.strategy))
        _gen[key] = g
    return g


def gaussian_filter(kernel_size, sigma):
    """The 1-D filter of gaussian_blur (tf2/data_util.py:338-343): radius = int(kernel_size / 2),
    size 2*radius+1, exp(-x^2 / (2 sigma^2)) normalised to sum 1 (float32).  `sigma`: a float, or a tensor [k]
    (one filter per row, computed where the tensor lives)."""
    radius = int(kernel_size / 2)
    sig = torch.as_tensor(sigma, dtype=torch.float32)
    x = torch.arange(-radius, radius + 1, dtype=torch.float32, device=sig.device)
    f = torch.exp(-torch.pow(x, 2.0) / (2.0 * torch.pow(sig.reshape(-1, 1), 2.0)))
    f = f / f.sum(dim=1, keepdim=True)
    return f if sig.dim() else f[0]


_prob_columns = {}


def _per_view(p, k, dev, what):
    """A probability as the right-hand side of `rand(k, b) < .`: a scalar as it is (today's expression), a sequence of k numbers
    as a float32 [k, 1] column on the device (made once per (device, values): the hot path copies nothing from the host)."""
    if not isinstance(p, (list, tuple, np.ndarray)) and not torch.is_tensor(p):
        return p
    vals = tuple(float(v) for v in (p.tolist() if hasattr(p, 'tolist') else p))
    if len(vals) != k:
        raise ValueError('%s: %d probabilities for %d views' % (what, len(vals), k))
    key = (str(dev), vals)
    if key not in _prob_columns:
        _prob_columns[key] = torch.tensor(vals, dtype=torch.float32).reshape(k, 1).to(dev)
    return _prob_columns[key]


def _any_positive(p):
    if torch.is_tensor(p):
        p = p.tolist()
    return any(float(v) > 0 for v in (p if isinstance(p, (list, tuple, np.ndarray)) else (p,)))


def batch_random_blur_tensor(images, height, width, blur_probability=0.5, sigmas=None, selectors=None,
                             solarize_probability=0.0, solarize=None, threshold=0.5):
    """Fused form used by Model: images float32 [b,H,W,3k] -> blurred/clipped tensor of the same shape.
    sigmas [k] / selectors [k,b] may be given explicitly (tests); otherwise drawn like the reference:
    sigma ~ U(0.1, 2.0) once per view (:405), selector = uniform(0,1) < p per image (:425-430).
    blur_probability / solarize_probability: a scalar, or one number per view.  solarize [k,b] of 0/1: the solarization coins
    (drawn as uniform(0,1) < solarize_probability when that is > 0 for some view); an image whose coin is set has every element
    v >= threshold replaced by 1 - v AFTER the blur's clip (ops.batch_blur).  The device generator is consumed in the order sigmas,
    blur selectors, solarization coins, and the coins are drawn only when some solarize probability is positive: at the defaults
    it is consumed exactly as before the coins existed, and the launches are those of simclr_batch_blur."""
    b, H, W, C = images.shape
    k = C // 3
    dev = images.device
    if sigmas is None:
        sigmas = 0.1 + 1.9 * torch.rand(k, generator=_generator(dev), device=dev)
    else:
        sigmas = torch.as_tensor(sigmas, dtype=torch.float32).to(dev)
    if selectors is None:
        selectors = (torch.rand(k, b, generator=_generator(dev), device=dev) < _per_view(blur_probability, k, dev, 'blur_probability')).float()
    if solarize is None and _any_positive(solarize_probability):
        solarize = (torch.rand(k, b, generator=_generator(dev), device=dev)
                    < _per_view(solarize_probability, k, dev, 'solarize_probability')).float()
    filt = gaussian_filter(height // 10, sigmas)                                                  # :406-407
    sel = torch.as_tensor(selectors, dtype=torch.float32).to(dev).contiguous()
    if solarize is not None:
        solarize = torch.as_tensor(solarize, dtype=torch.float32).to(dev).contiguous()
    return ops.batch_blur(images.contiguous(), filt.contiguous(), sel, solarize, threshold)


_no_blur = {}


def apply_view_plan(images, plan, height=None, local=False, sigmas=None, selectors=None, solarize=None):
    """The device-side stages of the resolved augmentation plan (flags.aug_plan) on a block of views [b,H,W,3k]: random blur, then
    solarization, in one pass over the block.  `height` sizes the filter (default: the block's own).
    Global views (view a is channels 0:3): the plan's per-view blur and solarize probabilities.  local=True (the low-resolution
    views of multi-crop, blurred at their own size): probability 0.5 and no solarization, whatever the recipe.
    A plan that blurs and solarizes nothing returns `images` itself and launches nothing.  Probabilities that are equal across the
    views are passed as the scalar they are, so the `simclr` plan draws and launches exactly what a run without the recipe flags
    does.  No blur (--use_blur=False, or both probabilities 0) with solarization on: a 1-tap filter and zero selectors, no sigma
    and no selector is drawn -- copy, clip, solarize.
    sigmas / selectors / solarize: explicit draws (tests), as in batch_random_blur_tensor; local views take no coins."""
    b, H, W, C = images.shape
    k = C // 3
    height = H if height is None else height
    if local:
        if not plan.use_blur:
            return images
        return batch_random_blur_tensor(images, height, W, 0.5, sigmas=sigmas, selectors=selectors)
    blur_p, sol_p = _views_of(plan.blur_probs, k, '--blur_probs'), _views_of(plan.solarize_probs, k, '--solarize_probs')
    if not _any_positive(sol_p):
        if not _any_positive(blur_p):
            return images
        return batch_random_blur_tensor(images, height, W, blur_p, sigmas=sigmas, selectors=selectors)
    if not _any_positive(blur_p):
        dev = images.device
        key = (str(dev), k, b)
        if key not in _no_blur:
            _no_blur[key] = (torch.ones(k, 1, device=dev), torch.zeros(k, b, device=dev))
        filt, sel = _no_blur[key]
        if solarize is None:
            solarize = (torch.rand(k, b, generator=_generator(dev), device=dev) < _per_view(sol_p, k, dev, '--solarize_probs')).float()
        solarize = torch.as_tensor(solarize, dtype=torch.float32).to(dev).contiguous()
        return ops.batch_blur(images.contiguous(), filt, sel, solarize, plan.solarize_threshold)
    return batch_random_blur_tensor(images, height, W, blur_p, sigmas=sigmas, selectors=selectors, solarize_probability=sol_p,
                                    solarize=solarize, threshold=plan.solarize_threshold)


def _views_of(probs, k, flag):
    """The plan's (view a, view b) pair for a block of k views: the scalar when both are equal (any k), the pair for k = 2."""
    if len(set(probs)) == 1:
        return probs[0]
    if len(probs) != k:
        raise ValueError('%s=%s names %d views, the block has %d' % (flag, ','.join('%g' % p for p in probs), len(probs), k))
    return tuple(probs)


def batch_random_blur(images_list, height, width, blur_probability=0.5):
    """Apply efficient batch data transformations (tf2/data_util.py:413-440): list of [b,H,W,3]
    tensors in, list of blurred + clipped tensors out."""
    x = torch.cat(list(images_list), dim=3)
    y = batch_random_blur_tensor(x, height, width, blur_probability)
    return list(torch.split(y, 3, dim=3))


# --------------------------------------------------------------------------- crop / flip / colour jitter (input pipeline)
CROP_PROPORTION = 0.875            # tf2/data_util.py:22
JITTER_COMPONENTS = (0.8, 0.8, 0.8, 0.2)    # brightness, contrast, saturation, hue per unit of strength, tf2/data_util.py:70-73
PARAM_FIELDS = ('crop_y', 'crop_x', 'crop_h', 'crop_w', 'flip', 'jitter_on', 'perm0', 'perm1', 'perm2', 'perm3',
                'brightness', 'contrast', 'saturation', 'hue', 'gray_on', 'pad')
_np_rng = {}


def _rng():
    """numpy generator of this replica (seeded with the replica id, like the per-replica tf.data pipelines)."""
    from .comm import replica_id
    from .resnet import RT
    r = replica_id(RT.strategy)
    if r not in _np_rng:
        _np_rng[r] = np.random.default_rng(0xA06 + 104729 * r)
    return _np_rng[r]


def _lrint(x):
    return np.rint(x).astype(np.int64)


def sample_crop_boxes(rng, heights, widths, out_h, out_w, max_attempts=100, area_range=(0.08, 1.0), min_object_covered=0.1):
    """tf.image.sample_distorted_bounding_box as crop_and_resize calls it (tf2/data_util.py:298-320: whole-image box,
    min_object_covered 0.1, aspect ratio in [3/4, 4/3] * out_w/out_h, area in [0.08, 1], 100 attempts, then the whole
    image), vectorised over the images; the per-attempt arithmetic follows TensorFlow's GenerateRandomCrop
    (float32 areas, lrintf roundings).  heights / widths: int arrays [m].  Returns int64 [m, 4] = (y, x, h, w).
    area_range / min_object_covered: the sampler's two other arguments (the defaults are the reference's call).  The cover test
    rejects every box below min_object_covered of the image, so an area range that starts lower is silently truncated unless the
    cover is lowered with it: the local crops of SwAV's multi-crop pass their minimum scale as the cover."""
    Hh = np.asarray(heights, dtype=np.int64)
    Ww = np.asarray(widths, dtype=np.int64)
    m = Hh.shape[0]
    f32 = np.float32
    ar0 = out_w / out_h
    lo, hi = f32(3. / 4 * ar0), f32(4. / 3. * ar0)
    box = np.stack([np.zeros(m, np.int64), np.zeros(m, np.int64), Hh, Ww], 1)
    todo = np.ones(m, bool)
    min_area = f32(area_range[0]) * Ww.astype(f32) * Hh.astype(f32)
    max_area = f32(area_range[1]) * Ww.astype(f32) * Hh.astype(f32)
    for _ in range(max_attempts):
        if not todo.any():
            break
        ar = (rng.random(m).astype(f32) * (hi - lo) + lo).astype(np.float64)
        h = _lrint(np.sqrt(min_area / ar.astype(f32)))
        max_h = _lrint(np.sqrt(max_area / ar.astype(f32)))
        over = _lrint(max_h * ar) > Ww
        alt = ((Ww + 0.5 - 0.0000001) / ar).astype(np.int64)
        alt = np.where(_lrint(alt * ar) > Ww, alt - 1, alt)
        max_h = np.where(over, alt, max_h)
        max_h = np.minimum(max_h, Hh)
        h = np.minimum(h, max_h)
        h = h + np.floor(rng.random(m) * (max_h - h + 1)).astype(np.int64) * (h < max_h)
        w = _lrint(h * ar)
        area = (w * h).astype(np.float64)
        small = area < min_area
        h = np.where(small, h + 1, h); w = np.where(small, _lrint(h * ar), w); area = (w * h).astype(np.float64)
        big = area > max_area
        h = np.where(big, h - 1, h); w = np.where(big, _lrint(h * ar), w); area = (w * h).astype(np.float64)
        ok = ~((area < min_area) | (area > max_area) | (w > Ww) | (h > Hh) | (w <= 0) | (h <= 0))
        y = np.floor(rng.random(m) * np.maximum(Hh - h, 1)).astype(np.int64) * (h < Hh)
        x = np.floor(rng.random(m) * np.maximum(Ww - w, 1)).astype(np.int64) * (w < Ww)
        ok &= (w * h) / (Ww * Hh).astype(np.float64) >= min_object_covered    # of the whole-image box
        take = todo & ok
        box[take] = np.stack([y, x, h, w], 1)[take]
        todo &= ~ok
    return box


def draw_train_params(b, heights, widths, height, width, color_jitter_strength=1.0, crop=True, flip=True, views=2,
                      rng=None, area_range=(0.08, 1.0), min_object_covered=0.1, jitter_components=None):
    """Random draws of preprocess_for_train (tf2/data_util.py:443-475) for `views` views of each of `b` images.
    heights / widths: per-image source sizes (int or arrays).  Returns float32 [b, views, 16] laid out as PARAM_FIELDS.
    area_range / min_object_covered: sample_crop_boxes's; draw_local_params sets them for SwAV's local views.
    jitter_components: four non-negative numbers (brightness, contrast, saturation, hue); the range of each factor is its
    component times color_jitter_strength.  None: the reference's (0.8, 0.8, 0.8, 0.2)."""
    cb, cc_, cs, ch = JITTER_COMPONENTS if jitter_components is None else (float(v) for v in jitter_components)
    rng = _rng() if rng is None else rng
    m = b * views
    Hh = np.repeat(np.broadcast_to(np.asarray(heights, np.int64), (b,)), views)
    Ww = np.repeat(np.broadcast_to(np.asarray(widths, np.int64), (b,)), views)
    p = np.zeros((m, len(PARAM_FIELDS)), np.float32)
    p[:, 0:4] = (sample_crop_boxes(rng, Hh, Ww, height, width, area_range=area_range, min_object_covered=min_object_covered)
                 if crop else np.stack([0 * Hh, 0 * Ww, Hh, Ww], 1))
    if flip:
        p[:, 4] = rng.random(m) < 0.5                                              # :463
    s = float(color_jitter_strength)
    if s > 0:                                                                      # :380-389
        p[:, 5] = rng.random(m) < 0.8
        p[:, 6:10] = np.argsort(rng.random((m, 4)), axis=1)                        # a uniform random order, :168
        bb, cc, ss, hh = cb * s, cc_ * s, cs * s, ch * s                           # :70-73 (0.8 s, 0.8 s, 0.8 s, 0.2 s)
        p[:, 10] = rng.uniform(max(1.0 - bb, 0.0), 1.0 + bb, m)                    # :37-39
        p[:, 11] = rng.uniform(1 - cc, 1 + cc, m)
        p[:, 12] = rng.uniform(1 - ss, 1 + ss, m)
        p[:, 13] = rng.uniform(-hh, hh, m)
        p[:, 14] = rng.random(m) < 0.2
    return p.reshape(b, views, len(PARAM_FIELDS))


def draw_local_params(b, heights, widths, size, views, min_scale, max_scale, color_jitter_strength=1.0, rng=None,
                      jitter_components=None):
    """draw_train_params for the `views` LOCAL views of SwAV's multi-crop (Caron et al. 2020, section 4): square crops of `size`
    pixels whose area is a [min_scale, max_scale] share of the image, the same flip and colour jitter as the global views.  The
    cover is the minimum scale: left at the sampler's 0.1, a [0.05, 0.14] range would silently become [0.1, 0.14].
    Returns float32 [b, views, 16]."""
    return draw_train_params(b, heights, widths, size, size, color_jitter_strength, views=views, rng=rng,
                             area_range=(float(min_scale), float(max_scale)), min_object_covered=float(min_scale),
                             jitter_components=jitter_components)


def _sizes(images, sizes):
    b, Hs, Ws, _ = images.shape
    if sizes is None:
        return np.full(b, Hs), np.full(b, Ws)
    sz = np.asarray(sizes.cpu() if torch.is_tensor(sizes) else sizes)
    return sz[:, 0], sz[:, 1]


def preprocess_for_train_batch(images, height, width, color_jitter_strength=0., crop=True, flip=True, impl='simclrv2',
                               sizes=None, views=1, params=None):
    """Batched preprocess_for_train (tf2/data_util.py:443-475).  images: device tensor [b, Hs, Ws, 3], uint8 or float32
    in [0,1] -- a canvas; `sizes` [b, 2] gives each image's valid (height, width) inside it (default: the whole canvas).
    Returns float32 [b, height, width, 3*views].  views=1 with color_jitter_strength=0 is train_mode=finetune's
    preprocessing (tf2/data.py:52-58: one view, crop + flip, no colour distortion)."""
    if impl != 'simclrv2':
        raise ValueError('Unknown impl {} for random brightness.'.format(impl))      # the build ships simclrv2 only
    b = images.shape[0]
    if params is None:
        hs, ws = _sizes(images, sizes)
        params = draw_train_params(b, hs, ws, height, width, color_jitter_strength, crop, flip, views)
    if not torch.is_tensor(params):
        params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32))
    params = params.to(images.device, non_blocking=True)
    return ops.augment_views(images.contiguous(), params.contiguous(), height, width)


def two_view_batch(images, height, width, color_jitter_strength=1.0, sizes=None, params=None):
    """tf2/data.py:52-62: `xs = [preprocess(image), preprocess(image)]; concat(xs, -1)` for the whole batch ->
    [b, height, width, 6], the tensor Model.__call__ consumes."""
    return preprocess_for_train_batch(images, height, width, color_jitter_strength, sizes=sizes, views=2, params=params)


def center_crop_boxes(heights, widths, height, width, crop_proportion=CROP_PROPORTION):
    """tf2/data_util.py:175-243 (_compute_crop_shape + center_crop offsets) for arrays of image sizes."""
    f32 = np.float32
    ih, iw = np.asarray(heights).astype(f32), np.asarray(widths).astype(f32)
    ar = width / height
    wider = ar > iw / ih
    ch = np.where(wider, np.rint(f32(crop_proportion / ar) * iw), np.rint(f32(crop_proportion) * ih)).astype(np.int64)
    cw = np.where(wider, np.rint(f32(crop_proportion) * iw), np.rint(f32(crop_proportion * ar) * ih)).astype(np.int64)
    Hh, Ww = np.asarray(heights, np.int64), np.asarray(widths, np.int64)
    return np.stack([((Hh - ch) + 1) // 2, ((Ww - cw) + 1) // 2, ch, cw], 1)


def preprocess_for_eval_batch(images, height, width, crop=True, sizes=None):
    """Batched preprocess_for_eval (tf2/data_util.py:478-499): central crop (CROP_PROPORTION) + bicubic resize + clip."""
    b = images.shape[0]
    hs, ws = _sizes(images, sizes)
    p = np.zeros((b, 1, len(PARAM_FIELDS)), np.float32)
    p[:, 0, 0:4] = center_crop_boxes(hs, ws, height, width) if crop else np.stack([0 * hs, 0 * ws, hs, ws], 1)
    return preprocess_for_train_batch(images, height, width, params=p)


# --------------------------------------------------------------------------- the same, from packed variable-size records
def preprocess_for_train_batch_ragged(packed, table, height, width, color_jitter_strength=0., crop=True, flip=True,
                                      impl='simclrv2', views=1, params=None, table_dev=None):
    """preprocess_for_train_batch for a batch held as packed records.  packed: device uint8 [nbytes], the images HWC,
    tightly packed, back to back; table: HOST int64 [b, 3] = (byte offset, height, width) per image (checked before the
    launch, ops.augment_views_ragged).  No canvas, no padding: the bytes are what the on-disk format holds.
    Returns float32 [b, height, width, 3*views], bitwise the canvas function's result for the same images and draws."""
    if impl != 'simclrv2':
        raise ValueError('Unknown impl {} for random brightness.'.format(impl))
    table = np.asarray(table)
    b = table.shape[0]
    if params is None:
        params = draw_train_params(b, table[:, 1], table[:, 2], height, width, color_jitter_strength, crop, flip, views)
    if not torch.is_tensor(params):
        params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32))
    params = params.to(packed.device, non_blocking=True)
    return ops.augment_views_ragged(packed, table, params.contiguous(), height, width, table_dev=table_dev)


def two_view_batch_ragged(packed, table, height, width, color_jitter_strength=1.0, params=None, table_dev=None):
    """two_view_batch (tf2/data.py:52-62) from packed records -> [b, height, width, 6]."""
    return preprocess_for_train_batch_ragged(packed, table, height, width, color_jitter_strength, views=2, params=params,
                                             table_dev=table_dev)


def eval_params(heights, widths, height, width, crop=True):
    """The parameter table [b, 1, 16] of preprocess_for_eval: the central crop box (or the whole image), nothing else."""
    hs, ws = np.asarray(heights, np.int64), np.asarray(widths, np.int64)
    p = np.zeros((hs.shape[0], 1, len(PARAM_FIELDS)), np.float32)
    p[:, 0, 0:4] = center_crop_boxes(hs, ws, height, width) if crop else np.stack([0 * hs, 0 * ws, hs, ws], 1)
    return p


def preprocess_for_eval_batch_ragged(packed, table, height, width, crop=True, table_dev=None):
    """preprocess_for_eval_batch (tf2/data_util.py:478-499) from packed records -> [b, height, width, 3]."""
    table = np.asarray(table)
    p = eval_params(table[:, 1], table[:, 2], height, width, crop)
    return preprocess_for_train_batch_ragged(packed, table, height, width, params=p, table_dev=table_dev)
