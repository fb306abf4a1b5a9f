"""Pure-torch restatement of what the reference does around the model when it rescales images: scale_img (utils/torch_utils.py:475-495),
the multi-scale size rule of DetectionTrainer.preprocess_batch (models/yolo/detect/train.py:100-114), _descale_pred / _clip_augmented
(nn/tasks.py:399-439) and ATen's bilinear formula (align_corners=False) written out one float32 operation at a time.

tests/test_tta_ref_cpu.py holds every function here to the fixtures the REAL reference produced (tests/golden/make_tta_golden.py); the GPU
tests then compare the kernels with these functions on inputs of their own, on a machine that has no reference."""
import math

import numpy as np
import torch

PAD_VALUE = 0.447  # scale_img's padding: the ImageNet mean
TTA_SCALES = (1, 0.83, 0.67)
TTA_FLIPS = (None, 3, None)


def bilinear_taps(out_size, in_size):
    """-> (i0, i1 int64 [out], l0, l1 float32 [out]): scale = in / out; s = max((dst + 0.5) * scale - 0.5, 0); i0 = floor(s);
    i1 = min(i0 + 1, in - 1); l1 = s - i0; l0 = 1 - l1 - every step rounded to float32."""
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size), dtype=torch.float32)
    dst = torch.arange(out_size, dtype=torch.float32)
    s = ((dst + 0.5) * scale - 0.5).clamp(min=0)
    i0 = s.floor().to(torch.int64).clamp(max=in_size - 1)
    i1 = (i0 + 1).clamp(max=in_size - 1)
    l1 = s - i0.to(torch.float32)
    l0 = 1.0 - l1
    return i0, i1, l0, l1


def bilinear_resize(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) for float32 NCHW x, as the explicit formula
    l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d)."""
    assert x.dtype == torch.float32 and x.dim() == 4
    y0, y1, ly0, ly1 = (t.to(x.device) for t in bilinear_taps(size[0], x.shape[2]))
    x0, x1, lx0, lx1 = (t.to(x.device) for t in bilinear_taps(size[1], x.shape[3]))
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    bot = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    return ly0[:, None] * top + ly1[:, None] * bot


def to_unit(img):
    """uint8 -> float / 255 as the reference converts (train.py:100); float32 passes through"""
    return img.float() / 255 if img.dtype == torch.uint8 else img


def scale_image(img, size, padded_size=None, pad_value=0.0, flip=None, normalize=None):
    """what ops.scale_image computes: convert, flip, resize (identity size: untouched), pad right and below."""
    if normalize is None:
        normalize = img.dtype == torch.uint8
    x = to_unit(img) if normalize else img.float()
    for f in (() if flip is None else ((flip,) if isinstance(flip, int) else tuple(flip))):
        x = x.flip(f)
    size = (size, size) if isinstance(size, int) else tuple(size)
    if tuple(x.shape[2:]) != size:
        x = bilinear_resize(x, size)
    hp, wp = size if padded_size is None else padded_size
    out = torch.full((x.shape[0], x.shape[1], hp, wp), pad_value, dtype=torch.float32, device=x.device)
    out[:, :, : size[0], : size[1]] = x
    return out


def scale_img_sizes(h, w, ratio, same_shape=False, gs=32):
    """-> ((hs, ws), (hp, wp)) of scale_img"""
    s = (int(h * ratio), int(w * ratio))
    if not same_shape:
        h, w = (math.ceil(x * ratio / gs) * gs for x in (h, w))
    return s, (h, w)


def scale_img(img, ratio=1.0, same_shape=False, gs=32):
    if ratio == 1.0:
        return img
    s, p = scale_img_sizes(img.shape[2], img.shape[3], ratio, same_shape, gs)
    return scale_image(img, s, p, PAD_VALUE)


def multi_scale_size(h, w, imgsz, stride, rng):
    """the size preprocess_batch stretches an h x w batch to (train.py:101-112); (h, w) itself when sf == 1.  Draws once from rng."""
    sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5 + stride)) // stride * stride
    sf = sz / max(h, w)
    if sf != 1:
        return tuple(math.ceil(x * sf / stride) * stride for x in (h, w))
    return (h, w)


def preprocess_img(img, imgsz, stride, multi_scale, rng):
    x = to_unit(img)
    if multi_scale:
        ns = multi_scale_size(x.shape[2], x.shape[3], imgsz, stride, rng)
        if ns != tuple(x.shape[2:]):
            x = bilinear_resize(x, ns)
    return x


def descale_pred(p, flips, scale, img_size):
    """_descale_pred without the in-place edit of p: [B, 4 + nc, A] -> new tensor"""
    p = p.clone()
    p[:, :4] /= scale
    if flips == 2:
        p[:, 1] = img_size[0] - p[:, 1]
    elif flips == 3:
        p[:, 0] = img_size[1] - p[:, 0]
    return p


def clip_ranges(anchors, nl=3):
    """[(lo, hi)] per prediction: _clip_augmented's slices ([..., :-i] of the first, [..., i:] of the last) as index ranges"""
    g = sum(4 ** x for x in range(nl))
    idx = [range(int(a)) for a in anchors]
    i = (len(idx[0]) // g) * sum(4 ** x for x in range(1))
    idx[0] = idx[0][:-i]
    i = (len(idx[-1]) // g) * sum(4 ** (nl - 1 - x) for x in range(1))
    idx[-1] = idx[-1][i:]
    return [(r.start, r.stop) for r in idx]


def clip_augmented(y, nl=3):
    r = clip_ranges([t.shape[-1] for t in y], nl)
    return [t[..., lo:hi] for t, (lo, hi) in zip(y, r)]


def tta_merge(preds, scales, flips, img_size, nl=3):
    """torch.cat(_clip_augmented([_descale_pred(...)]), -1)"""
    return torch.cat(clip_augmented([descale_pred(p, f, s, img_size) for p, s, f in zip(preds, scales, flips)], nl), -1)


def seeded_model_state(state_dict, seed):
    """reproducible non-trivial weights for a detection model of either side: golden_weights.seeded_state over the floating-point entries in
    SORTED key order (so the result does not depend on a side's registration order), DFL's fixed kernel and the counters left alone,
    running variances made positive."""
    from golden_weights import seeded_state

    keys = sorted(k for k, v in state_dict.items() if v.dtype.is_floating_point and v.dim() > 0 and ".dfl." not in k)
    new = seeded_state({k: tuple(state_dict[k].shape) for k in keys}, seed)
    for k in new:
        if k.endswith("running_var"):
            new[k] = new[k].abs() + 0.5
    return new


def seeded_u8(seed, shape):
    """a uint8 image batch from numpy's frozen legacy stream"""
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=tuple(shape)).astype(np.uint8))
