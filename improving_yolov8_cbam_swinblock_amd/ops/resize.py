"""Image rescaling around the model (csrc/resize.hip): bilinear resize + uint8 conversion + flip + pad as one launch, and the merge of the
test-time-augmentation passes as one launch.  No gradient flows through either."""
import ctypes

import torch

from .base import L, check, ptr, stream_ptr


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def scale_image(img, size, padded_size=None, pad_value=0.0, flip=None, normalize=None):
    """F.pad(F.interpolate(x, size, mode="bilinear", align_corners=False), [0, Wp - ws, 0, Hp - hs], pad_value) with
    x = img.flip(flip) (flip: None, 2 = up-down, 3 = left-right, or a tuple of both) of img.float() / 255 for uint8 images
    (normalize=None: divide exactly when the image is uint8; False keeps 0..255 values; float32 images are taken as they are).
    img: [B, C, H, W] uint8 or float32 on the device; size: (hs, ws) or an int; padded_size: (Hp, Wp), default `size`.
    -> a new float32 NCHW-contiguous [B, C, Hp, Wp] tensor.  size == (H, W) copies the converted source exactly."""
    if not torch.is_tensor(img) or not img.is_cuda:
        raise RuntimeError("libyolo_mi355 kernels need tensors on the MI355X (cuda) device; there is no CPU path")
    if img.dim() != 4 or img.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"scale_image takes a [B, C, H, W] uint8 or float32 image batch, got {tuple(img.shape)} {img.dtype}")
    hs, ws = _pair(size)
    hp, wp = _pair(padded_size) if padded_size is not None else (hs, ws)
    if hs <= 0 or ws <= 0 or hs > hp or ws > wp:
        raise ValueError(f"scale_image: size {(hs, ws)} must be positive and lie within the padded size {(hp, wp)}")
    flips = () if flip is None else ((int(flip),) if isinstance(flip, int) else tuple(int(f) for f in flip))
    if any(f not in (2, 3) for f in flips):
        raise ValueError(f"scale_image: flip is None, 2 (up-down), 3 (left-right) or both, got {flip!r}")
    is_u8 = img.dtype == torch.uint8
    if normalize is None:
        normalize = is_u8
    if normalize and not is_u8:
        raise ValueError("scale_image: normalize=True divides uint8 images by 255; a float32 image is taken as it is")
    img = img.detach()
    if not img.is_contiguous():
        img = img.contiguous()
    b, c, h, w = (int(v) for v in img.shape)
    out = torch.empty((b, c, hp, wp), dtype=torch.float32, device=img.device)
    if out.numel() == 0:
        return out
    check(L().ymi_scale_image(ptr(img), int(is_u8), b * c, h, w, ptr(out), hp, wp, hs, ws, float(pad_value), int(bool(normalize)), int(3 in flips),
                              int(2 in flips), stream_ptr()), "scale_image")
    return out


def tta_clip_ranges(anchors, nl=3):
    """the anchor sub-range [lo, hi) each augmented pass keeps: _clip_augmented of reference nn/tasks.py:422-439 (the first pass loses its
    last A // g anchors - the coarsest level's share -, the last pass its first (A // g) * 4^(nl-1) - the finest level's -, g = sum 4^k),
    with the reference's slice semantics (`[..., :-0]` is empty)."""
    g = sum(4 ** x for x in range(nl))
    out = [range(int(a)) for a in anchors]
    out[0] = out[0][: -(len(out[0]) // g)]
    out[-1] = out[-1][(len(out[-1]) // g) * 4 ** (nl - 1) :]  # (one prediction: the second cut counts what the first left, as the reference does)
    return [(r.start, r.stop) for r in out]


def tta_merge(preds, scales, flips, img_size, ranges=None):
    """torch.cat([_descale_pred(p, flip, scale, img_size)[..., lo:hi] for every pass], -1) of reference nn/tasks.py:394-439 as one launch.
    preds: up to three decoded Detect outputs [B, 4 + nc, A_i] float32; scales / flips (None or 0, 2, 3) per pass; img_size: (H, W) of the
    original image, or one per pass; ranges: [(lo, hi)] per pass, default everything.  -> [B, 4 + nc, sum(hi - lo)] float32."""
    n = len(preds)
    if not 1 <= n <= 3 or len(scales) != n or len(flips) != n:
        raise ValueError("tta_merge takes one to three predictions with a scale and a flip code each")
    for p in preds:
        if not p.is_cuda:
            raise RuntimeError("libyolo_mi355 kernels need tensors on the MI355X (cuda) device; there is no CPU path")
        if p.dim() != 3 or p.dtype != torch.float32 or p.shape[:2] != preds[0].shape[:2] or p.shape[1] < 4:
            raise ValueError(f"tta_merge takes decoded Detect outputs [B, 4 + nc, A] in float32 of one batch and class count, got {tuple(p.shape)} {p.dtype}")
    preds = [p.detach() if p.is_contiguous() else p.detach().contiguous() for p in preds]
    sizes = [tuple(img_size)] * n if not isinstance(img_size[0], (tuple, list, torch.Size)) else [tuple(s) for s in img_size]
    ranges = [(0, int(p.shape[2])) for p in preds] if ranges is None else [(int(lo), int(hi)) for lo, hi in ranges]
    for (lo, hi), p in zip(ranges, preds):
        if not 0 <= lo <= hi <= p.shape[2]:
            raise ValueError(f"tta_merge: anchor range [{lo}, {hi}) outside [0, {p.shape[2]}]")
    b, rows = int(preds[0].shape[0]), int(preds[0].shape[1])
    out = torch.empty((b, rows, sum(hi - lo for lo, hi in ranges)), dtype=torch.float32, device=preds[0].device)
    if out.numel() == 0:
        return out
    i64 = ctypes.c_int64 * n
    check(L().ymi_tta_merge(n, (ctypes.c_void_p * n)(*[p.data_ptr() for p in preds]), i64(*[int(p.shape[2]) for p in preds]), i64(*[r[0] for r in ranges]),
                            i64(*[r[1] for r in ranges]), (ctypes.c_float * n)(*[float(s) for s in scales]), (ctypes.c_int32 * n)(*[int(f or 0) for f in flips]),
                            i64(*[int(s[0]) for s in sizes]), i64(*[int(s[1]) for s in sizes]), b, rows, ptr(out), stream_ptr()), "tta_merge")
    return out
