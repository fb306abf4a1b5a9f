"""Image rescaling around the model (csrc/resize.hip): bilinear resize + uint8 conversion + flip + pad as one launch, the merge of the
test-time-augmentation passes as one launch, the letterbox of a ragged list of images as one launch per 32 images and the way back of the
boxes to each image's own pixel grid as one launch.  No gradient flows through any of them."""
import ctypes

import numpy as np
import torch

from .._lib import LetterboxImage
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


def letterbox_geometry(shape, new_shape=(640, 640), auto=False, scale_fill=False, scaleup=True, center=True, stride=32):
    """the host arithmetic of LetterBox.__call__ (reference data/augment.py:1562-1590), statement for statement - Python's round is part of
    the contract.  shape: (h, w) of the image -> ((hs, ws), (top, bottom, left, right), ratio) with ratio = (r_h, r_w)."""
    shape = (int(shape[0]), int(shape[1]))
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    # Scale ratio (new / old)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:  # only scale down, do not scale up
        r = min(r, 1.0)
    ratio = r, r  # width, height ratios
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]  # wh padding
    if auto:  # minimum rectangle
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)  # wh padding
    elif scale_fill:  # stretch
        dw, dh = 0.0, 0.0
        new_unpad = (new_shape[1], new_shape[0])
        ratio = new_shape[1] / shape[1], new_shape[0] / shape[0]  # width, height ratios
    if center:
        dw /= 2  # divide padding into 2 sides
        dh /= 2
    top, bottom = int(round(dh - 0.1)) if center else 0, int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)) if center else 0, int(round(dw + 0.1))
    return (new_unpad[1], new_unpad[0]), (top, bottom, left, right), (float(ratio[1]), float(ratio[0]))


def _as_u8_image(im):
    """-> (torch uint8 [h, w, 3] contiguous, on_device)"""
    if isinstance(im, np.ndarray):
        im = torch.from_numpy(np.ascontiguousarray(im))
    if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.shape[0] == 0 or im.shape[1] == 0:
        raise ValueError(f"letterbox takes (h, w, 3) uint8 images, got {type(im).__name__} {tuple(getattr(im, 'shape', ()))} {getattr(im, 'dtype', None)}")
    return im.detach().contiguous(), im.is_cuda


def letterbox(images, new_shape=(640, 640), auto=False, scale_fill=False, scaleup=True, center=True, stride=32, bgr=True, pad_value=114, normalize=True,
              device=None):
    """LetterBox (reference data/augment.py:1479-1603) of every image and the conversion of engine/predictor.py:151-162 (BGR -> RGB, HWC -> CHW,
    float / 255), csrc/resize.hip: one launch per 32 images writes the whole float32 batch.
    images: a list of (h, w, 3) uint8 numpy arrays or torch tensors of any sizes, on the host or the device.  Host images are packed into ONE
    staging buffer and uploaded with ONE copy.  With `auto` all images must share a shape, as in the reference (any list whose letterboxed
    sizes differ is refused).  normalize=False keeps 0..255 values; bgr=False keeps the channel order.
    -> (img [n, 3, H, W] float32 on the device, ratio_pad) with ratio_pad[i] = ((r_h, r_w), (left, top))."""
    if torch.is_tensor(images) or isinstance(images, np.ndarray):
        images = [images] if images.ndim == 3 else list(images)
    if not len(images):
        raise ValueError("letterbox: no images")
    ims = [_as_u8_image(im) for im in images]
    if device is None:
        device = next((im.device for im, on in ims if on), torch.device("cuda", torch.cuda.current_device()))
    geo = [letterbox_geometry(im.shape[:2], new_shape, auto, scale_fill, scaleup, center, stride) for im, _ in ims]
    sizes = {(t + hs + b, l + ws + r) for (hs, ws), (t, b, l, r), _ in geo}
    if len(sizes) != 1:
        raise ValueError(f"letterbox: the images letterbox to different sizes {sorted(sizes)}; auto needs images of one shape")
    (H, W), = sizes
    host = [i for i, (_, on) in enumerate(ims) if not on]
    staged = {}
    if host:  # one staging buffer, one copy
        offs = np.cumsum([0] + [(ims[i][0].numel() + 15) // 16 * 16 for i in host])
        stage = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
        for i, o in zip(host, offs):
            stage[int(o) : int(o) + ims[i][0].numel()] = ims[i][0].reshape(-1)
        dev_stage = stage.to(device, non_blocking=True)
        staged = {i: dev_stage.data_ptr() + int(o) for i, o in zip(host, offs)}
    n = len(ims)
    table = (LetterboxImage * n)()
    for i, ((im, on), ((hs, ws), (t, _, l, _), _)) in enumerate(zip(ims, geo)):
        table[i] = LetterboxImage(staged[i] if not on else im.data_ptr(), int(im.shape[0]), int(im.shape[1]), hs, ws, t, l)
    out = torch.empty((n, 3, H, W), dtype=torch.float32, device=device)
    check(L().ymi_letterbox_batch(table, n, ptr(out), H, W, int(pad_value), int(bool(normalize)), int(bool(bgr)), stream_ptr()), "letterbox_batch")
    return out, [(g[2], (g[1][2], g[1][0])) for g in geo]


def scale_boxes_params(img_shape, ori_shape, ratio_pad=None):
    """(gain, pad_x, pad_y, w0, h0) of one image: the head of scale_boxes (reference utils/ops.py:110-118), statement for statement."""
    img1_shape, img0_shape = img_shape, ori_shape
    if ratio_pad is None:  # calculate from img0_shape
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])  # gain  = old / new
        pad = (
            round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1),
            round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1),
        )  # wh padding
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    return [float(gain), float(pad[0]), float(pad[1]), float(img0_shape[1]), float(img0_shape[0])]


def _scale_boxes_launch(det, count, params, padding, xywh, out):
    """det / out: [B, rows, cols] views with unit column stride and dense rows-of-rows (stride(0) == rows * stride(1))"""
    b, rows, cols = (int(v) for v in det.shape)
    check(L().ymi_scale_boxes(ptr(det), int(det.stride(1)) if rows > 1 else cols, ptr(count), ptr(params), b, rows, cols, int(bool(padding)), int(bool(xywh)),
                              ptr(out), int(out.stride(1)) if rows > 1 else cols, stream_ptr()), "scale_boxes")
    return out


def scale_boxes(det, count, img_shape, ori_shapes, ratio_pads=None, padding=True, xywh=False, inplace=False):
    """scale_boxes + clip_boxes (reference utils/ops.py:93-127, :335-354) on what ops.detect_nms leaves, one launch for the batch, on the device.
    det [B, max_det, 6] float32, count [B] int32; img_shape: (h, w) of the network input; ori_shapes: (h0, w0) per image (or one for all);
    ratio_pads: per image ((r_h, r_w), (pad_x, pad_y)) or None = derived from the shapes as the reference does.
    -> det in each image's own pixels, clipped; rows at or beyond count stay zero.  inplace=True edits det and returns it."""
    if not det.is_cuda:
        raise RuntimeError("libyolo_mi355 kernels need tensors on the MI355X (cuda) device; there is no CPU path")
    if det.dim() != 3 or det.shape[2] < 4 or det.dtype != torch.float32 or not det.is_contiguous():
        raise ValueError(f"scale_boxes takes a contiguous float32 [B, max_det, 4+] tensor, got {tuple(det.shape)} {det.dtype}")
    b = int(det.shape[0])
    if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (b,) or not count.is_cuda):
        raise ValueError("scale_boxes: count is an int32 [B] tensor on the device")
    if isinstance(ori_shapes[0], (int, float)):
        ori_shapes = [ori_shapes] * b
    if ratio_pads is None or (len(ratio_pads) == 2 and ratio_pads[0] is not None and isinstance(ratio_pads[0][0], (int, float))):  # one for all
        ratio_pads = [ratio_pads] * b
    if len(ori_shapes) != b or len(ratio_pads) != b:
        raise ValueError("scale_boxes: one original shape (and one ratio_pad) per image")
    det = det.detach()
    params = torch.tensor([scale_boxes_params(img_shape, o, rp) for o, rp in zip(ori_shapes, ratio_pads)], dtype=torch.float32).reshape(b, 5).to(det.device)
    return _scale_boxes_launch(det, count, params, padding, xywh, det if inplace else torch.empty_like(det))


def scale_rows(boxes, params5, padding=True, xywh=False):
    """the same kernel, in place, on one [n, 4+] float32 device tensor or view (unit column stride): utils.ops.scale_boxes / clip_boxes."""
    if boxes.dim() != 2 or boxes.shape[1] < 4 or boxes.dtype != torch.float32 or (boxes.shape[1] > 1 and boxes.stride(1) != 1):
        raise ValueError(f"scale_boxes / clip_boxes take a float32 [n, 4+] tensor with unit column stride, got {tuple(boxes.shape)} {boxes.dtype} strides {boxes.stride()}")
    if boxes.shape[0]:
        params = torch.tensor(params5, dtype=torch.float32).reshape(1, 5).to(boxes.device)
        v = boxes.detach().unsqueeze(0)
        _scale_boxes_launch(v, None, params, padding, xywh, v)
    return boxes
