"""Pure-torch restatement, in the operation order include/ymi.h gives for ymi_letterbox_batch and ymi_scale_boxes, of the reference's
inference path around the model: LetterBox (data/augment.py:1479-1603), BasePredictor.preprocess (engine/predictor.py:144-162), scale_boxes and
clip_boxes (utils/ops.py:93-127, :335-354), the validator's _prepare_batch / _prepare_pred (models/yolo/detect/val.py:135-172) and the Boxes
properties (engine/results.py:1113-1256).

tests/test_letterbox_ref_cpu.py holds every function here to the fixtures the REAL reference produced (tests/golden/make_predict_golden.py); the
GPU tests then compare the kernels with these functions bit for bit, on a machine that has no reference.

`fault=` plants one mistake (the CPU test asserts that the fixtures notice each): "no_tenth" centre offset without the - 0.1, "floor" floor for
round in the interpolated size, "rgb" channel order kept, "no_clip" boxes not clipped, "reciprocal" a product with 1 / gain for the division,
"pad0" border 0 for 114."""
import math

import numpy as np
import torch

import tta_ref as TR

PAD_LEVEL = 114

# name: images [(seed, h, w)], target and LetterBox's switches.  The first eight are the sizes of the issue's table.
CASES = {
    "s37x53": dict(images=[(501, 37, 53)], new_shape=64),
    "s75x101": dict(images=[(502, 75, 101)], new_shape=96),
    "s90x60": dict(images=[(503, 90, 60)], new_shape=64),
    "s33x100": dict(images=[(504, 33, 100)], new_shape=96),
    "s120x67": dict(images=[(505, 120, 67)], new_shape=64),
    "s200x150": dict(images=[(506, 200, 150)], new_shape=64),
    "s48x64_identity": dict(images=[(507, 48, 64)], new_shape=64),      # identity size, pad only
    "s64x64_nothing": dict(images=[(508, 64, 64)], new_shape=64),       # nothing to do
    "auto_shared": dict(images=[(509, 50, 83), (510, 50, 83)], new_shape=96, auto=True),  # 58 x 96 in the minimum rectangle 64 x 96
    "scale_fill": dict(images=[(511, 41, 70)], new_shape=64, scale_fill=True),
    "no_scaleup": dict(images=[(512, 30, 44)], new_shape=64, scaleup=False),              # smaller than the target: stays 30 x 44
    "not_centred": dict(images=[(513, 37, 53)], new_shape=64, center=False),
    "odd_identity": dict(images=[(514, 45, 64)], new_shape=64),                           # 19 rows of padding: top 9, bottom 10
    "rect_target": dict(images=[(515, 71, 45)], new_shape=(64, 96)),                      # a (h, w) target
}
TABLE_CASES = list(CASES)[:8]
PRE_CASES = ("s37x53", "s48x64_identity", "auto_shared")  # the fixtures that also hold BasePredictor.preprocess's output
SWITCHES = ("auto", "scale_fill", "scaleup", "center", "stride")


def case_switches(c):
    return dict(auto=c.get("auto", False), scale_fill=c.get("scale_fill", False), scaleup=c.get("scaleup", True), center=c.get("center", True),
                stride=c.get("stride", 32))


def seeded_image(seed, h, w):
    """an (h, w, 3) uint8 image from numpy's frozen legacy stream"""
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def case_images(name):
    return [seeded_image(*spec) for spec in CASES[name]["images"]]


def seeded_boxes(seed, n, shape, cols=6):
    """n rows (x1, y1, x2, y2, conf, cls) around a (h, w) image: corners from 12 pixels outside to 12 inside every border, so that every border
    is straddled, plus rows that lie wholly outside, on the border, and a zero row"""
    rs = np.random.RandomState(seed)
    h, w = shape
    b = np.zeros((n, cols), dtype=np.float32)
    b[:, 0] = rs.uniform(-12, w + 12, n)
    b[:, 1] = rs.uniform(-12, h + 12, n)
    b[:, 2] = b[:, 0] + rs.uniform(0, w / 2, n)
    b[:, 3] = b[:, 1] + rs.uniform(0, h / 2, n)
    b[0, :4] = (-5.5, -7.25, 3.5, 2.75)             # straddles the top-left corner
    b[1, :4] = (w - 4.5, h - 3.25, w + 6.5, h + 9)  # straddles the bottom-right corner
    b[2, :4] = (-30, -30, -20, -20)                 # wholly outside
    b[3, :4] = (0, 0, w, h)                         # on the border
    b[4, :4] = (w + 3, 5, w + 9, 11)                # beyond the right edge
    if cols > 4:
        b[:, 4] = rs.uniform(0.05, 1, n)
        b[:, 5] = rs.randint(0, 3, n)
    return torch.from_numpy(b)


# ---------------------------------------------------------------------------------------------------------------- letterbox
def geometry(shape, new_shape, auto=False, scale_fill=False, scaleup=True, center=True, stride=32, fault=None):
    """-> ((hs, ws), (top, bottom, left, right), (r_h, r_w)): LetterBox.__call__'s host arithmetic"""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    ratio = r, r
    rnd = math.floor if fault == "floor" else round
    new_unpad = int(rnd(shape[1] * r)), int(rnd(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)
    elif scale_fill:
        dw, dh = 0.0, 0.0
        new_unpad = (new_shape[1], new_shape[0])
        ratio = new_shape[1] / shape[1], new_shape[0] / shape[0]
    if center:
        dw /= 2
        dh /= 2
    tenth = 0.0 if fault == "no_tenth" else 0.1
    top, bottom = int(round(dh - tenth)) if center else 0, int(round(dh + 0.1))
    left, right = int(round(dw - tenth)) if center else 0, int(round(dw + 0.1))
    return (new_unpad[1], new_unpad[0]), (top, bottom, left, right), (float(ratio[1]), float(ratio[0]))


def resize_values(img, size):
    """the float32 interpolation of the BYTE VALUES of an (h, w, 3) uint8 tensor to (hs, ws), before rounding -> float32 [hs, ws, 3]"""
    x = img.permute(2, 0, 1)[None].float()
    return TR.bilinear_resize(x, size)[0].permute(1, 2, 0)


def resize_u8(img, size):
    """(h, w, 3) uint8 tensor -> (hs, ws, 3) uint8: resize_values rounded to a grey level by floor(v + 0.5); the identity size returns the bytes"""
    if tuple(img.shape[:2]) == tuple(size):
        return img
    return (resize_values(img, size) + 0.5).floor().to(torch.uint8)


def letterbox_u8(img, new_shape, fault=None, **switches):
    """what LetterBox(new_shape, **switches)(image=img) returns: -> ((H, W, 3) uint8 tensor, ((r_h, r_w), (left, top)))"""
    img = torch.from_numpy(np.ascontiguousarray(img)) if isinstance(img, np.ndarray) else img
    (hs, ws), (top, bottom, left, right), ratio = geometry(tuple(img.shape[:2]), new_shape, fault=fault, **switches)
    out = torch.full((top + hs + bottom, left + ws + right, 3), 0 if fault == "pad0" else PAD_LEVEL, dtype=torch.uint8)
    out[top : top + hs, left : left + ws] = resize_u8(img, (hs, ws))
    return out, (ratio, (left, top))


def letterbox(images, new_shape, bgr=True, normalize=True, fault=None, **switches):
    """what ops.letterbox computes -> (float32 [n, 3, H, W], ratio_pad): letterbox_u8 of every image, then predictor.py:153-161"""
    outs, rps = zip(*[letterbox_u8(im, new_shape, fault=fault, **switches) for im in images])
    im = torch.stack(outs)
    if bgr and fault != "rgb":
        im = im.flip(-1)
    im = im.permute(0, 3, 1, 2).contiguous().float()
    if normalize:
        im = im / 255
    return im, list(rps)


# --------------------------------------------------------------------------------------------------------------- scale_boxes
def scale_boxes_params(img_shape, ori_shape, ratio_pad=None, fault=None):
    """(gain, pad_x, pad_y, w0, h0): the head of scale_boxes"""
    if ratio_pad is None:
        gain = min(img_shape[0] / ori_shape[0], img_shape[1] / ori_shape[1])
        tenth = 0.0 if fault == "no_tenth" else 0.1
        pad = (round((img_shape[1] - ori_shape[1] * gain) / 2 - tenth), round((img_shape[0] - ori_shape[0] * gain) / 2 - tenth))
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    return float(gain), float(pad[0]), float(pad[1]), float(ori_shape[1]), float(ori_shape[0])


def scale_rows(boxes, params, padding=True, xywh=False, fault=None):
    """[n, 4+] float32 -> new tensor, in the header's order: subtract the pad, IEEE float32 division by float32(gain), clamp, copy the rest"""
    gain, px, py, w0, h0 = (torch.tensor(v, dtype=torch.float32) for v in params)
    out = boxes.clone()
    x1, y1, x2, y2 = (boxes[:, i] for i in range(4))
    if padding:
        x1, y1 = x1 - px, y1 - py
        if not xywh:
            x2, y2 = x2 - px, y2 - py
    if fault == "reciprocal":
        rc = torch.tensor(1.0, dtype=torch.float32) / gain
        x1, y1, x2, y2 = x1 * rc, y1 * rc, x2 * rc, y2 * rc
    else:
        x1, y1, x2, y2 = x1 / gain, y1 / gain, x2 / gain, y2 / gain
    if fault != "no_clip":
        zero = torch.tensor(0.0)
        x1, x2 = (torch.minimum(torch.maximum(v, zero), w0) for v in (x1, x2))
        y1, y2 = (torch.minimum(torch.maximum(v, zero), h0) for v in (y1, y2))
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x1, y1, x2, y2
    return out


def scale_boxes(det, count, img_shape, ori_shapes, ratio_pads=None, padding=True, xywh=False, fault=None):
    """what ops.scale_boxes computes on (det [B, max_det, 6], count [B]) -> new det; rows at or beyond count are zero"""
    out = torch.zeros_like(det)
    for b in range(det.shape[0]):
        n = int(count[b])
        rp = None if ratio_pads is None else ratio_pads[b]
        out[b, :n] = scale_rows(det[b, :n], scale_boxes_params(img_shape, ori_shapes[b], rp, fault), padding, xywh, fault)
    return out


def xywh2xyxy(x):
    xy, half = x[..., :2], x[..., 2:] / 2
    return torch.cat((xy - half, xy + half), -1)


def xyxy2xywh(x):
    return torch.stack(((x[:, 0] + x[:, 2]) / 2, (x[:, 1] + x[:, 3]) / 2, x[:, 2] - x[:, 0], x[:, 3] - x[:, 1]), 1)


def prepare_labels(bboxes, imgsz, ori_shape, ratio_pad):
    """_prepare_batch's boxes: normalised xywh [n, 4] -> xyxy in the pixels of the original image"""
    h, w = imgsz
    box = xywh2xyxy(bboxes.float()) * torch.tensor([w, h, w, h], dtype=torch.float32)
    return scale_rows(box, scale_boxes_params(imgsz, ori_shape, ratio_pad))


def boxes_properties(data, orig_shape):
    """the Boxes properties of engine/results.py on data [n, 6]"""
    xyxy = data[:, :4]
    wh = torch.tensor([orig_shape[1], orig_shape[0], orig_shape[1], orig_shape[0]], dtype=torch.float32)
    return dict(xyxy=xyxy, conf=data[:, -2], cls=data[:, -1], xywh=xyxy2xywh(xyxy), xyxyn=xyxy / wh, xywhn=xyxy2xywh(xyxy) / wh)


# the validator fixture's batch: two images letterboxed to 64 x 96, with the ori_shape / ratio_pad a letterboxing dataset attaches
VAL_IMGSZ = (64, 96)
VAL_ORI = [(50, 83), (120, 150)]


def val_batch():
    """-> (batch dict without the image, predictions [[n_i, 6]]) rebuilt from seeds"""
    rs = np.random.RandomState(601)
    ratio_pads = []
    for h0, w0 in VAL_ORI:
        (hs, ws), (top, _, left, _), _ = geometry((h0, w0), VAL_IMGSZ)
        ratio_pads.append(((hs / h0, ws / w0), (left, top)))  # (as the reference's dataset states the resize ratio: resized / original)
    n = 9
    xy = rs.uniform(0.15, 0.85, (n, 2))
    wh = rs.uniform(0.05, 0.5, (n, 2))
    batch = dict(batch_idx=torch.tensor([0, 0, 0, 0, 1, 1, 1, 1, 1], dtype=torch.float32), cls=torch.from_numpy(rs.randint(0, 3, (n, 1)).astype(np.float32)),
                 bboxes=torch.from_numpy(np.concatenate([xy, wh], 1).astype(np.float32)), ori_shape=list(VAL_ORI), ratio_pad=ratio_pads)
    preds = [seeded_boxes(611 + i, 12, VAL_IMGSZ) for i in range(2)]
    return batch, preds
