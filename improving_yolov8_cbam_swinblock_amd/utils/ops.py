"""small helpers with the reference's names (ultralytics/utils/ops.py)."""
import math

import torch


def make_divisible(x, divisor):
    """reference utils/ops.py:130-143."""
    if isinstance(divisor, torch.Tensor):
        divisor = int(divisor.max())
    return math.ceil(x / divisor) * divisor


def xywh2xyxy(x):
    """reference utils/ops.py:432-449."""
    xy, half = x[..., :2], x[..., 2:] / 2
    return torch.cat((xy - half, xy + half), -1)


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, nc=0,
                        max_nms=30000, max_wh=7680, labels=(), rotated=False, end2end=False):
    """reference utils/ops.py:181-332 -> list of [n_i, 6] tensors (x1, y1, x2, y2, conf, cls), one per image, on the prediction's device.
    prediction: the decoded Detect output [B, 4 + nc, A], or the (y, maps) tuple of the eval forward.  With `nc` given and nm mask
    coefficient rows behind the nc scores (Segment's output [B, 4 + nc + nm, A]) the rows are [n_i, 6 + nm], the kept anchors' coefficients
    behind the six columns, as in the reference (ops.detect_nms_seg).  The work is ops.detect_nms (HIP,
    csrc/nms.hip); this wrapper adds the ONE synchronisation: the counts go to the host once, then the rows are sliced.  Equal scores are
    ordered by ascending anchor, then class (the reference leaves ties to its libraries).  The reference's wall-clock `time_limit` break
    (ops.py:328-330) is deliberately not reproduced: a result that depends on the host's clock cannot be pinned.  The input is not
    modified.  An empty `classes` list keeps nothing, as in the reference.  Not built: rotated boxes, apriori labels, end2end models."""
    from .. import ops

    if not 0 <= conf_thres <= 1:
        raise ValueError(f"invalid confidence threshold {conf_thres}: valid values are between 0.0 and 1.0")
    if not 0 <= iou_thres <= 1:
        raise ValueError(f"invalid IoU threshold {iou_thres}: valid values are between 0.0 and 1.0")
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if rotated or end2end or (labels is not None and len(labels)) or prediction.shape[-1] == 6:
        raise NotImplementedError("non_max_suppression: rotated boxes, apriori labels and end2end outputs are not built")
    if nc and prediction.shape[1] - 4 - nc != 0:
        if not prediction.is_cuda:  # (a NotImplementedError is a RuntimeError: the plain rows' "no CPU path" refusal, named for what is missing)
            raise NotImplementedError(f"non_max_suppression: {prediction.shape[1] - 4 - nc} mask channels behind {nc} classes are gathered by the NMS "
                                      "kernel on the MI355X (cuda) device (ops.detect_nms_seg); a host path for them is not built")
        det, coef, count = ops.detect_nms_seg(prediction, nc, conf_thres, iou_thres, multi_label=multi_label, agnostic=agnostic, classes=classes,
                                              max_det=max_det, max_nms=max_nms, max_wh=max_wh)
        rows = torch.cat((det, coef), 2)
        return [rows[i, :n] for i, n in enumerate(count.tolist())]
    det, count = ops.detect_nms(prediction, conf_thres, iou_thres, multi_label=multi_label, agnostic=agnostic, classes=classes, max_det=max_det,
                                max_nms=max_nms, max_wh=max_wh)
    return [det[i, :n] for i, n in enumerate(count.tolist())]


def xyxy2xywh(x):
    """reference utils/ops.py:412-429."""
    assert x.shape[-1] == 4, f"input shape last dimension expected 4 but input shape is {x.shape}"
    y = torch.empty_like(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2  # x center
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2  # y center
    y[..., 2] = x[..., 2] - x[..., 0]  # width
    y[..., 3] = x[..., 3] - x[..., 1]  # height
    return y


def clip_boxes(boxes, shape):
    """reference utils/ops.py:335-354: clamps x to [0, shape[1]] and y to [0, shape[0]] in place and returns its argument.  A cuda [n, 4+]
    float32 tensor or view goes through ymi_scale_boxes (gain 1, no padding: x / 1 is x); host tensors - the validator's few label boxes -
    take the reference's statements."""
    if boxes.is_cuda:
        from .. import ops

        return ops.scale_rows(boxes, [1.0, 0.0, 0.0, float(shape[1]), float(shape[0])], padding=False)
    boxes[..., 0] = boxes[..., 0].clamp(0, shape[1])  # x1
    boxes[..., 1] = boxes[..., 1].clamp(0, shape[0])  # y1
    boxes[..., 2] = boxes[..., 2].clamp(0, shape[1])  # x2
    boxes[..., 3] = boxes[..., 3].clamp(0, shape[0])  # y2
    return boxes


def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None, padding=True, xywh=False):
    """reference utils/ops.py:93-127: boxes [n, 4+] from the letterboxed img1_shape (h, w) back to img0_shape, clipped, IN PLACE; returns its
    argument.  Gain and pad are the reference's host arithmetic (ops.scale_boxes_params); a cuda tensor or view such as pred[:, :4] goes
    through ymi_scale_boxes (csrc/resize.hip), host tensors - the validator's few label boxes - take the reference's statements."""
    from .. import ops

    gain, pad_x, pad_y, w0, h0 = ops.scale_boxes_params(img1_shape, img0_shape, ratio_pad)
    if boxes.is_cuda:
        return ops.scale_rows(boxes, [gain, pad_x, pad_y, w0, h0], padding=padding, xywh=xywh)
    if padding:
        boxes[..., 0] -= pad_x  # x padding
        boxes[..., 1] -= pad_y  # y padding
        if not xywh:
            boxes[..., 2] -= pad_x  # x padding
            boxes[..., 3] -= pad_y  # y padding
    boxes[..., :4] /= gain
    return clip_boxes(boxes, img0_shape)


def crop_mask(masks, boxes):
    """reference utils/ops.py:661-677: masks [n, h, w] times the indicator of boxes [n, 4] (x1, y1, x2, y2 in mask pixels): column c is
    kept where c >= x1 and c < x2, row r where r >= y1 and r < y2.  Torch statements on the tensors' own device (the fused form on the
    device is ops.process_mask)."""
    _, h, w = masks.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    c = torch.arange(w, device=masks.device, dtype=x1.dtype)[None, None, :]
    r = torch.arange(h, device=masks.device, dtype=x1.dtype)[None, :, None]
    return masks * ((c >= x1) * (c < x2) * (r >= y1) * (r < y2))


def process_mask(protos, masks_in, bboxes, shape, upsample=False):
    """reference utils/ops.py:680-710, per image: protos [nm, mh, mw], masks_in [n, nm] (the NMS rows' coefficient columns), bboxes [n, 4] in
    the pixels of the network input `shape` = (h, w) -> [n, mh, mw], or [n, h, w] with upsample=True.
    Returns uint8 0 / 1 where the reference returns float 0 / 1: the values are the same, a mask stack is a quarter the size.  cuda tensors
    go through ops.process_mask (HIP, csrc/maskdec.hip: nm = 32 only); host tensors take the reference's torch statements."""
    if protos.is_cuda:
        from .. import ops

        img = torch.zeros(masks_in.shape[0], dtype=torch.int32, device=protos.device)
        return ops.process_mask(protos[None], bboxes[:, :4], masks_in, img, shape, upsample=upsample)[0]
    c, mh, mw = protos.shape
    ih, iw = shape
    masks = (masks_in.float() @ protos.float().view(c, -1)).view(-1, mh, mw)
    boxes = bboxes[:, :4].float().clone()
    boxes[:, 0] *= mw / iw
    boxes[:, 2] *= mw / iw
    boxes[:, 3] *= mh / ih
    boxes[:, 1] *= mh / ih
    masks = crop_mask(masks, boxes)
    if upsample:
        masks = torch.nn.functional.interpolate(masks[None], tuple(shape), mode="bilinear", align_corners=False)[0]
    return masks.gt(0.0).to(torch.uint8)


def process_mask_native(protos, masks_in, bboxes, shape):
    """reference utils/ops.py:713-730 (retina_masks: prototypes upsampled before the crop): not built."""
    raise NotImplementedError("process_mask_native (retina_masks) is not built: use process_mask(..., upsample=True)")


def scale_masks(masks, shape, padding=True):
    """reference utils/ops.py:733-757 (masks resampled into the original image): not built."""
    raise NotImplementedError("scale_masks (masks resampled to the original image, retina_masks) is not built: masks stay at the letterboxed input shape")
