"""ops.val_match: the validator's per-image work after NMS as one launch (csrc/valmatch.hip, include/ymi.h: ymi_val_match)."""
import ctypes

import torch

from .._lib import VALMATCH_CHUNK, VALMATCH_MAX_DET, VALMATCH_MAX_LEVELS, check, ptr, stream_ptr
from .base import L
from .resize import scale_boxes_params

VAL_MATCH_LABEL_CHUNK = VALMATCH_CHUNK  # label rows the kernel stages at a time (tests size their label tables by it)


def val_match(det, count, batch_idx, cls, bboxes, img_shape, levels, ori_shapes=None, ratio_pads=None, single_cls=False, cm=None, cm_conf=0.25,
              cm_iou=0.45):
    """models/yolo/detect/val.py:174-216 after NMS - label boxes, box_iou, match_predictions at every IoU level and, with `cm`,
    ConfusionMatrix.process_batch - for a whole batch, one launch, on the device; nothing synchronises.
    det [B, max_det, 6] float32 and count [B] int32 as ops.detect_nms / ops.scale_boxes leave them; batch_idx [L], cls [L] (or [L, 1]),
    bboxes [L, 4] normalised xywh: the batch's labels in the batch's own order, on the device; img_shape: (h, w) of the network input;
    levels: the IoU levels (a host sequence or tensor, at most 16); ori_shapes / ratio_pads: per image as ops.scale_boxes takes them -
    then the labels are matched in native space, where ops.scale_boxes has put the detections; cm: an int32 [(nc + 1), (nc + 1)] device
    tensor that the batch's confusion counts are ADDED to (row: predicted class, column: labelled class, nc: background).
    -> tp [B, max_det, len(levels)] uint8 on the device, zero past the count."""
    if not det.is_cuda:
        raise RuntimeError("libyolo_mi355 kernels need tensors on the MI355X (cuda) device; there is no CPU path")
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous():
        raise ValueError(f"val_match takes a contiguous float32 [B, max_det, 6] tensor, got {tuple(det.shape)} {det.dtype}")
    b, max_det = int(det.shape[0]), int(det.shape[1])
    if not 1 <= max_det <= VALMATCH_MAX_DET or b < 1:
        raise ValueError(f"val_match: max_det in [1, {VALMATCH_MAX_DET}] and at least one image, got {tuple(det.shape)}")
    if count.dtype != torch.int32 or tuple(count.shape) != (b,) or not count.is_cuda or not count.is_contiguous():
        raise ValueError("val_match: count is an int32 [B] tensor on the device")
    lv = [float(v) for v in (levels.tolist() if torch.is_tensor(levels) else levels)]
    if not 1 <= len(lv) <= VALMATCH_MAX_LEVELS:
        raise ValueError(f"val_match: 1 to {VALMATCH_MAX_LEVELS} IoU levels, got {len(lv)}")
    dev = det.device
    n_lab = int(batch_idx.numel())
    if int(cls.numel()) != n_lab or int(bboxes.numel()) != 4 * n_lab:
        raise ValueError(f"val_match: {n_lab} batch_idx rows, {cls.numel()} classes, {tuple(bboxes.shape)} boxes")
    lab_img = batch_idx.detach().to(dev).reshape(-1).to(torch.int32).contiguous()
    lab_cls = cls.detach().to(dev).reshape(-1).float().contiguous()
    lab_box = bboxes.detach().to(dev).reshape(-1, 4).float().contiguous()
    native = None
    if ori_shapes is not None:
        if isinstance(ori_shapes[0], (int, float)):
            ori_shapes = [ori_shapes] * b
        if ratio_pads is None or (len(ratio_pads) == 2 and ratio_pads[0] is not None and isinstance(ratio_pads[0][0], (int, float))):  # one for all
            ratio_pads = [ratio_pads] * b
        if len(ori_shapes) != b or len(ratio_pads) != b:
            raise ValueError("val_match: one original shape (and one ratio_pad) per image")
        native = torch.tensor([scale_boxes_params(img_shape, o, rp) for o, rp in zip(ori_shapes, ratio_pads)], dtype=torch.float32).reshape(b, 5).to(dev)
    nc = 0
    if cm is not None:
        if not cm.is_cuda or cm.dtype != torch.int32 or cm.dim() != 2 or cm.shape[0] != cm.shape[1] or cm.shape[0] < 2 or not cm.is_contiguous():
            raise ValueError("val_match: cm is a contiguous int32 [(nc + 1), (nc + 1)] tensor on the device")
        nc = int(cm.shape[0]) - 1
    tp = torch.empty((b, max_det, len(lv)), dtype=torch.uint8, device=dev)
    arr = (ctypes.c_float * len(lv))(*lv)
    check(L().ymi_val_match(ptr(det.detach()), ptr(count), b, max_det, ptr(lab_img), ptr(lab_cls), ptr(lab_box), n_lab, float(img_shape[1]), float(img_shape[0]),
                            ptr(native), arr, len(lv), int(bool(single_cls)), ptr(tp), ptr(cm), nc, float(cm_conf), float(cm_iou), stream_ptr()), "val_match")
    return tp


def val_match_masks(det, count, batch_idx, cls, inter, area_pred, area_gt, levels, single_cls=False):
    """val_match's tp rule with mask_iou in place of box_iou (reference models/yolo/segment/val.py:231-273, overlap=True), one launch
    (ymi_val_match_masks): the overlap of detection d with the image's j-th label (table order) is
    inter[d, j + 1] / ((area_gt[j + 1] + area_pred[d]) - inter[d, j + 1] + 1e-7) in float32 on ops.mask_overlap's integer counts; labels at or
    beyond n_bins - 1 overlap nothing.  -> tp_m [B, max_det, len(levels)] uint8 on the device, zero past the count."""
    if not det.is_cuda:
        raise RuntimeError("libyolo_mi355 kernels need tensors on the MI355X (cuda) device; there is no CPU path")
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous():
        raise ValueError(f"val_match_masks takes a contiguous float32 [B, max_det, 6] tensor, got {tuple(det.shape)} {det.dtype}")
    b, max_det = int(det.shape[0]), int(det.shape[1])
    if not 1 <= max_det <= VALMATCH_MAX_DET or b < 1:
        raise ValueError(f"val_match_masks: max_det in [1, {VALMATCH_MAX_DET}] and at least one image, got {tuple(det.shape)}")
    if count.dtype != torch.int32 or tuple(count.shape) != (b,) or not count.is_cuda or not count.is_contiguous():
        raise ValueError("val_match_masks: count is an int32 [B] tensor on the device")
    n_bins = int(inter.shape[-1])
    for name, t, shape in (("inter", inter, (b, max_det, n_bins)), ("area_pred", area_pred, (b, max_det)), ("area_gt", area_gt, (b, n_bins))):
        if tuple(t.shape) != shape or t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"val_match_masks: {name} is a contiguous int32 {shape} device tensor, got {tuple(t.shape)} {t.dtype}")
    lv = [float(v) for v in (levels.tolist() if torch.is_tensor(levels) else levels)]
    if not 1 <= len(lv) <= VALMATCH_MAX_LEVELS:
        raise ValueError(f"val_match_masks: 1 to {VALMATCH_MAX_LEVELS} IoU levels, got {len(lv)}")
    dev = det.device
    n_lab = int(batch_idx.numel())
    if int(cls.numel()) != n_lab:
        raise ValueError(f"val_match_masks: {n_lab} batch_idx rows, {cls.numel()} classes")
    lab_img = batch_idx.detach().to(dev).reshape(-1).to(torch.int32).contiguous()
    lab_cls = cls.detach().to(dev).reshape(-1).float().contiguous()
    tp = torch.empty((b, max_det, len(lv)), dtype=torch.uint8, device=dev)
    arr = (ctypes.c_float * len(lv))(*lv)
    check(L().ymi_val_match_masks(ptr(det.detach()), ptr(count), b, max_det, ptr(lab_img), ptr(lab_cls), n_lab, ptr(inter), ptr(area_pred), ptr(area_gt), n_bins,
                                  arr, len(lv), int(bool(single_cls)), ptr(tp), stream_ptr()), "val_match_masks")
    return tp
