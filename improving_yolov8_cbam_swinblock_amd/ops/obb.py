"""Oriented-box ops over the C ABI (csrc/loss.hip): the OBB head's angle, the dense xywhr targets, v8OBBLoss's stages and the head's eval
output (reference: nn/modules/head.py:211-238, utils/loss.py:607-720, utils/tal.py:329-416, utils/metrics.py:178-239).  The loss, the targets
and the decode are the detection ops' bodies (ops.blocks: _loss_forward / _loss_backward, _dense_targets, _decode, one_width_grads) with the
oriented entry points and the angle."""
import torch

from .._lib import check, is_nhwc, ptr, stream_ptr
from .base import L
from .blocks import _OBB_FAMILY, _decode, _dense_targets, _loss_backward, _loss_forward, _map_array, one_width_grads


def _logit_maps(maps):
    """the one-channel angle logit maps as the kernels read them: NHWC memory (the [:, :1] view of a padded buffer is read in place)."""
    return [t if is_nhwc(t) else t.contiguous(memory_format=torch.channels_last) for t in maps]


class _ObbAngle(torch.autograd.Function):
    """per-level logit maps [B, 1, H, W] -> angle [B, 1, A] float32 = (sigmoid(logit) - 0.25) * pi in anchor order, one launch (replaces the
    reference's view + cat + sigmoid + scale, head.py:225-227); backward: one launch into the logit-gradient maps."""

    @staticmethod
    def forward(ctx, *maps):
        b = maps[0].shape[0]
        anchors = sum(int(t.shape[2] * t.shape[3]) for t in maps)
        angle = torch.empty((b, 1, anchors), dtype=torch.float32, device=maps[0].device)
        check(L().ymi_obb_angle_fwd(len(maps), _map_array(maps), ptr(angle), stream_ptr()), "obb_angle_fwd")
        ctx.save_for_backward(*maps)
        return angle

    @staticmethod
    def backward(ctx, g):
        maps = ctx.saved_tensors
        if g.dtype != torch.float32 or not g.is_contiguous():
            g = g.to(torch.float32).contiguous()
        pairs = one_width_grads(maps, torch.empty_like)
        check(L().ymi_obb_angle_bwd(len(maps), _map_array(maps), ptr(g), _map_array([p[0] for p in pairs]), stream_ptr()), "obb_angle_bwd")
        return tuple(p[1] for p in pairs)


def obb_angle(logit_maps):
    """-> angle [B, 1, A] float32 radians in [-pi/4, 3pi/4] (differentiable)."""
    maps = _logit_maps(list(logit_maps))
    if any(t.dim() != 4 or t.shape[1] != 1 for t in maps):
        raise ValueError(f"obb_angle takes one-channel maps [B, 1, H, W], got {[tuple(t.shape) for t in maps]}")
    if not maps[0].is_cuda:
        raise RuntimeError("libyolo_mi355 kernels need tensors on the MI355X (cuda) device; there is no CPU path")
    return _ObbAngle.apply(*maps)


def obb_targets(batch_idx, cls, bboxes, batch_size, max_boxes, img_w, img_h, device):
    """ragged (image, class, xywhr) rows -> dense [B, max_boxes, 6] (class, xywh in pixels, angle) behind the reference's tiny-box filter
    (loss.py:652-657)."""
    n = int(batch_idx.numel())
    if bboxes.numel() != n * 5:
        raise ValueError(f"oriented-box labels are [n, 5] xywhr rows, got {tuple(bboxes.shape)} for {n} labels")
    return _dense_targets(L().ymi_obb_targets, "obb_targets", 5, batch_idx, cls, bboxes, batch_size, max_boxes, img_w, img_h, device)


class _ObbLoss(torch.autograd.Function):
    """(box maps, class maps, angle) -> (loss [3] * scale[:3], items [3] = loss * scale[3:]) as _DetectLoss, with the rotated decode, metric,
    box term and the angle's gradient."""

    @staticmethod
    def forward(ctx, targets, strides, topk, alpha, beta, scale6, angle, *maps):
        return _loss_forward(ctx, _OBB_FAMILY, targets, strides, topk, alpha, beta, scale6, maps, angle=angle)[:2]

    @staticmethod
    def backward(ctx, gl, _gitems):
        return _loss_backward(ctx, _OBB_FAMILY, gl, has_angle=True)


def obb_loss(box_maps, cls_maps, angle, strides, targets, scale6, topk=10, alpha=0.5, beta=6.0):
    """-> (loss [3] * scale6[:3] (differentiable in the maps and the angle), items [3] = loss * scale6[3:] (detached))."""
    return _ObbLoss.apply(targets, tuple(strides), topk, alpha, beta, scale6, angle, *box_maps, *cls_maps)


def detect_decode_obb(box_maps, cls_maps, angle, strides):
    """OBB's eval output cat([dist2rbox boxes * stride, class sigmoids, angle], 1) -> [B, 4 + nc + 1, A] float32 in one launch (no gradient)."""
    b = box_maps[0].shape[0]
    anchors = sum(int(t.shape[2] * t.shape[3]) for t in box_maps)
    angle = angle.detach()
    if angle.numel() != b * anchors or angle.dtype != torch.float32 or not angle.is_contiguous():
        raise ValueError(f"detect_decode_obb: angle {tuple(angle.shape)} {angle.dtype} is not the float32 [B, 1, A] of {b} images of {anchors} anchors")
    return _decode(L().ymi_detect_decode_obb, "detect_decode_obb", box_maps, cls_maps, strides, 1, ptr(angle))
