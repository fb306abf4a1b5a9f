"""Oriented-box ops over the C ABI (csrc/loss.hip): the OBB head's angle, the dense xywhr targets, v8OBBLoss's stages and the head's eval
output (reference: nn/modules/head.py:211-238, utils/loss.py:607-720, utils/tal.py:329-416, utils/metrics.py:178-239)."""
import ctypes

import torch

from .._lib import as_ymi, check, is_nhwc, ptr, stream_ptr, workspace
from .base import L
from .blocks import _map_array
from .conv import padded_grad_like


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
        pairs = [padded_grad_like(t, zero=False) for t in maps]
        if len({p[0].shape[1] for p in pairs}) != 1:  # (levels padded differently: the kernel takes one width)
            pairs = [(v, v) for v in (torch.empty_like(t) for t in maps)]
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
    out = torch.empty(batch_size, max_boxes, 6, dtype=torch.float32, device=device)
    bi = batch_idx.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    cl = cls.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    bb = bboxes.to(device=device, dtype=torch.float32).reshape(-1, 5).contiguous()
    check(L().ymi_obb_targets(ptr(bi) if n else None, ptr(cl) if n else None, ptr(bb) if n else None, n, batch_size, max_boxes, float(img_w),
                              float(img_h), ptr(out), stream_ptr()), "obb_targets")
    return out


class _ObbLoss(torch.autograd.Function):
    """(box maps, class maps, angle) -> (loss [3] * scale[:3], items [3] = loss * scale[3:]) as _DetectLoss, with the rotated decode, metric,
    box term and the angle's gradient."""

    @staticmethod
    def forward(ctx, targets, strides, topk, alpha, beta, scale6, angle, *maps):
        nl = len(maps) // 2
        box, cls = maps[:nl], maps[nl:]
        dev = box[0].device
        b = box[0].shape[0]
        anchors = sum(int(t.shape[2] * t.shape[3]) for t in box)
        g = int(targets.shape[1])
        if angle.numel() != b * anchors or angle.dtype != torch.float32 or not angle.is_contiguous() or tuple(targets.shape) != (b, g, 6):
            raise ValueError(f"obb_loss: angle {tuple(angle.shape)} {angle.dtype} / targets {tuple(targets.shape)} do not belong to {b} images of {anchors} anchors")
        sb, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(L().ymi_obb_loss_sizes(b, anchors, g, ctypes.byref(sb), ctypes.byref(wb)), "obb_loss_sizes")
        state = torch.empty(sb.value, dtype=torch.uint8, device=dev)
        ws = workspace(wb.value, dev, "obbloss")
        out = torch.empty(6, dtype=torch.float32, device=dev)
        st = (ctypes.c_float * nl)(*[float(s) for s in strides])
        check(
            L().ymi_obb_loss_fwd(nl, _map_array(box), _map_array(cls), ptr(angle), st, ptr(targets), g, int(topk), float(alpha), float(beta), ptr(scale6),
                                 ptr(out), ptr(state), state.numel(), ptr(ws), ws.numel(), stream_ptr()),
            "obb_loss_fwd",
        )
        ctx.save_for_backward(state, scale6, angle, *maps)
        ctx.strides = st
        loss, items = out[:3], out[3:]
        ctx.mark_non_differentiable(items)
        ctx.set_materialize_grads(False)
        return loss, items

    @staticmethod
    def backward(ctx, gl, _gitems):
        state, scale6, angle, *maps = ctx.saved_tensors
        nl = len(maps) // 2
        box, cls = maps[:nl], maps[nl:]
        if gl is None:
            return (None,) * (7 + len(maps))
        if gl.dtype != torch.float32 or not gl.is_contiguous():
            gl = gl.to(torch.float32).contiguous()
        dbox = [torch.empty_like(t) for t in box]
        pairs = [padded_grad_like(t, zero=False) for t in cls]
        if len({p[0].shape[1] for p in pairs}) != 1:
            pairs = [(v, v) for v in (padded_grad_like(t)[1] for t in cls)]
        dcls_k, dcls = [p[0] for p in pairs], [p[1] for p in pairs]
        dangle = torch.empty_like(angle)
        check(
            L().ymi_obb_loss_bwd(nl, _map_array(box), _map_array(cls), ptr(angle), ctx.strides, ptr(state), state.numel(), ptr(gl), ptr(scale6),
                                 _map_array(dbox), _map_array(dcls_k), ptr(dangle), stream_ptr()),
            "obb_loss_bwd",
        )
        return (None, None, None, None, None, None, dangle, *dbox, *dcls)


def obb_loss(box_maps, cls_maps, angle, strides, targets, scale6, topk=10, alpha=0.5, beta=6.0):
    """-> (loss [3] * scale6[:3] (differentiable in the maps and the angle), items [3] = loss * scale6[3:] (detached))."""
    return _ObbLoss.apply(targets, tuple(strides), topk, alpha, beta, scale6, angle, *box_maps, *cls_maps)


def detect_decode_obb(box_maps, cls_maps, angle, strides):
    """OBB's eval output cat([dist2rbox boxes * stride, class sigmoids, angle], 1) -> [B, 4 + nc + 1, A] float32 in one launch (no gradient)."""
    nl = len(box_maps)
    b = box_maps[0].shape[0]
    nc = cls_maps[0].shape[1]
    anchors = sum(int(t.shape[2] * t.shape[3]) for t in box_maps)
    angle = angle.detach()
    if angle.numel() != b * anchors or angle.dtype != torch.float32 or not angle.is_contiguous():
        raise ValueError(f"detect_decode_obb: angle {tuple(angle.shape)} {angle.dtype} is not the float32 [B, 1, A] of {b} images of {anchors} anchors")
    y = torch.empty((b, 4 + nc + 1, anchors), dtype=torch.float32, device=box_maps[0].device)
    st = (ctypes.c_float * nl)(*[float(s) for s in strides])
    check(L().ymi_detect_decode_obb(nl, _map_array([t.detach() for t in box_maps]), _map_array([t.detach() for t in cls_maps]), ptr(angle), st, ptr(y),
                                    stream_ptr()), "detect_decode_obb")
    return y
