"""Instance segmentation ops over the C ABI (csrc/seg.hip, csrc/loss.hip): Proto's transposed convolution as a 1x1 GEMM + depth to space,
the detection loss that hands its assignment over, the mask loss, Segment's decode (reference: nn/modules/block.py:80-100,
nn/modules/head.py:186-208, utils/loss.py:258-438)."""
import ctypes

import torch

from .._lib import ACT_NONE, as_ymi, check, chunk_elems, empty_nhwc, is_nhwc, ptr, stream_ptr, workspace, ymi_dtype
from .base import L, _byref, _note_use, grad_nhwc, join_of
from .blocks import _DETECT_FAMILY, _DetectLoss, _decode, _loss_forward, _map_array
from .conv import _dgrad_joined

NM = 32  # prototypes the mask-loss kernels are built for (csrc/seg.hip)


def depth_to_space2(x):
    """[N, 4C, H, W] (channel (2a + b) * C + c) -> [N, C, 2H, 2W]; no gradient of its own (see _ConvTranspose2x2)."""
    n, c4, h, w = x.shape
    out = empty_nhwc(n, c4 // 4, 2 * h, 2 * w, x.dtype, x.device)
    check(L().ymi_depth_to_space2(_byref(as_ymi(x)), _byref(as_ymi(out)), stream_ptr()), "depth_to_space2")
    return out


def space_to_depth2(x):
    """the inverse: [N, C, 2H, 2W] -> [N, 4C, H, W]."""
    n, c, h2, w2 = x.shape
    out = empty_nhwc(n, 4 * c, h2 // 2, w2 // 2, x.dtype, x.device)
    check(L().ymi_space_to_depth2(_byref(as_ymi(x)), _byref(as_ymi(out)), stream_ptr()), "space_to_depth2")
    return out


class _ConvTranspose2x2(torch.autograd.Function):
    """nn.ConvTranspose2d(c1, c2, 2, 2, 0, bias=True) on an internal tensor.  Kernel 2 at stride 2 has no overlapping taps:
    y[n, o, 2i + a, 2j + b] = sum_c x[n, c, i, j] * W[c, o, a, b] + bias[o] is a 1x1 convolution with the [4 * c2, c1] weight
    Wg[(2a + b) * c2 + o, c] = W[c, o, a, b] and the bias repeated four times, followed by depth to space.  Backward: space to depth of
    the output gradient, then the 1x1 data- and weight-gradient GEMMs; dW and dbias are returned in the module's own layout.  The GEMM
    view of the weight is a temporary, so its operands are packed per call and its weight gradient is complete when this returns
    (neither the weight arena nor the deferred slab sums, which both know operands by their parameter)."""

    @staticmethod
    def forward(ctx, x, weight, bias, join=None):
        dtype, dev = x.dtype, x.device
        c1, c2 = weight.shape[0], weight.shape[1]
        n, cp, h, w = x.shape
        _note_use(weight)
        wg = weight.detach().permute(2, 3, 1, 0).reshape(4 * c2, c1).contiguous()
        wp = torch.empty(4 * c2 * cp, dtype=dtype, device=dev)
        check(L().ymi_pack_conv_weight_fwd(ptr(wg), 4 * c2, c1, 1, 1, cp, ymi_dtype(dtype), ptr(wp), stream_ptr()), "pack_conv_weight_fwd")
        b4 = bias.detach().float().repeat(4) if bias is not None else None
        deep = empty_nhwc(n, 4 * c2, h, w, dtype, dev)
        check(L().ymi_conv2d_fwd(_byref(as_ymi(x)), ptr(wp), 4 * c2, 1, 1, 1, None, ptr(b4), ACT_NONE, None, _byref(as_ymi(deep)), None, None, stream_ptr()),
              "conv2d_fwd")
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.join = join
        return depth_to_space2(deep)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        dtype, dev = x.dtype, x.device
        c1, c2 = weight.shape[0], weight.shape[1]
        dy = space_to_depth2(grad_nhwc(g, dtype))
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wg = weight.detach().permute(2, 3, 1, 0).reshape(4 * c2, c1).contiguous()
            wd = torch.empty(4 * c2 * c1, dtype=dtype, device=dev)
            check(L().ymi_pack_conv_weight_dgrad_ex(ptr(wg), 4 * c2, 4 * c2, c1, 1, 1, 1, ymi_dtype(dtype), ptr(wd), stream_ptr()), "pack_conv_weight_dgrad")
            dx = _dgrad_joined(ctx.join, dy, None, 1, 1, x.shape, dtype, packed=(wd, c1))
        elif ctx.join is not None:
            raise RuntimeError("conv_transpose2x2: a joined input needs its data gradient")
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or need_b:
            ty, tx = as_ymi(dy), as_ymi(x)
            dwg = torch.empty((4 * c2, c1), dtype=torch.float32, device=dev)
            dbg = torch.empty(ty.c, dtype=torch.float32, device=dev) if need_b else None
            ws = workspace(L().ymi_conv2d_bwd_weight_workspace(ty.n * ty.h * ty.w, ty.c, tx.c, 1, 1), dev, "wgrad")
            check(L().ymi_conv2d_bwd_weight(_byref(tx), _byref(ty), 4 * c2, c1, 1, 1, 1, ptr(dwg), ptr(dbg), ptr(ws), ws.numel(), stream_ptr()), "conv2d_bwd_weight")
            if ctx.needs_input_grad[1]:
                dw = dwg.view(2, 2, c2, c1).permute(3, 2, 0, 1).contiguous()
            if need_b:
                db = dbg[: 4 * c2].view(4, c2).sum(0)
        return dx, dw, db, None


def conv_transpose2x2_ok(m, dtype):
    """an nn.ConvTranspose2d the GEMM + depth-to-space form covers: kernel 2, stride 2, no padding, channels in whole 16-byte chunks."""
    ch = chunk_elems(dtype)
    return (m.kernel_size == (2, 2) and m.stride == (2, 2) and m.padding == (0, 0) and m.output_padding == (0, 0) and m.dilation == (1, 1) and m.groups == 1
            and m.in_channels % ch == 0 and m.out_channels % ch == 0)


def conv_transpose2x2(x, weight, bias):
    return _ConvTranspose2x2.apply(x, weight, bias, join_of(x))


# ---- detection loss + mask loss ------------------------------------------------------------------------------------------------------
class _DetectLossAssign(_DetectLoss):
    """_DetectLoss whose forward also returns the assignment's gt index per anchor [B, A] int32 (-1: background); the three loss sums, their
    gradients and the saved state are the detection criterion's own (one forward body: blocks._loss_forward)."""

    @staticmethod
    def forward(ctx, targets, strides, topk, alpha, beta, scale6, *maps):
        return _loss_forward(ctx, _DETECT_FAMILY, targets, strides, topk, alpha, beta, scale6, maps, assign=True)

    @staticmethod
    def backward(ctx, gl, _gitems, _ggidx):
        return _DetectLoss.backward(ctx, gl, _gitems)


def detect_loss_assign(box_maps, cls_maps, strides, targets, scale6, topk=10, alpha=0.5, beta=6.0):
    """-> (loss [3], items [3], gidx [B, A] int32): ops.detect_loss and the assignment it made."""
    return _DetectLossAssign.apply(targets, tuple(strides), topk, alpha, beta, scale6, *box_maps, *cls_maps)


class _MaskLoss(torch.autograd.Function):
    """(detection loss [3] scaled, coefficient maps, prototype map) -> (loss [4] = (box, seg, cls, dfl) scaled for backward, items [4] scaled
    for logging): the mask term of v8SegmentationLoss, and the criterion's two results from its last kernel.  The box / cls / dfl entries
    are copies of the detection loss's; their gradient goes back to it unchanged."""

    @staticmethod
    def forward(ctx, det_loss, det_items, gidx, targets, masks, scale6, topk, img_w, img_h, proto, *mc):
        dev = proto.device
        b = proto.shape[0]
        anchors = sum(int(t.shape[2] * t.shape[3]) for t in mc)
        g = int(targets.shape[1])
        if tuple(gidx.shape) != (b, anchors) or gidx.dtype != torch.int32 or not gidx.is_contiguous() or tuple(targets.shape) != (b, g, 5):
            raise ValueError(f"mask_loss: gidx {tuple(gidx.shape)} {gidx.dtype} / targets {tuple(targets.shape)} do not belong to {b} images of {anchors} anchors")
        sb = ctypes.c_size_t(0)
        check(L().ymi_mask_loss_sizes(b, anchors, g, int(topk), _byref(sb)), "mask_loss_sizes")
        state = torch.empty(sb.value, dtype=torch.uint8, device=dev)
        det6 = torch.cat([det_loss.detach().reshape(3), det_items.reshape(3)])  # the kernel reads the six numbers from one buffer
        out = torch.empty(8, dtype=torch.float32, device=dev)
        mf32 = int(masks.dtype == torch.float32)
        check(
            L().ymi_mask_loss_fwd(len(mc), _map_array(mc), _byref(as_ymi(proto)), ptr(masks), mf32, masks.shape[1], masks.shape[2], ptr(gidx), ptr(targets), g,
                                  int(topk), float(img_w), float(img_h), ptr(det6), ptr(scale6), ptr(out), ptr(state), state.numel(), stream_ptr()),
            "mask_loss_fwd",
        )
        ctx.save_for_backward(state, scale6, masks, proto, *mc)
        ctx.cfg = (g, int(topk), mf32)
        loss, items = out[:4], out[4:]
        ctx.mark_non_differentiable(items)
        ctx.set_materialize_grads(False)
        return loss, items

    @staticmethod
    def backward(ctx, gl, _gitems):
        state, scale6, masks, proto, *mc = ctx.saved_tensors
        nin = 10 + len(mc)
        if gl is None:
            return (None,) * nin
        g, topk, mf32 = ctx.cfg
        if gl.dtype != torch.float32 or not gl.is_contiguous():
            gl = gl.to(torch.float32).contiguous()
        dmc = [torch.zeros_like(t) for t in mc]  # (rows of background anchors stay zero)
        dproto = empty_nhwc(*proto.shape, proto.dtype, proto.device)
        out8 = torch.cat([gl, gl])  # (the kernel reads entry 1; a [4] gradient padded to the forward's [8] layout)
        check(
            L().ymi_mask_loss_bwd(len(mc), _map_array(mc), _byref(as_ymi(proto)), ptr(masks), mf32, masks.shape[1], masks.shape[2], g, topk, ptr(state),
                                  state.numel(), ptr(out8), ptr(scale6), _map_array(dmc), _byref(as_ymi(dproto)), stream_ptr()),
            "mask_loss_bwd",
        )
        gdet = torch.stack((gl[0], gl[2], gl[3]))
        return (gdet, None, None, None, None, None, None, None, None, dproto, *dmc)


def mask_loss(det_loss, det_items, gidx, targets, masks, scale6, topk, img_w, img_h, proto, mc_maps):
    """-> (loss [4] (differentiable), items [4] (detached)) in the reference's order box, seg, cls, dfl."""
    if proto.shape[1] != NM or any(t.shape[1] != NM for t in mc_maps):
        raise NotImplementedError(f"the mask-loss kernels are built for nm = {NM} prototypes, got {proto.shape[1]}")
    return _MaskLoss.apply(det_loss, det_items, gidx, targets, masks, scale6, int(topk), float(img_w), float(img_h), proto, *mc_maps)


def detect_decode_seg(box_maps, cls_maps, mc_maps, strides):
    """Segment's eval output cat([Detect._inference, mc], 1) -> [B, 4 + nc + nm, A] float32 in one launch (no gradient)."""
    return _decode(L().ymi_detect_decode_seg, "detect_decode_seg", box_maps, cls_maps, strides, mc_maps[0].shape[1], _map_array([t.detach() for t in mc_maps]))


# ---- mask decode and mask overlap (csrc/maskdec.hip) ---------------------------------------------------------------------------------
MASK_MAX_BINS = 256  # YMI_MASK_MAX_BINS


def _proto_map(proto, who):
    """the prototype map as the kernels take it: [B, nm, mh, mw] bfloat16 / float32 in NHWC memory (what Proto's eval output is; anything
    else is brought there)."""
    if proto.dim() != 4:
        raise ValueError(f"{who}: the prototype map is [B, nm, mh, mw], got {tuple(proto.shape)}")
    if proto.shape[1] != NM:
        raise NotImplementedError(f"{who}: the mask kernels are built for nm = {NM} prototypes, got {proto.shape[1]}")
    if not proto.is_cuda:
        raise RuntimeError("libyolo_mi355 kernels need tensors on the MI355X (cuda) device; there is no CPU path")
    proto = proto.detach()
    if proto.dtype not in (torch.float32, torch.bfloat16):
        proto = proto.float()
    if not is_nhwc(proto):
        proto = proto.contiguous(memory_format=torch.channels_last)
    return proto


def process_mask(proto, box, coef, img, shape, upsample=False):
    """process_mask of reference utils/ops.py:680-710 for rows of a whole batch, one launch (ymi_process_mask).  proto [B, 32, mh, mw]
    (Proto's eval output); box [N, 4] float32 in the pixels of the network input `shape` = (ih, iw); coef [N, 32]; img [N] int: the row's
    image (outside [0, B): a zero mask) -> (mask [N, mh, mw] (upsample=False) or [N, ih, iw] (upsample=True) uint8 0 / 1, area [N] int32: the
    mask's sum).  Nothing synchronises."""
    proto = _proto_map(proto, "process_mask")
    n = int(box.shape[0])
    ih, iw = int(shape[0]), int(shape[1])
    if box.dim() != 2 or box.shape[1] != 4 or tuple(coef.shape) != (n, NM) or int(img.numel()) != n:
        raise ValueError(f"process_mask: box {tuple(box.shape)}, coef {tuple(coef.shape)}, img {tuple(img.shape)} are not N rows of 4, {NM} and 1")
    dev = proto.device
    box = box.detach().to(dev, torch.float32).contiguous()
    coef = coef.detach().to(dev, torch.float32).contiguous()
    img = img.detach().to(dev).reshape(-1).to(torch.int32).contiguous()
    oh, ow = (ih, iw) if upsample else (int(proto.shape[2]), int(proto.shape[3]))
    mask = torch.empty((n, oh, ow), dtype=torch.uint8, device=dev)
    area = torch.empty((n,), dtype=torch.int32, device=dev)
    if n:
        check(L().ymi_process_mask(_byref(as_ymi(proto)), ptr(box), ptr(coef), ptr(img), n, ih, iw, int(bool(upsample)), ptr(mask), ptr(area), stream_ptr()),
              "process_mask")
    return mask, area


def mask_overlap(det, coef, count, proto, masks, shape, n_bins=MASK_MAX_BINS):
    """the integer counts mask_iou needs, for a batch, one launch and no mask stack (ymi_mask_overlap).  det [B, max_det, 6], coef
    [B, max_det, 32], count [B] as ops.detect_nms_seg leaves them (boxes in the pixels of the network input `shape` = (ih, iw)); proto
    [B, 32, mh, mw]; masks [B, mh, mw] uint8 or float32: the batch's overlap encoding (0 background, v: the image's v-th object)
    -> (inter [B, max_det, n_bins], area_pred [B, max_det], area_gt [B, n_bins]) int32 on the device.  An encoding of another size than the
    prototype map is refused (the reference would resample it)."""
    proto = _proto_map(proto, "mask_overlap")
    b, max_det = int(det.shape[0]), int(det.shape[1])
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous() or not det.is_cuda:
        raise ValueError(f"mask_overlap takes a contiguous float32 [B, max_det, 6] device tensor, got {tuple(det.shape)} {det.dtype}")
    if tuple(coef.shape) != (b, max_det, NM) or coef.dtype != torch.float32 or not coef.is_contiguous() or not coef.is_cuda:
        raise ValueError(f"mask_overlap: coef is a contiguous float32 [B, max_det, {NM}] device tensor, got {tuple(coef.shape)} {coef.dtype}")
    if count.dtype != torch.int32 or tuple(count.shape) != (b,) or not count.is_cuda or not count.is_contiguous():
        raise ValueError("mask_overlap: count is an int32 [B] tensor on the device")
    if masks.dim() != 3 or masks.shape[0] != b:
        raise ValueError(f"mask_overlap: the overlap encoding is [B, mh, mw], got {tuple(masks.shape)} for {b} images")
    if tuple(masks.shape[1:]) != tuple(proto.shape[2:]):
        raise NotImplementedError(f"mask_overlap: the overlap encoding is {tuple(masks.shape[1:])}, the prototype map {tuple(proto.shape[2:])}; "
                                  "resampling the encoding (reference segment/val.py:266-268) is not built")
    if not 1 <= int(n_bins) <= MASK_MAX_BINS:
        raise ValueError(f"mask_overlap: n_bins in [1, {MASK_MAX_BINS}], got {n_bins}")
    dev = det.device
    masks = masks.detach().to(dev)
    if masks.dtype not in (torch.uint8, torch.float32):
        masks = masks.float()
    masks = masks.contiguous()
    inter = torch.empty((b, max_det, int(n_bins)), dtype=torch.int32, device=dev)
    area_pred = torch.empty((b, max_det), dtype=torch.int32, device=dev)
    area_gt = torch.empty((b, int(n_bins)), dtype=torch.int32, device=dev)
    check(L().ymi_mask_overlap(ptr(det.detach()), ptr(coef.detach()), ptr(count), b, max_det, _byref(as_ymi(proto)), int(shape[0]), int(shape[1]), ptr(masks),
                               int(masks.dtype == torch.float32), masks.shape[1], masks.shape[2], int(n_bins), ptr(inter), ptr(area_pred), ptr(area_gt),
                               stream_ptr()), "mask_overlap")
    return inter, area_pred, area_gt
