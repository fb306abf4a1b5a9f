"""CPU restatements for the segmentation tests, in the dtype of their inputs (float64-capable): Proto with its transposed convolution written as
the 1x1 GEMM + depth-to-space the kernels run, and the mask term of v8SegmentationLoss in batched form.  TEST INFRASTRUCTURE ONLY: it states
the mathematics of reference nn/modules/block.py:80-100, utils/loss.py:349-438 and utils/ops.py:661-677 independently of both the reference's
program text and the kernels'."""
import torch
import torch.nn.functional as F


def depth_to_space2(deep):
    """[N, 4C, H, W] with channel (2a + b) * C + c -> [N, C, 2H, 2W] at (2y + a, 2x + b)."""
    n, c4, h, w = deep.shape
    c = c4 // 4
    return deep.view(n, 2, 2, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, 2 * h, 2 * w)


def space_to_depth2(wide):
    n, c, h2, w2 = wide.shape
    return wide.view(n, c, h2 // 2, 2, w2 // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(n, 4 * c, h2 // 2, w2 // 2)


def conv_transpose2x2(x, weight, bias):
    """nn.ConvTranspose2d(c1, c2, 2, 2, 0) as four 1x1 GEMMs: weight [c1, c2, 2, 2] viewed as [4 * c2, c1], bias repeated."""
    c1, c2 = weight.shape[:2]
    wg = weight.permute(2, 3, 1, 0).reshape(4 * c2, c1, 1, 1)
    return depth_to_space2(F.conv2d(x, wg, bias.repeat(4) if bias is not None else None))


def conv_bn_silu(x, w, gamma, beta, eps=1e-3):
    """train-mode Conv block: convolution with 'same' padding, BatchNorm on the batch statistics, SiLU."""
    y = F.conv2d(x, w, None, 1, w.shape[-1] // 2)
    mean = y.mean((0, 2, 3), keepdim=True)
    var = y.var((0, 2, 3), unbiased=False, keepdim=True)
    y = (y - mean) / torch.sqrt(var + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return y * torch.sigmoid(y)


def proto_forward(x, sd):
    """Proto in train mode from its state dict (tensors of x's dtype)."""
    y = conv_bn_silu(x, sd["cv1.conv.weight"], sd["cv1.bn.weight"], sd["cv1.bn.bias"])
    y = conv_transpose2x2(y, sd["upsample.weight"], sd["upsample.bias"])
    y = conv_bn_silu(y, sd["cv2.conv.weight"], sd["cv2.bn.weight"], sd["cv2.bn.bias"])
    return conv_bn_silu(y, sd["cv3.conv.weight"], sd["cv3.bn.weight"], sd["cv3.bn.bias"])


def dense_targets(batch, B, img_hw):
    """[B, G, 4] xyxy pixels of the labels in row order (zeros in unused slots)."""
    bi = batch["batch_idx"].reshape(-1).long()
    G = max(1, int(torch.bincount(bi, minlength=B).max()) if bi.numel() else 1)
    out = torch.zeros(B, G, 4, dtype=torch.float64)
    h, w = img_hw
    for b in range(B):
        rows = batch["bboxes"].reshape(-1, 4)[bi == b].double()
        for k, (cx, cy, bw, bh) in enumerate(rows.tolist()):
            out[b, k] = torch.tensor([(cx - bw / 2) * w, (cy - bh / 2) * h, (cx + bw / 2) * w, (cy + bh / 2) * h], dtype=torch.float64)
    return out


def nearest_masks(masks, mh, mw):
    """the overlap masks read at (mh, mw) with F.interpolate(mode="nearest")'s index rule: source = min(floor(dst * in / out), in - 1)."""
    B, H, W = masks.shape
    if (H, W) == (mh, mw):
        return masks
    ys = torch.clamp(torch.floor(torch.arange(mh, dtype=torch.float32) * (torch.tensor(H, dtype=torch.float32) / mh)).long(), max=H - 1)
    xs = torch.clamp(torch.floor(torch.arange(mw, dtype=torch.float32) * (torch.tensor(W, dtype=torch.float32) / mw)).long(), max=W - 1)
    return masks[:, ys][:, :, xs]


def mask_loss(mc, proto, gidx, boxes, masks, img_hw):
    """the mask term, batched.  mc [B, nm, A], proto [B, nm, mh, mw] (their dtype is the arithmetic's), gidx [B, A] gt index or -1,
    boxes [B, G, 4] xyxy pixels, masks [B, H, W] overlap encoding -> scalar: sum over foreground anchors of
    mean_over_all_pixels(BCE(logit, gt) * inside_box) / normalised box area, divided by the number of foreground anchors (0 without any)."""
    dt = proto.dtype
    B, nm, mh, mw = proto.shape
    fg = gidx >= 0
    n = int(fg.sum())
    if n == 0:
        return (proto * 0).sum() + (mc * 0).sum()
    masks = nearest_masks(masks.float(), mh, mw)
    h, w = img_hw
    scale = torch.tensor([w, h, w, h], dtype=dt)
    r = torch.arange(mw, dtype=dt).view(1, 1, mw)
    c = torch.arange(mh, dtype=dt).view(1, mh, 1)
    total = proto.new_zeros(())
    for b in range(B):
        idx = fg[b].nonzero().reshape(-1)
        if idx.numel() == 0:
            continue
        k = gidx[b, idx].long()
        norm = boxes[b, k].to(dt) / scale
        area = (norm[:, 2] - norm[:, 0]) * (norm[:, 3] - norm[:, 1])
        mx = norm * torch.tensor([mw, mh, mw, mh], dtype=dt)
        logit = torch.einsum("kn,khw->nhw", mc[b][:, idx], proto[b])
        gt = (masks[b][None] == (k + 1).view(-1, 1, 1).float()).to(dt)
        bce = logit.clamp(min=0) - logit * gt + torch.log1p(torch.exp(-logit.abs()))
        x1, y1, x2, y2 = (mx[:, i].view(-1, 1, 1) for i in range(4))
        crop = ((r >= x1) & (r < x2) & (c >= y1) & (c < y2)).to(dt)
        total = total + ((bce * crop).mean((1, 2)) / area).sum()
    return total / n
