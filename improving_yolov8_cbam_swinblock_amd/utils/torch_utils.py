"""step-path utilities with the reference's names (ultralytics/utils/torch_utils.py)."""
import math

import torch
import torch.nn as nn


def initialize_weights(model):
    """BN eps / momentum and in-place activations as the reference sets them (torch_utils.py:462-472)."""
    for m in model.modules():
        t = type(m)
        if t is nn.BatchNorm2d:
            m.eps = 1e-3
            m.momentum = 0.03
        elif t in {nn.Hardswish, nn.LeakyReLU, nn.ReLU, nn.ReLU6, nn.SiLU}:
            m.inplace = True


def fuse_conv_and_bn(conv, bn):
    """fold BN running statistics into a biased conv (reference torch_utils.py:240-271)."""
    fused = (
        nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups, bias=True)
        .requires_grad_(False)
        .to(conv.weight.device)
    )
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    fused.weight.copy_(conv.weight * scale.view(-1, 1, 1, 1))
    b0 = torch.zeros_like(bn.running_mean) if conv.bias is None else conv.bias
    fused.bias.copy_((b0 - bn.running_mean) * scale + bn.bias)
    return fused


def scale_img(img, ratio=1.0, same_shape=False, gs=32):
    """reference torch_utils.py:475-495: the image batch resized bilinearly to (int(h * ratio), int(w * ratio)) and padded right and below
    with 0.447 to the next multiple of gs of (h * ratio, w * ratio) - or, same_shape=True, back to (h, w).  ratio == 1.0 returns img itself.
    One launch of ops.scale_image (resize and padding in one pass); uint8 images are converted to float / 255 in it as well."""
    if ratio == 1.0:
        return img
    from .. import ops

    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    if not same_shape:
        h, w = (math.ceil(x * ratio / gs) * gs for x in (h, w))
    return ops.scale_image(img, s, (h, w), pad_value=0.447)


def intersect_dicts(da, db, exclude=()):
    """reference torch_utils.py: keys of da present in db with equal shapes."""
    return {k: v for k, v in da.items() if k in db and all(x not in k for x in exclude) and v.shape == db[k].shape}
