"""Float64 restatement, in plain torch, of the PSA attention core on its packed layout and of the reference's block.py Attention module around
it (train mode).  It pins what the kernels and the module must agree on: qkv rows hold, per head, [q (kd) | k (kd) | v (hd)]; scores are scaled
by kd^-0.5; the softmax runs over the keys of the token's own image; v_out is the V columns compacted to [T, heads * hd].  Gradients come from
autograd on these functions."""
import torch
import torch.nn.functional as F


def split_packed(qkv, L, heads, kd):
    """[T, heads * (2 kd + hd)] token rows (images of L consecutive tokens) -> q, k [images, heads, L, kd], v [images, heads, L, hd]."""
    T, C3 = qkv.shape
    per = C3 // heads
    hd = per - 2 * kd
    assert per * heads == C3 and hd > 0 and T % L == 0, (qkv.shape, L, heads, kd)
    x = qkv.reshape(T // L, L, heads, per).permute(0, 2, 1, 3)
    return x[..., :kd], x[..., kd : 2 * kd], x[..., 2 * kd :]


def pack(q, k, v):
    """inverse of split_packed -> [T, heads * (2 kd + hd)]."""
    x = torch.cat([q, k, v], -1)  # [images, heads, L, per]
    b, h, L, per = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * L, h * per)


def tokens_of(x):
    """[images, heads, L, d] -> [T, heads * d]."""
    b, h, L, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b * L, h * d)


def psa_attention_ref(qkv, L, heads, kd):
    """-> (out, v_out), both [T, heads * hd], in qkv's dtype (use float64)."""
    q, k, v = split_packed(qkv, L, heads, kd)
    p = torch.softmax((q @ k.transpose(-1, -2)) * kd ** -0.5, -1)
    return tokens_of(p @ v), tokens_of(v)


def conv_bn_train(x, w, gamma, beta, eps, groups=1):
    """bias-free convolution with 'same' padding -> BatchNorm on batch statistics (NCHW)."""
    y = F.conv2d(x, w, None, 1, w.shape[-1] // 2, 1, groups)
    mean, var = y.mean((0, 2, 3), keepdim=True), y.var((0, 2, 3), unbiased=False, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


def attention_module_ref(p, x, heads, kd, eps=1e-3):
    """train-mode forward of Attention(dim, heads, .) on NCHW x from the parameter dict p (state-dict names -> float64 tensors):
    proj(attention(qkv(x)) + pe(v)), every Conv block without activation."""
    b, c, h, w = x.shape
    qkv = conv_bn_train(x, p["qkv.conv.weight"], p["qkv.bn.weight"], p["qkv.bn.bias"], eps)
    tok = qkv.permute(0, 2, 3, 1).reshape(b * h * w, -1)  # NHWC pixels as tokens
    o, v = psa_attention_ref(tok, h * w, heads, kd)
    to_map = lambda t: t.reshape(b, h, w, c).permute(0, 3, 1, 2)  # noqa: E731
    y = to_map(o) + conv_bn_train(to_map(v), p["pe.conv.weight"], p["pe.bn.weight"], p["pe.bn.bias"], eps, groups=c)
    return conv_bn_train(y, p["proj.conv.weight"], p["proj.bn.weight"], p["proj.bn.bias"], eps)
