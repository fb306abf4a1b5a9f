"""Bottleneck / C2f / SPPF / DFL / C3 family / PSA attention blocks (reference: ultralytics/nn/modules/block.py)."""
import torch
import torch.nn as nn

from ... import ops
from .conv import Conv, DWConv, GhostConv


class DFL(nn.Module):
    """expectation over the 16-bin box distribution (reference block.py:58-77); frozen weights 0..15.
    Inference-side decode on [B, 4*c1, A] tensors: tiny, stays in torch ops."""

    def __init__(self, c1=16):
        super().__init__()
        self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
        self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
        self.c1 = c1

    def forward(self, x):
        b, _, a = x.shape
        p = x.view(b, 4, self.c1, a).float().softmax(2)
        return (p * self.conv.weight.view(1, 1, self.c1, 1).float()).sum(2)


class Bottleneck(nn.Module):
    """x + cv2(cv1(x)) when shortcut and c1 == c2 (reference block.py:479-488); the add rides in
    cv2's BN/SiLU kernel."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2

    def forward(self, x, out=None):
        xi = ops.to_internal(x)
        # the shortcut rides in cv2's BatchNorm + SiLU kernel when cv1's operand IS the tensor to add.  A width that is not a
        # multiple of the 16-byte chunk reaches cv1 as a zero-padded copy (more channels than cv2 produces): the add is then a
        # separate launch on the caller's tensor and autograd forms the gradient sum
        fused_add = self.add and xi.shape[1] == self.cv2.conv.out_channels
        if fused_add and self.training and ops.join_of(xi) is None:
            ops.mark_join(xi, 2)  # consumers of x here: cv1 and the shortcut; their gradient sum forms in cv1's data-gradient epilogue
        h = self.cv1(xi)
        if fused_add or not self.add:
            return self.cv2(h, residual=xi if self.add else None, out=out)
        return ops.add_residual(self.cv2(h), x, out)


class C2f(nn.Module):
    """cv1 -> 2 chunks -> n chained Bottlenecks -> concat -> cv2 (reference block.py:279-304).
    The chunks are channel slices of cv1's NHWC output (no copy)."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    def forward(self, x, out=None):
        """out: optional ops.OutSlot for the block's result (a slice of a later Concat's buffer; train mode)."""
        x = ops.to_internal(x)
        buf, slot = None, (lambda j: None)
        dt = x.dtype
        dense = self.c % ops.chunk_elems(dt) == 0
        if self.training and hasattr(self.cv1, "bn") and dense:
            # train mode: cv1 and every Bottleneck write straight into their slice of the concat buffer
            n, _, h, w = x.shape
            buf = ops.empty_nhwc(n, (2 + len(self.m)) * self.c, h, w, dt, x.device)
            slot = lambda j: ops.OutSlot(buf, j * self.c)  # noqa: E731
        t, last = ops.c2f_split(self.cv1(x, out=slot(0)), self.c)  # (both chunks, second chunk): channel slices, no copy
        ys = [t]  # both chunks go into the concat at once: they are adjacent in memory
        first_join = None
        for j, m in enumerate(self.m):
            # consumers of a Bottleneck's input: its cv1, its shortcut (if any) and - for j >= 1, where the input is the
            # previous Bottleneck's output - the concat; the right half of t reaches the concat through c2f_split instead
            # Marked whenever the Bottleneck consumes `last` itself (a width in whole 16-byte chunks: to_internal is the identity),
            # with or without the concat buffer - ops.concat is a join-aware consumer either way.  Other widths reach the
            # Bottleneck as padded copies: autograd sums their gradients and nothing is marked.
            if dense:
                ops.mark_join(last, self._reads(m) + int(j >= 1), force=(j == 0))
                if j == 0:
                    first_join = ops.join_of(last)
            last = m(last, out=slot(2 + j))
            ys.append(last)
        # the concat's gradient for the right half of t and the first Bottleneck's input gradient are summed in the latter's epilogue
        return self.cv2(ops.concat(ys, buf, split_join=(first_join, self.c) if first_join is not None else None), out=out)

    forward_split = forward

    @staticmethod
    def _reads(m):
        """how many join-aware ops of member block m read its input: a Bottleneck's cv1 and, with a shortcut, cv2's residual."""
        return 1 + int(m.add)


class SPPF(nn.Module):
    """cv1 -> three chained k x k max-pools -> concat(4) -> cv2 (reference block.py:201-226); the
    pools and the concat are one LDS-staged kernel (csrc/pool.hip)."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)  # attribute kept for parity with the reference

    def forward(self, x, out=None):
        x = ops.to_internal(x)
        c_ = self.cv1.conv.out_channels
        cat = None
        if self.training and hasattr(self.cv1, "bn") and c_ % ops.chunk_elems(x.dtype) == 0:
            n, _, h, w = x.shape
            cat = ops.empty_nhwc(n, 4 * c_, h, w, x.dtype, x.device)  # cv1 writes y0 straight into slice 0 of the concat buffer
        y0 = self.cv1(x, out=ops.OutSlot(cat, 0) if cat is not None else None)
        return self.cv2(ops.sppf_pool_cat(y0, self.m.kernel_size, cat), out=out)


class C3(nn.Module):
    """cv3(cat(m(cv1(x)), cv2(x))) with n Bottlenecks of kernels (1, 1), (3, 3) (reference block.py:314-338).  In train mode the last
    Bottleneck and cv2 write their halves of the concat buffer."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0) for _ in range(n)))

    def forward(self, x, out=None):
        """out: optional ops.OutSlot for the block's result (train mode), handed to cv3."""
        x = ops.to_internal(x)
        c_ = self.cv2.conv.out_channels
        buf, slot = None, (lambda j: None)
        if self.training and hasattr(self.cv2, "bn") and c_ % ops.chunk_elems(x.dtype) == 0:
            n, _, h, w = x.shape
            buf = ops.empty_nhwc(n, 2 * c_, h, w, x.dtype, x.device)
            slot = lambda j: ops.OutSlot(buf, j * c_)  # noqa: E731
        a = self.cv1(x)
        for j, m in enumerate(self.m):
            # (a Bottleneck takes an output slot; a GhostBottleneck's sum is its own launch and reaches the buffer through the concat's copy)
            a = m(a, out=slot(0)) if (isinstance(m, Bottleneck) and j == len(self.m) - 1) else m(a)
        b = self.cv2(x, out=slot(1))
        return self.cv3(ops.concat([a, b], buf), out=out)


class GhostBottleneck(nn.Module):
    """conv(x) + shortcut(x): GhostConv -> (stride 2: depthwise) -> GhostConv without activation, beside an identity or a depthwise +
    pointwise shortcut (reference block.py:426-452)."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(
            GhostConv(c1, c_, 1, 1),
            DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
            GhostConv(c_, c2, 1, 1, act=False),
        )
        self.shortcut = nn.Sequential(DWConv(c1, c1, k, s, act=False), Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()

    def forward(self, x):
        x = ops.to_internal(x)
        return ops.add_residual(self.conv(x), self.shortcut(x))


class C3Ghost(C3):
    """C3 with GhostBottlenecks (reference block.py:406-423)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(GhostBottleneck(c_, c_) for _ in range(n)))


class C3k(C3):
    """C3 whose n Bottlenecks have two k x k kernels (reference block.py:1110-1129)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, k=3):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=(k, k), e=1.0) for _ in range(n)))


class C3k2(C2f):
    """C2f whose members are C3k(c, c, 2) blocks (c3k) or plain Bottlenecks with the default e = 0.5 (reference block.py:1088-1107)."""

    def __init__(self, c1, c2, n=1, c3k=False, e=0.5, g=1, shortcut=True):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(C3k(self.c, self.c, 2, shortcut, g) if c3k else Bottleneck(self.c, self.c, shortcut, g) for _ in range(n))

    @staticmethod
    def _reads(m):
        """a C3k reads its input with cv1 and cv2 and has no shortcut of its own."""
        return 2 if isinstance(m, C3k) else 1 + int(m.add)


class Attention(nn.Module):
    """full-map self-attention with keys narrower than values and a depthwise positional term (reference block.py:1278-1338):
    proj(attention(qkv(x)) + pe(v)).  qkv's output is packed per head as [q (key_dim) | k (key_dim) | v (head_dim)]; the attention core is
    ops.psa_attention on the NHWC tensor's pixels as tokens, which also returns v compacted for `pe`; the sum rides in pe's kernel."""

    def __init__(self, dim, num_heads=8, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim**-0.5
        nh_kd = self.key_dim * num_heads
        h = dim + nh_kd * 2
        self.qkv = Conv(dim, h, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

    def forward(self, x, residual=None, out=None):
        """residual: added to the result in proj's kernel (PSABlock's shortcut); out: optional ops.OutSlot (train mode)."""
        x = ops.to_internal(x)
        h, w = x.shape[2:]
        o, v = ops.psa_attention(self.qkv(x), h * w, self.num_heads, self.key_dim)
        y = self.pe(v, residual=o)
        return self.proj(y, residual=residual, out=out)


class PSABlock(nn.Module):
    """x + attn(x), then + ffn of that (reference block.py:1341-1391); both shortcuts ride as residuals of the last convolution of their branch."""

    def __init__(self, c, attn_ratio=0.5, num_heads=4, shortcut=True):
        super().__init__()
        self.attn = Attention(c, attn_ratio=attn_ratio, num_heads=num_heads)
        self.ffn = nn.Sequential(Conv(c, c * 2, 1), Conv(c * 2, c, 1, act=False))
        self.add = shortcut

    def forward(self, x, out=None):
        x = ops.to_internal(x)
        return _psa_body(self.attn, self.ffn, x, self.add, self.training, out)


def _psa_body(attn, ffn, x, add, training, out=None):
    """the two residual branches PSABlock and PSA share.  A tensor read by a convolution and by a shortcut has two join-aware consumers: its
    gradient sum forms in the convolution's data-gradient epilogue.  A caller that already attached a join to x has counted both."""
    if add and training and ops.join_of(x) is None:
        ops.mark_join(x, 2)  # attn.qkv and the shortcut (proj's residual)
    y = attn(x, residual=x if add else None)
    if add and training:
        ops.mark_join(y, 2)  # ffn[0] and the shortcut (ffn[1]'s residual)
    h = ffn[0](y)
    return ffn[1](h, residual=y if add else None, out=out)


def _split_for_psa(t, c, twice):
    """(a, b) = channel halves of cv1's output; b is read by the first attention block - twice when that block has a shortcut."""
    a, b = ops.chan_split2(t, c)
    j = ops.join_of(b)
    if j is not None and twice:
        j.n = 2
    return a, b


class PSA(nn.Module):
    """cv2(cat(a, b + attn(b) + ffn(..))) on the halves of cv1's output (reference block.py:1394-1449)."""

    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.attn = Attention(self.c, attn_ratio=0.5, num_heads=self.c // 64)
        self.ffn = nn.Sequential(Conv(self.c, self.c * 2, 1), Conv(self.c * 2, self.c, 1, act=False))

    def forward(self, x, out=None):
        x = ops.to_internal(x)
        a, b = _split_for_psa(self.cv1(x), self.c, self.training)
        b = _psa_body(self.attn, self.ffn, b, True, self.training)
        y = ops.concat([a, b])
        return self.cv2(y, out=out)


class C2PSA(nn.Module):
    """PSA refactored to stack n PSABlocks on the second half of cv1's output (reference block.py:1452-1507)."""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, attn_ratio=0.5, num_heads=self.c // 64) for _ in range(n)))

    def forward(self, x, out=None):
        x = ops.to_internal(x)
        a, b = _split_for_psa(self.cv1(x), self.c, self.training and len(self.m) > 0 and self.m[0].add)
        for m in self.m:
            b = m(b)
        y = ops.concat([a, b])
        return self.cv2(y, out=out)


class _Up2x2(nn.ConvTranspose2d):
    """Proto's transposed convolution: an nn.ConvTranspose2d (same state-dict keys, weight [c1, c2, 2, 2]) whose forward is the MFMA 1x1 GEMM
    with the weight viewed as [4 * c2, c1], followed by the depth-to-space kernel (ops.conv_transpose2x2)."""

    def forward(self, x):
        x = ops.to_internal(x)
        if not ops.conv_transpose2x2_ok(self, x.dtype):
            raise NotImplementedError(f"ConvTranspose2d({self.in_channels}, {self.out_channels}, {self.kernel_size}, {self.stride}) in {x.dtype}: built for "
                                      f"kernel 2, stride 2, no padding and channel counts in whole 16-byte chunks (multiples of {ops.chunk_elems(x.dtype)})")
        return ops.conv_transpose2x2(x, self.weight, self.bias)


class Proto(nn.Module):
    """mask prototypes: Conv 3x3 -> ConvTranspose2d 2x2 stride 2 -> Conv 3x3 -> Conv 1x1 (reference block.py:80-100)."""

    def __init__(self, c1, c_=256, c2=32):
        super().__init__()
        self.cv1 = Conv(c1, c_, k=3)
        self.upsample = _Up2x2(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = Conv(c_, c_, k=3)
        self.cv3 = Conv(c_, c2)

    def forward(self, x):
        return self.cv3(self.cv2(self.upsample(self.cv1(x))))
