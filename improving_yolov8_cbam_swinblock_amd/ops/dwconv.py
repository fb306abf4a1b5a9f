"""Depthwise Conv blocks (groups == cin == cout) as autograd Functions over csrc/dwconv.hip: train-mode conv + BatchNorm + activation, the
eval / fused affine form, and GhostConv's tail, which writes beside its input in one buffer and forms that input's gradient sum in the
data-gradient kernel (reference: nn/modules/conv.py:37-91 with g = c1 = c2, :194-209 DWConv, :329-371 GhostConv).

The weight stays the module's [C, 1, k, k] float32 tensor: no packed operand, no arena entry.  Weight gradients are complete when backward
returns (never deferred, never on the rider schedule): they are small streaming launches."""
import torch

from .._lib import ACT_NONE, ACT_SILU, as_ymi, check, chunk_elems, empty_nhwc, ptr, stream_ptr, workspace
from .base import L, _byref, _conv_out_hw, _count_batch, _dense_ok, _join_plain, _note_use, grad_nhwc, join_of
from .conv import _bn_act_bwd
from .weights import _new_dw


def _check_dw(x, weight, k, what):
    c = x.shape[1]
    if tuple(weight.shape) != (c, 1, k, k):
        raise RuntimeError(f"{what}: weight {tuple(weight.shape)} is not the depthwise [{c}, 1, {k}, {k}] of a {c}-channel input")
    ch = chunk_elems(x.dtype)
    if c % ch != 0:
        raise NotImplementedError(f"{what}: a depthwise convolution over {c} channels in {x.dtype}: the kernels read channels in whole 16-byte chunks "
                                  f"(multiples of {ch}) - use float32 for this width")
    if not _dense_ok(x, x.dtype):
        raise RuntimeError(f"{what}: input must be an internal NHWC tensor (ops.to_internal)")


def _dw_dgrad(draw, weight, k, stride, in_shape, add=None):
    """dx = depthwise data gradient (+ add) -> a new NHWC tensor of in_shape."""
    dx = empty_nhwc(*in_shape, draw.dtype, draw.device)
    check(L().ymi_dwconv2d_bwd_data(_byref(as_ymi(draw)), ptr(weight.detach()), k, stride, _byref(as_ymi(add)) if add is not None else None,
                                    _byref(as_ymi(dx)), stream_ptr()), "dwconv2d_bwd_data")
    return dx


def _dw_wgrad(x, draw, k, stride, weight):
    """dw [C, 1, k, k] float32, complete when the call returns control of the stream (ordered two-level sum); written straight into the
    parameter's gradient bucket inside ops.grad_arena."""
    n, c, ho, wo = draw.shape
    dw = _new_dw(c, 1, k, x.device, (weight,), None)
    ws = workspace(int(L().ymi_dwconv2d_bwd_weight_workspace(n, ho, wo, c, k)), x.device, "dwwgrad")
    check(L().ymi_dwconv2d_bwd_weight(_byref(as_ymi(x)), _byref(as_ymi(draw)), k, stride, ptr(dw), ptr(ws), ws.numel(), stream_ptr()), "dwconv2d_bwd_weight")
    return dw


class _DwConvBnAct(torch.autograd.Function):
    """act(BatchNorm_train(depthwise conv(x))) (+ residual).  cat: GhostConv's form (conv.py:370-371) - x IS channels [0, C) of the buffer whose
    channels [C, 2C) `slot` names; the result is the 2C-channel tensor [x | block(x)] (no copy), and backward adds the gradient of the left
    half to x's data gradient inside the data-gradient kernel."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, k, stride, eps, momentum, act, residual, slot, cat, join=None, res_join=None):
        dtype, dev = x.dtype, x.device
        n, c, h, w = x.shape
        ho, wo = _conv_out_hw(h, w, k, stride)
        _note_use(weight)
        raw = empty_nhwc(n, c, ho, wo, dtype, dev)
        out = slot.view(n, c, ho, wo, dtype) if slot is not None else empty_nhwc(n, c, ho, wo, dtype, dev)
        stats = torch.empty((2, c), dtype=torch.float32, device=dev)
        need = (int(L().ymi_dwconv2d_stat_blocks(n, ho, wo, c)) * 2 * c + 2 * c) * 4
        ws = workspace(need, dev, "conv")
        check(
            L().ymi_dwconv2d_bn_act_fwd(
                _byref(as_ymi(x)), ptr(weight.detach()), k, stride, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), momentum, eps, act,
                _byref(as_ymi(residual)) if residual is not None else None, _byref(as_ymi(raw)), _byref(as_ymi(out)), ptr(stats[0]), ptr(stats[1]),
                ptr(ws), ws.numel(), stream_ptr(),
            ),
            "dwconv2d_bn_act_fwd",
        )
        ctx.save_for_backward(x, weight, gamma, beta, raw, stats)
        ctx.cfg = (k, stride, act, residual is not None, cat)
        ctx.joins = (join, res_join)
        if cat:
            buf = slot.buf
            if stride != 1 or slot.off != c or x.data_ptr() != buf[:, :c].data_ptr() or x.stride() != buf[:, :c].stride():
                raise RuntimeError("_DwConvBnAct(cat): x must be channels [0, C) of the buffer whose channels [C, 2C) the block writes")
            return buf[:, : 2 * c]
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, gamma, beta, raw, stats = ctx.saved_tensors
        k, stride, act, has_res, cat = ctx.cfg
        dtype = x.dtype
        c = x.shape[1]
        dout = grad_nhwc(dout, dtype)
        dleft = None
        if cat:
            dleft, dout = dout[:, :c], dout[:, c:]
        draw, dgamma, dbeta = _bn_act_bwd(dout, raw, stats, act, gamma, beta)
        # tensors with several consumers (GradJoin): every consumer arrives at the join - the residual hand-through first, so that when x is both
        # input and residual the data gradient is the later arrival - and the last one returns the total (sums by accumulate launches here)
        join, res_join = ctx.joins
        dres = _join_plain(res_join, dout) if (has_res and ctx.needs_input_grad[11]) else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _join_plain(join, _dw_dgrad(draw, weight, k, stride, x.shape, dleft))
        dw = _dw_wgrad(x, draw, k, stride, weight) if ctx.needs_input_grad[1] else None  # (a frozen weight: no launch)
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None, None, dres, None, None, None, None


def dwconv_bn_act(x, weight, bn, k, stride, act=ACT_SILU, residual=None, slot=None, cat=False):
    """train-mode depthwise Conv block on an internal (NHWC) tensor; updates bn.running_* in place.  slot: optional OutSlot.
    cat (with slot): GhostConv's tail, see _DwConvBnAct."""
    if bn.momentum is None:
        raise RuntimeError("BatchNorm with cumulative moving average (momentum=None) is not supported")
    _check_dw(x, weight, k, "dwconv_bn_act")
    out = _DwConvBnAct.apply(x, weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, int(k), int(stride), float(bn.eps), float(bn.momentum), int(act),
                             residual, slot, bool(cat), join_of(x), join_of(residual) if residual is not None else None)
    _count_batch(bn)
    return out


class _DwConvAffineAct(torch.autograd.Function):
    """y = act(scale * depthwise conv(x) + bias) (+ residual), one kernel: eval-mode blocks (BatchNorm folded into scale / bias) and fused
    modules (conv.py:81-91).  Differentiable as _ConvAffineAct is: without activation, scale and trainable bias."""

    @staticmethod
    def forward(ctx, x, weight, scale, bias, k, stride, act, residual, join=None, res_join=None):
        n, c, h, w = x.shape
        ho, wo = _conv_out_hw(h, w, k, stride)
        _note_use(weight)
        y = empty_nhwc(n, c, ho, wo, x.dtype, x.device)
        check(L().ymi_dwconv2d_fwd(_byref(as_ymi(x)), ptr(weight.detach()), k, stride, ptr(scale), ptr(bias), act,
                                   _byref(as_ymi(residual)) if residual is not None else None, _byref(as_ymi(y)), None, None, stream_ptr()), "dwconv2d_fwd")
        ctx.unsupported = None
        if act != ACT_NONE or scale is not None or (bias is not None and bias.requires_grad):
            ctx.unsupported = "backward through a fused activation / BN-folded depthwise conv is not implemented (use train mode or act=none)"
        ctx.save_for_backward(x, weight)
        ctx.cfg = (k, stride, residual is not None)
        ctx.joins = (join, res_join)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.unsupported:
            raise NotImplementedError(ctx.unsupported)
        x, weight = ctx.saved_tensors
        k, stride, has_res = ctx.cfg
        dy = grad_nhwc(dy, x.dtype)
        join, res_join = ctx.joins  # (as _DwConvBnAct.backward: the residual arrives first, the last arrival returns the total)
        dres = _join_plain(res_join, dy) if (has_res and ctx.needs_input_grad[7]) else None
        dx = _join_plain(join, _dw_dgrad(dy, weight, k, stride, x.shape)) if ctx.needs_input_grad[0] else None
        dw = _dw_wgrad(x, dy, k, stride, weight) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None, None, None, dres, None, None


def dwconv_affine_act(x, weight, scale, bias, k, stride, act=ACT_NONE, residual=None):
    _check_dw(x, weight, k, "dwconv_affine_act")
    return _DwConvAffineAct.apply(x, weight, scale, bias, int(k), int(stride), int(act), residual, join_of(x), join_of(residual) if residual is not None else None)
