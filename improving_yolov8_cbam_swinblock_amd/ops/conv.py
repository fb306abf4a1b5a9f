"""Convolution blocks as autograd Functions over the C ABI: data-gradient helpers (joined sums, multi-problem launches), Conv + BatchNorm + SiLU,
the direct first layer, Detect's sibling pairs and its lockstep training path, biased convolutions / linears (reference: nn/modules/conv.py:37-91,
nn/modules/head.py:36-76)."""
import ctypes
from collections import namedtuple
from dataclasses import make_dataclass

import torch

from .. import _lib
from .._lib import ACT_NONE, ACT_SILU, ConvProblem, DgradProblem, as_ymi, check, chunk_elems, empty_nhwc, is_nhwc, ptr, stream_ptr, workspace
from .base import (
    HOOKS, RUN, L, _GradBuffer, _GradSlot, _accumulate, _as4d, _byref, _conv_out_hw, _count_batch, _deferred_twice, _dense_ok, _in_backward,
    _join_plain, _note_use, _prep_adds, _stat_acc, compute_dtype, grad_nhwc, join_of, mark_join, round_up,
)
from .weights import (
    _adoptable, _defer_wgrad, _new_dw, _wgrad_maybe_async, pack_conv_dgrad, pack_conv_dgrad_pair, pack_conv_fwd, pack_conv_fwd_pair,
)

# One data-gradient GEMM, prepared (_dgrad_prepare) and not yet launched: dy and its descriptor ty, the packed operand wd, cin / k / stride, the
# addends of the GEMM's epilogue (fused: at most two) and those beyond them (rest: accumulate launches after the GEMM), the result dx that is
# handed out (input channels zero-padded) and dxv = dx[:, :cin], which the kernel writes.
DgradJob = namedtuple("DgradJob", "dy ty wd cin k stride fused rest dx dxv")
# One stride-1 convolution of _conv_fwd_multi: input, packed forward operand, output width, kernel size, output; optionally a bias, or its
# statistics rows (part / pstride / poff: see ymi_conv_problem).  blocks: the statistics rows written, filled in by _conv_fwd_multi.
FwdProblem = make_dataclass("FwdProblem", ["x", "wp", "cout", "k", "y", ("bias", object, None), ("part", object, None), ("pstride", int, 0), ("poff", int, 0),
                                           ("blocks", int, 0)])


def _dgrad_prepare(dy, weight4, k, stride, in_shape, dtype, adds=None, out=None, packed=None):
    """the arguments of one data-gradient GEMM (see _dgrad) -> DgradJob; _dgrad_finish completes it after the launch.
    in_shape: [N, C_in(padded), H, W], or [T, C_in] of a token matrix (k = 1, stride 1)."""
    shape = tuple(in_shape)
    cp = shape[1]
    ty = as_ymi(dy)
    if packed is not None:
        wd, cin = packed
    else:
        cin = weight4.shape[1]
        wd = pack_conv_dgrad(weight4, ty.c, stride, dtype)
    dx = out if (out is not None and tuple(out.shape) == shape and cp == cin) else None
    if dx is None:
        dx = empty_nhwc(*shape, dtype, dy.device) if len(shape) == 4 else torch.empty(shape, dtype=dtype, device=dy.device)
    dxv = dx
    if cp != cin:
        dx.zero_()
        dxv = dx[:, :cin]
    adds = _prep_adds(adds, dtype)
    sparse = k == 1 and stride > 1  # pixels between the strides receive no gradient: the kernel leaves them as prepared here (zeros)
    if sparse and cp == cin:
        dx.zero_()  # (_dgrad_joined never passes an in-place `out` in this case)
    fused = adds[:2] if (cp == cin and not sparse) else []
    return DgradJob(dy, ty, wd, cin, k, stride, fused, adds[len(fused):], dx, dxv)


def _dgrad_finish(job):
    if job.rest:
        _accumulate(job.dxv, job.rest)
    return job.dx


def _dgrad(dy, weight4, k, stride, in_shape, dtype, adds=None, out=None, packed=None):
    """dx [N, C_in(padded), H, W] (NHWC) from dy and the OIHW weight (+ up to two addends summed in the GEMM's
    epilogue, further ones by accumulate launches); zero-padded input channels get zero.  out: write the result into this
    NHWC view (it may be one of the addends: the epilogue reads an addend before it stores the sum).
    packed: (operand, cin) of an already packed data-gradient operand (weight4 is then unused)."""
    return _dgrad_launch(_dgrad_prepare(dy, weight4, k, stride, in_shape, dtype, adds, out, packed))


def _dgrad_launch(j):
    a1 = _byref(as_ymi(j.fused[0])) if len(j.fused) > 0 else None
    a2 = _byref(as_ymi(j.fused[1])) if len(j.fused) > 1 else None
    check(L().ymi_conv2d_bwd_data_add(_byref(j.ty), ptr(j.wd), j.cin, j.k, j.k, j.stride, a1, a2, _byref(as_ymi(j.dxv)), stream_ptr()), "conv2d_bwd_data")
    return _dgrad_finish(j)


def _width_class(c, dtype):
    """problems of one multi-problem GEMM launch must agree on this (the K-step form of the kernel: csrc/igemm.hip launch_igemm_n)."""
    cpt = int(c) // chunk_elems(dtype)
    return (cpt % 4 == 0, cpt % 8 == 0)


def _launch_grouped(items, key, struct, fill, entry, what):
    """one launch of a multi-problem entry point per group of items of equal key(item), at most 8 problems a launch.  fill(q, item) sets
    the ctypes record q and returns what q points to (kept alive until the call returns).  -> [(item, q)] of everything launched."""
    groups = {}
    for it in items:
        groups.setdefault(key(it), []).append(it)
    done = []
    for g in groups.values():
        for s in range(0, len(g), 8):
            chunk = g[s : s + 8]
            arr = (struct * len(chunk))()
            keep = [fill(q, it) for q, it in zip(arr, chunk)]  # noqa: F841 (alive across the call)
            check(entry(arr, len(chunk), stream_ptr()), what)
            done += zip(chunk, arr)
    return done


def _fill_dgrad(q, j):
    ts = [j.ty, as_ymi(j.dxv)] + [as_ymi(a) for a in j.fused]
    for name, t in zip(("dy", "dx", "add1", "add2"), ts):
        setattr(q, name, ctypes.pointer(t))
    q.w_dgrad_packed, q.cin, q.k = j.wd.data_ptr(), j.cin, j.k
    return ts


def _fill_fwd(q, p):
    ts = [as_ymi(p.x), as_ymi(p.y)]
    q.x, q.y = ctypes.pointer(ts[0]), ctypes.pointer(ts[1])
    q.w_packed, q.cout, q.kh, q.kw, q.stride, q.act = p.wp.data_ptr(), p.cout, p.k, p.k, 1, ACT_NONE
    if p.bias is not None:
        q.bias = p.bias.data_ptr()
    if p.part is not None:
        q.stat_partials, q.stat_stride, q.stat_offset = p.part.data_ptr(), p.pstride, p.poff
    return ts


def _dgrad_multi(jobs, dtype):
    """the stride-1 data-gradient GEMMs of several INDEPENDENT convolutions (jobs of _dgrad_prepare), one launch per width class."""
    if any(j.stride != 1 for j in jobs):
        raise RuntimeError("_dgrad_multi: stride 1 only")
    _launch_grouped(jobs, lambda j: _width_class(j.ty.c, dtype), DgradProblem, _fill_dgrad, L().ymi_conv2d_bwd_data_multi, "conv2d_bwd_data_multi")
    return [_dgrad_finish(j) for j in jobs]


def _conv_fwd_multi(problems, dtype):
    """several INDEPENDENT stride-1 convolutions (FwdProblem), one launch per width class and statistics mode; fills in their `blocks`."""
    for p, q in _launch_grouped(problems, lambda p: (_width_class(p.x.shape[1], dtype), p.part is not None), ConvProblem, _fill_fwd,
                                L().ymi_conv2d_fwd_multi, "conv2d_fwd_multi"):
        p.blocks = int(q.stat_blocks)


def _dgrad_joined_prepare(join, dy, weight4, k, stride, in_shape, dtype, packed=None):
    """-> (job, deposit): the data-gradient GEMM of a consumer of a (possibly joined) tensor, with the join's earlier contributions as
    addends when this is the last consumer; deposit: the result is a contribution to hand to the join (_dgrad_joined_finish)."""
    adds = join.arrive() if join is not None else []
    out = None
    if adds is not None and join is not None and join.dst is not None:
        # the tensor's gradient has a prepared place (a channel slice of its producer's gradient buffer: _ChanSplit2): the total goes there
        cand = join.dst.view(dtype)
        join.dst = None
        if cand is not None and tuple(cand.shape) == tuple(in_shape) and _dense_ok(cand, dtype) and not (k == 1 and stride > 1):
            out = cand
    elif adds is not None and join is not None and join.out is not None:
        out, join.out = join.out, None
        if len(adds) < 2 and _dense_ok(out, dtype) and tuple(out.shape) == tuple(in_shape) and not (k == 1 and stride > 1):
            adds = list(adds) + [out]  # the contribution already in the buffer rides as an addend; the total replaces it
        else:
            out = None  # (left for _C2fSplit's own add)
    return _dgrad_prepare(dy, weight4, k, stride, in_shape, dtype, adds, out, packed), adds is None


def _dgrad_joined_finish(join, dx, deposit):
    if deposit:
        join.deposit(dx)
        return None
    return dx


def _dgrad_joined(join, dy, weight4, k, stride, in_shape, dtype, packed=None):
    """data gradient of a consumer of a (possibly joined) tensor: deposits (and returns None) unless it is the last consumer."""
    job, deposit = _dgrad_joined_prepare(join, dy, weight4, k, stride, in_shape, dtype, packed)
    return _dgrad_joined_finish(join, _dgrad_launch(job), deposit)


def _stat_ws_bytes(m, o):
    """workspace of one train-mode BatchNorm over an [m, o] GEMM output: scale, shift and the statistics rows of every row block (float32)."""
    return (L().ymi_conv2d_stat_blocks(m, o) * 2 * o + 2 * o) * 4


def _bn_act_bwd(dout, raw, stats, act, gamma, beta, second=None):
    """backward of act(BatchNorm_train(raw)) -> (draw, dgamma, dbeta).  second = (gamma_b, beta_b, oa): the channels from oa on belong to a
    second BatchNorm with these parameters (two Conv blocks side by side in one buffer)."""
    o, dev = raw.shape[1], raw.device
    draw = empty_nhwc(*raw.shape, raw.dtype, dev)
    # two separate tensors: AccumulateGrad adopts them as .grad without a clone (views would be copied)
    dgamma = torch.empty(o, dtype=torch.float32, device=dev)
    dbeta = torch.empty(o, dtype=torch.float32, device=dev)
    ws = workspace(2048 * 2 * o * 4 + 256, dev, "bnbwd")
    if second is None:
        check(L().ymi_bn_act_bwd(_byref(as_ymi(dout)), _byref(as_ymi(raw)), ptr(gamma), ptr(stats[0]), ptr(stats[1]), ptr(beta), act,
                                 _byref(as_ymi(draw)), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream_ptr()), "bn_act_bwd")
    else:
        gamma_b, beta_b, oa = second
        check(L().ymi_bn_act_bwd_pair(_byref(as_ymi(dout)), _byref(as_ymi(raw)), ptr(gamma), ptr(beta), ptr(gamma_b), ptr(beta_b), oa, ptr(stats[0]), ptr(stats[1]),
                                      act, _byref(as_ymi(draw)), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(), stream_ptr()), "bn_act_bwd_pair")
    return draw, dgamma, dbeta


def _conv1x1_bwd_fused(dout, raw, stats, act, gamma, beta, x, weight, job):
    """the backward of a 1x1 stride-1 Conv block as ymi_conv1x1_bn_act_bwd: job (of _dgrad_prepare) names the result, the packed operand and the
    addends of the data gradient.  -> (dgamma, dbeta, dw), the weight gradient complete or registered with the pass's deferred slab sum as
    _wgrad's; None when the tensors are outside the kernel's scope (nothing was launched).  The launch runs on the current stream and is
    never held for a rider: the next layer waits for its dx."""
    lib = L()
    o, cin = weight.shape[0], weight.shape[1]
    dev = x.device
    a1 = _byref(as_ymi(job.fused[0])) if len(job.fused) > 0 else None
    a2 = _byref(as_ymi(job.fused[1])) if len(job.fused) > 1 else None
    tdo, traw, tx, tdx = as_ymi(dout), as_ymi(raw), as_ymi(x), as_ymi(job.dxv)
    if not lib.ymi_conv1x1_bn_act_bwd_ok(_byref(tdo), _byref(traw), _byref(tx), a1, a2, _byref(tdx)):
        return None
    dgamma = torch.empty(o, dtype=torch.float32, device=dev)
    dbeta = torch.empty(o, dtype=torch.float32, device=dev)
    params = (weight,)
    defer = RUN.defer and _in_backward() and _adoptable(params)
    dw = _new_dw(o, cin, 1, dev, params, None)
    need = int(lib.ymi_conv1x1_bn_act_bwd_workspace(tdo.n * tdo.h * tdo.w, o, cin))
    # (the slabs live in the workspace: a deferred sum needs it alive until the end-of-pass flush)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if defer else workspace(need, dev, "conv1x1bwd")
    rec = _lib.WgradPending() if defer else None
    if defer:
        _defer_wgrad(rec, (ws, x, dout, raw), weight)
    check(lib.ymi_conv1x1_bn_act_bwd(_byref(tdo), _byref(traw), ptr(gamma), ptr(stats[0]), ptr(stats[1]), ptr(beta), act, _byref(tx), ptr(job.wd), a1, a2,
                                     _byref(tdx), ptr(dgamma), ptr(dbeta), ptr(dw), ptr(ws), ws.numel(), _byref(rec) if defer else None, stream_ptr()),
          "conv1x1_bn_act_bwd")
    return dgamma, dbeta, dw


class _ConvBnAct(torch.autograd.Function):
    """act(BatchNorm_train(conv(x))) (+ residual).  Reference: Conv.forward, nn/modules/conv.py:69-79
    (+ Bottleneck add, nn/modules/block.py:488)."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, running_mean, running_var, stride, eps, momentum, act, residual, slot=None, join=None, res_join=None):
        dtype = x.dtype
        o, i, k, _ = weight.shape
        n, cp, h, w = x.shape
        ho, wo = _conv_out_hw(h, w, k, stride)
        dev = x.device
        _note_use(weight)
        wp = pack_conv_fwd(weight, cp, dtype)
        raw = empty_nhwc(n, o, ho, wo, dtype, dev)
        out = slot.view(n, o, ho, wo, dtype) if slot is not None else empty_nhwc(n, o, ho, wo, dtype, dev)
        stats = torch.empty((2, o), dtype=torch.float32, device=dev)
        ws = workspace(_stat_ws_bytes(n * ho * wo, o), dev, "conv")
        res = residual
        tres = _byref(as_ymi(res)) if res is not None else None
        if (HOOKS["stat_atomics"] and o % 4 == 0 and L().ymi_conv2d_bn_silu_fwd_acc_ok(_byref(as_ymi(raw)), _byref(as_ymi(out)), tres)
                and all(t is None or t.data_ptr() % 16 == 0 for t in (gamma, beta, running_mean, running_var))):
            # statistics as fixed-point atomic sums, finalized in the affine pass's prologue: two launches instead of three (or four)
            acc = _stat_acc(o, dev)
            check(
                L().ymi_conv2d_bn_silu_fwd_acc(
                    _byref(as_ymi(x)), ptr(wp), o, k, k, stride, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                    momentum, eps, act, tres, _byref(as_ymi(raw)), _byref(as_ymi(out)), ptr(stats[0]), ptr(stats[1]), ptr(acc), stream_ptr(),
                ),
                "conv2d_bn_silu_fwd_acc",
            )
        else:
            check(
                L().ymi_conv2d_bn_silu_fwd(
                    _byref(as_ymi(x)), ptr(wp), o, k, k, stride, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var),
                    momentum, eps, act, tres, _byref(as_ymi(raw)), _byref(as_ymi(out)), ptr(stats[0]), ptr(stats[1]), ptr(ws), ws.numel(), stream_ptr(),
                ),
                "conv2d_bn_silu_fwd",
            )
        ctx.save_for_backward(x, weight, gamma, beta, raw, stats)
        ctx.cfg = (stride, act, i, residual is not None)
        ctx.joins = (join, res_join)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, gamma, beta, raw, stats = ctx.saved_tensors
        stride, act, cin, has_res = ctx.cfg
        dtype = x.dtype
        o, _, k, _ = weight.shape
        dout = grad_nhwc(dout, dtype)
        join, res_join = ctx.joins
        want_dx, want_dw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # the residual hand-through first: when x is both the input and the residual (Bottleneck shortcut), the data
        # gradient below is then the join's last consumer and adds `dout` in its epilogue
        hand_res = has_res and ctx.needs_input_grad[10]
        if (HOOKS["fused_bwd_1x1"] and want_dx and want_dw and k == 1 and stride == 1 and dtype == torch.bfloat16 and o in (64, 128)
                and x.shape[1] == cin and cin <= 128 and not _deferred_twice((weight,))):
            # a 1x1 block: BatchNorm apply, data gradient and weight gradient in ONE kernel, draw is never stored (csrc/wgrad.hip: conv1x1_bwd_kernel).
            # One 128-wide block of input channels only: with two or three column blocks, each forming draw again, the kernel measured level with
            # or slower than the three launches (profiles/conv1x1_bwd_fused_ab.txt); the library's scope is wider than this routing rule.
            dres = _join_plain(res_join, dout) if hand_res else None
            job, deposit = _dgrad_joined_prepare(join, dout, weight, k, stride, x.shape, dtype)  # (dout stands in for draw: the same shape)
            done = _conv1x1_bwd_fused(dout, raw, stats, act, gamma, beta, x, weight, job)
            if done is None:  # outside the kernel's scope after all: the three launches, with the job as prepared
                draw, dgamma, dbeta = _bn_act_bwd(dout, raw, stats, act, gamma, beta)
                dx = _dgrad_joined_finish(join, _dgrad_launch(job._replace(dy=draw, ty=as_ymi(draw))), deposit)
                dw, _ = _wgrad_maybe_async(x, draw, o, cin, k, stride, False, (weight,))
            else:
                dgamma, dbeta, dw = done
                dx = _dgrad_joined_finish(join, _dgrad_finish(job), deposit)
            return dx, dw, dgamma, dbeta, None, None, None, None, None, None, dres, None, None, None
        draw, dgamma, dbeta = _bn_act_bwd(dout, raw, stats, act, gamma, beta)
        dres = _join_plain(res_join, dout) if hand_res else None
        dx = None
        if want_dx:
            dx = _dgrad_joined(join, draw, weight, k, stride, x.shape, dtype)
        dw = None
        if want_dw:  # (a frozen conv weight: no GEMM, and nothing for a deferred slab sum to write into)
            dw, _ = _wgrad_maybe_async(x, draw, o, cin, k, stride, False, (weight,))
        return dx, dw, dgamma, dbeta, None, None, None, None, None, None, dres, None, None, None


def conv_bn_act(x, weight, bn, stride, act=ACT_SILU, residual=None, slot=None):
    """train-mode Conv block on an internal (NHWC) tensor; updates bn.running_* in place.  slot: optional OutSlot.
    Tensors marked with mark_join() (several consumers) have their gradient sums formed in the data-gradient epilogue."""
    if bn.momentum is None:
        raise RuntimeError("BatchNorm with cumulative moving average (momentum=None) is not supported")
    if torch.is_grad_enabled() and weight.shape[0] % chunk_elems(x.dtype) != 0 and (x.requires_grad or weight.requires_grad):
        # the backward kernels (BatchNorm backward, data / weight gradient GEMMs) read the output gradient in 16-byte chunks
        raise NotImplementedError(f"training a Conv with {weight.shape[0]} output channels in {x.dtype}: the backward kernels need channel counts in "
                                  f"whole 16-byte chunks (multiples of {chunk_elems(x.dtype)}); every standard YOLOv8 width is - use float32 for this width")
    out = _ConvBnAct.apply(x, weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, int(stride), float(bn.eps), float(bn.momentum), int(act), residual, slot,
                           join_of(x), join_of(residual) if residual is not None else None)
    _count_batch(bn)
    return out


class _FirstConvBnAct(torch.autograd.Function):
    """The model's first Conv block on the caller's float32 NCHW image (reference yolov8.yaml:738 through conv.py:50-79) as direct
    kernels that never store the raw convolution output (csrc/first_conv.hip): forward = statistics pass, finalize, apply pass;
    backward = reduce pass, final sums, fused BatchNorm-apply + weight-gradient pass - each recomputes the 27-tap convolution from the
    NHWC bfloat16 4-channel copy of the image that the statistics pass leaves behind (26 MB saved for backward instead of a 52 MB
    padded copy + the 210 MB raw output).  The image receives no gradient."""

    @staticmethod
    def forward(ctx, img, weight, gamma, beta, running_mean, running_var, eps, momentum, act):
        n, c, h, w = img.shape
        o = weight.shape[0]
        dt = torch.bfloat16
        dev = img.device
        ho, wo = _conv_out_hw(h, w, 3, 2)
        _note_use(weight)
        x4 = torch.empty((n, h, w, 4), dtype=dt, device=dev).permute(0, 3, 1, 2)
        out = empty_nhwc(n, o, ho, wo, dt, dev)
        stats = torch.empty((2, o), dtype=torch.float32, device=dev)
        need = (2 * o + (L().ymi_first_conv_stat_blocks(n, h, w) + 64) * 2 * o) * 4
        ws = workspace(need, dev, "conv")
        check(
            L().ymi_first_conv_bn_act_fwd(ptr(img), n, c, h, w, ptr(weight.detach()), o, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), momentum, eps,
                                          act, _byref(as_ymi(x4)), _byref(as_ymi(out)), ptr(stats[0]), ptr(stats[1]), ptr(ws), ws.numel(), stream_ptr()),
            "first_conv_bn_act_fwd",
        )
        ctx.save_for_backward(x4, weight, gamma, beta, stats)
        ctx.act = act
        return out

    @staticmethod
    def backward(ctx, dout):
        x4, weight, gamma, beta, stats = ctx.saved_tensors
        o, cin, k, _ = weight.shape
        dev = x4.device
        dout = grad_nhwc(dout, torch.bfloat16)
        dgamma = torch.empty(o, dtype=torch.float32, device=dev)
        dbeta = torch.empty(o, dtype=torch.float32, device=dev)
        n, _, h, w = x4.shape
        need = int(L().ymi_first_conv_bwd_workspace(n, h, w, o))
        defer = (ctx.needs_input_grad[1] and RUN.defer and _in_backward() and _adoptable((weight,)) and not _deferred_twice((weight,)))
        dw = _new_dw(o, cin, k, dev, (weight,), None)
        # (the slabs live in the workspace: a deferred sum needs it alive until the end-of-pass flush)
        ws = torch.empty(need, dtype=torch.uint8, device=dev) if defer else workspace(need, dev, "firstconv")
        rec = _lib.WgradPending() if defer else None
        if defer:
            _defer_wgrad(rec, (ws, x4, dout), weight)
        check(
            L().ymi_first_conv_bn_act_bwd(_byref(as_ymi(x4)), ptr(weight.detach()), cin, o, ptr(gamma), ptr(beta), ptr(stats[0]), ptr(stats[1]), ctx.act,
                                          _byref(as_ymi(dout)), ptr(dgamma), ptr(dbeta), ptr(dw), ptr(ws), ws.numel(), _byref(rec) if defer else None, stream_ptr()),
            "first_conv_bn_act_bwd",
        )
        return None, (dw if ctx.needs_input_grad[1] else None), dgamma, dbeta, None, None, None, None, None


def first_conv_ok(x, conv, residual, slot):
    """the direct first-layer kernel applies: a float32 NCHW image that needs no gradient, bfloat16 compute, 3x3 stride 2, <= 4 input channels."""
    return (residual is None and slot is None and torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()
            and x.shape[1] <= 4 and not x.requires_grad and conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.in_channels == x.shape[1]
            and conv.out_channels in (16, 32, 48, 64) and x.shape[2] % 2 == 0 and x.shape[3] % 4 == 0 and x.data_ptr() % 16 == 0 and compute_dtype(x) == torch.bfloat16
            and HOOKS["first_conv"])


def first_conv_bn_act(img, weight, bn, act=ACT_SILU):
    if bn.momentum is None:
        raise RuntimeError("BatchNorm with cumulative moving average (momentum=None) is not supported")
    out = _FirstConvBnAct.apply(img, weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps), float(bn.momentum), int(act))
    _count_batch(bn)
    return out


class _ChanSplit2(torch.autograd.Function):
    """(t[:, :c], t[:, c:]) of an NHWC tensor as two views whose gradients are formed IN PLACE in one buffer: each view carries a GradJoin
    with a prepared destination (GradJoin.dst), its consumer's data-gradient GEMM writes its slice of the buffer, and backward hands the
    buffer on without a copy (autograd's own slices would zero-fill two full tensors and add them).  Falls back to copies when a gradient
    arrives somewhere else."""

    @staticmethod
    def forward(ctx, t, c):
        ctx.c, ctx.shape = c, tuple(t.shape)
        ctx.gb = _ChanSplit2.last = _GradBuffer(t.shape, t.device)  # (chan_split2 picks it up right after apply)
        return t[:, :c], t[:, c:]

    @staticmethod
    def backward(ctx, ga, gb):
        c = ctx.c
        buf = ctx.gb.buf
        ctx.gb.buf = None
        n, ctot, h, w = ctx.shape
        g0 = ga if ga is not None else gb
        if buf is None or buf.dtype != g0.dtype:
            buf = empty_nhwc(n, ctot, h, w, g0.dtype, g0.device)
        for g, dst in ((ga, buf[:, :c]), (gb, buf[:, c:])):
            if g is None:
                dst.zero_()
            elif not (g.data_ptr() == dst.data_ptr() and g.stride() == dst.stride() and g.dtype == dst.dtype):
                check(L().ymi_copy(_byref(as_ymi(grad_nhwc(g, buf.dtype))), _byref(as_ymi(dst)), stream_ptr()), "copy")
        return buf, None


def chan_split2(t, c):
    """-> (t[:, :c], t[:, c:]); in training each half is marked with a join whose total lands in the matching slice of ONE gradient buffer."""
    a, b = _ChanSplit2.apply(t, int(c))
    if torch.is_grad_enabled() and t.requires_grad:
        gb, _ChanSplit2.last = getattr(_ChanSplit2, "last", None), None
        if gb is not None:
            for v, lo, hi in ((a, 0, int(c)), (b, int(c), t.shape[1])):
                mark_join(v, 1, force=True)
                j = join_of(v)
                if j is not None:
                    j.dst = _GradSlot(gb, lo, hi)
    return a, b


class _ConvBnActPair(torch.autograd.Function):
    """two Conv blocks of the SAME input as one convolution with oA + oB output channels: Detect's sibling branches cv2[i][0] / cv3[i][0]
    (reference head.py:44-59,71-72).  BatchNorm is per channel, so the result is exactly the two separate blocks; parameters stay the
    reference's separate tensors (their packed operands lie side by side in the weight arena).  The data gradient is ONE GEMM with
    K = taps * (oA + oB) (the GradJoin sum of the two branches disappears into the accumulator), the weight gradient one GEMM whose
    [oA + oB, cin, k, k] result is handed out as two views."""

    @staticmethod
    def forward(ctx, x, wa, ga, ba, rma, rva, wb, gb, bb, rmb, rvb, stride, eps, momentum, act, join):
        dtype = x.dtype
        oa, i, k, _ = wa.shape
        ob = wb.shape[0]
        o = oa + ob
        n, cp, h, w = x.shape
        ho, wo = _conv_out_hw(h, w, k, stride)
        dev = x.device
        _note_use(wa, wb)
        wp = pack_conv_fwd_pair(wa, wb, cp, dtype)
        raw = empty_nhwc(n, o, ho, wo, dtype, dev)
        out = empty_nhwc(n, o, ho, wo, dtype, dev)
        stats = torch.empty((2, o), dtype=torch.float32, device=dev)
        ws = workspace(_stat_ws_bytes(n * ho * wo, o), dev, "conv")
        check(
            L().ymi_conv2d_bn_silu_fwd_pair(
                _byref(as_ymi(x)), ptr(wp), o, oa, k, k, stride, ptr(ga), ptr(ba), ptr(rma), ptr(rva), ptr(gb), ptr(bb), ptr(rmb), ptr(rvb),
                momentum, eps, act, _byref(as_ymi(raw)), _byref(as_ymi(out)), ptr(stats[0]), ptr(stats[1]), ptr(ws), ws.numel(), stream_ptr(),
            ),
            "conv2d_bn_silu_fwd_pair",
        )
        ctx.save_for_backward(x, wa, wb, ga, ba, gb, bb, raw, stats)
        ctx.cfg = (stride, act, i)
        ctx.join = join
        return out

    @staticmethod
    def backward(ctx, dout):
        x, wa, wb, ga, ba, gb, bb, raw, stats = ctx.saved_tensors
        stride, act, cin = ctx.cfg
        dtype = x.dtype
        oa, _, k, _ = wa.shape
        o = oa + wb.shape[0]
        dout = grad_nhwc(dout, dtype)
        draw, dgamma, dbeta = _bn_act_bwd(dout, raw, stats, act, ga, ba, (gb, bb, oa))
        dx = None
        if ctx.needs_input_grad[0]:
            wd = pack_conv_dgrad_pair(wa, wb, stride, dtype)
            dx = _dgrad_joined(ctx.join, draw, None, k, stride, x.shape, dtype, packed=(wd, cin))
        nig = ctx.needs_input_grad
        dwa = dwb = None
        if nig[1] or nig[6]:
            # one GEMM for both weights; the two gradients are the halves of its [oA + oB, cin, k, k] result.  Deferred only when BOTH
            # parameters adopt their half (a frozen one would leave its half's memory to the allocator before the batched slab sum runs)
            dw, _ = _wgrad_maybe_async(x, draw, o, cin, k, stride, False, (wa, wb), pair_rows=oa)
            dwa, dwb = (dw[:oa] if nig[1] else None), (dw[oa:] if nig[6] else None)
        return (dx, dwa, dgamma[:oa], dbeta[:oa], None, None, dwb, dgamma[oa:], dbeta[oa:], None, None, None, None, None, None, None)


def conv_bn_act_pair(x, conv_a, bn_a, conv_b, bn_b, act=ACT_SILU):
    """train-mode act(BN_a(conv_a(x))) and act(BN_b(conv_b(x))) from ONE convolution -> [N, oA + oB, H', W'] (the first block's channels first).
    conv_*: nn.Conv2d parameter containers of equal kernel / stride / input width; widths in whole 16-byte chunks."""
    wa, wb = conv_a.weight, conv_b.weight
    if wa.shape[1:] != wb.shape[1:] or conv_a.stride != conv_b.stride:
        raise RuntimeError("conv_bn_act_pair: the two convolutions must share kernel size, stride and input width")
    if bn_a.momentum is None or bn_b.momentum is None or bn_a.eps != bn_b.eps or bn_a.momentum != bn_b.momentum:
        raise RuntimeError("conv_bn_act_pair: the two BatchNorms must share eps and momentum (initialize_weights sets them alike)")
    ch = chunk_elems(x.dtype)
    if wa.shape[0] % ch or wb.shape[0] % ch:
        raise NotImplementedError(f"conv_bn_act_pair: output widths {wa.shape[0]} / {wb.shape[0]} must be multiples of {ch} in {x.dtype}")
    out = _ConvBnActPair.apply(x, wa, bn_a.weight, bn_a.bias, bn_a.running_mean, bn_a.running_var, wb, bn_b.weight, bn_b.bias, bn_b.running_mean,
                               bn_b.running_var, int(conv_a.stride[0]), float(bn_a.eps), float(bn_a.momentum), int(act), join_of(x))
    _count_batch(bn_a)
    _count_batch(bn_b)
    return out


# One level of the Detect head as _DetectTrain takes it: the level's input, the four Conv blocks a0 = cv2[i][0], b0 = cv3[i][0], a1 = cv2[i][1],
# b1 = cv3[i][1] (convolution weight, BatchNorm gamma, beta, running mean, running variance) and the biased 1x1 outputs oa = cv2[i][2], ob = cv3[i][2].
# The argument order of forward, the gradient order of backward and the count per level all come from this one list.
_Level = namedtuple("_Level", """x
    a0_w a0_gamma a0_beta a0_mean a0_var
    b0_w b0_gamma b0_beta b0_mean b0_var
    a1_w a1_gamma a1_beta a1_mean a1_var
    b1_w b1_gamma b1_beta b1_mean b1_var
    oa_w oa_bias ob_w ob_bias""")
# what backward needs of a level: these arguments, then per BatchNorm stage the raw convolution output, the batch statistics and the activated output
_SAVED_ARGS = "x a0_w b0_w a0_gamma a0_beta b0_gamma b0_beta a1_w b1_w a1_gamma a1_beta b1_gamma b1_beta oa_w ob_w".split()
_Saved = namedtuple("_Saved", _SAVED_ARGS + "raw1 st1 h1 raw2 st2 h2".split())
# a level's sizes: input [n, cp, h, w], branch widths c2 / c3 (o = c2 + c3 side by side in one buffer), m = n * h * w rows, and its place in the workspace
_Geo = namedtuple("_Geo", "n cp h w c2 c3 o m ws_off stat_bytes")


def _per_level(rec, flat, nl):
    """flat: nl consecutive groups of len(rec._fields) values -> [rec] per level."""
    n = len(rec._fields)
    return [rec._make(flat[l * n : (l + 1) * n]) for l in range(nl)]


def _detect_args(xs, levels):
    """-> the tensor arguments of _DetectTrain: per level the fields of _Level.  levels: per level (cv2[i][0], cv3[i][0], cv2[i][1], cv3[i][1], cv2[i][2], cv3[i][2])."""
    t = []
    for x, (a0, b0, a1, b1, oa, ob) in zip(xs, levels):
        t.append(x)
        for m in (a0, b0, a1, b1):
            t += [m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var]
        t += [oa.weight, oa.bias, ob.weight, ob.bias]
    return t


def _detect_grads(per_level):
    """what _DetectTrain.backward returns: None for `meta`, then one entry per field of _Level and level (per_level: dicts field -> gradient; absent: None)."""
    return (None,) + tuple(g for d in per_level for g in _Level(**{**dict.fromkeys(_Level._fields), **d}))


class _DetectTrain(torch.autograd.Function):
    """the train-mode Detect head of ALL levels (reference head.py:66-74 loops over the levels; per level cv2[i] / cv3[i] are
    Conv -> Conv -> biased 1x1, head.py:44-59), its stages run in lockstep across the levels: every GEMM stage is ONE launch over the
    problems of all levels (ymi_conv2d_fwd_multi / ymi_conv2d_bwd_data_multi) - the 40 x 40 and 20 x 20 levels fill a fraction of the
    chip on their own.  Per level the arithmetic is that of _ConvBnActPair (first convolutions), two _ConvBnAct side by side in one
    buffer (second convolutions, one BatchNorm pass over both) and two _ConvAffineAct.  Outputs per level: box map [N, 64, H, W] and
    the class map in a buffer padded to whole 16-byte rows."""

    @staticmethod
    def forward(ctx, meta, *t):
        nl, eps, momentum, joins, ncpad = meta
        lv = _per_level(_Level, t, nl)
        dtype, dev = lv[0].x.dtype, lv[0].x.device
        lib = L()
        geo = []
        need = 0
        for v in lv:
            n, cp, h, w = v.x.shape
            c2, c3 = v.a0_w.shape[0], v.b0_w.shape[0]
            g = _Geo(n, cp, h, w, c2, c3, c2 + c3, n * h * w, need, _stat_ws_bytes(n * h * w, c2 + c3))
            geo.append(g)
            need += 2 * g.stat_bytes  # two BatchNorm stages
            _note_use(v.a0_w, v.b0_w, v.a1_w, v.b1_w, v.oa_w, v.ob_w)
        ws = workspace(need, dev, "detect").view(torch.float32)

        def region(g, stage):
            """-> scale, shift, statistics rows of a level's BatchNorm stage."""
            base, o = (g.ws_off + stage * g.stat_bytes) // 4, g.o
            return ws[base : base + o], ws[base + o : base + 2 * o], ws[base + 2 * o : base + g.stat_bytes // 4]

        def bn_stage(probs_of_level, stage, raws, bns):
            """the multi-problem GEMM of a stage, then per level: statistics -> scale / shift, affine + SiLU.  bns: per level (gamma, beta, running mean,
            running variance) of the cv2 block, then of the cv3 block."""
            _conv_fwd_multi([p for ps in probs_of_level for p in ps], dtype)
            outs, stats = [], []
            for g, ps, raw, bn in zip(geo, probs_of_level, raws, bns):
                blocks = ps[0].blocks
                if any(p.blocks != blocks for p in ps):
                    raise RuntimeError("_DetectTrain: the convolutions of one BatchNorm group ran with different row tiles")
                scale, shift, part = region(g, stage)
                st = torch.empty((2, g.o), dtype=torch.float32, device=dev)
                out = empty_nhwc(g.n, g.o, g.h, g.w, dtype, dev)
                check(lib.ymi_bn_finalize_pair(ptr(part), blocks, g.m, g.o, g.c2, *map(ptr, bn), momentum, eps, ptr(scale), ptr(shift), ptr(st[0]), ptr(st[1]),
                                               stream_ptr()), "bn_finalize_pair")
                check(lib.ymi_scale_shift_act(_byref(as_ymi(raw)), ptr(scale), ptr(shift), ACT_SILU, None, _byref(as_ymi(out)), stream_ptr()), "scale_shift_act")
                outs.append(out)
                stats.append(st)
            return outs, stats

        # stage 1: the two first convolutions of a level as ONE (they read the same input)
        raw1 = [empty_nhwc(g.n, g.o, g.h, g.w, dtype, dev) for g in geo]
        probs = [[FwdProblem(v.x, pack_conv_fwd_pair(v.a0_w, v.b0_w, g.cp, dtype), g.o, v.a0_w.shape[2], r, part=region(g, 0)[2], pstride=g.o)]
                 for v, g, r in zip(lv, geo, raw1)]
        h1, st1 = bn_stage(probs, 0, raw1, [(v.a0_gamma, v.a0_beta, v.a0_mean, v.a0_var, v.b0_gamma, v.b0_beta, v.b0_mean, v.b0_var) for v in lv])
        # stage 2: the second convolutions read their half of h1 and write their half of one buffer; one BatchNorm pass over both
        raw2 = [empty_nhwc(g.n, g.o, g.h, g.w, dtype, dev) for g in geo]
        probs = []
        for v, g, hh, r in zip(lv, geo, h1, raw2):
            c2, c3 = g.c2, g.c3
            part = region(g, 1)[2]
            probs.append([FwdProblem(hh[:, :c2], pack_conv_fwd(v.a1_w, c2, dtype), c2, v.a1_w.shape[2], r[:, :c2], part=part, pstride=g.o, poff=0),
                          FwdProblem(hh[:, c2:], pack_conv_fwd(v.b1_w, c3, dtype), c3, v.b1_w.shape[2], r[:, c2:], part=part, pstride=g.o, poff=c2)])
        h2, st2 = bn_stage(probs, 1, raw2, [(v.a1_gamma, v.a1_beta, v.a1_mean, v.a1_var, v.b1_gamma, v.b1_beta, v.b1_mean, v.b1_var) for v in lv])
        # stage 3: the biased 1x1 outputs
        outs, probs = [], []
        for v, g, hh in zip(lv, geo, h2):
            c2, c3 = g.c2, g.c3
            ob, nc = v.oa_w.shape[0], v.ob_w.shape[0]
            box = empty_nhwc(g.n, ob, g.h, g.w, dtype, dev)
            cls = empty_nhwc(g.n, ncpad, g.h, g.w, dtype, dev)  # (padded channels are never read: see _ConvAffineAct)
            probs += [FwdProblem(hh[:, :c2], pack_conv_fwd(v.oa_w, c2, dtype), ob, 1, box, bias=v.oa_bias),
                      FwdProblem(hh[:, c2:], pack_conv_fwd(v.ob_w, c3, dtype), nc, 1, cls[:, :nc] if ncpad != nc else cls, bias=v.ob_bias)]
            outs += [box, cls]
        _conv_fwd_multi(probs, dtype)
        saved = []
        for v, r1, s1, a1, r2, s2, a2 in zip(lv, raw1, st1, h1, raw2, st2, h2):
            saved += _Saved(*[getattr(v, f) for f in _SAVED_ARGS], r1, s1, a1, r2, s2, a2)
        ctx.save_for_backward(*saved)
        ctx.bias_params = [(v.oa_bias if v.oa_bias.requires_grad else None, v.ob_bias if v.ob_bias.requires_grad else None) for v in lv]  # (leaf parameters: no cycle)
        ctx.meta = (nl, joins, ncpad, geo)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gout):
        nl, joins, ncpad, geo = ctx.meta
        sv = _per_level(_Saved, ctx.saved_tensors, nl)
        need = [v._asdict() for v in _per_level(_Level, ctx.needs_input_grad[1:], nl)]
        grads = [{} for _ in range(nl)]  # per level: field of _Level -> gradient
        dtype, dev = sv[0].x.dtype, sv[0].x.device

        def dgrad_halves(branches):
            """branches(l) -> (dy, weight) of the level's cv2 and of its cv3 convolution: their data gradients into the two halves of one buffer
            per level, ONE launch over all levels -> the buffers."""
            jobs, bufs = [], []
            for l, g in enumerate(geo):
                pair = branches(l)
                buf = empty_nhwc(g.n, g.o, g.h, g.w, dtype, dev)
                for (dy, wt), lo, hi in zip(pair, (0, g.c2), (g.c2, g.o)):
                    jobs.append(_dgrad_prepare(dy, None, wt.shape[2], 1, (g.n, hi - lo, g.h, g.w), dtype, [], buf[:, lo:hi],
                                               (pack_conv_dgrad(wt, dy.shape[1], 1, dtype), hi - lo)))
                bufs.append(buf)
            _dgrad_multi(jobs, dtype)
            return bufs

        # stage 3: data gradients of the 1x1 outputs into the two halves of dh2, weight / bias gradients per convolution
        dys = []

        def stage3(l):
            g, s = geo[l], sv[l]
            dbox, dcls = gout[2 * l], gout[2 * l + 1]
            dbox = grad_nhwc(dbox, dtype) if dbox is not None else torch.zeros((g.n, g.h, g.w, s.oa_w.shape[0]), dtype=dtype, device=dev).permute(0, 3, 1, 2)
            dcls = grad_nhwc(dcls, dtype) if dcls is not None else torch.zeros((g.n, g.h, g.w, ncpad), dtype=dtype, device=dev).permute(0, 3, 1, 2)
            dys.append((dbox, dcls))
            return (dbox, s.oa_w), (dcls, s.ob_w)

        dh2 = dgrad_halves(stage3)
        for g, s, nd, gr, dy, bias in zip(geo, sv, need, grads, dys, ctx.bias_params):
            for fw, fb, wt, xin, dyh, bp in (("oa_w", "oa_bias", s.oa_w, s.h2[:, : g.c2], dy[0], bias[0]), ("ob_w", "ob_bias", s.ob_w, s.h2[:, g.c2 :], dy[1], bias[1])):
                if nd[fw] or nd[fb]:
                    dw, db = _wgrad_maybe_async(xin, dyh, wt.shape[0], xin.shape[1], 1, 1, True, (wt, bp))
                    gr[fw] = dw.view(wt.shape) if nd[fw] else None
                    gr[fb] = db if nd[fb] else None
        # stage 2: BatchNorm backward over both second convolutions, their data gradients into the halves of dh1, their weight gradients
        draws = []

        def stage2(l):
            s, c2 = sv[l], geo[l].c2
            draw, dgamma, dbeta = _bn_act_bwd(dh2[l], s.raw2, s.st2, ACT_SILU, s.a1_gamma, s.a1_beta, (s.b1_gamma, s.b1_beta, c2))
            grads[l].update(a1_gamma=dgamma[:c2], a1_beta=dbeta[:c2], b1_gamma=dgamma[c2:], b1_beta=dbeta[c2:])
            draws.append(draw)
            return (draw[:, :c2], s.a1_w), (draw[:, c2:], s.b1_w)

        dh1 = dgrad_halves(stage2)
        dh2 = None
        for g, s, nd, gr, draw in zip(geo, sv, need, grads, draws):
            for fw, wt, lo, hi in (("a1_w", s.a1_w, 0, g.c2), ("b1_w", s.b1_w, g.c2, g.o)):
                if nd[fw]:
                    gr[fw], _ = _wgrad_maybe_async(s.h1[:, lo:hi], draw[:, lo:hi], hi - lo, hi - lo, wt.shape[2], 1, False, (wt,))
        # stage 1: BatchNorm backward, ONE data gradient per level (the pair's, joined with the input's other consumers), the pair's weight gradient
        jobs, draws = [], []
        for l, (g, s, gr) in enumerate(zip(geo, sv, grads)):
            c2 = g.c2
            draw, dgamma, dbeta = _bn_act_bwd(dh1[l], s.raw1, s.st1, ACT_SILU, s.a0_gamma, s.a0_beta, (s.b0_gamma, s.b0_beta, c2))
            gr.update(a0_gamma=dgamma[:c2], a0_beta=dbeta[:c2], b0_gamma=dgamma[c2:], b0_beta=dbeta[c2:])
            draws.append(draw)
            if need[l]["x"]:
                jobs.append((l,) + _dgrad_joined_prepare(joins[l], draw, None, s.a0_w.shape[2], 1, s.x.shape, dtype,
                                                         (pack_conv_dgrad_pair(s.a0_w, s.b0_w, 1, dtype), s.a0_w.shape[1])))
        dh1 = None
        if jobs:
            dxs = _dgrad_multi([j[1] for j in jobs], dtype)
            for (l, _, deposit), dx in zip(jobs, dxs):
                grads[l]["x"] = _dgrad_joined_finish(joins[l], dx, deposit)
        for g, s, nd, gr, draw in zip(geo, sv, need, grads, draws):
            if nd["a0_w"] or nd["b0_w"]:
                dw, _ = _wgrad_maybe_async(s.x, draw, g.o, s.a0_w.shape[1], s.a0_w.shape[2], 1, False, (s.a0_w, s.b0_w), pair_rows=g.c2)
                gr["a0_w"] = dw[: g.c2] if nd["a0_w"] else None
                gr["b0_w"] = dw[g.c2 :] if nd["b0_w"] else None
        return _detect_grads(grads)


def detect_train_ok(levels, dtype):
    """the lockstep form needs: at most 4 levels (8 problems a launch), 3x3 / 3x3 / 1x1 stride-1 branches with SiLU Conv blocks, branch
    widths in whole 16-byte chunks and of ONE width class (both halves of a stage ride in one launch, which fixes the row tile the
    shared statistics rows are counted in), BatchNorms with one eps / momentum."""
    if not HOOKS["detect_multi"] or not (1 <= len(levels) <= 4):
        return False
    ch = chunk_elems(dtype)
    eps = mom = None
    for a0, b0, a1, b1, oa, ob in levels:
        c2, c3 = a0.conv.out_channels, b0.conv.out_channels
        if c2 % ch or c3 % ch or _width_class(c2, dtype) != _width_class(c3, dtype) or oa.out_channels % ch:
            return False
        for m, k in ((a0, 3), (b0, 3), (a1, 3), (b1, 3)):
            cv, bn = m.conv, getattr(m, "bn", None)
            if (bn is None or not isinstance(m.act, torch.nn.SiLU) or cv.kernel_size != (k, k) or cv.stride != (1, 1) or cv.groups != 1 or cv.dilation != (1, 1)
                    or cv.bias is not None or bn.momentum is None):
                return False
            if eps is None:
                eps, mom = bn.eps, bn.momentum
            if bn.eps != eps or bn.momentum != mom:
                return False
        if a1.conv.in_channels != c2 or b1.conv.in_channels != c3 or a0.conv.in_channels != b0.conv.in_channels:
            return False
        for m, cin in ((oa, c2), (ob, c3)):
            if m.kernel_size != (1, 1) or m.stride != (1, 1) or m.in_channels != cin or m.bias is None:
                return False
    return True


def detect_train(xs, levels):
    """xs: the internal input tensor of each level; levels: per level (cv2[i][0], cv3[i][0], cv2[i][1], cv3[i][1], cv2[i][2], cv3[i][2]) ->
    ([box map], [class map]) exactly as the per-level modules would give them."""
    dtype = xs[0].dtype
    bn0 = levels[0][0].bn
    nc = levels[0][5].out_channels
    ncpad = round_up(nc, chunk_elems(dtype))
    outs = _DetectTrain.apply((len(levels), float(bn0.eps), float(bn0.momentum), [join_of(x) for x in xs], ncpad), *_detect_args(xs, levels))
    for lv in levels:
        for m in lv[:4]:
            _count_batch(m.bn)
    box = list(outs[0::2])
    cls = [(_ChanSlice.apply(c, nc) if ncpad != nc else c) for c in outs[1::2]]
    return box, cls


# ------------------------------------------------------------------- conv / linear with affine epilogue
class _ConvAffineAct(torch.autograd.Function):
    """y = act(scale*conv(x) + bias) (+ residual), one kernel.  Used for eval-mode Conv (BN folded into
    scale/bias: conv.py:81-91 and utils/torch_utils.py:240-271), Detect's biased 1x1 outputs
    (head.py:45-59) and every nn.Linear of SwinBlock (swin_block.py:29-35) with k = 1."""

    @staticmethod
    def forward(ctx, x, weight, scale, bias, stride, act, residual, cout_pad, join=None, res_join=None):
        dtype = x.dtype
        w4 = _as4d(weight)
        o, i, k, _ = w4.shape
        dev = x.device
        _note_use(weight)
        wp = pack_conv_fwd(weight, x.shape[1], dtype)
        if x.dim() == 4:
            n, cp, h, w = x.shape
            ho, wo = _conv_out_hw(h, w, k, stride)
            # (padded channels - an output whose width is not a whole 16-byte chunk, e.g. Detect's class map at nc = 1 - are never
            # read: every consumer sees the [:, :o] view, and the GRADIENT's padded channels are zeros written by its producer)
            y = empty_nhwc(n, cout_pad, ho, wo, dtype, dev)
            yv = y[:, :o] if cout_pad != o else y
        else:
            y = torch.empty((x.shape[0], cout_pad), dtype=dtype, device=dev)
            yv = y[:, :o] if cout_pad != o else y
        check(
            L().ymi_conv2d_fwd(_byref(as_ymi(x)), ptr(wp), o, k, k, stride, ptr(scale), ptr(bias), act,
                               _byref(as_ymi(residual)) if residual is not None else None, _byref(as_ymi(yv)), None, None, stream_ptr()),
            "conv2d_fwd",
        )
        if act != ACT_NONE or scale is not None:
            ctx.unsupported = "backward through a fused activation / BN-folded conv is not implemented (use train mode or act=none)"
        else:
            ctx.unsupported = None
        ctx.save_for_backward(x, weight)
        ctx.bias_param = bias if (bias is not None and bias.requires_grad) else None  # (a leaf parameter: no cycle)
        ctx.cfg = (stride, i, bias is not None, residual is not None, cout_pad)
        ctx.joins = (join, res_join)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.unsupported:
            raise NotImplementedError(ctx.unsupported)
        x, weight = ctx.saved_tensors
        stride, cin, has_bias, has_res, cout_pad = ctx.cfg
        dtype = x.dtype
        w4 = _as4d(weight)
        o, _, k, _ = w4.shape
        dy = grad_nhwc(dy, dtype)
        join, res_join = ctx.joins
        dres = None
        if has_res and ctx.needs_input_grad[6]:
            dres = _join_plain(res_join, dy[:, :o] if cout_pad != o else dy)
        dx = None
        if ctx.needs_input_grad[0]:
            # (the parameter itself, 2-D for a linear, not its 4-D view: the weight arena knows packed operands by their parameter)
            dx = _dgrad_joined(join, dy, weight, k, stride, x.shape, dtype)
        dw = db = None
        need_w, need_b = ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[3]
        if need_w or need_b:
            # (the bias gradient comes out of the same launch; a frozen weight with a trainable bias gets its complete, un-deferred result)
            dw, db = _wgrad_maybe_async(x, dy, o, cin, k, stride, has_bias, (weight, ctx.bias_param))
            dw = dw.view(weight.shape) if need_w else None
            db = db if need_b else None
        return dx, dw, None, db, None, None, dres, None, None, None


def conv_affine_act(x, weight, scale=None, bias=None, stride=1, act=ACT_NONE, residual=None, pad_out=False):
    w4 = _as4d(weight)
    o = w4.shape[0]
    cout_pad = round_up(o, chunk_elems(x.dtype)) if pad_out else o
    y = _ConvAffineAct.apply(x, weight, scale, bias, int(stride), int(act), residual, cout_pad, join_of(x), join_of(residual) if residual is not None else None)
    if cout_pad != o:
        y = _ChanSlice.apply(y, o)
    return y


class _ChanSlice(torch.autograd.Function):
    """y[:, :o] of a channel-padded tensor.  Backward: the gradient of the padded tensor with zeros in the padded channels.  When
    the incoming gradient already IS the [:, :o] view of such a padded buffer (the detection loss writes its class-map gradients
    that way, pads zeroed) the buffer is handed through; otherwise zeros + copy, as autograd's own slice would do."""

    @staticmethod
    def forward(ctx, y, o):
        ctx.shape = tuple(y.shape)
        return y[:, :o]

    @staticmethod
    def backward(ctx, g):
        base = RUN.padded.pop(g.data_ptr(), None)  # (python attributes do not survive the trip through the engine: keyed on the address)
        if (base is not None and tuple(base.shape) == ctx.shape and base.dtype == g.dtype and base.stride() == g.stride()
                and tuple(g.shape) == (ctx.shape[0], g.shape[1]) + ctx.shape[2:]):
            return base, None
        full = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device).contiguous(memory_format=torch.channels_last) if len(ctx.shape) == 4 \
            else torch.zeros(ctx.shape, dtype=g.dtype, device=g.device)
        full[:, : g.shape[1]].copy_(g)
        return full, None


def padded_grad_like(t, zero=True):
    """a gradient buffer for tensor t: if t is the [:, :c] view of a channel-padded NHWC tensor (pixel stride ld > c), a buffer of the
    PADDED shape (see _ChanSlice.backward, which hands it through); else an empty tensor like t.  -> (tensor for the kernel, [:, :c] view
    to return to autograd).  zero=False: the kernel that fills it writes zeros into the padding channels itself."""
    if t.dim() == 4 and is_nhwc(t):
        ld = as_ymi(t).ld
        n, c, h, w = t.shape
        if ld != c and ld % chunk_elems(t.dtype) == 0 and ld - c < chunk_elems(t.dtype):
            base = empty_nhwc(n, ld, h, w, t.dtype, t.device)
            if zero:
                base.zero_()
            if len(RUN.padded) > 64:  # (gradients that never reached a _ChanSlice: do not keep their buffers alive)
                RUN.padded.clear()
            RUN.padded[base.data_ptr()] = base  # (until _ChanSlice.backward takes it)
            return base, base[:, :c]
    e = torch.empty_like(t)
    return e, e


def linear(x, weight, bias=None, residual=None):
    """token GEMM: x [T, Cin] @ weight[Cout, Cin]^T + bias (+ residual)."""
    return _ConvAffineAct.apply(x, weight, None, bias, 1, ACT_NONE, residual, weight.shape[0], join_of(x), join_of(residual) if residual is not None else None)
