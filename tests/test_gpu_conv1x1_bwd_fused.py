"""The fused backward of a 1x1 stride-1 Conv block (csrc/wgrad.hip: conv1x1_bwd_kernel behind ymi_conv1x1_bn_act_bwd): BatchNorm apply, data
gradient and weight gradient in one kernel, against float64 host references of autograd's backward of Conv.forward (nn/modules/conv.py:69-79).

  placement  small-integer operands through the C ABI, activation none, statistics chosen so that the apply coefficients are (c0, c1, c2) =
             (1, 0, 0) or (1, 1, a per-channel integer) and draw is an integer: dx and dW must equal float64 bit for bit (gemm_exact Gate 1).
             How the coefficients come about: gamma = 1, beta = 0, mean = 0, invstd = 1 make c0 = 1, c1 = sum(dout raw) / P and
             c2 = sum(dout) / P.  The operands start from an integer tensor d whose pixels cancel, per channel, inside the raw = +1 and inside
             the raw = -1 group (sum d = sum d raw = 0); dout = d + c2 + c1 raw then has exactly the wanted sums and draw = dout - c1 raw - c2 = d.
  precision  SiLU and real coefficients: float64 products of the library's own draw (ymi_bn_act_bwd), Gate 2's derived bound; the three-launch
             path is held to the same bound beside it.
  modules    C2f blocks forward and backward with the hook on and off; a captured training step against eager steps.
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_exact as gx
from improving_yolov8_cbam_swinblock_amd import _lib, ops
from improving_yolov8_cbam_swinblock_amd._lib import ACT_NONE, ACT_SILU, as_ymi, check, ptr, stream_ptr
from improving_yolov8_cbam_swinblock_amd.ops import weights as W
from improving_yolov8_cbam_swinblock_amd.ops.base import HOOKS

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENTINEL = 77.0


def dev():
    return torch.device("cuda:0")


def _ref(t):
    return ctypes.byref(as_ymi(t)) if t is not None else None


def nhwc(t):
    """host NCHW float tensor -> device bfloat16, NHWC memory, dense."""
    return t.to(dev()).to(BF).contiguous(memory_format=torch.channels_last)


def in_slice(t, ld, lo):
    """-> (view, buffer): t's values as channels [lo, lo + c) of a [n + 2, h, w, ld] buffer of sentinels - guard images before and after the
    tensor's pixels, guard channels on both sides of every pixel."""
    n, c, h, w = t.shape
    buf = torch.full((n + 2, h, w, ld), SENTINEL, dtype=BF, device=dev())
    view = buf[1 : n + 1, :, :, lo : lo + c].permute(0, 3, 1, 2)
    view.copy_(t)
    return view, buf


def guards_intact(buf, c, lo):
    g = buf.clone()
    g[1:-1, :, :, lo : lo + c] = SENTINEL
    return bool((g == SENTINEL).all())


def fused(dout, raw, gamma, mean, inv, beta, act, x, weight, adds, dx, pending):
    """ymi_conv1x1_bn_act_bwd -> (dgamma, dbeta, dw); dx is written in place."""
    L = _lib.lib()
    o, i = weight.shape[:2]
    ty, tx = as_ymi(dout), as_ymi(x)
    a1 = _ref(adds[0]) if len(adds) > 0 else None
    a2 = _ref(adds[1]) if len(adds) > 1 else None
    assert L.ymi_conv1x1_bn_act_bwd_ok(_ref(dout), _ref(raw), _ref(x), a1, a2, _ref(dx)) == 1
    wd = W.pack_conv_dgrad(weight, o, 1, BF)
    m = ty.n * ty.h * ty.w
    ws = torch.empty(int(L.ymi_conv1x1_bn_act_bwd_workspace(m, o, i)), dtype=torch.uint8, device=dev())
    dgamma, dbeta = torch.empty(o, device=dev()), torch.empty(o, device=dev())
    dw = torch.full((o, i, 1, 1), float("nan"), device=dev())
    rec = _lib.WgradPending() if pending else None
    check(L.ymi_conv1x1_bn_act_bwd(_ref(dout), _ref(raw), ptr(gamma), ptr(mean), ptr(inv), ptr(beta), act, _ref(x), ptr(wd), a1, a2, _ref(dx), ptr(dgamma), ptr(dbeta),
                                   ptr(dw), ptr(ws), ws.numel(), ctypes.byref(rec) if pending else None, stream_ptr()), "conv1x1_bn_act_bwd")
    if pending:
        tab = torch.empty(8 * ctypes.sizeof(_lib.WgradPending), dtype=torch.uint8, device=dev())
        check(L.ymi_wgrad_reduce_batch((_lib.WgradPending * 1)(rec), 1, ptr(tab), stream_ptr()), "wgrad_reduce_batch")
    torch.cuda.synchronize()
    return dgamma, dbeta, dw


def three_launches(dout, raw, gamma, mean, inv, beta, act, x, weight, adds):
    """the path the fused kernel replaces -> (draw, dx, dw, dgamma, dbeta)."""
    L = _lib.lib()
    o, i = weight.shape[:2]
    draw = _lib.empty_nhwc(*raw.shape, BF, dev())
    dgamma, dbeta = torch.empty(o, device=dev()), torch.empty(o, device=dev())
    ws = torch.empty(2048 * 2 * o * 4 + 256, dtype=torch.uint8, device=dev())
    check(L.ymi_bn_act_bwd(_ref(dout), _ref(raw), ptr(gamma), ptr(mean), ptr(inv), ptr(beta), act, _ref(draw), ptr(dgamma), ptr(dbeta), ptr(ws), ws.numel(),
                           stream_ptr()), "bn_act_bwd")
    dx = _lib.empty_nhwc(*x.shape, BF, dev())
    wd = W.pack_conv_dgrad(weight, o, 1, BF)
    check(L.ymi_conv2d_bwd_data_add(_ref(draw), ptr(wd), i, 1, 1, 1, _ref(adds[0]) if len(adds) > 0 else None, _ref(adds[1]) if len(adds) > 1 else None, _ref(dx),
                                    stream_ptr()), "conv2d_bwd_data_add")
    dw, _ = W._wgrad(x, draw, o, i, 1, 1, False)
    torch.cuda.synchronize()
    return draw, dx, dw, dgamma, dbeta


def cancelling(gen, p, c, groups):
    """[p, c] small integers whose sum over the pixels of every group (groups: [p] of 0 / 1, the same for every channel) is zero per channel:
    random values and their negatives (and a zero in an odd group), in a per-channel random order."""
    out = torch.zeros(p, c)
    for g in (0, 1):
        idx = torch.nonzero(groups == g).flatten()
        n = idx.numel()
        half = gx.ints((n // 2, c), gen, -2, 2)
        vals = torch.cat([half, -half, torch.zeros(n % 2, c)], 0)
        order = torch.argsort(torch.rand(n, c, generator=gen), dim=0)
        out[idx] = torch.gather(vals, 0, order)
    return out


SHAPES = [(2, 5, 7), (2, 24, 24)]  # 70 pixels: not a multiple of 32, one split; 1152: several splits with a ragged last one


@pytest.mark.parametrize("pending", [False, True], ids=["immediate", "pending"])
@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("nadd", [0, 1, 2])
@pytest.mark.parametrize("c1", [0, 1], ids=["c=100", "c=11k"])
@pytest.mark.parametrize("cin", [64, 96, 192, 256])
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("shape", SHAPES, ids=["70px", "1152px"])
def test_placement_exact(shape, cout, cin, c1, nadd, sliced, pending):
    n, h, w = shape
    p = n * h * w
    gen = torch.Generator().manual_seed(1000 * cout + 10 * cin + 4 * nadd + 2 * c1 + p)
    # the float32 final pass must land on the intended coefficients: sum / P with P's float32 reciprocal
    ic = np.float32(1.0) / np.float32(p)
    assert np.float32(p) * ic == 1.0 and all(np.float32(p * k) * ic == k for k in (-2, -1, 1, 2))
    groups = (torch.randperm(p, generator=gen) % 2)
    d = cancelling(gen, p, cout, groups)  # = draw
    if c1:  # raw = +1 / -1 by group: raw^2 = 1 and sum raw = 0 (the groups are equally large)
        assert p % 2 == 0
        rawv = (1.0 - 2.0 * groups.float())[:, None].expand(p, cout)
    else:  # any raw that is constant inside a group keeps sum(dout raw) = 0: a per-channel integer for each group
        rawv = torch.where(groups[:, None] == 0, gx.ints((1, cout), gen, -2, 2), gx.ints((1, cout), gen, -2, 2))
    c2 = gx.ints((cout,), gen, -2, 2) if c1 else torch.zeros(cout)
    doutv = d + c2[None, :] + (rawv if c1 else 0.0)
    to4 = lambda t, c: t.reshape(n, h, w, c).permute(0, 3, 1, 2)
    dout_h, raw_h, draw_h = to4(doutv, cout), to4(rawv, cout), to4(d, cout)
    x_h = gx.ints((n, cin, h, w), gen, -2, 2, density=0.5, nonzero=False)
    w_h = gx.ints((cout, cin, 1, 1), gen, -1, 1, density=0.25, nonzero=False)
    adds_h = [gx.ints((n, cin, h, w), gen, -3, 3, nonzero=False) for _ in range(nadd)]
    dx_ref = gx.dgrad64(draw_h, w_h, x_h.shape, 1) + sum(a.double() for a in adds_h)
    dx_mag = gx.dgrad_mag(draw_h, w_h, x_h.shape, 1) + sum(a.double().abs() for a in adds_h)
    dw_ref, dw_mag = gx.wgrad64(x_h, draw_h, w_h.shape, 1), gx.wgrad_mag(x_h, draw_h, w_h.shape, 1)
    _, splits, slab_bf16, _ = gx.wgrad_plan(p, cout, cin, True)
    dx_exp = gx.exact_expected(dx_ref, dx_mag, BF, what="dx")
    dw_exp = gx.exact_expected(dw_ref, dw_mag, torch.float32, slab_bf16=slab_bf16, what="dW")

    x = nhwc(x_h)
    bufs = {}
    if sliced:
        dout, bufs["dout"] = in_slice(nhwc(dout_h), cout + 64, 32)
        dx, bufs["dx"] = in_slice(torch.full(x_h.shape, SENTINEL), cin + 40, 24)
    else:
        dout = nhwc(dout_h)
        dx = nhwc(torch.full(x_h.shape, SENTINEL))
    raw = nhwc(raw_h)
    adds = [nhwc(a) for a in adds_h]
    if nadd:  # the last addend IS dx
        dx.copy_(adds[-1])
        adds[-1] = dx
    weight = w_h.to(dev())
    ones, zeros = torch.ones(cout, device=dev()), torch.zeros(cout, device=dev())
    dgamma, dbeta, dw = fused(dout, raw, ones, zeros, ones, zeros, ACT_NONE, x, weight, adds, dx, pending)
    assert float((dbeta.cpu() - p * c2).abs().max()) == 0.0 and float((dgamma.cpu() - (p if c1 else 0)).abs().max()) == 0.0, "the statistics the case is built on"
    gx.check_exact(f"dx {shape} {cin}->{cout} splits {splits}", dx, dx_exp)
    gx.check_exact(f"dW {shape} {cin}->{cout} splits {splits}", dw, dw_exp)
    if sliced:
        assert guards_intact(bufs["dx"], cin, 24), "bytes around dx's slice changed"
        assert guards_intact(bufs["dout"], cout, 32), "bytes around dout's slice changed"


def real_case(n, h, w, cin, cout, seed):
    gen = torch.Generator().manual_seed(seed)
    raw_h = torch.randn(n, cout, h, w, generator=gen)
    dout_h = torch.randn(n, cout, h, w, generator=gen)
    x_h = torch.randn(n, cin, h, w, generator=gen)
    w_h = torch.randn(cout, cin, 1, 1, generator=gen) * cin ** -0.5
    gamma = (0.5 + torch.rand(cout, generator=gen)).to(dev())
    beta = (0.2 * torch.randn(cout, generator=gen)).to(dev())
    raw = nhwc(raw_h)
    r = raw.float()
    mean = r.mean((0, 2, 3))
    inv = (r.var((0, 2, 3), unbiased=False) + 1e-3).rsqrt()
    return nhwc(dout_h), raw, nhwc(x_h), w_h.to(dev()), gamma, beta, mean.contiguous(), inv.contiguous(), gen


# (n, h, w, cin, cout): float32 slabs (5 splits); bfloat16 slabs (4096 pixels at 128 channels: 16 splits)
PRECISION = [(2, 24, 24, 96, 64), (2, 24, 24, 256, 128), (4, 32, 32, 128, 128)]


@pytest.mark.parametrize("nadd", [0, 2])
@pytest.mark.parametrize("n,h,w,cin,cout", PRECISION)
def test_precision_silu(n, h, w, cin, cout, nadd):
    dout, raw, x, weight, gamma, beta, mean, inv, gen = real_case(n, h, w, cin, cout, 7 * cin + cout + nadd)
    adds = [nhwc(torch.randn(n, cin, h, w, generator=gen)) for _ in range(nadd)]
    draw, dx3, dw3, dgamma3, dbeta3 = three_launches(dout, raw, gamma, mean, inv, beta, ACT_SILU, x, weight, adds)
    dx = _lib.empty_nhwc(n, cin, h, w, BF, dev())
    dgamma, dbeta, dw = fused(dout, raw, gamma, mean, inv, beta, ACT_SILU, x, weight, adds, dx, False)
    assert torch.equal(dgamma, dgamma3) and torch.equal(dbeta, dbeta3), "the same reduce and final pass"
    p = n * h * w
    wb = weight.to(BF)  # the packed operand's values
    dx_ref = gx.dgrad64(draw, wb, x.shape, 1) + sum(a.double().cpu() for a in adds)
    dx_mag = gx.dgrad_mag(draw, wb, x.shape, 1) + sum(a.double().cpu().abs() for a in adds)
    dx_bound = gx.bound_plain(dx_ref, dx_mag, cout + nadd, BF)
    dw_ref, dw_mag = gx.wgrad64(x, draw, weight.shape, 1), gx.wgrad_mag(x, draw, weight.shape, 1)
    _, splits, slab_bf16, _ = gx.wgrad_plan(p, cout, cin, True)
    assert slab_bf16 == (p >= 4096)
    dw_bound = gx.bound_plain(dw_ref, dw_mag, p, torch.float32) + (gx.R_BF16 * dw_mag if slab_bf16 else 0.0)  # one more rounding of each split partial
    worst = {}
    for name, gdx, gdw in (("fused", dx, dw), ("three launches", dx3, dw3)):
        worst[name] = (gx.check_bound(f"dx {name}", gdx, dx_ref, dx_bound), gx.check_bound(f"dW {name}", gdw, dw_ref, dw_bound))
    print(f"\n[conv1x1 bwd {cin}->{cout} {p} px, {splits} splits, {nadd} addends] worst err / bound (dx, dW): {worst}")


@pytest.mark.parametrize("act", [ACT_SILU, ACT_NONE])
@pytest.mark.parametrize("c", [64, 128])
def test_draw_bits_are_the_apply_pass(c, act):
    """with W = identity every dx element is one draw element: the kernel's bfloat16 draw must be the words ymi_bn_act_bwd writes."""
    dout, raw, x, _, gamma, beta, mean, inv, _ = real_case(2, 9, 11, c, c, 31 + c)
    weight = torch.eye(c, device=dev()).reshape(c, c, 1, 1).contiguous()
    draw, _, _, _, _ = three_launches(dout, raw, gamma, mean, inv, beta, act, x, weight, [])
    dx = _lib.empty_nhwc(*x.shape, BF, dev())
    fused(dout, raw, gamma, mean, inv, beta, act, x, weight, [], dx, False)
    assert torch.equal(dx.view(torch.int16), draw.view(torch.int16))


def test_scope_query():
    L = _lib.lib()
    t = lambda c, dt=BF: _lib.empty_nhwc(2, c, 8, 8, dt, dev())
    ok = lambda dout, raw, x, dx: L.ymi_conv1x1_bn_act_bwd_ok(_ref(dout), _ref(raw), _ref(x), None, None, _ref(dx))
    assert ok(t(64), t(64), t(96), t(96)) == 1 and ok(t(128), t(128), t(512), t(512)) == 1
    assert ok(t(256), t(256), t(64), t(64)) == 0   # output channels
    assert ok(t(64), t(64), t(520), t(520)) == 0   # input channels
    assert ok(t(64, torch.float32), t(64, torch.float32), t(64, torch.float32), t(64, torch.float32)) == 0
    assert ok(t(64), t(64), t(96), t(64)) == 0     # dx is x's shape


# ---- module level ----------------------------------------------------------------------------------------------------------------------------
def _c2f_grads(args, shape, hook, seed):
    import improving_yolov8_cbam_swinblock_amd.nn.modules as PM

    torch.manual_seed(seed)
    m = PM.C2f(*args)
    for b in m.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.eps, b.momentum = 1e-3, 0.03
            b.weight.data.uniform_(0.5, 1.5)
            b.bias.data.normal_(0, 0.3)
    m = m.to(dev()).train()
    x = torch.randn(*shape).bfloat16().float().to(dev()).requires_grad_(True)
    calls = []
    orig = ops.conv._conv1x1_bwd_fused
    ops.conv._conv1x1_bwd_fused = lambda *a: calls.append(1) or orig(*a)
    HOOKS["fused_bwd_1x1"] = hook
    try:
        with torch.autocast("cuda", dtype=BF):
            y = m(x)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 1)).to(dev()).to(y.dtype)
        g = torch.autograd.grad(y, [x] + list(m.parameters()), gy)
    finally:
        HOOKS["fused_bwd_1x1"] = True
        ops.conv._conv1x1_bwd_fused = orig
    torch.cuda.synchronize()
    return y, dict(zip(["x"] + [n for n, _ in m.named_parameters()], g)), len(calls)


@pytest.mark.parametrize("args,shape,routed", [((64, 64, 1, True), (2, 64, 24, 20), 2), ((128, 128, 2, True), (2, 128, 24, 20), 1)], ids=["C2f(64)", "C2f(128)"])
def test_c2f_hook_on_and_off(args, shape, routed):
    """C2f forward and backward with the fused kernel (cv1 and cv2 are its 1x1 blocks: 64->64 / 96->64, 128->128 / 256->128; the routing rule of
    ops/conv.py sends blocks of up to 128 input channels to it, so 256->128 keeps the three launches on both sides) and with the three launches.  Every gradient agrees within test_gpu_bf16_matched.py's bounds - 1e-3, 2e-3 on convolution weights.  cv2 is the first block of
    the backward pass, so its dout is the same tensor on both paths and its dgamma / dbeta - the same reduce and final pass - are bit-identical;
    the blocks behind it see a dout that went through a differently ordered sum."""
    y1, on, n_on = _c2f_grads(args, shape, True, 3)
    y0, off, n_off = _c2f_grads(args, shape, False, 3)
    assert n_on == routed and n_off == 0
    assert torch.equal(y1, y0)
    assert torch.equal(on["cv2.bn.weight"], off["cv2.bn.weight"]) and torch.equal(on["cv2.bn.bias"], off["cv2.bn.bias"])
    errs = {n: gx.rel(on[n], off[n]) for n in on}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print(f"\n[C2f{args} hook on vs off] worst " + " ".join(f"{n} {e:.2e}" for n, e in worst))
    for n, e in errs.items():
        assert e <= (2e-3 if n.endswith("conv.weight") else 1e-3), (n, e)


# ---- captured step ---------------------------------------------------------------------------------------------------------------------------
def _steps(graph, hook, count):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    calls = []
    orig = ops.conv._conv1x1_bwd_fused
    ops.conv._conv1x1_bwd_fused = lambda *a: calls.append(1) or orig(*a)
    HOOKS["fused_bwd_1x1"] = hook
    try:
        torch.manual_seed(0)
        model = DetectionModel("yolov8s.yaml", ch=3, nc=1).to(dev())
        step = TrainStep(model, world_size=1, lr=0.01, graph=graph)
        batch = synthetic_batch(2, 128, dev(), 1)
        losses = torch.stack([step(batch).float().cpu().clone() for _ in range(count)])
        torch.cuda.synchronize()
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    finally:
        HOOKS["fused_bwd_1x1"] = True
        ops.conv._conv1x1_bwd_fused = orig
    del step, model
    return losses, state, len(calls)


def test_captured_step_equals_eager_steps():
    """TrainStep(graph=True) on yolov8s, two images of 128 x 128, hook on: graph mode runs 3 eager warm-up steps before its first replay, so
    replay i is eager step i + 3 - three replays equal eager steps 3..5 bit for bit, loss items and model state.  With the hook off no fused
    launch is made (the parent's path) and the step stays beside the fused one."""
    le, se, ne = _steps(False, True, 6)
    lg, sg, ng = _steps(True, True, 3)
    assert ne > 0 and ng > 0, "the fused path was not taken"
    dl = float((lg - le[3:6]).abs().max())
    ds = max(float((sg[k].double() - se[k].double()).abs().max()) for k in se)
    print(f"\n[captured vs eager, hook on] max |loss diff| {dl:.3e}, max |state diff| {ds:.3e}")
    assert torch.equal(lg, le[3:6]), (lg, le[3:6])
    assert all(torch.equal(sg[k], se[k]) for k in se), [k for k in se if not torch.equal(sg[k], se[k])][:5]
    l0, s0, n0 = _steps(True, False, 3)
    assert n0 == 0
    torch.testing.assert_close(l0, lg, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("n,h,w,cin,cout", [(4, 32, 32, 128, 128), (2, 24, 24, 96, 64), (2, 9, 11, 64, 64), (8, 40, 24, 64, 64)],
                         ids=["patch-bf16slabs", "patch-f32slabs", "raster", "patch-8x4-bf16slabs"])
def test_dw_equals_the_three_launches_bit_for_bit(n, h, w, cin, cout):
    """the fused kernel sums a split's pixels in wgrad_kernel's order (patch order where the map tiles, raster order elsewhere) with the same
    MFMA sequence on the same bfloat16 draw, so every split partial, every rounded slab and dW itself equal the three launches' words: a
    training step moves by the data gradient's rounding at most, not by re-ordered weight-gradient sums."""
    dout, raw, x, weight, gamma, beta, mean, inv, _ = real_case(n, h, w, cin, cout, 5 * cin + cout + h)
    _, dx3, dw3, _, _ = three_launches(dout, raw, gamma, mean, inv, beta, ACT_SILU, x, weight, [])
    dx = _lib.empty_nhwc(n, cin, h, w, BF, dev())
    _, _, dw = fused(dout, raw, gamma, mean, inv, beta, ACT_SILU, x, weight, [], dx, False)  # (the per-launch slab sum on both sides)
    print(f"\n[{n}x{h}x{w} {cin}->{cout}] dx words that differ from the data-gradient GEMM's: {int((dx.view(torch.int16) != dx3.view(torch.int16)).sum())} of {dx.numel()}")
    assert torch.equal(dw, dw3)
