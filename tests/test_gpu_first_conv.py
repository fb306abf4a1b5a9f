"""GPU: the direct first-layer kernel (csrc/first_conv.hip: 3x3 stride-2 convolution that reads the float32 NCHW image itself) against the
implicit-GEMM path on the same bfloat16 arithmetic - outputs, running statistics, parameter gradients - and against the
quantisation-matched oracle (the reference's Conv block with the product's storage roundings).  Through the C entry points: the image
copy the statistics pass leaves behind (x4) bit for bit, and the backward's two routes (its own slab sum, a deferred record summed by
ymi_wgrad_reduce_batch) against each other and against themselves."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


def _conv(cin, cout, seed):
    from improving_yolov8_cbam_swinblock_amd.nn.modules import Conv

    torch.manual_seed(seed)
    m = Conv(cin, cout, 3, 2).to(dev()).train()
    m.bn.eps, m.bn.momentum = 1e-3, 0.03
    m.bn.weight.data.uniform_(0.5, 1.5)
    m.bn.bias.data.uniform_(-0.5, 0.5)
    return m


def _count_direct_calls(monkeypatch):
    """calls of ops.first_conv_bn_act (the name nn/modules/conv.py looks up) from here on"""
    from improving_yolov8_cbam_swinblock_amd import ops

    calls = []
    inner = ops.first_conv_bn_act

    def counted(*a, **kw):
        calls.append(1)
        return inner(*a, **kw)

    monkeypatch.setattr(ops, "first_conv_bn_act", counted)
    return calls


def _run(m, img, direct, monkeypatch):
    from improving_yolov8_cbam_swinblock_amd import ops

    monkeypatch.setitem(ops.HOOKS, "first_conv", bool(direct))
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(img)
    (y.float() * torch.linspace(-1, 1, y.shape[1], device=y.device).view(1, -1, 1, 1)).sum().backward()
    torch.cuda.synchronize()
    return y.detach().float(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}, {n: b.detach().clone() for n, b in m.named_buffers()}


def _same_block(got, ref):
    # the same bfloat16 products in another float32 summation order: a few outputs land on the other side of a bfloat16 rounding
    assert rel(got[0], ref[0]) <= 2e-3, rel(got[0], ref[0])
    for k in ref[1]:
        assert rel(got[1][k], ref[1][k]) <= 5e-3, (k, rel(got[1][k], ref[1][k]))
    for k in ref[2]:
        if ref[2][k].dtype.is_floating_point:
            assert rel(got[2][k], ref[2][k]) <= 1e-4, (k, rel(got[2][k], ref[2][k]))
        else:
            assert torch.equal(got[2][k], ref[2][k])


# (3, 32, 1, 130, 188): Ho = 65 - nine tile rows, the last holds one row; Wo = 94 - two tile columns, the last 30 pixels wide
@pytest.mark.parametrize("cin,cout,n,h,w", [(3, 32, 2, 64, 256), (3, 16, 1, 40, 72), (3, 48, 2, 24, 136), (4, 64, 1, 16, 128), (1, 32, 3, 8, 8), (3, 32, 1, 130, 188)])
def test_first_conv_direct_matches_the_gemm_path(cin, cout, n, h, w, monkeypatch):
    from improving_yolov8_cbam_swinblock_amd import ops

    m = _conv(cin, cout, 0)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    img = torch.rand(n, cin, h, w, device=dev())
    calls = _count_direct_calls(monkeypatch)
    monkeypatch.setitem(ops.HOOKS, "first_conv", True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert ops.first_conv_ok(img, m.conv, None, None)
    ref = _run(m, img, False, monkeypatch)
    assert not calls, "the generic arm took the direct path"
    m.load_state_dict(state)
    got = _run(m, img, True, monkeypatch)
    assert len(calls) == 1, "the direct arm did not take the direct path"
    _same_block(got, ref)


def test_first_conv_refuses_a_width_that_is_no_multiple_of_4(monkeypatch):
    """w = 190: first_conv_ok is false with the hook on, and the module gives the generic path's result."""
    from improving_yolov8_cbam_swinblock_amd import ops

    m = _conv(3, 32, 0)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    img = torch.rand(1, 3, 130, 190, device=dev())
    calls = _count_direct_calls(monkeypatch)
    monkeypatch.setitem(ops.HOOKS, "first_conv", True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not ops.first_conv_ok(img, m.conv, None, None)
        assert ops.first_conv_ok(img[..., :188].contiguous(), m.conv, None, None)  # (the width alone refuses it)
    ref = _run(m, img, False, monkeypatch)
    m.load_state_dict(state)
    got = _run(m, img, True, monkeypatch)
    assert not calls
    _same_block(got, ref)


def test_first_conv_direct_vs_matched_oracle(monkeypatch):
    """against the CPU oracle with the product's storage roundings (oracle/quant.py): forward / BatchNorm gradients 1e-3, weight gradient
    4e-3 - the bounds of tests/test_gpu_bf16_matched.py for Conv blocks."""
    import oracle.modules as OM
    from oracle import quant
    from improving_yolov8_cbam_swinblock_amd.nn.modules import Conv

    torch.manual_seed(11)
    o = OM.Conv(3, 32, 3, 2)
    o.bn.eps, o.bn.momentum = 1e-3, 0.03
    o.bn.weight.data.uniform_(0.5, 1.5)
    o.bn.bias.data.normal_(0, 0.3)
    quant.round_weights_(o)
    m = Conv(3, 32, 3, 2)
    m.bn.eps, m.bn.momentum = 1e-3, 0.03
    m.load_state_dict(o.state_dict())
    m = m.to(dev()).train()
    o.train()
    x = torch.rand(2, 3, 96, 160).bfloat16().float()
    gy = torch.randn(2, 32, 48, 80).bfloat16().float()
    with quant.storage(torch.bfloat16):
        yo = o(x)
        go = torch.autograd.grad(yo, list(o.parameters()), gy)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yg = m(x.to(dev()))
    gg = torch.autograd.grad(yg, list(m.parameters()), gy.to(dev()).to(yg.dtype))
    errs = {"fwd": rel(yg, yo)}
    for a, b, n in zip(gg, go, ["w", "gamma", "beta"]):
        errs[n] = rel(a, b)
    print("\n[matched first conv] " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert all(e <= (4e-3 if n == "w" else 1e-3) for n, e in errs.items()), errs


# ---- through the C entry points ------------------------------------------------------------------------------------------------------------
def _forward(c, cout, n, h, w, seed):
    """ymi_first_conv_bn_act_fwd on seeded inputs; x4 and out hold a sentinel before the call."""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd._lib import as_ymi, check, lib as L, ptr, stream_ptr

    g = torch.Generator().manual_seed(seed)
    t = {"img": torch.rand(n, c, h, w, generator=g).to(dev()), "w": (torch.randn(cout, c, 3, 3, generator=g) * 0.2).to(dev()),
         "gamma": (torch.rand(cout, generator=g) + 0.5).to(dev()), "beta": (torch.rand(cout, generator=g) - 0.5).to(dev()),
         "rmean": torch.zeros(cout, device=dev()), "rvar": torch.ones(cout, device=dev()), "stats": torch.empty(2, cout, device=dev())}
    t["x4"] = torch.full((n, h, w, 4), -3.0, dtype=torch.bfloat16, device=dev()).permute(0, 3, 1, 2)
    t["out"] = torch.full((n, h // 2, w // 2, cout), -3.0, dtype=torch.bfloat16, device=dev()).permute(0, 3, 1, 2)
    need = (2 * cout + (L().ymi_first_conv_stat_blocks(n, h, w) + 64) * 2 * cout) * 4
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    check(L().ymi_first_conv_bn_act_fwd(ptr(t["img"]), n, c, h, w, ptr(t["w"]), cout, ptr(t["gamma"]), ptr(t["beta"]), ptr(t["rmean"]), ptr(t["rvar"]), 0.03, 1e-3,
                                        ops.ACT_SILU, ctypes.byref(as_ymi(t["x4"])), ctypes.byref(as_ymi(t["out"])), ptr(t["stats"][0]), ptr(t["stats"][1]),
                                        ptr(ws), ws.numel(), stream_ptr()), "first_conv_bn_act_fwd")
    torch.cuda.synchronize()
    return t


# (1, 3, 8, 8): smaller than a tile, halo outside the image on all sides; (3, 1, 18, 132): 2 x 2 tiles, the last tile row holds one output
# row, the last tile column two pixels; (4, 1, 16, 128): exactly one tile, on the fourth-channel path
@pytest.mark.parametrize("c,n,h,w", [(1, 3, 8, 8), (3, 1, 18, 132), (4, 1, 16, 128)])
def test_first_conv_image_copy_is_bit_exact(c, n, h, w):
    """x4 = the image rounded to bfloat16, NHWC, the unused channels zero, every pixel written."""
    t = _forward(c, 16, n, h, w, 5)
    want = torch.zeros(n, h, w, 4, dtype=torch.bfloat16, device=dev())
    want[..., :c] = t["img"].to(torch.bfloat16).permute(0, 2, 3, 1)
    got = t["x4"].permute(0, 2, 3, 1).contiguous()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())
    assert bool((got[..., c:].view(torch.int16) == 0).all())


def _backward(t, c, cout, dout, deferred):
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd._lib import WgradPending, as_ymi, check, lib as L, ptr, stream_ptr

    n, _, h, w = t["x4"].shape
    dw = torch.full((cout, c, 3, 3), float("nan"), device=dev())
    dgamma = torch.full((cout,), float("nan"), device=dev())
    dbeta = torch.full((cout,), float("nan"), device=dev())
    ws = torch.empty(int(L().ymi_first_conv_bwd_workspace(n, h, w, cout)), dtype=torch.uint8, device=dev())
    rec = WgradPending()
    check(L().ymi_first_conv_bn_act_bwd(ctypes.byref(as_ymi(t["x4"])), ptr(t["w"]), c, cout, ptr(t["gamma"]), ptr(t["beta"]), ptr(t["stats"][0]), ptr(t["stats"][1]),
                                        ops.ACT_SILU, ctypes.byref(as_ymi(dout)), ptr(dgamma), ptr(dbeta), ptr(dw), ptr(ws), ws.numel(),
                                        ctypes.byref(rec) if deferred else None, stream_ptr()), "first_conv_bn_act_bwd")
    if deferred:
        table = torch.empty(ctypes.sizeof(WgradPending), dtype=torch.uint8, device=dev())
        check(L().ymi_wgrad_reduce_batch((WgradPending * 1)(rec), 1, ptr(table), stream_ptr()), "wgrad_reduce_batch")
    torch.cuda.synchronize()
    return dw, dgamma, dbeta


# (3, 16, 1, 40, 72): 3 tiles in one workgroup, which stops early; (3, 32, 2, 48, 132): 12 tiles, three full workgroups;
# (3, 64, 1, 16, 640): 5 tiles, the second workgroup holds one
@pytest.mark.parametrize("c,cout,n,h,w", [(3, 16, 1, 40, 72), (3, 32, 2, 48, 132), (3, 64, 1, 16, 640)])
def test_first_conv_backward_routes_agree_bit_for_bit(c, cout, n, h, w):
    """dW, dgamma, dbeta: the entry point's own slab sum and a deferred record summed by ymi_wgrad_reduce_batch give the same bits, and
    each route repeats itself."""
    t = _forward(c, cout, n, h, w, 7)
    g = torch.Generator().manual_seed(8)
    dout = torch.randn(n, h // 2, w // 2, cout, generator=g).to(device=dev(), dtype=torch.bfloat16).permute(0, 3, 1, 2)
    own = [_backward(t, c, cout, dout, False) for _ in range(2)]
    rec = [_backward(t, c, cout, dout, True) for _ in range(2)]
    for name, a, a2, b, b2 in zip(("dW", "dgamma", "dbeta"), own[0], own[1], rec[0], rec[1]):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, a2), name + ": the direct route does not repeat itself"
        assert torch.equal(b, b2), name + ": the deferred route does not repeat itself"
        assert torch.equal(a, b), name + ": the two routes differ"
