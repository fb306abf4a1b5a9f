"""The OBB head and its two kernels on the GPU: the head against the reference's own outputs (tests/golden/obb_head_nc3.npz, written by
tests/golden/make_obb_golden.py) at the bounds test_gpu_seg_modules.py uses for the Segment head; ymi_obb_angle_fwd / _bwd and
ymi_detect_decode_obb per element against float64 (tests/obb_ref.py)."""
import pytest
import torch

import obb_ref as R
from conftest import golden_state, load_golden
from obb_common import CH, HEAD_SEED, NC, NE, STRIDE, head_inputs, loss_case
from psa_common import seeded_module_state
from test_gpu_modules_golden import BF16_TOL, F32_TOL, P, close, dev, run, set_bn, t
from test_gpu_psa_modules import _close_param_grads, _fuse

pytestmark = pytest.mark.gpu
A96 = 189  # anchors of a 96 x 96 image: 144 + 36 + 9


def _head():
    m = P().OBB(NC, NE, CH)
    set_bn(m)
    m.stride = torch.tensor(STRIDE)
    m.load_state_dict(seeded_module_state(m, HEAD_SEED), strict=True)
    m = m.to(dev())
    m.stride = m.stride.to(dev())
    return m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_obb_head_vs_reference(dtype):
    """OBB(3, 1, (32, 64, 128)): train output (feats, angle), gradients of the three inputs and of every parameter, running statistics, the
    decoded eval output [B, 4 + nc + 1, A] before and after fuse(), and the split form the loss reads."""
    m = _head()
    d = load_golden("obb_head_nc3")
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    gtol = dict(atol=tol["atol"] * 2, rtol=0)
    xs, gys, ga = head_inputs()
    xs = [x.to(dev()).requires_grad_(True) for x in xs]
    state = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    feats, angle = run(m, list(xs), dtype)
    for i, y in enumerate(feats):
        close(y, t(d[f"y_train{i}"]), tol, f"obb train map {i}")
    close(angle, t(d["angle"]), tol, "obb angle")
    assert angle.shape == (2, NE, A96) and angle.dtype == torch.float32
    params = [q for q in m.parameters() if q.requires_grad]
    names = [n for n, q in m.named_parameters() if q.requires_grad]
    outs = list(feats) + [angle]
    gouts = [g.to(dev()).to(y.dtype) for g, y in zip(gys + [ga], outs)]
    gs = torch.autograd.grad(outs, xs + params, gouts, allow_unused=True)
    for i in range(len(xs)):
        close(gs[i], t(d[f"g.x{i}"]), gtol, f"obb grad x{i}")
    _close_param_grads(d, names, gs[len(xs):], gtol, "obb")
    sd = m.state_dict()
    for k, v in golden_state(d, "after.").items():
        close(sd[k].float(), v.float(), tol, f"obb running stat {k}")
    m.load_state_dict(state, strict=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        sp = m.forward_split(list(xs))
    assert torch.equal(sp.angle.detach(), angle.detach())
    for i in range(3):
        assert torch.equal(torch.cat([sp.box[i].detach(), sp.cls[i].detach()], 1).float(), feats[i].detach().float())
    m.eval()
    with torch.no_grad():
        y, (feats_e, angle_e) = run(m, [x.detach() for x in xs], dtype)
        assert y.shape == (2, 4 + NC + NE, A96) and y.dtype == torch.float32
        close(y, t(d["y_eval"]), tol, "obb decoded eval output")
        close(angle_e, t(d["angle_eval"]), tol, "obb eval angle")
        assert torch.equal(y[:, 4 + NC:], angle_e)  # the angle row is a copy
        _fuse(m)
        close(run(m, [x.detach() for x in xs], dtype)[0], t(d["y_fused"]), tol, "obb decoded eval output after fuse")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
def test_obb_angle_kernels_per_element(dtype, padded):
    """one-channel logit maps of four odd levels (more than one workgroup: 17 * 19 = 323 anchors on the first), dense or the [:, :1] view of an
    8-channel buffer: the forward within four float32 roundings of (sigmoid(x) - 0.25) * pi in float64 on the stored logits, the backward
    within those plus the stored gradient's own rounding; padding channels of the gradient buffer exact zeros"""
    from improving_yolov8_cbam_swinblock_amd import ops

    g = torch.Generator().manual_seed(7)
    shapes = [(17, 19), (9, 5), (3, 2), (1, 1)]
    B = 3
    logits = []
    for h, w in shapes:
        v = (torch.randn(B, 8 if padded else 1, h, w, generator=g) * 3).to(dev()).to(dtype).contiguous(memory_format=torch.channels_last)
        logits.append((v[:, :1] if padded else v).requires_grad_(True))
    A = sum(h * w for h, w in shapes)
    angle = ops.obb_angle(logits)
    assert angle.shape == (B, 1, A) and angle.dtype == torch.float32
    x64 = [v.detach().double().cpu().requires_grad_(True) for v in logits]
    want = R.angle_of(x64)
    eps = 2.0 ** -24
    assert float((angle.detach().cpu().double() - want.detach()).abs().max()) <= 4 * eps * 3.2
    ga = torch.randn(B, 1, A, generator=g)
    gs = torch.autograd.grad(angle, logits, ga.to(dev()))
    ws = torch.autograd.grad(want, x64, ga.double())
    store = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    assert all(got.shape == w_.shape and got.dtype == dtype for got, w_ in zip(gs, ws))
    got = torch.cat([v.detach().cpu().double().reshape(B, 1, -1) for v in gs], 2)
    ref = torch.cat([v.reshape(B, 1, -1) for v in ws], 2)
    # s carries one float32 rounding, so s * (1 - s) is off by up to 2^-24 in absolute terms (times |dangle| * pi); the products and the
    # stored value add relative roundings
    assert bool(((got - ref).abs() <= (8 * eps + store) * ref.abs() + ga.double().abs() * 3.2 * 2 * eps).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_obb_angle_bwd_zeroes_padding_channels(dtype):
    import ctypes

    from improving_yolov8_cbam_swinblock_amd import _lib

    B, h, w = 2, 5, 7
    x = torch.randn(B, 8, h, w, device=dev()).to(dtype).contiguous(memory_format=torch.channels_last)
    dx = torch.full((B, 8, h, w), 7.0, device=dev()).to(dtype).contiguous(memory_format=torch.channels_last)
    da = torch.randn(B, 1, h * w, device=dev())
    arr = lambda ts: (_lib.YmiTensor * len(ts))(*[_lib.as_ymi(v) for v in ts])  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().ymi_obb_angle_bwd(1, arr([x[:, :1]]), ctypes.c_void_p(da.data_ptr()), arr([dx]), stream), "obb_angle_bwd")
    torch.cuda.synchronize()
    assert (dx[:, 1:] == 0).all() and (dx[:, 0] != 7.0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["obb_loss_rect", "obb_loss_four"])
def test_detect_decode_obb_per_element(name, dtype):
    """box rows at the bound of the loss's decode stage (pb), scores within four float32 roundings, the angle row a copy"""
    from improving_yolov8_cbam_swinblock_amd import ops

    c = loss_case(name)
    feats = [v.to(dev()).to(dtype) for v in c["feats"]]
    box = [v[:, :64].contiguous(memory_format=torch.channels_last) for v in feats]
    cls = [v[:, 64:].contiguous(memory_format=torch.channels_last) for v in feats]
    angle = c["angle"].to(dev())
    y = ops.detect_decode_obb(box, cls, angle, list(c["strides"])).cpu()
    want = R.eval_output(c, feats=[v.float().cpu() for v in feats])
    nc = c["nc"]
    assert y.shape == (c["B"], 4 + nc + 1, c["A"])
    err = R.scaled_err(y[:, :4], want[:, :4])
    print(name, "box rows", err)
    assert err <= max(R.KERNEL_FACTOR * R.REF32_DISTANCE["pb"], 1e-6)
    assert float((y[:, 4: 4 + nc].double() - want[:, 4: 4 + nc]).abs().max()) <= 4 * 2.0 ** -24
    assert torch.equal(y[:, 4 + nc], c["angle"][:, 0])
