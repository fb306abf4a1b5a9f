"""DWConv / GhostConv / GhostBottleneck / C3 / C3Ghost on the GPU against the reference's own outputs (tests/golden/ghost_*.npz, written by
tests/golden/make_ghost_golden.py), exactly as test_gpu_modules_golden.py::test_conv_family_vs_reference holds the dense family: train
forward, gradients of x and of every parameter at twice the forward tolerance, running statistics, eval forward, eval forward after fuse().
The bounds are that file's F32_TOL / BF16_TOL - the project's contract with the reference."""
import pytest
import torch

from conftest import golden_state, load_golden
from ghost_common import CASES
from test_gpu_modules_golden import BF16_TOL, F32_TOL, P, close, dev, grads_of, run, set_bn, t

pytestmark = pytest.mark.gpu


def _module(name):
    ctor, args, _ = CASES[name]
    d = load_golden(name)
    m = getattr(P(), ctor)(*args)
    set_bn(m)
    m.load_state_dict(golden_state(d), strict=True)
    return m.to(dev()), d


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_ghost_family_vs_reference(name, dtype):
    from improving_yolov8_cbam_swinblock_amd.utils.torch_utils import fuse_conv_and_bn

    m, d = _module(name)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    m.train()
    x = t(d["x"]).to(dev()).requires_grad_(True)
    y = run(m, x, dtype)
    close(y, t(d["y_train"]), tol, f"{name} train fwd")
    params = [p for p in m.parameters() if p.requires_grad]
    names = ["x"] + [n for n, p in m.named_parameters() if p.requires_grad]
    gs = grads_of(y, [x] + params, t(d["gy"]).to(dev()))
    gtol = dict(atol=tol["atol"] * 2, rtol=0)
    for n, g in zip(names, gs):
        assert g is not None, f"{name}: no gradient for {n}"
        close(g, t(d["g." + n]), gtol, f"{name} grad {n}")
    sd = m.state_dict()
    for k, v in golden_state(d, "after.").items():
        close(sd[k].float(), v.float(), tol, f"{name} running stat {k}")
    m.eval()
    with torch.no_grad():
        close(run(m, x.detach(), dtype), t(d["y_eval"]), tol, f"{name} eval fwd")
        for sub in m.modules():  # BaseModel.fuse
            if isinstance(sub, P().Conv) and hasattr(sub, "bn"):
                sub.conv = fuse_conv_and_bn(sub.conv, sub.bn)
                delattr(sub, "bn")
                sub.forward = sub.forward_fuse
        close(run(m, x.detach(), dtype), t(d["y_fused"]), tol, f"{name} eval fwd after fuse")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_ghostconv_train_output_is_one_buffer_and_equals_the_concat_form(dtype):
    """train mode: cv1 writes channels [0, c_) and the depthwise cv2 channels [c_, 2 c_) of ONE buffer - no concat copy - and the gradient of
    cv1's output (it feeds the concat and cv2) forms inside cv2's data-gradient kernel.  Output and gradients equal, bit for bit, the form
    with separate tensors and ops.concat (autograd's sum of the two gradients rounds once, as the kernel's epilogue does)."""
    from improving_yolov8_cbam_swinblock_amd import ops

    m, d = _module("ghost_ghostconv_16_32_k1_s1")
    m.train()
    x = t(d["x"]).to(dev())
    state = {k: v.clone() for k, v in m.state_dict().items()}
    xi = ops.to_internal(x, dtype).detach().requires_grad_(True)
    launched = {"concat": 0}
    real = ops.concat

    def spy(*a, **kw):
        launched["concat"] += 1
        return real(*a, **kw)

    ops.concat = spy
    try:
        y = m(xi)
    finally:
        ops.concat = real
    assert launched["concat"] == 0  # no concat, hence no copy launch
    c_ = m.cv1.conv.out_channels
    assert y.shape[1] == 2 * c_ and ops.as_ymi(y).ld == 2 * c_
    left, right = y[:, :c_], y[:, c_:]
    assert right.data_ptr() == left.data_ptr() + c_ * y.element_size()  # the two halves lie side by side in one buffer
    gy = t(d["gy"]).to(dev()).to(dtype)
    params = [p for p in m.parameters()]
    got = torch.autograd.grad(y, [xi] + params, gy)
    # the same block as separate tensors + ops.concat, from the same state
    m.load_state_dict(state, strict=True)
    xj = xi.detach().clone().requires_grad_(True)
    y1 = m.cv1(xj)
    y2 = ops.concat([y1, m.cv2(y1)])
    ref = torch.autograd.grad(y2, [xj] + params, gy)
    assert torch.equal(y, y2)
    for n, a, b in zip(["x"] + [k for k, _ in m.named_parameters()], got, ref):
        if dtype == torch.float32 or not n.startswith(("x", "cv1")):
            assert torch.equal(a, b), n
        else:  # bfloat16: the kernel adds in float32 and rounds once, autograd adds two rounded tensors and rounds again
            close(a, b, BF16_TOL, n)


def _ref_conv_block(m, x, p):
    """float64 restatement of a Conv block in train mode (conv -> BatchNorm with batch statistics -> activation) on the parameters p"""
    cv = m.conv
    y = torch.nn.functional.conv2d(x, p[id(cv.weight)], None, cv.stride, cv.padding, 1, cv.groups)
    mean, var = y.mean((0, 2, 3), keepdim=True), y.var((0, 2, 3), unbiased=False, keepdim=True)
    z = (y - mean) / torch.sqrt(var + m.bn.eps) * p[id(m.bn.weight)].view(1, -1, 1, 1) + p[id(m.bn.bias)].view(1, -1, 1, 1)
    return z * torch.sigmoid(z) if isinstance(m.act, torch.nn.SiLU) else z


def test_bottleneck_with_depthwise_cv2_keeps_the_joined_gradient():
    """Bottleneck(c, c, True, g=c, e=1): x feeds cv1 and the shortcut and carries a GradJoin (two consumers); cv2 is depthwise and takes x as its
    residual.  The depthwise Function must arrive at the join, or cv1's deposit is lost: every gradient against float64 autograd."""
    torch.manual_seed(3)
    m = P().Bottleneck(16, 16, True, g=16, e=1.0)
    assert m.cv2.depthwise and not m.cv1.depthwise
    set_bn(m)
    with torch.no_grad():
        for q in m.parameters():
            q.copy_(torch.randn_like(q) * 0.3 + (1.0 if q.dim() == 1 else 0.0))
    x0 = torch.randn(2, 16, 9, 7)
    gy = torch.randn(2, 16, 9, 7)
    p64 = {id(q): q.detach().double().requires_grad_(True) for q in m.parameters()}
    x64 = x0.double().requires_grad_(True)
    ref = torch.autograd.grad(x64 + _ref_conv_block(m.cv2, _ref_conv_block(m.cv1, x64, p64), p64), [x64] + [p64[id(q)] for q in m.parameters()], gy.double())
    m = m.to(dev()).train()
    x = x0.to(dev()).requires_grad_(True)
    y = m(x)
    got = grads_of(y, [x] + list(m.parameters()), gy.to(dev()))
    gtol = dict(atol=F32_TOL["atol"] * 2, rtol=0)
    for n, a, b in zip(["x"] + [k for k, _ in m.named_parameters()], got, ref):
        assert a is not None, n
        close(a, b.float(), gtol, f"depthwise bottleneck grad {n}")


def test_dwconv_row_beside_a_concat_keeps_the_joined_gradient():
    """a model whose DWConv row shares its input with a Concat: on the loss path that input carries a GradJoin of two consumers, and the
    DWConv writes into its slot of the concat buffer.  The gradients equal those of the same step with every layer-level join left to autograd."""
    from ghost_common import e2e_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    cfg = {"nc": 3, "backbone": [[-1, 1, "Conv", [16, 3, 2]], [-1, 1, "DWConv", [16, 3, 1]], [[-1, 0], 1, "Concat", [1]], [-1, 1, "Conv", [32, 3, 2]],
                                 [-1, 1, "Conv", [64, 3, 2]]], "head": [[[2, 3, 4], 1, "Detect", ["nc"]]]}
    torch.manual_seed(5)
    model = DetectionModel(cfg, ch=3, nc=3).to(dev()).train()
    assert model.model[1].depthwise
    plan = model._graph_plan()
    assert plan["consumers"].get(0) == 2 and 1 in plan["slot"] and 0 in plan["slot"]
    batch = {k: v.to(dev()) for k, v in e2e_batch().items()}
    grads = []
    for joins in (True, False):
        model._plan = plan if joins else {"slot": plan["slot"], "consumers": {}}
        model.zero_grad(set_to_none=True)
        loss, _ = model(batch)
        loss.sum().backward()
        grads.append({n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None})
    assert set(grads[0]) == set(grads[1]) and "model.0.conv.weight" in grads[0]
    for n in grads[0]:
        a, b = grads[0][n].double(), grads[1][n].double()
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-12, (n, float((a - b).norm()), float(b.norm()))


def test_frozen_depthwise_weight_gets_no_gradient():
    m, d = _module("ghost_dwconv_16_k3_s1")
    m.conv.weight.requires_grad_(False)
    m.train()
    x = t(d["x"]).to(dev()).requires_grad_(True)
    y = m(x)
    gx, gg, gb = grads_of(y, [x, m.bn.weight, m.bn.bias], t(d["gy"]).to(dev()))
    gtol = dict(atol=F32_TOL["atol"] * 2, rtol=0)
    close(gx, t(d["g.x"]), gtol, "grad x")
    close(gg, t(d["g.bn.weight"]), gtol, "grad bn.weight")
    assert m.conv.weight.grad is None
