"""yolov8-ghost end to end on the GPU: yolov8s-ghost against the reference's maps, loss and gradients (tests/golden/ghost_e2e_s, seeded
weights: tests/ghost_common.py), eval before / after fuse(), the captured training step against the eager one, and scale n (a 4-channel
depthwise layer: float32 only)."""
import pytest
import torch

from conftest import load_golden, sample_errors
from ghost_common import E2E_NC, e2e_batch, e2e_state
from test_gpu_modules_golden import F32_TOL, close, dev, run

pytestmark = pytest.mark.gpu


def _model(scale="s"):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    torch.manual_seed(0)
    model = DetectionModel(f"yolov8{scale}-ghost.yaml", ch=3, nc=E2E_NC)
    model.load_state_dict(e2e_state(model), strict=True)
    return model.to(dev())


def _zero_gradient_biases(model):
    """{parameter name: GhostConv module} of the BatchNorm biases whose gradient is ZERO in exact arithmetic, named from the structure: the bias
    of the last depthwise block (conv[2].cv2, no activation) of a GhostBottleneck with an identity shortcut inside a C3Ghost.  A per-channel
    constant added there reaches - through the additions of the shortcuts and the concat, which pass constants on - only 1x1 convolutions
    followed by train-mode BatchNorms (the next GhostBottleneck's conv[0].cv1, finally the C3Ghost's cv3), whose mean subtraction removes it.
    (conv[2].cv1's bias is not in the list: its output also feeds the 5x5 depthwise convolution, whose zero padding sees a constant.)"""
    from improving_yolov8_cbam_swinblock_amd.nn.modules import C3Ghost

    names = {id(p): n for n, p in model.named_parameters()}
    out = {}
    for c3 in model.modules():
        if isinstance(c3, C3Ghost):
            for gb in c3.m:
                if isinstance(gb.shortcut, torch.nn.Identity):
                    out[names[id(gb.conv[2].cv2.bn.bias)]] = gb.conv[2]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_yolov8s_ghost_vs_reference(dtype):
    """float32: the three train-mode maps to F32_TOL, the loss to 2e-3, every parameter gradient (stored elements, relative L2 and norm)
    to twice the map tolerance.  bfloat16: finite maps and gradients, the loss within the existing end-to-end bound (0.1).

    Ten gradients are zero in exact arithmetic (_zero_gradient_biases): the reference's values there are its own rounding noise (norms of 1e-6
    beside 1e+2 for their neighbours), against which no relative bound means anything.  For exactly those the test asserts what the
    kernel owes instead: dbeta[c] is the sum over the P = N H W pixels of the block's output gradient (no activation), so it lies within
    P u sum|dout| (u = 2^-24: the worst case of a float32 sum of P terms) of the float64 sum of the gradient the block received."""
    d = load_golden("ghost_e2e_s")
    model = _model().train()
    zero = _zero_gradient_biases(model) if dtype == torch.float32 else {}
    douts = {}

    def record(name):
        def forward_hook(module, inputs, output):  # (returns None: the output passes through unchanged)
            output.register_hook(lambda g: douts.__setitem__(name, g.detach().double().cpu()))
        return forward_hook

    for n, ghost in zero.items():
        ghost.register_forward_hook(record(n))
    batch = {k: v.to(dev()) for k, v in e2e_batch().items()}
    preds = run(model, batch["img"], dtype)
    for i, p in enumerate(preds):
        if dtype == torch.float32:
            close(p, torch.from_numpy(d[f"pred{i}"]), F32_TOL, f"ghost e2e map {i}")
        else:
            assert torch.isfinite(p.float()).all(), f"ghost e2e map {i}"
    loss, _ = model.init_criterion()(preds, batch)
    ltol = 2e-3 if dtype == torch.float32 else 0.1
    print(f"[ghost e2e {dtype}] loss {loss.float().cpu().tolist()} reference {d['loss'].tolist()}")
    assert torch.allclose(loss.float().cpu(), torch.from_numpy(d["loss"]), rtol=ltol, atol=ltol), (loss, d["loss"])
    loss.sum().backward()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert all(torch.isfinite(g.float()).all() for g in grads.values())
    if dtype == torch.float32:
        assert len(grads) == sum(1 for k in d if k.startswith(("gfull.", "gsample."))) and len(zero) == 10 and set(zero) <= set(grads)
        tol2 = 2 * F32_TOL["atol"]
        errs = sample_errors("g", d, {n: g for n, g in grads.items() if n not in zero})
        print(f"[ghost e2e f32] {len(errs)} gradient records, worst relative error {max(e[1] for e in errs):.3e}, worst norm error {max(e[2] for e in errs):.3e}")
        bad = [e for e in errs if e[1] > tol2 or e[2] > tol2]
        assert not bad, bad[:5]
        for n in zero:
            g = douts[n]
            c = g.shape[1] // 2
            right = g[:, c:]  # the depthwise half of the GhostConv's output: what conv[2].cv2's BatchNorm receives
            P = right.shape[0] * right.shape[2] * right.shape[3]
            err = (grads[n].double().cpu() - right.sum((0, 2, 3))).abs()
            bound = P * 2.0 ** -24 * right.abs().sum((0, 2, 3))
            print(f"[ghost e2e f32] {n}: |dbeta - sum dout| max {float(err.max()):.3e}, bound min {float(bound.min()):.3e}, |dbeta| max {float(grads[n].abs().max()):.3e}")
            assert bool((err <= bound).all()), (n, float((err - bound).max()))


def test_yolov8s_ghost_eval_agrees_before_and_after_fuse():
    model = _model().eval()
    img = e2e_batch()["img"].to(dev())
    with torch.no_grad():
        y0, _ = model(img)
        y1, _ = model.fuse()(img)
    assert model.is_fused()
    close(y1, y0, F32_TOL, "fused eval")


def test_ghost_train_step_graph_equals_eager():
    """TrainStep(graph=True) on yolov8s-ghost, two images of 128 x 128, SGD: graph mode runs 3 eager warm-up steps before its first replay, so
    replay i is eager step i + 3; losses and final weights agree as test_gpu_fullsize.py::test_hip_graph_step_matches_eager_and_is_isolated
    asserts for the stock model.  Nothing in the depthwise path may allocate or synchronise under capture."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    losses, params = {}, {}
    probe = ("model.0.conv.weight", "model.1.cv2.conv.weight", "model.2.m.0.conv.0.cv2.conv.weight", "model.4.cv3.bn.weight", "model.21.m.0.conv.2.cv2.conv.weight")
    for mode, steps in (("eager", 6), ("graph", 3)):
        torch.manual_seed(0)
        model = DetectionModel("yolov8s-ghost.yaml", ch=3, nc=1).to(dev())
        step = TrainStep(model, world_size=1, lr=0.01, graph=mode == "graph")
        batch = synthetic_batch(2, 128, dev(), 1)
        losses[mode] = torch.stack([step(batch).float().cpu().clone() for _ in range(steps)])
        sd = model.state_dict()
        params[mode] = {k: sd[k].detach().float().cpu().clone() for k in probe}
        del step, model
    assert torch.isfinite(losses["graph"]).all()
    torch.testing.assert_close(losses["graph"], losses["eager"][3:6], rtol=2e-2, atol=2e-2)
    for k in probe:
        a, b = params["graph"][k], params["eager"][k]
        err = float((a - b).norm() / b.norm().clamp(min=1e-9))
        assert err < 5e-3, (k, err)


def test_yolov8n_ghost_trains_in_float32_and_refuses_bfloat16():
    """scale n has a 4-channel depthwise layer: whole 16-byte chunks in float32 (4 channels), not in bfloat16 (8)"""
    model = _model("n").train()
    batch = {k: v.to(dev()) for k, v in e2e_batch().items()}
    loss, _ = model(batch)
    loss.sum().backward()
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert torch.isfinite(loss).all() and all(g is not None and torch.isfinite(g).all() for g in grads)
    model.zero_grad()
    with pytest.raises(NotImplementedError, match="16-byte chunks"):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            model(batch)
