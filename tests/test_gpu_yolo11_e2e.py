"""YOLO11 end to end on the GPU: yolo11n against the reference's maps, loss and gradients (tests/golden/psa_e2e_n, seeded weights:
tests/psa_common.py), the captured training step against the eager one, fuse() + predict + DetectionPredictor, bfloat16 training."""
import pytest
import torch

from conftest import load_golden, sample_errors
from psa_common import E2E_NC, e2e_batch, e2e_state
from test_gpu_modules_golden import F32_TOL, close, dev, run

pytestmark = pytest.mark.gpu


def _model(scale="n"):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    torch.manual_seed(0)
    model = DetectionModel(f"yolo11{scale}.yaml", ch=3, nc=E2E_NC)
    model.load_state_dict(e2e_state(model), strict=True)
    return model.to(dev())


def _zero_gradient_biases(model):
    """{parameter name: Conv block} of the BatchNorm biases whose gradient is ZERO in exact arithmetic, named from the structure of C2PSA.  All
    three blocks have no activation, so the bias is a per-channel constant added to the block's output:
      attn.pe       its output (o + pe(v)) meets only attn.proj, a 1x1 convolution followed by a train-mode BatchNorm, whose mean subtraction
                    removes a constant;
      attn.proj, ffn[1] of the LAST PSABlock: the constant rides the shortcut additions into C2PSA.cv2 (1x1 + train-mode BatchNorm) and, for
                    proj, into ffn[0] (the same): removed in both.
    (Part of attn.qkv's bias - the key columns - is zero too, the softmax being invariant to a constant added to every key; the tensor as a
    whole is not, so it stays in the relative comparison.)"""
    from improving_yolov8_cbam_swinblock_amd.nn.modules import C2PSA

    names = {id(p): n for n, p in model.named_parameters()}
    out = {}
    for blk in model.modules():
        if isinstance(blk, C2PSA):
            for j, m in enumerate(blk.m):
                out[names[id(m.attn.pe.bn.bias)]] = m.attn.pe
                if j == len(blk.m) - 1:
                    out[names[id(m.attn.proj.bn.bias)]] = m.attn.proj
                    out[names[id(m.ffn[1].bn.bias)]] = m.ffn[1]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_yolo11n_vs_reference(dtype):
    """float32: the three train-mode maps to F32_TOL, the loss to 2e-3, every parameter gradient (stored elements, relative L2 and norm) to
    twice the map tolerance - the bounds of test_gpu_ghost_e2e.py.  bfloat16: finite maps and gradients, the loss within 0.1 (scale n's
    narrowest depthwise width is 64: whole 16-byte chunks).

    Three gradients are zero in exact arithmetic (_zero_gradient_biases): the reference's values there are its own rounding noise.  For
    exactly those the test asserts what the kernel owes instead, as the ghost test does: dbeta[c] is the sum over the P = N H W pixels of the
    block's output gradient, so it lies within P u sum|dout| (u = 2^-24) of the float64 sum of the gradient the block received."""
    d = load_golden("psa_e2e_n")
    model = _model().train()
    zero = _zero_gradient_biases(model) if dtype == torch.float32 else {}
    douts = {}

    def record(name):
        def forward_hook(module, inputs, output):  # (returns None: the output passes through unchanged)
            output.register_hook(lambda g: douts.__setitem__(name, g.detach().double().cpu()))
        return forward_hook

    for n, blk in zero.items():
        blk.register_forward_hook(record(n))
    batch = {k: v.to(dev()) for k, v in e2e_batch().items()}
    preds = run(model, batch["img"], dtype)
    for i, p in enumerate(preds):
        if dtype == torch.float32:
            close(p, torch.from_numpy(d[f"pred{i}"]), F32_TOL, f"yolo11n e2e map {i}")
        else:
            assert torch.isfinite(p.float()).all(), f"yolo11n e2e map {i}"
    loss, _ = model.init_criterion()(preds, batch)
    ltol = 2e-3 if dtype == torch.float32 else 0.1
    print(f"[yolo11n e2e {dtype}] loss {loss.float().cpu().tolist()} reference {d['loss'].tolist()}")
    assert torch.allclose(loss.float().cpu(), torch.from_numpy(d["loss"]), rtol=ltol, atol=ltol), (loss, d["loss"])
    loss.sum().backward()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert all(torch.isfinite(g.float()).all() for g in grads.values())
    if dtype == torch.float32:
        assert len(grads) == sum(1 for k in d if k.startswith(("gfull.", "gsample."))) and len(zero) == 3 and set(zero) <= set(grads)
        tol2 = 2 * F32_TOL["atol"]
        errs = sample_errors("g", d, {n: g for n, g in grads.items() if n not in zero})
        print(f"[yolo11n e2e f32] {len(errs)} gradient records, worst relative error {max(e[1] for e in errs):.3e}, worst norm error {max(e[2] for e in errs):.3e}")
        bad = [e for e in errs if e[1] > tol2 or e[2] > tol2]
        assert not bad, bad[:5]
        for n in zero:
            g = douts[n]
            P = g.shape[0] * g.shape[2] * g.shape[3]
            err = (grads[n].double().cpu() - g.sum((0, 2, 3))).abs()
            bound = P * 2.0 ** -24 * g.abs().sum((0, 2, 3))
            print(f"[yolo11n e2e f32] {n}: |dbeta - sum dout| max {float(err.max()):.3e}, bound min {float(bound.min()):.3e}, |dbeta| max {float(grads[n].abs().max()):.3e}")
            assert bool((err <= bound).all()), (n, float((err - bound).max()))


def test_yolo11n_loss_path_equals_the_plain_forward():
    """model(batch) - the split head, the concat slots and the layer-level joins of the graph plan - gives the gradients of the step in which
    every layer-level join is left to autograd."""
    model = _model().train()
    plan = model._graph_plan()
    assert 10 in plan["consumers"] or 10 in plan["slot"]  # the C2PSA row takes part in the plan
    batch = {k: v.to(dev()) for k, v in e2e_batch().items()}
    grads = []
    for joins in (True, False):
        model._plan = plan if joins else {"slot": plan["slot"], "consumers": {}}
        model.zero_grad(set_to_none=True)
        loss, _ = model(batch)
        loss.sum().backward()
        grads.append({n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None})
    assert set(grads[0]) == set(grads[1]) and "model.0.conv.weight" in grads[0]
    zero = set(_zero_gradient_biases(model))
    for n in grads[0]:
        if n in zero:
            continue
        a, b = grads[0][n].double(), grads[1][n].double()
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-12, (n, float((a - b).norm()), float(b.norm()))


def test_yolo11n_train_step_graph_equals_eager():
    """TrainStep(graph=True) on yolo11n, two images of 128 x 128, SGD: graph mode runs 3 eager warm-up steps before its first replay, so replay i
    is eager step i + 3; losses and final weights agree as test_gpu_ghost_e2e.py demands of the ghost model.  Nothing in the attention or
    depthwise paths may allocate or synchronise under capture."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    losses, params = {}, {}
    probe = ("model.0.conv.weight", "model.2.m.0.cv1.conv.weight", "model.6.m.0.m.1.cv2.conv.weight", "model.10.m.0.attn.qkv.conv.weight",
             "model.10.m.0.attn.pe.conv.weight", "model.10.m.0.ffn.1.bn.weight", "model.23.cv3.0.0.0.conv.weight", "model.23.cv3.2.1.1.conv.weight")
    for mode, steps in (("eager", 6), ("graph", 3)):
        torch.manual_seed(0)
        model = DetectionModel("yolo11n.yaml", ch=3, nc=1).to(dev())
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


def test_yolo11n_fuse_predict_and_predictor():
    """eval output after fuse() equals the unfused one within F32_TOL; DetectionPredictor runs the fused model on one small image and its
    boxes are the NMS of that output."""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.predictor import DetectionPredictor
    from improving_yolov8_cbam_swinblock_amd.engine.results import Results

    model = _model().eval()
    img = e2e_batch()["img"][:1].to(dev())
    with torch.no_grad():
        y0, maps0 = model.predict(img)
        y1, _ = model.fuse().predict(img)
    assert model.is_fused() and y0.shape == (1, 4 + E2E_NC, sum((128 // s) ** 2 for s in (8, 16, 32))) and len(maps0) == 3
    close(y1, y0, F32_TOL, "fused eval")
    p = DetectionPredictor(model, imgsz=128, conf=0.001, dtype=torch.float32)
    res = p(img)
    assert len(res) == 1 and isinstance(res[0], Results) and res[0].orig_shape == (128, 128)
    det, count = ops.detect_nms(y1, 0.001, 0.7, max_det=300)
    assert int(count[0]) > 0 and res[0].boxes.data.shape == (int(count[0]), 6)
    assert torch.equal(res[0].boxes.data[:, 4:].cpu(), det[0, : int(count[0]), 4:].cpu())


def test_yolo11s_trains_in_bfloat16():
    """scale s, bfloat16, through the loss path: finite loss and a gradient for every trainable parameter (four heads of 64 in C2PSA)"""
    model = _model("s").train()
    batch = {k: v.to(dev()) for k, v in e2e_batch().items()}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss, _ = model(batch)
    loss.sum().backward()
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert model.model[10].m[0].attn.num_heads == 4
    assert torch.isfinite(loss.float()).all() and all(g is not None and torch.isfinite(g.float()).all() for g in grads)
