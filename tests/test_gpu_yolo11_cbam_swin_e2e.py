"""YOLO11-CBAM-Swin end to end on the GPU: yolo11m-cbam-swin (SwinBlock(512, 2) at rows 7 and 17: head_dim 256; CBAM at row 10; two C2PSA rows)
against the reference's maps, loss and gradients (tests/golden/swin512_e2e_m and .g1, seeded weights: tests/psa_common.py), the captured training step
against the eager one, fuse() + predict + DetectionPredictor, the loss path with and without layer-level joins, bfloat16 training."""
import json

import pytest
import torch

from conftest import GOLDEN, load_golden, sample_errors
from psa_common import E2E_NC, e2e_batch, e2e_state
from test_gpu_modules_golden import F32_TOL, close, dev, run
from test_gpu_yolo11_e2e import _zero_gradient_biases

pytestmark = pytest.mark.gpu

YAML = "yolo11m-cbam-swin.yaml"


def _model():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    torch.manual_seed(0)
    model = DetectionModel(YAML, ch=3, nc=E2E_NC)
    model.load_state_dict(e2e_state(model), strict=True)
    return model.to(dev())


def _zero_gradients(model):
    """{parameter name: block whose OUTPUT gradient sums to that parameter's gradient} of the gradients that are zero in exact arithmetic:
    the BatchNorm biases test_gpu_yolo11_e2e.py::_zero_gradient_biases names in the two C2PSA rows, and model.17.mlp.2.bias - fc2's bias of the
    neck's SwinBlock is a per-channel constant of the block's output map, which only ever meets 1x1 convolutions followed by train-mode
    BatchNorm (through Upsample and Concat into row 20's cv1, and through the Concat of row 22 into row 23's cv1): the mean subtraction removes
    it.  (Row 7's constant meets row 8's padded 3x3 convolution, whose border pixels see it differently: not zero.)"""
    out = dict(_zero_gradient_biases(model))
    out["model.17.mlp.2.bias"] = model.model[17]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_yolo11m_cbam_swin_vs_reference(dtype):
    """float32: the three train-mode maps to F32_TOL, the loss to 2e-3, every non-zero parameter gradient record (stored elements, relative L2
    and norm) to twice the map tolerance - the bounds of test_gpu_yolo11_e2e.py::test_yolo11n_vs_reference.  (The reference's own float32 run
    differs from its float64 run by 4.9e-5 on the maps and 3.5e-4 on the worst gradient, whole tensors in relative L2: swin512_e2e_m.json.  The
    issue that asked for this test quotes 2.9e-4 for the latter; the generator's figure is the one recorded.)  bfloat16: finite maps and
    gradients, the loss within 0.1.

    Seven gradients are zero in exact arithmetic (the fixture's JSON lists them from a float64 run of the reference: norms <= 6e-15 against
    >= 3e-10 for every other): the reference's float32 values there are its own rounding noise.  For exactly those the test asserts what the
    kernel owes: the gradient is the sum over the P = N H W pixels of the gradient the block's output received, so it lies within
    P u sum|dout| (u = 2^-24) of that sum in float64."""
    d = {**load_golden("swin512_e2e_m"), **load_golden("swin512_e2e_m.g1")}  # (the gradient records of the later parameters: a second file)
    info = json.loads((GOLDEN / "swin512_e2e_m.json").read_text())
    model = _model().train()
    assert model.model[7].attn.num_heads == 2 and model.model[7].dim == 512 and model.model[17].dim == 512
    zero = _zero_gradients(model) if dtype == torch.float32 else {}
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
            close(p, torch.from_numpy(d[f"pred{i}"]), F32_TOL, f"yolo11m-cbam-swin e2e map {i}")
        else:
            assert torch.isfinite(p.float()).all(), f"yolo11m-cbam-swin e2e map {i}"
    loss, _ = model.init_criterion()(preds, batch)
    ltol = 2e-3 if dtype == torch.float32 else 0.1
    print(f"[yolo11m-cbam-swin e2e {dtype}] loss {loss.float().cpu().tolist()} reference {d['loss'].tolist()}")
    assert torch.allclose(loss.float().cpu(), torch.from_numpy(d["loss"]), rtol=ltol, atol=ltol), (loss, d["loss"])
    loss.sum().backward()
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert all(torch.isfinite(g.float()).all() for g in grads.values())
    if dtype == torch.float32:
        assert set(zero) == set(info["zero_in_exact_arithmetic"]) and len(zero) == 7 and set(zero) <= set(grads)
        assert set(grads) == set(info["params_with_grad"]) and len(grads) == sum(1 for k in d if k.startswith(("gfull.", "gsample.")))
        tol2 = 2 * F32_TOL["atol"]
        errs = sample_errors("g", d, {n: g for n, g in grads.items() if n not in zero})
        print(f"[yolo11m-cbam-swin e2e f32] {len(errs)} gradient records, worst relative error {max(e[1] for e in errs):.3e}, "
              f"worst norm error {max(e[2] for e in errs):.3e}")
        bad = [e for e in errs if e[1] > tol2 or e[2] > tol2]
        assert not bad, bad[:5]
        for n in zero:
            g = douts[n]
            P = g.shape[0] * g.shape[2] * g.shape[3]
            err = (grads[n].double().cpu() - g.sum((0, 2, 3))).abs()
            bound = P * 2.0 ** -24 * g.abs().sum((0, 2, 3))
            print(f"[yolo11m-cbam-swin e2e f32] {n}: |grad - sum dout| max {float(err.max()):.3e}, bound min {float(bound.min()):.3e}, "
                  f"|grad| max {float(grads[n].abs().max()):.3e}")
            assert bool((err <= bound).all()), (n, float((err - bound).max()))


def test_loss_path_equals_the_plain_forward():
    """model(batch) - the split head, the concat slots and the layer-level joins of the graph plan, where the SwinBlock of row 7 and the CBAM of
    row 10 each feed a later Concat - gives the gradients of the step in which every layer-level join is left to autograd."""
    model = _model().train()
    plan = model._graph_plan()
    assert plan["slot"][7][0] == 15 and plan["slot"][10][0] == 25 and plan["slot"][17][0] == 22
    assert plan["consumers"].get(7) == 2 and plan["consumers"].get(10) == 2 and plan["consumers"].get(17) == 2  # each: the next row + a Concat
    batch = {k: v.to(dev()) for k, v in e2e_batch().items()}
    grads = []
    for joins in (True, False):
        model._plan = plan if joins else {"slot": plan["slot"], "consumers": {}}
        model.zero_grad(set_to_none=True)
        loss, _ = model(batch)
        loss.sum().backward()
        grads.append({n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None})
    assert set(grads[0]) == set(grads[1]) and "model.7.attn.in_proj_weight" in grads[0]
    zero = set(_zero_gradients(model))
    for n in grads[0]:
        if n in zero:
            continue
        a, b = grads[0][n].double(), grads[1][n].double()
        assert float((a - b).norm()) <= 1e-4 * float(b.norm()) + 1e-12, (n, float((a - b).norm()), float(b.norm()))


def test_train_step_graph_equals_eager():
    """TrainStep(graph=True), two images of 128 x 128, SGD: graph mode runs 3 eager warm-up steps before its first replay, so replay i is eager
    step i + 3; losses and final weights agree as test_gpu_yolo11_e2e.py demands of yolo11n.  Nothing in the wide attention path may allocate
    or synchronise under capture."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    losses, params = {}, {}
    probe = ("model.0.conv.weight", "model.7.attn.in_proj_weight", "model.7.norm1.weight", "model.10.ca.shared_MLP.0.weight",
             "model.12.m.0.attn.qkv.conv.weight", "model.13.m.0.ffn.1.bn.weight", "model.17.mlp.2.weight", "model.17.attn.out_proj.weight",
             "model.27.cv3.0.0.0.conv.weight", "model.27.cv3.2.1.1.conv.weight")
    for mode, steps in (("eager", 6), ("graph", 3)):
        torch.manual_seed(0)
        model = DetectionModel(YAML, ch=3, nc=1).to(dev())
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


def test_fuse_predict_and_predictor():
    """eval output after fuse() equals the unfused one within F32_TOL; DetectionPredictor runs the fused model on one small image and its boxes
    are the NMS of that output."""
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


def test_scale_without_512_channels_raises_at_the_first_forward():
    """SwinBlock's 512 is not width-scaled: at scale s row 6 has 256 channels and the block refuses them (the reference raises in
    LayerNorm(512) during the forward it runs at construction)."""
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    model = DetectionModel("yolo11s-cbam-swin.yaml", ch=3, nc=E2E_NC).to(dev()).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="normalized_shape"):
        model.predict(torch.zeros(1, 3, 64, 64, device=dev()))
