"""OBBModel end to end on the GPU: yolov8n-obb / yolo11n-obb against the reference's fixtures (tests/golden/obb_e2e_*.npz: loss, items and every
parameter's gradient record, at the bounds of the segmentation models' end-to-end test), the captured training step against eager steps bit for
bit, a save / load round trip, and every combination that is refused."""
import json

import pytest
import torch

from conftest import GOLDEN, load_golden, sample_errors
from obb_common import E2E_MODELS, E2E_NC, e2e_batch, e2e_state
from test_gpu_modules_golden import F32_TOL, close, dev
from test_gpu_yolo11_e2e import _zero_gradient_biases

pytestmark = pytest.mark.gpu


def _batch():
    return {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in e2e_batch().items()}


@pytest.mark.parametrize("name", list(E2E_MODELS))
def test_obb_model_end_to_end_vs_reference(name):
    """nc = 3, two 128 x 128 images, float32: loss and items within 2e-3, every parameter gradient record within twice the map tolerance;
    bfloat16: finite, and the criterion on the bf16 maps within 0.1 of the float32 kernels on the same maps."""
    from improving_yolov8_cbam_swinblock_amd.nn.modules import OBBPreds
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import OBBModel

    d = load_golden(name)
    meta = json.loads((GOLDEN / f"{name}.json").read_text())
    model = OBBModel(E2E_MODELS[name], ch=3, nc=E2E_NC)
    model.load_state_dict(e2e_state(model), strict=True)
    model = model.to(dev()).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    batch = _batch()
    loss, items = model(batch)
    print(f"[{name} f32] loss items {items.cpu().tolist()} reference {d['loss_items'].tolist()}")
    assert loss.shape == (3,) and items.shape == (3,)
    assert torch.allclose(items.cpu(), torch.from_numpy(d["loss_items"]), rtol=2e-3, atol=2e-3), (items, d["loss_items"])
    assert torch.allclose(loss.detach().cpu(), torch.from_numpy(d["loss"]), rtol=2e-3, atol=2e-3)
    loss.sum().backward()
    named = dict(model.named_parameters())
    with_grad = [n for n, q in named.items() if q.grad is not None]
    assert sorted(with_grad) == sorted(meta["params_with_grad"])
    zero = _zero_gradient_biases(model)
    errs = sample_errors("g", d, {n: named[n].grad for n in with_grad if n not in zero})
    tol2 = 2 * F32_TOL["atol"]
    print(f"[{name} f32] {len(errs)} gradient records, worst relative error {max(e[1] for e in errs):.3e}, worst norm error {max(e[2] for e in errs):.3e}")
    bad = [e for e in errs if e[1] > tol2 or e[2] > tol2]
    assert not bad, bad[:5]
    model.load_state_dict(state, strict=True)
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        preds = model._predict_once(batch["img"], split_head=True)
    assert isinstance(preds, OBBPreds) and preds.angle.dtype == torch.float32 and all(q.dtype == torch.bfloat16 for q in preds.box + preds.cls)
    crit = model.init_criterion()
    loss16, items16 = crit(preds, batch)
    loss16.sum().backward()
    wide = OBBPreds([q.detach().float() for q in preds.box], [q.detach().float() for q in preds.cls], preds.angle.detach())
    _, items32 = crit(wide, batch)
    print(f"[{name} bf16] loss items {items16.cpu().tolist()} float32 kernels on the same maps {items32.cpu().tolist()}")
    assert torch.isfinite(items16).all() and all(torch.isfinite(q.grad).all() for q in model.parameters() if q.grad is not None)
    assert torch.allclose(items16.cpu(), items32.cpu(), rtol=0.1, atol=0.1), (items16, items32)


@pytest.mark.parametrize("mode", [True, "split"], ids=["graph", "split"])
def test_yolov8n_obb_captured_step_equals_eager_bit_for_bit(mode):
    """graph mode runs 3 eager warm-up steps before its first replay, so replay i is eager step i + 3: the loss items of three replays and the
    weights behind them equal the eager run's, bit for bit"""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_obb_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import OBBModel

    losses, params = {}, {}
    for name, graph, steps in (("eager", False, 6), ("graph", mode, 3)):
        torch.manual_seed(0)
        model = OBBModel("yolov8n-obb.yaml", ch=3, nc=2).to(dev())
        step = TrainStep(model, world_size=1, lr=0.01, graph=graph)
        batch = synthetic_obb_batch(2, 128, dev(), 1)
        assert batch["bboxes"].shape == (8, 5)
        losses[name] = torch.stack([step(batch).float().cpu().clone() for _ in range(steps)])
        params[name] = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()}
        del step, model
    print(f"[yolov8n-obb {mode}] eager items {losses['eager'][3:6].tolist()} captured {losses['graph'].tolist()}")
    diff = {k: float((params["graph"][k] - params["eager"][k]).abs().max()) for k in params["eager"] if not torch.equal(params["graph"][k], params["eager"][k])}
    print(f"[yolov8n-obb {mode}] state entries that differ: {len(diff)} of {len(params['eager'])}; worst {max(diff.values()) if diff else 0.0:.3e}")
    assert losses["graph"].shape == (3, 3) and torch.isfinite(losses["graph"]).all()
    assert float(losses["eager"][:, 0].min()) > 0  # the rotated box term is alive
    assert torch.equal(losses["graph"], losses["eager"][3:6])
    assert not diff, list(diff.items())[:5]


def test_obb_model_fuses_saves_and_loads(tmp_path):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import OBBModel

    model = OBBModel("yolov8n-obb.yaml", ch=3, nc=E2E_NC)
    model.load_state_dict(e2e_state(model), strict=True)
    model = model.to(dev()).eval()
    img = e2e_batch()["img"].to(dev())
    with torch.no_grad():
        y0, (feats, angle) = model(img)
    assert y0.shape == (2, 4 + E2E_NC + 1, 336) and angle.shape == (2, 1, 336)
    path = tmp_path / "obb.pt"
    torch.save({"model": model.state_dict()}, path)
    other = OBBModel("yolov8n-obb.yaml", ch=3, nc=E2E_NC)
    assert other.load(torch.load(path, weights_only=True)["model"]) == len(model.state_dict())
    other = other.to(dev()).eval()
    with torch.no_grad():
        assert torch.equal(other(img)[0], y0)
        other.fuse()
        close(other(img)[0], y0, F32_TOL, "fused eval")


def test_obb_combinations_that_are_not_built_raise():
    from improving_yolov8_cbam_swinblock_amd.engine.predictor import DetectionPredictor
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, augment_batch, synthetic_obb_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from improving_yolov8_cbam_swinblock_amd.nn.modules import OBB
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import OBBModel

    with pytest.raises(NotImplementedError, match="ne = 1"):
        OBB(3, 2, (32, 64, 128))
    model = OBBModel("yolov8n-obb.yaml", ch=3, nc=1).to(dev())
    for kw in (dict(graph="tail"), dict(world_size=2, graph=True), dict(graph=True, image_shapes=2)):
        with pytest.raises(NotImplementedError, match="OBBModel"):
            TrainStep(model, **kw)
    step = TrainStep(model, graph=False)
    with pytest.raises(NotImplementedError, match="accumulation"):
        step(synthetic_obb_batch(2, 128, dev(), 1), update=False)
    with pytest.raises(NotImplementedError, match="rotated NMS"):
        DetectionValidator(model)
    with pytest.raises(NotImplementedError, match="rotated NMS"):
        DetectionPredictor(model)
    model.eval()
    with pytest.raises(NotImplementedError, match="rotated boxes"):
        model.predict(torch.zeros(1, 3, 64, 64, device=dev()), augment=True)
    import numpy as np

    sample = {"img": np.zeros((64, 64, 3), np.uint8), "labels": np.zeros((1, 6), np.float32)}
    with pytest.raises(NotImplementedError, match="oriented"):
        augment_batch([sample], 64, mosaic=False)
    batch = synthetic_obb_batch(2, 128, dev(), 1)
    batch["bboxes"] = batch["bboxes"][:, :4].contiguous()
    model.train()
    with pytest.raises((TypeError, ValueError), match="xywhr"):
        model(batch)
