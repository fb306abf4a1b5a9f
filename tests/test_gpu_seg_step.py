"""TrainStep on a SegmentationModel: the captured step against eager steps, by the rule of test_gpu_yolo11_e2e.py's step test (graph mode runs
3 eager warm-up steps before its first replay, so replay i is eager step i + 3; loss items within 2e-2, probed weights within 5e-3 relative
L2), and the combinations that are not built."""
import pytest
import torch

from test_gpu_modules_golden import dev

pytestmark = pytest.mark.gpu

PROBE = ("model.0.conv.weight", "model.4.m.0.cv1.conv.weight", "model.22.cv2.0.0.conv.weight", "model.22.cv3.1.2.weight", "model.22.cv4.0.0.conv.weight",
         "model.22.cv4.2.2.bias", "model.22.proto.cv1.conv.weight", "model.22.proto.upsample.weight", "model.22.proto.upsample.bias",
         "model.22.proto.cv3.bn.weight")


@pytest.mark.parametrize("mode", [True, "split"], ids=["graph", "split"])
def test_yolov8n_seg_captured_step_equals_eager(mode):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_seg_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    losses, params = {}, {}
    for name, graph, steps in (("eager", False, 6), ("graph", mode, 3)):
        torch.manual_seed(0)
        model = SegmentationModel("yolov8n-seg.yaml", ch=3, nc=1).to(dev())
        step = TrainStep(model, world_size=1, lr=0.01, graph=graph)
        batch = synthetic_seg_batch(2, 128, dev(), 1)
        losses[name] = torch.stack([step(batch).float().cpu().clone() for _ in range(steps)])
        sd = model.state_dict()
        params[name] = {k: sd[k].detach().float().cpu().clone() for k in PROBE}
        del step, model
    print(f"[yolov8n-seg {mode}] eager items {losses['eager'][3:6].tolist()} captured {losses['graph'].tolist()}")
    assert losses["graph"].shape == (3, 4) and torch.isfinite(losses["graph"]).all()
    assert float(losses["eager"][:, 1].min()) > 0  # the mask term is alive
    torch.testing.assert_close(losses["graph"], losses["eager"][3:6], rtol=2e-2, atol=2e-2)
    for k in PROBE:
        a, b = params["graph"][k], params["eager"][k]
        err = float((a - b).norm() / b.norm().clamp(min=1e-9))
        assert err < 5e-3, (k, err)


def test_captured_step_reads_the_masks_of_each_batch():
    """batch["masks"] is a static INPUT of the graph: a replay with other masks (the same image and labels, the masks mirrored) equals the
    eager step on that batch, and differs from the step that would have seen the old masks."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_seg_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    def run(graph, last_mirrored):
        torch.manual_seed(0)
        model = SegmentationModel("yolov8n-seg.yaml", ch=3, nc=1).to(dev())
        step = TrainStep(model, world_size=1, lr=0.01, graph=graph)
        a = synthetic_seg_batch(2, 128, dev(), 1)
        b = dict(a, masks=a["masks"].flip(-1).contiguous()) if last_mirrored else a
        for _ in range(1 if graph else 4):  # (the first captured call applies its batch four times: three warm-up steps and a replay)
            step(a)
        return step(b).float().cpu().clone()

    eager_b, eager_a, graph_b = run(False, True), run(False, False), run(True, True)
    print(f"[masks] eager mirrored {eager_b.tolist()} eager unchanged {eager_a.tolist()} captured mirrored {graph_b.tolist()}")
    torch.testing.assert_close(graph_b, eager_b, rtol=2e-2, atol=2e-2)
    # the mirrored masks are really another problem: stale masks would miss the comparison above by more than twice its tolerance
    assert abs(float(eager_b[1]) - float(eager_a[1])) > 2 * (2e-2 + 2e-2 * float(eager_b[1]))


def test_segmentation_steps_that_are_not_built_raise():
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_seg_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    model = SegmentationModel("yolov8n-seg.yaml", ch=3, nc=1).to(dev())
    with pytest.raises(NotImplementedError, match="SegmentationModel"):
        TrainStep(model, graph="tail")
    step = TrainStep(model, graph=False)
    with pytest.raises(NotImplementedError, match="accumulation"):
        step(synthetic_seg_batch(2, 128, dev(), 1), update=False)
    batch = synthetic_seg_batch(2, 128, dev(), 1)
    batch["masks"] = batch["masks"].cpu()
    with pytest.raises(ValueError, match="masks"):
        TrainStep(model, graph=True)(batch)
