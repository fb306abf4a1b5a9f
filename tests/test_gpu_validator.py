"""GPU: engine.validator.DetectionValidator end to end.

The comparison is teacher-forced on the PRODUCT's decoded y: the test takes the y the validator's own eval forward produced, copies it
to the host and feeds it through tests/nms_exact.py and then through utils.metrics (both held to the reference on the CPU by
tests/test_host_nms_check.py).  The forward's 1e-3 agreement with the reference thereby stays out of a discontinuous comparison (DESIGN
section 2 argues the same for arg-max routing): detections must be equal, metrics must agree within 1e-9."""
import json

import numpy as np
import pytest
import torch

import nms_exact as NX
from conftest import GOLDEN, golden_state, load_golden

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _tiny_model(nc):
    """the e2e_tiny_seed7 graph: nc 1 with the fixture's weights, nc 3 with weights rebuilt from a seed."""
    from golden_weights import seeded_state
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    model = DetectionModel(cfg, ch=3, nc=nc)
    if nc == 1:
        model.load_state_dict(golden_state(load_golden("e2e_tiny_seed7")), strict=True)
    else:
        sd = model.state_dict()
        new = seeded_state({k: tuple(v.shape) for k, v in sd.items() if v.dtype.is_floating_point and v.dim() > 0 and ".dfl." not in k}, 77)
        for k in new:
            if k.endswith("running_var"):
                new[k] = new[k].abs() + 0.5
        model.load_state_dict(new, strict=False)
    return model.to(dev())


def _raise_class_bias(model, img, want=(200, 5000), conf=0.001):
    """shift the class branch's bias until every image has some hundreds of candidates above conf (asserted)."""
    with torch.no_grad():
        y = model.eval()(img)[0]
        top = y[:, 4:].amax(1).flatten().sort(descending=True)[0]
        target = float(top[min(len(top) - 1, 400 * img.shape[0])])  # the score that leaves ~400 anchors per image above it
        shift = float(np.log(0.02 / (1 - 0.02)) - np.log(max(target, 1e-12) / max(1 - target, 1e-12)))
        for m in model.model[-1].cv3:
            m[-1].bias.add_(shift)
        y = model(img)[0].cpu()
    n = [NX.candidates(y[b], conf, True)[1].numel() for b in range(y.shape[0])]
    assert all(want[0] <= v for v in n), n
    return n


def _expected(ys, batches, conf, iou, max_det, nc, agnostic=False, zero_class=False):
    """the test-side pipeline on the product's own y: nms_exact, then the matcher and the metrics of utils.metrics."""
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import DetMetrics, box_iou, match_predictions

    iouv = torch.linspace(0.5, 0.95, 10)
    images, dets = [], []
    for y, batch in zip(ys, batches):
        det, count = NX.nms_exact(y.cpu(), conf, iou, multi_label=True, agnostic=agnostic, max_det=max_det)
        h, w = batch["img"].shape[2:]
        bidx = batch["batch_idx"].cpu().reshape(-1)
        for b in range(y.shape[0]):
            rows = det[b, : int(count[b])].clone()
            if zero_class:
                rows[:, 5] = 0
            sel = bidx == b
            xywh = batch["bboxes"].cpu().float()[sel]
            half = xywh[:, 2:] / 2
            gt = torch.cat((xywh[:, :2] - half, xywh[:, :2] + half), 1) * torch.tensor([w, h, w, h], dtype=torch.float32)
            images.append((rows, gt, batch["cls"].cpu().float().reshape(-1)[sel]))
            dets.append(rows)
    stats = NX.accumulate(images, box_iou, lambda pc, tc, i: match_predictions(pc, tc, i, iouv), iouv)
    dm = DetMetrics(names={i: str(i) for i in range(nc)})
    dm.process(**stats)
    return dets, dm.results_dict


@pytest.mark.parametrize("nc", [1, 3])
def test_validator_equals_the_test_side_pipeline_on_the_products_y(nc):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator

    model = _tiny_model(nc)
    batches = [synthetic_batch(2, 256, dev(), 11 + i) for i in range(2)]
    if nc == 3:
        for i, b in enumerate(batches):
            b["cls"] = (torch.arange(b["cls"].numel(), device=dev()).float().reshape(-1, 1) + i) % 3
    with torch.no_grad():
        assert model.eval()(batches[0]["img"])[0].shape[2] == 1344  # 256^2: 32^2 + 16^2 + 8^2 anchors
    n = _raise_class_bias(model, torch.cat([b["img"] for b in batches]))
    model.train()
    v = DetectionValidator(model)
    assert (v.conf, v.iou, v.max_det, v.single_cls, v.agnostic_nms, v.dtype) == (0.001, 0.7, 300, False, False, torch.bfloat16)
    ys, post = [], v.postprocess
    v.postprocess = lambda preds: (ys.append(preds[0].detach().clone()), post(preds))[1]
    res = v(batches)
    assert model.training, "the validator must restore the mode it found"
    assert len(ys) == 2 and v.seen == 4
    seen = [NX.candidates(y[b].cpu(), 0.001, True)[1].numel() for y in ys for b in range(y.shape[0])]
    assert min(seen) >= 200, seen  # some hundreds of candidates per image in the y the validator worked on
    dets, want = _expected(ys, batches, 0.001, 0.7, 300, nc)
    print(f"[nc {nc}] candidates per image (float32 probe) {n}; detections {[len(d) for d in dets]}; {({k: round(float(x), 4) for k, x in res.items()})}")
    assert sum(len(d) for d in dets) > 0
    for got, d in zip(v.detections, dets):
        assert NX.same_bits(got, d), "detections differ from nms_exact on the product's y"
    assert list(res) == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"]
    for k in res:
        assert abs(float(res[k]) - float(want[k])) <= 1e-9, (k, res[k], want[k])
    assert v.get_stats() == res


@pytest.mark.parametrize("mode", ["single_cls", "agnostic_nms"])
def test_single_cls_and_agnostic_nms(mode):
    """single_cls: class-agnostic suppression, and predictions AND labels count as class 0 (the reference zeroes the labels in its dataset);
    agnostic_nms: class-agnostic suppression with the classes kept.  Both against the test-side pipeline on the product's y."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator

    model = _tiny_model(3)
    batches = [synthetic_batch(2, 256, dev(), 41 + i) for i in range(2)]
    for i, b in enumerate(batches):
        b["cls"] = (torch.arange(b["cls"].numel(), device=dev()).float().reshape(-1, 1) + i) % 3
    _raise_class_bias(model, torch.cat([b["img"] for b in batches]))
    v = DetectionValidator(model, **{mode: True})
    ys, post = [], v.postprocess
    v.postprocess = lambda preds: (ys.append(preds[0].detach().clone()), post(preds))[1]
    res = v(batches)
    want_batches = batches
    if mode == "single_cls":
        want_batches = [dict(b, cls=torch.zeros_like(b["cls"])) for b in batches]
    dets, want = _expected(ys, want_batches, 0.001, 0.7, 300, 3, agnostic=True, zero_class=mode == "single_cls")
    assert sum(len(d) for d in dets) > 0
    classes = torch.cat([d[:, 5] for d in v.detections])
    assert bool((classes == 0).all()) if mode == "single_cls" else classes.unique().numel() > 1
    for got, d in zip(v.detections, dets):
        assert NX.same_bits(got, d)
    for k in res:
        assert abs(float(res[k]) - float(want[k])) <= 1e-9, (k, res[k], want[k])
    assert all(bool((b["cls"] == (torch.arange(b["cls"].numel(), device=dev()).float().reshape(-1, 1) + i) % 3).all()) for i, b in enumerate(batches)), "the batch was modified"


class _FromLabels(torch.nn.Module):
    """stands in for a model: its eval forward returns a y synthesised from the batch's own labels (one anchor per label, the label's box,
    score 0.9 - 0.01 j at the label's class; every other anchor scores 0)."""

    class _Head(torch.nn.Module):
        def __init__(self, nc):
            super().__init__()
            self.nc = nc

    def __init__(self, nc, batches, anchors=1344, empty=False):
        super().__init__()
        self.model = torch.nn.ModuleList([self._Head(nc)])
        self.ys, self.calls = [], 0
        for batch in batches:
            B, _, h, w = batch["img"].shape
            y = torch.zeros(B, 4 + nc, anchors)
            if not empty:
                bidx = batch["batch_idx"].cpu().long().reshape(-1)
                for b in range(B):
                    rows = torch.nonzero(bidx == b).flatten()
                    for j, r in enumerate(rows):
                        a = 7 + 13 * j
                        y[b, :4, a] = batch["bboxes"].cpu().float()[r] * torch.tensor([w, h, w, h], dtype=torch.float32)
                        y[b, 4 + int(batch["cls"].cpu().reshape(-1)[r]), a] = 0.9 - 0.01 * j
            self.ys.append(y.to(dev()))

    def forward(self, img):
        assert not self.training
        self.calls += 1
        return self.ys[self.calls - 1], None


def test_perfect_predictions():
    """y synthesised from the labels themselves: every label is found at every IoU threshold, precision and recall are 1.  The reference's
    compute_ap (metrics.py:540-570) reads the envelope at recall 1.0 as its trailing sentinel 0, so a perfect curve integrates to 0.995
    over the 101 points, not to 1: that value, which utils.metrics shares with the reference to 1e-9, is what is asserted."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator

    batches = [synthetic_batch(2, 256, dev(), 21 + i) for i in range(2)]
    res = DetectionValidator(_FromLabels(1, batches))(batches)
    print({k: float(v) for k, v in res.items()})
    assert abs(res["metrics/precision(B)"] - 1.0) <= 1e-9 and abs(res["metrics/recall(B)"] - 1.0) <= 1e-9
    assert abs(res["metrics/mAP50(B)"] - 0.995) <= 1e-9 and abs(res["metrics/mAP50-95(B)"] - 0.995) <= 1e-9


def test_all_background_gives_zeros():
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator

    batches = [synthetic_batch(2, 256, dev(), 31)]
    for b in batches:  # no labels at all
        b["batch_idx"], b["cls"], b["bboxes"] = b["batch_idx"][:0], b["cls"][:0], b["bboxes"][:0]
    zeros = {k: 0.0 for k in ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"]}
    v = DetectionValidator(_FromLabels(1, batches, empty=True))  # ... and no detections
    assert {k: float(x) for k, x in v(batches).items()} == zeros and v.seen == 2
    model = _tiny_model(1)
    _raise_class_bias(model, batches[0]["img"])
    v = DetectionValidator(model)  # detections, but nothing to find
    assert {k: float(x) for k, x in v(batches).items()} == zeros and sum(len(d) for d in v.detections) > 0
    assert not model.training


def test_validation_between_graph_replays_leaves_training_bit_identical():
    """TrainStep(graph=True): 3 steps, DetectionValidator(step.ema.ema), 3 more steps == 6 uninterrupted steps, parameters and EMA bit
    for bit; the EMA model stays in eval mode."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    runs = []
    for validate in (False, True):
        torch.manual_seed(0)
        model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1).to(dev()).train()
        batch = synthetic_batch(2, 320, dev(), 1)
        step = TrainStep(model, world_size=1, lr=0.01, graph=True)
        for _ in range(3):
            step(batch)
        if validate:
            v = DetectionValidator(step.ema.ema)
            res = v([batch, synthetic_batch(2, 320, dev(), 2)])
            assert not step.ema.ema.training and model.training and v.seen == 4
            assert all(np.isfinite(float(x)) for x in res.values())
        for _ in range(3):
            step(batch)
        torch.cuda.synchronize()
        runs.append(({k: p.detach().clone() for k, p in model.state_dict().items()}, {k: p.detach().clone() for k, p in step.ema.ema.state_dict().items()}))
        del step, model
    (w0, e0), (w1, e1) = runs
    bad = [k for k in w0 if not torch.equal(w0[k], w1[k])] + ["ema." + k for k in e0 if not torch.equal(e0[k], e1[k])]
    assert not bad, bad[:8]
