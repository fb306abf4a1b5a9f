"""Segmentation on the CPU (no GPU): parse_model's layer tables of both segmentation model files against the reference's, and the restatements
of tests/seg_ref.py against the reference's own outputs (tests/golden/seg_*.npz, written by tests/golden/make_seg_golden.py) - they are the
second reference of the GPU tests, so they are held to the fixtures first."""
import json

import pytest
import torch

from conftest import GOLDEN, load_golden
from psa_common import seeded_module_state
import seg_common
from seg_common import LOSS_CASES, PROTO_CASE, PROTO_SEED, SCALES, level_hw, loss_case
from golden_weights import seeded_inputs
import seg_ref


def _tables():
    return json.loads((GOLDEN / "seg_parse_tables.json").read_text())


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("family", ["yolov8", "yolo11"])
def test_parse_tables_match_the_reference(family, scale):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    ref = _tables()[f"{family}-seg:{scale}"]
    m = SegmentationModel(f"{family}{scale}-seg.yaml", ch=3, nc=3)
    got = [{"i": l.i, "f": l.f, "type": l.type.split(".")[-1], "np": int(l.np)} for l in m.model]
    assert [g["type"] for g in got] == [("Upsample" if r["type"] == "Upsample" else r["type"]) for r in ref["layers"]]
    assert [(g["i"], g["f"], g["np"]) for g in got] == [(r["i"], r["f"], r["np"]) for r in ref["layers"]]
    assert list(m.save) == ref["save"] and [float(s) for s in m.stride] == ref["stride"]
    assert sum(p.numel() for p in m.parameters()) == ref["params"]
    if ref["state"]:
        head = {k: list(v.shape) for k, v in m.state_dict().items() if k.startswith(f"model.{len(m.model) - 1}.")}
        assert head == ref["state"]


def test_segmentation_model_refuses_what_is_not_built():
    from types import SimpleNamespace

    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel
    from improving_yolov8_cbam_swinblock_amd.utils.loss import v8SegmentationLoss

    m = SegmentationModel("yolov8n-seg.yaml", nc=3)
    m.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, overlap_mask=False)
    with pytest.raises(NotImplementedError, match="loss.py:427-428"):
        v8SegmentationLoss(m)


def test_depth_to_space_pair_is_a_permutation_and_the_gemm_view_is_the_transposed_convolution():
    torch.manual_seed(3)
    deep = torch.randn(2, 4 * 8, 5, 3, dtype=torch.float64)
    assert torch.equal(seg_ref.space_to_depth2(seg_ref.depth_to_space2(deep)), deep)
    x = torch.randn(2, 8, 5, 3, dtype=torch.float64)
    w, b = torch.randn(8, 12, 2, 2, dtype=torch.float64), torch.randn(12, dtype=torch.float64)
    ref = torch.nn.functional.conv_transpose2d(x, w, b, 2)
    assert (seg_ref.conv_transpose2x2(x, w, b) - ref).abs().max() < 1e-12


def test_proto_restatement_against_the_reference():
    name, args, xshape = PROTO_CASE
    d = load_golden(name)
    import improving_yolov8_cbam_swinblock_amd.nn.modules as M

    m = M.Proto(*args)
    sd = {k: v.double() for k, v in seeded_module_state(m, PROTO_SEED).items()}
    x, gy = seeded_inputs(PROTO_SEED, xshape, d["y_train"].shape)
    x = x.double().requires_grad_(True)
    y = seg_ref.proto_forward(x, sd)
    assert (y - torch.from_numpy(d["y_train"]).double()).abs().max() < 1e-4
    (gx,) = torch.autograd.grad(y, x, gy.double())
    assert (gx - torch.from_numpy(d["g.x"]).double()).abs().max() < 2e-4


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_mask_loss_restatement_against_the_reference(name):
    """float64 restatement against the float32 reference: the distance printed here is what the GPU test's own tolerance is derived from."""
    d = load_golden(name)
    feats, mc, proto, batch = loss_case(name)
    img_hw = LOSS_CASES[name][0]
    gidx = torch.from_numpy(d["gidx"]).long()
    B = proto.shape[0]
    mc64, p64 = mc.double().requires_grad_(True), proto.double().requires_grad_(True)
    seg = seg_ref.mask_loss(mc64, p64, gidx, seg_ref.dense_targets(batch, B, img_hw), batch["masks"], img_hw)
    ref = float(d["items"][1]) / 7.5
    print(f"[{name}] seg loss float64 {float(seg.detach()):.9f} reference float32 {ref:.9f} relative distance {abs(float(seg.detach()) - ref) / max(ref, 1e-12):.2e}")
    assert abs(float(seg) - ref) <= 2e-5 * max(1.0, ref)
    gmc, gp = torch.autograd.grad(seg * 7.5 * B, [mc64, p64])
    for got, key in ((gmc, "g.mc"), (gp, "g.proto")):
        want = torch.from_numpy(d[key]).double()
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        print(f"[{name}] {key}: reference float32 against float64, max abs err {err:.3e} / max |g| {scale:.3e} = {err / max(scale, 1e-300):.2e}")
        assert err <= 3.5e-7 * scale, key  # (measured 1.7e-7 .. 3.4e-7: the GPU test's float32 gradient bound is four times this)
    if name == "seg_loss_nofg":
        assert float(seg) == 0.0 and not gmc.any() and not gp.any()
    if name == "seg_loss_edge":  # the narrow box (label 2 of image 0) has foreground anchors, and their crop is one column wide
        boxes = seg_ref.dense_targets(batch, B, img_hw)[0, 2] / 4
        assert int((gidx[0] == 2).sum()) >= 1 and int((gidx[0] == 1).sum()) == 0
        assert int(torch.ceil(boxes[2])) - int(torch.ceil(boxes[0])) == 1
    if name == "seg_loss_many":
        assert int((gidx[0] >= 0).sum()) > 64 and int((gidx[1] >= 0).sum()) == 0
    assert sum(h * w for h, w in level_hw(img_hw)) == gidx.shape[1]


def test_no_case_has_a_box_edge_on_a_mask_pixel_boundary():
    """crop_mask compares integer pixel indices with float32 box edges: an edge ON a pixel boundary is decided by the last bit of the
    reference's own float32 arithmetic and moves a whole row of the crop.  The cases keep clear of that, so they test the kernel."""
    for name, (img_hw, boxes, _) in LOSS_CASES.items():
        assert seg_common.mask_edges_off_grid(boxes, (img_hw[0] // 4, img_hw[1] // 4)), name
    seg_common.e2e_batch()
    assert seg_common.mask_edges_off_grid(seg_common.E2E_BOXES, (32, 32))


def test_inference_side_refuses_a_segmentation_model():
    """what is not built raises with a message before anything runs: the predictor, the validator, test-time augmentation"""
    from improving_yolov8_cbam_swinblock_amd.engine.predictor import DetectionPredictor
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    m = SegmentationModel("yolov8n-seg.yaml", nc=3).eval()
    with pytest.raises(NotImplementedError, match="SegmentationModel"):
        DetectionPredictor(m)
    with pytest.raises(NotImplementedError, match="SegmentationModel"):
        DetectionValidator(m)
    with pytest.raises(NotImplementedError, match="mask coefficients"):
        m.predict(torch.zeros(1, 3, 64, 64), augment=True)
