"""CPU: the inference side of segmentation without a device - tests/segpred_ref.py (the restatement the GPU tests use) held to the reference's
fixtures (tests/golden/make_segpred_golden.py), the host halves of utils.ops / utils.metrics / engine.results, every refusal, and the ABI."""
import json
import re

import numpy as np
import pytest
import torch

import segpred_ref as SR
from conftest import GOLDEN, ROOT

PKG = "improving_yolov8_cbam_swinblock_amd"


def fixture_masks(name, mode):
    proto, box, _, _ = SR.decode_case(name)
    c = SR.DECODE_CASES[name]
    shape = (box.shape[0], *(c["shape"] if mode == "up" else c["mhw"]))
    with np.load(GOLDEN / f"segpred_decode_{name}.npz") as z:
        return SR.unpack_masks(z[mode], shape)


# ---- the restatement against the reference's masks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["low", "up"])
@pytest.mark.parametrize("name", ["exact_24x40", "exact_160"])
def test_exact_inputs_give_the_reference_masks_in_any_precision_and_order(name, mode):
    proto, box, coef, img = SR.decode_case(name)
    shape, up = SR.DECODE_CASES[name]["shape"], mode == "up"
    want = fixture_masks(name, mode).bool()
    v32 = SR.process_mask_values(proto, box, coef, img, shape, up, torch.float32)
    v64 = SR.process_mask_values(proto, box, coef, img, shape, up, torch.float64)
    assert torch.equal(v32.double(), v64), "float32 must be exact on these inputs"
    perm = torch.randperm(SR.NM, generator=torch.Generator().manual_seed(1))
    assert torch.equal(SR.process_mask_values(proto[:, perm], box, coef[:, perm], img, shape, up, torch.float32), v32), "a channel order changes the sum"
    assert torch.equal(v32 > 0, want)
    assert torch.equal(proto.to(torch.bfloat16).float(), proto), "the prototypes must be exact in bfloat16"


def test_exact_case_holds_the_box_cases_the_kernels_must_get_right():
    proto, box, coef, img = SR.decode_case("exact_24x40")
    low = fixture_masks("exact_24x40", "low")
    edges = SR.crop_edges(box, (24, 40), (96, 160))
    assert edges[0].tolist() == [2.0, 1.0, 30.0, 20.0] and int(low[0, :, :2].sum()) == 0 and int(low[0, :, 30:].sum()) == 0
    assert int(low[3].sum()) == 0 and int(low[4].sum()) == 0 and int(low[5].sum()) == 0, "zero-area and outside boxes"
    assert int(low[6].sum()) == 0 and int(low[11].sum()) == 0 and img[6] == -1 and img[11] == 2, "rows of no image"
    assert int(low[7].sum()) == 0, "all-zero logits are not in the mask"
    assert torch.equal(low[8].bool(), proto[int(img[8]), 0] > 0) and int((proto[int(img[8]), 0] == 0).sum()) > 0, "exact zeros inside a full box"
    assert int(low[2].sum()) > 200 and len({int(v) for v in img.tolist()}) == 4


@pytest.mark.parametrize("mode", ["low", "up"])
def test_real_inputs_agree_with_the_reference_outside_the_recorded_margin(mode):
    proto, box, coef, img = SR.decode_case("real_24x40")
    note = json.loads((GOLDEN / "segpred_decode.json").read_text())["real_24x40"][mode]
    want = fixture_masks("real_24x40", mode).bool()
    v64 = SR.process_mask_values(proto, box, coef, img, (96, 160), mode == "up", torch.float64)
    v32 = SR.process_mask_values(proto, box, coef, img, (96, 160), mode == "up", torch.float32)
    open_ = (v64 != 0) & (v64.abs() < note["margin"])
    assert int(open_.sum()) <= 0.001 * int((v64 != 0).sum())
    assert torch.equal((v32 > 0)[~open_], want[~open_]) and torch.equal((v64 > 0)[~open_], want[~open_])
    assert float((v32.double() - v64).abs().max()) <= note["margin"]


@pytest.mark.parametrize("name", list(SR.DECODE_CASES))
def test_utils_process_mask_on_the_host_is_the_reference(name):
    """host tensors take the reference's torch statements, image by image; uint8 where the reference returns float"""
    from improving_yolov8_cbam_swinblock_amd.utils.ops import crop_mask, process_mask

    proto, box, coef, img = SR.decode_case(name)
    shape = SR.DECODE_CASES[name]["shape"]
    for mode, up in (("low", False), ("up", True)):
        want = fixture_masks(name, mode)
        for b in range(proto.shape[0]):
            sel = torch.nonzero(img == b).reshape(-1)
            got = process_mask(proto[b], coef[sel], box[sel], shape, upsample=up)
            assert got.dtype == torch.uint8 and torch.equal(got, want[sel])
    m = torch.ones(2, 4, 6)
    got = crop_mask(m, torch.tensor([[1.0, 0.5, 3.0, 2.5], [0.0, 0.0, 6.0, 4.0]]))
    assert got[0].tolist() == [[0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]] and bool(got[1].all())


# ---- overlap, matching, metrics --------------------------------------------------------------------------------------------------------------
def host_masks(case):
    B, max_det = case["det"].shape[:2]
    n = B * max_det
    img = torch.arange(B, dtype=torch.int32).repeat_interleave(max_det)
    v = SR.process_mask_values(case["proto"], case["det"].view(n, 6)[:, :4], case["coef"].view(n, SR.NM), img, case["shape"], False)
    live = (torch.arange(max_det)[None] < case["count"][:, None]).view(n, 1, 1)
    return ((v > 0) & live).view(B, max_det, *case["proto"].shape[2:])


def test_mask_iou_and_the_host_matching_equal_the_reference_fixture():
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import mask_iou, match_predictions

    case = SR.match_case(**SR.REF_MATCH)
    masks = host_masks(case)
    with np.load(GOLDEN / "segpred_match.npz") as z:
        want_tp_m, want_iou = torch.from_numpy(z["tp_m"]), torch.from_numpy(z["iou0"])
    cls0 = SR.image_labels(case["lab_img"], case["lab_cls"], 0)
    nl, n = len(cls0), int(case["count"][0])
    gt = (case["enc"][0][None].long() == torch.arange(nl).view(nl, 1, 1) + 1).float()
    iou = mask_iou(gt.view(nl, -1), masks[0, :n].reshape(n, -1).float())
    assert iou.dtype == torch.float32 and torch.equal(iou, want_iou)
    # the same quotient from integer counts: what the device path forms
    inter, area_pred, area_gt = SR.overlap_counts(masks, case["count"], case["enc"], 256)
    fi = inter[0, :n, 1 : nl + 1].t().float()
    assert torch.equal(fi / ((area_gt[0, 1 : nl + 1, None].float() + area_pred[0, None, :n].float()) - fi + 1e-7), want_iou)
    got = SR.tp_m_host(masks, case, match_predictions, mask_iou)
    assert int(want_tp_m.sum()) >= 8 and torch.equal(got, want_tp_m)


def test_planted_tie_has_equal_overlaps_and_takes_the_first_label_in_table_order():
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import mask_iou, match_predictions

    case = SR.match_case(**PLANTED)
    masks = host_masks(case)
    rows = torch.nonzero(case["lab_img"] == 0).reshape(-1)
    inter, area_pred, area_gt = SR.overlap_counts(masks, case["count"], case["enc"], 256)
    tied = [j for j in range(len(rows)) if int(inter[0, 0, j + 1]) == 24 and int(area_gt[0, j + 1]) == 48]
    assert len(tied) == 2 and int(area_pred[0, 0]) == 48, (inter[0, 0, : len(rows) + 1].tolist(), area_gt[0, : len(rows) + 1].tolist())
    tp_m = SR.tp_m_host(masks, case, match_predictions, mask_iou, iouv=torch.tensor([0.3]))
    assert int(tp_m[0, 0, 0]) == 1  # inter 24 / union 72 = 1 / 3 with either label


PLANTED = dict(seed=41, counts=[40, 3], labels=[3, 2], max_det=48, nc=3, planted_tie=True)


def test_segment_metrics_equal_the_reference_fixture():
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import SegmentMetrics, box_iou, match_predictions
    from improving_yolov8_cbam_swinblock_amd.utils.ops import xywh2xyxy

    case = SR.match_case(**SR.REF_MATCH)
    want = json.loads((GOLDEN / "segpred_metrics.json").read_text())
    with np.load(GOLDEN / "segpred_match.npz") as z:
        tp_m, tp_ref = z["tp_m"], z["tp"]
    stats = dict(tp=[], tp_m=[], conf=[], pred_cls=[], target_cls=[])
    scale = torch.tensor([case["shape"][1], case["shape"][0]] * 2, dtype=torch.float32)
    for b in range(len(case["count"])):
        n = int(case["count"][b])
        cls = SR.image_labels(case["lab_img"], case["lab_cls"], b)
        pred = case["det"][b, :n]
        tp = np.zeros((n, 10), dtype=bool)
        if n and len(cls):
            tp = match_predictions(pred[:, 5], cls, box_iou(xywh2xyxy(case["lab_box"][case["lab_img"] == b]) * scale, pred[:, :4]), SR.IOUV).numpy()
            assert np.array_equal(tp, tp_ref[b, :n].astype(bool))
        if n or len(cls):
            for k, v in zip(stats, (tp, tp_m[b, :n].astype(bool), pred[:, 4].numpy(), pred[:, 5].numpy(), cls.numpy())):
                stats[k].append(v)
    sm = SegmentMetrics(names={i: str(i) for i in range(SR.REF_MATCH["nc"])})
    assert sm.results_dict == dict(zip(want["keys"], [0.0] * 9)), "nothing processed: every metric is zero"
    sm.process(**{k: np.concatenate(v, 0) for k, v in stats.items()})
    got = sm.results_dict
    assert list(got) == want["keys"] and len(got) == 9 and list(got)[4:8] == [k.replace("(B)", "(M)") for k in list(got)[:4]]
    assert np.allclose(list(got.values()), want["results"], rtol=0, atol=1e-9)
    assert np.allclose(sm.seg.all_ap, want["seg_ap"], rtol=0, atol=1e-9) and np.allclose(sm.box.all_ap, want["box_ap"], rtol=0, atol=1e-9)
    assert sm.fitness == sm.seg.fitness() + sm.box.fitness() and abs(sm.fitness - want["fitness"]) <= 1e-9
    assert list(sm.ap_class_index) == want["ap_class_index"] and len(sm.mean_results()) == 8 and len(sm.class_result(0)) == 8


def test_seg_nms_fixture_rows_are_the_box_rows_with_the_kept_anchors_coefficients():
    """the reference's [n, 6 + nm] rows: six columns equal to the detection fixture of the same case, the rest a gather"""
    import nms_exact as NX

    c = SR.SEG_NMS
    y = SR.with_coefficients(NX.case_input(c["case"]), c["nm"], c["seed"])
    with np.load(GOLDEN / "segpred_nms.npz") as z:
        rows, counts = torch.from_numpy(z["rows"]), z["counts"]
    want, _ = NX.load_expected(c["case"])
    assert counts.tolist() == [len(w) for w in want] and NX.same_bits(rows[:, :6].contiguous(), torch.cat(want, 0))
    det, count = NX.padded(want, 300)
    coef = SR.kept_coefficients(y, NX.CASES[c["case"]]["nc"], det, count)
    live = torch.arange(300)[None] < count[:, None]
    assert NX.same_bits(coef[live], rows[:, 6:].contiguous())


# ---- Masks / Results -------------------------------------------------------------------------------------------------------------------------
def test_masks_and_results_on_the_host():
    from improving_yolov8_cbam_swinblock_amd.engine.results import Boxes, Masks, Results

    data = torch.zeros(2, 8, 12, dtype=torch.uint8)
    data[1, 2:4] = 1
    m = Masks(data, (80, 120))
    assert len(m) == 2 and tuple(m.shape) == (2, 8, 12) and m.orig_shape == (80, 120) and m.data is data
    assert torch.equal(m.cpu().data, data) and isinstance(m.cpu(), Masks) and len(Masks(data[0], (80, 120))) == 1
    for name in ("xy", "xyn"):
        with pytest.raises(NotImplementedError, match="contour"):
            getattr(m, name)
    boxes = torch.tensor([[1.0, 2.0, 3.0, 4.0, 0.9, 1.0], [2.0, 2.0, 5.0, 6.0, 0.8, 0.0]])
    r = Results((80, 120), path="a.jpg", names={0: "x"}, boxes=boxes, masks=data)
    assert isinstance(r.masks, Masks) and isinstance(r.boxes, Boxes) and len(r) == 2 and r.masks.orig_shape == (80, 120)
    c = r.cpu()
    assert torch.equal(c.masks.data, data) and torch.equal(c.boxes.data, boxes) and "masks=2" in repr(r)
    plain = Results((80, 120), path="a.jpg", boxes=boxes)
    assert plain.masks is None and plain.cpu().masks is None
    assert repr(plain) == "Results(path='a.jpg', orig_shape=(80, 120), boxes=2)", "the repr of a box-only result is unchanged"
    assert Results((80, 120), None, None, boxes).masks is None  # masks is a new LAST keyword


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_what_is_not_built_is_refused_with_a_message():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.predictor import DetectionPredictor, SegmentationPredictor
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator, SegmentationValidator
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel, SegmentationModel
    from improving_yolov8_cbam_swinblock_amd.utils.ops import process_mask_native, scale_masks

    seg = SegmentationModel("yolov8n-seg.yaml", nc=3).eval()
    with pytest.raises(NotImplementedError, match="retina_masks"):
        process_mask_native(torch.zeros(32, 4, 4), torch.zeros(1, 32), torch.zeros(1, 4), (16, 16))
    with pytest.raises(NotImplementedError, match="scale_masks"):
        scale_masks(torch.zeros(1, 1, 4, 4), (16, 16))
    with pytest.raises(NotImplementedError, match="retina_masks"):
        SegmentationPredictor(seg, retina_masks=True)
    with pytest.raises(NotImplementedError, match="test-time augmentation"):
        SegmentationPredictor(seg, augment=True)
    with pytest.raises(NotImplementedError, match="test-time augmentation"):
        SegmentationValidator(seg, augment=True)
    with pytest.raises(NotImplementedError, match="overlap_mask"):
        SegmentationValidator(seg, overlap_mask=False)
    with pytest.raises(NotImplementedError, match="save_json"):
        SegmentationValidator(seg, save_json=True)
    with pytest.raises(NotImplementedError, match="save_json / save_txt"):
        SegmentationValidator(seg, save_txt=True)
    for op, args in ((ops.process_mask, (torch.zeros(1, 16, 4, 4), torch.zeros(1, 4), torch.zeros(1, 16), torch.zeros(1), (16, 16))),
                     (ops.mask_overlap, (torch.zeros(1, 3, 6), torch.zeros(1, 3, 16), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 16, 4, 4),
                                         torch.zeros(1, 4, 4), (16, 16)))):
        with pytest.raises(NotImplementedError, match="nm = 32"):
            op(*args)
    # the detection classes still refuse a segmentation model and now name the classes that take one; those refuse a detector
    with pytest.raises(NotImplementedError, match="SegmentationPredictor"):
        DetectionPredictor(seg)
    with pytest.raises(NotImplementedError, match="SegmentationValidator"):
        DetectionValidator(seg)
    det = DetectionModel("yolov8n.yaml", ch=3, nc=3).eval()
    with pytest.raises(ValueError, match="Segment"):
        SegmentationPredictor(det)
    with pytest.raises(ValueError, match="Segment"):
        SegmentationValidator(det)
    v = SegmentationValidator(seg, match="device", loss=True)
    assert v.loss_names == ("val/box_loss", "val/seg_loss", "val/cls_loss", "val/dfl_loss") and list(v.stats) == ["tp_m", "tp", "conf", "pred_cls", "target_cls"]


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_in_the_header_and_the_binding():
    from improving_yolov8_cbam_swinblock_amd import _lib

    header = (ROOT / "include" / "ymi.h").read_text()
    names = ["ymi_detect_nms_seg", "ymi_process_mask", "ymi_mask_overlap", "ymi_val_match_masks"]
    for n in names:
        assert re.search(rf"\bint {n}\(", header), n
        assert n in _lib.exported_symbols()
    # the argument counts of header and binding agree
    for n in names:
        decl = re.search(rf"\bint {n}\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == len(_lib._SIGNATURES[n][1]), n
    mk = (ROOT / PKG / "csrc" / "Makefile").read_text()
    assert "FLAGS_maskdec := -ffp-contract=off" in mk and (ROOT / PKG / "csrc" / "maskdec.hip").exists()
