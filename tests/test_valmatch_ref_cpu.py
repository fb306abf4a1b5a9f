"""CPU: the yardsticks of the validation-statistics tests are themselves checked.

utils.metrics.ConfusionMatrix (the host path) and tests/valmatch_ref.py (the float32 restatement the GPU tests compare ops.val_match with)
must equal the matrices the reference's ConfusionMatrix.process_batch produced (tests/golden/confusion_matrix.json, written by
tests/golden/make_confusion_golden.py); valmatch_ref's tp must equal utils.metrics' box_iou + match_predictions bit for bit (those are
held to the reference by tests/test_host_nms_check.py); planted faults in the restatement must be noticed.  The input conditions the
fixture rests on are asserted here too, never skipped."""
import json

import numpy as np
import pytest
import torch

import nms_exact as NX
import valmatch_ref as VR
from conftest import GOLDEN

IOUV = torch.linspace(0.5, 0.95, 10)


def _fixture():
    return json.loads((GOLDEN / "confusion_matrix.json").read_text())


def _label_rows(lab_img, b):
    return torch.nonzero(lab_img == b).flatten()


@pytest.mark.parametrize("name", VR.CASES)
def test_confusion_matrix_equals_the_reference(name):
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import ConfusionMatrix

    nc, images = VR.case(name)
    want = np.array(_fixture()[name], dtype=np.int64)
    cm = ConfusionMatrix(nc, conf=0.001)  # the validator's default confidence: taken as 0.25, as the reference takes it
    assert cm.conf == 0.25 and cm.iou_thres == 0.45 and cm.matrix.shape == (nc + 1, nc + 1) and ConfusionMatrix(nc, conf=None).conf == 0.25
    assert ConfusionMatrix(nc, conf=0.3).conf == 0.3
    for det, xywh, cls in images:
        cm.process_batch(det if len(det) else None, VR.label_boxes(xywh, VR.IMGSZ, VR.IMGSZ), cls)
    assert np.array_equal(cm.matrix, want), (cm.matrix, want)
    tp, fp = cm.tp_fp()
    assert np.array_equal(tp, np.diag(want)[:-1]) and np.array_equal(fp, (want.sum(1) - np.diag(want))[:-1])


@pytest.mark.parametrize("name", VR.CASES)
def test_restatement_equals_the_host_path_and_the_fixture(name):
    """valmatch_ref.match on the packed batch, the label table shuffled: tp against box_iou + match_predictions on the label boxes
    DetectionValidator.update_metrics forms (xywh2xyxy * scale), the matrix against the reference's."""
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import box_iou, match_predictions
    from improving_yolov8_cbam_swinblock_amd.utils.ops import xywh2xyxy

    nc, images = VR.case(name)
    det, count, lab_img, lab_cls, lab_box = VR.pack(images, 300, shuffle_seed=3)
    tp, cm = VR.match(det, count, lab_img, lab_cls, lab_box, (VR.IMGSZ, VR.IMGSZ), IOUV, nc=nc)
    assert np.array_equal(cm, np.array(_fixture()[name], dtype=np.int64))
    scale = torch.tensor([VR.IMGSZ] * 4, dtype=torch.float32)
    for b, (rows, _, _) in enumerate(images):
        sel = _label_rows(lab_img, b)
        lab = xywh2xyxy(lab_box[sel]) * scale
        assert NX.same_bits(lab, VR.label_boxes(lab_box[sel], VR.IMGSZ, VR.IMGSZ))
        want = torch.zeros(300, 10, dtype=torch.uint8)
        if len(rows) and len(sel):
            iou = box_iou(lab, rows[:, :4])
            assert NX.same_bits(iou, VR.iou_matrix(lab, rows[:, :4]))
            want[: len(rows)] = match_predictions(rows[:, 5], lab_cls[sel], iou, IOUV).to(torch.uint8)
        assert torch.equal(tp[b], want), (name, b)


def test_native_label_boxes_equal_the_host_statements():
    """label_boxes(native=...) against utils.ops.scale_boxes on host tensors, for shapes and pads that clip on every side"""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.utils.ops import scale_boxes, xywh2xyxy

    _, images = VR.case("dense_a")
    xywh = images[0][1]
    for ori, rp in (((480, 640), None), ((1080, 1920), None), ((333, 517), ((0.731, 0.731), (41.0, 87.0))), ((200, 300), ((1.9, 1.9), (120.0, 7.0)))):
        want = scale_boxes((640, 640), xywh2xyxy(xywh) * torch.tensor([640.0] * 4), ori, ratio_pad=rp)
        got = VR.label_boxes(xywh, 640, 640, ops.scale_boxes_params((640, 640), ori, rp))
        assert NX.same_bits(got, want), (ori, rp)
    assert bool((got == 0).any()) and bool((got[:, 2] == 300).any() or (got[:, 3] == 200).any()), "the last geometry must clip"


def test_cases_meet_the_conditions_the_fixture_rests_on():
    for name in VR.CASES:
        _, images = VR.case(name)
        distinct, gap_cm, gap_lv, gap_conf = VR.conditions(images)
        print(f"[{name}] |iou - 0.45| >= {gap_cm:.2e}, |iou - level| >= {gap_lv:.2e}, |conf - 0.25| >= {gap_conf:.2e}, lost claims {VR.lost_claims(images)}")
        assert distinct and gap_cm >= NX.MARGIN_MIN and gap_lv >= NX.MARGIN_MIN and gap_conf > 0, name
        if name.startswith("steal"):
            assert VR.lost_claims(images) > 0
    assert max(len(d) for d, _, _ in VR.case("dense_a")[1]) == 300
    assert float(IOUV[0]) == 0.5 and float(IOUV[5]) == 0.75  # the planted batch's exact IoUs meet exact levels


def test_planted_batch_gives_the_hand_worked_result():
    det, count, lab_img, lab_cls, lab_box = VR.planted()
    tp, cm = VR.match(det, count, lab_img, lab_cls, lab_box, VR.PLANTED_SHAPE, IOUV, nc=VR.PLANTED_NC)
    assert ["".join(str(int(v)) for v in row) for row in tp[3, : int(count[3])]] == VR.PLANTED_TP3
    assert int(tp[:3].sum()) == 0 and int(tp[3, int(count[3]) :].sum()) == 0, "junk past the count was read"
    assert cm.tolist() == VR.PLANTED_CM and int(cm.sum()) == 17
    # the tie rule: with G1 and G2 exchanged in the table the matrix's detection 7 goes to G2 (class 2)
    swap = torch.arange(len(lab_img))
    swap[9], swap[10] = 10, 9
    _, cm2 = VR.match(det, count, lab_img[swap], lab_cls[swap], lab_box[swap], VR.PLANTED_SHAPE, IOUV, nc=VR.PLANTED_NC)
    assert cm2[0, 2] == cm[0, 2] + 1 and cm2[0, 0] == cm[0, 0] - 1 and cm2[3, 0] == cm[3, 0] + 1 and cm2[3, 2] == cm[3, 2] - 1


def _all_results(fault=None):
    out = []
    for name in VR.CASES:
        nc, images = VR.case(name)
        out.append(VR.match(*VR.pack(images, 300, shuffle_seed=3), (VR.IMGSZ, VR.IMGSZ), IOUV, nc=nc, fault=fault) + (name,))
    out.append(VR.match(*VR.planted(), VR.PLANTED_SHAPE, IOUV, nc=VR.PLANTED_NC, fault=fault) + ("planted",))
    return out


@pytest.mark.parametrize("fault", VR.FAULTS)
def test_planted_fault_in_the_restatement_is_flagged(fault):
    """`>` in place of `>=` (the planted batch's IoUs of exactly 0.5 and 0.75), the class mask dropped (wrong-class detections of the seeded
    cases), the holder chosen by rank instead of by IoU (the steal cases, against the reference's matrices)."""
    fixture = _fixture()
    good, bad = _all_results(), _all_results(fault)
    differs = [name for (tp, cm, name), (ftp, fcm, _) in zip(good, bad) if not torch.equal(tp, ftp) or not np.array_equal(cm, fcm)]
    print(f"[{fault}] noticed by {differs}")
    assert differs, f"no case notices {fault}"
    if fault == "gt":
        assert "planted" in differs
    if fault == "owner_by_rank":
        caught = [name for _, fcm, name in bad if name in fixture and not np.array_equal(fcm, np.array(fixture[name]))]
        assert any(n.startswith("steal") for n in caught), caught


def test_val_match_has_no_cpu_path():
    from improving_yolov8_cbam_swinblock_amd import ops

    det, count, lab_img, lab_cls, lab_box = VR.planted()
    with pytest.raises(RuntimeError, match="MI355X|cuda"):
        ops.val_match(det, count, lab_img, lab_cls, lab_box, VR.PLANTED_SHAPE, IOUV)
    assert ops.VAL_MATCH_LABEL_CHUNK == 1024


def test_val_match_argument_checks_on_the_host():
    """the argument checks run before any launch, so they can be held to on a machine without a GPU"""
    import ctypes

    from improving_yolov8_cbam_swinblock_amd import _lib

    L = _lib.lib()
    one = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before it launches
    lv = (ctypes.c_float * 17)(*[0.5] * 17)
    args = lambda max_det, n_levels, cm, nc: (one, one, 2, max_det, one, one, one, 8, 640.0, 640.0, None, lv, n_levels, 0, one, cm, nc, 0.25, 0.45, None)  # noqa: E731
    assert L.ymi_val_match(*args(4096, 10, None, 0)) == -1 and b"max_det" in L.ymi_last_error()
    assert L.ymi_val_match(*args(300, 17, None, 0)) == -1 and b"levels" in L.ymi_last_error()
    assert L.ymi_val_match(*args(300, 0, None, 0)) == -1 and b"levels" in L.ymi_last_error()
    assert L.ymi_val_match(*args(300, 10, one, 0)) == -1 and b"nc" in L.ymi_last_error()
    assert L.ymi_val_match(one, one, 2, 300, None, one, one, 8, 640.0, 640.0, None, lv, 10, 0, one, None, 0, 0.25, 0.45, None) == -1 and b"label" in L.ymi_last_error()
