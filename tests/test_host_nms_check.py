"""CPU: the yardsticks of the post-processing tests are themselves checked against the reference's fixtures.

tests/nms_exact.py (the float32 restatement the GPU tests compare ops.detect_nms with) must equal, bit for bit, what the reference's
non_max_suppression returned for every committed case (tests/golden/make_val_golden.py; its stand-in for torchvision.ops.nms is disclosed
there), and must notice planted faults.  utils/metrics.py (host code) must equal the reference's box_iou, matcher, ap_per_class and
DetMetrics.  The input conditions of the guarded cases - distinct candidate scores, float64 margin >= 1e-5 - are asserted, never skipped."""
import json

import numpy as np
import pytest
import torch

import nms_exact as NX
from conftest import GOLDEN


@pytest.mark.parametrize("name", list(NX.CASES))
def test_nms_exact_equals_the_reference_fixture(name):
    c = NX.CASES[name]
    y = NX.case_input(name)
    want, recorded = NX.load_expected(name)
    max_det = c.get("max_det", 300)
    det, count = NX.nms_exact(y, c["conf"], c["iou"], **NX.nms_kwargs(c))
    wdet, wcount = NX.padded(want, max_det)
    assert torch.equal(count, wcount), (count, wcount)
    assert NX.same_bits(det, wdet), "rows or their order differ from the reference's"
    info = NX.margin(y, c["conf"], c["iou"], **NX.nms_kwargs(c))
    margins = np.array([m[0] for m in info])
    print(f"[{name}] counts {count.tolist()[:8]} float64 margin {margins.min():.3e}")
    assert np.array_equal(margins, recorded), "the margin recorded with the fixture is not the margin of this input"
    if c["guarded"]:
        assert all(m[2] for m in info), "candidate scores repeat in a guarded case"
        assert margins.min() >= NX.MARGIN_MIN, margins
        for (_, rows64, _), w in zip(info, want):  # the float64 scan keeps the same set: the case is decided by the input, not by rounding
            assert NX.same_bits(rows64, w)


FAULTS = [("ge", "iou_equals_threshold"), ("class_compare", "high_class_offgrid"), ("no_max_nms", "nc80_over_max_nms"),
          ("no_max_nms", "nc3_max_nms_300"), ("unstable_ties", "tie_scores")]


@pytest.mark.parametrize("fault,name", FAULTS)
def test_planted_fault_in_the_restatement_is_flagged(fault, name):
    c = NX.CASES[name]
    y = NX.case_input(name)
    want, _ = NX.load_expected(name)
    wdet, wcount = NX.padded(want, c.get("max_det", 300))
    det, count = NX.nms_exact(y, c["conf"], c["iou"], **NX.nms_kwargs(c))
    assert NX.same_bits(det, wdet) and torch.equal(count, wcount)
    fdet, fcount = NX.nms_exact(y, c["conf"], c["iou"], fault=fault, **NX.nms_kwargs(c))
    assert not (NX.same_bits(fdet, wdet) and torch.equal(fcount, wcount)), f"the fixture does not notice {fault}"


def test_cases_cover_what_they_claim():
    """more than max_nms candidates, an image without candidates, an image where every candidate survives, ties of both kinds."""
    n = lambda name, b=0: NX.candidates(NX.case_input(name)[b], NX.CASES[name]["conf"], NX.CASES[name]["multi_label"], NX.CASES[name].get("classes"))
    assert n("nc80_over_max_nms")[1].numel() > 30000
    assert n("nc3_max_nms_300")[1].numel() > 300
    assert 19000 <= n("nc3_b3")[1].numel() <= 30000
    assert n("empty_and_all_survive", 1)[1].numel() == 0
    want, _ = NX.load_expected("empty_and_all_survive")
    assert len(want[1]) == 0 and len(want[2]) == n("empty_and_all_survive", 2)[1].numel() == 40
    s = n("tie_scores")[1]
    assert torch.unique(s).numel() < s.numel() // 4
    yb = NX.case_input("tie_best_class")[0, 4:]
    assert bool((yb == yb[0:1]).all())
    want, _ = NX.load_expected("tie_best_class")
    assert len(want[0]) and bool((want[0][:, 5] == 0).all())  # the first of the equal classes
    want, _ = NX.load_expected("high_class_offgrid")
    assert float(want[0][:, 5].min()) >= 60


# ---- utils.metrics against the reference --------------------------------------------------------------------------------------------
def _ref():
    return json.loads((GOLDEN / "val_metrics.json").read_text())


@pytest.mark.parametrize("name", list(NX.METRIC_CASES))
def test_metrics_equal_the_reference(name):
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import DetMetrics, box_iou, match_predictions

    ref = _ref()[name]
    iouv = torch.linspace(0.5, 0.95, 10)
    stats = NX.accumulate(NX.metric_case(name), box_iou, lambda pc, tc, iou: match_predictions(pc, tc, iou, iouv), iouv)
    assert np.array_equal(stats["tp"].astype(int).reshape(-1, 10), np.array(ref["tp"], dtype=int).reshape(-1, 10)), "tp matrices differ"
    dm = DetMetrics(names={i: str(i) for i in range(NX.METRIC_CASES[name]["nc"])})
    dm.process(**stats)
    assert list(dm.results_dict) == ref["keys"] == dm.keys + ["fitness"]
    b = dm.box
    for key, got in (("results", list(dm.results_dict.values())), ("p", b.p), ("r", b.r), ("f1", b.f1), ("ap", b.all_ap), ("maps", b.maps)):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        assert got.size == want.size and (got.shape == want.shape or got.size == 0), (key, got.shape, want.shape)
        err = float(np.abs(got - want).max()) if got.size else 0.0
        print(f"[{name}] {key}: max abs difference {err:.2e}")
        assert err <= 1e-9, (key, err)
    assert [int(v) for v in b.ap_class_index] == ref["ap_class_index"]
    assert dm.mean_results() == list(dm.results_dict.values())[:4] and dm.fitness == dm.results_dict["fitness"]


def test_metric_cases_cover_what_they_claim():
    ref = _ref()
    mixed = NX.metric_case("mixed")
    assert len(mixed[2][0]) == 0 and len(mixed[2][2]) > 0 and len(mixed[5][2]) == 0 and len(mixed[5][0]) > 0
    assert 0.05 < ref["mixed"]["results"][3] < 0.95  # neither trivial end
    absent = NX.metric_case("absent_class")
    pred = torch.cat([d[:, 5] for d, _, _ in absent])
    lab = torch.cat([c for _, _, c in absent])
    assert bool((pred == 3).any()) and not bool((lab == 3).any()) and bool((lab == 2).any()) and not bool((pred == 2).any())
    assert ref["no_detections"]["results"] == [0.0] * 5 and ref["no_labels"]["results"] == [0.0] * 5


def test_box_iou_equals_the_reference():
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import box_iou

    det, gt, _ = NX.metric_case("mixed")[0]
    got = box_iou(gt, det[:, :4])
    assert got.dtype == torch.float32
    assert np.array_equal(got.double().numpy(), np.array(_ref()["box_iou_mixed0"]))


def test_perfect_predictions_give_the_reference_arithmetics_0_995():
    """P = R = 1, and AP = 0.995: the closed curve's point (1, 0) is what the 101-point sampling reads at recall 1.0, in the reference as here."""
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import DetMetrics, box_iou, match_predictions

    iouv = torch.linspace(0.5, 0.95, 10)
    images = [(torch.cat((gt, (0.9 - 0.01 * torch.arange(len(gt)))[:, None], cls[:, None]), 1), gt, cls) for _, gt, cls in NX.metric_case("no_detections")]
    stats = NX.accumulate(images, box_iou, lambda pc, tc, iou: match_predictions(pc, tc, iou, iouv), iouv)
    dm = DetMetrics(names={0: "0", 1: "1"})
    dm.process(**stats)
    res = dm.results_dict
    assert abs(res["metrics/precision(B)"] - 1.0) <= 1e-9 and abs(res["metrics/recall(B)"] - 1.0) <= 1e-9
    assert abs(res["metrics/mAP50(B)"] - 0.995) <= 1e-9 and abs(res["metrics/mAP50-95(B)"] - 0.995) <= 1e-9


def test_post_processing_has_no_cpu_path():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.utils.ops import non_max_suppression

    y = NX.case_input("iou_equals_threshold")
    with pytest.raises(RuntimeError, match="MI355X|cuda"):
        ops.detect_nms(y, 0.25, 0.45)
    with pytest.raises(RuntimeError, match="MI355X|cuda"):
        non_max_suppression(y)
    with pytest.raises(RuntimeError, match="MI355X|cuda"):
        non_max_suppression((y, None), multi_label=True)
    y3 = NX.case_input("tie_scores")  # three class rows: nc=2 would make the third a mask channel
    for kw in (dict(rotated=True), dict(end2end=True), dict(labels=[torch.zeros(1, 5)]), dict(nc=2)):
        with pytest.raises(NotImplementedError):
            non_max_suppression(y3, **kw)


def test_nms_size_query_and_argument_checks_on_the_host():
    """the size query and the argument checks run before any launch, so they can be held to on a machine without a GPU."""
    import ctypes

    from improving_yolov8_cbam_swinblock_amd import _lib

    L = _lib.lib()
    wb = ctypes.c_size_t(0)
    assert L.ymi_detect_nms_sizes(32, 8400, 80, 30000, 300, ctypes.byref(wb)) == 0
    assert wb.value == 32 * 32768 * 8 + 128  # DESIGN section 1 row f5 quotes these
    assert L.ymi_detect_nms_sizes(16, 33600, 80, 30000, 300, ctypes.byref(wb)) == 0
    assert wb.value == 16 * 32768 * 8 + 64
    assert L.ymi_detect_nms_sizes(1, 100, 1, 30000, 300, ctypes.byref(wb)) == 0 and wb.value == 128 * 8 + 16  # never more keys than candidates can exist
    assert L.ymi_detect_nms_sizes(1, 8400, 80, 30000, 4096, ctypes.byref(wb)) == -1
    assert L.ymi_detect_nms_sizes(0, 8400, 80, 30000, 300, ctypes.byref(wb)) == -1
    one = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused before it launches
    args = lambda conf, iou, ws: (one, 1, 3, 8400, conf, iou, 1, 0, None, 0, 300, 30000, 7680.0, one, one, one, ws, None)
    assert L.ymi_detect_nms(*args(1.5, 0.5, 1 << 30)) == -1 and b"conf_thres" in L.ymi_last_error()
    assert L.ymi_detect_nms(*args(0.5, -0.1, 1 << 30)) == -1 and b"iou_thres" in L.ymi_last_error()
    assert L.ymi_detect_nms(*args(0.5, 0.5, 1024)) == -4 and b"workspace" in L.ymi_last_error()
