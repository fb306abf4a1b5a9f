"""GPU: the inference side of segmentation - ops.detect_nms_seg (csrc/nms.hip), ops.process_mask and ops.mask_overlap (csrc/maskdec.hip),
ops.val_match_masks (csrc/valmatch.hip), SegmentationPredictor and SegmentationValidator.

Every expectation comes from the reference's fixtures (tests/golden/make_segpred_golden.py), from tests/segpred_ref.py / tests/nms_exact.py
(held to those fixtures on the CPU by tests/test_segpred_cpu.py and tests/test_host_nms_check.py) or from utils.metrics on the host.  Masks on
exact inputs, NMS rows, integer counts and tp_m must be EQUAL; masks on real-valued inputs must agree wherever the float64 value is further
from 0 than the margin the generator recorded (four times the float32 reference's own distance from float64), and at most 0.1 % of the pixels
a box reaches may lie inside it."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import nms_exact as NX
import seg_common
import segpred_ref as SR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def fixture_masks(name, mode):
    c = SR.DECODE_CASES[name]
    n = 3 if name == "exact_160" else 12
    with np.load(GOLDEN / f"segpred_decode_{name}.npz") as z:
        return SR.unpack_masks(z[mode], (n, *(c["shape"] if mode == "up" else c["mhw"])))


# ---- mask decode -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["low", "up"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", ["exact_24x40", "exact_160"])
def test_process_mask_on_exact_inputs_equals_the_reference_bit_for_bit(name, dtype, mode):
    from improving_yolov8_cbam_swinblock_amd import ops

    proto, box, coef, img = SR.decode_case(name)
    shape = SR.DECODE_CASES[name]["shape"]
    want = fixture_masks(name, mode)
    p = proto.to(dev(), dtype)
    for layout in (p, p.contiguous(memory_format=torch.channels_last)):  # the kernels read NHWC memory: what Proto writes; NCHW is brought there
        mask, area = ops.process_mask(layout, box.to(dev()), coef.to(dev()), img.to(dev()), shape, upsample=mode == "up")
        torch.cuda.synchronize()
        assert mask.dtype == torch.uint8 and area.dtype == torch.int32 and tuple(mask.shape) == tuple(want.shape)
        bad = torch.nonzero(mask.cpu() != want)
        assert not len(bad), f"{len(bad)} pixels differ, first (row, y, x) {bad[0].tolist()}"
        assert torch.equal(area.cpu().long(), want.long().sum((1, 2))), "area is the mask's sum"
    assert int(want.sum()) > 1000


@pytest.mark.parametrize("mode", ["low", "up"])
def test_process_mask_on_real_inputs_agrees_outside_the_recorded_margin(mode):
    from improving_yolov8_cbam_swinblock_amd import ops

    proto, box, coef, img = SR.decode_case("real_24x40")
    note = json.loads((GOLDEN / "segpred_decode.json").read_text())["real_24x40"][mode]
    want = fixture_masks("real_24x40", mode).bool()
    v64 = SR.process_mask_values(proto, box, coef, img, (96, 160), mode == "up", torch.float64)
    mask, area = ops.process_mask(proto.to(dev(), torch.bfloat16), box.to(dev()), coef.to(dev()), img.to(dev()), (96, 160), upsample=mode == "up")
    torch.cuda.synchronize()
    got = mask.cpu().bool()
    open_ = (v64 != 0) & (v64.abs() < note["margin"])
    reached = int((v64 != 0).sum())
    print(f"[real {mode}] margin {note['margin']:.3e}, {int(open_.sum())} of {reached} reached pixels inside it, "
          f"{int((got != want).sum())} pixels differ from the reference anywhere")
    assert int(open_.sum()) <= 0.001 * reached
    bad = torch.nonzero((got != want) & ~open_)
    assert not len(bad), f"{len(bad)} pixels outside the margin differ, first {bad[0].tolist()} value {float(v64[tuple(bad[0].tolist())]):.3e}"
    assert torch.equal(area.cpu().long(), got.long().sum((1, 2)))


def test_utils_process_mask_takes_device_tensors_to_the_kernel():
    from improving_yolov8_cbam_swinblock_amd.utils.ops import process_mask

    proto, box, coef, img = SR.decode_case("exact_24x40")
    for mode, up in (("low", False), ("up", True)):
        want = fixture_masks("exact_24x40", mode)
        for b in range(2):
            sel = torch.nonzero(img == b).reshape(-1)
            got = process_mask(proto[b].to(dev()), coef[sel].to(dev()), box[sel].to(dev()), (96, 160), upsample=up)
            assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want[sel])


def test_mask_kernels_refuse_other_prototype_counts_and_other_encoding_sizes():
    from improving_yolov8_cbam_swinblock_amd import _lib, ops

    L = _lib.lib()
    proto = torch.zeros(1, 4, 4, 16, device=dev()).permute(0, 3, 1, 2)
    t = _lib.as_ymi(proto)
    z = torch.zeros(64, device=dev())
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    assert L.ymi_process_mask(ctypes.byref(t), p(z), p(z), p(z), 1, 16, 16, 0, p(z), p(z), None) == -1
    assert "nm = 32" in L.ymi_last_error().decode()
    proto = torch.zeros(1, 32, 8, 8, device=dev())
    det, coef, count = torch.zeros(1, 4, 6, device=dev()), torch.zeros(1, 4, 32, device=dev()), torch.zeros(1, dtype=torch.int32, device=dev())
    with pytest.raises(NotImplementedError, match="resampl"):
        ops.mask_overlap(det, coef, count, proto, torch.zeros(1, 16, 16, dtype=torch.uint8, device=dev()), (32, 32))
    t = _lib.as_ymi(proto.contiguous(memory_format=torch.channels_last))
    assert L.ymi_mask_overlap(p(det), p(coef), p(count), 1, 4, ctypes.byref(t), 32, 32, p(z), 0, 16, 16, 256, p(z), p(z), p(z), None) == -1
    assert "resample" in L.ymi_last_error().decode()


# ---- NMS rows with coefficients ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nms_expectation(name):
    c = NX.CASES[name]
    y = NX.case_input(name)
    return y, NX.nms_exact(y, c["conf"], c["iou"], **NX.nms_kwargs(c))


@pytest.mark.parametrize("nm", [32, 5])
@pytest.mark.parametrize("name", list(NX.CASES))
def test_detect_nms_seg_keeps_detect_nms_rows_and_gathers_the_coefficients(name, nm):
    from improving_yolov8_cbam_swinblock_amd import ops

    c = NX.CASES[name]
    y, (want_det, want_count) = nms_expectation(name)
    y_seg = SR.with_coefficients(y, nm, 100 + nm)
    kw = NX.nms_kwargs(c)
    det, coef, count = ops.detect_nms_seg(y_seg.to(dev()), c["nc"], c["conf"], c["iou"], **kw)
    pdet, pcount = ops.detect_nms(y.to(dev()), c["conf"], c["iou"], **kw)
    torch.cuda.synchronize()
    det, coef, count = det.cpu(), coef.cpu(), count.cpu()
    assert torch.equal(count, want_count) and torch.equal(count, pcount.cpu())
    assert NX.same_bits(det, want_det), "rows differ from nms_exact"
    assert NX.same_bits(det, pdet.cpu()), "rows differ from ops.detect_nms on y[:, :4 + nc]"
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (y.shape[0], det.shape[1], nm)
    assert NX.same_bits(coef, SR.kept_coefficients(y_seg, c["nc"], det, count)), "coefficient rows (zero padding included)"


def test_non_max_suppression_with_mask_channels_equals_the_reference_rows():
    from improving_yolov8_cbam_swinblock_amd.utils.ops import non_max_suppression

    s = SR.SEG_NMS
    c = NX.CASES[s["case"]]
    y = SR.with_coefficients(NX.case_input(s["case"]), s["nm"], s["seed"]).to(dev())
    before = y.clone()
    with np.load(GOLDEN / "segpred_nms.npz") as z:
        rows, counts = torch.from_numpy(z["rows"]), z["counts"].tolist()
    out = non_max_suppression((y, None), c["conf"], c["iou"], multi_label=c["multi_label"], nc=c["nc"])
    assert torch.equal(y, before) and [len(o) for o in out] == counts
    assert all(o.is_cuda and o.shape[1] == 6 + s["nm"] for o in out) and NX.same_bits(torch.cat(out, 0).cpu(), rows)


# ---- overlap counts and mask matching ----------------------------------------------------------------------------------------------------------
MATCH_CASES = {
    "reference": SR.REF_MATCH,
    "planted_tie": dict(seed=41, counts=[40, 3], labels=[3, 2], max_det=48, nc=3, planted_tie=True),
    "repeats": dict(seed=42, counts=[100, 0, 7, 64], labels=[9, 5, 0, 30], max_det=100, nc=4),     # identical masks: equal overlaps between detections
    "long_table": dict(seed=43, counts=[30] * 6, labels=[200] * 6, max_det=32, nc=5),             # 1200 rows: the table passes through LDS twice
}


def _device_counts(case, enc=None, n_bins=256):
    from improving_yolov8_cbam_swinblock_amd import ops

    det, coef, count = case["det"].to(dev()), case["coef"].to(dev()), case["count"].to(dev())
    enc = case["enc"] if enc is None else enc
    return (det, count) + ops.mask_overlap(det, coef, count, case["proto"].to(dev(), torch.bfloat16), enc.to(dev()), case["shape"], n_bins=n_bins)


def _device_masks(case):
    """ops.process_mask(upsample=False) on every row of the batch, rows past the count included (their result is not used)."""
    from improving_yolov8_cbam_swinblock_amd import ops

    B, max_det = case["det"].shape[:2]
    img = torch.arange(B, dtype=torch.int32).repeat_interleave(max_det)
    mask, _ = ops.process_mask(case["proto"].to(dev(), torch.bfloat16), case["det"].view(-1, 6)[:, :4].to(dev()), case["coef"].view(-1, SR.NM).to(dev()),
                               img.to(dev()), case["shape"])
    return mask.cpu().view(B, max_det, *mask.shape[1:])


@pytest.mark.parametrize("name", list(MATCH_CASES))
def test_mask_overlap_and_val_match_masks_equal_the_host_path(name):
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import mask_iou, match_predictions

    case = SR.match_case(**MATCH_CASES[name])
    masks = _device_masks(case)
    want = SR.overlap_counts(masks, case["count"], case["enc"], 256)
    det, count, inter, area_pred, area_gt = _device_counts(case)
    for got, w, what in zip((inter, area_pred, area_gt), want, ("inter", "area_pred", "area_gt")):
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), w), what
    f_inter, f_pred, f_gt = _device_counts(case, enc=case["enc"].float())[2:]
    assert torch.equal(f_inter, inter) and torch.equal(f_pred, area_pred) and torch.equal(f_gt, area_gt), "a float32 encoding counts the same"
    assert int(area_pred.sum()) > 0 and int(inter[..., 1:].sum()) > 0
    tp_m = ops.val_match_masks(det, count, case["lab_img"].to(dev()), case["lab_cls"].to(dev()).reshape(-1, 1), inter, area_pred, area_gt, SR.IOUV)
    torch.cuda.synchronize()
    assert tp_m.dtype == torch.uint8 and tuple(tp_m.shape) == (*case["det"].shape[:2], 10)
    host = SR.tp_m_host(masks, case, match_predictions, mask_iou)
    bad = torch.nonzero(tp_m.cpu() != host)
    assert not len(bad), f"{len(bad)} tp_m elements differ from mask_iou + match_predictions, first (image, detection, level) {bad[0].tolist()}"
    assert torch.equal(SR.tp_m_from_counts(*want, case, match_predictions), host)
    print(f"[{name}] tp_m hits per level {host.sum((0, 1)).tolist()}")
    assert int(host[..., 0].sum()) > 0
    if name == "reference":
        with np.load(GOLDEN / "segpred_match.npz") as z:
            assert torch.equal(tp_m.cpu(), torch.from_numpy(z["tp_m"])), "the reference's _process_batch(masks=True, overlap=True)"
    if name == "planted_tie":
        assert int(inter[0, 0].cpu().eq(24).sum()) == 2, "detection 0 overlaps two labels equally"
        low = ops.val_match_masks(det, count, case["lab_img"].to(dev()), case["lab_cls"].to(dev()), inter, area_pred, area_gt, [0.3])
        assert torch.equal(low.cpu(), SR.tp_m_host(masks, case, match_predictions, mask_iou, iouv=torch.tensor([0.3]))) and int(low[0, 0, 0]) == 1
    if name == "repeats":
        single = ops.val_match_masks(det, count, case["lab_img"].to(dev()), case["lab_cls"].to(dev()), inter, area_pred, area_gt, SR.IOUV, single_cls=True)
        want_single = SR.tp_m_host(masks, case, match_predictions, mask_iou, single_cls=True)
        assert torch.equal(single.cpu(), want_single) and int(want_single.sum()) > int(host.sum())


def test_labels_beyond_the_bins_overlap_nothing_and_rows_past_the_count_are_zero():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import match_predictions

    case = SR.match_case(**MATCH_CASES["repeats"])
    masks = _device_masks(case)
    want = SR.overlap_counts(masks, case["count"], case["enc"], 4)
    det, count, inter, area_pred, area_gt = _device_counts(case, n_bins=4)
    assert tuple(inter.shape) == (4, 100, 4) and all(torch.equal(g.cpu(), w) for g, w in zip((inter, area_pred, area_gt), want))
    past = torch.arange(100)[None] >= case["count"][:, None]
    assert int(inter.cpu()[past].abs().sum()) == 0 and int(area_pred.cpu()[past].abs().sum()) == 0
    tp_m = ops.val_match_masks(det, count, case["lab_img"].to(dev()), case["lab_cls"].to(dev()), inter, area_pred, area_gt, SR.IOUV)
    assert torch.equal(tp_m.cpu(), SR.tp_m_from_counts(*want, case, match_predictions))
    assert int(tp_m.cpu()[past].sum()) == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def e2e_model(cfg):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    model = SegmentationModel(cfg, ch=3, nc=seg_common.E2E_NC)
    model.load_state_dict(seg_common.e2e_state(model), strict=True)
    return model.to(dev()).eval()


@pytest.mark.parametrize("cfg", list(seg_common.E2E_MODELS.values()))
def test_predictor_returns_boxes_and_masks_equal_to_the_composition_of_the_ops(cfg):
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.predictor import SegmentationPredictor
    from improving_yolov8_cbam_swinblock_amd.engine.results import Masks

    model = e2e_model(cfg)
    rs = np.random.RandomState(3)
    images = [rs.randint(0, 256, size=(96, 128, 3)).astype(np.uint8), rs.randint(0, 256, size=(150, 100, 3)).astype(np.uint8)]
    pred = SegmentationPredictor(model, imgsz=128, conf=1e-4, iou=0.7, max_det=20)
    results = pred(images, paths=["a", "b"])
    assert len(results) == 2 and sum(len(r) for r in results) > 0, "no detection at this confidence"
    with torch.no_grad():
        img, ori = pred.preprocess(images)
        y, (_, _, proto) = pred.inference(img)
        det, coef, count = ops.detect_nms_seg(y, 3, 1e-4, 0.7, max_det=20)
        counts = count.tolist()
        scaled = ops.scale_boxes(det.clone(), count, (128, 128), ori)
    for k, r in enumerate(results):
        n = counts[k]
        masks, area = ops.process_mask(proto, det[k, :n, :4], coef[k, :n], torch.full((n,), k, dtype=torch.int32), (128, 128), upsample=True)
        keep = area > 0
        assert r.orig_shape == tuple(images[k].shape[:2]) and r.path == "ab"[k]
        assert NX.same_bits(r.boxes.data, scaled[k, :n][keep])
        if int(keep.sum()):
            assert isinstance(r.masks, Masks) and r.masks.data.dtype == torch.uint8 and tuple(r.masks.shape) == (len(r), 128, 128)
            assert torch.equal(r.masks.data, masks[keep]) and int(r.masks.data.sum((1, 2)).min()) > 0, "no all-zero mask is kept"
            assert torch.equal(r.cpu().masks.data, masks[keep].cpu())
        else:
            assert r.masks is None and len(r) == 0
    assert any(r.masks is not None for r in results)


@pytest.mark.parametrize("cfg", list(seg_common.E2E_MODELS.values()))
def test_validator_device_and_host_paths_agree(cfg):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_seg_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import SegmentationValidator
    from improving_yolov8_cbam_swinblock_amd.utils.metrics import SegmentMetrics

    model = e2e_model(cfg)
    batch = synthetic_seg_batch(2, 128, dev(), 5)
    batch["cls"] = (torch.arange(8, device=dev()) % 3).float().view(-1, 1)
    out, stats = {}, {}
    for match in ("device", "host"):
        v = SegmentationValidator(model, conf=1e-4, max_det=50, match=match, loss=match == "device")
        out[match] = v(batch)
        stats[match] = {k: torch.cat(s, 0) for k, s in v.stats.items()}
        assert v.seen == 2 and not model.training
    assert len(stats["host"]["tp"]) > 0, "no detection at this confidence"
    for k in ("tp", "tp_m", "conf", "pred_cls", "target_cls"):
        assert torch.equal(stats["device"][k], stats["host"][k]), k
    assert stats["host"]["tp_m"].shape == stats["host"]["tp"].shape and stats["host"]["tp_m"].dtype == torch.bool
    keys = SegmentMetrics.keys + ["fitness"]
    assert list(out["host"]) == keys and len(keys) == 9
    assert all(out["device"][k] == out["host"][k] for k in keys)
    loss = [out["device"][k] for k in ("val/box_loss", "val/seg_loss", "val/cls_loss", "val/dfl_loss")]
    assert all(np.isfinite(loss)) and loss[1] > 0


def test_captured_graph_of_forward_nms_overlap_and_matching_replays_on_new_data():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_seg_batch

    model = e2e_model("yolov8n-seg.yaml")
    batches = [synthetic_seg_batch(2, 128, dev(), s) for s in (7, 8)]
    lab_img, lab_cls = batches[0]["batch_idx"].to(torch.int32), (torch.arange(8, device=dev()) % 3).float()  # (both batches: four boxes per image)

    def eager(x, enc):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y, (_, _, proto) = model(x)
            det, coef, count = ops.detect_nms_seg(y, 3, 1e-4, 0.7, multi_label=True, max_det=50)
            counts = ops.mask_overlap(det, coef, count, proto, enc, (128, 128))
            return (det, coef, count) + counts + (ops.val_match_masks(det, count, lab_img, lab_cls, *counts, SR.IOUV),)

    x, enc = batches[0]["img"].clone(), batches[0]["masks"].clone()
    for _ in range(2):
        eager(x, enc)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = eager(x, enc)
    for b in (batches[1], batches[0]):
        x.copy_(b["img"])
        enc.copy_(b["masks"])
        graph.replay()
        torch.cuda.synchronize()
        rep = [t.cpu().clone() for t in held]
        want = [t.cpu() for t in eager(b["img"], b["masks"])]
        assert int(want[2].sum()) > 0 and int(want[4].sum()) > 0, "no detection, or no mask pixel"
        for i, (g, w) in enumerate(zip(rep, want)):
            assert NX.same_bits(g, w), f"output {i} differs between replay and eager"
