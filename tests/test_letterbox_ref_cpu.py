"""CPU: tests/letterbox_ref.py - the pure-torch restatement of the reference's inference path around the model that the GPU tests compare the
kernels with - held bit for bit to every fixture the real reference produced (tests/golden/make_predict_golden.py).

What the fixtures pin and what they cannot is said in that generator's DISCLOSURE: OpenCV is not installed where they were made, so the
interpolated pixel VALUES are pinned to the rule include/ymi.h writes out, not to OpenCV; sizes, offsets, ratio_pad, channel order, conversion,
the identity-size pixels, the boxes and the Boxes properties are the reference's own.  The resize rule is held separately to
F.interpolate in float64.  Boxes are compared as values (torch.equal: +0 and -0 compare equal)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import letterbox_ref as LR
from conftest import GOLDEN, load_golden

# float32 and float64 interpolation differ by 1.6e-3 to 1.7e-3 grey levels at worst over TABLE_CASES' shapes (printed below); pixels whose
# float64 value lies within 1e-2 - 6 times that - of a half grey level may round either way, everything else must agree
NEAR_HALF = 1e-2
NEAR_HALF_SHARE = 0.03  # the float64 reference alone puts 1.8-2.2 % of a case's pixels that near a half


def t(a):
    return torch.from_numpy(np.asarray(a))


def fixture_rp(d, i):
    return ((float(d[f"rp{i}_gain"]), float(d[f"rp{i}_gain"])), tuple(int(v) for v in d[f"rp{i}_pad"]))


def check_letterbox_case(name, fault=None):
    """every letterbox comparison of one case -> list of the names of those that fail"""
    d, c = load_golden(f"predict_{name}"), LR.CASES[name]
    sw, images, bad = LR.case_switches(c), LR.case_images(name), []
    outs, rps = zip(*[LR.letterbox_u8(im, c["new_shape"], fault=fault, **sw) for im in images])
    ref = t(d["out"])
    if tuple(torch.stack(outs).shape) != tuple(ref.shape):
        return ["shape"]
    if not torch.equal(torch.stack(outs), ref):
        bad.append("letterboxed image")
    if [list(rp[1]) for rp in rps] != d["pad_left_top"].tolist():
        bad.append("(left, top)")
    if "pre_u8" in d:
        got, _ = LR.letterbox(images, c["new_shape"], fault=fault, **sw)
        if got.dtype != torch.float32 or not torch.equal(got, t(d["pre_u8"]).float() / 255):
            bad.append("preprocess output")
    return bad


def check_boxes_case(name, fault=None):
    d, bad = load_golden(f"predict_{name}"), []
    img1 = tuple(d["out"].shape[1:3])
    for i, (_, h0, w0) in enumerate(LR.CASES[name]["images"]):
        boxes, img0 = LR.seeded_boxes(700 + i, 24, img1), (h0, w0)
        b4 = boxes[:, :4].contiguous()
        forms = {
            "none": LR.scale_rows(b4, LR.scale_boxes_params(img1, img0, None, fault), fault=fault),
            "rp": LR.scale_rows(b4, LR.scale_boxes_params(img1, img0, fixture_rp(d, i), fault), fault=fault),
            "nopad": LR.scale_rows(b4, LR.scale_boxes_params(img1, img0, None, fault), padding=False, fault=fault),
            "xywh": LR.scale_rows(b4, LR.scale_boxes_params(img1, img0, None, fault), xywh=True, fault=fault),
            "clip": LR.scale_rows(b4, (1.0, 0.0, 0.0, float(w0), float(h0)), padding=False, fault=fault),
            "rows": LR.scale_rows(boxes, LR.scale_boxes_params(img1, img0, None, fault), fault=fault),
        }
        bad += [f"{k}{i}" for k, v in forms.items() if not torch.equal(v, t(d[f"{k}{i}"]))]
    return bad


@pytest.mark.parametrize("name", list(LR.CASES))
def test_letterbox_restatement_equals_the_reference_bit_for_bit(name):
    assert check_letterbox_case(name) == []
    d, c = load_golden(f"predict_{name}"), LR.CASES[name]
    (hs, ws), (top, bottom, left, right), ratio = LR.geometry(c["images"][0][1:], c["new_shape"], **LR.case_switches(c))
    print(f"[{name}] {c['images'][0][1:]} -> {hs}x{ws} at (top {top}, left {left}) (bottom {bottom}, right {right}) in {d['out'].shape[1:3]}, ratio {ratio}")
    ident = (hs, ws) == tuple(c["images"][0][1:])
    if ident:  # wholly the reference's own pixels: the source bytes inside, 114 outside
        ref, img = t(d["out"])[0], t(LR.case_images(name)[0])
        assert torch.equal(ref[top : top + hs, left : left + ws], img)
        mask = torch.ones(ref.shape[:2], dtype=torch.bool)
        mask[top : top + hs, left : left + ws] = False
        assert bool((ref[mask] == LR.PAD_LEVEL).all())


def test_the_cases_cover_every_branch():
    geo = {n: LR.geometry(c["images"][0][1:], c["new_shape"], **LR.case_switches(c)) for n, c in LR.CASES.items()}
    assert geo["s37x53"][0] == (45, 64) and geo["s37x53"][1][:2] == (9, 10), "odd total padding: top != bottom"
    assert geo["s90x60"][1][2:] == (10, 11)
    assert geo["s48x64_identity"][0] == (48, 64) and geo["s64x64_nothing"][1] == (0, 0, 0, 0)
    assert geo["auto_shared"][0] == (58, 96) and geo["auto_shared"][1] == (3, 3, 0, 0)
    assert geo["scale_fill"][0] == (64, 64) and geo["scale_fill"][2] == (64 / 41, 64 / 70)
    assert geo["no_scaleup"][0] == (30, 44) and geo["no_scaleup"][2] == (1.0, 1.0)
    assert geo["not_centred"][1] == (0, 19, 0, 0)
    assert geo["odd_identity"][1][:2] == (9, 10)
    assert geo["rect_target"][0] == (64, 41)


def test_pre_transform_takes_auto_only_for_one_shape_with_rect():
    table = json.loads((GOLDEN / "predict_pre_transform.json").read_text())
    assert table == [["auto_shared", 1, 64, 96, 64, 96], ["auto_shared", 0, 96, 96, 96, 96], ["s37x53", 1, 96, 96, 96, 96]]
    for name, rect, *shapes in table:
        images = LR.case_images(name) + ([LR.seeded_image(520, 40, 53)] if name == "s37x53" else [])
        same = len({im.shape for im in images}) == 1
        outs = [LR.letterbox_u8(im, (96, 96), auto=bool(same and rect))[0] for im in images]
        assert [int(v) for o in outs for v in o.shape[:2]] == shapes


@pytest.mark.parametrize("name", list(LR.CASES))
def test_scale_boxes_restatement_equals_the_reference(name):
    assert check_boxes_case(name) == []


def test_scale_boxes_batch_form_keeps_rows_beyond_count_zero():
    det = torch.stack([LR.seeded_boxes(41, 10, (64, 64)), LR.seeded_boxes(42, 10, (64, 64))])
    count = torch.tensor([4, 0], dtype=torch.int32)
    out = LR.scale_boxes(det, count, (64, 64), [(37, 53), (90, 60)])
    assert bool((out[0, 4:] == 0).all()) and bool((out[1] == 0).all())
    assert torch.equal(out[0, :4], LR.scale_rows(det[0, :4], LR.scale_boxes_params((64, 64), (37, 53))))
    assert torch.equal(out[0, :4, 4:], det[0, :4, 4:])


def test_validator_preparation_equals_the_reference():
    d = load_golden("predict_val_prepare")
    batch, preds = LR.val_batch()
    for si in range(2):
        sel = batch["batch_idx"] == si
        got = LR.prepare_labels(batch["bboxes"][sel], LR.VAL_IMGSZ, batch["ori_shape"][si], batch["ratio_pad"][si])
        assert torch.equal(got, t(d[f"bbox{si}"])) and torch.equal(batch["cls"][sel].squeeze(-1), t(d[f"cls{si}"]))
        predn = LR.scale_rows(preds[si], LR.scale_boxes_params(LR.VAL_IMGSZ, batch["ori_shape"][si], batch["ratio_pad"][si]))
        assert torch.equal(predn, t(d[f"predn{si}"]))
        assert not torch.equal(predn[:, :4], preds[si][:, :4])


def test_boxes_properties_equal_the_reference():
    d = load_golden("predict_boxes")
    got = LR.boxes_properties(LR.seeded_boxes(801, 7, (37, 53)), (37, 53))
    assert int(d["n"]) == 7
    for k, v in got.items():
        assert torch.equal(v, t(d[k])), k


def test_the_packages_host_arithmetic_equals_the_restatements():
    """ops.letterbox_geometry, ops.scale_boxes_params, utils.ops.scale_boxes / clip_boxes on host tensors and engine.results.Boxes are host code:
    compared here, exactly, without a GPU"""
    from improving_yolov8_cbam_swinblock_amd.engine.results import Boxes, Results
    from improving_yolov8_cbam_swinblock_amd.ops.resize import letterbox_geometry, scale_boxes_params
    from improving_yolov8_cbam_swinblock_amd.utils import ops as uops

    for name, c in LR.CASES.items():
        d = load_golden(f"predict_{name}")
        sw, img1 = LR.case_switches(c), tuple(d["out"].shape[1:3])
        for i, (_, h0, w0) in enumerate(c["images"]):
            g = letterbox_geometry((h0, w0), c["new_shape"], **sw)
            assert g == LR.geometry((h0, w0), c["new_shape"], **sw)
            assert [g[1][2], g[1][0]] == d["pad_left_top"][i].tolist() and (g[1][0] + g[0][0] + g[1][1], g[1][2] + g[0][1] + g[1][3]) == img1
            rp = fixture_rp(d, i)
            assert tuple(scale_boxes_params(img1, (h0, w0))) == LR.scale_boxes_params(img1, (h0, w0))
            assert tuple(scale_boxes_params(img1, (h0, w0), rp)) == LR.scale_boxes_params(img1, (h0, w0), rp)
            boxes = LR.seeded_boxes(700 + i, 24, img1)
            b4 = boxes[:, :4].contiguous()
            x = b4.clone()
            assert uops.scale_boxes(img1, x, (h0, w0)) is x and torch.equal(x, t(d[f"none{i}"]))
            assert torch.equal(uops.scale_boxes(img1, b4.clone(), (h0, w0), ratio_pad=rp), t(d[f"rp{i}"]))
            assert torch.equal(uops.scale_boxes(img1, b4.clone(), (h0, w0), padding=False), t(d[f"nopad{i}"]))
            assert torch.equal(uops.scale_boxes(img1, b4.clone(), (h0, w0), xywh=True), t(d[f"xywh{i}"]))
            assert torch.equal(uops.clip_boxes(b4.clone(), (h0, w0)), t(d[f"clip{i}"]))
            full = boxes.clone()
            uops.scale_boxes(img1, full[:, :4], (h0, w0))  # a view of the [n, 6] rows, as construct_result passes it
            assert torch.equal(full, t(d[f"rows{i}"]))
    d = load_golden("predict_boxes")
    b = Boxes(LR.seeded_boxes(801, 7, (37, 53)), (37, 53))
    assert len(b) == 7 and b.orig_shape == (37, 53) and torch.equal(b.data, b.cpu().data)
    for k in ("xyxy", "conf", "cls", "xywh", "xyxyn", "xywhn"):
        assert torch.equal(getattr(b, k), t(d[k])), k
    r = Results((37, 53, 3), path="a.jpg", names={0: "0"}, boxes=b.data)
    assert r.orig_shape == (37, 53) and len(r.boxes) == 7 and r.names == {0: "0"} and r.path == "a.jpg"


@pytest.mark.parametrize("name", LR.TABLE_CASES[:6] + ["scale_fill", "auto_shared", "rect_target"])
def test_resize_rule_agrees_with_float64_interpolation(name):
    """the float32 rule against F.interpolate(double, bilinear, align_corners=False) followed by the same rounding: equal everywhere except on
    pixels whose float64 value lies within NEAR_HALF of a half grey level, where they may differ by one level; those are at most 3 % of a case"""
    c = LR.CASES[name]
    (hs, ws), _, _ = LR.geometry(c["images"][0][1:], c["new_shape"], **LR.case_switches(c))
    img = t(LR.case_images(name)[0])
    got = LR.resize_u8(img, (hs, ws)).to(torch.int64)
    v64 = F.interpolate(img.permute(2, 0, 1)[None].double(), size=(hs, ws), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    ref = (v64 + 0.5).floor().to(torch.int64)
    near = ((v64 - v64.floor()) - 0.5).abs() <= NEAR_HALF
    spread = float((LR.resize_values(img, (hs, ws)).double() - v64).abs().max())
    diff = (got - ref).abs()
    share = float(near.float().mean())
    print(f"[{name}] {tuple(img.shape[:2])} -> {hs}x{ws}: float32 vs float64 values differ by at most {spread:.2e} grey levels; {int((diff > 0).sum())} of "
          f"{diff.numel()} levels differ; {100 * share:.2f} % of the pixels lie within {NEAR_HALF} of a half level (bound {100 * NEAR_HALF_SHARE:.0f} %)")
    assert bool((diff[~near] == 0).all()), "a pixel away from a half level rounds differently"
    assert int(diff.max()) <= 1
    assert share <= NEAR_HALF_SHARE


FAULTS = {
    "no_tenth": ("s37x53", "letterbox"),    # dh / 2 = 9.5: round(9.5) is 10, round(9.4) is 9
    "floor": ("s37x53", "letterbox"),       # 37 * r = 44.68: 45, not 44
    "rgb": ("s37x53", "letterbox"),
    "pad0": ("s48x64_identity", "letterbox"),
    "no_clip": ("s37x53", "boxes"),
    "reciprocal": ("s90x60", "boxes"),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_faults_are_noticed(fault):
    name, kind = FAULTS[fault]
    check = check_letterbox_case if kind == "letterbox" else check_boxes_case
    assert check(name) == []
    bad = check(name, fault=fault)
    print(f"[{fault}] on {name}: {bad}")
    assert bad, f"the fixtures of {name} do not notice the planted fault {fault!r}"
    if fault == "no_tenth":  # the offset of scale_boxes' own derivation too: (64 - 45) / 2 = 9.5 rounds to 10, 9.4 to 9
        assert check_boxes_case("odd_identity", fault="no_tenth")
    if fault == "rgb":
        assert bad == ["preprocess output"], "the channel order is the conversion's, not LetterBox's"
