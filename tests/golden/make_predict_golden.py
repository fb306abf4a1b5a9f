"""Generate the prediction-path fixtures under tests/golden/ by running the REAL reference on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/make_predict_golden.py

Same import shim as make_val_golden.py (cv2 stubbed, the torchvision version patched, YOLO_OFFLINE).  What runs is the reference's own LetterBox
(data/augment.py:1479-1603), BasePredictor.preprocess and pre_transform (engine/predictor.py:144-191; unbound, on a namespace that carries imgsz,
args.rect, device and a model stub with pt, fp16 and stride), ops.scale_boxes and ops.clip_boxes (utils/ops.py:93-127, :335-354),
DetectionValidator._prepare_batch and _prepare_pred (models/yolo/detect/val.py:135-172; unbound, on a namespace that carries the device) and
Boxes (engine/results.py:1041-1256).

DISCLOSURE: OpenCV is not installed here, so the two cv2 calls inside LetterBox are supplied by this file - OUR code, not the reference's and not
OpenCV's.  `copy_make_border` is a constant border.  `resize` is the rule include/ymi.h writes out for ymi_letterbox_batch (the float32
bilinear formula at OpenCV INTER_LINEAR's source coordinate (dst + 0.5) * (in / out) - 0.5 on the byte values, rounded by floor(v + 0.5)),
taken from tests/letterbox_ref.py.  So the fixtures pin everything the reference DECIDES - interpolated size, offsets, ratio_pad, channel order,
conversion, scaled and clipped boxes, Boxes properties - and the pixel values of the identity-size cases are wholly the reference's own; the
interpolated pixel values are pinned to the stated rule only.  OpenCV itself interpolates uint8 images with 11-bit fixed-point coefficients and
may differ from the exactly rounded value by one grey level; no fixture here can say anything about that.

The inputs are rebuilt from seeds by tests/letterbox_ref.py (seeded_image, seeded_boxes, val_batch); the fixtures hold expected outputs only."""
import importlib.metadata as md
import os
import sys
from pathlib import Path
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import letterbox_ref as LR  # noqa: E402

INTER_LINEAR, BORDER_CONSTANT = 1, 0


def resize(img, dsize, interpolation=None):
    """stand-in for cv2.resize (see DISCLOSURE above); dsize is (width, height) as OpenCV takes it"""
    assert interpolation == INTER_LINEAR and img.dtype == np.uint8 and img.ndim == 3
    return LR.resize_u8(torch.from_numpy(np.ascontiguousarray(img)), (int(dsize[1]), int(dsize[0]))).numpy()


def copy_make_border(img, top, bottom, left, right, border_type, value=None):
    """stand-in for cv2.copyMakeBorder with BORDER_CONSTANT (see DISCLOSURE above)"""
    assert border_type == BORDER_CONSTANT and min(top, bottom, left, right) >= 0
    h, w, c = img.shape
    out = np.empty((h + top + bottom, w + left + right, c), dtype=img.dtype)
    out[...] = np.asarray(value[:c], dtype=img.dtype)
    out[top : top + h, left : left + w] = img
    return out


def import_reference():
    os.environ.setdefault("YOLO_OFFLINE", "true")
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/ulcfg")
    os.environ.setdefault("YOLO_VERBOSE", "false")
    cv2 = MagicMock(__version__="4.10.0")
    cv2.resize, cv2.copyMakeBorder, cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = resize, copy_make_border, INTER_LINEAR, BORDER_CONSTANT
    sys.modules.setdefault("cv2", cv2)
    orig = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else orig(n)
    sys.path.insert(0, str(REF))
    import ultralytics.data.augment as augment
    import ultralytics.engine.predictor as predictor
    import ultralytics.engine.results as results
    import ultralytics.utils.ops as ops
    from ultralytics.models.yolo.detect.val import DetectionValidator

    assert augment.cv2.resize is resize and augment.cv2.copyMakeBorder is copy_make_border
    return augment, predictor, results, ops, DetectionValidator


def save(name, **arrays):
    path = OUT / f"{name}.npz"
    np.savez_compressed(path, **arrays)
    print(f"{name}.npz  {path.stat().st_size / 1024:.1f} kB", flush=True)


def letterbox_fixtures(augment, predictor, ops):
    for name, c in LR.CASES.items():
        sw = LR.case_switches(c)
        images = LR.case_images(name)
        lb = augment.LetterBox(c["new_shape"], **sw)
        outs = [lb(image=im.copy()) for im in images]
        assert all(o.dtype == np.uint8 for o in outs)
        # ratio_pad as LetterBox states it for a dataset: labels["ratio_pad"] = (what was there, (left, top)); the image goes in as labels["img"]
        labelled = [lb(labels={"img": im.copy(), "ratio_pad": "RATIO", "instances": MagicMock()}) for im in images]
        pads = np.array([lab["ratio_pad"][1] for lab in labelled], dtype=np.int64)
        assert all(lab["ratio_pad"][0] == "RATIO" and np.array_equal(lab["img"], o) for lab, o in zip(labelled, outs))
        # BasePredictor.preprocess with this LetterBox as its pre_transform (pre_transform itself is run below where its own switches apply)
        holder = SimpleNamespace(device=torch.device("cpu"), model=SimpleNamespace(fp16=False), pre_transform=lambda im: [lb(image=x) for x in im])
        pre = predictor.BasePredictor.preprocess(holder, [im.copy() for im in images])
        u8 = (pre * 255).round().to(torch.uint8)
        assert pre.dtype == torch.float32 and torch.equal(u8.float() / 255, pre), "the fixture stores preprocess's output as the bytes it is exactly k / 255 of"
        # boxes: scale_boxes in its forms, on the letterboxed image's pixel grid
        img1, arrays = tuple(outs[0].shape[:2]), {}
        for i, im in enumerate(images):
            img0 = tuple(im.shape[:2])
            boxes = LR.seeded_boxes(700 + i, 24, img1)
            arrays[f"none{i}"] = ops.scale_boxes(img1, boxes[:, :4].clone(), img0).numpy()
            gain = min(img1[0] / img0[0], img1[1] / img0[1])
            rp = ((gain * 1.01, gain * 1.01), (int(pads[i][0]) + 1, int(pads[i][1])))  # a ratio_pad that differs from the derived one
            arrays[f"rp{i}"] = ops.scale_boxes(img1, boxes[:, :4].clone(), img0, ratio_pad=rp).numpy()
            arrays[f"rp{i}_gain"] = np.float64(rp[0][0])
            arrays[f"rp{i}_pad"] = np.array(rp[1], dtype=np.int64)
            arrays[f"nopad{i}"] = ops.scale_boxes(img1, boxes[:, :4].clone(), img0, padding=False).numpy()
            arrays[f"xywh{i}"] = ops.scale_boxes(img1, boxes[:, :4].clone(), img0, xywh=True).numpy()
            arrays[f"clip{i}"] = ops.clip_boxes(boxes[:, :4].clone(), img0).numpy()
            full = boxes.clone()
            full[:, :4] = ops.scale_boxes(img1, full[:, :4], img0)  # as construct_result calls it: a view of the [n, 6] rows
            arrays[f"rows{i}"] = full.numpy()
        if name in LR.PRE_CASES:  # (the conversion is the same statement for every case: three fixtures carry its output)
            arrays["pre_u8"] = u8.numpy()
        save(f"predict_{name}", out=np.stack(outs), pad_left_top=pads, **arrays)


def pre_transform_fixture(predictor):
    """pre_transform's own switch: auto = same shapes and rect and model.pt"""
    table = []
    for name, rect in (("auto_shared", True), ("auto_shared", False), ("s37x53", True)):
        images = LR.case_images(name)
        if name == "s37x53":
            images = images + [LR.seeded_image(520, 40, 53)]  # two shapes: never auto
        holder = SimpleNamespace(imgsz=(96, 96), args=SimpleNamespace(rect=rect), model=SimpleNamespace(pt=True, stride=32, fp16=False))
        outs = predictor.BasePredictor.pre_transform(holder, images)
        table.append([name, int(rect)] + [int(v) for o in outs for v in o.shape[:2]])
    return table


def validator_fixture(DetectionValidator):
    batch, preds = LR.val_batch()
    batch["img"] = torch.zeros(2, 3, *LR.VAL_IMGSZ)
    holder = SimpleNamespace(device=torch.device("cpu"))
    arrays = {}
    for si in range(2):
        pb = DetectionValidator._prepare_batch(holder, si, batch)
        arrays[f"bbox{si}"], arrays[f"cls{si}"] = pb["bbox"].numpy(), pb["cls"].numpy()
        arrays[f"predn{si}"] = DetectionValidator._prepare_pred(holder, preds[si].clone(), pb).numpy()
    save("predict_val_prepare", **arrays)


def boxes_fixture(results):
    data = LR.seeded_boxes(801, 7, (37, 53))
    b = results.Boxes(data.clone(), (37, 53))
    save("predict_boxes", **{k: getattr(b, k).numpy() for k in ("xyxy", "conf", "cls", "xywh", "xyxyn", "xywhn")}, n=np.int64(len(b)))


if __name__ == "__main__":
    import json

    torch.set_num_threads(8)
    ref_augment, ref_predictor, ref_results, ref_ops, ref_validator = import_reference()
    letterbox_fixtures(ref_augment, ref_predictor, ref_ops)
    (OUT / "predict_pre_transform.json").write_text(json.dumps(pre_transform_fixture(ref_predictor)) + "\n")
    validator_fixture(ref_validator)
    boxes_fixture(ref_results)
