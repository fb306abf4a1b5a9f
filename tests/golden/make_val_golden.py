"""Generate the post-processing and validation fixtures under tests/golden/ by running the REAL reference on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/make_val_golden.py --choose-seeds   # once: picks the per-image seeds -> nms_seeds.json
    python tests/golden/make_val_golden.py                  # nms_<case>.npz and val_metrics.json from the committed seeds

Same import shim as make_golden.py (cv2 stubbed, the torchvision version patched, YOLO_OFFLINE).  What runs is the reference's own
non_max_suppression, box_iou, BaseValidator.match_predictions (unbound, on a namespace that carries iouv), ap_per_class and DetMetrics.

DISCLOSURE: torchvision is not installed here, so `torchvision.ops.nms`, the one call inside the reference's wrapper that the reference
does not contain, is supplied by `greedy_nms` below - OUR code, written out from the operator's definition (stable descending sort by
score; area = (x2 - x1) * (y2 - y1); inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)); iou = inter / (area_i + area_j -
inter); suppress when iou > threshold; float32 throughout).  Everything around it is the reference's: candidate rules, multi_label
expansion, class filter, class offset, max_nms cut, max_det.

The inputs are rebuilt from seeds by tests/nms_exact.py (cluster_image, special_input, metric_case); the fixtures hold only expected rows,
counts, tp matrices, metric values and the recorded float64 margins."""
import importlib.metadata as md
import json
import os
import sys
import types
from pathlib import Path
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import nms_exact as NX  # noqa: E402


def import_reference():
    os.environ.setdefault("YOLO_OFFLINE", "true")
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/ulcfg")
    os.environ.setdefault("YOLO_VERBOSE", "false")
    sys.modules.setdefault("cv2", MagicMock(__version__="4.10.0"))
    orig = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else orig(n)
    sys.path.insert(0, str(REF))
    import ultralytics.engine.validator as validator
    import ultralytics.utils.metrics as metrics
    import ultralytics.utils.ops as ops

    tv = types.ModuleType("torchvision")
    tv.ops = types.ModuleType("torchvision.ops")
    tv.ops.nms = greedy_nms
    sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, tv.ops
    return ops, metrics, validator


def greedy_nms(boxes, scores, iou_threshold):
    """stand-in for torchvision.ops.nms (see DISCLOSURE above) -> indices of the kept boxes in descending score order."""
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes[order].float()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr = torch.tensor(iou_threshold, dtype=torch.float32)
    dead = torch.zeros(len(b), dtype=torch.bool)
    keep = []
    for i in range(len(b)):
        if dead[i]:
            continue
        keep.append(i)
        w = (torch.minimum(b[i, 2], b[i + 1 :, 2]) - torch.maximum(b[i, 0], b[i + 1 :, 0])).clamp(min=0)
        h = (torch.minimum(b[i, 3], b[i + 1 :, 3]) - torch.maximum(b[i, 1], b[i + 1 :, 1])).clamp(min=0)
        inter = w * h
        dead[i + 1 :] |= inter / ((area[i] + area[i + 1 :]) - inter) > thr
    return order[torch.tensor(keep, dtype=torch.long)]


def case_args(c):
    return dict(conf_thres=c["conf"], iou_thres=c["iou"], **NX.nms_kwargs(c))


def image_ok(yi, c):
    gap, _, distinct = NX.margin(yi[None], **case_args(c))[0]
    return gap >= 2 * NX.MARGIN_MIN and distinct, gap


def choose_seeds():
    """per image of every seeded case the first seed (counting up from a per-case base) whose input has distinct candidate scores and a
    float64 margin of at least twice MARGIN_MIN."""
    seeds = {}
    for ci, (name, c) in enumerate(NX.CASES.items()):
        want = c["B"] if c["kind"] == "cluster" else (1 if name == "empty_and_all_survive" else 0)
        got, s = [], 1000 * (ci + 1)
        while len(got) < want:
            yi = torch.from_numpy(NX.case_image(c, s))
            ok, gap = image_ok(yi, c)
            print(f"{name}: seed {s} margin {gap:.2e} {'taken' if ok else 'passed over'}", flush=True)
            if ok:
                got.append(s)
            s += 1
        if want:
            seeds[name] = got
    (OUT / "nms_seeds.json").write_text(json.dumps(seeds, indent=1) + "\n")


def nms_fixtures(ops):
    seeds = NX.load_seeds()
    for name, c in NX.CASES.items():
        y = NX.case_input(name, seeds)
        res = ops.non_max_suppression(y.clone(), c["conf"], c["iou"], classes=c.get("classes"), agnostic=c.get("agnostic", False),
                                      multi_label=c["multi_label"], max_det=c.get("max_det", 300), max_nms=c.get("max_nms", 30000),
                                      max_time_img=1e6)
        info = NX.margin(y, **case_args(c))
        margins = np.array([m[0] for m in info], dtype=np.float64)
        if c["guarded"]:
            assert all(m[2] for m in info) and margins.min() >= NX.MARGIN_MIN, (name, margins)
        rows = torch.cat([r.float() for r in res], 0).numpy() if any(len(r) for r in res) else np.zeros((0, 6), np.float32)
        path = OUT / f"nms_{name}.npz"
        np.savez_compressed(path, rows=rows.astype(np.float32), counts=np.array([len(r) for r in res], dtype=np.int32), margins=margins)
        print(f"nms_{name}.npz  {path.stat().st_size / 1024:.1f} kB  counts {[len(r) for r in res][:8]} margin {margins.min():.2e}", flush=True)


def metric_fixtures(metrics, validator):
    iouv = torch.linspace(0.5, 0.95, 10)
    holder = SimpleNamespace(iouv=iouv)
    match = lambda pc, tc, iou: validator.BaseValidator.match_predictions(holder, pc, tc, iou)  # noqa: E731
    out = {}
    for name, c in NX.METRIC_CASES.items():
        images = NX.metric_case(name)
        stats = NX.accumulate(images, metrics.box_iou, match, iouv)
        dm = metrics.DetMetrics(names={i: str(i) for i in range(c["nc"])})
        dm.process(**stats)
        b = dm.box
        out[name] = dict(
            tp=stats["tp"].astype(int).tolist(),
            results=[float(v) for v in dm.results_dict.values()],
            keys=list(dm.results_dict.keys()),
            p=np.asarray(b.p, dtype=np.float64).tolist(),
            r=np.asarray(b.r, dtype=np.float64).tolist(),
            f1=np.asarray(b.f1, dtype=np.float64).tolist(),
            ap=np.asarray(b.all_ap, dtype=np.float64).tolist(),
            ap_class_index=[int(v) for v in b.ap_class_index],
            maps=np.asarray(b.maps, dtype=np.float64).tolist(),
        )
        print(name, {k: round(v, 4) for k, v in zip(out[name]["keys"], out[name]["results"])}, flush=True)
    # box_iou on its own: a few rows of the first case
    det, gt, _ = NX.metric_case("mixed")[0]
    out["box_iou_mixed0"] = metrics.box_iou(gt, det[:, :4]).double().numpy().tolist()
    (OUT / "val_metrics.json").write_text(json.dumps(out) + "\n")


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--choose-seeds" in sys.argv:
        choose_seeds()
    else:
        ref_ops, ref_metrics, ref_validator = import_reference()
        nms_fixtures(ref_ops)
        metric_fixtures(ref_metrics, ref_validator)
