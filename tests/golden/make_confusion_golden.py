"""Generate tests/golden/confusion_matrix.json by running the REAL reference's ConfusionMatrix.process_batch on the CPU.

Run in the build container only (needs the reference checkout that make_val_golden.py names):

    python tests/golden/make_confusion_golden.py

Same import shim as make_val_golden.py (import_reference).  The inputs are rebuilt from seeds by tests/valmatch_ref.py (the four
nms_exact.METRIC_CASES, two dense cases with up to 300 detections per image, two cases in which detections lose the label they claim to a
better one); the fixture holds only the matrices.  Per image the reference is called as models/yolo/detect/val.py:195-214 calls it:
detections=None for an image without detections, not at all for an image with neither detections nor labels, the label boxes as
xywh2xyxy(bboxes) * (w, h, w, h) in float32.

Asserted for EVERY case, never skipped (pick another seed in valmatch_ref.SEEDED until they hold): the candidate IoUs above 0.3 are
pairwise distinct within an image (the reference leaves equal IoUs to argsort); every IoU keeps nms_exact.MARGIN_MIN from 0.45 and from
the ten tp levels; no confidence equals 0.25; the steal cases contain detections that lose their claim."""
import json
import sys
from pathlib import Path

import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))

import nms_exact as NX  # noqa: E402
import valmatch_ref as VR  # noqa: E402
from make_val_golden import import_reference  # noqa: E402


def main():
    _, metrics, _ = import_reference()
    out = {}
    for name in VR.CASES:
        nc, images = VR.case(name)
        distinct, gap_cm, gap_lv, gap_conf = VR.conditions(images)
        assert distinct, f"{name}: equal candidate IoUs above 0.3: try the next seed"
        assert gap_cm >= NX.MARGIN_MIN and gap_lv >= NX.MARGIN_MIN, f"{name}: an IoU within {NX.MARGIN_MIN} of 0.45 or of a level ({gap_cm:.2e}, {gap_lv:.2e}): try the next seed"
        assert gap_conf > 0, f"{name}: a confidence equals 0.25: try the next seed"
        lost = VR.lost_claims(images)
        assert lost > 0 or not name.startswith("steal"), f"{name}: no detection loses its claim"
        cm = metrics.ConfusionMatrix(nc=nc, conf=VR.CM_CONF, iou_thres=VR.CM_IOU)
        for det, xywh, cls in images:
            if not len(det) and not len(cls):
                continue
            cm.process_batch(det if len(det) else None, VR.label_boxes(xywh, VR.IMGSZ, VR.IMGSZ), cls)
        out[name] = [[int(v) for v in row] for row in cm.matrix]
        total = sum(sum(r) for r in out[name])
        print(f"{name}: detections {[len(d) for d, _, _ in images]} sum {total} lost claims {lost} |iou - 0.45| >= {gap_cm:.1e} |iou - level| >= {gap_lv:.1e} "
              f"|conf - 0.25| >= {gap_conf:.1e}", flush=True)
    (OUT / "confusion_matrix.json").write_text(json.dumps(out) + "\n")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
