"""Generate the fixtures of the inference side of segmentation under tests/golden/ by running the REAL reference on the CPU (the reference's
tree must be present).  Writes data only:

    segpred_nms.npz            non_max_suppression(nc=3) on a Segment-shaped input: the [n, 6 + nm] rows of every image and their counts
    segpred_decode_<case>.npz  process_mask(upsample=False / True) per image on tests/segpred_ref.py::DECODE_CASES, bit-packed
    segpred_decode.json        per real-valued case and mode: the float32 reference's largest distance from the float64 restatement over
                               the pixels a box reaches, and the margin (four times that) inside which a test leaves a pixel's sign open
    segpred_match.npz          on segpred_ref.REF_MATCH: mask_iou of image 0, SegmentationValidator._process_batch with and without masks
                               (tp_m, tp), and the statistics rows SegmentMetrics was fed
    segpred_metrics.json       SegmentMetrics.results_dict of those rows, and the per-class values of both Metrics

    python tests/golden/make_segpred_golden.py

Same import shim as make_val_golden.py (cv2 stubbed, the torchvision version patched, YOLO_OFFLINE) and the same DISCLOSED stand-in for
torchvision.ops.nms (make_val_golden.greedy_nms: our code, written out from the operator's definition).  Nothing is stored that a seed rebuilds:
the inputs come from tests/segpred_ref.py and tests/nms_exact.py on both sides."""
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_val_golden import import_reference  # noqa: E402

import nms_exact as NX  # noqa: E402
import segpred_ref as SR  # noqa: E402


def nms_fixture(ops):
    c = NX.CASES[SR.SEG_NMS["case"]]
    y = SR.with_coefficients(NX.case_input(SR.SEG_NMS["case"]), SR.SEG_NMS["nm"], SR.SEG_NMS["seed"])
    res = ops.non_max_suppression(y.clone(), c["conf"], c["iou"], multi_label=c["multi_label"], nc=c["nc"], max_time_img=1e6)
    rows = torch.cat([r.float() for r in res], 0).numpy()
    np.savez_compressed(OUT / "segpred_nms.npz", rows=rows.astype(np.float32), counts=np.array([len(r) for r in res], dtype=np.int32))
    print("segpred_nms.npz", rows.shape, [len(r) for r in res])


def reference_masks(ops, proto, box, coef, img, shape, upsample):
    """the reference's process_mask image by image, its rows put back in row order; rows of no image stay zero (the reference has no such rows)."""
    oh, ow = shape if upsample else proto.shape[2:]
    out = torch.zeros(box.shape[0], oh, ow)
    for b in range(proto.shape[0]):
        sel = torch.nonzero(img == b).reshape(-1)
        if len(sel):
            out[sel] = ops.process_mask(proto[b], coef[sel], box[sel], shape, upsample=upsample)
    return out


def reference_values(ops, proto, box, coef, img, shape, upsample):
    """the float32 values the reference thresholds, from its own statements (the matmul, crop_mask, F.interpolate of process_mask)."""
    B, c, mh, mw = proto.shape
    out = torch.zeros(box.shape[0], *(shape if upsample else (mh, mw)))
    for b in range(B):
        sel = torch.nonzero(img == b).reshape(-1)
        if not len(sel):
            continue
        m = (coef[sel] @ proto[b].float().view(c, -1)).view(-1, mh, mw)
        m = ops.crop_mask(m, SR.crop_edges(box[sel], (mh, mw), shape))
        out[sel] = F.interpolate(m[None], shape, mode="bilinear", align_corners=False)[0] if upsample else m
    return out


def decode_fixtures(ops):
    notes = {}
    for name, c in SR.DECODE_CASES.items():
        proto, box, coef, img = SR.decode_case(name)
        arrays = {}
        for mode, up in (("low", False), ("up", True)):
            m = reference_masks(ops, proto, box, coef, img, c["shape"], up)
            v32 = reference_values(ops, proto, box, coef, img, c["shape"], up)
            assert torch.equal(v32 > 0, m.bool()), "the restated statements are not the reference's process_mask"
            v64 = SR.process_mask_values(proto, box, coef, img, c["shape"], up, torch.float64)
            dist = float((v32.double() - v64).abs().max())
            if c["kind"] == "exact":
                assert dist == 0.0 and torch.equal(v64 > 0, m.bool()), (name, mode, dist)
                inside = SR.process_mask_values(torch.ones_like(proto), box, torch.ones_like(coef), img, c["shape"], False, torch.float64) != 0
                zero = int(((SR.process_mask_values(proto, box, coef, img, c["shape"], False, torch.float64) == 0) & inside).sum())
                print(f"{name} {mode}: exact; on {int(m.sum())} of {m.numel()}; low-resolution logits that are exactly 0 inside a box: {zero}")
            else:
                reach = v64 != 0
                margin = 4 * dist
                out = reach & (v64.abs() < margin)
                notes.setdefault(name, {})[mode] = dict(distance=dist, margin=margin, reached=int(reach.sum()), left_out=int(out.sum()),
                                                        largest=float(v64.abs().max()), sign_disagreements=int(((v32 > 0) != (v64 > 0)).sum()))
                print(name, mode, notes[name][mode])
            arrays[mode] = SR.pack_masks(m.bool().numpy())
        np.savez_compressed(OUT / f"segpred_decode_{name}.npz", **arrays)
    (OUT / "segpred_decode.json").write_text(json.dumps(notes, indent=1) + "\n")


def match_fixtures(ops, metrics, validator):
    from ultralytics.models.yolo.segment.val import SegmentationValidator

    case = SR.match_case(**SR.REF_MATCH)
    iouv = SR.IOUV
    holder = SimpleNamespace(iouv=iouv)
    holder.match_predictions = lambda pc, tc, iou: validator.BaseValidator.match_predictions(holder, pc, tc, iou)
    B, max_det = case["det"].shape[:2]
    tp = np.zeros((B, max_det, len(iouv)), dtype=np.uint8)
    tp_m = np.zeros_like(tp)
    stats = dict(tp=[], tp_m=[], conf=[], pred_cls=[], target_cls=[])
    iou0 = None
    scale = torch.tensor([case["shape"][1], case["shape"][0]] * 2, dtype=torch.float32)
    for b in range(B):
        n = int(case["count"][b])
        sel = case["lab_img"] == b
        cls, bbox = case["lab_cls"][sel], ops.xywh2xyxy(case["lab_box"][sel]) * scale
        pred = case["det"][b, :n]
        if n and len(cls):
            masks = ops.process_mask(case["proto"][b], case["coef"][b, :n], pred[:, :4], case["shape"])
            gt = case["enc"][b][None].float()
            tp[b, :n] = SegmentationValidator._process_batch(holder, pred, bbox, cls).numpy()
            tp_m[b, :n] = SegmentationValidator._process_batch(holder, pred, bbox, cls, masks, gt, True, masks=True).numpy()
            if iou0 is None:
                nl = len(cls)
                onehot = torch.where(gt.repeat(nl, 1, 1) == torch.arange(nl).view(nl, 1, 1) + 1, 1.0, 0.0)
                iou0 = metrics.mask_iou(onehot.view(nl, -1), masks.view(n, -1))
                for j in range(nl):  # no two detections overlap a label equally at or above the first level: the reference leaves such ties to argsort
                    hi = iou0[j][iou0[j] >= 0.5]
                    assert len(hi.unique()) == len(hi), (j, hi)
        if n or len(cls):
            stats["tp"].append(tp[b, :n].astype(bool)), stats["tp_m"].append(tp_m[b, :n].astype(bool))
            stats["conf"].append(pred[:, 4].numpy()), stats["pred_cls"].append(pred[:, 5].numpy()), stats["target_cls"].append(cls.numpy())
    stats = {k: np.concatenate(v, 0) for k, v in stats.items()}
    np.savez_compressed(OUT / "segpred_match.npz", tp=tp, tp_m=tp_m, iou0=iou0.numpy())
    sm = metrics.SegmentMetrics(names={i: str(i) for i in range(SR.REF_MATCH["nc"])})
    sm.process(**stats)
    out = dict(keys=list(sm.results_dict.keys()), results=[float(v) for v in sm.results_dict.values()],
               box_ap=np.asarray(sm.box.all_ap, dtype=np.float64).tolist(), seg_ap=np.asarray(sm.seg.all_ap, dtype=np.float64).tolist(),
               ap_class_index=[int(v) for v in sm.ap_class_index], fitness=float(sm.fitness))
    (OUT / "segpred_metrics.json").write_text(json.dumps(out) + "\n")
    print("tp_m hits per level", tp_m.sum((0, 1)).tolist(), "tp hits", tp.sum((0, 1)).tolist())
    print({k: round(v, 4) for k, v in zip(out["keys"], out["results"])})


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref_ops, ref_metrics, ref_validator = import_reference()
    nms_fixture(ref_ops)
    decode_fixtures(ref_ops)
    match_fixtures(ref_ops, ref_metrics, ref_validator)
