"""Float32 restatement of the detection post-processing for tests (a helper like gemm_exact.py / attn_exact.py, not a conftest).

`nms_exact` restates reference utils/ops.py:181-332 with torchvision.ops.nms written out, in torch on the CPU, one float32 operation
per step in the order include/ymi.h gives for ymi_detect_nms: boxes x -+ w/2, candidates by strict `>`, order by descending score with
ties by ascending anchor then class (the library's own rule), the max_nms cut, the class offset b + cls * max_wh as a product and a
sum, iou = inter / (area_i + area_j - inter), suppression by strict `>`, the first max_det kept.  `fault=` plants one deliberate error
(tests/test_host_nms_check.py asserts that each is noticed).  `margin` repeats the greedy scan in float64 and returns the smallest
|iou - iou_thres| over the pairs the scan compares: a case whose margin is >= MARGIN_MIN has the same kept set under ANY correct float32
arithmetic (a float32 IoU carries about six roundings, ~4e-7 relative; 1e-5 is 25 times that).

The inputs of the committed cases are rebuilt from seeds (numpy's frozen MT19937 stream), so the fixtures under tests/golden/ hold only
what the reference produced.  CASES names every case; tests/golden/nms_seeds.json holds the per-image seeds chosen by
tests/golden/make_val_golden.py --choose-seeds so that the guarded cases meet the margin and have distinct candidate scores."""
import json
from pathlib import Path

import numpy as np
import torch

MARGIN_MIN = 1e-5
GOLDEN = Path(__file__).resolve().parent / "golden"


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def candidates(yi, conf_thres, multi_label, classes=None):
    """yi [4 + nc, A] float32 -> (box [n, 4] xyxy, score [n], cls [n] int64) in (anchor, class) order."""
    yi = yi.float()
    nc = yi.shape[0] - 4
    x, y, hw, hh = yi[0], yi[1], yi[2] / 2, yi[3] / 2
    box = torch.stack((x - hw, y - hh, x + hw, y + hh), 1)  # [A, 4]
    s = yi[4:].t()  # [A, nc]
    conf = torch.tensor(conf_thres, dtype=torch.float32)
    if multi_label and nc > 1:
        a, c = torch.where(s > conf)  # row-major: anchors ascending, classes ascending inside an anchor
        score = s[a, c]
    else:
        score = s.max(1)[0]
        c = torch.where(s == score[:, None], torch.arange(nc)[None], nc).min(1)[0]  # the first maximum
        a = torch.where(score > conf)[0]
        score, c = score[a], c[a]
    if classes is not None:
        keep = (c[:, None] == torch.tensor(sorted(classes))[None]).any(1)
        a, c, score = a[keep], c[keep], score[keep]
    return box[a], score, c


def _iou_with(boxes, areas, i, dtype_ops=None):
    """torchvision.ops.nms' IoU of box i with every box, each step one operation of the tensors' dtype."""
    xx1 = torch.maximum(boxes[i, 0], boxes[:, 0])
    yy1 = torch.maximum(boxes[i, 1], boxes[:, 1])
    xx2 = torch.minimum(boxes[i, 2], boxes[:, 2])
    yy2 = torch.minimum(boxes[i, 3], boxes[:, 3])
    w = (xx2 - xx1).clamp(min=0)
    h = (yy2 - yy1).clamp(min=0)
    inter = w * h
    return inter / ((areas[i] + areas) - inter)


def greedy(boxes, iou_thres, max_det, fault=None, same_class=None):
    """boxes [n, 4] in scan order -> (indices kept, at most max_det; smallest |iou - thr| in the boxes' dtype over compared pairs)."""
    n = boxes.shape[0]
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    thr = torch.tensor(iou_thres, dtype=boxes.dtype)
    alive = torch.ones(n, dtype=torch.bool)
    keep, gap, p = [], float("inf"), 0
    while len(keep) < max_det:
        rest = torch.nonzero(alive[p:])
        if not rest.numel():
            break
        i = p + int(rest[0])
        keep.append(i)
        iou = _iou_with(boxes, areas, i)
        if same_class is not None:
            iou = torch.where(same_class[i] == same_class, iou, torch.zeros_like(iou))
        later = alive.clone()
        later[: i + 1] = False
        if later.any():
            d = (iou[later] - thr).abs()
            d = d[~torch.isnan(d)]
            if d.numel():
                gap = min(gap, float(d.min()))
        sup = (iou >= thr) if fault == "ge" else (iou > thr)
        alive &= ~(sup & later)
        alive[i] = False
        p = i + 1
    return keep, gap


def nms_image(yi, conf_thres, iou_thres, multi_label=False, agnostic=False, classes=None, max_det=300, max_nms=30000, max_wh=7680, fault=None,
              dtype=torch.float32):
    """one image -> (rows [k, 6] float32 in kept order, margin of the scan in `dtype`, candidate scores before the cut)."""
    box, score, cls = candidates(yi, conf_thres, multi_label, classes)
    all_scores = score
    if fault == "unstable_ties":  # equal scores in descending index order
        order = (score.numel() - 1) - torch.sort(score.flip(0), descending=True, stable=True)[1]
    else:
        order = torch.sort(score, descending=True, stable=True)[1]
    if fault != "no_max_nms":
        order = order[:max_nms]
    box, score, cls = box[order], score[order], cls[order]
    if fault == "class_compare":  # a class test in place of the offset: misses the rounding the offset applies to the coordinates
        shifted, same = box, (None if agnostic else cls)
    else:
        off = cls.float() * float(0 if agnostic else max_wh)  # float32 product
        shifted, same = box + off[:, None], None  # one float32 addition per coordinate
    keep, gap = greedy(shifted.to(dtype), iou_thres, max_det, fault, same)
    k = torch.tensor(keep, dtype=torch.long)
    rows = torch.cat((box[k], score[k, None], cls[k, None].float()), 1) if len(keep) else torch.zeros(0, 6)
    return rows, gap, all_scores


def nms_exact(y, conf_thres=0.25, iou_thres=0.45, *, multi_label=False, agnostic=False, classes=None, max_det=300, max_nms=30000, max_wh=7680, fault=None):
    """y [B, 4 + nc, A] (CPU) -> (det [B, max_det, 6] float32 zero-padded, count [B] int32): what ops.detect_nms must return, bit for bit."""
    y = y.detach().float().cpu()
    det = torch.zeros(y.shape[0], max_det, 6)
    count = torch.zeros(y.shape[0], dtype=torch.int32)
    for b in range(y.shape[0]):
        rows, _, _ = nms_image(y[b], conf_thres, iou_thres, multi_label, agnostic, classes, max_det, max_nms, max_wh, fault)
        det[b, : rows.shape[0]] = rows
        count[b] = rows.shape[0]
    return det, count


def margin(y, conf_thres=0.25, iou_thres=0.45, *, multi_label=False, agnostic=False, classes=None, max_det=300, max_nms=30000, max_wh=7680):
    """-> per image (float64 margin, kept rows of the float64 scan, whether all candidate scores are distinct).  The float64 scan works on the
    float32 offset boxes (they are the data) and takes the IoU in float64."""
    out = []
    for b in range(y.shape[0]):
        rows, gap, scores = nms_image(y[b], conf_thres, iou_thres, multi_label, agnostic, classes, max_det, max_nms, max_wh, dtype=torch.float64)
        out.append((gap, rows, bool(torch.unique(scores).numel() == scores.numel())))
    return out


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------
def cluster_image(seed, A, nc, imgsz=640, density=1.0, grid=0.25, targets=(12, 60)):
    """one image [4 + nc, A]: boxes around a few targets, a `density` share of the (anchor, class) scores spread over (0.002, 0.999)
    without repeats, the rest below 0.0005.  grid > 0: coordinates on a `grid`-pixel lattice and every box one of 36 variants of its target
    (centre moved by -1, 0, 1 steps of ~12 % of the target's size per axis, two widths, two heights), so that the IoUs the scan meets are a
    few ten thousand distinct rationals and a seed can be found where none lies within 1e-5 of the threshold.  grid = 0: continuous
    jitter, off-grid float32 coordinates (the unguarded case)."""
    rs = np.random.RandomState(seed)
    T = rs.randint(targets[0], targets[1] + 1)
    tc = rs.uniform(0.1, 0.9, size=(T, 2)) * imgsz
    twh = rs.uniform(0.04, 0.3, size=(T, 2)) * imgsz
    t = rs.randint(0, T, size=A)
    if grid:
        tc = np.round(tc / grid) * grid
        twh = np.maximum(np.round(twh / (2 * grid)), 2) * (2 * grid)
        step = np.maximum(np.round(0.12 * twh / grid), 1) * grid
        wide = np.maximum(np.round(1.25 * twh / (2 * grid)), 2) * (2 * grid)
        ctr = tc[t] + rs.randint(-1, 2, size=(A, 2)) * step[t]
        wh = np.where(rs.randint(0, 2, size=(A, 2)) == 1, wide[t], twh[t])
    else:
        ctr = tc[t] + rs.normal(0, 0.08, size=(A, 2)) * twh[t]
        wh = twh[t] * np.exp(rs.normal(0, 0.12, size=(A, 2)))
    n = A * nc
    rank = rs.permutation(n).astype(np.float64)
    s = 0.002 + 0.997 * (rank + 0.5) / n
    cold = rs.uniform(size=n) >= density
    s[cold] = s[cold] * 0.0005
    return np.concatenate((ctr.T, wh.T, s.reshape(A, nc).T), 0).astype(np.float32)


# name -> parameters.  kind "cluster": one cluster_image per seed in nms_seeds.json; "special": special_input(name).
# guarded: distinct candidate scores and a float64 margin >= MARGIN_MIN are asserted (the seeds were chosen for it).
CASES = {
    "nc3_b3": dict(kind="cluster", B=3, A=8400, nc=3, conf=0.001, iou=0.7, multi_label=True, guarded=True),
    "nc1_b1_det10": dict(kind="cluster", B=1, A=8400, nc=1, conf=0.25, iou=0.45, multi_label=True, max_det=10, guarded=True),
    # 80 k candidates, the cut at 30000 changes the result (agnostic and max_det 2048: the scan reaches the end of the list)
    "nc80_over_max_nms": dict(kind="cluster", B=1, A=8400, nc=80, conf=0.001, iou=0.6, multi_label=True, agnostic=True, max_det=2048, density=0.12,
                              targets=(150, 200), guarded=True),
    "nc80_multi": dict(kind="cluster", B=1, A=8400, nc=80, conf=0.001, iou=0.6, multi_label=True, density=0.03, guarded=True),
    "nc80_best_agnostic_det1": dict(kind="cluster", B=3, A=8400, nc=80, conf=0.25, iou=0.45, multi_label=False, agnostic=True, max_det=1, guarded=True),
    "nc80_best": dict(kind="cluster", B=1, A=8400, nc=80, conf=0.25, iou=0.6, multi_label=False, guarded=True),
    "nc3_filter": dict(kind="cluster", B=1, A=8400, nc=3, conf=0.25, iou=0.6, multi_label=True, classes=[0, 2], guarded=True),
    "nc3_agnostic": dict(kind="cluster", B=1, A=8400, nc=3, conf=0.001, iou=0.45, multi_label=True, agnostic=True, density=0.3, guarded=True),
    "nc3_max_nms_300": dict(kind="cluster", B=1, A=8400, nc=3, conf=0.001, iou=0.7, multi_label=True, max_nms=300, guarded=True),
    "nc3_b32": dict(kind="cluster", B=32, A=8400, nc=3, conf=0.001, iou=0.7, multi_label=True, density=0.25, max_det=100, guarded=True),
    "nc3_1280": dict(kind="cluster", B=1, A=33600, nc=3, imgsz=1280, conf=0.25, iou=0.7, multi_label=True, density=0.3, guarded=True),
    "empty_and_all_survive": dict(kind="special", B=3, A=8400, nc=3, conf=0.25, iou=0.45, multi_label=True, guarded=True),
    "tie_scores": dict(kind="special", B=1, A=2100, nc=3, conf=0.25, iou=0.45, multi_label=True, guarded=False),
    "tie_best_class": dict(kind="special", B=1, A=2100, nc=3, conf=0.25, iou=0.45, multi_label=False, guarded=False),
    "iou_equals_threshold": dict(kind="special", B=1, A=64, nc=1, conf=0.25, iou=0.5, multi_label=False, guarded=False),
    "high_class_offgrid": dict(kind="special", B=1, A=2100, nc=80, conf=0.25, iou=0.7, multi_label=False, guarded=False),
}
_NMS_KEYS = ("multi_label", "agnostic", "classes", "max_det", "max_nms", "max_wh")


def nms_kwargs(case):
    """the keyword arguments of nms_exact / ops.detect_nms / non_max_suppression that a case sets."""
    return {k: case[k] for k in _NMS_KEYS if k in case}


def special_input(name, seeds=None):
    c = CASES[name]
    A, nc = c["A"], c["nc"]
    rs = np.random.RandomState(len(name) * 7919)
    y = np.zeros((c["B"], 4 + nc, A), dtype=np.float32)
    y[:, 2:4] = 8.0
    if name == "empty_and_all_survive":
        y[0] = cluster_image(seeds[0], A, nc)  # an ordinary image (seed chosen for the margin)
        y[1] = cluster_image(12, A, nc)
        y[1, 4:] *= 0.2  # ... with every score below conf: no candidate
        k = 40  # image 2: 40 candidates on a lattice of disjoint boxes, distinct scores: all survive
        a = rs.choice(A, k, replace=False)
        y[2, 0, a] = 50.0 + 90.0 * (np.arange(k) % 6)
        y[2, 1, a] = 50.0 + 80.0 * (np.arange(k) // 6)
        y[2, 2:4, a] = 40.0
        y[2, 4 + (np.arange(k) % nc), a] = 0.3 + 0.6 * (rs.permutation(k) + 0.5) / k
    elif name in ("tie_scores", "tie_best_class"):
        y[0] = cluster_image(21, A, nc, density=0.5)
        s = y[0, 4:]
        if name == "tie_scores":  # scores on a coarse lattice: many candidates share a score, across anchors and classes
            s[...] = np.where(s > 0.25, np.round(s * 16) / 16, s)
        else:  # every anchor's classes share the best score: the first class must be taken; anchors tie too
            s[...] = np.round(s.max(0, keepdims=True) * 32) / 32
    elif name == "iou_equals_threshold":  # two boxes with inter 50, union 100: iou is 0.5 exactly; `>` keeps both
        y[0, :4, 0] = (5.0, 5.0, 10.0, 10.0)
        y[0, :4, 1] = (5.0, 2.5, 10.0, 5.0)
        y[0, 4, 0], y[0, 4, 1] = 0.9, 0.8
        y[0, :4, 2] = (30.0, 30.0, 10.0, 10.0)  # and a pair above it
        y[0, :4, 3] = (30.0, 30.5, 10.0, 9.0)
        y[0, 4, 2], y[0, 4, 3] = 0.7, 0.6
    elif name == "high_class_offgrid":  # small off-grid boxes of classes 60..79: the offset (4.6e5 .. 6.1e5) rounds coordinates to 1/32 .. 1/16
        t = rs.randint(0, 40, size=A)
        tc = rs.uniform(40, 600, size=(40, 2))
        y[0, 0:2] = (tc[t] + rs.normal(0, 0.25, size=(A, 2))).T
        y[0, 2:4] = rs.uniform(1.5, 3.0, size=(2, A))
        y[0, 4 + 60 + (t % 20), np.arange(A)] = 0.26 + 0.7 * (rs.permutation(A) + 0.5) / A
    else:
        raise KeyError(name)
    return torch.from_numpy(y)


def case_image(c, seed):
    return cluster_image(seed, c["A"], c["nc"], c.get("imgsz", 640), c.get("density", 1.0), targets=c.get("targets", (12, 60)))


def load_seeds():
    return json.loads((GOLDEN / "nms_seeds.json").read_text())


def case_input(name, seeds=None):
    """-> y [B, 4 + nc, A] float32 (CPU) of a committed case."""
    c = CASES[name]
    seeds = (seeds or load_seeds()).get(name)
    if c["kind"] == "special":
        return special_input(name, seeds)
    assert len(seeds) == c["B"]
    return torch.from_numpy(np.stack([case_image(c, s) for s in seeds]))


def load_expected(name):
    """the reference's result of a case (tests/golden/nms_<name>.npz) -> (list of [n_i, 6] tensors, recorded float64 margins)."""
    with np.load(GOLDEN / f"nms_{name}.npz") as z:
        counts, rows, margins = z["counts"], z["rows"], z["margins"]
    out, o = [], 0
    for n in counts:
        out.append(torch.from_numpy(rows[o : o + int(n)].copy()))
        o += int(n)
    return out, margins


def padded(rows_list, max_det):
    """list of [n_i, 6] -> (det [B, max_det, 6] zero-padded, count [B] int32)."""
    det = torch.zeros(len(rows_list), max_det, 6)
    for b, r in enumerate(rows_list):
        det[b, : r.shape[0]] = r
    return det, torch.tensor([r.shape[0] for r in rows_list], dtype=torch.int32)


def same_bits(a, b):
    """equal as bit patterns (float32 tensors viewed as int32; distinguishes -0.0 and NaN payloads)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    return bool(torch.equal(a, b))


# ---- seeded inputs of the metric fixtures ---------------------------------------------------------------------------------------------
METRIC_CASES = {
    "mixed": dict(seed=5, images=8, nc=3),             # ordinary: hits, near misses, duplicates, strays; one image without detections, one without labels
    "absent_class": dict(seed=6, images=6, nc=4),      # class 3 is predicted but never labelled; class 2 is labelled but never predicted
    "no_detections": dict(seed=7, images=4, nc=2),     # labels everywhere, not one detection
    "no_labels": dict(seed=8, images=4, nc=2),         # detections everywhere, not one label
}


def metric_case(name):
    """-> list of per-image (det [n, 6] float32, gt_box [m, 4] xyxy float32, gt_cls [m] float32), rebuilt from the case's seed."""
    c = METRIC_CASES[name]
    rs = np.random.RandomState(c["seed"])
    nc, out = c["nc"], []
    for i in range(c["images"]):
        m = rs.randint(3, 9)
        ctr, wh = rs.uniform(80, 560, size=(m, 2)), rs.uniform(30, 160, size=(m, 2))
        gt = np.concatenate((ctr - wh / 2, ctr + wh / 2), 1)
        lab_classes = nc - 1 if name == "absent_class" else nc
        gcls = rs.randint(0, lab_classes, size=m).astype(np.float64)
        rows = []
        for j in range(m):  # per label: up to three detections at growing jitter (hit, near miss, duplicate), some with the wrong class
            for k in range(rs.randint(0, 4)):
                jit = rs.normal(0, 0.02 + 0.06 * k, size=4) * np.concatenate((wh[j], wh[j]))
                cls = gcls[j] if rs.uniform() < 0.8 else float(rs.randint(0, nc))
                if name == "absent_class" and cls == 2:
                    cls = 3.0
                rows.append(np.concatenate((gt[j] + jit, [rs.uniform(0.05, 0.99), cls])))
        for k in range(rs.randint(0, 4)):  # strays
            c0, w0 = rs.uniform(80, 560, size=2), rs.uniform(20, 100, size=2)
            cls = float(rs.randint(0, nc))
            rows.append(np.concatenate((c0 - w0 / 2, c0 + w0 / 2, [rs.uniform(0.05, 0.6), 3.0 if name == "absent_class" and cls == 2 else cls])))
        det = np.array(rows, dtype=np.float32).reshape(-1, 6)
        det = det[np.argsort(-det[:, 4], kind="stable")]
        if name == "no_detections" or (name == "mixed" and i == 2):
            det = det[:0]
        if name == "no_labels" or (name == "mixed" and i == 5):
            gt, gcls = gt[:0], gcls[:0]
        out.append((torch.from_numpy(det), torch.from_numpy(gt.astype(np.float32)), torch.from_numpy(gcls.astype(np.float32))))
    return out


def accumulate(images, box_iou, match_predictions, iouv):
    """the validator's statistics (reference val.py:174-216) over metric_case images with the given box_iou / matcher ->
    dict of numpy arrays tp [n, 10] bool, conf, pred_cls, target_cls."""
    stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
    for det, gt, gcls in images:
        if not len(det) and not len(gcls):
            continue
        tp = torch.zeros(len(det), len(iouv), dtype=torch.bool)
        if len(det) and len(gcls):
            tp = match_predictions(det[:, 5], gcls, box_iou(gt, det[:, :4]))
        for k, v in zip(stats, (tp, det[:, 4], det[:, 5], gcls)):
            stats[k].append(v)
    return {k: torch.cat(v, 0).numpy() for k, v in stats.items()}
