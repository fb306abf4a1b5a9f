"""Float32 restatement of the validator's per-image work after NMS, for tests (a helper like nms_exact.py, not a conftest).

`match` restates the contract include/ymi.h gives for ymi_val_match in torch / numpy on the CPU, one float32 operation per step in the
header's order: label boxes (cx -+ w / 2) * W, optionally to native pixels ((v - pad) / gain, clamped), iou = inter / (((area_l + area_p)
- inter) + 1e-7f), the tp matrix by the claim / strength / better-ranked-maximum form, and the confusion matrix by the claim / holder
form with the library's tie rule.  tests/test_valmatch_ref_cpu.py holds it to utils.metrics (box_iou + match_predictions, bit for bit) and
to the reference's ConfusionMatrix (tests/golden/confusion_matrix.json); tests/test_gpu_valmatch.py holds ops.val_match to it.  `fault=`
plants one deliberate error.

The inputs of every case are rebuilt from seeds (numpy's frozen MT19937 stream): the fixture holds only the matrices the reference
produced.  tests/golden/make_confusion_golden.py asserts for every case that the candidate IoUs above 0.3 are pairwise distinct within an
image, that every IoU keeps nms_exact.MARGIN_MIN from 0.45 and that no confidence equals 0.25 (`conditions`)."""
import numpy as np
import torch

import nms_exact as NX

IMGSZ = 640
CM_CONF, CM_IOU = 0.25, 0.45
FAULTS = ("gt", "no_class_mask", "owner_by_rank")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def label_boxes(xywh, img_w, img_h, native=None):
    """normalised xywh float32 [m, 4] -> xyxy float32 [m, 4] in the network input's pixels; native = (gain, pad_x, pad_y, w0, h0): in native
    pixels, clamped.  Every step one float32 operation."""
    b = torch.as_tensor(xywh).float().reshape(-1, 4)
    W, H = torch.tensor(float(img_w), dtype=torch.float32), torch.tensor(float(img_h), dtype=torch.float32)
    hw, hh = b[:, 2] / 2, b[:, 3] / 2
    x1, y1, x2, y2 = (b[:, 0] - hw) * W, (b[:, 1] - hh) * H, (b[:, 0] + hw) * W, (b[:, 1] + hh) * H
    if native is not None:
        gain, pad_x, pad_y, w0, h0 = (torch.tensor(float(v), dtype=torch.float32) for v in native)
        zero = torch.zeros((), dtype=torch.float32)
        x1, x2 = (torch.minimum(torch.maximum((v - pad_x) / gain, zero), w0) for v in (x1, x2))
        y1, y2 = (torch.minimum(torch.maximum((v - pad_y) / gain, zero), h0) for v in (y1, y2))
    return torch.stack((x1, y1, x2, y2), 1)


def iou_matrix(lab, pred):
    """xyxy float32 [m, 4] x [n, 4] -> [m, n] float32, the header's steps."""
    a, b = lab.float()[:, None, :], pred.float()[None, :, :]
    iw = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp(min=0)
    ih = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp(min=0)
    inter = iw * ih
    area_l = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_p = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    return inter / (((area_l + area_p) - inter) + torch.tensor(1e-7, dtype=torch.float32))


def _class_ids(values, nc):
    v = np.trunc(np.asarray(values, dtype=np.float64).reshape(-1))
    return np.where((v > -1) & (v < nc), v, -1).astype(np.int64)


def image_tp(rows, lab, lab_cls, levels, fault=None):
    """one image: rows [n, 6] ranked, lab [m, 4] xyxy, lab_cls [m] -> uint8 [n, T]."""
    n, m = rows.shape[0], lab.shape[0]
    out = np.zeros((n, len(levels)), dtype=np.uint8)
    if n == 0 or m == 0:
        return out
    iou = iou_matrix(lab, rows[:, :4]).numpy()
    same = (lab_cls.numpy().reshape(-1, 1) == rows[:, 5].numpy().reshape(1, -1)).astype(np.float32)
    overlap = iou if fault == "no_class_mask" else iou * same
    claim = overlap.argmax(axis=0)  # first maximum in table order
    s = overlap[claim, np.arange(n)]
    earlier = np.tril(np.ones((n, n), dtype=bool), -1) & (claim[:, None] == claim[None, :])  # [d, e]: e < d with the same claim
    best_before = np.where(earlier, s[None, :], -np.inf).max(axis=1)
    for t, level in enumerate(levels):
        level = np.float32(level)
        reach = (s > level) if fault == "gt" else (s >= level)
        taken = (best_before > level) if fault == "gt" else (best_before >= level)
        out[:, t] = reach & ~taken
    return out


def image_cm(matrix, rows, lab, lab_cls, nc, cm_conf=CM_CONF, cm_iou=CM_IOU, fault=None):
    """one image's counts are added to matrix [(nc + 1), (nc + 1)] int64."""
    rows = rows[(rows[:, 4].numpy() > np.float32(cm_conf)).nonzero()[0]]
    dc, gc = _class_ids(rows[:, 5].numpy(), nc), _class_ids(lab_cls.numpy(), nc)
    n, m = len(dc), len(gc)
    holder = np.full(m, -1, dtype=np.int64)
    if n and m:
        iou = iou_matrix(lab, rows[:, :4]).numpy()
        claim = iou.argmax(axis=0)
        ci = iou[claim, np.arange(n)]
        for d in range(n):
            if not ci[d] > np.float32(cm_iou):
                continue
            h = holder[claim[d]]
            if h < 0 or (fault != "owner_by_rank" and ci[d] > ci[h]):  # equal: the lower detection index keeps the label
                holder[claim[d]] = d
    holds = np.zeros(n, dtype=bool)
    holds[holder[holder >= 0]] = True
    for l in range(m):
        if holder[l] < 0:
            if gc[l] >= 0:
                matrix[nc, gc[l]] += 1
        elif gc[l] >= 0 and dc[holder[l]] >= 0:
            matrix[dc[holder[l]], gc[l]] += 1
    for d in range(n):
        if not holds[d] and dc[d] >= 0:
            matrix[dc[d], nc] += 1


def match(det, count, lab_img, lab_cls, lab_box, img_shape, levels, native=None, single_cls=False, nc=None, cm_conf=CM_CONF, cm_iou=CM_IOU, fault=None):
    """the contract of ymi_val_match on CPU tensors: det [B, max_det, 6], count [B], the label table (lab_img [L], lab_cls [L], lab_box
    [L, 4] normalised xywh), img_shape (h, w), native: None or [B][5] -> (tp uint8 [B, max_det, T], matrix int64 [(nc + 1), (nc + 1)] or
    None when nc is None)."""
    det, count = det.detach().cpu().float(), count.detach().cpu().long()
    lab_img, lab_cls = torch.as_tensor(lab_img).cpu().long().reshape(-1), torch.as_tensor(lab_cls).cpu().float().reshape(-1)
    lab_box = torch.as_tensor(lab_box).cpu().float().reshape(-1, 4)
    levels = [float(v) for v in (levels.tolist() if torch.is_tensor(levels) else levels)]
    B, max_det = det.shape[:2]
    tp = np.zeros((B, max_det, len(levels)), dtype=np.uint8)
    matrix = np.zeros((nc + 1, nc + 1), dtype=np.int64) if nc is not None else None
    for b in range(B):
        n = int(min(max(int(count[b]), 0), max_det))
        rows = det[b, :n].clone()
        sel = lab_img == b
        cls = lab_cls[sel]
        lab = label_boxes(lab_box[sel], img_shape[1], img_shape[0], None if native is None else native[b])
        if single_cls:
            rows[:, 5] = 0
            cls = torch.zeros_like(cls)
        tp[b, :n] = image_tp(rows, lab, cls, levels, fault)
        if matrix is not None:
            image_cm(matrix, rows, lab, cls, nc, cm_conf, cm_iou, fault)
    return torch.from_numpy(tp), matrix


# ---- seeded cases --------------------------------------------------------------------------------------------------------------------
def to_xywh(gt_xyxy, imgsz=IMGSZ):
    """pixel xyxy [m, 4] -> normalised xywh float32 (formed in float64: the float32 table is the data from here on)."""
    g = np.asarray(gt_xyxy, dtype=np.float64).reshape(-1, 4)
    return torch.from_numpy(np.stack(((g[:, 0] + g[:, 2]) / 2, (g[:, 1] + g[:, 3]) / 2, g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]), 1) / imgsz).float()


# the two dense cases: up to 300 detections per image; the steal cases: detections that lose the label they claim to a better one.
# The seeds were chosen so that `conditions` holds (make_confusion_golden.py asserts it and says which seed to try next).
SEEDED = {
    "dense_a": dict(kind="dense", seed=101, images=3, nc=5),
    "dense_b": dict(kind="dense", seed=203, images=2, nc=80),
    "steal_a": dict(kind="steal", seed=303, images=4, nc=3),
    "steal_b": dict(kind="steal", seed=404, images=4, nc=3),
}
CASES = list(NX.METRIC_CASES) + list(SEEDED)


def _dense_image(rs, nc):
    m = rs.randint(30, 61)
    ctr, wh = rs.uniform(40, 600, size=(m, 2)), rs.uniform(24, 120, size=(m, 2))
    gt = np.concatenate((ctr - wh / 2, ctr + wh / 2), 1)
    gcls = rs.randint(0, nc, size=m).astype(np.float64)
    rows = []
    for j in range(m):
        for k in range(rs.randint(2, 8)):  # hits, near misses and duplicates at growing jitter, a fifth with another class
            jit = rs.normal(0, 0.015 + 0.03 * k, size=4) * np.concatenate((wh[j], wh[j]))
            cls = gcls[j] if rs.uniform() < 0.8 else float(rs.randint(0, nc))
            rows.append(np.concatenate((gt[j] + jit, [rs.uniform(0.002, 0.99), cls])))
    for k in range(rs.randint(10, 40)):  # strays
        c0, w0 = rs.uniform(40, 600, size=2), rs.uniform(16, 90, size=2)
        rows.append(np.concatenate((c0 - w0 / 2, c0 + w0 / 2, [rs.uniform(0.002, 0.6), float(rs.randint(0, nc))])))
    det = np.array(rows, dtype=np.float32).reshape(-1, 6)
    det = det[np.argsort(-det[:, 4], kind="stable")][:300]
    return det, gt, gcls


def _steal_image(rs, nc):
    """labels in overlapping pairs (A, B); per pair: a weak and a strong claimant of A in either rank order (the weak one loses A and does
    not fall back to B, which it also overlaps), sometimes a detection on B alone, sometimes a wrong class."""
    pairs = rs.randint(2, 5)
    gt, gcls, rows = [], [], []
    for p in range(pairs):
        c = np.array([110.0 + 140.0 * p, rs.uniform(150, 480)])
        wh = rs.uniform(60, 110, size=2)
        a = np.concatenate((c - wh / 2, c + wh / 2))
        shift = np.array([0.0, wh[1] * rs.uniform(0.35, 0.5)])
        b = a + np.concatenate((shift, shift))
        gt += [a, b]
        ca = float(rs.randint(0, nc))
        gcls += [ca, float(rs.randint(0, nc))]
        conf = rs.uniform(0.3, 0.95, size=3)
        strong = a + rs.normal(0, 0.02, size=4) * np.concatenate((wh, wh))
        weak = a + np.concatenate((shift, shift)) * rs.uniform(0.2, 0.3) + rs.normal(0, 0.01, size=4) * np.concatenate((wh, wh))
        rows.append(np.concatenate((strong, [conf[0], ca if rs.uniform() < 0.8 else float(rs.randint(0, nc))])))
        rows.append(np.concatenate((weak, [conf[1], ca])))
        if rs.uniform() < 0.5:
            rows.append(np.concatenate((b + rs.normal(0, 0.03, size=4) * np.concatenate((wh, wh)), [conf[2], gcls[-1]])))
        if rs.uniform() < 0.5:  # below the matrix's confidence: takes part in tp, not in the matrix
            rows.append(np.concatenate((a + rs.normal(0, 0.015, size=4) * np.concatenate((wh, wh)), [rs.uniform(0.05, 0.2), ca])))
    det = np.array(rows, dtype=np.float32).reshape(-1, 6)
    det = det[np.argsort(-det[:, 4], kind="stable")]
    return det, np.array(gt), np.array(gcls)


def case(name):
    """-> (nc, list of per-image (det [n, 6] float32 ranked, xywh [m, 4] float32 normalised, cls [m] float32)); the network input is IMGSZ square."""
    if name in NX.METRIC_CASES:
        return NX.METRIC_CASES[name]["nc"], [(det, to_xywh(gt.numpy()), cls) for det, gt, cls in NX.metric_case(name)]
    c = SEEDED[name]
    rs = np.random.RandomState(c["seed"])
    out = []
    for _ in range(c["images"]):
        det, gt, gcls = (_dense_image if c["kind"] == "dense" else _steal_image)(rs, c["nc"])
        out.append((torch.from_numpy(det), to_xywh(gt), torch.from_numpy(gcls.astype(np.float32))))
    return c["nc"], out


def conditions(images):
    """-> (all IoUs above 0.3 pairwise distinct within each image, smallest |iou - 0.45|, smallest |iou - level| over the ten levels, smallest
    |conf - 0.25|), IoUs in float64 on the float32 boxes."""
    distinct, gap_cm, gap_lv, gap_conf = True, np.inf, np.inf, np.inf
    levels = np.linspace(0.5, 0.95, 10)
    for det, xywh, _ in images:
        if len(det):
            gap_conf = min(gap_conf, float(np.abs(det[:, 4].double().numpy() - 0.25).min()))
        if not len(det) or not len(xywh):
            continue
        lab = label_boxes(xywh, IMGSZ, IMGSZ).double()
        a, b = lab[:, None, :], det[:, :4].double()[None, :, :]
        iw = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0])).clamp(min=0)
        ih = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1])).clamp(min=0)
        inter = iw * ih
        iou = (inter / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter + 1e-7)).numpy().ravel()
        high = iou[iou > 0.3]
        distinct = distinct and len(np.unique(high)) == len(high) and len(np.unique(high.astype(np.float32))) == len(high)
        gap_cm = min(gap_cm, float(np.abs(iou - 0.45).min()))
        gap_lv = min(gap_lv, float(np.abs(iou[:, None] - levels[None, :]).min()))
    return distinct, gap_cm, gap_lv, gap_conf


def lost_claims(images, cm_conf=CM_CONF, cm_iou=CM_IOU):
    """how many detections claim a label for the matrix and lose it to a better claimant"""
    lost = 0
    for det, xywh, _ in images:
        rows = det[det[:, 4] > cm_conf]
        if not len(rows) or not len(xywh):
            continue
        iou = iou_matrix(label_boxes(xywh, IMGSZ, IMGSZ), rows[:, :4]).numpy()
        claim, ci = iou.argmax(0), iou.max(0)
        for d in np.flatnonzero(ci > np.float32(cm_iou)):
            lost += bool((ci[(claim == claim[d])] > ci[d]).any())
    return lost


def pack(images, max_det, shuffle_seed=None):
    """per-image lists -> (det [B, max_det, 6] zero-padded, count [B] int32, lab_img [L] int32, lab_cls [L], lab_box [L, 4]); with a seed
    the label table is shuffled (a stable relative order inside each image is NOT kept: the table order is the shuffled one)."""
    det, count = NX.padded([d for d, _, _ in images], max_det)
    lab_img = torch.cat([torch.full((len(c),), i, dtype=torch.int32) for i, (_, _, c) in enumerate(images)])
    lab_cls = torch.cat([c.float() for _, _, c in images])
    lab_box = torch.cat([x.float().reshape(-1, 4) for _, x, _ in images])
    if shuffle_seed is not None:
        perm = torch.from_numpy(np.random.RandomState(shuffle_seed).permutation(len(lab_img)))
        lab_img, lab_cls, lab_box = lab_img[perm], lab_cls[perm], lab_box[perm]
    return det, count, lab_img, lab_cls, lab_box


# ---- the planted batch ---------------------------------------------------------------------------------------------------------------
PLANTED_NC, PLANTED_SHAPE, PLANTED_MAX_DET = 3, (128, 128), 16
# image 3 in ranked order, (x1, y1, x2, y2, conf, cls):
_PLANTED_ROWS = [
    (10, 10, 30, 22.4, 0.95, 0),    # 0: on label A at 0.62: holds A up to level 0.60
    (10, 10, 30, 26.4, 0.90, 0),    # 1: on A at 0.82: correct only above 0.62
    (10, 10, 30, 28.4, 0.85, 0),    # 2: on A at 0.92: correct only above 0.82; holds A in the matrix
    (50, 10, 70, 28.4, 0.80, 2),    # 3: 0.92 on B (class 1), 0.674 on C (class 2): tp through C, the matrix through B
    (80, 10, 84, 11, 0.75, 0),      # 4: 4 / 8 on D: exactly 0.5
    (80, 40, 84, 43, 0.70, 0),      # 5: 12 / 16 on E: exactly 0.75
    (100, 60, 110, 68, 0.65, 1),    # 6: 0.8 on F1 and on F2 (same box, same class)
    (100, 90, 110, 98, 0.60, 0),    # 7: 0.8 on G1 (class 0) and G2 (class 2): the lower table row, G1, in the matrix
    (100, 110, 120, 125, 0.55, 0),  # 8 and 9: the same box on H: the lower detection index holds H
    (100, 110, 120, 125, 0.50, 1),
    (10, 10, 30, 30, 0.10, 0),      # 10: A itself, below the matrix's confidence: correct at 0.95 only, absent from the matrix
]
_PLANTED_LABELS = [  # (image, cls, x1, y1, x2, y2) in TABLE order: the images interleave
    (3, 0, 10, 10, 30, 30),      # A
    (0, 1, 20, 20, 60, 60),
    (3, 1, 50, 10, 70, 30),      # B
    (3, 2, 50, 10, 70, 22.4),    # C
    (0, 2, 70, 70, 100, 120),
    (3, 0, 80, 10, 84, 12),      # D
    (3, 0, 80, 40, 84, 44),      # E
    (3, 1, 100, 60, 110, 70),    # F1
    (3, 1, 100, 60, 110, 70),    # F2
    (3, 0, 100, 90, 110, 100),   # G1
    (3, 2, 100, 90, 110, 100),   # G2
    (3, 0, 100, 110, 120, 125),  # H
]
# tp of image 3 at the ten levels 0.50 .. 0.95, worked out by hand from the comments above
PLANTED_TP3 = ["1110000000", "0001111000", "0000000110", "1111000000", "1000000000", "1111110000", "1111111000", "1111111000", "1111111111", "0000000000",
               "0000000001"]
PLANTED_CM = [[5, 0, 0, 3], [0, 1, 0, 2], [0, 1, 0, 0], [0, 2, 3, 0]]  # by hand: rows predicted 0, 1, 2, background; sum 17


def planted():
    """B = 4, nc = 3: image 0 labels only, image 1 detections only, image 2 neither, image 3 the rows above; junk past every count.
    -> (det, count, lab_img, lab_cls, lab_box)"""
    M = PLANTED_MAX_DET
    junk = torch.tensor([10.0, 10.0, 30.0, 30.0, 0.99, 0.0])  # label A's own box at a high confidence: it would match if it were read
    det = junk.repeat(4, M, 1).clone()
    count = torch.tensor([0, 3, 0, len(_PLANTED_ROWS)], dtype=torch.int32)
    det[1, :3] = torch.tensor([[5, 5, 40, 40, 0.9, 0], [60, 60, 90, 90, 0.5, 1], [20, 70, 50, 100, 0.2, 2]], dtype=torch.float32)
    det[3, : len(_PLANTED_ROWS)] = torch.tensor(_PLANTED_ROWS, dtype=torch.float32)
    lab = np.array(_PLANTED_LABELS, dtype=np.float64)
    return (det, count, torch.from_numpy(lab[:, 0].astype(np.int32)), torch.from_numpy(lab[:, 1].astype(np.float32)), to_xywh(lab[:, 2:], PLANTED_SHAPE[0]))
