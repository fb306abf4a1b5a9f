"""Detection metrics under the reference's public names: box_iou, mask_iou, match_predictions, ConfusionMatrix, compute_ap, ap_per_class, Metric, DetMetrics,
SegmentMetrics.

The text of this module is the project's own, written from the definitions of the quantities.  What is shared with the reference
(ultralytics/utils/metrics.py, engine/validator.py) is the interface - names, signatures, result keys - and the numbers: the tp matrices and
the confusion matrices are equal and P, R, AP per class and the means agree within 1e-9 on the reference-generated fixtures
(tests/test_host_nms_check.py, tests/test_valmatch_ref_cpu.py).

Definitions.  Detections are ranked by descending confidence.  At one IoU threshold a detection is *correct* when it claims a label of its own
class that it overlaps by at least the threshold and no better-ranked detection claimed that label (a detection claims the label it overlaps
most).  For one class, precision after k detections is (correct among the first k) / k and recall is (correct among the first k) / labels.
AP is the area under the precision envelope (the largest precision at any recall at least as large) over recall in [0, 1], sampled at
101 equally spaced recalls and integrated by the trapezoid rule.  P and R are read off the precision / recall-over-confidence curves at
the confidence where the box-filtered class-mean F1 peaks.

Where the work runs.  box_iou, match_predictions and ConfusionMatrix.process_batch here are HOST code: the statement of the quantities, and the
validator's match="host" path.  The validator's match="device" path computes the same tp matrices and the same confusion matrix on the device with one
launch per batch (ops.val_match, csrc/valmatch.hip) and crosses to the host once per validation; tools/probes/val_match_probe.py times the two
paths ("Validation statistics on the device", says what has been measured).  ap_per_class and what follows it stay host numpy float64: they run once per validation on
all rows.  No plotting."""
import numpy as np
import torch

CONF_GRID = 1000   # confidence samples of the P / R / F1 curves
RECALL_GRID = 101  # recall samples of the AP integral


def box_iou(box1, box2, eps=1e-7):
    """[N, 4] x [M, 4] xyxy -> [N, M] IoU in float32: inter / (area1 + area2 - inter + eps)."""
    a = torch.as_tensor(box1).float()[:, None, :]
    b = torch.as_tensor(box2).float()[None, :, :]
    wh = (torch.min(a[..., 2:], b[..., 2:]) - torch.max(a[..., :2], b[..., :2])).clamp_(0)
    inter = wh[..., 0] * wh[..., 1]
    da, db = a[..., 2:] - a[..., :2], b[..., 2:] - b[..., :2]
    return inter / (da[..., 0] * da[..., 1] + db[..., 0] * db[..., 1] - inter + eps)


def match_predictions(pred_classes, true_classes, iou, iouv):
    """-> bool [detections, thresholds]: which detections are correct at each threshold of iouv.  iou: [labels, detections] (box_iou(gt, pred));
    detections are in ranked order (NMS output order).  One greedy pass per threshold: every detection claims the same-class label it overlaps
    most, provided the overlap reaches the threshold; a label claimed more than once goes to the best-ranked claimant."""
    pred_classes, true_classes = torch.as_tensor(pred_classes).cpu(), torch.as_tensor(true_classes).cpu()
    n_lab, n_det = int(true_classes.shape[0]), int(pred_classes.shape[0])
    levels = [float(t) for t in torch.as_tensor(iouv).cpu().tolist()]
    out = np.zeros((n_det, len(levels)), dtype=bool)
    if n_lab == 0 or n_det == 0:
        return torch.from_numpy(out)
    same = (true_classes.reshape(-1, 1) == pred_classes.reshape(1, -1)).numpy()
    overlap = torch.as_tensor(iou).cpu().numpy().astype(np.float32) * same  # float32, zero where the classes differ
    claim = overlap.argmax(axis=0)                    # per detection: the label it overlaps most
    strength = overlap[claim, np.arange(n_det)]
    for t, level in enumerate(levels):
        owner = np.full(n_lab, -1)
        for d in np.flatnonzero(strength >= np.float32(level)):   # ascending = ranked order
            if owner[claim[d]] < 0:
                owner[claim[d]] = d
                out[d, t] = True
    return torch.from_numpy(out)


class ConfusionMatrix:
    """counts of (predicted class, labelled class) pairs of a detector, `matrix` [(nc + 1), (nc + 1)] int64: row = predicted class, column =
    labelled class, index nc = background (a detection that holds no label / a label no detection claims).  Reference
    utils/metrics.py:295-407 for task "detect", without the plots.

    Rule (process_batch, one image).  Only detections with conf > `conf` take part; IoU is taken regardless of class.  A detection claims the
    label it overlaps most, if that IoU exceeds `iou_thres` (both thresholds compared in float32, as a float32 tensor compares with a Python
    number); a label goes to the claimant that overlaps it most.  The holder of a label counts at [its class, the label's class]; every other
    detection - no claim, or a claim lost to a better one: it does not fall back to its next label - at [its class, nc]; a label nobody
    claims at [nc, its class].  Equal IoUs (the reference leaves them to argsort): the lower label index for a detection's claim, then the
    lower detection index for a label's holder - the rule of ymi_val_match, which fills the same matrix on the device.  Class ids are
    truncated to integers; an update in which one lies outside [0, nc) is not counted."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        self.nc = int(nc)
        self.conf = 0.25 if conf in {None, 0.001} else conf  # the validator's default confidence would count every stray: the reference substitutes 0.25
        self.iou_thres = iou_thres
        self.matrix = np.zeros((self.nc + 1, self.nc + 1), dtype=np.int64)

    def _count(self, rows, cols):
        rows, cols = np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(cols, dtype=np.int64).reshape(-1)
        ok = (rows >= 0) & (rows <= self.nc) & (cols >= 0) & (cols <= self.nc)
        np.add.at(self.matrix, (rows[ok], cols[ok]), 1)

    def _class_ids(self, values):
        """float class column -> int64 ids, truncated; outside [0, nc): -1"""
        v = np.trunc(np.asarray(values, dtype=np.float64).reshape(-1))
        return np.where((v >= 0) & (v < self.nc), v, -1).astype(np.int64)

    def process_batch(self, detections, gt_bboxes, gt_cls):
        """detections [n, 6] (x1, y1, x2, y2, conf, cls) or None, gt_bboxes [m, 4] xyxy, gt_cls [m]: one image."""
        gt_cls = torch.as_tensor(gt_cls).detach().cpu().reshape(-1)
        gc = self._class_ids(gt_cls.numpy())
        det = torch.zeros(0, 6) if detections is None else torch.as_tensor(detections).detach().cpu().float().reshape(-1, 6)
        det = det[(det[:, 4].numpy() > np.float32(self.conf)).nonzero()[0]]
        dc = self._class_ids(det[:, 5].numpy())
        n_lab, n_det = len(gc), len(dc)
        background = np.full(1, self.nc, dtype=np.int64)
        if n_lab == 0 or n_det == 0:
            self._count(dc, np.broadcast_to(background, dc.shape))
            self._count(np.broadcast_to(background, gc.shape), gc)
            return
        iou = box_iou(torch.as_tensor(gt_bboxes).detach().cpu().reshape(-1, 4), det[:, :4]).numpy()  # [labels, detections] float32
        claim = iou.argmax(axis=0)                                 # first maximum: the lower label index
        strength = iou[claim, np.arange(n_det)]
        claims = strength > np.float32(self.iou_thres)
        holder = np.full(n_lab, -1, dtype=np.int64)
        for d in np.flatnonzero(claims):                           # ascending, strict: the lower detection index keeps an equal IoU
            if holder[claim[d]] < 0 or strength[d] > strength[holder[claim[d]]]:
                holder[claim[d]] = d
        held = holder >= 0
        holds = np.zeros(n_det, dtype=bool)
        holds[holder[held]] = True
        both = held & (gc >= 0) & (dc[np.where(held, holder, 0)] >= 0)
        self._count(dc[holder[both]], gc[both])
        self._count(np.broadcast_to(background, (int((~held).sum()),)), gc[~held])
        self._count(dc[~holds], np.broadcast_to(background, (int((~holds).sum()),)))

    def tp_fp(self):
        """-> (true positives, false positives) per class, without the background row."""
        tp = self.matrix.diagonal()
        fp = self.matrix.sum(1) - tp
        return tp[:-1], fp[:-1]


def smooth(y, f=0.05):
    """moving average of y over a centred window of about 2 f len(y) samples (odd length), the ends continued with the end values."""
    y = np.asarray(y, dtype=np.float64)
    half = (int(round(2 * f * len(y))) // 2) // 2
    width = 2 * half + 1
    run = np.cumsum(np.concatenate(([0.0], np.pad(y, half, mode="edge"))))
    return (run[width:] - run[:-width]) / width


def compute_ap(recall, precision):
    """one class, one threshold: recall / precision after each ranked detection -> (AP, precision envelope, recall points).  The curve is
    closed with the points (0, 1) and (1, 0); the envelope makes precision non-increasing in recall."""
    r = np.concatenate(([0.0], np.asarray(recall, dtype=np.float64), [1.0]))
    p = np.concatenate(([1.0], np.asarray(precision, dtype=np.float64), [0.0]))
    envelope = np.maximum.accumulate(p[::-1])[::-1]
    grid = np.linspace(0.0, 1.0, RECALL_GRID)
    v = np.interp(grid, r, envelope)
    area = float(np.sum((v[1:] + v[:-1]) * np.diff(grid)) / 2)
    return area, envelope, r


def _ranked_curves(hits, n_labels, eps):
    """hits [k, T] bool in ranked order -> (recall [k, T], precision [k, T]) after each detection."""
    found = np.cumsum(hits, axis=0, dtype=np.float64)
    seen = np.arange(1, hits.shape[0] + 1, dtype=np.float64)[:, None]
    return found / (n_labels + eps), found / seen


def _over_confidence(grid, conf_ranked, values_ranked, above):
    """a ranked curve as a function of the confidence threshold: below the lowest confidence it keeps its last value, above the highest it is `above`."""
    return np.interp(grid, conf_ranked[::-1], values_ranked[::-1], right=above)


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16):
    """tp [n, T] bool, conf [n], pred_cls [n], target_cls [m] -> (tp count, fp count, p, r, f1, ap [classes, T], classes with labels, p_curve, r_curve,
    f1_curve, confidence grid, precision over recall at the first threshold), per class that has labels, in ascending class order."""
    tp, conf, pred_cls = np.asarray(tp), np.asarray(conf), np.asarray(pred_cls)
    rank = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[rank], conf[rank], pred_cls[rank]
    classes, labels_of = np.unique(np.asarray(target_cls), return_counts=True)
    grid = np.linspace(0.0, 1.0, CONF_GRID)
    ap = np.zeros((len(classes), tp.shape[1]))
    p_curve, r_curve = np.zeros((len(classes), CONF_GRID)), np.zeros((len(classes), CONF_GRID))
    pr_rows = []
    for row, (c, n_labels) in enumerate(zip(classes, labels_of)):
        mine = pred_cls == c
        if not mine.any() or n_labels == 0:
            continue
        recall, precision = _ranked_curves(tp[mine], n_labels, eps)
        r_curve[row] = _over_confidence(grid, conf[mine], recall[:, 0], 0.0)
        p_curve[row] = _over_confidence(grid, conf[mine], precision[:, 0], 1.0)
        for t in range(tp.shape[1]):
            ap[row, t], envelope, r_points = compute_ap(recall[:, t], precision[:, t])
            if t == 0:
                pr_rows.append(np.interp(grid, r_points, envelope))
    pr_at_first = np.array(pr_rows) if pr_rows else np.zeros((1, CONF_GRID))
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    peak = int(smooth(f1_curve.mean(axis=0), 0.1).argmax()) if len(classes) else 0
    p, r, f1 = p_curve[:, peak], r_curve[:, peak], f1_curve[:, peak]
    n_tp = np.round(r * labels_of)
    n_fp = np.round(n_tp / (p + eps) - n_tp)
    return n_tp, n_fp, p, r, f1, ap, classes.astype(int), p_curve, r_curve, f1_curve, grid, pr_at_first


def _mean(values):
    values = np.asarray(values, dtype=np.float64)
    return float(values.mean()) if values.size else 0.0


class Metric:
    """per-class precision, recall, F1 and AP [classes, thresholds] of the classes that have labels, and their means (0 when there are none)."""

    def __init__(self):
        self.p, self.r, self.f1, self.ap_class_index = np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, dtype=int)
        self.all_ap = np.zeros((0, 10))
        self.nc = 0

    def update(self, results):
        """results: ap_per_class(...)[2:]."""
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index, self.p_curve, self.r_curve, self.f1_curve, self.px, self.prec_values = results

    ap50 = property(lambda self: self.all_ap[:, 0])
    ap = property(lambda self: self.all_ap.mean(axis=1) if len(self.all_ap) else np.zeros(0))
    mp = property(lambda self: _mean(self.p))
    mr = property(lambda self: _mean(self.r))
    map50 = property(lambda self: _mean(self.all_ap[:, 0]))
    map75 = property(lambda self: _mean(self.all_ap[:, 5]))
    map = property(lambda self: _mean(self.all_ap))

    def mean_results(self):
        return [self.mp, self.mr, self.map50, self.map]

    def class_result(self, i):
        return self.p[i], self.r[i], self.ap50[i], self.ap[i]

    @property
    def maps(self):
        """mAP50-95 per class id; classes without labels carry the mean."""
        per_class = np.full(self.nc, self.map, dtype=np.float64)
        per_class[np.asarray(self.ap_class_index, dtype=int)] = self.ap
        return per_class

    def fitness(self):
        """the model-selection score: a tenth of mAP50 and nine tenths of mAP50-95."""
        return 0.1 * self.map50 + 0.9 * self.map


class DetMetrics:
    """precision, recall, mAP50 and mAP50-95 of a detector from the validator's statistics."""

    keys = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)"]

    def __init__(self, names=None):
        self.names = dict(names or {})
        self.box = Metric()

    def process(self, tp, conf, pred_cls, target_cls):
        self.box.nc = len(self.names)
        self.box.update(ap_per_class(tp, conf, pred_cls, target_cls)[2:])

    def mean_results(self):
        return self.box.mean_results()

    def class_result(self, i):
        return self.box.class_result(i)

    maps = property(lambda self: self.box.maps)
    fitness = property(lambda self: self.box.fitness())
    ap_class_index = property(lambda self: self.box.ap_class_index)

    @property
    def results_dict(self):
        out = dict(zip(self.keys, self.mean_results()))
        out["fitness"] = self.fitness
        return out


def mask_iou(mask1, mask2, eps=1e-7):
    """[N, n] x [M, n] flattened 0 / 1 masks -> [N, M] IoU in float32: inter / ((area1 + area2) - inter + eps) (reference utils/metrics.py:137).
    Every sum is an integer count, exact in float32 below 2^24 pixels, so the result does not depend on the order of summation; the device
    path forms the same quotient from ops.mask_overlap's integer counts (ops.val_match_masks)."""
    a, b = torch.as_tensor(mask1).float(), torch.as_tensor(mask2).float()
    inter = torch.matmul(a, b.T).clamp_(0)
    union = (a.sum(1)[:, None] + b.sum(1)[None]) - inter
    return inter / (union + eps)


class SegmentMetrics:
    """box and mask precision, recall, mAP50 and mAP50-95 of a segmentation model from the validator's statistics (reference
    utils/metrics.py:932-1066); fitness is the sum of the two Metrics' fitness."""

    keys = [f"metrics/{k}({t})" for t in "BM" for k in ("precision", "recall", "mAP50", "mAP50-95")]

    def __init__(self, names=None):
        self.names = dict(names or {})
        self.box, self.seg = Metric(), Metric()

    def process(self, tp, tp_m, conf, pred_cls, target_cls):
        self.seg.nc = self.box.nc = len(self.names)
        self.seg.update(ap_per_class(tp_m, conf, pred_cls, target_cls)[2:])
        self.box.update(ap_per_class(tp, conf, pred_cls, target_cls)[2:])

    def mean_results(self):
        return self.box.mean_results() + self.seg.mean_results()

    def class_result(self, i):
        return self.box.class_result(i) + self.seg.class_result(i)

    maps = property(lambda self: self.box.maps + self.seg.maps)
    fitness = property(lambda self: self.seg.fitness() + self.box.fitness())
    ap_class_index = property(lambda self: self.box.ap_class_index)

    @property
    def results_dict(self):
        return dict(zip(self.keys + ["fitness"], self.mean_results() + [self.fitness]))
