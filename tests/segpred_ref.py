"""Seeded inputs and the torch restatement of the inference side of segmentation, shared by tests/golden/make_segpred_golden.py (which runs the
reference on the same inputs), tests/test_segpred_cpu.py (which holds the restatement to the reference's fixtures) and
tests/test_gpu_segpred.py (which holds the kernels to both).

process_mask_values restates process_mask (reference utils/ops.py:680-710) for rows of a whole batch, in float32 or float64, and returns the
values BEFORE the `> 0` threshold, so that a test can tell a pixel whose sign is decided by rounding from one that is simply wrong.  The crop
edges are float32 products in both precisions: which pixels a box keeps is part of the statement, not of its rounding.

Exact inputs: prototypes k / 16 with |k| <= 64 (exact in bfloat16 too) and coefficients k / 8 with |k| <= 32.  Every product is a multiple of
1 / 128 below 32, every 32-term sum a multiple of 1 / 128 below 1024, and the bilinear weights at the ratio 4 are multiples of 1 / 8: all sums are
exact in float32 in any order, fused or not, so the masks are the same bits in every implementation, logits that are exactly 0 (strict `>`:
not in the mask) included."""
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = Path(__file__).resolve().parent / "golden"
NM = 32
IOUV = torch.linspace(0.5, 0.95, 10)

# name -> kind, images, prototype map (mh, mw), network input (ih, iw), seed
DECODE_CASES = {
    "exact_24x40": dict(kind="exact", B=2, mhw=(24, 40), shape=(96, 160), seed=11),   # non-square, no whole tile of either decode form
    "exact_160": dict(kind="exact", B=1, mhw=(160, 160), shape=(640, 640), seed=12),  # the multi-tile walk of the upsample form
    "real_24x40": dict(kind="real", B=2, mhw=(24, 40), shape=(96, 160), seed=13),
}


def _bf16_round(t):
    return t.to(torch.bfloat16).float()


def _random_boxes(rs, n, shape):
    ih, iw = shape
    ctr = rs.uniform(0.2, 0.8, size=(n, 2)) * (iw, ih)
    wh = rs.uniform(0.15, 0.7, size=(n, 2)) * (iw, ih)
    return np.concatenate((ctr - wh / 2, ctr + wh / 2), 1).astype(np.float32)


def decode_case(name):
    """-> (proto [B, 32, mh, mw] float32 holding bfloat16-representable values, box [N, 4] float32 in input pixels, coef [N, 32] float32,
    img [N] int32)."""
    c = DECODE_CASES[name]
    rs = np.random.RandomState(c["seed"])
    B, (mh, mw), shape = c["B"], c["mhw"], c["shape"]
    ih, iw = shape
    if c["kind"] == "real":
        proto = _bf16_round(torch.from_numpy(rs.normal(0, 1, size=(B, NM, mh, mw)).astype(np.float32)))
        n = 12
        coef = torch.from_numpy(rs.normal(0, 0.7, size=(n, NM)).astype(np.float32))
        box = torch.from_numpy(_random_boxes(rs, n, shape))
        img = torch.from_numpy((np.arange(n) % B).astype(np.int32))
        return proto, box, coef, img
    proto = torch.from_numpy(rs.randint(-64, 65, size=(B, NM, mh, mw)).astype(np.float32) / 16)
    if name == "exact_160":
        n = 3
        coef = torch.from_numpy(rs.randint(-32, 33, size=(n, NM)).astype(np.float32) / 8)
        box = torch.from_numpy(_random_boxes(rs, n, shape))
        box[1] = torch.tensor([-3.0, -3.0, 700.0, 700.0])       # every tile
        box[2] = torch.tensor([256.0, 16.0, 512.0, 320.0])      # edges on tile borders and on integer mask coordinates
        return proto, box, coef, torch.zeros(n, dtype=torch.int32)
    n = 12
    coef = torch.from_numpy(rs.randint(-32, 33, size=(n, NM)).astype(np.float32) / 8)
    box = torch.from_numpy(_random_boxes(rs, n, shape))
    img = torch.from_numpy((np.arange(n) % B).astype(np.int32))
    box[0] = torch.tensor([8.0, 4.0, 120.0, 80.0])              # edges exactly on the integer mask coordinates 2, 1, 30, 20
    box[1] = torch.tensor([0.0, 0.0, float(iw), float(ih)])     # ... and exactly on the map's border
    box[2] = torch.tensor([-10.0, -10.0, 500.0, 500.0])         # covers everything
    box[3] = torch.tensor([40.0, 40.0, 40.0, 40.0])             # zero area
    box[4] = torch.tensor([200.0, 120.0, 260.0, 150.0])         # wholly outside, beyond the far corner
    box[5] = torch.tensor([-50.0, -50.0, -10.0, -10.0])         # wholly outside, before the origin
    img[6] = -1                                                 # a row of no image
    coef[7] = 0.0                                               # every logit exactly 0: an empty mask under the strict comparison
    box[7] = torch.tensor([-1.0, -1.0, 200.0, 200.0])
    coef[8] = 0.0
    coef[8, 0] = 1.0                                            # the mask is channel 0 > 0; its zeros (about one pixel in 129) are exact-zero logits
    box[8] = torch.tensor([-1.0, -1.0, 200.0, 200.0])
    img[11] = B                                                 # a row of no image, on the other side
    return proto, box, coef, img


def crop_edges(box, mhw, shape):
    """process_mask's downsampled_bboxes: one float32 product per edge with the float32 value of the Python ratio."""
    (mh, mw), (ih, iw) = mhw, shape
    out = box.float().clone()
    out[:, 0] *= mw / iw
    out[:, 2] *= mw / iw
    out[:, 3] *= mh / ih
    out[:, 1] *= mh / ih
    return out


def process_mask_values(proto, box, coef, img, shape, upsample, dtype=torch.float32):
    """-> values [N, oh, ow] in `dtype` whose `> 0` is the mask: the cropped logits (zero outside the box, zero for rows of no image),
    resampled bilinearly (align_corners=False) to `shape` when upsample."""
    B, nm, mh, mw = proto.shape
    n = box.shape[0]
    edges = crop_edges(box, (mh, mw), shape)
    cols = torch.arange(mw, dtype=torch.float32)[None, None, :]
    rows = torch.arange(mh, dtype=torch.float32)[None, :, None]
    x1, y1, x2, y2 = (edges[:, i, None, None] for i in range(4))
    keep = (cols >= x1) & (cols < x2) & (rows >= y1) & (rows < y2)
    logits = torch.zeros(n, mh, mw, dtype=dtype)
    for b in range(B):
        sel = torch.nonzero(img == b).reshape(-1)
        if len(sel):
            logits[sel] = (coef[sel].to(dtype) @ proto[b].to(dtype).view(nm, -1)).view(-1, mh, mw)
    live = ((img >= 0) & (img < B))[:, None, None]
    logits = torch.where(keep & live, logits, torch.zeros((), dtype=dtype))
    if upsample:
        logits = F.interpolate(logits[None], tuple(shape), mode="bilinear", align_corners=False)[0]
    return logits


def pack_masks(m):
    """bool / 0-1 [N, H, W] -> the fixture's bit-packed rows."""
    return np.packbits(np.asarray(m, dtype=np.uint8).reshape(m.shape[0], -1), axis=1)


def unpack_masks(bits, shape):
    n, h, w = shape
    return torch.from_numpy(np.unpackbits(bits, axis=1)[:, : h * w].reshape(n, h, w).copy())


# ---- overlap counts and mask matching ------------------------------------------------------------------------------------------------------
def overlap_counts(masks, count, enc, n_bins):
    """masks [B, max_det, mh, mw] 0 / 1 (host), count [B], enc [B, mh, mw] -> (inter [B, max_det, n_bins], area_pred [B, max_det],
    area_gt [B, n_bins]) int32, formed with integer sums; rows past the count are zero."""
    B, max_det = masks.shape[:2]
    inter = torch.zeros(B, max_det, n_bins, dtype=torch.int32)
    area_pred = torch.zeros(B, max_det, dtype=torch.int32)
    area_gt = torch.zeros(B, n_bins, dtype=torch.int32)
    e = enc.long()
    for b in range(B):
        n = int(count[b])
        valid = (e[b] >= 0) & (e[b] < n_bins) & (enc[b].double() == e[b].double())
        area_gt[b] = torch.bincount(e[b][valid].reshape(-1), minlength=n_bins).int()
        for d in range(n):
            on = masks[b, d].bool()
            area_pred[b, d] = int(on.sum())
            inter[b, d] = torch.bincount(e[b][on & valid].reshape(-1), minlength=n_bins).int()
    return inter, area_pred, area_gt


def image_labels(lab_img, lab_cls, b):
    """the classes of image b's rows in table order."""
    return lab_cls.reshape(-1)[lab_img.reshape(-1) == b].float()


def match_case(seed, counts, labels, max_det, nc, mhw=(40, 40), ratio=4, planted_tie=False, distinct=False):
    """a batch for the overlap and matching tests.  counts / labels: detections and labels per image.  Labels are rectangles on the prototype
    grid, painted into the overlap encoding in table order (value = 1 + index among the image's rows of the SHUFFLED table, later rows on
    top).  Prototype channel k of an image is +1 inside a jittered copy of one of its label rectangles and -1 outside; a detection has a one-hot
    (sometimes two-hot: the intersection) coefficient row and a box around its rectangle, partly cutting it.  Detections past 32 per image
    repeat patterns: identical masks, equal overlaps.  distinct: one channel per detection (at most 32) - no two detections alike.
    planted_tie: image 0 gets two labels of one class, mirror images about a detection's mask (equal overlap with both).
    -> dict(det, coef, count, proto, enc, lab_img, lab_cls, lab_box, shape)."""
    rs = np.random.RandomState(seed)
    B, (mh, mw) = len(counts), mhw
    shape = (mh * ratio, mw * ratio)
    img_rows, cls_rows, rect_rows = [], [], []
    for b in range(B):
        for _ in range(labels[b]):
            w, h = rs.randint(4, mw // 2), rs.randint(4, mh // 2)
            x, y = rs.randint(0, mw - w), rs.randint(0, mh - h)
            img_rows.append(b), cls_rows.append(rs.randint(0, nc)), rect_rows.append((x, y, x + w, y + h))
    if planted_tie:
        img_rows += [0, 0]
        cls_rows += [1, 1]
        rect_rows += [(12, 30, 20, 36), (4, 30, 12, 36)]
    perm = rs.permutation(len(img_rows))
    lab_img = torch.tensor([img_rows[i] for i in perm], dtype=torch.int32)
    lab_cls = torch.tensor([cls_rows[i] for i in perm], dtype=torch.float32)
    rects = [rect_rows[i] for i in perm]
    enc = torch.zeros(B, mh, mw, dtype=torch.uint8)
    seen = [0] * B
    for r, b in zip(rects, lab_img.tolist()):
        seen[b] += 1
        enc[b, r[1] : r[3], r[0] : r[2]] = seen[b]
    lab_box = torch.tensor([[(r[0] + r[2]) / 2 / mw, (r[1] + r[3]) / 2 / mh, (r[2] - r[0]) / mw, (r[3] - r[1]) / mh] for r in rects],
                           dtype=torch.float32).reshape(-1, 4)
    proto = -torch.ones(B, NM, mh, mw)
    det = torch.from_numpy(rs.uniform(1, 100, size=(B, max_det, 6)).astype(np.float32))  # junk past the count
    coef = torch.from_numpy(rs.normal(size=(B, max_det, NM)).astype(np.float32))
    for b in range(B):
        mine = [i for i, v in enumerate(lab_img.tolist()) if v == b]
        pat = []
        for k in range(NM):
            if mine:
                x1, y1, x2, y2 = rects[mine[rs.randint(len(mine))]]
                j = rs.randint(-2, 3, size=4)
                x1, y1, x2, y2 = max(x1 + j[0], 0), max(y1 + j[1], 0), min(x2 + j[2], mw), min(y2 + j[3], mh)
            else:
                x1, y1 = rs.randint(0, mw - 8), rs.randint(0, mh - 8)
                x2, y2 = x1 + rs.randint(3, 8), y1 + rs.randint(3, 8)
            if planted_tie and b == 0 and k == 0:
                x1, y1, x2, y2 = 8, 30, 16, 36
            proto[b, k, y1:y2, x1:x2] = 1.0
            pat.append((x1, y1, x2, y2))
        n = counts[b]
        conf = np.sort(rs.uniform(0.002, 0.99, size=n))[::-1]
        for d in range(n):
            k = d % NM
            coef[b, d] = 0.0
            coef[b, d, k] = 1.0
            x1, y1, x2, y2 = pat[k]
            if not distinct and d % 7 == 3:
                coef[b, d, (k + 5) % NM] = 1.0
            cut = rs.uniform(-1.5, 2.5, size=4)  # in mask pixels: positive widens the box past the rectangle, negative cuts into it
            if planted_tie and b == 0 and d == 0:
                cut = np.array([1.0, 1.0, 1.0, 1.0])
            bx = np.array([x1 - cut[0], y1 - cut[1], x2 + cut[2], y2 + cut[3]]) * ratio
            owner = [i for i in mine if rects[i][0] <= (x1 + x2) / 2 < rects[i][2] and rects[i][1] <= (y1 + y2) / 2 < rects[i][3]]
            dcls = float(lab_cls[owner[0]]) if owner and rs.uniform() < 0.85 else float(rs.randint(0, nc))
            if planted_tie and b == 0 and d == 0:
                dcls = 1.0
            det[b, d] = torch.tensor([bx[0], bx[1], bx[2], bx[3], conf[d], dcls], dtype=torch.float32)
    return dict(det=det, coef=coef, count=torch.tensor(counts, dtype=torch.int32), proto=proto, enc=enc, lab_img=lab_img, lab_cls=lab_cls,
                lab_box=lab_box, shape=shape)


# the case the reference's _process_batch is recorded on: an image with detections and labels, one without detections, one without labels;
# no two detections of an image alike (the reference leaves equal overlaps to argsort)
REF_MATCH = dict(seed=31, counts=[20, 0, 12], labels=[6, 4, 0], max_det=24, nc=3, distinct=True)


def tp_m_host(masks, case, match_predictions, mask_iou, iouv=IOUV, single_cls=False):
    """the host path per image (reference segment/val.py:231-273 with masks=True, overlap=True): the one-hot of the encoding, mask_iou,
    match_predictions.  masks [B, max_det, mh, mw] 0 / 1 on the host -> tp_m [B, max_det, levels] uint8, zero past the count."""
    det, count, enc = case["det"], case["count"], case["enc"]
    B, max_det = det.shape[:2]
    out = torch.zeros(B, max_det, len(iouv), dtype=torch.uint8)
    for b in range(B):
        n = int(count[b])
        cls = image_labels(case["lab_img"], case["lab_cls"], b)
        nl = len(cls)
        if not n or not nl:
            continue
        index = torch.arange(nl).view(nl, 1, 1) + 1
        gt = torch.where(enc[b][None].float().repeat(nl, 1, 1) == index, 1.0, 0.0)
        iou = mask_iou(gt.view(nl, -1), masks[b, :n].reshape(n, -1).float())
        pc = det[b, :n, 5]
        if single_cls:
            pc, cls = torch.zeros_like(pc), torch.zeros_like(cls)
        out[b, :n] = match_predictions(pc, cls, iou, iouv).to(torch.uint8)
    return out


# ---- Segment-shaped NMS input --------------------------------------------------------------------------------------------------------------
def with_coefficients(y, nm, seed):
    """y [B, 4 + nc, A] -> [B, 4 + nc + nm, A]: seeded normal coefficient rows behind the scores."""
    g = torch.Generator().manual_seed(seed)
    return torch.cat((y, torch.randn(y.shape[0], nm, y.shape[2], generator=g)), 1)


def kept_coefficients(y_seg, nc, det, count):
    """the coefficient rows of the kept anchors, found from the rows themselves: the anchor whose class score and decoded box are the row's,
    bit for bit (the first such anchor).  -> [B, max_det, nm], zero past the count."""
    B, max_det = det.shape[:2]
    nm = y_seg.shape[1] - 4 - nc
    out = torch.zeros(B, max_det, nm)
    for b in range(B):
        yb = y_seg[b]
        hw, hh = yb[2] / 2, yb[3] / 2
        box = torch.stack((yb[0] - hw, yb[1] - hh, yb[0] + hw, yb[1] + hh), 1)
        for i in range(int(count[b])):
            r = det[b, i]
            hit = torch.nonzero((yb[4 + int(r[5])] == r[4]) & (box == r[None, :4]).all(1)).reshape(-1)
            assert len(hit), (b, i, r.tolist())
            out[b, i] = yb[4 + nc :, int(hit[0])]
    return out


SEG_NMS = dict(case="nc3_b3", nm=32, seed=77)  # the Segment-shaped input the reference's non_max_suppression(nc=3) is recorded on


def tp_m_from_counts(inter, area_pred, area_gt, case, match_predictions, iouv=IOUV, single_cls=False):
    """the host matching on integer counts: mask_iou's quotient in float32, labels at or beyond n_bins - 1 overlap nothing."""
    det, count = case["det"], case["count"]
    B, max_det = det.shape[:2]
    n_bins = inter.shape[2]
    out = torch.zeros(B, max_det, len(iouv), dtype=torch.uint8)
    for b in range(B):
        n = int(count[b])
        cls = image_labels(case["lab_img"], case["lab_cls"], b)
        nl = len(cls)
        if not n or not nl:
            continue
        iou = torch.zeros(nl, n)
        k = min(nl, n_bins - 1)
        fi = inter[b, :n, 1 : k + 1].t().float()
        iou[:k] = fi / ((area_gt[b, 1 : k + 1, None].float() + area_pred[b, None, :n].float()) - fi + 1e-7)
        pc = det[b, :n, 5]
        if single_cls:
            pc, cls = torch.zeros_like(pc), torch.zeros_like(cls)
        out[b, :n] = match_predictions(pc, cls, iou, iouv).to(torch.uint8)
    return out
