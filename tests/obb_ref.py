"""The oriented-box stages of csrc/loss.hip restated in float64 on the CPU, one function per stage.

Formulas: the reference's utils/loss.py (v8OBBLoss :607-720, RotatedBboxLoss :111-132), utils/tal.py (RotatedTaskAlignedAssigner :329-361,
dist2rbox :397-416, bbox2dist :391), utils/metrics.py (probiou :198-239, _get_covariance_matrix :178-195), utils/ops.py (xywhr2xyxyxyxy
:573-601) and nn/modules/head.py (OBB :211-238).  The stages that never read a box (top-k, claim, per-gt maxima) are tests/loss_exact.py's.
`restate` returns every buffer the kernels keep, by name and in their layout:

    targets [B,G,6]  dense rows (class, xywh pixels, angle)        pb [B,A,5]   decoded boxes (x, y, w, h grid units, angle)
    inside [B,G,A]   label and centre inside its rectangle         ov, al       overlap (probiou clamped at 0), alignment metric
    mpos, gidx, pa, po, wgt, lab, tss, loss, loss6                 as loss_exact.restate
    tgt [B,A,5]      target (xywh / stride, angle)                 dbox, dcls, dangle   gradients by autograd on this graph

The discrete rules:

    tiny_filter    a row is dropped unless w * img_h >= 2 and h * img_w >= 2 (the WIDTH against the image height)      (loss.py:655-656)
    label          a dense row is a label when x + y + w + h + r > 0                                                    (loss.py:659)
    inside         0 <= ap.ab <= ab.ab and 0 <= ap.ad <= ad.ad: a centre on an edge is inside                           (tal.py:349-361)
    top-k, claim   loss_exact's topk_picks / one_gt_per_anchor
    dfl_target     the target's UNROTATED extents: bbox2dist(anchor, xywh2xyxy(target xywh)) clamped to [0, 15 - 0.01]  (loss.py:126)

`fault=` plants one wrong rule (FAULTS); `margins` gives, per discrete decision, its float64 distance from flipping, and `uncertain` the
(gt, anchor) decisions a float32 evaluation may decide otherwise (margin below THRESHOLD)."""
import math

import torch

from loss_exact import ALPHA, BETA, GRAD_LOSS, HYP, REG, TAL_EPS, TOPK, _carve, anchor_grid, clamped_label, out_scale, scaled_err, topk_picks, views  # noqa: F401

FAULTS = ("inside_gt", "filter_width_by_width", "dfl_rotated_extents", "angle_centre_grad_dropped")
# (Swapping gt and pred in probiou is no fault that could be planted: the function is symmetric in its two boxes to the last bit - its sums and
# products commute, and its one ordered factor (x2 - x1) * (y1 - y2) changes both signs.  tests/test_obb_cpu.py asserts the symmetry instead.)
# margin under which a decision is left out of the comparison: inside test in pixels^2 relative to the edge's squared length, filter and label
# in their own units, gaps relative.  2^-16: float32 evaluates the dot products of ~100-pixel coordinates to about 2^-24 * 1e4 absolute.
THRESHOLD = dict(inside=2.0 ** -16, topk_gap=2.0 ** -14, claim_gap=2.0 ** -14, filter=2.0 ** -16, label=2.0 ** -16)
MAX_LEFT_OUT = 0.02  # at most this share of a case's (gt, anchor) decisions may be left out


def dense_targets(case, dtype=torch.float64, fault=None):
    """loss.py:652-657: the tiny filter, then ragged rows -> [B, G, 6] in stable order.  -> (targets, [(margin of the filter decision, row)])"""
    B, G = case["B"], case["G"]
    bi, cl, bb = case["batch"]["batch_idx"], case["batch"]["cls"].reshape(-1), case["batch"]["bboxes"].to(dtype)
    out = torch.zeros(B, G, 6, dtype=dtype)
    fm = []
    iw, ih = case["img_w"], case["img_h"]
    keep = []
    for i in range(bb.shape[0]):
        rw = bb[i, 2] * (iw if fault == "filter_width_by_width" else ih)
        rh = bb[i, 3] * (ih if fault == "filter_width_by_width" else iw)
        keep.append(bool(rw >= 2) and bool(rh >= 2))
        fm.append((float(min(abs(rw - 2), abs(rh - 2))), i))
    for b in range(B):
        rows = [i for i in range(bb.shape[0]) if keep[i] and int(bi[i]) == b][:G]
        for k, i in enumerate(rows):
            out[b, k] = torch.stack([cl[i].to(dtype), bb[i, 0] * iw, bb[i, 1] * ih, bb[i, 2] * iw, bb[i, 3] * ih, bb[i, 4]])
    return out, fm


def decode(x, angle, ax, ay):
    """DFL expectation, dist2rbox: x [B, A, 4, 16] logits, angle [B, A] -> pb [B, A, 5] grid units"""
    d = x.softmax(-1) @ torch.arange(REG, dtype=x.dtype)
    xf, yf = (d[..., 2] - d[..., 0]) / 2, (d[..., 3] - d[..., 1]) / 2
    cs, sn = torch.cos(angle), torch.sin(angle)
    return torch.stack([xf * cs - yf * sn + ax, xf * sn + yf * cs + ay, d[..., 0] + d[..., 2], d[..., 1] + d[..., 3], angle], -1)


def covariance(b):
    a, bb, c = b[..., 2] ** 2 / 12, b[..., 3] ** 2 / 12, b[..., 4]
    cs, sn = torch.cos(c), torch.sin(c)
    return a * cs ** 2 + bb * sn ** 2, a * sn ** 2 + bb * cs ** 2, (a - bb) * cs * sn


def probiou(o1, o2, eps=1e-7):
    """metrics.py:198-231 in the reference's operand order (last dim 5: xywhr)"""
    x1, y1, x2, y2 = o1[..., 0], o1[..., 1], o2[..., 0], o2[..., 1]
    a1, b1, c1 = covariance(o1)
    a2, b2, c2 = covariance(o2)
    den = (a1 + a2) * (b1 + b2) - (c1 + c2) ** 2
    t1 = ((a1 + a2) * (y1 - y2) ** 2 + (b1 + b2) * (x1 - x2) ** 2) / (den + eps) * 0.25
    t2 = ((c1 + c2) * (x2 - x1) * (y1 - y2)) / (den + eps) * 0.5
    t3 = (den / (4 * ((a1 * b1 - c1 ** 2).clamp(min=0) * (a2 * b2 - c2 ** 2).clamp(min=0)).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    return 1 - (1.0 - (-bd).exp() + eps).sqrt()


def inside_test(gt, px, py, fault=None):
    """tal.py:349-361 on gt [B, G, 5] (pixels) and centres px, py [A] -> (inside [B, G, A], margin [B, G, A]: the distance of the nearest of the
    four comparisons from flipping, relative to its edge's squared length)"""
    x, y, w, h, r = (gt[..., i][..., None] for i in range(5))
    cs, sn = torch.cos(r), torch.sin(r)
    v1x, v1y, v2x, v2y = w / 2 * cs, w / 2 * sn, -h / 2 * sn, h / 2 * cs
    ax_, ay_ = x + v1x + v2x, y + v1y + v2y
    abx, aby = (x + v1x - v2x) - ax_, (y + v1y - v2y) - ay_
    adx, ady = (x - v1x + v2x) - ax_, (y - v1y + v2y) - ay_
    apx, apy = px - ax_, py - ay_
    nab, nad = abx * abx + aby * aby, adx * adx + ady * ady
    dab, dad = apx * abx + apy * aby, apx * adx + apy * ady
    if fault == "inside_gt":
        ins = (dab > 0) & (dab < nab) & (dad > 0) & (dad < nad)
    else:
        ins = (dab >= 0) & (dab <= nab) & (dad >= 0) & (dad <= nad)
    one = torch.ones_like(nab)
    margin = torch.minimum(torch.minimum(dab.abs(), (nab - dab).abs()) / torch.maximum(nab, one), torch.minimum(dad.abs(), (nad - dad).abs()) / torch.maximum(nad, one))
    return ins, margin


def restate(case, dtype=torch.float64, grad_loss=GRAD_LOSS, grad_scale=None, scale6=None, fault=None, feats=None, angle=None, mpos=None, gidx=None,
            topk=TOPK):
    """every stage on the case's inputs (tests/obb_common.py::loss_case).  feats / angle: other inputs (e.g. bf16-rounded maps); mpos / gidx: a
    given assignment in place of the restated one."""
    assert fault is None or fault in FAULTS, fault
    B, nc, G, A = case["B"], case["nc"], case["G"], case["A"]
    fl = [t.detach().to(dtype).requires_grad_(True) for t in (feats or case["feats"])]  # [B, 64 + nc, h, w]
    ang = (angle if angle is not None else case["angle"]).detach().to(dtype).reshape(B, A).requires_grad_(True)
    x = torch.cat([t[:, : 4 * REG].permute(0, 2, 3, 1).reshape(B, -1, 4, REG) for t in fl], 1)
    sc = torch.cat([t[:, 4 * REG:].permute(0, 2, 3, 1).reshape(B, -1, nc) for t in fl], 1)
    ax, ay, st, _ = anchor_grid(case["levels"], case["strides"], dtype)
    out = {}
    targets, fmargin = dense_targets(case, dtype, fault)
    gt = targets[..., 1:]
    gsum = gt.sum(-1)
    valid = gsum > 0
    pb = decode(x, ang, ax, ay)
    out.update(targets=targets, pb=pb.detach(), valid=valid, filter_margin=fmargin, label_margin=gsum.abs())
    with torch.no_grad():
        ins, imargin = inside_test(gt, ax * st, ay * st, fault)
        m = ins & valid[..., None]
        lab_g = clamped_label(targets, nc)
        pd = pb.detach().clone()
        pd[..., :4] *= st[None, :, None]
        pd = pd[:, None].expand(B, G, A, 5)
        gtb = gt[:, :, None, :].expand(B, G, A, 5)
        raw = probiou(gtb, pd)
        ov = torch.where(m, raw.clamp(min=0), torch.zeros_like(raw))
        score = torch.sigmoid(sc).gather(2, lab_g[:, None, :].expand(B, A, G)).permute(0, 2, 1)
        al = torch.where(m, score.pow(ALPHA) * ov.pow(BETA), torch.zeros_like(ov))
        out.update(ov=ov, al=al, inside=m, inside_margin=imargin)
        if mpos is None:
            mpos = torch.zeros(B, G, A, dtype=torch.bool)
            for b in range(B):
                for k in range(G):
                    if valid[b, k]:
                        picks = topk_picks(al[b, k], min(topk, A))
                        mpos[b, k, picks] = m[b, k, picks]
        mpos = mpos.bool()
        cnt = mpos.sum(1)
        ks = torch.arange(G)[None, :, None]
        first = torch.where(mpos, ks, G).amin(1)
        if gidx is None:
            best = torch.where(ov == ov.amax(1, keepdim=True), ks, G).amin(1)
            gidx = torch.where(cnt > 1, best, torch.where(cnt == 1, first, torch.full_like(first, -1)))
        gidx = gidx.long()
        fg = gidx >= 0
        own = (gidx[:, None, :] == ks) & fg[:, None, :]
        pa = torch.where(own, al, torch.zeros_like(al)).amax(-1)
        po = torch.where(own, ov, torch.zeros_like(ov)).amax(-1)
        gi = gidx.clamp(min=0)
        al_a = al.gather(1, gi[:, None, :])[:, 0]
        wgt = torch.where(fg, al_a * po.gather(1, gi) / (pa.gather(1, gi) + TAL_EPS), torch.zeros_like(al_a))
        tg = gt.gather(1, gi[..., None].expand(B, A, 5)).clone()
        tg[..., :4] /= st[None, :, None]
        tgt = torch.where(fg[..., None], tg, torch.zeros(B, A, 5, dtype=dtype))
        lab = torch.where(fg, lab_g.gather(1, gi), torch.full_like(gi, -1))
        tss = wgt.sum()
        out.update(mpos=mpos, gidx=gidx, claimers=cnt, pa=pa, po=po, wgt=wgt, tgt=tgt, lab=lab, tss=tss, fg=fg)
    den = tss.clamp(min=1.0)
    tscore = torch.zeros(B, A, nc, dtype=dtype).scatter_(2, lab.clamp(0, nc - 1)[..., None], (wgt * fg)[..., None])
    s_cls = (sc.clamp(min=0) - sc * tscore + torch.log1p(torch.exp(-sc.abs()))).sum()
    w_fg = wgt * fg
    pbl = pb
    if fault == "angle_centre_grad_dropped":  # the centre's dependence on the angle cut: the gradient reaches the angle through the covariance only
        pbl = torch.cat([decode(x, ang.detach(), ax, ay)[..., :4], ang[..., None]], -1)
    # (background anchors are masked BEFORE probiou: a zero target box has no finite slope)
    safe_t = torch.where(fg[..., None], tgt, pbl.detach())
    pi = probiou(pbl, safe_t)
    s_box = torch.where(fg, (1.0 - pi) * w_fg, torch.zeros_like(pi)).sum()
    if fault == "dfl_rotated_extents":  # the axis-aligned hull of the rotated target instead of its own extents
        cs, sn = torch.cos(tgt[..., 4]).abs(), torch.sin(tgt[..., 4]).abs()
        hw, hh = (tgt[..., 2] * cs + tgt[..., 3] * sn) / 2, (tgt[..., 2] * sn + tgt[..., 3] * cs) / 2
    else:
        hw, hh = tgt[..., 2] / 2, tgt[..., 3] / 2
    raw_t = torch.stack([ax - (tgt[..., 0] - hw), ay - (tgt[..., 1] - hh), (tgt[..., 0] + hw) - ax, (tgt[..., 1] + hh) - ay], -1)
    tt = raw_t.clamp(0, REG - 1 - 0.01)
    tl = tt.floor().long().clamp(max=REG - 1)
    wl = (tl + 1).to(dtype) - tt
    wr = 1 - wl
    lse = torch.logsumexp(x, -1)
    xl = x.gather(-1, tl[..., None])[..., 0]
    xr = x.gather(-1, (tl + 1).clamp(max=REG - 1)[..., None])[..., 0]
    s_dfl = ((((lse - xl) * wl + (lse - xr) * wr).mean(-1)) * w_fg).sum()
    loss = torch.stack([s_box, s_cls, s_dfl]) / den
    s6 = torch.tensor(scale6 if scale6 is not None else out_scale(B), dtype=dtype)
    out.update(loss=loss.detach(), loss6=torch.cat([loss.detach() * s6[:3], loss.detach() * s6[3:]]))
    gl = torch.tensor(grad_loss, dtype=dtype)
    gs = torch.ones(3, dtype=dtype) if grad_scale is None else torch.tensor(grad_scale, dtype=dtype)
    grads = torch.autograd.grad((loss * gl * gs).sum(), fl + [ang], allow_unused=True)
    out["dfeats"] = [g if g is not None else torch.zeros_like(t) for g, t in zip(grads[:-1], fl)]
    out["dangle"] = (grads[-1] if grads[-1] is not None else torch.zeros_like(ang)).reshape(B, 1, A)
    return out


def eval_output(case, dtype=torch.float64, feats=None, angle=None):
    """OBB's eval output [B, 4 + nc + 1, A]: dist2rbox boxes * stride, class sigmoids, angle"""
    B, nc, A = case["B"], case["nc"], case["A"]
    fl = [t.to(dtype) for t in (feats or case["feats"])]
    ang = (angle if angle is not None else case["angle"]).to(dtype).reshape(B, A)
    x = torch.cat([t[:, : 4 * REG].permute(0, 2, 3, 1).reshape(B, -1, 4, REG) for t in fl], 1)
    sc = torch.cat([t[:, 4 * REG:].permute(0, 2, 3, 1).reshape(B, -1, nc) for t in fl], 1)
    ax, ay, st, _ = anchor_grid(case["levels"], case["strides"], dtype)
    pb = decode(x, ang, ax, ay)
    return torch.cat([(pb[..., :4] * st[None, :, None]).permute(0, 2, 1), torch.sigmoid(sc).permute(0, 2, 1), ang[:, None]], 1)


def angle_of(logits, dtype=torch.float64):
    """head.py:225-227 on per-level logit maps [B, 1, h, w] -> [B, 1, A]"""
    B = logits[0].shape[0]
    return (torch.sigmoid(torch.cat([t.to(dtype).reshape(B, 1, -1) for t in logits], 2)) - 0.25) * math.pi


def margins(case, r=None, topk=TOPK):
    """per discrete decision its float64 distance from flipping -> {kind: [(margin, where)]}: filter (rows), label (dense rows), inside (every
    (label, anchor)), topk_gap ((k-th - (k+1)-th metric) / k-th per label with more than k positive metrics... or any), claim_gap (anchors
    picked by several labels)"""
    r = r or restate(case)
    B, G, A = case["B"], case["G"], case["A"]
    out = dict(filter=list(r["filter_margin"]), label=[], inside=[], topk_gap=[], claim_gap=[])
    for b in range(B):
        for k in range(G):
            if float(r["targets"][b, k].abs().sum()) > 0:
                out["label"].append((float(r["label_margin"][b, k]), (b, k)))
            if not r["valid"][b, k]:
                continue
            out["inside"] += [(float(v), (b, k, a)) for a, v in enumerate(r["inside_margin"][b, k])]
            kk = min(topk, A)
            vals = torch.sort(r["al"][b, k], descending=True).values
            if kk < A and float(vals[kk - 1]) > 0:  # (picks of metric 0 lie outside the box and are filtered whichever they are)
                out["topk_gap"].append(((float(vals[kk - 1]) - float(vals[kk])) / float(vals[kk - 1]), (b, k)))
        for a in (r["claimers"][b] > 1).nonzero().flatten().tolist():
            o = torch.sort(r["ov"][b, :, a], descending=True).values
            out["claim_gap"].append(((float(o[0]) - float(o[1])) / max(float(o[0]), 1e-300), (b, a)))
    return out


def uncertain(case, r=None):
    """-> (mask [B, G, A] of the (gt, anchor) decisions left out of an equality check, share of the case's decisions it is): the inside test
    within THRESHOLD (exact zeros apart), every anchor of a label whose k-th / (k+1)-th metric gap is within it, every label at an anchor whose claim gap is; a
    filter or label decision within its threshold leaves the whole image out"""
    r = r or restate(case)
    B, G, A = case["B"], case["G"], case["A"]
    m = margins(case, r)
    mask = torch.zeros(B, G, A, dtype=torch.bool)
    for v, (b, k, a) in m["inside"]:
        if 0.0 < v < THRESHOLD["inside"]:  # (a margin of exactly 0 is an edge through a centre at angle 0: every product exact in float32 too)
            mask[b, k, a] = True
    for v, (b, k) in m["topk_gap"]:
        if v < THRESHOLD["topk_gap"]:
            mask[b, k] = True
    for v, (b, a) in m["claim_gap"]:
        if v < THRESHOLD["claim_gap"]:
            mask[b, :, a] = True
    bi = case["batch"]["batch_idx"]
    for v, i in m["filter"]:
        if v < THRESHOLD["filter"]:
            mask[int(bi[i])] = True
    for v, (b, k) in m["label"]:
        if v < THRESHOLD["label"]:
            mask[b] = True
    return mask, float(mask.float().mean()) if mask.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------- buffer layouts
def carve_state(B, A):
    BA = B * A
    return _carve([("tgt", torch.float32, BA * 5), ("wgt", torch.float32, BA), ("lab", torch.int32, BA), ("scal", torch.float32, 4)])


def carve_work(B, A, G):
    BA, BGA, BG = B * A, B * A * G, B * G
    return _carve([("pb", torch.float32, BA * 5), ("ov", torch.float32, BGA), ("al", torch.float32, BGA), ("mpos", torch.uint8, BGA),
                   ("gidx", torch.int32, BA), ("pa", torch.float32, BG), ("po", torch.float32, BG), ("tss_part", torch.float32, BA // 256 + B + 1),
                   ("part", torch.float32, (BA * 4 // 256 + 2) * 3), ("inm", torch.uint8, BGA)])


# Distance of the reference's float32 arithmetic from this restatement, per stage, worst case, in the scale of scaled_err (figures rounded up to two
# digits; measured and asserted by tests/test_obb_cpu.py::test_float32_distance_per_stage).  loss, dfeats and dangle: the REAL reference's
# fixtures (tests/golden/obb_loss_*.npz, float32 on the CPU); the stage buffers, which the reference does not hand out: this restatement run in
# float32, statement by statement the reference's operand order.  The GPU bounds of tests/test_gpu_obb_loss.py are KERNEL_FACTOR times these,
# floored at F32_FLOOR.
REF32_DISTANCE = {"targets": 2.1e-8, "pb": 8.0e-8, "ov": 1.8e-7, "al": 5.7e-7, "pa": 2.3e-7, "po": 1.3e-7, "tgt": 2.1e-8, "wgt": 7.1e-7, "tss": 9.7e-8,
                  "loss": 1.3e-7, "loss6": 1.3e-7, "dfeats": 4.1e-7, "dangle": 2.6e-6}
# Worst kernel figures on the MI355X when this was written (float32 maps, every case, same scale): within KERNEL_FACTOR times the float32
# reference's everywhere even without the floor (nearest: pa at 3.8 times, dbox at 2.3, the rest below 2) - sincosf / expf / logf / powf and
# the reduction order differ from torch's.  With bfloat16 maps the forward stages stay there (tss 2.0e-7, loss6 1.6e-7 are the only larger ones).
GPU_DISTANCE = {"targets": 2.0e-8, "pb": 1.2e-7, "ov": 1.8e-7, "al": 8.8e-7, "pa": 8.8e-7, "po": 1.4e-7, "tgt": 2.0e-8, "wgt": 9.2e-7, "tss": 1.4e-7,
                "loss6": 1.1e-7, "dbox": 9.6e-7, "dcls": 5.0e-7, "dangle": 2.4e-6}
KERNEL_FACTOR = 4.0
F32_FLOOR = 1e-3  # tests/test_gpu_modules_golden.py F32_TOL
