"""The detection loss of csrc/loss.hip restated stage by stage in float64 on the CPU, and the cases that check it.

Formulas: the reference's utils/loss.py (v8DetectionLoss.__call__ :201-255, preprocess :175-190, BboxLoss :86-108, DFLoss :65-83),
utils/tal.py (TaskAlignedAssigner :14-327, bbox2dist :391) and utils/metrics.py (bbox_iou :74-134, xywh=False, CIoU=True): the sources
oracle/loss.py cites.  `restate` returns every buffer the kernels keep, by name and in the kernels' layout:

    targets [B,G,5]   dense label rows (class, xyxy pixels)             pb [B,A,4]    decoded boxes, grid units
    ov, al  [B,G,A]   overlap (CIoU clamped at 0), alignment metric     mpos [B,G,A]  top-k picks that lie inside their gt (before the
    gidx    [B,A]     gt index per anchor, -1: background                             one-gt-per-anchor step)
    pa, po  [B,G]     per gt, largest metric / overlap among its anchors
    tgt [B,A,4]       target box, grid units (zeros on background)      wgt, lab [B,A]  weight (sum of target scores), class (-1: background)
    tss               sum of weights       loss [3]   (box, cls, dfl) sums / max(tss, 1)      loss6 [6]  loss * out_scale[:3], loss * out_scale[3:]
    dbox, dcls        per level [B,H,W,64] / [B,H,W,nc]: gradients of sum_k grad_loss[k] * grad_scale[k] * loss[k], by autograd on this graph
                      (alpha of CIoU detached, as under the reference's no_grad; targets and weights are constants)

The discrete rules, each stated once:

    centre_inside     min(px - x1, py - y1, x2 - px, y2 - py) > 1e-9: a centre on the box edge is outside           (tal.py:276-296)
    padding_row       a target row with sum(box) <= 0 is no label                                                   (loss.py:221)
    topk_picks        per label the first min(topk, A) anchors in (metric descending, index ascending) order; picks of metric 0 are
                      kept; every pick is then filtered by centre_inside.  (The reference leaves the order of equal metrics to
                      torch.topk; the kernels fix it to the lower index.)                                           (tal.py:196-228, :145)
    one_gt_per_anchor an anchor picked by several labels goes to the arg-max of the overlap over ALL labels of the image, first wins;
                      an anchor picked by one label goes to it                                                      (tal.py:298-326)
    clamped_label     class index clamped to [0, nc - 1]                                                            (tal.py:260)
    dfl_target        side distance clamped to [0, 15 - 0.01]                                                       (loss.py:75, tal.py:391)

`fault=` plants one wrong rule (FAULTS); `margins` returns, per discrete decision, its float64 distance from flipping; `carve_state` /
`carve_work` restate the buffer layouts of loss.hip (order, element types, each take rounded up to 256 bytes)."""
import math

import torch

TOPK, ALPHA, BETA, REG = 10, 0.5, 6.0, 16
TAL_EPS = 1e-9
HYP = (7.5, 0.5, 1.5)  # box, cls, dfl gains (cfg/default.yaml)
GRAD_LOSS = (0.7, -1.3, 2.1)  # the non-uniform upstream gradient of every gradient check

FAULTS = ("ciou_swapped", "centre_ge", "ties_high", "first_claimer", "argmax_claimers", "no_tss_clamp", "hw_swapped", "img_swapped",
          "grad_permuted", "dfl_clamp_15", "label_unclamped")

# ---------------------------------------------------------------------------------------------------------------------------------- cases
# labels: explicit rows (image, class, cx, cy, w, h normalised) followed by `random` = [(image, count)] seeded rows.  exempt: the exact-tie
# situations of the case, decided identically in float32 and float64 (nothing to guard).  Seeds were picked on the CPU until the guards
# of tests/test_host_loss_check.py held for the reference arithmetic alone.
_L3 = dict(levels=((8, 8), (4, 4), (2, 2)), strides=(8.0, 16.0, 32.0))
_CROWDED_ROWS = [
    (0, 5, 0.5, 0.5, 0.625, 0.625),        # r0 edges x, y = 12 and 52 run exactly through level-0 centres (4 + 8 i)
    (0, 10, 0.3125, 0.59375, 0.40625, 0.3125),   # r1, r2 two identical rows
    (0, 10, 0.3125, 0.59375, 0.40625, 0.3125),
    (0, 20, 0.65625, 0.40625, 0.4375, 0.34375),  # r3, r4 one box, two classes: equal overlaps, the lower row wins
    (0, 21, 0.65625, 0.40625, 0.4375, 0.34375),
    (0, 30, 0.5, 0.5, 0.09375, 0.09375),   # r5 x, y in [29, 35]: contains no centre of any level (pa = 0)
    (0, 40, 0.125, 0.0625, 0.21875, 0.09375),  # r6 x in [1, 15], y in [1, 7]: anchors 0 and 1 only; their large predicted boxes give CIoU <= 0
]
CASES = {
    "base": dict(_L3, B=2, nc=3, random=[(0, 3), (1, 2)], seed=1, guarded=True, exempt=("zero_metric_picks",)),
    "rect": dict(levels=((12, 20), (6, 10), (3, 5)), strides=(8.0, 16.0, 32.0), B=3, nc=5, rows=[(0, 2, 0.5, 0.5, 0.97, 0.45)],
                 random=[(0, 3), (2, 7)], seed=1, guarded=True, exempt=("zero_metric_picks",)),
    "four_levels": dict(levels=((8, 16), (4, 8), (2, 4), (1, 2)), strides=(8.0, 16.0, 32.0, 64.0), B=1, nc=1,
                        rows=[(0, 0, 0.40, 0.45, 0.17, 0.3)], seed=1, guarded=True, exempt=("zero_metric_picks",)),
    "one_level_short": dict(levels=((3, 3),), strides=(32.0,), B=1, nc=2, random=[(0, 2)], seed=15, guarded=False, exempt=()),
    "crowded": dict(_L3, B=2, nc=80, rows=_CROWDED_ROWS, random=[(0, 5), (1, 3)], crowd=True, seed=1, guarded=True,
                    exempt=("identical_rows", "identical_boxes", "edge_through_centres", "zero_metric_picks")),
    "labels_out_of_range": dict(_L3, B=1, nc=3, rows=[(0, 7, 0.4, 0.5, 0.5, 0.4), (0, -1, 0.6, 0.45, 0.4, 0.55)], seed=1, guarded=False, exempt=()),
    "no_labels": dict(_L3, B=2, nc=3, max_boxes=1, seed=1, guarded=False, exempt=()),
    "long_row": dict(levels=((104, 100),), strides=(8.0,), B=1, nc=1, random=[(0, 3)], seed=1, guarded=False, exempt=()),
}
GUARDED = tuple(n for n, c in CASES.items() if c["guarded"])

_case_cache = {}


def build(name):
    """inputs of a case, float32, made once and never written: box / cls maps per level [B,H,W,64] / [B,H,W,nc] (NHWC), the ragged labels
    batch_idx [n], cls [n], bboxes [n,4], image size, G (target rows per image)"""
    if name in _case_cache:
        return _case_cache[name]
    c = CASES[name]
    gen = torch.Generator().manual_seed(1000 + c["seed"])
    B, nc = c["B"], c["nc"]
    box, cls = [], []
    for H, W in c["levels"]:
        m = torch.randn(B, H, W, 4 * REG + nc, generator=gen)
        box.append((m[..., : 4 * REG] * 2).contiguous())
        cls.append(m[..., 4 * REG:].contiguous())
    rows = [tuple(float(v) for v in r) for r in c.get("rows", [])]
    for img, count in c.get("random", []):
        if c.get("crowd"):
            ctr, wh = torch.rand(count, 2, generator=gen) * 0.3 + 0.35, torch.rand(count, 2, generator=gen) * 0.4 + 0.2
        else:
            ctr, wh = torch.rand(count, 2, generator=gen) * 0.5 + 0.25, torch.rand(count, 2, generator=gen) * 0.4 + 0.1
        lab = torch.randint(0, nc, (count,), generator=gen)
        rows += [(float(img), float(lab[i]), *ctr[i].tolist(), *wh[i].tolist()) for i in range(count)]
    rows.sort(key=lambda r: r[0])  # (stable: the order inside an image is the row order)
    t = torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)
    counts = [int((t[:, 0] == b).sum()) for b in range(B)]
    (H0, W0), s0 = c["levels"][0], c["strides"][0]
    inp = dict(name=name, B=B, nc=nc, levels=c["levels"], strides=c["strides"], box=box, cls=cls, batch_idx=t[:, 0].contiguous(),
               labels=t[:, 1].contiguous(), bboxes=t[:, 2:].contiguous(), img_w=W0 * s0, img_h=H0 * s0, G=c.get("max_boxes", max(counts + [1])),
               A=sum(h * w for h, w in c["levels"]))
    _case_cache[name] = inp
    return inp


def out_scale(B):
    """the criterion's two results from one launch: loss * gain * batch (differentiated) and loss * gain (logged)"""
    return [g * B for g in HYP] + list(HYP)


# ---------------------------------------------------------------------------------------------------------------------------- restatement
def anchor_grid(levels, strides, dtype=torch.float64, fault=None):
    """-> ax, ay (grid units), stride, level per anchor [A]; anchor a of level l is pixel q = a - off[l], row-major (y, x)"""
    ax, ay, st, lv = [], [], [], []
    for l, ((H, W), s) in enumerate(zip(levels, strides)):
        q = torch.arange(H * W)
        w = H if fault == "hw_swapped" else W
        y = q // w
        x = q - y * w
        ax.append(x.to(dtype) + 0.5)
        ay.append(y.to(dtype) + 0.5)
        st.append(torch.full((H * W,), s, dtype=dtype))
        lv.append(torch.full((H * W,), l))
    return torch.cat(ax), torch.cat(ay), torch.cat(st), torch.cat(lv)


def dense_targets(inp, dtype=torch.float64, fault=None):
    """loss.py:175-190 preprocess: ragged rows -> [B, G, 5] (class, xyxy pixels), empty slots zero"""
    B, G = inp["B"], inp["G"]
    sw, sh = (inp["img_h"], inp["img_w"]) if fault == "img_swapped" else (inp["img_w"], inp["img_h"])
    out = torch.zeros(B, G, 5, dtype=dtype)
    bb = inp["bboxes"].to(dtype)
    for b in range(B):
        rows = (inp["batch_idx"] == b).nonzero().flatten().tolist()[:G]
        for k, i in enumerate(rows):
            cx, cy, bw, bh = bb[i, 0] * sw, bb[i, 1] * sh, bb[i, 2] * sw, bb[i, 3] * sh
            out[b, k] = torch.stack([inp["labels"][i].to(dtype), cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2])
    return out


def ciou(b1, b2, eps=1e-7):
    """metrics.py:74-134 on xyxy boxes (last dim 4); alpha is a constant"""
    x1, y1, x2, y2 = b1.unbind(-1)
    X1, Y1, X2, Y2 = b2.unbind(-1)
    w1, h1, w2, h2 = x2 - x1, y2 - y1 + eps, X2 - X1, Y2 - Y1 + eps
    inter = (torch.minimum(x2, X2) - torch.maximum(x1, X1)).clamp(min=0) * (torch.minimum(y2, Y2) - torch.maximum(y1, Y1)).clamp(min=0)
    union = w1 * h1 + w2 * h2 - inter + eps
    iou = inter / union
    cw = torch.maximum(x2, X2) - torch.minimum(x1, X1)
    ch = torch.maximum(y2, Y2) - torch.minimum(y1, Y1)
    c2 = cw ** 2 + ch ** 2 + eps
    rho2 = ((X1 + X2 - x1 - x2) ** 2 + (Y1 + Y2 - y1 - y2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    alpha = (v / (v - iou + (1 + eps))).detach()
    return iou - (rho2 / c2 + v * alpha)


def centre_dmin(ax, ay, st, gt):
    """signed distance of every anchor centre from the nearest edge of every gt box, pixels: [B, G, A]"""
    px, py = (ax * st)[None, None], (ay * st)[None, None]
    g = gt[:, :, None, :]
    return torch.minimum(torch.minimum(px - g[..., 0], py - g[..., 1]), torch.minimum(g[..., 2] - px, g[..., 3] - py))


def clamped_label(targets, nc):
    return targets[..., 0].long().clamp(0, nc - 1)  # (.long() truncates toward zero, as the kernel's (int))


def topk_picks(al_row, k, high=False):
    """the first k indices in (value descending, index ascending) order; `high`: the planted fault, ties to the higher index"""
    n = al_row.numel()
    if high:
        order = (n - 1) - torch.sort(-al_row.flip(0), stable=True).indices
    else:
        order = torch.sort(-al_row, stable=True).indices
    return order[:k]


def restate(inp, dtype=torch.float64, grad_loss=GRAD_LOSS, grad_scale=None, scale6=None, fault=None, box=None, cls=None, mpos=None,
            gidx=None, topk=TOPK):
    """every stage of the loss on the case's inputs.  box / cls: other maps (e.g. bf16-rounded ones); mpos / gidx: a given assignment
    (the kernel's own, for the bfloat16 comparison) in place of the restated one."""
    assert fault is None or fault in FAULTS, fault
    inp = build(inp) if isinstance(inp, str) else inp
    B, nc, G, A = inp["B"], inp["nc"], inp["G"], inp["A"]
    box_l = [t.detach().to(dtype).requires_grad_(True) for t in (box or inp["box"])]
    cls_l = [t.detach().to(dtype).requires_grad_(True) for t in (cls or inp["cls"])]
    x = torch.cat([t.reshape(B, -1, 4, REG) for t in box_l], 1)  # [B, A, 4, 16]
    sc = torch.cat([t.reshape(B, -1, nc) for t in cls_l], 1)  # [B, A, nc]
    ax, ay, st, _ = anchor_grid(inp["levels"], inp["strides"], dtype, fault)
    out = {}

    # targets, DFL decode
    targets = dense_targets(inp, dtype, fault)
    gt = targets[..., 1:]
    valid = gt.sum(-1) > 0  # padding_row
    dist = x.softmax(-1) @ torch.arange(REG, dtype=dtype)  # [B, A, 4]
    pb = torch.stack([ax - dist[..., 0], ay - dist[..., 1], ax + dist[..., 2], ay + dist[..., 3]], -1)
    out["targets"], out["pb"] = targets, pb.detach()

    with torch.no_grad():
        # alignment metric
        dmin = centre_dmin(ax, ay, st, gt)
        inside = (dmin >= 0) if fault == "centre_ge" else (dmin > TAL_EPS)  # centre_inside
        m = inside & valid[..., None]
        lab_g = clamped_label(targets, nc)  # [B, G]
        pd = (pb.detach() * st[None, :, None])[:, None].expand(B, G, A, 4)
        gtb = gt[:, :, None, :].expand(B, G, A, 4)
        c = ciou(pd, gtb) if fault == "ciou_swapped" else ciou(gtb, pd)
        ov = torch.where(m, c.clamp(min=0), torch.zeros_like(c))
        score = torch.sigmoid(sc).gather(2, lab_g[:, None, :].expand(B, A, G)).permute(0, 2, 1)  # [B, G, A]
        al = torch.where(m, score.pow(ALPHA) * ov.pow(BETA), torch.zeros_like(ov))
        out["ov"], out["al"], out["inside"], out["valid"], out["dmin"], out["ciou_raw"] = ov, al, inside, valid, dmin, c

        # topk_picks
        if mpos is None:
            mpos = torch.zeros(B, G, A, dtype=torch.bool)
            for b in range(B):
                for k in range(G):
                    if valid[b, k]:
                        picks = topk_picks(al[b, k], min(topk, A), high=fault == "ties_high")
                        mpos[b, k, picks] = inside[b, k, picks]
        mpos = mpos.bool()
        out["mpos"] = mpos

        # one_gt_per_anchor
        cnt = mpos.sum(1)  # [B, A]
        ks = torch.arange(G)[None, :, None]
        first = torch.where(mpos, ks, G).amin(1)
        if gidx is None:
            if fault == "argmax_claimers":
                o = torch.where(mpos, ov, torch.full_like(ov, -1.0))
            else:
                o = ov
            best = torch.where(o == o.amax(1, keepdim=True), ks, G).amin(1)  # first wins
            if fault == "first_claimer":
                best = first
            gidx = torch.where(cnt > 1, best, torch.where(cnt == 1, first, torch.full_like(first, -1)))
        gidx = gidx.long()
        out["gidx"], out["claimers"] = gidx, cnt

        # per-gt maxima, targets per anchor
        fg = gidx >= 0
        own = (gidx[:, None, :] == ks) & fg[:, None, :]  # [B, G, A]
        pa = torch.where(own, al, torch.zeros_like(al)).amax(-1)
        po = torch.where(own, ov, torch.zeros_like(ov)).amax(-1)
        gi = gidx.clamp(min=0)
        al_a = al.gather(1, gi[:, None, :])[:, 0]
        wgt = torch.where(fg, al_a * po.gather(1, gi) / (pa.gather(1, gi) + TAL_EPS), torch.zeros_like(al_a))
        tgt = torch.where(fg[..., None], gt.gather(1, gi[..., None].expand(B, A, 4)) / st[None, :, None], torch.zeros(B, A, 4, dtype=dtype))
        raw_lab = targets[..., 0].long() if fault == "label_unclamped" else lab_g
        lab = torch.where(fg, raw_lab.gather(1, gi), torch.full_like(gi, -1))
        tss = wgt.sum()
        out.update(pa=pa, po=po, wgt=wgt, tgt=tgt, lab=lab, tss=tss)

    # loss sums
    den = tss if fault == "no_tss_clamp" else tss.clamp(min=1.0)
    lab_c = lab.clamp(0, nc - 1)
    tscore = torch.zeros(B, A, nc, dtype=dtype).scatter_(2, lab_c[..., None], (wgt * fg)[..., None])
    s_cls = (sc.clamp(min=0) - sc * tscore + torch.log1p(torch.exp(-sc.abs()))).sum()
    w_fg = wgt * fg
    s_box = ((1.0 - ciou(pb, tgt)) * w_fg).sum()
    axy = torch.stack([ax, ay], -1)[None]
    raw_t = torch.cat([axy - tgt[..., :2], tgt[..., 2:] - axy], -1)  # [B, A, 4]
    tt = raw_t.clamp(0, float(REG - 1) if fault == "dfl_clamp_15" else REG - 1 - 0.01)  # dfl_target
    tl = tt.floor().long().clamp(max=REG - 1)
    wl = (tl + 1).to(dtype) - tt
    wr = 1 - wl
    lse = torch.logsumexp(x, -1)
    xl = x.gather(-1, tl[..., None])[..., 0]
    xr = x.gather(-1, (tl + 1).clamp(max=REG - 1)[..., None])[..., 0]
    s_dfl = ((((lse - xl) * wl + (lse - xr) * wr).mean(-1)) * w_fg).sum()
    loss = torch.stack([s_box, s_cls, s_dfl]) / den
    out["loss"] = loss.detach()
    s6 = torch.tensor(scale6 if scale6 is not None else out_scale(B), dtype=dtype)
    out["loss6"] = torch.cat([loss.detach() * s6[:3], loss.detach() * s6[3:]])
    out["raw_t"], out["fg"] = raw_t.detach(), fg

    # gradients
    gl = torch.tensor(grad_loss, dtype=dtype)
    if fault == "grad_permuted":
        gl = gl[[1, 2, 0]]
    gs = torch.ones(3, dtype=dtype) if grad_scale is None else torch.tensor(grad_scale, dtype=dtype)
    grads = torch.autograd.grad((loss * gl * gs).sum(), box_l + cls_l)
    out["dbox"], out["dcls"] = list(grads[: len(box_l)]), list(grads[len(box_l):])
    return out


def decode(inp, dtype=torch.float64, box=None, cls=None, mc=None):
    """Detect._inference (head.py:103-142): [B, 4 + nc (+ nm), A]: xywh pixels, sigmoid scores, mask coefficients as they are"""
    B, nc = inp["B"], inp["nc"]
    x = torch.cat([t.to(dtype).reshape(B, -1, 4, REG) for t in (box or inp["box"])], 1)
    sc = torch.cat([t.to(dtype).reshape(B, -1, nc) for t in (cls or inp["cls"])], 1)
    ax, ay, st, _ = anchor_grid(inp["levels"], inp["strides"], dtype)
    d = x.softmax(-1) @ torch.arange(REG, dtype=dtype)
    x1, y1, x2, y2 = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
    rows = [torch.stack([(x1 + x2) / 2 * st, (y1 + y2) / 2 * st, (x2 - x1) * st, (y2 - y1) * st], 1), torch.sigmoid(sc).permute(0, 2, 1)]
    if mc is not None:
        rows.append(torch.cat([t.to(dtype).reshape(B, -1, t.shape[-1]) for t in mc], 1).permute(0, 2, 1))
    return torch.cat(rows, 1)


# -------------------------------------------------------------------------------------------------------------------------------- margins
def margins(inp, r=None, topk=TOPK):
    """per discrete decision of the case, its float64 distance from flipping -> {kind: [(margin, where), ...]}; decisions that are exact
    ties (margin exactly 0: identical rows, an edge through centres, picks of metric 0) are returned under "<kind>_exact".

    centre       |dmin - eps|, pixels, every (label, anchor)
    ciou_sign    |ciou| of every in-box pair (the clamp at 0)
    topk_gap     (k-th - (k+1)-th metric) / k-th of every label, k = min(topk, A)
    claim_gap    (best - second overlap) / best at every anchor picked by several labels
    grad_sides   |b1 - b2| per coordinate and the raw intersection width / height against 0, grid units, every foreground anchor of
                 positive weight (the indicator functions of the CIoU gradient)"""
    inp = build(inp) if isinstance(inp, str) else inp
    r = r or restate(inp)
    B, G, A = inp["B"], inp["G"], inp["A"]
    out = {k: [] for k in ("centre", "centre_exact", "ciou_sign", "topk_gap", "topk_gap_exact", "claim_gap", "claim_gap_exact", "grad_sides")}
    for b in range(B):
        for k in range(G):
            if not r["valid"][b, k]:
                continue
            d = r["dmin"][b, k]
            for a in range(A):
                v = float(d[a])
                out["centre_exact" if v == 0.0 else "centre"].append((abs(v - TAL_EPS), (b, k, a)))
                if r["inside"][b, k, a]:
                    out["ciou_sign"].append((abs(float(r["ciou_raw"][b, k, a])), (b, k, a)))
            kk = min(topk, A)
            if kk < A:
                vals = torch.sort(r["al"][b, k], descending=True).values
                vk, vn = float(vals[kk - 1]), float(vals[kk])
                if vk == vn:
                    out["topk_gap_exact"].append((0.0, (b, k, vk)))
                else:
                    out["topk_gap"].append(((vk - vn) / vk, (b, k)))
        for a in (r["claimers"][b] > 1).nonzero().flatten().tolist():
            o = torch.sort(r["ov"][b, :, a], descending=True).values
            if G < 2:
                continue
            if float(o[0]) == float(o[1]):
                out["claim_gap_exact"].append((0.0, (b, a, float(o[0]))))
            else:
                out["claim_gap"].append(((float(o[0]) - float(o[1])) / float(o[0]), (b, a)))
        for a in ((r["gidx"][b] >= 0) & (r["wgt"][b] > 0)).nonzero().flatten().tolist():
            p, t = r["pb"][b, a], r["tgt"][b, a]
            iw = float(torch.minimum(p[2], t[2]) - torch.maximum(p[0], t[0]))
            ih = float(torch.minimum(p[3], t[3]) - torch.maximum(p[1], t[1]))
            out["grad_sides"].append((min(float((p - t).abs().min()), abs(iw), abs(ih)), (b, a)))
    return out


# ------------------------------------------------------------------------------------------------------------------------- buffer layouts
def _carve(takes):
    """[(name, dtype, elements)] -> ({name: (byte offset, dtype, elements)}, total bytes): every take is rounded up to 256 bytes"""
    lay, used = {}, 0
    for name, dt, n in takes:
        lay[name] = (used, dt, n)
        used += (n * torch.empty((), dtype=dt).element_size() + 255) // 256 * 256
    return lay, used


def carve_state(B, A):
    """loss.hip carve_state: what the forward leaves for the backward"""
    BA = B * A
    return _carve([("tgt", torch.float32, BA * 4), ("wgt", torch.float32, BA), ("lab", torch.int32, BA), ("scal", torch.float32, 4)])


def carve_work(B, A, G):
    """loss.hip carve_work: the forward's scratch buffers"""
    BA, BGA, BG = B * A, B * A * G, B * G
    return _carve([("pb", torch.float32, BA * 4), ("ov", torch.float32, BGA), ("al", torch.float32, BGA), ("mpos", torch.uint8, BGA),
                   ("gidx", torch.int32, BA), ("pa", torch.float32, BG), ("po", torch.float32, BG), ("tss_part", torch.float32, BA // 256 + B + 1),
                   ("part", torch.float32, (BA * 4 // 256 + 2) * 3)])


def written(B, A):
    """elements of the takes that hold more than the forward writes: one weight sum per finalize workgroup (ceil(A / 256) per image), three
    sums per loss workgroup (ceil(B A 4 / 256)), scal[0]"""
    return {"tss_part": (A + 255) // 256 * B, "part": (B * A * 4 + 255) // 256 * 3, "scal": 1}


def views(buf, layout):
    """a uint8 tensor holding a carved buffer -> {name: typed view of the take}"""
    out = {}
    for name, (off, dt, n) in layout.items():
        out[name] = buf[off: off + n * torch.empty((), dtype=dt).element_size()].view(dt)
    return out


# ---------------------------------------------------------------------------------------------------------------------------- comparison
def scaled_err(got, ref):
    """worst |got - ref| / (|ref| + max |ref|) over the elements: per element, against the stage's largest magnitude, no floor.  A stage that
    is zero throughout must be reproduced exactly."""
    got, ref = torch.as_tensor(got).detach().double().reshape(-1), torch.as_tensor(ref).detach().double().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float("inf")
    big = float(ref.abs().max())
    if big == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float(((got - ref).abs() / (ref.abs() + big)).max())


# Distance of the float32 oracle (oracle/loss.py on the CPU) from this restatement, per stage, worst guarded case, in the scale of scaled_err:
# measured and asserted by tests/test_host_loss_check.py::test_oracle_float32_distance_per_stage (figures rounded up to two digits).  The GPU
# bounds of tests/test_gpu_loss_exact.py are 8 times these.
ORACLE_DISTANCE = {"targets": 3.7e-8, "pb": 9.1e-8, "ov": 3.2e-7, "al": 8.2e-7, "pa": 5.1e-7, "po": 9.9e-8, "tgt": 3.7e-8, "wgt": 8.4e-7, "tss": 7.1e-7,
                   "loss": 3.1e-8, "loss6": 3.1e-8, "dbox": 8.2e-7, "dcls": 2.4e-7}
KERNEL_FACTOR = 8.0
