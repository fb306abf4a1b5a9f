"""What tests/golden/make_seg_golden.py and the segmentation tests share: the head and loss cases, their seeds and their batches.  Weights and
inputs are rebuilt from seeds on both sides (tests/golden_weights.py); the fixtures store only what the reference produced."""
import numpy as np
import torch

from golden_weights import seeded_array, seeded_inputs
from psa_common import seeded_module_state

NC, NM, NPR, CH, STRIDE = 3, 32, 32, (32, 64, 128), (8.0, 16.0, 32.0)  # Segment(3, 32, 32, (32, 64, 128)) with strides 8, 16, 32
HEAD_SEED, PROTO_SEED, LOSS_SEED, E2E_SEED = 4100, 4150, 4200, 41
SCALES = ("n", "s", "m")
E2E_NC, E2E_BATCH, E2E_SIZE = 3, 2, 128
E2E_MODELS = {"seg_e2e_v8n": "yolov8n-seg.yaml", "seg_e2e_11n": "yolo11n-seg.yaml"}
HYP = dict(box=7.5, cls=0.5, dfl=1.5, overlap_mask=True)

PROTO_CASE = ("seg_proto_32", (32, 32, 32), (2, 32, 6, 5))  # name, Proto(c1, c_, c2), input shape (odd map: 30 pixels, no multiple of a tile)


def level_hw(img_hw):
    """map sizes of the three levels for an image of (h, w): stride-2 convolutions with 'same' padding round up."""
    h, w = img_hw
    out = []
    for s in (8, 16, 32):
        out.append((-(-h // s), -(-w // s)))
    return out


def ellipse_masks(boxes_by_image, hw):
    """overlap encoding [B, h, w] uint8: pixel = 1 + index of the LAST label of the image whose ellipse (inscribed in its box) covers it."""
    h, w = hw
    ys = (torch.arange(h, dtype=torch.float32) + 0.5) / h
    xs = (torch.arange(w, dtype=torch.float32) + 0.5) / w
    out = torch.zeros(len(boxes_by_image), h, w, dtype=torch.uint8)
    for b, boxes in enumerate(boxes_by_image):
        for k, (cx, cy, bw, bh) in enumerate(boxes):
            inside = ((xs[None, :] - cx) / (bw / 2)) ** 2 + ((ys[:, None] - cy) / (bh / 2)) ** 2 <= 1.0
            out[b][inside] = k + 1
    return out


def _random_boxes(rs, n):
    ctr = rs.uniform(0.2, 0.8, size=(n, 2))
    wh = rs.uniform(0.1, 0.35, size=(n, 2))
    return [tuple(float(v) for v in (*c, *s)) for c, s in zip(ctr, wh)]


def _loss_cases():
    rs = np.random.RandomState(LOSS_SEED)
    # (no box edge lies on a mask-pixel boundary, where the last bit of a float32 coordinate would decide a whole row of the crop: test_seg_cpu.py)
    base = [[(0.3013, 0.3521, 0.4021, 0.4517), (0.6532, 0.6011, 0.5017, 0.4033), (0.5021, 0.5013, 0.2519, 0.7027)], [(0.5517, 0.4521, 0.6023, 0.5519)]]
    cases = {
        # name: (image (h, w), boxes per image (cx, cy, w, h normalised), mask size relative to the prototype map)
        "seg_loss_base": ((96, 96), base, 1),
        "seg_loss_nonsquare": ((80, 112), [[(0.3013, 0.4021, 0.3517, 0.5013), (0.7021, 0.5513, 0.4017, 0.4521)], [(0.5017, 0.5023, 0.5511, 0.6019)]], 1),  # prototypes 20 x 28
        # image 0: 20 boxes on 128 x 128 (336 anchors), more foreground anchors than one 64-record tile; image 1: no labels
        "seg_loss_many": ((128, 128), [_random_boxes(rs, 20), []], 1),
        # a box that reaches the image border; one narrower than a mask pixel between two mask columns (mask x in (10.2, 10.8)): every anchor
        # centre is an integer mask coordinate, so it can hold none and stays without foreground, as in the reference (an empty crop with a
        # foreground anchor cannot occur); and a narrow one around a column (mask x in (12.2, 13.8), anchor centres at x = 13; thinner ones overlap no
        # prediction and the assignment gives them nothing): its two foreground anchors have a crop ONE pixel wide
        "seg_loss_edge": ((96, 96), [[(0.80, 0.5013, 0.40, 0.6021), (10.5 / 24, 0.5011, 0.6 / 24, 0.5017), (13.0 / 24, 0.4513, 1.6 / 24, 0.2013)],
                                     [(0.2513, 0.8507, 0.5026, 0.2986)]], 1),
        "seg_loss_masks2x": ((96, 96), base, 2),  # masks at twice the prototype size: the nearest rule
        "seg_loss_nofg": ((96, 96), [[], []], 1),
    }
    return cases


LOSS_CASES = _loss_cases()


def loss_case(name, mask_dtype=torch.uint8):
    """-> (feats [B, 64 + nc, h, w] per level, mc [B, nm, A], proto [B, nm, mh, mw], batch) of a loss case, everything float32 on the CPU."""
    img_hw, boxes, mscale = LOSS_CASES[name]
    seed = LOSS_SEED + 10 * list(LOSS_CASES).index(name)
    B = len(boxes)
    hws = level_hw(img_hw)
    rs = np.random.RandomState(seed)
    feats = [torch.from_numpy(seeded_array(rs, (B, 64 + NC, h, w))) for h, w in hws]
    A = sum(h * w for h, w in hws)
    mc = torch.from_numpy(seeded_array(rs, (B, NM, A), 0.5))
    mh, mw = img_hw[0] // 4, img_hw[1] // 4
    proto = torch.from_numpy(seeded_array(rs, (B, NM, mh, mw), 0.5))
    rows = [(b, k % NC, *bx) for b, bxs in enumerate(boxes) for k, bx in enumerate(bxs)]
    t = torch.tensor(rows, dtype=torch.float32).reshape(-1, 6)
    masks = ellipse_masks(boxes, (mh * mscale, mw * mscale)).to(mask_dtype)
    batch = {"batch_idx": t[:, 0].clone(), "cls": t[:, 1:2].clone(), "bboxes": t[:, 2:6].clone(), "masks": masks,
             "max_boxes": max(1, max(len(b) for b in boxes))}
    return feats, mc, proto, batch


def head_inputs():
    """([x per level], [gy of the train maps per level], gy of mc, gy of p) of the Segment head case: two 96 x 96 images, maps 12, 6, 3."""
    xs, gys = [], []
    for i, (c, (h, w)) in enumerate(zip(CH, level_hw((96, 96)))):
        x, gy = seeded_inputs(HEAD_SEED + 10 * i, (2, c, h, w), (2, 64 + NC, h, w))
        xs.append(x)
        gys.append(gy)
    A = sum(h * w for h, w in level_hw((96, 96)))
    gmc, gp = seeded_inputs(HEAD_SEED + 50, (2, NM, A), (2, NM, 24, 24))
    return xs, gys, gmc, gp


def mask_edges_off_grid(boxes_by_image, mask_hw, margin=1e-4):
    """every box edge, in mask pixels, is at least `margin` away from an integer - or lies on / outside the map's border, where clamping decides"""
    mh, mw = mask_hw
    for boxes in boxes_by_image:
        for cx, cy, bw, bh in boxes:
            for v, size in ((cx - bw / 2, mw), (cx + bw / 2, mw), (cy - bh / 2, mh), (cy + bh / 2, mh)):
                m = v * size
                if 1e-6 < m < size - 1e-6 and abs(m - round(m)) < margin:
                    return False
    return True


E2E_BOXES = None


def e2e_state(model):
    return seeded_module_state(model, E2E_SEED)


def e2e_batch():
    img, _ = seeded_inputs(E2E_SEED, (E2E_BATCH, 3, E2E_SIZE, E2E_SIZE), (1,))
    img = (img * 0.25 + 0.5).clamp(0, 1)
    global E2E_BOXES
    boxes = E2E_BOXES = [[(0.3513, 0.4021, 0.4517, 0.5013), (0.7021, 0.6513, 0.4017, 0.4521)], [(0.5017, 0.5023, 0.6011, 0.5519), (0.3013, 0.7021, 0.3017, 0.3513), (0.7517, 0.3021, 0.3513, 0.4017)]]
    rows = [(b, k % E2E_NC, *bx) for b, bxs in enumerate(boxes) for k, bx in enumerate(bxs)]
    t = torch.tensor(rows, dtype=torch.float32)
    return {"img": img, "batch_idx": t[:, 0].clone(), "cls": t[:, 1:2].clone(), "bboxes": t[:, 2:6].clone(),
            "masks": ellipse_masks(boxes, (E2E_SIZE // 4, E2E_SIZE // 4)), "max_boxes": 3}
