"""What tests/golden/make_obb_golden.py and the oriented-box tests share: the head and loss cases, their seeds and their batches.  Weights and
inputs are rebuilt from seeds on both sides (tests/golden_weights.py); the fixtures store only what the reference produced."""
import math

import numpy as np
import torch

from golden_weights import seeded_array, seeded_inputs
from psa_common import seeded_module_state

NC, NE, CH, STRIDE = 3, 1, (32, 64, 128), (8.0, 16.0, 32.0)  # OBB(3, 1, (32, 64, 128)) with strides 8, 16, 32
HEAD_SEED, LOSS_SEED, E2E_SEED = 5100, 5200, 51
SCALES = ("n", "s", "m")
E2E_NC, E2E_BATCH, E2E_SIZE = 3, 2, 128
E2E_MODELS = {"obb_e2e_v8n": "yolov8n-obb.yaml", "obb_e2e_11n": "yolo11n-obb.yaml"}
HYP = dict(box=7.5, cls=0.5, dfl=1.5)
PI = math.pi

_L3 = ((8, 8), (4, 4), (2, 2))
# name: levels (h, w), strides, nc, rows (image, class, cx, cy, w, h normalised, angle); image size = level 0 * stride 0.  No edge of a box runs
# through an anchor centre (coordinates off every grid), so the inside test is decided well away from a tie.
LOSS_CASES = {
    # 64 x 64, A = 84.  Image 0: angles -pi/4, 0 and pi/2, width and height unequal, a class at nc - 1; image 1 has no labels (only padding rows)
    "obb_loss_square": dict(levels=_L3, strides=STRIDE, nc=3, B=2, rows=[
        (0, 0, 0.3513, 0.4021, 0.5017, 0.2513, -PI / 4), (0, 2, 0.6521, 0.6013, 0.3011, 0.5519, 0.0), (0, 1, 0.5017, 0.4523, 0.6021, 0.2017, PI / 2)]),
    # 96 (h) x 64 (w): 12 x 8, 6 x 4, 3 x 2.  Image 0 opens with the tiny-filter rows: width 0.0205 * 96 = 1.968 < 2 is dropped, 0.0215 * 96 =
    # 2.064 stays although 0.0215 * 64 = 1.376 < 2 (scaled by the image WIDTH it would go, and every later gt index of the image would shift);
    # then an angle just below 3 pi / 4.  Image 1 has two labels, so its last slots are padding rows.  Its second box, at angle 0 with x in
    # [4, 20] and y in [0, 24] pixels, has edges that run EXACTLY through anchor centres (x = 4 and 20 on level 0, y = 24 on level 1; every
    # product is exact in float32 and float64 alike): those centres are inside (>=), and with fewer strictly inside than topk they are picked.
    "obb_loss_rect": dict(levels=((12, 8), (6, 4), (3, 2)), strides=STRIDE, nc=3, B=2, rows=[
        (0, 1, 0.5013, 0.5021, 0.0205, 0.4017, 0.2), (0, 2, 0.4519, 0.4013, 0.0215, 0.5021, 0.1), (0, 0, 0.5521, 0.5517, 0.6013, 0.3019, 3 * PI / 4 - 1e-3),
        (0, 2, 0.4017, 0.3021, 0.4513, 0.2517, 0.7), (1, 2, 0.5019, 0.6013, 0.5517, 0.4021, 1.1), (1, 0, 0.1875, 0.125, 0.25, 0.25, 0.0)]),
    # LOSS_MAXL levels; a square box: the covariance is isotropic and c = 0 whatever the angle
    "obb_loss_four": dict(levels=((8, 16), (4, 8), (2, 4), (1, 2)), strides=(8.0, 16.0, 32.0, 64.0), nc=1, B=1, rows=[
        (0, 0, 0.4013, 0.4521, 0.3017, 0.6034, 0.9), (0, 0, 0.7019, 0.5513, 0.2517, 0.5034, 0.4)]),
    "obb_loss_nolabels": dict(levels=_L3, strides=STRIDE, nc=3, B=2, rows=[]),
    # crowded: six overlapping boxes around the centre, anchors claimed by several; a 11 x 9 pixel box that holds fewer centres than topk
    "obb_loss_crowded": dict(levels=_L3, strides=STRIDE, nc=3, B=1, rows=[
        (0, 0, 0.5013, 0.5021, 0.5517, 0.3513, 0.3), (0, 1, 0.4521, 0.5513, 0.4519, 0.4017, -0.5), (0, 2, 0.5517, 0.4519, 0.3521, 0.5013, 1.3),
        (0, 0, 0.4817, 0.4713, 0.6019, 0.2521, 2.0), (0, 1, 0.5321, 0.5217, 0.3013, 0.3013, 0.8), (0, 2, 0.5119, 0.4917, 0.4013, 0.4517, PI / 2),
        (0, 1, 0.2013, 0.8021, 0.1719, 0.1407, 0.6)]),
}


def level_hw(img_hw):
    h, w = img_hw
    return [(-(-h // s), -(-w // s)) for s in (8, 16, 32)]


def loss_case(name):
    """-> dict of a loss case, float32 on the CPU: feats [B, 64 + nc, h, w] per level, angle [B, 1, A] in (-pi/4, 3pi/4), the batch, and the
    case's facts (levels, strides, nc, B, G, A, image size)."""
    c = LOSS_CASES[name]
    rs = np.random.RandomState(LOSS_SEED + 10 * list(LOSS_CASES).index(name))
    B, nc = c["B"], c["nc"]
    feats = [torch.from_numpy(seeded_array(rs, (B, 64 + nc, h, w))) * 2 for h, w in c["levels"]]
    A = sum(h * w for h, w in c["levels"])
    angle = (torch.sigmoid(torch.from_numpy(seeded_array(rs, (B, 1, A))) * 2) - 0.25) * PI
    t = torch.tensor(c["rows"], dtype=torch.float32).reshape(-1, 7)
    counts = [int((t[:, 0] == b).sum()) for b in range(B)]
    (h0, w0), s0 = c["levels"][0], c["strides"][0]
    batch = {"batch_idx": t[:, 0].clone(), "cls": t[:, 1:2].clone(), "bboxes": t[:, 2:7].clone(), "max_boxes": max(counts + [1])}
    return dict(name=name, feats=feats, angle=angle.float().contiguous(), batch=batch, levels=c["levels"], strides=c["strides"], nc=nc, B=B, A=A,
                G=batch["max_boxes"], img_h=h0 * s0, img_w=w0 * s0)


def head_inputs():
    """([x per level], [gy of the train maps per level], gy of the angle) of the OBB head case: two 96 x 96 images, maps 12, 6, 3."""
    xs, gys = [], []
    for i, (c, (h, w)) in enumerate(zip(CH, level_hw((96, 96)))):
        x, gy = seeded_inputs(HEAD_SEED + 10 * i, (2, c, h, w), (2, 64 + NC, h, w))
        xs.append(x)
        gys.append(gy)
    A = sum(h * w for h, w in level_hw((96, 96)))
    _, ga = seeded_inputs(HEAD_SEED + 50, (1,), (2, NE, A))
    return xs, gys, ga


def e2e_state(model):
    return seeded_module_state(model, E2E_SEED)


E2E_ROWS = [(0, 0, 0.3513, 0.4021, 0.4517, 0.3013, 0.4), (0, 1, 0.7021, 0.6513, 0.4017, 0.2521, -0.6), (1, 2, 0.5017, 0.5023, 0.6011, 0.3519, 1.2),
            (1, 0, 0.3013, 0.7021, 0.3017, 0.2513, 2.1), (1, 1, 0.7517, 0.3021, 0.2513, 0.4017, 0.0)]


def e2e_batch():
    img, _ = seeded_inputs(E2E_SEED, (E2E_BATCH, 3, E2E_SIZE, E2E_SIZE), (1,))
    img = (img * 0.25 + 0.5).clamp(0, 1)
    t = torch.tensor(E2E_ROWS, dtype=torch.float32)
    return {"img": img, "batch_idx": t[:, 0].clone(), "cls": t[:, 1:2].clone(), "bboxes": t[:, 2:7].clone(), "max_boxes": 3}
