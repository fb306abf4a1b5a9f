"""Numpy restatement, in the operation order include/ymi.h gives for ymi_augment_batch and ymi_augment_boxes, of the reference's training
augmentation at perspective = 0: Mosaic._mosaic4 (data/augment.py:658-714) with _update_labels / _cat_labels (:788-864), RandomPerspective
(:1017-1078, :1080-1112, :1185-1300), RandomHSV (:1346-1382), RandomFlip (:1433-1476), LetterBox._update_labels (:1605-1633) and Format's
normalisation (:2072-2074).

tests/test_augment_ref_cpu.py holds every function here to fixtures the REAL reference produced (tests/golden/make_augment_golden.py); the GPU
tests then compare the kernels with these functions on a machine that has no reference.

DISCLOSURE.  `warp_affine` and `bgr2hsv` / `hsv2bgr` state OpenCV's warpAffine INTER_LINEAR fixed-point scheme and its 8-bit BGR <-> HSV
conversion AS RECALLED; so does `invert_affine` (the order of operations in which warpAffine inverts the forward matrix), which the
product's ops.invert_affine copies: that order is pinned by nothing independent, only its result is checked (A composed with M is the identity to a
few ulp, tests/test_augment_ref_cpu.py).  OpenCV is not installed where this was written: they are NOT verified against OpenCV.  include/ymi.h's rule is the
contract, and the fixture script uses these very functions as its cv2 stand-ins - so the fixtures pin everything the reference DECIDES (placement,
matrix, every label step, every random draw, table building, stage order) and pin the interpolated and recoloured grey levels to the rule only.

`fault=` plants one mistake (the CPU test asserts that the fixtures notice each): "no_round16" the + 16 of the coordinate left out, "border0"
border level 0 for 114, "canvas_fill0" a materialised canvas whose uncovered part is 0 (taps do not resolve per source), "hsv_sat0" lut_sat[0]
not zeroed (INERT: 0 * (r + 1) is 0 before the assignment, whatever the gain - see the CPU test), "hsv_no_sat" the saturation table left out (a colour-stage fault a
fixture CAN notice), "flip_before_warp" the canvas flipped instead of the warped image, "no_candidates" box_candidates skipped, "area_thr_seg" the
segment threshold 0.01 for 0.10, "no_cat_clip" _cat_labels' clip and zero-area removal skipped."""
import math

import numpy as np

BORDER = 114
S = 64  # the side every case here trains at
SOURCES = [(37, 53), (64, 48), (64, 64), (50, 64)]  # (h, w) of the four images of the test data set


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def seeded_image(seed, h, w):
    """an (h, w, 3) uint8 image from numpy's frozen legacy stream: smooth blobs plus noise, so that hue, saturation and value all vary, with a
    white, a black and a grey patch (saturation 0: what lut_sat[0] = 0 is about)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 120 * np.sin(xx / rs.uniform(3, 9) + rs.uniform(0, 6)) * np.cos(yy / rs.uniform(3, 9) + c) for c in range(3)], -1)
    img = np.clip(img + rs.randint(-20, 21, size=(h, w, 3)), 0, 255).astype(np.uint8)
    img[2:8, 2:8] = 255
    img[h - 9 : h - 3, w - 9 : w - 3] = 0
    img[h // 2 - 3 : h // 2 + 3, w // 2 - 3 : w // 2 + 3] = 131
    return img


def seeded_labels(seed, n, centre=(0.1, 0.9), side=(0.06, 0.45)):
    """n rows (cls, x, y, w, h) normalised: centres over the whole image, sides from 6 % to 45 %"""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 5), dtype=np.float32)
    out[:, 0] = rs.randint(0, 3, n)
    out[:, 1:3] = rs.uniform(*centre, (n, 2))
    out[:, 3:5] = rs.uniform(*side, (n, 2))
    lo, hi = out[:, 1:3] - out[:, 3:5] / 2, out[:, 1:3] + out[:, 3:5] / 2  # (kept inside the image, as a label file's boxes are)
    lo, hi = np.clip(lo, 0, 1), np.clip(hi, 0, 1)
    out[:, 1:3], out[:, 3:5] = (lo + hi) / 2, hi - lo
    return out


def dataset(labels="normal"):
    """the four-image data set of the cases -> list of {"img", "labels" [n, 5]}.  labels: "normal" (5, 3, 4, 6 rows), "none", "tiny" (boxes
    of under 2 % of a side: every one fails box_candidates' w2 > 2) or "big" (three boxes with sides of 30 % to 90 % per image: zoomed in,
    the window keeps only a few per cent of some)"""
    out = []
    for i, (h, w) in enumerate(SOURCES):
        lab = seeded_labels(40 + i, (5, 3, 4, 6)[i]) if labels != "big" else seeded_labels(112 + i, 3, centre=(0.2, 0.8), side=(0.3, 0.9))
        if labels == "none":
            lab = lab[:0]
        elif labels == "tiny":
            lab[:, 3:5] = np.float32(0.015)
        out.append({"img": seeded_image(10 + i, h, w), "labels": lab})
    return out


# The hyper-parameters of v8_transforms the cases use (the reference's defaults, cfg/default.yaml) and what a case changes.
HYP = dict(mosaic=1.0, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.0, fliplr=0.5,
           mixup=0.0, copy_paste=0.0, copy_paste_mode="flip")
# Scripted cases: "unit" is the list of numbers in [0, 1] the random stream hands out in place of its draws (uniform(a, b) = a + (b - a) * u,
# random() = u, choices(population, k) = population[int(u * len)] per pick; np.random.uniform(-1, 1, 3) takes three), in v8_transforms' order:
#   mosaic test, 3 partners, yc, xc, | perspective x 2, angle, scale, shear x 2, translate x 2, | mixup test, | hsv x 3, | flipud, fliplr
def _unit(yc, xc, scale=0.5, angle=0.5, tx=0.5, ty=0.5, hsv=(0.2, 0.9, 0.7), ud=0.9, lr=0.9, partners=(0.3, 0.6, 0.9), shear=(0.5, 0.5)):
    return [0.5, *partners, yc, xc, 0.5, 0.5, angle, scale, *shear, tx, ty, 0.5, *hsv, ud, lr]


CASES = {
    # the mosaic centre at both extremes of [-border, 2s + border] = [32, 96]: at (32, 32) the top-left image is cropped to its last 32 x 32 and
    # lies outside the 64 x 64 window, at (96, 96) the bottom-right quadrant is outside
    "centre_lo": dict(index=0, unit=_unit(0.0, 0.0)),
    "centre_hi": dict(index=1, unit=_unit(1.0, 1.0, tx=0.1, ty=0.8)),
    "scale05": dict(index=2, unit=_unit(0.4, 0.7, scale=0.0, tx=0.0, ty=1.0)),
    "scale15": dict(index=3, unit=_unit(0.6, 0.3, scale=1.0, tx=1.0, ty=0.0)),
    "rot10": dict(index=0, unit=_unit(0.5, 0.5, angle=1.0, scale=0.7), hyp=dict(degrees=10.0)),
    "rot10_shear": dict(index=1, unit=_unit(0.3, 0.6, angle=0.0, scale=0.6, shear=(0.9, 0.2)), hyp=dict(degrees=10.0, shear=5.0)),
    "flip_none": dict(index=2, unit=_unit(0.45, 0.55, scale=0.3, tx=0.2, ty=0.9, ud=0.9, lr=0.9), hyp=dict(flipud=0.5)),
    "flip_lr": dict(index=2, unit=_unit(0.45, 0.55, scale=0.3, tx=0.2, ty=0.9, ud=0.9, lr=0.1), hyp=dict(flipud=0.5)),
    "flip_ud": dict(index=2, unit=_unit(0.45, 0.55, scale=0.3, tx=0.2, ty=0.9, ud=0.1, lr=0.9), hyp=dict(flipud=0.5)),
    "flip_both": dict(index=2, unit=_unit(0.45, 0.55, scale=0.3, tx=0.2, ty=0.9, ud=0.1, lr=0.1), hyp=dict(flipud=0.5)),
    "no_hsv": dict(index=3, unit=_unit(0.5, 0.4)[:15] + [0.9, 0.1], hyp=dict(hsv_h=0.0, hsv_s=0.0, hsv_v=0.0)),  # (no hsv draws)
    "no_labels": dict(index=0, unit=_unit(0.5, 0.5, scale=0.6), labels="none"),
    # zoomed in on big boxes: three rows keep between 1 % and 10 % of their area (box_candidates' area_thr is 0.10 for boxes, 0.01 for segments)
    "area_edge": dict(index=3, unit=_unit(0.6, 0.3, scale=1.0, tx=0.9, ty=0.2), labels="big"),
    "all_filtered": dict(index=1, unit=_unit(0.5, 0.5, scale=0.4), labels="tiny"),
    # mosaic = 0: the mosaic test fails (no partner, no centre draw) and RandomPerspective letterboxes the 37 x 53 image itself first
    "single": dict(index=0, unit=[0.5] + _unit(0, 0, scale=0.8, tx=0.3, ty=0.6, lr=0.1)[6:], hyp=dict(mosaic=0.0)),
    "single_rot": dict(index=3, unit=[0.5] + _unit(0, 0, scale=0.3, angle=0.9, tx=0.6, ty=0.4)[6:], hyp=dict(mosaic=0.0, degrees=10.0)),
}
SEEDS = (1, 2, 3)  # cases "seed<k>": the real random streams, random.seed(k) and np.random.seed(k), default hyper-parameters, image k % 4


def case_hyp(c):
    return {**HYP, **c.get("hyp", {})}


class ScriptedRandom:
    """stands in for the `random` module (and, through .np, for `np.random`): hands out the scripted unit numbers, records every call"""

    def __init__(self, unit):
        self.unit, self.calls = list(unit), []
        self.np = self

    def _next(self, what):
        assert self.unit, f"the script ran out at {what}"
        return self.unit.pop(0)

    def uniform(self, a, b, size=None):
        if size is not None:  # np.random.uniform(-1, 1, 3)
            v = np.array([a + (b - a) * self._next("np.uniform") for _ in range(size)], dtype=np.float64)
            self.calls.append(("np.uniform", [float(x) for x in v]))
            return v
        v = a + (b - a) * self._next("uniform")
        self.calls.append(("uniform", v))
        return v

    def random(self):
        v = self._next("random")
        self.calls.append(("random", v))
        return v

    def choices(self, population, k=1):
        v = [population[min(int(self._next("choices") * len(population)), len(population) - 1)] for _ in range(k)]
        self.calls.append(("choices", list(v)))
        return v


class RecordingRandom:
    """the real `random` / `np.random` streams, every call recorded with its result"""

    def __init__(self):
        import random

        self._r, self.calls, self.np = random, [], self

    def uniform(self, a, b, size=None):
        if size is not None:
            v = np.random.uniform(a, b, size)
            self.calls.append(("np.uniform", [float(x) for x in v]))
            return v
        v = self._r.uniform(a, b)
        self.calls.append(("uniform", v))
        return v

    def random(self):
        v = self._r.random()
        self.calls.append(("random", v))
        return v

    def choices(self, population, k=1):
        v = self._r.choices(population, k=k)
        self.calls.append(("choices", list(v)))
        return v


# ---------------------------------------------------------------------------------------------------------------- host geometry
def mosaic_placement(i, xc, yc, h, w, s):
    """_mosaic4's branch i -> (x1a, y1a, x2a, y2a, x1b, y1b)"""
    if i == 0:
        x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
        x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
    elif i == 1:
        x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
        x1b, y1b = 0, h - (y2a - y1a)
    elif i == 2:
        x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
        x1b, y1b = w - (x2a - x1a), 0
    else:
        x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
        x1b, y1b = 0, 0
    return x1a, y1a, x2a, y2a, x1b, y1b


def rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D by its documented formula, in double"""
    a = angle * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    return np.array([[alpha, beta, (1 - alpha) * center[0] - beta * center[1]], [-beta, alpha, beta * center[0] + (1 - alpha) * center[1]]], dtype=np.float64)


def invert_affine(M):
    """what warpAffine does to a forward 2 x 3 matrix before it maps destination to source: the inverse, in double -> 6 Python floats"""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(-1)[:6]]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11
    m[1] *= -D
    m[3] *= -D
    m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def hsv_luts(r, fault=None):
    """RandomHSV's three tables from its gains r (:1372-1377) -> uint8 [768]"""
    x = np.arange(0, 256, dtype=np.float64)
    lut_hue = ((x + r[0] * 180) % 180).astype(np.uint8)
    lut_sat = np.clip(x * (r[1] + 1), 0, 255).astype(np.uint8)
    lut_val = np.clip(x * (r[2] + 1), 0, 255).astype(np.uint8)
    if fault != "hsv_sat0":
        lut_sat[0] = 0
    return np.concatenate([lut_hue, lut_sat, lut_val])


# ---------------------------------------------------------------------------------------------------------------- the image rule
def _rn(x):
    return np.rint(x).astype(np.int64)  # round-half-even


def canvas_taps(sources, placements, canvas_hw, cy, cx, border, fault=None):
    """canvas pixel (cy, cx) for index arrays -> int64 [..., 3]: each tap resolved by itself (header: the first placement that holds it, else the border)"""
    ch, cw = canvas_hw
    out = np.full(cy.shape + (3,), border, dtype=np.int64)
    inside = (cy >= 0) & (cy < ch) & (cx >= 0) & (cx < cw)
    if fault == "canvas_fill0":
        out[inside] = 0
    found = np.zeros(cy.shape, dtype=bool)
    for img, (x1a, y1a, x2a, y2a, x1b, y1b) in zip(sources, placements):
        m = inside & ~found & (cx >= x1a) & (cx < x2a) & (cy >= y1a) & (cy < y2a)
        out[m] = img[cy[m] - y1a + y1b, cx[m] - x1a + x1b]
        found |= m
    return out


def warp_affine(sources, placements, canvas_hw, A, size, border=BORDER, fault=None, flip=(False, False)):
    """header steps 1-2 -> uint8 [size, size, 3] BGR.  A: the inverse matrix, 6 doubles.  flip = (ud, lr) of the output."""
    if fault == "border0":
        border = 0
    ys, xs = np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64)
    if flip[0] and fault != "flip_before_warp":
        ys = size - 1 - ys
    if flip[1] and fault != "flip_before_warp":
        xs = size - 1 - xs
    if fault == "flip_before_warp" and (flip[0] or flip[1]):  # the canvas is flipped, then warped
        ch, cw = canvas_hw
        sources = [s[::-1] if flip[0] else s for s in sources]
        sources = [s[:, ::-1] if flip[1] else s for s in sources]
        fp = []
        for s, (x1a, y1a, x2a, y2a, x1b, y1b) in zip(sources, placements):
            h, w = s.shape[:2]
            if flip[0]:
                y1a, y2a, y1b = ch - y2a, ch - y1a, h - (y1b + (y2a - y1a))
            if flip[1]:
                x1a, x2a, x1b = cw - x2a, cw - x1a, w - (x1b + (x2a - x1a))
            fp.append((x1a, y1a, x2a, y2a, x1b, y1b))
        placements = fp
    r16 = 0 if fault == "no_round16" else 16
    X = (_rn(A[0] * xs * 1024.0)[None, :] + _rn((A[1] * ys + A[2]) * 1024.0)[:, None] + r16) >> 5
    Y = (_rn(A[3] * xs * 1024.0)[None, :] + _rn((A[4] * ys + A[5]) * 1024.0)[:, None] + r16) >> 5
    sx, fx, sy, fy = X >> 5, (X & 31)[..., None], Y >> 5, (Y & 31)[..., None]
    tap = lambda dy, dx: canvas_taps(sources, placements, canvas_hw, sy + dy, sx + dx, border, fault)  # noqa: E731
    out = ((32 - fx) * (32 - fy) * tap(0, 0) + fx * (32 - fy) * tap(0, 1) + (32 - fx) * fy * tap(1, 0) + fx * fy * tap(1, 1) + 512) >> 10
    return out.astype(np.uint8)


_IDX = np.arange(256, dtype=np.float64)
with np.errstate(divide="ignore"):
    SDIV = np.where(_IDX > 0, np.rint((255 << 12) / _IDX), 0).astype(np.int64)
    HDIV = np.where(_IDX > 0, np.rint((180 << 12) / (6.0 * _IDX)), 0).astype(np.int64)


def bgr2hsv(img):
    """header step 3, forward -> uint8 [..., 3] (h in [0, 180), s, v)"""
    b, g, r = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(b, np.maximum(g, r))
    d = v - np.minimum(b, np.minimum(g, r))
    s = (d * SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * HDIV[d] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], -1).astype(np.uint8)


def hsv2bgr(hsv):
    """header step 3, backward, float32 with every operation rounded on its own -> uint8 [..., 3]"""
    f = np.float32
    h8, s8, v8 = (hsv[..., c] for c in range(3))
    H = h8.astype(f) * (f(6) / f(180))
    Sx = s8.astype(f) * (f(1) / f(255))
    V = v8.astype(f) * (f(1) / f(255))
    k = np.floor(H).astype(np.int64)
    fr = H - k.astype(f)
    bad = (k < 0) | (k >= 6)
    k, fr = np.where(bad, 0, k), np.where(bad, f(0), fr).astype(f)
    one = f(1)
    t = [V, V * (one - Sx), V * (one - Sx * fr), V * (one - Sx * (one - fr))]
    sector = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    tabs = np.stack(t, -1)
    out = np.take_along_axis(tabs, sector[k], -1)
    out = np.where((s8 == 0)[..., None], V[..., None], out).astype(f)
    return np.clip(np.rint(out * f(255)), 0, 255).astype(np.uint8)


def apply_hsv(img, lut, fault=None):
    hsv = bgr2hsv(img)
    sat = hsv[..., 1] if fault == "hsv_no_sat" else lut[256 + hsv[..., 1].astype(np.int64)]
    return hsv2bgr(np.stack([lut[hsv[..., 0]], sat, lut[512 + hsv[..., 2].astype(np.int64)]], -1))


def to_batch_image(u8, bgr=True, normalize=True):
    """header step 4: BGR HWC uint8 -> float32 [3, s, s]"""
    x = u8[..., ::-1] if bgr else u8
    x = np.ascontiguousarray(x.transpose(2, 0, 1)).astype(np.float32)
    return x / np.float32(255) if normalize else x


def augment_image_u8(g, border=BORDER, fault=None):
    """one table row g (see `geometry`) -> uint8 [s, s, 3] BGR after warp, colour and flips"""
    out = warp_affine(g["sources"], g["placements"], g["canvas_hw"], g["A"], g["size"], border, fault, (g["flip_ud"], g["flip_lr"]))
    if g["hsv"] is not None:
        out = apply_hsv(out, hsv_luts(g["hsv"], fault), fault)
    return out


# ---------------------------------------------------------------------------------------------------------------- the label rule
def augment_labels(rows, images, area_thr=0.10, fault=None):
    """header steps 1-7 of ymi_augment_boxes.  rows float32 [n, 7]; images: list of dicts with the fields of ymi_augment_label_image
    -> (keep bool [n], out float32 [n, 6] = (image, cls, xywh normalised), margins: per row the distance of every decision to its threshold)"""
    f = np.float32
    n = len(rows)
    keep, out, margins = np.zeros(n, dtype=bool), np.zeros((n, 6), dtype=f), [None] * n
    if fault == "area_thr_seg":
        area_thr = 0.01
    area_thr = f(area_thr)
    for i in range(n):
        b, k = int(rows[i, 0]), int(rows[i, 1])
        m = images[b]
        if not (m["row_start"] <= i < m["row_end"]):
            continue
        x, y, w, h = (f(v) for v in rows[i, 3:7])
        hw, hh = w / f(2), h / f(2)
        box = [x - hw, y - hh, x + hw, y + hh]
        sw, sh, rw, rh, pw, ph = (f(m[key][k]) for key in ("src_w", "src_h", "ratio_w", "ratio_h", "padw", "padh"))
        box = [box[0] * sw * rw + pw, box[1] * sh * rh + ph, box[2] * sw * rw + pw, box[3] * sh * rh + ph]
        mg = {}
        if m["canvas"] > 0 and fault != "no_cat_clip":
            c = f(m["canvas"])
            mg["cat_clip"] = min(min(abs(v), abs(v - c)) for v in box)
            box = [min(max(v, f(0)), c) for v in box]
            area = (box[2] - box[0]) * (box[3] - box[1])
            mg["cat_area"] = float(area)
            if not area > 0:
                margins[i] = mg
                continue
        x1, y1, x2, y2 = box
        M = [f(v) for v in m["M"]]
        X = [M[0] * cx + M[1] * cy + M[2] for cx, cy in ((x1, y1), (x2, y2), (x1, y2), (x2, y1))]
        Y = [M[3] * cx + M[4] * cy + M[5] for cx, cy in ((x1, y1), (x2, y2), (x1, y2), (x2, y1))]
        new = [min(X), min(Y), max(X), max(Y)]
        size_w, size_h = f(m["size_w"]), f(m["size_h"])
        mg["clip"] = min(min(abs(new[0]), abs(new[0] - size_w)), min(abs(new[2]), abs(new[2] - size_w)), min(abs(new[1]), abs(new[1] - size_h)),
                         min(abs(new[3]), abs(new[3] - size_h)))
        new = [min(max(new[0], f(0)), size_w), min(max(new[1], f(0)), size_h), min(max(new[2], f(0)), size_w), min(max(new[3], f(0)), size_h)]
        s, eps = f(m["scale"]), f(1e-16)
        w1, h1 = x2 * s - x1 * s, y2 * s - y1 * s
        w2, h2 = new[2] - new[0], new[3] - new[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            ar = max(w2 / (h2 + eps), h2 / (w2 + eps))
            ratio = w2 * h2 / (w1 * h1 + eps)
        mg.update(w2=float(w2), h2=float(h2), ratio=float(ratio), ar=float(ar), w1h1=float(w1 * h1))
        margins[i] = mg
        ok = (w2 > 2) and (h2 > 2) and (ratio > area_thr) and (ar < 100)
        if not ok and fault != "no_candidates":
            continue
        cx, cy = (new[0] + new[2]) / f(2), (new[1] + new[3]) / f(2)
        if m["flip_ud"]:
            cy = size_h - cy
        if m["flip_lr"]:
            cx = size_w - cx
        keep[i] = True
        out[i] = (f(b), rows[i, 2], cx / size_w, cy / size_h, w2 / size_w, h2 / size_h)
    return keep, out, margins


def decisions_clear(margins, margin_px=1e-3, area_thr=0.10):
    """-> list of (row, what) whose box_candidates quantities or clip decisions lie within the GPU tests' coordinate tolerance of a threshold.
    w2, h2 against 2 and the clips are distances in pixels; the area ratio moves by at most (w2 + h2) * margin / (w1 * h1), the aspect ratio by
    ar * margin * (1 / w2 + 1 / h2)."""
    bad = []
    for i, mg in enumerate(margins):
        if mg is None:
            continue
        if "cat_clip" in mg and 0 < mg["cat_clip"] < margin_px:
            bad.append((i, "cat_clip"))
        if "cat_area" in mg and 0 < mg["cat_area"] < margin_px * 256:
            bad.append((i, "cat_area"))
        if "w2" not in mg:
            continue
        if 0 < mg["clip"] < margin_px:
            bad.append((i, "clip"))
        if abs(mg["w2"] - 2) < 2 * margin_px or abs(mg["h2"] - 2) < 2 * margin_px:
            bad.append((i, "wh_thr"))
        if mg["w1h1"] > 0 and abs(mg["ratio"] - area_thr) < 2 * margin_px * (mg["w2"] + mg["h2"] + 1) / mg["w1h1"] + 1e-6:
            bad.append((i, "area_thr"))
        if mg["w2"] > 0 and mg["h2"] > 0 and abs(mg["ar"] - 100) < 2 * margin_px * mg["ar"] * (1 / mg["w2"] + 1 / mg["h2"]) + 1e-4:
            bad.append((i, "ar_thr"))
    return bad


def compact(keep, out):
    """-> (batch_idx [m], cls [m, 1], bboxes [m, 4]) of the kept rows in their order"""
    k = out[keep]
    return k[:, 0].copy(), k[:, 1:2].copy(), k[:, 2:6].copy()


# ---------------------------------------------------------------------------------------------------------------- a sample's geometry
def affine_forward(canvas_hw, border, draws, hyp):
    """RandomPerspective.affine_transform's matrix (:1042-1071) from its draws -> (M float32 [3, 3], (w, h) of the output, s)"""
    size = canvas_hw[1] + border[1] * 2, canvas_hw[0] + border[0] * 2
    C = np.eye(3, dtype=np.float32)
    C[0, 2] = -canvas_hw[1] / 2
    C[1, 2] = -canvas_hw[0] / 2
    P = np.eye(3, dtype=np.float32)
    P[2, 0], P[2, 1] = draws["perspective"]
    R = np.eye(3, dtype=np.float32)
    R[:2] = rotation_matrix_2d((0, 0), draws["angle"], draws["scale"])
    Sh = np.eye(3, dtype=np.float32)
    Sh[0, 1] = math.tan(draws["shear"][0] * math.pi / 180)
    Sh[1, 0] = math.tan(draws["shear"][1] * math.pi / 180)
    T = np.eye(3, dtype=np.float32)
    T[0, 2] = draws["translate"][0] * size[0]
    T[1, 2] = draws["translate"][1] * size[1]
    return T @ Sh @ R @ P @ C, size, draws["scale"]


def geometry(data, index, params, s=S):
    """what one sample becomes -> the table row as a dict (image side and label side) plus its label rows [n, 6] = (slot, cls, xywh).
    params: {"mosaic": None | {"indexes", "yc", "xc"}, "affine": draws, "hsv": None | gains, "flipud", "fliplr"} - what data.augment draws."""
    import letterbox_ref as LR
    import torch

    mos = params["mosaic"]
    lab = dict(src_w=[1] * 4, src_h=[1] * 4, ratio_w=[1] * 4, ratio_h=[1] * 4, padw=[0] * 4, padh=[0] * 4)
    if mos is not None:
        members = [data[index]] + [data[j] for j in mos["indexes"]]
        sources = [m["img"] for m in members]
        placements = [mosaic_placement(i, mos["xc"], mos["yc"], im.shape[0], im.shape[1], s) for i, im in enumerate(sources)]
        canvas_hw, border = (2 * s, 2 * s), (-s // 2, -s // 2)
        for i, (im, p) in enumerate(zip(sources, placements)):
            lab["src_w"][i], lab["src_h"][i], lab["padw"][i], lab["padh"][i] = im.shape[1], im.shape[0], p[0] - p[4], p[1] - p[5]
        rows = [np.concatenate([np.full((len(m["labels"]), 1), i, dtype=np.float32), m["labels"]], 1) for i, m in enumerate(members)]
        canvas = 2 * s
    else:  # RandomPerspective's pre_transform: LetterBox(new_shape=(s, s)) of the image itself, then the warp with border (0, 0)
        im = data[index]["img"]
        boxed, rp = LR.letterbox_u8(torch.from_numpy(im), (s, s))
        boxed = boxed.numpy()
        sources, placements, canvas_hw, border = [boxed], [(0, 0, boxed.shape[1], boxed.shape[0], 0, 0)], boxed.shape[:2], (0, 0)
        (r_h, r_w), (left, top) = rp
        lab["src_w"][0], lab["src_h"][0], lab["ratio_w"][0], lab["ratio_h"][0], lab["padw"][0], lab["padh"][0] = im.shape[1], im.shape[0], r_w, r_h, left, top
        rows = [np.concatenate([np.zeros((len(data[index]["labels"]), 1), dtype=np.float32), data[index]["labels"]], 1)]
        canvas = 0
    M, size, scale = affine_forward(canvas_hw, border, params["affine"], None)
    assert size == (s, s)
    lab.update(M=[float(v) for v in M[:2].reshape(-1)], scale=scale, size_w=size[0], size_h=size[1], canvas=canvas, flip_ud=bool(params["flipud"]),
               flip_lr=bool(params["fliplr"]))
    return dict(sources=sources, placements=placements, canvas_hw=canvas_hw, A=invert_affine(M[:2]), M=M, size=s, hsv=params["hsv"],
                flip_ud=bool(params["flipud"]), flip_lr=bool(params["fliplr"]), label=lab, rows=np.concatenate(rows, 0).astype(np.float32))


def batch_rows(geos):
    """the label side of a batch -> (rows float32 [n, 7], images: the per-image dicts with row_start / row_end)"""
    rows, images, at = [], [], 0
    for b, g in enumerate(geos):
        r = g["rows"]
        rows.append(np.concatenate([np.full((len(r), 1), b, dtype=np.float32), r], 1))
        images.append({**g["label"], "row_start": at, "row_end": at + len(r)})
        at += len(r)
    return (np.concatenate(rows, 0) if rows else np.zeros((0, 7), np.float32)).astype(np.float32), images


def augment_batch(geos, bgr=True, normalize=True, fault=None):
    """what ops.augment_batch computes -> (img float32 [B, 3, s, s], batch_idx, cls, bboxes, count [B], keep)"""
    img = np.stack([to_batch_image(augment_image_u8(g, fault=fault), bgr, normalize) for g in geos])
    rows, images = batch_rows(geos)
    keep, out, _ = augment_labels(rows, images, fault=fault)
    bi, cls, bb = compact(keep, out)
    count = np.array([int(keep[m["row_start"] : m["row_end"]].sum()) for m in images], dtype=np.int32)
    return img, bi, cls, bb, count, keep


def params_from_calls(values, hyp):
    """the draws of one v8_transforms call, in its order, as the parameter dict: values is the flat list of what the stream handed out
    (uniform / random: the value; choices: the list; np.uniform: the list of three BEFORE the multiplication by the gains)"""
    v = list(values)
    mosaic = None
    if not v.pop(0) > hyp["mosaic"]:
        idx = v.pop(0)
        mosaic = {"indexes": [int(j) for j in idx], "yc": int(v.pop(0)), "xc": int(v.pop(0))}
    affine = {"perspective": (v.pop(0), v.pop(0)), "angle": v.pop(0), "scale": v.pop(0)}
    affine["shear"] = (v.pop(0), v.pop(0))
    affine["translate"] = (v.pop(0), v.pop(0))
    v.pop(0)  # MixUp's test
    hsv = None
    if hyp["hsv_h"] or hyp["hsv_s"] or hyp["hsv_v"]:
        hsv = [float(x) for x in np.asarray(v.pop(0)) * [hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"]]]
    flipud = v.pop(0) < hyp["flipud"]
    fliplr = v.pop(0) < hyp["fliplr"]
    assert not v
    return {"mosaic": mosaic, "affine": affine, "hsv": hsv, "flipud": bool(flipud), "fliplr": bool(fliplr)}
