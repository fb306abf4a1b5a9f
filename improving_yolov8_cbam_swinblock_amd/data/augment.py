"""The reference's augmentation classes by name and constructor (ultralytics/data/augment.py): LetterBox (:1479-1603) on ops.letterbox
(csrc/resize.hip), and Mosaic, RandomPerspective, RandomHSV, RandomFlip and v8_transforms as the parameter source of ops.augment_batch
(csrc/augment.hip)."""
import random

import numpy as np

from .. import ops


class LetterBox:
    """LetterBox(new_shape, auto, scale_fill, scaleup, center, stride)(image=img) -> the letterboxed image [h', w', 3] float32 on the device,
    grey levels 0..255 in the image's own channel order (what the reference returns as a uint8 array, before the predictor's conversion;
    ops.letterbox does both in one launch for a list).  The `labels` form updates a dataset's Instances, which this package has not."""

    def __init__(self, new_shape=(640, 640), auto=False, scale_fill=False, scaleup=True, center=True, stride=32):
        self.new_shape = new_shape
        self.auto = auto
        self.scale_fill = scale_fill
        self.scaleup = scaleup
        self.stride = stride
        self.center = center  # Put the image in the middle or top-left

    def __call__(self, labels=None, image=None):
        if labels is not None or image is None:
            raise NotImplementedError("LetterBox: the labels form needs the dataset's Instances, which are not built; call it with image=...")
        out, _ = ops.letterbox([image], self.new_shape, auto=self.auto, scale_fill=self.scale_fill, scaleup=self.scaleup, center=self.center,
                               stride=self.stride, bgr=False, normalize=False)
        return out[0].permute(1, 2, 0)


# ---------------------------------------------------------------------------------------------------------------- training augmentation
# The reference's training transforms (ultralytics/data/augment.py) with their names, constructor arguments and defaults.  Here they DRAW
# PARAMETERS only: the pixel and label work is ops.augment_batch's (csrc/augment.hip), one launch for the batch.  Each consumes `random` and
# `np.random` in exactly the reference's order, so the same seeds give the same parameters as the reference's pipeline would use.


class Mosaic:
    """Mosaic(dataset, imgsz, p, n)() -> None when the test `random.uniform(0, 1) > p` says no mosaic (drawn BEFORE p is looked at, as
    BaseMixTransform.__call__ :386 does), else {"indexes": the three partners, "yc", "xc": the centre} (:545-568, :684).
    dataset: anything with `buffer` (the indexes partners are picked from) and `__len__`."""

    def __init__(self, dataset, imgsz=640, p=1.0, n=4):
        assert 0 <= p <= 1.0, f"The probability should be in range [0, 1], but got {p}."
        assert n in {4, 9}, "grid must be equal to 4 or 9."
        if n == 9:
            raise NotImplementedError("Mosaic-9 needs _mosaic9's placement (reference data/augment.py:716-786)")
        self.dataset = dataset
        self.p = p
        self.imgsz = imgsz
        self.border = (-imgsz // 2, -imgsz // 2)  # width, height
        self.n = n

    def get_indexes(self, buffer=True):
        if buffer:  # select images from buffer
            return random.choices(list(self.dataset.buffer), k=self.n - 1)
        else:  # select any images
            return [random.randint(0, len(self.dataset) - 1) for _ in range(self.n - 1)]

    def __call__(self, pick_partners=True):
        if random.uniform(0, 1) > self.p:
            return None
        indexes = self.get_indexes() if pick_partners else None
        s = self.imgsz
        yc, xc = (int(random.uniform(-x, 2 * s + x)) for x in self.border)  # mosaic center x, y
        return {"indexes": indexes, "yc": yc, "xc": xc}


class RandomPerspective:
    """RandomPerspective(degrees, translate, scale, shear, perspective, border, pre_transform)() -> the eight draws of affine_transform
    (:1049-1068) in its order, as ops.affine_matrix takes them."""

    def __init__(self, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, border=(0, 0), pre_transform=None):
        if perspective:
            raise NotImplementedError("perspective != 0 needs cv2.warpPerspective and the perspective division (reference data/augment.py:1075, :1107)")
        self.degrees = degrees
        self.translate = translate
        self.scale = scale
        self.shear = shear
        self.perspective = perspective
        self.border = border  # mosaic border
        self.pre_transform = pre_transform

    def __call__(self):
        p = (random.uniform(-self.perspective, self.perspective), random.uniform(-self.perspective, self.perspective))
        a = random.uniform(-self.degrees, self.degrees)
        s = random.uniform(1 - self.scale, 1 + self.scale)
        shear = (random.uniform(-self.shear, self.shear), random.uniform(-self.shear, self.shear))
        translate = (random.uniform(0.5 - self.translate, 0.5 + self.translate), random.uniform(0.5 - self.translate, 0.5 + self.translate))
        return {"perspective": p, "angle": a, "scale": s, "shear": shear, "translate": translate}


class RandomHSV:
    """RandomHSV(hgain, sgain, vgain)() -> the three gains r (:1371), or None - without a draw - when all three are 0 (:1367)"""

    def __init__(self, hgain=0.5, sgain=0.5, vgain=0.5):
        self.hgain = hgain
        self.sgain = sgain
        self.vgain = vgain

    def __call__(self):
        if self.hgain or self.sgain or self.vgain:
            r = np.random.uniform(-1, 1, 3) * [self.hgain, self.sgain, self.vgain]  # random gains
            return [float(v) for v in r]
        return None


class RandomFlip:
    """RandomFlip(p, direction, flip_idx)() -> whether to flip.  A flip draws `random.random()` whatever p is - a vertical flip at p = 0 too
    (:1465, :1468)."""

    def __init__(self, p=0.5, direction="horizontal", flip_idx=None):
        assert direction in {"horizontal", "vertical"}, f"Support direction `horizontal` or `vertical`, got {direction}"
        assert 0 <= p <= 1.0, f"The probability should be in range [0, 1], but got {p}."
        if flip_idx is not None and len(flip_idx):
            raise NotImplementedError("keypoints need the flip_idx permutation (reference data/augment.py:1472-1473)")
        self.p = p
        self.direction = direction
        self.flip_idx = flip_idx

    def __call__(self):
        return random.random() < self.p


class V8Transforms:
    """what v8_transforms' Compose draws for one sample, in its order (:2399-2439): Mosaic [test, partners, centre], RandomPerspective [8],
    MixUp's test (:386, drawn although mixup = 0), Albumentations (no draw without that package), RandomHSV [3], RandomFlip vertical [1],
    RandomFlip horizontal [1].  Format's channel-order draw (:2107) belongs to the data set, not to this Compose, and is not drawn.
    () -> the parameter dict ops.augment_batch takes."""

    def __init__(self, mosaic, affine, mixup, hsv, flipud, fliplr):
        self.mosaic, self.affine, self.mixup, self.hsv, self.flipud, self.fliplr = mosaic, affine, mixup, hsv, flipud, fliplr

    def __call__(self, pick_partners=True):
        mosaic = self.mosaic(pick_partners)
        affine = self.affine()
        if not random.uniform(0, 1) > self.mixup:
            raise NotImplementedError("MixUp needs a second augmented sample and the blend (reference data/augment.py:867-949)")
        hsv = self.hsv()
        flipud = self.flipud()
        fliplr = self.fliplr()
        return {"mosaic": mosaic, "affine": affine, "hsv": hsv, "flipud": flipud, "fliplr": fliplr}


V8_DEFAULTS = dict(mosaic=1.0, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, flipud=0.0,
                   fliplr=0.5, mixup=0.0, copy_paste=0.0)  # the reference's cfg/default.yaml


def v8_transforms(dataset, imgsz, hyp=None, stretch=False):
    """v8_transforms (reference data/augment.py:2375-2439) as a parameter source.  hyp: a mapping or namespace with the reference's names;
    what it leaves out takes the reference's default."""
    get = (lambda k: hyp.get(k, V8_DEFAULTS[k])) if isinstance(hyp, dict) else (lambda k: getattr(hyp, k, V8_DEFAULTS[k]))
    if stretch:
        raise NotImplementedError("stretch=True warps the image without the LetterBox pre_transform (reference data/augment.py:2406)")
    if get("copy_paste"):
        raise NotImplementedError("CopyPaste works on segments (reference data/augment.py:1676-1734)")
    if getattr(dataset, "use_keypoints", False) or getattr(dataset, "use_segments", False):
        raise NotImplementedError("segments and keypoints need apply_segments / apply_keypoints (reference data/augment.py:1114-1183)")
    mosaic = Mosaic(dataset, imgsz=imgsz, p=get("mosaic"))
    affine = RandomPerspective(degrees=get("degrees"), translate=get("translate"), scale=get("scale"), shear=get("shear"), perspective=get("perspective"),
                               pre_transform=LetterBox(new_shape=(imgsz, imgsz)))
    return V8Transforms(mosaic, affine, get("mixup"), RandomHSV(hgain=get("hsv_h"), sgain=get("hsv_s"), vgain=get("hsv_v")),
                        RandomFlip(direction="vertical", p=get("flipud")), RandomFlip(direction="horizontal", p=get("fliplr")))
