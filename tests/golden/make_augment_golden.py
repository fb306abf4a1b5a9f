"""Generate the training-augmentation fixtures under tests/golden/ by running the REAL reference on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/make_augment_golden.py

Same import shim as make_predict_golden.py (cv2 stubbed, the torchvision version patched, YOLO_OFFLINE).  What runs is the reference's own
v8_transforms Compose (data/augment.py:2375-2439) on a four-image data set: Mosaic.__call__ / get_indexes / _mosaic4 / _update_labels /
_cat_labels, RandomPerspective.__call__ with affine_transform, apply_bboxes and box_candidates (and its LetterBox pre_transform when the mosaic
test fails), MixUp's and Albumentations' tests, RandomHSV, both RandomFlips, then Format (:2013-2078) for the normalised labels.  So the mosaic
placement, the matrix, every label step, the table building and every random draw are the reference's own code.

DISCLOSURE: OpenCV is not installed here, so the cv2 calls are supplied by this file - OUR code, not the reference's and not OpenCV's:
`warpAffine` (the fixed-point INTER_LINEAR rule include/ymi.h writes out for ymi_augment_batch, from tests/augment_ref.py), `cvtColor` for
COLOR_BGR2HSV / COLOR_HSV2BGR (the header's integer forward and float32 backward rule, likewise), `split` / `merge` / `LUT` (plain indexing),
`getRotationMatrix2D` (its documented formula), and `resize` / `copyMakeBorder` as in make_predict_golden.py.  The warp rule and the colour round
trip are OpenCV's schemes AS RECALLED and are NOT verified against OpenCV: interpolated and recoloured grey levels are pinned to the stated rule
only; no fixture here can say anything about OpenCV itself.  albumentations is not installed either: Albumentations(p=1.0) finds no transform
and draws nothing, as in any installation without that package.

Cases are scripted (tests/augment_ref.py CASES: the random stream hands out chosen numbers, so that the mosaic centre sits at its extremes, the
scale at 0.5 and 1.5, the angle at 10 degrees, every flip combination occurs) or seeded (random.seed(k), np.random.seed(k): the real streams).
The inputs are rebuilt from seeds by tests/augment_ref.py; the fixtures hold expected outputs and the recorded draws only."""
import importlib.metadata as md
import json
import os
import random
import sys
from pathlib import Path
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np
import torch

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))

import augment_ref as AR  # noqa: E402
import letterbox_ref as LR  # noqa: E402

INTER_LINEAR, BORDER_CONSTANT, COLOR_BGR2HSV, COLOR_HSV2BGR = 1, 0, 40, 54


def resize(img, dsize, interpolation=None):
    assert interpolation == INTER_LINEAR and img.dtype == np.uint8 and img.ndim == 3
    return LR.resize_u8(torch.from_numpy(np.ascontiguousarray(img)), (int(dsize[1]), int(dsize[0]))).numpy()


def copy_make_border(img, top, bottom, left, right, border_type, value=None):
    assert border_type == BORDER_CONSTANT and min(top, bottom, left, right) >= 0
    h, w, c = img.shape
    out = np.empty((h + top + bottom, w + left + right, c), dtype=img.dtype)
    out[...] = np.asarray(value[:c], dtype=img.dtype)
    out[top : top + h, left : left + w] = img
    return out


def get_rotation_matrix_2d(angle, center, scale):
    return AR.rotation_matrix_2d(center, angle, scale)


def warp_affine(img, M, dsize, borderValue=None):
    """stand-in for cv2.warpAffine, INTER_LINEAR, BORDER_CONSTANT (see DISCLOSURE above); dsize is (width, height)"""
    assert img.dtype == np.uint8 and img.ndim == 3 and dsize[0] == dsize[1] and tuple(borderValue) == (114, 114, 114) and M.shape == (2, 3)
    h, w = img.shape[:2]
    return AR.warp_affine([img], [(0, 0, w, h, 0, 0)], (h, w), AR.invert_affine(M), int(dsize[0]), border=114)


def cvt_color(img, code, dst=None):
    """stand-in for cv2.cvtColor, 8-bit BGR <-> HSV (see DISCLOSURE above)"""
    assert img.dtype == np.uint8 and code in (COLOR_BGR2HSV, COLOR_HSV2BGR)
    out = AR.bgr2hsv(img) if code == COLOR_BGR2HSV else AR.hsv2bgr(img)
    if dst is not None:
        dst[...] = out
        return dst
    return out


def import_reference():
    os.environ.setdefault("YOLO_OFFLINE", "true")
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/ulcfg")
    os.environ.setdefault("YOLO_VERBOSE", "false")
    cv2 = MagicMock(__version__="4.10.0")
    cv2.resize, cv2.copyMakeBorder, cv2.INTER_LINEAR, cv2.BORDER_CONSTANT = resize, copy_make_border, INTER_LINEAR, BORDER_CONSTANT
    cv2.getRotationMatrix2D, cv2.warpAffine, cv2.cvtColor, cv2.COLOR_BGR2HSV, cv2.COLOR_HSV2BGR = get_rotation_matrix_2d, warp_affine, cvt_color, COLOR_BGR2HSV, COLOR_HSV2BGR
    cv2.split = lambda im: tuple(np.ascontiguousarray(im[..., c]) for c in range(im.shape[2]))
    cv2.merge = lambda chans: np.stack(chans, -1)
    cv2.LUT = lambda src, lut: lut[src]
    sys.modules.setdefault("cv2", cv2)
    orig = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else orig(n)
    sys.path.insert(0, str(REF))
    import ultralytics.data.augment as augment
    from ultralytics.utils.instance import Instances

    assert augment.cv2.warpAffine is warp_affine and augment.cv2.cvtColor is cvt_color
    return augment, Instances


class Dataset:
    """what v8_transforms and Mosaic ask of a data set"""

    def __init__(self, data, Instances):
        self.items, self.Instances = data, Instances
        self.buffer = list(range(len(data)))
        self.data, self.use_keypoints = {}, False

    def __len__(self):
        return len(self.items)

    def get_image_and_label(self, i):
        d = self.items[i]
        h, w = d["img"].shape[:2]
        inst = self.Instances(d["labels"][:, 1:].copy(), np.zeros((0, 1000, 2), dtype=np.float32), None, bbox_format="xywh", normalized=True)
        return dict(img=d["img"].copy(), cls=d["labels"][:, :1].copy(), instances=inst, resized_shape=(h, w), ori_shape=(h, w), im_file=f"{i}.jpg",
                    ratio_pad=(1.0, 1.0))


def run_case(augment, Instances, name, index, hyp, labels, stream, store_canvas):
    data = AR.dataset(labels)
    ds = Dataset(data, Instances)
    ns = SimpleNamespace(**hyp)
    transforms = augment.v8_transforms(ds, AR.S, ns)
    seen = {}
    orig = augment.RandomPerspective.affine_transform

    def spy(self, img, border):
        out = orig(self, img, border)
        seen.update(canvas=img.copy(), M=out[1].copy(), scale=float(out[2]), size=tuple(self.size))
        return out

    augment.RandomPerspective.affine_transform = spy
    real_random, real_np_random = augment.random, augment.np.random
    augment.random = stream
    np_proxy = SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    np_proxy.random = stream.np
    augment.np = np_proxy
    try:
        out = transforms(ds.get_image_and_label(index))
    finally:
        augment.random, augment.np = real_random, np
        augment.RandomPerspective.affine_transform = orig
    assert real_np_random is np.random
    img = np.ascontiguousarray(out["img"])
    assert img.dtype == np.uint8 and img.shape == (AR.S, AR.S, 3)
    fmt = augment.Format(bbox_format="xywh", normalize=True, return_mask=False, return_keypoint=False, return_obb=False, batch_idx=True, mask_ratio=4,
                         mask_overlap=True, bgr=0.0)
    formatted = fmt(dict(out, img=img.copy()))
    nl = len(formatted["bboxes"])
    arrays = dict(img=img, cls=np.asarray(formatted["cls"], dtype=np.float32).reshape(nl, 1), bboxes=np.asarray(formatted["bboxes"], dtype=np.float32).reshape(nl, 4),
                  M=seen["M"], scale=np.float64(seen["scale"]))
    assert seen["size"] == (AR.S, AR.S) and seen["M"].dtype == np.float32
    if store_canvas:
        arrays["canvas"] = seen["canvas"]
    path = OUT / f"augment_{name}.npz"
    np.savez_compressed(path, **arrays)
    print(f"augment_{name}.npz  {path.stat().st_size / 1024:.1f} kB  kept {nl}", flush=True)


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref_augment, ref_instances = import_reference()
    draws = {}
    for name, c in AR.CASES.items():
        stream = AR.ScriptedRandom(c["unit"])
        run_case(ref_augment, ref_instances, name, c["index"], AR.case_hyp(c), c.get("labels", "normal"), stream, name in ("centre_lo", "centre_hi", "scale15"))
        assert not stream.unit, f"{name}: {len(stream.unit)} scripted numbers left over"
        draws[name] = {"kinds": [kind for kind, _ in stream.calls], "values": [v for _, v in stream.calls]}
    for k in AR.SEEDS:
        random.seed(k)
        np.random.seed(k)
        stream = AR.RecordingRandom()
        run_case(ref_augment, ref_instances, f"seed{k}", k % 4, dict(AR.HYP), "normal", stream, k == 1)
        draws[f"seed{k}"] = {"kinds": [kind for kind, _ in stream.calls], "values": [v for _, v in stream.calls]}
    (OUT / "augment_draws.json").write_text(json.dumps(draws) + "\n")
