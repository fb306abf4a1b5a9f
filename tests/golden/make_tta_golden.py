"""Generate the image-rescaling and test-time-augmentation fixtures under tests/golden/ by running the REAL reference on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/make_tta_golden.py

Same import shim as make_golden.py (cv2 stubbed, the torchvision version patched, YOLO_OFFLINE).  What runs is the reference's own
scale_img (utils/torch_utils.py:475-495), DetectionTrainer.preprocess_batch (models/yolo/detect/train.py:90-115; called unbound on a
namespace that carries args.multi_scale, args.imgsz, stride and device) and DetectionModel.predict(x, augment=True) (nn/tasks.py:374-439).

Files (data only):
    tta_scale_<case>.npz   uint8 input, the reference's scale_img(input.float() / 255 [flipped left-right]) and the call's arguments
    tta_pre_<case>.npz     uint8 input, preprocess_batch's output image under random.seed(k)
    tta_multiscale_sizes.json   the sizes preprocess_batch produces for random.seed(0..63) on three input shapes (integers only)
    tta_descale.npz        seeded predictions, the reference's _descale_pred of each (flips none / up-down / left-right) and
                           torch.cat(_clip_augmented([...]), -1) of the three
    tta_tiny.npz           uint8 input and predict(x, augment=True)[0] of the width-reduced model of e2e_tiny_seed7_yaml.json at nc 3, weights
                           rebuilt from a seed by tests/tta_ref.py::seeded_model_state (not stored)"""
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

import tta_ref as TR  # noqa: E402

SCALE_CASES = {  # name: (input seed, input shape, ratio, same_shape, gs, flip)
    "a83": (101, (2, 3, 96, 128), 0.83, False, 32, None),      # 79 x 106 in 96 x 128: ws % 4 = 2, padding on both axes
    "a67_lr": (101, (2, 3, 96, 128), 0.67, False, 32, 3),       # 64 x 85 in 96 x 96, flipped left-right: ws % 4 = 1
    "b83": (102, (1, 3, 40, 72), 0.83, False, 32, None),        # 33 x 59 in 64 x 64
    "b83_same": (102, (1, 3, 40, 72), 0.83, True, 32, None),    # 33 x 59 in 40 x 72 (same_shape)
    "b150": (102, (1, 3, 40, 72), 1.5, False, 32, None),        # up-scaling: 60 x 108 in 64 x 128
    "b100": (102, (1, 3, 40, 72), 1.0, False, 32, None),        # ratio 1.0: the input itself
}
PRE_CASES = {  # name: (input seed, input shape, imgsz, stride, random.seed); None: the first seed of tta_multiscale_sizes.json that gives PRE_WANT's size
    "down32": (201, (1, 3, 64, 64), 64, 32, None),
    "up96": (201, (1, 3, 64, 64), 64, 32, None),
    "same64": (201, (1, 3, 64, 64), 64, 32, None),
    "rect96": (202, (1, 3, 48, 64), 64, 32, None),
    "plain": (201, (1, 3, 64, 64), 64, 32, -1),  # multi_scale off
}
PRE_WANT = {"down32": (32, 32), "up96": (96, 96), "same64": (64, 64), "rect96": (96, 96)}
SIZE_SHAPES = [(64, 64), (48, 64), (80, 56)]
TINY_SEED, TINY_NC, TINY_SHAPE = 77, 3, (2, 3, 96, 128)


def import_reference():
    os.environ.setdefault("YOLO_OFFLINE", "true")
    os.environ.setdefault("YOLO_CONFIG_DIR", "/tmp/ulcfg")
    os.environ.setdefault("YOLO_VERBOSE", "false")
    sys.modules.setdefault("cv2", MagicMock(__version__="4.10.0"))
    orig = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else orig(n)
    sys.path.insert(0, str(REF))
    import ultralytics.nn.tasks as tasks
    import ultralytics.utils.torch_utils as tu
    from ultralytics.models.yolo.detect.train import DetectionTrainer

    return tasks, tu, DetectionTrainer


def save(name, **arrays):
    path = OUT / f"{name}.npz"
    np.savez_compressed(path, **arrays)
    print(f"{name}.npz  {path.stat().st_size / 1024:.1f} kB", flush=True)


def scale_fixtures(tu):
    for name, (seed, shape, ratio, same, gs, flip) in SCALE_CASES.items():
        u8 = TR.seeded_u8(seed, shape)
        x = u8.float() / 255
        y = tu.scale_img(x.flip(flip) if flip else x, ratio, same_shape=same, gs=gs)
        if ratio == 1.0:
            assert y is x
        save(f"tta_scale_{name}", img=u8.numpy(), out=y.numpy().astype(np.float32), ratio=np.float64(ratio), same_shape=np.int64(same), gs=np.int64(gs),
             flip=np.int64(flip or 0))


def run_preprocess(trainer_cls, u8, imgsz, stride, seed):
    holder = SimpleNamespace(args=SimpleNamespace(multi_scale=seed is None or seed >= 0, imgsz=imgsz), stride=stride, device=torch.device("cpu"))
    if seed is not None and seed >= 0:
        random.seed(seed)
    return trainer_cls.preprocess_batch(holder, {"img": u8.clone()})["img"]


def pre_fixtures(trainer_cls):
    # the integer rule over many seeds
    table = []
    for h, w in SIZE_SHAPES:
        for k in range(64):
            out = run_preprocess(trainer_cls, torch.zeros(1, 1, h, w, dtype=torch.uint8), 64, 32, k)
            table.append([h, w, 64, 32, k, int(out.shape[2]), int(out.shape[3])])
    (OUT / "tta_multiscale_sizes.json").write_text(json.dumps(table) + "\n")
    for name, (seed, shape, imgsz, stride, k) in PRE_CASES.items():
        u8 = TR.seeded_u8(seed, shape)
        if k is None:  # the first random.seed that gives the wanted size
            k = next(r[4] for r in table if (r[0], r[1]) == tuple(shape[2:]) and (r[5], r[6]) == PRE_WANT[name])
        out = run_preprocess(trainer_cls, u8, imgsz, stride, k)
        if name in PRE_WANT:
            assert tuple(out.shape[2:]) == PRE_WANT[name], (name, out.shape)
        save(f"tta_pre_{name}", img=u8.numpy(), out=out.numpy().astype(np.float32), imgsz=np.int64(imgsz), stride=np.int64(stride), seed=np.int64(k))


def descale_fixture(tasks):
    rs = np.random.RandomState(401)
    img_size = (96, 128)
    preds = [torch.from_numpy((rs.rand(2, 7, a) * 120).astype(np.float32)) for a in (252, 252, 189)]
    out = {f"p{i}": p.numpy() for i, p in enumerate(preds)}
    ys = []
    for i, (p, s, f) in enumerate(zip(preds, (1, 0.83, 0.67), (None, 3, 2))):  # (the up-down flip is not in _predict_augment's list: covered here)
        y = tasks.DetectionModel._descale_pred(p.clone(), f, s, img_size)
        out[f"d{i}"] = y.numpy()
        ys.append(y)
    holder = SimpleNamespace(model=[SimpleNamespace(nl=3)])
    out["merged"] = torch.cat(tasks.DetectionModel._clip_augmented(holder, ys), -1).numpy()
    save("tta_descale", scales=np.array([1, 0.83, 0.67]), flips=np.array([0, 3, 2]), img_size=np.array(img_size), **out)


def tiny_fixture(tasks):
    cfg = json.loads((OUT / "e2e_tiny_seed7_yaml.json").read_text())
    torch.manual_seed(7)
    model = tasks.DetectionModel(cfg, ch=3, nc=TINY_NC, verbose=False)
    missing = model.load_state_dict(TR.seeded_model_state(model.state_dict(), TINY_SEED), strict=False)
    assert not missing.unexpected_keys
    model.eval()
    u8 = TR.seeded_u8(301, TINY_SHAPE)
    x = u8.float() / 255
    with torch.no_grad():
        y, none = model.predict(x, augment=True)
        y1 = model.predict(x)[0]
    assert none is None
    save("tta_tiny", img=u8.numpy(), y=y.numpy().astype(np.float32), y_plain=y1.numpy().astype(np.float32), stride=model.stride.numpy(),
         nc=np.int64(TINY_NC), seed=np.int64(TINY_SEED))
    print("tta_tiny: y", tuple(y.shape), "plain", tuple(y1.shape), "max", float(y.abs().max()), flush=True)


if __name__ == "__main__":
    torch.set_num_threads(8)
    ref_tasks, ref_tu, ref_trainer = import_reference()
    scale_fixtures(ref_tu)
    pre_fixtures(ref_trainer)
    descale_fixture(ref_tasks)
    tiny_fixture(ref_tasks)
