"""Time the image-rescaling kernels and what is built on them, on one MI355X (not a test; bench.py does not read it).

    python tools/probes/resize_probe.py [--out profiles/resize_probe.txt] [--batch 32] [--reps 30]

HIP events around repeated calls in one process, medians; every shape is warmed up before it is timed; the variants of a comparison alternate.
  1. ops.scale_image for uint8 640^2 -> float32 640^2 (conversion only) and -> 960^2 (bilinear), against the ATen chain it replaces
     (.float() / 255, F.interpolate), with the bytes each must move (read the source once, write the destination once) as a share of the
     6.3 TB/s a streaming kernel reaches here; the test-time-augmentation sizes (flip + 0.83 / 0.67 + pad) against flip + interpolate + pad;
     ops.tta_merge against _descale_pred + _clip_augmented + cat in ATen.
  2. predict(augment=True) of yolov8s-CBAM-Swin in bf16 against three plain forwards at 640^2.
  3. TrainStep(graph=True, image_shapes=N) over the multi-scale sizes of imgsz 640 (320 ... 960, stride 32) against eager steps on the same
     batches: a seeded draw of sizes, per-step wall time after every shape has been captured.
"""
import argparse
import math
import random
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

HBM_TBS = 6.3  # achievable streaming bandwidth of an MI355X


def timed_alternating(fns, reps, warmup=3):
    """{name: median ms} of HIP-event timings; the variants run in turn, so drift hits all of them alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40, help="multi-scale training steps timed per mode")
    ap.add_argument("--shapes", type=int, default=6, help="distinct multi-scale sizes in the training comparison (each is captured once)")
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_probe measures on the MI355X: no GPU here, nothing measured")

    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, preprocess_batch, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    dev = torch.device("cuda:0")
    B = args.batch
    lines = [f"device {torch.cuda.get_device_name(0)}; batch {B}; HIP events, medians of {args.reps}; shares of {HBM_TBS} TB/s"]

    def report(name, ms, nbytes=None, base=None):
        s = f"{name:<74}: {ms:8.3f} ms"
        if nbytes is not None:
            s += f"  {nbytes / 1e6:7.1f} MB  {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (ms * 1e-3) / (HBM_TBS * 1e12):5.1f} % of the bandwidth"
        if base is not None:
            s += f"  ({base / ms:4.1f}x the ATen chain's {base:.3f} ms)"
        lines.append(s)
        print(s, flush=True)

    # ---- 1. the kernels -------------------------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, 3, 640, 640), dtype=torch.uint8, generator=g).to(dev)
    xf = u8.float() / 255
    for size in (640, 960):
        def aten(size=size):
            x = u8.float() / 255
            return x if size == 640 else F.interpolate(x, size=(size, size), mode="bilinear", align_corners=False)

        t = timed_alternating({"hip": lambda size=size: ops.scale_image(u8, (size, size)), "aten": aten}, args.reps)
        nbytes = u8.numel() + B * 3 * size * size * 4
        report(f"scale_image uint8 640^2 -> float32 {size}^2", t["hip"], nbytes, t["aten"])
    for ratio, flip in ((0.83, 3), (0.67, None)):
        hs = int(640 * ratio)
        hp = math.ceil(640 * ratio / 32) * 32

        def aten(hs=hs, hp=hp, flip=flip):
            x = xf.flip(flip) if flip else xf
            return F.pad(F.interpolate(x, size=(hs, hs), mode="bilinear", align_corners=False), [0, hp - hs, 0, hp - hs], value=0.447)

        t = timed_alternating({"hip": lambda hs=hs, hp=hp, flip=flip: ops.scale_image(xf, (hs, hs), (hp, hp), 0.447, flip=flip), "aten": aten}, args.reps)
        report(f"scale_image float32 640^2 -> {hs} in {hp}{', flipped' if flip else ''} (TTA pass)", t["hip"], xf.numel() * 4 + B * 3 * hp * hp * 4, t["aten"])
    nc = 80
    preds = [torch.rand(B, 4 + nc, a, device=dev) * 600 for a in (8400, 6069, 4116)]
    scales, flips, ranges = (1, 0.83, 0.67), (None, 3, None), ops.tta_clip_ranges([8400, 6069, 4116], 3)

    def aten_merge():
        ys = []
        for p, s, f in zip(preds, scales, flips):
            p = p.clone()  # (the reference edits the model's output in place; the clone keeps the timed input fixed)
            p[:, :4] /= s
            x, y, wh, cls = p.split((1, 1, 2, nc), 1)
            if f == 3:
                x = 640 - x
            ys.append(torch.cat((x, y, wh, cls), 1))
        return torch.cat([y[..., lo:hi] for y, (lo, hi) in zip(ys, ranges)], -1)

    t = timed_alternating({"hip": lambda: ops.tta_merge(preds, scales, flips, (640, 640), ranges), "aten": aten_merge}, args.reps)
    kept = sum(hi - lo for lo, hi in ranges)
    report(f"tta_merge 3 x [B, {4 + nc}, A] -> [B, {4 + nc}, {kept}]", t["hip"], 2 * B * (4 + nc) * kept * 4, t["aten"])

    # ---- 2. the augmented forward ---------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    model = DetectionModel("yolov8s.yaml", ch=3, nc=1).to(dev).eval()

    def fwd(augment):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            if augment:
                return model.predict(xf, augment=True)
            return [model.predict(xf) for _ in range(3)]

    t = timed_alternating({"tta": lambda: fwd(True), "plain3": lambda: fwd(False)}, max(5, args.reps // 3))
    report("predict(augment=True), yolov8s-CBAM-Swin 640^2 bf16 (1 + 0.83 + 0.67)", t["tta"])
    report("three plain forwards at 640^2 (for scale: the augmented passes are smaller)", t["plain3"])
    del model

    # ---- 3. multi-scale training ----------------------------------------------------------------------------------------------------
    if not args.skip_train:
        rng = random.Random(0)
        sizes = []
        while len(set(sizes)) < args.shapes:  # the sizes preprocess_batch draws at imgsz 640, stride 32, until `shapes` distinct ones occurred
            sizes.append(rng.randrange(320, 992) // 32 * 32)
        sizes = (sizes * (args.steps // len(sizes) + 1))[: args.steps]
        base = synthetic_batch(B, 640, dev, 1)
        base["img"] = u8
        batches = {s: preprocess_batch(dict(base, img=ops.scale_image(u8, (s, s))), 640, 32) for s in set(sizes)}  # (float32 already: passes through)
        res = {}
        for mode in ("eager", "graph"):
            torch.manual_seed(0)
            model = DetectionModel("yolov8s.yaml", ch=3, nc=1).to(dev)
            step = TrainStep(model, world_size=1, lr=0.01, graph=mode == "graph", image_shapes=args.shapes if mode == "graph" else 1)
            for s in sorted(set(sizes)):  # every shape once: eager warm-up / capture
                step(batches[s])
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for s in sizes:
                items = step(batches[s])
            b.record()
            b.synchronize()
            res[mode] = a.elapsed_time(b) / len(sizes)
            assert torch.isfinite(items).all()
            del step, model
            torch.cuda.empty_cache()
        report(f"multi-scale step, {args.shapes} sizes {sorted(set(sizes))}: eager", res["eager"])
        report(f"multi-scale step, the same batches: graph=True, image_shapes={args.shapes}", res["graph"])
        lines.append(f"    graph / eager = {res['graph'] / res['eager']:.3f} per step (mean over {len(sizes)} steps, all shapes captured before the window)")
        print(lines[-1])
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
