"""Time the training-augmentation kernels on one MI355X (not a test; bench.py does not read it).

    python tools/probes/augment_probe.py [--out profiles/augment_probe.txt] [--reps 30]

HIP events around a window of repeated launches in one process, medians over `reps` windows; every shape is warmed up before it is timed.
  1. one ymi_augment_batch launch (through the C ABI, sources and table already on the device, destination allocated once) for B = 32 images
     of 640^2, each a mosaic of four 640 x 480 sources under v8_transforms' default draws, with and without the colour stage, and the bytes the
     launch moves at most (every source byte once, the float32 destination once) as a share of the 8 TB/s HBM peak.  A mosaic shows only part
     of its sources, so the bytes actually read are fewer: the share is an upper bound on the traffic, not a roofline.
  2. one ymi_augment_boxes launch for the batch's labels (8 rows per source image).
  3. ops.augment_batch from HOST images (geometry, packing into the staging buffer, the one upload, both launches, the read of the count), wall time.
  4. the yardstick: the ymi_letterbox_batch line of profiles/letterbox_probe.txt for 32 images of 480 x 640, quoted beside it.
"""
import argparse
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

HBM_PEAK_TBS = 8.0
WINDOW = 20  # launches per timed window


def windows(fn, reps, warmup=3):
    """median ms per call over `reps` windows of WINDOW calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(WINDOW):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / WINDOW)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_probe measures on the MI355X: no GPU here, nothing measured")

    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.data.augment import v8_transforms
    from improving_yolov8_cbam_swinblock_amd.ops.augment import pack_augment

    dev = torch.device("cuda:0")
    B, S, H, W, ROWS = 32, 640, 480, 640, 8
    lines = [f"device {torch.cuda.get_device_name(0)}; {B} images of {S}^2, each a mosaic of four {W}x{H} uint8 sources, v8_transforms' default draws (seed 0); "
             f"HIP events, medians of {args.reps} windows of {WINDOW} calls; shares of the {HBM_PEAK_TBS} TB/s HBM peak"]

    def report(name, ms, nbytes=None):
        s = f"{name:<100}: {ms:8.4f} ms"
        if nbytes is not None:
            s += f"  {nbytes / 1e6:7.1f} MB  {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (ms * 1e-3) / (HBM_PEAK_TBS * 1e12):5.1f} % of the peak"
        lines.append(s)
        print(s, flush=True)

    rs = np.random.RandomState(0)

    def one():
        lab = np.concatenate([rs.randint(0, 3, (ROWS, 1)), rs.uniform(0.2, 0.8, (ROWS, 2)), rs.uniform(0.05, 0.3, (ROWS, 2))], 1).astype(np.float32)
        return {"img": rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8), "labels": lab}

    host = []
    for _ in range(B):
        smp = one()
        smp["mix_labels"] = [one() for _ in range(3)]
        host.append(smp)
    on_dev = [{"img": torch.from_numpy(s["img"]).to(dev), "labels": s["labels"],
               "mix_labels": [{"img": torch.from_numpy(m["img"]).to(dev), "labels": m["labels"]} for m in s["mix_labels"]]} for s in host]
    random.seed(0)
    np.random.seed(0)
    draw = v8_transforms(None, S, None)
    params = [draw(pick_partners=False) for _ in range(B)]
    out = torch.empty(B, 3, S, S, device=dev)
    for hsv in (True, False):
        pr = params if hsv else [dict(p, hsv=None) for p in params]
        plan = pack_augment(on_dev, pr, S, dev)
        torch.cuda.synchronize()
        nbytes = plan.source_bytes + out.numel() * 4
        report(f"ymi_augment_batch {B} x (4 x {W}x{H} uint8) -> float32 {S}^2, {'warp + HSV + flip' if hsv else 'warp + flip, no colour stage'} (one launch)",
               windows(lambda: plan.images(out), args.reps), nbytes)
        report("  the same against the bytes of the destination and of one destination's worth of source pixels", windows(lambda: plan.images(out), args.reps),
               out.numel() * 4 + B * S * S * 3)
    n = plan.n
    bi, cl, bb = torch.empty(n, device=dev), torch.empty(n, 1, device=dev), torch.empty(n, 4, device=dev)
    keep, count = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(B + 1, dtype=torch.int32, device=dev)
    report(f"ymi_augment_boxes {n} label rows of {B} images (one launch, one workgroup)", windows(lambda: plan.labels(bi, cl, bb, keep, count), args.reps))
    t0 = []
    for _ in range(5):
        torch.cuda.synchronize()
        t = time.perf_counter()
        ops.augment_batch(host, params, S)
        torch.cuda.synchronize()
        t0.append((time.perf_counter() - t) * 1e3)
    report(f"ops.augment_batch from {B * 4} host images: geometry + pack + one upload of {B * 4 * H * W * 3 / 1e6:.1f} MB + both launches (host clock, median of 5)",
           statistics.median(t0))
    yard = ROOT / "profiles" / "letterbox_probe.txt"
    if yard.exists():
        for ln in yard.read_text().splitlines():
            if ln.startswith("ymi_letterbox_batch") and "480x640" in ln:
                lines.append("yardstick (profiles/letterbox_probe.txt): " + ln)
                print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
