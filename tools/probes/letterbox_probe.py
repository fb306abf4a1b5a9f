"""Time the letterbox and box-rescaling kernels on one MI355X (not a test; bench.py does not read it).

    python tools/probes/letterbox_probe.py [--out profiles/letterbox_probe.txt] [--reps 30]

HIP events around a window of repeated launches in one process, medians over `reps` windows; every shape is warmed up before it is timed.
  1. one ymi_letterbox_batch launch (through the C ABI, images already on the device, destination allocated once) for 32 images of
     1080 x 1920 -> 640^2 and 32 of 480 x 640 -> 640^2, with the bytes the launch must move (every source byte once, the float32 destination
     once) as a share of the 8 TB/s HBM peak; ops.letterbox on the same device images (table + allocation + launch) beside it; for scale
     ops.scale_image on a uint8 batch of the same destination size.
  2. ops.letterbox from HOST images (packing into the staging buffer, the one upload, the launch), wall time to a synchronise.
  3. one ymi_scale_boxes launch at (B 32, max_det 300), out of place.
"""
import argparse
import ctypes
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
        raise SystemExit("letterbox_probe measures on the MI355X: no GPU here, nothing measured")

    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd._lib import LetterboxImage, check, lib, ptr, stream_ptr

    dev = torch.device("cuda:0")
    B = 32
    lines = [f"device {torch.cuda.get_device_name(0)}; {B} images; HIP events, medians of {args.reps} windows of {WINDOW} calls; shares of the {HBM_PEAK_TBS} TB/s HBM peak"]

    def report(name, ms, nbytes=None):
        s = f"{name:<86}: {ms:8.4f} ms"
        if nbytes is not None:
            s += f"  {nbytes / 1e6:7.1f} MB  {nbytes / (ms * 1e-3) / 1e12:5.2f} TB/s = {100 * nbytes / (ms * 1e-3) / (HBM_PEAK_TBS * 1e12):5.1f} % of the peak"
        lines.append(s)
        print(s, flush=True)

    rs = np.random.RandomState(0)
    for h, w in ((1080, 1920), (480, 640)):
        host = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for _ in range(B)]
        imgs = [torch.from_numpy(im).to(dev) for im in host]
        (hs, ws), (top, _, left, _), _ = ops.letterbox_geometry((h, w), 640)
        table = (LetterboxImage * B)(*[LetterboxImage(im.data_ptr(), h, w, hs, ws, top, left) for im in imgs])
        out = torch.empty(B, 3, 640, 640, device=dev)

        def raw():
            check(lib().ymi_letterbox_batch(table, B, ptr(out), 640, 640, 114, 1, 1, stream_ptr()), "letterbox_batch")

        nbytes = B * h * w * 3 + out.numel() * 4
        report(f"ymi_letterbox_batch {B} x {h}x{w} uint8 -> {hs}x{ws} in float32 640^2 (one launch)", windows(raw, args.reps), nbytes)
        assert torch.equal(out, ops.letterbox(imgs, 640)[0])
        report(f"ops.letterbox on the same device images (table, allocation, launch)", windows(lambda: ops.letterbox(imgs, 640), args.reps), nbytes)
        t0 = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            ops.letterbox(host, 640)
            torch.cuda.synchronize()
            t0.append((time.perf_counter() - t) * 1e3)
        report(f"ops.letterbox from {B} host images: pack + one upload of {B * h * w * 3 / 1e6:.1f} MB + launch (host clock, median of 5)", statistics.median(t0))
        del imgs, host
    u8 = torch.randint(0, 256, (B, 3, 640, 640), dtype=torch.uint8, device=dev)
    report("for scale: ops.scale_image uint8 640^2 -> float32 640^2 (same destination)", windows(lambda: ops.scale_image(u8, (640, 640)), args.reps),
           u8.numel() + B * 3 * 640 * 640 * 4)

    M = 300
    det = torch.rand(B, M, 6, device=dev) * 640
    count = torch.randint(0, M + 1, (B,), dtype=torch.int32, device=dev)
    params = torch.tensor([[0.5, 0.0, 140.0, 1920.0, 1080.0]] * B, device=dev)
    res = torch.empty_like(det)

    def boxes():
        check(lib().ymi_scale_boxes(ptr(det), 6, ptr(count), ptr(params), B, M, 6, 1, 0, ptr(res), 6, stream_ptr()), "scale_boxes")

    report(f"ymi_scale_boxes B {B}, max_det {M} (one launch, out of place)", windows(boxes, args.reps), 2 * det.numel() * 4)
    report("ops.scale_boxes on the same (parameter upload, allocation, launch)",
           windows(lambda: ops.scale_boxes(det, count, (640, 640), (1080, 1920)), args.reps))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
