"""Time the inference side of segmentation on one MI355X (not a test; bench.py does not read it).

    python tools/probes/segpred_probe.py [--out profiles/segpred_probe.txt] [--reps 15] [--batches 4] [--passes 3]

One fresh process; every shape is warmed up before it is timed; HIP events around windows of launches, median with min and max over the windows.
  workload: batch 32, 640^2, nc 80, nm 32, bfloat16 prototypes [32, 32, 160, 160] (NHWC), max_det 300, every row live (9600 rows), boxes of
  40 .. 320 pixels a side, 20 labels per image in the overlap encoding.
  1. the four launches: ymi_detect_nms_seg, ymi_process_mask (upsample 0 and 1), ymi_mask_overlap, ymi_val_match_masks, each with the bytes
     HBM has to move for it - every output once, every input once (the prototype pixels inside overlapping crops are re-read, but the whole
     map is 52 MB and stays in cache) - and that traffic's share of the 8 TB/s HBM peak.
     process_mask(upsample=1) moves little else than its mask stores: 9600 * 640 * 640 bytes.
  2. for orientation, the torch composition of process_mask on the same device (matmul, crop, F.interpolate, gt), image by image.
  3. SegmentationValidator per batch with match="device" beside match="host" (yolov8s-seg, class bias raised until images keep 300 rows).
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

HBM_PEAK = 8.0e12  # bytes / s (specification)


def windows(fn, reps, per=5, warmup=2):
    """ms per call over `reps` windows of `per` calls -> (median, min, max)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / per)
    return statistics.median(out), min(out), max(out)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segpred_probe measures on the MI355X: no GPU here, nothing measured")

    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_seg_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import SegmentationValidator
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    dev = torch.device("cuda:0")
    B, nc, nm, A, max_det, S, M = 32, 80, 32, 8400, 300, 640, 160
    lines = [f"device {torch.cuda.get_device_name(0)}; batch {B}, {S}^2, nc {nc}, nm {nm}, bf16 prototypes {M}^2, max_det {max_det}; {args.reps} windows of 5 launches"]

    def report(s):
        lines.append(s)
        print(s, flush=True)

    def fmt(t, nbytes=None):
        s = f"median {t[0]:9.4f} ms  min {t[1]:9.4f}  max {t[2]:9.4f}"
        if nbytes is not None:
            s += f"   {nbytes / 1e6:9.1f} MB -> {nbytes / (t[0] * 1e-3) / 1e12:6.3f} TB/s = {100 * nbytes / (t[0] * 1e-3) / HBM_PEAK:5.1f} % of the HBM peak"
        return s

    g = torch.Generator().manual_seed(0)
    # a Segment-shaped NMS input whose images keep max_det rows: scattered boxes, a fifth of the anchors above conf
    y = torch.zeros(B, 4 + nc + nm, A)
    y[:, :2] = torch.rand(B, 2, A, generator=g) * S
    y[:, 2:4] = torch.rand(B, 2, A, generator=g) * 280 + 40
    y[:, 4 : 4 + nc] = torch.rand(B, nc, A, generator=g) * 0.002 * (torch.rand(B, 1, A, generator=g) < 0.2)
    y[:, 4 + nc :] = torch.randn(B, nm, A, generator=g)
    y = y.to(dev)
    proto = torch.randn(B, nm, M, M, generator=g).to(dev, torch.bfloat16).contiguous(memory_format=torch.channels_last)
    batch = synthetic_seg_batch(B, S, dev, 3, boxes_per_image=20)
    enc = batch["masks"]
    lab_img, lab_cls = batch["batch_idx"].to(torch.int32), torch.randint(0, nc, (B * 20,), generator=g).float().to(dev)

    det, coef, count = ops.detect_nms_seg(y, nc, 0.001, 0.7, multi_label=True, max_det=max_det)
    report(f"rows kept per image: min {int(count.min())} max {int(count.max())}")
    rows = det.view(-1, 6)[:, :4].contiguous()
    cf = coef.view(-1, nm).contiguous()
    img = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(max_det)
    n = rows.shape[0]
    # prototype pixels inside the crops (clamped to the map): what the dots have to read, 64 bytes each
    lo = (rows * (M / S)).clamp(0, M)
    crop_px = float(((lo[:, 2].ceil() - lo[:, 0].ceil()).clamp(min=0) * (lo[:, 3].ceil() - lo[:, 1].ceil()).clamp(min=0)).sum())
    levels = [0.5 + 0.05 * i for i in range(10)]
    proto_bytes = min(crop_px * 64, proto.numel() * 2)

    t = windows(lambda: ops.detect_nms_seg(y, nc, 0.001, 0.7, multi_label=True, max_det=max_det), args.reps)
    report(f"1a. ymi_detect_nms_seg (three kernels)        : {fmt(t, y.numel() * 4 + det.numel() * 4 + coef.numel() * 4)}")
    t = windows(lambda: ops.process_mask(proto, rows, cf, img, (S, S), upsample=False), args.reps)
    report(f"1b. ymi_process_mask upsample=0, {n} rows    : {fmt(t, n * M * M + proto_bytes)}")
    t = windows(lambda: ops.process_mask(proto, rows, cf, img, (S, S), upsample=True), args.reps, per=2)
    report(f"1c. ymi_process_mask upsample=1, {n} rows    : {fmt(t, n * S * S + proto_bytes)}   (mask stores {n * S * S / 1e6:.0f} MB)")
    t = windows(lambda: ops.mask_overlap(det, coef, count, proto, enc, (S, S)), args.reps)
    inter, area_pred, area_gt = ops.mask_overlap(det, coef, count, proto, enc, (S, S))
    report(f"1d. ymi_mask_overlap, {n} detections         : {fmt(t, proto_bytes + inter.numel() * 4 + enc.numel())}   ({crop_px / 1e6:.1f} M prototype pixels inside the crops)")
    t = windows(lambda: ops.val_match_masks(det, count, lab_img, lab_cls, inter, area_pred, area_gt, levels), args.reps)
    report(f"1e. ymi_val_match_masks, {lab_img.numel()} labels          : {fmt(t, inter.numel() * 4 + B * max_det * 10)}")

    def torch_composition(upsample):
        for b in range(B):
            r = slice(b * max_det, (b + 1) * max_det)
            m = (cf[r] @ proto[b].float().reshape(nm, -1)).view(-1, M, M)
            e = rows[r] * (M / S)
            c = torch.arange(M, device=dev, dtype=torch.float32)
            keep = (c[None, None, :] >= e[:, 0, None, None]) & (c[None, None, :] < e[:, 2, None, None]) & (c[None, :, None] >= e[:, 1, None, None]) & \
                (c[None, :, None] < e[:, 3, None, None])
            m = m * keep
            if upsample:
                m = F.interpolate(m[None], (S, S), mode="bilinear", align_corners=False)[0]
            m.gt_(0.0)

    report(f"2.  torch composition (matmul, crop, gt), image by image, upsample=0     : {fmt(windows(lambda: torch_composition(False), max(args.reps // 3, 3), per=1))}")
    report(f"    torch composition (matmul, crop, interpolate, gt), upsample=1        : {fmt(windows(lambda: torch_composition(True), max(args.reps // 3, 3), per=1))}")

    torch.manual_seed(0)
    model = SegmentationModel("yolov8s-seg.yaml", ch=3, nc=nc).to(dev).eval()
    batch["cls"] = lab_cls.view(-1, 1)
    batches = [batch] * args.batches
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):  # the class bias, raised until ~400 anchors per image score above 0.02
        top = model(batch["img"])[0][:, 4 : 4 + nc].amax(1).flatten().sort(descending=True)[0]
        target = float(top[400 * B])
        shift = float(np.log(0.02 / 0.98) - np.log(max(target, 1e-12) / max(1 - target, 1e-12)))
        for m in model.model[-1].cv3:
            m[-1].bias.add_(shift)
    host, device = SegmentationValidator(model, match="host"), SegmentationValidator(model, match="device")
    r_dev, r_host = device(batches[:1]), host(batches[:1])
    same = all(torch.equal(torch.cat(host.stats[k]), torch.cat(device.stats[k])) for k in host.stats) and r_dev == r_host
    per_image = [len(d) for d in device.detections]
    report(f"3.  yolov8s-seg, detections per image min {min(per_image)} max {max(per_image)}; tp, tp_m and results of the two paths equal on the warm-up batch: {same}")
    t_host, t_dev = [], []
    for _ in range(args.passes):
        t_host.append(wall(lambda: host(batches)) / args.batches)
        t_dev.append(wall(lambda: device(batches)) / args.batches)
    f3 = lambda v: f"median {statistics.median(v):9.3f} ms  min {min(v):9.3f}  max {max(v):9.3f}"  # noqa: E731
    report(f"    SegmentationValidator(match='host')   per batch, wall to a synchronise : {f3(t_host)}")
    report(f"    SegmentationValidator(match='device') per batch, wall to a synchronise : {f3(t_dev)}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
