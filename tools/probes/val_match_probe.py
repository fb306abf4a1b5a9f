"""Time a validation pass with the matching on the host and on the device, on one MI355X (not a test; bench.py does not read it).

    python tools/probes/val_match_probe.py [--out profiles/val_match_probe.txt] [--batches 20] [--reps 5]

One process, the variants alternating inside it; every shape is warmed up before it is timed.
  workload: yolov8s-CBAM-Swin eval at batch 32 / 640^2 / nc 80 under bf16 autocast, conf 0.001, the class bias raised until every image keeps
  max_det = 300 detections (as tests/test_gpu_validator.py::_raise_class_bias does), 20 labels per image, `batches` batches per pass.
  1. DetectionValidator(match="host")(batches): wall time per batch, to a synchronise (forward, NMS, one trip per batch, host matching).
  2. DetectionValidator(match="device")(batches): the same (forward, NMS, ymi_val_match, one trip per pass).
  for scale: the eval forward + ops.detect_nms alone over the same batches, to a synchronise.
  3. ymi_val_match alone, HIP events around windows of 20 launches, median of 30 windows, at (B 32, max_det 300, L 640) and at
     (B 32, max_det 2048, L 4096), all rows live, with the confusion matrix.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

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


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def kernel_input(B, max_det, labels_per_image, nc, dev, seed):
    """every row live: detections are jittered copies of the image's labels, ranked by confidence; the label table is shuffled"""
    g = torch.Generator().manual_seed(seed)
    L = B * labels_per_image
    box = torch.cat((torch.rand(L, 2, generator=g) * 0.8 + 0.1, torch.rand(L, 2, generator=g) * 0.22 + 0.03), 1)
    cls = torch.randint(0, nc, (L,), generator=g).float()
    img = torch.arange(B).repeat_interleave(labels_per_image)
    pick = torch.randint(0, labels_per_image, (B, max_det), generator=g) + torch.arange(B)[:, None] * labels_per_image
    half = box[pick][..., 2:] / 2
    xyxy = torch.cat((box[pick][..., :2] - half, box[pick][..., :2] + half), -1) * 640 + torch.randn(B, max_det, 4, generator=g) * 4
    conf = torch.sort(torch.rand(B, max_det, generator=g), 1, descending=True)[0]
    det = torch.cat((xyxy, conf[..., None], cls[pick][..., None]), -1).contiguous()
    perm = torch.randperm(L, generator=g)
    count = torch.full((B,), max_det, dtype=torch.int32)
    return det.to(dev), count.to(dev), img[perm].int().to(dev), cls[perm].to(dev), box[perm].contiguous().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_match_probe measures on the MI355X: no GPU here, nothing measured")

    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd._lib import check, lib, ptr, stream_ptr
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    dev = torch.device("cuda:0")
    B, nc = 32, 80
    lines = [f"device {torch.cuda.get_device_name(0)}; yolov8s-CBAM-Swin eval, batch {B}, 640^2, nc {nc}, bf16 autocast, conf 0.001, iou 0.7, max_det 300; "
             f"{args.batches} batches per pass, {args.reps} alternating passes per variant"]

    def report(s):
        lines.append(s)
        print(s, flush=True)

    torch.manual_seed(0)
    model = DetectionModel("yolov8s.yaml", ch=3, nc=nc).to(dev).eval()
    distinct = []
    for i in range(4):
        b = synthetic_batch(B, 640, dev, 100 + i, boxes_per_image=20)
        b["cls"] = torch.randint(0, nc, (b["cls"].numel(), 1), generator=torch.Generator().manual_seed(i)).float().to(dev)
        distinct.append(b)
    batches = [distinct[i % 4] for i in range(args.batches)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):  # the class bias, raised until ~400 anchors per image score above 0.02
        y = model(distinct[0]["img"])[0]
        top = y[:, 4:].amax(1).flatten().sort(descending=True)[0]
        target = float(top[400 * B])
        shift = float(np.log(0.02 / 0.98) - np.log(max(target, 1e-12) / max(1 - target, 1e-12)))
        for m in model.model[-1].cv3:
            m[-1].bias.add_(shift)

    host, device = DetectionValidator(model, match="host"), DetectionValidator(model, match="device")

    def forward_nms():
        with torch.no_grad():
            for b in batches:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    preds = model(b["img"])
                host.postprocess(preds)

    r_dev, r_host = device(batches[:2]), host(batches[:2])  # warm-up, and the two paths' results side by side
    assert all(torch.equal(a, b) for a, b in zip(host.detections, device.detections))
    assert all(torch.equal(torch.cat(host.stats[k]), torch.cat(device.stats[k])) for k in host.stats), "the two paths disagree"
    assert np.array_equal(host.confusion_matrix.matrix, device.confusion_matrix.matrix) and r_dev == r_host
    per_image = [len(d) for d in device.detections]
    report(f"detections per image min {min(per_image)} median {int(statistics.median(per_image))} max {max(per_image)}; {batches[0]['cls'].numel() // B} labels per image; "
           f"tp, statistics and confusion matrix of the two paths equal on the warm-up batches")
    forward_nms()
    t_host, t_dev, t_fwd = [], [], []
    for _ in range(args.reps):
        t_host.append(wall(lambda: host(batches)) / args.batches)
        t_dev.append(wall(lambda: device(batches)) / args.batches)
        t_fwd.append(wall(forward_nms) / args.batches)
    fmt = lambda v: f"median {statistics.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}"  # noqa: E731
    report(f"1. DetectionValidator(match='host')   per batch, wall to a synchronise : {fmt(t_host)}")
    report(f"2. DetectionValidator(match='device') per batch, wall to a synchronise : {fmt(t_dev)}")
    report(f"   eval forward + ops.detect_nms alone per batch, wall to a synchronise: {fmt(t_fwd)}")

    import ctypes

    lv = (ctypes.c_float * 10)(*[float(v) for v in torch.linspace(0.5, 0.95, 10)])

    for max_det, per in ((300, 20), (2048, 128)):
        det, count, lab_img, lab_cls, lab_box = kernel_input(B, max_det, per, nc, dev, 7)
        tp = torch.empty(B, max_det, 10, dtype=torch.uint8, device=dev)
        cm = torch.zeros(nc + 1, nc + 1, dtype=torch.int32, device=dev)

        def raw():
            check(lib().ymi_val_match(ptr(det), ptr(count), B, max_det, ptr(lab_img), ptr(lab_cls), ptr(lab_box), lab_img.numel(), 640.0, 640.0, None, lv, 10, 0,
                                      ptr(tp), ptr(cm), nc, 0.25, 0.45, stream_ptr()), "val_match")

        ms = windows(raw, args.kernel_reps)
        assert torch.equal(tp, ops.val_match(det, count, lab_img, lab_cls, lab_box, (640, 640), torch.linspace(0.5, 0.95, 10)))
        report(f"3. ymi_val_match B {B}, max_det {max_det}, L {lab_img.numel()} (one launch, all rows live, with the matrix; {int(tp[..., 0].sum())} correct at 0.5)"
               f": {ms:8.4f} ms   ops.val_match on the same (conversions, allocation, launch): {windows(lambda: ops.val_match(det, count, lab_img, lab_cls, lab_box, (640, 640), [0.5 + 0.05 * i for i in range(10)], cm=cm), args.kernel_reps):8.4f} ms")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
