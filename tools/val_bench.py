"""Time the detection post-processing next to the eval forward it follows (bench.py is the training yardstick and stays as it is).

    python tools/val_bench.py [--out profiles/val_postprocess.txt]           # timings with HIP events, one process
    rocprofv3 --kernel-trace --stats -d DIR -o nms -- python tools/val_bench.py --trace-only   # a trace of the NMS launches alone ...
    python tools/val_bench.py --kernel-table DIR/nms_results.db                                # ... and its per-kernel medians

Measured in one process on one MI355X:
  * the eval forward of yolov8s-CBAM-Swin at batch 32 / 640^2 under bf16 autocast (the yardstick: measurable on any commit);
  * ops.detect_nms on the seeded loaded input of the tests (tests/nms_exact.py cluster_image: nc 3, ~25 k candidates per image, batch 32) at
    conf 0.001 / iou 0.7 (validation settings) and at conf 0.25 / iou 0.45 (prediction settings), eager and as a replayed graph;
  * for scale, the time tests/nms_exact.py (torch on the host) takes for the same batch.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(fn, reps, warmup=3):
    """median / min of `reps` HIP-event timings of fn(), in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def kernel_table(db):
    """median duration per kernel and setting from the rocprofv3 database of a --trace-only run (5 calls per setting, in SETTINGS order)."""
    import re
    import sqlite3

    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    rows = [(re.search(r"nms_\w+_kernel", n).group(0), (e - s) / 1000) for n, s, e in rows if "nms_" in n]
    lines = []
    for g, (name, _) in enumerate(SETTINGS):
        per = {}
        for k, d in rows[g * 15 : (g + 1) * 15]:
            per.setdefault(k, []).append(d)
        lines.append(f"kernels    {name}: " + "  ".join(f"{k} {statistics.median(v):7.1f} us" for k, v in per.items()))
    return lines


SETTINGS = [("val  conf 0.001 iou 0.70", dict(conf_thres=0.001, iou_thres=0.7, multi_label=True)),
            ("pred conf 0.25  iou 0.45", dict(conf_thres=0.25, iou_thres=0.45, multi_label=False)),
            # class-agnostic: fewer than max_det boxes survive in most images, so the scan walks the whole sorted list (its longest run)
            ("val  agnostic, full scan", dict(conf_thres=0.001, iou_thres=0.7, multi_label=True, agnostic=True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-table", default="", help="print per-kernel medians from the database of a traced --trace-only run and exit")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-only", action="store_true", help="only a few detect_nms calls (for a kernel trace)")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()

    if args.kernel_table:
        print("\n".join(kernel_table(args.kernel_table)))
        return
    import nms_exact as NX
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    dev = torch.device("cuda:0")
    y_cpu = torch.from_numpy(np.stack([NX.cluster_image(5000 + i, 8400, 3) for i in range(args.batch)]))
    y = y_cpu.to(dev)
    settings = SETTINGS
    lines = [f"device {torch.cuda.get_device_name(0)}; batch {args.batch}; input: tests/nms_exact.py cluster_image seeds 5000.., A 8400, nc 3"]
    if args.trace_only:
        for _, kw in settings:
            for _ in range(5):
                ops.detect_nms(y, **kw)
        torch.cuda.synchronize()
        return

    torch.manual_seed(0)
    model = DetectionModel("yolov8s.yaml", ch=3, nc=1).to(dev).eval()
    img = torch.rand(args.batch, 3, 640, 640, device=dev)

    def forward():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model(img)

    med, best = timed(forward, args.reps)
    fwd = med
    lines.append(f"eval forward yolov8s-CBAM-Swin bs {args.batch} 640^2 bf16 (eager)      : median {med:8.3f} ms  min {best:8.3f} ms")
    for name, kw in settings:
        det, count = ops.detect_nms(y, **kw)
        torch.cuda.synchronize()
        cand = [int(NX.candidates(y_cpu[b], kw["conf_thres"], kw["multi_label"])[1].numel()) for b in range(min(4, args.batch))]
        med, best = timed(lambda: ops.detect_nms(y, **kw), args.reps)
        lines.append(f"detect_nms {name} (eager, 3 launches)            : median {med:8.3f} ms  min {best:8.3f} ms  = {100 * med / fwd:5.1f} % of the forward"
                     f"   candidates/image {cand}.. kept {count[:4].tolist()}..")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.detect_nms(y, **kw)
        med, best = timed(graph.replay, args.reps)
        lines.append(f"detect_nms {name} (graph replay)                 : median {med:8.3f} ms  min {best:8.3f} ms  = {100 * med / fwd:5.1f} % of the forward")
        if not args.no_host:
            t0 = time.perf_counter()
            NX.nms_exact(y_cpu, kw["conf_thres"], kw["iou_thres"], multi_label=kw["multi_label"], agnostic=kw.get("agnostic", False))
            lines.append(f"nms_exact  {name} (host, torch CPU, same batch)      : {1000 * (time.perf_counter() - t0):8.1f} ms")
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
