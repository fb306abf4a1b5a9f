"""Time the oriented-box kernels and the oriented-box training step on one MI355X (not a test; bench.py does not read it).

    python tools/probes/obb_probe.py [--out profiles/obb_probe.txt] [--rounds 5] [--part NAME]

Parts, each in a fresh child process of its own (without --part this script starts them one after the other and collects their lines):
    kernels  batch 32, 640 x 640, bfloat16, nc 15, the maps of yolov8s-obb's head on a synthetic batch: ymi_obb_angle_fwd / _bwd, ymi_obb_targets,
             ymi_detect_decode_obb beside ymi_detect_decode, and ymi_obb_loss_fwd + _bwd beside ymi_detect_loss_fwd + _bwd (the axis-aligned
             kernels, as the yardstick) on the same maps in the same process
    step     a captured training step of yolov8s-obb beside yolov8s-stock in the same process
HIP events around windows of launches; medians and spreads (min .. max) over the rounds.  No threshold is fixed in advance: the file states
what was found."""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
PARTS = ("kernels", "step")
BATCH, SIZE, NC = 32, 640, 15


def timed(fn, window, rounds):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(window):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / window * 1e3)
    return f"{statistics.median(ts):9.1f} us ({min(ts):.1f} .. {max(ts):.1f})"


def part_kernels(rounds):
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_obb_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import OBBModel

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = OBBModel("yolov8s-obb.yaml", ch=3, nc=NC).to(dev).train()
    head = model.model[-1]
    batch = synthetic_obb_batch(BATCH, SIZE, dev, 1)
    batch["cls"] = (torch.arange(batch["cls"].numel(), device=dev) % NC).float().view(-1, 1)
    crit = model.init_criterion()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        preds = model._predict_once(batch["img"], split_head=True)
    box = [t.detach().requires_grad_(True) for t in preds.box]
    cls = [t.detach().requires_grad_(True) for t in preds.cls]
    angle = preds.angle.detach().requires_grad_(True)
    logits = [torch.randn(BATCH, 8, t.shape[2], t.shape[3], device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)[:, :1].requires_grad_(True)
              for t in preds.box]
    g = batch["max_boxes"]
    t_obb = ops.obb_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], BATCH, g, SIZE, SIZE, dev)
    t_det = ops.detect_targets(batch["batch_idx"], batch["cls"], batch["bboxes"][:, :4], BATCH, g, SIZE, SIZE, dev)
    scale = torch.tensor([7.5 * BATCH, 0.5 * BATCH, 1.5 * BATCH, 7.5, 0.5, 1.5], device=dev)
    seed = torch.ones(3, device=dev)
    ga = torch.ones_like(angle)
    st = crit.stride_list

    def obb_fwd():
        return ops.obb_loss(box, cls, angle, st, t_obb, scale)

    def det_fwd():
        return ops.detect_loss(box, cls, st, t_det, scale)

    def ang_fwd():
        return ops.obb_angle(logits)

    anchors = angle.shape[-1]
    return [f"oriented-box kernels, batch {BATCH}, {SIZE} x {SIZE}, bfloat16 maps, nc {NC}, {anchors} anchors, max_boxes {g}:",
            f"  ymi_obb_angle_fwd                         {timed(ang_fwd, 20, rounds)}",
            f"  ymi_obb_angle_fwd + _bwd                  {timed(lambda: torch.autograd.grad(ang_fwd(), logits, ga), 20, rounds)}",
            f"  ymi_obb_targets                           {timed(lambda: ops.obb_targets(batch['batch_idx'], batch['cls'], batch['bboxes'], BATCH, g, SIZE, SIZE, dev), 20, rounds)}",
            f"  ymi_detect_decode_obb                     {timed(lambda: ops.detect_decode_obb(box, cls, angle, st), 20, rounds)}",
            f"  ymi_detect_decode          (yardstick)    {timed(lambda: ops.detect_decode(box, cls, st), 20, rounds)}",
            f"  ymi_obb_loss_fwd                          {timed(obb_fwd, 10, rounds)}",
            f"  ymi_detect_loss_fwd        (yardstick)    {timed(det_fwd, 10, rounds)}",
            f"  ymi_obb_loss_fwd + _bwd                   {timed(lambda: torch.autograd.grad(obb_fwd()[0], box + cls + [angle], seed), 10, rounds)}",
            f"  ymi_detect_loss_fwd + _bwd (yardstick)    {timed(lambda: torch.autograd.grad(det_fwd()[0], box + cls, seed), 10, rounds)}",
            f"  (head {type(head).__name__}, strides {st}; the times include the Python wrappers' allocations, the same on both sides)"]


def part_step(rounds):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch, synthetic_obb_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel, OBBModel

    dev = torch.device("cuda:0")
    out = []
    for name, ctor, mk in (("yolov8s-obb.yaml", OBBModel, synthetic_obb_batch), ("yolov8s-stock.yaml", DetectionModel, synthetic_batch)):
        torch.manual_seed(0)
        model = ctor(name, ch=3, nc=NC).to(dev)
        step = TrainStep(model, world_size=1, lr=0.01, graph=True)
        batch = mk(BATCH, SIZE, dev, 1)
        for _ in range(3):
            step(batch)
        torch.cuda.synchronize()
        ts = []
        for _ in range(rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                step(batch)
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) / 5)
        out.append(f"TrainStep(graph=True) {name:<20} batch {BATCH}, {SIZE} x {SIZE}, bfloat16, nc {NC}: {statistics.median(ts):8.2f} ms per step ({min(ts):.2f} .. {max(ts):.2f})")
        del step, model, batch
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--part", choices=PARTS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("obb_probe measures on the MI355X: no GPU here, nothing measured")
    if args.part:
        for line in {"kernels": part_kernels, "step": part_step}[args.part](args.rounds):
            print(line, flush=True)
        return
    lines = [f"device {torch.cuda.get_device_name(0)}; HIP events around windows of launches, median (min .. max) of {args.rounds} rounds; a fresh process per part"]
    for part in PARTS:
        proc = subprocess.run([sys.executable, __file__, "--part", part, "--rounds", str(args.rounds)], capture_output=True, text=True, timeout=600)
        if proc.returncode != 0:
            raise SystemExit(f"part {part} failed ({proc.returncode}):\n{proc.stdout[-2000:]}\n{proc.stderr[-2000:]}")
        lines += proc.stdout.strip().splitlines()
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
