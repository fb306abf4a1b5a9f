"""Time the segmentation kernels and the segmentation training step on one MI355X (not a test; bench.py does not read it).

    python tools/probes/seg_probe.py [--out profiles/seg_probe.txt] [--rounds 5] [--part NAME]

Parts, each in a fresh child process of its own (without --part this script starts them one after the other and collects their lines):
    loss     v8SegmentationLoss's mask stage (ops.mask_loss forward, and forward + backward) at batch 32, 640 x 640, bfloat16: prototypes
             160 x 160, the Segment maps of yolov8s-seg's head on a synthetic batch, the foreground count it meets - beside it, for orientation
             only, a batched torch restatement on the same device (einsum over all foreground anchors, BCE, crop by comparison masks)
    d2s      ymi_depth_to_space2 / ymi_space_to_depth2 on [32, 4 * 128, 80, 80] bfloat16 (yolov8s-seg's Proto)
    step     a captured training step of yolov8s-seg beside yolov8s-stock in the same process
HIP events around windows of launches; medians and spreads (min .. max) over the rounds.  No threshold is fixed in advance: the file states
what was found.  (process_mask is not built: nothing to time.)"""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
PARTS = ("loss", "d2s", "step")
BATCH, SIZE = 32, 640


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


def part_loss(rounds):
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_seg_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import SegmentationModel

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SegmentationModel("yolov8s-seg.yaml", ch=3, nc=1).to(dev).train()
    batch = synthetic_seg_batch(BATCH, SIZE, dev, 1)
    crit = model.init_criterion()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        preds = model._predict_once(batch["img"], split_head=True)
    box, cls = [t.detach() for t in preds.box], [t.detach() for t in preds.cls]
    mc = [t.detach().requires_grad_(True) for t in preds.mc]
    proto = preds.proto.detach().requires_grad_(True)
    targets = ops.detect_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], BATCH, batch["max_boxes"], SIZE, SIZE, dev)
    scale = torch.tensor([7.5 * BATCH, 0.5 * BATCH, 1.5 * BATCH, 7.5, 0.5, 1.5], device=dev)
    l3, i3, gidx = ops.detect_loss_assign(box, cls, crit.stride_list, targets, scale)
    nfg = int((gidx >= 0).sum())
    seed = torch.ones(4, device=dev)

    def fwd():
        return ops.mask_loss(l3, i3, gidx, targets, batch["masks"], scale, 10, SIZE, SIZE, proto, mc)

    def fwd_bwd():
        torch.autograd.grad(fwd()[0], [proto] + mc, seed)

    # orientation: the same mathematics in batched torch operations on the device
    fg = gidx >= 0
    bi, ai = fg.nonzero(as_tuple=True)
    k = gidx[bi, ai].long()
    tb = targets[bi, k, 1:5] / SIZE
    area = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
    mx = tb * (SIZE // 4)
    r = torch.arange(SIZE // 4, device=dev, dtype=torch.float32)
    crop = ((r[None, None, :] >= mx[:, 0, None, None]) & (r[None, None, :] < mx[:, 2, None, None]) & (r[None, :, None] >= mx[:, 1, None, None])
            & (r[None, :, None] < mx[:, 3, None, None]))
    gt = (batch["masks"][bi].float() == (k + 1).view(-1, 1, 1).float()).float()

    def torch_fwd():
        coef = torch.cat([m.reshape(BATCH, 32, -1) for m in mc], 2).float()[bi, :, ai]
        logit = torch.einsum("nk,nkhw->nhw", coef, proto.float()[bi])
        bce = torch.nn.functional.binary_cross_entropy_with_logits(logit, gt, reduction="none")
        return ((bce * crop).mean((1, 2)) / area).sum() / max(nfg, 1)

    def torch_fwd_bwd():
        torch.autograd.grad(torch_fwd(), [proto] + mc)

    return [f"mask loss, batch {BATCH}, {SIZE} x {SIZE}, bfloat16, prototypes 160 x 160, {nfg} foreground anchors, max_boxes {batch['max_boxes']}:",
            f"  ops.mask_loss forward            {timed(fwd, 10, rounds)}",
            f"  ops.mask_loss forward + backward {timed(fwd_bwd, 10, rounds)}",
            f"  batched torch forward            {timed(torch_fwd, 3, rounds)}   (orientation)",
            f"  batched torch forward + backward {timed(torch_fwd_bwd, 3, rounds)}   (orientation)"]


def part_d2s(rounds):
    from improving_yolov8_cbam_swinblock_amd import ops

    deep = torch.randn(BATCH, 4 * 128, 80, 80, device="cuda:0").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    wide = ops.depth_to_space2(deep)
    return [f"depth to space, [{BATCH}, 4 x 128, 80, 80] bfloat16:",
            f"  ymi_depth_to_space2 {timed(lambda: ops.depth_to_space2(deep), 20, rounds)}",
            f"  ymi_space_to_depth2 {timed(lambda: ops.space_to_depth2(wide), 20, rounds)}"]


def part_step(rounds):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch, synthetic_seg_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel, SegmentationModel

    dev = torch.device("cuda:0")
    out = []
    for name, ctor, mk in (("yolov8s-seg.yaml", SegmentationModel, synthetic_seg_batch), ("yolov8s-stock.yaml", DetectionModel, synthetic_batch)):
        torch.manual_seed(0)
        model = ctor(name, ch=3, nc=1).to(dev)
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
        out.append(f"TrainStep(graph=True) {name:<20} batch {BATCH}, {SIZE} x {SIZE}, bfloat16: {statistics.median(ts):8.2f} ms per step ({min(ts):.2f} .. {max(ts):.2f})")
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
        raise SystemExit("seg_probe measures on the MI355X: no GPU here, nothing measured")
    if args.part:
        for line in {"loss": part_loss, "d2s": part_d2s, "step": part_step}[args.part](args.rounds):
            print(line, flush=True)
        return
    lines = [f"device {torch.cuda.get_device_name(0)}; HIP events around windows of launches, median (min .. max) of {args.rounds} rounds; a fresh process per part"]
    for part in PARTS:
        proc = subprocess.run([sys.executable, __file__, "--part", part, "--rounds", str(args.rounds)], capture_output=True, text=True, timeout=900)
        if proc.returncode != 0:
            raise SystemExit(f"part {part} failed ({proc.returncode}):\n{proc.stdout[-2000:]}\n{proc.stderr[-2000:]}")
        lines += proc.stdout.strip().splitlines()
    print("\n".join(lines))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
