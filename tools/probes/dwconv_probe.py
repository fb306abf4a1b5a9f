"""Time the depthwise convolution kernels (csrc/dwconv.hip) on one MI355X (not a test; bench.py does not read it).

    python tools/probes/dwconv_probe.py [--out profiles/dwconv_probe.txt] [--rounds 5] [--no-step]

The depthwise layers of yolov8s-ghost at batch 32, 640 x 640 are 5x5 stride 1 on (channels / map side) 32/160, 8/160, 16/160, 64/80, 16/80,
32/80, 128/40, 256/20.  Per shape, in bfloat16, through the C ABI: the forward in its training form (raw output + statistics rows), the data
gradient and the weight gradient, and beside each the existing ymi_scale_shift_act on a tensor of the same shape - it reads one tensor and
writes one, the bytes the forward must move, so it is the yardstick a streaming kernel of this library is held to.  HIP events around windows
of WINDOW launches; `rounds` rounds in which the four kernels alternate; medians and spreads (min .. max) over the rounds.  No ratio is fixed
in advance: the file states what was found.  Last: one TrainStep(graph=True) step of yolov8s-ghost beside yolov8s-stock at the same batch.
"""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

SHAPES = [(32, 160), (8, 160), (16, 160), (64, 80), (16, 80), (32, 80), (128, 40), (256, 20)]
BATCH, K, STRIDE, WINDOW = 32, 5, 1, 20


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(WINDOW):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / WINDOW * 1e3  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-batch", type=int, default=BATCH)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_probe measures on the MI355X: no GPU here, nothing measured")

    from improving_yolov8_cbam_swinblock_amd._lib import as_ymi, check, empty_nhwc, lib, ptr, stream_ptr

    L, dev, dt = lib(), torch.device("cuda:0"), torch.bfloat16
    lines = [f"device {torch.cuda.get_device_name(0)}; batch {BATCH}, {K}x{K} stride {STRIDE} depthwise, bfloat16; HIP events, windows of {WINDOW} launches, "
             f"median (min .. max) of {args.rounds} rounds, microseconds per launch",
             f"{'C / HxW':<12}{'MB (read + write)':>18}  {'forward + statistics':>26}  {'data gradient':>26}  {'weight gradient (2 launches)':>30}  "
             f"{'ymi_scale_shift_act':>26}   forward / yardstick"]
    by = ctypes.byref
    for c, hw in SHAPES:
        g = torch.Generator().manual_seed(c * 1000 + hw)
        x, y, dy, dx = (empty_nhwc(BATCH, c, hw, hw, dt, dev) for _ in range(4))
        x.copy_(torch.randn(BATCH, c, hw, hw, generator=g))
        dy.copy_(torch.randn(BATCH, c, hw, hw, generator=g))
        w = (torch.randn(c, 1, K, K, generator=g) / K).to(dev)
        dw = torch.empty_like(w)
        scale, shift = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        part = torch.empty(int(L.ymi_dwconv2d_stat_blocks(BATCH, hw, hw, c)) * 2 * c, device=dev)
        blocks = ctypes.c_int64(0)
        need = int(L.ymi_dwconv2d_bwd_weight_workspace(BATCH, hw, hw, c, K))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        tx, ty, tdy, tdx = as_ymi(x), as_ymi(y), as_ymi(dy), as_ymi(dx)
        fns = {
            "fwd": lambda: check(L.ymi_dwconv2d_fwd(by(tx), ptr(w), K, STRIDE, None, None, 0, None, by(ty), ptr(part), by(blocks), stream_ptr()), "fwd"),
            "dgrad": lambda: check(L.ymi_dwconv2d_bwd_data(by(tdy), ptr(w), K, STRIDE, None, by(tdx), stream_ptr()), "dgrad"),
            "wgrad": lambda: check(L.ymi_dwconv2d_bwd_weight(by(tx), by(tdy), K, STRIDE, ptr(dw), ptr(ws), need, stream_ptr()), "wgrad"),
            "ssa": lambda: check(L.ymi_scale_shift_act(by(tx), ptr(scale), ptr(shift), 1, None, by(ty), stream_ptr()), "ssa"),
        }
        for fn in fns.values():  # warm every shape before it is timed
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                times[k].append(window(fn))
        cell = lambda k: f"{statistics.median(times[k]):8.1f} ({min(times[k]):7.1f} .. {max(times[k]):7.1f})"  # noqa: E731
        mb = 2 * x.numel() * 2 / 1e6
        s = (f"{f'{c} / {hw}x{hw}':<12}{mb:>18.1f}  {cell('fwd'):>26}  {cell('dgrad'):>26}  {cell('wgrad'):>30}  {cell('ssa'):>26}   "
             f"{statistics.median(times['fwd']) / statistics.median(times['ssa']):.2f}")
        lines.append(s)
        print(s, flush=True)
        del x, y, dy, dx, ws, part

    if not args.no_step:
        from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
        from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

        for name in ("yolov8s-ghost.yaml", "yolov8s-stock.yaml"):
            torch.manual_seed(0)
            model = DetectionModel(name, ch=3, nc=1).to(dev)
            step = TrainStep(model, world_size=1, lr=0.01, graph=True)
            batch = synthetic_batch(args.step_batch, 640, dev, 1)
            for _ in range(3):  # the warm-up steps, the capture and two replays
                step(batch)
            torch.cuda.synchronize()
            ts = []
            for _ in range(args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(5):
                    step(batch)
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) / 5)
            s = (f"TrainStep(graph=True) {name:<20} batch {args.step_batch}, 640 x 640, bfloat16: {statistics.median(ts):8.2f} ms per step "
                 f"({min(ts):.2f} .. {max(ts):.2f}), windows of 5 steps, {args.rounds} rounds")
            lines.append(s)
            print(s, flush=True)
            del step, model, batch
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
