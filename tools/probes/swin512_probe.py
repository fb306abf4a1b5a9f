"""Time window attention at head_dim 256 (csrc/swin.hip ymi_window_attention_fwd / _bwd, the 16-tile instantiations) and the training step of
yolo11m-cbam-swin on one MI355X (not a test; bench.py does not read it).

    python tools/probes/swin512_probe.py [--out profiles/swin512_probe.txt] [--repeats 3] [--rounds 5] [--no-step] [--no-sdpa]

SwinBlock(512, 2) on the P4 map of batch 32 at 640 x 640: 40 x 40 padded to 42 x 42, 36 windows of 49 tokens per image, T = 56,448 tokens,
C = 512, 2 heads of 256 - 2,304 workgroups per launch.  In bfloat16 (the tr kernels) and float32 (the tiled kernels: one launch forward, two
backward), through the C ABI.  Beside them, for orientation only, torch's scaled_dot_product_attention forward and backward on contiguous
[windows, heads, 49, 256] operands (it does not read the packed qkv rows).  Then one TrainStep(graph=True) step of yolo11m-cbam-swin beside
the stock yolo11m, both in the same process.

Every measurement runs in a fresh child process, `repeats` times: a child warms its shapes, times `rounds` windows of WINDOW launches (or of 5
steps) with HIP events in which the kernels alternate, and reports its median; the file states the median over the children and the spread
(min .. max) of the children's medians.  These are new shapes: no threshold is fixed in advance, the file states what was found."""
import argparse
import ctypes
import json
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

BATCH, SIDE, WS, C, HEADS, WINDOW = 32, 42, 7, 512, 2, 20
L = WS * WS
T = BATCH * SIDE * SIDE
MODELS = ("yolo11m-cbam-swin.yaml", "yolo11m.yaml")


def window(fn, n=WINDOW):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def child_attention(dtype_name, rounds, sdpa):
    from improving_yolov8_cbam_swinblock_amd._lib import as_ymi, check, lib, ptr, stream_ptr

    lb, dev, dt = lib(), torch.device("cuda:0"), getattr(torch, dtype_name)
    by = ctypes.byref
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(T, 3 * C, generator=g).to(dt).to(dev)
    dout = torch.randn(T, C, generator=g).to(dt).to(dev)
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
    lse = torch.empty(T, HEADS, dtype=torch.float32, device=dev)
    tq, to, tdo, tdq = (as_ymi(t) for t in (qkv, out, dout, dqkv))
    fns = {
        "fwd": lambda: check(lb.ymi_window_attention_fwd(by(tq), L, HEADS, by(to), ptr(lse), stream_ptr()), "fwd"),
        "bwd": lambda: check(lb.ymi_window_attention_bwd(by(tq), by(to), by(tdo), ptr(lse), L, HEADS, by(tdq), stream_ptr()), "bwd"),
    }
    if sdpa:
        q, k, v = (torch.randn(T // L, HEADS, L, C // HEADS, generator=g).to(dt).to(dev).requires_grad_(True) for _ in range(3))
        go = torch.randn(T // L, HEADS, L, C // HEADS, generator=g).to(dt).to(dev)
        held = {}

        def sdpa_fwd():
            held["o"] = torch.nn.functional.scaled_dot_product_attention(q, k, v)

        def sdpa_bwd():
            torch.autograd.grad(held["o"], (q, k, v), go, retain_graph=True)

        fns["sdpa_fwd"], fns["sdpa_bwd"] = sdpa_fwd, sdpa_bwd
    for fn in fns.values():  # warm every shape before it is timed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k_: [] for k_ in fns}
    for _ in range(rounds):
        for k_, fn in fns.items():
            times[k_].append(window(fn) * 1e3)  # us per call
    return {k_: statistics.median(v) for k_, v in times.items()}


def child_step(rounds, batch_size):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    dev, out = torch.device("cuda:0"), {}
    for name in MODELS:
        torch.manual_seed(0)
        model = DetectionModel(name, ch=3, nc=1).to(dev)
        step = TrainStep(model, world_size=1, lr=0.01, graph=True)
        batch = synthetic_batch(batch_size, 640, dev, 1)
        for _ in range(6):  # the warm-up steps, the capture and replays
            step(batch)
        torch.cuda.synchronize()
        out[name] = statistics.median(window(lambda: step(batch), 5) for _ in range(rounds))  # ms per step
        del step, model, batch
        torch.cuda.empty_cache()
    return out


def run_children(kind, repeats, extra):
    """`repeats` fresh processes of one measurement -> {key: [each child's median]}"""
    acc = {}
    for _ in range(repeats):
        p = subprocess.run([sys.executable, __file__, "--child", kind] + extra, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit(f"child {kind} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        for k_, v in json.loads(p.stdout.strip().splitlines()[-1]).items():
            acc.setdefault(k_, []).append(v)
    return acc


def cell(acc, key, fmt="8.1f"):
    if key not in acc:
        return "not run"
    v = acc[key]
    return f"{statistics.median(v):{fmt}} ({min(v):{fmt}} .. {max(v):{fmt}})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--step-batch", type=int, default=BATCH)
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swin512_probe measures on the MI355X: no GPU here, nothing measured")
    if args.child:
        kind = args.child
        res = child_step(args.rounds, args.step_batch) if kind == "step" else child_attention(kind, args.rounds, not args.no_sdpa)
        print(json.dumps(res), flush=True)
        return

    extra = ["--rounds", str(args.rounds), "--step-batch", str(args.step_batch)] + (["--no-sdpa"] if args.no_sdpa else [])
    lines = [f"device {torch.cuda.get_device_name(0)}; window attention T {T} (batch {BATCH}, {SIDE} x {SIDE} padded map), C {C}, {HEADS} heads of {C // HEADS}, "
             f"{L}-token windows, {T // L * HEADS} workgroups per launch",
             f"HIP events, windows of {WINDOW} launches, {args.rounds} rounds per process; median (min .. max) over {args.repeats} fresh processes of the "
             f"process medians, microseconds per call",
             f"{'dtype':<10}{'ymi_window_attention_fwd':>30}  {'ymi_window_attention_bwd':>30}  {'torch SDPA forward':>30}  {'torch SDPA backward':>30}"]
    for dtype_name, form in (("bfloat16", "tr"), ("float32", "tiled")):
        acc = run_children(dtype_name, args.repeats, extra)
        s = f"{dtype_name:<10}{cell(acc, 'fwd'):>30}  {cell(acc, 'bwd'):>30}  {cell(acc, 'sdpa_fwd'):>30}  {cell(acc, 'sdpa_bwd'):>30}   [{form} kernels]"
        lines.append(s)
        print(s, flush=True)
    if not args.no_step:
        acc = run_children("step", args.repeats, extra)
        for name in MODELS:
            s = (f"TrainStep(graph=True) {name:<24} batch {args.step_batch}, 640 x 640, bfloat16: {cell(acc, name, '8.2f')} ms per step, windows of 5 steps, "
                 f"{args.rounds} rounds per process, {args.repeats} processes (both models in each process)")
            lines.append(s)
            print(s, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
