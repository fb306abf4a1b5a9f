"""Time the PSA attention kernels (csrc/swin.hip ymi_psa_attention_fwd / _bwd) and the YOLO11 training step on one MI355X (not a test;
bench.py does not read it).

    python tools/probes/psa_probe.py [--out profiles/psa_probe.txt] [--rounds 5] [--no-step] [--no-sdpa]

C2PSA's attention at batch 32, 640 x 640 is a 20 x 20 map: L = 400 tokens per image, head_dim 64, key_dim 32, 2 heads at scale n and 4 at scale
s.  Per shape, in bfloat16, through the C ABI: the forward (with v_out) and the backward (two launches: dQ, then dK / dV with dv_add).  Beside
them, for orientation only, torch's scaled_dot_product_attention forward and backward on the same shapes (q, k of width 32, v of width 64,
contiguous [B, heads, L, d] operands: it does not read the packed layout and writes no v_out).  HIP events around windows of WINDOW launches;
`rounds` rounds in which the kernels alternate; medians and spreads (min .. max) over the rounds.  Last: one TrainStep(graph=True) step of
yolo11n and yolo11s beside yolov8s-stock at the same batch.  No threshold is fixed in advance: the file states what was found.
"""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

BATCH, TOKENS, KD, HD, WINDOW = 32, 400, 32, 64, 20
HEADS = (2, 4)


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
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--step-batch", type=int, default=BATCH)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("psa_probe measures on the MI355X: no GPU here, nothing measured")

    from improving_yolov8_cbam_swinblock_amd._lib import as_ymi, check, lib, ptr, stream_ptr

    L, dev, dt = lib(), torch.device("cuda:0"), torch.bfloat16
    lines = [f"device {torch.cuda.get_device_name(0)}; batch {BATCH}, {TOKENS} tokens per image, key_dim {KD}, head_dim {HD}, bfloat16; HIP events, windows of "
             f"{WINDOW} launches, median (min .. max) of {args.rounds} rounds, microseconds per call",
             f"{'heads':<6}{'ymi_psa_attention_fwd':>30}  {'ymi_psa_attention_bwd (2 launches)':>36}  {'torch SDPA forward':>30}  {'torch SDPA backward':>30}"]
    by = ctypes.byref
    for heads in HEADS:
        g = torch.Generator().manual_seed(heads)
        T = BATCH * TOKENS
        qkv = torch.randn(T, heads * (2 * KD + HD), generator=g).to(dt).to(dev)
        dout, dv_add = (torch.randn(T, heads * HD, generator=g).to(dt).to(dev) for _ in range(2))
        out, v_out, dqkv = torch.empty_like(dout), torch.empty_like(dout), torch.empty_like(qkv)
        lse = torch.empty(T, heads, dtype=torch.float32, device=dev)
        tq, to, tv, tdo, tda, tdq = (as_ymi(t) for t in (qkv, out, v_out, dout, dv_add, dqkv))
        fns = {
            "fwd": lambda: check(L.ymi_psa_attention_fwd(by(tq), TOKENS, heads, KD, by(to), by(tv), ptr(lse), stream_ptr()), "fwd"),
            "bwd": lambda: check(L.ymi_psa_attention_bwd(by(tq), by(to), by(tdo), ptr(lse), by(tda), TOKENS, heads, KD, by(tdq), stream_ptr()), "bwd"),
        }
        if not args.no_sdpa:
            q, k = (torch.randn(BATCH, heads, TOKENS, KD, generator=g).to(dt).to(dev).requires_grad_(True) for _ in range(2))
            v = torch.randn(BATCH, heads, TOKENS, HD, generator=g).to(dt).to(dev).requires_grad_(True)
            go = torch.randn(BATCH, heads, TOKENS, HD, generator=g).to(dt).to(dev)
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
        for _ in range(args.rounds):
            for k_, fn in fns.items():
                times[k_].append(window(fn))
        cell = lambda k_: f"{statistics.median(times[k_]):8.1f} ({min(times[k_]):7.1f} .. {max(times[k_]):7.1f})" if k_ in times else "not run"  # noqa: E731
        s = f"{heads:<6}{cell('fwd'):>30}  {cell('bwd'):>36}  {cell('sdpa_fwd'):>30}  {cell('sdpa_bwd'):>30}"
        lines.append(s)
        print(s, flush=True)

    if not args.no_step:
        from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
        from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

        for name in ("yolo11n.yaml", "yolo11s.yaml", "yolov8s-stock.yaml"):
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
