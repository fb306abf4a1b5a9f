"""SwinBlock forward + backward (train mode, bf16 autocast) with the fused MLP kernels of csrc/swin_mlp.hip against the unfused path, per width.

Same process, device events, warm-up first, the two sides alternating ROUNDS times; a side's figure per round is the median of REPS
forward + backward passes, the spread of a side is max - min of its round medians.  Sides: ops.HOOKS["fused_swin_mlp"] on / off (off = LayerNorm +
the two token GEMMs, the path of the commit before the 128 / 384 kernels).  Every width is routed for the measurement, whatever
ops/blocks.py routes in the model.  Writes profiles/swin_mlp_widths.txt (or the path given as the first argument)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from improving_yolov8_cbam_swinblock_amd import ops  # noqa: E402
from improving_yolov8_cbam_swinblock_amd.nn.modules import SwinBlock  # noqa: E402
from improving_yolov8_cbam_swinblock_amd.ops import blocks  # noqa: E402

ROUNDS, REPS, WARMUP = 5, 10, 5
# (C, batch, map side): 7 x 7 windows pad 80 -> 84 and 40 -> 42, so T = batch * 84^2 or batch * 42^2
SHAPES = [(384, 16, 80, "yolov8m-cbam-swin384 at batch 16, 1280^2: T = 112,896, hidden 1536"),
          (128, 32, 40, "the n-scale width at the s config's token count: T = 56,448, hidden 512"),
          (256, 32, 40, "control, yolov8s-cbam-swin at batch 32, 640^2: T = 56,448, hidden 1024 (profiles/r05_swin_mlp_fused.txt)")]


def measure(c, n, side):
    dev = torch.device("cuda:0")
    torch.manual_seed(c)
    m = SwinBlock(c, 2, 7).to(dev).train()
    x = torch.randn(n, c, side, side, device=dev).requires_grad_(True)
    wgt = torch.randn(n, c, side, side, device=dev)

    def step(fused):
        ops.HOOKS["fused_swin_mlp"] = fused
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(x)
        torch.autograd.grad((y.float() * wgt).sum(), [x] + list(m.parameters()))

    def median_ms(fused):
        e0 = [torch.cuda.Event(enable_timing=True) for _ in range(REPS)]
        e1 = [torch.cuda.Event(enable_timing=True) for _ in range(REPS)]
        for i in range(REPS):
            e0[i].record()
            step(fused)
            e1[i].record()
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in zip(e0, e1))
        return ts[len(ts) // 2]

    for _ in range(WARMUP):
        step(True)
        step(False)
    torch.cuda.synchronize()
    rounds = {True: [], False: []}
    for _ in range(ROUNDS):
        for fused in (True, False):
            rounds[fused].append(median_ms(fused))
    return rounds


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "swin_mlp_widths.txt")
    old, routed = ops.HOOKS["fused_swin_mlp"], blocks.FUSED_SWIN_MLP_WIDTHS
    blocks.FUSED_SWIN_MLP_WIDTHS = (128, 256, 384)
    lines = ["# SwinBlock(C, 2 heads, 7 x 7 windows) forward + backward, train mode, bf16 autocast, one MI355X: the fused MLP kernels (csrc/swin_mlp.hip)",
             "# against the unfused path (LayerNorm + two token GEMMs; HOOKS[\"fused_swin_mlp\"] = False).  tools/probes/swin_mlp_widths.py: one process,",
             f"# device events, {WARMUP} warm-up passes per side, then fused / unfused alternating {ROUNDS} times; a round's figure is the median of {REPS} passes (ms).",
             "# spread = max - min of a side's round medians; a width is routed in ops/blocks.py only if unfused - fused (medians of the rounds) exceeds",
             "# the larger spread of the two sides.  The whole block is timed (attention and both LayerNorms included), so the difference is the MLP's.",
             "#"]
    try:
        for c, n, side, what in SHAPES:
            r = measure(c, n, side)
            med = {k: sorted(v)[len(v) // 2] for k, v in r.items()}
            spread = {k: max(v) - min(v) for k, v in r.items()}
            gain = med[False] - med[True]
            noise = max(spread.values())
            verdict = "fused faster beyond the spread: routed" if gain > noise else "not faster beyond the spread: NOT routed"
            lines += [f"C = {c}  input [{n}, {c}, {side}, {side}]  ({what})",
                      "  fused    rounds " + " ".join(f"{v:.3f}" for v in r[True]) + f"   median {med[True]:.3f}  spread {spread[True]:.3f}",
                      "  unfused  rounds " + " ".join(f"{v:.3f}" for v in r[False]) + f"   median {med[False]:.3f}  spread {spread[False]:.3f}",
                      f"  unfused - fused = {gain:+.3f} ms ({100 * gain / med[False]:+.1f} % of the unfused block), noise {noise:.3f} ms: {verdict}"]
            print("\n".join(lines[-4:]), flush=True)
    finally:
        ops.HOOKS["fused_swin_mlp"], blocks.FUSED_SWIN_MLP_WIDTHS = old, routed
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
