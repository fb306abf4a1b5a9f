"""Time the SPPF pool cascade where the TILED kernels run, and digest its results, for two builds of the library (not a test).

    python tools/probes/pool_tiled_probe.py --parent-lib PATH/libyolo_mi355.so [--pairs 3] [--reps 100] [--out FILE]

bench.py's model has 20x20 SPPF maps, which the whole-map kernels serve; the tiled kernels (forward above 4800 pixels in bf16,
backward above 1920) are the path of large-image training and appear in no bench record.  Every measurement is a fresh child process
(the library is chosen at import: YMI_LIB), parent build (A) and this tree's build (B) alternating A B A B:
  - `ops.sppf_pool_cat` forward + backward at (1, 512, 60, 60) and (1, 256, 96, 96), bf16, k = 5, and - the whole-map kernels with a
    run-time k - at (8, 256, 20, 20) bf16 k = 9 and (2, 64, 40, 40) float32 k = 3, on NHWC operands (no layout conversion in the
    timed region): device events around each repetition, `reps` (>= 50) repetitions after 20 warm-up ones;
  - sha256 of the concat and of dx for these and for the map / tiled threshold shapes, on seeded random (not dyadic) inputs, so a
    changed low bit in any form shows as a changed digest.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve()
ROOT = HERE.parents[2]
TIMED = [(5, (1, 512, 60, 60), "bfloat16"), (5, (1, 256, 96, 96), "bfloat16"), (9, (8, 256, 20, 20), "bfloat16"), (3, (2, 64, 40, 40), "float32")]
DIGEST = TIMED + [(5, (8, 256, 20, 20), "bfloat16"), (7, (4, 64, 20, 20), "bfloat16"), (5, (2, 64, 40, 40), "bfloat16"), (9, (2, 8, 13, 17), "float32"),
                  (5, (2, 64, 40, 40), "float32"), (3, (1, 16, 64, 64), "float32"), (3, (1, 16, 96, 96), "float32"), (5, (1, 16, 48, 48), "bfloat16"),
                  (3, (1, 40, 72, 72), "bfloat16"), (9, (1, 8, 56, 56), "float32"), (11, (1, 24, 50, 70), "bfloat16")]


def child(reps):
    sys.path.insert(0, str(ROOT))
    import torch

    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd._lib import empty_nhwc

    dev = torch.device("cuda:0")

    def operands(k, shape, dtype):
        n, c, h, w = shape
        g = torch.Generator().manual_seed(k + c + h)
        x = empty_nhwc(n, c, h, w, dtype, dev)
        x.copy_(torch.randn(shape, generator=g))
        gy = empty_nhwc(n, 4 * c, h, w, dtype, dev)
        gy.copy_(torch.randn((n, 4 * c, h, w), generator=g))
        return x.requires_grad_(True), gy

    def digest(t):
        return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]

    out = {"timed": {}, "digest": {}}
    for k, shape, dt in DIGEST:
        x, gy = operands(k, shape, getattr(torch, dt))
        cat = ops.sppf_pool_cat(x, k)
        (dx,) = torch.autograd.grad(cat, x, gy)
        out["digest"][f"k{k} {shape} {dt}"] = digest(cat) + " " + digest(dx)
    for k, shape, dt in TIMED:
        x, gy = operands(k, shape, getattr(torch, dt))

        def once():
            torch.autograd.grad(ops.sppf_pool_cat(x, k), x, gy)

        for _ in range(20):
            once()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            once()
            b.record()
        torch.cuda.synchronize()
        us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        out["timed"][f"k{k} {shape} {dt}"] = {"median": statistics.median(us), "p10": us[len(us) // 10], "p90": us[len(us) * 9 // 10], "min": us[0], "n": len(us)}
    print("RESULT " + json.dumps(out), flush=True)


def run_child(lib, reps):
    env = dict(os.environ)
    env.pop("YMI_LIB", None)
    if lib:
        env["YMI_LIB"] = lib
    proc = subprocess.run([sys.executable, str(HERE), "--child", "--reps", str(reps)], capture_output=True, text=True, timeout=300, env=env)
    for line in proc.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"child with library {lib or 'of this tree'} failed ({proc.returncode}):\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(max(args.reps, 50))
    if not args.parent_lib:
        raise SystemExit("pool_tiled_probe compares two builds: give --parent-lib; nothing measured")
    lines = [f"ops.sppf_pool_cat forward + backward, device events per repetition, {max(args.reps, 50)} repetitions after 20 warm-up; A = {args.parent_lib}, B = this tree's library; "
             "one child process per run, alternating"]
    meds, digests = {}, {"A": None, "B": None}
    for r in range(args.pairs):
        for tag, lib in (("A", args.parent_lib), ("B", "")):
            res = run_child(lib, args.reps)
            for name, t in res["timed"].items():
                meds.setdefault(name, {"A": [], "B": []})[tag].append(t["median"])
                lines.append(f"run {2 * r + (tag == 'B') + 1} {tag} {name}: median {t['median']:.1f} us  p10 {t['p10']:.1f}  p90 {t['p90']:.1f}  min {t['min']:.1f}  (n {t['n']})")
            if digests[tag] is None:
                digests[tag] = res["digest"]
            elif digests[tag] != res["digest"]:
                lines.append(f"run {tag}: digests differ from the first {tag} run (not deterministic)")
    for name, m in meds.items():
        lines.append(f"{name}: A medians {min(m['A']):.1f} .. {max(m['A']):.1f} us, B medians {min(m['B']):.1f} .. {max(m['B']):.1f} us; "
                     f"B inside A's range: {all(min(m['A']) <= v <= max(m['A']) for v in m['B'])}")
    for name in digests["A"]:
        same = digests["A"][name] == digests["B"][name]
        lines.append(f"digest {name}: cat+dx {'identical' if same else 'DIFFER'} ({digests['A'][name]}{'' if same else ' | ' + digests['B'][name]})")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
