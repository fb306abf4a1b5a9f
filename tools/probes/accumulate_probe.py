"""Time gradient accumulation around the captured training step on one MI355X (not a test; bench.py does not read it).

    python tools/probes/accumulate_probe.py [--parent DIR] [--out profiles/accumulate_probe.txt] [--steps 60] [--rounds 2]

Workload: yolov8s.yaml (bench.py's model), nc 1, batch 32, 640^2, bf16, TrainStep(graph=True), warmed up; device events around every step,
`steps` (>= 50) steps per measurement.  Every measurement is a fresh child process of this script, so two source trees can be compared.
  (i)  the plain captured step (update= never passed) of this tree and of the parent commit's tree (--parent DIR: a checkout of the parent
       with its library built), alternating A B A B in this one command; median and spread of each.  They should agree within the spread:
       the default path launches what the parent launches.  Without --parent: "not measured".
  (ii) on this tree, no pass mark: a micro-step (update=False) beside a full step; an updating step with one micro-step pending (micro
       graph + update graph); the fold launch (FusedSGD.accumulate over the model's own gradients) alone.
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve()
ROOT = HERE.parents[2]


def summary(ms):
    ms = sorted(ms)
    return {"median": statistics.median(ms), "min": ms[0], "max": ms[-1], "p10": ms[len(ms) // 10], "p90": ms[len(ms) * 9 // 10], "n": len(ms)}


def child(args):
    sys.path.insert(0, args.root)
    import torch

    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = DetectionModel("yolov8s.yaml", ch=3, nc=1).to(dev)
    step = TrainStep(model, world_size=1, graph=True)
    batch = synthetic_batch(32, 640, dev, 1)

    def timed(fn, n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    for _ in range(10):
        step(batch)
    torch.cuda.synchronize()
    out = {"full": summary(timed(lambda: step(batch), args.steps))}
    if args.child == "accumulate":
        for _ in range(3):  # the first pair captures the micro and the update graph
            step(batch, update=False)
            step(batch)
        torch.cuda.synchronize()
        micro, upd = [], []
        for _ in range(args.steps):
            micro += timed(lambda: step(batch, update=False), 1)
            upd += timed(lambda: step(batch), 1)
        out["micro"], out["update_after_one_micro"] = summary(micro), summary(upd)
        out["full_again"] = summary(timed(lambda: step(batch), args.steps))
        grads = {p: torch.randn_like(p) for p in step.opt.params if p.requires_grad}
        step.opt.accumulate(grads)
        out["fold"] = summary(timed(lambda: step.opt.accumulate(grads), args.steps))
        step.opt.discard_pending()
        out["fold_bytes"] = 12 * sum(g.numel() for g in grads.values())
    print("RESULT " + json.dumps(out), flush=True)


def run_child(kind, root, steps):
    proc = subprocess.run([sys.executable, str(HERE), "--child", kind, "--root", str(root), "--steps", str(steps)], capture_output=True, text=True, timeout=900)
    for line in proc.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"child {kind} on {root} failed ({proc.returncode}):\n{proc.stdout[-2000:]}\n{proc.stderr[-4000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", default="")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("accumulate_probe measures on the MI355X: no GPU here, nothing measured")
    lines = [f"device {torch.cuda.get_device_name(0)}; yolov8s.yaml nc 1, batch 32, 640^2, bf16, TrainStep(graph=True); device events per step, {args.steps} steps per measurement, "
             "one child process per measurement"]

    def report(s):
        lines.append(s)
        print(s, flush=True)

    fmt = lambda r: f"median {r['median']:7.3f} ms  p10 {r['p10']:7.3f}  p90 {r['p90']:7.3f}  min {r['min']:7.3f}  max {r['max']:7.3f}  (n {r['n']})"  # noqa: E731
    report("(i) plain captured step, this tree (B) against the parent commit (A), alternating:")
    if args.parent:
        meds = {"A": [], "B": []}
        for r in range(args.rounds):
            for tag, root in (("A", args.parent), ("B", ROOT)):
                res = run_child("plain", root, args.steps)["full"]
                meds[tag].append(res["median"])
                report(f"    round {r} {tag} {'parent' if tag == 'A' else 'branch'}: {fmt(res)}")
        a, b = statistics.mean(meds["A"]), statistics.mean(meds["B"])
        report(f"    medians A {['%.3f' % v for v in meds['A']]} B {['%.3f' % v for v in meds['B']]}: branch - parent = {b - a:+.3f} ms ({(b - a) / a * 100:+.2f} %); "
               f"run-to-run spread of a tree's medians A {max(meds['A']) - min(meds['A']):.3f} B {max(meds['B']) - min(meds['B']):.3f} ms")
    else:
        report("    not measured (no --parent tree given)")
    res = run_child("accumulate", ROOT, args.steps)
    report("(ii) accumulation on this tree (no pass mark):")
    report(f"    full step (nothing pending)                 : {fmt(res['full'])}")
    report(f"    micro-step (update=False: micro graph)      : {fmt(res['micro'])}")
    report(f"    updating step, one micro-step pending       : {fmt(res['update_after_one_micro'])}   (micro graph + update graph)")
    report(f"    full step again, after the graphs exist     : {fmt(res['full_again'])}")
    gbs = res["fold_bytes"] / (res["fold"]["median"] * 1e-3) / 1e9
    report(f"    fold launch alone (eager, {res['fold_bytes'] / 1e6:.1f} MB moved)    : {fmt(res['fold'])}   = {gbs:.0f} GB/s, includes the host's launch set-up")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
