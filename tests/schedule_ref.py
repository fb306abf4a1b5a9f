"""A separate restatement of the reference trainer's schedule, written as the reference writes it: ONE loop over epochs and batches that
carries `accumulate`, the group learning rates, the momentum and `last_opt_step` as the trainer's attributes do (reference
engine/trainer.py:216-219 scheduler, :305-306 accumulate and weight decay, :330 nw, :352 scheduler.step(), :370-380 warm-up, :397-399 update
rule).  engine.trainer.WarmupSchedule computes each iteration from (epoch, i) instead; tests/test_schedule_cpu.py compares the two."""
import math

import numpy as np


def run(epochs, nb, batch, nbs=64, lr0=0.01, lrf=0.01, momentum=0.937, weight_decay=5e-4, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1,
        cos_lr=False, has_momentum=True):
    """-> (nw, scaled weight decay, [per iteration: dict(ni, accumulate, lrs, momentum, update)])"""
    if cos_lr:
        lf = lambda x: max((1 - math.cos(x * math.pi / epochs)) / 2, 0) * (lrf - 1) + 1  # noqa: E731  one_cycle(1, lrf, epochs)
    else:
        lf = lambda x: max(1 - x / epochs, 0) * (1.0 - lrf) + lrf  # noqa: E731
    accumulate = max(round(nbs / batch), 1)
    decay = weight_decay * batch * accumulate / nbs
    groups = [{"lr": lr0, "initial_lr": lr0} for _ in range(3)]
    if has_momentum:
        for g in groups:
            g["momentum"] = momentum
    nw = max(round(warmup_epochs * nb), 100) if warmup_epochs > 0 else -1
    last_opt_step = -1
    rows = []
    for epoch in range(epochs):
        for g in groups:  # scheduler.step(): LambdaLR
            g["lr"] = g["initial_lr"] * lf(epoch)
        for i in range(nb):
            ni = i + nb * epoch
            if ni <= nw:
                xi = [0, nw]
                accumulate = max(1, int(np.interp(ni, xi, [1, nbs / batch]).round()))
                for j, x in enumerate(groups):
                    x["lr"] = np.interp(ni, xi, [warmup_bias_lr if j == 0 else 0.0, x["initial_lr"] * lf(epoch)])
                    if "momentum" in x:
                        x["momentum"] = np.interp(ni, xi, [warmup_momentum, momentum])
            update = ni - last_opt_step >= accumulate
            if update:
                last_opt_step = ni
            rows.append({"ni": ni, "accumulate": accumulate, "lrs": [float(g["lr"]) for g in groups],
                         "momentum": float(groups[0]["momentum"]) if has_momentum else None, "update": update})
    return nw, decay, rows
