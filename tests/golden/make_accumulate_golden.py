"""Generate tests/golden/accumulate_tiny.* by running the REAL reference trainer code on CPU, float32, the way make_golden.py records
opt_step_tiny (cv2 stubbed): gradient accumulation as the reference does it (engine/trainer.py:394-399) - backward() on batch A, backward()
on batch B with AccumulateGrad summing into .grad, then ONE optimizer_step (clip on the summed gradient, SGD step, zero_grad, EMA update,
:614-622) - twice: (A, B, step), (A, B, step).

    python tests/golden/make_accumulate_golden.py

Stored (data only; accumulate_tiny.npz holds the batches and the first update, accumulate_tiny.s1.npz the second): the two seeded 2-image batches, the total gradient norm clip_grad_norm_ returned at each update, the loss of every backward,
and strided samples + norms of every parameter / EMA entry after each update (the model's initial weights are e2e_tiny's)."""
import json
import sys
from types import SimpleNamespace

import numpy as np
import torch

from make_golden import OUT, REPO, import_reference_package, save


def seeded_batch(seed, B=2, S=64, nb=3):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8).float() / 255  # 8-bit grey levels: stored as uint8 ("<tag>.img_u8")
    ctr = torch.rand(B * nb, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(B * nb, 2, generator=g) * 0.3 + 0.05
    return {"img": img, "batch_idx": torch.arange(B).repeat_interleave(nb).float(), "cls": torch.zeros(B * nb, 1), "bboxes": torch.cat((ctr, wh), 1)}


def main():
    sys.path.insert(0, str(REPO / "tests"))
    from golden_weights import grad_record

    tasks = import_reference_package()
    from ultralytics.engine.trainer import BaseTrainer
    from ultralytics.utils.loss import v8DetectionLoss
    from ultralytics.utils.torch_utils import ModelEMA

    torch.set_num_threads(4)
    d = json.loads((OUT / "e2e_tiny_seed7_yaml.json").read_text())
    z = np.load(OUT / "e2e_tiny_seed7.npz")
    torch.manual_seed(7)
    model = tasks.DetectionModel(d, ch=3, nc=1, verbose=False)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w.")}, strict=True)
    model.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5)
    for k, v in model.named_parameters():  # trainer.py:244-256: '.dfl' is always frozen
        if ".dfl" in k:
            v.requires_grad = False
    fake = SimpleNamespace(args=SimpleNamespace(lr0=0.01, momentum=0.937, warmup_bias_lr=0.1), data={"nc": 1})
    opt = BaseTrainer.build_optimizer(fake, model, name="SGD", lr=0.01, momentum=0.937, decay=5e-4)
    ema = ModelEMA(model)
    batches = {"A": seeded_batch(101), "B": seeded_batch(202)}
    names = {id(p): n for n, p in model.named_parameters()}
    arrays = {f"{tag}.{k}": v.numpy() for tag, b in batches.items() for k, v in b.items() if k != "img"}
    arrays.update({f"{tag}.img_u8": (b["img"] * 255).round().to(torch.uint8).numpy() for tag, b in batches.items()})
    meta = {"groups": [[names[id(p)] for p in g["params"]] for g in opt.param_groups], "norms": [], "loss": [], "optimizer": type(opt).__name__,
            "calls": [["A", False], ["B", True], ["A", False], ["B", True]]}
    model.train()
    crit = v8DetectionLoss(model)
    opt.zero_grad()  # trainer.py:346
    for step in range(2):
        for tag in ("A", "B"):
            b = batches[tag]
            loss, items = crit(model(b["img"]), b)
            loss.sum().backward()  # the second backward ACCUMULATES into .grad
            meta["loss"].append([float(v) for v in loss])
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=10.0)  # trainer.py:617, on the accumulated gradient
        opt.step()
        opt.zero_grad()
        ema.update(model)
        meta["norms"].append(float(norm))
        for n, p in model.state_dict().items():
            if p.dtype.is_floating_point:
                for kind, v in grad_record(p).items():
                    arrays[f"s{step}.p{kind}.{n}"] = v
        for n, p in ema.ema.state_dict().items():
            if p.dtype.is_floating_point:
                for kind, v in grad_record(p).items():
                    arrays[f"s{step}.e{kind}.{n}"] = v
    meta["ema_updates"] = ema.updates
    # two files, each under the size limit of a committed file: the batches + the first update, and the second update
    save("accumulate_tiny", **{k: v for k, v in arrays.items() if not k.startswith("s1.")})
    save("accumulate_tiny.s1", **{k: v for k, v in arrays.items() if k.startswith("s1.")})
    (OUT / "accumulate_tiny.json").write_text(json.dumps(meta))


if __name__ == "__main__":
    main()
