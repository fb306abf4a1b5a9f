"""Generate the depthwise / Ghost fixtures under tests/golden/ by running the REAL reference on the CPU (it runs where make_golden.py runs: the
reference's tree must be present; the import shim is make_golden.py's).  Writes data only:

    ghost_<case>.npz          one per entry of tests/ghost_common.py::CASES, in the form of the conv fixtures of make_golden.py
                              (x, w.*, y_train, gy, g.*, after.* running statistics, y_eval) plus y_fused: the eval output after
                              BaseModel.fuse()'s fold of every Conv block
    ghost_parse_tables.json   per layer type / from / parameter count, save list and strides of yolov8{n,s,m}-ghost.yaml at nc = 3
    ghost_e2e_s.npz / .json   yolov8s-ghost, nc = 3, two 128 x 128 images, seeded weights (nothing stored): train-mode maps, loss, gradient
                              records (tests/golden_weights.py::grad_record)
The model graphs are built from the REFERENCE's own cfg/models/v8/yolov8-ghost.yaml, so the tests pin this package's file to it.

    python tests/golden/make_ghost_golden.py

Own RNG streams: regenerating is bit-identical and touches no other fixture."""
import copy
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_golden import REF, import_reference_package, randomize, save, sd_np  # noqa: E402

from ghost_common import CASES, E2E_NC, INPUT_HW, SCALES, e2e_batch, e2e_state  # noqa: E402
from golden_weights import grad_record  # noqa: E402


REF_YAML = REF / "ultralytics" / "cfg" / "models" / "v8" / "yolov8-ghost.yaml"


def main():
    torch.set_num_threads(4)
    tasks = import_reference_package()
    import ultralytics.nn.modules.block as rb
    import ultralytics.nn.modules.conv as rc
    import yaml
    from ultralytics.utils.loss import v8DetectionLoss
    from ultralytics.utils.torch_utils import fuse_conv_and_bn, initialize_weights

    g = torch.Generator().manual_seed(2468)
    for name, (ctor, args, cin) in CASES.items():
        m = getattr(rc, ctor, None) or getattr(rb, ctor)
        m = m(*args)
        initialize_weights(m)
        randomize(m, g)
        before = sd_np(m)
        m.train()
        x = torch.randn(2, cin, *INPUT_HW, generator=g).requires_grad_(True)
        y = m(x)
        gy = torch.randn(y.shape, generator=g)
        params = [p for p in m.parameters() if p.requires_grad]
        pnames = [n for n, p in m.named_parameters() if p.requires_grad]
        grads = torch.autograd.grad(y, [x] + params, gy)
        after = sd_np(m, "after.")
        m.eval()
        with torch.no_grad():
            y_eval = m(x)
            f = copy.deepcopy(m)
            for sub in f.modules():  # BaseModel.fuse (tasks.py:210-238)
                if isinstance(sub, rc.Conv) and hasattr(sub, "bn"):
                    sub.conv = fuse_conv_and_bn(sub.conv, sub.bn)
                    delattr(sub, "bn")
                    sub.forward = sub.forward_fuse
            y_fused = f(x)
        save(name, x=x.detach().numpy(), y_train=y.detach().numpy(), y_eval=y_eval.numpy(), y_fused=y_fused.numpy(), gy=gy.numpy(),
             **{"g." + n: t.numpy() for n, t in zip(["x"] + pnames, grads)}, **before,
             **{k: v for k, v in after.items() if "running" in k or "num_batches" in k})

    table = {}
    for scale in SCALES:
        d = yaml.safe_load(REF_YAML.read_text())
        d["scale"] = scale
        torch.manual_seed(0)
        model = tasks.DetectionModel(d, ch=3, nc=E2E_NC, verbose=False)
        table[scale] = {
            "layers": [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model],
            "save": list(model.save),
            "stride": [float(s) for s in model.stride],
            "params": int(sum(p.numel() for p in model.parameters())),
        }
    (OUT / "ghost_parse_tables.json").write_text(json.dumps(table, indent=0))

    d = yaml.safe_load(REF_YAML.read_text())
    d["scale"] = "s"
    torch.manual_seed(0)
    model = tasks.DetectionModel(d, ch=3, nc=E2E_NC, verbose=False)
    model.load_state_dict(e2e_state(model), strict=True)
    model.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5)
    batch = e2e_batch()
    model.train()
    preds = model(batch["img"])
    loss, items = v8DetectionLoss(model)(preds, batch)
    loss.sum().backward()
    arrays = {f"pred{i}": p.detach().numpy() for i, p in enumerate(preds)}
    arrays.update(loss=loss.detach().numpy(), loss_items=items.numpy())
    for n, p in model.named_parameters():
        if p.grad is not None:
            for kind, v in grad_record(p.grad).items():
                arrays[f"g{kind}.{n}"] = v
    save("ghost_e2e_s", **arrays)
    (OUT / "ghost_e2e_s.json").write_text(json.dumps({"scale": "s", "nc": E2E_NC, "params_with_grad": [n for n, p in model.named_parameters() if p.grad is not None]}))


if __name__ == "__main__":
    main()
