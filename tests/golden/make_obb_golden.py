"""Generate the oriented-box fixtures under tests/golden/ by running the REAL reference on the CPU (the reference's tree must be present; the
import shim is make_golden.py's).  Writes data only:

    obb_parse_tables.json    per layer type / from / parameter count, save list, strides and parameter total of the reference's OBBModel built from
                             THIS package's cfg/models/v8/yolov8-obb.yaml and cfg/models/11/yolo11-obb.yaml at scales n, s, m, nc = 3; the head's
                             state-dict shapes at n
    obb_head_nc3.npz         OBB(3, 1, (32, 64, 128)), seeded: train maps / angle and their gradients, running statistics, eval output before
                             and after fuse
    obb_loss_<case>.npz      v8OBBLoss on seeded maps (tests/obb_common.py::LOSS_CASES): loss, items, the assignment (gidx), gradients
    obb_e2e_<model>.npz/json yolov8n-obb / yolo11n-obb, nc = 3, two 128 x 128 images, seeded weights: loss, items, gradient records

    python tests/golden/make_obb_golden.py

Nothing is stored that both sides can rebuild from a seed."""
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_golden import REPO, import_reference_package, save, sd_np  # noqa: E402

from golden_weights import grad_record  # noqa: E402
from make_psa_golden import fused_copy, grad_entries  # noqa: E402
from obb_common import CH, E2E_MODELS, E2E_NC, HEAD_SEED, HYP, LOSS_CASES, NC, NE, SCALES, STRIDE, e2e_batch, e2e_state, head_inputs, loss_case  # noqa: E402
from psa_common import seeded_module_state  # noqa: E402

CFG = REPO / "improving_yolov8_cbam_swinblock_amd" / "cfg" / "models"
YAMLS = {"yolov8-obb": CFG / "v8" / "yolov8-obb.yaml", "yolo11-obb": CFG / "11" / "yolo11-obb.yaml"}


def running(m):
    return {k: v for k, v in sd_np(m, "after.").items() if "running" in k or "num_batches" in k}


def main():
    torch.set_num_threads(4)
    tasks = import_reference_package()
    import ultralytics.nn.modules.conv as rc
    import ultralytics.nn.modules.head as rh
    import yaml
    from ultralytics.utils.loss import v8OBBLoss
    from ultralytics.utils.torch_utils import fuse_conv_and_bn, initialize_weights

    table = {}
    for fam, path in YAMLS.items():
        for scale in SCALES:
            d = yaml.safe_load(path.read_text())
            d["scale"] = scale
            torch.manual_seed(0)
            model = tasks.OBBModel(d, ch=3, nc=NC, verbose=False)
            table[f"{fam}:{scale}"] = {
                "layers": [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model],
                "save": list(model.save),
                "stride": [float(s) for s in model.stride],
                "params": int(sum(p.numel() for p in model.parameters())),
                "state": {k: list(v.shape) for k, v in model.state_dict().items() if k.startswith(f"model.{len(model.model) - 1}.")} if scale == "n" else None,
            }
    (OUT / "obb_parse_tables.json").write_text(json.dumps(table, indent=0))

    # OBB head
    legacy, rh.OBB.legacy = rh.OBB.legacy, True  # the v8 class branch (parse_model sets it per model)
    m = rh.OBB(NC, NE, CH)
    rh.OBB.legacy = legacy
    initialize_weights(m)
    m.stride = torch.tensor(STRIDE)
    m.load_state_dict(seeded_module_state(m, HEAD_SEED), strict=True)
    xs, gys, ga = head_inputs()
    xs = [t.requires_grad_(True) for t in xs]
    m.train()
    feats, angle = m(list(xs))
    params = [q for q in m.parameters() if q.requires_grad]
    pnames = [n for n, q in m.named_parameters() if q.requires_grad]
    grads = torch.autograd.grad(list(feats) + [angle], xs + params, gys + [ga])
    after = running(m)
    m.eval()
    with torch.no_grad():
        y_eval, (feats_e, angle_e) = m([t.detach() for t in xs])
        y_fused = fused_copy(m, rc, fuse_conv_and_bn)([t.detach() for t in xs])[0]
    arrays = {f"y_train{i}": t.detach().numpy() for i, t in enumerate(feats)}
    arrays.update(angle=angle.detach().numpy(), y_eval=y_eval.numpy(), y_fused=y_fused.numpy(), angle_eval=angle_e.numpy())
    arrays.update({f"g.x{i}": t.numpy() for i, t in enumerate(grads[: len(xs)])})
    save("obb_head_nc3", **arrays, **after, **grad_entries(pnames, grads[len(xs):]))

    # the criterion on seeded maps
    class Holder(torch.nn.Module):
        def __init__(self, head):
            super().__init__()
            self.model = torch.nn.ModuleList([head])
            self.args = SimpleNamespace(**HYP)

    for case in LOSS_CASES:
        c = loss_case(case)
        head = rh.OBB(c["nc"], NE, CH[: 1] * len(c["levels"]))
        head.stride = torch.tensor(c["strides"])
        holder = Holder(head.train())
        leaves = [t.requires_grad_(True) for t in c["feats"] + [c["angle"]]]
        crit = v8OBBLoss(holder)
        seen = {}
        real = crit.assigner.forward

        def spy(*a, _real=real, _seen=seen, **k):
            out = _real(*a, **k)
            _seen["fg"], _seen["idx"] = out[3], out[4]
            return out

        crit.assigner.forward = spy
        loss, items = crit((leaves[:-1], leaves[-1]), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in c["batch"].items()})
        grads = torch.autograd.grad(loss.sum(), leaves, allow_unused=True)
        gidx = torch.where(seen["fg"].bool(), seen["idx"], torch.full_like(seen["idx"], -1)).to(torch.int32)
        arrays = dict(loss=loss.detach().numpy(), items=items.numpy(), gidx=gidx.numpy())
        for n, g, t in zip([f"f{i}" for i in range(len(leaves) - 1)] + ["angle"], grads, leaves):
            arrays["g." + n] = (g if g is not None else torch.zeros_like(t)).numpy()
        print(case, "loss", items.tolist(), "foreground", (gidx >= 0).sum(1).tolist())
        save(case, **arrays)

    # end to end
    for name, cfg in E2E_MODELS.items():
        fam = "yolov8-obb" if "v8" in cfg else "yolo11-obb"
        d = yaml.safe_load(YAMLS[fam].read_text())
        d["scale"] = "n"
        torch.manual_seed(0)
        model = tasks.OBBModel(d, ch=3, nc=E2E_NC, verbose=False)
        model.load_state_dict(e2e_state(model), strict=True)
        model.args = SimpleNamespace(**HYP)
        batch = e2e_batch()
        model.train()
        preds = model(batch["img"])
        loss, items = v8OBBLoss(model)(preds, batch)
        loss.sum().backward()
        arrays = dict(loss=loss.detach().numpy(), loss_items=items.numpy())
        for n, q in model.named_parameters():
            if q.grad is not None:
                for kind, v in grad_record(q.grad).items():
                    arrays[f"g{kind}.{n}"] = v
        print(name, "loss", items.tolist())
        save(name, **arrays)
        (OUT / f"{name}.json").write_text(json.dumps({"scale": "n", "nc": E2E_NC, "params_with_grad": [n for n, q in model.named_parameters() if q.grad is not None]}))


if __name__ == "__main__":
    main()
