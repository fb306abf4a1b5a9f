"""Generate the segmentation fixtures under tests/golden/ by running the REAL reference on the CPU (the reference's tree must be present; the
import shim is make_golden.py's).  Writes data only:

    seg_parse_tables.json    per layer type / from / parameter count, save list, strides and parameter total of the reference's SegmentationModel
                             built from THIS package's cfg/models/v8/yolov8-seg.yaml and cfg/models/11/yolo11-seg.yaml at scales n, s, m, nc = 3
    seg_proto_32.npz         Proto(32, 32, 32), seeded: train output, gradients, running statistics, eval output before and after fuse
    seg_head_nc3.npz         Segment(3, 32, 32, (32, 64, 128)), seeded: train maps / mc / p and their gradients, eval output before and after fuse
    seg_loss_<case>.npz      v8SegmentationLoss on seeded maps (tests/seg_common.py::LOSS_CASES): loss, items, the assignment (gidx), gradients
    seg_e2e_<model>.npz/json yolov8n-seg / yolo11n-seg, nc = 3, two 128 x 128 images, seeded weights: loss, items, gradient records

    python tests/golden/make_seg_golden.py

Nothing is stored that both sides can rebuild from a seed."""
import copy
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_golden import REPO, import_reference_package, save, sd_np  # noqa: E402

from golden_weights import grad_record, seeded_inputs  # noqa: E402
from make_psa_golden import fused_copy, grad_entries  # noqa: E402
from psa_common import seeded_module_state  # noqa: E402
from seg_common import (CH, E2E_MODELS, E2E_NC, HEAD_SEED, HYP, LOSS_CASES, NC, NM, NPR, PROTO_CASE, PROTO_SEED, SCALES, STRIDE, e2e_batch, e2e_state,  # noqa: E402
                        head_inputs, loss_case)

CFG = REPO / "improving_yolov8_cbam_swinblock_amd" / "cfg" / "models"
YAMLS = {"yolov8-seg": CFG / "v8" / "yolov8-seg.yaml", "yolo11-seg": CFG / "11" / "yolo11-seg.yaml"}


def running(m):
    return {k: v for k, v in sd_np(m, "after.").items() if "running" in k or "num_batches" in k}


def main():
    torch.set_num_threads(4)
    tasks = import_reference_package()
    import ultralytics.nn.modules.block as rb
    import ultralytics.nn.modules.conv as rc
    import ultralytics.nn.modules.head as rh
    import yaml
    from ultralytics.utils.loss import v8SegmentationLoss
    from ultralytics.utils.torch_utils import fuse_conv_and_bn, initialize_weights

    table = {}
    for fam, path in YAMLS.items():
        for scale in SCALES:
            d = yaml.safe_load(path.read_text())
            d["scale"] = scale
            torch.manual_seed(0)
            model = tasks.SegmentationModel(d, ch=3, nc=NC, verbose=False)
            table[f"{fam}:{scale}"] = {
                "layers": [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model],
                "save": list(model.save),
                "stride": [float(s) for s in model.stride],
                "params": int(sum(p.numel() for p in model.parameters())),
                "state": {k: list(v.shape) for k, v in model.state_dict().items() if k.startswith(f"model.{len(model.model) - 1}.")} if scale == "n" else None,
            }
    (OUT / "seg_parse_tables.json").write_text(json.dumps(table, indent=0))

    # Proto
    name, args, xshape = PROTO_CASE
    m = rb.Proto(*args)
    initialize_weights(m)
    m.load_state_dict(seeded_module_state(m, PROTO_SEED), strict=True)
    m.train()
    x, gy = seeded_inputs(PROTO_SEED, xshape, (xshape[0], args[2], 2 * xshape[2], 2 * xshape[3]))
    x.requires_grad_(True)
    y = m(x)
    params = [p for p in m.parameters()]
    pnames = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + params, gy)
    after = running(m)
    m.eval()
    with torch.no_grad():
        y_eval = m(x)
        y_fused = fused_copy(m, rc, fuse_conv_and_bn)(x)
    save(name, y_train=y.detach().numpy(), y_eval=y_eval.numpy(), y_fused=y_fused.numpy(), **after, **{"g.x": grads[0].numpy()}, **grad_entries(pnames, grads[1:]))

    # Segment head
    legacy, rh.Segment.legacy = rh.Segment.legacy, True  # the v8 class branch (the reference's class default is the YOLO11 one; parse_model sets it per model)
    m = rh.Segment(NC, NM, NPR, CH)
    rh.Segment.legacy = legacy
    initialize_weights(m)
    m.stride = torch.tensor(STRIDE)
    m.load_state_dict(seeded_module_state(m, HEAD_SEED), strict=True)
    xs, gys, gmc, gp = head_inputs()
    xs = [t.requires_grad_(True) for t in xs]
    m.train()
    feats, mc, p = m(list(xs))
    params = [q for q in m.parameters() if q.requires_grad]
    pnames = [n for n, q in m.named_parameters() if q.requires_grad]
    grads = torch.autograd.grad(list(feats) + [mc, p], xs + params, gys + [gmc, gp])
    after = running(m)
    m.eval()
    with torch.no_grad():
        y_eval, (feats_e, mc_e, p_e) = m([t.detach() for t in xs])
        y_fused = fused_copy(m, rc, fuse_conv_and_bn)([t.detach() for t in xs])[0]
    arrays = {f"y_train{i}": t.detach().numpy() for i, t in enumerate(feats)}
    arrays.update(mc=mc.detach().numpy(), p=p.detach().numpy(), y_eval=y_eval.numpy(), y_fused=y_fused.numpy(), mc_eval=mc_e.numpy(), p_eval=p_e.numpy())
    arrays.update({f"g.x{i}": t.numpy() for i, t in enumerate(grads[: len(xs)])})
    save("seg_head_nc3", **arrays, **after, **grad_entries(pnames, grads[len(xs):]))

    # the criterion on seeded maps
    class Holder(torch.nn.Module):
        def __init__(self, head):
            super().__init__()
            self.model = torch.nn.ModuleList([head])
            self.args = SimpleNamespace(**HYP)

    holder = Holder(m.train())
    for case in LOSS_CASES:
        feats, mc, proto, batch = loss_case(case)
        leaves = [t.requires_grad_(True) for t in feats + [mc, proto]]
        crit = v8SegmentationLoss(holder)
        seen = {}
        real = crit.assigner.forward

        def spy(*a, _real=real, _seen=seen, **k):
            out = _real(*a, **k)
            _seen["fg"], _seen["idx"] = out[3], out[4]
            return out

        crit.assigner.forward = spy
        loss, items = crit((leaves[:3], leaves[3], leaves[4]), batch)
        grads = torch.autograd.grad(loss.sum(), leaves, allow_unused=True)
        gidx = torch.where(seen["fg"].bool(), seen["idx"], torch.full_like(seen["idx"], -1)).to(torch.int32)
        arrays = dict(loss=loss.detach().numpy(), items=items.numpy(), gidx=gidx.numpy())
        for n, g, t in zip(["f0", "f1", "f2", "mc", "proto"], grads, leaves):
            arrays["g." + n] = (g if g is not None else torch.zeros_like(t)).numpy()
        print(case, "loss", items.tolist(), "foreground", int((gidx >= 0).sum()), (gidx >= 0).sum(1).tolist())
        save(case, **arrays)

    # end to end
    for name, cfg in E2E_MODELS.items():
        fam = "yolov8-seg" if "v8" in cfg else "yolo11-seg"
        d = yaml.safe_load(YAMLS[fam].read_text())
        d["scale"] = "n"
        torch.manual_seed(0)
        model = tasks.SegmentationModel(d, ch=3, nc=E2E_NC, verbose=False)
        model.load_state_dict(e2e_state(model), strict=True)
        model.args = SimpleNamespace(**HYP)
        batch = e2e_batch()
        model.train()
        preds = model(batch["img"])
        loss, items = v8SegmentationLoss(model)(preds, batch)
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
