"""Generate the YOLO11 fixtures under tests/golden/ by running the REAL reference on the CPU (it runs where make_golden.py runs: the
reference's tree must be present; the import shim is make_golden.py's).  Writes data only:

    psa_<case>.npz           one per entry of tests/psa_common.py::CASES.  Small modules in the form of the ghost fixtures (x, w.*, y_train, gy,
                             g.*, after.* running statistics, y_eval, y_fused).  Modules above psa_common.SEEDED_ABOVE parameters store no weights
                             and no inputs (both sides rebuild them from the case's seed) and keep parameter gradients as
                             tests/golden_weights.py::grad_record entries (gfull.* | gsample.* + gnorm.*); g.x stays whole.
    psa_detect_nc3.npz       Detect(3, (32, 64, 128)) with the non-legacy class branch, seeded: train maps, their gradients, decoded eval output
                             (before and after fuse)
    psa_parse_tables.json    per layer type / from / parameter count, save list and strides of the reference's DetectionModel built from THIS
                             package's cfg/models/11/yolo11.yaml at scales n, s, m with nc = 3 (the reference's own file carries these rows
                             only as a comment)
    psa_e2e_n.npz / .json    yolo11n, nc = 3, two 128 x 128 images, seeded weights (nothing stored): train-mode maps, loss, gradient records

    python tests/golden/make_psa_golden.py

Own RNG streams: regenerating is bit-identical and touches no other fixture."""
import copy
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_golden import REPO, import_reference_package, randomize, save, sd_np  # noqa: E402

from golden_weights import grad_record  # noqa: E402
from psa_common import (CASES, DETECT_CASE, DETECT_CH, DETECT_NC, DETECT_SEED, DETECT_STRIDE, E2E_NC, SCALES, build, case_inputs, case_seed,  # noqa: E402
                        detect_inputs, e2e_batch, e2e_state, is_seeded, seeded_module_state)

PKG_YAML = REPO / "improving_yolov8_cbam_swinblock_amd" / "cfg" / "models" / "11" / "yolo11.yaml"


def fused_copy(m, rc, fuse_conv_and_bn):
    f = copy.deepcopy(m)
    for sub in f.modules():  # BaseModel.fuse (tasks.py:210-238)
        if isinstance(sub, rc.Conv) and hasattr(sub, "bn"):
            sub.conv = fuse_conv_and_bn(sub.conv, sub.bn)
            delattr(sub, "bn")
            sub.forward = sub.forward_fuse
    return f


def grad_entries(names, grads):
    out = {}
    for n, g in zip(names, grads):
        for kind, v in grad_record(g).items():
            out[f"g{kind}.{n}"] = v
    return out


def main():
    torch.set_num_threads(4)
    tasks = import_reference_package()
    import ultralytics.nn.modules.block as rb
    import ultralytics.nn.modules.conv as rc
    import ultralytics.nn.modules.head as rh
    import yaml
    from ultralytics.utils.loss import v8DetectionLoss
    from ultralytics.utils.torch_utils import fuse_conv_and_bn, initialize_weights

    g = torch.Generator().manual_seed(1357)
    for name in CASES:
        m = build(rb, name)
        initialize_weights(m)
        seeded = is_seeded(m)
        if seeded:
            m.load_state_dict(seeded_module_state(m, case_seed(name)), strict=True)
        else:
            randomize(m, g)
        before = sd_np(m)
        m.train()
        cin, hw = CASES[name][3], CASES[name][4]
        if seeded:
            with torch.no_grad():
                cout = copy.deepcopy(m).eval()(torch.zeros(1, cin, *hw)).shape[1]
            x, gy = case_inputs(name, cout)
            x.requires_grad_(True)
        else:
            x = torch.randn(2, cin, *hw, generator=g).requires_grad_(True)
        y = m(x)
        if not seeded:
            gy = torch.randn(y.shape, generator=g)
        params = [p for p in m.parameters() if p.requires_grad]
        pnames = [n for n, p in m.named_parameters() if p.requires_grad]
        grads = torch.autograd.grad(y, [x] + params, gy)
        after = {k: v for k, v in sd_np(m, "after.").items() if "running" in k or "num_batches" in k}
        m.eval()
        with torch.no_grad():
            y_eval = m(x)
            y_fused = fused_copy(m, rc, fuse_conv_and_bn)(x)
        common = dict(y_train=y.detach().numpy(), y_eval=y_eval.numpy(), y_fused=y_fused.numpy(), **after)
        if seeded:
            save(name, **common, **{"g.x": grads[0].numpy()}, **grad_entries(pnames, grads[1:]))
        else:
            save(name, x=x.detach().numpy(), gy=gy.numpy(), **common, **{"g." + n: t.numpy() for n, t in zip(["x"] + pnames, grads)}, **before)

    # Detect with the depthwise class branch
    rh.Detect.legacy = False
    m = rh.Detect(DETECT_NC, DETECT_CH)
    rh.Detect.legacy = True
    initialize_weights(m)
    m.stride = torch.tensor(DETECT_STRIDE)
    m.load_state_dict(seeded_module_state(m, DETECT_SEED), strict=True)
    xs, gys = detect_inputs(m.no)
    xs = [x.requires_grad_(True) for x in xs]
    m.train()
    maps = m(list(xs))
    params = [p for p in m.parameters() if p.requires_grad]
    pnames = [n for n, p in m.named_parameters() if p.requires_grad]
    grads = torch.autograd.grad(maps, xs + params, gys)
    after = {k: v for k, v in sd_np(m, "after.").items() if "running" in k or "num_batches" in k}
    m.eval()
    with torch.no_grad():
        y_eval, maps_eval = m([x.detach() for x in xs])
        y_fused, _ = fused_copy(m, rc, fuse_conv_and_bn)([x.detach() for x in xs])
    arrays = {f"y_train{i}": t.detach().numpy() for i, t in enumerate(maps)}
    arrays.update({f"y_eval_map{i}": t.numpy() for i, t in enumerate(maps_eval)})
    arrays.update({f"g.x{i}": t.numpy() for i, t in enumerate(grads[: len(xs)])})
    save(DETECT_CASE, y_eval=y_eval.numpy(), y_fused=y_fused.numpy(), **arrays, **after, **grad_entries(pnames, grads[len(xs):]))

    table = {}
    for scale in SCALES:
        d = yaml.safe_load(PKG_YAML.read_text())
        d["scale"] = scale
        torch.manual_seed(0)
        model = tasks.DetectionModel(d, ch=3, nc=E2E_NC, verbose=False)
        table[scale] = {
            "layers": [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model],
            "save": list(model.save),
            "stride": [float(s) for s in model.stride],
            "params": int(sum(p.numel() for p in model.parameters())),
            "state": {k: list(v.shape) for k, v in model.state_dict().items()} if scale == "n" else None,
        }
    (OUT / "psa_parse_tables.json").write_text(json.dumps(table, indent=0))

    d = yaml.safe_load(PKG_YAML.read_text())
    d["scale"] = "n"
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
    save("psa_e2e_n", **arrays)
    (OUT / "psa_e2e_n.json").write_text(json.dumps({"scale": "n", "nc": E2E_NC, "params_with_grad": [n for n, p in model.named_parameters() if p.grad is not None]}))


if __name__ == "__main__":
    main()
