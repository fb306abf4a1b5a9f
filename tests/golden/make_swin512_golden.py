"""Generate the YOLO11-CBAM-Swin fixtures under tests/golden/ by running the REAL reference on the CPU (it runs where make_golden.py runs: the
reference's tree must be present; the import shim is make_golden.py's).  Writes data only:

    swin_d512_*.npz              SwinBlock(512, 2) - head_dim 256 - in the LARGE_SWIN format of make_golden.py::swin_large_fixtures, seeded
                                 (conftest.load_large_swin / large_swin_grad_errors read them unchanged): four full 7 x 7 windows; padding tokens as
                                 keys; 196-token windows with padding
    swin512_parse_tables.json    per layer type / from / parameter count, save list, strides, parameter total (and at m the state-dict shapes) of the
                                 reference's DetectionModel built from the reference's OWN cfg/models/11/yolo11.yaml at scales m and l, nc = 3.  `np`
                                 is the parse-time count (CBAM's lazy MLP is not in it: 98), `params` the total after the stride probe built it.
    swin512_e2e_m.npz, swin512_e2e_m.g1.npz / .json
                                 yolo11m-cbam-swin (this package's YAML through the reference's parser; its state-dict shapes are asserted equal to the
                                 reference file's), nc = 3, two 128 x 128 images, seeded weights (nothing stored): train-mode maps, loss, gradient
                                 records - the records of the second half of the parameters (by stored bytes) in the .g1 file, so that each
                                 stays below 1 MiB; a test merges the two dicts.  The JSON also names the gradients that are ZERO in exact arithmetic: the same model and batch run in
                                 float64, every gradient whose float64 norm is below ZERO_NORM but not 0.0 (a float32 run shows
                                 rounding noise there), with the norms either side of the gap.

    python tests/golden/make_swin512_golden.py

The .npz files are ordinary zip archives that numpy.load reads as ever; their members are LZMA-compressed (zip method 14) with two
literal-position bits, which models float32 data by byte position and packs it to 83 % where deflate reaches 92 %: the 196-token SwinBlock case
is 1.06 MB deflated and 0.96 MB so.

Own RNG streams: regenerating is bit-identical and touches no other fixture."""
import copy
import io
import json
import lzma
import struct
import sys
import zipfile
from pathlib import Path
from types import SimpleNamespace
from unittest import mock

import numpy as np
import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_golden import REF, REPO, import_reference_package, load_leaf  # noqa: E402

from golden_weights import grad_record, seeded_inputs, seeded_state  # noqa: E402
from psa_common import E2E_NC, e2e_batch, e2e_state  # noqa: E402

PKG_YAML = REPO / "improving_yolov8_cbam_swinblock_amd" / "cfg" / "models" / "11" / "yolo11-cbam-swin.yaml"
REF_YAML = REF / "ultralytics" / "cfg" / "models" / "11" / "yolo11.yaml"
SCALES = ("m", "l")
ZERO_NORM = 1e-12  # float64 gradient norms: the exact zeros come out <= 6e-15, every other gradient >= 3e-10

SWIN512 = [
    # name, dim, heads, ws, B, H, W, seed, seeded weights
    ("swin_d512_14x14", 512, 2, 7, 1, 14, 14, 21, True),        # four full windows
    ("swin_d512_9x11", 512, 2, 7, 2, 9, 11, 22, True),          # 14 x 14 padded grid: padding tokens act as keys
    ("swin_d512_ws14_16x15", 512, 2, 14, 1, 16, 15, 23, True),  # 196-token windows with padding: the tiled kernels
]


LC, LP, PB, DICT = 1, 2, 2, 1 << 21  # lp = 2: the low two bits of the byte position select the literal model (4-byte elements)


class AlignedLZMA:
    """the compressor zipfile asks for a method-14 member, with the parameters above instead of the preset's.  A member is the 4-byte header
    (LZMA SDK version 9.4, property size 5), the five LZMA property bytes ((pb * 5 + lp) * 9 + lc, dictionary size) and the raw stream; the
    reader takes the parameters from those bytes, so any zip reader decodes it."""

    def __init__(self):
        self._comp = lzma.LZMACompressor(lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA1, "lc": LC, "lp": LP, "pb": PB, "dict_size": DICT,
                                                                    "preset": 9 | lzma.PRESET_EXTREME}])
        self._head = struct.pack("<BBHBI", 9, 4, 5, (PB * 5 + LP) * 9 + LC, DICT)

    def compress(self, data):
        head, self._head = self._head, b""
        return head + self._comp.compress(data)

    def flush(self):
        head, self._head = self._head, b""
        return head + self._comp.flush()


def save(name, **arrays):
    path = OUT / f"{name}.npz"
    with mock.patch.object(zipfile, "LZMACompressor", AlignedLZMA), zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy"), b.getvalue(), compress_type=zipfile.ZIP_LZMA)  # (ZipInfo's fixed date: the same bytes every time)
    with np.load(path) as back:
        assert set(back.files) == set(arrays) and all(np.array_equal(back[k], np.asanyarray(v)) for k, v in arrays.items()), name
    size = path.stat().st_size
    assert size < (1 << 20), (name, size)
    print(f"{name}.npz  {size / 1024:.1f} kB")


def swin512_fixtures():
    swin = load_leaf("ref_swin", "ultralytics/nn/modules/swin_block.py")
    for name, dim, heads, ws, B, H, W, seed, seeded in SWIN512:
        m = swin.SwinBlock(dim, heads, ws)
        m.load_state_dict(seeded_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed), strict=True)
        x, gy = seeded_inputs(seed, (B, dim, H, W), (B, dim, H, W))
        x.requires_grad_(True)
        y = m(x)
        names = [n for n, _ in m.named_parameters()]
        grads = torch.autograd.grad(y, [x] + list(m.parameters()), gy)
        arrays = dict(meta=np.array([dim, heads, ws, B, H, W, seed, int(seeded)]), y=y.detach().numpy())
        arrays["g.x"] = grads[0].numpy()
        for n, t in zip(names, grads[1:]):
            for kind, v in grad_record(t).items():
                arrays[f"g{kind}.{n}"] = v
        save(name, **arrays)


def build(tasks, yaml_path, scale):
    import yaml

    d = yaml.safe_load(Path(yaml_path).read_text())
    d["scale"] = scale
    torch.manual_seed(0)
    return tasks.DetectionModel(d, ch=3, nc=E2E_NC, verbose=False)


def parse_tables(tasks):
    table = {}
    for scale in SCALES:
        model = build(tasks, REF_YAML, scale)
        table[scale] = {
            "layers": [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model],
            "save": list(model.save),
            "stride": [float(s) for s in model.stride],
            "params": int(sum(p.numel() for p in model.parameters())),
            "state": {k: list(v.shape) for k, v in model.state_dict().items()} if scale == "m" else None,
        }
    (OUT / "swin512_parse_tables.json").write_text(dump_rows(table))
    return table


def dump_rows(table):
    """the table as JSON with one layer, and one state-dict entry, per line"""
    js, out = json.dumps, []
    for scale, t in table.items():
        layers = ",\n".join("  " + js(l) for l in t["layers"])
        state = "null" if t["state"] is None else "{\n" + ",\n".join(f"  {js(k)}: {js(v)}" for k, v in t["state"].items()) + "\n }"
        out.append(f'{js(scale)}: {{\n "layers": [\n{layers}\n ],\n "save": {js(t["save"])},\n "stride": {js(t["stride"])},\n'
                   f' "params": {js(t["params"])},\n "state": {state}\n}}')
    return "{\n" + ",\n".join(out) + "\n}\n"


def run_step(model, batch, loss_cls):
    model.train()
    preds = model(batch["img"])
    loss, items = loss_cls(model)(preds, batch)
    loss.sum().backward()
    return preds, loss, items


def e2e(tasks, table):
    from ultralytics.utils.loss import v8DetectionLoss

    model = build(tasks, PKG_YAML, "m")
    assert {k: list(v.shape) for k, v in model.state_dict().items()} == table["m"]["state"], "the package's YAML is not the reference's model"
    model.load_state_dict(e2e_state(model), strict=True)
    model.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5)
    batch = e2e_batch()
    m64 = copy.deepcopy(model).double()
    preds, loss, items = run_step(model, batch, v8DetectionLoss)
    arrays = {f"pred{i}": p.detach().numpy() for i, p in enumerate(preds)}
    arrays.update(loss=loss.detach().numpy(), loss_items=items.numpy())
    records = [{f"g{kind}.{n}": v for kind, v in grad_record(p.grad).items()} for n, p in model.named_parameters() if p.grad is not None]
    total, done, second = sum(v.nbytes for r in records for v in r.values()), 0, {}
    for r in records:  # parameter order: the first half of the stored bytes beside the maps, the rest in the .g1 file
        (arrays if done < total / 2 else second).update(r)
        done += sum(v.nbytes for v in r.values())
    save("swin512_e2e_m", **arrays)
    save("swin512_e2e_m.g1", **second)

    b64 = {k: (v.double() if k in ("img", "bboxes") else v) for k, v in batch.items()}
    preds64, loss64, _ = run_step(m64, b64, v8DetectionLoss)
    norms = {n: float(p.grad.norm()) for n, p in m64.named_parameters() if p.grad is not None}
    f32 = dict(model.named_parameters())
    # exactly 0.0 in both precisions (Detect's box branch on the 4 x 4 level: no positive anchor there): ordinary records, zero equals zero
    dead = sorted(n for n, v in norms.items() if v == 0.0)
    assert all(float(f32[n].grad.abs().max()) == 0.0 for n in dead), dead
    zero = sorted(n for n, v in norms.items() if 0.0 < v < ZERO_NORM)
    map_err = max(float((a.detach().double() - b.detach()).abs().max() / max(1.0, float(b.detach().abs().max())))
                  for a, b in zip(preds, preds64))
    grad_err = max(float((f32[n].grad.double() - p.grad).norm() / p.grad.norm())
                   for n, p in m64.named_parameters() if p.grad is not None and n not in zero and n not in dead)
    info = {
        "scale": "m", "nc": E2E_NC,
        "params_with_grad": [n for n, p in model.named_parameters() if p.grad is not None],
        "zero_in_exact_arithmetic": zero,
        "exactly_zero_in_both_precisions": dead,
        "float64_norm_largest_zero": max(norms[n] for n in zero) if zero else 0.0,
        "float64_norm_smallest_nonzero": min(v for n, v in norms.items() if n not in zero and n not in dead),
        "reference_float32_vs_float64": {"maps_scaled_max_abs": map_err, "worst_gradient_relative_l2": grad_err,
                                         "loss64": [float(v) for v in loss64.detach()]},
    }
    (OUT / "swin512_e2e_m.json").write_text(json.dumps(info, indent=0))
    print(json.dumps({k: v for k, v in info.items() if k != "params_with_grad"}, indent=1))


def main():
    torch.set_num_threads(4)
    which = sys.argv[1:] or ["swin", "tables", "e2e"]
    if "swin" in which:
        swin512_fixtures()
    if "tables" in which or "e2e" in which:
        tasks = import_reference_package()
        table = parse_tables(tasks)
        if "e2e" in which:
            e2e(tasks, table)


if __name__ == "__main__":
    main()
