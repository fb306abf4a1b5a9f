"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/ymi.h declares,
the host logic (YAML parser, module graph, state-dict keys, loss) matches the reference's fixtures, and
the product refuses to compute without the GPU (no fallback path)."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from conftest import GOLDEN, ROOT, golden_state, load_golden

PKG = ROOT / "improving_yolov8_cbam_swinblock_amd"


def header_functions():
    text = (ROOT / "include" / "ymi.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ymi_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
    from improving_yolov8_cbam_swinblock_amd import _lib

    if not _lib.LIB_PATH.exists():
        _lib.build()
    names = header_functions()
    assert len(names) >= 30
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    missing = [n for n in names if not hasattr(handle, n)]
    assert not missing, f"declared in include/ymi.h but not exported: {missing}"
    # the ctypes binding covers exactly the declared surface
    assert sorted(_lib.exported_symbols()) == names
    assert _lib.lib().ymi_version() == 1


def test_library_contains_gfx950_code_object_only():
    from improving_yolov8_cbam_swinblock_amd import _lib

    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-S", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    strings = subprocess.run(["strings", "-n", "6", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    archs = set(re.findall(r"amdgcn-amd-amdhsa--(gfx[0-9a-f]+)", strings))
    assert archs == {"gfx950"}, archs


def test_no_cpu_fallback():
    from improving_yolov8_cbam_swinblock_amd.nn.modules import CBAM, Conv, SwinBlock

    x = torch.randn(1, 8, 8, 8)
    for m in (Conv(8, 8, 3, 1), CBAM(8), SwinBlock(8, 2)):
        with pytest.raises(RuntimeError, match="MI355X|cuda"):
            m(x)


def test_product_does_not_import_the_oracle():
    for p in PKG.rglob("*.py"):
        src = p.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), p
    for p in (PKG / "csrc").glob("*"):
        if p.is_file() and p.suffix in (".hip", ".h", ".cpp", ".c", ""):  # sources and the Makefile (objects / stray tool caches are not product text)
            assert "oracle" not in p.read_text(errors="ignore"), p


def test_parse_model_tables_and_state_dict_keys():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import CFG_DIR, DetectionModel

    table = json.loads((GOLDEN / "parse_model_tables.json").read_text())
    for key, ref in table.items():
        fname, scale = key.split(":")
        cfg = yaml.safe_load((CFG_DIR / fname).read_text())
        cfg["scale"] = scale
        model = DetectionModel(cfg, ch=3)
        assert [m.type.split(".")[-1] for m in model.model] == [l["type"] for l in ref["layers"]], key
        assert [int(m.np) for m in model.model] == [l["np"] for l in ref["layers"]], key
        assert [m.f for m in model.model] == [l["f"] for l in ref["layers"]], key
        assert list(model.save) == ref["save"]
        assert [float(s) for s in model.stride] == ref["stride"]
        assert sum(p.numel() for p in model.parameters()) == ref["params"]
        assert {k: list(v.shape) for k, v in model.state_dict().items()} == ref["keys"], key


def test_yaml_name_resolution_and_scale_rule():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel, guess_model_scale, yaml_model_load

    assert guess_model_scale("yolov8s.yaml") == "s" and guess_model_scale("yolov8.yaml") == ""
    d = yaml_model_load("yolov8s.yaml")
    assert d["scale"] == "s" and d["backbone"][7][2] == "SwinBlock"
    assert yaml_model_load("yolov8n-cbam.yaml")["backbone"][9][2] == "CBAM"
    m = DetectionModel("yolov8s.yaml", ch=3, nc=1)
    assert sum(p.numel() for p in m.parameters()) == 13405269  # SURVEY.md 3.1 [measured on the reference]
    assert m.model[10].ca.shared_MLP[0].weight.shape == (32, 512, 1, 1)  # lazy CBAM: hidden = 512 // 16


def test_reference_state_dict_loads_strict():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    d = load_golden("e2e_tiny_seed7")
    model = DetectionModel(cfg, ch=3, nc=1)
    res = model.load_state_dict(golden_state(d), strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_oracle_loss_matches_reference_fixture_and_product_loss_has_no_cpu_path():
    """the oracle's loss is pinned by the reference-generated fixture here; the product's loss runs in HIP kernels only
    (its parity tests are GPU tests) and refuses CPU tensors."""
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel
    from oracle.loss import v8DetectionLoss as OracleLoss
    from oracle.tasks import DetectionModel as OracleModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    omodel = OracleModel(cfg, ch=3, nc=1)
    ocrit = OracleLoss(omodel)
    d = load_golden("loss_crowded")
    t = lambda a: torch.from_numpy(np.asarray(a))
    batch = {"batch_idx": t(d["batch_idx"]), "cls": t(d["cls"]), "bboxes": t(d["bboxes"])}
    p2 = [t(d[f"pred{i}"]).requires_grad_(True) for i in range(3)]
    l2, _ = ocrit(p2, batch)
    torch.testing.assert_close(l2, t(d["loss"]), rtol=1e-4, atol=1e-4)
    l2.sum().backward()
    for a, i in zip(p2, range(3)):
        torch.testing.assert_close(a.grad, t(d[f"g.pred{i}"]), rtol=1e-3, atol=1e-5)
    crit = DetectionModel(cfg, ch=3, nc=1).init_criterion()
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit([t(d[f"pred{i}"]) for i in range(3)], batch)


def _worker(rank, world, port, q):
    import os

    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from improving_yolov8_cbam_swinblock_amd.engine.ddp import allreduce_mean_gradients, broadcast_parameters, shard_seed

    torch.manual_seed(100 + rank)
    lin = torch.nn.Linear(5, 3)
    bn = torch.nn.BatchNorm1d(3)  # float buffers + an int64 counter: every dtype travels
    bn.running_mean.fill_(float(rank + 1))
    bn.num_batches_tracked.fill_(7 * (rank + 1))
    both = torch.nn.Sequential(lin, bn)
    broadcast_parameters(both, bucket_bytes=16)  # several flat chunks per dtype
    assert float(bn.running_mean[0]) == 1.0 and int(bn.num_batches_tracked) == 7, "buffers must come from rank 0"
    w0 = lin.weight.detach().clone()
    torch.manual_seed(shard_seed(1, rank))
    x = torch.randn(4, 5)
    lin(x).square().sum().backward()
    local = lin.weight.grad.clone()
    allreduce_mean_gradients(lin, world, bucket_bytes=16)
    q.put((rank, w0.numpy(), local.numpy(), lin.weight.grad.numpy()))
    dist.destroy_process_group()


def test_ddp_gradient_allreduce_gloo_world2():
    """N > 1 path: parameter broadcast + bucketed gradient all-reduce (mean), 2 ranks over gloo on CPU."""
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
    assert np.array_equal(res[0][1], res[1][1]), "parameters not identical after broadcast"
    mean = (res[0][2] + res[1][2]) / 2
    assert not np.allclose(res[0][2], res[1][2])  # different shards -> different local gradients
    for r in res:
        np.testing.assert_allclose(r[3], mean, rtol=1e-6, atol=1e-7)


def test_checkpoint_layout_and_weights_only_round_trip(tmp_path):
    """utils/checkpoint.py writes the reference's checkpoint keys (trainer.py:536-552) with plain containers in the
    weight slots, reads them back with weights_only=True, accepts a bare reference-style state_dict, and refuses a
    pickled-module checkpoint with an explanation instead of executing it."""
    import torch.nn as nn

    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel
    from improving_yolov8_cbam_swinblock_amd.utils.checkpoint import load_checkpoint, save_checkpoint

    torch.manual_seed(3)
    model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1)
    f = tmp_path / "last.pt"
    ckpt = save_checkpoint(f, model, epoch=7, best_fitness=0.5, train_args={"imgsz": 640})
    assert set(ckpt) >= {"epoch", "best_fitness", "model", "ema", "updates", "optimizer", "train_args", "train_metrics", "train_results", "date", "version", "license", "docs"}
    sd, back = load_checkpoint(f)
    assert back["epoch"] == 7 and back["train_args"]["imgsz"] == 640 and back["ema"] is None
    ref = model.state_dict()
    assert list(sd) == list(ref)
    for k, v in sd.items():  # stored as fp16 like the reference's EMA
        assert v.dtype == (torch.float16 if ref[k].dtype.is_floating_point else ref[k].dtype)
        assert torch.allclose(v.float(), ref[k].float(), rtol=1e-3, atol=1e-4)
    other = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1)
    assert other.load(f) == len(ref)
    assert torch.allclose(other.model[0].conv.weight, model.model[0].conv.weight.half().float())
    # a bare state_dict file (what the reference's `model.state_dict()` gives)
    g = tmp_path / "sd.pt"
    torch.save(model.state_dict(), g)
    assert other.load(g) == len(ref)
    assert torch.equal(other.model[0].conv.weight, model.model[0].conv.weight)
    # a pickled module (the reference's own format) is refused, not executed
    h = tmp_path / "pickled.pt"
    torch.save({"epoch": 0, "model": nn.Linear(2, 2), "ema": None}, h)
    with pytest.raises(RuntimeError, match="weights_only"):
        load_checkpoint(h)


def test_detect_level_declaration_matches_the_module_tree():
    """ops._Level (the one declaration of what a Detect level hands to _DetectTrain) against the module tree it is named after: every field of
    every level IS (identity) the parameter or buffer of cv2[i] / cv3[i] its name says; the per-level count is the number of gradients
    _DetectTrain.backward returns per level; a field's gradient lands at the position of its argument.  (The second convolutions of cv2 and
    cv3, and their BatchNorms, have equal shapes whenever c2 = c3: a transposed index there passes every shape check.)"""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.nn.modules import Detect

    for nc in (1, 3):
        _check_level_declaration(ops, Detect(nc, (32, 64, 128)))


def _check_level_declaration(ops, m):
    nl = len(m.cv2)
    assert nl == 3
    xs = [torch.zeros(1, c, 2, 2) for c in (32, 64, 128)]
    flat = ops._detect_args(xs, [(a[0], b[0], a[1], b[1], a[2], b[2]) for a, b in zip(m.cv2, m.cv3)])
    fields = ops._Level._fields
    assert len(fields) == 1 + 4 * 5 + 2 * 2 and len(set(fields)) == len(fields) and len(flat) == nl * len(fields)
    levels = ops._per_level(ops._Level, flat, nl)
    named = 0
    for i, lv in enumerate(levels):
        assert lv.x is xs[i]
        for block, mod in (("a0", m.cv2[i][0]), ("b0", m.cv3[i][0]), ("a1", m.cv2[i][1]), ("b1", m.cv3[i][1])):
            want = {"w": mod.conv.weight, "gamma": mod.bn.weight, "beta": mod.bn.bias, "mean": mod.bn.running_mean, "var": mod.bn.running_var}
            for part, tensor in want.items():
                assert getattr(lv, f"{block}_{part}") is tensor, (i, block, part)
                named += 1
        for out, mod in (("oa", m.cv2[i][2]), ("ob", m.cv3[i][2])):
            assert getattr(lv, f"{out}_w") is mod.weight and getattr(lv, f"{out}_bias") is mod.bias, (i, out)
            named += 2
    assert named == nl * (len(fields) - 1)  # every field but x was held to a module
    # gradients: one distinct marker per level and field; backward's return value puts each at the position of its argument in apply(meta, *flat)
    marks = [{f: object() for f in fields} for _ in range(nl)]
    grads = ops._detect_grads(marks)
    args = (None,) + tuple(flat)
    assert len(grads) == len(args) == 1 + nl * len(fields) and grads[0] is None
    for i, lv in enumerate(levels):
        for f in fields:
            (pos,) = [j for j, a in enumerate(args) if a is getattr(lv, f)]
            assert grads[pos] is marks[i][f], (i, f)
    assert ops._detect_grads([{}] * nl) == (None,) * (1 + nl * len(fields))  # (a gradient not produced is None)
    with pytest.raises(TypeError):
        ops._detect_grads([{"a1_gama": 0}] + [{}] * (nl - 1))  # a name that is no field is an error, not a dropped gradient
