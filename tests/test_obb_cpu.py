"""Oriented boxes on the CPU: the model files against the reference's parse tables, and the float64 restatement of tests/obb_ref.py against the
reference's fixtures (tests/golden/obb_*.npz/json, written by tests/golden/make_obb_golden.py from the real reference).

  parse tables    layer table, save list, strides, parameter totals of OBBModel from cfg/models/v8/yolov8-obb.yaml and cfg/models/11/yolo11-obb.yaml
                  at n, s, m with nc = 3 equal the reference's; the head's state-dict keys and shapes at n
  restatement     obb_ref in float64 reproduces every obb_loss_* fixture: the assignment equal, loss, items and gradients close
  float32         the distance of the reference's float32 arithmetic from obb_ref, per stage, is what obb_ref.REF32_DISTANCE records; at most 2 %
                  of a case's (gt, anchor) decisions lie within obb_ref.THRESHOLD, and outside them the float32 assignment equals the float64 one
  planted faults  each wrong rule of obb_ref.FAULTS makes at least one case fail; probiou is symmetric bit for bit (why swapping its boxes is
                  no fault)"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import obb_ref as R
from obb_common import LOSS_CASES, NC, SCALES, loss_case

GOLDEN = Path(__file__).resolve().parent / "golden"
REL_F64 = 5e-6  # the fixtures are float32 results: loss and gradients of the reference within a few float32 roundings of float64


def gold(name):
    return np.load(GOLDEN / f"{name}.npz")


_r = {}


def restated(name, dtype=torch.float64, fault=None):
    key = (name, dtype, fault)
    if key not in _r:
        c = loss_case(name)
        _r[key] = R.restate(c, dtype=dtype, grad_loss=(1.0, 1.0, 1.0), grad_scale=R.out_scale(c["B"])[:3], fault=fault)
    return _r[key]


def fixture_errors(name, r):
    """-> (assignment equal, worst scaled error of loss, items and the gradients) of a restatement against the reference's fixture"""
    d = gold(name)
    same = bool((torch.from_numpy(d["gidx"]).long() == r["gidx"]).all())
    errs = [R.scaled_err(d["loss"], r["loss6"][:3]), R.scaled_err(d["items"], r["loss6"][3:]), R.scaled_err(d["g.angle"], r["dangle"])]
    errs += [R.scaled_err(d[f"g.f{i}"], g) for i, g in enumerate(r["dfeats"])]
    return same, max(errs)


@pytest.mark.parametrize("fam", ["yolov8-obb", "yolo11-obb"])
@pytest.mark.parametrize("scale", SCALES)
def test_parse_tables_equal_the_reference(fam, scale):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import OBBModel

    want = json.loads((GOLDEN / "obb_parse_tables.json").read_text())[f"{fam}:{scale}"]
    model = OBBModel(f"{fam.replace('-obb', '')}{scale}-obb.yaml", ch=3, nc=NC)
    got = [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model]
    assert got == want["layers"]
    assert list(model.save) == want["save"] and [float(s) for s in model.stride] == want["stride"]
    assert sum(p.numel() for p in model.parameters()) == want["params"]
    if want["state"] is not None:
        last = f"model.{len(model.model) - 1}."
        assert {k: list(v.shape) for k, v in model.state_dict().items() if k.startswith(last)} == want["state"]


def test_parameter_totals_and_exports():
    import improving_yolov8_cbam_swinblock_amd.nn.modules as M
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import OBBModel

    assert sum(p.numel() for p in OBBModel("yolov8n-obb.yaml", nc=3).parameters()) == 3083100
    assert sum(p.numel() for p in OBBModel("yolo11n-obb.yaml", nc=3).parameters()) == 2662092
    assert issubclass(M.OBB, M.Detect) and M.OBBPreds is not None
    with pytest.raises(NotImplementedError, match="ne = 1"):
        M.OBB(3, 2, (32, 64, 128))
    m = OBBModel("yolov8n-obb.yaml", nc=3)
    assert m.boundary_layers() == {4: 1, 6: 1, 9: 2}  # (the same edges as the stock graph; the head reads layers of the head only)
    plan = m._graph_plan()["consumers"]
    assert plan[15] == 3 and plan[18] == 3 and plan[21] == 2  # paired box + class convolution, cv4, (the next Conv)


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_restatement_reproduces_the_fixture(name):
    same, err = fixture_errors(name, restated(name))
    print(name, "worst scaled error against the reference's float32 fixture", err)
    assert same and err <= REL_F64


def test_float32_distance_per_stage():
    """the reference's float32 arithmetic against float64: per stage, the worst case; the record of obb_ref.REF32_DISTANCE covers it and is no
    more than twice what is measured (it is a record, not a loose bound)"""
    worst = {k: 0.0 for k in R.REF32_DISTANCE}
    for name in LOSS_CASES:
        r, r32, d = restated(name), restated(name, torch.float32), gold(name)
        for k in ("targets", "pb", "ov", "al", "pa", "po", "tgt", "wgt", "tss"):
            worst[k] = max(worst[k], R.scaled_err(r32[k], r[k]))
        worst["loss"] = max(worst["loss"], R.scaled_err(d["items"], r["loss6"][3:]))
        worst["loss6"] = max(worst["loss6"], R.scaled_err(np.concatenate([d["loss"], d["items"]]), r["loss6"]))
        worst["dfeats"] = max([worst["dfeats"]] + [R.scaled_err(d[f"g.f{i}"], g) for i, g in enumerate(r["dfeats"])])
        worst["dangle"] = max(worst["dangle"], R.scaled_err(d["g.angle"], r["dangle"]))
    print({k: float(f"{v:.2g}") for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= R.REF32_DISTANCE[k] <= max(2.0 * v, 1e-7), (k, v, R.REF32_DISTANCE[k])


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_float32_reference_stays_inside_the_margins(name):
    c = loss_case(name)
    r = restated(name)
    left, share = R.uncertain(c, r)
    assert share <= R.MAX_LEFT_OUT
    keep = ~left
    r32 = restated(name, torch.float32)
    assert (r32["inside"] == r["inside"])[keep].all() and (r32["mpos"] == r["mpos"])[keep].all()
    a_keep = keep.all(1)
    assert (r32["gidx"] == r["gidx"])[a_keep].all()
    assert (torch.from_numpy(gold(name)["gidx"]).long() == r["gidx"])[a_keep].all()  # the real reference in float32


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_fault_fails_a_case(fault):
    caught = []
    for name in LOSS_CASES:
        same, err = fixture_errors(name, restated(name, fault=fault))
        if not same or err > REL_F64:
            caught.append(name)
    print(fault, "caught by", caught)
    assert caught


def test_probiou_is_symmetric_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float32, torch.float64):
        a = torch.rand(4096, 5, generator=g, dtype=dtype) * torch.tensor([60, 60, 40, 40, 3.0], dtype=dtype)
        b = torch.rand(4096, 5, generator=g, dtype=dtype) * torch.tensor([60, 60, 40, 40, 3.0], dtype=dtype)
        assert torch.equal(R.probiou(a, b), R.probiou(b, a))


def test_tiny_filter_and_padding_rows():
    c = loss_case("obb_loss_rect")
    t, _ = R.dense_targets(c)
    assert t.shape == (2, 4, 6)
    assert float(t[0, 0, 3]) == pytest.approx(0.0215 * 64, rel=1e-6)  # the 1.968-pixel row went, the 2.064-pixel row leads
    assert (t[0, 3] == 0).all() and (t[1, 2:] == 0).all()  # padding rows
    r = restated("obb_loss_rect")
    assert r["valid"].tolist() == [[True, True, True, False], [True, True, False, False]]
    assert int(t[1, 0, 0]) == NC - 1
