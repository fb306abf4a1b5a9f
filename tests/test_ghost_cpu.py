"""Depthwise / Ghost modules without a GPU: the three ghost scales build, their graph tables equal the reference's
(tests/golden/ghost_parse_tables.json), the reference's state dicts load strictly, and what has no kernel still refuses."""
import json

import pytest

from conftest import GOLDEN, golden_state, load_golden
from ghost_common import CASES, E2E_NC, SCALES


def P():
    import improving_yolov8_cbam_swinblock_amd.nn.modules as M

    return M


@pytest.mark.parametrize("scale", SCALES)
def test_ghost_model_tables_equal_the_reference(scale):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    ref = json.loads((GOLDEN / "ghost_parse_tables.json").read_text())[scale]
    model = DetectionModel(f"yolov8{scale}-ghost.yaml", ch=3, nc=E2E_NC)
    got = [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model]
    assert got == ref["layers"]
    assert list(model.save) == ref["save"]
    assert [float(s) for s in model.stride] == ref["stride"]
    assert sum(p.numel() for p in model.parameters()) == ref["params"]


@pytest.mark.parametrize("name", list(CASES))
def test_reference_state_dicts_load_strictly(name):
    ctor, args, _ = CASES[name]
    m = getattr(P(), ctor)(*args)
    m.load_state_dict(golden_state(load_golden(name)), strict=True)


def test_only_pure_depthwise_groups_have_kernels():
    Conv = P().Conv
    with pytest.raises(NotImplementedError, match="pure depthwise only"):
        Conv(8, 16, 3, g=8)
    with pytest.raises(NotImplementedError):
        Conv(8, 8, 7, g=8)
    with pytest.raises(NotImplementedError, match="pure depthwise only"):
        Conv(8, 8, 3, g=8, d=2)
    with pytest.raises(NotImplementedError):
        Conv(8, 8, 5)  # dense 5x5: no kernel
    assert Conv(8, 8, 5, g=8).depthwise and not Conv(8, 8, 3).depthwise


def test_ghost_yaml_resolves_by_scale():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import yaml_model_load

    d = yaml_model_load("yolov8s-ghost.yaml")
    assert d["scale"] == "s" and d["backbone"][1][2] == "GhostConv" and d["backbone"][2][2] == "C3Ghost"
