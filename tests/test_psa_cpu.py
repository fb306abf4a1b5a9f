"""YOLO11 without a GPU: the three scales build with the reference's layer tables (tests/golden/psa_parse_tables.json), the reference's state dicts
load strictly into the new modules, the float64 restatement of the packed-layout attention (tests/psa_ref.py) reproduces the reference's
Attention fixtures, and what has no kernel still refuses."""
import json

import pytest
import torch

from conftest import GOLDEN, golden_state, load_golden
from psa_common import (CASES, DETECT_CASE, DETECT_CH, DETECT_NC, DETECT_SEED, E2E_NC, SCALES, build, case_inputs, case_seed, is_seeded,
                        seeded_module_state)


def P():
    import improving_yolov8_cbam_swinblock_amd.nn.modules as M

    return M


def tables():
    return json.loads((GOLDEN / "psa_parse_tables.json").read_text())


@pytest.mark.parametrize("scale", SCALES)
def test_yolo11_tables_equal_the_reference(scale):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    ref = tables()[scale]
    model = DetectionModel(f"yolo11{scale}.yaml", ch=3, nc=E2E_NC)
    got = [{"i": m.i, "f": m.f, "type": m.type.split(".")[-1], "np": int(m.np)} for m in model.model]
    assert got == ref["layers"]
    assert list(model.save) == ref["save"]
    assert [float(s) for s in model.stride] == ref["stride"]
    assert sum(p.numel() for p in model.parameters()) == ref["params"]
    assert model.model[-1].legacy is False and P().Detect.legacy is True  # the instance took the depthwise branch; the class default is v8's


def test_yolo11n_state_dict_keys_and_shapes_equal_the_reference():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    ref = tables()["n"]["state"]
    got = {k: list(v.shape) for k, v in DetectionModel("yolo11n.yaml", ch=3, nc=E2E_NC).state_dict().items()}
    assert got == ref


def test_c3k2_members_follow_the_scale():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    M = P()
    n = DetectionModel("yolo11n.yaml", ch=3, nc=E2E_NC).model
    m = DetectionModel("yolo11m.yaml", ch=3, nc=E2E_NC).model
    assert isinstance(n[2].m[0], M.Bottleneck) and isinstance(n[6].m[0], M.C3k)
    assert all(isinstance(m[i].m[0], M.C3k) for i in (2, 4, 6, 8, 13, 16, 19, 22))  # m, l, x: C3k members whatever the row says
    assert isinstance(n[10], M.C2PSA) and n[10].m[0].attn.num_heads == 2 and n[10].m[0].attn.key_dim == 32


def test_v8_yaml_keeps_the_legacy_detect_branch():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    det = DetectionModel("yolov8n.yaml", ch=3, nc=E2E_NC).model[-1]
    assert det.legacy is True and isinstance(det.cv3[0][0], P().Conv) and det.cv3[0][0].conv.kernel_size == (3, 3)


def test_yolo11_yaml_resolves_by_scale():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import yaml_model_load

    d = yaml_model_load("yolo11s.yaml")
    assert d["scale"] == "s" and d["backbone"][2][2] == "C3k2" and d["backbone"][10][2] == "C2PSA" and len(d["backbone"]) == 11 and len(d["head"]) == 13


@pytest.mark.parametrize("name", list(CASES))
def test_reference_state_dicts_load_strictly(name):
    m = build(P(), name)
    d = load_golden(name)
    if is_seeded(m):  # no weights stored: the key set and shapes are the reference's if its running statistics load strictly on top of the seed
        state = seeded_module_state(m, case_seed(name))
        after = golden_state(d, "after.")
        assert set(after) == {k for k in state if "running" in k or "num_batches" in k}
        state.update(after)
    else:
        state = golden_state(d)
    m.load_state_dict(state, strict=True)


def test_nonlegacy_detect_has_the_reference_structure():
    M = P()
    M.Detect.legacy = False
    try:
        m = M.Detect(DETECT_NC, DETECT_CH)
    finally:
        M.Detect.legacy = True
    d = load_golden(DETECT_CASE)
    state = seeded_module_state(m, DETECT_SEED)
    after = golden_state(d, "after.")
    assert set(after) == {k for k in state if "running" in k or "num_batches" in k}
    names = {n for n, _ in m.named_parameters() if _.requires_grad}
    stored = {k.split(".", 1)[1] for k in d if k.startswith(("gfull.", "gsample."))}
    assert names == stored
    assert m.cv3[0][0][0].depthwise and m.cv3[0][0][1].conv.kernel_size == (1, 1) and m.cv3[2][1][0].conv.groups == 32 and not m.pair_ok


@pytest.mark.parametrize("name", ["psa_attention_64_h1", "psa_attention_64_h2"])
def test_packed_attention_restatement_reproduces_the_reference(name):
    """tests/psa_ref.py on the Attention fixtures: forward and every gradient.  The reference computed in float32: 1e-4 of the tensor's largest
    magnitude separates a layout, scale or v_out mistake (errors of order one) from float32 rounding (1e-6)."""
    from psa_ref import attention_module_ref

    _, _, kwargs, _, _ = CASES[name]
    d = load_golden(name)
    M = P()
    m = build(M, name)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in d.items() if k.startswith("w.") and k.endswith(("conv.weight", "bn.weight", "bn.bias"))}
    p = {k[2:]: v for k, v in p.items()}
    x = torch.from_numpy(d["x"]).double().requires_grad_(True)
    y = attention_module_ref(p, x, m.num_heads, m.key_dim)
    names = [n for n, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + [p[n] for n in names], torch.from_numpy(d["gy"]).double())

    def close(a, b, what):
        b = torch.from_numpy(b).double()
        err, scale = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
        assert err <= 1e-4 * scale, (name, what, err, scale)

    close(y.detach(), d["y_train"], "y_train")
    for n, g in zip(["x"] + names, grads):
        close(g, d["g." + n], "grad " + n)


def test_packed_layout_helpers_round_trip():
    from psa_ref import pack, psa_attention_ref, split_packed

    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(3 * 10, 2 * (2 * 4 + 8), generator=g, dtype=torch.float64)
    q, k, v = split_packed(qkv, 10, 2, 4)
    assert q.shape == (3, 2, 10, 4) and v.shape == (3, 2, 10, 8) and torch.equal(pack(q, k, v), qkv)
    assert torch.equal(q[1, 1, 3], qkv[13, 16:20]) and torch.equal(k[1, 1, 3], qkv[13, 20:24]) and torch.equal(v[1, 0, 3], qkv[13, 8:16])
    o, vo = psa_attention_ref(qkv, 10, 2, 4)
    assert torch.equal(vo[:, :8], qkv[:, 8:16]) and torch.equal(vo[:, 8:], qkv[:, 24:32]) and o.shape == (30, 16)
    # images do not mix: changing image 2 leaves image 0's output alone
    qkv2 = qkv.clone()
    qkv2[20:] += 1.0
    assert torch.equal(psa_attention_ref(qkv2, 10, 2, 4)[0][:20], o[:20])


def test_refusals_that_still_hold():
    M = P()
    with pytest.raises(NotImplementedError):
        M.Conv(8, 8, 5)  # dense 5x5: no kernel
    with pytest.raises(NotImplementedError, match="dilation 1"):
        M.Conv(8, 8, 3, d=2)
    with pytest.raises(NotImplementedError, match="pure depthwise only"):
        M.DWConv(8, 12, 3)  # gcd(8, 12) = 4 groups: not depthwise
    with pytest.raises(NotImplementedError):
        M.C3k(32, 32, 1, k=5)  # dense 5x5 Bottlenecks


def test_library_binding_lists_the_psa_entry_points():
    from improving_yolov8_cbam_swinblock_amd import _lib

    assert {"ymi_psa_attention_fwd", "ymi_psa_attention_bwd"} <= set(_lib.exported_symbols())
