"""YOLO11-CBAM-Swin without a GPU: scales m and l build with the reference's layer tables (tests/golden/swin512_parse_tables.json, from the
reference's own active yolo11.yaml), the window-attention dispatch above head_dim 192 (the LDS
images, the form chosen, both gates of tests/attn_exact.py on the emulated rounding points) and the oracle's SwinBlock(512, 2) against the
reference's outputs."""
import json

import numpy as np
import pytest
import torch

import attn_exact as A
from conftest import GOLDEN, large_swin_grad_errors, load_large_swin
from psa_common import E2E_NC

BF, F32 = torch.bfloat16, torch.float32
SWIN512 = ["swin_d512_14x14", "swin_d512_9x11", "swin_d512_ws14_16x15"]
WIDE_HDS = (196, 224, 252, 256)


def tables():
    return json.loads((GOLDEN / "swin512_parse_tables.json").read_text())


def form_above_192(L, hd, dtype, tiled_opt=0):
    """swin.hip attn_form for 192 < hd <= 256, restated here (attn_exact.attn_form covers hd <= 192 and stays as it is): bfloat16 windows of at
    most 64 tokens keep the tr kernels (their image fits: attn_lds below); float32 has no one-tile kernel this wide (its backward image would
    need 174,336 B at hdp 224); more than 64 tokens, or the attn_tiled option, is tiled as ever."""
    assert 192 < hd <= 256 and hd % 4 == 0
    if L > 64 or tiled_opt:
        return "tiled"
    return "tr" if dtype == BF else "tiled"


# ---------------------------------------------------------------------------------------------------------------- model tables
@pytest.mark.parametrize("scale", ["m", "l"])
def test_tables_equal_the_reference(scale):
    """The reference counts CBAM's row at parse time, before the stride probe builds its MLP (98 = the 7 x 7 spatial convolution), so `np` is
    compared row by row as test_oracle_golden.py::test_parse_model_tables does and the total separately."""
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    ref = tables()[scale]
    model = DetectionModel(f"yolo11{scale}-cbam-swin.yaml", ch=3, nc=E2E_NC)
    assert [m.type.split(".")[-1] for m in model.model] == [l["type"] for l in ref["layers"]]
    assert [int(m.np) for m in model.model] == [l["np"] for l in ref["layers"]]
    assert [m.f for m in model.model] == [l["f"] for l in ref["layers"]]
    assert [m.i for m in model.model] == [l["i"] for l in ref["layers"]]
    assert list(model.save) == ref["save"] == [4, 7, 10, 17, 20, 23, 26]
    assert [float(s) for s in model.stride] == ref["stride"] == [8.0, 16.0, 32.0]
    assert sum(p.numel() for p in model.parameters()) == ref["params"] == {"m": 27383931, "l": 33106043}[scale]
    assert int(model.model[10].np) == 98 and int(model.model[7].np) == int(model.model[17].np) == 3152384
    assert model.model[7].attn.num_heads == 2 and model.model[7].dim == 512 and model.model[10].ca.shared_MLP[0].weight.shape[0] == 512 // 16


def test_state_dict_keys_and_shapes_equal_the_reference():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    ref = tables()["m"]["state"]
    got = {k: list(v.shape) for k, v in DetectionModel("yolo11m-cbam-swin.yaml", ch=3, nc=E2E_NC).state_dict().items()}
    assert got == ref


def test_yaml_resolves_by_scale_and_carries_the_active_rows():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import yaml_model_load

    d = yaml_model_load("yolo11l-cbam-swin.yaml")
    rows = d["backbone"] + d["head"]
    assert d["scale"] == "l" and d["nc"] == 1 and len(rows) == 28
    assert [(i, r[2]) for i, r in enumerate(rows) if r[2] in ("SwinBlock", "CBAM", "C2PSA")] == [
        (7, "SwinBlock"), (10, "CBAM"), (12, "C2PSA"), (13, "C2PSA"), (17, "SwinBlock")]
    assert rows[7][3] == [512] and rows[17][3] == [512] and rows[15][0] == [-1, 7] and rows[22][0] == [-1, 17] and rows[25][0] == [-1, 10]
    assert rows[27][0] == [20, 23, 26]


# ---------------------------------------------------------------------------------------------------------------- dispatch mirror
def test_lds_images_above_head_dim_192():
    """the tr images fit at every width up to 256; the float32 one-tile backward does not (so float32 goes to the tiled kernels, whose image
    does not depend on the head width)."""
    for hd in range(196, 257, 4):
        hdp = (hd + 31) // 32 * 32
        fwd, bwd = A.attn_lds(64, hd, True, False)[1], A.attn_lds(64, hd, True, True)[1]
        assert (fwd, bwd) == {224: (98304, 137216), 256: (110592, 153600)}[hdp], (hd, fwd, bwd)
        assert bwd <= A.LDS_MAX
        assert A.attn_lds(64, hd, False, True)[0] == {224: 174336, 256: 191744}[hdp] > A.LDS_MAX
    # the widths that run today are as they were
    assert A.attn_lds(64, 192, True, True)[1] == 120832 and A.attn_lds(64, 192, False, True)[0] == 156928


def test_dispatch_rule_above_head_dim_192():
    for hd in range(196, 257, 4):  # (the same form serves both directions)
        for L in (1, 49, 64):
            assert form_above_192(L, hd, BF) == "tr" and form_above_192(L, hd, F32) == "tiled"
            assert form_above_192(L, hd, BF, 1) == "tiled"
        for L in (65, 196, 256):
            assert form_above_192(L, hd, BF) == "tiled" and form_above_192(L, hd, F32) == "tiled"
    # at 192 and below the old mirror speaks, unchanged
    assert A.attn_form(64, 192, F32, 0, True) == "onetile-f32" and A.attn_form(49, 192, BF, 0, True) == "tr"


def test_library_holds_both_tile_counts_and_no_bf16_one_tile_kernel():
    """the tr and tiled kernels exist with 12 and 16 head-dimension tiles; the one-tile kernels keep their float32-only form."""
    from improving_yolov8_cbam_swinblock_amd._lib import LIB_PATH

    if not LIB_PATH.exists():
        pytest.skip("libyolo_mi355.so is not built: no kernel names to read (build() makes it before the suite runs)")
    image = LIB_PATH.read_bytes()
    for kernel in ("window_attn_fwd_tr_kernel", "window_attn_bwd_tr_kernel"):
        for n in (12, 16):
            assert f"{kernel}ILi{n}EE".encode() in image, (kernel, n)
    for kernel in ("window_attn_tiled_fwd_kernel", "window_attn_tiled_dq_kernel", "window_attn_tiled_dkv_kernel"):
        for ty in ("f", "DF16b"):
            for n in (12, 16):
                assert f"{kernel}I{ty}Li{n}EE".encode() in image, (kernel, ty, n)
    for name in ("window_attn_fwd_kernelIDF16b", "window_attn_bwd_kernelIDF16b"):
        assert name.encode() not in image, name


# ------------------------------------------------------------------------------------------------------- both gates on the emulation
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _real(shape, gen, dtype, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype).float()


def _emu_all(form, dtype, q, k, v, dO):
    O, lse = A.emu_attn_fwd(form, q, k, v, dtype)
    got = {"O": O, "lse": lse}
    got.update(A.emu_attn_bwd(form, q, k, v, O, dO, lse, dtype))
    return got


FORMS = [("tr", BF), ("tiled", BF), ("tiled", F32)]
FORM_IDS = [f"{f}-{'bf16' if d == BF else 'f32'}" for f, d in FORMS]


@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
def test_gate1_emulation_exact_above_192(form, dtype):
    g = _gen(41)
    for L in ([1, 49, 64] if form == "tr" else [1, 49, 64, 65, 196]):
        for hd in WIDE_HDS:
            assert A.onehot_ok(L, hd)
            q, k, v, dO, pi = A.onehot_operands(2, 2, L, hd, g)
            q, k, v, dO = (t.to(dtype).float() for t in (q, k, v, dO))
            what = f"emu {form} L{L} hd{hd}"
            A.onehot_check(q, k, pi, what)
            exp = A.onehot_expected(q, k, v, dO, dtype)
            A.check_onehot(what, _emu_all(form, dtype, q, k, v, dO), exp, form, ("O", "lse", "dV", "dQ", "dK"))


@pytest.mark.parametrize("form,dtype", FORMS, ids=FORM_IDS)
def test_gate2_emulation_within_bound_above_192(form, dtype):
    """attn_exact's derived per-element bound, unchanged: the emulated rounding points of each form at the new widths stay inside it."""
    worst = {}
    Ls = [49, 64, 33] if form == "tr" else [49, 65, 196]
    for si, (L, hd) in enumerate((L, hd) for L in Ls for hd in WIDE_HDS):
        for rep in range(2):
            g = _gen(700 + 10 * si + rep)
            sh = (2, 2, L, hd)
            qk = 3.0 if rep % 2 else 1.0
            q, k = _real(sh, g, dtype, qk), _real(sh, g, dtype, qk)
            v, dO = _real(sh, g, dtype), _real(sh, g, dtype)
            ref = A.attn_ref64(q, k, v, dO)
            b = A.attn_bounds(q, k, v, dO, ref, dtype, form)
            got = _emu_all(form, dtype, q, k, v, dO)
            for n in ("O", "lse", "dV", "dQ", "dK"):
                worst[n] = max(worst.get(n, 0.0), A.check_bound(f"emu {form} L{L} hd{hd} {n}", got[n], ref[n], b[n], A.locate_attn(form)))
    print(f"emulated {form} {dtype} hd 196..256: worst Gate 2 ratio " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    assert all(w <= 1.0 for w in worst.values())


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("name", SWIN512)
def test_oracle_swin_block_512(name):
    """oracle.modules.SwinBlock(512, 2) against the reference's outputs, with the bounds test_oracle_golden.py uses for LARGE_SWIN."""
    from oracle import modules as OM

    m, x, gy, d, seeded = load_large_swin(name, lambda dim, heads, ws: OM.SwinBlock(dim, heads, ws))
    assert seeded and m.attn.num_heads == 2 and m.attn.embed_dim == 512
    x = x.requires_grad_(True)
    y = m(x)
    torch.testing.assert_close(y, torch.from_numpy(np.asarray(d["y"])), rtol=1e-4, atol=2e-5)
    grads = torch.autograd.grad(y, [x] + list(m.parameters()), gy)
    torch.testing.assert_close(grads[0], torch.from_numpy(np.asarray(d["g.x"])), rtol=1e-4, atol=1e-4)
    for n, emax, erel in large_swin_grad_errors(d, seeded, [k for k, _ in m.named_parameters()], grads[1:]):
        assert erel < 1e-4 or emax < 1e-5, (n, emax, erel)
