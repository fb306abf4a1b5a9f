"""CPU: the element-by-element CBAM checks of tests/cbam_exact.py, tested themselves.

The float64 restatement reproduces the reference's outputs and gradients in the golden fixtures (free routing: the first-index rule is
the reference's tie rule); the hand-written backward agrees with autograd over the restatement; the dispatch mirror agrees with the
library and the cases reach the branches they claim; a float32 emulation of the kernels' rounding points passes every gate on every
case; each planted fault is flagged with its location at the smallest case that can show it; and the tensor-wide gate of the module
tests accepts two of those faults at the benchmark's CBAM shape - the gap the element-by-element checks close."""
import re

import pytest
import torch
import yaml

import cbam_exact as X
from conftest import ROOT, load_golden

BF, F32 = torch.bfloat16, torch.float32
FIXTURES = ["cbam_lazy_c32", "cbam_c64", "cbam_lazy_c512", "cbam_ties_c32", "cbam_ties_flatca_c32"]
C1, C2, C3, C4, C5, C6, C7 = X.CASES


def dname(dtype):
    return "bf16" if dtype == BF else "f32"


def nhwc(a):
    return torch.from_numpy(a).double().permute(0, 2, 3, 1).contiguous()


def fixture_inputs(d):
    return {"x": nhwc(d["x"]), "dout": nhwc(d["gy"]), "w1": torch.from_numpy(d["w.ca.shared_MLP.0.weight"]).double()[:, :, 0, 0],
            "w2": torch.from_numpy(d["w.ca.shared_MLP.2.weight"]).double()[:, :, 0, 0], "wsa": torch.from_numpy(d["w.sa.conv.weight"]).double()[0]}


# ------------------------------------------------------------------------------------------------------- restatement against the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_fixtures(name):
    """outputs and gradients of the reference (float32 arithmetic, float32 storage) from the float64 restatement with FREE routing: on the
    tie fixtures that is the statement that the first-index rule is the reference's.  Tolerances: float32 noise of the reference."""
    d = load_golden(name)
    inp = fixture_inputs(d)
    leaves = [inp[k].clone().requires_grad_(True) for k in ("x", "w1", "w2", "wsa")]
    f = X.ref_forward(*leaves)
    torch.testing.assert_close(f["out"].detach().float(), nhwc(d["y"]).float(), rtol=1e-5, atol=1e-6)
    if "ca" in d:
        torch.testing.assert_close(f["ca"].detach().float(), torch.from_numpy(d["ca"])[:, :, 0, 0], rtol=1e-5, atol=1e-6)
    gx, gw1, gw2, gwsa = torch.autograd.grad(f["out"], leaves, inp["dout"])
    for got, key in ((gx.permute(0, 3, 1, 2), "g.x"), (gw1[:, :, None, None], "g.ca.shared_MLP.0.weight"), (gw2[:, :, None, None], "g.ca.shared_MLP.2.weight"),
                     (gwsa[None], "g.sa.conv.weight")):
        torch.testing.assert_close(got.float(), torch.from_numpy(d[key]), rtol=1e-4, atol=2e-5, msg=lambda m, key=key: f"{name} {key}: {m}")
    # the hand-written backward (the one the bounds are built on) is autograd's, routed by the given indices
    saved = {k: v.detach() for k, v in f.items()}
    f2 = X.ref_forward(*leaves, pool_argmax=saved["pool_argmax"], smap_argmax=saved["smap_argmax"])
    auto = dict(zip(("dx", "dw1", "dw2", "dwsa"), torch.autograd.grad(f2["out"], leaves, inp["dout"])))
    hand, _, _ = X.ref_backward(inp["x"], inp["dout"], inp["w1"], inp["w2"], inp["wsa"], saved, F32)
    for n in auto:
        torch.testing.assert_close(hand[n], auto[n], rtol=1e-11, atol=1e-13, msg=lambda m, n=n: f"{name} hand {n}: {m}")
        torch.testing.assert_close(auto[n], {"dx": gx, "dw1": gw1, "dw2": gw2, "dwsa": gwsa}[n], rtol=0, atol=0)


# -------------------------------------------------------------------------------------------------------------------------- dispatch mirror
def test_cases_reach_the_branches_they_claim():
    b = {c: X.branches(c) for c in X.CASES}
    assert b[C1]["ksa"] == 3 and b[C1]["map_below_stencil"] and b[C1]["pool_idle_pixel_lanes"] and b[C1]["acc_slots"] == 1 and b[C1]["wsa_tail"]
    assert b[C2]["pool_overhang"] and b[C2]["pool_idle_pixel_lanes"] and b[C2]["map_below_stencil"] and b[C2]["np_not_multiple_of_4"]
    assert 0 < b[C3]["pool_four_in_flight_lanes"] < 16 and b[C3]["pb"] == 2
    assert b[C4]["second_trip_lanes"] == 1 and b[C4]["hidden_above_waves"] and b[C4]["pb"] == 3 and b[C4]["ksa"] == 3 and b[C4]["acc_slots"] == 2
    assert b[C4]["pool_overhang"]
    assert b[C5]["w_unroll_tail"] and not any(b[c]["w_unroll_tail"] for c in X.CASES if c != C5)
    assert b[C6]["wsa_main_and_tail"] and b[C6]["pb"] == 24 and b[C6]["acc_slots"] == 2
    assert b[C7]["acc_slots"] == 4 and b[C7]["pb_capped"] and b[C7]["pb"] == 64 and b[C7]["bwd_pool_grid_stride"] and b[C7]["wsa_main_loop"]
    assert X.ge_blocks(C7[0] * C7[2] * C7[3], C7[1]) == 4096
    assert not any(b[c]["bwd_pool_grid_stride"] or b[c]["pb_capped"] or b[c]["acc_slots"] > 2 for c in X.CASES if c != C7)
    assert not any(b[c]["wsa_main_loop"] for c in (C1, C2, C3, C4, C5))
    assert X.pool_grid(C2[0], C2[1]) == (1, 3) and X.pool_grid(C4[0], C4[1]) == (5, 1) and X.pixel_grid(45) == 12


def test_workspace_mirror_matches_the_library_and_holds_the_carve_up():
    from improving_yolov8_cbam_swinblock_amd import _lib

    assert [X.cbam_pb(v) for v in (1, 32, 33, 72, 750, 2048, 2049, 2112, 10 ** 6)] == [1, 1, 2, 3, 24, 64, 64, 64, 64]
    shapes = list(X.CASES) + [(n, c, h, w, hd, 7) for n in (1, 5) for c in (4, 36, 1024) for h, w in ((1, 1), (3, 5), (47, 45)) for hd in (1, 3, 64)]
    for N, C, H, W, Hd, _ in shapes:
        lay, used = X.workspace_layout(N, H, W, C, Hd)
        need = X.workspace_bytes(N, H, W, C, Hd)
        assert int(_lib.lib().ymi_cbam_bwd_workspace(N, H, W, C, Hd)) == need
        assert used * 4 <= need - 256, (N, C, H, W, Hd)  # the carve-up fits even from a base that had to be moved up to alignment
        offs = sorted(lay.values())
        assert all(o % 4 == 0 for o, _ in offs) and all(o0 + n0 <= o1 for (o0, n0), (o1, _) in zip(offs, offs[1:]))


# ----------------------------------------------------------------------------------------------------------- emulation against the bounds
def run_emulation(case, dtype, ties=False, fwd_fault=None, bwd_fault=None):
    inp = X.make_inputs(case, dtype, ties=ties)
    tag = f"emulation {case} {dname(dtype)}" + (" ties" if ties else "")
    f = X.emu_forward(inp, dtype, fwd_fault)
    rf = X.check_forward(tag, f, inp, dtype)
    b = X.emu_backward(inp, f, dtype, bwd_fault)
    rb, margin = X.check_backward(tag, b, f, inp, dtype)
    return {**rf, **rb}, margin


SMALL = [(c, t) for c in X.CASES[:6] for t in (False,)] + [(C2, True), (C4, True)]


@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
def test_emulation_passes_every_gate_on_every_case(dtype):
    worst = {}
    for case, ties in SMALL + [(C7, False)]:
        ratios, margin = run_emulation(case, dtype, ties)
        assert margin > 1.0, f"{case}: a ReLU gate of the backward lies within float32 rounding of 0 (margin {margin:.3g}); choose another seed"
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"\n[cbam emulation {dname(dtype)}] worst error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) < 1.0


# -------------------------------------------------------------------------------------------------------------------------- planted faults
# fault -> (case, ties, forward fault?, the stage that must be named)
PLANTED = {
    "pool_last_max": (C2, True, True, "pool_argmax"),
    "pool_lane_order_tie": (C4, True, True, "pool_argmax"),
    "pool_drop_last_block": (C2, False, True, "pooled.max"),
    "chan_last_max": (C2, True, True, "smap_argmax"),
    "stats_drop_second_trip": (C4, False, True, "smap.mean"),
    "stencil_not_flipped": (C2, False, False, "dx"),
    "dmean_over_hw": (C1, False, False, "dx"),
    "da_not_over_hw": (C2, False, False, "dx"),
    "drop_part_row": (C2, False, False, "dcap"),
    "drop_pb_partial": (C3, False, False, "dz"),
    "drop_acc_slot3": (C7, False, False, "dcap"),
    "wsa_drop_tail": (C1, False, False, "dwsa"),
    "w_drop_image8": (C5, False, False, "dw1"),
    "hsum_one_relu": (C2, False, False, "hsum"),
}


def test_every_fault_of_the_emulation_is_planted():
    assert set(PLANTED) == set(X.FAULTS)


@pytest.mark.parametrize("fault", list(PLANTED))
@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
def test_planted_fault_is_flagged_with_its_location(fault, dtype):
    case, ties, fwd, stage = PLANTED[fault]
    run_emulation(case, dtype, ties)  # clean: passes
    with pytest.raises(AssertionError) as e:
        run_emulation(case, dtype, ties, fwd_fault=fault if fwd else None, bwd_fault=None if fwd else fault)
    msg = str(e.value)
    assert re.search(rf"stage {re.escape(stage)} \((n|hidden|c|j)=\d+", msg), msg
    for also in {"drop_part_row": ["dw2"], "drop_pb_partial": ["dw2"], "drop_acc_slot3": ["dw2"], "hsum_one_relu": ["dw2"], "w_drop_image8": ["dw1.from_ws", "dw2.from_ws"],
                 "da_not_over_hw": ["dx.from_ws"], "wsa_drop_tail": ["dwsa.from_du"]}.get(fault, []):
        assert f"stage {also} (" in msg, (also, msg)
    assert re.search(r"\d+ of \d+ elements wrong", msg), msg
    if fault == "w_drop_image8":
        assert "stage dw2 (" in msg, msg  # both weight gradients lose the image


def test_a_single_bf16_out_element_off_by_one_ulp_is_flagged():
    """at the element whose magnitude lies closest above a power of two (r |ref| is then about half a bfloat16 ulp), moved away from ref."""
    inp = X.make_inputs(C1, BF)
    f = X.emu_forward(inp, BF)
    X.check_forward("clean", f, inp, BF)
    ref, _ = X.stage_out(inp["x"], f["ca"].double(), f["sa"].double(), BF)
    away = (f["out"].double().abs() >= ref.abs()).reshape(-1)
    frac = (ref.abs() / torch.exp2(torch.floor(torch.log2(ref.abs())))).reshape(-1)
    idx = int(torch.where(away, frac, torch.full_like(frac, 9.0)).argmin())
    assert bool(away[idx])
    bad = dict(f, out=X.bf16_ulp_up(f["out"], idx))
    with pytest.raises(AssertionError, match=r"stage out \(n=0, h=0, w=0, c=%d\)" % idx) as e:
        X.check_forward("one ulp", bad, inp, BF)
    assert "1 of 4 elements wrong" in str(e.value)


# ------------------------------------------------------------------------------------------------------------------------------ gap shown
def benchmark_cbam_shape(imgsz=640):
    """(C, H, W) of the CBAM row of the benchmark model (cfg/models/v8/yolov8.yaml at scale s) at imgsz x imgsz."""
    cfg = yaml.safe_load((ROOT / "improving_yolov8_cbam_swinblock_amd" / "cfg" / "models" / "v8" / "yolov8.yaml").read_text())
    _, width, max_ch = cfg["scales"]["s"]
    ch, stride = 3, 1
    for _, _, mod, args in cfg["backbone"]:
        if mod == "CBAM":
            return ch, imgsz // stride, imgsz // stride
        if mod in ("Conv", "C2f", "SPPF"):
            ch = int(-(-min(args[0], max_ch) * width // 8) * 8)
        if mod == "Conv" and len(args) > 2 and args[2] == 2:
            stride *= 2
    raise AssertionError("no CBAM row")


@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
def test_the_module_gate_accepts_faults_the_element_checks_flag(dtype):
    """at the benchmark's CBAM shape (batch 32 of 640 x 640) the tensor-wide relative-L2 gate of the module tests (1e-3 in float32,
    BF16_MODULE_BOUNDS['CBAM'] in bfloat16) accepts
      (a) one pixel's channel maximum routed to the wrong channel: every gradient within the gate in both dtypes (4e-4 on dx in float32);
      (b) the tail trip of cbam_bwd_wsa_kernel dropped for one thread: dwsa moves by 6.3e-3, inside the bfloat16 gate (1e-2), the
          dtype the benchmark trains in; the float32 gate (1e-3) does see this one, so only the bfloat16 acceptance is asserted.
    tests/cbam_exact.py flags both in both dtypes, with the location."""
    from test_gpu_fuzz import BF16_MODULE_BOUNDS

    C, H, W = benchmark_cbam_shape()
    assert (C, H, W) == (512, 20, 20)
    fwd_gate, grad_gate = (1e-3, 1e-3) if dtype == F32 else BF16_MODULE_BOUNDS["CBAM"]
    case = (32, C, H, W, C // 16, 7)
    inp = X.make_inputs(case, dtype)
    f = X.emu_forward(inp, dtype)
    free = X.ref_forward(inp["x"], inp["w1"], inp["w2"], inp["wsa"])
    ref, _, _ = X.ref_backward(inp["x"], inp["dout"], inp["w1"], inp["w2"], inp["wsa"], free, dtype)
    if dtype == BF:  # the bfloat16 module gate compares with the quantisation-matched reference: out and dx rounded as the module stores them
        free["out"], ref["dx"] = free["out"].to(BF).double(), ref["dx"].to(BF).double()
    assert X.rel(f["out"], free["out"]) <= fwd_gate
    # (a) pixel (n=1, h=7, w=3): the maximum's gradient goes to the channel after the right one
    wrong = dict(f, smap_argmax=f["smap_argmax"].clone())
    wrong["smap_argmax"][1, 7, 3] = (wrong["smap_argmax"][1, 7, 3] + 1) % C
    errs = {n: X.rel(v, ref[n]) for n, v in X.emu_backward(inp, wrong, dtype).items() if n in ref and n != "du"}
    print(f"\n[cbam gap {dname(dtype)}] mis-routed element: " + "  ".join(f"{n} {v:.2e}" for n, v in errs.items()))
    assert max(errs.values()) <= grad_gate, errs
    with pytest.raises(AssertionError, match=r"stage smap_argmax \(n=1, h=7, w=3\)"):
        X.check_forward("mis-routed", wrong, inp, dtype)
    # (b) thread 0 of every block loses its tail trip (its 13th: pixel 12288 = (n=30, h=14, w=8))
    assert X.cdiv(32 * H * W, 1024) == 13
    clean = X.emu_backward(inp, f, dtype)
    dropped = X.emu_backward(inp, f, dtype, fault="wsa_drop_tail_thread0")
    errs = {n: X.rel(v, ref[n]) for n, v in dropped.items() if n in ref and n != "du"}
    print(f"[cbam gap {dname(dtype)}] dropped tail element: " + "  ".join(f"{n} {v:.2e}" for n, v in errs.items()))
    assert not torch.equal(dropped["dwsa"], clean["dwsa"])
    if dtype == BF:
        assert max(errs.values()) <= grad_gate, errs
    X.check_backward("clean", clean, f, inp, dtype)
    with pytest.raises(AssertionError, match=r"stage dwsa.from_du \(j=\d, ky=\d, kx=\d\)"):
        X.check_backward("dropped tail", dropped, f, inp, dtype)
