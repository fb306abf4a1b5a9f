"""CPU: the element-by-element checks of tests/first_conv_exact.py, tested themselves.

A float64 model of the first-layer kernels (ideal arithmetic with the stored roundings) passes every stage on every kind of operands; each
planted fault - one at a time - is flagged at the stage it belongs to; and the tensor-wide relative-L2 gates of tests/test_gpu_first_conv.py
(2e-3 on the output, 5e-3 on the gradients, at their own tolerance) accept the placement faults at the same shape: the gap the element
checks close.  The shapes of those demonstrations are the smallest at which the old gate lets the fault through - it is a property of the
gate that a fault of k pixels out of P passes once k / P is below (2e-3 / relative size)^2:
    one tap of one corner pixel shifted by a column          2 x 3 x 160 x 640    1 pixel of 51,200
    the last partial 16-pixel group out of the statistics    1 x 3 x 4 x 40964    2 pixels of 20,482 per row (the output moves through scale / shift only;
                                                             the 1e-4 gate on the buffers is the one that needs this width: 6.3e-4 at w = 5124)
    a biased variance in running_var                         2 x 3 x 160 x 640    var / P: the buffers' 1e-4 gate sees it at P = 1188 (4.5e-4), not at 51,200
    image 1's top halo row read from image 0's last row      2048 x 3 x 128 x 4   2 pixels of 262,144: the gate does notice this fault at
                                                             ordinary shapes (6.3e-3 at 32 x 3 x 640 x 4) and lets it pass from ~10^5 output rows on
The rounding faults (truncation, bfloat16 accumulation, statistics of the unrounded convolution, a d(raw) left in float32, xhat of the
unrounded raw) are shown at the shapes of the GPU cases; what the old gates make of them is printed.
The case list of the GPU tests is checked against the geometry it claims, recomputed here from the shapes, and the geometry mirror
against the library."""
import pytest
import torch

import first_conv_exact as X
import gemm_exact as G

OUT_GATE, GRAD_GATE = 2e-3, 5e-3  # tests/test_gpu_first_conv.py _same_block


def stages(err):
    return {line.split("stage ")[1].split(" ")[0] for line in str(err.value).split("\n") if "stage " in line and "wrong" in line}


# ------------------------------------------------------------------------------------------------------------------------------- the helpers
def test_bfloat16_rounding_of_float64_is_one_rounding():
    g = torch.Generator().manual_seed(0)
    v = torch.randn(100000, generator=g, dtype=torch.float64) * torch.exp2(torch.randint(-20, 20, (100000,), generator=g).double())
    f = v.float()  # float32 values: torch's own float32 -> bfloat16 conversion is round-to-nearest-even of these
    assert torch.equal(X.rne_bf16(f.double()), f.to(torch.bfloat16).double())
    assert torch.equal(X.trunc_bf16(f.double()), (f.view(torch.int32) & -65536).view(torch.float32).double())
    # a float64 just above a bfloat16 tie: through float32 it lands ON the tie and then rounds to even - the wrong side
    tie = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30], dtype=torch.float64)
    assert float(X.rne_bf16(tie)) == 1.0 + 2.0 ** -7 and float(tie.float().to(torch.bfloat16)) == 1.0
    assert torch.equal(X.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.75, 300.0], dtype=torch.float64)), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0], dtype=torch.float64))


def test_silu_derivative_constant_follows_the_convention():
    """twice the measured worst value, rounded up to one digit"""
    assert X.SILU_GRAD_F32 == 2e-7 and 2 * X.MEASURED_SILU_GRAD <= X.SILU_GRAD_F32 < 2 * X.MEASURED_SILU_GRAD + 1e-7


# -------------------------------------------------------------------------------------------------------------------------- geometry claimed
def test_geometry_mirror_matches_the_library():
    from improving_yolov8_cbam_swinblock_amd import _lib

    L = _lib.lib()
    for n, h, w in list(X.SHAPES.values()) + [(32, 640, 640), (4, 640, 640)]:
        g = X.geometry(n, h, w)
        assert int(L.ymi_first_conv_stat_blocks(n, h, w)) == g["units"]
        for co in (16, 32, 48, 64):
            assert int(L.ymi_first_conv_bwd_workspace(n, h, w, co)) == (g["units"] * 2 * co + 5 * co + g["wgs"] * co * 72) * 4 + 1024
    assert (_lib.ACT_NONE, _lib.ACT_SILU, _lib.ACT_GELU) == (X.ACT_NONE, X.ACT_SILU, X.ACT_GELU)
    assert X.geometry(32, 640, 640)["units"] == 6400 and X.geometry(32, 640, 640)["staged"] and not X.geometry(4, 640, 640)["staged"]


def test_cases_reach_the_geometry_they_claim():
    g = {k: X.geometry(*v) for k, v in X.SHAPES.items()}
    pick = lambda k, *names: tuple(g[k][q] for q in names)  # noqa: E731
    assert pick("sub", "tiles_h", "tiles_w", "units", "last_tile_w", "last_tile_rows") == (1, 1, 3, 4, 4)  # smaller than a tile
    assert pick("one", "units", "last_tile_w", "last_tile_rows", "wgs") == (1, X.FC_TW, X.FC_TH, 1)  # exactly one tile
    assert pick("2x2", "tiles_h", "tiles_w", "units", "last_tile_w", "last_tile_rows", "wgs", "last_wg_tiles") == (2, 2, 8, 2, 1, 2, 4)
    assert pick("3x2", "tiles_h", "tiles_w", "units", "last_tile_w", "wgs", "last_wg_tiles") == (3, 2, 6, 30, 2, 2) and 30 % 16 != 0
    assert pick("5", "tiles_h", "tiles_w", "units", "wgs", "last_wg_tiles", "last_tile_w") == (1, 5, 5, 2, 1, X.FC_TW)
    assert pick("1100", "units", "wgs", "last_tile_rows", "last_tile_w", "staged") == (1100, 275, 1, 2, True)
    assert not any(g[k]["staged"] for k in g if k != "1100") and 1100 > 16 * X.BN_STAGE_ROWS
    multi = [s for s in X.CASES if g[s[1]]["units"] // X.SHAPES[s[1]][0] > 1]  # more than one tile per image
    assert {s[3] for s in multi} == {16, 32, 48, 64} and {s[2] for s in multi} == {1, 2, 3, 4}
    assert {s[1] for s in X.CASES if s[0] == "int"} == set(X.SHAPES)  # every shape under Gate 1
    assert {s[0] for s in X.CASES} == {"int", "dyadic", "pos"} and all(g[s[1]]["units"] > 1 for s in X.CASES if s[0] == "pos")
    assert len(set(X.CASES)) == len(X.CASES)
    # ymi_bn_finalize: fewer rows than slices, tail only, main loop without and with a tail, several trips, the last count without
    # staging and the first with it, layer 0's count at batch 32
    B = X.FIN_BLOCKS
    assert B == (1, 31, 32, 33, 96, 97, 128, 129, 400, 1024, 1025, 1088, 6400)
    fw = {b: X.finalize_walk(b) for b in B}
    fin = lambda b: (fw[b]["final"]["main"], fw[b]["final"]["tail"], fw[b]["final"]["idle"])  # noqa: E731
    assert fin(1) == (0, 1, 31) and fin(31) == (0, 1, 1) and fin(32) == (0, 1, 0) and fin(33) == (0, 2, 0) and fin(96) == (0, 3, 0)
    assert fin(97) == (1, 3, 0) and fin(128) == (1, 0, 0) and fin(129) == (1, 1, 0) and fin(400) == (3, 1, 0) and fin(1024) == (8, 0, 0)
    assert not fw[1024]["staged"] and all(fw[b]["staged"] and fin(b) == (0, 2, 0) for b in (1025, 1088, 6400))
    assert fw[1025]["stage"] == {"main": 1, "tail": 1, "idle": 0} and fw[1088]["stage"] == {"main": 1, "tail": 1, "idle": 0}
    assert fw[6400]["stage"]["main"] == 6 and fw[6400]["stage"]["tail"] >= 1
    assert 1024 == 16 * X.BN_STAGE_ROWS and X.geometry(32, 640, 640)["units"] == 6400
    for b in B:
        rows, count = X.finalize_rows(b, 80)
        assert count == 8 * b and float(rows[:, 0].abs().max()) <= 8 and 64 <= float(rows[:, 1].min()) and float(rows[:, 1].max()) <= 128
        if b > 1:
            assert bool((rows[1:] != rows[:-1]).any(0).all()) and bool((rows[:, :, 1:] != rows[:, :, :-1]).any())


# ------------------------------------------------------------------------------------------------------------ the model passes every stage
SMALL = [s for s in X.CASES if s[1] != "1100"] + [("int", "1100", 3, 16)]


@pytest.mark.parametrize("act", [X.ACT_NONE, X.ACT_SILU], ids=["none", "silu"])
def test_the_model_passes_every_stage_on_every_case(act):
    worst = {}
    for spec in SMALL:
        case = X.case_of(spec)
        ratios = X.check_forward(f"model {case}", X.model_forward(case, act), case, act)
        if case.exact:
            for affine in (True, False):
                ratios.update(X.check_backward(f"model {case}", X.model_backward(case, act, affine), case, act, affine))
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\n[first conv model] worst error / bound: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst.pop("undecided") <= 0.01  # pixels whose d(raw) the reference cannot decide
    assert max(worst.values()) <= 1.0


def test_gate2_undecided_share_at_the_documented_shape():
    """2 x 3 x 48 x 264 -> 32 channels, operands uniform in [0.25, 1], gamma(64): 0.13 % of the elements have two candidates; signed
    operands (2.3 %) are not used for this gate"""
    r = X.forward_reference(X.make_case("pos", 2, 3, 48, 264, 32))
    assert 0.0005 <= r.share <= 0.003, r.share


# ---------------------------------------------------------------------------------------------------------------------------- planted faults
# fault -> (kind, n, c, h, w, cout, the stages that must be named, whether the old L2 gate must accept it at this shape)
FORWARD = {
    "tap_shift_corner": ("int", 2, 3, 160, 640, 16, {"out", "partials"}, True),
    "halo_from_previous_image": ("int", 2048, 3, 128, 4, 16, {"out", "partials"}, True),
    "stats_drop_partial_group": ("int", 1, 3, 4, 40964, 16, {"partials", "save_mean", "save_invstd", "running_var"}, True),
    "truncate": ("pos", 2, 3, 18, 132, 32, {"out"}, False),
    "bf16_accumulate": ("pos", 2, 3, 18, 132, 32, {"out"}, False),
    "biased_running_var": ("int", 2, 3, 160, 640, 16, {"running_var"}, True),
    "stats_unrounded": ("dyadic", 2, 3, 18, 132, 48, {"save_invstd", "partials"}, True),
}
BACKWARD = {
    "draw_f32": ("int", 2, 3, 18, 132, 32, {"dW"}, True),
    "dw_drop_pixel": ("int", 1, 3, 16, 640, 64, {"dW"}, True),
    "dgamma_unrounded_xhat": ("dyadic", 2, 3, 18, 132, 48, {"dgamma"}, True),
}


def test_every_fault_of_the_model_is_planted():
    assert set(FORWARD) == set(X.FWD_FAULTS) and set(BACKWARD) == set(X.BWD_FAULTS)


@pytest.mark.parametrize("fault", list(FORWARD))
def test_planted_forward_fault_is_flagged(fault):
    kind, n, c, h, w, co, want, accepted = FORWARD[fault]
    case = X.make_case(kind, n, c, h, w, co)
    for act in (X.ACT_SILU,) if n * h * w > 100000 else (X.ACT_NONE, X.ACT_SILU):
        clean = X.model_forward(case, act)
        X.check_forward("clean", clean, case, act)
        bad = X.model_forward(case, act, fault)
        with pytest.raises(AssertionError) as e:
            X.check_forward(fault, bad, case, act)
        assert want <= stages(e), (want, stages(e))
        assert "elements wrong" in str(e.value)
        old = G.rel(bad["out"], clean["out"])
        buf = max(G.rel(bad[k], clean[k]) for k in ("running_mean", "running_var"))
        print(f"\n[first conv fault] {fault} at {case} act {act}: flagged at {sorted(stages(e))}; old gates: out {old:.2e} (gate {OUT_GATE:.0e}) buffers {buf:.2e} (gate 1e-4)")
        if accepted:
            assert old <= OUT_GATE and buf <= 1e-4, (old, buf)
        if fault in ("tap_shift_corner", "halo_from_previous_image"):
            where = "n=%d, h=%d, w=%d" % ((n - 1, h // 2 - 1, w // 2 - 1) if fault == "tap_shift_corner" else (1, 0, 0))
            assert where in str(e.value), str(e.value)  # the element is named


@pytest.mark.parametrize("fault", list(BACKWARD))
def test_planted_backward_fault_is_flagged(fault):
    kind, n, c, h, w, co, want, accepted = BACKWARD[fault]
    case = X.make_case(kind, n, c, h, w, co)
    for act, affine in ((X.ACT_SILU, True), (X.ACT_NONE, True), (X.ACT_SILU, False)):
        clean = X.model_backward(case, act, affine)
        X.check_backward("clean", clean, case, act, affine)
        bad = X.model_backward(case, act, affine, fault)
        with pytest.raises(AssertionError) as e:
            X.check_backward(fault, bad, case, act, affine)
        assert stages(e) == want, (want, stages(e))
        old = max(G.rel(bad[k], clean[k]) for k in clean)
        print(f"\n[first conv fault] {fault} at {case} act {act} affine {affine}: flagged at {sorted(stages(e))}; old gate: {old:.2e} (gate {GRAD_GATE:.0e})")
        if accepted:
            assert old <= GRAD_GATE, old


def test_a_single_out_element_one_bfloat16_step_off_is_flagged():
    """Gate 2: the element moved one bfloat16 step away from both candidates' references"""
    case = X.make_case("pos", 2, 3, 18, 132, 32)
    out = X.model_forward(case, X.ACT_SILU)
    X.check_forward("clean", out, case, X.ACT_SILU)
    r = X.forward_reference(case)
    ref, _ = X.out_reference(r.raw, r.stats, case.gamma, case.beta, X.ACT_SILU)
    v = out["out"].clone()
    c, wl = divmod(int(ref[1, :, 8, 64:].abs().argmax()), 2)  # the largest element of the last tile (one row, two pixels) of image 1
    idx = (1, c, 8, 64 + wl)
    step = X.ulp_bf16(v[idx]) * (1.0 if v[idx] >= ref[idx] else -1.0)
    v[idx] += 1.5 * step
    with pytest.raises(AssertionError, match=r"1 of \d+ elements wrong") as e:
        X.check_forward("one step", dict(out, out=v), case, X.ACT_SILU)
    assert f"(n=1, h=8, w={64 + wl}, c={c})" in str(e.value) and "unit 7 (tile row 1, column 1)" in str(e.value)


def test_a_dropped_or_doubled_finalize_row_moves_a_sum():
    rows, count = X.finalize_rows(1025, 48)
    one = torch.ones(48)
    ref = X.finalize_reference(rows, count, one, 0 * one, 0 * one, one)
    X.check_finalize("clean", {k: ref[k] for k in ("scale", "shift", "save_mean", "save_invstd", "running_mean", "running_var")}, ref)
    for bad_rows in (rows[:-1], torch.cat([rows, rows[1024:]]), torch.cat([rows[:64], rows[65:]])):
        bad = X.finalize_reference(bad_rows, count, one, 0 * one, 0 * one, one)
        with pytest.raises(AssertionError):
            X.check_finalize("row", {k: bad[k] for k in ("scale", "save_invstd")}, ref)
