"""CPU: the element-wise Swin checks of tests/attn_exact.py - the dispatch mirror, both gates against a float32 emulation of every kernel
form's rounding points, and planted faults that the checks must flag with their location.

Where the suite's tensor-wide relative-L2 gate (4e-3 forward, 1e-2 gradients: test_gpu_bf16_matched.py FWD_BOUND / GRAD_BOUND) accepts
the same fault at the benchmark's attention shape (56448 tokens, C = 256, 2 heads, 49-token windows), that is asserted too: it is the
gap these checks close."""
import pytest
import torch

import attn_exact as A

BF, F32 = torch.bfloat16, torch.float32
FWD_GATE = 4e-3  # the forward relative-L2 gate (the gradient gate, 1e-2, already flags the gradient faults planted here)
FORMS = [("tr", BF), ("onetile-f32", F32), ("tiled", BF), ("tiled", F32)]
BENCH_T, BENCH_C, BENCH_HEADS, BENCH_L = 56448, 256, 2, 49


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _raises(fn, *args, **kw):
    with pytest.raises(AssertionError) as e:
        fn(*args, **kw)
    return str(e.value)


def _real(shape, gen, dtype, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype).float()


def _emu_all(form, dtype, q, k, v, dO):
    O, lse = A.emu_attn_fwd(form, q, k, v, dtype)
    got = {"O": O, "lse": lse}
    got.update(A.emu_attn_bwd(form, q, k, v, O, dO, lse, dtype))
    return got


# ---------------------------------------------------------------------------------------------------------------- 1. dispatch mirror
def test_generic_bf16_one_tile_kernels_are_unreachable():
    """window_attn_fwd_kernel<bf16_t> / window_attn_bwd_kernel<bf16_t> would run only if the tr kernels' LDS exceeded 160 KiB at L <= 64; it
    never does for a head_dim the launcher accepts (<= 192, a multiple of 4), nor does the float32 one-tile image, so the launchers do not
    look at the size and the library does not hold the bfloat16 instantiations."""
    for hd in range(4, 193, 4):
        for bwd in (False, True):
            _, lds_tr = A.attn_lds(64, hd, True, bwd)
            assert lds_tr <= A.LDS_MAX, (hd, bwd, lds_tr)
            assert A.attn_lds(64, hd, False, bwd)[0] <= A.LDS_MAX, (hd, bwd)
            for L in range(1, 65):
                assert A.attn_form(L, hd, BF, 0, bwd) == "tr", (L, hd, bwd)
                assert A.attn_form(L, hd, BF, 1, bwd) == "tiled"
            assert A.attn_form(65, hd, BF, 0, bwd) == "tiled"
    # the float32 one-tile backward at head_dim 192: 156,928 of 163,840 bytes
    assert A.attn_lds(64, 192, False, True)[0] == 156928
    assert A.attn_form(64, 192, F32, 0, True) == "onetile-f32"
    # every launched kernel's mangled name is in the library as a registration string
    from improving_yolov8_cbam_swinblock_amd._lib import LIB_PATH

    if not LIB_PATH.exists():
        return  # not built: the dispatch mirror above is all there is to check
    image = LIB_PATH.read_bytes()
    for name in ("window_attn_fwd_kernelIf", "window_attn_bwd_kernelIf", "window_attn_fwd_tr_kernel", "window_attn_bwd_tr_kernel"):
        assert name.encode() in image, name
    for name in ("window_attn_fwd_kernelIDF16b", "window_attn_bwd_kernelIDF16b"):
        assert name.encode() not in image, name


def test_stage_and_layernorm_forms():
    assert A.stage_width(128, [(1 << 20, 768), (1 << 20, 256)]) == 16
    assert A.stage_width(128, [((1 << 20) + 8, 768)]) == 8  # 4 bfloat16 elements off
    assert A.stage_width(20, [(1 << 20, 768)]) == 8
    assert A.stage_width(128, [(1 << 20, 772)]) == 8
    assert A.ln_form(256, BF, 256, 256, [0, 256, 512, 1024]) == "half"
    assert A.ln_form(256, BF, 260, 256, [0, 256, 512, 1024]) == "G1"
    assert A.ln_form(252, BF, 252, 252, [0, 256, 512, 1024]) == "G1"  # 252 % 8 != 0
    assert A.ln_form(516, F32, 516, 516, [0] * 4) == "G3"
    assert A.ln_form(1024, BF, 1024, 1024, [0] * 4) == "G4"
    assert A.ln_bwd_blocks(1) == 1 and A.ln_bwd_blocks(56448) == 1764 and A.ln_bwd_blocks(112896) == 2048


# ------------------------------------------------------------------------------------------------------- 2. both gates pass the emulation
@pytest.mark.parametrize("form,dtype", FORMS, ids=[f"{f}-{'bf16' if d == BF else 'f32'}" for f, d in FORMS])
def test_gate1_emulation_exact(form, dtype):
    g = _gen(11)
    Ls = [1, 4, 8, 16, 49, 64] if form != "tiled" else [1, 4, 8, 16, 49, 64, 65, 196]
    for L in Ls:
        for hd in (4, 8, 12, 20, 128, 192):
            if not A.onehot_ok(L, hd):
                continue
            q, k, v, dO, pi = A.onehot_operands(2, 2, L, hd, g)
            q, k, v, dO = (t.to(dtype).float() for t in (q, k, v, dO))
            what = f"emu {form} L{L} hd{hd}"
            A.onehot_check(q, k, pi, what)
            exp = A.onehot_expected(q, k, v, dO, dtype)
            A.check_onehot(what, _emu_all(form, dtype, q, k, v, dO), exp, form, ("O", "lse", "dV", "dQ", "dK"))


def test_gate1_refuses_a_case_that_is_not_one_hot():
    g = _gen(12)
    q, k, v, dO, pi = A.onehot_operands(1, 1, 16, 8, g)
    assert "not a one-hot case" in _raises(A.onehot_check, q, k * 0.25, pi, "weak")
    assert not A.onehot_ok(16, 4) and A.onehot_ok(8, 4) and A.onehot_ok(128, 8) and not A.onehot_ok(129, 8) and A.onehot_ok(256, 12)


GATE2_SHAPES = [(16, 4), (49, 20), (64, 128), (49, 192), (33, 100)]
GATE2_TILED = [(65, 96), (100, 48), (196, 128)]


@pytest.mark.parametrize("form,dtype", FORMS, ids=[f"{f}-{'bf16' if d == BF else 'f32'}" for f, d in FORMS])
def test_gate2_emulation_within_bound(form, dtype):
    worst = {}
    shapes = GATE2_SHAPES + (GATE2_TILED if form == "tiled" else [])
    for si, (L, hd) in enumerate(shapes):
        for rep in range(6):
            g = _gen(100 * si + rep)
            sh = (3, 2, L, hd)
            qk = 3.0 if rep % 2 else 1.0
            q, k = _real(sh, g, dtype, qk), _real(sh, g, dtype, qk)
            v, dO = _real(sh, g, dtype), _real(sh, g, dtype)
            ref = A.attn_ref64(q, k, v, dO)
            b = A.attn_bounds(q, k, v, dO, ref, dtype, form)
            got = _emu_all(form, dtype, q, k, v, dO)
            for n in ("O", "lse", "dV", "dQ", "dK"):
                worst[n] = max(worst.get(n, 0.0), A.check_bound(f"emu {form} L{L} hd{hd} {n}", got[n], ref[n], b[n], A.locate_attn(form)))
    print(f"emulated {form} {dtype}: worst Gate 2 ratio " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))
    assert all(w <= 1.0 for w in worst.values())


LN_CASES = [(4, 0, None), (12, 3, (1, 5, 7)), (64, 7, (2, 9, 11)), (252, 7, (1, 8, 13)), (256, 14, (1, 15, 17)), (260, 0, None),
            (516, 3, (2, 4, 5)), (1024, 7, (1, 7, 9))]


def _ln_inputs(C, ws, geo, dtype, g):
    if ws == 0:
        T = 37
        x = _real((T, C), g, dtype, 2.0) + 0.5
        pix = None
    else:
        n, h, w = geo
        img = (_real((n, h, w, C), g, dtype, 2.0) + 0.5).to(dtype).float()
        x, pix = A.window_tokens(img, ws)
    gam = torch.randn(C, generator=g) * 0.5 + 1.0
    bet = torch.randn(C, generator=g) * 0.3
    return x.to(dtype).float(), pix, gam, bet


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_layernorm_emulation_within_bound(dtype):
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    worst = {}
    for i, (C, ws, geo) in enumerate(LN_CASES):
        g = _gen(200 + i)
        x, pix, gam, bet = _ln_inputs(C, ws, geo, dtype, g)
        out, mu, rs = A.emu_ln_fwd(x, gam, bet, eps, dtype)
        ref = A.ln_fwd_ref64(x, gam, bet, eps)
        b = A.ln_fwd_bounds(x, gam, bet, eps, ref, dtype)
        worst["out"] = max(worst.get("out", 0), A.check_bound("emu ln out", out, ref["out"], b["out"]))
        worst["mean"] = max(worst.get("mean", 0), A.check_bound("emu ln mean", mu, ref["mu"].squeeze(1), b["mu"] + 1e-300))
        worst["rstd"] = max(worst.get("rstd", 0), A.check_bound("emu ln rstd", rs, ref["rstd"].squeeze(1), b["rstd"]))
        dy = _real(x.shape, g, dtype)
        if pix is not None:
            dy[pix < 0] *= 8
        add = _real(x.shape, g, dtype)
        for a in (None, add):
            dx, dgam, dbet = A.emu_ln_bwd(x, dy, gam, mu, rs, dtype, a)
            r2 = A.ln_bwd_ref64(x, dy, gam, mu, rs, a)
            b2 = A.ln_bwd_bounds(dy, r2, dtype, a)
            for n, v in (("dx", dx), ("dgamma", dgam), ("dbeta", dbet)):
                worst[n] = max(worst.get(n, 0), A.check_bound(f"emu ln {n}", v, r2[n], b2[n]))
    print(f"emulated LayerNorm {dtype}: worst Gate 2 ratio " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()))


def test_layernorm_parameter_tree_counts_the_cap():
    """at the model's token counts the 2048-block cap puts several tokens on each wave: the bound counts them."""
    assert A.ln_tree_adds(112896) == 14 + 3 + 16 + 3 + 2
    assert A.ln_tree_adds(5) == 2 + 3 + 1 + 3 + 2  # one block of four waves: two tokens on wave 0


# ------------------------------------------------------------------------------------------------------------------ 3. planted faults
def _onehot(seed, nw, heads, L, hd, dtype=BF):
    q, k, v, dO, pi = A.onehot_operands(nw, heads, L, hd, _gen(seed))
    return q, k, v, dO, pi, A.onehot_expected(q, k, v, dO, dtype)


_BENCH = {}


def _bench_attention():
    """N(0, 1) bfloat16 q, k, v at the benchmark's attention shape and the float64 O (cached: two tests use it)."""
    if not _BENCH:
        g = _gen(22)
        sh = (BENCH_T // BENCH_L, BENCH_HEADS, BENCH_L, BENCH_C // BENCH_HEADS)
        q, k, v = _real(sh, g, BF), _real(sh, g, BF), _real(sh, g, BF)
        _BENCH["v"] = (q, k, v, A.attn_ref64(q, k, v)["O"])
    return _BENCH["v"]


def test_unmasked_padding_key_is_flagged_and_passes_the_relative_gate():
    q, k, v, dO, pi, exp = _onehot(21, 3, 2, 49, 128)
    O, lse = A.emu_attn_fwd("tr", q, k, v, BF, unmask=(1, 0))
    msg = _raises(A.check_onehot, "fwd", {"O": O, "lse": lse}, exp, "tr", ("O",))
    assert "window=1, head=0" in msg and "form tr" in msg
    # on real operands at the benchmark's attention shape the relative-L2 gate accepts the same fault
    q, k, v, full = _bench_attention()
    good, _ = A.emu_attn_fwd("tr", q[:4], k[:4], v[:4], BF)
    bad, _ = A.emu_attn_fwd("tr", q[:4], k[:4], v[:4], BF, unmask=(1, 0))
    r = float((bad - good).double().norm() / full.norm())
    assert 0 < r <= FWD_GATE, r


def test_last_query_taking_row_l_minus_2_is_flagged():
    q, k, v, dO, pi, exp = _onehot(23, 3, 2, 49, 128)
    O, lse = A.emu_attn_fwd("tr", q, k, v, BF)
    O[2, :, 48] = O[2, :, 47]
    if bool((O[2, :, 48] == exp["O"][2, :, 48].float()).all()):
        pytest.fail("targets of rows 47 and 48 coincide in both heads: pick another seed")
    msg = _raises(A.check_onehot, "fwd", {"O": O, "lse": lse}, exp, "tr", ("O",))
    assert "window=2" in msg and "token=48" in msg
    # the relative-L2 gate accepts the same fault on real operands at the benchmark's shape
    full = _bench_attention()[3]
    bad = full.clone()
    bad[2, 0, 48] = bad[2, 0, 47]
    assert 0 < A.rel(bad, full) <= FWD_GATE


def test_dk_written_into_the_neighbouring_heads_columns_is_flagged():
    q, k, v, dO, pi, exp = _onehot(24, 3, 2, 49, 128)
    O, lse = A.emu_attn_fwd("tr", q, k, v, BF)
    got = A.emu_attn_bwd("tr", q, k, v, O, dO, lse, BF)
    dK = got["dK"].clone()
    dK[1, 1] = dK[1, 0]
    dK[1, 0] = -99.0  # the sentinel the GPU test fills outputs with: head 0's columns were never written
    got["dK"] = dK
    msg = _raises(A.check_onehot, "bwd", got, exp, "tr", ("dK",))
    assert "window=1, head=0" in msg and "token=" in msg


def test_scale_of_the_padded_head_dim_is_flagged():
    """1/sqrt(hdp) = 1/sqrt(32) instead of 1/sqrt(20) at head_dim 20: the lse check (both gates) and Gate 2 on O flag it."""
    q, k, v, dO, pi, exp = _onehot(25, 3, 2, 49, 20)
    O, lse = A.emu_attn_fwd("tr", q, k, v, BF, scale=A.f32_scale(32))
    assert "lse" in _raises(A.check_onehot, "fwd", {"O": O, "lse": lse}, exp, "tr", ("lse",))
    g = _gen(26)
    sh = (3, 2, 49, 20)
    q, k, v = _real(sh, g, BF), _real(sh, g, BF), _real(sh, g, BF)
    ref = A.attn_ref64(q, k, v)
    b = A.attn_bounds(q, k, v, None, ref, BF, "tr")
    O, lse = A.emu_attn_fwd("tr", q, k, v, BF, scale=A.f32_scale(32))
    assert "Gate 2" in _raises(A.check_bound, "lse", lse, ref["lse"], b["lse"], A.locate_attn("tr"))
    assert "Gate 2" in _raises(A.check_bound, "O", O, ref["O"], b["O"], A.locate_attn("tr"))


def test_layernorm_variance_over_c_minus_1_is_flagged():
    g = _gen(27)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    x, pix, gam, bet = _ln_inputs(256, 7, (2, 9, 11), F32, g)
    ref = A.ln_fwd_ref64(x, gam, bet, eps)
    b = A.ln_fwd_bounds(x, gam, bet, eps, ref, F32)
    out, mu, rs = A.emu_ln_fwd(x, gam, bet, eps, F32, var_div=255)
    loc = A.locate_tokens(pix, (9, 11), "G1")
    assert "Gate 2" in _raises(A.check_bound, "ln rstd", rs, ref["rstd"].squeeze(1), b["rstd"])
    msg = _raises(A.check_bound, "ln out", out, ref["out"], b["out"], loc)
    assert "form G1" in msg and "(n=" in msg
    # the relative-L2 gate accepts the same fault on the benchmark's LayerNorm token matrix (56448 x 256)
    xb = _real((BENCH_T, BENCH_C), g, F32, 2.0) + 0.5
    gb, bb = torch.randn(BENCH_C, generator=g) * 0.5 + 1.0, torch.randn(BENCH_C, generator=g) * 0.3
    good, _, _ = A.emu_ln_fwd(xb, gb, bb, eps, F32)
    bad, _, _ = A.emu_ln_fwd(xb, gb, bb, eps, F32, var_div=BENCH_C - 1)
    assert 0 < A.rel(bad, good) <= FWD_GATE


def test_padding_tokens_dropped_from_dbeta_are_flagged():
    g = _gen(28)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    x, pix, gam, bet = _ln_inputs(64, 7, (2, 9, 11), BF, g)
    _, mu, rs = A.emu_ln_fwd(x, gam, bet, eps, BF)
    dy = _real(x.shape, g, BF)
    dy[pix < 0] *= 8
    dx, dgam, dbet = A.emu_ln_bwd(x, dy, gam, mu, rs, BF, drop_padding_dbeta=pix < 0)
    ref = A.ln_bwd_ref64(x, dy, gam, mu, rs)
    b = A.ln_bwd_bounds(dy, ref, BF)
    A.check_bound("dgamma", dgam, ref["dgamma"], b["dgamma"])
    assert "Gate 2" in _raises(A.check_bound, "dbeta", dbet, ref["dbeta"], b["dbeta"])


def test_window_tokens_follow_the_reference_order():
    """the gather mirror against the committed window-index fixture's rule: token t of window (b, wh, ww) is pixel (wh*ws + t // ws, ...)."""
    img = torch.arange(2 * 9 * 11, dtype=torch.float32).view(2, 9, 11, 1) + 1
    tok, pix = A.window_tokens(img, 7)
    assert tok.shape == (2 * 14 * 14, 1)
    real = pix >= 0
    assert bool((tok[real, 0] == pix[real].float() + 1).all()) and bool((tok[~real] == 0).all())
    # window 1 of image 0 starts at pixel (0, 7); its token 8 is pixel (1, 8); window 2 starts at (7, 0) of image 0
    assert int(pix[49 + 8]) == 1 * 11 + 8 and int(pix[2 * 49]) == 7 * 11 and int(pix[49 + 4]) == -1
