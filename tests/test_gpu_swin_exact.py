"""GPU: the Swin kernels of csrc/swin.hip checked element by element (tests/attn_exact.py).

Window attention forward / backward through the C ABI in every kernel form the dispatcher has: tr (bfloat16 one-tile), one-tile
float32 and tiled in both dtypes, the tiled form both forced (option attn_tiled = 1, windows of <= 64 tokens) and natural (> 64).
Every case runs Gate 2 (a per-element float64 bound on N(0, 1) operands and on a x3 q / k variant) and, where its construction allows
(hd - 1 >= ceil(log2 L)), Gate 1 (one-hot attention: O, dV, dQ, dK bit for bit, lse within 2 float32 ulps).  Outputs are filled with a
sentinel first and whatever lies outside the written region must keep it; every (token, head) entry of lse must be written; a forward
without lse gives the same out; each form run twice gives bit-identical results.  LayerNorm forward and backward (with the window
gather, padding at the bottom and right, the half-wave bfloat16 kernel and the G = 1..4 kernels, the addend absent, separate or
aliased to dx) are checked against float64 in the same way.  The model's attention shapes and LayerNorm token matrices run Gate 2.

One line per case: form, dtype, shape, worst Gate 2 ratio.  YMI_SWIN_SOAK=N adds N random shapes per attention form."""
import contextlib
import ctypes
import math
import os
import random

import pytest
import torch

import attn_exact as A
from improving_yolov8_cbam_swinblock_amd._lib import as_ymi, check, get_option, lib, ptr, set_option, stream_ptr

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SENTINEL = -99.0
SOAK = int(os.environ.get("YMI_SWIN_SOAK", "0"))
HDS = [4, 8, 12, 20, 32, 48, 96, 100, 128, 160, 188, 192]
LS = [1, 4, 9, 16, 49, 63, 64, 65, 100, 128, 196, 256]
HEADS = [1, 2, 3, 6]
LAYOUTS = ["dense", "qkv_ld+4", "qkv_ld+8", "qkv_off4", "wide_ld"]
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
NWIN = 3


def dev():
    return torch.device("cuda:0")


def dname(dtype):
    return "bf16" if dtype == BF else "f32"


@contextlib.contextmanager
def options(**kv):
    """set library options for the block; the earlier values come back afterwards, whatever happens inside."""
    old = {k: get_option(k) for k in kv}
    try:
        for k, v in kv.items():
            set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            set_option(k, v)


def byref(t):
    return ctypes.byref(as_ymi(t)) if t is not None else None


def untouched(what, buf, lo, hi):
    """columns [lo, hi) of the rows of `buf` are the written region; the rest keeps the sentinel."""
    rest = torch.cat([buf[:, :lo], buf[:, hi:]], 1).float()
    assert bool((rest == SENTINEL).all()), f"{what}: {int((rest != SENTINEL).sum())} elements outside the written columns changed"


# ================================================================================================ attention
def attn_layout(layout, C):
    """-> (qkv ld, qkv column offset, out ld, dout ld, dqkv ld); every ld a multiple of 4."""
    return {
        "dense": (3 * C, 0, C, C, 3 * C),
        "qkv_ld+4": (3 * C + 4, 0, C, C, 3 * C),
        "qkv_ld+8": (3 * C + 8, 0, C, C, 3 * C),
        "qkv_off4": (3 * C + 8, 4, C, C, 3 * C),
        "wide_ld": (3 * C + 4, 4, C + 8, C + 12, 3 * C + 8),
    }[layout]


class AttnRun:
    """device buffers of one attention launch: qkv (a column slice of a wider buffer), out, lse, dout, dqkv (sentinel-filled)."""

    def __init__(self, T, C, heads, dtype, layout):
        self.T, self.C, self.heads, self.dtype = T, C, heads, dtype
        self.qld, self.qoff, self.old, self.dld, self.gld = attn_layout(layout, C)
        d = dev()
        self.qbuf = torch.full((T, self.qld), SENTINEL, dtype=dtype, device=d)
        self.qkv = self.qbuf[:, self.qoff : self.qoff + 3 * C]
        self.dbuf = torch.full((T, self.dld), SENTINEL, dtype=dtype, device=d)
        self.dout = self.dbuf[:, :C]

    def load(self, qkv_h, dout_h):
        self.qkv.copy_(qkv_h.to(device=dev(), dtype=self.dtype))
        self.dout.copy_(dout_h.to(device=dev(), dtype=self.dtype))

    def fwd(self, L, with_lse=True):
        d = dev()
        obuf = torch.full((self.T, self.old), SENTINEL, dtype=self.dtype, device=d)
        lse = torch.full((self.T * self.heads + 16,), float("nan"), device=d)
        check(lib().ymi_window_attention_fwd(byref(self.qkv), L, self.heads, byref(obuf[:, : self.C]), ptr(lse) if with_lse else None, stream_ptr()),
              "window_attention_fwd")
        torch.cuda.synchronize()
        return obuf, lse

    def bwd(self, L, obuf, lse):
        gbuf = torch.full((self.T, self.gld), SENTINEL, dtype=self.dtype, device=dev())
        check(lib().ymi_window_attention_bwd(byref(self.qkv), byref(obuf[:, : self.C]), byref(self.dout), ptr(lse), L, self.heads,
                                            byref(gbuf[:, : 3 * self.C]), stream_ptr()), "window_attention_bwd")
        torch.cuda.synchronize()
        return gbuf

    def stage(self, hd, bwd):
        es = 2 if self.dtype == BF else 4
        srcs = [(self.qkv.data_ptr(), self.qld)] + ([(self.dout.data_ptr(), self.dld)] if bwd else [])
        return A.stage_width(hd, srcs) if es == 2 else 0


def attn_outputs(run, L, obuf, lse, gbuf):
    C, H = run.C, run.heads
    got = {"O": A.heads_view(obuf[:, :C].double(), L, H), "lse": lse[: run.T * H].view(run.T // L, L, H).permute(0, 2, 1).double()}
    if gbuf is not None:
        dq, dk, dv = A.split_qkv(gbuf[:, : 3 * C].double(), L, H)
        got.update(dQ=dq, dK=dk, dV=dv)
    return got


def run_and_check_layout(run, L, tag):
    """forward twice (bit-identical), forward without lse (same out), backward twice (bit-identical); sentinel and lse coverage."""
    ob, lse = run.fwd(L)
    nl = run.T * run.heads
    assert bool(torch.isfinite(lse[:nl]).all()), f"{tag}: {int((~torch.isfinite(lse[:nl])).sum())} (token, head) lse entries not written"
    assert bool(torch.isnan(lse[nl:]).all()), f"{tag}: lse written past its end"
    ob2, lse2 = run.fwd(L)
    assert torch.equal(ob, ob2) and torch.equal(lse[:nl], lse2[:nl]), f"{tag}: two forward runs differ"
    ob3, _ = run.fwd(L, with_lse=False)
    assert torch.equal(ob, ob3), f"{tag}: the forward without lse gives another out"
    untouched(tag + " out", ob, 0, run.C)
    gb = run.bwd(L, ob, lse)
    gb2 = run.bwd(L, ob, lse)
    assert torch.equal(gb, gb2), f"{tag}: two backward runs differ"
    untouched(tag + " dqkv", gb, 0, 3 * run.C)
    return ob, lse, gb


def attn_gate2(run, L, hd, gen, qk_scale, form_b, tag):
    T, C = run.T, run.C
    qkv_h = torch.randn(T, 3 * C, generator=gen)
    qkv_h[:, : 2 * C] *= qk_scale
    dout_h = torch.randn(T, C, generator=gen)
    run.load(qkv_h, dout_h)
    ob, lse, gb = run_and_check_layout(run, L, tag)
    q, k, v = A.split_qkv(run.qkv.double(), L, run.heads)
    dO = A.heads_view(run.dout.double(), L, run.heads)
    ref = A.attn_ref64(q, k, v, dO)
    b = A.attn_bounds(q, k, v, dO, ref, run.dtype, form_b)
    return A.check_attn(tag, attn_outputs(run, L, ob, lse, gb), ref, b, form_b, ("O", "lse", "dV", "dQ", "dK"))


def attn_gate1(run, L, hd, gen, form, tag):
    nw = run.T // L
    q, k, v, dO, pi = A.onehot_operands(nw, run.heads, L, hd, gen)
    A.onehot_check(q, k, pi, tag)
    run.load(torch.cat([A.tokens_view(q), A.tokens_view(k), A.tokens_view(v)], 1), A.tokens_view(dO))
    ob, lse, gb = run_and_check_layout(run, L, tag)
    exp = A.onehot_expected(q.to(dev()), k.to(dev()), v.to(dev()), dO.to(dev()), run.dtype)
    A.check_onehot(tag, attn_outputs(run, L, ob, lse, gb), exp, form, ("O", "lse", "dV", "dQ", "dK"))


def attn_case(dtype, L, hd, heads, force, layout, seed, nw=NWIN):
    T, C = nw * L, heads * hd
    form_f, form_b = A.attn_form(L, hd, dtype, force, False), A.attn_form(L, hd, dtype, force, True)
    run = AttnRun(T, C, heads, dtype, layout)
    st = f" stage {run.stage(hd, False)}B/{run.stage(hd, True)}B" if form_f == "tr" else ""
    tag = f"attn {dname(dtype)} L{L} hd{hd} heads{heads} windows{nw} {layout} attn_tiled={force} fwd {form_f} bwd {form_b}{st}"
    gen = torch.Generator().manual_seed(seed)
    with options(attn_tiled=force):
        worst = max(attn_gate2(run, L, hd, gen, s, form_b, tag) for s in (1.0, 3.0))
        g1 = "n/a"
        if A.onehot_ok(L, hd):
            attn_gate1(run, L, hd, gen, form_b, tag)
            g1 = "exact"
    return f"{tag}: Gate 1 {g1}, worst Gate 2 {worst:.3f}"


def _attn_cases():
    cases = []
    for dtype in (BF, F32):
        for force in (0, 1):
            for li, L in enumerate(LS):
                if force and L > 64:
                    continue
                for j in range(2):
                    hd = HDS[(2 * li + j) % len(HDS)]
                    cases.append((dtype, L, hd, HEADS[(li + j + force) % 4], force, LAYOUTS[(2 * li + j + 3 * force) % 5], 1000 * li + 10 * j + force))
    # the float32 one-tile backward at head_dim 192 (156,928 of 163,840 bytes of LDS) at a full 64-token tile, and 96 / 100 tiled chunks
    cases += [(F32, 64, 192, 1, 0, "wide_ld", 7), (BF, 65, 96, 2, 0, "dense", 8), (F32, 100, 100, 3, 0, "qkv_off4", 9), (BF, 64, 100, 1, 1, "qkv_ld+4", 10)]
    return cases


SOAK_FORMS = [("tr", BF, 0), ("onetile-f32", F32, 0), ("tiled", BF, 1), ("tiled", F32, 1), ("tiled", BF, 0), ("tiled", F32, 0)]


def _soak_cases():
    """YMI_SWIN_SOAK=N: N random shapes per attention form (none by default)."""
    cases = []
    for fi, (form, dtype, force) in enumerate(SOAK_FORMS):
        rnd = random.Random(4242 + fi)
        for i in range(SOAK):
            L = rnd.randint(65, 256) if (form == "tiled" and not force) else rnd.randint(1, 64)
            cases.append((dtype, L, 4 * rnd.randint(1, 48), rnd.choice(HEADS), force, rnd.choice(LAYOUTS), 5000 + 100 * fi + i, rnd.randint(3, 6)))
    return cases


ATTN_CASES = _attn_cases() + _soak_cases()


@pytest.mark.parametrize("case", ATTN_CASES, ids=[f"{dname(c[0])}-L{c[1]}-hd{c[2]}-h{c[3]}-t{c[4]}-{c[5]}" + (f"-soak{c[6]}" if len(c) > 7 else "")
                                                  for c in ATTN_CASES])
def test_attention_form(case):
    print(attn_case(*case))


def test_attn_tiled_option_is_restored():
    before = get_option("attn_tiled")
    with pytest.raises(RuntimeError):
        with options(attn_tiled=1):
            assert get_option("attn_tiled") == 1
            raise RuntimeError("inside")
    assert get_option("attn_tiled") == before


def model_swin_shape(yaml_name, imgsz):
    """-> (map side, channels, heads) of the model's SwinBlocks at this image size: the SwinBlock rows of the YAML,
    the stride of the map they run on (stride-2 Conv rows before the first one), window size 7 and 2 heads (SwinBlock's defaults)."""
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import yaml_model_load

    d = yaml_model_load(yaml_name)
    rows = d["backbone"] + d["head"]
    first = next(i for i, r in enumerate(rows) if r[2] == "SwinBlock")
    stride = 2 ** sum(1 for r in rows[:first] if r[2] == "Conv" and len(r[3]) >= 3 and r[3][2] == 2)
    dim = rows[first][3][0]
    side = imgsz // stride
    return side, dim, 2


MODEL_ATTN = [
    # the benchmark (bench.py defaults: yolov8s.yaml, batch 32, 640): 56448 tokens x 256, 2 heads, 49-token windows
    ("bench", "yolov8s.yaml", 32, 640, 7, 56448, 256),
    # config 5 at its stated per-GPU size (batch 16, 1280; bench.py's size table): 112896 x 384, head_dim 192, and its ws-14 row
    ("cfg5", "yolov8m-cbam-swin384.yaml", 16, 1280, 7, 112896, 384),
    ("cfg5-ws14", "yolov8m-cbam-swin384.yaml", 16, 1280, 14, 112896, 384),
]


@pytest.mark.parametrize("case", MODEL_ATTN, ids=[c[0] for c in MODEL_ATTN])
def test_attention_model_shape(case):
    name, yml, batch, img, ws, t_issue, c_issue = case
    side, C, heads = model_swin_shape(yml, img)
    hp = (side + ws - 1) // ws * ws
    T = batch * hp * hp
    assert (T, C) == (t_issue, c_issue), (name, T, C)
    L, hd = ws * ws, C // heads
    form_b = A.attn_form(L, hd, BF, 0, True)
    run = AttnRun(T, C, heads, BF, "dense")
    tag = f"attn model {name} bf16 T{T} C{C} heads{heads} L{L} hd{hd} fwd {A.attn_form(L, hd, BF, 0, False)} bwd {form_b}"
    gen = torch.Generator().manual_seed(31)
    qkv_h, dout_h = torch.randn(T, 3 * C, generator=gen), torch.randn(T, C, generator=gen)
    run.load(qkv_h, dout_h)
    ob, lse = run.fwd(L)
    gb = run.bwd(L, ob, lse)
    q, k, v = A.split_qkv(run.qkv.double(), L, heads)
    dO = A.heads_view(run.dout.double(), L, heads)
    got = attn_outputs(run, L, ob, lse, gb)
    ref = A.attn_ref64(q, k, v, dO)
    b = A.attn_bounds(q, k, v, dO, ref, BF, form_b)
    worst = A.check_attn(tag, got, ref, b, form_b, ("O", "lse", "dV", "dQ", "dK"))
    print(f"{tag}: worst Gate 2 {worst:.3f}")


# ================================================================================================ LayerNorm
LN_CS = [4, 12, 64, 252, 256, 260, 384, 512, 516, 768, 1024]
LN_WS = [0, 3, 7, 14]
LN_GEO = {3: (2, 4, 5), 7: (2, 9, 11), 14: (1, 15, 17)}  # padding in both H and W
LN_T0 = [29, 37, 101]  # ws = 0 token matrices: odd counts (the half kernel pairs tokens), one below 32


class LnRun:
    def __init__(self, dtype, C, ws, geo, layout):
        """layout: 'dense', 'x_off4' (x 4 elements off: the half kernel's 16-byte alignment fails), 'wide_ld' (x / out / dx ld = C + 4)."""
        self.dtype, self.C, self.ws, self.layout = dtype, C, ws, layout
        xoff = 4 if layout == "x_off4" else 0
        xld = C + 4 if layout == "wide_ld" else C + 2 * xoff
        self.old = C + 4 if layout == "wide_ld" else C
        self.xoff, self.xld = xoff, xld
        if ws == 0:
            T = geo
            self.shape = (T,)
            self.T, self.pix, self.hw = T, None, None
        else:
            n, h, w = geo
            self.shape = (n, h, w)
            hp, wp = (h + ws - 1) // ws * ws, (w + ws - 1) // ws * ws
            self.T, self.hw = n * hp * wp, (h, w)
            _, self.pix = A.window_tokens(torch.zeros(n, h, w, 1), ws)

    def image(self, fill=SENTINEL):
        """-> (buffer, logical view): [T, ld] token matrix (ws = 0) or an NHWC image [n, h, w, ld] seen as NCHW."""
        buf = torch.full(self.shape + (self.xld,), fill, dtype=self.dtype, device=dev())
        sl = buf[..., self.xoff : self.xoff + self.C]
        return buf, (sl if self.ws == 0 else sl.permute(0, 3, 1, 2))

    def tokens(self, t):
        """a buffer of image()'s layout -> [T, C] token rows (padding rows zero)."""
        s = t[..., self.xoff : self.xoff + self.C].double()
        return s if self.ws == 0 else A.window_tokens(s, self.ws)[0]

    def real(self):
        return torch.ones(self.T, dtype=torch.bool) if self.pix is None else self.pix >= 0


def ln_case(dtype, C, ws, geo, layout, seed):
    run = LnRun(dtype, C, ws, geo, layout)
    gen = torch.Generator().manual_seed(seed)
    d = dev()
    xbuf, xv = run.image()
    xh = torch.randn(run.shape + (C,), generator=gen) * 2.0 + 0.5
    xbuf[..., run.xoff : run.xoff + C] = xh.to(device=d, dtype=dtype)
    gam = (torch.randn(C, generator=gen) * 0.5 + 1.0).to(d)
    bet = (torch.randn(C, generator=gen) * 0.3).to(d)
    T = run.T
    obuf = torch.full((T, run.old), SENTINEL, dtype=dtype, device=d)
    stats = torch.full((2, T + 8), float("nan"), device=d)
    form = A.ln_form(C, dtype, run.xld, run.old, [xv.data_ptr(), obuf.data_ptr(), gam.data_ptr(), bet.data_ptr()])
    where = f"ws{ws} " + (f"T{geo}" if ws == 0 else "x".join(map(str, geo)))
    tag = f"layernorm {dname(dtype)} C{C} {where} T={T} {layout} form {form}"
    check(lib().ymi_layernorm_fwd(byref(xv), ws, ptr(gam), ptr(bet), ctypes.c_float(EPS), byref(obuf[:, :C]), ptr(stats[0]), ptr(stats[1]), stream_ptr()),
          "layernorm_fwd")
    torch.cuda.synchronize()
    untouched(tag + " out", obuf, 0, C)
    assert bool(torch.isnan(stats[:, T:]).all()), f"{tag}: mean / rstd written past their end"
    x = run.tokens(xbuf)
    real = run.real().to(d)
    loc = A.locate_tokens(run.pix, run.hw or (1, 1), form)
    ref = A.ln_fwd_ref64(x, gam, bet, EPS)
    b = A.ln_fwd_bounds(x, gam, bet, EPS, ref, dtype)
    out = obuf[:, :C].double()
    mu_k, rs_k = stats[0, :T].double(), stats[1, :T].double()
    pad = ~real
    worst = A.check_bound(tag + " out", out[real], ref["out"][real], b["out"][real])
    worst = max(worst, A.check_bound(tag + " mean", mu_k[real], ref["mu"].squeeze(1)[real], b["mu"][real] + 1e-300))
    worst = max(worst, A.check_bound(tag + " rstd", rs_k[real], ref["rstd"].squeeze(1)[real], b["rstd"][real]))
    if bool(pad.any()):
        # padding tokens normalise to exactly beta; their statistics are mean 0 and rsqrtf(eps)
        A.check_exact(tag + " padding out == beta", out[pad], bet.to(dtype).double().expand(int(pad.sum()), C), loc)
        A.check_exact(tag + " padding mean", mu_k[pad], torch.zeros(int(pad.sum()), dtype=torch.float64, device=d))
        r_eps = torch.tensor(1.0 / math.sqrt(EPS), dtype=torch.float64)
        assert bool(((rs_k[pad] - r_eps.to(d)).abs() <= 2 * A.f32_ulp(r_eps).to(d)).all()), f"{tag}: padding rstd not within 2 ulp of rsqrtf(eps)"
    # ---- backward: the addend absent, separate, aliased to dx (accumulate = 1); dy on padding tokens x 8
    dy_h = torch.randn(T, C, generator=gen)
    if run.pix is not None:
        dy_h[run.pix < 0] *= 8
    dybuf = torch.full((T, run.old), SENTINEL, dtype=dtype, device=d)
    dybuf[:, :C] = dy_h.to(device=d, dtype=dtype)
    dy = dybuf[:, :C]
    blocks = A.ln_bwd_blocks(T)
    wsp = torch.empty(blocks * 2 * C * 4 + 256, dtype=torch.uint8, device=d)
    add_h = torch.randn(run.shape + (C,), generator=gen)
    for mode in ("absent", "separate", "aliased"):
        dxbuf, dxv = run.image()
        addbuf, addv = None, None
        if mode == "separate":
            addbuf, addv = run.image()
            addbuf[..., run.xoff : run.xoff + C] = add_h.to(device=d, dtype=dtype)
        if mode == "aliased":
            dxbuf[..., run.xoff : run.xoff + C] = add_h.to(device=d, dtype=dtype)
        dg = torch.full((2, C + 8), float("nan"), device=d)  # [dgamma, dbeta]
        if mode == "separate":
            rc = lib().ymi_layernorm_bwd_add(byref(xv), ws, byref(dy), ptr(gam), ptr(stats[0]), ptr(stats[1]), byref(addv), byref(dxv), ptr(dg[0]), ptr(dg[1]),
                                           ptr(wsp), wsp.numel(), stream_ptr())
        else:
            rc = lib().ymi_layernorm_bwd(byref(xv), ws, byref(dy), ptr(gam), ptr(stats[0]), ptr(stats[1]), byref(dxv), 1 if mode == "aliased" else 0,
                                       ptr(dg[0]), ptr(dg[1]), ptr(wsp), wsp.numel(), stream_ptr())
        check(rc, "layernorm_bwd")
        torch.cuda.synchronize()
        add_tok = None
        if mode != "absent":
            add_tok = run.tokens(addbuf if mode == "separate" else run_image_of(run, add_h, dtype))
        r2 = A.ln_bwd_ref64(x, dy, gam, stats[0, :T], stats[1, :T], add_tok)
        b2 = A.ln_bwd_bounds(dy, r2, dtype, add_tok)
        btag = f"{tag} backward addend {mode}"
        dx_tok = run.tokens(dxbuf)
        worst = max(worst, A.check_bound(btag + " dx", dx_tok[real], r2["dx"][real], b2["dx"][real]))
        worst = max(worst, A.check_bound(btag + " dgamma", dg[0, :C], r2["dgamma"], b2["dgamma"]))
        worst = max(worst, A.check_bound(btag + " dbeta", dg[1, :C], r2["dbeta"], b2["dbeta"]))
        assert bool(torch.isnan(dg[:, C:]).all()), f"{btag}: dgamma / dbeta written past their end"
        rest = torch.cat([dxbuf[..., : run.xoff], dxbuf[..., run.xoff + C :]], -1).float()
        assert bool((rest == SENTINEL).all()), f"{btag}: dx written outside its channels"
        if mode == "absent":
            assert not bool((dxbuf[..., run.xoff : run.xoff + C].float() == SENTINEL).any()), f"{btag}: dx pixels left unwritten"
    return f"{tag}: worst Gate 2 {worst:.3f}"


def run_image_of(run, t_h, dtype):
    buf, _ = run.image()
    buf[..., run.xoff : run.xoff + run.C] = t_h.to(device=dev(), dtype=dtype)
    return buf


def _ln_cases():
    cases = []
    for dtype in (BF, F32):
        for ci, C in enumerate(LN_CS):
            for wi, ws in enumerate(LN_WS):
                geo = LN_T0[(ci + wi) % 3] if ws == 0 else LN_GEO[ws]
                layouts = ["dense"]
                if dtype == BF and C <= 256:
                    layouts.append("x_off4" if (ci + wi) % 2 else "wide_ld")  # force the G-form where the half kernel would run
                elif (ci + wi) % 3 == 0:
                    layouts.append("wide_ld")
                for lay in layouts:
                    cases.append((dtype, C, ws, geo, lay, 100 * ci + 10 * wi + len(lay)))
    return cases


LN_CASES = _ln_cases()


@pytest.mark.parametrize("case", LN_CASES, ids=[f"{dname(c[0])}-C{c[1]}-ws{c[2]}-{c[4]}" for c in LN_CASES])
def test_layernorm(case):
    print(ln_case(*case))


LN_MODEL = [("bench", "yolov8s.yaml", 32, 640, 256), ("cfg5", "yolov8m-cbam-swin384.yaml", 16, 1280, 384)]


@pytest.mark.parametrize("case", LN_MODEL, ids=[c[0] for c in LN_MODEL])
def test_layernorm_model_token_matrix(case):
    """norm1 of the model's SwinBlock: the window gather of the [batch, side, side, C] map, bfloat16."""
    name, yml, batch, img, c_issue = case
    side, C, _ = model_swin_shape(yml, img)
    assert C == c_issue
    print(ln_case(BF, C, 7, (batch, side, side), "dense", 55) + f" (model {name})")
