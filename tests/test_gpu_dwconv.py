"""The depthwise convolution kernels (csrc/dwconv.hip) element by element through the C ABI, against float64 conv2d(groups=C) and its
autograd on the CPU.  The references take the operands AS STORED (bfloat16 operands are rounded before the float64 run; the float32
weights enter as they are) and raw outputs are rounded where the product rounds, so every bound below is derived, not measured:

  u = 2^-24 (float32 unit roundoff).  A float32 sum of n products accumulated by fma in any order is within n * u * sum|a_i b_i| of
  the exact sum.  A result stored in bfloat16 adds one rounding, 2^-9 |y| (2^-8 is asserted); one stored in float32 adds u |y|, which
  the factor 2 on the accumulation term covers (|y| <= sum|x w|).
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_modules_golden import BF16_TOL, F32_TOL, close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 777.0
GUARD = 64
EINVAL, EWORKSPACE = -1, -4

SHAPES = [(1, 8, 5, 5), (2, 16, 13, 9), (2, 40, 20, 20), (1, 256, 7, 6), (3, 24, 33, 47),
          (1, 264, 6, 9)]  # 264 channels: two forward tiles of 256 / three weight-gradient tiles of 128 channels, the last one chunk (bf16) wide
F32_ONLY = [(2, 4, 13, 9), (2, 12, 13, 9)]
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
CASES = [(sh, k, s, dt) for dt in ("bf16", "f32") for sh in SHAPES + (F32_ONLY if dt == "f32" else []) for k, s in KS]
IDS = [f"{'x'.join(map(str, sh))}-k{k}s{s}-{dt}" for sh, k, s, dt in CASES]
SMALL = [c for c in CASES if c[0] in ((2, 16, 13, 9), (1, 264, 6, 9))]
SMALL_IDS = [i for c, i in zip(CASES, IDS) if c in SMALL]


def _L():
    from improving_yolov8_cbam_swinblock_amd import _lib

    return _lib, _lib.lib()


def _dt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _stream():
    return _L()[0].stream_ptr()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _tensor(n, c, h, w, dtype, values=None, ld=None, off=0):
    """-> (buffer, logical [n, c, h, w] view): NHWC rows of stride ld (>= off + c) over a buffer with GUARD extra rows; everything holds the
    SENTINEL except the view, which holds `values` (a CPU NCHW tensor) when given."""
    ld = c if ld is None else ld
    buf = torch.full((n * h * w + GUARD, ld), SENTINEL, dtype=dtype, device="cuda:0")
    v = buf[: n * h * w].view(n, h, w, ld).permute(0, 3, 1, 2)[:, off : off + c]
    if values is not None:
        v.copy_(values.to(dtype))
    return buf, v


def _untouched(buf, rows, lo, hi):
    """guard rows and the channels outside [lo, hi) of the rows in use still hold the sentinel"""
    return bool((buf[rows:] == SENTINEL).all()) and bool((buf[:rows, :lo] == SENTINEL).all()) and bool((buf[:rows, hi:] == SENTINEL).all())


def _y(t):
    lib, _ = _L()
    return ctypes.byref(lib.as_ymi(t))


def _out_hw(h, w, k, s):
    p = k // 2
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def _case(shape, k, s, dt):
    """operands as stored and the float64 references: computed once per case, shared by the tests, never modified"""
    n, c, h, w = shape
    dtype = _dt(dt)
    g = torch.Generator().manual_seed(hash((shape, k, s)) % (2 ** 31))
    ho, wo = _out_hw(h, w, k, s)
    x = (torch.randn(n, c, h, w, generator=g) * 1.2 + 0.2).to(dtype)
    wt = torch.randn(c, 1, k, k, generator=g) / k
    dy = torch.randn(n, c, ho, wo, generator=g).to(dtype)
    x64 = x.double().requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, s, k // 2, 1, c)
    gx, gw = torch.autograd.grad(y64, [x64, w64], dy.double())
    absxw = F.conv2d(x.double().abs(), wt.double().abs(), None, s, k // 2, 1, c)
    # sum |dy w| per input element and sum |dy x| per weight element: the same adjoints on absolute values
    xa = x.double().abs().requires_grad_(True)
    wa = wt.double().abs().requires_grad_(True)
    ax, aw = torch.autograd.grad(F.conv2d(xa, wa, None, s, k // 2, 1, c), [xa, wa], dy.double().abs())
    return dict(n=n, c=c, h=h, w=w, ho=ho, wo=wo, k=k, s=s, dtype=dtype, x=x, wt=wt, dy=dy, y=y64.detach(), absxw=absxw, gx=gx, gw=gw, abs_dyw=ax,
                abs_dyx=aw)


def _fwd_bound(d, y, absxw):
    if d["dtype"] == torch.bfloat16:
        return 2.0 ** -8 * y.abs() + 25 * U * absxw
    return 2 * 25 * U * absxw


def _check(got, ref, bound, what):
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), what
    over = (got - ref).abs() - bound
    worst = float(over.max())
    assert worst <= 0, f"{what}: error exceeds the derived bound by {worst:.3e} (max error {float((got - ref).abs().max()):.3e})"


def _forward(d, strided=False, **kw):
    """ymi_dwconv2d_fwd on the case's operands -> (rc, y view, y buffer, x buffer)"""
    lib, L = _L()
    n, c, h, w, ho, wo = (d[q] for q in ("n", "c", "h", "w", "ho", "wo"))
    xb, x = _tensor(n, c, h, w, d["dtype"], d["x"], ld=2 * c if strided else None, off=c if strided else 0)
    yb, y = _tensor(n, c, ho, wo, d["dtype"], None, ld=2 * c if strided else None)
    wt = d["wt"].cuda()
    rc = L.ymi_dwconv2d_fwd(_y(x), _p(wt), d["k"], d["s"], _p(kw.get("scale")), _p(kw.get("bias")), kw.get("act", 0),
                            _y(kw["res"]) if kw.get("res") is not None else None, _y(y), _p(kw.get("part")), kw.get("blocks"), _stream())
    torch.cuda.synchronize()
    return rc, y, yb, xb


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_within_the_derived_bound(case):
    d = _case(*case)
    rc, y, yb, _ = _forward(d)
    assert rc == 0, _L()[1].ymi_last_error()
    _check(y, d["y"], _fwd_bound(d, d["y"], d["absxw"]), "forward")
    assert _untouched(yb, d["n"] * d["ho"] * d["wo"], 0, d["c"])


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_forward_on_channel_slices_touches_nothing_else(case):
    """x is channels [C, 2C) of one 2C-wide buffer, y channels [0, C) of another: same result, guard rows and foreign channels unchanged"""
    d = _case(*case)
    rc, y, yb, xb = _forward(d, strided=True)
    assert rc == 0, _L()[1].ymi_last_error()
    _check(y, d["y"], _fwd_bound(d, d["y"], d["absxw"]), "forward (slices)")
    assert _untouched(yb, d["n"] * d["ho"] * d["wo"], 0, d["c"])
    assert _untouched(xb, d["n"] * d["h"] * d["w"], d["c"], 2 * d["c"])


@pytest.mark.parametrize("act", [0, 1], ids=["none", "silu"])
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_eval_form_scale_bias_act_residual(case, act):
    """y = act(scale * conv + bias) + residual.  z = scale * conv + bias carries |scale| times the accumulation error plus two float32
    roundings (2u (|scale conv| + |bias|)); SiLU has slope <= 1.1 and its v_exp_f32 / v_rcp_f32 form is good to 2^-20 (|z| + 1) (one ulp
    each, the exponent's argument rounded at |z| <= 16); the sum with the stored residual is rounded once on store (2^-8 / u)."""
    d = _case(*case)
    g = torch.Generator().manual_seed(5)
    c = d["c"]
    scale = torch.rand(c, generator=g) + 0.5
    bias = torch.randn(c, generator=g) * 0.3
    res = torch.randn(d["n"], c, d["ho"], d["wo"], generator=g).to(d["dtype"])
    _, rv = _tensor(d["n"], c, d["ho"], d["wo"], d["dtype"], res)
    rc, y, yb, _ = _forward(d, scale=scale.cuda(), bias=bias.cuda(), act=act, res=rv)
    assert rc == 0, _L()[1].ymi_last_error()
    sc, bi = scale.double().view(1, c, 1, 1), bias.double().view(1, c, 1, 1)
    z = sc * d["y"] + bi
    ref = (z * torch.sigmoid(z) if act else z) + res.double()
    acc = (2 if d["dtype"] == torch.float32 else 1) * 25 * U * d["absxw"]
    bound = 1.1 * (sc.abs() * acc + 2 * U * ((sc * d["y"]).abs() + bi.abs())) + (2.0 ** -20 * (z.abs() + 1) if act else 0) \
        + (2.0 ** -8 if d["dtype"] == torch.bfloat16 else 2 * U) * ref.abs()
    _check(y, ref, bound, "eval form")
    assert _untouched(yb, d["n"] * d["ho"] * d["wo"], 0, c)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_statistics_rows_sum_the_rounded_output(case):
    """rows [blocks][2][C]: summed over the blocks in float64 they equal the float64 sum / sum of squares of the raw output AS STORED within
    P u sum|v| (the worst case of a float32 sum of P terms; the squares add one rounding each: P + 1)."""
    _, L = _L()
    d = _case(*case)
    c, P = d["c"], d["n"] * d["ho"] * d["wo"]
    cap = int(L.ymi_dwconv2d_stat_blocks(d["n"], d["ho"], d["wo"], c))
    part = torch.full((cap * 2 * c + GUARD,), SENTINEL, dtype=torch.float32, device="cuda:0")
    blocks = ctypes.c_int64(0)
    rc, y, yb, _ = _forward(d, part=part, blocks=ctypes.byref(blocks))
    assert rc == 0, L.ymi_last_error()
    assert 1 <= blocks.value <= cap
    _check(y, d["y"], _fwd_bound(d, d["y"], d["absxw"]), "raw output")
    rows = part[: blocks.value * 2 * c].view(blocks.value, 2, c).double().sum(0).cpu()
    assert bool((part[blocks.value * 2 * c :] == SENTINEL).all())
    v = y.detach().double().cpu()
    _check(rows[0], v.sum((0, 2, 3)), P * U * v.abs().sum((0, 2, 3)), "sum rows")
    _check(rows[1], (v * v).sum((0, 2, 3)), (P + 1) * U * (v * v).sum((0, 2, 3)), "sum-of-squares rows")


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_train_entry_is_batchnorm_of_the_rounded_raw_output(case):
    """ymi_dwconv2d_bn_act_fwd: out, saved mean / inverse deviation and the running statistics (unbiased variance, momentum 0.03, eps 1e-3)
    against a float64 train-mode BatchNorm + SiLU of the raw tensor as stored; the project's module tolerances."""
    _, L = _L()
    d = _case(*case)
    tol = F32_TOL if d["dtype"] == torch.float32 else BF16_TOL
    n, c, ho, wo = d["n"], d["c"], d["ho"], d["wo"]
    g = torch.Generator().manual_seed(9)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    rm0, rv0 = torch.randn(c, generator=g) * 0.2, torch.rand(c, generator=g) + 0.5
    res = torch.randn(n, c, ho, wo, generator=g).to(d["dtype"])
    _, x = _tensor(n, c, d["h"], d["w"], d["dtype"], d["x"])
    _, raw = _tensor(n, c, ho, wo, d["dtype"])
    ob, out = _tensor(n, c, ho, wo, d["dtype"])
    _, rv = _tensor(n, c, ho, wo, d["dtype"], res)
    dev = [t.cuda() for t in (d["wt"], gamma, beta, rm0, rv0)]
    stats = torch.empty(2, c, device="cuda:0")
    need = (int(L.ymi_dwconv2d_stat_blocks(n, ho, wo, c)) * 2 * c + 2 * c) * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    args = lambda nbytes: (_y(x), _p(dev[0]), d["k"], d["s"], _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), 0.03, 1e-3, 1, _y(rv), _y(raw), _y(out),  # noqa: E731
                           _p(stats[0]), _p(stats[1]), _p(ws), nbytes, _stream())
    assert L.ymi_dwconv2d_bn_act_fwd(*args(need - 1)) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ob == SENTINEL).all())  # a refused call launches nothing
    assert L.ymi_dwconv2d_bn_act_fwd(*args(need)) == 0, L.ymi_last_error()
    torch.cuda.synchronize()
    v = raw.detach().double().cpu()
    _check(raw, d["y"], _fwd_bound(d, d["y"], d["absxw"]), "raw")
    P = n * ho * wo
    mean, var = v.mean((0, 2, 3)), v.var((0, 2, 3), unbiased=False)
    inv = 1.0 / torch.sqrt(var + 1e-3)
    z = (v - mean.view(1, c, 1, 1)) * (inv * gamma.double()).view(1, c, 1, 1) + beta.double().view(1, c, 1, 1)
    close(out, (z * torch.sigmoid(z) + res.double()).float(), tol, "out")
    close(stats[0], mean.float(), tol, "save_mean")
    close(stats[1], inv.float(), tol, "save_invstd")
    close(dev[3], (0.97 * rm0.double() + 0.03 * mean).float(), tol, "running_mean")
    close(dev[4], (0.97 * rv0.double() + 0.03 * var * P / (P - 1)).float(), tol, "running_var")


def _dgrad(d, mode, strided=False):
    lib, L = _L()
    n, c, h, w, ho, wo = (d[q] for q in ("n", "c", "h", "w", "ho", "wo"))
    g = torch.Generator().manual_seed(3)
    addv = torch.randn(n, c, h, w, generator=g).to(d["dtype"])
    _, dy = _tensor(n, c, ho, wo, d["dtype"], d["dy"], ld=2 * c if strided else None, off=c if strided else 0)
    xb, dx = _tensor(n, c, h, w, d["dtype"], addv if mode == "alias" else None, ld=2 * c if strided else None)
    add = dx if mode == "alias" else (_tensor(n, c, h, w, d["dtype"], addv)[1] if mode == "add" else None)
    wt = d["wt"].cuda()
    rc = L.ymi_dwconv2d_bwd_data(_y(dy), _p(wt), d["k"], d["s"], _y(add) if add is not None else None, _y(dx), _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ymi_last_error()
    ref = d["gx"] + (addv.double() if mode != "none" else 0)
    acc = (2 if d["dtype"] == torch.float32 else 1) * 25 * U * d["abs_dyw"]
    bound = acc + (2.0 ** -8 if d["dtype"] == torch.bfloat16 else 2 * U) * ref.abs()
    _check(dx, ref, bound, f"data gradient ({mode})")
    assert _untouched(xb, n * h * w, 0, c)


@pytest.mark.parametrize("mode", ["none", "add", "alias"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_data_gradient_within_the_derived_bound(case, mode):
    """dx = dgrad(dy) (+ add; add may be dx itself): the forward bound with dy in place of x, the sum with the stored addend rounded once"""
    _dgrad(_case(*case), mode)


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_data_gradient_on_channel_slices(case):
    _dgrad(_case(*case), "alias", strided=True)


def _wgrad(case, strided):
    _, L = _L()
    d = _case(*case)
    n, c, h, w, ho, wo, k = (d[q] for q in ("n", "c", "h", "w", "ho", "wo", "k"))
    _, x = _tensor(n, c, h, w, d["dtype"], d["x"], ld=2 * c if strided else None, off=c if strided else 0)
    _, dy = _tensor(n, c, ho, wo, d["dtype"], d["dy"], ld=2 * c if strided else None)
    need = int(L.ymi_dwconv2d_bwd_weight_workspace(n, ho, wo, c, k))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda:0")
    runs = []
    for _ in range(2):
        dw = torch.full((c * k * k + GUARD,), SENTINEL, device="cuda:0")
        assert L.ymi_dwconv2d_bwd_weight(_y(x), _y(dy), k, d["s"], _p(dw), _p(ws), need, _stream()) == 0, L.ymi_last_error()
        torch.cuda.synchronize()
        assert bool((dw[c * k * k :] == SENTINEL).all())
        runs.append(dw[: c * k * k].view(c, 1, k, k).clone())
        ws.fill_(255)  # the second run may not depend on what the first left in the workspace
    assert torch.equal(runs[0], runs[1])
    _check(runs[0], d["gw"], n * ho * wo * U * d["abs_dyx"], "weight gradient")
    dw = torch.full((c * k * k,), SENTINEL, device="cuda:0")
    assert L.ymi_dwconv2d_bwd_weight(_y(x), _y(dy), k, d["s"], _p(dw), _p(ws), need - 1, _stream()) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weight_gradient_bound_and_bit_reproducibility(case):
    """|err| <= P u sum|dy x| per element (two-level float32 sum over P = N Ho Wo pixels); two runs are bit-identical"""
    _wgrad(case, False)


@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_weight_gradient_on_channel_slices(case):
    _wgrad(case, True)


def test_refusals_return_einval_and_launch_nothing():
    lib, L = _L()
    w = torch.randn(16, 1, 7, 7, device="cuda:0")

    def fwd(c, k, s, dtype, null=False):
        _, x = _tensor(1, c, 6, 6, dtype, torch.zeros(1, c, 6, 6))
        ho, wo = _out_hw(6, 6, k, s) if s in (1, 2) else (2, 2)
        yb, y = _tensor(1, c, ho, wo, dtype)
        rc = L.ymi_dwconv2d_fwd(None if null else _y(x), _p(w), k, s, None, None, 0, None, _y(y), None, None, _stream())
        torch.cuda.synchronize()
        assert bool((yb == SENTINEL).all())
        return rc

    assert fwd(12, 3, 1, torch.bfloat16) == EINVAL and b"16-byte" in L.ymi_last_error()
    assert fwd(16, 7, 1, torch.bfloat16) == EINVAL
    assert fwd(16, 3, 3, torch.bfloat16) == EINVAL
    assert fwd(16, 3, 1, torch.bfloat16, null=True) == EINVAL
    _, dy = _tensor(1, 16, 6, 6, torch.bfloat16, torch.zeros(1, 16, 6, 6))
    xb, dx = _tensor(1, 16, 6, 6, torch.bfloat16)
    assert L.ymi_dwconv2d_bwd_data(_y(dy), None, 3, 1, None, _y(dx), _stream()) == EINVAL
    assert L.ymi_dwconv2d_bwd_data(_y(dy), _p(w), 7, 1, None, _y(dx), _stream()) == EINVAL
    assert L.ymi_dwconv2d_bwd_weight(_y(dx), _y(dy), 3, 3, _p(w), _p(w), 1 << 20, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((xb == SENTINEL).all())
