"""The fused SwinBlock MLP kernels (csrc/swin_mlp.hip) at the other two SwinBlock widths of the model files, 128 and 384 channels: the support
table, forward and backward data path against float64 with the product's rounding points, against the unfused kernels, and through the module.
The 256-channel instantiation keeps tests/test_gpu_swin_mlp_fused.py; the bounds here are that file's (bf16-rounding bounds: they do not grow with K)."""
import ctypes
import functools

import pytest
import torch

from swin_mlp_exact import decode_pre

pytestmark = pytest.mark.gpu

WIDTHS = [128, 384]
GUARD = 64          # sentinel rows behind row T of every row-major output
SENTINEL = -1984.0  # (exact in bf16; no input here comes near it)


def _lib():
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    return L, L.lib()


def _reference(x, gamma, beta, eps, w1, b1, w2, b2):
    """float64 on the bf16-rounded operands, with the product's storage roundings (u, pre, post in bf16): test_gpu_swin_mlp_fused.py::_reference"""
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    u = ((xd - mu) * rs * gamma.double() + beta.double()).to(torch.bfloat16)
    w1b, w2b = w1.to(torch.bfloat16).double(), w2.to(torch.bfloat16).double()
    pre = (u.double() @ w1b.t() + b1.double()).to(torch.bfloat16)
    post = torch.nn.functional.gelu(pre.double()).to(torch.bfloat16)
    out = post.double() @ w2b.t() + b2.double() + xd
    return u, mu[:, 0], rs[:, 0], pre, out


def _rows(t, c, ld, fill=None):
    """a [t, c] bf16 view with row stride ld over a buffer of t + GUARD rows; with `fill`, every element of the buffer holds it"""
    buf = torch.empty((t + GUARD, ld), dtype=torch.bfloat16, device="cuda:0")
    if fill is not None:
        buf.fill_(fill)
    return buf, buf[:t, :c]


def _untouched(buf, t, c):
    """the guard rows, and the pad columns of the rows in use, still hold the sentinel"""
    return bool((buf[t:] == SENTINEL).all()) and bool((buf[:t, c:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _case(c, t, hidden, strided=False):
    """inputs (as test_gpu_swin_mlp_fused.py::_inputs with c a parameter and w1 scaled by 1 / sqrt(c)), one training forward, the float64 reference:
    computed once per shape, shared by the tests below, never modified"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(1000 * c + t + hidden)
    dev = torch.device("cuda:0")
    ld = c + 8 if strided else c
    xbuf, x = _rows(t, c, ld, 0.0)
    x.copy_((torch.randn(t, c, generator=g) * 1.5 + 0.3).to(torch.bfloat16))
    gamma = (torch.rand(c, generator=g) + 0.5).to(dev)
    beta = (torch.randn(c, generator=g) * 0.3).to(dev)
    w1 = (torch.randn(hidden, c, generator=g) / c ** 0.5).to(dev)
    b1 = (torch.randn(hidden, generator=g) * 0.2).to(dev)
    w2 = (torch.randn(c, hidden, generator=g) / (hidden ** 0.5)).to(dev)
    b2 = (torch.randn(c, generator=g) * 0.2).to(dev)
    eps = 1e-5
    assert lib.ymi_swin_ln_mlp_supported(c, hidden, L.YMI_BF16)
    packed = torch.empty(lib.ymi_swin_ln_mlp_pack_elems(c, hidden), dtype=torch.bfloat16, device=dev)
    L.check(lib.ymi_swin_ln_mlp_pack(L.ptr(w1), L.ptr(w2), c, hidden, L.ptr(packed), L.stream_ptr()), "pack")
    ubuf, u = _rows(t, c, ld, SENTINEL)
    obuf, out = _rows(t, c, ld, SENTINEL)
    stats = torch.empty((2, t), dtype=torch.float32, device=dev)
    pre = torch.empty(lib.ymi_swin_ln_mlp_pre_elems(t, hidden), dtype=torch.bfloat16, device=dev)
    L.check(
        lib.ymi_swin_ln_mlp_fwd(ctypes.byref(L.as_ymi(x)), L.ptr(gamma), L.ptr(beta), eps, L.ptr(packed), L.ptr(b1), L.ptr(b2), hidden, ctypes.byref(L.as_ymi(u)),
                                L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(pre), ctypes.byref(L.as_ymi(out)), L.stream_ptr()),
        "swin_ln_mlp_fwd",
    )
    torch.cuda.synchronize()
    ref = _reference(x, gamma, beta, eps, w1, b1, w2, b2)
    return dict(c=c, t=t, hidden=hidden, ld=ld, x=x, gamma=gamma, beta=beta, eps=eps, w1=w1, b1=b1, w2=w2, b2=b2, packed=packed, u=u, ubuf=ubuf, out=out, obuf=obuf,
                stats=stats, pre=pre, ref=ref)


def test_support_table():
    """what the library takes - bf16, C in {128, 256, 384}, hidden a multiple of 32 within the width's LDS cap (4096 at 384) - and what the model routes"""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.ops import blocks

    L, lib = _lib()
    for c, hidden in [(128, 512), (384, 1536), (384, 32), (256, 1024), (384, 4096)]:
        assert lib.ymi_swin_ln_mlp_supported(c, hidden, L.YMI_BF16), (c, hidden)
    for c, hidden in [(320, 1280), (512, 2048), (384, 48), (384, 4096 + 32), (384, 8192)]:
        assert not lib.ymi_swin_ln_mlp_supported(c, hidden, L.YMI_BF16), (c, hidden)
    assert not lib.ymi_swin_ln_mlp_supported(384, 1536, L.YMI_F32)
    assert set(blocks.FUSED_SWIN_MLP_WIDTHS) <= {128, 256, 384}
    for c in blocks.FUSED_SWIN_MLP_WIDTHS:
        fc1 = torch.nn.Linear(c, 4 * c)
        assert ops.swin_ln_mlp_ok(torch.zeros((392, c), dtype=torch.bfloat16, device="cuda:0"), fc1), c


FWD_SHAPES = [(33, 32, False), (100, 64, False), (421, 128, False), (421, None, False), (100, 64, True)]  # hidden None = 4 C, the model's


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("t,hidden,strided", FWD_SHAPES)
def test_forward_against_float64(c, t, hidden, strided):
    """one chunk; two (the ring's prologue only); four (the three-stage ring wraps); the model's hidden width; a partial wave, a partial tile and
    two workgroups; row-strided x / u / out"""
    k = _case(c, t, hidden or 4 * c, strided)
    ru, rmu, rrs, rpre, rout = k["ref"]
    stats, u, out = k["stats"], k["u"], k["out"]
    e_mu = (stats[0].double() - rmu).abs().max().item()
    e_rs = ((stats[1].double() - rrs) / rrs).abs().max().item()
    du = (u.double() - ru.double()).abs()
    share_u = (du > 0).double().mean().item()
    err = (out.double() - rout).abs().max().item()
    rel = ((out.double() - rout).norm() / rout.norm()).item()
    print(f"\n[widths fwd C {c} T {t} hidden {k['hidden']} ld {k['ld']}] mean {e_mu:.2e} rstd {e_rs:.2e} u mismatch share {share_u:.2e} "
          f"out max {err / rout.abs().max().item():.2e} rel L2 {rel:.2e}")
    assert e_mu < 1e-5
    assert e_rs < 1e-5
    # u: the same value up to ONE bf16 step where the f32 LayerNorm arithmetic rounds the other way
    assert (du <= 2.0 ** -7 * ru.double().abs() + 1e-6).all() and share_u < 0.02
    assert err <= 2e-2 * rout.abs().max().item(), f"out: {err}"
    assert rel < 4e-3, f"out relative L2 {rel}"
    assert _untouched(k["ubuf"], t, c) and _untouched(k["obuf"], t, c)


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("t,hidden", [(33, 32), (421, None)])
def test_eval_equals_train(c, t, hidden):
    """the training variant only stores more: out with u = NULL is bit-identical"""
    L, lib = _lib()
    k = _case(c, t, hidden or 4 * c)
    obuf, out = _rows(t, c, c, SENTINEL)
    L.check(
        lib.ymi_swin_ln_mlp_fwd(ctypes.byref(L.as_ymi(k["x"])), L.ptr(k["gamma"]), L.ptr(k["beta"]), k["eps"], L.ptr(k["packed"]), L.ptr(k["b1"]), L.ptr(k["b2"]), k["hidden"],
                                None, None, None, None, ctypes.byref(L.as_ymi(out)), L.stream_ptr()),
        "swin_ln_mlp_fwd",
    )
    torch.cuda.synchronize()
    assert torch.equal(out, k["out"])
    assert _untouched(obuf, t, c)


@pytest.mark.parametrize("c", WIDTHS)
def test_forward_matches_the_unfused_kernels(c):
    """the kernels it replaces (ymi_layernorm_fwd + ymi_swin_mlp_fwd) on the same operands: same rounding points, different accumulation order"""
    L, lib = _lib()
    t, hidden = 421, 4 * c
    k = _case(c, t, hidden)
    x = k["x"]
    u2 = torch.empty_like(x)
    st2 = torch.empty((2, t), dtype=torch.float32, device=x.device)
    L.check(lib.ymi_layernorm_fwd(ctypes.byref(L.as_ymi(x)), 0, L.ptr(k["gamma"]), L.ptr(k["beta"]), k["eps"], ctypes.byref(L.as_ymi(u2)), L.ptr(st2[0]), L.ptr(st2[1]),
                                  L.stream_ptr()), "ln")
    w1p = k["w1"].to(torch.bfloat16).contiguous()
    w2p = k["w2"].to(torch.bfloat16).contiguous()
    pre2 = torch.empty((t, hidden), dtype=torch.bfloat16, device=x.device)
    post2 = torch.empty_like(pre2)
    out2 = torch.empty_like(x)
    L.check(lib.ymi_swin_mlp_fwd(ctypes.byref(L.as_ymi(u2)), L.ptr(w1p), L.ptr(k["b1"]), hidden, L.ptr(w2p), L.ptr(k["b2"]), ctypes.byref(L.as_ymi(x)),
                                 ctypes.byref(L.as_ymi(pre2)), ctypes.byref(L.as_ymi(post2)), ctypes.byref(L.as_ymi(out2)), L.stream_ptr()), "mlp")
    torch.cuda.synchronize()
    assert (k["u"].float() - u2.float()).abs().max().item() <= 2.0 ** -7 * u2.float().abs().max().item()
    assert ((k["out"].float() - out2.float()).norm() / out2.float().norm()).item() < 3e-3


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("t,hidden,strided", [(33, 32, False), (421, None, False), (421, None, True)])
def test_backward_data_path_against_float64(c, t, hidden, strided):
    """post = gelu(pre), d_pre = bf16(d_out W2) * gelu'(pre), d_u = d_pre W1, all as written row-major, against the float64 chain; the saved
    pre-activations the kernel reads back, decoded from their private layout (tests/swin_mlp_exact.py), against that chain's pre with the
    bounds of tests/test_gpu_swin_mlp_fused.py::test_fused_forward_against_float64"""
    L, lib = _lib()
    hidden = hidden or 4 * c
    k = _case(c, t, hidden)
    dev = k["x"].device
    g = torch.Generator().manual_seed(t + c)
    _, dout = _rows(t, c, c + 8 if strided else c, 0.0)
    dout.copy_((torch.randn(t, c, generator=g) * 0.5).to(torch.bfloat16))
    # post / dpre: the first t rows of buffers padded to whole 256-token tiles (the kernel stores every row of its tiles)
    cap = lib.ymi_swin_ln_mlp_pre_elems(t, hidden)
    post = torch.full((cap,), float("nan"), dtype=torch.bfloat16, device=dev).view(-1, hidden)[:t]
    dpre = torch.full((cap,), float("nan"), dtype=torch.bfloat16, device=dev).view(-1, hidden)[:t]
    dubuf, du = _rows(t, c, c, SENTINEL)
    L.check(lib.ymi_swin_ln_mlp_bwd_data(ctypes.byref(L.as_ymi(dout)), L.ptr(k["packed"]), L.ptr(k["pre"]), hidden, ctypes.byref(L.as_ymi(post)), ctypes.byref(L.as_ymi(dpre)),
                                         ctypes.byref(L.as_ymi(du)), L.stream_ptr()), "bwd_data")
    torch.cuda.synchronize()
    pd = k["ref"][3].double()
    dp = (decode_pre(k["pre"], c, t, hidden).double() - pd).abs()
    assert dp.max().item() <= 2.0 ** -6 * pd.abs().max().item()
    assert (dp > 2.0 ** -8 * (pd.abs() + 0.05)).double().mean().item() < 0.02
    rpost = torch.nn.functional.gelu(pd)
    w1b, w2b = k["w1"].to(torch.bfloat16).double(), k["w2"].to(torch.bfloat16).double()
    dpost = (dout.double() @ w2b).to(torch.bfloat16).double()
    grad = 0.5 * (1 + torch.erf(pd / 2 ** 0.5)) + pd * torch.exp(-pd * pd / 2) / (2 * torch.pi) ** 0.5
    rdpre = dpost * grad
    rdu = rdpre.to(torch.bfloat16).double() @ w1b
    dpo = (post.double() - rpost).abs()
    share_post = (dpo > 2.0 ** -7 * rpost.abs() + 1e-6).double().mean().item()
    e_dpre = ((dpre.double() - rdpre).norm() / rdpre.norm()).item()
    m_dpre = (dpre.double() - rdpre).abs().max().item() / rdpre.abs().max().item()
    e_du = ((du.double() - rdu).norm() / rdu.norm()).item()
    m_du = (du.double() - rdu).abs().max().item() / rdu.abs().max().item()
    print(f"\n[widths bwd C {c} T {t} hidden {hidden}] post beyond one step {share_post:.2e} dpre L2 {e_dpre:.2e} max {m_dpre:.2e} du L2 {e_du:.2e} max {m_du:.2e}")
    # post: within one bf16 step but where the kernel's f32 pre-activation rounded the other way (fewer than 2 %), and then by one step of pre
    assert share_post < 0.02
    assert (dpo <= 2.0 ** -6 * rpost.abs() + 1e-3).all()
    assert e_dpre < 4e-3, f"dpre {e_dpre}"
    assert m_dpre <= 3e-2
    assert e_du < 6e-3, f"du {e_du}"
    assert m_du <= 3e-2
    assert _untouched(dubuf, t, c)


def _rel(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("shape", [(2, 14, 14), (1, 10, 10)])  # T = 392; 10 x 10 padded to 14 x 14, T = 196
def test_through_the_module(c, shape):
    """SwinBlock(c, 2, 7), train mode, bf16 autocast: fused against unfused (HOOKS["fused_swin_mlp"]), output and every gradient"""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.nn.modules import SwinBlock
    from improving_yolov8_cbam_swinblock_amd.ops import blocks

    n, h, w = shape
    dev = torch.device("cuda:0")
    torch.manual_seed(17 * c + h)
    m = SwinBlock(c, 2, 7).to(dev).train()
    x = torch.randn(n, c, h, w, device=dev)
    wgt = torch.randn(n, c, h, w, device=dev)
    names = ["x"] + [nm for nm, _ in m.named_parameters()]
    probe = torch.zeros((8, c), dtype=torch.bfloat16, device=dev)

    def run(fused):
        # (a width the measurement left unrouted in the model is routed for this test: the kernels stay under test through the module)
        old, routed = ops.HOOKS["fused_swin_mlp"], blocks.FUSED_SWIN_MLP_WIDTHS
        ops.HOOKS["fused_swin_mlp"] = fused
        blocks.FUSED_SWIN_MLP_WIDTHS = (128, 256, 384)
        try:
            assert bool(ops.swin_ln_mlp_ok(probe, m.mlp[0])) == fused
            xg = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = m(xg)
            grads = torch.autograd.grad((y.float() * wgt).sum(), [xg] + list(m.parameters()))
            torch.cuda.synchronize()
            return y, grads
        finally:
            ops.HOOKS["fused_swin_mlp"], blocks.FUSED_SWIN_MLP_WIDTHS = old, routed

    yf, gf = run(True)
    yu, gu = run(False)
    errs = {"fwd": _rel(yf, yu)}
    for nm, a, b in zip(names, gf, gu):
        errs[nm] = _rel(a, b)
    print(f"\n[widths module C {c} {shape}] " + " ".join(f"{nm} {e:.2e}" for nm, e in errs.items()))
    assert errs["fwd"] < 3e-3, errs
    for nm in names:
        assert errs[nm] <= 1e-2, (nm, errs)  # GRAD_BOUND of tests/test_gpu_bf16_matched.py:36, the SwinBlock gradient bound (its line 230)
