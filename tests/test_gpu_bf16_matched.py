"""GPU: the bf16 kernels the benchmark times, held to a QUANTISATION-MATCHED oracle, and arg-max routing on tied values.

Why: float32 parity mode runs other kernel instantiations (v_mfma_f32_16x16x4_f32, no ping-pong tile, the
non-transposed attention kernels) than the bf16 step of bench.py, and a bf16 result compared with the plain float32
oracle needs bounds of 2e-2 .. 0.35 that a wrong row of a ragged tile would fit in.  Here both sides see the SAME
bf16-representable inputs, weights and output gradients, and the oracle rounds at the product's storage points
(oracle/quant.py: raw convolution output, block outputs, LayerNorm / QKV / attention / MLP tensors and their gradients),
so what is left is accumulation order plus the rare value that rounds the other way.  Bounds are written at the asserts.

Index work is bit-exact work: the max-pool cascade and CBAM's two max reductions are also run in float32 on inputs
quantised to 16 levels (nearly every max is tied) against fixtures produced by the reference's own modules
(tests/golden/make_golden.py ties) - ATen's "first maximum in scan order" rule (block.py:220-226, cbam.py:9,36,50).
"""
import numpy as np
import pytest
import torch

from conftest import LARGE_SWIN, golden_state, load_golden, load_large_swin

pytestmark = pytest.mark.gpu

# Relative-L2 bounds.  An UNMATCHED bf16 rounding of a tensor is 2^-9 / sqrt(3) = 1.1e-3; with matched storage points what is
# left is the fraction of values that round the other way because the float32 accumulation order differs (measured 1e-5 .. 1e-4
# per Conv block), plus, in SwinBlock, the probabilities P, which the attention kernels round before normalising (one-shot
# kernel) or per key tile against the running maximum (tiled kernel) where the oracle rounds softmax's output (measured
# 1e-3 / 2.7e-3 forward, up to 3.9e-3 on gradients).
CONV_BOUND = 1e-3
# Weight gradients: the split-K partial sums (one per pixel split, a float32 sum over >= 256 pixels) leave wgrad_kernel as
# bfloat16 slabs and are summed in float32 (csrc/wgrad.hip, round 3: half the slab traffic); the oracle has no such storage
# point.  One rounding of a partial is 1.1e-3 of ITS magnitude; on the sum of a zero-mean gradient that is 1.7e-3 whatever the number
# of splits (measured 1.66e-3 from 16 to 85 slabs: test_wgrad_bf16_slabs_at_bs32_model_shapes).  Launches with fewer than 16 splits
# keep float32 slabs (round 4: they write little slab traffic anyway; 1e-5 .. 5e-5 there), and the bound is 2e-3 for every case.
# float32 parity mode keeps float32 slabs.
WGRAD_BOUND = 2e-3
FWD_BOUND = 4e-3
GRAD_BOUND = 1e-2


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.asarray(a))


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


def q(x):
    """bf16-representable float32 values."""
    return x.bfloat16().float()


@pytest.mark.parametrize("cin,cout,k,s,hw", [(32, 64, 3, 2, 64), (64, 64, 3, 1, 40), (96, 64, 1, 1, 40), (256, 128, 1, 1, 20), (128, 256, 3, 2, 40),
                                             (64, 64, 3, 2, 21), (64, 128, 3, 2, 37),
                                             # >= 300 tiles of 256x128: the ping-pong form of igemm_kernel, forward and data gradient, ragged last
                                             # tile; 1x1; the four parity classes of a stride-2 data gradient in one launch
                                             (128, 128, 3, 1, 141), (256, 256, 1, 1, 100), (128, 256, 3, 2, 200),
                                             # more 3x3 stride-1 shapes: two column blocks, 64-column tiles, odd map sizes, tiles that straddle images
                                             # (this set also pinned round 3's LDS-resident 3x3 kernel, see profiles/r03_conv_bench_dconv3.txt)
                                             (128, 128, 3, 1, 80), (256, 256, 3, 1, 20), (128, 64, 3, 1, 40), (64, 128, 3, 1, 23), (32, 64, 3, 1, 61)])
def test_conv_block_bf16_vs_matched_oracle(cin, cout, k, s, hw):
    """Conv (conv -> train-mode BatchNorm -> SiLU) in bf16: igemm_kernel<bf16> with the statistics epilogue, the affine + SiLU
    kernel, BatchNorm backward, the data-gradient GEMM and wgrad_kernel, against the oracle on identical bf16-valued operands."""
    import oracle.modules as OM
    from oracle import quant
    from improving_yolov8_cbam_swinblock_amd.nn.modules import Conv

    torch.manual_seed(cin + cout)
    o = OM.Conv(cin, cout, k, s)
    for b in o.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.eps, b.momentum = 1e-3, 0.03
            b.weight.data.uniform_(0.5, 1.5)
            b.bias.data.normal_(0, 0.3)
    quant.round_weights_(o)
    m = Conv(cin, cout, k, s)
    for b in m.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.eps, b.momentum = 1e-3, 0.03
    m.load_state_dict(o.state_dict())
    m = m.to(dev()).train()
    o.train()
    x = q(torch.randn(4, cin, hw, hw))
    ho = (hw + 2 * (k // 2) - k) // s + 1
    gy = q(torch.randn(4, cout, ho, ho))
    xo = x.clone().requires_grad_(True)
    with quant.storage(torch.bfloat16):
        yo = o(xo)
        go = torch.autograd.grad(yo, [xo] + list(o.parameters()), gy)
    xg = x.to(dev()).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yg = m(xg)
    assert yg.dtype == torch.bfloat16
    gg = torch.autograd.grad(yg, [xg] + list(m.parameters()), gy.to(dev()).to(yg.dtype))
    errs = {"fwd": rel(yg, yo)}
    for a, b, n in zip(gg, go, ["x", "w", "gamma", "beta"]):
        errs[n] = rel(a, q(b) if n == "x" else b)   # the product stores the input gradient in bf16; the oracle's leaf gradient is not a stored tensor
    print(f"\n[matched conv {cin}->{cout} k{k} s{s} {hw}] " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert all(e <= (WGRAD_BOUND if n == "w" else CONV_BOUND) for n, e in errs.items()), errs


@pytest.mark.parametrize("cin,cout,k,hw", [(128, 128, 3, 80), (64, 64, 3, 160), (256, 128, 1, 80)])
def test_wgrad_bf16_slabs_at_bs32_model_shapes(cin, cout, k, hw):
    """the weight gradient at three layer shapes of the bs-32 step (dozens of bfloat16 first-level slabs per launch) against the matched
    oracle's float32 sum: <= 2e-3.  Measured 1.66e-3 at all three - the same as a launch with 16 slabs: for a zero-mean gradient the
    partial sums are as large as the total divided by sqrt(splits), so the relative error of the sum of rounded partials does NOT fall
    with the number of splits (round 3's comment claimed it would); it is one bfloat16 rounding's worth, 1.1e-3 x ~1.5, whatever the count."""
    import oracle.modules as OM
    from oracle import quant
    from improving_yolov8_cbam_swinblock_amd.nn.modules import Conv

    torch.manual_seed(cin + cout + k)
    o = OM.Conv(cin, cout, k, 1)
    _bn_defaults(o, randomize=True)
    quant.round_weights_(o)
    m = Conv(cin, cout, k, 1)
    _bn_defaults(m)
    m.load_state_dict(o.state_dict())
    m = m.to(dev()).train()
    o.train()
    x = q(torch.randn(32, cin, hw, hw))
    gy = q(torch.randn(32, cout, hw, hw))
    with quant.storage(torch.bfloat16):
        yo = o(x)
        (gw,) = torch.autograd.grad(yo, [o.conv.weight], gy)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yg = m(x.to(dev()))
    (gg,) = torch.autograd.grad(yg, [m.conv.weight], gy.to(dev()).to(yg.dtype))
    e = rel(gg, gw)
    print(f"\n[bs-32 wgrad {cin}->{cout} k{k} {hw}] dW {e:.2e}")
    assert e <= 2e-3, e


def _bn_defaults(m, randomize=False):
    for b in m.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.eps, b.momentum = 1e-3, 0.03
            if randomize:
                b.weight.data.uniform_(0.5, 1.5)
                b.bias.data.normal_(0, 0.3)


@pytest.mark.parametrize("kind,args,shape", [("Bottleneck", (64, 64, True, 1, ((3, 3), (3, 3)), 1.0), (4, 64, 40, 40)),
                                             ("C2f", (128, 128, 2, True), (4, 128, 40, 40)), ("C2f", (96, 64, 1, False), (2, 96, 80, 80)),
                                             ("SPPF", (256, 256, 5), (4, 256, 20, 20))])
def test_conv_composites_bf16_vs_matched_oracle(kind, args, shape):
    """Bottleneck (shortcut in cv2's BatchNorm + SiLU kernel), C2f (concat slots, gradient joins in the data-gradient epilogues) and
    SPPF (pool cascade between two 1x1 blocks) in bf16 against the storage-matched oracle."""
    import oracle.modules as OM
    from oracle import quant
    import improving_yolov8_cbam_swinblock_amd.nn.modules as PM

    torch.manual_seed(len(kind) + shape[1])
    o = getattr(OM, kind)(*args)
    _bn_defaults(o, True)
    quant.round_weights_(o)
    m = getattr(PM, kind)(*args)
    _bn_defaults(m)
    m.load_state_dict(o.state_dict())
    m = m.to(dev()).train()
    o.train()
    x = q(torch.randn(*shape))
    xo = x.clone().requires_grad_(True)
    with quant.storage(torch.bfloat16):
        yo = o(xo)
        gy = q(torch.randn(yo.shape))
        go = torch.autograd.grad(yo, [xo] + list(o.parameters()), gy)
    xg = x.to(dev()).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yg = m(xg)
    gg = torch.autograd.grad(yg, [xg] + list(m.parameters()), gy.to(dev()).to(yg.dtype))
    names = ["x"] + [n for n, _ in m.named_parameters()]
    errs = {"fwd": rel(yg, yo)}
    for n, a, b in zip(names, gg, go):
        errs[n] = rel(a, q(b) if n == "x" else b)
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    print(f"\n[matched {kind}{shape}] fwd {errs['fwd']:.2e}; worst " + " ".join(f"{n} {e:.2e}" for n, e in worst))
    assert errs["fwd"] <= FWD_BOUND, errs["fwd"]
    # SPPF: a value that rounds the other way in front of the pools re-routes a window's gradient (arg-max is discontinuous)
    bound = 3e-2 if kind == "SPPF" else GRAD_BOUND
    assert all(e <= bound for e in errs.values()), worst


@pytest.mark.parametrize("name", LARGE_SWIN + ["swin_d64_h4_20x20", "swin_d64_14x21"])
def test_swin_block_bf16_vs_matched_oracle(name):
    """SwinBlock in bf16 (gather + LayerNorm, the token GEMMs with their GELU / GELU' epilogues, window_attn_*_tr_kernel or the
    tiled attention kernels, LayerNorm backward with addends) against the oracle on identical bf16-valued operands, at the
    shapes of the reference fixtures (head_dim 32..192, 49- and 196-token windows, padded and unpadded)."""
    import oracle.modules as OM
    from oracle import quant
    from improving_yolov8_cbam_swinblock_amd.nn.modules import SwinBlock

    if name in LARGE_SWIN:
        o, x, gy, d, seeded = load_large_swin(name, lambda dim, heads, ws: OM.SwinBlock(dim, heads, ws))
        dim, heads, ws = o.dim, o.attn.num_heads, o.window_size
    else:
        d = load_golden(name)
        dim, heads, ws = d["x"].shape[1], int(d["heads"]), 7
        o = OM.SwinBlock(dim, heads, ws)
        o.load_state_dict(golden_state(d), strict=True)
        x, gy = t(d["x"]), t(d["gy"])
    quant.round_weights_(o)
    m = SwinBlock(dim, heads, ws)
    m.load_state_dict(o.state_dict(), strict=True)
    m = m.to(dev()).train()
    x, gy = q(x), q(gy)
    xo = x.clone().requires_grad_(True)
    with quant.storage(torch.bfloat16):
        yo = o(xo)
        go = torch.autograd.grad(yo, [xo] + list(o.parameters()), gy)
    xg = x.to(dev()).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yg = m(xg)
    gg = torch.autograd.grad(yg, [xg] + list(m.parameters()), gy.to(dev()).to(yg.dtype))
    names = ["x"] + [n for n, _ in m.named_parameters()]
    errs = {"fwd": rel(yg, yo)}
    for n, a, b in zip(names, gg, go):
        if n.endswith("in_proj_bias"):
            # the key third of the bias has a zero true gradient (softmax is invariant to a per-query constant): compare q and v thirds
            a, b = torch.cat((a[:dim], a[2 * dim:])), torch.cat((b[:dim], b[2 * dim:]))
        errs[n] = rel(a, b)
    print(f"\n[matched swin {name}] " + " ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    # six stored tensors in series in the forward, as many gradients in the backward: sqrt(6) x the single-rounding figure
    assert errs["fwd"] <= FWD_BOUND, errs
    for n in names:
        assert errs[n] <= GRAD_BOUND, (n, errs)


@pytest.mark.parametrize("k", [5, 7])
def test_maxpool_cascade_routes_ties_like_the_reference(k):
    """float32, inputs on 16 levels: values and routed gradients equal the reference's bit for bit (dyadic data: every sum exact)."""
    from improving_yolov8_cbam_swinblock_amd import ops

    d = load_golden(f"pool_ties_k{k}")
    x = t(d["x"]).to(dev()).requires_grad_(True)
    cat = ops.sppf_pool_cat(ops.to_internal(x, torch.float32), k)
    assert torch.equal(cat.float().cpu(), t(d["y"]))
    (gx,) = torch.autograd.grad(cat, x, t(d["gy"]).to(dev()))
    assert torch.equal(gx.float().cpu(), t(d["g.x"]))


@pytest.mark.parametrize("k,shape,dtype", [
    (5, (8, 256, 20, 20), torch.float32), (7, (8, 256, 20, 20), torch.float32), (5, (2, 64, 40, 40), torch.float32),
    (5, (8, 256, 20, 20), torch.bfloat16), (7, (4, 64, 20, 20), torch.bfloat16), (5, (2, 64, 40, 40), torch.bfloat16),
    (9, (2, 8, 13, 17), torch.float32),    # odd map, a window size without a compiled specialisation
    (3, (1, 16, 64, 64), torch.float32),   # backward too large for the whole-map kernel: stage by stage through the workspace
    (3, (1, 16, 96, 96), torch.float32),   # forward too: the tiled kernel
    # The tiled kernels in bfloat16.  The tiled backward rounds the running gradient to bfloat16 between its three stages, and the
    # equality below still holds EXACTLY, so it is not to be loosened: with these 16-level inputs every running gradient is a multiple
    # of 1/8 below 32 in magnitude, which bfloat16 holds exactly (stage-by-stage rounding and one final rounding of the oracle's
    # gradients give identical tensors for both shapes; largest magnitude 24.5 for the first row, 21.0 for the second).
    (5, (1, 16, 48, 48), torch.bfloat16),  # 2304 px > 1920: tiled backward at the model's k (forward: map form); C = 16 is half a
                                           # 32-channel slab (the overhang branch); 12 x 24 tiles, halos on both axes
    (3, (1, 40, 72, 72), torch.bfloat16),  # 5184 px > 4800: tiled forward too; C = 40: one full slab and one of a single chunk
    (9, (1, 8, 56, 56), torch.float32),    # tiled backward, run-time k, 4-pixel radius: 14 x 14 tiles of 149,120 LDS bytes, just under the limit
])
def test_maxpool_cascade_ties_at_model_shapes(k, shape, dtype):
    """the same at the model's SPPF shapes against the oracle (whose tie rule the fixtures above pin to the reference); bf16: the
    values are exact and the gradient, summed exactly in f32, is rounded once (whole-map kernel: the running gradient stays f32)."""
    import oracle.modules as OM
    from improving_yolov8_cbam_swinblock_amd import ops

    g = torch.Generator().manual_seed(k + shape[1])
    x = (torch.randint(0, 16, shape, generator=g).float() - 8) * 0.25
    gy = (torch.randint(0, 16, (shape[0], 4 * shape[1], shape[2], shape[3]), generator=g).float() - 8) * 0.125
    xo = x.clone().requires_grad_(True)
    ys = [xo]
    for _ in range(3):
        ys.append(OM.maxpool_same(ys[-1], k))
    co = torch.cat(ys, 1)
    (go,) = torch.autograd.grad(co, xo, gy)
    xg = x.to(dev()).requires_grad_(True)
    cg = ops.sppf_pool_cat(ops.to_internal(xg, dtype), k)
    (gg,) = torch.autograd.grad(cg, xg, gy.to(dev()))
    assert torch.equal(cg.float().cpu(), co.detach())
    assert torch.equal(gg.float().cpu(), go.to(dtype).float())


@pytest.mark.parametrize("name", ["cbam_ties_c32", "cbam_ties_flatca_c32"])
def test_cbam_routes_ties_like_the_reference(name):
    """float32 CBAM on tied inputs against the reference's own outputs: AdaptiveMaxPool2d (per-channel spatial max) and
    torch.max over channels (`flatca`: ca = 0.5 for every channel, so x * ca is tied across channels too)."""
    from improving_yolov8_cbam_swinblock_amd.nn.modules import CBAM

    d = load_golden(name)
    m = CBAM()
    if m.ca.shared_MLP is None:
        m.ca.create_mlp(d["x"].shape[1])
    m.load_state_dict(golden_state(d), strict=True)
    m = m.to(dev())
    x = t(d["x"]).to(dev()).requires_grad_(True)
    y = m(x)
    assert float((y.detach().float().cpu() - t(d["y"])).abs().max()) <= 1e-5
    names = ["x"] + [n for n, _ in m.named_parameters()]
    gs = torch.autograd.grad(y, [x] + list(m.parameters()), t(d["gy"]).to(dev()))
    for n, g in zip(names, gs):
        ref = t(d["g." + n])
        # a mis-routed tie moves single elements of dx by O(|gy|) ~ 1: float32 summation noise only is allowed
        assert float((g.float().cpu() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), n
