"""The final pass of a BatchNorm backward, riding in a weight-gradient launch and as its own launch: one function (csrc/common.h bn_final_block).

A deferred weight-gradient launch held back by ymi_wgrad_hold(1) is issued by the next BatchNorm backward of its stream with that layer's final pass
(dbeta, dgamma, the apply pass's coefficients) as extra workgroups at the front of its grid (csrc/wgrad.hip); with nothing held the pass is
chan_reduce_final_kernel (csrc/reduce_bwd.hip).  Both call the same body - 256 threads playing four row slices each, or 1024 playing one - so every
output word must be equal whichever ran, for every partial-row count that takes another branch of the body (fewer rows than slices, tail loop only,
main loop and tail, several main-loop trips), for channel counts that leave a rider workgroup half empty, and for the second gamma / beta of a pair.
The carrier's own result stays exact (tests/test_gpu_gemm_forms.py's Gate 1): the rider workgroups do not disturb it.
Reference behaviour: BatchNorm2d's backward inside Conv (nn/modules/conv.py:66-67,79)."""
import ctypes

import pytest
import torch

from test_gpu_gemm_forms import BF, F32, WGRAD, dname, wgrad_case, wgrad_verify
from test_gpu_handoff import _bn_bwd_reference

pytestmark = pytest.mark.gpu

FILL = 0xA5  # the byte a carrier's workspace holds until its launch writes the first slab


def reduce_blocks(pixels, c, cap=512):
    """partial rows of the reduce pass (csrc/reduce_bwd.hip reduce_blocks, red_cap at its default)"""
    tg = 1
    while tg < c // 4:
        tg <<= 1
    tg = min(tg, 256)
    ppb = min(64, max(16, (256 // tg) * 4))
    b = min(cap, max(1, -(-pixels // ppb)))
    return (b + 7) // 8 * 8


# shape (n, c, h, w), partial rows, split of a pair (0: one gamma / beta)
CASES = [
    ((1, 8, 5, 7), 8, 0),          # fewer rows than slices, C < 32
    ((2, 40, 24, 24), 24, 0),      # C not a multiple of 32: a half-empty rider workgroup
    ((2, 512, 20, 20), 56, 0),     # 16 rider workgroups, tail loop only
    ((2, 192, 40, 40), 200, 0),    # main loop and tail
    ((4, 64, 80, 80), 400, 0),     # several main-loop trips
    ((2, 96, 20, 20), 32, 64),     # ymi_bn_act_bwd_pair: second gamma / beta from channel 64 on
]
# carriers: deferred weight-gradient launches with >= 8 splits (the 1-D XCD-mapped grid a rider can join), each another kernel:
# dtype, name in WGRAD, row tile, bf16 slabs
CARRIERS = [(BF, "8-15 splits", 32, False), (BF, ">=16 splits", 64, True), (BF, "row tile 128", 128, False), (F32, "8-15 splits", 64, False)]


def _carrier_spec(name):
    (spec,) = [s for s in WGRAD if s[0] == name] or [s for s in WGRAD if s[0].startswith(name)]  # the row of that name, else the one it begins
    return spec


def _inputs(shape, dtype, split):
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    dev = torch.device("cuda:0")
    n, c, h, w = shape
    gen = torch.Generator(device="cpu").manual_seed(n * 1000 + c)
    raw = L.empty_nhwc(n, c, h, w, dtype, dev)
    dout = L.empty_nhwc(n, c, h, w, dtype, dev)
    raw.copy_(torch.randn(n, c, h, w, generator=gen) * 1.5)
    dout.copy_(torch.randn(n, c, h, w, generator=gen) * 0.3)
    gamma = (torch.rand(c, generator=gen) + 0.5).to(dev)
    beta = (torch.randn(c, generator=gen) * 0.2).to(dev)
    mean = raw.float().mean((0, 2, 3))
    inv = torch.rsqrt(raw.float().var((0, 2, 3), unbiased=False) + 1e-3)
    ws = torch.empty(2048 * 2 * c * 4 + 256, dtype=torch.uint8, device=dev)
    # a pair hands the library two parameter sets; the reference sees the channels in one row
    params = (gamma[:split].clone(), beta[:split].clone(), gamma[split:].clone(), beta[split:].clone()) if split else None
    return dout, raw, gamma, beta, mean, inv, ws, params


def _bn_bwd(dout, raw, gamma, beta, mean, inv, ws, params, split):
    """the BatchNorm + SiLU backward on the current stream into outputs poisoned with NaN -> draw, dgamma, dbeta"""
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    c = raw.shape[1]
    draw = L.empty_nhwc(*raw.shape, raw.dtype, raw.device)
    draw.fill_(float("nan"))
    dgamma = torch.full((c,), float("nan"), device=raw.device)
    dbeta = torch.full((c,), float("nan"), device=raw.device)
    ty = lambda t: ctypes.byref(L.as_ymi(t))
    if split:
        g1, b1, g2, b2 = params
        L.check(L.lib().ymi_bn_act_bwd_pair(ty(dout), ty(raw), L.ptr(g1), L.ptr(b1), L.ptr(g2), L.ptr(b2), split, L.ptr(mean), L.ptr(inv), L.ACT_SILU,
                                            ty(draw), L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws), ws.numel(), L.stream_ptr()), "bn_act_bwd_pair")
    else:
        L.check(L.lib().ymi_bn_act_bwd(ty(dout), ty(raw), L.ptr(gamma), L.ptr(mean), L.ptr(inv), L.ptr(beta), L.ACT_SILU, ty(draw), L.ptr(dgamma),
                                       L.ptr(dbeta), L.ptr(ws), ws.numel(), L.stream_ptr()), "bn_act_bwd")
    return draw, dgamma, dbeta


def _behind_a_held_carrier(carrier, seed, bn_args, expect_ride):
    """hold the carrier, run the BatchNorm backward behind it, release, sum the carrier's slabs -> the BatchNorm backward's outputs.
    Asserts that the carrier was held, that the BatchNorm backward issued it (expect_ride) or left it alone, and that its dW / dbias are exact."""
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    cdtype, cname, bm, slab16 = carrier
    L.check(L.lib().ymi_wgrad_hold(1), "wgrad_hold(1)")
    try:
        tag, rec, out, (_, _, got_slab16) = wgrad_case(cdtype, _carrier_spec(cname), True, seed, ws_fill=FILL)
        assert rec.splits >= 8, (tag, rec.splits)
        assert f" row tile {bm} " in tag and got_slab16 == slab16, f"{tag}: planned as another kernel than row tile {bm}, bf16 slabs {slab16}"
        cws = out[4]
        torch.cuda.synchronize()
        before = cws.clone()
        assert bool((before == FILL).all()), f"{tag}: the launch was not held"
        got = _bn_bwd(*bn_args)
        torch.cuda.synchronize()
        if expect_ride:
            assert not torch.equal(cws, before), f"{tag}: the BatchNorm backward did not issue the held launch"
        else:
            assert torch.equal(cws, before), f"{tag}: a BatchNorm backward that cannot carry a rider issued the held launch"
    finally:
        L.check(L.lib().ymi_wgrad_hold(0), "wgrad_hold(0)")
    recs = (type(rec) * 1)(rec)
    table = torch.empty(ctypes.sizeof(rec), dtype=torch.uint8, device=cws.device)
    L.check(L.lib().ymi_wgrad_reduce_batch(recs, 1, L.ptr(table), L.stream_ptr()), "wgrad_reduce_batch")
    torch.cuda.synchronize()
    wgrad_verify(tag, out)
    return got


def _same_every_word(got, own):
    for name, a, b in zip(("draw", "dgamma", "dbeta"), got, own):
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} words differ between the held-carrier call and the own launch"


@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{'x'.join(map(str, c[0]))}-rows{c[1]}" for c in CASES])
def test_final_pass_riding_equals_its_own_launch_every_word(case, dtype):
    shape, rows, split = CASES[case]
    n, c, h, w = shape
    assert reduce_blocks(n * h * w, c) == rows, (shape, reduce_blocks(n * h * w, c), rows)
    *args, params = _inputs(shape, dtype, split)
    bn_args = (*args, params, split)
    own = _bn_bwd(*bn_args)  # nothing held: chan_reduce_final_kernel
    torch.cuda.synchronize()
    carrier = CARRIERS[(case + 2 * (dtype == BF)) % len(CARRIERS)]  # every carrier serves both BatchNorm dtypes
    got = _behind_a_held_carrier(carrier, 700 + case, bn_args, expect_ride=True)
    _same_every_word(got, own)
    # and both are right: test_gpu_handoff.py's bounds (f32 accumulation of <= 2000-term chains: <= 1e-5 of the sum of magnitudes; draw: float32
    # rounding, or the stored bfloat16 rounding)
    dout, raw, gamma, beta, mean, inv = args[:6]
    rdraw, rdgamma, rdbeta, mag_g, mag_b = _bn_bwd_reference(dout, raw, gamma, beta, mean, inv)
    draw, dgamma, dbeta = got
    eg, eb = (dgamma.double() - rdgamma).abs(), (dbeta.double() - rdbeta).abs()
    ed, dtol = (draw.double() - rdraw).abs().max().item(), 1e-4 if dtype == F32 else 2e-2
    print(f"bn final {dname(dtype)} {shape} rows {rows} carrier {dname(carrier[0])} {carrier[1]}: dgamma err/mag {(eg / (mag_g + 1e-30)).max().item():.2e} "
          f"dbeta {(eb / (mag_b + 1e-30)).max().item():.2e} (bound 1e-5) draw {ed / (rdraw.abs().max().item() + 1e-6):.2e} (bound {dtol:.0e})")
    assert (eg <= 1e-5 * mag_g + 1e-30).all(), "dgamma"
    assert (eb <= 1e-5 * mag_b + 1e-30).all(), "dbeta"
    assert ed <= dtol * (rdraw.abs().max().item() + 1e-6), "draw"


def test_wide_batchnorm_does_not_ride():
    """1032 channels are two channel rows of the reduce pass: the rider is refused, the final pass is its own launch and the held launch stays held"""
    *args, params = _inputs((1, 1032, 4, 4), BF, 0)
    bn_args = (*args, params, 0)
    own = _bn_bwd(*bn_args)
    torch.cuda.synchronize()
    got = _behind_a_held_carrier(CARRIERS[0], 731, bn_args, expect_ride=False)
    _same_every_word(got, own)
