"""The three streaming passes of a Conv block's BatchNorm, each through every branch of its pixel walk.

The forward affine pass (csrc/elementwise.hip scale_shift_act_fixed_kernel), the backward reduce pass and the backward apply pass
(csrc/reduce_bwd.hip chan_reduce_kernel, bn_act_bwd_apply_kernel) walk pixels the same way: a thread keeps one 4-channel group, takes U = 4
pixels per trip with the next trip's loads issued before this trip's arithmetic, and finishes with a one-pixel tail loop.  A thread therefore
runs one of three branches - no pixel at all, the tail only, full trips and then the tail - and which one depends on the launch grid.  This file
restates the two grid rules and the XCD ownership of the pixel axis on the host, computes the per-thread pixel counts each case produces, asserts
that the case list reaches {0, 1, U-1, U, U+1, 2U, 2U+1} under both rules, and checks every output word of the C entry points against a float64
restatement.  The train-mode finalize rule (mean, clamped variance, 1 / sqrt(var + eps), momentum update with the unbiased variance) stands in
bn_finalize_kernel's launch and in the affine pass's prologue: the last test pins both.
Reference behaviour: Conv.forward = act(bn(conv(x))) with BatchNorm2d in train mode and its backward (nn/modules/conv.py:66-67,79)."""
import math

import pytest
import torch

from test_gpu_bn_final import reduce_blocks
from test_gpu_gemm_forms import BF, F32, byref, dname, on_dev, options, out_dev
from test_gpu_handoff import _bn_bwd_reference

pytestmark = pytest.mark.gpu

U = 4  # EW_U, RED_U, APPLY_U: pixels per trip of the walk
EW_PPT, EW_CAP, RED_CAP = 64, 512, 512  # the library's defaults of ew_ppt, ew_cap, red_cap

# Worst |err| / (|x * scale| + |shift| + |res| + 1) of the float32 affine pass against float64, over every case and form of this file, measured on the
# commit before the walk became one function: 1.46e-07 (GELU, whose erf is Abramowitz & Stegun 7.1.26 with absolute error <= 1.5e-7; SiLU through
# v_exp_f32 / v_rcp_f32: 1.38e-07; no activation: 8.27e-08).  The arithmetic is required not to change, so the bound is twice that, rounded up to
# one digit.  bfloat16 outputs add the stored rounding, 2^-8 |ref| (measured beyond it: 3.11e-08).
EW_F32_BOUND = 3e-7
# Worst |err| / (|ref| + 1) of save_mean, save_invstd, running_mean, running_var against float64 statistics of the library's own raw output, both
# entry points and both dtypes, same commit: 6.29e-08 (running_var; save_invstd 4.14e-08, save_mean 1.70e-08, running_mean 1.35e-08).  Twice that, one digit.
STAT_BOUND = 2e-7


# ------------------------------------------------------------------------------------------------ the grid rules, restated
def xcd_span(p):
    """csrc/common.h ymi_xcd_span"""
    return (((p + 63) >> 6) + 7) >> 3 << 6


def xcd_range(p, block, grid):
    """csrc/common.h xcd_range (xcd_shift at its default 0) -> lo, hi, index among the XCD's workgroups, their number"""
    span = xcd_span(p)
    lo = (block & 7) * span
    hi = min(lo + span, p)
    return min(lo, p), hi, block >> 3, grid >> 3


def stream_blocks(p, rows, ppt=EW_PPT, cap=EW_CAP):
    """workgroups of the affine and apply passes: ~ppt pixels per thread, one resident round for small maps, the cap, a multiple of 8"""
    gb = -(-p // (rows * ppt))
    if gb < 1024:
        gb = min(-(-p // rows), 1024)
    return (min(gb, cap) + 7) // 8 * 8


def stream_counts(p, c, cap=EW_CAP):
    """pixels walked by each thread of an affine / apply launch (fixed-group form: c / 4 <= 256), as a set"""
    groups = c // 4
    rows = 256 // groups
    grid = stream_blocks(p, rows, cap=cap)
    counts = set()
    for block in range(grid):
        lo, hi, bi, nbx = xcd_range(p, block, grid)
        step = nbx * rows
        for ty in range(rows):
            first = lo + bi * rows + ty
            counts.add(0 if first >= hi else -(-(hi - first) // step))
    return counts


def reduce_counts(p, c, cap=RED_CAP):
    """pixels walked by each thread of a reduce launch (threads whose channel group exists), as a set"""
    tg = 1
    while tg < c // 4:
        tg <<= 1
    rows = 256 // min(tg, 256)
    grid = reduce_blocks(p, c, cap)
    counts = set()
    for block in range(grid):
        lo, hi, bi, nbx = xcd_range(p, block, grid)
        per = -(-(hi - lo) // nbx)
        p0 = min(lo + bi * per, hi)
        p1 = min(p0 + per, hi)
        for ty in range(rows):
            counts.add(0 if p0 + ty >= p1 else -(-(p1 - p0 - ty) // rows))
    return counts


# shape (n, c, h, w), value of ew_cap and red_cap (None: defaults), per-thread pixel counts under the affine / apply rule and under the reduce rule
WALK_CASES = [
    ((1, 192, 9, 9), None, {0, 1, 2, 4, 5}, {0, 4, 5, 16}),  # 48 groups: 16 idle threads in every workgroup
    ((1, 512, 9, 9), 8, {0, 8, 9, 32}, {0, 8, 9, 32}),       # one workgroup per XCD: two and more trips
    ((1, 64, 5, 7), None, {0, 2, 3}, {0, 2, 3}),             # tail loop only
    ((1, 8, 5, 7), None, {0, 1}, {0, 1}),
]
# more than 1024 channels: the flat group-stride forms of the affine and apply passes, two channel rows of the reduce pass
CASES = WALK_CASES + [((2, 1032, 4, 4), None, None, None)]
NOVEC = ((1, 6, 5, 7), None, None, None)  # channels no multiple of 4: the scalar affine form (float32 only)


def case_id(case):
    return "x".join(map(str, case[0])) + (f"-cap{case[1]}" if case[1] else "")


def caps(cap):
    return options(ew_cap=cap, red_cap=cap) if cap else options()


def test_cases_walk_every_branch_under_both_grid_rules():
    """no pixel, tail only (1, U - 1), exactly one trip (U), a trip and the tail (U + 1), two trips (2U), two trips and the tail (2U + 1)"""
    need = {0, 1, U - 1, U, U + 1, 2 * U, 2 * U + 1}
    seen_stream, seen_reduce = set(), set()
    for (n, c, h, w), cap, want_stream, want_reduce in WALK_CASES:
        s, r = stream_counts(n * h * w, c, cap or EW_CAP), reduce_counts(n * h * w, c, cap or RED_CAP)
        assert s == want_stream and r == want_reduce, ((n, c, h, w), cap, sorted(s), sorted(r))
        seen_stream |= s
        seen_reduce |= r
    assert need <= seen_stream, f"affine / apply rule: no case gives a thread {sorted(need - seen_stream)} pixels"
    assert need <= seen_reduce, f"reduce rule: no case gives a thread {sorted(need - seen_reduce)} pixels"
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    assert (L.get_option("ew_ppt"), L.get_option("ew_cap"), L.get_option("red_cap")) == (EW_PPT, EW_CAP, RED_CAP)


# ------------------------------------------------------------------------------------------------ inputs, shared by the tests of a case
_inputs_cache = {}


def inputs(shape, dtype):
    """seeded raw / second operand / per-channel vectors of a case, made once and never written again"""
    key = (shape, dtype)
    if key not in _inputs_cache:
        from improving_yolov8_cbam_swinblock_amd import _lib as L

        dev = torch.device("cuda:0")
        n, c, h, w = shape
        gen = torch.Generator(device="cpu").manual_seed(n * 1000 + c)
        raw = L.empty_nhwc(n, c, h, w, dtype, dev)
        other = L.empty_nhwc(n, c, h, w, dtype, dev)  # the residual of the affine pass, dout of the backward
        raw.copy_(torch.randn(n, c, h, w, generator=gen) * 1.5)
        other.copy_(torch.randn(n, c, h, w, generator=gen) * 0.3)
        gamma = (torch.rand(c, generator=gen) + 0.5).to(dev)
        beta = (torch.randn(c, generator=gen) * 0.2).to(dev)
        mean = raw.float().mean((0, 2, 3))
        inv = torch.rsqrt(raw.float().var((0, 2, 3), unbiased=False) + 1e-3)
        _inputs_cache[key] = (raw, other, gamma, beta, mean, inv)
    return _inputs_cache[key]


def poisoned(like):
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    t = L.empty_nhwc(*like.shape, like.dtype, like.device)
    t.fill_(float("nan"))
    return t


# ------------------------------------------------------------------------------------------------ the forward affine pass
def act64(z, act):
    if act == 1:
        return z * torch.sigmoid(z)
    if act == 2:
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return z


def affine_call(raw, scale, shift, act, res):
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    out = poisoned(raw)
    L.check(L.lib().ymi_scale_shift_act(byref(raw), L.ptr(scale), L.ptr(shift), act, byref(res), byref(out), L.stream_ptr()), "scale_shift_act")
    return out


def affine_error(out, raw, scale, shift, act, res):
    """-> worst float32-part error in units of (|x * scale| + |shift| + |res| + 1), after taking off what a bfloat16 store may round"""
    x = raw.double()
    sc = scale.double()[None, :, None, None] if scale is not None else torch.ones((), dtype=torch.float64, device=raw.device)
    sh = shift.double()[None, :, None, None] if shift is not None else torch.zeros((), dtype=torch.float64, device=raw.device)
    r = res.double() if res is not None else torch.zeros_like(x)
    ref = act64(x * sc + sh, act) + r
    err = (out.double() - ref).abs()
    assert not bool(torch.isnan(out).any()), "output words left unwritten"
    if out.dtype == BF:
        err = (err - 2.0 ** -8 * ref.abs()).clamp(min=0.0)
    return float((err / ((x * sc).abs() + sh.abs() + r.abs() + 1.0)).max())


AFFINE_FORMS = [(act, with_res, with_affine) for act in (0, 1, 2) for with_res in (False, True) for with_affine in (True, False)]


def affine_outputs(case, dtype):
    """every form of the affine pass on one case -> [(form, out, error)]"""
    shape, cap = case[0], case[1]
    raw, other, gamma, beta, _, _ = inputs(shape, dtype)
    got = []
    with caps(cap):
        for act, with_res, with_affine in AFFINE_FORMS:
            scale, shift, res = (gamma if with_affine else None), (beta if with_affine else None), (other if with_res else None)
            out = affine_call(raw, scale, shift, act, res)
            got.append(((act, with_res, with_affine), out, affine_error(out, raw, scale, shift, act, res)))
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("case,dtype", [(c, d) for c in CASES for d in (F32, BF)] + [(NOVEC, F32)], ids=lambda v: dname(v) if isinstance(v, torch.dtype) else case_id(v))
def test_affine_pass_every_word(case, dtype):
    """ymi_scale_shift_act: activation none / SiLU / GELU, with and without a residual, scale and shift given or both null"""
    got = affine_outputs(case, dtype)
    worst = max(e for _, _, e in got)
    for form, _, e in got:
        print(f"affine {dname(dtype)} {case_id(case)} act {form[0]} residual {form[1]} scale/shift {form[2]}: err {e:.2e} (bound {EW_F32_BOUND:.0e})")
    assert worst <= EW_F32_BOUND, (case_id(case), [(f, e) for f, _, e in got if e > EW_F32_BOUND])


# ------------------------------------------------------------------------------------------------ the backward reduce and apply passes
def bn_bwd_outputs(case, dtype):
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    shape, cap = case[0], case[1]
    raw, dout, gamma, beta, mean, inv = inputs(shape, dtype)
    c = shape[1]
    draw = poisoned(raw)
    dgamma = torch.full((c,), float("nan"), device=raw.device)
    dbeta = torch.full((c,), float("nan"), device=raw.device)
    rows = reduce_blocks(raw.numel() // c, c, cap or RED_CAP)
    ws = torch.empty((rows * 2 * c + 6 * c) * 4 + 64 * c * 8, dtype=torch.uint8, device=raw.device)  # partial rows, coefficients, the bn_tail option's rows
    with caps(cap):
        L.check(L.lib().ymi_bn_act_bwd(byref(dout), byref(raw), L.ptr(gamma), L.ptr(mean), L.ptr(inv), L.ptr(beta), L.ACT_SILU, byref(draw), L.ptr(dgamma),
                                       L.ptr(dbeta), L.ptr(ws), ws.numel(), L.stream_ptr()), "bn_act_bwd")
        torch.cuda.synchronize()
    return draw, dgamma, dbeta


@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bn_backward_every_word(case, dtype):
    """ymi_bn_act_bwd (SiLU): the reduce pass's sums and the apply pass's draw, tests/test_gpu_handoff.py's reference and bounds"""
    draw, dgamma, dbeta = bn_bwd_outputs(case, dtype)
    raw, dout, gamma, beta, mean, inv = inputs(case[0], dtype)
    rdraw, rdgamma, rdbeta, mag_g, mag_b = _bn_bwd_reference(dout, raw, gamma, beta, mean, inv)
    eg, eb = (dgamma.double() - rdgamma).abs(), (dbeta.double() - rdbeta).abs()
    ed, dtol = (draw.double() - rdraw).abs().max().item(), 1e-4 if dtype == F32 else 2e-2
    print(f"bn backward {dname(dtype)} {case_id(case)}: dgamma err/mag {(eg / (mag_g + 1e-30)).max().item():.2e} dbeta {(eb / (mag_b + 1e-30)).max().item():.2e} "
          f"(bound 1e-5) draw {ed / (rdraw.abs().max().item() + 1e-6):.2e} (bound {dtol:.0e})")
    assert (eg <= 1e-5 * mag_g + 1e-30).all(), "dgamma"
    assert (eb <= 1e-5 * mag_b + 1e-30).all(), "dbeta"
    assert not bool(torch.isnan(draw).any()) and ed <= dtol * (rdraw.abs().max().item() + 1e-6), "draw"


def colsum_output(case, dtype):
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    shape, cap = case[0], case[1]
    raw = inputs(shape, dtype)[0]
    c = shape[1]
    out = torch.full((c,), float("nan"), device=raw.device)
    ws = torch.empty(reduce_blocks(raw.numel() // c, c, cap or RED_CAP) * 2 * c * 4, dtype=torch.uint8, device=raw.device)
    with caps(cap):
        L.check(L.lib().ymi_colsum(byref(raw), L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()), "colsum")
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_colsum_every_word(case, dtype):
    """ymi_colsum: the reduce pass with one input.  float32 accumulation of short chains: <= 1e-5 of the sum of magnitudes, as for dbeta"""
    out = colsum_output(case, dtype)
    x = inputs(case[0], dtype)[0].double()
    err, mag = (out.double() - x.sum((0, 2, 3))).abs(), x.abs().sum((0, 2, 3))
    print(f"colsum {dname(dtype)} {case_id(case)}: err/mag {(err / (mag + 1e-30)).max().item():.2e} (bound 1e-5)")
    assert (err <= 1e-5 * mag + 1e-30).all()


# ------------------------------------------------------------------------------------------------ the finalize rule, in both of its places
FIN_SHAPE = (2, 16, 12, 12, 64)  # n, cin, h, w, cout of a 1x1 convolution
MOMENTUM, EPS = 0.03, 1e-3


def conv_bn_outputs(dtype, acc):
    """Conv 1x1 + train-mode BatchNorm + SiLU through ymi_conv2d_bn_silu_fwd_acc (finalize in the affine pass's prologue) or
    ymi_conv2d_bn_silu_fwd (bn_finalize_kernel) -> raw, out, save_mean, save_invstd, running_mean, running_var, and the parameters"""
    from improving_yolov8_cbam_swinblock_amd import _lib as L
    from improving_yolov8_cbam_swinblock_amd import ops

    n, cin, h, w, cout = FIN_SHAPE
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    x, _ = on_dev(torch.randn(n, cin, h, w, generator=g), dtype)
    wp = ops.pack_conv_fwd((torch.randn(cout, cin, 1, 1, generator=g) * 0.25).to(dev), cin, dtype)
    gamma, beta = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.2).to(dev)
    rm0, rv0 = (torch.randn(cout, generator=g) * 0.1).to(dev), (torch.rand(cout, generator=g) + 0.5).to(dev)
    rm, rv = rm0.clone(), rv0.clone()
    raw, _ = out_dev(n, cout, h, w, dtype, fill=float("nan"))
    out, _ = out_dev(n, cout, h, w, dtype, fill=float("nan"))
    sm, si = torch.full((cout,), float("nan"), device=dev), torch.full((cout,), float("nan"), device=dev)
    if acc:
        stat = torch.zeros(4, 2, cout, dtype=torch.int64, device=dev)
        L.check(L.lib().ymi_conv2d_bn_silu_fwd_acc(byref(x), L.ptr(wp), cout, 1, 1, 1, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), MOMENTUM, EPS, L.ACT_SILU,
                                                   None, byref(raw), byref(out), L.ptr(sm), L.ptr(si), L.ptr(stat), L.stream_ptr()), "conv2d_bn_silu_fwd_acc")
    else:
        rows = L.lib().ymi_conv2d_stat_blocks(n * h * w, cout) + 64  # (+ bn_finalize's staging rows)
        ws = torch.empty((rows * 2 * cout + 2 * cout) * 4, dtype=torch.uint8, device=dev)
        L.check(L.lib().ymi_conv2d_bn_silu_fwd(byref(x), L.ptr(wp), cout, 1, 1, 1, L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), MOMENTUM, EPS, L.ACT_SILU,
                                               None, byref(raw), byref(out), L.ptr(sm), L.ptr(si), L.ptr(ws), ws.numel(), L.stream_ptr()), "conv2d_bn_silu_fwd")
    torch.cuda.synchronize()
    return (raw, out, sm, si, rm, rv), (gamma, beta, rm0, rv0)


@pytest.mark.parametrize("acc", [True, False], ids=["prologue", "finalize-kernel"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
def test_finalize_rule_in_both_places(dtype, acc):
    """saved and running statistics and the activated output against float64 statistics of the library's own raw convolution output"""
    (raw, out, sm, si, rm, rv), (gamma, beta, rm0, rv0) = conv_bn_outputs(dtype, acc)
    y = raw.double()
    assert not bool(torch.isnan(y).any())
    count = y.shape[0] * y.shape[2] * y.shape[3]
    mean = y.mean((0, 2, 3))
    var = ((y * y).mean((0, 2, 3)) - mean * mean).clamp(min=0.0)
    inv = 1.0 / torch.sqrt(var + EPS)
    want = {
        "save_mean": (sm, mean),
        "save_invstd": (si, inv),
        "running_mean": (rm, (1.0 - MOMENTUM) * rm0.double() + MOMENTUM * mean),
        "running_var": (rv, (1.0 - MOMENTUM) * rv0.double() + MOMENTUM * var * count / (count - 1.0)),
    }
    errs = {k: float(((got.double() - ref).abs() / (ref.abs() + 1.0)).max()) for k, (got, ref) in want.items()}
    scale = gamma.double() * inv
    shift = beta.double() - mean * scale
    eo = affine_error(out, raw, scale, shift, 1, None)
    print(f"finalize {dname(dtype)} {'prologue' if acc else 'finalize-kernel'}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f" (bound {STAT_BOUND:.0e}) out {eo:.2e} (bound {EW_F32_BOUND:.0e})")
    assert max(errs.values()) <= STAT_BOUND, errs
    assert eo <= EW_F32_BOUND, eo
