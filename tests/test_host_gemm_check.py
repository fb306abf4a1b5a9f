"""CPU: the element-wise GEMM checks of tests/gemm_exact.py catch the faults the suite's tensor-wide gates let through.

Each test plants one fault in a float64 result and asserts that the new checker flags it.  For the three placement faults (one element
off by one, one pixel missing from one weight-gradient sum, one tap dropped at one map corner) it also asserts that the relative-L2 gate
at 1e-3 that test_gpu_bf16_matched.py / test_gpu_fuzz.py use accepts the same fault at this shape: that is the gap the new checks close.
The two precision faults (bfloat16 accumulation, truncation instead of round-to-nearest-even) are planted at small K, where a relative
L2 bound is weakest, and must fail Gate 2."""
import pytest
import torch

import gemm_exact as G

REL_GATE = 1e-3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _conv_case(seed=1):
    g = _gen(seed)
    x = G.ints((4, 64, 40, 40), g)
    w = G.ints((128, 64, 3, 3), g, lo=-1, hi=1, density=0.05)
    ref, mag = G.conv_fwd64(x, w, 1), G.conv_fwd_mag(x, w, 1)
    return x, w, ref, mag


def _raises(fn, *args, **kw):
    with pytest.raises(AssertionError) as e:
        fn(*args, **kw)
    return str(e.value)


def test_gate1_accepts_the_exact_result_and_refuses_inexact_cases():
    x, w, ref, mag = _conv_case()
    exp = G.exact_expected(ref, mag, torch.bfloat16, what="fwd")
    G.check_exact("fwd", exp.to(torch.bfloat16), exp)
    # a case whose values do not fit bfloat16 is refused before any comparison
    big = torch.ones(1, 257, 4, 4)  # 257 is no bfloat16 value
    wb = torch.ones(1, 257, 1, 1)
    msg = _raises(G.exact_expected, G.conv_fwd64(big, wb, 1), G.conv_fwd_mag(big, wb, 1), torch.bfloat16, what="big")
    assert "not an exact case" in msg
    # exact values whose partial sums do not fit bfloat16 slabs: 300 terms of +-1 summing to 0
    alt = torch.ones(1, 300, 2, 2)
    wa = ((torch.arange(300) % 2) * 2 - 1).float().view(1, 300, 1, 1)
    msg = _raises(G.exact_expected, G.conv_fwd64(alt, wa, 1), G.conv_fwd_mag(alt, wa, 1), torch.bfloat16, slab_bf16=True, what="slab")
    assert "not an exact case" in msg


def test_one_element_off_by_one():
    x, w, ref, mag = _conv_case()
    exp = G.exact_expected(ref, mag, torch.bfloat16, what="fwd")
    got = exp.clone()
    got[2, 77, 13, 29] += 1.0
    assert G.rel(got, exp) <= REL_GATE  # the old gate accepts it
    loc = G.gemm_locator((128, 128), 4 * 40 * 40, G.fwd_row(40, 40))
    msg = _raises(G.check_exact, "fwd", got, exp, loc)
    assert "1 of" in msg and "(n=2, h=13, w=29, c=77)" in msg and "M-tile" in msg and "XCD" in msg


def test_one_pixel_missing_from_one_weight_gradient_sum():
    g = _gen(3)
    x = G.ints((2, 32, 48, 48), g, lo=-1, hi=1)
    dy = G.ints((2, 64, 48, 48), g, lo=-1, hi=1, density=0.5)
    ref, mag = G.wgrad64(x, dy, (64, 32, 3, 3), 1), G.wgrad_mag(x, dy, (64, 32, 3, 3), 1)
    exp = G.exact_expected(ref, mag, torch.float32, what="dw")
    # drop output pixel (n=1, h=20, w=31) from dW[co=5, ci=9, kh=0, kw=2]: the term dy[1, 5, 20, 31] * x[1, 9, 19, 32]
    n, h, w_, co, ci, kh, kw = 1, 20, 31, 5, 9, 0, 2
    term = float(dy[n, co, h, w_] * x[n, ci, h + kh - 1, w_ + kw - 1])
    if term == 0.0:
        dy[n, co, h, w_] = 1.0
        x[n, ci, h + kh - 1, w_ + kw - 1] = 1.0
        ref, mag = G.wgrad64(x, dy, (64, 32, 3, 3), 1), G.wgrad_mag(x, dy, (64, 32, 3, 3), 1)
        exp = G.exact_expected(ref, mag, torch.float32, what="dw")
        term = 1.0
    got = exp.clone()
    got[co, ci, kh, kw] -= term
    assert G.rel(got, exp) <= REL_GATE
    _raises(G.check_exact, "dw", got, exp)


def test_one_tap_dropped_at_one_map_corner():
    g = _gen(4)
    x = G.ints((2, 16, 320, 320), g)
    w = G.ints((16, 16, 3, 3), g, lo=-1, hi=1, density=0.5)
    ref, mag = G.conv_fwd64(x, w, 1), G.conv_fwd_mag(x, w, 1)
    exp = G.exact_expected(ref, mag, torch.bfloat16, what="fwd")
    # output pixel (n=1, h=319, w=319) - the last pixel of the last image - loses tap (dh, dw) = (0, -1): input pixel (319, 318), every channel
    got = exp.clone()
    got[1, :, 319, 319] -= (w[:, :, 1, 0].double() * x[1, :, 319, 318].double()).sum(1)
    assert int((got != exp).sum()) > 0
    assert G.rel(got, exp) <= REL_GATE
    msg = _raises(G.check_exact, "fwd", got, exp, G.gemm_locator((64, 64), 2 * 320 * 320, G.fwd_row(320, 320)))
    assert "h=319, w=319" in msg


def _small_k_gemm(seed=5, m=512, k=72, n=96):
    g = _gen(seed)
    a = G.positive((m, k), g, dtype=torch.bfloat16).double()
    b = G.positive((k, n), g, dtype=torch.bfloat16).double()
    return a, b, a @ b


def test_gate2_accepts_float32_accumulation_rounded_once():
    a, b, ref = _small_k_gemm()
    got = (a.float() @ b.float()).to(torch.bfloat16)
    G.check_bound("gemm", got, ref, G.bound_plain(ref, ref, a.shape[1], torch.bfloat16))
    got32 = a.float() @ b.float()
    G.check_bound("gemm f32", got32, ref, G.bound_plain(ref, ref, a.shape[1], torch.float32))


def test_sum_accumulated_in_bfloat16():
    a, b, ref = _small_k_gemm()
    acc = torch.zeros(ref.shape, dtype=torch.bfloat16)
    for k in range(a.shape[1]):
        acc = (acc.float() + (a[:, k : k + 1] * b[k : k + 1, :]).float()).to(torch.bfloat16)
    _raises(G.check_bound, "gemm", acc, ref, G.bound_plain(ref, ref, a.shape[1], torch.bfloat16))


def test_bfloat16_rounding_by_truncation():
    a, b, ref = _small_k_gemm(6)
    f = (a.float() @ b.float()).contiguous()
    trunc = (f.view(torch.int32) & ~0xFFFF).view(torch.float32)
    _raises(G.check_bound, "gemm", trunc, ref, G.bound_plain(ref, ref, a.shape[1], torch.bfloat16))


def test_an_extra_rounding_to_bfloat16_fails_gate2_for_float32_outputs():
    a, b, ref = _small_k_gemm(7)
    got = (a.float() @ b.float()).to(torch.bfloat16).float()
    _raises(G.check_bound, "gemm", got, ref, G.bound_plain(ref, ref, a.shape[1], torch.float32))


@pytest.mark.parametrize("bm", [32, 64, 128, 256])
def test_xcd_ownership_partitions_the_m_blocks(bm):
    """the mirror of igemm.hip's ownership rule the failure reports use: every M block has exactly one XCD, including M whose span is
    not a multiple of the tile and XCDs that own nothing."""
    for m in (1, 63, 100, 257, 1500, 4097, 76800):
        nmb = (m + bm - 1) // bm
        owners = [G.xcd_of_block(m, bm, mb) for mb in range(nmb)]
        assert all(o >= 0 for o in owners), (m, bm)
        counts = [0] * 8
        for x in range(8):
            f, l = G.xcd_blocks(m, bm, x)
            counts[x] = max(0, l - f)
        assert sum(counts) == nmb, (m, bm, counts)
