"""Element-by-element checks of the implicit-GEMM family (csrc/igemm.hip, csrc/wgrad.hip) against float64 host references.

A helper module for the tests (not a conftest).  Two gates:

  Gate 1 (placement): small-integer operands.  Every partial sum of an output element is an integer bounded by its MAGNITUDE
  sum(|a| |b|), so when the magnitude fits the storage format (< 2^24 for float32 points, <= 256 for bfloat16 points) every order
  and every split of the sum is exact, and the kernel's result must equal the float64 reference bit for bit.  The checker asserts
  the magnitude condition itself: a case that is not exact fails loudly instead of flaking.

  Gate 2 (precision): positive real operands, so the magnitude equals |reference|.  Per element
      |got - ref| <= r |ref| + (1 + r) gamma_K mag        r = 2^-8 (one RNE rounding to bfloat16) or 2^-24 (float32)
  gamma_K = K u / (1 - K u), u = 2^-24, bounds a float32 sum of K terms in any order (products of bfloat16 values are exact in
  float32; float32 products add one rounding each, which K counts).  Rounding the accumulated value z to the storage format adds
  r |z| <= r (|ref| + gamma_K mag).  Accumulating in bfloat16, rounding twice or truncating instead of rounding to nearest all
  exceed this bound; Gate 1 cannot see them.

Failures name the number of bad elements and the worst five as (n, h, w, c), with the GEMM row, its M-tile and N-tile in the tile
form that ran and the XCD that owns the tile (igemm.hip's ownership rule: XCD x runs the M blocks whose first row lies in its span
ymi_xcd_span(M) of the pixel order).
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24  # unit roundoff of float32
R_BF16 = 2.0 ** -8  # relative error of one round-to-nearest-even to bfloat16 (8-bit significand: half an ulp is 2^-8 of the value)
BF16_EXACT = 256.0  # integers up to 2^8 are bfloat16 values
F32_EXACT = 2.0 ** 24


def unit(dtype):
    return R_BF16 if dtype == torch.bfloat16 else U32


def gamma(k):
    ku = k * U32
    assert ku < 0.5, k
    return ku / (1.0 - ku)


# ---- float64 references (NCHW logical tensors, any device; the result lives on the host) -----------------------------------------
def _h(t):
    return t.detach().double().cpu()


def conv_fwd64(x, w, stride):
    k = w.shape[-1]
    return F.conv2d(_h(x), _h(w), stride=stride, padding=k // 2)


def conv_fwd_mag(x, w, stride):
    return conv_fwd64(_h(x).abs(), _h(w).abs(), stride)


def dgrad64(dy, w, x_shape, stride):
    k = w.shape[-1]
    return torch.nn.grad.conv2d_input(tuple(x_shape), _h(w), _h(dy), stride=stride, padding=k // 2)


def dgrad_mag(dy, w, x_shape, stride):
    return dgrad64(_h(dy).abs(), _h(w).abs(), x_shape, stride)


def wgrad64(x, dy, w_shape, stride):
    k = w_shape[-1]
    return torch.nn.grad.conv2d_weight(_h(x), tuple(w_shape), _h(dy), stride=stride, padding=k // 2)


def wgrad_mag(x, dy, w_shape, stride):
    return wgrad64(_h(x).abs(), _h(dy).abs(), w_shape, stride)


# ---- operands ----------------------------------------------------------------------------------------------------------------------
def ints(shape, gen, lo=-2, hi=2, density=1.0, nonzero=True):
    """integers in [lo, hi] (zero excluded when `nonzero`), each kept with probability `density` (float32, host)."""
    vals = [v for v in range(lo, hi + 1) if v != 0 or not nonzero]
    idx = torch.randint(0, len(vals), tuple(shape), generator=gen)
    t = torch.tensor(vals, dtype=torch.float32)[idx]
    if density < 1.0:
        t = t * (torch.rand(tuple(shape), generator=gen) < density).float()
    return t


def positive(shape, gen, lo=0.25, hi=1.0, dtype=torch.float32):
    """positive reals representable in `dtype` (float32 values on the host)."""
    return (lo + (hi - lo) * torch.rand(tuple(shape), generator=gen)).to(dtype).float()


# ---- tile bookkeeping (mirrors of igemm.hip's host side) ------------------------------------------------------------------------------
def xcd_span(m):
    """common.h ymi_xcd_span."""
    return (((m + 63) >> 6) + 7) >> 3 << 6


def xcd_blocks(m, bm, x):
    """[first, last) M blocks of XCD x (igemm_kernel's ownership rule)."""
    span, nmb = xcd_span(m), (m + bm - 1) // bm
    first = (x * span + bm - 1) // bm
    return first, min(((x + 1) * span + bm - 1) // bm, nmb)


def xcd_of_block(m, bm, mb):
    for x in range(8):
        f, l = xcd_blocks(m, bm, x)
        if f <= mb < l:
            return x
    return -1


def choose_tile(m, cout, ktot, bf16, fast, force=(0, 0)):
    """-> (bm, bn, honoured): igemm.hip choose_tile.  `fast`: every problem of the launch has whole-chunk taps (cpt % 4 == 0),
    the condition of the 256x128 ping-pong form.  honoured: whether a force (bm, bn) != (0, 0) was taken."""
    blocks = lambda bm, bn: ((m + bm - 1) // bm) * ((cout + bn - 1) // bn)
    if cout <= 32:
        t = (128, 32)
    elif cout <= 64:
        t = (128 if blocks(128, 64) >= 400 else 64, 64)
    elif blocks(128, 128) >= 400:
        t = (128, 64 if ktot <= 384 else 128)
    elif blocks(128, 64) >= 400:
        t = (128, 64)
    else:
        t = (64, 64)
    if bf16 and cout >= 128 and fast and blocks(256, 128) >= 300:
        t = (256, 128)
    fbm, fbn = force
    ok = fbm > 0 and fbn > 0 and (cout <= 32 if fbn <= 32 else True) and (fbm < 256 or (bf16 and fast))
    if ok:
        t = (fbm, fbn)
    return t[0], t[1], ok


def refusal_reason(force, cout, bf16, fast):
    fbm, fbn = force
    if fbn <= 32 and cout > 32:
        return f"{fbm}x{fbn} needs cout <= 32 (cout {cout})"
    if fbm == 256 and not bf16:
        return "256x128 is the bfloat16 ping-pong form"
    if fbm == 256 and not fast:
        return "256x128 needs input channels in whole 32-deep steps"
    return ""


def kform(cin, dtype, fast_only=False):
    """K-step form of a single-problem launch: 'wide' (bf16, 64-deep), 'fast' (32-deep bf16 / 16-deep f32), 'general'."""
    ch = 8 if dtype == torch.bfloat16 else 4
    cpt = cin // ch
    if dtype == torch.bfloat16 and cpt % 8 == 0 and not fast_only:
        return "wide"
    return "fast" if cpt % 4 == 0 else "general"


def dgrad_launches(n, h, w, cin, cout_dy, k, stride, dtype, force=(0, 0)):
    """-> list of launches of ymi_conv2d_bwd_data_add (igemm.hip dgrad_impl): dicts with the parity class(es), M per class, tile and
    whether a force was honoured.  h, w: dx's map; cout_dy: dy's channels (the K axis); cin: dx's channels (the GEMM's N)."""
    bf16 = dtype == torch.bfloat16
    ch = 8 if bf16 else 4
    cpt = cout_dy // ch
    pad = k // 2
    classes = []
    for cls in range(1 if stride == 1 else 4):
        ph, pw = (0, 0) if stride == 1 else (cls // 2, cls % 2)
        nt = sum(1 for i in range(k) for j in range(k) if (ph + pad - i) % stride == 0 and (pw + pad - j) % stride == 0)
        ho, wo = (h - ph + stride - 1) // stride, (w - pw + stride - 1) // stride
        if nt > 0 and ho > 0 and wo > 0:
            classes.append({"ph": ph, "pw": pw, "ho": ho, "wo": wo, "M": n * ho * wo, "ktot": nt * cpt * ch})
    fast = cpt % 4 == 0
    if cin >= 64 and len(classes) > 1:
        mmax = max(c["M"] for c in classes)
        bm, bn, ok = choose_tile(mmax * len(classes), cin, max(c["ktot"] for c in classes), bf16, fast, force)
        for c in classes:
            c.update(bm=bm, bn=bn, honoured=ok)
    else:
        for c in classes:
            c["bm"], c["bn"], c["honoured"] = choose_tile(c["M"], cin, c["ktot"], bf16, fast, force)
    return classes


def wgrad_plan(mpix, coutp, ng, bf16, targets=(1280, 768)):
    """-> (row tile, splits, slab_bf16, lanes): wgrad.hip wgrad_bm / wgrad_plan / the batched-sum lane count."""
    if not bf16:
        bm = 64
    elif coutp <= 32:
        bm = 32
    else:
        bm = 128 if (coutp >= 128 and coutp % 128 == 0) or coutp >= 256 else 64
    tiles = ((ng + 127) // 128) * ((coutp + bm - 1) // bm)
    target = targets[1] if bm == 128 else targets[0]
    s = (target + tiles - 1) // tiles
    smax = (mpix + 255) // 256
    s = max(1, min(s, smax))
    if s >= 8:
        s = (s + 7) // 8 * 8 if (s + 7) // 8 * 8 <= smax else s // 8 * 8
    pps = (mpix + s - 1) // s
    pps = (pps + 31) // 32 * 32
    s = (mpix + pps - 1) // pps
    lanes = 32 if s > 128 else 16 if s > 32 else 8 if s > 8 else 4
    return bm, s, bool(bf16 and s >= 16), lanes


def patch_width(ho, wo, mpix, bf16, patch_on=True):
    """wgrad.hip: the widest power-of-two patch width (32 .. 1) dividing Wo with 32 / width dividing Ho; 0: raster walk."""
    if not (bf16 and patch_on and mpix % 32 == 0):
        return 0
    for sh in range(5, -1, -1):
        if wo % (1 << sh) == 0 and ho % (32 >> sh) == 0:
            return 1 << sh
    return 0


# ---- locating elements ------------------------------------------------------------------------------------------------------------------
def gemm_locator(tile, m_total, row_of):
    """-> f(n, c, h, w) -> text: GEMM row, M-tile / N-tile of `tile` = (bm, bn) and the owning XCD.  row_of(n, h, w) -> GEMM row
    (or None for an element no GEMM row writes)."""
    bm, bn = tile

    def f(n, c, h, w):
        m = row_of(n, h, w)
        if m is None:
            return "no GEMM row"
        mb = m // bm
        return f"m={m} tile {bm}x{bn} M-tile {mb} N-tile {c // bn} XCD {xcd_of_block(m_total, bm, mb)}"

    return f


def fwd_row(ho, wo):
    return lambda n, h, w: (n * ho + h) * wo + w


def _fmt(idx, shape):
    if len(shape) == 4:
        n, c, h, w = idx
        return f"(n={n}, h={h}, w={w}, c={c})", (n, c, h, w)
    return str(tuple(idx)), None


def report(what, got, ref, bad, err, locate=None, limit=5):
    cnt = int(bad.sum())
    flat = torch.where(bad.reshape(-1), err.reshape(-1).nan_to_num(float("inf")), torch.full_like(err.reshape(-1), -1.0))
    order = torch.argsort(flat, descending=True)[: min(limit, cnt)]
    lines = [f"{what}: {cnt} of {bad.numel()} elements wrong; worst:"]
    for o in order.tolist():
        idx = list(torch.unravel_index(torch.tensor(o), bad.shape))
        idx = [int(i) for i in idx]
        txt, nchw = _fmt(idx, bad.shape)
        loc = f"  [{locate(*nchw)}]" if (locate and nchw is not None) else ""
        lines.append(f"  {txt}: got {float(got.reshape(-1)[o])!r} expected {float(ref.reshape(-1)[o])!r}{loc}")
    return "\n".join(lines)


# ---- Gate 1 -------------------------------------------------------------------------------------------------------------------------------
def exact_expected(ref, mag, dtype, slab_bf16=False, what=""):
    """the float64 reference as the storage format holds it, after asserting that the case is exact: magnitude < 2^24 (the float32
    accumulator; <= 256 where bfloat16 slabs hold partial sums) and the value itself representable (so its RNE conversion is itself)."""
    mmax = float(mag.max()) if mag.numel() else 0.0
    assert mmax < F32_EXACT, f"{what}: not an exact case: magnitude {mmax} >= 2^24"
    if slab_bf16:
        assert mmax <= BF16_EXACT, f"{what}: not an exact case: magnitude {mmax} > 256 with bfloat16 slabs"
    exp = ref.float().to(dtype).double()
    bad = exp != ref
    assert not bool(bad.any()), f"{what}: not an exact case: {int(bad.sum())} reference values are not {dtype} values (max |ref| {float(ref.abs().max())})"
    return exp


def check_exact(what, got, expected, locate=None):
    """Gate 1: bit-for-bit equality (got: any dtype / device; expected: float64 host)."""
    g = _h(got)
    assert g.shape == expected.shape, (what, tuple(g.shape), tuple(expected.shape))
    bad = ~(g == expected)
    if bool(bad.any()):
        raise AssertionError(report(what + " [Gate 1, exact]", g, expected, bad, (g - expected).abs(), locate))
    return 0.0


# ---- Gate 2 -------------------------------------------------------------------------------------------------------------------------------
def bound_plain(ref, mag, k_terms, dtype):
    """|got - ref| bound of a float32 K-term sum (plus affine terms counted in k_terms) rounded once to `dtype`."""
    r = unit(dtype)
    return r * ref.abs() + (1.0 + r) * gamma(k_terms) * mag


def bound_res2nd(z_ref, z_mag, k_terms, extra, dtype):
    """the res2nd storage points (igemm.hip: addends joined after the value was rounded into the LDS image - when the output rows are not
    4-element aligned, or after an activation): the float32 K-term sum is rounded to `dtype`, the addend `extra` added in float32 and the
    sum rounded again.  -> (reference, bound)."""
    r = unit(dtype)
    e_s = r * z_ref.abs() + (1.0 + r) * gamma(k_terms) * z_mag
    ref = z_ref + extra
    e = e_s + U32 * (z_ref.abs() + extra.abs() + e_s)
    return ref, r * ref.abs() + (1.0 + r) * e


def check_bound(what, got, ref, bound, locate=None):
    """Gate 2: per-element |got - ref| <= bound.  -> worst err / bound."""
    g = _h(got)
    assert g.shape == ref.shape, (what, tuple(g.shape), tuple(ref.shape))
    err = (g - ref).abs()
    bad = ~(err <= bound)  # (NaN fails)
    if bool(bad.any()):
        raise AssertionError(report(what + " [Gate 2, float64 bound]", g, ref, bad, err / bound.clamp(min=1e-300), locate))
    return float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0


# Activations of the epilogue (common.h silu_f / gelu_f) in float64, with the Lipschitz constants of the bound: max |silu'| = 1.0998,
# max |gelu'| = 1.1289.  Their float32 evaluation adds at most a few ulp of the result (16 allowed) and, for GELU, erf_as's absolute
# error 1.5e-7 times |x| / 2.
SILU_LIP, GELU_LIP = 1.1, 1.13


def silu64(z):
    return z * torch.sigmoid(z)


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def bound_act(z_ref, z_err, act_ref, act, dtype_stage, extra_ref=None, final_dtype=None):
    """bound on |stored act(stage(z)) (+ extra) - (act(z_ref) (+ extra))| where the kernel's float32 value z is within z_err of z_ref
    and is first rounded to `dtype_stage` (the LDS image), the activation evaluated in float32, the addend added in float32 and the result
    rounded to `final_dtype`."""
    r_s = unit(dtype_stage)
    e_stage = r_s * z_ref.abs() + (1.0 + r_s) * z_err
    lip = SILU_LIP if act == "silu" else GELU_LIP
    e_act = lip * e_stage + 16 * U32 * (act_ref.abs() + lip * e_stage) + (1e-7 * z_ref.abs() if act == "gelu" else 0.0)
    out_ref = act_ref + (extra_ref if extra_ref is not None else 0.0)
    e_sum = e_act + (2 * U32 * (act_ref.abs() + e_act + extra_ref.abs()) if extra_ref is not None else 0.0)
    r_f = unit(final_dtype or dtype_stage)
    return out_ref, r_f * out_ref.abs() + (1.0 + r_f) * e_sum


def gelu_grad64(z):
    """d gelu / dz = Phi(z) + z phi(z) (common.h gelu_grad_f in float64); |gelu'| <= 1.13."""
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def bound_mul(g_ref, g_err, x, dtype):
    """the activation-gradient multiplier epilogue (igemm.hip mul1: y = stored(v) * act'(x)): the kernel's float32 value v is within g_err
    of g_ref, is rounded to `dtype` (the stored value the product uses), multiplied in float32 by gelu_grad_f(x) - x is an operand the kernel
    reads, so act'(x) is evaluated at the same point on both sides; its float32 evaluation carries erf_as's 1.5e-7 / 2 and a few ulp
    (16 allowed) - and the product is rounded to `dtype`.  -> (reference, bound)."""
    d = gelu_grad64(x)
    r = unit(dtype)
    e1 = r * g_ref.abs() + (1.0 + r) * g_err
    e_d = 1e-7 + 16 * U32 * (d.abs() + 0.4 * x.abs())
    ref = g_ref * d
    e_p = e1 * (d.abs() + e_d) + g_ref.abs() * e_d
    e_p = e_p + U32 * (ref.abs() + e_p)
    return ref, r * ref.abs() + (1.0 + r) * e_p


def rel(a, b):
    """the suite's tensor-wide relative-L2 gate (test_gpu_bf16_matched.py, test_gpu_fuzz.py, ...)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))
