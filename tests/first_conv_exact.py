"""Element-by-element checks of the first-layer kernels (csrc/first_conv.hip) and of ymi_bn_finalize (csrc/elementwise.hip) against float64
host references.  A helper module for the tests (not a conftest); operands, gamma(), U32 and R_BF16 are those of tests/gemm_exact.py.

The kernel's arithmetic (header of first_conv.hip): image and weight rounded to bfloat16; the 27 products accumulated in float32 (an MFMA
over K = 36, padded to 64); the sum rounded to bfloat16 = `raw`; everything downstream computed from `raw`.  References are float64 of the
operands AS STORED.  Three kinds of operands:

  "int"    (Gate 1, placement)  image in {-1, 0, 1}, weights in {-2 .. 2}: |raw| <= 54 and sum|x||w| <= 256, so `raw` is an exact small
           integer whatever the order of the sum, and the per-tile partial rows (sums of raw and raw^2 over <= 512 pixels, integers
           below 2^24) are known bit for bit.  A misplaced tap, pixel or channel moves raw by at least 1.
  "dyadic" (Gate 1 with a real rounding)  image and weights in {-16 .. 16} / 16: every partial sum is a multiple of 2^-8 below 2^24 * 2^-8,
           so the float32 accumulation is still exact in any order, but the sum needs up to 13 bits: raw = RNE_bf16(conv64) is known bit
           for bit AND is a rounded value.  Only here can "statistics of the unrounded convolution" or "xhat of the unrounded raw" show.
  "pos"    (Gate 2, precision of the accumulation)  image and weights from gemm_exact.positive (bfloat16 values in [0.25, 1]): the
           float32 accumulate z has |z - conv64| <= e = gamma(64) mag, mag = conv(|x|, |w|) = conv64, so raw is RNE(conv64 - e) or
           RNE(conv64 + e): at most two neighbouring bfloat16 values.  float64 is rounded to bfloat16 directly (through float32 rounds
           twice).  An `out` element passes if it is within the bound of the reference from either candidate; no element is left out.
           The share of elements with two candidates is printed and may not exceed 1 % (0.13 % at 2 x 3 x 48 x 264 -> 32 channels).

Bounds (all derived; SB = STAT_BOUND and EW = EW_F32_BOUND are the project's measured constants of tests/test_gpu_bn_stream.py):
  statistics   save_mean, save_invstd, running_mean, running_var: |got - ref| <= SB (|ref| + 1) against float64 statistics of raw
               (unbiased variance in the running update, momentum 0.03, eps 1e-3).  "pos": plus the interval the undecided elements
               leave: raw = mid + eta, |eta_i| <= delta_i = hi_i - lo_i, so |d mean| <= sum delta / P and, since sum (mid_i - m) = 0,
               |d var| <= (2 sum |mid_i - m| delta_i + sum delta_i^2) / P; d inv = d var / 2 (var - d var + eps)^-3/2.  Also "pos": the
               per-tile sums are float32 sums of values that are not integers, a term passes through FC_SUM_DEPTH = 14 additions, so
               d mean += gamma(14) E|raw| and d var += gamma(15) E[raw^2] + 2 |mean| gamma(14) E|raw| (+ its square): sumsq / count -
               mean^2 cancels 50 to 1 on these operands (SB was measured on centred data; Gate 1's sums are exact).
  out          ref = act(raw scale + shift), scale = gamma inv, shift = beta - mean scale in float64.
               d_sc = |gamma| d_inv + u |scale|, d_sh = d_mean (|scale| + d_sc) + |mean| d_sc + 2u (|beta| + |mean scale|), with
               d_mean = SB (|mean| + 1), d_inv = SB (|inv| + 1) (+ the "pos" intervals): the statistics term.
               e = Lip (|raw| d_sc + d_sh) + EW (|raw scale| + |shift| + 1), Lip = 1.1 (SiLU) or 1;  bound = 2^-8 |ref| + (1 + 2^-8) e.
  partial rows "int": bit for bit.  "dyadic": gamma(513) sum|term| per tile (a float32 sum of <= 512 terms, the squares one rounding more).
  dbeta/dgamma xhat = (raw - mean) inv, z = xhat gamma + beta, dz = dout act'(z); float32: e_xh = 3u (|raw inv| + |mean inv|),
               e_z = |gamma| e_xh + 2u (|xhat gamma| + |beta|), e_dz = |dout| (e_z / 2 + SG (|z| + 1)) + u |dz| (max |silu''| = 1/2; SG below; no
               activation: e_dz = 0), e_t = e_dz (|xhat| + e_xh) + |dz| e_xh + u |dz xhat|.
               bound = gamma(P + 2) sum|term| + sum e_term: a float32 sum over P pixels in any order, the stored rounding included.
  dW           d(raw) = bf16(dz c0 - (raw c1 + c2)), the coefficients in float64 from the reference dgamma / dbeta by common.h
               bn_coef_write.  Its float32 evaluation is within e_d of the float64 value: e_dz through c0, the roundings of the
               coefficients and of the expression, and the distance of the sums the kernel built c1 and c2 from to the reference
               sums - the kernel's own dgamma / dbeta are its outputs, so that distance is known (capped by their bounds, which
               stand in when the outputs are not given: as worst cases of a P-term sum they alone would leave 10 - 20 % of the
               pixels undecided at P = 1188).  A pixel is UNDECIDED when the float64 value lies within e_d of a bfloat16 rounding
               boundary.  bound = gamma(P + 8) sum |x||d(raw)| + sum over the undecided pixels of |x| ulp_bf16(d(raw)).

SG = SILU_GRAD_F32 (|z| + 1): |silu_grad_f(z) - silu'(z)| of common.h's v_exp_f32 / v_rcp_f32 form at the same float32 argument (it grows
with |z|: 1 - s is formed from the rounded s and multiplied by z).  No constant for the derivative existed; measured through
ymi_first_conv_bn_act_bwd (one-hot dout per channel, gamma / beta null, mean 0, integer raw, so that dbeta[ch] IS
silu_grad_f(fl32(raw inv[ch]))) over 5120 arguments in [-54, 54] on commit 9b96dfd, the parent of the commit that adds this file, whose
kernels it leaves unchanged: worst 9.198e-08 (|z| + 1) = MEASURED_SILU_GRAD (6.84e-07 absolute).  Twice that, rounded up to one digit
(the convention of test_gpu_bn_stream.py): 2e-7.
"""
import functools

import torch
import torch.nn.functional as F

import gemm_exact as G
from gemm_exact import R_BF16, U32, gamma, ints, positive

BF = torch.bfloat16
FC_TH, FC_TW, FC_WG_TILES, BN_STAGE_ROWS = 8, 64, 4, 64  # first_conv.hip, common.h
MOMENTUM, EPS = 0.03, 1e-3
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
# additions a term of a per-tile partial sum passes through (FcStats / FcSums): 8 in its lane (2 rows x 4 groups), 4 levels over the 16 lanes of
# a DPP row, 2 over the four waves; the tiles are then summed in double.  The float32 sum of a tile is within gamma(14) sum|term| of the
# exact one (gamma(15) for the squares, one more rounding)
FC_SUM_DEPTH = 14
MEASURED_SILU_GRAD = 9.198e-08  # in units of |z| + 1, commit 9b96dfd
SILU_GRAD_F32 = 2e-7


@functools.lru_cache(maxsize=None)
def project_bounds():
    """(STAT_BOUND, EW_F32_BOUND) of tests/test_gpu_bn_stream.py, the project's documented constants"""
    import test_gpu_bn_stream as S

    return S.STAT_BOUND, S.EW_F32_BOUND


# ---- bfloat16 from float64, correctly ------------------------------------------------------------------------------------------------------
def ulp_bf16(v):
    """spacing of the bfloat16 values in the binade of |v| (8-bit significand): 2^(e - 8) for |v| in [2^(e-1), 2^e)"""
    _, e = torch.frexp(v.abs().double())
    return torch.exp2((e - 8).double())


def rne_bf16(v):
    """float64 -> the nearest bfloat16 value, ties to even, in ONE rounding (torch.round rounds halves to even; the scaling is exact)"""
    u = ulp_bf16(v)
    return torch.round(v.double() / u) * u


def trunc_bf16(v):
    u = ulp_bf16(v)
    return torch.trunc(v.double() / u) * u


def silu_grad64(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


# ---- geometry (mirrors of first_conv.hip's host side) ------------------------------------------------------------------------------------------
def geometry(n, h, w):
    ho, wo = h // 2, w // 2
    th, tw = -(-ho // FC_TH), -(-wo // FC_TW)
    units = n * th * tw
    wgs = -(-units // FC_WG_TILES)
    return {"ho": ho, "wo": wo, "tiles_h": th, "tiles_w": tw, "units": units, "last_tile_w": wo - (tw - 1) * FC_TW,
            "last_tile_rows": ho - (th - 1) * FC_TH, "wgs": wgs, "last_wg_tiles": units - (wgs - 1) * FC_WG_TILES,
            "staged": units > 16 * BN_STAGE_ROWS, "P": n * ho * wo}


def fwd_workspace_floats(n, h, w, cout):
    return 2 * cout + (geometry(n, h, w)["units"] + BN_STAGE_ROWS) * 2 * cout


def tile_sums(v):
    """[n, co, ho, wo] -> [unit, co] sums over each tile's pixels inside the map, unit = (n * tiles_h + th) * tiles_w + tw"""
    n, co, ho, wo = v.shape
    th, tw = -(-ho // FC_TH), -(-wo // FC_TW)
    p = F.pad(v, (0, tw * FC_TW - wo, 0, th * FC_TH - ho))
    return p.reshape(n, co, th, FC_TH, tw, FC_TW).sum((3, 5)).permute(0, 2, 3, 1).reshape(n * th * tw, co)


def locate(case):
    g = geometry(case.n, case.h, case.w)

    def f(n, c, h, w):
        th, tw = h // FC_TH, w // FC_TW
        return f"unit {(n * g['tiles_h'] + th) * g['tiles_w'] + tw} (tile row {th}, column {tw}) wave {h % 4} group {w % FC_TW // 16} channel tile {c // 16}"

    return f


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """operands of one case, as the caller hands them over (float32 on the host) and as stored (float64 of the bfloat16 values)"""

    def __init__(self, kind, n, c, h, w, cout, seed=0):
        self.kind, self.n, self.c, self.h, self.w, self.cout, self.seed = kind, n, c, h, w, cout, seed
        g = torch.Generator().manual_seed(1000003 * seed + 7919 * n + 131 * c + 17 * h + 3 * w + cout + {"int": 0, "dyadic": 1, "pos": 2}[kind])
        if kind == "int":
            self.img, self.wt = ints((n, c, h, w), g, -1, 1, nonzero=False), ints((cout, c, 3, 3), g, -2, 2, nonzero=False)
        elif kind == "dyadic":
            self.img, self.wt = ints((n, c, h, w), g, -16, 16, nonzero=False) / 16.0, ints((cout, c, 3, 3), g, -16, 16, nonzero=False) / 16.0
        else:
            self.img, self.wt = positive((n, c, h, w), g, dtype=BF), positive((cout, c, 3, 3), g, dtype=BF)
        self.x, self.ws = self.img.to(BF).double(), self.wt.to(BF).double()
        assert torch.equal(self.x, self.img.double()) and torch.equal(self.ws, self.wt.double())  # (every kind is bfloat16-representable)
        self.gamma, self.beta = (torch.rand(cout, generator=g) + 0.5), (torch.rand(cout, generator=g) - 0.5)
        self.rm0, self.rv0 = torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5
        self.dout = torch.randn(n, cout, h // 2, w // 2, generator=g).to(BF).float()
        self.bwd_mix = torch.rand(2, cout, generator=g)  # where the backward's save_mean / save_invstd sit relative to raw's own
        self.geo = geometry(n, h, w)

    @property
    def exact(self):
        return self.kind != "pos"

    def __repr__(self):
        return f"{self.kind}-{self.n}x{self.c}x{self.h}x{self.w}-co{self.cout}"


@functools.lru_cache(maxsize=None)
def make_case(kind, n, c, h, w, cout, seed=0):
    return Case(kind, n, c, h, w, cout, seed)


def conv64(x, w):
    return F.conv2d(x, w, stride=2, padding=1)


def _ch(v):
    return v.double().view(1, -1, 1, 1)


# ---- forward reference ---------------------------------------------------------------------------------------------------------------------------
def stats_of(raw, rm0, rv0):
    """the train-mode rule in float64: mean, clamped biased variance, 1 / sqrt(var + eps), momentum update with the UNBIASED variance"""
    P = raw.shape[0] * raw.shape[2] * raw.shape[3]
    mean = raw.mean((0, 2, 3))
    var = ((raw * raw).mean((0, 2, 3)) - mean * mean).clamp(min=0.0)
    return {"save_mean": mean, "var": var, "save_invstd": 1.0 / torch.sqrt(var + EPS), "running_mean": (1.0 - MOMENTUM) * rm0.double() + MOMENTUM * mean,
            "running_var": (1.0 - MOMENTUM) * rv0.double() + MOMENTUM * (var * P / (P - 1.0) if P > 1 else var)}


def act64(z, act):
    return G.silu64(z) if act == ACT_SILU else z


def out_reference(raw, st, gam, bet, act, d_mean_x=0.0, d_inv_x=0.0):
    """-> (reference, bound) of the block's output from `raw` (module docstring, "out")"""
    SB, EW = project_bounds()
    mean, inv, g, b = _ch(st["save_mean"]), _ch(st["save_invstd"]), _ch(gam), _ch(bet)
    scale = g * inv
    shift = b - mean * scale
    d_m = SB * (mean.abs() + 1.0) + d_mean_x
    d_i = SB * (inv.abs() + 1.0) + d_inv_x
    d_sc = g.abs() * d_i + U32 * scale.abs()
    d_sh = d_m * (scale.abs() + d_sc) + mean.abs() * d_sc + 2 * U32 * (b.abs() + (mean * scale).abs())
    ref = act64(raw * scale + shift, act)
    lip = G.SILU_LIP if act == ACT_SILU else 1.0
    e = lip * (raw.abs() * d_sc + d_sh) + EW * ((raw * scale).abs() + shift.abs() + 1.0)
    return ref, R_BF16 * ref.abs() + (1.0 + R_BF16) * e


class ForwardRef:
    pass


@functools.lru_cache(maxsize=None)
def forward_reference(case):
    r = ForwardRef()
    conv = conv64(case.x, case.ws)
    mag = conv64(case.x.abs(), case.ws.abs())
    what = f"{case}"
    r.conv, r.P = conv, case.geo["P"]
    r.share = 0.0
    r.d_mean = r.d_var = r.d_inv = torch.zeros(case.cout, dtype=torch.float64)
    if case.kind == "int":
        raw = G.exact_expected(conv, mag, BF, slab_bf16=True, what=what)
        assert float(raw.abs().max()) <= 54
        r.cands = (raw, raw)
    elif case.kind == "dyadic":
        assert float(mag.max()) * 256 < G.F32_EXACT and torch.equal(conv * 256, torch.round(conv * 256)), f"{what}: not an exact case"
        raw = rne_bf16(conv)
        r.cands = (raw, raw)
    else:
        assert torch.equal(mag, conv)
        e = gamma(64) * mag
        lo, hi = rne_bf16(conv - e), rne_bf16(conv + e)
        assert bool((hi - lo <= ulp_bf16(hi)).all()), f"{what}: more than two candidates"
        r.share = float((lo != hi).double().mean())
        print(f"[first conv Gate 2] {what}: {100 * r.share:.3f} % of the elements have two candidates")
        assert r.share <= 0.01, f"{what}: undecided share {r.share}"
        raw = rne_bf16(conv)  # one of the two candidates everywhere
        r.cands = (lo, hi)
        delta = hi - lo
        m = raw.mean((0, 2, 3))
        r.d_mean = delta.sum((0, 2, 3)) / r.P
        r.d_var = (2 * ((raw - _ch(m)).abs() * delta).sum((0, 2, 3)) + (delta * delta).sum((0, 2, 3))) / r.P
        # ... and the float32 per-tile sums, which positive operands do not leave exact (mean^2 is ~50 times the variance here)
        hi_m, hi_e2 = hi.mean((0, 2, 3)), (hi * hi).mean((0, 2, 3))
        d_m_sum = gamma(FC_SUM_DEPTH) * hi_m
        r.d_mean = r.d_mean + d_m_sum
        r.d_var = r.d_var + gamma(FC_SUM_DEPTH + 1) * hi_e2 + 2 * hi_m * d_m_sum + d_m_sum * d_m_sum
    r.raw = raw
    r.stats = stats_of(raw, case.rm0, case.rv0)
    if case.kind == "pos":
        r.d_inv = 0.5 * r.d_var * ((r.stats["var"] - r.d_var).clamp(min=0.0) + EPS) ** -1.5
    P = r.P
    r.stat_extra = {"save_mean": r.d_mean, "save_invstd": r.d_inv, "running_mean": MOMENTUM * r.d_mean, "running_var": MOMENTUM * r.d_var * (P / (P - 1.0) if P > 1 else 1.0)}
    if case.exact:
        r.partials = torch.stack([tile_sums(raw), tile_sums(raw * raw)], 1)  # [unit][2][co]
        r.partials_mag = torch.stack([tile_sums(raw.abs()), tile_sums(raw * raw)], 1)
        if case.kind == "int":
            assert float(r.partials_mag.max()) < G.F32_EXACT and torch.equal(r.partials, torch.round(r.partials))
    return r


def _collect(failures, fn, *a):
    try:
        return fn(*a)
    except AssertionError as e:
        failures.append(str(e))
        return float("inf")


def _raise(failures):
    if failures:
        raise AssertionError("\n".join(failures))


def check_forward(tag, got, case, act):
    """got: any of partials [unit, 2, co], save_mean, save_invstd, running_mean, running_var [co], out [n, co, ho, wo] -> worst error / bound
    per stage.  Raises ONE AssertionError naming every stage that fails, its number of bad elements and the worst five (out: with their tile)."""
    SB, _ = project_bounds()
    r = forward_reference(case)
    ratios, failures = {}, []
    if "partials" in got and case.exact:
        p = got["partials"].detach().double().cpu()
        what = f"{tag}: stage partials [unit][sum | sum of squares][channel]"
        if case.kind == "int":
            _collect(failures, G.check_exact, what, p, r.partials)
        else:
            ratios["partials"] = _collect(failures, G.check_bound, what, p, r.partials, gamma(513) * r.partials_mag + 1e-300)
    for k in ("save_mean", "save_invstd", "running_mean", "running_var"):
        if k in got:
            ref = r.stats[k]
            ratios[k] = _collect(failures, G.check_bound, f"{tag}: stage {k} [channel]", got[k], ref, SB * (ref.abs() + 1.0) + r.stat_extra[k])
    if "out" in got:
        g = got["out"].detach().double().cpu()
        assert g.shape == r.raw.shape, (tuple(g.shape), tuple(r.raw.shape))
        ok, ratio = None, None
        for cand in (r.cands if not case.exact else r.cands[:1]):
            ref, bound = out_reference(cand, r.stats, case.gamma, case.beta, act, _ch(r.d_mean), _ch(r.d_inv))
            q = ((g - ref).abs() / bound).nan_to_num(float("inf"))
            ok = (q <= 1.0) if ok is None else ok | (q <= 1.0)
            ratio = q if ratio is None else torch.minimum(ratio, q)
        if not bool(ok.all()):
            ref, _ = out_reference(r.raw, r.stats, case.gamma, case.beta, act)
            failures.append(G.report(f"{tag}: stage out [{'Gate 1' if case.exact else 'Gate 2, either candidate'}]", g, ref, ~ok, ratio, locate(case)))
        ratios["out"] = float(ratio.max())
    _raise(failures)
    return ratios


# ---- backward reference (exact kinds) ----------------------------------------------------------------------------------------------------------
class BackwardRef:
    pass


@functools.lru_cache(maxsize=None)
def backward_reference(case, act, affine=True):
    assert case.exact, "the backward is checked on operands whose raw is known bit for bit"
    f = forward_reference(case)
    raw, P = f.raw, f.P
    r = BackwardRef()
    # save_mean / save_invstd of the test's choosing (float32 values, near raw's own so that xhat is O(1)): they need not come from a forward
    sd = torch.sqrt(f.stats["var"] + EPS)
    r.mean = (f.stats["save_mean"] + (case.bwd_mix[0].double() - 0.5) * 0.4 * sd).float()
    r.inv = ((0.7 + 0.6 * case.bwd_mix[1].double()) / sd).float()
    g = _ch(case.gamma) if affine else torch.ones(1, case.cout, 1, 1, dtype=torch.float64)
    b = _ch(case.beta) if affine else torch.zeros(1, case.cout, 1, 1, dtype=torch.float64)
    mu, iv, dy = _ch(r.mean), _ch(r.inv), case.dout.double()
    silu = act == ACT_SILU
    xh = (raw - mu) * iv
    z = xh * g + b
    dz = dy * silu_grad64(z) if silu else dy
    e_xh = 3 * U32 * ((raw * iv).abs() + (mu * iv).abs())
    e_z = g.abs() * e_xh + 2 * U32 * ((xh * g).abs() + b.abs())
    e_dz = dy.abs() * (0.5 * e_z + SILU_GRAD_F32 * (z.abs() + 1.0)) + U32 * dz.abs() if silu else torch.zeros_like(dz)
    t = dz * xh
    e_t = e_dz * (xh.abs() + e_xh) + dz.abs() * e_xh + U32 * t.abs()
    s = lambda v: v.sum((0, 2, 3))  # noqa: E731
    r.dbeta, r.dgamma = s(dz), s(t)
    r.dbeta_bound = gamma(P + 2) * s(dz.abs()) + s(e_dz)
    r.dgamma_bound = gamma(P + 2) * s(t.abs()) + s(e_t)
    r.xh, r.dz = xh, dz
    # the apply coefficients by common.h bn_coef_write, in float64 from the reference sums
    k1, k2 = _ch(r.dbeta) / P, _ch(r.dgamma) / P
    p0, p1 = iv, -mu * iv
    a0, a1 = p0 * g, p1 * g + b
    c0, c1, c2 = g * p0, g * p0 * p0 * k2, g * p0 * (k1 + p1 * k2)
    d = dz * c0 - (raw * c1 + c2)
    e_z4 = 4 * U32 * ((raw * a0).abs() + (p1 * g).abs() + b.abs())
    e_dz4 = dy.abs() * (0.5 * e_z4 + SILU_GRAD_F32 * (z.abs() + 1.0)) + U32 * dz.abs() if silu else torch.zeros_like(dz)
    # everything of e_d but the share of the sums the coefficients are made of (dw_bound adds it)
    r.e_d0 = e_dz4 * c0.abs() + dz.abs() * U32 * c0.abs() + raw.abs() * 5 * U32 * c1.abs() + 6 * U32 * (g * p0).abs() * (k1.abs() + (p1 * k2).abs()) \
        + 3 * U32 * ((dz * c0).abs() + (raw * c1).abs() + c2.abs())
    r.raw, r.g, r.p0, r.p1, r.P = raw, g, p0, p1, P
    r.d, r.dr = d, rne_bf16(d)
    r.dW = G.wgrad64(case.x, r.dr, (case.cout, case.c, 3, 3), 2)
    r.dW_mag = G.wgrad_mag(case.x, r.dr, (case.cout, case.c, 3, 3), 2)
    return r


def dw_bound(case, r, dev_b=None, dev_g=None):
    """-> (bound of dW per element, share of undecided pixels).  dev_b, dev_g: how far the sums the kernel made its coefficients of are
    from the reference dbeta / dgamma - the kernel's own outputs, when the caller has them (never more than their bounds), else the bounds."""
    db = r.dbeta_bound if dev_b is None else torch.minimum(dev_b.abs(), r.dbeta_bound)
    dg = r.dgamma_bound if dev_g is None else torch.minimum(dev_g.abs(), r.dgamma_bound)
    e_c1 = r.g.abs() * r.p0 * r.p0 * _ch(dg) / r.P
    e_c2 = (r.g * r.p0).abs() * (_ch(db) + r.p1.abs() * _ch(dg)) / r.P
    e_d = r.e_d0 + r.raw.abs() * e_c1 + e_c2
    undecided = (0.5 * ulp_bf16(r.d) - (r.d - r.dr).abs()) <= e_d
    wshape = (case.cout, case.c, 3, 3)
    bound = gamma(r.P + 8) * r.dW_mag + G.wgrad64(case.x.abs(), undecided.double() * ulp_bf16(r.d.abs() + e_d), wshape, 2)
    return bound, float(undecided.double().mean())


def check_backward(tag, got, case, act, affine=True):
    """got: any of dbeta, dgamma [co], dW [co, c, 3, 3] -> worst error / bound per stage"""
    r = backward_reference(case, act, affine)
    ratios, failures = {}, []
    dev = {k: got[k].detach().double().cpu() - ref for k, ref in (("dbeta", r.dbeta), ("dgamma", r.dgamma)) if k in got}
    dW_bound, ratios["undecided"] = dw_bound(case, r, dev.get("dbeta"), dev.get("dgamma"))
    for k, ref, bound in (("dbeta", r.dbeta, r.dbeta_bound), ("dgamma", r.dgamma, r.dgamma_bound), ("dW", r.dW, dW_bound)):
        if k in got:
            ratios[k] = _collect(failures, G.check_bound, f"{tag}: stage {k}", got[k], ref, bound + 1e-300)
    _raise(failures)
    return ratios


# ---- a float64 model of the kernels, with one planted fault at a time ---------------------------------------------------------------------------
FWD_FAULTS = ("tap_shift_corner", "halo_from_previous_image", "stats_drop_partial_group", "truncate", "bf16_accumulate", "biased_running_var", "stats_unrounded")
BWD_FAULTS = ("draw_f32", "dw_drop_pixel", "dgamma_unrounded_xhat")


def model_forward(case, act, fault=None):
    """the outputs of ymi_first_conv_bn_act_fwd as ideal arithmetic gives them (float64, the stored roundings applied), `fault` planted"""
    assert fault is None or fault in FWD_FAULTS
    x, w = case.x, case.ws
    n, ho, wo = case.n, case.geo["ho"], case.geo["wo"]
    conv = conv64(x, w)
    if fault == "tap_shift_corner":  # the centre tap of the last pixel of the last image reads the column to its left
        ih, iw = 2 * (ho - 1), 2 * (wo - 1)
        conv[n - 1, :, ho - 1, wo - 1] += (w[:, :, 1, 1] * (x[n - 1, :, ih, iw - 1] - x[n - 1, :, ih, iw])[None, :]).sum(1)
    if fault == "halo_from_previous_image":  # image 1's top halo row is image 0's last row, not zero
        conv[1, :, 0, :] += F.conv2d(x[0:1, :, case.h - 1 :, :], w[:, :, 0:1, :], stride=(1, 2), padding=(0, 1))[0, :, 0, :]
    if case.exact:
        raw = rne_bf16(conv)
    else:
        z32 = F.conv2d(x.float(), w.float(), stride=2, padding=1)  # a float32 accumulation of the 27 exact products
        raw = z32.to(BF).double()
        if fault == "truncate":
            raw = trunc_bf16(z32.double())
        if fault == "bf16_accumulate":
            acc = torch.zeros_like(z32).to(BF)
            xp = F.pad(x.float(), (1, 1, 1, 1))
            for kh in range(3):
                for kw in range(3):
                    for c in range(case.c):
                        acc = (acc.float() + xp[:, c : c + 1, kh : kh + 2 * ho : 2, kw : kw + 2 * wo : 2] * w[:, c, kh, kw].float().view(1, -1, 1, 1)).to(BF)
            raw = acc.double()
    sraw = conv if fault == "stats_unrounded" else raw  # what the statistics pass sums
    if fault == "stats_drop_partial_group":  # the last, partial 16-pixel group of every tile row is missing from the sums (not from the count)
        assert wo % 16 != 0
        sraw = sraw.clone()
        sraw[..., wo // 16 * 16 :] = 0.0
    P = case.geo["P"]
    s1, s2 = tile_sums(sraw), tile_sums(sraw * sraw)
    mean = s1.sum(0) / P
    var = (s2.sum(0) / P - mean * mean).clamp(min=0.0)
    unb = var if fault == "biased_running_var" or P == 1 else var * P / (P - 1.0)
    out = {"partials": torch.stack([s1, s2], 1), "save_mean": mean, "save_invstd": 1.0 / torch.sqrt(var + EPS), "running_mean": (1.0 - MOMENTUM) * case.rm0.double() + MOMENTUM * mean,
           "running_var": (1.0 - MOMENTUM) * case.rv0.double() + MOMENTUM * unb}
    scale = _ch(case.gamma) * _ch(out["save_invstd"])
    out["out"] = rne_bf16(act64(raw * scale + (_ch(case.beta) - _ch(mean) * scale), act))
    return out


def model_backward(case, act, affine=True, fault=None):
    assert fault is None or fault in BWD_FAULTS
    r = backward_reference(case, act, affine)
    f = forward_reference(case)
    dgamma = r.dgamma
    if fault == "dgamma_unrounded_xhat":
        dgamma = (r.dz * (f.conv - _ch(r.mean)) * _ch(r.inv)).sum((0, 2, 3))
    dr = r.d if fault == "draw_f32" else r.dr
    wshape = (case.cout, case.c, 3, 3)
    dW = G.wgrad64(case.x, dr, wshape, 2)
    if fault == "dw_drop_pixel":  # the largest term of dW[0, 0, 1, 1] is missing
        terms = case.x[:, 0, 0::2, 0::2] * dr[:, 0]
        dW = dW.clone()
        dW[0, 0, 1, 1] -= terms.reshape(-1)[terms.abs().reshape(-1).argmax()]
    return {"dbeta": r.dbeta, "dgamma": dgamma, "dW": dW}


# ---- case lists of the GPU tests ------------------------------------------------------------------------------------------------------------------
SHAPES = {"sub": (3, 8, 8), "one": (1, 16, 128), "2x2": (2, 18, 132), "3x2": (1, 34, 188), "5": (1, 16, 640), "1100": (1100, 2, 4)}
# (kind, shape, c, cout): every cout and every c with a multi-tile shape, every shape under Gate 1
CASES = [
    ("int", "sub", 1, 32), ("int", "one", 4, 64), ("int", "2x2", 3, 32), ("int", "2x2", 2, 48), ("int", "3x2", 3, 16), ("int", "3x2", 1, 64),
    ("int", "5", 4, 48), ("int", "5", 3, 64), ("int", "1100", 3, 16), ("int", "1100", 2, 32),
    ("dyadic", "sub", 3, 16), ("dyadic", "2x2", 3, 48), ("dyadic", "3x2", 2, 32),
    ("pos", "2x2", 3, 32), ("pos", "3x2", 4, 64), ("pos", "5", 1, 16), ("pos", "5", 2, 48),
]


def case_of(spec):
    kind, shape, c, cout = spec
    n, h, w = SHAPES[shape]
    return make_case(kind, n, c, h, w, cout)


def case_id(spec):
    kind, shape, c, cout = spec
    return f"{kind}-{'x'.join(map(str, SHAPES[shape]))}-c{c}-co{cout}"


# ---- ymi_bn_finalize on synthetic partial rows ---------------------------------------------------------------------------------------------------
FIN_BLOCKS = (1, 31, 32, 33, 96, 97, 128, 129, 400, 1024, 1025, 1088, 6400)
FIN_CHANNELS = (16, 48, 80)


def finalize_walk(blocks):
    """the row walks of ymi_bn_finalize restated -> the most main-loop trips and tail trips any thread makes in bn_finalize_kernel (32
    slices, four chains 32 rows apart, 128 rows per trip), the threads without a row, and the same for stat_rows_reduce_kernel (64 row
    groups x 4 slices, 16 x 64 rows per trip) when there are more than 16 * BN_STAGE_ROWS rows"""
    def walk(rows, starts, reach, trip, tail_step):
        main = tail = idle = 0
        for s0 in starts:
            b, m, t = s0, 0, 0
            while b + reach < rows:
                m, b = m + 1, b + trip
            while b < rows:
                t, b = t + 1, b + tail_step
            main, tail, idle = max(main, m), max(tail, t), idle + (m + t == 0)
        return {"main": main, "tail": tail, "idle": idle}

    R = BN_STAGE_ROWS
    staged = blocks > 16 * R
    out = {"staged": staged, "final": walk(R if staged else blocks, range(32), 96, 128, 32)}
    if staged:
        out["stage"] = walk(blocks, [g + R * sl for g in range(R) for sl in range(4)], 12 * R, 16 * R, 4 * R)
    return out


def finalize_rows(blocks, C):
    """[blocks, 2, C] float32: row sums in [-8, 8], row sums of squares in [64, 128], different by row and channel; count = 8 blocks"""
    b = torch.arange(blocks).view(-1, 1)
    c = torch.arange(C).view(1, -1)
    s1 = ((b * 7 + c * 3) % 17 - 8).float()
    s2 = (64 + (b * 5 + c * 11) % 65).float()
    rows = torch.stack([s1, s2], 1).contiguous()
    assert float(rows.abs().sum(0).max()) < G.F32_EXACT  # every float32 chain is exact
    return rows, 8 * blocks


def finalize_reference(rows, count, gam, bet, rm0, rv0, momentum=MOMENTUM, eps=EPS):
    s = rows.double().sum(0)
    mean = s[0] / count
    var = (s[1] / count - mean * mean).clamp(min=0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    scale = gam.double() * inv
    return {"scale": scale, "shift": bet.double() - mean * scale, "save_mean": mean, "save_invstd": inv, "var": var,
            "running_mean": (1.0 - momentum) * rm0.double() + momentum * mean, "running_var": (1.0 - momentum) * rv0.double() + momentum * var * count / (count - 1.0)}


def check_finalize(tag, got, ref, extra=None):
    SB, _ = project_bounds()
    for k, v in got.items():
        G.check_bound(f"{tag}: stage {k} [channel]", v, ref[k], SB * (ref[k].abs() + 1.0) + (extra[k] if extra and k in extra else 0.0))
