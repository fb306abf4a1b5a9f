"""Element-by-element checks of the fused SwinBlock MLP kernels (csrc/swin_mlp.hip: LayerNorm-2 + fc1 + GELU + fc2 + skip forward, and the
data path of the backward) against float64.

A helper module for the tests (not a conftest), in the shape of tests/attn_exact.py, whose report / check_exact / check_bound and LayerNorm
bound it reuses.  Notation: u = 2^-24 (float32 unit roundoff), r = 2^-8 (one RNE rounding to bfloat16), gamma_K = K u / (1 - K u), mag = the
expression of a stage on absolute values, ulp(v) = the bfloat16 spacing at v.  Everything here is device-agnostic torch.

Host mirrors, each restated from the source: Cfg (MlpCfg<C>: waves, workgroup tile, LDS tile, hidden cap), unit_of_row / unit_of_pos, the four
packed weight images of swin_mlp_pack_kernel (pack_images), the private pre-activation layout [tile of BM][chunk][wave][g][lane][8]
(decode_pre by view and permutation, encode_pre by the kernel's address arithmetic), and locators: a failing element is named as
(token, channel or hidden unit) with workgroup, wave, lane, and for a hidden unit its chunk, ring stage (chunk % 3), lane half, g (= fc2
k-step) and element; for a channel its accumulator tile and row, its fc1 k-step / lane half / element, and under Gate 1 the chunks that
feed it (the fc1 k-steps that feed a hidden unit).

Gate 1 (placement, bit for bit).  Operands for which every stored value is predictable exactly (gate1_operands):
  x[t] = m_t + s_tc a_t with s balanced +-1 (C/2 each), m_t a multiple of 1/8 in [-2, 2], a_t in {1/4, 1/2, 1, 3/2, 2, 3}: every partial sum of a
    row and of its squared deviations is exact in float32 (asserted), so mean = m_t, x - mean = +-a_t and xhat = +-1 / sqrt(1 + eps / a_t^2).
  gamma in {1, 2}, beta in {-3..3} with |beta| != gamma: the exact u is within gamma eps / (2 a^2) <= 1.6e-4 of a NONZERO integer |n| <= 5.  The
    kernel's float32 error on it: q / C + eps (2 roundings), rsqrtf (2 ulps), three products / sums -> <= 10 u (|xhat gamma| + |beta|); the
    distance of the float64 u from a bfloat16 rounding boundary is asserted to be >= 64 times that.
  w1: two nonzeros in {+-1, +-2} per hidden unit, b1 a multiple of 1/2 chosen so that all four sign combinations give a pre-activation that is
    a multiple of 1/2 in [-2, 16] (asserted on the float64 pre).  For every value in use, gelu64 and gelu'64 are asserted to lie >= MARGIN = 8
    times delta_gelu / delta_grad (below) from a bfloat16 rounding boundary, so the stored post and gelu' are the rounded float64 values.
  w2: two nonzeros of equal magnitude 1 or 2 per hidden unit (column), b2 a multiple of 1/4: every product post w2 is a multiple of the smallest
    ulp(post) in use, and every partial sum of an output element is exact in float32 when sum |post||w2| + |b2| + |x| < 2^24 ulp: asserted
    per element (NotExact otherwise: a case that is not exact fails loudly).
  dout in {0, +-1}: d_post = dout W2 is in {0, +-1, +-2, +-4} (asserted), a power of two commutes with the rounding of d_post gelu'(pre), and
    d_u's partial sums are exact under the same magnitude condition on sum |d_pre||w1| (asserted).
Expected u, pre, post, out, d_pre, d_u are the float64 results rounded once to bfloat16.

Gate 2 (precision, per element, real operands).  Each stage against float64 of that stage fed the kernel's own stored input:
  mean, rstd  1e-5 absolute / relative (the bounds of tests/test_gpu_swin_mlp_fused.py)
  u           attn_exact.ln_fwd_bounds: r |ref| + (1 + r)(float32 terms of the mean, the variance, rsqrtf and the affine map)
  pre         vs u_stored bf16(w1)^T + b1:      r |ref| + (1 + r) gamma_{C+1} mag
  post        vs gelu64(pre_stored):             r |ref| + (1 + r) delta_gelu(pre)
  out         vs bf16(gelu64(pre_stored)) bf16(w2)^T + b2 + x:
              r |ref| + (1 + r)(gamma_{hidden+2} mag + sum_j amb_j s_j |w2_cj|), amb_j = 1 where gelu64(pre_j) lies within delta_gelu of a
              rounding boundary; the kernel's post is then within s_j = delta_gelu + ulp(|gelu64| + delta_gelu) of the reference's (two values
              delta apart, each rounded by half an ulp), otherwise equal to it; the share of such units is asserted < 2 %
  d_pre       vs bf16(d_post64) gelu'64(pre_stored), d_post64 = dout bf16(w2): the float32 d_post is within e1 = gamma_C mag of d_post64, so its
              rounding is bf16(d_post64) or, where d_post64 is within e1 of a boundary (amb), within s = e1 + ulp(|d_post64| + e1) of it:
              r |ref| + (1 + r)(amb s |gelu'| + (|d_post| + amb s) delta_grad + 2u |ref|)
  d_u         vs d_pre_stored bf16(w1):          r |ref| + (1 + r) gamma_hidden mag

delta_gelu, delta_grad (errors of gelu_fast and of the backward's gelu' in float32, csrc/swin_mlp.hip).  With z = |x| / sqrt 2, t = 1 / (1 + p z),
gelu_fast(x) = max(x, 0) - |x| w, w = P(t) e, e = exp(-x^2 / 2), P the Abramowitz-Stegun 7.1.26 polynomial halved:
  * approximation: |erf error| <= 1.5e-7 (A-S 7.1.26), so 0.75e-7 on w = erfc / 2, absolute;
  * t: the folded constant and the fma round once each, v_rcp_f32 is 1 ulp = 2u (csrc/common.h) -> 4u relative.  t |P'(t)| = |dP/dz| (1 + p z) / p
    <= (1 / sqrt pi) / 0.3276 = 1.72 for the function P approximates (a degree-5 fit within 1e-7 has the same derivative to ~1e-5) -> 8u;
  * Horner: four fmas, partial results <= 0.73 -> 3u; the five float32 coefficients -> 2.24u; P t and (P t) e one rounding each of a value
    <= 0.5 -> 1u.  Together with t: 14.3u absolute on P, <= 16u taken;
  * e: the argument s^2 = (k |x|)^2 carries 5u relative (k, two products), i.e. 2.5u x^2 on e; v_exp_f32 is 1 ulp = 2u (common.h); a result
    below 2^-126 flushes to zero (< 1e-37 absolute).  On w <= e / 2: e (1 + 1.25 x^2) u;
  delta_w(x) = 0.75e-7 + exp(-x^2 / 2) (17 + 1.25 x^2) u
  delta_gelu(x) = |x| delta_w(x) + u |gelu(x)|                     (the last fma rounds once; v_max is exact)
  gelu'(x) = Phi(x) + x phi(x): Phi is w or 1 - w (one more rounding, <= u), x c e carries 2u (c, product) + the error of e, the fma rounds
  once (|gelu'| <= 1.13):  delta_grad(x) = delta_w(x) + |x phi(x)| (4 + 2.5 x^2) u + 2.2u
None of these is read off the kernel; no other tolerance in this module or its tests is a measured number.

emu_fwd / emu_bwd restate both kernels' rounding points in float32 torch (LayerNorm in float32; bfloat16 u, pre, post; float32 accumulation
chunk by chunk; one final rounding; the backward's bfloat16 d_post) and take planted faults for tests/test_host_swin_mlp_check.py.
"""
import collections
import math

import torch

import attn_exact as A

U32 = A.U32
R = A.R_BF16
gamma = A.gamma
BF = torch.bfloat16
WIDTHS = (128, 256, 384)
HC = 32  # hidden units per chunk
PAD = 256  # tokens the pre / post / d_pre buffers are padded to
LDS_MAX = 160 * 1024
STAT_BOUND = 1e-5  # mean (absolute) and rstd (relative)
MARGIN = 8.0  # Gate 1: gelu / gelu' of a value in use lies this many delta from a rounding boundary
MARGIN_LN = 64.0
AMB_SHARE = 0.02
PRE_LO, PRE_HI = -2.0, 16.0
DPOST_SET = (0.0, 1.0, 2.0, 4.0)


class NotExact(AssertionError):
    """a Gate 1 case whose construction does not make every stored value exact"""


# ---- mirrors of the kernels' bookkeeping -----------------------------------------------------------------------------------------------------
class Cfg:
    """MlpCfg<C> of csrc/swin_mlp.hip"""

    def __init__(self, c):
        assert c in WIDTHS, c
        self.c = c
        self.nw = 4 if c > 256 else 8  # waves per workgroup, 32 tokens each
        self.nt = 64 * self.nw
        self.bm = 32 * self.nw  # tokens per workgroup
        self.ks = c // 16  # k-steps of the rows form
        self.ct = c // 32  # accumulator tiles of a wave
        self.img = 32 * c * 2  # bytes of one chunk image
        self.stage = 2 * self.img
        self.store = self.nw * 32 * 2 * c  # output staging image
        self.lds_tile = max(3 * self.stage, self.store)
        self.hidden_max = min(8192, (LDS_MAX - self.lds_tile) // 4)


def cfg(c):
    return Cfg(c)


def supported(c, hidden):
    return c in WIDTHS and hidden % HC == 0 and HC <= hidden <= cfg(c).hidden_max


def pack_elems(c, hidden):
    return 4 * c * hidden


def pre_elems(tokens, hidden):
    return (tokens + PAD - 1) // PAD * PAD * hidden


def unit_of_row(rho):
    """hidden unit of the chunk in row rho of fc1's 32 x 32 result tile"""
    return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3)


def unit_of_pos(p):
    """hidden unit of the chunk at position p of fc2's k order (k-step p >> 4, lane half (p >> 3) & 1, element p & 7)"""
    return 16 * ((p >> 3) & 1) + 8 * (p >> 4) + (p & 7)


def pack_images(w1, w2):
    """w1 [hidden, C], w2 [C, hidden] float32 -> the four fragment-major bfloat16 images of swin_mlp_pack_kernel, [4 * hidden * C]"""
    hidden, c = w1.shape
    w1b, w2b = w1.to(BF), w2.to(BF)
    n = c * hidden
    i = torch.arange(n, device=w1.device)
    j, lane, blk = i & 7, (i >> 3) & 63, i >> 9
    ks = c // 16
    s, jc = blk % ks, blk // ks  # rows form
    hu = jc * 32 + unit_of_row(lane & 31)
    ch = 16 * s + 8 * (lane >> 5) + j
    img0, img2 = w1b[hu, ch], w2b[ch, hu]
    s, ct = blk & 1, (blk % ks) >> 1  # cols form
    ch = 32 * ct + (lane & 31)
    hu = jc * 32 + unit_of_pos(16 * s + 8 * (lane >> 5) + j)
    img1, img3 = w2b[ch, hu], w1b[hu, ch]
    return torch.cat([img0, img1, img2, img3])


def decode_pre(pre_priv, c, tokens, hidden):
    """private layout [tile of BM][chunk][wave][g][lane = 32 half + lane32][8] -> [tokens, hidden]: element e is hidden unit
    32 chunk + 16 half + 8 g + e of token BM tile + 32 wave + lane32"""
    k = cfg(c)
    tiles = (tokens + k.bm - 1) // k.bm
    v = pre_priv.reshape(-1)[: tiles * k.bm * hidden].view(tiles, hidden // HC, k.nw, 2, 2, 32, 8)
    return v.permute(0, 2, 5, 1, 4, 3, 6).reshape(tiles * k.bm, hidden)[:tokens]


def encode_pre(pre, c, fill=0.0):
    """[tokens, hidden] -> a buffer of pre_elems elements in the private layout, by the forward kernel's address arithmetic:
    offset = ((tile nch + chunk) NW + wave) 1024 + 512 g + 8 lane + e"""
    k = cfg(c)
    tokens, hidden = pre.shape
    nch = hidden // HC
    out = torch.full((pre_elems(tokens, hidden),), fill, dtype=pre.dtype, device=pre.device)
    t = torch.arange(tokens, device=pre.device).view(-1, 1)
    j = torch.arange(hidden, device=pre.device).view(1, -1)
    tile, wave, lane32 = t // k.bm, (t % k.bm) // 32, t % 32
    chunk, p = j // HC, j % HC
    half, g, e = p // 16, (p % 16) // 8, p % 8
    off = ((tile * nch + chunk) * k.nw + wave) * 1024 + 512 * g + 8 * (32 * half + lane32) + e
    out[off.reshape(-1)] = pre.reshape(-1)
    return out


def where_token(c, t):
    k = cfg(c)
    return f"wg {t // k.bm} wave {(t % k.bm) // 32} lane32 {t % 32}"


def where_unit(j):
    p = j % HC
    return f"chunk {j // HC} stage {(j // HC) % 3} half {p // 16} g {(p % 16) // 8} e {p % 8}"


def loc_hidden(c, w1=None, pre=None):
    """locator of a [T, hidden] element; with a sparse w1 the fc1 k-steps that feed the unit, with pre the stored pre-activation"""

    def f(idx):
        t, j = idx
        s = f"(token={t}, unit={j}) {where_token(c, t)} {where_unit(j)}"
        if w1 is not None:
            s += f" fc1 k-steps {sorted(set((torch.nonzero(w1[j]).view(-1) // 16).tolist()))}"
        if pre is not None:
            s += f" pre={float(pre[t, j])}"
        return s

    return f


def loc_channel(c, w2=None):
    """locator of a [T, C] element; with a sparse w2 the chunks (and ring stages) whose hidden units feed the channel"""

    def f(idx):
        t, ch = idx
        s = f"(token={t}, channel={ch}) {where_token(c, t)} acc tile {ch // 32} row {ch % 32} k-step {ch // 16} half {(ch % 16) // 8} e {ch % 8}"
        if w2 is not None:
            chunks = sorted(set((torch.nonzero(w2[ch]).view(-1) // HC).tolist()))
            s += f" fed by chunks {chunks} stages {sorted(set(x % 3 for x in chunks))}"
        return s

    return f


def loc_token(c):
    return lambda idx: f"(token={idx[0]}) {where_token(c, idx[0])}"


# ---- the case list of a width (tests/test_gpu_swin_mlp_exact.py runs it on the GPU, tests/test_host_swin_mlp_check.py on the emulation) -------------
Case = collections.namedtuple("Case", "t hidden strided gate1")


def case_list(c):
    """hidden: 1, 2, 3, 4, 7 chunks, the model's 4 C and the width's cap (T = 33 only); T: 1, 31, 33, BM, 2 BM, BM + 1, 421; the full hidden list at
    T = 33 and 421, the full T list at hidden = 96 and 4 C; three row-strided cases.  Every case runs Gate 2; every case runs Gate 1 as well:
    the magnitude condition holds at the caps too (gate1_expected asserts it)."""
    k = cfg(c)
    hs = [32, 64, 96, 128, 224, 4 * c]
    ts = [1, 31, 33, k.bm, 2 * k.bm, k.bm + 1, 421]
    cases = [(t, h, False) for t in (33, 421) for h in hs] + [(t, h, False) for h in (96, 4 * c) for t in ts]
    cases += [(33, k.hidden_max, False), (33, 96, True), (k.bm + 1, 96, True), (421, 4 * c, True)]
    seen, out = set(), []
    for cs in cases:
        if cs not in seen:
            seen.add(cs)
            out.append(Case(*cs, True))
    return out


def assert_coverage(c):
    """the case list of a width reaches every branch, and the Gate 1 operands of its cases put a nonzero weight on every channel of fc1's K axis
    (every k-step, lane half and element), on every row of fc2's / d_u's output, and on every hidden-unit position of a chunk in both products"""
    k = cfg(c)
    cases = case_list(c)
    chunks = {cs.hidden // HC for cs in cases}
    assert chunks >= {1, 2, 3, 4, 7, 4 * c // HC, k.hidden_max // HC}, chunks
    ts = {cs.t for cs in cases}
    assert 1 in ts and any(1 < t < 32 for t in ts) and any(t > 32 and t % 32 == 1 and t < k.bm for t in ts), ts
    assert {k.bm, 2 * k.bm, k.bm + 1} <= ts and any(t > k.bm and t % 32 > 1 for t in ts), ts
    assert {cs.strided for cs in cases} == {False, True}
    assert any(cs.hidden == k.hidden_max and cs.t == 33 for cs in cases)
    ch1 = torch.zeros(c, dtype=torch.bool)
    ch2 = torch.zeros(c, dtype=torch.bool)
    pos1 = torch.zeros(HC, dtype=torch.bool)
    pos2 = torch.zeros(HC, dtype=torch.bool)
    for cs in cases:
        if not cs.gate1:
            continue
        o = gate1_operands(c, min(cs.t, 2), cs.hidden)  # (the weights do not depend on T)
        ch1 |= (o["w1"] != 0).any(0)
        ch2 |= (o["w2"] != 0).any(1)
        pos1 |= (o["w1"] != 0).any(1).view(-1, HC).any(0)
        pos2 |= (o["w2"] != 0).any(0).view(-1, HC).any(0)
    assert bool(ch1.all()), f"fc1 K positions without a weight: {torch.nonzero(~ch1).view(-1).tolist()}"
    assert bool(ch2.all()), f"fc2 output rows without a weight: {torch.nonzero(~ch2).view(-1).tolist()}"
    assert bool(pos1.all()) and bool(pos2.all())


# ---- float64 pieces --------------------------------------------------------------------------------------------------------------------------
def bf(v):
    """one RNE rounding to bfloat16, as float64"""
    return v.to(BF).double()


def _exp2_of(v):
    """(exponent e with 2^e <= |v| < 2^(e+1), as float64 tensor); 0 -> a very small exponent"""
    _, ex = torch.frexp(v.double().abs().clamp(min=1e-300))
    return (ex - 1).double()


def bf16_ulp(v):
    return torch.exp2(_exp2_of(v) - 7)


def boundary_dist(v):
    """distance of |v| from the nearest midpoint of two adjacent bfloat16 values (float64); infinite at 0"""
    v = v.double().abs()
    ulp = bf16_ulp(v)
    frac = torch.remainder(v / ulp, 1.0)
    d = (frac - 0.5).abs() * ulp
    return torch.where(v == 0, torch.full_like(d, float("inf")), d)


def phi64(x):
    return torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)


def gelu64(x):
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * phi64(x)


def delta_w(x):
    return 0.75e-7 + torch.exp(-x * x / 2) * (17 + 1.25 * x * x) * U32


def delta_gelu(x):
    return x.abs() * delta_w(x) + U32 * gelu64(x).abs()


def delta_grad(x):
    return delta_w(x) + (x * phi64(x)).abs() * (4 + 2.5 * x * x) * U32 + 2.2 * U32


# ---- operands --------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(sum(int(v) * m for v, m in zip(key, (1000003, 10007, 101, 7, 1))) + 12345)
    return g


def _pick(values, shape, gen):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=gen)]


def gate1_operands(c, t, hidden):
    """Gate 1's operands (module docstring) as float32 host tensors; the weights depend on (c, hidden) only"""
    gw, gx = _gen(c, hidden, 1), _gen(c, hidden, 2, t)
    gam = _pick([1.0, 2.0], (c,), gw)
    beta = torch.randint(-3, 4, (c,), generator=gw).float()
    beta = torch.where(beta.abs() == gam, 3 * torch.sign(beta), beta)  # |beta| != gamma: u = +-gamma + beta is never 0
    assert bool((beta.abs() != gam).all()) and bool((beta.abs() <= 3).all())
    hu = torch.arange(hidden)
    # w1: channels perm[(h + off) % c] and perm[(h + off + roll) % c]: distinct, and every channel once hidden >= c
    perm = torch.randperm(c, generator=gw)
    off, roll = int(torch.randint(0, c, (1,), generator=gw)), int(torch.randint(1, c, (1,), generator=gw))
    ca, cb = perm[(hu + off) % c], perm[(hu + off + roll) % c]
    wa, wb = _pick([1.0, -1.0, 2.0, -2.0], (hidden,), gw), _pick([1.0, -1.0, 2.0, -2.0], (hidden,), gw)
    w1 = torch.zeros(hidden, c)
    w1[hu, ca], w1[hu, cb] = wa, wb
    spread = wa.abs() * gam[ca] + wb.abs() * gam[cb]  # <= 8
    lo, hi = PRE_LO + spread, PRE_HI - spread
    centre = lo + torch.floor(torch.rand(hidden, generator=gw) * ((hi - lo) * 2 + 1)) / 2
    b1 = centre - (wa * beta[ca] + wb * beta[cb])
    # w2: two channels per hidden unit, equal magnitude
    perm2 = torch.randperm(c, generator=gw)
    off2, roll2 = int(torch.randint(0, c, (1,), generator=gw)), int(torch.randint(1, c, (1,), generator=gw))
    cc, cd = perm2[(hu + off2) % c], perm2[(hu + off2 + roll2) % c]
    mg = _pick([1.0, 2.0], (hidden,), gw)
    w2 = torch.zeros(c, hidden)
    w2[cc, hu], w2[cd, hu] = mg * _pick([1.0, -1.0], (hidden,), gw), mg * _pick([1.0, -1.0], (hidden,), gw)
    b2 = torch.randint(-8, 9, (c,), generator=gw).float() / 4
    # tokens
    m = torch.randint(-16, 17, (t, 1), generator=gx).float() / 8
    a = _pick([0.25, 0.5, 1.0, 1.5, 2.0, 3.0], (t, 1), gx)
    sign = torch.where(torch.rand(t, c, generator=gx).argsort(1) < c // 2, 1.0, -1.0)
    x = m + sign * a
    dout = _pick([0.0, 1.0, -1.0], (t, c), gx)
    return dict(c=c, t=t, hidden=hidden, x=x, gamma=gam, beta=beta, eps=1e-5, w1=w1, b1=b1, w2=w2, b2=b2, dout=dout)


def real_operands(c, t, hidden, xscale=1.0, seed=0):
    """N(0, 1)-scaled operands, the distribution of tests/test_gpu_swin_mlp_widths.py::_case (at C = 256 that of test_gpu_swin_mlp_fused.py::_inputs)"""
    g = _gen(c, t, hidden, int(xscale * 16), seed)
    x = ((torch.randn(t, c, generator=g) * 1.5 + 0.3) * xscale).to(BF).float()
    gam = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.3
    w1 = torch.randn(hidden, c, generator=g) / c ** 0.5
    b1 = torch.randn(hidden, generator=g) * 0.2
    w2 = torch.randn(c, hidden, generator=g) / hidden ** 0.5
    b2 = torch.randn(c, generator=g) * 0.2
    dout = (torch.randn(t, c, generator=g) * 0.5).to(BF).float()
    return dict(c=c, t=t, hidden=hidden, x=x, gamma=gam, beta=beta, eps=1e-5, w1=w1, b1=b1, w2=w2, b2=b2, dout=dout)


def to_device(o, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in o.items()}


def eps32(o):
    """the float32 value the kernel adds"""
    return float(torch.tensor(o["eps"], dtype=torch.float32))


# ---- Gate 1 ------------------------------------------------------------------------------------------------------------------------------------
def _need(cond, msg):
    if not bool(cond):
        raise NotExact("Gate 1 construction: " + msg)


def _margins(values, f, delta):
    """min over the values of (distance of f(v) from a bfloat16 rounding boundary) / delta(v), and the value that attains it"""
    ratio = boundary_dist(f(values)) / delta(values)
    i = int(torch.argmin(ratio))
    return float(ratio[i]), float(values[i])


def gate1_expected(o):
    """-> dict u, pre, post, out, dpre, du (float64: the float64 results rounded once to bfloat16), mean, rstd.  Asserts every condition the
    construction rests on (NotExact)."""
    c, hidden = o["c"], o["hidden"]
    x, g, b = o["x"].double(), o["gamma"].double(), o["beta"].double()
    w1, b1, w2, b2, dout = o["w1"].double(), o["b1"].double(), o["w2"].double(), o["b2"].double(), o["dout"].double()
    for name in ("x", "w1", "w2", "dout"):
        _need((bf(o[name]) == o[name].double()).all(), f"{name} is not bfloat16-exact")
    # LayerNorm: sums exact in float32 in any order (every partial sum is a multiple of 2^-3 / 2^-6 below 2^24 of them)
    _need(x.abs().sum(1).max() * 8 < 2 ** 24 and (x * 8 == (x * 8).round()).all(), "row sums of x are not exact in float32")
    ref = A.ln_fwd_ref64(x, g, b, eps32(o))
    d = x - ref["mu"]
    _need((d.abs().amax(1) == d.abs().amin(1)).all() and (d * 8 == (d * 8).round()).all(), "x - mean is not +-a")
    _need((d * d).sum(1).max() * 64 < 2 ** 24, "the squared deviations do not sum exactly in float32")
    u64 = ref["out"]
    u = bf(u64)
    _need((u == u.round()).all() and (u != 0).all() and (u.abs() <= 5).all(), "u is not a small nonzero integer")
    f32err = 10 * U32 * ((ref["xhat"] * g).abs() + b.abs())
    mu_ = float((boundary_dist(u64) / f32err).min())
    _need(mu_ >= MARGIN_LN, f"u: margin {mu_:.1f} < {MARGIN_LN}")
    # fc1
    pre = u @ w1.t() + b1
    _need((pre * 2 == (pre * 2).round()).all() and pre.min() >= PRE_LO and pre.max() <= PRE_HI, f"pre not a multiple of 1/2 in [{PRE_LO}, {PRE_HI}]: "
          f"{float(pre.min())} .. {float(pre.max())}")
    vals = torch.unique(pre)
    mg, vg = _margins(vals, gelu64, delta_gelu)
    _need(mg >= MARGIN, f"gelu({vg}) lies {mg:.2f} delta_gelu from a rounding boundary (< {MARGIN})")
    md, vd = _margins(vals, gelu_grad64, delta_grad)
    _need(md >= MARGIN, f"gelu'({vd}) lies {md:.2f} delta_grad from a rounding boundary (< {MARGIN})")
    post = bf(gelu64(pre))
    # fc2 + bias + skip: exact partial sums
    step = float(bf16_ulp(post[post != 0]).min()) if bool((post != 0).any()) else 1.0
    _need((b2 / step == (b2 / step).round()).all() and (x / step == (x / step).round()).all(), "b2 / x are not multiples of the smallest post step")
    mag = post.abs() @ w2.abs().t() + b2.abs() + x.abs()
    _need(mag.max() < 2 ** 24 * step, f"out: sum |post||w2| + |b2| + |x| = {float(mag.max())} >= 2^24 * {step}")
    out = bf(post @ w2.t() + b2 + x)
    # backward
    dpost = dout @ w2
    _need(torch.isin(dpost.abs(), torch.tensor(DPOST_SET, dtype=torch.float64, device=dpost.device)).all(), "d_post outside {0, +-1, +-2, +-4}")
    grad = gelu_grad64(pre)
    dpre = bf(dpost * grad)
    _need((dpre == dpost * bf(grad)).all(), "d_post does not commute with the rounding")
    step2 = float(bf16_ulp(dpre[dpre != 0]).min()) if bool((dpre != 0).any()) else 1.0
    mag2 = dpre.abs() @ w1.abs()
    _need(mag2.max() < 2 ** 24 * step2, f"d_u: sum |d_pre||w1| = {float(mag2.max())} >= 2^24 * {step2}")
    du = bf(dpre @ w1)
    return dict(u=u, pre=pre, post=post, out=out, dpre=dpre, du=du, mean=ref["mu"].squeeze(1), rstd=ref["rstd"].squeeze(1),
                margins=dict(u=mu_, gelu=mg, grad=md))


def check_stats(what, got_mean, got_rstd, mean, rstd, c):
    e_mu = (got_mean.double() - mean).abs()
    e_rs = ((got_rstd.double() - rstd) / rstd).abs()
    for name, e, got, ref in (("mean", e_mu, got_mean, mean), ("rstd", e_rs, got_rstd, rstd)):
        bad = ~(e < STAT_BOUND)
        if bool(bad.any()):
            raise AssertionError(A.report(f"{what} {name} [1e-5]", got.double(), ref, bad, e, loc_token(c)))
    return float(e_mu.max()) / STAT_BOUND, float(e_rs.max()) / STAT_BOUND


def gate1_check(what, o, exp, got):
    """got: dict of [T, .] tensors (pre decoded).  Bit for bit; the statistics within the 1e-5 bounds."""
    c = o["c"]
    w1, w2 = o["w1"], o["w2"]
    check_stats(what, got["mean"], got["rstd"], exp["mean"], exp["rstd"], c)
    locs = dict(u=loc_channel(c), pre=loc_hidden(c, w1), post=loc_hidden(c, w1, exp["pre"]), out=loc_channel(c, w2), dpre=loc_hidden(c, None, exp["pre"]),
                du=loc_channel(c))
    for n, loc in locs.items():
        A.check_exact(f"{what} {n}", got[n], exp[n], loc)


# ---- Gate 2 ------------------------------------------------------------------------------------------------------------------------------------
def gate2_forward(what, o, got):
    """got: mean, rstd, u, pre (decoded), out of a training forward -> dict of worst error / bound per stage"""
    c, hidden = o["c"], o["hidden"]
    x, g, b = o["x"].double(), o["gamma"].double(), o["beta"].double()
    w1b, w2b, b1, b2 = bf(o["w1"]), bf(o["w2"]), o["b1"].double(), o["b2"].double()
    ratios = {}
    ref = A.ln_fwd_ref64(x, g, b, eps32(o))
    ratios["mean"], ratios["rstd"] = check_stats(what, got["mean"], got["rstd"], ref["mu"].squeeze(1), ref["rstd"].squeeze(1), c)
    ratios["u"] = A.check_bound(f"{what} u", got["u"], ref["out"], A.ln_fwd_bounds(x, g, b, eps32(o), ref, BF)["out"], loc_channel(c))
    us = got["u"].double()
    rpre = us @ w1b.t() + b1
    mag = us.abs() @ w1b.abs().t() + b1.abs()
    ratios["pre"] = A.check_bound(f"{what} pre", got["pre"], rpre, R * rpre.abs() + (1 + R) * gamma(c + 1) * mag, loc_hidden(c))
    ps = got["pre"].double()
    p64 = gelu64(ps)
    post = bf(p64)
    amb = boundary_dist(p64) <= delta_gelu(ps)  # (else the float32 gelu lies in the same rounding cell: the kernel's post IS bf16(gelu64))
    share = float(amb.double().mean())
    assert share < AMB_SHARE, f"{what}: {share:.3%} of the hidden units lie within delta_gelu of a rounding boundary"
    rout = post @ w2b.t() + b2 + x
    mag = post.abs() @ w2b.abs().t() + b2.abs() + x.abs()
    dg = delta_gelu(ps)
    slack = (amb.double() * (dg + bf16_ulp(p64.abs() + dg))) @ w2b.abs().t()
    ratios["out"] = A.check_bound(f"{what} out", got["out"], rout, R * rout.abs() + (1 + R) * (gamma(hidden + 2) * mag + slack), loc_channel(c))
    ratios["amb"] = share
    return ratios


def gate2_backward(what, o, pre_stored, got):
    """got: post, dpre, du of the backward run on the stored pre-activations pre_stored [T, hidden]"""
    c, hidden = o["c"], o["hidden"]
    w1b, w2b, dout = bf(o["w1"]), bf(o["w2"]), o["dout"].double()
    ps = pre_stored.double()
    ratios = {}
    p64 = gelu64(ps)
    ratios["post"] = A.check_bound(f"{what} post", got["post"], p64, R * p64.abs() + (1 + R) * delta_gelu(ps), loc_hidden(c, None, ps))
    d64 = dout @ w2b
    e1 = gamma(c) * (dout.abs() @ w2b.abs())
    dpb = bf(d64)
    step = (boundary_dist(d64) <= e1).double() * (e1 + bf16_ulp(d64.abs() + e1))
    g64 = gelu_grad64(ps)
    ref = dpb * g64
    bound = R * ref.abs() + (1 + R) * (step * g64.abs() + (dpb.abs() + step) * delta_grad(ps) + 2 * U32 * ref.abs())
    ratios["dpre"] = A.check_bound(f"{what} dpre", got["dpre"], ref, bound, loc_hidden(c, None, ps))
    ds = got["dpre"].double()
    rdu = ds @ w1b
    ratios["du"] = A.check_bound(f"{what} du", got["du"], rdu, R * rdu.abs() + (1 + R) * gamma(hidden) * (ds.abs() @ w1b.abs()), loc_channel(c))
    return ratios


def fmt_ratios(r):
    return " ".join(f"{k} {v:.3f}" for k, v in r.items())


# ---- float32 emulation of the kernels' rounding points, with planted faults ----------------------------------------------------------------
def _st(v):
    return v.to(BF).float()


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _trunc_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emu_gelu_fast(x, grad_sign_fault=False):
    """gelu_fast and the backward's gelu' operation by operation in float32 -> (gelu, gelu')"""
    x = x.float()
    ax = x.abs()
    t = 1.0 / _fma(_f32(0.3275911) * _f32(0.70710678118654752440), ax, _f32(1.0))
    s = ax * _f32(0.84932180028801904272)
    e = torch.exp2(-(s * s))
    p = _f32(0.5) * _f32(1.061405429)
    for coef in (-1.453152027, 1.421413741, -0.284496736, 0.254829592):
        p = _fma(p, t, _f32(0.5 if coef > 0 else -0.5) * _f32(abs(coef)))
    w = p * t * e
    gelu = _fma(-ax, w, torch.clamp(x, min=0.0))
    phi = torch.where(x >= 0, 1.0 - w, w)
    xc = x * _f32(0.39894228040143267794)
    if grad_sign_fault:
        xc = torch.where(x < 0, -xc, xc)
    return gelu, _fma(xc, e, phi)


def emu_fwd(o, fault=None):
    """-> dict mean, rstd, u, pre [T, hidden], post, out (float32 holding the stored values).  fault: None or a tuple (name, parameters...):
    out_trunc | double_round | acc_bf16_per_chunk | (b1_missing, unit) | (b2_missing, first channel of 4, last token) | tanh_gelu |
    (swap_units, j1, j2) | (drop_last_kstep, chunk) | (stale_stage, chunk) | skip_clamped | (tile_chunk_missing, tile, chunk)"""
    name = fault[0] if fault else None
    c, hidden, t = o["c"], o["hidden"], o["x"].shape[0]
    x = o["x"].float()
    inv_c = _f32(1.0) / _f32(float(c))
    mu = x.sum(1, keepdim=True) * inv_c
    d = x - mu
    rs = torch.rsqrt((d * d).sum(1, keepdim=True) * inv_c + _f32(o["eps"]))
    u = _st(d * rs * o["gamma"].float() + o["beta"].float())
    w1b, w2b = _st(o["w1"]), _st(o["w2"])
    b1 = o["b1"].float().clone()
    if name == "b1_missing":
        b1[fault[1]] = 0.0
    pre32 = u @ w1b.t() + b1
    if name == "drop_last_kstep":
        sl = slice(HC * fault[1], HC * fault[1] + HC)
        pre32[:, sl] = u[:, : c - 16] @ w1b[sl, : c - 16].t() + b1[sl]
    pre = _st(pre32)
    if name == "tanh_gelu":
        post = _st(0.5 * pre * (1.0 + torch.tanh(0.7978845608028654 * (pre + 0.044715 * pre * pre * pre))))
    else:
        post = _st(emu_gelu_fast(pre)[0])
    acc = torch.zeros(t, c)
    for jc in range(hidden // HC):
        sl = slice(HC * jc, HC * jc + HC)
        ws = w2b[:, sl]
        if name == "stale_stage" and jc == fault[1]:
            ws = w2b[:, HC * (jc - 3) : HC * (jc - 3) + HC]
        if name == "swap_units" and jc == fault[1] // HC:
            ws = ws.clone()
            a, b = fault[1] % HC, fault[2] % HC
            ws[:, [a, b]] = ws[:, [b, a]]
        part = post[:, sl] @ ws.t()
        if name == "tile_chunk_missing" and jc == fault[2]:
            part[:, 32 * fault[1] : 32 * fault[1] + 32] = 0.0
        acc = acc + part
        if name == "acc_bf16_per_chunk":
            acc = _st(acc)
    skip = x.clone()
    if name == "skip_clamped":
        skip[t - 1] = x[t - 2]
    b2 = o["b2"].float()
    if name == "double_round":
        out = _st(_st(acc + b2) + skip)
    else:
        v = acc + b2
        if name == "b2_missing":
            v[t - 1, fault[1] : fault[1] + 4] = acc[t - 1, fault[1] : fault[1] + 4]
        v = v + skip
        out = _trunc_bf16(v) if name == "out_trunc" else _st(v)
    return dict(mean=mu.squeeze(1), rstd=rs.squeeze(1), u=u, pre=pre, post=post, out=out)


def emu_bwd(o, pre, fault=None):
    """-> dict post, dpre, du from the stored pre-activations.  fault: dpost_unrounded | grad_sign | tanh_gelu (post only)"""
    name = fault[0] if fault else None
    c, hidden, t = o["c"], o["hidden"], o["x"].shape[0]
    w1b, w2b = _st(o["w1"]), _st(o["w2"])
    d1 = o["dout"].float() @ w2b
    gelu, grad = emu_gelu_fast(pre, grad_sign_fault=name == "grad_sign")
    if name == "tanh_gelu":
        gelu = 0.5 * pre * (1.0 + torch.tanh(0.7978845608028654 * (pre + 0.044715 * pre * pre * pre)))
    dpre = _st((d1 if name == "dpost_unrounded" else _st(d1)) * grad)
    acc = torch.zeros(t, c)
    for jc in range(hidden // HC):
        sl = slice(HC * jc, HC * jc + HC)
        acc = acc + dpre[:, sl] @ w1b[sl]
    return dict(post=_st(gelu), dpre=dpre, du=_st(acc))
