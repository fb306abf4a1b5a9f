"""Element-by-element checks of the Swin kernels (csrc/swin.hip: window attention forward / backward, LayerNorm with the window
gather and its backward) against float64 references.

A helper module for the tests (not a conftest); it mirrors tests/gemm_exact.py.  Notation as there: u = 2^-24 (float32 unit
roundoff), r = 2^-8 (one RNE rounding to bfloat16) or u (float32 storage), gamma_k = k u / (1 - k u), sc = 1 / sqrt(hd).  Tensors of
one attention launch are handled per (window, head) as [windows, heads, L, hd]; everything here is device-agnostic torch.

Dispatch mirror (swin.hip ymi_window_attention_fwd / _bwd, ymi_layernorm_fwd): `attn_form` names the attention kernel that runs
('tr' = bfloat16 one-tile with transposed LDS reads, 'onetile-f32', 'tiled' = flash-style 64 x 64 tiles) and
`stage_width` the tr staging width; `ln_form` names the LayerNorm kernel ('half' = bfloat16 half-wave, or 'G1'..'G4').

Gate 1 (placement): one-hot attention.  All inputs are bfloat16-exact integers.  Per (window, head) every query m gets a target key
pi(m); K[j, d] = c s_d b_{d mod nb}(j) (+-1 code of j, nb = ceil(log2 L)) for d < hd - 1 and K[j, hd - 1] = c; Q[m] = K[pi(m)] on the
code dims and Q[m, hd - 1] = -c hd; c = 16, s a random sign per dimension, V and dO +-1.  The selected raw score is -c^2 = -2^8 (its
scaled value is exact in float32 for every scale, with or without a fused multiply-add), a zero padding key scores 0 and would take
the weight, and every other real key trails by 2 c^2 floor((hd - 1) / nb) sc >= 128 after scaling, where float32 exp is exactly 0.
So O = V[pi(m)], dV[j] = sum over {m: pi(m) = j} of dO[m], dQ = dK = 0 bit for bit, and lse = fl(-c^2 * fl(1 / sqrt(hd))) (2 float32 ulps
allowed).  `onehot_check` refuses a case whose float64 scores do not give a scaled gap >= 110 and -(selected) sc >= 16.

Gate 2 (precision): a per-element float64 bound on real operands.  Per query m
    e_mj = sc gamma_hd sum_d |q_md||k_jd| + 2u |s_mj|        (float32 score; the scaling rounds once)      E_m = max_j e_mj
    R_m  = max_j (max score - s_mj)
    delta_m = 2 E_m + 4u (1 + R_m)                             (relative error of exp(s - max): argument error 2E, __expf's own)
    kappa_m = 2 delta_m + gamma_L + 2u                         (numerator and denominator, the L-term sum, 1/l and the product)
    |dO_md| <= r |O_md| + (1 + r)(r_P + kappa_m) sum_j p_mj |v_jd|       r_P: rounding of the stored P (2^-8 in bfloat16, u in f32)
    |d dV_jd| <= r |dV_jd| + (1 + r) sum_m (r_P + kappa_m) p_mj |dO_md|
    e_dP = gamma_hd sum_d |dO||V|
    e_Delta: tr recomputes Delta = sum_j P dP in float32: sum_j p (kappa |dP| + e_dP) + gamma_L sum_j p |dP|;
             the one-tile float32 and the tiled forms take Delta = dO . O_stored: sum_d |dO| bound_O + gamma_hd sum_d |dO||O|
    e_dS = r |dS| + sc p (kappa |dP - Delta| + e_dP + e_Delta) + 2u |dS|         (dS = sc p (dP - Delta), stored in the dtype)
    |d dQ| <= r |dQ| + (1 + r)(sum_j e_dS |K| + gamma_L sum_j |dS||K|), dK likewise with Q.
The saved log-sum-exp: |d lse_m| <= E_m + (delta_m + gamma_L)(1 + 2 (delta_m + gamma_L)) + 4u (1 + |lse_m| + log L)
(the maximum's error, log of the sum's relative error, __logf and the final addition).

LayerNorm forward: float32 mean and variance sums of C terms, rsqrtf within 2 ulp (4u), one rounding to the dtype:
    e_mu = gamma_{C+1} sum|x| / C;   e_var = (gamma_{C+3} (C var + C e_mu^2) + C e_mu^2) / C + 2u (var + eps + .);
    rho = x/2 + x^2 + 4u with x = e_var / (var + eps) (relative error of rstd);
    |d out| <= r |out| + (1 + r)(1 + 8u)(|g| (rstd e_mu + |x - mu| rstd rho + 2u |xhat|) + 2u |xhat g| + u |b|)
    (1 + 8u: the products of two first-order errors).  The backward reference is float64 built from the kernel's own saved mean /
rstd (teacher-forced), so each direction counts only its own roundings; dgamma / dbeta count the additions along the kernel's tree:
tokens per wave, the four-wave LDS sum (3), chan_reduce_final's per-thread chain (ceil(blocks / 128) + 3) and its double combination
and final rounding (2).

The float32 P V (and P^T dO) accumulation has no gamma_L term of its own in these formulas: in bfloat16 it is at most 2^-8 of the r_P
term (L <= 256), and in float32 the emulated and measured ratios stay below 0.1.

Worst ratio error / bound of the CPU emulations of each form's rounding points (tests/test_host_attn_check.py: fixed seeds, N(0, 1)
operands and a x3 q / k variant, L 16..196, hd 4..192), as O / lse / dV / dQ / dK:
    tr bf16      0.723 / 0.078 / 0.809 / 0.763 / 0.860
    one-tile f32 0.032 / 0.071 / 0.047 / 0.018 / 0.022
    tiled bf16   0.732 / 0.078 / 0.809 / 0.329 / 0.525
    tiled f32    0.031 / 0.071 / 0.047 / 0.021 / 0.023
LayerNorm, as out / mean / rstd / dx / dgamma / dbeta:  bf16 0.995 / 0.031 / 0.165 / 0.994 / 0.061 / 0.016;
f32 0.206 / 0.257 / 0.209 / 0.221 / 0.064 / 0.048.  (The bfloat16 out and dx reach 0.99 where the one rounding to bfloat16 is close to
half an ulp: that term alone is r |ref|.)

Failures name the number of bad elements and the worst five as (window, head, token-in-window, column) or (n, h, w, c) with the
kernel form, as gemm_exact.report does.
"""
import math

import torch

U32 = 2.0 ** -24
R_BF16 = 2.0 ** -8
LDS_MAX = 160 * 1024
C1HOT = 16  # Gate 1's code amplitude: the selected raw score is -C1HOT^2 = -2^8


def unit(dtype):
    return R_BF16 if dtype == torch.bfloat16 else U32


def gamma(k):
    ku = k * U32
    assert ku < 0.5, k
    return ku / (1.0 - ku)


def f32_scale(hd):
    """the kernels' 1.0f / sqrtf((float)hd) (both operations correctly rounded in float32)."""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd), dtype=torch.float32)))


# ---- dispatch mirrors ------------------------------------------------------------------------------------------------------------------
def attn_lds(L, hd, bf16, bwd):
    """-> (lds of the generic one-tile kernels, lds of the tr kernels), restated independently of swin.hip's attn_one_tile_lds / attn_tr_lds."""
    hdp = (hd + 31) // 32 * 32
    es, pad = (2, 8) if bf16 else (4, 4)
    rs, ts = (hdp + pad) * es, (64 + pad) * es
    gsz = max(64 * rs, hdp * ts)
    lds = 2 * gsz + (3 if bwd else 1) * 64 * ts + (64 * 4 if bwd else 0)
    lds_tr = (4 if bwd else 3) * 64 * (hdp + 8) * 2 + (2 if bwd else 1) * 64 * (64 + 8) * 2
    return lds, lds_tr


def attn_form(L, hd, dtype, tiled_opt=0, bwd=False):
    """swin.hip attn_form: the LDS size plays no part (every one-tile image fits: static_asserts there, attn_lds here)."""
    if L > 64 or tiled_opt:
        return "tiled"
    return "tr" if dtype == torch.bfloat16 else "onetile-f32"


def stage_width(hd, srcs):
    """tr staging (attn_stage_rows): 16-byte chunks when hd % 8 == 0 and every source (data_ptr, ld) is 16-byte aligned with ld % 8 == 0
    (the head / section offsets are then multiples of 8 elements too); 8-byte chunks otherwise."""
    wide = hd % 8 == 0 and all(ld % 8 == 0 and p % 16 == 0 for p, ld in srcs)
    return 16 if wide else 8


def ln_form(C, dtype, x_ld, out_ld, ptrs):
    """ymi_layernorm_fwd: the half-wave bfloat16 kernel or the one-wave kernel with G = ceil(C / 256) channel groups."""
    half = dtype == torch.bfloat16 and C <= 256 and C % 8 == 0 and x_ld % 8 == 0 and out_ld % 8 == 0 and all(p % 16 == 0 for p in ptrs)
    return "half" if half else f"G{min(4, max(1, (C + 255) // 256))}"


def ln_bwd_blocks(T):
    return int(max(1, min(2048, (T + 31) // 32)))


def ln_tree_adds(T):
    """additions along the longest path of the dgamma / dbeta sums: tokens per wave, the four-wave LDS sum, chan_reduce_final's chain
    per thread (stride 128 plus the stride-32 remainder), its double combination and the rounding to float."""
    b = ln_bwd_blocks(T)
    tpw = (T + 4 * b - 1) // (4 * b)
    return tpw + 3 + (b + 127) // 128 + 3 + 2


# ---- layout ------------------------------------------------------------------------------------------------------------------------------
def heads_view(x, L, heads):
    """[T, heads * hd] token rows (windows of L consecutive tokens) -> [windows, heads, L, hd]."""
    T, C = x.shape
    return x.reshape(T // L, L, heads, C // heads).permute(0, 2, 1, 3)


def tokens_view(x):
    """inverse of heads_view: [windows, heads, L, hd] -> [T, heads * hd]."""
    nw, H, L, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(nw * L, H * hd)


def split_qkv(qkv, L, heads):
    C = qkv.shape[1] // 3
    return [heads_view(qkv[:, i * C : (i + 1) * C], L, heads) for i in range(3)]


def window_tokens(img, ws):
    """NHWC image [n, h, w, C] -> [T, C] token rows in window order (zeros for the padding at the bottom and right, swin_block.py:41-50)
    and the token -> pixel map (n, h, w), -1 for padding."""
    n, h, w, C = img.shape
    hp, wp = (h + ws - 1) // ws * ws, (w + ws - 1) // ws * ws
    pad = torch.zeros((n, hp, wp, C), dtype=img.dtype, device=img.device)
    pad[:, :h, :w] = img
    idx = torch.full((n, hp, wp), -1, dtype=torch.int64, device=img.device)
    idx[:, :h, :w] = torch.arange(n * h * w, device=img.device).view(n, h, w)

    def order(t):
        s = t.shape[3:] if t.dim() > 3 else ()
        return t.reshape(n, hp // ws, ws, wp // ws, ws, *s).permute(0, 1, 3, 2, 4, *range(5, 5 + len(s))).reshape(n * hp * wp, *s)

    return order(pad), order(idx)


# ---- float64 references ----------------------------------------------------------------------------------------------------------------
def attn_ref64(q, k, v, dout=None):
    """float64 attention per (window, head) on [windows, heads, L, hd] operands (the dtype's values)."""
    q, k, v = q.double(), k.double(), v.double()
    sc = 1.0 / math.sqrt(q.shape[-1])
    S = q @ k.transpose(-1, -2)
    s = S * sc
    mx = s.amax(-1, keepdim=True)
    e = torch.exp(s - mx)
    l = e.sum(-1, keepdim=True)
    P = e / l
    r = {"s": s, "P": P, "O": P @ v, "lse": (mx + torch.log(l)).squeeze(-1), "sc": sc}
    if dout is not None:
        dO = dout.double()
        dP = dO @ v.transpose(-1, -2)
        Dl = (P * dP).sum(-1, keepdim=True)
        dS = sc * P * (dP - Dl)  # the scale folded in, as the kernels store it
        r.update(dP=dP, Delta=Dl.squeeze(-1), dS=dS, dQ=dS @ k, dK=dS.transpose(-1, -2) @ q, dV=P.transpose(-1, -2) @ dO)
    return r


def attn_bounds(q, k, v, dout, ref, dtype, form):
    """Gate 2 bounds (module docstring) for O, lse and, with dout, dQ / dK / dV of kernel form `form`."""
    q, k, v = q.double(), k.double(), v.double()
    u, r = U32, unit(dtype)
    rP = unit(dtype)
    L, hd = q.shape[-2], q.shape[-1]
    sc, s, P = ref["sc"], ref["s"], ref["P"]
    absS = q.abs() @ k.abs().transpose(-1, -2)
    E = (sc * gamma(hd) * absS + 2 * u * s.abs()).amax(-1)
    R = (s.amax(-1, keepdim=True) - s).amax(-1)
    delta = 2 * E + 4 * u * (1 + R)
    kappa = 2 * delta + gamma(L) + 2 * u
    b = {}
    Pv = P @ v.abs()
    b["O"] = r * ref["O"].abs() + (1 + r) * (rP + kappa).unsqueeze(-1) * Pv
    dl = delta + gamma(L)
    b["lse"] = E + dl * (1 + 2 * dl) + 4 * u * (1 + ref["lse"].abs() + math.log(max(L, 1)))
    if dout is None:
        return b
    dO = dout.double()
    dP, Dl, dS = ref["dP"], ref["Delta"].unsqueeze(-1), ref["dS"]
    b["dV"] = r * ref["dV"].abs() + (1 + r) * (P * (rP + kappa).unsqueeze(-1)).transpose(-1, -2) @ dO.abs()
    e_dP = gamma(hd) * (dO.abs() @ v.abs().transpose(-1, -2))
    if form == "tr":
        e_D = (P * (kappa.unsqueeze(-1) * dP.abs() + e_dP)).sum(-1, keepdim=True) + gamma(L) * (P * dP.abs()).sum(-1, keepdim=True)
    else:
        e_D = (dO.abs() * b["O"]).sum(-1, keepdim=True) + gamma(hd) * (dO.abs() * ref["O"].abs()).sum(-1, keepdim=True)
    e_dS = r * dS.abs() + sc * P * (kappa.unsqueeze(-1) * (dP - Dl).abs() + e_dP + e_D) + 2 * u * dS.abs()
    b["dQ"] = r * ref["dQ"].abs() + (1 + r) * (e_dS @ k.abs() + gamma(L) * dS.abs() @ k.abs())
    b["dK"] = r * ref["dK"].abs() + (1 + r) * (e_dS.transpose(-1, -2) @ q.abs() + gamma(L) * dS.abs().transpose(-1, -2) @ q.abs())
    return b


def ln_fwd_ref64(x, g, b, eps):
    """x: [T, C] token rows (padding rows zero), g / b: float32 parameters, eps: the float32 value the kernel adds."""
    x, g, b = x.double(), g.double(), b.double()
    C = x.shape[1]
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mu) * rstd
    return {"mu": mu, "var": var, "rstd": rstd, "xhat": xhat, "out": xhat * g + b, "C": C}


def ln_fwd_bounds(x, g, b, eps, ref, dtype):
    u, r = U32, unit(dtype)
    x, g, b = x.double(), g.double(), b.double()
    C = ref["C"]
    mu, var, rstd, xhat = ref["mu"], ref["var"], ref["rstd"], ref["xhat"]
    e_mu = gamma(C + 1) * x.abs().sum(1, keepdim=True) / C
    e_q = gamma(C + 3) * (C * var + C * e_mu ** 2) + C * e_mu ** 2
    ve = var + eps
    e_ve = e_q / C + 2 * u * (ve + e_q / C)
    xr = e_ve / ve
    rho = 0.5 * xr + xr ** 2 + 4 * u
    e_out = (g.abs() * (rstd * e_mu + (x - mu).abs() * rstd * rho + 2 * u * xhat.abs()) + 2 * u * (xhat * g).abs() + u * b.abs()) * (1 + 8 * u)
    return {"mu": e_mu.squeeze(1), "rstd": (rho * rstd).squeeze(1), "out": r * ref["out"].abs() + (1 + r) * e_out}


def ln_bwd_ref64(x, dy, g, mu_k, rstd_k, add=None):
    """teacher-forced float64 backward from the kernel's saved statistics.  x, dy: [T, C] token rows; add: [T, C] addend or None."""
    x, dy, g = x.double(), dy.double(), g.double()
    mu, rs = mu_k.double().view(-1, 1), rstd_k.double().view(-1, 1)
    C = x.shape[1]
    xh = (x - mu) * rs
    gd = g * dy
    s1 = gd.mean(1, keepdim=True)
    s2 = (gd * xh).mean(1, keepdim=True)
    inner = gd - s1 - xh * s2
    dx = rs * inner + (add.double() if add is not None else 0.0)
    return {"xh": xh, "gd": gd, "s1": s1, "s2": s2, "inner": inner, "rs": rs, "dx": dx, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0), "C": C}


def ln_bwd_bounds(dy, ref, dtype, add=None):
    u, r = U32, unit(dtype)
    C, T = ref["C"], dy.shape[0]
    dy = dy.double()
    xh, gd, s1, s2, inner, rs = ref["xh"], ref["gd"], ref["s1"], ref["s2"], ref["inner"], ref["rs"]
    e_s1 = gamma(C + 2) * gd.abs().sum(1, keepdim=True) / C
    e_s2 = gamma(C + 5) * (gd * xh).abs().sum(1, keepdim=True) / C
    A = gd.abs() + s1.abs() + (xh * s2).abs()
    e_in = e_s1 + xh.abs() * e_s2 + 2 * u * (xh * s2).abs() + 4 * u * A
    e_dx = (rs * e_in + u * rs * inner.abs() + u * ref["dx"].abs()) * (1 + 8 * u)
    k = ln_tree_adds(T)
    return {
        "dx": r * ref["dx"].abs() + (1 + r) * e_dx,
        "dgamma": gamma(k + 3) * (dy * xh).abs().sum(0) + 1e-300,
        "dbeta": gamma(k) * dy.abs().sum(0) + 1e-300,
    }


# ---- Gate 1: one-hot attention --------------------------------------------------------------------------------------------------------
def code_bits(L):
    return max(1, math.ceil(math.log2(L))) if L > 1 else 1


def onehot_ok(L, hd):
    return hd - 1 >= code_bits(L)


def onehot_operands(nw, heads, L, hd, gen):
    """-> q, k, v, dout [nw, heads, L, hd] (float32 host, bfloat16-exact integers) and the targets pi [nw, heads, L]."""
    assert onehot_ok(L, hd), (L, hd)
    nb, c = code_bits(L), float(C1HOT)
    j = torch.arange(L).view(L, 1)
    d = torch.arange(hd - 1).view(1, hd - 1)
    bits = (((j >> (d % nb)) & 1) * 2 - 1).float()  # [L, hd - 1]
    sign = torch.randint(0, 2, (nw, heads, 1, hd - 1), generator=gen).float() * 2 - 1
    k = torch.empty(nw, heads, L, hd)
    k[..., : hd - 1] = c * sign * bits
    k[..., hd - 1] = c
    pi = torch.randint(0, L, (nw, heads, L), generator=gen)
    q = torch.gather(k, 2, pi.unsqueeze(-1).expand(nw, heads, L, hd)).clone()
    q[..., hd - 1] = -c * hd
    v = torch.randint(0, 2, (nw, heads, L, hd), generator=gen).float() * 2 - 1
    dout = torch.randint(0, 2, (nw, heads, L, hd), generator=gen).float() * 2 - 1
    return q, k, v, dout, pi


def onehot_check(q, k, pi, what=""):
    """refuse a case that is not one-hot: scaled gap >= 110 and -(selected score) * scale >= 16, from the float64 scores."""
    q, k = q.double(), k.double()
    L, hd = q.shape[-2], q.shape[-1]
    s = (q @ k.transpose(-1, -2)) / math.sqrt(hd)
    sel = torch.gather(s, -1, pi.to(s.device).unsqueeze(-1)).squeeze(-1)
    assert bool((-sel >= 16).all()), f"{what}: not a one-hot case: -(selected score) * scale {float((-sel).min())} < 16"
    if L > 1:
        oth = s.scatter(-1, pi.to(s.device).unsqueeze(-1), float("-inf")).amax(-1)
        gap = float((sel - oth).min())
        assert gap >= 110, f"{what}: not a one-hot case: scaled gap {gap} < 110"


def onehot_expected(q, k, v, dout, dtype):
    """Gate 1's expected values: the float64 results rounded to the storage dtype (float64 keeps residues like e^-512) and lse."""
    ref = attn_ref64(q, k, v, dout)
    out = {n: ref[n].to(dtype).double() for n in ("O", "dV", "dQ", "dK")}
    hd = q.shape[-1]
    out["lse"] = torch.full(ref["lse"].shape, float(torch.tensor(-float(C1HOT ** 2), dtype=torch.float32) * torch.tensor(f32_scale(hd), dtype=torch.float32)),
                            dtype=torch.float64, device=q.device)
    return out


def f32_ulp(x):
    """float32 ulp of |x| (float64 tensor)."""
    a = x.abs().float().clamp(min=2.0 ** -126)
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


# ---- reports and checks ------------------------------------------------------------------------------------------------------------------
ATTN_AXES = ("window", "head", "token", "col")


def locate_attn(form):
    return lambda idx: "(" + ", ".join(f"{n}={i}" for n, i in zip(ATTN_AXES, idx)) + f") form {form}"


def locate_tokens(pix_map, hw, form):
    """[T, C] token rows: (n, h, w, c) of the token's pixel (padding tokens named so), with the kernel form."""
    h, w = hw

    def f(idx):
        t, c = idx[0], idx[-1]
        p = int(pix_map[t]) if pix_map is not None else -2
        if p == -2:
            return f"(token={t}, c={c}) form {form}"
        if p < 0:
            return f"(token={t} padding, c={c}) form {form}"
        return f"(n={p // (h * w)}, h={p // w % h}, w={p % w}, c={c}) form {form}"

    return f


def report(what, got, ref, bad, err, locate=None, limit=5):
    cnt = int(bad.sum())
    flat = torch.where(bad.reshape(-1), err.reshape(-1).nan_to_num(float("inf")), torch.full_like(err.reshape(-1), -1.0))
    order = torch.argsort(flat, descending=True)[: min(limit, cnt)]
    lines = [f"{what}: {cnt} of {bad.numel()} elements wrong; worst:"]
    g, r = got.reshape(-1), ref.reshape(-1)
    for o in order.tolist():
        idx = [int(i) for i in torch.unravel_index(torch.tensor(o), tuple(bad.shape))]
        loc = locate(idx) if locate else str(tuple(idx))
        lines.append(f"  {loc}: got {float(g[o])!r} expected {float(r[o])!r}")
    return "\n".join(lines)


def check_exact(what, got, expected, locate=None):
    g = got.double()
    assert g.shape == expected.shape, (what, tuple(g.shape), tuple(expected.shape))
    bad = ~(g == expected)
    if bool(bad.any()):
        raise AssertionError(report(what + " [Gate 1, exact]", g, expected, bad, (g - expected).abs(), locate))


def check_bound(what, got, ref, bound, locate=None):
    """per-element |got - ref| <= bound (NaN fails) -> worst err / bound."""
    g = got.double()
    assert g.shape == ref.shape, (what, tuple(g.shape), tuple(ref.shape))
    err = (g - ref).abs()
    bad = ~(err <= bound)
    ratio = err / bound.clamp(min=1e-300)
    if bool(bad.any()):
        raise AssertionError(report(what + " [Gate 2, float64 bound]", g, ref, bad, ratio, locate))
    return float(ratio.max()) if err.numel() else 0.0


def check_attn(what, got, ref, bounds, form, names):
    """Gate 2 over the named attention outputs (dict of [windows, heads, L(, hd)] tensors) -> worst ratio."""
    return max(check_bound(f"{what} {n}", got[n], ref[n], bounds[n], locate_attn(form)) for n in names)


def check_onehot(what, got, exp, form, names):
    for n in names:
        if n == "lse":
            err = (got["lse"].double() - exp["lse"]).abs()
            tol = 2 * f32_ulp(exp["lse"])
            bad = ~(err <= tol)
            if bool(bad.any()):
                raise AssertionError(report(f"{what} lse [Gate 1, 2 float32 ulps]", got["lse"].double(), exp["lse"], bad, err, locate_attn(form)))
        else:
            check_exact(f"{what} {n}", got[n], exp[n], locate_attn(form))


def rel(a, b):
    """the suite's tensor-wide relative-L2 gate."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


# ---- CPU emulation of the kernels' rounding points (float32 torch; used by tests/test_host_attn_check.py) ---------------------------
def _st(x, dtype):
    return x.to(dtype).float()


def emu_attn_fwd(form, q, k, v, dtype, scale=None, unmask=None):
    """-> (O stored, lse) of kernel form `form` on [windows, heads, L, hd] float32 operands.  `scale` overrides 1/sqrt(hd) (a planted
    fault); `unmask` = (window, head) includes one zero padding key in that block (a planted fault)."""
    q, k, v = q.float(), k.float(), v.float()
    sc = f32_scale(q.shape[-1]) if scale is None else scale
    if unmask is not None:
        w, h = unmask
        zk = torch.zeros_like(k[:, :, :1])
        O, lse = emu_attn_fwd(form, q, torch.cat([k, zk], 2), torch.cat([v, zk], 2), dtype, scale)
        Ob, lseb = emu_attn_fwd(form, q, k, v, dtype, scale)
        Ob[w, h], lseb[w, h] = O[w, h], lse[w, h]
        return Ob, lseb
    if form != "tiled":
        s = (q @ k.transpose(-1, -2)) * sc
        mx = s.amax(-1, keepdim=True)
        e = torch.exp(s - mx)
        l = e.sum(-1, keepdim=True)
        p = _st(e * (1.0 / l), dtype)
        return _st(p @ v, dtype), (mx + torch.log(l)).squeeze(-1)
    L = k.shape[2]
    m_run = torch.full(q.shape[:-1] + (1,), float("-inf"))
    l_run = torch.zeros_like(m_run)
    o = torch.zeros(q.shape)
    for k0 in range(0, L, 64):
        s = (q @ k[:, :, k0 : k0 + 64].transpose(-1, -2)) * sc
        m_new = torch.maximum(m_run, s.amax(-1, keepdim=True))
        alpha = torch.exp(m_run - m_new)
        e = torch.exp(s - m_new)
        l_run = l_run * alpha + e.sum(-1, keepdim=True)
        o = o * alpha + _st(e, dtype) @ v[:, :, k0 : k0 + 64]
        m_run = m_new
    return _st(o * (1.0 / l_run), dtype), (m_run + torch.log(l_run)).squeeze(-1)


def emu_attn_bwd(form, q, k, v, o_st, dout, lse, dtype):
    """-> dict dQ, dK, dV (stored) of kernel form `form`: P recomputed from lse; Delta from P dP (tr) or dO . O_stored."""
    q, k, v, dO = q.float(), k.float(), v.float(), dout.float()
    sc = f32_scale(q.shape[-1])
    s = q @ k.transpose(-1, -2)
    dP = dO @ v.transpose(-1, -2)
    p = torch.exp(s * sc - lse.unsqueeze(-1))
    Dl = (p * dP).sum(-1, keepdim=True) if form == "tr" else (dO * o_st.float()).sum(-1, keepdim=True)
    ds = p * (dP - Dl) * sc
    P, dS = _st(p, dtype), _st(ds, dtype)
    return {"dV": _st(P.transpose(-1, -2) @ dO, dtype), "dK": _st(dS.transpose(-1, -2) @ q, dtype), "dQ": _st(dS @ k, dtype)}


def emu_ln_fwd(x, g, b, eps, dtype, var_div=None):
    """-> (out stored, mean, rstd) in float32.  var_div overrides C as the variance divisor (a planted fault)."""
    x = x.float()
    C = x.shape[1]
    mu = x.sum(1, keepdim=True) / C
    q = ((x - mu) * (x - mu)).sum(1, keepdim=True)
    rs = torch.rsqrt(q / float(var_div or C) + eps)
    return _st((x - mu) * rs * g.float() + b.float(), dtype), mu.squeeze(1), rs.squeeze(1)


def emu_ln_param_sum(terms):
    """float32 dgamma / dbeta along the kernel's tree: per-wave token chains, four-wave LDS sum, chan_reduce_final (4 chains of stride
    128 per thread plus the stride-32 remainder, then double)."""
    T, C = terms.shape
    b = ln_bwd_blocks(T)
    nwv = 4 * b
    tpw = (T + nwv - 1) // nwv
    padded = torch.zeros(tpw * nwv, C)
    padded[:T] = terms.float()
    waves = torch.zeros(nwv, C)
    for i in range(tpw):
        waves = waves + padded[i * nwv : (i + 1) * nwv]
    w4 = waves.view(b, 4, C)
    part = ((w4[:, 0] + w4[:, 1]) + w4[:, 2]) + w4[:, 3]
    out = torch.zeros(C, dtype=torch.float64)
    for sl in range(32):
        acc = [torch.zeros(C) for _ in range(4)]
        bb = sl
        while bb + 96 < b:
            for i in range(4):
                acc[i] = acc[i] + part[bb + 32 * i]
            bb += 128
        while bb < b:
            acc[0] = acc[0] + part[bb]
            bb += 32
        out = out + ((acc[0].double() + acc[1].double()) + (acc[2].double() + acc[3].double()))
    return out.float()


def emu_ln_bwd(x, dy, g, mu, rs, dtype, add=None, drop_padding_dbeta=None):
    """-> (dx stored, dgamma, dbeta) in float32.  drop_padding_dbeta: boolean [T] of tokens left out of dbeta (a planted fault)."""
    x, d, g = x.float(), dy.float(), g.float()
    C = x.shape[1]
    xh = (x - mu.view(-1, 1)) * rs.view(-1, 1)
    gd = g * d
    s1 = gd.sum(1, keepdim=True) / C
    s2 = (gd * xh).sum(1, keepdim=True) / C
    dx = rs.view(-1, 1) * (gd - s1 - xh * s2) + (add.float() if add is not None else 0.0)
    db_terms = d if drop_padding_dbeta is None else d * (~drop_padding_dbeta).float().view(-1, 1)
    return _st(dx, dtype), emu_ln_param_sum(d * xh), emu_ln_param_sum(db_terms)
