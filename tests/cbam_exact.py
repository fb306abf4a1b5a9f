"""Element-by-element checks of the CBAM kernels (csrc/cbam.hip): device-agnostic torch, shared by tests/test_host_cbam_check.py (CPU:
the checks against a float32 emulation of the kernels and against planted faults) and tests/test_gpu_cbam_exact.py (the kernels).

Layout here: x, out, dout, dx [N, H, W, C]; pooled [N, 2, C] (avg, max); pool_argmax, ca [N, C]; smap [N, H, W, 2] (mean, max);
smap_argmax, sa [N, H, W]; w1 [Hd, C]; w2 [C, Hd]; wsa [2, K, K].  References are float64 and take the dtype's VALUES.

The forward hands back every intermediate, so every kernel is checked on its own, "teacher-forced": a stage's reference is computed in
float64 from the KERNEL's outputs of the stage before, so a stage answers for its own roundings only.  The backward is computed from the
kernel's saved tensors and indices, so the float64 backward routes exactly as the kernel did.

Exact checks (bit equality, no tolerance)
  pooled[:, 1]      = max over pixels of x
  pool_argmax       = the FIRST pixel h * W + w that attains it
  smap[..., 1]      = max over c of the float32 product fl(x * ca), ca the kernel's own (one correctly rounded multiply: torch float32)
  smap_argmax       = the FIRST channel that attains it

Bounds (every other output):  |got - ref| <= r |ref| + gamma_k A
  u = 2^-24; r = 2^-8 for an output stored as bfloat16, u for float32; gamma_k = k u / (1 - k u);
  A = the float64 expression of ref with every operand and intermediate replaced by its absolute value (1 - s becomes 1 + s), so no
      cancellation is counted;
  k = the depth of the output in float32 operations: inputs 0, a + b -> max(ka, kb) + 1, a * b -> ka + kb + 1 (the relative errors of
      both factors multiply), a division (correctly rounded) + 1.  A sum that starts at 0.f counts that first addition too.  An fma
      that -ffp-contract=fast forms only removes a rounding.
  Where the output is rounded to bfloat16 AFTER the float32 arithmetic, E = gamma_k A is the error before the store and the bound is
  r |ref| + (1 + r) E  (|rd(v) - v| <= r |v| <= r (|ref| + E)).
  sigmoidf_ = v_rcp_f32(1 + v_exp_f32(-z * log2 e)), each "~1 ulp" = 2u relative (common.h).  Relative error of the result: the
  rounded constant and the multiply move the exponent by 2u |z| log2 e, i.e. e^-z by 2u |z| relatively; exp2 2u; the addition u;
  rcp 2u; d sigma / sigma = -(1 - sigma) de / e.  With one unit for the second-order terms: (6 + 2|z|) u sigma.  The argument's own
  error passes through sigma' <= 1/4.  So for a sigmoid output A = Az / 4 with z's k, plus (6 + 2|z|) u |ref|.

k per output, T = ceil(C / 256), PB = cbam_pb(HW), Pw = ceil(HW / (4 PB)), with the loop or line each term comes from:
  pooled[:, 0]  ceil(HW / 16) + 17     cbam_pool_kernel: `sum[r] += v` per pixel lane (pool_pixel, both pixel loops), 16 x `s += s_sum[q]`, `s / HW`
  ca            z: ceil(C / 64) + Hd + 9   cbam_mlp_kernel: (hidden_unit) `w * sp[c]` 1, `acc_a +=` ceil(C / 64), wave_sum 6, (relu_sum) fmaxf + fmaxf 1,
                                           `wr[h] * hs[h]` 1, `z +=` Hd; then sigmoidf_
  smap[..., 0]  4T + 8                 cbam_stats_kernel: `v * cap` 1, `s += t` 4T, wave_sum 6, `s / C` 1
  sa            u: 9                   cbam_apply_kernel: `wsa * smap` 1, the inner `+` 1, `u +=` 1 (K * K <= 64: one tap a lane),
                                       wave_sum 6; then sigmoidf_
  out           2                      `v * cap * sa`, then the store rounds to the dtype
  du            k_du = 4T + 11         cbam_bwd_du_kernel: `d * v * cap` 2, `s +=` 4T, wave_sum 6, `s * a` 1, `* (1 - a)` 2
  dx1           k_du + 11              cbam_bwd_dx_kernel: `g * wsa` 1, `d0 +=` 1, wave_sum 6, `d0 / C` 1, the two `+` of dx1 2
  dx, 1st part  k_du + 12              `dx1 * cap`; a bfloat16 dx is ROUNDED HERE (first store) ...
  dcap          k_du + 12 + Pw + 3     `dx1 * v` 1, `acc +=` Pw, `part[0] + .. + part[3]` 3
  dz            k_dz = k_du + 18 + Pw + PB   cbam_bwd_mlp_kernel: `s += dcap` PB, `s * a` 1, `* (1 - a)` 2
  hsum          k_hs = ceil(C / 64) + 8  (hidden_unit) `w * sp` 1, `acc_a +=` ceil(C / 64), wave_sum 6, (relu_sum) fmaxf + fmaxf 1
  dh            k_dh = k_dz + ceil(C / 64) + 7   `w2 * sdz` 1, `g +=` ceil(C / 64), wave_sum 6
  dpool         k_dp = k_dh + 1 + Hd   `dh * w` 1, `da +=` Hd
  dw2           k_dz + k_hs + 1 + N    cbam_bwd_w_kernel: `dz * hsum` (two computed factors), `s +=` N
  dw1           k_dh + 2 + N           `dpre * pooled` 1, the inner `+` 1, `s +=` N
  dwsa          k_du + 24 + ceil(ceil(NP / 1024) / 2)   cbam_bwd_wsa_kernel: `du * smap` 1, the longer of the two chains, `s0 + s1` 1,
                                       wave_sum 6, 16 x `tot += red[q]`
The backward's intermediates lie in the workspace (`workspace_layout`), so each of its kernels is ALSO checked on its own, teacher-forced
like the forward (the nested |.| of the end-to-end A above counts the cancellation inside du and dz again in everything after them):
  du, dcap, dz, hsum, dpre, dpool as stages; dwsa.from_du (k = 24 + ceil(ceil(NP / 1024) / 2)) from the kernel's du; dw1.from_ws,
  dw2.from_ws from the kernel's dz, hsum, dpre; dx.from_ws from the kernel's du and dpool (stages_from_workspace lists the k).
  dx            k_dp + 4               cbam_bwd_pool_kernel: `1.f / HW` 1, `da * inv` 1, `+ dm` 1, `v +=` 1; ... and a bfloat16 dx is
                                       ROUNDED A SECOND TIME by this kernel's store: the kernel reads back the rounded first part, so
                                       E = gamma_k A + r A_first (1 + gamma), A_first the |.| expression of dx1 * ca.
The ReLU gates of the backward are decided by the reference's own float64 signs of W1 avg and W1 max; `gate_margin` (|pre| over its
rounding bound) must be > 1 on every case the tests use, so a float32 rounding cannot flip one (test_host_cbam_check asserts it).

Worst error / bound over the cases of the tests (tests/test_host_cbam_check.py prints the first, tests/test_gpu_cbam_exact.py the second):
  output         emulation f32  bf16   kernels (MI355X) f32  bf16
  pooled.avg         0.093      0.024          0.093         0.024
  ca                 0.031      0.042          0.037         0.026
  smap.mean          0.056      0.066          0.072         0.058
  sa                 0.182      0.182          0.168         0.168
  out                0.660      0.996          0.656         0.996
  dx                 0.025      0.788          0.017         0.788
  dw1                0.000      0.000          0.000         0.000
  dw2                0.001      0.001          0.001         0.001
  dwsa               0.020      0.013          0.020         0.013
  du                 0.055      0.033          0.055         0.031
  dwsa.from_du       0.044      0.041          0.034         0.048
  dcap               0.091      0.097          0.100         0.089
  dz                 0.315      0.356          0.341         0.334
  hsum               0.050      0.040          0.050         0.040
  dpre               0.070      0.079          0.160         0.086
  dpool              0.258      0.291          0.213         0.278
  dw2.from_ws        0.473      0.475          0.483         0.474
  dw1.from_ws        0.434      0.440          0.447         0.492
  dx.from_ws         0.257      0.983          0.206         0.983
out in bfloat16 reaches 0.996 because r |ref| IS the half ulp where the mantissa is 1.0; the end-to-end dw1 / dw2 bounds are loose by the
nested |.| (the workspace stages are the sharp ones).  bfloat16 dx: about a tenth of the elements lie OUTSIDE the bound a single rounding
would give (where dx1 * ca and the pool term cancel, by up to 1e3 times it) and inside the two-rounding bound: the second rounding is
real and at those elements it dominates.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
BF, F32 = torch.bfloat16, torch.float32
LOG2E = 1.44269504088896340736

# (N, C, H, W, Hd, K): what each reaches is asserted through `branches` (test_cases_reach_the_branches_they_claim)
CASES = [
    (1, 4, 1, 1, 1, 3),
    (3, 36, 3, 5, 4, 7),
    (2, 64, 9, 7, 8, 7),
    (1, 260, 8, 9, 17, 3),
    (9, 128, 6, 6, 16, 7),
    (3, 320, 30, 25, 20, 7),
    (2, 1024, 48, 44, 64, 7),
]


def unit(dtype):
    return 2.0 ** -8 if dtype == BF else U


def gamma(k):
    return k * U / (1.0 - k * U)


def cdiv(a, b):
    return -(-a // b)


# ---- dispatch mirror (csrc/cbam.hip: cbam_pb, ymi_cbam_bwd_workspace, the launch lines of ymi_cbam_fwd / ymi_cbam_bwd) ---------------------
def cbam_pb(HW):
    return max(1, min(64, (HW + 31) // 32))


def workspace_layout(N, H, W, C, Hd):
    """-> ({name: (first float, floats)}, floats used): the carve-up, every sub-buffer on a 4-float boundary."""
    PB = cbam_pb(H * W)
    off, lay = 0, {}
    for name, cnt in (("du", N * H * W), ("dcap", N * PB * C), ("dz", N * C), ("hsum", N * Hd), ("dpre", 2 * N * Hd), ("dpool", 2 * N * C)):
        lay[name] = (off, cnt)
        off += (cnt + 3) // 4 * 4
    return lay, off


def workspace_bytes(N, H, W, C, Hd):
    """the size formula: the six sub-buffers, 4 floats of slack for each boundary, 256 bytes for the base alignment."""
    PB = cbam_pb(H * W)
    return (N * H * W + N * PB * C + N * C + 3 * N * Hd + 2 * N * C + 6 * 4) * 4 + 256


def pool_grid(N, C):
    return (cdiv(C, 64), N)


def pixel_grid(NP):
    return cdiv(NP, 4)


def ge_blocks(NP, C):
    return min(4096, cdiv(NP * (C // 4), 256))


def branches(case):
    """which branches of the kernels a case reaches, from the shapes alone."""
    N, C, H, W, Hd, K = case
    HW, NP = H * W, N * H * W
    trips = [cdiv(NP - t, 1024) for t in range(min(NP, 1024))]  # per thread of cbam_bwd_wsa_kernel
    return {
        "wsa_main_loop": NP > 1024,
        "wsa_tail": any(t % 2 for t in trips),
        "wsa_main_and_tail": NP > 1024 and any(t % 2 for t in trips),
        "pb": cbam_pb(HW),
        "pb_capped": (HW + 31) // 32 > 64,
        "acc_slots": cdiv(C, 256),
        "second_trip_lanes": max(0, cdiv(C - 256, 4)) if C > 256 else 0,  # lanes of a wave with a second 256-channel trip
        "bwd_pool_grid_stride": NP * (C // 4) > ge_blocks(NP, C) * 256,
        "pool_overhang": C % 64 != 0,
        "pool_idle_pixel_lanes": HW < 16,
        "pool_four_in_flight_lanes": max(0, min(16, HW - 48)),  # pixel lanes whose first trip is the four-in-flight loop
        "w_unroll_tail": N > 8 and N % 8 != 0,
        "ksa": K,
        "map_below_stencil": H < K or W < K,
        "hidden_above_waves": Hd > 16,
        "np_not_multiple_of_4": NP % 4 != 0,
    }


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def make_inputs(case, dtype, seed=0, ties=False):
    """x, dout N(0, 1) rounded to the dtype (as float64 values); w1, w2, wsa float32 values; wsa random, hence asymmetric.
    ties: x on 8 levels and w2 = 0 (ca = 0.5 everywhere): every maximum is tied many times."""
    N, C, H, W, Hd, K = case
    g = torch.Generator().manual_seed(1000 * seed + N * 7 + C * 13 + H * 17 + W + (5 if ties else 0))
    if ties:
        x = (torch.randint(0, 8, (N, H, W, C), generator=g).float() - 4.0) * 0.25 + 0.125
    else:
        x = torch.randn((N, H, W, C), generator=g)
    dout = torch.randn((N, H, W, C), generator=g)
    w1 = torch.randn((Hd, C), generator=g) / math.sqrt(C)
    w2 = torch.randn((C, Hd), generator=g) / math.sqrt(Hd)
    if ties:
        w2 = torch.zeros_like(w2)
    wsa = torch.randn((2, K, K), generator=g) * 0.2
    return {"x": x.to(dtype).double(), "dout": dout.to(dtype).double(), "w1": w1.double(), "w2": w2.double(), "wsa": wsa.double()}


# ---- float64 restatement ----------------------------------------------------------------------------------------------------------------
def first_argmax(v, dim):
    """index of the FIRST element along dim that attains the maximum."""
    m = v.amax(dim, keepdim=True)
    shape = [1] * v.dim()
    shape[dim] = v.shape[dim]
    idx = torch.arange(v.shape[dim], device=v.device).view(shape)
    return torch.where(v == m, idx, v.shape[dim]).amin(dim)


def last_argmax(v, dim):
    m = v.amax(dim, keepdim=True)
    shape = [1] * v.dim()
    shape[dim] = v.shape[dim]
    idx = torch.arange(v.shape[dim], device=v.device).view(shape)
    return torch.where(v == m, idx, -1).amax(dim)


def corr(s, w):
    """zero-padded cross-correlation of s [N, Cin, H, W] with w [Cout, Cin, K, K] -> [N, Cout, H, W] (unfold + einsum: float64 on any device)."""
    N, _, H, W = s.shape
    K = w.shape[-1]
    return torch.einsum("nkp,ok->nop", F.unfold(s, K, padding=K // 2), w.reshape(w.shape[0], -1)).view(N, w.shape[0], H, W)


def ref_forward(x, w1, w2, wsa, pool_argmax=None, smap_argmax=None):
    """float64 CBAM forward.  With the two index tensors given, both maxima are READ THROUGH gather at those indices, so autograd over
    this function (and ref_backward) routes exactly as the indices say; without them the first-index rule decides."""
    N, H, W, C = x.shape
    K = wsa.shape[-1]
    xf = x.reshape(N, H * W, C)
    if pool_argmax is None:
        pool_argmax = first_argmax(xf.detach(), 1)
    pooled = torch.stack([xf.mean(1), xf.gather(1, pool_argmax[:, None, :])[:, 0]], 1)
    hs = torch.relu(pooled[:, 0] @ w1.T) + torch.relu(pooled[:, 1] @ w1.T)
    ca = torch.sigmoid(hs @ w2.T)
    x1 = x * ca[:, None, None, :]
    if smap_argmax is None:
        smap_argmax = first_argmax(x1.detach(), 3)
    smap = torch.stack([x1.mean(3), x1.gather(3, smap_argmax[..., None])[..., 0]], 3)
    sa = torch.sigmoid(corr(smap.permute(0, 3, 1, 2), wsa[None])[:, 0])
    return {"pooled": pooled, "pool_argmax": pool_argmax, "ca": ca, "smap": smap, "smap_argmax": smap_argmax, "sa": sa, "out": x1 * sa[..., None]}


def _sig_bound(ref, z, Az, kz):
    return U * ref.abs() + gamma(kz) * Az / 4 + (6 + 2 * z.abs()) * U * ref.abs()


def stage_avg(x):
    N, H, W, C = x.shape
    HW = H * W
    ref, A = x.sum((1, 2)) / HW, x.abs().sum((1, 2)) / HW
    return ref, U * ref.abs() + gamma(cdiv(HW, 16) + 17) * A


def stage_ca(pooled, w1, w2):
    C, Hd = w2.shape
    a, m = pooled[:, 0] @ w1.T, pooled[:, 1] @ w1.T
    Ah = pooled[:, 0].abs() @ w1.abs().T + pooled[:, 1].abs() @ w1.abs().T
    z = (torch.relu(a) + torch.relu(m)) @ w2.T
    ref = torch.sigmoid(z)
    return ref, _sig_bound(ref, z, Ah @ w2.abs().T, cdiv(C, 64) + Hd + 9)


def stage_smean(x, ca):
    C = x.shape[-1]
    t = x * ca[:, None, None, :]
    ref, A = t.sum(3) / C, t.abs().sum(3) / C
    return ref, U * ref.abs() + gamma(4 * cdiv(C, 256) + 8) * A


def stage_smax(x, ca):
    """exact: float32 products on the CPU, maximum, first index."""
    t = x.float().cpu() * ca.float().cpu()[:, None, None, :]
    return t.amax(3), first_argmax(t, 3)


def stage_sa(smap, wsa):
    K = wsa.shape[-1]
    s = smap.permute(0, 3, 1, 2)
    z, Az = corr(s, wsa[None])[:, 0], corr(s.abs(), wsa.abs()[None])[:, 0]
    ref = torch.sigmoid(z)
    return ref, _sig_bound(ref, z, Az, 9)


def stage_out(x, ca, sa, dtype):
    ref = x * ca[:, None, None, :] * sa[..., None]
    r = unit(dtype)
    return ref, r * ref.abs() + (1 + r) * gamma(2) * ref.abs()


def stage_dwsa(du, smap, K):
    """B5 from the kernel's own du (workspace): dwsa[j][t] = sum_p du[p] smap[p + off_t][j]."""
    N, H, W = du.shape
    unf = F.unfold(smap.permute(0, 3, 1, 2), K, padding=K // 2)
    ref = torch.einsum("nkp,np->k", unf, du.reshape(N, H * W)).view(2, K, K)
    A = torch.einsum("nkp,np->k", unf.abs(), du.abs().reshape(N, H * W)).view(2, K, K)
    return ref, U * ref.abs() + gamma(24 + cdiv(cdiv(N * H * W, 1024), 2)) * A


def stages_from_workspace(inp, saved, ws, dtype):
    """B2 .. B6 teacher-forced: each from the kernels' own workspace tensors of the stage before (float64) -> {stage: (ref, bound)}.
    k: dcap 15 + Pw (`g * wsa` 1, `d0 +=` 1, wave_sum 6, `/ C` 1, dx1 2, `dx1 * v` 1, `acc +=` Pw, part 3); dz PB + 3; hsum ceil(C/64) + 8;
    dpre ceil(C/64) + 7; dpool 1 + Hd; dw2 1 + N; dw1 2 + N; dx 13 (first part 12, `1.f / HW` and `da * inv` and `+ dm` 3, `v +=` 1) with
    the first bfloat16 rounding of dx as in ref_backward."""
    x, dout, w1, w2, wsa = (inp[k] for k in ("x", "dout", "w1", "w2", "wsa"))
    ca, pooled, pam, sam, sa = (saved[k] for k in ("ca", "pooled", "pool_argmax", "smap_argmax", "sa"))
    N, H, W, C = x.shape
    Hd, HW, PB, c64 = w1.shape[0], H * W, cbam_pb(H * W), cdiv(C, 64)
    Pw, r = cdiv(HW, 4 * PB), unit(dtype)
    cab, sab = ca[:, None, None, :], sa[..., None]
    wf = wsa.flip(-1, -2)[:, None]
    d, Ad = corr(ws["du"][:, None], wf), corr(ws["du"].abs()[:, None], wf.abs())
    hot = torch.arange(C, device=x.device) == sam[..., None]
    dx1 = dout * sab + (d[:, 0] / C)[..., None] + hot * d[:, 1][..., None]
    Adx1 = dout.abs() * sab + (Ad[:, 0] / C)[..., None] + hot * Ad[:, 1][..., None]

    def blocks(t):  # [N, H, W, C] -> [N, PB, C]: block pb sums the pixels q with (q // 4) % PB == pb
        t = t.reshape(N, HW, C)
        pad = cdiv(HW, 4 * PB) * 4 * PB - HW
        t = torch.cat([t, t.new_zeros(N, pad, C)], 1)
        return t.view(N, -1, PB, 4, C).sum((1, 3))

    out = {"dcap": (blocks(dx1 * x), gamma(15 + Pw) * blocks(Adx1 * x.abs()))}
    s, As = ws["dcap"].sum(1), ws["dcap"].abs().sum(1)
    out["dz"] = (s * ca * (1 - ca), gamma(PB + 3) * As * ca * (1 + ca))
    a, m = pooled[:, 0] @ w1.T, pooled[:, 1] @ w1.T
    Aa, Am = pooled[:, 0].abs() @ w1.abs().T, pooled[:, 1].abs() @ w1.abs().T
    out["hsum"] = (torch.relu(a) + torch.relu(m), gamma(c64 + 8) * (Aa + Am))
    gate = torch.stack([(a > 0), (m > 0)], 1).double()
    out["dpre"] = ((ws["dz"] @ w2)[:, None, :] * gate, gamma(c64 + 7) * (ws["dz"].abs() @ w2.abs())[:, None, :] * gate)
    out["dpool"] = (ws["dpre"] @ w1, gamma(1 + Hd) * (ws["dpre"].abs() @ w1.abs()))
    out["dw2.from_ws"] = (ws["dz"].T @ ws["hsum"], gamma(1 + N) * (ws["dz"].abs().T @ ws["hsum"].abs()))
    out["dw1.from_ws"] = (torch.einsum("njh,njc->hc", ws["dpre"], pooled), gamma(2 + N) * torch.einsum("njh,njc->hc", ws["dpre"].abs(), pooled.abs()))
    phot = (torch.arange(HW, device=x.device)[None, :, None] == pam[:, None, :]).view(N, H, W, C)
    dp = ws["dpool"]
    dx = dx1 * cab + dp[:, 0][:, None, None, :] / HW + phot * dp[:, 1][:, None, None, :]
    Adxa = Adx1 * cab
    Adx = Adxa + dp[:, 0].abs()[:, None, None, :] / HW + phot * dp[:, 1].abs()[:, None, None, :]
    E = gamma(13) * Adx + (r * Adxa * (1 + gamma(12)) if dtype == BF else 0.0)
    out["dx.from_ws"] = (dx, r * dx.abs() + (1 + r) * E)
    return {k: (v, (U * v.abs() + b) if k != "dx.from_ws" else b) for k, (v, b) in out.items()}


def ref_backward(x, dout, w1, w2, wsa, saved, dtype):
    """float64 backward by hand from the kernel's saved tensors, each value with its |.| companion -> ({name: ref}, {name: bound}, info)."""
    ca, pooled, pam, smap, sam, sa = (saved[k] for k in ("ca", "pooled", "pool_argmax", "smap", "smap_argmax", "sa"))
    N, H, W, C = x.shape
    Hd, K = w1.shape[0], wsa.shape[-1]
    HW, NP, R, T, PB = H * W, N * H * W, K // 2, cdiv(C, 256), cbam_pb(H * W)
    Pw, c64 = cdiv(HW, 4 * PB), cdiv(C, 64)
    r = unit(dtype)
    cab, sab = ca[:, None, None, :], sa[..., None]
    # B1
    s, As = (dout * x * cab).sum(3), (dout * x * cab).abs().sum(3)
    du, Adu = s * sa * (1 - sa), As * sa * (1 + sa)
    k_du = 4 * T + 11
    # B2: dsm[p][j] = sum_t du[p - off_t] wsa[j][t] = correlation with the flipped stencil
    wf = wsa.flip(-1, -2)[:, None]
    d, Ad = corr(du[:, None], wf), corr(Adu[:, None], wf.abs())
    hot = torch.arange(C, device=x.device) == sam[..., None]
    dx1 = dout * sab + (d[:, 0] / C)[..., None] + hot * d[:, 1][..., None]
    Adx1 = dout.abs() * sab + (Ad[:, 0] / C)[..., None] + hot * Ad[:, 1][..., None]
    dxa, Adxa = dx1 * cab, Adx1 * cab
    dca, Adca = (dx1 * x).sum((1, 2)), (Adx1 * x.abs()).sum((1, 2))
    # B3
    dz, Adz = dca * ca * (1 - ca), Adca * ca * (1 + ca)
    k_dz = k_du + 18 + Pw + PB
    a, m = pooled[:, 0] @ w1.T, pooled[:, 1] @ w1.T
    Aa, Am = pooled[:, 0].abs() @ w1.abs().T, pooled[:, 1].abs() @ w1.abs().T
    k_pre = c64 + 7
    margin = torch.minimum(a.abs() / (gamma(k_pre) * Aa).clamp(min=1e-300), m.abs() / (gamma(k_pre) * Am).clamp(min=1e-300))
    hsum, Ahs, k_hs = torch.relu(a) + torch.relu(m), Aa + Am, k_pre + 1
    dh, Adh = dz @ w2, Adz @ w2.abs()
    k_dh = k_dz + c64 + 7
    ga, gm = (a > 0).double(), (m > 0).double()
    da, dm = (dh * ga) @ w1, (dh * gm) @ w1
    Ada, Adm = (Adh * ga) @ w1.abs(), (Adh * gm) @ w1.abs()
    k_dp = k_dh + 1 + Hd
    # B4
    dw2, Adw2 = dz.T @ hsum, Adz.T @ Ahs
    dw1 = (dh * ga).T @ pooled[:, 0] + (dh * gm).T @ pooled[:, 1]
    Adw1 = (Adh * ga).T @ pooled[:, 0].abs() + (Adh * gm).T @ pooled[:, 1].abs()
    # B5: dwsa[j][t] = sum_p du[p] smap[p + off_t][j]
    unf = F.unfold(smap.permute(0, 3, 1, 2), K, padding=R)  # [N, 2 K K, HW], rows (j, ty, tx)
    dwsa = torch.einsum("nkp,np->k", unf, du.reshape(N, HW)).view(2, K, K)
    Adwsa = torch.einsum("nkp,np->k", unf.abs(), Adu.reshape(N, HW)).view(2, K, K)
    k_dwsa = k_du + 24 + cdiv(cdiv(NP, 1024), 2)
    # B6
    phot = (torch.arange(HW, device=x.device)[None, :, None] == pam[:, None, :]).view(N, H, W, C)
    dx = dxa + da[:, None, None, :] / HW + phot * dm[:, None, None, :]
    Adx = Adxa + Ada[:, None, None, :] / HW + phot * Adm[:, None, None, :]
    E = gamma(k_dp + 4) * Adx + (r * Adxa * (1 + gamma(k_du + 12)) if dtype == BF else 0.0)
    ref = {"dx": dx, "dw1": dw1, "dw2": dw2, "dwsa": dwsa, "du": du}
    bound = {
        "dx": r * dx.abs() + (1 + r) * E,
        "dw1": U * dw1.abs() + gamma(k_dh + 2 + N) * Adw1,
        "dw2": U * dw2.abs() + gamma(k_dz + k_hs + 1 + N) * Adw2,
        "dwsa": U * dwsa.abs() + gamma(k_dwsa) * Adwsa,
        "du": U * du.abs() + gamma(k_du) * Adu,
    }
    return ref, bound, {"gate_margin": float(margin.min()), "du": du, "dz": dz, "hsum": hsum, "dpool": torch.stack([da, dm], 1)}


# ---- reports and checks -----------------------------------------------------------------------------------------------------------------------
AXES = {"nhwc": ("n", "h", "w", "c"), "nc": ("n", "c"), "nhw": ("n", "h", "w"), "w1": ("hidden", "c"), "w2": ("c", "hidden"), "wsa": ("j", "ky", "kx"), "npc": ("n", "pb", "c"), "nh": ("n", "hidden"),
        "njh": ("n", "j", "hidden"), "njc": ("n", "j", "c")}
STAGE_AXES = {"pooled.avg": "nc", "pooled.max": "nc", "pool_argmax": "nc", "ca": "nc", "smap.mean": "nhw", "smap.max": "nhw", "smap_argmax": "nhw",
              "sa": "nhw", "out": "nhwc", "dx": "nhwc", "dw1": "w1", "dw2": "w2", "dwsa": "wsa", "du": "nhw", "dwsa.from_du": "wsa", "dcap": "npc", "dz": "nc", "hsum": "nh", "dpre": "njh",
              "dpool": "njc", "dw1.from_ws": "w1", "dw2.from_ws": "w2", "dx.from_ws": "nhwc"}


def locate(stage):
    names = AXES[STAGE_AXES[stage]]
    return lambda idx: f"stage {stage} (" + ", ".join(f"{n}={i}" for n, i in zip(names, idx)) + ")"


def report(what, got, ref, bad, err, loc, limit=5):
    """the number of bad elements and the worst five with their index and the stage."""
    cnt = int(bad.sum())
    flat = torch.where(bad.reshape(-1), err.reshape(-1).nan_to_num(float("inf")), torch.full_like(err.reshape(-1), -1.0))
    order = torch.argsort(flat, descending=True)[: min(limit, cnt)]
    lines = [f"{what}: {cnt} of {bad.numel()} elements wrong; worst:"]
    g, r = got.reshape(-1), ref.reshape(-1)
    for o in order.tolist():
        idx = [int(i) for i in torch.unravel_index(torch.tensor(o), tuple(bad.shape))]
        lines.append(f"  {loc(idx)}: got {float(g[o])!r} expected {float(r[o])!r}")
    return "\n".join(lines)


def check_exact(what, stage, got, expected):
    g, e = got.double().cpu(), expected.double().cpu()
    assert g.shape == e.shape, (what, stage, tuple(g.shape), tuple(e.shape))
    bad = ~(g == e)
    if bool(bad.any()):
        raise AssertionError(report(f"{what} {stage} [exact]", g, e, bad, (g - e).abs(), locate(stage)))


def check_bound(what, stage, got, ref, bound):
    """per-element |got - ref| <= bound (NaN fails) -> worst err / bound."""
    g = got.double()
    assert g.shape == ref.shape, (what, stage, tuple(g.shape), tuple(ref.shape))
    err = (g - ref).abs()
    bad = ~(err <= bound)
    ratio = err / bound.clamp(min=1e-300)
    if bool(bad.any()):
        raise AssertionError(report(f"{what} {stage} [float64 bound]", g, ref, bad, ratio, locate(stage)))
    return float(ratio.max()) if err.numel() else 0.0


def check_forward(what, got, inp, dtype):
    """every forward output of the kernels (or of the emulation) `got`, each stage from got's outputs of the stage before -> {stage: ratio}."""
    x, w1, w2, wsa = inp["x"], inp["w1"], inp["w2"], inp["wsa"]
    N, H, W, C = x.shape
    xf = x.reshape(N, H * W, C)
    ratios = {}
    check_exact(what, "pooled.max", got["pooled"][:, 1], xf.amax(1))
    check_exact(what, "pool_argmax", got["pool_argmax"], first_argmax(xf, 1))
    ratios["pooled.avg"] = check_bound(what, "pooled.avg", got["pooled"][:, 0], *stage_avg(x))
    ratios["ca"] = check_bound(what, "ca", got["ca"], *stage_ca(got["pooled"].double(), w1, w2))
    mx, am = stage_smax(x, got["ca"])
    check_exact(what, "smap.max", got["smap"][..., 1], mx)
    check_exact(what, "smap_argmax", got["smap_argmax"], am)
    ratios["smap.mean"] = check_bound(what, "smap.mean", got["smap"][..., 0], *stage_smean(x, got["ca"].double()))
    ratios["sa"] = check_bound(what, "sa", got["sa"], *stage_sa(got["smap"].double(), wsa))
    ratios["out"] = check_bound(what, "out", got["out"], *stage_out(x, got["ca"].double(), got["sa"].double(), dtype))
    return ratios


def saved_f64(got):
    return {k: (got[k].long() if "argmax" in k else got[k].double()) for k in ("ca", "pooled", "pool_argmax", "smap", "smap_argmax", "sa")}


def check_backward(what, got, saved, inp, dtype):
    """dx, dw1, dw2, dwsa of `got` against the float64 backward from the saved tensors -> ({name: ratio}, gate margin)."""
    ref, bound, info = ref_backward(inp["x"], inp["dout"], inp["w1"], inp["w2"], inp["wsa"], saved_f64(saved), dtype)
    ratios, failures = {}, []
    for n in ("dx", "dw1", "dw2", "dwsa"):  # all four are looked at, so a report names every output a defect reaches
        try:
            ratios[n] = check_bound(what, n, got[n], ref[n], bound[n])
        except AssertionError as e:
            failures.append(str(e))
    if "du" in got:  # the workspace: every kernel of the backward on its own, from the kernels' own intermediates before it
        sv = saved_f64(saved)
        stages = [("du", got["du"], ref["du"], bound["du"])]
        stages.append(("dwsa.from_du", got["dwsa"]) + stage_dwsa(got["du"].double(), sv["smap"], inp["wsa"].shape[-1]))
        if "dcap" in got:
            ws = {k: got[k].double() for k in ("du", "dcap", "dz", "hsum", "dpre", "dpool")}
            for name, (r_, b_) in stages_from_workspace(inp, sv, ws, dtype).items():
                stages.append((name, got[name.split(".")[0]], r_, b_))
        for name, g_, r_, b_ in stages:
            try:
                ratios[name] = check_bound(what, name, g_, r_, b_)
            except AssertionError as e:
                failures.append(str(e))
    if failures:
        raise AssertionError("\n".join(failures))
    return ratios, info["gate_margin"]


def rel(a, b):
    """the suite's tensor-wide relative-L2 gate."""
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp(min=1e-12))


# ---- float32 emulation of the kernels' rounding points (CPU; tests/test_host_cbam_check.py) -----------------------------------------------
# Same grouping of every sum as the kernels; products are rounded before they are added (an fma on the device only removes a rounding);
# exp2 and the reciprocal come from float32 libm.  `fault` plants one named defect (FAULTS).
FAULTS = ("pool_last_max", "pool_lane_order_tie", "pool_drop_last_block", "chan_last_max", "stats_drop_second_trip", "stencil_not_flipped",
          "dmean_over_hw", "da_not_over_hw", "drop_part_row", "drop_pb_partial", "drop_acc_slot3", "wsa_drop_tail", "w_drop_image8", "hsum_one_relu")


def _seq_sum(terms, dim):
    """0.f + t0 + t1 + ... in order along dim (float32)."""
    s = torch.zeros_like(terms.select(dim, 0))
    for i in range(terms.shape[dim]):
        s = s + terms.select(dim, i)
    return s


def _wave_sum(v):
    """the xor butterfly over the last dim of 64 lanes: lane 0's value (the halving tree; float addition commutes)."""
    assert v.shape[-1] == 64
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _pad_to(t, dim, mult, value=0.0):
    n = t.shape[dim]
    extra = cdiv(n, mult) * mult - n
    if extra == 0:
        return t
    shape = list(t.shape)
    shape[dim] = extra
    return torch.cat([t, torch.full(shape, value, dtype=t.dtype)], dim)


def _sigmoid32(z):
    return torch.reciprocal(1.0 + torch.exp2(-z * torch.tensor(LOG2E, dtype=torch.float32)))


def _lane_dot(w, v):
    """sum_c w[..., c] v[..., c] as a wave does it: lane = c % 64, trips in order, then the butterfly."""
    t = _pad_to(w * v, -1, 64)
    return _wave_sum(_seq_sum(t.view(*t.shape[:-1], -1, 64), -2))


def _chan_lanes(t):
    """[..., C] -> [..., 64] per-lane sums in the order of the pixel-per-wave kernels: channel = lane * 4 + 256 * i + r, i then r."""
    t = _pad_to(t, -1, 256)
    t = t.view(*t.shape[:-1], -1, 64, 4)  # [..., i, lane, r]
    s = torch.zeros_like(t[..., 0, :, 0])
    for i in range(t.shape[-3]):
        for r in range(4):
            s = s + t[..., i, :, r]
    return s


def emu_forward(inp, dtype, fault=None):
    x = inp["x"].float()
    w1, w2, wsa = inp["w1"].float(), inp["w2"].float(), inp["wsa"].float()
    N, H, W, C = x.shape
    HW, Hd, K = H * W, w1.shape[0], wsa.shape[-1]
    xf = x.view(N, HW, C)
    # cbam_pool_kernel: pixel p on pixel lane p % 16, its pixels in order; then the 16 lanes in order
    lanes = _pad_to(xf, 1, 16).view(N, -1, 16, C)
    avg = _seq_sum(_seq_sum(lanes, 1), 1) / torch.tensor(float(HW))
    lm = _pad_to(xf, 1, 16, float("-inf")).view(N, -1, 16, C)
    mx = xf.amax(1)
    pam = first_argmax(xf, 1)
    if fault == "pool_last_max":
        pam = last_argmax(xf, 1)
    if fault == "pool_lane_order_tie":  # the lowest pixel lane that holds the maximum wins, whatever its pixel index
        lane_max, lane_first = lm.amax(1), first_argmax(lm, 1) * 16 + torch.arange(16)[None, :, None]
        pam = lane_first.gather(1, first_argmax(lane_max, 1)[:, None, :])[:, 0]
    pooled = torch.stack([avg, mx], 1)
    pam = pam.to(torch.int32)
    if fault == "pool_drop_last_block":
        pooled[:, :, C // 64 * 64:] = float("nan")
        pam[:, C // 64 * 64:] = -1
    # cbam_mlp_kernel
    a, m = _lane_dot(w1[None], pooled[:, None, 0]), _lane_dot(w1[None], pooled[:, None, 1])
    hs = torch.relu(a) + torch.relu(m)
    ca = _sigmoid32(_seq_sum(w2[None] * hs[:, None, :], 2))
    # cbam_stats_kernel
    t = x * ca[:, None, None, :]
    ts = t[..., :256] if fault == "stats_drop_second_trip" else t
    smean = _wave_sum(_chan_lanes(ts)) / torch.tensor(float(C))
    sam = (last_argmax(t, 3) if fault == "chan_last_max" else first_argmax(t, 3)).to(torch.int32)
    smap = torch.stack([smean, t.amax(3)], 3)
    # cbam_apply_kernel: one tap per lane
    unf = F.unfold(smap.permute(0, 3, 1, 2), K, padding=K // 2).view(N, 2, K * K, HW)
    wk = wsa.view(2, K * K)
    taps = wk[0][None, :, None] * unf[:, 0] + wk[1][None, :, None] * unf[:, 1]
    sa = _sigmoid32(_wave_sum(_pad_to(taps.permute(0, 2, 1), -1, 64))).view(N, H, W)
    out = ((x * ca[:, None, None, :]) * sa[..., None]).to(dtype)
    return {"pooled": pooled, "pool_argmax": pam, "ca": ca, "smap": smap, "smap_argmax": sam, "sa": sa, "out": out}


def emu_backward(inp, saved, dtype, fault=None):
    x, dout = inp["x"].float(), inp["dout"].float()
    w1, w2, wsa = inp["w1"].float(), inp["w2"].float(), inp["wsa"].float()
    ca, pooled, smap, sa = (saved[k].float() for k in ("ca", "pooled", "smap", "sa"))
    pam, sam = saved["pool_argmax"].long(), saved["smap_argmax"].long()
    N, H, W, C = x.shape
    HW, NP, Hd, K = H * W, N * H * W, w1.shape[0], wsa.shape[-1]
    KK, PB = K * K, cbam_pb(H * W)
    cab = ca[:, None, None, :]
    # B1
    s = _wave_sum(_chan_lanes(dout * x * cab))
    du = s * sa * (1.0 - sa)
    # B2: lane t holds du[p - off_t] * wsa[j][t]; unfold row t' holds du[p + off_t'], so t' = KK - 1 - t
    unf = F.unfold(du[:, None], K, padding=K // 2)  # [N, KK, HW]
    if fault != "stencil_not_flipped":
        unf = unf.flip(1)
    wk = wsa.view(2, KK)
    d0 = _wave_sum(_pad_to((unf * wk[0][None, :, None]).permute(0, 2, 1), -1, 64)).view(N, H, W)
    d1 = _wave_sum(_pad_to((unf * wk[1][None, :, None]).permute(0, 2, 1), -1, 64)).view(N, H, W)
    dmean = d0 / torch.tensor(float(HW if fault == "dmean_over_hw" else C))
    hot = torch.arange(C) == sam[..., None]
    dx1 = dout * sa[..., None] + dmean[..., None] + torch.where(hot, d1[..., None], torch.zeros(()))
    dx = (dx1 * cab).to(dtype)  # first store
    prod = dx1 * x
    if fault == "drop_acc_slot3":
        prod[..., 768:] = 0.0
    acc = _seq_sum(_pad_to(prod.view(N, HW, C), 1, 4 * PB).view(N, -1, 4 * PB, C), 1).view(N, PB, 4, C)  # wave (pb, wv): pixels pb*4+wv + 4 PB j
    dcap = acc[:, :, 0] + acc[:, :, 1] + acc[:, :, 2] + acc[:, :, 3] if fault != "drop_part_row" else acc[:, :, 0] + acc[:, :, 1] + acc[:, :, 3]
    # B3
    sd = _seq_sum(dcap[:, : PB - 1] if fault == "drop_pb_partial" and PB > 1 else dcap, 1)
    dz = sd * ca * (1.0 - ca)
    a, m = _lane_dot(w1[None], pooled[:, None, 0]), _lane_dot(w1[None], pooled[:, None, 1])
    hsum = torch.relu(a + m) if fault == "hsum_one_relu" else torch.relu(a) + torch.relu(m)
    dh = _lane_dot(w2.T[None], dz[:, None, :])
    dpa, dpm = torch.where(a > 0, dh, torch.zeros(())), torch.where(m > 0, dh, torch.zeros(()))
    da, dm = _seq_sum(dpa[:, :, None] * w1[None], 1), _seq_sum(dpm[:, :, None] * w1[None], 1)
    # B4
    keep = [n for n in range(N) if not (fault == "w_drop_image8" and n == 8)]
    dw2 = _seq_sum((dz[:, :, None] * hsum[:, None, :])[keep], 0)
    dw1 = _seq_sum((dpa[:, :, None] * pooled[:, None, 0] + dpm[:, :, None] * pooled[:, None, 1])[keep], 0)
    # B5: thread tid takes p = tid + 1024 j; even trips on chain 0, odd trips on chain 1 (the odd one out, the tail, joins chain 0)
    sun = F.unfold(smap.permute(0, 3, 1, 2), K, padding=K // 2).permute(1, 0, 2).reshape(2 * KK, NP)
    terms = _pad_to(du.reshape(1, NP) * sun, 1, 2048).view(2 * KK, -1, 2, 1024)
    if fault in ("wsa_drop_tail", "wsa_drop_tail_thread0"):  # the second: one thread only (not in FAULTS: the gap test's variant)
        for tid in range(min(NP, 1024) if fault == "wsa_drop_tail" else 1):
            n_t = cdiv(NP - tid, 1024)
            if n_t % 2:
                terms[:, (n_t - 1) // 2, 0, tid] = 0.0
    s01 = _seq_sum(terms[:, :, 0], 1) + _seq_sum(terms[:, :, 1], 1)
    dwsa = _seq_sum(_wave_sum(s01.view(2 * KK, 16, 64)), 1).view(2, K, K)
    # B6
    inv = torch.tensor(1.0) / torch.tensor(float(1 if fault == "da_not_over_hw" else HW))
    phot = (torch.arange(HW)[None, :, None] == pam[:, None, :]).view(N, H, W, C)
    v = dx.float() + (da[:, None, None, :] * inv + torch.where(phot, dm[:, None, None, :], torch.zeros(())))
    return {"dx": v.to(dtype), "dw1": dw1, "dw2": dw2, "dwsa": dwsa, "du": du, "dcap": dcap, "dz": dz, "hsum": hsum, "dpre": torch.stack([dpa, dpm], 1),
            "dpool": torch.stack([da, dm], 1)}


def bf16_ulp_up(t, flat_index):
    """t (bfloat16) with ONE element moved one bfloat16 ulp away from zero."""
    o = t.clone()
    bits = o.view(torch.int16).reshape(-1)
    bits[flat_index] += 1
    return o
