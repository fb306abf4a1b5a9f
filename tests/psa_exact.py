"""Element-by-element gates for the PSA attention kernels (csrc/swin.hip ymi_psa_attention_fwd / _bwd), built on tests/attn_exact.py: the same
two gates, restated for qkv packed per head as [q (kd) | k (kd) | v (hd)] with kd != hd.  A helper module for the tests (not a conftest).

The PSA entry points always run the tiled (flash-style) kernels, so every bound takes attn_exact's `tiled` rows.

Gate 1 (placement) is attn_exact's one-hot construction on the SCORE operands: Q and K are `onehot_operands(.., kd, ..)` (code over kd - 1
dimensions, selected raw score -2^8, scaled by kd^-0.5), V and dO are +-1 of width hd.  It demands O = V[pi(m)], v_out = V, dV[j] = sum of the dO
rows that select j, and dQ = dK = 0, bit for bit; lse within 2 float32 ulps.  It needs kd - 1 >= ceil(log2 L) (`attn_exact.onehot_ok(L, kd)`):
with kd = 4 that is L <= 8, so the grid's kd = 4 cases pass Gate 1 only at L = 1 and are held by Gate 2 alone elsewhere.

Gate 2 (precision) is `attn_exact.attn_bounds` with two widths.  What carries over with hd -> kd, because the term counts the roundings of a
contraction over the score width: gamma_kd in e_mj (the float32 score), and sc = kd^-0.5 everywhere.  What does NOT carry over with kd and takes
the value width hd instead, because the contraction runs over V's columns: gamma_hd in e_dP = gamma_hd sum_d |dO||V| (dP = dO V^T) and in the
tiled e_Delta's gamma_hd sum_d |dO||O| (Delta = dO . O_stored).  gamma_L, r, r_P, delta_m and kappa_m do not depend on a width.  No term is added,
dropped or scaled: with kd = hd `psa_bounds` equals `attn_bounds(.., form="tiled")` term for term."""
import math

import torch

import attn_exact as AE
from psa_ref import split_packed


def psa_bounds(q, k, v, dout, ref, dtype):
    """Gate 2 bounds for O, lse and, with dout, dQ / dK / dV: q, k [images, heads, L, kd], v, dout [images, heads, L, hd]; ref = AE.attn_ref64."""
    q, k, v = q.double(), k.double(), v.double()
    u, r = AE.U32, AE.unit(dtype)
    rP = AE.unit(dtype)
    L, kd, hd = q.shape[-2], q.shape[-1], v.shape[-1]
    sc, s, P = ref["sc"], ref["s"], ref["P"]
    absS = q.abs() @ k.abs().transpose(-1, -2)
    E = (sc * AE.gamma(kd) * absS + 2 * u * s.abs()).amax(-1)
    R = (s.amax(-1, keepdim=True) - s).amax(-1)
    delta = 2 * E + 4 * u * (1 + R)
    kappa = 2 * delta + AE.gamma(L) + 2 * u
    b = {}
    b["O"] = r * ref["O"].abs() + (1 + r) * (rP + kappa).unsqueeze(-1) * (P @ v.abs())
    dl = delta + AE.gamma(L)
    b["lse"] = E + dl * (1 + 2 * dl) + 4 * u * (1 + ref["lse"].abs() + math.log(max(L, 1)))
    if dout is None:
        return b
    dO = dout.double()
    dP, Dl, dS = ref["dP"], ref["Delta"].unsqueeze(-1), ref["dS"]
    b["dV"] = r * ref["dV"].abs() + (1 + r) * (P * (rP + kappa).unsqueeze(-1)).transpose(-1, -2) @ dO.abs()
    e_dP = AE.gamma(hd) * (dO.abs() @ v.abs().transpose(-1, -2))
    e_D = (dO.abs() * b["O"]).sum(-1, keepdim=True) + AE.gamma(hd) * (dO.abs() * ref["O"].abs()).sum(-1, keepdim=True)  # the tiled form's Delta
    e_dS = r * dS.abs() + sc * P * (kappa.unsqueeze(-1) * (dP - Dl).abs() + e_dP + e_D) + 2 * u * dS.abs()
    b["dQ"] = r * ref["dQ"].abs() + (1 + r) * (e_dS @ k.abs() + AE.gamma(L) * dS.abs() @ k.abs())
    b["dK"] = r * ref["dK"].abs() + (1 + r) * (e_dS.transpose(-1, -2) @ q.abs() + AE.gamma(L) * dS.abs().transpose(-1, -2) @ q.abs())
    return b


def onehot_psa_operands(images, heads, L, kd, hd, gen):
    """-> q, k [images, heads, L, kd], v, dout [images, heads, L, hd] (float32 host, bfloat16-exact integers) and the targets pi."""
    q, k, _, _, pi = AE.onehot_operands(images, heads, L, kd, gen)
    v = torch.randint(0, 2, (images, heads, L, hd), generator=gen).float() * 2 - 1
    dout = torch.randint(0, 2, (images, heads, L, hd), generator=gen).float() * 2 - 1
    return q, k, v, dout, pi


def lse_heads(lse, L):
    """[T, heads] -> [images, heads, L]."""
    T, heads = lse.shape
    return lse.reshape(T // L, L, heads).permute(0, 2, 1)


def outputs(qkv, out, v_out, lse, dqkv, L, heads, kd):
    """what a launch pair produced, per (image, head): O, V (the compacted copy), lse, dQ, dK, dV."""
    hd = qkv.shape[1] // heads - 2 * kd
    got = {"O": AE.heads_view(out, L, heads), "V": AE.heads_view(v_out, L, heads), "lse": lse_heads(lse, L)}
    assert got["O"].shape[-1] == hd
    if dqkv is not None:
        got["dQ"], got["dK"], got["dV"] = split_packed(dqkv, L, heads, kd)
    return got
