"""The fused optimizer step (csrc/optim.hip) restated in float64, and a driver that calls its entry points directly.

  scalars()     everything opt_finalize_kernel writes into the 64-byte state record, in Python floats, with the float32 rounding points
                the kernel documents (or, round32=False, with none of them: what torch.optim computes on float64 parameters).
  update()      one step of one tensor in float64 from float32 inputs, after torch.optim's single-tensor formulas as the comments of
                opt_update (csrc/optim.hip) name them; restate_step() applies it to a list of entries.
  scaled_err()  per-element error over the magnitudes that entered the result.
  F32_DISTANCE  the distance of float32 torch.optim (+ clip_grad_norm_ + the oracle's ModelEMA) from this restatement, measured by
                tests/test_host_optim_check.py; the bounds of tests/test_gpu_optim_exact.py are MARGIN times these.
  Pool, build_table, pack_state / unpack_state, hyper_vector, launch_*: the direct driver (needs the GPU only when called).
  Toy           a module whose tensor lengths sit on every edge of the kernels' chunking (shared with test_gpu_grad_accumulate.py).

Importing this file needs no GPU."""
import ctypes
import math
import struct

import numpy as np
import torch
import torch.nn as nn

RULES = {0: "SGD", 1: "AdamW", 2: "Adam", 3: "Adamax", 4: "NAdam", 5: "RAdam", 6: "RMSprop"}
CHUNK = 4096  # ymi_opt_chunk_elems(); the GPU test asserts it
QUANT = ("p", "buf", "sec", "ema")

# worst scaled_err of float32 torch.optim (CPU, foreach=False) against update(), one step from a shared float32 state, over 8 steps of the
# host test's model; rounded up to two digits.  test_host_optim_check.py::test_f32_distance_is_what_is_recorded keeps them honest.
F32_DISTANCE = {
    "SGD": {"p": 6.0e-8, "buf": 1.1e-7, "sec": 0.0, "ema": 1.7e-7},
    "AdamW": {"p": 1.5e-7, "buf": 1.1e-7, "sec": 1.8e-7, "ema": 2.3e-7},
    "Adam": {"p": 1.3e-7, "buf": 1.2e-7, "sec": 2.1e-7, "ema": 1.7e-7},
    "Adamax": {"p": 7.5e-8, "buf": 1.2e-7, "sec": 1.1e-7, "ema": 1.7e-7},
    "NAdam": {"p": 1.5e-7, "buf": 1.2e-7, "sec": 2.0e-7, "ema": 2.2e-7},
    "RAdam": {"p": 6.0e-8, "buf": 1.2e-7, "sec": 1.9e-7, "ema": 1.7e-7},
    "RMSprop": {"p": 6.5e-8, "buf": 1.3e-7, "sec": 2.1e-7, "ema": 1.6e-7},
}
# the kernel rounds the per-step scalars (clip * scale, lr / bc1, lr * c0 ...) to float32 where torch holds doubles, and may contract
# a multiply-add: a handful of extra roundings on a chain of about as many
MARGIN = 4.0


def f32(x):
    return float(np.float32(x))


def ulps32(a, b):
    """distance of two float32 values in units of the last place (0 for equal values, inf = inf)"""
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(v & 0x7FFFFFFF) for v in (ia, ib))
    return abs(ia - ib)


# ------------------------------------------------------------------------------------------------------------------ hyper and state
def hyper_vector(rule, lr, wd, beta1, *, max_norm=10.0, ema_decay=0.9999, tau=2000.0, nesterov=False, gscale=1.0, beta2=0.999, eps=1e-8,
                 momentum_decay=4e-3, round32=True):
    """the 20 floats of optim.hip's `hyper` as engine/optim.py::hyper_values fills them (lr, wd: one value per group; beta1 is the momentum of
    SGD / RMSprop; beta2 is RMSprop's alpha).  round32: every entry rounded to float32, as the device array holds it."""
    h = [*lr, *wd, beta1, max_norm, ema_decay, tau, 1.0 if nesterov else 0.0, gscale, 0.0, 0.0, float(rule), 0.0, 0.0, 0.0, 0.0, 0.0]
    if rule:
        h[12], h[13], h[15] = beta2, eps, 1 - beta2
        h[16] = 1 - beta1 if rule != 6 else 0.0
    if rule == 4:
        h[17] = momentum_decay
        if round32:
            h[18], h[19] = beta1 - f32(beta1), momentum_decay - f32(momentum_decay)
    return [f32(v) for v in h] if round32 else [float(v) for v in h]


STATE_FMT = "<4f2q2f4fd"  # clip, norm, ema_d, ema_1md, updates, steps, inv_bc1, bc2_sqrt, c0..c3, mu_product
STATE_KEYS = ("clip", "norm", "ema_d", "ema_1md", "updates", "steps", "inv_bc1", "bc2_sqrt", "c0", "c1", "c2", "c3", "mu_product")
assert struct.calcsize(STATE_FMT) == 64


def zero_state(**kw):
    s = {k: 0 if k in ("updates", "steps") else 0.0 for k in STATE_KEYS}
    s.update(kw)
    return s


def pack_state(s):
    return struct.pack(STATE_FMT, *(s[k] for k in STATE_KEYS))


def unpack_state(raw):
    return dict(zip(STATE_KEYS, struct.unpack(STATE_FMT, bytes(raw))))


def radam_rho(beta2, t):
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    return rho_inf - 2.0 * t * beta2 ** t / (1.0 - beta2 ** t), rho_inf


def radam_guard(beta2, steps):
    """RAdam switches its rectification on where rho_t > 5, and with beta2 = 0.999 rho_5 = 4.996: the decision must not hang on rounding.
    For every step count a test uses rho_t is at least 1e-3 from 5, with the double beta2 and with the one rebuilt from its float32 complement."""
    for t in steps:
        for b2 in (beta2, 1.0 - f32(1.0 - beta2)):
            rho = radam_rho(b2, t)[0]
            assert abs(rho - 5.0) >= 1e-3, f"RAdam: rho_{t} = {rho} with beta2 = {b2!r} is within 1e-3 of the switch"


def scalars(hyper, state_in, sumsq, *, norm=None, round32=True, fault=None):
    """the state record after opt_finalize_kernel, from the record before it and the total of the per-chunk sums of squares.
    norm: take this (float32) norm instead of sqrt(sumsq) - `clip` is exact given the device's norm.  Fields the kernel does not write keep
    their value.  The result carries the hyper vector under 'hyper' for update()."""
    h = hyper
    r = f32 if round32 else float
    s = dict(state_in)
    s["hyper"] = list(h)
    nrm = r(math.sqrt(sumsq)) if norm is None else float(norm)
    # norm is rounded to float32 BEFORE the quotient, and the quotient is float32 arithmetic with 1e-6f
    coef = float(np.float32(h[7]) / (np.float32(nrm) + np.float32(1e-6))) if round32 else (h[7] / (nrm + 1e-6) if h[7] > 0 else 1.0)
    s["norm"] = nrm
    s["clip"] = min(coef, 1.0) if h[7] > 0 else 1.0
    u = int(state_in["updates"]) + 1
    s["updates"] = u
    ue = u - 1 if fault == "ema_updates_minus_1" else u
    d = h[8] * (1.0 - math.exp(-ue / h[9]))
    s["ema_d"], s["ema_1md"] = r(d), r(1.0 - d)
    t = int(state_in["steps"]) + 1
    s["steps"] = t
    rule = int(h[14])
    if rule:
        # the betas are rebuilt from their float32 complements
        b1, b2 = 1.0 - h[16], 1.0 - h[15]
        tb = t - 1 if fault == "bias_correction_t_minus_1" else t
        bc1, bc2 = 1.0 - b1 ** tb, 1.0 - b2 ** tb
        s["inv_bc1"] = r(1.0 / bc1) if bc1 != 0.0 else math.inf
        s["bc2_sqrt"] = r(math.sqrt(bc2))
        if rule == 4:
            b1x, md = h[6] + h[18], h[17] + h[19]  # head + tail
            mu = b1x * (1.0 - 0.5 * 0.96 ** (t * md))
            mu_next = b1x * (1.0 - 0.5 * 0.96 ** ((t + 1) * md))
            if fault == "nadam_mu_next_is_mu":
                mu_next = mu
            # torch keeps mu_product as a float32 tensor and multiplies it in place: one float32 rounding per step, in either mode
            mp = float(np.float32(1.0 if t == 1 else state_in["mu_product"]) * np.float32(mu))
            s["mu_product"] = mp
            s["c0"] = r((1.0 - mu) / (1.0 - mp))
            s["c1"] = r(mu_next / (1.0 - mp * mu_next))
            s["c2"] = r(bc2)
        elif rule == 5:
            radam_guard(b2, [t])
            rho_t, rho_inf = radam_rho(b2, t + 1 if fault == "radam_one_step_early" else t)
            if rho_t > 5.0:
                s["c0"] = r(math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)))
                s["c1"] = 1.0
            else:
                s["c0"], s["c1"] = 1.0, 0.0
    return s


# ------------------------------------------------------------------------------------------------------------------------ the update
def update(rule, nesterov, p, g, buf, sec, ema, lr, wd, s, *, ema_only=False, fault=None, chunk=CHUNK):
    """one step of one tensor in float64.  p, g, buf, sec, ema: flat tensors (float32 inputs, or float64 carried state) or None; s: scalars().
    g is None: no gradient - p, buf, sec unchanged, the EMA still moves.  ema_only: an EMA-only entry (buffers, frozen parameters).
    -> (p, buf, sec, ema) in float64, None where the input was None."""
    h = s["hyper"]
    dbl = lambda t: None if t is None else t.detach().double().reshape(-1).clone()  # noqa: E731
    p0, g, b0, v0, e0 = dbl(p), dbl(g), dbl(buf), dbl(sec), dbl(ema)
    pn, bn, vn = p0, b0, v0
    if g is not None and not ema_only:
        mom, b2, eps, omb2, omb1 = h[6], h[12], h[13], h[15], h[16]
        gr = g * (s["clip"] if fault == "clip_without_scale" else s["clip"] * h[11])
        if fault == "decay_in_undecayed_group" and wd == 0.0:
            wd = 5e-4
        decoupled = rule == 1 and fault != "adamw_decay_on_gradient"
        if wd != 0.0 and not decoupled:
            gr = gr + wd * p0                                     # grad.add(param, alpha=weight_decay)
        if rule == 0:                                             # torch.optim.SGD
            bn = b0 * mom + gr                                    # buf.mul_(momentum).add_(grad); the first step's clone is the same from buf = 0
            gr = gr + mom * bn if (nesterov and fault != "nesterov_dropped") else bn
            pn = p0 - lr * gr
        elif rule in (1, 2):                                      # torch.optim.AdamW / Adam
            pw = p0 * (1.0 - lr * wd) if decoupled else p0        # param.mul_(1 - lr * weight_decay)
            bn = b0 + (gr - b0) * omb1                            # exp_avg.lerp_(grad, 1 - beta1)
            vn = v0 * b2 + omb2 * gr * gr                         # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
            denom = vn.sqrt() / (s["bc2_sqrt"] + eps) if fault == "eps_inside_the_quotient" else vn.sqrt() / s["bc2_sqrt"] + eps
            pn = pw - (lr * s["inv_bc1"]) * (bn / denom)          # param.addcdiv_(exp_avg, denom, value=-lr / bias_correction1)
        elif rule == 3:                                           # torch.optim.Adamax
            bn = b0 + (gr - b0) * omb1
            vn = torch.maximum(v0 * b2, gr.abs()) + eps if fault == "adamax_eps_outside_max" else torch.maximum(v0 * b2, gr.abs() + eps)
            pn = p0 - (lr * s["inv_bc1"]) * (bn / vn)
        elif rule == 4:                                           # torch.optim.NAdam
            bn = b0 + (gr - b0) * omb1
            vn = v0 * b2 + omb2 * gr * gr
            denom = (vn / s["c2"]).sqrt() + eps
            pn = p0 - (lr * s["c0"]) * (gr / denom) - (lr * s["c1"]) * (bn / denom)
        elif rule == 5:                                           # torch.optim.RAdam
            bn = b0 + (gr - b0) * omb1
            vn = v0 * b2 + omb2 * gr * gr
            bce = bn * s["inv_bc1"]
            pn = p0 - bce * lr * (s["bc2_sqrt"] / (vn.sqrt() + eps)) * s["c0"] if s["c1"] != 0.0 else p0 - bce * lr
        else:                                                     # torch.optim.RMSprop(momentum > 0)
            vn = v0 * b2 + omb2 * gr * gr
            avg = vn.sqrt() + eps
            bn = (b0 + gr / avg) * mom if fault == "rmsprop_momentum_after_quotient" else b0 * mom + gr / avg
            pn = p0 - lr * bn
        if fault == "last_element_unchanged":
            pn[-1], bn[-1] = p0[-1], b0[-1]
        if fault == "element_after_chunk_boundary_twice" and pn.numel() > chunk:
            one = update(rule, nesterov, pn[chunk:chunk + 1], g[chunk:chunk + 1], bn[chunk:chunk + 1], None if vn is None else vn[chunk:chunk + 1], None, lr, wd, s)
            pn[chunk], bn[chunk] = one[0][0], one[1][0]
    en = None
    if e0 is not None:
        en = e0 * s["ema_d"] + s["ema_1md"] * (p0 if fault == "ema_of_old_parameter" else pn)  # v *= d; v += (1 - d) * model value
    return pn, bn, vn, en


def restate_step(rule, nesterov, entries, s, **kw):
    """update() over entries = [{'p', 'g', 'buf', 'sec', 'ema', 'group', 'ema_only'}] -> [(p, buf, sec, ema)]"""
    h = s["hyper"]
    return [update(rule, nesterov, e["p"], e.get("g"), e.get("buf"), e.get("sec"), e.get("ema"), h[e.get("group", 0)], h[3 + e.get("group", 0)], s,
                   ema_only=e.get("ema_only", False), **kw) for e in entries]


def scaled_err(got, ref, old, extra=None):
    """|got - ref| per element over the magnitudes that entered the result: |old| + |ref - old| (+ extra).  Never over the result alone: an
    updated value passes through zero, and a relative error there says nothing.  Equal values give 0 whatever the scale; a difference at
    scale 0 gives inf."""
    got, ref, old = (t.detach().double().reshape(-1).cpu() for t in (got, ref, old))
    scale = old.abs() + (ref - old).abs()
    if extra is not None:
        scale = scale + extra.detach().double().reshape(-1).cpu().abs()
    err = (got - ref).abs()
    out = err / scale
    out[err == 0] = 0.0
    out[torch.isnan(got) | torch.isnan(out)] = math.inf
    return out


def operand_extra(rule, e, s, ref):
    """the operand magnitudes of the two moments beyond |old| + |ref - old|: the gradient enters them as g * clip * scale + wd * p, two terms
    that may cancel in their sum while the float32 rounding of each stays.  m = |g| clip scale + wd |p| (AdamW: no decay term) enters
    `buf` as m (SGD), (1 - beta1) m (the lerp rules) or m / (sqrt(v) + eps) (RMSprop) and `sec` as (1 - beta2) m^2 (Adamax: m).
    e: the entry before the step; ref: update()'s result for it."""
    if e.get("g") is None or e.get("ema_only"):
        return {}
    h = s["hyper"]
    m = e["g"].detach().double().reshape(-1).cpu().abs() * (s["clip"] * h[11])
    if rule != 1:
        m = m + h[3 + e.get("group", 0)] * e["p"].detach().double().reshape(-1).cpu().abs()
    lr, eps = h[e.get("group", 0)], h[13]
    if rule == 0:
        out = {"buf": m}
        dp = lr * (1.0 + h[6] if h[10] else 1.0)
    elif rule == 6:
        out = {"buf": m / (ref[2].cpu().sqrt() + eps), "sec": h[15] * m * m}
        dp = lr
    else:
        out = {"buf": h[16] * m, "sec": m if rule == 3 else h[15] * m * m}
        v = ref[2].cpu()
        if rule in (1, 2):
            dp = lr * s["inv_bc1"] / (v.sqrt() / s["bc2_sqrt"] + eps)
        elif rule == 3:
            dp = lr * s["inv_bc1"] / v
        elif rule == 4:
            dp = lr * s["c1"] / ((v / s["c2"]).sqrt() + eps)
        else:
            dp = lr * s["inv_bc1"] * (s["c0"] * s["bc2_sqrt"] / (v.sqrt() + eps) if s["c1"] else 1.0)
    # the parameter moves by dp * buf (dp = |d p / d buf| of the rule): the magnitudes that entered buf enter p times dp
    b0 = e["buf"].detach().double().reshape(-1).cpu()
    out["p"] = dp * (b0.abs() + (ref[1].cpu() - b0).abs() + out["buf"])
    out["ema"] = s["ema_1md"] * out["p"]  # ... and the EMA takes (1 - d) of the new parameter
    return out


def errors(rule, e, s, ref, got):
    """{quantity: scaled_err per element} of got = (p, buf, sec, ema) against ref = update()'s result for entry e (None entries skipped)"""
    extra = operand_extra(rule, e, s, ref)
    return {q: scaled_err(g, r, e[q], extra.get(q)) for q, r, g in zip(QUANT, ref, got) if r is not None and g is not None}


def sumsq_exact(grads, gscale):
    """float64 sum of (g * scale)^2 over the gradients that exist"""
    return float(sum(((g.detach().double().cpu() * gscale) ** 2).sum() for g in grads if g is not None))


# ------------------------------------------------------------------------------------------------------------------------- the data
def make_data(n, seed):
    """-> {'p', 'g', 'buf', 'sec', 'ema'} float32, n elements: normal values; every 7th element (i % 7 == 3) carries a gradient and moments
    1e-8 times smaller (a dead unit: there eps decides the step) and every 11th gradient (i % 11 == 5) is exactly 0"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(n, generator=gen)  # noqa: E731
    p, g, buf, sec, ema = rn(), rn() * 0.3, rn() * 0.1, rn().square() * 0.05 + 1e-4, rn()
    i = torch.arange(n)
    tiny = i % 7 == 3
    g[tiny] *= 1e-8
    buf[tiny] *= 1e-8
    sec[tiny] *= 1e-16
    g[i % 11 == 5] = 0.0
    return {"p": p, "g": g, "buf": buf, "sec": sec, "ema": ema}


class Toy(nn.Module):
    """tensor lengths on every edge of the chunking (c = ymi_opt_chunk_elems), one view 4 bytes past a 16-byte boundary, a parameter that
    never receives a gradient, 450 three-element tensors (with the others more than YMI_OPT_MAX_GRADS: a second launch range) and a
    BatchNorm, whose running statistics are EMA-only entries"""

    def __init__(self, c, device="cuda:0"):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        mk = lambda n: nn.Parameter(torch.randn(n, generator=g).to(device))  # noqa: E731
        for k, n in enumerate((1, 7, c - 1, c, c + 1, 3 * c + 5)):
            setattr(self, f"w{k}", mk(n))
        base = torch.randn(1001, generator=g).to(device)
        self.odd = nn.Parameter(base[1:])          # a view: 4 bytes past a 16-byte boundary
        self.nograd = mk(9)                        # never receives a gradient
        self.small_bias = nn.ParameterList([mk(3) for _ in range(450)])  # group 0; with the others 458 tensors: a second launch range
        self.bn = nn.BatchNorm1d(37).to(device)    # weight: group 2; running_mean / running_var: EMA-only
        with torch.no_grad():
            for t in (self.bn.weight, self.bn.bias, self.bn.running_mean):
                t.copy_(torch.randn(37, generator=g))
            self.bn.running_var.copy_(torch.rand(37, generator=g) + 0.5)


# ---------------------------------------------------------------------------------------------------------------- the direct driver
GUARD = 8            # guard words between slices
POISON = 0x7FC0BEEF  # a NaN pattern


class Pool:
    """one device buffer filled with a NaN pattern; tensors are carved from it with guard words between them, each slice a chosen number
    of bytes past a 16-byte boundary"""

    def __init__(self, words, device):
        self.bits = torch.full((words,), POISON, dtype=torch.int32, device=device)
        self.f = self.bits.view(torch.float32)
        assert self.f.data_ptr() % 16 == 0
        self.cur = GUARD
        self.inside = torch.zeros(words, dtype=torch.bool)

    def take(self, values, off_bytes=0):
        assert off_bytes % 4 == 0 and 0 <= off_bytes < 16 and values.dtype == torch.float32
        n = values.numel()
        start = (self.cur + 3) // 4 * 4 + off_bytes // 4
        assert start + n + GUARD <= self.bits.numel(), "pool too small"
        t = self.f[start:start + n]
        t.copy_(values.reshape(-1))
        self.inside[start:start + n] = True
        self.cur = start + n + GUARD
        assert t.data_ptr() % 16 == off_bytes
        return t

    def snapshot(self):
        return self.bits.clone()

    def outside_unchanged(self, snap):
        """guard words and every pool byte outside the slices keep their bits"""
        m = (~self.inside).to(self.bits.device)
        return torch.equal(self.bits[m], snap[m]) and bool((self.bits[m] == POISON).all())


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def build_table(entries, chunk, device):
    """entries: [{'p', 'buf', 'ema', 'sec', 'acc': tensors or None, 'numel', 'group'}] -> (OptEntry table, chunk map, first chunk of each entry
    (+ the total)) on the device"""
    from improving_yolov8_cbam_swinblock_amd._lib import OptEntry

    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    tab = (OptEntry * len(entries))()
    cmap, first = [], []
    for i, e in enumerate(entries):
        tab[i] = OptEntry(ptr(e.get("p")), ptr(e.get("buf")), ptr(e.get("ema")), e["numel"], e.get("group", 0), 0, ptr(e.get("sec")), ptr(e.get("acc")))
        first.append(len(cmap))
        cmap.extend((i, c) for c in range((e["numel"] + chunk - 1) // chunk))
    first.append(len(cmap))
    table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(device)
    return table, torch.tensor(cmap, dtype=torch.int32).reshape(-1, 2).contiguous().to(device), first


def launch_ranges(first, lo, hi):
    """[(first tensor, n tensors, first chunk, n chunks)] over entries lo..hi, at most YMI_OPT_MAX_GRADS tensors per launch"""
    from improving_yolov8_cbam_swinblock_amd._lib import OPT_MAX_GRADS

    return [(a, min(a + OPT_MAX_GRADS, hi) - a, first[a], first[min(a + OPT_MAX_GRADS, hi)] - first[a]) for a in range(lo, hi, OPT_MAX_GRADS)]


def _grad_array(grads, a, n):
    arr = (ctypes.c_void_p * n)()
    for i in range(n):
        if grads[a + i] is not None:
            arr[i] = grads[a + i].data_ptr()
    return arr


def launch_norm(table, cmap, first, grads, hyper, partials, state, n_grad, finalize=True):
    """ymi_opt_grad_norm over entries 0..n_grad in launch ranges; finalize is requested on the last call only"""
    from improving_yolov8_cbam_swinblock_amd import _lib

    vp = ctypes.c_void_p
    rs = launch_ranges(first, 0, n_grad)
    for k, (a, n, c0, nc) in enumerate(rs):
        _lib.check(_lib.lib().ymi_opt_grad_norm(vp(table.data_ptr()), vp(cmap.data_ptr() + c0 * 8), a, n, nc, _grad_array(grads, a, n), vp(hyper.data_ptr()),
                                                vp(partials.data_ptr()), c0, first[n_grad], vp(state.data_ptr()),
                                                1 if finalize and k == len(rs) - 1 else 0, _lib.stream_ptr()), "opt_grad_norm")
    return rs


def launch_update(table, cmap, first, grads, hyper, state, rule, lo, hi):
    """ymi_opt_update over entries lo..hi; grads None: the EMA-only mode (host_grads null)"""
    from improving_yolov8_cbam_swinblock_amd import _lib

    vp = ctypes.c_void_p
    rs = launch_ranges(first, lo, hi)
    for a, n, c0, nc in rs:
        _lib.check(_lib.lib().ymi_opt_update(vp(table.data_ptr()), vp(cmap.data_ptr() + c0 * 8), a, n, nc, _grad_array(grads, a, n) if grads is not None else None,
                                             vp(hyper.data_ptr()), vp(state.data_ptr()), rule, _lib.stream_ptr()), "opt_update")
    return rs


def launch_accumulate(table, cmap, first, grads, lo, hi):
    from improving_yolov8_cbam_swinblock_amd import _lib

    vp = ctypes.c_void_p
    rs = launch_ranges(first, lo, hi)
    for a, n, c0, nc in rs:
        _lib.check(_lib.lib().ymi_opt_grad_accumulate(vp(table.data_ptr()), vp(cmap.data_ptr() + c0 * 8), a, n, nc, _grad_array(grads, a, n), _lib.stream_ptr()),
                   "opt_grad_accumulate")
    return rs


def state_to_device(s, device):
    return torch.frombuffer(bytearray(pack_state(s)), dtype=torch.uint8).to(device)


def state_from_device(t):
    return unpack_state(t.cpu().numpy().tobytes())


# ------------------------------------------------------------------------------------------------- checks shared by the GPU tests
def bound(rule, q):
    return MARGIN * F32_DISTANCE[RULES[rule]][q]


def record_mismatches(dev, s, rule):
    """the device's state record against scalars() evaluated on the same inputs -> list of mismatches (empty: agreement).  `updates`, `steps`
    and `mu_product` are exact, `clip` is exact given the device's `norm` (s must have been evaluated with norm=dev['norm']), every other
    float is within 1 float32 ulp: the device's double exp / pow / sqrt may differ from the host's in the last place."""
    bad = [(k, dev[k], s[k]) for k in ("updates", "steps", "clip", "norm") if dev[k] != s[k]]
    if rule == 4 and dev["mu_product"] != s["mu_product"]:
        bad.append(("mu_product", dev["mu_product"], s["mu_product"]))
    for k in ("ema_d", "ema_1md", "inv_bc1", "bc2_sqrt", "c0", "c1", "c2", "c3"):
        if ulps32(dev[k], s[k]) > 1:
            bad.append((k, dev[k], s[k]))
    return bad


def _flat_host(ts):
    """[device tensors or None] -> [flat float32 CPU tensors or None] with one device-to-host copy"""
    have = [t for t in ts if t is not None]
    if not have:
        return [None] * len(ts)
    flat = torch.cat([t.detach().reshape(-1) for t in have]).cpu()
    parts = iter(flat.split([t.numel() for t in have]))
    return [None if t is None else next(parts) for t in ts]


def class_entries(opt, grads=None):
    """the tensors of a built FusedSGD-family optimizer as entries of restate_step, copied to the host.  grads: {parameter: gradient}"""
    ents = opt._entries
    cols = {"p": [e[0] for e in ents], "buf": [e[1] for e in ents], "ema": [e[2] for e in ents],
            "sec": [opt.second[i] if opt.RULE and i < opt.n_sgd else None for i in range(len(ents))],
            "g": [grads.get(e[0]) if grads is not None and i < opt.n_sgd else None for i, e in enumerate(ents)]}
    cols = {k: _flat_host(v) for k, v in cols.items()}
    return [{"p": cols["p"][i], "buf": cols["buf"][i], "ema": cols["ema"][i], "sec": cols["sec"][i], "g": cols["g"][i], "group": e[3],
             "ema_only": i >= opt.n_sgd} for i, e in enumerate(ents)]


def class_before(opt, grads):
    """call before opt.step(grads): -> what class_after needs"""
    if opt._stale():
        opt._build()
    opt.sync_hyper()
    torch.cuda.synchronize()
    return {"entries": class_entries(opt, grads), "state": state_from_device(opt._state)}


def class_after(opt, before, worst=None):
    """call after opt.step(): the device's record against scalars() on the device's own partial sums, and every element of every parameter,
    moment and EMA tensor against update() from the state before the step, each within MARGIN * F32_DISTANCE.  -> scalars()"""
    torch.cuda.synchronize()
    rule = int(opt.RULE)
    hyper = [float(v) for v in opt._hyper.cpu().tolist()]
    dev = state_from_device(opt._state)
    grads = [e["g"] for e in before["entries"]]
    exact = sumsq_exact(grads, hyper[11])
    got_sum = float(opt._partials.double().sum())
    assert abs(got_sum - exact) <= 27 * 2.0 ** -24 * exact, (got_sum, exact)
    s = scalars(hyper, before["state"], got_sum, norm=dev["norm"])
    assert ulps32(dev["norm"], f32(math.sqrt(got_sum))) <= 1
    assert not record_mismatches(dev, s, rule), record_mismatches(dev, s, rule)
    res = restate_step(rule, hyper[10] != 0.0, before["entries"], s)
    after = class_entries(opt)
    for i, (e, r, a) in enumerate(zip(before["entries"], res, after)):
        if e["g"] is None:  # no gradient: parameter and moments keep their bits
            assert all(a[q] is None or bits_equal(a[q], e[q]) for q in ("p", "buf", "sec")), i
        for q, err in errors(rule, e, s, r, (a["p"], a["buf"], a["sec"], a["ema"])).items():
            err = float(err.max())
            if worst is not None:
                worst[q] = max(worst.get(q, 0.0), err)
            assert err <= bound(rule, q), (RULES[rule], "entry", i, e["p"].numel(), q, err, bound(rule, q))
    return s
