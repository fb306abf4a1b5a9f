"""CPU: the float64 restatement of the optimizer step (tests/optim_exact.py) is checked before anything is measured against it.

  * It reproduces torch.optim.{SGD, AdamW, Adam, Adamax, NAdam, RAdam, RMSprop} (foreach=False) with clip_grad_norm_ and the oracle's
    ModelEMA.update on float64 CPU parameters over 8 steps, to float64 rounding: learning rates and betas change between steps, groups with
    and without weight decay, a parameter without a gradient, the clip on and off, RAdam's rectification switching on inside the run,
    NAdam's mu_product equal to torch's own state tensor.
  * Float32 torch.optim is measured against it, one step at a time from a shared float32 state; the printed figures
    (optim_exact.F32_DISTANCE holds them, rounded up) are what the bounds of tests/test_gpu_optim_exact.py rest on.
  * A plain per-element relative error is useless for that comparison, and scaled_err is not: shown.
  * Each planted fault moves a named quantity of a named case beyond the bound the GPU test uses."""
import math
from pathlib import Path

import pytest
import torch
import torch.nn as nn

import optim_exact as X
from oracle.trainer import ModelEMA, build_optimizer, optimizer_step

STEPS = 8
NAMES = {0: "SGD", 1: "AdamW", 2: "Adam", 3: "Adamax", 4: "NAdam", 5: "RAdam", 6: "RMSProp"}  # oracle.trainer.build_optimizer's names
STATE_KEYS = {0: ("momentum_buffer", None), 1: ("exp_avg", "exp_avg_sq"), 2: ("exp_avg", "exp_avg_sq"), 3: ("exp_avg", "exp_inf"),
              4: ("exp_avg", "exp_avg_sq"), 5: ("exp_avg", "exp_avg_sq"), 6: ("momentum_buffer", "square_avg")}
DECAY = 5e-4


class HostModel(nn.Module):
    """the reference's three groups: 'bias' in the name (no decay), plain weights (decay), norm weights (no decay); a parameter that never
    receives a gradient; BatchNorm running statistics as EMA-only entries"""

    def __init__(self, n=20000):
        super().__init__()
        d = X.make_data(n, 1)
        self.w = nn.Parameter(d["p"].clone())
        self.head_bias = nn.Parameter(X.make_data(n // 4, 2)["p"])
        self.frozen = nn.Parameter(X.make_data(64, 3)["p"])
        self.bn = nn.BatchNorm1d(n // 8)
        with torch.no_grad():
            self.bn.weight.copy_(X.make_data(n // 8, 4)["p"])
            self.bn.bias.copy_(X.make_data(n // 8, 5)["p"])


def group_of(name):
    return 0 if "bias" in name else 2 if name == "bn.weight" else 1


def schedule(rule, k):
    """learning rates (one per group), beta1 / momentum and beta2 / alpha of step k: they change between steps"""
    base = 0.01 if rule in (0, 6) else 0.002
    lr = [base * (1.0 + 0.1 * k), base * (0.5 + 0.05 * k), base * 2.0 / (1 + k)]
    b1 = (0.937 if rule in (0, 6) else 0.9) - (0.01 if k >= 3 else 0.0)
    b2 = (0.99 if rule == 6 else 0.999) - (0.001 if k >= 6 else 0.0)
    return lr, b1, b2


def apply_schedule(opt, rule, k):
    lr, b1, b2 = schedule(rule, k)
    for grp, v in zip(opt.param_groups, lr):
        grp["lr"] = v
        grp["foreach"] = False
        if rule in (0, 6):
            grp["momentum"] = b1
            if rule == 6:
                grp["alpha"] = b2
        else:
            grp["betas"] = (b1, b2)
    return lr, b1, b2


def set_grads(model, k, dtype):
    """gradients of step k (none for `frozen`); odd steps are small, so that the clip is off there; BatchNorm's statistics move"""
    out = {}
    for i, (n, p) in enumerate(model.named_parameters()):
        if n == "frozen":
            continue
        g = X.make_data(p.numel(), 100 + 10 * k + i)["g"] * (0.01 if k % 2 else 1.0)
        p.grad = g.to(dtype).clone()  # (clip_grad_norm_ scales p.grad in place: the caller keeps the unclipped values)
        out[n] = g
    with torch.no_grad():
        model.bn.running_mean.add_(X.make_data(model.bn.num_features, 200 + k)["g"].to(dtype))
    return out


def entries_of(model, opt, ema, rule, grads):
    """the model's float state as entries of restate_step, read from the model, torch's optimizer state and the EMA copy"""
    kb, ks = STATE_KEYS[rule]
    esd = ema.ema.state_dict()
    out = {}
    for n, p in model.named_parameters():
        st = opt.state.get(p, {})
        buf = st.get(kb)
        out[n] = {"p": p.detach().clone(), "g": grads.get(n), "buf": torch.zeros_like(p) if buf is None else buf.detach().clone(),
                  "sec": None if ks is None else (torch.zeros_like(p) if ks not in st else st[ks].detach().clone()), "ema": esd[n].clone(), "group": group_of(n)}
    for n, b in model.named_buffers():
        if b.dtype.is_floating_point:
            out[n] = {"p": b.detach().clone(), "ema": esd[n].clone(), "ema_only": True}
    return out


def after_of(model, opt, ema, rule):
    kb, ks = STATE_KEYS[rule]
    esd = ema.ema.state_dict()
    out = {}
    for n, p in model.named_parameters():
        st = opt.state.get(p, {})
        out[n] = (p.detach(), st.get(kb), st.get(ks) if ks else None, esd[n])
    for n, b in model.named_buffers():
        if b.dtype.is_floating_point:
            out[n] = (b.detach(), None, None, esd[n])
    return out


def hyper_of(rule, lr, b1, b2, round32, gscale=1.0):
    wd = (0.0, DECAY, 0.0)
    return X.hyper_vector(rule, lr, wd, b1, nesterov=rule == 0, beta2=b2, gscale=gscale, round32=round32)


# ------------------------------------------------------------------------------------------------- the restatement against torch.optim
@pytest.mark.parametrize("rule", sorted(X.RULES))
def test_restatement_reproduces_torch_optim_in_float64(rule):
    model = HostModel(4000).double()
    opt = build_optimizer(model, lr=0.01, momentum=0.9, decay=DECAY, name=NAMES[rule])
    ema = ModelEMA(model)
    state = X.zero_state()
    carried = None
    worst, rectified = 0.0, []
    for k in range(STEPS):
        lr, b1, b2 = apply_schedule(opt, rule, k)
        grads = set_grads(model, k, torch.float64)
        # torch sees the mean over two ranks; the restatement gets their sum and the scale 0.5
        entries = entries_of(model, opt, ema, rule, {n: g.double() * 2.0 for n, g in grads.items()})
        if carried is not None:  # the restatement carries its own float64 state through the run (a buffer's value is the model's)
            for n, e in entries.items():
                for q, v in zip(X.QUANT, carried[n]):
                    if v is not None and q in e and not (q == "p" and e.get("ema_only")):
                        e[q] = v
        s = X.scalars(hyper_of(rule, lr, b1, b2, False, gscale=0.5), state, X.sumsq_exact([e.get("g") for e in entries.values()], 0.5), round32=False)
        norm = optimizer_step(model, opt, ema)
        assert abs(float(norm) - s["norm"]) <= 1e-13 * s["norm"]
        assert (s["clip"] < 1.0) == (k % 2 == 0), (k, s["norm"])
        names = list(entries)
        res = X.restate_step(rule, rule == 0, [entries[n] for n in names], s)
        got = after_of(model, opt, ema, rule)
        for n, r in zip(names, res):
            if n == "frozen":  # torch has no state for a parameter that never had a gradient
                assert got[n][1] is None and float(r[1].abs().max()) == 0.0
            for q, err in X.errors(rule, entries[n], s, r, got[n]).items():
                err = float(err.max())
                worst = max(worst, err)
                # float64 rounding: 2^-53 a rounding, a dozen roundings a step, 8 steps of carried state, and on the dead units
                # (make_data) a quotient g / (sqrt(v) + eps) that amplifies the error of v some tenfold
                assert err <= 1e-12, (X.RULES[rule], k, n, q, err)
        if rule == 4:
            assert s["mu_product"] == float(opt.state[model.w]["mu_product"]), k
        if rule == 5:
            rectified.append(s["c1"])
        assert s["steps"] == k + 1 == s["updates"] == ema.updates
        carried = dict(zip(names, res))
        state = {k2: v for k2, v in s.items() if k2 != "hyper"}
    if rule == 5:
        assert rectified[:5] == [0.0] * 5 and rectified[5:] == [1.0] * 3  # the rectification switches on inside the run
    print(f"[optim restatement] {X.RULES[rule]}: worst scaled error against float64 torch.optim over {STEPS} steps {worst:.1e}")


def test_scalars_follow_clip_grad_norm_and_model_ema():
    """the record's norm / clip against torch.nn.utils.clip_grad_norm_ and its EMA decay against oracle.trainer.ModelEMA, in float64"""
    g = [X.make_data(n, 7 + n)["g"].double() for n in (5, 4097, 300)]
    for scale, max_norm in ((1.0, 10.0), (1e-3, 10.0), (1.0, 0.5), (0.0, 10.0)):
        ps = [nn.Parameter(torch.zeros_like(t)) for t in g]
        for p, t in zip(ps, g):
            p.grad = t * scale
        before = [p.grad.clone() for p in ps]
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm=max_norm)
        h = X.hyper_vector(0, (0.01,) * 3, (0.0,) * 3, 0.9, max_norm=max_norm, gscale=scale, round32=False)
        s = X.scalars(h, X.zero_state(), X.sumsq_exact(g, scale), round32=False)
        assert abs(s["norm"] - float(norm)) <= 1e-14 * max(float(norm), 1e-300)
        assert (s["clip"] < 1.0) == (float(norm) > max_norm)
        for p, b in zip(ps, before):
            assert float((p.grad - b * s["clip"]).abs().max()) <= 1e-15 * max(float(b.abs().max()), 1e-300)
    assert X.scalars(X.hyper_vector(0, (0.01,) * 3, (0.0,) * 3, 0.9, max_norm=0.0), X.zero_state(), 1e6)["clip"] == 1.0
    m = nn.Linear(3, 2).double()
    for tau, updates in ((2000.0, 0), (2000.0, 1999), (50.0, 7)):
        ema = ModelEMA(m, decay=0.9999, tau=tau, updates=updates)
        s = X.scalars(X.hyper_vector(0, (0.01,) * 3, (0.0,) * 3, 0.9, tau=tau, round32=False), X.zero_state(updates=updates), 0.0, round32=False)
        assert s["ema_d"] == ema.decay(updates + 1) and s["ema_1md"] == 1 - ema.decay(updates + 1) and s["updates"] == updates + 1


def test_radam_guard():
    X.radam_guard(0.999, range(1, 20))
    X.radam_guard(0.998, range(1, 20))
    assert X.radam_rho(0.999, 5)[0] < 5.0 < X.radam_rho(0.999, 6)[0]
    with pytest.raises(AssertionError):
        X.radam_guard(0.9999, [5])  # rho_5 -> 5 from below as beta2 -> 1: 4.9996 here, a step count no test may use with this beta2


# ------------------------------------------------------------------------------------------------------ float32 torch.optim, measured
_measured = {}


def measured(rule):
    """worst scaled_err per quantity of float32 torch.optim (+ clip_grad_norm_ + ModelEMA) against the restatement, each step from the
    float32 run's own state"""
    if rule in _measured:
        return _measured[rule]
    model = HostModel()
    opt = build_optimizer(model, lr=0.01, momentum=0.9, decay=DECAY, name=NAMES[rule])
    ema = ModelEMA(model)
    worst = dict.fromkeys(X.QUANT, 0.0)
    plain = 0.0
    for k in range(STEPS):
        lr, b1, b2 = apply_schedule(opt, rule, k)
        grads = set_grads(model, k, torch.float32)
        entries = entries_of(model, opt, ema, rule, grads)
        st = opt.state.get(model.w, {})
        state = X.zero_state(updates=k, steps=k, mu_product=float(st["mu_product"]) if "mu_product" in st else 0.0)
        norm = optimizer_step(model, opt, ema)
        s = X.scalars(hyper_of(rule, lr, b1, b2, True), state, X.sumsq_exact(grads.values(), 1.0), norm=float(norm))
        assert X.ulps32(s["norm"], X.f32(math.sqrt(X.sumsq_exact(grads.values(), 1.0)))) <= 8
        names = list(entries)
        res = X.restate_step(rule, rule == 0, [entries[n] for n in names], s)
        got = after_of(model, opt, ema, rule)
        for n, r in zip(names, res):
            for q, err in X.errors(rule, entries[n], s, r, got[n]).items():
                worst[q] = max(worst[q], float(err.max()))
            plain = max(plain, float(((got[n][0].double() - r[0]).abs() / r[0].abs()).max()))
    _measured[rule] = (worst, plain)
    return _measured[rule]


@pytest.mark.parametrize("rule", sorted(X.RULES))
def test_f32_distance_is_what_is_recorded(rule):
    worst, plain = measured(rule)
    rec = X.F32_DISTANCE[X.RULES[rule]]
    print(f"[optim f32 distance] {X.RULES[rule]:8s} " + "  ".join(f"{q} {worst[q]:.2e} (recorded {rec[q]:.1e})" for q in X.QUANT)
          + f"   plain relative error of p {plain:.1e}")
    for q in X.QUANT:
        if rule == 0 and q == "sec":
            assert worst[q] == 0.0 == rec[q]
            continue
        assert worst[q] <= rec[q] <= 2.0 * worst[q], (X.RULES[rule], q, worst[q], rec[q])


def test_plain_relative_error_is_useless_here():
    """updated parameters pass through zero: by per-element relative error float32 SGD lies a hundred times further from float64 than by
    scaled_err, and how far is a matter of how close to zero one of 28 000 values happens to land"""
    worst, plain = measured(0)
    assert plain > 50 * worst["p"] and worst["p"] < 1e-7, (plain, worst)
    assert float(X.scaled_err(torch.tensor([1.0, 0.0]), torch.tensor([1.0, 0.0]), torch.tensor([0.0, 0.0])).max()) == 0.0
    assert math.isinf(float(X.scaled_err(torch.tensor([1e-30]), torch.tensor([0.0]), torch.tensor([0.0])).max()))
    assert math.isinf(float(X.scaled_err(torch.tensor([math.nan]), torch.tensor([1.0]), torch.tensor([1.0])).max()))


# -------------------------------------------------------------------------------------------------------------------- planted faults
# fault -> (rule, quantity it must move, keyword arguments of the case)
FAULTS = {
    "nesterov_dropped": (0, "p", {}),
    "decay_in_undecayed_group": (0, "buf", {}),
    "adamw_decay_on_gradient": (1, "buf", {}),
    "clip_without_scale": (0, "buf", {"gscale": 0.5}),
    "bias_correction_t_minus_1": (2, "p", {"steps": 3}),
    "eps_inside_the_quotient": (1, "p", {}),
    "adamax_eps_outside_max": (3, "sec", {}),
    "nadam_mu_next_is_mu": (4, "p", {"steps": 3}),
    "radam_one_step_early": (5, "p", {"steps": 4}),
    "rmsprop_momentum_after_quotient": (6, "buf", {}),
    "ema_of_old_parameter": (0, "ema", {}),
    "ema_updates_minus_1": (0, "ema", {}),
    "last_element_unchanged": (0, "p", {}),
    "element_after_chunk_boundary_twice": (0, "p", {}),
}


def fault_case(rule, fault=None, gscale=1.0, steps=0):
    """the update-kernel case of the GPU test: three groups, a tensor of one chunk and a tail, a planted state record"""
    n = X.CHUNK + 37
    assert (n - 1) % 7 != 3 and X.CHUNK % 7 != 3 and (n - 1) % 11 != 5 and X.CHUNK % 11 != 5  # neither watched element is a dead or zero-gradient one
    base = 0.01 if rule in (0, 6) else 0.002
    h = X.hyper_vector(rule, (base, 0.5 * base, 2 * base), (0.0, DECAY, 0.0), 0.937 if rule in (0, 6) else 0.9, nesterov=rule == 0,
                       beta2=0.99 if rule == 6 else 0.999, gscale=gscale)
    entries = []
    for grp in range(3):
        d = X.make_data(n, 40 + grp)
        if rule == 0:
            d["sec"] = None
        entries.append({**d, "group": grp})
    s = X.scalars(h, X.zero_state(steps=steps, updates=steps, mu_product=0.43), X.sumsq_exact([e["g"] for e in entries], gscale), fault=fault)
    return entries, s, X.restate_step(rule, rule == 0, entries, s, fault=fault)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_fault_is_beyond_the_gpu_bound(fault):
    rule, q, kw = FAULTS[fault]
    entries, s, clean = fault_case(rule, **kw)
    bad = fault_case(rule, fault=fault, **kw)[2]
    moved = max(float(X.errors(rule, e, s, c, b)[q].max()) for e, c, b in zip(entries, clean, bad))
    bound = X.MARGIN * X.F32_DISTANCE[X.RULES[rule]][q]
    print(f"[optim fault] {fault}: {X.RULES[rule]} {q} moves by {moved:.1e} (GPU bound {bound:.1e})")
    assert moved > 2.0 * bound, (fault, moved, bound)


def test_update_body_is_built_with_its_own_contraction():
    """vector path, tail and scalar path of opt_update_kernel round alike only while the one element body states its fused multiply-adds itself
    and the build honours its contract(off) pragma (the GPU test holds the paths to bit equality; this holds the build to what that needs)"""
    csrc = Path(__file__).resolve().parents[1] / "improving_yolov8_cbam_swinblock_amd" / "csrc"
    assert "FLAGS_optim := -ffp-contract=fast-honor-pragmas" in (csrc / "Makefile").read_text()
    src = (csrc / "optim.hip").read_text()
    # the body: the scalar overload of opt_update, up to the float4 overload that calls it four times
    body = src[src.index("Updated<float> opt_update(const StepScalars& k"):src.index("Updated<f32x4> opt_update(const StepScalars& k")]
    assert body.index("{") < body.index("#pragma clang fp contract(off)") < body.index("fmaf(")  # the pragma heads the compound statement
    assert "#pragma clang fp contract(off)" in body and "o.ema = fmaf(ev, k.d, k.omd * o.p);" in body
    assert src.count("fmaf(ev,") == 1 and src.count("k.omd *") == 1  # the EMA line is defined once: no path has a copy to drift


@pytest.mark.parametrize("rule", sorted(X.RULES))
def test_host_hyper_values_follow_the_layout_of_the_restatement(rule):
    """engine/optim.py::hyper_values (built by field name, in the order of optim.hip's enum Hyper) against optim_exact.hyper_vector (built by
    index): the two statements of the 20-float layout agree for every class, with a distinct lr and weight decay in every group.  No device:
    the optimizers build no tables before their first step."""
    from improving_yolov8_cbam_swinblock_amd.engine import optim as O

    model = X.Toy(X.CHUNK, "cpu")
    ema = O.ModelEMA(model, decay=0.9995, tau=1500)
    common = {"decay": 5e-4, "max_norm": 7.0, "ema": ema}
    adam = {"betas": (0.91, 0.9985), "eps": 3e-8, **common}
    opt = {0: lambda: O.FusedSGD(model, lr=0.01, momentum=0.93, nesterov=True, **common), 1: lambda: O.FusedAdamW(model, lr=0.002, **adam),
           2: lambda: O.FusedAdamW(model, lr=0.002, decoupled=False, **adam), 3: lambda: O.FusedAdamax(model, lr=0.002, **adam),
           4: lambda: O.FusedNAdam(model, lr=0.002, momentum_decay=3e-3, **adam), 5: lambda: O.FusedRAdam(model, lr=0.002, **adam),
           6: lambda: O.FusedRMSprop(model, lr=0.01, momentum=0.93, alpha=0.985, eps=3e-8, **common)}[rule]()
    assert opt.RULE == rule and opt._table is None
    lr, wd = (0.011, 0.0052, 0.023), (1e-5, 5e-4, 2e-4)
    for grp, a, b in zip(opt.param_groups, lr, wd):
        grp["lr"], grp["weight_decay"] = a, b
    opt.world = 4
    beta1, beta2 = (0.93, 0.985 if rule == 6 else 0.999) if rule in (0, 6) else (0.91, 0.9985)
    want = X.hyper_vector(rule, lr, wd, beta1, max_norm=7.0, ema_decay=0.9995, tau=1500.0, nesterov=rule == 0, gscale=0.25, beta2=beta2, eps=3e-8,
                          momentum_decay=3e-3, round32=False)
    got = opt.hyper_values()
    assert len(got) == 20 == len(O.HYPER_FIELDS) + 4 and all(type(v) is float for v in got)
    if rule == 4:  # the float32 tails of beta1 and momentum_decay, which hyper_vector leaves 0 without round32
        assert got[18:] == [0.91 - X.f32(0.91), 3e-3 - X.f32(3e-3)] and all(got[18:])
        got = got[:18] + [0.0, 0.0]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert opt._table is None  # (nothing was built, nothing touched a device)
