"""GPU: the three kernels of csrc/optim.hip, called directly through ymi_opt_grad_norm / ymi_opt_update / ymi_opt_grad_accumulate on tables
of the test's own and through the optimizer classes, against the float64 restatement tests/optim_exact.py, element by element.

Bounds: per rule and quantity MARGIN (4) times the distance of float32 torch.optim from the restatement (optim_exact.F32_DISTANCE, measured
by tests/test_host_optim_check.py), in the scale of optim_exact.scaled_err / operand_extra.  Per-chunk sums of squares: every term is
non-negative, so the relative error is at most the number of roundings on the longest summation path times 2^-24 (SUMSQ_ROUNDINGS)."""
import pytest
import torch

import optim_exact as X

pytestmark = pytest.mark.gpu

# opt_sumsq_kernel, one chunk of 4096: a term (g * gs) * (g * gs) carries 3 roundings (g * gs enters twice, the product once).
#   vector path: 3 additions inside the four-term expression, 4 `acc +=` (a thread makes 4 trips), 6 shuffle rounds, 2 for the four waves: 18
#   scalar path (gradient off a 16-byte boundary): 16 `acc +=` (16 trips of one element), 6 shuffle rounds, 2 for the four waves:          27
SUMSQ_ROUNDINGS = {True: 18, False: 27}


def dev():
    return torch.device("cuda:0")


def chunk():
    from improving_yolov8_cbam_swinblock_amd import _lib

    c = int(_lib.lib().ymi_opt_chunk_elems())
    assert c == X.CHUNK
    return c


def lengths():
    c = chunk()
    return (1, 3, 4, 5, 1023, 1024, 1025, c - 1, c, c + 1, 3 * c + 5)


def host(pool_host, t):
    """the slice of the pool's host copy that device slice t occupies"""
    return pool_host[t.storage_offset():t.storage_offset() + t.numel()]


_worst = {}


def note(kind, label, errs):
    w = _worst.setdefault((kind, label), {})
    for q, v in errs.items():
        w[q] = max(w.get(q, 0.0), v)


def report(kind, label, rule):
    w = _worst.get((kind, label), {})
    print(f"[optim exact] {kind:8s} {label:20s} " + "  ".join(f"{q} {w[q]:.2e} / {X.bound(rule, q):.1e}" for q in X.QUANT if q in w))


# ---------------------------------------------------------------------------------------------------------------- norm and state
def norm_case(name):
    """-> (gradient values per entry (None: no gradient), byte offset per gradient, hyper kwargs, state_in kwargs, rule)"""
    gs = [X.make_data(n, 300 + i)["g"] for i, n in enumerate(lengths())]
    gs.insert(5, None)  # an entry with a null gradient between entries that have one
    off = [0] * len(gs)
    kw, st, rule = {}, {}, 0
    if name == "clip_inactive":
        gs = [None if g is None else g * 1e-3 for g in gs]
    elif name == "max_norm_0":
        kw = {"max_norm": 0.0}
    elif name == "zero_gradients":
        gs = [None if g is None else torch.zeros_like(g) for g in gs]
    elif name == "scale_half":
        kw = {"gscale": 0.5}
    elif name == "misaligned":
        off = [4 * (1 + i % 3) for i in range(len(gs))]
    elif name == "updates_below_tau":
        st = {"updates": 1999}
    elif name == "radam_crosses_switch":
        st, rule = {"steps": 5}, 5
    elif name == "radam_before_switch":
        st, rule = {"steps": 4}, 5
    elif name == "two_ranges":
        gs = gs[:6] + [X.make_data(3, 400 + i)["g"] for i in range(450)] + gs[6:]
        off = [0] * len(gs)
    else:
        assert name == "clip_active"
    return gs, off, kw, st, rule


NORM_CASES = ("clip_active", "clip_inactive", "max_norm_0", "zero_gradients", "scale_half", "misaligned", "updates_below_tau", "radam_before_switch",
              "radam_crosses_switch", "two_ranges")


@pytest.mark.parametrize("name", NORM_CASES)
def test_norm_partials_and_state_record(name):
    c = chunk()
    values, off, kw, st, rule = norm_case(name)
    pool = X.Pool(sum(v.numel() + 16 for v in values if v is not None) + 4096, dev())
    grads = [None if v is None else pool.take(v, o) for v, o in zip(values, off)]
    numel = [v.numel() if v is not None else 1025 for v in values]
    table, cmap, first = X.build_table([{"numel": n} for n in numel], c, dev())
    partials = pool.take(torch.full((first[-1],), 123.0))
    h = X.hyper_vector(rule, (0.01, 0.02, 0.03), (0.0, 5e-4, 0.0), 0.9, **kw)
    state_in = X.zero_state(inv_bc1=7.5, bc2_sqrt=8.5, c0=1.25, c1=2.25, c2=3.25, c3=4.25, mu_product=0.43, clip=9.0, norm=9.0, **st)
    hyper, state = torch.tensor(h, dtype=torch.float32, device=dev()), X.state_to_device(state_in, dev())
    snap = pool.snapshot()
    rs = X.launch_norm(table, cmap, first, grads, hyper, partials, state, len(grads))
    torch.cuda.synchronize()
    assert len(rs) == (2 if name == "two_ranges" else 1) and (name != "two_ranges" or (rs[1][0] == 448 and rs[1][2] > 0))
    ph = pool.f.cpu()
    got = host(ph, partials).double()
    gscale = h[11]
    worst = 0.0
    for i, g in enumerate(values):
        for k in range(first[i], first[i + 1]):
            if g is None:
                assert float(got[k]) == 0.0, (i, k)  # chunks of entries with a null gradient are exactly 0
                continue
            ref = float(((g[(k - first[i]) * c:(k - first[i] + 1) * c].double() * gscale) ** 2).sum())
            err = abs(float(got[k]) - ref) / ref if ref else abs(float(got[k]))
            worst = max(worst, err)
            assert err <= SUMSQ_ROUNDINGS[off[i] == 0] * 2.0 ** -24, (name, i, numel[i], k, float(got[k]), ref)
    now, lo = pool.bits.clone(), partials.storage_offset()  # gradients are never written, nor is anything else outside the partial sums
    now[lo:lo + partials.numel()] = snap[lo:lo + partials.numel()]
    assert torch.equal(now, snap)
    d = X.state_from_device(state)
    s = X.scalars(h, state_in, float(got.sum()), norm=d["norm"])
    assert X.ulps32(d["norm"], X.f32(float(got.sum()) ** 0.5)) <= 1
    assert not X.record_mismatches(d, s, rule), X.record_mismatches(d, s, rule)
    assert d["updates"] == state_in["updates"] + 1 and d["steps"] == state_in["steps"] + 1  # finalize ran once, on the last call
    if name in ("clip_active", "misaligned", "two_ranges", "scale_half"):
        assert d["clip"] < 1.0
    if name == "scale_half":
        full = X.sumsq_exact(values, 1.0) ** 0.5
        assert abs(d["norm"] - 0.5 * full) <= 1e-6 * full and abs(d["clip"] - 10.0 / (0.5 * full)) <= 1e-6 * d["clip"]
    if name in ("clip_inactive", "max_norm_0", "zero_gradients"):
        assert d["clip"] == 1.0 and (name != "zero_gradients" or d["norm"] == 0.0) and (name != "max_norm_0" or d["norm"] > 10.0)
    if name == "updates_below_tau":
        assert d["updates"] == 2000 and 0.63 < d["ema_d"] < 0.6322  # decay * (1 - 1 / e)
    if rule == 5:
        assert (d["c1"], d["c0"] != 1.0) == ((1.0, True) if name == "radam_crosses_switch" else (0.0, False))
    else:
        assert (d["inv_bc1"], d["bc2_sqrt"], d["c0"], d["c1"], d["c2"], d["c3"], d["mu_product"]) == (7.5, 8.5, 1.25, 2.25, 3.25, 4.25, 0.43)  # SGD writes none
    print(f"[optim exact] sumsq {name}: worst relative error of a chunk {worst:.2e} (bound {SUMSQ_ROUNDINGS[off[0] == 0] * 2.0 ** -24:.2e})")


@pytest.mark.parametrize("rule", sorted(X.RULES))
def test_state_record_over_consecutive_finalize_launches(rule):
    """14 launches from a zero record: every scalar of every rule against scalars() fed its own previous record; NAdam's mu_product is bit-equal
    to the float32 running product throughout"""
    c = chunk()
    g = X.make_data(c + 5, 77)["g"].to(dev())
    table, cmap, first = X.build_table([{"numel": g.numel()}], c, dev())
    partials = torch.zeros(first[-1], device=dev())
    h = X.hyper_vector(rule, (0.01, 0.02, 0.03), (0.0, 5e-4, 0.0), 0.937 if rule in (0, 6) else 0.9, beta2=0.99 if rule == 6 else 0.999, tau=5.0)
    hyper, state = torch.tensor(h, dtype=torch.float32, device=dev()), X.state_to_device(X.zero_state(), dev())
    s = X.zero_state()
    for k in range(14):
        X.launch_norm(table, cmap, first, [g], hyper, partials, state, 1)
        d = X.state_from_device(state)
        s = X.scalars(h, {q: v for q, v in s.items() if q != "hyper"}, float(partials.double().sum()), norm=d["norm"])
        assert not X.record_mismatches(d, s, rule), (k, X.record_mismatches(d, s, rule))
        if rule == 4:
            assert d["mu_product"] == s["mu_product"] == X.f32(d["mu_product"]) and 0.0 < d["mu_product"] < 1.0
    assert d["steps"] == 14 == d["updates"]


# ------------------------------------------------------------------------------------------------------------------ the update kernel
UPDATE_CASES = {"SGD": (0, False, 3), "SGD-nesterov": (0, True, 3), "AdamW": (1, False, 3), "Adam": (2, False, 3), "Adamax": (3, False, 3), "NAdam": (4, False, 3),
                "RAdam-before-switch": (5, False, 4), "RAdam-rectified": (5, False, 5), "RMSprop": (6, False, 3)}
MIS_LEN = 2 * 1024 + 7  # two trips of the 1024-element stride and a scalar tail


def update_layout(rule, pool):
    """entries over the pool: the edge lengths in three groups, a null gradient in between, two entries without an EMA pointer, 450
    three-element tensors (a second launch range), and one tensor six times over - all pointers aligned, then each of the five 4 bytes off"""
    specs = [(n, i % 3, True, True, ()) for i, n in enumerate(lengths())]
    specs.insert(5, (1025, 1, False, True, ()))
    specs += [(1027, 1, True, False, ()), (2, 0, True, False, ())]
    specs += [(3, i % 3, True, True, ()) for i in range(450)]
    quants = ("p", "g", "buf", "sec", "ema") if rule else ("p", "g", "buf", "ema")
    specs += [(MIS_LEN, 1, True, True, ())] + [(MIS_LEN, 1, True, True, (q,)) for q in quants]
    entries, data = [], []
    for i, (n, grp, has_g, has_ema, mis) in enumerate(specs):
        d = X.make_data(n, 999 if n == MIS_LEN else 500 + i)
        if not rule:
            d["sec"] = None
        if not has_ema:
            d["ema"] = None
        e = {"numel": n, "group": grp}
        for q, v in d.items():
            e[q] = None if v is None else pool.take(v, 4 if q in mis else 0)
        if not has_g:
            d["g"] = None  # the slice exists and must stay untouched; the kernel is not handed it
        entries.append(e)
        data.append({**d, "group": grp})
    return entries, data


def planted(rule, nesterov, steps, data):
    base = 0.01 if rule in (0, 6) else 0.002
    h = X.hyper_vector(rule, (base, 0.5 * base, 2 * base), (0.0, 5e-4, 0.0), 0.937 if rule in (0, 6) else 0.9, nesterov=nesterov,
                       beta2=0.99 if rule == 6 else 0.999, gscale=0.5)
    s = X.scalars(h, X.zero_state(steps=steps, updates=steps, mu_product=0.43), X.sumsq_exact([d["g"] for d in data], 0.5))
    assert s["clip"] < 1.0
    return h, s


@pytest.mark.parametrize("case", sorted(UPDATE_CASES))
def test_update_kernel_every_word(case):
    rule, nesterov, steps = UPDATE_CASES[case]
    c = chunk()
    pool = X.Pool(700_000, dev())
    entries, data = update_layout(rule, pool)
    h, s = planted(rule, nesterov, steps, data)
    table, cmap, first = X.build_table(entries, c, dev())
    hyper, state = torch.tensor(h, dtype=torch.float32, device=dev()), X.state_to_device(s, dev())
    grads = [e["g"] if d["g"] is not None else None for e, d in zip(entries, data)]
    snap = pool.snapshot()
    before = pool.f.cpu()
    rs = X.launch_update(table, cmap, first, grads, hyper, state, rule, 0, len(entries))
    torch.cuda.synchronize()
    assert len(rs) == 2 and rs[1][0] == 448 and rs[1][2] > 0
    assert pool.outside_unchanged(snap)
    assert X.pack_state(s) == bytes(state.cpu().numpy().tobytes())  # the record is read, never written
    after = pool.f.cpu()
    ref = X.restate_step(rule, nesterov, data, s)
    for i, (e, d, r) in enumerate(zip(entries, data, ref)):
        assert X.bits_equal(host(after, e["g"]), host(before, e["g"])), i  # gradients are never written
        got = tuple(None if e[q] is None else host(after, e[q]) for q in X.QUANT)
        if d["g"] is None:
            assert all(e[q] is None or X.bits_equal(host(after, e[q]), host(before, e[q])) for q in ("p", "buf", "sec")), i
            assert not X.bits_equal(got[3], host(before, e["ema"]))  # its EMA moves
        errs = {q: float(v.max()) for q, v in X.errors(rule, d, s, r, got).items()}
        note("update", case, errs)
        for q, v in errs.items():
            assert v <= X.bound(rule, q), (case, "entry", i, e["numel"], q, v, X.bound(rule, q))
    # vector and scalar path share one body: the aligned copy and the five misaligned ones of the same data agree bit for bit (they did not,
    # for any rule, while the body's multiply-adds were left to -ffp-contract=fast: the EMA rounded by lane and by path)
    n_mis = 6 if rule else 5
    for e in entries[-n_mis + 1:]:
        for q in X.QUANT:
            if e[q] is not None:
                assert X.bits_equal(host(after, e[q]), host(after, entries[-n_mis][q])), (case, q, [k for k in e if k in X.QUANT and e[k] is not None and e[k].data_ptr() % 16])
    report("update", case, rule)


def test_update_kernel_ema_only_mode():
    """host_grads null: parameters, moments and gradients keep their bits, every EMA moves by the planted decay"""
    c = chunk()
    pool = X.Pool(700_000, dev())
    entries, data = update_layout(1, pool)
    h, s = planted(1, False, 3, data)
    table, cmap, first = X.build_table(entries, c, dev())
    hyper, state = torch.tensor(h, dtype=torch.float32, device=dev()), X.state_to_device(s, dev())
    snap = pool.snapshot()
    before = pool.f.cpu()
    X.launch_update(table, cmap, first, None, hyper, state, 0, 0, len(entries))
    torch.cuda.synchronize()
    assert pool.outside_unchanged(snap)
    after = pool.f.cpu()
    worst = 0.0
    for i, (e, d) in enumerate(zip(entries, data)):
        for q in ("p", "g", "buf", "sec"):
            assert X.bits_equal(host(after, e[q]), host(before, e[q])), (i, q)
        if e["ema"] is not None:
            r = X.update(1, False, d["p"], None, None, None, d["ema"], 0.0, 0.0, s, ema_only=True)
            err = float(X.scaled_err(host(after, e["ema"]), r[3], d["ema"]).max())
            worst = max(worst, err)
            assert err <= X.bound(0, "ema"), (i, e["numel"], err)
    print(f"[optim exact] EMA-only mode: ema {worst:.2e} / {X.bound(0, 'ema'):.1e}")


# -------------------------------------------------------------------------------------------------------------- the accumulate kernel
def test_accumulate_kernel_is_float32_addition():
    c = chunk()
    pool = X.Pool(400_000, dev())
    specs = [(n, 0, 0, True, True) for n in lengths()]
    specs += [(MIS_LEN, 4, 0, True, True), (MIS_LEN, 0, 4, True, True), (MIS_LEN, 8, 12, True, True), (1025, 0, 0, False, True), (1025, 0, 0, True, False)]
    specs += [(3, 0, 0, True, True) for _ in range(450)]
    entries, grads, want = [], [], []
    for i, (n, og, oa, has_g, has_acc) in enumerate(specs):
        d = X.make_data(n, 700 + i)
        g, acc = pool.take(d["g"], og), pool.take(d["p"], oa)
        entries.append({"numel": n, "acc": acc if has_acc else None, "g": g, "accv": acc})
        grads.append(g if has_g else None)
        want.append(d["p"] + d["g"] if has_g and has_acc else d["p"])  # float32 addition on the host: exact
    table, cmap, first = X.build_table(entries, c, dev())
    snap = pool.snapshot()
    before = pool.f.cpu()
    rs = X.launch_accumulate(table, cmap, first, grads, 0, len(entries))
    torch.cuda.synchronize()
    assert len(rs) == 2 and pool.outside_unchanged(snap)
    after = pool.f.cpu()
    for i, (e, w) in enumerate(zip(entries, want)):
        assert X.bits_equal(host(after, e["g"]), host(before, e["g"])), i
        assert X.bits_equal(host(after, e["accv"]), w), (i, e["numel"])


# ----------------------------------------------------------------------------------------------------------------- through the classes
def make_optimizer(kind, model, ema):
    from improving_yolov8_cbam_swinblock_amd.engine.optim import FusedAdamW, FusedSGD
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import build_optimizer

    if kind == "FusedSGD":
        return FusedSGD(model, lr=0.01, ema=ema)
    if kind in ("FusedAdamW", "FusedAdam"):
        return FusedAdamW(model, lr=0.002, ema=ema, decoupled=kind == "FusedAdamW")
    return build_optimizer(model, name=kind, lr=0.01 if kind == "RMSProp" else 0.002, momentum=0.937 if kind == "RMSProp" else 0.9, ema=ema)


def toy_grads(model, k):
    """{parameter: gradient} of step k: none for `nograd`, the odd parameter's 4 bytes off a 16-byte boundary, small on odd steps (clip off)"""
    out = {}
    for i, (n, p) in enumerate(model.named_parameters()):
        if n == "nograd":
            continue
        t = (X.make_data(p.numel() + 1, 800 + 40 * k + i % 40)["g"] * (0.01 if k % 2 else 1.0)).to(dev())
        out[p] = t[1:] if n == "odd" else t[:-1].clone()
    return out


@pytest.mark.parametrize("kind", ("FusedSGD", "FusedAdamW", "FusedAdam", "Adamax", "NAdam", "RAdam", "RMSProp"))
def test_classes_step_by_step(kind):
    """8 steps of every optimizer class on the Toy module with a ModelEMA: each step against update() re-seeded from the device's float32 state
    before it; the clip on (even steps) and off, world = 2 from the fifth step, learning rates moving, BatchNorm statistics moving"""
    from improving_yolov8_cbam_swinblock_amd.engine.optim import ModelEMA

    model = X.Toy(chunk(), dev())
    ema = ModelEMA(model)
    opt = make_optimizer(kind, model, ema)
    worst, clips = {}, []
    for k in range(8):
        for gi, grp in enumerate(opt.param_groups):
            grp["lr"] = grp["initial_lr"] * (1.0 + 0.1 * k) / (1 + gi)
        opt.world = 2 if k >= 4 else 1
        with torch.no_grad():
            model.bn.running_mean.add_(0.1 * (k + 1))
        grads = toy_grads(model, k)
        before = X.class_before(opt, grads)
        opt.step(grads)
        s = X.class_after(opt, before, worst)
        clips.append(s["clip"])
        assert s["hyper"][11] == (0.5 if k >= 4 else 1.0) and s["steps"] == k + 1 == s["updates"] == ema.updates
    rule = int(opt.RULE)
    assert len(opt.ranges) >= 3 and any(e["ema_only"] for e in before["entries"]) and all((c < 1.0) == (k % 2 == 0) for k, c in enumerate(clips)), clips
    assert rule == {"FusedSGD": 0, "FusedAdamW": 1, "FusedAdam": 2, "Adamax": 3, "NAdam": 4, "RAdam": 5, "RMSProp": 6}[kind]
    if rule == 5:
        assert s["c1"] == 1.0  # the rectification switched on inside the run
    note("classes", kind, worst)
    report("classes", kind, rule)


def test_stand_alone_model_ema_update():
    """ModelEMA.update (sgd=False): every entry EMA-only - the model keeps its bits, the counter and the decay move on the device"""
    from improving_yolov8_cbam_swinblock_amd.engine.optim import FusedSGD, ModelEMA

    model = X.Toy(chunk(), dev())
    ema = ModelEMA(model, tau=3.0)
    worst = {}
    for k in range(8):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(0.01 * (k + 1))
            model.bn.running_var.mul_(1.1)
        if ema._own is None:  # the optimizer ModelEMA.update builds for itself, built here so that the first update is checked as well
            ema._own = FusedSGD(model, lr=0.0, ema=ema, sgd=False)
        before = X.class_before(ema._own, None)
        ema.update(model)
        s = X.class_after(ema._own, before, worst)
        assert s["updates"] == k + 1 == ema.updates and s["norm"] == 0.0 and s["clip"] == 1.0
    print(f"[optim exact] stand-alone EMA: ema {worst['ema']:.2e} / {X.bound(0, 'ema'):.1e}")
