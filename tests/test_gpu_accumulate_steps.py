"""GPU: gradient accumulation through TrainStep(batch, update=...) - eager against the reference trainer's own accumulation
(tests/golden/accumulate_tiny.*), the captured forms against eager, the untouched default path, the refusals, and train_epoch with the
reference's warm-up schedule (reference engine/trainer.py:305-306, 371-399, 614-622)."""
import json

import pytest
import torch

from conftest import GOLDEN, check_update_steps, golden_state, load_golden

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def test_accumulated_steps_match_the_reference_trainer():
    """float32, eager, calls (A, False), (B, True), (A, False), (B, True) against the reference's backward(A), backward(B), optimizer_step,
    twice.  Bounds: those of test_train_steps_match_reference_trainer_fixture for SGD - (7e-5, 2e-3) on the updates, (1.2e-4, 5e-3) on the
    gradient norms (the norm here is that of the accumulated total, which is what the reference clips)."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    meta = json.loads((GOLDEN / "accumulate_tiny.json").read_text())
    d = load_golden("accumulate_tiny")
    d.update(load_golden("accumulate_tiny.s1"))
    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    model = DetectionModel(cfg, ch=3, nc=1)
    model.load_state_dict(golden_state(load_golden("e2e_tiny_seed7")), strict=True)
    model = model.to(dev())
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    step = TrainStep(model, world_size=1, lr=0.01, dtype=torch.float32, optimizer="SGD", momentum=0.937)
    names = {id(p): n for n, p in model.named_parameters()}
    assert [[names[id(p)] for p in g["params"]] for g in step.opt.param_groups] == meta["groups"]
    batches = {}
    for tag in "AB":
        batches[tag] = {k: torch.from_numpy(d[f"{tag}.{k}"]).to(dev()) for k in ("batch_idx", "cls", "bboxes")}
        batches[tag]["img"] = (torch.from_numpy(d[f"{tag}.img_u8"]).float() / 255).to(dev())
    states, ema_states, k = [], [], 0
    for tag, update in meta["calls"]:
        before = step.ema.updates
        step(batches[tag], update=update)
        if not update:
            assert step.ema.updates == before and step.opt.pending == 1
            continue
        torch.cuda.synchronize()
        got, want = step.opt.grad_norm(), meta["norms"][k]
        print(f"[accumulated update {k}] gradient norm {got:.6f} reference {want:.6f} relative {abs(got - want) / want:.2e}")
        assert abs(got - want) <= (1.2e-4, 5e-3)[k] * want
        states.append({n: v.detach().cpu().clone() for n, v in model.state_dict().items()})
        ema_states.append({n: v.detach().cpu().clone() for n, v in step.ema.ema.state_dict().items()})
        k += 1
    check_update_steps(d, init, states, ema_states, step_tol=(7e-5, 2e-3))
    assert step.ema.updates == meta["ema_updates"] == 2 and step.opt.pending == 0


# ---- captured forms follow eager ------------------------------------------------------------------------------------------------
PATTERN = [True, False, True, False, False, True, True]
_RUNS = {}


def run_pattern(mode, pattern, warm_at=None):
    """one TrainStep driven through `pattern` (yolov8n-cbam, nc 1, 2 x 320 x 320, bf16, SGD), every call with a batch of its own.  A captured
    mode runs 3 eager warm-up steps inside the plain call that captures its first graph, so the eager run takes 3 plain steps of the same
    batch before its call `warm_at`, as test_graph_replay_follows_lr_schedule aligns them."""
    key = (mode, tuple(pattern), warm_at)
    if key in _RUNS:
        return _RUNS[key]
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    torch.manual_seed(0)
    model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1).to(dev())
    step = TrainStep(model, world_size=1, lr=0.01, graph={"eager": False, "graph": True, "split": "split"}[mode], optimizer="SGD")
    batches = [synthetic_batch(2, 320, dev(), 1 + i) for i in range(len(pattern))]
    head_bn_weight = [p for n, p in model.model[-1].named_parameters() if n.endswith("bn.weight")][0]  # a BatchNorm weight of the Detect head
    first_bn = model.model[0].bn
    out = {"loss": [], "snap": []}
    for i, update in enumerate(pattern):
        # a copy per call: a captured step adopts the first batch's tensors as its static inputs and later batches are copied INTO them
        # (and the copy is dropped after the call, so a graph still reading it would read memory the allocator has back)
        if mode == "eager" and i == warm_at:
            for _ in range(3):
                step({k: v.clone() if torch.is_tensor(v) else v for k, v in batches[i].items()})
        batch = {k: v.clone() if torch.is_tensor(v) else v for k, v in batches[i].items()}
        out["loss"].append(step(batch, update=update).detach().float().cpu().clone())
        if not update:
            torch.cuda.synchronize()
            out["snap"].append(dict(params=[p.detach().clone() for p in model.parameters()], momentum=[m.clone() for m in step.opt.momentum],
                                    ema=[v.clone() for v in step.ema.ema.state_dict().values()], running_mean=first_bn.running_mean.clone(),
                                    updates=step.ema.updates, steps=step.opt.steps_taken()))
    torch.cuda.synchronize()
    out.update(w0=model.model[0].conv.weight.detach().clone(), bn=head_bn_weight.detach().clone(), steps=step.opt.steps_taken(), updates=step.ema.updates,
               pending=step.opt.pending + step._flat_pending, full_graph=any(rec.graph is not None for rec in step._shapes.values()))
    _RUNS[key] = out
    return out


def compare_with_eager(got, ref, pattern):
    for i, (a, b) in enumerate(zip(got["loss"], ref["loss"])):
        print(f"call {i} update={pattern[i]} loss {a.tolist()} eager {b.tolist()}")
        assert torch.allclose(a, b, rtol=2e-2, atol=2e-2), (i, a, b)
    print("conv0 weight", rel(got["w0"], ref["w0"]), "head bn weight", rel(got["bn"], ref["bn"]))
    assert rel(got["w0"], ref["w0"]) < 5e-3 and rel(got["bn"], ref["bn"]) < 5e-3
    assert got["steps"] == ref["steps"] and got["updates"] == ref["updates"] and got["pending"] == ref["pending"] == 0


@pytest.mark.parametrize("mode", ["graph", "split"])
def test_captured_accumulation_follows_eager(mode):
    ref, got = run_pattern("eager", PATTERN, 0), run_pattern(mode, PATTERN)
    compare_with_eager(got, ref, PATTERN)
    assert got["updates"] == 3 + sum(PATTERN)
    for run in (ref, got):  # between the micro-steps of calls 4 and 5 only the BatchNorm statistics move
        a, b = run["snap"][1], run["snap"][2]
        for k in ("params", "momentum"):
            assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k
        assert (a["updates"], a["steps"]) == (b["updates"], b["steps"])
        assert not torch.equal(a["running_mean"], b["running_mean"])
        # (the EMA copy holds running statistics too, but it is only written by an update)
        assert all(torch.equal(x, y) for x, y in zip(a["ema"], b["ema"]))


@pytest.mark.parametrize("mode", ["graph", "split"])
def test_first_call_may_be_a_micro_step(mode):
    """update=False before anything was captured: the batch is applied once as an eager micro-step and the graphs are captured without
    being executed - no warm-up iteration updates, folds twice or moves the BatchNorm statistics, so eager needs no alignment."""
    pattern = [False, True, False, False, True]
    ref, got = run_pattern("eager", pattern), run_pattern(mode, pattern)
    compare_with_eager(got, ref, pattern)
    assert got["updates"] == 2 and got["steps"] == 2
    assert rel(got["snap"][0]["running_mean"], ref["snap"][0]["running_mean"]) < 5e-3
    assert mode == "split" or not got["full_graph"]  # graph=True: the full-step graph was never needed


@pytest.mark.parametrize("mode", ["graph", "split"])
def test_plain_call_after_a_first_micro_step_reads_the_same_static_batch(mode):
    """micro graph first, full-step graph second: the plain call 2 finds a static batch in place (the micro graph reads it) and must load
    its batch into those tensors, not adopt new ones - or calls 3 and 4 would replay the micro graph on call 1's data, or on freed memory.
    graph=True captures the full-step graph in call 2, behind 3 warm-up steps of that batch; the split schedule captured everything in
    call 0 and replays."""
    pattern = [False, True, True, False, True]
    warm_at = 2 if mode == "graph" else None
    ref, got = run_pattern("eager", pattern, warm_at), run_pattern(mode, pattern)
    compare_with_eager(got, ref, pattern)
    assert got["full_graph"] and got["updates"] == got["steps"] == (6 if mode == "graph" else 3)


@pytest.mark.parametrize("mode", ["eager", "graph", "split"])
def test_default_path_allocates_and_captures_nothing_new(mode):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1).to(dev())
    step = TrainStep(model, world_size=1, graph={"eager": False, "graph": True, "split": "split"}[mode])
    batch = synthetic_batch(2, 320, dev(), 1)
    for _ in range(5):
        step(batch)
    torch.cuda.synchronize()
    assert step.opt._arena is None and step.opt._acc == [] and step.opt.pending == 0
    assert step._micro is None and step._update_graph is None and step._flat_arena is None and step._flat_fold is None and step._flat_pending == 0


def test_update_false_is_refused_where_it_is_out_of_scope():
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1).to(dev())
    batch = synthetic_batch(2, 320, dev(), 1)
    for kw, word in ((dict(graph="tail"), "tail"), (dict(graph=True, image_shapes=2), "image_shapes"), (dict(world_size=2), "world_size")):
        step = TrainStep(model, ema=False, **kw)
        with pytest.raises(ValueError, match=word):
            step(batch, update=False)
        assert step.opt._arena is None and step.opt.pending == 0
        for h in step.buckets._hooks:
            h.remove()


@pytest.mark.parametrize("nbs, graph", [(8, False), (64, False), (64, True)])
def test_train_epoch_follows_the_warmup_schedule(nbs, graph):
    """nbs = 8 is the issue's case (the warm-up is 100 iterations by the reference's max(..., 100), so the whole run is warm-up and the
    accumulation count stays 1 over its 12 iterations); nbs = 64 ramps the count to 4 within them, so micro-steps do occur.
    graph=True: the loss items are the graphs' static output tensors, rewritten by every replay, and the schedule reaches the replays through
    the hyper-parameter array; the first plain call takes 3 warm-up steps before it captures, so 3 more updates are counted.
    tloss: the running mean (t * i + x) / (i + 1) against the plain mean of the 6 items in float32 - a few ulp per step: 1e-5 relative."""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, WarmupSchedule, synthetic_batch, train_epoch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    kw = dict(epochs=2, nb=6, batch=2, nbs=nbs, warmup_epochs=0.5, lr0=0.01, lrf=0.01, momentum=0.937, weight_decay=5e-4)
    model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1).to(dev())
    step = TrainStep(model, world_size=1, lr=0.01, optimizer="SGD", graph=graph)
    batches = [synthetic_batch(2, 320, dev(), 1 + i) for i in range(6)]
    seen = []
    warmup_steps = 3 if graph else 0

    def recording(batch, update=True):
        items = step(batch, update=update)
        seen.append((update, items.detach().clone()))
        return items

    recording.opt = step.opt
    sched, twin = WarmupSchedule(**kw), WarmupSchedule(**kw)
    assert sched.nw == 100
    want = [twin.advance(twin.at(e, i)) for e in range(2) for i in range(6)]
    n_updates = sum(r.update for r in want)
    trailing = 0 if nbs == 8 else 1  # nbs = 64: the last iteration is a micro-step, its gradients stay pending as in the reference
    assert n_updates == (12 if nbs == 8 else 5) and [r.update for r in want][-2:] == ([True, True] if nbs == 8 else [True, False])
    for epoch in range(2):
        seen.clear()
        # (copies: a captured step adopts its first batch's tensors as static inputs and copies later batches into them)
        tloss = train_epoch(recording, [{k: v.clone() if torch.is_tensor(v) else v for k, v in b.items()} for b in batches], sched, epoch)
        torch.cuda.synchronize()
        assert [u for u, _ in seen] == [r.update for r in want[epoch * 6: epoch * 6 + 6]]
        assert torch.allclose(tloss, torch.stack([x for _, x in seen]).mean(0), rtol=1e-5, atol=0)
    assert step.ema.updates == n_updates + warmup_steps == step.opt.steps_taken() and step.opt.pending == trailing
    assert (step._micro is not None) == (step._update_graph is not None) == any(rec.graph is not None for rec in step._shapes.values()) == graph
    last = want[-1]
    assert [g["lr"] for g in step.opt.param_groups] == last.lrs and all(g["momentum"] == last.momentum for g in step.opt.param_groups)
    assert step.opt.param_groups[1]["weight_decay"] == sched.weight_decay and step.opt.param_groups[0]["weight_decay"] == 0.0
    # what the last update read on the device (hyper[0..2] learning rates, [4] the decayed group's weight decay, [6] momentum), in float32
    applied = [r for r in want if r.update][-1]
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).tolist()
    hyper = step.opt._hyper.cpu().tolist()
    assert hyper[:3] == f32(applied.lrs) and [hyper[4], hyper[6]] == f32([sched.weight_decay, applied.momentum])
