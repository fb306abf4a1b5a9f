"""Optimizer step of the reference trainer as multi-tensor HIP launches (csrc/optim.hip).

reference: ultralytics/engine/trainer.py:788-849 (build_optimizer: biases / decayed weights / norm weights, SGD with
nesterov momentum), :614-622 (optimizer_step: clip_grad_norm_(10.0) -> step -> zero_grad -> EMA update) and
utils/torch_utils.py:620-685 (ModelEMA).

`FusedSGD` keeps torch.optim.SGD's surface (`param_groups` with lr / momentum / weight_decay / nesterov that schedulers
may rewrite, `state_dict()` / `load_state_dict()` in torch.optim.SGD's format, `zero_grad`) but `step()` is three
launches over every parameter: global gradient norm, clip coefficient (+ EMA decay, update counter), update (+ EMA).
Hyper-parameters live in a device array that is rewritten only when `param_groups` change, so a HIP graph that captured
`step()` follows the learning-rate schedule.
"""
import ctypes
import math
from collections import namedtuple
from copy import deepcopy

import torch
import torch.nn as nn

from .. import _lib
from .._lib import OPT_MAX_GRADS, OptEntry, OptState, check, stream_ptr

# the 20 floats of csrc/optim.hip's `hyper`, in the order of its enum Hyper (lr and wd: one value per parameter group)
HYPER_FIELDS = ("lr", "wd", "momentum", "max_norm", "ema_decay", "ema_tau", "nesterov", "grad_scale", "beta2", "eps", "rule", "one_minus_beta2", "one_minus_beta1",
                "momentum_decay", "beta1_tail", "momentum_decay_tail")
_HYPER_ZERO = dict.fromkeys(HYPER_FIELDS[2:], 0.0)
_STATE_DTYPE = {ctypes.c_float: torch.float32, ctypes.c_int64: torch.int64, ctypes.c_double: torch.float64}
# field of the state record -> (the type to view the record in, the field's index in that view)
_STATE_SLOT = {name: (_STATE_DTYPE[t], getattr(OptState, name).offset // ctypes.sizeof(t)) for name, t in OptState._fields_}
Range = namedtuple("Range", "first n chunk0 n_chunks has_grads")  # one launch: tensors [first, first + n), chunks [chunk0, chunk0 + n_chunks)


def build_table(entries, dev):
    """[OptEntry] -> (host table, device table, device chunk map [(tensor, chunk)], first chunk of each entry (+ the total))"""
    chunk = int(_lib.lib().ymi_opt_chunk_elems())
    tab = (OptEntry * len(entries))(*entries)
    cmap, first = [], []
    for i, e in enumerate(entries):
        first.append(len(cmap))
        cmap.extend((i, c) for c in range((e.numel + chunk - 1) // chunk))
    first.append(len(cmap))
    table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
    return tab, table, torch.tensor(cmap, dtype=torch.int32).reshape(-1, 2).contiguous().to(dev), first


def param_groups_of(model):
    """(biases, decayed weights, norm weights) by the reference's rule (trainer.py:815-825): 'bias' in the full
    parameter name -> no decay; parameters of normalisation layers -> no decay; everything else decays.  Frozen parameters (the DFL
    projection) are grouped as well, exactly as the reference does: tensors without a gradient are skipped by the step."""
    g_bias, g_w, g_norm = [], [], []
    norm = tuple(v for k, v in nn.__dict__.items() if "Norm" in k)
    for module_name, module in model.named_modules():
        for param_name, p in module.named_parameters(recurse=False):
            fullname = f"{module_name}.{param_name}" if module_name else param_name
            if "bias" in fullname:
                g_bias.append(p)
            elif isinstance(module, norm) or "logit_scale" in fullname:
                g_norm.append(p)
            else:
                g_w.append(p)
    return g_bias, g_w, g_norm


class ModelEMA:
    """exponential moving average of every floating-point entry of the model's state_dict (parameters AND buffers),
    reference utils/torch_utils.py:620-685: decay(x) = decay * (1 - exp(-x / tau)), ema = d*ema + (1-d)*model.
    `update()` alone is one multi-tensor launch; attached to a FusedSGD it rides in the optimizer's update pass."""

    def __init__(self, model, decay=0.9999, tau=2000, updates=0):
        self.ema = deepcopy(model).eval()  # (the copy gets a fresh ops.ModelState: arenas are never copied or shared)
        self.updates = updates
        self.decay_max, self.tau = float(decay), float(tau)
        self.decay = lambda x: decay * (1 - math.exp(-x / tau))
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self.enabled = True
        self._own = None  # FusedSGD used for stand-alone updates

    def pairs(self, model):
        """[(model tensor, ema tensor)] over floating-point state_dict entries, in state_dict order."""
        msd, esd = model.state_dict(), self.ema.state_dict()
        return [(msd[k], v) for k, v in esd.items() if v.dtype.is_floating_point]

    def update(self, model):
        if not self.enabled:
            return
        if self._own is None or self._own.model is not model:
            self._own = FusedSGD(model, lr=0.0, ema=self, sgd=False)
        self._own.step()

    def update_attr(self, model, include=(), exclude=("process_group", "reducer")):
        if self.enabled:
            for k, v in model.__dict__.items():
                if (len(include) and k not in include) or k.startswith("_") or k in exclude:
                    continue
                setattr(self.ema, k, v)


class FusedSGD:
    """SGD(momentum, nesterov) over the reference's three parameter groups + gradient clipping (+ EMA), fused."""

    RULE = 0  # csrc/optim.hip enum Rule: 0 SGD-momentum, 1 AdamW, 2 Adam, 3 Adamax, 4 NAdam, 5 RAdam, 6 RMSprop
    # state_dict() / load_state_dict(), in torch.optim's format of the class: (state key, the list that holds its tensors) in torch's order;
    # whether `step` is stored (then a parameter has state only once it stepped with a gradient); further per-parameter entries, each a field of
    # the state record with a method of its name; the group keys restored on load; the group keys torch appends after `params`
    STATE_BUFFERS = (("momentum_buffer", "momentum"),)
    STORES_STEP = False
    EXTRA_STATE = ()
    LOAD_KEYS = ("lr", "initial_lr", "momentum", "nesterov", "weight_decay")
    GROUP_DEFAULTS = {"maximize": False, "foreach": None, "differentiable": False, "fused": None}

    def __init__(self, model, lr=0.01, momentum=0.937, decay=5e-4, nesterov=True, max_norm=10.0, ema=None, sgd=True):
        self.model = model
        g_bias, g_w, g_norm = param_groups_of(model) if sgd else ([], [], [])
        # group order of the reference's optimizer: [biases] + add_param_group(weights, decay) + add_param_group(norm weights)
        self.param_groups = [
            {"params": g_bias, "lr": lr, "initial_lr": lr, "momentum": momentum, "nesterov": nesterov, "weight_decay": 0.0, "dampening": 0},
            {"params": g_w, "lr": lr, "initial_lr": lr, "momentum": momentum, "nesterov": nesterov, "weight_decay": decay, "dampening": 0},
            {"params": g_norm, "lr": lr, "initial_lr": lr, "momentum": momentum, "nesterov": nesterov, "weight_decay": 0.0, "dampening": 0},
        ]
        self.max_norm = float(max_norm) if max_norm else 0.0
        self.world = 1  # gradients are scaled by 1 / world inside the kernels (grad_scale): TrainStep hands over the SUM over ranks and sets this
        self.ema = ema
        self.sgd = sgd
        self._state = None
        self._table = None
        self._hyper_host = None
        # gradient accumulation (accumulate()): a float32 arena the parameters' gradients are folded into, allocated on first use
        self._arena = None
        self._acc = []       # per parameter: its slice of the arena
        self._acc_seen = set()  # indices of the parameters that received a gradient since the arena was cleared
        self.pending = 0     # folds since the last update

    # ---- device tables ---------------------------------------------------------------------------------------------
    def _build(self):
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("FusedSGD runs in libyolo_mi355 kernels: the model must be on the MI355X (cuda) device; there is no CPU path")
        ema_of = {}
        if self.ema is not None:
            for mt, et in self.ema.pairs(self.model):
                ema_of[mt.data_ptr()] = et
        old = dict(zip((id(p) for p in getattr(self, "params", [])), getattr(self, "momentum", [])))  # rebuild after model.to(): keep the momentum
        self.params, entries = [], []
        self.momentum = []
        for gi, grp in enumerate(self.param_groups):
            for p in grp["params"]:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedSGD updates contiguous float32 parameters")
                buf = old[id(p)].to(p.device) if id(p) in old and old[id(p)].shape == p.shape else torch.zeros_like(p)
                self.params.append(p)
                self.momentum.append(buf)
                e = ema_of.pop(p.data_ptr(), None)
                entries.append((p, buf, e, gi))
        old2 = dict(zip(old.keys(), getattr(self, "second", [])))
        self.second = []  # Adam / AdamW: exp_avg_sq per parameter
        if self.RULE:
            for p in self.params:
                self.second.append(old2[id(p)].to(p.device) if id(p) in old2 and old2[id(p)].shape == p.shape else torch.zeros_like(p))
        self.n_sgd = len(entries)
        # EMA-only entries: buffers (BN running statistics) and frozen parameters
        self.ema_only = []
        if self.ema is not None:
            for mt, et in self.ema.pairs(self.model):
                if mt.data_ptr() in ema_of:
                    ema_of.pop(mt.data_ptr())
                    if mt.dtype != torch.float32 or et.dtype != torch.float32:
                        raise RuntimeError("ModelEMA entries must be float32")
                    entries.append((mt, None, et, 0))
                    self.ema_only.append(mt)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._tab_host, self._table, self._cmap, first_chunk_of = build_table(
            [OptEntry(ptr(p), ptr(buf), ptr(e), p.numel(), gi, 0, ptr(self.second[i]) if self.RULE and i < self.n_sgd else None, None)
             for i, (p, buf, e, gi) in enumerate(entries)], dev)
        # sgd=False (stand-alone ModelEMA.update): every entry goes through the gradient path with no gradients, so the
        # counter / decay kernel runs and the update kernel leaves parameters alone
        self.ranges = []
        for lo, hi, has in ((0, self.n_sgd, True), (self.n_sgd, len(entries), not self.sgd)):
            for a in range(lo, hi, OPT_MAX_GRADS):
                b = min(a + OPT_MAX_GRADS, hi)
                self.ranges.append(Range(a, b - a, first_chunk_of[a], first_chunk_of[b] - first_chunk_of[a], has))
        self._entries = entries
        self._arena, self._acc, self.pending = None, [], 0  # (a rebuild drops pending sums: the tensors they belonged to are gone)
        self._acc_seen = set()
        self.n_grad_chunks = first_chunk_of[self.n_sgd] if self.sgd else first_chunk_of[-1]
        self._partials = torch.zeros(max(self.n_grad_chunks, 1), dtype=torch.float32, device=dev)
        had = getattr(self, "_state", None) is not None
        steps = self._state_get("steps") if had else 0  # rebuild: keep Adam's t ...
        mu_product = self._state_get("mu_product") if had else 0.0  # ... and NAdam's running product
        self._state = torch.zeros(ctypes.sizeof(OptState), dtype=torch.uint8, device=dev)
        if steps:
            self._state_set("steps", steps)
            self._state_set("mu_product", mu_product)
        self._dev_updates = 0  # host mirror of the device-side EMA update counter (the record's `updates`); see _sync_updates
        self._hyper = torch.zeros(20, dtype=torch.float32, device=dev)
        self._hyper_host = None  # a fresh device array: the next sync_hyper() must fill it
        self._ptrs = [p.data_ptr() for p, *_ in entries]

    def _stale(self):
        return self._table is None or any(p.data_ptr() != q for (p, *_), q in zip(self._entries, self._ptrs))

    # ---- the state record (OptState) by field name ---------------------------------------------------------------------------
    def _state_get(self, name):
        """one device->host read"""
        dtype, k = _STATE_SLOT[name]
        return self._state.view(dtype)[k].item()

    def _state_set(self, name, value):
        """one fill on the device"""
        dtype, k = _STATE_SLOT[name]
        self._state.view(dtype)[k] = value

    # ---- the hyper array by field name ---------------------------------------------------------------------------------------
    def hyper_values(self):
        """the 20 floats of csrc/optim.hip's `hyper` as Python floats (host only): what every class sets, then what _rule_fields() adds"""
        g, ema = self.param_groups, self.ema
        v = {**_HYPER_ZERO, "max_norm": self.max_norm, "ema_decay": ema.decay_max if ema is not None else 0.0, "ema_tau": ema.tau if ema is not None else 1.0,
             "grad_scale": 1.0 / self.world, "rule": self.RULE, **self._rule_fields()}
        assert len(v) == len(_HYPER_ZERO), set(v) - set(_HYPER_ZERO)  # (a hook named a field the layout does not have)
        return [float(grp["lr"]) for grp in g] + [float(grp["weight_decay"]) for grp in g] + [float(v[k]) for k in _HYPER_ZERO]

    def sync_hyper(self):
        """push lr / momentum / weight decay to the device if a scheduler changed them (call before replaying a graph
        that captured step(); step() calls it itself)."""
        host = self.hyper_values()
        if host != self._hyper_host:
            self._hyper.copy_(torch.tensor(host, dtype=torch.float32))
            self._hyper_host = host
        self._sync_updates()

    def _rule_fields(self):
        """the hyper fields this class sets, after checking that the three groups agree on them"""
        g = self.param_groups
        if any(grp["momentum"] != g[0]["momentum"] or grp["nesterov"] != g[0]["nesterov"] for grp in g):
            raise RuntimeError("FusedSGD: momentum / nesterov are shared by the three groups (as the reference sets them)")
        return {"momentum": g[0]["momentum"], "nesterov": 1.0 if g[0]["nesterov"] else 0.0}

    def _sync_updates(self):
        """the kernel derives the EMA decay from a DEVICE counter; `ema.updates` is the host's view of it.  A caller may set
        the host value at any time - checkpoint.resume, or the reference's idiom `ema.updates = ckpt["updates"]`
        (trainer.py:771) - possibly after the tables were built: push it whenever it differs from what the device holds
        (runs before every step and before every graph replay, outside captured regions)."""
        if self.ema is not None and self._table is not None and int(self.ema.updates) != self._dev_updates:
            self._state_set("updates", int(self.ema.updates))
            self._dev_updates = int(self.ema.updates)

    def count_updates(self, delta):
        """bookkeeping of HIP-graph replays (engine.trainer.TrainStep): a replayed step advanced the device counter (+1); a
        captured, not executed, step did not (-1).  Keeps the host count and the mirror of the device counter together."""
        if self.ema is not None:
            self.ema.updates += delta
            self._dev_updates += delta

    # ---- the step --------------------------------------------------------------------------------------------------
    def _gather(self, r, grads_of):
        """the gradients of range r -> (ctypes array of their addresses, null where there is none; whether there is any; the float32 contiguous
        copies made of gradients that were not, to keep alive until the launches are issued)"""
        arr, found, keep = (ctypes.c_void_p * r.n)(), False, []
        for i, p in enumerate(self.params[r.first:r.first + r.n]):  # (empty for the ranges of EMA-only entries)
            g = grads_of.get(p) if grads_of is not None else p.grad
            if g is not None:
                if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
                    g = g.to(torch.float32).contiguous()
                    keep.append(g)
                arr[i] = g.data_ptr()
                found = True
        return arr, found, keep

    def step(self, grads_of=None):
        """grads_of: optional {param: gradient tensor} (default: p.grad).  Parameters without a gradient keep their
        value and momentum (torch.optim.SGD skips them) but still enter the EMA."""
        if self.pending:
            self.accumulate(grads_of)  # the updating step's own gradients join the sums ...
            return self.step_pending()  # ... and the update reads the arena as "the gradient"
        if self._stale():
            self._build()
        self.sync_hyper()
        L = _lib.lib()
        vp = ctypes.c_void_p
        tab, hyper, state, st = vp(self._table.data_ptr()), vp(self._hyper.data_ptr()), vp(self._state.data_ptr()), stream_ptr()
        gathered = [self._gather(r, grads_of) if r.has_grads else None for r in self.ranges]  # (holds the converted copies until the launches are issued)
        last_grad = max((i for i, r in enumerate(self.ranges) if r.has_grads), default=-1)
        for i, r in enumerate(self.ranges):
            if r.has_grads and r.n_chunks:
                check(L.ymi_opt_grad_norm(tab, vp(self._cmap.data_ptr() + r.chunk0 * 8), r.first, r.n, r.n_chunks, gathered[i][0], hyper, vp(self._partials.data_ptr()),
                                          r.chunk0, self.n_grad_chunks, state, 1 if i == last_grad else 0, st), "opt_grad_norm")
        if last_grad < 0:
            raise RuntimeError("FusedSGD.step(): nothing to update")
        for i, r in enumerate(self.ranges):
            if r.n_chunks:
                check(L.ymi_opt_update(tab, vp(self._cmap.data_ptr() + r.chunk0 * 8), r.first, r.n, r.n_chunks, gathered[i][0] if r.has_grads else None, hyper, state,
                                       int(self.RULE), st), "opt_update")
        if self.ema is not None:
            self.ema.updates += 1
            self._dev_updates += 1

    # ---- gradient accumulation outside autograd (reference trainer.py:305,397) -----------------------------------------
    def _ensure_arena(self):
        """the accumulation arena: one zeroed float32 buffer, every parameter's slice starting on a 16-byte boundary; its addresses go into
        the entry table IN PLACE (graphs that captured step() hold the table's address)."""
        if self._stale():
            self._build()
        if self._arena is not None:
            return
        offs, total = [], 0
        for p in self.params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        dev = self._table.device
        self._arena = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        self._acc = [self._arena[o : o + p.numel()].view_as(p) for o, p in zip(offs, self.params)]
        for i, a in enumerate(self._acc):
            self._tab_host[i].acc = a.data_ptr()
        self._table.copy_(torch.frombuffer(bytearray(bytes(self._tab_host)), dtype=torch.uint8))

    def accumulate(self, grads_of=None):
        """fold p.grad (or grads_of[p]) into the arena: acc += g in float32, one launch per range of the entry table.  Autograd never
        accumulates: the caller drops the gradients afterwards (zero_grad(set_to_none=True)), so every backward starts from p.grad is
        None.  Sums form in call order.  Parameters without a gradient are skipped."""
        self._ensure_arena()
        L = _lib.lib()
        tab = ctypes.c_void_p(self._table.data_ptr())
        st = stream_ptr()
        keep = []
        for r in self.ranges:
            if not (r.has_grads and r.n_chunks) or r.first >= self.n_sgd:
                continue
            arr, found, copies = self._gather(r, grads_of)
            keep += copies
            self._acc_seen.update(r.first + i for i in range(r.n) if arr[i])
            if found:
                check(L.ymi_opt_grad_accumulate(tab, ctypes.c_void_p(self._cmap.data_ptr() + r.chunk0 * 8), r.first, r.n, r.n_chunks, arr, st), "opt_grad_accumulate")
        self.pending += 1

    def step_pending(self):
        """the update from the accumulated sums (clip on the total's norm, as the reference clips what AccumulateGrad summed), then the
        arena is cleared - after the update has read it, on the same stream - and `pending` reset."""
        if self._arena is None or not self._acc_seen:
            raise RuntimeError("FusedSGD.step_pending(): nothing accumulated")
        self.pending = 0
        self.step({self.params[i]: self._acc[i] for i in sorted(self._acc_seen)})
        self._arena.zero_()
        self._acc_seen = set()

    def discard_pending(self):
        """drop the accumulated sums (the reference zeroes resumed gradients at trainer.py:346)."""
        if self._arena is not None:
            self._arena.zero_()
        self._acc_seen = set()
        self.pending = 0

    def grad_norm(self):
        """total gradient norm of the last step (before clipping), as clip_grad_norm_ returns it: one device->host read."""
        return self._state_get("norm")

    def steps_taken(self):
        """optimizer steps taken so far (Adam's t), counted on the device (one device->host read)."""
        return self._state_get("steps") if self._table is not None else 0

    def zero_grad(self, set_to_none=True):
        for grp in self.param_groups:
            for p in grp["params"]:
                if set_to_none:
                    p.grad = None
                elif p.grad is not None:
                    p.grad.zero_()

    # ---- torch.optim-compatible state (checkpoint contract: trainer.py:546 stores optimizer.state_dict()) ---------------
    def state_dict(self):
        if self._table is None:
            self._build()
        t = float(self.steps_taken()) if self.STORES_STEP else 0.0
        defaults = self.GROUP_DEFAULTS | ({"fused": None, "decoupled_weight_decay": self.RULE == 1} if self.RULE in (1, 2) else {})
        state, groups, idx = {}, [], 0
        for grp in self.param_groups:
            ids = []
            for p in grp["params"]:
                if not self.STORES_STEP or (t > 0 and p.requires_grad):  # torch creates a parameter's state at its first step with a gradient
                    state[idx] = ({"step": torch.tensor(t)} if self.STORES_STEP else {}) | {k: getattr(self, a)[idx] for k, a in self.STATE_BUFFERS}
                    for k in self.EXTRA_STATE:
                        state[idx][k] = torch.tensor(getattr(self, k)())
                ids.append(idx)
                idx += 1
            groups.append({k: v for k, v in grp.items() if k != "params"} | {"params": ids} | defaults)
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        if self._table is None:
            self._build()
        for grp, saved in zip(self.param_groups, sd["param_groups"]):
            for k in self.LOAD_KEYS:
                if k in saved:
                    grp[k] = tuple(saved[k]) if k == "betas" else saved[k]
        steps = 0
        for idx, st in sd["state"].items():
            for k, a in self.STATE_BUFFERS:
                buf = st[k] if self.STORES_STEP else st.get(k)  # (torch.optim.SGD holds None before a parameter's first step)
                if buf is not None:
                    getattr(self, a)[int(idx)].copy_(buf.to(torch.float32))
            if self.STORES_STEP:
                steps = max(steps, int(float(st["step"])))
            for k in self.EXTRA_STATE:
                if k in st:
                    self._state_set(k, float(st[k]))
        if self.STORES_STEP:
            self._state_set("steps", steps)  # one t for every parameter (they step together)


class FlatFold:
    """dst[i] += src over flat float32 buffers through ymi_opt_grad_accumulate: a one-entry table per destination.  The split-graph schedule
    of engine.trainer.TrainStep folds its flat gradient buckets into a flat arena of the same layout with it (one launch per bucket) and
    adds the arena back into the buckets before the exchange of the updating step."""

    def __init__(self, dsts):
        for d in dsts:
            if d.dtype != torch.float32 or not d.is_contiguous() or d.dim() != 1:
                raise RuntimeError("FlatFold adds flat contiguous float32 buffers")
        _, self._table, self._cmap, first = build_table([OptEntry(None, None, None, d.numel(), 0, 0, None, d.data_ptr()) for d in dsts], dsts[0].device)
        self._range = [(a, b - a) for a, b in zip(first, first[1:])]  # (first chunk, chunks) of each destination
        self.dsts = list(dsts)

    def add(self, i, src):
        if src.dtype != torch.float32 or not src.is_contiguous() or src.numel() != self.dsts[i].numel():
            raise RuntimeError("FlatFold.add: a contiguous float32 buffer of the destination's length")
        c0, nc = self._range[i]
        if nc:
            arr = (ctypes.c_void_p * 1)(src.data_ptr())
            check(_lib.lib().ymi_opt_grad_accumulate(ctypes.c_void_p(self._table.data_ptr()), ctypes.c_void_p(self._cmap.data_ptr() + c0 * 8), i, 1, nc, arr,
                                                     stream_ptr()), "opt_grad_accumulate")


class FusedAdamW(FusedSGD):
    """torch.optim.AdamW over the reference's three parameter groups (trainer.py:829-830 `optim.AdamW(g[2], lr=lr,
    betas=(momentum, 0.999), weight_decay=0.0)` + the two add_param_group calls; what optimizer='auto' picks for runs of at most
    10000 iterations, :812) + gradient clipping (+ EMA), in the same three launches as FusedSGD.  `decoupled=False` is
    torch.optim.Adam (weight decay added to the gradient).  `param_groups` carry torch's Adam keys (lr, betas, eps, weight_decay);
    state_dict() / load_state_dict() use torch.optim.Adam's layout (step, exp_avg, exp_avg_sq per parameter)."""

    RULE = 1
    SECOND_KEY = "exp_avg_sq"  # (Adamax: exp_inf)
    STATE_BUFFERS = (("exp_avg", "momentum"), (SECOND_KEY, "second"))
    STORES_STEP = True
    LOAD_KEYS = ("lr", "initial_lr", "betas", "eps", "weight_decay")
    GROUP_DEFAULTS = {"maximize": False, "foreach": None, "capturable": False, "differentiable": False}

    def __init__(self, model, lr=0.001, betas=(0.9, 0.999), eps=1e-8, decay=5e-4, max_norm=10.0, ema=None, decoupled=True):
        super().__init__(model, lr=lr, momentum=betas[0], decay=decay, nesterov=False, max_norm=max_norm, ema=ema)
        self.RULE = 1 if decoupled else 2
        for grp in self.param_groups:
            for k in ("momentum", "nesterov", "dampening"):
                grp.pop(k)
            grp.update(betas=(float(betas[0]), float(betas[1])), eps=float(eps), amsgrad=False)

    def _rule_fields(self):
        g = self.param_groups
        if any(tuple(grp["betas"]) != tuple(g[0]["betas"]) or grp["eps"] != g[0]["eps"] for grp in g):
            raise RuntimeError("FusedAdamW: betas / eps are shared by the three groups (as the reference sets them)")
        b1, b2 = g[0]["betas"]
        return {"momentum": b1, "beta2": b2, "eps": g[0]["eps"], "one_minus_beta2": 1 - b2, "one_minus_beta1": 1 - b1}

    @property
    def exp_avg(self):
        return self.momentum


class FusedAdamax(FusedAdamW):
    """torch.optim.Adamax (reference trainer.py:829-830 with name 'Adamax'): exp_inf = max(beta2 * exp_inf, |g| + eps),
    p -= lr / (1 - beta1^t) * exp_avg / exp_inf; weight decay added to the gradient.  State layout: step, exp_avg, exp_inf."""

    SECOND_KEY = "exp_inf"
    STATE_BUFFERS = (("exp_avg", "momentum"), (SECOND_KEY, "second"))

    def __init__(self, model, lr=0.002, betas=(0.9, 0.999), eps=1e-8, decay=5e-4, max_norm=10.0, ema=None):
        super().__init__(model, lr=lr, betas=betas, eps=eps, decay=decay, max_norm=max_norm, ema=ema, decoupled=False)
        self.RULE = 3
        for grp in self.param_groups:
            grp.pop("amsgrad", None)


class FusedNAdam(FusedAdamW):
    """torch.optim.NAdam (momentum_decay 4e-3, weight decay added to the gradient): the Nesterov momentum schedule
    mu_t = beta1 (1 - 0.5 * 0.96^(t * momentum_decay)) and its running product are kept on the device.  State: step, mu_product, exp_avg, exp_avg_sq."""

    EXTRA_STATE = ("mu_product",)

    def __init__(self, model, lr=0.002, betas=(0.9, 0.999), eps=1e-8, decay=5e-4, max_norm=10.0, ema=None, momentum_decay=4e-3):
        super().__init__(model, lr=lr, betas=betas, eps=eps, decay=decay, max_norm=max_norm, ema=ema, decoupled=False)
        self.RULE = 4
        for grp in self.param_groups:
            grp.pop("amsgrad", None)
            grp.update(momentum_decay=float(momentum_decay), decoupled_weight_decay=False)

    def _rule_fields(self):
        """... and momentum_decay, with the float32 tails of beta1 and momentum_decay (the device rebuilds both to double precision)."""
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))  # noqa: E731
        b1, md = float(self.param_groups[0]["betas"][0]), float(self.param_groups[0]["momentum_decay"])
        return super()._rule_fields() | {"momentum_decay": md, "beta1_tail": b1 - f32(b1), "momentum_decay_tail": md - f32(md)}

    def mu_product(self):
        return self._state_get("mu_product") if self.steps_taken() else 1.0


class FusedRAdam(FusedAdamW):
    """torch.optim.RAdam (weight decay added to the gradient): the variance-rectified step once rho_t > 5, plain bias-corrected momentum before."""

    def __init__(self, model, lr=0.001, betas=(0.9, 0.999), eps=1e-8, decay=5e-4, max_norm=10.0, ema=None):
        super().__init__(model, lr=lr, betas=betas, eps=eps, decay=decay, max_norm=max_norm, ema=ema, decoupled=False)
        self.RULE = 5
        for grp in self.param_groups:
            grp.pop("amsgrad", None)
            grp.update(decoupled_weight_decay=False)


class FusedRMSprop(FusedSGD):
    """torch.optim.RMSprop(lr, momentum=momentum) as the reference builds it (trainer.py:831-832): alpha 0.99, eps 1e-8, not centered;
    square_avg = alpha * square_avg + (1 - alpha) g^2, buf = momentum * buf + g / (sqrt(square_avg) + eps), p -= lr * buf.
    State layout: step, square_avg, momentum_buffer."""

    RULE = 6
    STATE_BUFFERS = (("square_avg", "second"), ("momentum_buffer", "momentum"))
    STORES_STEP = True
    LOAD_KEYS = ("lr", "initial_lr", "momentum", "alpha", "eps", "weight_decay")
    GROUP_DEFAULTS = FusedAdamW.GROUP_DEFAULTS

    def __init__(self, model, lr=0.01, momentum=0.937, alpha=0.99, eps=1e-8, decay=5e-4, max_norm=10.0, ema=None):
        super().__init__(model, lr=lr, momentum=momentum, decay=decay, nesterov=False, max_norm=max_norm, ema=ema)
        for grp in self.param_groups:
            for k in ("nesterov", "dampening"):
                grp.pop(k)
            grp.update(alpha=float(alpha), eps=float(eps), centered=False)

    def _rule_fields(self):
        g = self.param_groups
        if any(grp["momentum"] != g[0]["momentum"] or grp["alpha"] != g[0]["alpha"] or grp["eps"] != g[0]["eps"] for grp in g):
            raise RuntimeError("FusedRMSprop: momentum / alpha / eps are shared by the three groups (as the reference sets them)")
        return {"momentum": g[0]["momentum"], "beta2": g[0]["alpha"], "eps": g[0]["eps"], "one_minus_beta2": 1 - g[0]["alpha"]}
