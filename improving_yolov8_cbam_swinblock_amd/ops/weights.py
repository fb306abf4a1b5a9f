"""Weight operands and weight gradients: the per-step weight arena and its pack launches, gradient buckets as GEMM outputs (grad_arena), the
split-K weight-gradient GEMM with its deferred (batched) slab sum, side-stream and rider schedules (reference: the backward of
Conv / nn.Linear weights, nn/modules/conv.py:50-91)."""
import contextlib
import ctypes
import os

import torch

from .. import _lib
from .._lib import ACT_GELU, ACT_NONE, ACT_SILU, ConvProblem, DgradProblem, as_ymi, check, chunk_elems, empty_nhwc, is_nhwc, ptr, stream_ptr, workspace, ymi_dtype
from .base import (  # noqa: F401
    HOOKS, RUN, L, _as4d, _byref, _deferred_twice, _in_backward, compute_dtype, round_up,
)

# ------------------------------------------------------------------------------------ weights
class _PackDesc(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("dst_fwd", ctypes.c_void_p), ("dst_dgrad", ctypes.c_void_p), ("o", ctypes.c_int32),
                ("i", ctypes.c_int32), ("kh", ctypes.c_int32), ("kw", ctypes.c_int32), ("ipad", ctypes.c_int32), ("opad", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("ostride", ctypes.c_int32), ("o_off", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class WeightArena:
    """All conv / linear weights of a model packed into kernel operand layouts by ONE launch per step.

    Life cycle: while `recording`, the per-call packers below note (weight, padding, stride) of every use during one
    full forward+backward; `build()` then allocates one arena and a device descriptor table; afterwards `pack()`
    (called at the start of each training forward) refreshes every operand with a single kernel and the per-call
    packers return views of the arena.  A use that was not recorded simply falls back to its own pack launch.

    A spec holds ONE weight, or a PAIR of weights of the same input that run as one convolution (Detect's sibling branches,
    reference head.py:71-72): the pair's forward operands lie back to back ([oA + oB][tap][ipad]) and its data-gradient operand has
    the two column ranges side by side ([i][tap][oA + oB], ymi_pack_desc.ostride / o_off)."""

    def __init__(self):
        self.specs = {}      # id(weight) | (id(wA), id(wB)) -> dict(weights, o (tuple), i, k, ipad, opad, stride)
        self.dtype = None
        self.built = False
        self.fresh = False   # operands correspond to the current weight values
        self.views = {}

    def note(self, weight, dtype, ipad=None, opad=None, stride=1, pair=None):
        """pair: the second weight when (weight, pair) run as one convolution (opad is then the two real widths' sum)."""
        if self.built:
            return
        ws = (weight,) if pair is None else (weight, pair)
        w4 = [_as4d(w) for w in ws]
        i, k = w4[0].shape[1], w4[0].shape[2]
        key = id(weight) if pair is None else (id(weight), id(pair))
        sp = self.specs.setdefault(key, dict(weights=ws, o=tuple(w.shape[0] for w in w4), i=i, k=k, ipad=None, opad=None, stride=1))
        if ipad is not None:
            sp["ipad"] = ipad
        if opad is not None:
            sp["opad"], sp["stride"] = opad, stride
        self.dtype = dtype

    def build(self):
        if not self.specs:
            return
        dev = next(iter(self.specs.values()))["weights"][0].device
        es = 2 if self.dtype == torch.bfloat16 else 4
        total, plan = 0, []
        for key, sp in self.specs.items():
            if sp["k"] > 3:
                raise RuntimeError("weight arena: kernels larger than 3x3 are not packed in one launch (the pack kernel's LDS tile holds nine taps)")
            osum = sum(sp["o"])
            nf = osum * sp["k"] ** 2 * sp["ipad"] if sp["ipad"] else 0
            nd = sp["i"] * sp["k"] ** 2 * sp["opad"] if sp["opad"] else 0
            offf, total = total, total + round_up(nf, 8)
            offd, total = total, total + round_up(nd, 8)
            plan.append((key, sp, nf, nd, offf, offd))
        self.arena = torch.empty(total, dtype=self.dtype, device=dev)
        ndesc = sum(len(sp["weights"]) for _, sp, *_ in plan)
        descs = (_PackDesc * ndesc)()
        starts = [0]
        base = self.arena.data_ptr()
        self.params = []
        n = 0
        for key, sp, nf, nd, offf, offd in plan:
            pair = len(sp["weights"]) == 2
            k2 = sp["k"] ** 2
            o_off = 0
            for w, o in zip(sp["weights"], sp["o"]):
                # (a pair: forward rows of the second weight follow the first's; in the data-gradient operand each weight owns the
                # columns [o_off, o_off + o) of rows that are opad = oA + oB long - the widths are whole 16-byte chunks, no padding between)
                opad_w = (o if pair else sp["opad"]) if nd else 0
                descs[n] = _PackDesc(w.data_ptr(), base + (offf + o_off * k2 * (sp["ipad"] or 0)) * es if nf else None, base + offd * es if nd else None,
                                     o, sp["i"], sp["k"], sp["k"], sp["ipad"] or 0, opad_w, sp["stride"], (sp["opad"] if (pair and nd) else 0), o_off if pair else 0, 0)
                # workgroups: one per 32 x 32 tile of (output, input) channels, padded extents included (include/ymi.h)
                wgs = ((max(o, opad_w) + 31) // 32) * ((max(sp["i"], sp["ipad"] if nf else 0) + 31) // 32)
                starts.append(starts[-1] + wgs)
                self.params.append(w)
                o_off += o
                n += 1
            self.views[key] = (self.arena[offf : offf + nf] if nf else None, self.arena[offd : offd + nd] if nd else None, sp["ipad"], sp["opad"], sp["stride"])
        raw = bytes(descs)
        self.descs = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
        self.starts = torch.tensor(starts, dtype=torch.int32).to(dev)
        self.count, self.blocks = ndesc, starts[-1]
        self.ptrs = [w.data_ptr() for w in self.params]  # the descriptor table holds these raw addresses
        self.built = True

    def stale(self):
        """a parameter's storage moved since build() (model.to() / .float() / any re-allocating Module._apply swaps
        param.data under the same Parameter object): the descriptor table then points at freed memory."""
        return any(w.data_ptr() != p or w.device != self.arena.device for w, p in zip(self.params, self.ptrs))

    def pack(self):
        check(L().ymi_pack_conv_weights_batch(ptr(self.descs), ptr(self.starts), self.count, self.blocks, ymi_dtype(self.dtype), stream_ptr()), "pack_conv_weights_batch")
        # an operand is valid for exactly the weight VALUES it was packed from: Tensor._version counts in-place
        # updates (optimizer steps, load_state_dict), so a module called on its own after an update never sees the
        # operands of the previous step
        self.versions = {id(w): w._version for w in self.params}
        self.fresh = True

    def _view(self, weight, dtype, pair=None):
        if not (self.built and self.fresh and dtype == self.dtype):
            return None
        key = id(weight) if pair is None else (id(weight), id(pair))
        v = self.views.get(key)
        if v is None or any(self.versions.get(id(w)) != w._version for w in ((weight,) if pair is None else (weight, pair))):
            return None
        return v

    def lookup_fwd(self, weight, ipad, dtype, pair=None):
        v = self._view(weight, dtype, pair)
        return v[0] if v is not None and v[0] is not None and v[2] == ipad else None

    def lookup_dgrad(self, weight, opad, stride, dtype, pair=None):
        v = self._view(weight, dtype, pair)
        return v[1] if v is not None and v[1] is not None and v[3] == opad and v[4] == stride else None


class ModelState:
    """What a model carries from one forward to the next (BaseModel._state): its WeightArena, its BatchNorm statistics arena, the forward
    epoch and, during a forward, the num_batches_tracked counters to advance.  `forward()` makes it RUN.model for one model forward.
    A deep copy or pickle of the model gets a fresh one (the arenas hold operands of THIS model's parameters)."""

    def __init__(self):
        self.arena = None           # WeightArena of the training forwards
        self.stats = None           # int64 statistics arena, sized by the previous training forward's demand
        self.epoch = 0              # model forwards so far (_note_use)
        self.acc = None             # the statistics arena while a training forward hands it out (_stat_acc)
        self.cursor = self.need = 0
        self.counters = []

    def __reduce__(self):
        return ModelState, ()

    @contextlib.contextmanager
    def forward(self, x, training):
        """one model forward.  Training forwards on the GPU zero the statistics arena with one fill; with autograd recording they also pack
        every weight with one launch: the first forward+backward records the uses, the second builds the arena.  Eval / no-grad forwards
        keep the per-call packers and drop nothing."""
        cuda = torch.is_tensor(x) and x.is_cuda
        self.epoch += 1
        self.acc = None
        if training and cuda and HOOKS["stat_atomics"]:
            if self.stats is None or self.stats.device != x.device or self.need > self.stats.numel():
                self.stats = torch.zeros(max(self.need * 2, 1 << 16), dtype=torch.int64, device=x.device)
            else:
                self.stats.zero_()
            self.acc = self.stats
        self.cursor = self.need = 0
        RUN.arena = None
        if training and cuda and torch.is_grad_enabled():
            dt = compute_dtype(x)
            a = self.arena
            if a is None or (a.dtype is not None and a.dtype != dt) or (a.built and a.stale()):  # (stale: parameter storage moved - model.to() ...)
                a = self.arena = WeightArena()
            elif not a.built and a.specs:
                a.build()
            if a.built:
                a.pack()
            RUN.arena = a
        prev, RUN.model = RUN.model, self
        try:
            yield self
        finally:
            RUN.model, self.acc = prev, None
            pending, self.counters = self.counters, []
            if pending:
                torch._foreach_add_(pending, 1)


def set_weight_arena(arena):
    """the WeightArena the packers read until the next model forward, which sets its own (ModelState.forward); None: per-call packs."""
    RUN.arena = arena


def pack_conv_fwd(weight, cin_pad, dtype):
    arena = RUN.arena
    if arena is not None:
        hit = arena.lookup_fwd(weight, cin_pad, dtype)
        if hit is not None:
            return hit
        arena.note(weight, dtype, ipad=cin_pad)
    weight = _as4d(weight)
    o, i, kh, kw = weight.shape
    buf = torch.empty(o * kh * kw * cin_pad, dtype=dtype, device=weight.device)
    check(L().ymi_pack_conv_weight_fwd(ptr(weight.detach()), o, i, kh, kw, cin_pad, ymi_dtype(dtype), ptr(buf), stream_ptr()), "pack_conv_weight_fwd")
    return buf


def pack_conv_dgrad(weight, cout_pad, stride, dtype):
    arena = RUN.arena
    if arena is not None:
        hit = arena.lookup_dgrad(weight, cout_pad, stride, dtype)
        if hit is not None:
            return hit
        arena.note(weight, dtype, opad=cout_pad, stride=stride)
    weight = _as4d(weight)
    o, i, kh, kw = weight.shape
    buf = torch.empty(cout_pad * i * kh * kw, dtype=dtype, device=weight.device)
    check(L().ymi_pack_conv_weight_dgrad_ex(ptr(weight.detach()), o, cout_pad, i, kh, kw, stride, ymi_dtype(dtype), ptr(buf), stream_ptr()), "pack_conv_weight_dgrad")
    return buf


def pack_conv_fwd_pair(wa, wb, cin_pad, dtype):
    """forward operand of two convolutions of one input run as ONE: [oA + oB][kh][kw][cin_pad] (a view of the arena once it is built)."""
    arena = RUN.arena
    if arena is not None:
        hit = arena.lookup_fwd(wa, cin_pad, dtype, pair=wb)
        if hit is not None:
            return hit
        arena.note(wa, dtype, ipad=cin_pad, pair=wb)
    w = torch.cat([wa.detach(), wb.detach()], 0)  # (only until the arena exists - the warm-up steps - and in stand-alone use: never inside a captured graph)
    o, i, kh, kw = w.shape
    buf = torch.empty(o * kh * kw * cin_pad, dtype=dtype, device=w.device)
    check(L().ymi_pack_conv_weight_fwd(ptr(w), o, i, kh, kw, cin_pad, ymi_dtype(dtype), ptr(buf), stream_ptr()), "pack_conv_weight_fwd")
    return buf


def pack_conv_dgrad_pair(wa, wb, stride, dtype):
    """data-gradient operand of the pair: [i][tap][oA + oB] per stride-parity class."""
    otot = wa.shape[0] + wb.shape[0]
    arena = RUN.arena
    if arena is not None:
        hit = arena.lookup_dgrad(wa, otot, stride, dtype, pair=wb)
        if hit is not None:
            return hit
        arena.note(wa, dtype, opad=otot, stride=stride, pair=wb)
    w = torch.cat([wa.detach(), wb.detach()], 0)
    o, i, kh, kw = w.shape
    buf = torch.empty(o * i * kh * kw, dtype=dtype, device=w.device)
    check(L().ymi_pack_conv_weight_dgrad_ex(ptr(w), o, o, i, kh, kw, stride, ymi_dtype(dtype), ptr(buf), stream_ptr()), "pack_conv_weight_dgrad")
    return buf


# Where weight gradients should be WRITTEN: {id(parameter): float32 tensor of the parameter's shape}.  engine.trainer's several-rank
# schedule registers the slices of its flat all-reduce buckets here, so that a weight gradient is born inside its bucket and no pack
# copy of the 53.6 MB of gradients is needed before the exchange (RUN.grad_views; None: fresh tensors).
@contextlib.contextmanager
def _setting(name, value):
    """RUN.<name> = value inside the context, the previous value after it."""
    prev = getattr(RUN, name)
    setattr(RUN, name, value)
    try:
        yield
    finally:
        setattr(RUN, name, prev)


def grad_arena(views):
    return _setting("grad_views", views)


def _new_dw(cout, cin, k, dev, params, pair_rows):
    if RUN.grad_views is not None and not pair_rows and params and params[0] is not None:
        v = RUN.grad_views.get(id(params[0]))
        if v is not None and v.numel() == cout * cin * k * k and v.dtype == torch.float32 and v.is_contiguous() and v.device == dev:
            return v.view(cout, cin, k, k)
    return torch.empty((cout, cin, k, k), dtype=torch.float32, device=dev)


def _wgrad(x, dy, cout, cin, k, stride, want_bias, params=(), pair_rows=None):
    """-> (dw [cout, cin, k, k] f32, dbias [cout] f32 | None).  params: the parameters these gradients belong to.
    pair_rows: params are TWO weights whose gradients are the row ranges [0, pair_rows) and [pair_rows, cout) of dw (_ConvBnActPair)."""
    if RUN.defer and _in_backward() and _adoptable(params) and not _deferred_twice(params):
        owner = (params[0], params[1], int(pair_rows)) if pair_rows else (params[0] if params else None)
        bias_owner = params[1] if (want_bias and not pair_rows and len(params) > 1) else None
        return _wgrad_deferred(x, dy, cout, cin, k, stride, want_bias, owner, _new_dw(cout, cin, k, x.device, params, pair_rows), bias_owner)
    dev = x.device
    dw = _new_dw(cout, cin, k, dev, params, pair_rows)
    ty, tx = as_ymi(dy), as_ymi(x)
    db = torch.empty(ty.c, dtype=torch.float32, device=dev) if want_bias else None  # (column sums of every channel of dy, padded ones included)
    need = L().ymi_conv2d_bwd_weight_workspace(ty.n * ty.h * ty.w, ty.c, tx.c, k, k)
    ws = workspace(need, dev, "wgrad")
    check(L().ymi_conv2d_bwd_weight(_byref(tx), _byref(ty), cout, cin, k, k, stride, ptr(dw), ptr(db), ptr(ws), ws.numel(), stream_ptr()), "conv2d_bwd_weight")
    return dw, (db[:cout] if want_bias else None)


def _adoptable(params):
    """True when AccumulateGrad will adopt freshly returned gradient tensors of these parameters as `.grad` WITHOUT reading
    them during the pass: no gradient accumulated yet, and no hooks that run when the gradient arrives."""
    for p in params:
        if p is None:
            continue
        if not p.requires_grad:
            # autograd drops the returned tensor at once: a deferred slab sum would later write into memory the allocator has
            # already handed to another tensor of the pass (round-3 ADVICE)
            return False
        if p.grad is not None or getattr(p, "_backward_hooks", None) or getattr(p, "_post_accumulate_grad_hooks", None):
            return False
    return True


# ---- weight gradients on a second stream ------------------------------------------------------------------------
# Inside `async_wgrad()` (the training step's backward) every weight-gradient GEMM (+ its slab reduce) is enqueued on a
# side stream that forks from the current one: it depends only on (x, dz), and nothing downstream needs dW before the
# optimizer, while the data-gradient / BatchNorm chain of the next layers continues on the current stream.  The small
# 20x20 / 40x40 layers leave CUs idle in their tails; two independent kernel chains fill them.  Captured in a HIP graph
# this becomes a parallel branch.  The operands are kept alive until the join so the allocator cannot hand their memory
# to the main stream while the side stream still reads them.
def _side_stream(dev):
    s = RUN.side_streams.get(dev.index)
    if s is None:
        s = RUN.side_streams[dev.index] = torch.cuda.Stream(device=dev)
    return s


@contextlib.contextmanager
def async_wgrad(enabled=True):
    with _setting("side", bool(enabled)):
        try:
            yield
        finally:
            join_side_stream()


def join_side_stream():
    """make the current stream wait for the weight-gradient stream (no-op when nothing is pending)."""
    if RUN.side_pending:
        cur = torch.cuda.current_stream()
        cur.wait_stream(_side_stream(cur.device))
        RUN.side_pending = False
        RUN.side_keep.clear()


def _wgrad_maybe_async(x, dy, cout, cin, k, stride, want_bias, params=(), pair_rows=None):
    if not RUN.side:
        return _wgrad(x, dy, cout, cin, k, stride, want_bias, params, pair_rows)
    cur = torch.cuda.current_stream()
    side = _side_stream(x.device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        out = _wgrad(x, dy, cout, cin, k, stride, want_bias, params, pair_rows)
    RUN.side_keep.append((x, dy))
    RUN.side_pending = True
    return out


# ---- slab sums of ALL weight gradients of a backward pass in one launch ---------------------------------------------
# Inside `deferred_wgrad()` every weight-gradient GEMM of a backward pass leaves its split-K slabs un-summed and registers a
# record; a callback the autograd engine runs when the pass ends (before backward() returns) sums them all with ONE launch
# (ymi_wgrad_reduce_batch).  Until then the returned dW tensors hold no data.  That is only safe when NOTHING reads a weight
# gradient before the pass is over:
#   * AccumulateGrad must adopt the tensor as `.grad` (p.grad is None when the pass starts).  With gradient accumulation
#     - a second backward() before zero_grad, as the reference trainer does for nbs / batch > 1 (trainer.py:305,397) -
#     AccumulateGrad runs `p.grad += dw` DURING the pass and would read the unfilled tensor;
#   * no post-accumulate-grad hooks (the overlapped DDP schedule of engine/ddp.py) and no tensor hooks on parameters.
# So the deferral is OPT-IN: engine.trainer.TrainStep, which zeroes gradients with set_to_none=True after every step and
# knows its DDP schedule, enables it around its backward.  Everywhere else (plain autograd use of the modules, gradient
# accumulation, hooks) each weight gradient is complete when its Function returns.
def deferred_wgrad(enabled=True):
    """context manager: batch the split-K slab sums of every weight gradient of the backward passes run inside it.  The
    caller guarantees the conditions above; parameters that already hold a gradient are detected by _wgrad and not deferred."""
    return _setting("defer", bool(enabled))


@contextlib.contextmanager
def wgrad_riders(enabled=True):
    """context manager around a backward pass with deferred weight gradients on ONE stream (engine.trainer.TrainStep's captured steps): the
    library holds each deferred weight-gradient launch back until the next BatchNorm backward, whose final pass then rides in it
    (include/ymi.h: ymi_wgrad_hold).  Leaving the context issues a launch still held."""
    enabled = bool(enabled) and HOOKS["wgrad_rider"]
    with _setting("riders", enabled):
        if enabled:
            check(L().ymi_wgrad_hold(1), "wgrad_hold")
        try:
            yield
        except BaseException:
            if enabled:
                check(L().ymi_wgrad_hold(2), "wgrad_hold")
                L().ymi_wgrad_hold(0)
            raise
        if enabled:
            check(L().ymi_wgrad_hold(0), "wgrad_hold")


def _take_pass():
    """-> (records, keep-alives, owners, bias) of the current pass, which RUN no longer holds."""
    out = RUN.records, RUN.keep, RUN.owners, RUN.bias
    RUN.records, RUN.keep, RUN.owners, RUN.bias, RUN.task = [], [], [], [], None
    return out


def _discard_stale_pass():
    """records of an earlier pass whose end-of-pass callback never ran (the engine drops callbacks when a backward raises) are stale:
    their gradient tensors are gone - discard them, and a launch the library still holds back for a rider: it belongs to that pass too."""
    if RUN.records:
        L().ymi_wgrad_hold(2)
    _take_pass()


def _defer_wgrad(rec, keep, owner, bias=None):
    """register a deferred slab sum with the running backward pass BEFORE its launch fills `rec` (the first of a pass queues the flush).
    keep: slabs and operands, alive until the flush has been enqueued; owner: the weight (see _flush_wgrads); bias: (bias parameter,
    bias-gradient buffer, real width) | None."""
    task = torch._C._current_graph_task_id()
    if RUN.task != task:
        _discard_stale_pass()
        torch.autograd.Variable._execution_engine.queue_callback(_flush_wgrads)
        RUN.task = task
    RUN.records.append(rec)
    RUN.keep.append(keep)
    RUN.owners.append(owner)
    RUN.bias.append(bias)


def _flush_wgrads():
    recs, keep, owners, biases = _take_pass()
    if not recs:
        return
    # Every node of the pass has run: a parameter's AccumulateGrad has either ADOPTED the returned tensor (p.grad is that
    # memory - the usual case, and the reason the tensor must not be referenced from here: a second reference makes
    # AccumulateGrad clone it) or, if the gradient layout contract failed, stored a clone of the still unfilled tensor and
    # dropped the original.  In the second case the sum is written straight into p.grad instead of into freed memory.
    for rec, owner in zip(recs, owners):
        if isinstance(owner, tuple):
            # two parameters share one [oA + oB, ...] result as its two row ranges (_ConvBnActPair): both must have ADOPTED their view -
            # a cloned half cannot be redirected (the sum is one write of the whole tensor), so that case is refused loudly
            pa, pb, rows = owner
            per_row = rec.cin_real * rec.ntaps * 4
            if pa.grad is None and pb.grad is None:
                continue  # (torch.autograd.grad: the two views are handed to the caller as they are, nothing was accumulated)
            ok = (pa.grad is not None and pb.grad is not None and pa.grad.data_ptr() == rec.dw and pb.grad.data_ptr() == rec.dw + rows * per_row)
            if not ok:
                raise RuntimeError("deferred weight gradient of a convolution pair: AccumulateGrad did not adopt both halves of the result")
            continue
        g = owner.grad if owner is not None else None
        if g is not None and g.data_ptr() != rec.dw and g.dtype == torch.float32 and g.is_contiguous():
            rec.dw = g.data_ptr()
    dev = keep[0][0].device
    n = len(recs)
    tab = RUN.table
    if tab is None or tab.device != dev or tab.numel() < n * ctypes.sizeof(_lib.WgradPending):
        tab = RUN.table = torch.empty(max(n, 128) * ctypes.sizeof(_lib.WgradPending), dtype=torch.uint8, device=dev)
    arr = (_lib.WgradPending * n)(*recs)
    def late_bias():
        # bias gradients are summed by the batched launch too (into the buffer their Function returned a view of).  Usually AccumulateGrad
        # adopted that view; where it stored a clone instead, the clone gets the finished sum here
        for b in biases:
            if b is not None and b[0] is not None:
                g = b[0].grad
                if g is not None and g.data_ptr() != b[1].data_ptr():
                    g.copy_(b[1][: b[2]])

    if RUN.side:  # the GEMMs ran on the side stream: the sum follows them there (joined by async_wgrad's exit)
        # (slabs produced on the CURRENT stream - the first layer's fused backward - must be complete too)
        _side_stream(dev).wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(_side_stream(dev)):
            check(L().ymi_wgrad_reduce_batch(arr, n, ptr(tab), stream_ptr()), "wgrad_reduce_batch")
            late_bias()
        RUN.side_pending = True
    else:
        check(L().ymi_wgrad_reduce_batch(arr, n, ptr(tab), stream_ptr()), "wgrad_reduce_batch")
        late_bias()
    del keep


def _wgrad_deferred(x, dy, cout, cin, k, stride, want_bias, owner=None, dw=None, bias_owner=None):
    """as _wgrad, with the slab sum left to the end of the backward pass.  The gradient tensor itself is owned by autograd (see
    _flush_wgrads).  owner: the weight."""
    dev = x.device
    if dw is None:
        dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=dev)
    ty, tx = as_ymi(dy), as_ymi(x)
    db = torch.empty(ty.c, dtype=torch.float32, device=dev) if want_bias else None
    need = L().ymi_conv2d_bwd_weight_workspace(ty.n * ty.h * ty.w, ty.c, tx.c, k, k)
    ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
    rec = _lib.WgradPending()
    # (db, the BASE of the returned bias-gradient view, stays referenced until the flush: the batched sum also writes the bias gradient
    # - its per-split partials come out of the GEMM - so that memory must not return to the allocator first; holding the base does not
    # keep AccumulateGrad from adopting the view)
    _defer_wgrad(rec, (ws, x, dy, db), owner, (bias_owner, db, cout) if want_bias else None)
    check(L().ymi_conv2d_bwd_weight_deferred(_byref(tx), _byref(ty), cout, cin, k, k, stride, ptr(dw), ptr(db), ptr(ws), ws.numel(), _byref(rec), stream_ptr()),
          "conv2d_bwd_weight")
    return dw, (db[:cout] if want_bias else None)
