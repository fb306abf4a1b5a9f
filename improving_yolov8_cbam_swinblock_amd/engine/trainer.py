"""Training step of the hot path (reference: ultralytics/engine/trainer.py:383-399,614-622,788-849 and
models/yolo/detect/train.py:90-115), reduced to what the benchmark step needs: bf16 autocast forward,
v8 detection loss, backward (+ RCCL gradient mean), gradient clip 10.0, SGD-nesterov step, EMA update."""
import collections
import contextlib
import math
import os
import random

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops
from ..nn.modules.head import OBB, Segment
from .ddp import GradientBuckets
from .optim import FlatFold, FusedAdamax, FusedAdamW, FusedNAdam, FusedRAdam, FusedRMSprop, FusedSGD, ModelEMA

# weight-gradient GEMMs on a second stream during backward (ops.async_wgrad) in EAGER steps; YMI_WGRAD_STREAM=0 keeps
# one stream.  Graph-replayed steps stay single-stream: measured no wall-time gain there, and concurrent kernels stretch
# each other's durations, which would blur the per-kernel roofline measurement.
ASYNC_WGRAD = os.environ.get("YMI_WGRAD_STREAM", "1") != "0"


def build_optimizer(model, name="SGD", lr=0.01, momentum=0.937, decay=5e-4, ema=None, iterations=1e5, nc=None):
    """reference build_optimizer (trainer.py:788-849) + optimizer_step's clip (:617): three parameter groups (biases, decayed
    weights, norm weights) and
      * 'SGD'  (:832-833)  nesterov momentum, as the fused HIP step FusedSGD;
      * 'AdamW' / 'Adam' (:829-830)  betas = (momentum, 0.999), as FusedAdamW;
      * 'Adamax' / 'NAdam' / 'RAdam' (:829-830) and 'RMSProp' (:831-832) with torch's default hyper-parameters, as FusedAdamax / FusedNAdam /
        FusedRAdam / FusedRMSprop (the same three launches, another compiled rule);
      * 'auto' (:804-813)  SGD(lr 0.01, momentum 0.9) for more than 10000 iterations, else AdamW(lr = round(0.002 * 5 / (4 + nc), 6),
        beta1 0.9) - the caller's lr / momentum are ignored, as in the reference.
    The gradients the step is handed are already the mean over ranks (GradientBuckets.finish divides once), so the step itself
    never scales by the world size."""
    if name == "auto":
        if nc is None:
            nc = getattr(model, "nc", None) or getattr(model.model[-1], "nc", 10)
        lr_fit = round(0.002 * 5 / (4 + nc), 6)
        name, lr, momentum = ("SGD", 0.01, 0.9) if iterations > 10000 else ("AdamW", lr_fit, 0.9)
    known = {x.lower(): x for x in ("Adam", "Adamax", "AdamW", "NAdam", "RAdam", "RMSProp", "SGD")}
    name = known.get(str(name).lower())
    if name == "SGD":
        return FusedSGD(model, lr=lr, momentum=momentum, decay=decay, nesterov=True, max_norm=10.0, ema=ema)
    if name in ("AdamW", "Adam"):
        return FusedAdamW(model, lr=lr, betas=(momentum, 0.999), decay=decay, max_norm=10.0, ema=ema, decoupled=name == "AdamW")
    if name in ("Adamax", "NAdam", "RAdam"):  # trainer.py:829-830: getattr(optim, name)(g[2], lr=lr, betas=(momentum, 0.999), weight_decay=0.0)
        cls = {"Adamax": FusedAdamax, "NAdam": FusedNAdam, "RAdam": FusedRAdam}[name]
        return cls(model, lr=lr, betas=(momentum, 0.999), decay=decay, max_norm=10.0, ema=ema)
    if name == "RMSProp":  # trainer.py:831-832: optim.RMSprop(g[2], lr=lr, momentum=momentum)
        return FusedRMSprop(model, lr=lr, momentum=momentum, decay=decay, max_norm=10.0, ema=ema)
    raise NotImplementedError(f"optimizer {name!r} is not one of the reference's (trainer.py:827-840)")


def synthetic_batch(batch, imgsz, device, seed, boxes_per_image=4):
    """the synthetic batch of SURVEY.md section 8(d) config 3: U[0,1) images, 4 boxes per image, class 0."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(batch, 3, imgsz, imgsz, generator=g)
    n = batch * boxes_per_image
    ctr = torch.rand(n, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(n, 2, generator=g) * 0.3 + 0.05
    return {
        "img": img.to(device),
        "batch_idx": torch.arange(batch).repeat_interleave(boxes_per_image).float().to(device),
        "cls": torch.zeros(n, 1, device=device),
        "bboxes": torch.cat((ctr, wh), 1).to(device),
        "max_boxes": boxes_per_image,
    }


def synthetic_seg_batch(batch, imgsz, device, seed, boxes_per_image=4):
    """synthetic_batch with "masks": the overlap encoding [B, imgsz / 4, imgsz / 4] uint8 of an ellipse inscribed in every box (pixel value =
    1 + index of the box among its image's labels, later boxes on top) - the batch a SegmentationModel trains on."""
    out = synthetic_batch(batch, imgsz, device, seed, boxes_per_image)
    m = imgsz // 4
    c = (torch.arange(m, dtype=torch.float32, device=device) + 0.5) / m
    boxes = out["bboxes"].view(batch, boxes_per_image, 4)
    masks = torch.zeros(batch, m, m, dtype=torch.uint8, device=device)
    for k in range(boxes_per_image):
        cx, cy, bw, bh = (boxes[:, k, i].view(batch, 1, 1) for i in range(4))
        inside = ((c.view(1, 1, m) - cx) / (bw / 2)) ** 2 + ((c.view(1, m, 1) - cy) / (bh / 2)) ** 2 <= 1.0
        masks[inside] = k + 1
    out["masks"] = masks
    return out


def synthetic_obb_batch(batch, imgsz, device, seed, boxes_per_image=4):
    """synthetic_batch with oriented labels: "bboxes" [n, 5] = (xywh normalised, angle in radians drawn from [-pi/4, 3pi/4), the range of the
    OBB head's output) - the batch an OBBModel trains on."""
    out = synthetic_batch(batch, imgsz, device, seed, boxes_per_image)
    g = torch.Generator().manual_seed(seed + 1)
    r = (torch.rand(batch * boxes_per_image, 1, generator=g) - 0.25) * math.pi
    out["bboxes"] = torch.cat((out["bboxes"], r.to(device)), 1)
    return out


def preprocess_batch(batch, imgsz, stride, multi_scale=False, rng=random, device=None):
    """DetectionTrainer.preprocess_batch of reference models/yolo/detect/train.py:90-115 -> a NEW dict whose "img" is float32 NCHW on the
    device: a uint8 image batch (what a dataloader produces; host or device) becomes img.float() / 255, and with multi_scale the batch is
    stretched bilinearly to a size drawn as the reference draws it - the same `random.seed` gives the same sizes:
        sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5 + stride)) // stride * stride;  sf = sz / max(h, w);
        no resize when sf == 1, else to ceil(x * sf / stride) * stride per side.
    Conversion and resize are ONE launch (ops.scale_image): no float copy of the input size is made on the way.  A float32 image is taken as
    already normalised.  Labels are normalised coordinates and pass through untouched.  The result is what layer 0's direct kernels take
    (ops.first_conv_ok).  device: where a host batch goes (default: the current cuda device)."""
    img = batch["img"]
    if img.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"preprocess_batch takes uint8 or float32 images, got {img.dtype}")
    if not img.is_cuda:
        img = img.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
    h, w = (int(v) for v in img.shape[2:])
    ns = (h, w)
    if multi_scale:
        stride = int(stride)
        sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5 + stride)) // stride * stride
        sf = sz / max(h, w)
        if sf != 1:
            ns = tuple(math.ceil(x * sf / stride) * stride for x in (h, w))
    if ns != (h, w) or img.dtype == torch.uint8 or not img.is_contiguous():
        img = ops.scale_image(img, ns)
    out = dict(batch)
    out["img"] = img
    return out


def augment_batch(samples, imgsz, hyp=None, mosaic=True, transforms=None, device=None):
    """A training batch from loaded images, augmented on the device as the reference's v8_transforms does at its defaults (data/augment.py
    :2375-2439: mosaic, scale / translate (/ rotate / shear), HSV, flips) -> the dict TrainStep.__call__ takes, "max_boxes" set.
    samples[i]: {"img": (h, w, 3) uint8 BGR, "labels" [n, 5] = (cls, xywh normalised) or "cls" + "bboxes", "mix_labels": its three mosaic
    partners, likewise} - the data loader picked the partners, so Mosaic's own pick is not drawn here (data.augment.v8_transforms(dataset,
    ...)() draws it too, for a caller that lets the stream choose).  hyp: mapping or namespace with the reference's names; missing ones take
    the reference's defaults.  mosaic=False is hyp.mosaic = 0.  A sample whose mosaic test fails is letterboxed to imgsz by ops.letterbox and
    then warped alone with border 0, as RandomPerspective's pre_transform does (:1220-1221).  The draws consume `random` / `np.random`."""
    from ..data.augment import V8_DEFAULTS, v8_transforms

    for smp in samples:
        lab, box = smp.get("labels"), smp.get("bboxes")
        if (lab is not None and len(lab) and lab.shape[-1] == 6) or (box is not None and len(box) and box.shape[-1] == 5):
            raise NotImplementedError("augment_batch warps axis-aligned (cls, xywh) labels: oriented xywhr rows would need their corners warped and "
                                      "refitted (the reference's segment-based path), which is not built")
    if transforms is None:
        h = dict(V8_DEFAULTS)
        h.update(hyp if isinstance(hyp, dict) else {k: getattr(hyp, k) for k in V8_DEFAULTS if hasattr(hyp, k)} if hyp is not None else {})
        if not mosaic:
            h["mosaic"] = 0.0
        transforms = v8_transforms(None, imgsz, h)
    params = [transforms(pick_partners=False) for _ in samples]
    alone = [i for i, p in enumerate(params) if p["mosaic"] is None]
    samples = list(samples)
    if alone:  # pre_transform: LetterBox(new_shape=(imgsz, imgsz)), the grey levels kept in the image's own channel order
        boxed, ratio_pad = ops.letterbox([samples[i]["img"] for i in alone], (imgsz, imgsz), bgr=False, normalize=False, device=device)
        boxed = boxed.permute(0, 2, 3, 1).to(torch.uint8).contiguous()
        for j, i in enumerate(alone):
            smp = {k: v for k, v in samples[i].items() if k != "mix_labels"}
            smp.update(img=boxed[j], ori_shape=tuple(int(v) for v in samples[i]["img"].shape[:2]), ratio_pad=ratio_pad[j])
            samples[i] = smp
    out = ops.augment_batch(samples, params, imgsz, device=device)
    return {k: out[k] for k in ("img", "batch_idx", "cls", "bboxes", "max_boxes")}


class _CapturedShape:
    """what TrainStep keeps per image shape, and the only place it keeps it: the static batch (adopted from the first batch of the shape), and
    - filled in by the capture - the loss items the graphs write, the shape's plain-step graphs (graph: the full step, or graph="tail"'s
    forward + backward, or G1; graph2: G2) and, for graph="tail", the gradient tensors its graph rewrites in place."""

    __slots__ = ("static", "items", "graph", "graph2", "grads")

    def __init__(self, static):
        self.static = static
        self.items = self.graph = self.graph2 = self.grads = None


class TrainStep:
    """one optimisation step: forward under autocast, loss.sum() * world (reference trainer.py:386-388), backward
    with bucketed RCCL mean, then the reference's optimizer_step (trainer.py:614-622) as the fused HIP step: global-norm
    clip 10.0 (bf16 needs no GradScaler), SGD-nesterov over the three parameter groups, EMA update; zero_grad.

    graph=True replays the step as a HIP graph (every kernel of libyolo_mi355 only enqueues on the stream it is
    given, so the capture is legal; needs static shapes: batch["max_boxes"] must be set):
      * one rank: the whole step (forward, loss, backward, clip, update, EMA) is one graph;
      * several ranks (or graph="split": the same schedule on one rank, for tests): THREE graphs with the RCCL calls - which cannot
        be captured - between them, so that the exchange overlaps compute as the reference's DDP reducer does (trainer.py:278):
          G1  forward + loss + the HEAD's backward (down to the backbone / head boundary of the YAML), head gradients copied
              into bucket 0's flat buffer                     -> all-reduce of bucket 0 starts (RCCL's own stream)
          G2  the BACKBONE's backward, its gradients copied into bucket 1's flat buffer (runs beside bucket 0's all-reduce)
                                                              -> all-reduce of bucket 1 starts
          G3  clip + update + EMA reading the gradient SUMS from the flat buffers (the step scales by 1 / world itself)
        The backward is split with torch.autograd.grad at the boundary tensors (BaseModel.boundary_layers); gradient joins of
        boundary tensors (ops.GradJoin) carry the head's contribution into the backbone's pass.
      * graph="tail": the round-3 multi-rank form (forward + backward as one graph, gradient mean and update eager behind it).
    Every captured call goes the same way: `_select` finds the record (_CapturedShape) of batch["img"]'s shape in `_shapes` and loads the
    batch into its static tensors - or makes the record, which adopts the batch's tensors - and the record's graphs replay (`_replay`).  A
    record without graphs gets them from `_capture`, the one capture routine, which expects the record's batch to have just been applied
    eagerly (`_settle` behind it) and executes nothing.  Helpers are handed the record; nothing of a shape is kept on the step itself.
    image_shapes=N (multi-scale training, preprocess_batch(multi_scale=True)) is how many records there may be: up to N distinct shapes of
    batch["img"] are captured, one graph (two with the split schedule; the update graph G3 reads no activation and is shared) per shape.  A
    batch of a NEW shape is applied exactly once: as an eager step, after which that shape's graphs are captured WITHOUT being executed; later
    batches of the shape replay.  Everything that does not depend on the activation shape - parameters, optimizer state, the EMA, the weight
    arena, the gradient buckets - is shared by all shapes' graphs, which also share the first graph's memory pool.  Label tensors and
    max_boxes stay static across all shapes.  Scratch buffers are the hazard: `_lib.workspace` and the model's statistics arena REPLACE a
    buffer when a larger shape asks for more, while the smaller shape's graph still holds the old address, so every capture keeps what its
    launches address alive (_hold_captured).  The default, image_shapes=1, is the same path with one record and another warm-up policy: the
    first plain call applies its batch with 3 eager steps (allocator, lazy state, workspaces), captures, and replays.
    Learning rates / momentum changed through `opt.param_groups` reach a replayed graph: they are read from a device
    array (`FusedSGD.sync_hyper`).

    What must NOT be inside a captured region (found in round 2, tools/graph_cat_probe.py): torch.cat / torch.stack -
    and therefore torch.nn.utils.clip_grad_norm_.  On this ROCm build ATen's cat stages its tensor metadata through a
    host buffer that a memcpy NODE copies to the device; a replay copies whatever that host buffer holds by then (any
    later eager cat/stack rewrites it), so the replayed cat reads wrong pointers: silently wrong values, or a memory
    fault.  The captured step contains only kernels of this library and elementwise ATen ops."""

    def __init__(self, model, world_size=1, lr=0.01, dtype=torch.bfloat16, bucket_bytes=32 << 20, graph=False, ema=True, optimizer="SGD",
                 momentum=0.937, decay=5e-4, image_shapes=1):
        self.model = model
        self.world = world_size
        self.dtype = dtype
        self.ema = ModelEMA(model) if ema is True else (ema or None)
        self.opt = build_optimizer(model, name=optimizer, lr=lr, momentum=momentum, decay=decay, ema=self.ema)
        self.use_graph = bool(graph)
        self.segment = isinstance(model.model[-1], Segment)
        if self.segment and (world_size != 1 or graph == "tail"):
            # (built and tested: eager, graph=True and graph="split" on one rank)
            raise NotImplementedError('TrainStep on a SegmentationModel is built for one rank, eager, graph=True or graph="split": '
                                      f"world_size={world_size}, graph={graph!r} is not")
        self.obb = isinstance(model.model[-1], OBB)
        if self.obb and (world_size != 1 or graph == "tail" or int(image_shapes) != 1):
            # (built and tested: eager, graph=True and graph="split" on one rank, one image shape)
            raise NotImplementedError('TrainStep on an OBBModel is built for one rank and one image shape, eager, graph=True or graph="split": '
                                      f"world_size={world_size}, graph={graph!r}, image_shapes={image_shapes} is not")
        self.full_graph = self.use_graph and world_size == 1 and graph not in ("split", "tail")
        self.overlap_graphs = self.use_graph and not self.full_graph and graph != "tail"
        self.params = [p for p in model.parameters() if p.requires_grad]
        groups = None
        if self.overlap_graphs:
            # bucket 0 = the head's parameters (their gradients are complete when G1 ends), bucket 1 = the backbone's
            nb = len(model.yaml["backbone"])
            head_ids = {id(p) for m in model.model if m.i >= nb for p in m.parameters()}
            self._head_params = [p for p in reversed(self.params) if id(p) in head_ids]
            self._back_params = [p for p in reversed(self.params) if id(p) not in head_ids]
            self._boundary = model.boundary_layers()
            groups = [self._head_params, self._back_params]
        self.buckets = GradientBuckets(model, world_size, bucket_bytes, overlap=not self.use_graph, groups=groups)
        # the buckets hold gradient SUMS over ranks; the fused step applies 1 / world (the grad scale of its hyper array) - no divide launches
        self.opt.world = world_size
        self._seed = None
        self._held = []  # model-side buffers the captured graphs write (_hold_captured)
        self.image_shapes = int(image_shapes)
        if self.image_shapes < 1:
            raise ValueError("image_shapes counts the image shapes a graph is kept for: at least 1")
        if self.image_shapes > 1 and self.use_graph and not (self.full_graph or self.overlap_graphs):
            raise ValueError('graph="tail" replays one static shape: image_shapes > 1 needs graph=True or graph="split"')
        self._shapes = {}  # tuple(img.shape) -> _CapturedShape, at most image_shapes of them; the first one's graph owns the memory pool
        self._graph3 = None  # the split schedule's update graph, shared by all shapes
        # several ranks: the process group's watchdog thread polls its events while this thread captures; only this thread's calls may
        # invalidate the capture
        self._capture_mode = "global" if world_size == 1 else "thread_local"
        self._comm_events = None  # time_exposed_communication(): [(event after the backward's last graph, event after the wait for the buckets)]
        # gradient accumulation (update=False): nothing of it exists until a micro-step is asked for
        self._micro = self._micro_items = self._update_graph = self._micro_table = None  # graph=True: forward + backward + fold; step from the arena + clear
        self._flat_arena = self._flat_fold = None                    # split schedule: the buckets' sums over micro-steps
        self._flat_pending = 0

    def __call__(self, batch, update=True):
        """update=False: a micro-step - forward, loss, backward, the gradients folded into the optimizer's accumulation arena, zero_grad; no
        gradient exchange, no optimizer step, no EMA update.  update=True with micro-steps pending completes the update from the sums."""
        if not update or self.opt.pending or self._flat_pending:
            return self._accumulating_call(batch, update)
        if not self.use_graph:
            return self.eager_step(batch)
        rec = self._select(batch)
        if rec.graph is not None:
            return self._replay(rec)
        # The first plain call of this shape.  image_shapes == 1: 3 warm-up steps (allocator, lazy state, workspaces), capture, replay - the
        # batch is applied 4 times.  image_shapes > 1: the batch is applied exactly once, by the eager step; its graphs serve the batches to come.
        once = self.image_shapes > 1
        for _ in range(1 if once else 3):
            items = self.eager_step(rec.static)
        self._settle()
        self._capture(rec)
        return items if once else self._replay(rec)

    def _replay(self, rec):
        if self.overlap_graphs:
            return self._replay_split(rec)
        if self.full_graph:
            self.opt.sync_hyper()  # scheduler changes reach the captured update through the device array
            rec.graph.replay()
            self.opt.count_updates(+1)  # the captured step advanced the device counter
        else:
            rec.graph.replay()
            self._reduce_and_update(rec.grads)
            self.opt.zero_grad(set_to_none=True)  # drops references only: the graph owns its gradient buffers
        return rec.items

    # ---- static batches and their records ---------------------------------------------------------------------------------------------
    def _select(self, batch):
        """-> the record whose static tensors now hold `batch`: the one of batch["img"]'s shape, loaded; or a new one that adopts the batch's
        own tensors (rec.graph is None: the caller applies the batch eagerly and captures).  The first batch's tensors become the static
        inputs of every graph of that shape, whichever is captured first - later batches are copied into them, so no capture is left
        reading tensors nobody fills any more.  Only the image may change shape: labels and max_boxes are static across all shapes."""
        if batch.get("max_boxes") is None:
            raise ValueError("graph=True needs batch['max_boxes'] (static target shape)")
        if self.segment and not (torch.is_tensor(batch.get("masks")) and batch["masks"].is_cuda):
            raise ValueError("graph=True on a SegmentationModel needs batch['masks'] on the device: it is a static input of the captured graph")
        key = tuple(batch["img"].shape)
        first = next(iter(self._shapes.values()), None)
        # image_shapes == 1: the one record takes every batch - another image shape fails the static-shape check like any other tensor
        rec = self._shapes.get(key) if self.image_shapes > 1 else first
        if rec is not None:
            self._match_static(rec.static, batch)
            return rec
        if len(self._shapes) >= self.image_shapes:
            raise ValueError(f"graph=True with image_shapes={self.image_shapes}: batch['img'] has the new shape {key}, captured are {sorted(self._shapes)}")
        if first is not None:
            self._match_static(first.static, batch, skip=("img",), copy=False)
        rec = self._shapes[key] = _CapturedShape(dict(batch))
        return rec

    @staticmethod
    def _match_static(static, batch, skip=(), copy=True):
        """check `batch` against the static batch a graph reads (keys in `skip` left out) and, with copy, load it into those tensors."""
        for k, v in batch.items():
            ref = static.get(k)
            if k in skip or v is ref:
                continue
            if torch.is_tensor(v):
                if not torch.is_tensor(ref) or v.shape != ref.shape:  # copy_ would broadcast silently (e.g. a shorter label tensor)
                    raise ValueError(f"graph=True replays static shapes: batch['{k}'] is {tuple(v.shape)}, captured {tuple(ref.shape) if torch.is_tensor(ref) else ref!r}")
                if copy:
                    ref.copy_(v)
            elif v != ref:
                raise ValueError(f"graph=True: batch['{k}'] = {v!r} differs from the captured value {ref!r}")

    # ---- capture ------------------------------------------------------------------------------------------------------------------------
    def _settle(self):
        """between the eager application of a batch and a capture: the lazy state a capture must find in place, because its construction
        stages host tables - the weight arena (built from the uses the step recorded), the optimizer's tables, the hyper-parameter array -
        and a synchronised device.  Behind a full eager_step only the arena can still be missing (after ONE step; the second forward
        builds it otherwise): the optimizer built its tables in step(), and sync_hyper() behind a step that just called it stages nothing."""
        arena = self.model._state.arena
        if arena is not None and not arena.built and arena.specs:
            arena.build()
        if self.opt._stale():
            self.opt._build()
        self.opt.sync_hyper()  # a capture must not stage the hyper-parameter array
        torch.cuda.synchronize()

    def _hold_captured(self):
        """a graph just captured launches that write the model's statistics arena, pack into its weight arena and stage the batched slab sum
        in RUN.table, and they address the scratch buffers `_lib.workspace` handed out during the capture: keep all of them referenced for as
        long as the graphs live, whatever the model, a later pass or a larger image shape replaces them with (a workspace is REPLACED when a
        larger request arrives; a replay of the smaller shape's graph would otherwise write memory the allocator has given to someone else)."""
        st = self.model._state
        dev = next(iter(self.params)).device
        self._held.append((st.stats, st.arena, ops.RUN.table, _lib.live_workspaces(dev)))

    def _capture(self, rec):
        """capture the plain step's graphs of rec's shape into rec, WITHOUT executing them: the full step, graph="tail"'s forward + backward,
        or G1 and G2 (and G3, once).  The caller has just applied rec.static eagerly and called _settle().  The first record's graph starts
        a fresh memory pool - also behind a micro graph - and every later shape's graphs share it."""
        first = next(iter(self._shapes.values()))
        pool = first.graph.pool() if first.graph is not None else None
        rec.graph = torch.cuda.CUDAGraph()
        if self.overlap_graphs:
            return self._capture_split(rec, pool)
        with torch.cuda.graph(rec.graph, pool=pool, capture_error_mode=self._capture_mode):
            rec.items = self.eager_step(rec.static) if self.full_graph else self._forward_backward(rec.static)
        self._hold_captured()
        if self.full_graph:
            self.opt.count_updates(-1)  # the capture recorded the update without running it
        else:  # the gradients the replays rewrite in place
            rec.grads = {p: p.grad for p in self.params if p.grad is not None}

    def _capture_split(self, rec, pool):
        """G1 and G2 of rec's shape; G3 reads the flat gradient buckets and the optimizer's own state only - nothing of an activation's
        shape - so the first capture's is replayed for every shape."""
        mode = self._capture_mode
        # conv / linear weight gradients are written straight into the flat buckets (ops.grad_arena): only the small vectors (BatchNorm
        # and LayerNorm parameters, biases, the paired Detect weights) are copied there
        arena = {id(p): v for bi in range(len(self.buckets.buckets)) for p, v in zip(self.buckets.buckets[bi], self.buckets.flat_views(bi)) if p.dim() >= 2}
        with torch.cuda.graph(rec.graph, pool=pool, capture_error_mode=mode), ops.grad_arena(arena):
            rec.items, hg, pairs = self._head_pass(rec.static)
            self._pack(0, self._head_params, hg)
        self._hold_captured()
        del hg
        rec.graph2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(rec.graph2, pool=rec.graph.pool(), capture_error_mode=mode), ops.grad_arena(arena):
            self._backbone_pass(pairs)
            self._pack(1, self._back_params, [p.grad for p in self._back_params])
        self._hold_captured()
        del pairs
        self.buckets.wait_all(divide=False)  # (nothing in flight: points .grad at the flat slices the update graph will read)
        if self._graph3 is None:
            self._graph3 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph3, pool=rec.graph.pool(), capture_error_mode=mode):
                self.opt.step(None)
            self.opt.count_updates(-1)  # captured, not executed
        self.opt.zero_grad(set_to_none=True)

    # ---- gradient accumulation (reference trainer.py:305,397) ------------------------------------------------------------------------
    def _accumulating_call(self, batch, update):
        if self.segment:
            raise NotImplementedError("gradient accumulation (update=False) is not built for a SegmentationModel")
        if self.obb:
            raise NotImplementedError("gradient accumulation (update=False) is not built for an OBBModel")
        if not update:
            if self.use_graph and not (self.full_graph or self.overlap_graphs):
                raise ValueError('update=False is not supported with graph="tail": gradient accumulation needs eager mode, graph=True or graph="split"')
            if self.image_shapes > 1:
                raise ValueError("update=False is not supported with image_shapes > 1: gradient accumulation keeps one static image shape")
            if not self.use_graph and self.world > 1:
                raise ValueError("update=False is not supported eagerly with world_size > 1: the overlapped bucket hooks would start an exchange "
                                 'during micro-steps (use graph=True or graph="split")')
        if not self.use_graph:
            items = self._forward_backward(batch)
            if update:
                self.opt.step()  # micro-steps pending: folds these gradients too, steps from the arena, clears it
            else:
                self.opt.accumulate()
            self.opt.zero_grad(set_to_none=True)
            return items
        rec = self._select(batch)
        if self.overlap_graphs:
            if self._flat_arena is None:
                self._flat_arena = [torch.zeros_like(f) for f in self.buckets._flat]
                self._flat_fold = FlatFold(self._flat_arena + list(self.buckets._flat))
            if rec.graph is None:
                return self._first_split_micro(rec)
            return self._replay_split(rec, update, arena=True)
        if self._micro is None:
            return self._first_micro(rec)
        if self.opt._table is not self._micro_table:
            # FusedSGD._build() (parameters moved) replaced the entry table and dropped the arena: both graphs address the old ones
            raise RuntimeError("the optimizer rebuilt its device tables after the micro and update graphs were captured: make a new TrainStep")
        if update:
            self.opt.sync_hyper()
        self._micro.replay()
        self.opt.pending += 1
        if update:
            # The update graph steps the parameters that had a gradient when it was captured (opt._acc_seen then, restored since and left
            # alone by replays); the micro graph folds exactly those, every time: _first_micro checked that the two sets are one.
            self._update_graph.replay()
            self.opt.pending = 0
            self.opt.count_updates(+1)
        return self._micro_items

    def _first_micro(self, rec):
        """graph=True, the first update=False call: the batch is applied exactly once, as an eager micro-step; after it the micro graph
        (forward + backward + fold + zero_grad) and the shape-independent update graph (step from the arena + clear) are captured WITHOUT
        being executed - the rule a new image shape follows.  The full-step graph is not touched; the micro graph shares its memory pool
        when it exists."""
        items = self._forward_backward(rec.static)
        self.opt.accumulate()
        self.opt.zero_grad(set_to_none=True)
        self._settle()
        folded, self.opt._acc_seen = self.opt._acc_seen, set()  # (to see what the captured fold takes on its own)
        pool = rec.graph.pool() if rec.graph is not None else None
        self._micro, self._micro_table = torch.cuda.CUDAGraph(), self.opt._table
        with torch.cuda.graph(self._micro, pool=pool, capture_error_mode="global"):
            self._micro_items = self._forward_backward(rec.static)
            self.opt.accumulate()
            self.opt.zero_grad(set_to_none=True)
        self._hold_captured()
        pending, seen = self.opt.pending - 1, set(self.opt._acc_seen)  # the capture recorded a fold without running it
        if seen != set(folded):  # (the update graph below steps `seen`; the micro graph folds what its backward produced)
            raise RuntimeError("the captured backward produced gradients for other parameters than the eager micro-step before it")
        self._update_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._update_graph, pool=self._micro.pool(), capture_error_mode="global"):
            self.opt.step_pending()
        self.opt.count_updates(-1)  # captured, not executed
        self.opt.pending, self.opt._acc_seen = pending, seen
        return items

    def _first_split_micro(self, rec):
        """the split schedule, update=False before anything was captured: the batch is applied once as an eager micro-step (each bucket
        packed and folded into the flat arena), then G1 .. G3 are captured unexecuted."""
        items = self._forward_backward(rec.static)
        for bi, params in enumerate(self.buckets.buckets):
            self._pack(bi, params, [p.grad for p in params])
            self._flat_fold.add(bi, self.buckets._flat[bi])
        self.opt.zero_grad(set_to_none=True)
        self._flat_pending += 1
        self._settle()
        self._capture(rec)
        return items

    def discard_pending(self):
        """drop the sums of micro-steps not yet applied."""
        self.opt.discard_pending()
        for a in self._flat_arena or ():
            a.zero_()
        self._flat_pending = 0

    # ---- the three-graph schedule -----------------------------------------------------------------------------------------------
    def _replay_split(self, rec, update=True, arena=False):
        """G1 -> all-reduce of bucket 0 starts -> G2 -> all-reduce of bucket 1 starts -> wait for both -> G3.  arena (gradient accumulation):
        a micro-step (update=False) stops behind G2 and, instead of starting an all-reduce, folds each flat bucket into a flat arena of the
        same layout (one launch per bucket); the updating step adds the arena into the buckets BEFORE their all-reduce, so G3 reads the sums
        it always reads.  The plain step passes neither and touches nothing of the arena."""
        self.opt.sync_hyper()  # scheduler changes reach the captured update through the device array
        nb = len(self.buckets._flat)
        for bi, g in enumerate((rec.graph, rec.graph2)):
            g.replay()
            if not update:
                self._flat_fold.add(bi, self.buckets._flat[bi])
                continue
            if arena:
                self._flat_fold.add(nb + bi, self._flat_arena[bi])  # bucket += sums of the micro-steps
            self.buckets.start(bi)  # the head's gradient sums travel while the backbone's backward runs
        if update:
            ev = self._comm_event_pair()
            if ev:
                ev[0].record()          # (completes when the backbone's backward does)
            self.buckets.wait_all(divide=False)  # the current stream waits for both; .grad = the flat buffers' slices
            if ev:
                ev[1].record()          # (completes once the compute stream may go on: the gap is communication nothing hid)
            self._graph3.replay()
            self.opt.count_updates(+1)
            if arena:
                for a in self._flat_arena:
                    a.zero_()  # after the update has read the buckets the sums went into
                self._flat_pending = 0
        else:
            self._flat_pending += 1
        self.opt.zero_grad(set_to_none=True)
        return rec.items

    def _head_pass(self, batch):
        """forward + loss + the backward of everything behind the backbone / head boundary (the head reads detached leaves of the
        boundary tensors: BaseModel._predict_once) -> (loss items, head gradients aligned with self._head_params,
        [(boundary tensor, gradient the head formed for it)])."""
        model = self.model
        model._taps = dict(self._boundary)
        try:
            loss, items = self._forward(batch)
            taps = model._taps
        finally:
            model._taps = None
        pairs = [v for v in taps.values() if isinstance(v, tuple)]
        leaves = [leaf for _, leaf in pairs]
        # torch.autograd.grad, not backward(): the leaves are channel slices of concat buffers (not dense), and AccumulateGrad would
        # re-lay every gradient it stores for them out as NCHW-contiguous copies; captured gradients are handed over as they are
        with self._wgrad_schedule():
            grads = torch.autograd.grad([loss], leaves + self._head_params, [self._seed], allow_unused=True)
        return items, list(grads[len(leaves):]), [(orig, g) for (orig, _), g in zip(pairs, grads[: len(leaves)])]

    def _backbone_pass(self, pairs):
        """the backbone's backward, from the boundary tensors with the gradients the head left in their leaves.  A boundary tensor that
        also has backbone consumers carries a gradient join: the head's gradient is deposited there and the backbone consumer that
        arrives last adds it in its data-gradient epilogue; the others are roots of the pass."""
        roots, grads = [], []
        for orig, g in pairs:
            if g is None:
                continue
            j = ops.join_of(orig)
            if j is not None:
                adds = j.arrive()
                if adds is None:
                    j.deposit(g)
                    continue
                g = ops._accumulate(g, adds) if adds else g  # (no backbone consumer left to arrive: the head's gradient is the total)
            roots.append(orig)
            grads.append(g)
        with self._wgrad_schedule():
            torch.autograd.backward(roots, grads)

    def _pack(self, bi, params, grads):
        """gradients -> the slices of bucket bi's flat buffer (one multi-tensor copy; parameters without a gradient keep zeros there)."""
        views = self.buckets.flat_views(bi)
        where = {id(p): v for p, v in zip(self.buckets.buckets[bi], views)}
        dst, src = [], []
        for p, g in zip(params, grads):
            if g is not None and not (g.data_ptr() == where[id(p)].data_ptr() and g.dtype == where[id(p)].dtype):  # (weight gradients are born there: ops.grad_arena)
                dst.append(where[id(p)])
                src.append(g if g.dtype == where[id(p)].dtype else g.to(where[id(p)].dtype))
        if dst:
            torch._foreach_copy_(dst, src)

    # ---- forward, backward, update ------------------------------------------------------------------------------------------------------
    def _forward(self, batch):
        """-> (loss, loss items); behind it self._seed is the backward's seed.  The backward of loss.sum() * world (reference
        trainer.py:386-388, 394) is seeded directly with d(total)/d(loss) = world: the sum, the multiplication and their backward nodes
        would be five one-element launches."""
        self.model.train()
        with torch.autocast("cuda", dtype=self.dtype, enabled=self.dtype != torch.float32):
            loss, items = self.model(batch)
        if self._seed is None or self._seed.device != loss.device or self._seed.numel() != loss.numel():  # ([3] detection, [4] segmentation)
            self._seed = torch.full((loss.numel(),), float(self.world), dtype=torch.float32, device=loss.device)
        return loss, items

    @contextlib.contextmanager
    def _wgrad_schedule(self):
        """around every backward pass of the step.  This step owns its gradients: zero_grad(set_to_none=True) after every update, so
        AccumulateGrad adopts the tensors the weight-gradient Functions return and nothing reads them before the pass is over - the
        condition under which their slab sums may be batched into one launch at the end of the pass (ops.deferred_wgrad; parameters that
        do hold a gradient or a hook - the overlapped DDP schedule - are detected there and reduced at once).  Eager steps put the
        weight-gradient GEMMs on a side stream, joined on exit (ops.async_wgrad); captured steps run on one stream, and there the
        BatchNorm-backward final passes ride in the weight-gradient launches (ops.wgrad_riders)."""
        with ops.deferred_wgrad(True), ops.async_wgrad(ASYNC_WGRAD and not self.use_graph), ops.wgrad_riders(self.use_graph):
            yield

    def _forward_backward(self, batch):
        loss, items = self._forward(batch)
        with self._wgrad_schedule():
            torch.autograd.backward([loss], [self._seed])
        return items

    def _reduce_and_update(self, grads_of=None):
        ev = self._comm_event_pair()
        if ev:
            ev[0].record()
        self.buckets.finish(grads_of, divide=False)  # world > 1: leaves the SUM in .grad (views of the flat buckets); the step scales by 1 / world
        if ev:
            ev[1].record()
        self.opt.step(grads_of if self.world == 1 else None)

    def eager_step(self, batch):
        items = self._forward_backward(batch)
        self._reduce_and_update()
        self.opt.zero_grad(set_to_none=True)
        return items

    # ---- exposed-communication probe (bench.py's several-rank line) ---------------------------------------------------------------
    def time_exposed_communication(self, on=True):
        """from now on every step brackets its wait for the gradient exchange with two events on the compute stream: what elapses between them
        is exchange time the backward did not hide (three-graph schedule: behind the backbone's backward; tail / eager: the whole exchange)."""
        self._comm_events = [] if on else None

    def _comm_event_pair(self):
        if self._comm_events is None or self.world == 1:
            return None
        pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self._comm_events.append(pair)
        return pair

    def exposed_communication_ms(self):
        """mean milliseconds per step between the two events (call after a synchronize); None when nothing was timed"""
        ev = self._comm_events or []
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev) if ev else None


ScheduleAt = collections.namedtuple("ScheduleAt", "ni accumulate lrs momentum update")


class WarmupSchedule:
    """the reference trainer's schedule arithmetic as host code, and nothing else (reference engine/trainer.py):
      :305  accumulate = max(round(nbs / batch), 1)
      :306  weight_decay *= batch * accumulate / nbs
      :330  nw = max(round(warmup_epochs * nb), 100) if warmup_epochs > 0 else -1
      :216 / :218  lf: one_cycle(1, lrf, epochs) with cos_lr, else the linear ramp max(1 - x / epochs, 0) * (1 - lrf) + lrf
      :371-380  for ni <= nw: accumulate, the group learning rates (the bias group down from warmup_bias_lr, the others up from 0, towards
                lr0 * lf(epoch)) and the momentum (from warmup_momentum) are np.interp'ed over [0, nw]; np.round: halves go to even
      :397-399  an iteration updates when ni - last_opt_step >= accumulate.
    Outside the warm-up the learning rates are LambdaLR's lr0 * lf(epoch) (:219, :352) and accumulate keeps its last warm-up value.
    `last_opt_step` is the only state: `at()` reads it, `advance()` / `apply()` move it."""

    def __init__(self, epochs, nb, batch, nbs=64, lr0=0.01, lrf=0.01, momentum=0.937, weight_decay=5e-4, warmup_epochs=3.0, warmup_momentum=0.8,
                 warmup_bias_lr=0.1, cos_lr=False):
        self.epochs, self.nb, self.batch, self.nbs = int(epochs), int(nb), batch, nbs
        self.lr0, self.lrf, self.momentum, self.cos_lr = lr0, lrf, momentum, bool(cos_lr)
        self.warmup_momentum, self.warmup_bias_lr = warmup_momentum, warmup_bias_lr
        self.accumulate = max(round(nbs / batch), 1)
        self.weight_decay = weight_decay * batch * self.accumulate / nbs
        self.nw = max(round(warmup_epochs * nb), 100) if warmup_epochs > 0 else -1
        self.last_opt_step = -1

    def lf(self, x):
        if self.cos_lr:
            return max((1 - math.cos(x * math.pi / self.epochs)) / 2, 0) * (self.lrf - 1) + 1
        return max(1 - x / self.epochs, 0) * (1.0 - self.lrf) + self.lrf

    def at(self, epoch, i, warmup_bias_lr=None):
        """-> ScheduleAt(ni, accumulate, [lr of the bias / weight / norm group], momentum, update) of iteration i of `epoch`."""
        ni = i + self.nb * epoch
        target = self.lr0 * self.lf(epoch)
        if ni <= self.nw:
            xi = [0, self.nw]
            bias0 = self.warmup_bias_lr if warmup_bias_lr is None else warmup_bias_lr
            accumulate = max(1, int(np.interp(ni, xi, [1, self.nbs / self.batch]).round()))
            lrs = [float(np.interp(ni, xi, [bias0 if j == 0 else 0.0, target])) for j in range(3)]
            momentum = float(np.interp(ni, xi, [self.warmup_momentum, self.momentum]))
        else:
            accumulate = max(1, int(np.float64(self.nbs / self.batch).round())) if self.nw >= 0 else self.accumulate
            lrs, momentum = [target] * 3, self.momentum
        return ScheduleAt(ni, accumulate, lrs, momentum, ni - self.last_opt_step >= accumulate)

    def advance(self, rec):
        """the iteration `rec` describes has run (:399)."""
        if rec.update:
            self.last_opt_step = rec.ni
        return rec

    def apply(self, opt, epoch, i):
        """write iteration i's values into opt.param_groups and advance -> the ScheduleAt.  As in the reference only groups that have a
        "momentum" key get the momentum; the Adam family (betas instead) warms its bias group up from 0, the reference's warmup_bias_lr for
        the optimizer it picks itself (:816)."""
        has_momentum = "momentum" in opt.param_groups[0]
        rec = self.at(epoch, i, warmup_bias_lr=None if has_momentum else 0.0)
        for j, grp in enumerate(opt.param_groups):
            grp["lr"] = rec.lrs[j]
            if "momentum" in grp:
                grp["momentum"] = rec.momentum
        opt.param_groups[1]["weight_decay"] = self.weight_decay  # (:306: the decayed group is built with the scaled value)
        return self.advance(rec)


def train_epoch(step, batches, schedule, epoch):
    """the batch loop of the reference's epoch (trainer.py:367-399): schedule -> TrainStep(batch, update=...) -> running mean of the loss items
    (:389-391), kept on the device: nothing is read back per iteration.  -> tloss (None for no batches).  Gradients pending when the epoch
    ends stay pending, as in the reference."""
    tloss = None
    for i, batch in enumerate(batches):
        rec = schedule.apply(step.opt, epoch, i)
        items = step(batch, update=rec.update)
        tloss = (tloss * i + items) / (i + 1) if tloss is not None else items.detach().clone()
    return tloss
