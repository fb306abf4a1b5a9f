"""v8 detection loss (reference: ultralytics/utils/loss.py:152-255 v8DetectionLoss, utils/tal.py:14-327
TaskAlignedAssigner, utils/metrics.py:74-134 CIoU).

The mathematics lives in csrc/loss.hip: DFL decode, task-aligned assignment, CIoU / DFL / BCE sums and their
gradients run as ten small HIP launches on the NHWC maps the Detect convolutions write (no [B, 8400, .] copies,
no boolean indexing, every shape static given the maximum number of boxes per image, so the whole step can be
captured in a HIP graph).  This module only mirrors the reference's criterion interface.
"""
from types import SimpleNamespace

import torch

from .. import ops

DEFAULT_HYP = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5)  # reference cfg/default.yaml:98-100


class SplitPreds:
    """train-mode Detect output before the channel concat: box[i] [B, 64, H, W], cls[i] [B, nc, H, W]."""

    def __init__(self, box, cls):
        self.box, self.cls = box, cls


def _nhwc_map(t, box):
    """the tensor itself when the kernels can read it: NHWC memory (a channel slice of a wider, padded buffer is fine: the kernels
    take a pixel stride), 16-byte-aligned rows for box maps; else a dense NHWC copy (differentiable)."""
    if ops.is_nhwc(t) and (not box or (t.data_ptr() % 16 == 0 and (ops.as_ymi(t).ld * t.element_size()) % 16 == 0)):
        return t
    return t.contiguous(memory_format=torch.channels_last)


class v8DetectionLoss:
    """criterion(preds, batch) -> (loss * batch_size [3], loss.detach() [3]) as reference loss.py:201-255."""

    def __init__(self, model, tal_topk=10):
        det = model.model[-1]
        self.hyp = getattr(model, "args", None) or DEFAULT_HYP
        self.stride = det.stride
        self.nc = det.nc
        self.reg_max = det.reg_max
        self.no = det.nc + det.reg_max * 4
        self.device = next(model.parameters()).device
        self.topk, self.alpha, self.beta = tal_topk, 0.5, 6.0  # reference loss.py:169
        self.gains = torch.tensor([self.hyp.box, self.hyp.cls, self.hyp.dfl], dtype=torch.float, device=self.device)
        self.stride_list = [float(v) for v in det.stride]  # host copy: no device->host reads on the step path
        self._scales = {}  # batch size -> device [6] = (gains * B, gains)

    def max_boxes(self, batch_idx, batch_size):
        """largest number of labels in one image (one device->host read; pass batch["max_boxes"] to avoid it)."""
        if batch_idx.numel() == 0:
            return 0
        return int(torch.bincount(batch_idx.reshape(-1).long(), minlength=batch_size).max())

    name = "v8DetectionLoss"  # in the refusal of CPU tensors

    def __call__(self, preds, batch):
        """the criterion's one body; a subclass overrides the steps that differ: _split (how preds gives box maps, class maps and its
        extras), _targets (the dense target rows, and what is asked of the labels) and _finish (the loss op)."""
        box, cls, extras = self._split(preds)
        if not box[0].is_cuda:
            raise RuntimeError(f"{self.name} runs in libyolo_mi355 kernels: predictions must be on the MI355X (cuda) device; there is no CPU path")
        box = [_nhwc_map(t, True) for t in box]
        cls = [_nhwc_map(t if t.dtype == box[0].dtype else t.to(box[0].dtype), False) for t in cls]
        B = box[0].shape[0]
        targets = self._targets(batch, box, extras)
        # both results leave the last loss kernel: loss * gains * B (differentiable) and loss * gains (reference loss.py:250-255)
        scale = self._scales.get(B)
        if scale is None:
            gh = [float(self.hyp.box), float(self.hyp.cls), float(self.hyp.dfl)]
            scale = self._scales[B] = torch.tensor([g * B for g in gh] + gh, dtype=torch.float32, device=box[0].device)
        return self._finish(box, cls, targets, scale, extras, batch)

    def _split_feats(self, feats):
        """[B, no, H, W] maps (reference layout): split the channels again (loss.py:205-207)."""
        return [f[:, : self.reg_max * 4] for f in feats], [f[:, self.reg_max * 4 :] for f in feats]

    def _split(self, preds):
        """-> (box maps, class maps, extras): SplitPreds, or the per-level [B, no, H, W] maps of a Detect output (the train-mode list, or the
        second entry of the eval-mode tuple)."""
        if hasattr(preds, "box") and hasattr(preds, "cls"):
            return list(preds.box), list(preds.cls), None
        return (*self._split_feats(preds[1] if isinstance(preds, tuple) else preds), None)

    targets_op = "detect_targets"  # the ops function that makes the dense target rows

    def _targets(self, batch, box, extras):
        """the dense target rows of the batch, by ops.<targets_op>, for the image the first level's map and stride span."""
        B = box[0].shape[0]
        h, w = box[0].shape[2:]
        s0 = self.stride_list[0]
        g = batch.get("max_boxes")
        if g is None:
            g = self.max_boxes(batch["batch_idx"], B)
        g = max(int(g), 1)  # an all-background batch still needs one (empty) slot per image
        return getattr(ops, self.targets_op)(batch["batch_idx"], batch["cls"], batch["bboxes"], B, g, w * s0, h * s0, box[0].device)

    def _finish(self, box, cls, targets, scale, extras, batch):
        return ops.detect_loss(box, cls, self.stride_list, targets, scale, self.topk, self.alpha, self.beta)


class v8SegmentationLoss(v8DetectionLoss):
    """criterion(preds, batch) -> (loss * batch_size [4], loss.detach() [4]) in the order box, seg, cls, dfl (reference loss.py:258-438).

    preds: the Segment head's SegPreds (training fast path), its train-mode output (feats, mc [B, nm, A], p) or its eval output (y, (feats,
    mc, p)).  batch["masks"]: the overlap encoding [B, Hm, Wm], uint8 or float32 (pixel value = 1 + index of the object among the image's
    labels, 0 = background), read at the prototype map's size with F.interpolate(mode="nearest")'s index rule inside the kernel.
    The detection stages run once (ops.detect_loss_assign: box, cls and dfl are v8DetectionLoss's numbers bit for bit) and hand the
    assignment to the mask stage (ops.mask_loss, csrc/seg.hip); every shape is static given max_boxes and nothing is read back."""

    def __init__(self, model, tal_topk=10):
        super().__init__(model, tal_topk)
        self.overlap = bool(getattr(self.hyp, "overlap_mask", True))
        if not self.overlap:
            raise NotImplementedError("overlap_mask=False (one mask per label, reference loss.py:427-428) is not built: the mask-loss kernel reads "
                                      "the overlap encoding [B, H, W]")
        self.nm = model.model[-1].nm

    def _split(self, preds):
        """SegPreds, the train-mode output (feats, mc [B, nm, A], p) or the eval output (y, (feats, mc, p)) -> extras (mc maps, proto)."""
        from ..nn.modules.head import SegPreds

        if isinstance(preds, SegPreds):
            return list(preds.box), list(preds.cls), (list(preds.mc), preds.proto)
        feats, mcat, proto = preds if len(preds) == 3 else preds[1]
        B = mcat.shape[0]
        sizes = [int(f.shape[2] * f.shape[3]) for f in feats]
        mc = [m.reshape(B, self.nm, f.shape[2], f.shape[3]) for m, f in zip(mcat.split(sizes, 2), feats)]
        return (*self._split_feats(feats), (mc, proto))

    def _finish(self, box, cls, targets, scale, extras, batch):
        mc, proto = extras
        dt = box[0].dtype
        mc = [_nhwc_map(t if t.dtype == dt else t.to(dt), True) for t in mc]
        proto = _nhwc_map(ops.to_internal(proto, dt), True)
        masks = batch["masks"]
        if masks.dim() != 3 or masks.shape[0] != proto.shape[0]:
            raise ValueError(f"batch['masks'] must be the overlap encoding [B, H, W], got {tuple(masks.shape)}")
        if masks.dtype not in (torch.uint8, torch.float32):
            masks = masks.float()
        masks = masks.to(proto.device).contiguous()
        h, w = box[0].shape[2:]
        s0 = self.stride_list[0]
        loss3, items3, gidx = ops.detect_loss_assign(box, cls, self.stride_list, targets, scale, self.topk, self.alpha, self.beta)
        return ops.mask_loss(loss3, items3, gidx, targets, masks, scale, self.topk, w * s0, h * s0, proto, mc)


class v8OBBLoss(v8DetectionLoss):
    """criterion(preds, batch) -> (loss * batch_size [3], loss.detach() [3]) as box, cls, dfl (reference loss.py:607-720).

    preds: the OBB head's OBBPreds (training fast path), its train-mode output (feats, angle [B, 1, A]) or its eval output (y, (feats, angle)).
    batch["bboxes"]: [n, 5] xywhr rows, xywh normalised, the angle in radians.  The stages run in csrc/loss.hip (ops.obb_loss): the rotated
    decode, inside test, probiou metric and box term, with the detection loss's top-k, claim and final-sum kernels between them; every shape is
    static given max_boxes and nothing is read back."""

    name = "v8OBBLoss"
    targets_op = "obb_targets"

    def _split(self, preds):
        if hasattr(preds, "angle"):  # OBBPreds
            return list(preds.box), list(preds.cls), preds.angle
        # (feats, angle), or the eval tuple (y, (feats, angle)): split the channels again (loss.py:636-640)
        feats, angle = preds if isinstance(preds[0], (list, tuple)) else preds[1]
        return (*self._split_feats(feats), angle)

    def _targets(self, batch, box, angle):
        B = box[0].shape[0]
        A = sum(int(t.shape[2] * t.shape[3]) for t in box)
        if tuple(angle.shape) != (B, 1, A):
            raise ValueError(f"v8OBBLoss: the angle is [B, 1, A] = {(B, 1, A)}, got {tuple(angle.shape)}")
        bboxes = batch["bboxes"]
        if bboxes.numel() and (bboxes.dim() != 2 or bboxes.shape[1] != 5):
            raise TypeError(f"v8OBBLoss: batch['bboxes'] holds xywhr rows [n, 5], got {tuple(bboxes.shape)}: is this an oriented-box dataset?")
        return super()._targets(batch, box, angle)

    def _finish(self, box, cls, targets, scale, angle, batch):
        if angle.dtype != torch.float32 or not angle.is_contiguous():
            angle = angle.float().contiguous()
        return ops.obb_loss(box, cls, angle, self.stride_list, targets, scale, self.topk, self.alpha, self.beta)
