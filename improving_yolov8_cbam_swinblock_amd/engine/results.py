"""Minimal Boxes and Results with the reference's names and arithmetic (ultralytics/engine/results.py:187-280, :1041-1256).  Tensors stay on the
device they arrive on; there is no plotting, saving, masks, keypoints or tracking."""
import torch

from ..utils.ops import xyxy2xywh


class Boxes:
    """data [n, 6] rows (x1, y1, x2, y2, conf, cls) in the pixels of the original image; orig_shape (h, w)."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        n = boxes.shape[-1]
        assert n == 6, f"expected 6 values but got {n}"  # xyxy, conf, cls
        self.data = boxes
        self.orig_shape = orig_shape

    @property
    def shape(self):
        return self.data.shape

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def xywh(self):
        return xyxy2xywh(self.xyxy)

    def _wh(self):
        """(w, h, w, h) as a tensor beside the data: x /= w by a tensor is the IEEE quotient on the host and on the device alike, where a
        division by a Python scalar becomes a product with its reciprocal on the device (one ulp off the reference's host result)"""
        h, w = self.orig_shape[:2]
        return torch.tensor([w, h, w, h], dtype=self.data.dtype, device=self.data.device)

    @property
    def xyxyn(self):
        return self.xyxy / self._wh()  # xyxy[..., [0, 2]] /= orig_shape[1]; xyxy[..., [1, 3]] /= orig_shape[0]

    @property
    def xywhn(self):
        return xyxy2xywh(self.xyxy) / self._wh()

    def cpu(self):
        return Boxes(self.data.cpu(), self.orig_shape)

    def __len__(self):
        return len(self.data)

    def __repr__(self):
        return f"Boxes(n={len(self)}, orig_shape={tuple(self.orig_shape)})"


class Results:
    """one image's detections: orig_shape (h, w), boxes (Boxes), names ({class id: name}), path."""

    def __init__(self, orig_shape, path=None, names=None, boxes=None):
        self.orig_shape = tuple(int(v) for v in orig_shape[:2])
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None and not isinstance(boxes, Boxes) else boxes
        self.names = names
        self.path = path

    def cpu(self):
        return Results(self.orig_shape, self.path, self.names, self.boxes.cpu() if self.boxes is not None else None)

    def __len__(self):
        return len(self.boxes) if self.boxes is not None else 0

    def __repr__(self):
        return f"Results(path={self.path!r}, orig_shape={self.orig_shape}, boxes={len(self)})"
