"""Minimal Boxes, Masks and Results with the reference's names and arithmetic (ultralytics/engine/results.py:187-280, :1041-1256, :1259-1330).
Tensors stay on the device they arrive on; there is no plotting, saving, mask contours (Masks.xy / xyn), keypoints or tracking."""
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


class Masks:
    """data [n, H, W] uint8 0 / 1 masks at the letterboxed network input's shape, one per box and in the boxes' order; orig_shape (h, w) of
    the image (reference engine/results.py:1259).  The reference holds float 0 / 1; contour tracing (xy, xyn) is not built."""

    def __init__(self, masks, orig_shape):
        if masks.ndim == 2:
            masks = masks[None, :]
        assert masks.ndim == 3, f"expected [n, H, W] masks but got {tuple(masks.shape)}"
        self.data = masks
        self.orig_shape = orig_shape

    @property
    def shape(self):
        return self.data.shape

    @property
    def xy(self):
        raise NotImplementedError("Masks.xy: contour tracing (the reference's cv2.findContours step) is not built")

    @property
    def xyn(self):
        raise NotImplementedError("Masks.xyn: contour tracing (the reference's cv2.findContours step) is not built")

    def cpu(self):
        return Masks(self.data.cpu(), self.orig_shape)

    def __len__(self):
        return len(self.data)

    def __repr__(self):
        return f"Masks(n={len(self)}, shape={tuple(self.data.shape[1:])}, orig_shape={tuple(self.orig_shape)})"


class Results:
    """one image's detections: orig_shape (h, w), boxes (Boxes), names ({class id: name}), path, masks (Masks or None)."""

    def __init__(self, orig_shape, path=None, names=None, boxes=None, masks=None):
        self.orig_shape = tuple(int(v) for v in orig_shape[:2])
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None and not isinstance(boxes, Boxes) else boxes
        self.masks = Masks(masks, self.orig_shape) if masks is not None and not isinstance(masks, Masks) else masks
        self.names = names
        self.path = path

    def cpu(self):
        return Results(self.orig_shape, self.path, self.names, self.boxes.cpu() if self.boxes is not None else None,
                       self.masks.cpu() if self.masks is not None else None)

    def __len__(self):
        return len(self.boxes) if self.boxes is not None else 0

    def __repr__(self):
        tail = f", masks={len(self.masks)}" if self.masks is not None else ""
        return f"Results(path={self.path!r}, orig_shape={self.orig_shape}, boxes={len(self)}{tail})"
