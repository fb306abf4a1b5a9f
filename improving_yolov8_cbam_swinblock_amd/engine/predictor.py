"""Prediction on real images: reference engine/predictor.py:144-191 (preprocess, pre_transform) with models/yolo/detect/predict.py:33-102
(postprocess, construct_result).

Per chunk of `batch` images: ops.letterbox (one upload, one launch per 32 images), the eval forward under autocast, ops.detect_nms with the
predictor's arguments (no multi_label), ops.scale_boxes on the device with gain and pad derived from the shapes as construct_result's
scale_boxes call derives them, then ONE trip of the counts to the host to slice the rows.  Boxes stay on the device."""
import numpy as np
import torch

from .. import ops
from .results import Results


class DetectionPredictor:
    """DetectionPredictor(model)(images) -> [Results].  images: a list of (h, w, 3) uint8 BGR images (numpy or torch, host or device) of any
    sizes, or one such image; or a float [B, 3, H, W] tensor, which passes through unletterboxed and unnormalised as in the reference.
    The model's train / eval mode is restored."""

    _segment = False  # SegmentationPredictor: the model's head carries mask coefficients

    def __init__(self, model, imgsz=640, conf=0.25, iou=0.7, classes=None, agnostic_nms=False, max_det=300, batch=32, dtype=torch.bfloat16,
                 augment=False, rect=False):
        layers = getattr(model, "model", None)
        if layers is not None and getattr(layers[-1], "ne", 0):
            raise NotImplementedError("a predictor on an OBBModel needs rotated NMS (batch_probiou), boxes with their angle in image coordinates and an OBB "
                                      "results class: not built yet; the head's eval output [B, 4 + nc + 1, A] is model(img)[0]")
        if bool(layers is not None and getattr(layers[-1], "nm", 0)) != self._segment:
            if self._segment:
                raise ValueError("SegmentationPredictor takes a model whose head is a Segment; a detector goes to DetectionPredictor")
            raise NotImplementedError("DetectionPredictor on a SegmentationModel: its NMS rows carry mask coefficients; use engine.predictor.SegmentationPredictor")
        self.model = model
        self.imgsz = (int(imgsz), int(imgsz)) if isinstance(imgsz, int) else (int(imgsz[0]), int(imgsz[1]))
        self.conf, self.iou, self.classes, self.agnostic_nms, self.max_det = conf, iou, classes, agnostic_nms, max_det
        self.batch = int(batch)
        self.dtype = dtype
        self.augment = bool(augment)
        self.rect = bool(rect)
        self.stride = int(max(float(s) for s in getattr(model, "stride", [32])))
        self.names = getattr(model, "names", None)
        self.device = next(model.parameters()).device

    def preprocess(self, im):
        """-> (img [n, 3, H, W] float32 on the device, [(h0, w0)]); reference predictor.py:144-191."""
        if torch.is_tensor(im) and im.dim() == 4:
            if not im.is_floating_point():
                raise ValueError("DetectionPredictor: a [B, 3, H, W] tensor is taken as a prepared float batch; pass uint8 images as a list of (h, w, 3)")
            return im.to(self.device).float(), [tuple(im.shape[2:])] * im.shape[0]
        same_shapes = len({tuple(x.shape) for x in im}) == 1
        img, _ = ops.letterbox(im, self.imgsz, auto=same_shapes and self.rect, stride=self.stride, device=self.device)
        return img, [tuple(int(v) for v in x.shape[:2]) for x in im]

    def inference(self, img):
        kw = {"augment": True} if self.augment else {}
        if self.dtype == torch.float32:
            return self.model(img, **kw)
        with torch.autocast("cuda", dtype=self.dtype):
            return self.model(img, **kw)

    def postprocess(self, preds, img, ori_shapes):
        """-> (det [n, max_det, 6] in each image's own pixels, count [n]), both on the device; reference predict.py:54-64 and :101."""
        y = preds[0] if isinstance(preds, (list, tuple)) else preds
        det, count = ops.detect_nms(y, self.conf, self.iou, agnostic=self.agnostic_nms, classes=self.classes, max_det=self.max_det)
        return ops.scale_boxes(det, count, tuple(img.shape[2:]), ori_shapes, inplace=True), count

    def __call__(self, images, paths=None):
        if isinstance(images, np.ndarray) or (torch.is_tensor(images) and images.dim() == 3):
            images = [images]
        n = len(images)
        paths = [None] * n if paths is None else list(paths)
        was_training = self.model.training
        self.model.eval()
        results = []
        try:
            for i in range(0, n, self.batch):
                with torch.no_grad():
                    img, ori_shapes = self.preprocess(images[i : i + self.batch])
                    det, count = self.postprocess(self.inference(img), img, ori_shapes)
                for k, c in enumerate(count.tolist()):  # the chunk's one trip to the host
                    results.append(Results(ori_shapes[k], path=paths[i + k], names=self.names, boxes=det[k, :c]))
        finally:
            self.model.train(was_training)
        return results


class SegmentationPredictor(DetectionPredictor):
    """SegmentationPredictor(model)(images) -> [Results] with `boxes` and `masks` (reference models/yolo/segment/predict.py).  Per chunk: the
    eval forward, ops.detect_nms_seg, the chunk's one trip of the counts to the host, ops.process_mask(upsample=True) on the packed kept rows
    at the letterboxed input shape, then ops.scale_boxes (construct_result's order: the masks are cut with the boxes still in input pixels),
    and rows whose mask is empty are dropped (predict.py:110-112).  The area filter costs ONE further host trip per chunk (the areas [rows]
    int32); the masks themselves stay on the device.  masks.data is [n, H, W] uint8 at the letterboxed input shape; a result in which nothing
    is kept has masks None.  Not built, refused here: retina_masks (process_mask_native) and test-time augmentation."""

    _segment = True

    def __init__(self, model, imgsz=640, conf=0.25, iou=0.7, classes=None, agnostic_nms=False, max_det=300, batch=32, dtype=torch.bfloat16,
                 augment=False, rect=False, retina_masks=False):
        if augment:
            raise NotImplementedError("SegmentationPredictor: test-time augmentation merges box rows only; it is not built for mask coefficients")
        if retina_masks:
            raise NotImplementedError("SegmentationPredictor: retina_masks (process_mask_native, masks at the original image's size) is not built")
        super().__init__(model, imgsz=imgsz, conf=conf, iou=iou, classes=classes, agnostic_nms=agnostic_nms, max_det=max_det, batch=batch, dtype=dtype,
                         rect=rect)
        self.nc = int(model.model[-1].nc)

    def postprocess(self, preds, img, ori_shapes):
        """-> (det [n, max_det, 6] still in the input's pixels, coef [n, max_det, nm], count [n], proto [n, nm, mh, mw]), all on the device."""
        y, tail = preds[0], preds[1]
        proto = tail[-1] if isinstance(tail, (list, tuple)) else tail
        det, coef, count = ops.detect_nms_seg(y, self.nc, self.conf, self.iou, agnostic=self.agnostic_nms, classes=self.classes, max_det=self.max_det)
        return det, coef, count, proto

    def __call__(self, images, paths=None):
        if isinstance(images, np.ndarray) or (torch.is_tensor(images) and images.dim() == 3):
            images = [images]
        n = len(images)
        paths = [None] * n if paths is None else list(paths)
        was_training = self.model.training
        self.model.eval()
        results = []
        try:
            for i in range(0, n, self.batch):
                with torch.no_grad():
                    img, ori_shapes = self.preprocess(images[i : i + self.batch])
                    det, coef, count, proto = self.postprocess(self.inference(img), img, ori_shapes)
                    counts = count.tolist()  # the chunk's one trip to the host
                    max_det = det.shape[1]
                    rows = torch.tensor([k * max_det + j for k, c in enumerate(counts) for j in range(c)], dtype=torch.long).to(det.device)
                    row_img = torch.tensor([k for k, c in enumerate(counts) for _ in range(c)], dtype=torch.int32).to(det.device)
                    masks, area = ops.process_mask(proto, det.view(-1, 6)[rows, :4], coef.view(-1, coef.shape[2])[rows], row_img, tuple(img.shape[2:]),
                                                   upsample=True)
                    det = ops.scale_boxes(det, count, tuple(img.shape[2:]), ori_shapes, inplace=True)
                    keep = (area > 0).cpu()  # the area filter's trip
                first = 0
                for k, c in enumerate(counts):
                    sel = torch.nonzero(keep[first : first + c]).reshape(-1).to(det.device)
                    results.append(Results(ori_shapes[k], path=paths[i + k], names=self.names, boxes=det[k, :c][sel],
                                           masks=masks[first : first + c][sel] if len(sel) else None))
                    first += c
        finally:
            self.model.train(was_training)
        return results
