"""Validation of a detector: reference engine/validator.py:125-254 with models/yolo/detect/val.py:113-133,174-216,240-253,275-290.

Per batch: the eval forward under autocast, ops.detect_nms on the device (multi_label, as val.py:123-133), one trip of (det, count)
to the host, then per image the matching of at most max_det detections to the labels and the statistics lists - host code on a few
hundred numbers.  There is no dataloader: batches arrive as engine.trainer.synthetic_batch makes them (img, batch_idx, cls, bboxes as
normalised xywh).  A batch that also carries `ori_shape` and `ratio_pad` per image, as a letterboxing dataset attaches them, is matched
in native space (val.py:135-172): the predictions go through ops.scale_boxes on the device before the one trip to the host, the labels
through the same arithmetic on the host."""
import numpy as np
import torch

from .. import ops
from ..utils.metrics import DetMetrics, box_iou, match_predictions
from ..utils.ops import scale_boxes, xywh2xyxy


class DetectionValidator:
    """DetectionValidator(model)(batches) -> results_dict (metrics/precision(B), metrics/recall(B), metrics/mAP50(B), metrics/mAP50-95(B),
    fitness).  `model` may be the trained model or TrainStep's `step.ema.ema`; its train / eval mode is restored."""

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, single_cls=False, agnostic_nms=False, dtype=torch.bfloat16, augment=False):
        self.model = model
        self.augment = bool(augment)  # test-time augmentation: the forward is model.predict(img, augment=True) (reference engine/validator.py:214)
        self.conf, self.iou, self.max_det = conf, iou, max_det
        self.single_cls, self.agnostic_nms = single_cls, agnostic_nms
        self.dtype = dtype
        self.iouv = torch.linspace(0.5, 0.95, 10)
        self.nc = int(model.model[-1].nc)
        self.init_metrics()

    def init_metrics(self):
        self.metrics = DetMetrics(names={i: str(i) for i in range(self.nc)})
        self.seen = 0
        self.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
        self.detections = []  # per image [n, 6] as matched (single_cls: class column 0), kept for callers that want the boxes

    def postprocess(self, preds):
        """-> (det [B, max_det, 6], count [B]) on the device; reference val.py:113-133."""
        y = preds[0] if isinstance(preds, (list, tuple)) else preds
        return ops.detect_nms(y, self.conf, self.iou, multi_label=True, agnostic=self.single_cls or self.agnostic_nms, max_det=self.max_det)

    def update_metrics(self, det, count, batch):
        """det / count on the host; reference val.py:174-216 and :135-155 (labels to pixels of the network input)."""
        h, w = batch["img"].shape[2:]
        bidx = batch["batch_idx"].detach().cpu().reshape(-1)
        cls_all = batch["cls"].detach().cpu().float().reshape(-1)
        box_all = batch["bboxes"].detach().cpu().float().reshape(-1, 4)
        scale = torch.tensor([w, h, w, h], dtype=torch.float32)
        native = "ori_shape" in batch and "ratio_pad" in batch
        for si in range(det.shape[0]):
            self.seen += 1
            pred = det[si, : int(count[si])].clone()
            sel = bidx == si
            cls, bbox = cls_all[sel], box_all[sel]
            if len(cls):
                bbox = xywh2xyxy(bbox) * scale
                if native:  # native-space labels (val.py:154); the predictions were brought there on the device
                    scale_boxes((h, w), bbox, batch["ori_shape"][si], ratio_pad=batch["ratio_pad"][si])
            if self.single_cls:  # one class on both sides: the reference zeroes the predictions here and the labels in its dataset (which this package has not)
                pred[:, 5] = 0
                cls = torch.zeros_like(cls)
            self.detections.append(pred)
            if not len(pred):
                if len(cls):
                    self._append(torch.zeros(0, len(self.iouv), dtype=torch.bool), pred[:, 4], pred[:, 5], cls)
                continue
            tp = torch.zeros(len(pred), len(self.iouv), dtype=torch.bool)
            if len(cls):
                tp = match_predictions(pred[:, 5], cls, box_iou(bbox, pred[:, :4]), self.iouv)
            self._append(tp, pred[:, 4], pred[:, 5], cls)

    def _append(self, tp, conf, pred_cls, target_cls):
        for k, v in zip(("tp", "conf", "pred_cls", "target_cls"), (tp, conf, pred_cls, target_cls)):
            self.stats[k].append(v)

    def get_stats(self):
        """reference val.py:240-253; with nothing accumulated (no labels and no detections anywhere) every metric is zero."""
        if self.stats["tp"]:
            self.metrics.process(**{k: torch.cat(v, 0).numpy() for k, v in self.stats.items()})
        return self.metrics.results_dict

    def __call__(self, batches):
        if isinstance(batches, dict):
            batches = [batches]
        was_training = self.model.training
        self.init_metrics()
        self.model.eval()
        try:
            for batch in batches:
                with torch.no_grad():
                    kw = {"augment": True} if self.augment else {}  # (only then: any module that maps an image batch to predictions can be validated)
                    if self.dtype == torch.float32:
                        preds = self.model(batch["img"], **kw)
                    else:
                        with torch.autocast("cuda", dtype=self.dtype):
                            preds = self.model(batch["img"], **kw)
                    det, count = self.postprocess(preds)
                    if "ori_shape" in batch and "ratio_pad" in batch:  # native-space predictions (val.py:157-172)
                        det = ops.scale_boxes(det, count, tuple(batch["img"].shape[2:]), batch["ori_shape"], batch["ratio_pad"], inplace=True)
                self.update_metrics(det.cpu(), count.cpu(), batch)
        finally:
            self.model.train(was_training)
        return self.get_stats()
