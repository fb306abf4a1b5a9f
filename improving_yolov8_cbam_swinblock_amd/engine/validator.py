"""Validation of a detector: reference engine/validator.py:125-254 with models/yolo/detect/val.py:113-133,174-216,240-253,275-290.

Per batch: the eval forward under autocast, ops.detect_nms on the device (multi_label, as val.py:123-133), ops.scale_boxes when the batch
carries `ori_shape` and `ratio_pad` per image, as a letterboxing dataset attaches them (native-space matching, val.py:135-172), then the
matching of at most max_det detections per image to the labels.  There is no dataloader: batches arrive as engine.trainer.synthetic_batch
makes them (img, batch_idx, cls, bboxes as normalised xywh).

match="device": the matching, the tp matrices and the confusion matrix are ONE launch per batch (ops.val_match); det, count and
tp stay on the device, the batch loop copies nothing to the host and never synchronises, and one vectorised host step after the last batch
builds `stats`, `detections`, `seen`, the matrix and the label counts.  Results are flushed to the host every FLUSH_EVERY batches.
match="host" (the default): one trip of (det, count) to the host per batch, then per image box_iou, utils.metrics.match_predictions and
ConfusionMatrix.process_batch in host code.  It stays the default because callers and tests/test_gpu_predict.py observe the label boxes
through this module's box_iou, which the device path never calls.  Both paths give the same tp matrices and the same confusion matrix, bit for bit
(tests/test_gpu_valmatch.py); tools/probes/val_match_probe.py times the two ("Validation statistics on the device")."""
import numpy as np
import torch

from .. import ops
from ..utils.metrics import ConfusionMatrix, DetMetrics, SegmentMetrics, box_iou, mask_iou, match_predictions
from ..utils.ops import process_mask, scale_boxes, xywh2xyxy

# Device path: batches whose results are held on the device before one trip takes them to the host.  A batch holds det, count and tp:
# max_det * (24 + 10) + 4 bytes per image, 0.33 MB at batch 32 / max_det 300, so 64 batches are 21 MB at most; a COCO-sized validation
# (5000 images, 157 batches of 32) makes three trips instead of 157.
FLUSH_EVERY = 64


class DetectionValidator:
    """DetectionValidator(model)(batches) -> results_dict (metrics/precision(B), metrics/recall(B), metrics/mAP50(B), metrics/mAP50-95(B),
    fitness; with loss=True also val/box_loss, val/cls_loss, val/dfl_loss: the mean over the batches of model.loss(batch, preds)[1],
    reference engine/validator.py:219,235).  `model` may be the trained model or TrainStep's `step.ema.ema`; its train / eval mode is
    restored.  After a call: `stats`, `detections` (per image [n, 6] host tensors as matched), `seen`, `confusion_matrix`
    (utils.metrics.ConfusionMatrix), `nt_per_class` and `nt_per_image` (labels / images with a label per class, reference val.py:248-249)."""

    _segment = False   # SegmentationValidator: the model's head carries mask coefficients
    _extra_keys = ()   # statistics held per detection beside tp (SegmentationValidator: tp_m)
    loss_names = ("val/box_loss", "val/cls_loss", "val/dfl_loss")

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, single_cls=False, agnostic_nms=False, dtype=torch.bfloat16, augment=False, match="host",
                 loss=False):
        if match not in ("device", "host"):
            raise ValueError(f"match is 'device' or 'host', got {match!r}")
        if getattr(model.model[-1], "ne", 0):
            raise NotImplementedError("a validator on an OBBModel needs rotated NMS and batch_probiou matching of xywhr labels: not built yet; "
                                      "model.loss(batch) gives the validation loss")
        if bool(getattr(model.model[-1], "nm", 0)) != self._segment:
            if self._segment:
                raise ValueError("SegmentationValidator takes a model whose head is a Segment; a detector goes to DetectionValidator")
            raise NotImplementedError("DetectionValidator on a SegmentationModel: its NMS rows carry mask coefficients; use engine.validator.SegmentationValidator")
        self.model = model
        self.augment = bool(augment)  # test-time augmentation: the forward is model.predict(img, augment=True) (reference engine/validator.py:214)
        self.conf, self.iou, self.max_det = conf, iou, max_det
        self.single_cls, self.agnostic_nms = single_cls, agnostic_nms
        self.dtype = dtype
        self.match, self.with_loss = match, bool(loss)
        self.iouv = torch.linspace(0.5, 0.95, 10)
        self.nc = int(model.model[-1].nc)
        self.init_metrics()

    def init_metrics(self):
        self.metrics = DetMetrics(names={i: str(i) for i in range(self.nc)})
        self.seen = 0
        self.stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
        self.detections = []  # per image [n, 6] as matched (single_cls: class column 0), kept for callers that want the boxes
        self.confusion_matrix = ConfusionMatrix(self.nc, conf=self.conf)
        self.nt_per_class = np.zeros(self.nc, dtype=np.int64)
        self.nt_per_image = np.zeros(self.nc, dtype=np.int64)
        self.loss = None            # loss=True: the device sum of the batches' loss items
        self._target_img = []       # per image (host path) or per flush (device path): the distinct classes labelled in an image
        self._held, self._cm_dev = [], None
        self._levels = [float(v) for v in self.iouv.tolist()]

    def postprocess(self, preds):
        """-> (det [B, max_det, 6], count [B]) on the device; reference val.py:113-133."""
        y = preds[0] if isinstance(preds, (list, tuple)) else preds
        return ops.detect_nms(y, self.conf, self.iou, multi_label=True, agnostic=self.single_cls or self.agnostic_nms, max_det=self.max_det)

    def batch_results(self, preds, batch):
        """-> (det, count) on the device as the matching takes them: NMS, then native-space boxes when the batch carries the shapes."""
        det, count = self.postprocess(preds)
        if "ori_shape" in batch and "ratio_pad" in batch:  # native-space predictions (val.py:157-172)
            det = ops.scale_boxes(det, count, tuple(batch["img"].shape[2:]), batch["ori_shape"], batch["ratio_pad"], inplace=True)
        return det, count

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
            self._target_img.append(cls.unique())
            self.confusion_matrix.process_batch(pred, bbox, cls)
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

    def update_metrics_device(self, det, count, batch, *extra):
        """det / count on the device: one launch, nothing crosses to the host.  The batch's results are held until the next flush.
        extra: [B, max_det, ...] device tensors held beside tp, one per name of _extra_keys."""
        if self._cm_dev is None:
            self._cm_dev = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int32, device=det.device)
        native = "ori_shape" in batch and "ratio_pad" in batch
        tp = ops.val_match(det, count, batch["batch_idx"], batch["cls"], batch["bboxes"], tuple(batch["img"].shape[2:]), self._levels,
                           ori_shapes=batch["ori_shape"] if native else None, ratio_pads=batch["ratio_pad"] if native else None,
                           single_cls=self.single_cls, cm=self._cm_dev, cm_conf=self.confusion_matrix.conf, cm_iou=self.confusion_matrix.iou_thres)
        self._held.append((det, count, tp, batch["batch_idx"].detach().reshape(-1), batch["cls"].detach().reshape(-1)) + tuple(extra))
        if len(self._held) >= FLUSH_EVERY:
            self._flush()

    def _flush(self):
        """the held batches -> host, five copies whatever their number, then the statistics of their images in one vectorised step."""
        if not self._held:
            return
        dets, counts, tps, bidx, cls, *extras = zip(*self._held)
        self._held = []
        sizes = [int(d.shape[0]) for d in dets]                      # images per batch (shapes: host numbers)
        first = np.concatenate(([0], np.cumsum(sizes)))[:-1]         # index of a batch's first image within this flush
        n_lab = [int(b.numel()) for b in bidx]
        det = torch.cat(dets, 0).cpu()
        count = torch.cat(counts, 0).cpu().long()
        tp = torch.cat(tps, 0).cpu()
        lab_img = torch.cat([b.float() for b in bidx], 0).cpu().long()
        lab_cls = torch.cat([c.float() for c in cls], 0).cpu()
        in_batch = (lab_img >= 0) & (lab_img < torch.from_numpy(np.repeat(sizes, n_lab)))   # rows of image indices no image has belong to nobody
        lab_img = lab_img + torch.from_numpy(np.repeat(first, n_lab))
        lab_img, lab_cls = lab_img[in_batch], lab_cls[in_batch]
        if self.single_cls:
            det[:, :, 5] = 0
            lab_cls = torch.zeros_like(lab_cls)
        live = torch.arange(det.shape[1])[None, :] < count[:, None]  # [images, max_det]
        rows = det[live]                                             # image by image, ranked order inside an image
        self.seen += int(det.shape[0])
        self.detections.extend(rows.split(count.tolist()))
        order = torch.sort(lab_img, stable=True)[1]                  # image by image, table order inside an image
        self._append(tp[live].bool(), rows[:, 4], rows[:, 5], lab_cls[order])
        for key, parts in zip(self._extra_keys, extras):
            self.stats[key].append(torch.cat(parts, 0).cpu()[live].bool())
        pairs = torch.unique(torch.stack((lab_img, lab_cls.long()), 1), dim=0) if len(lab_img) else torch.zeros(0, 2, dtype=torch.long)
        self._target_img.append(pairs[:, 1].float())

    def get_stats(self):
        """reference val.py:240-253; with nothing accumulated (no labels and no detections anywhere) every metric is zero."""
        if self.stats["tp"]:
            self.metrics.process(**{k: torch.cat(v, 0).numpy() for k, v in self.stats.items()})
        out = self.metrics.results_dict
        if self.with_loss and self.loss is not None:
            out.update(zip(self.loss_names, self._loss_mean))
        return out

    def _finish(self, n_batches):
        if self.match == "device":
            self._flush()
            if self._cm_dev is not None:
                self.confusion_matrix.matrix = self._cm_dev.cpu().numpy().astype(np.int64)
        count = lambda parts: np.bincount(torch.cat(parts).numpy().astype(int), minlength=self.nc) if parts else np.zeros(self.nc, dtype=np.int64)  # noqa: E731
        self.nt_per_class = count(self.stats["target_cls"])
        self.nt_per_image = count(self._target_img)
        if self.with_loss and self.loss is not None:
            self._loss_mean = [float(v) for v in (self.loss / n_batches).cpu()]

    def __call__(self, batches):
        if isinstance(batches, dict):
            batches = [batches]
        was_training = self.model.training
        self.init_metrics()
        self.model.eval()
        n_batches = 0
        try:
            for batch in batches:
                n_batches += 1
                with torch.no_grad():
                    kw = {"augment": True} if self.augment else {}  # (only then: any module that maps an image batch to predictions can be validated)
                    if self.dtype == torch.float32:
                        preds = self.model(batch["img"], **kw)
                        if self.with_loss:
                            items = self.model.loss(batch, preds)[1]
                    else:
                        with torch.autocast("cuda", dtype=self.dtype):
                            preds = self.model(batch["img"], **kw)
                            if self.with_loss:
                                items = self.model.loss(batch, preds)[1]
                    if self.with_loss:
                        self.loss = items.detach().clone() if self.loss is None else self.loss + items.detach()
                    held = self.batch_results(preds, batch)
                    if self.match == "device":
                        self.update_metrics_device(held[0], held[1], batch, *held[2:])
                if self.match == "host":
                    self.update_metrics(*(t.cpu() for t in held), batch)
            self._finish(n_batches)
        finally:
            self.model.train(was_training)
        return self.get_stats()


class SegmentationValidator(DetectionValidator):
    """SegmentationValidator(model)(batches) -> SegmentMetrics.results_dict: the four (B) keys, the four (M) keys and fitness (seg + box); with
    loss=True also val/box_loss, val/seg_loss, val/cls_loss, val/dfl_loss.  Reference models/yolo/segment/val.py.  Batches are
    engine.trainer.synthetic_seg_batch's: the detector's entries and "masks", the overlap encoding [B, mh, mw] at the prototype map's size.
    Per batch: ops.detect_nms_seg, the mask work on the boxes still in network-input pixels, only then ops.scale_boxes; the box statistics follow
    exactly as in DetectionValidator and tp_m is held beside tp.
    match="device": ops.mask_overlap + ops.val_match_masks - no mask is ever stored and nothing crosses to the host until the flush.
    match="host": the reference's statements per image - process_mask(upsample=False), the one-hot of the encoding, mask_iou,
    match_predictions - after one trip of the counts.  Both give the same tp_m, bit for bit (tests/test_gpu_segpred.py).
    Not built, refused here: overlap_mask=False, test-time augmentation, save_json / save_txt (process_mask_native, RLE and polygon output)."""

    _segment = True
    _extra_keys = ("tp_m",)
    loss_names = ("val/box_loss", "val/seg_loss", "val/cls_loss", "val/dfl_loss")

    def __init__(self, model, conf=0.001, iou=0.7, max_det=300, single_cls=False, agnostic_nms=False, dtype=torch.bfloat16, augment=False, match="host",
                 loss=False, overlap_mask=True, save_json=False, save_txt=False):
        if augment:
            raise NotImplementedError("SegmentationValidator: test-time augmentation merges box rows only; it is not built for mask coefficients")
        if not overlap_mask:
            raise NotImplementedError("SegmentationValidator: overlap_mask=False (one ground-truth mask per label) is not built; batches carry the overlap encoding")
        if save_json or save_txt:
            raise NotImplementedError("SegmentationValidator: save_json / save_txt (process_mask_native, RLE and polygon output) are not built")
        super().__init__(model, conf=conf, iou=iou, max_det=max_det, single_cls=single_cls, agnostic_nms=agnostic_nms, dtype=dtype, match=match, loss=loss)

    def init_metrics(self):
        super().init_metrics()
        self.metrics = SegmentMetrics(names={i: str(i) for i in range(self.nc)})
        self.stats = dict(tp_m=[], tp=[], conf=[], pred_cls=[], target_cls=[])

    def postprocess(self, preds):
        """-> (det [B, max_det, 6], coef [B, max_det, nm], count [B], proto [B, nm, mh, mw]) on the device; reference segment/val.py:92-105."""
        y, tail = preds[0], preds[1]
        proto = tail[-1] if isinstance(tail, (list, tuple)) else tail
        det, coef, count = ops.detect_nms_seg(y, self.nc, self.conf, self.iou, multi_label=True, agnostic=self.single_cls or self.agnostic_nms,
                                              max_det=self.max_det)
        return det, coef, count, proto

    def _tp_m_host(self, det, coef, count, proto, batch):
        """segment/val.py:231-273 per image with masks=True, overlap=True -> tp_m [B, max_det, levels] uint8 (host), zero past the count."""
        shape = tuple(batch["img"].shape[2:])
        counts = count.tolist()  # this path's trip of the counts
        bidx = batch["batch_idx"].detach().cpu().reshape(-1)
        cls_all = batch["cls"].detach().cpu().float().reshape(-1)
        tp_m = torch.zeros((det.shape[0], det.shape[1], len(self._levels)), dtype=torch.uint8)
        for si, n in enumerate(counts):
            cls = cls_all[bidx == si]
            nl = len(cls)
            if not n or not nl:
                continue
            pred_masks = process_mask(proto[si], coef[si, :n], det[si, :n, :4], shape).cpu()
            enc = batch["masks"][si].detach().cpu().float()
            if tuple(enc.shape) != tuple(pred_masks.shape[1:]):
                raise NotImplementedError(f"SegmentationValidator: the overlap encoding is {tuple(enc.shape)}, the masks {tuple(pred_masks.shape[1:])}; "
                                          "resampling the encoding (reference segment/val.py:266-268) is not built")
            index = torch.arange(nl).view(nl, 1, 1) + 1
            gt_masks = torch.where(enc[None].repeat(nl, 1, 1) == index, 1.0, 0.0)
            iou = mask_iou(gt_masks.view(nl, -1), pred_masks.view(n, -1).float())
            pred_cls = det[si, :n, 5].cpu()
            if self.single_cls:
                pred_cls, cls = torch.zeros_like(pred_cls), torch.zeros_like(cls)
            tp_m[si, :n] = match_predictions(pred_cls, cls, iou, self.iouv).to(torch.uint8)
        return tp_m

    def batch_results(self, preds, batch):
        """-> (det, count, tp_m): the mask matching on the unscaled boxes, then the detector's box step."""
        det, coef, count, proto = self.postprocess(preds)
        shape = tuple(batch["img"].shape[2:])
        if self.match == "device":
            inter, area_pred, area_gt = ops.mask_overlap(det, coef, count, proto, batch["masks"], shape)
            tp_m = ops.val_match_masks(det, count, batch["batch_idx"], batch["cls"], inter, area_pred, area_gt, self._levels, single_cls=self.single_cls)
        else:
            tp_m = self._tp_m_host(det, coef, count, proto, batch)
        if "ori_shape" in batch and "ratio_pad" in batch:
            det = ops.scale_boxes(det, count, shape, batch["ori_shape"], batch["ratio_pad"], inplace=True)
        return det, count, tp_m

    def update_metrics(self, det, count, tp_m, batch):
        """the detector's host statistics, and tp_m beside every tp it appends (an image with neither detections nor labels appends nothing)."""
        super().update_metrics(det, count, batch)
        bidx = batch["batch_idx"].detach().cpu().reshape(-1)
        for si in range(det.shape[0]):
            n = int(count[si])
            if n or bool((bidx == si).any()):
                self.stats["tp_m"].append(tp_m[si, :n].bool())
