"""GPU: validation statistics on the device - ops.val_match (csrc/valmatch.hip: ymi_val_match) and DetectionValidator(match="device").

Every expectation comes from tests/valmatch_ref.py (held to utils.metrics and to the reference's confusion matrices on the CPU by
tests/test_valmatch_ref_cpu.py), from utils.metrics on the host, or from the reference's fixture; none comes from the device path.  tp and
the confusion matrix must be EQUAL: the kernel is stated one float32 operation at a time in include/ymi.h and valmatch_ref restates it."""
import json

import numpy as np
import pytest
import torch

import nms_exact as NX
import valmatch_ref as VR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

IOUV = torch.linspace(0.5, 0.95, 10)


def dev():
    return torch.device("cuda:0")


def _check(det, count, lab_img, lab_cls, lab_box, img_shape, nc, levels=IOUV, geometry=None, single_cls=False):
    """ops.val_match on the device against valmatch_ref.match on the host: tp and matrix equal.  geometry: (ori_shapes, ratio_pads).
    The matrix starts from ones, so that the kernel is seen to ADD."""
    from improving_yolov8_cbam_swinblock_amd import ops

    native, kw = None, {}
    if geometry is not None:
        native = [ops.scale_boxes_params(img_shape, o, rp) for o, rp in zip(*geometry)]
        kw = dict(ori_shapes=geometry[0], ratio_pads=geometry[1])
    want_tp, want_cm = VR.match(det, count, lab_img, lab_cls, lab_box, img_shape, levels, native=native, single_cls=single_cls, nc=nc)
    cm = torch.ones((nc + 1, nc + 1), dtype=torch.int32, device=dev())
    junk_before = det.clone()
    d = det.to(dev())
    tp = ops.val_match(d, count.to(dev()), lab_img.to(dev()), lab_cls.to(dev()).reshape(-1, 1), lab_box.to(dev()), img_shape, levels, single_cls=single_cls,
                       cm=cm, **kw)
    tp_plain = ops.val_match(d, count.to(dev()), lab_img.to(dev()).float(), lab_cls.to(dev()), lab_box.to(dev()), img_shape, levels, single_cls=single_cls, **kw)
    torch.cuda.synchronize()
    assert tp.dtype == torch.uint8 and tuple(tp.shape) == tuple(want_tp.shape)
    assert torch.equal(d.cpu(), junk_before), "the detections were modified"
    bad = torch.nonzero(tp.cpu() != want_tp)
    assert not len(bad), f"{len(bad)} tp elements differ, first (image, detection, level) {bad[0].tolist()}"
    assert torch.equal(tp_plain.cpu(), want_tp), "tp depends on whether the matrix is asked for"
    assert np.array_equal(cm.cpu().numpy().astype(np.int64) - 1, want_cm), (cm.cpu().numpy() - 1, want_cm)
    return want_tp, want_cm


def _random_batch(seed, counts, labels, max_det, nc, img_shape=(640, 640), native=None):
    """counts / labels: detections and labels per image.  Detections are jittered copies of the image's label boxes (in native pixels when
    `native` is given), a fifth with another class, ranked by confidence; rows past the count hold junk; the label table is shuffled."""
    rs = np.random.RandomState(seed)
    B = len(counts)
    det = torch.from_numpy(rs.uniform(1, 600, size=(B, max_det, 6)).astype(np.float32))
    xywh, cls, img = [], [], []
    for b in range(B):
        m, n = labels[b], counts[b]
        x = np.concatenate((rs.uniform(0.1, 0.9, size=(m, 2)), rs.uniform(0.03, 0.25, size=(m, 2))), 1).astype(np.float32)
        c = rs.randint(0, nc, size=m).astype(np.float32)
        xywh.append(torch.from_numpy(x))
        cls.append(torch.from_numpy(c))
        img.append(torch.full((m,), b, dtype=torch.int32))
        if n:
            if m:
                lab = VR.label_boxes(x, img_shape[1], img_shape[0], None if native is None else native[b]).numpy().astype(np.float64)
                pick = rs.randint(0, m, size=n)
                wh = np.maximum(lab[pick, 2:] - lab[pick, :2], 4.0)
                box = lab[pick] + rs.normal(0, 0.07, size=(n, 4)) * np.concatenate((wh, wh), 1)
                dcls = np.where(rs.uniform(size=n) < 0.8, c[pick], rs.randint(0, nc, size=n))
            else:
                ctr, wh = rs.uniform(50, 500, size=(n, 2)), rs.uniform(10, 100, size=(n, 2))
                box, dcls = np.concatenate((ctr - wh / 2, ctr + wh / 2), 1), rs.randint(0, nc, size=n)
            conf = np.sort(rs.uniform(0.002, 0.99, size=n))[::-1]
            det[b, :n] = torch.from_numpy(np.concatenate((box, conf[:, None], dcls[:, None]), 1).astype(np.float32))
    lab_img, lab_cls, lab_box = torch.cat(img), torch.cat(cls), torch.cat(xywh)
    perm = torch.from_numpy(rs.permutation(len(lab_img)))
    return det, torch.tensor(counts, dtype=torch.int32), lab_img[perm], lab_cls[perm], lab_box[perm]


# ---- ops.val_match ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VR.CASES)
def test_fixture_cases(name):
    nc, images = VR.case(name)
    det, count, lab_img, lab_cls, lab_box = VR.pack(images, 300, shuffle_seed=3)
    if name != "no_labels":
        runs = int((lab_img[1:] != lab_img[:-1]).sum()) + 1
        assert runs > len(images), "the shuffled table must not keep an image's labels together"
    _, cm = _check(det, count, lab_img, lab_cls, lab_box, (VR.IMGSZ, VR.IMGSZ), nc)
    assert np.array_equal(cm, np.array(json.loads((GOLDEN / "confusion_matrix.json").read_text())[name])), "the reference's matrix"


def test_planted_batch():
    det, count, lab_img, lab_cls, lab_box = VR.planted()
    tp, cm = _check(det, count, lab_img, lab_cls, lab_box, VR.PLANTED_SHAPE, VR.PLANTED_NC)
    assert ["".join(str(int(v)) for v in row) for row in tp[3, : int(count[3])]] == VR.PLANTED_TP3 and cm.tolist() == VR.PLANTED_CM


@pytest.mark.parametrize("n_levels", [1, 10])
def test_full_300_detections_and_320_labels_on_one_image(n_levels):
    det, count, lab_img, lab_cls, lab_box = _random_batch(11, [300, 40, 0], [320, 7, 5], 300, 5)
    tp, _ = _check(det, count, lab_img, lab_cls, lab_box, (640, 640), 5, levels=IOUV[:n_levels] if n_levels > 1 else [0.5])
    assert 20 < int(tp[0, :, 0].sum()) < 300


def test_max_det_2048_full_and_two_and_a_half_label_chunks_on_one_image():
    from improving_yolov8_cbam_swinblock_amd import ops

    m = 5 * ops.VAL_MATCH_LABEL_CHUNK // 2
    det, count, lab_img, lab_cls, lab_box = _random_batch(12, [2048, 100], [m, 300], 2048, 80)
    assert int((lab_img == 0).sum()) == m == 2560
    tp, cm = _check(det, count, lab_img, lab_cls, lab_box, (640, 640), 80)
    assert int(tp[0, :, 0].sum()) > 200 and int(np.trace(cm)) > 100


def test_single_cls():
    det, count, lab_img, lab_cls, lab_box = _random_batch(13, [120, 0, 60], [30, 4, 12], 128, 4)
    plain, _ = VR.match(det, count, lab_img, lab_cls, lab_box, (640, 640), IOUV, nc=4)
    tp, cm = _check(det, count, lab_img, lab_cls, lab_box, (640, 640), 4, single_cls=True)
    assert not torch.equal(tp, plain) and cm[0, 0] + cm[0, 4] + cm[4, 0] == cm.sum()


def test_native_space_with_a_shape_and_a_pad_per_image():
    from improving_yolov8_cbam_swinblock_amd import ops

    shape = (384, 640)
    ori = [(480, 640), (1080, 1920), (333, 517), (200, 300)]
    pads = [None, None, ((0.731, 0.731), (41.0, 87.0)), ((1.9, 1.9), (120.0, 7.0))]
    native = [ops.scale_boxes_params(shape, o, rp) for o, rp in zip(ori, pads)]
    det, count, lab_img, lab_cls, lab_box = _random_batch(14, [90, 150, 60, 80], [20, 30, 15, 25], 160, 3, img_shape=shape, native=native)
    plain, _ = VR.match(det, count, lab_img, lab_cls, lab_box, shape, IOUV, nc=3)
    tp, _ = _check(det, count, lab_img, lab_cls, lab_box, shape, 3, geometry=(ori, pads))
    assert not torch.equal(tp, plain) and all(int(tp[b, :, 0].sum()) > 5 for b in range(4))


@pytest.mark.parametrize("B", [1, 33])
def test_batch_sizes(B):
    rs = np.random.RandomState(B)
    counts = [int(v) for v in rs.randint(0, 65, size=B)]
    labels = [int(v) for v in rs.randint(0, 12, size=B)]
    det, count, lab_img, lab_cls, lab_box = _random_batch(15 + B, counts, labels, 64, 3)
    _check(det, count, lab_img, lab_cls, lab_box, (320, 320), 3)


def test_an_empty_label_table_and_argument_checks():
    from improving_yolov8_cbam_swinblock_amd import ops

    det, count, _, _, _ = _random_batch(16, [10, 0], [0, 0], 16, 2)
    none = torch.zeros(0)
    _, cm = _check(det, count, none.int(), none, none.reshape(0, 4), (640, 640), 2)
    assert cm[:2, 2].sum() == int((det[0, :10, 4] > 0.25).sum())
    d, c = det.to(dev()), count.to(dev())
    with pytest.raises(ValueError):
        ops.val_match(d, c, none, none, none.reshape(0, 4), (640, 640), [0.5] * 17)
    with pytest.raises(ValueError):
        ops.val_match(d, c.long(), none, none, none.reshape(0, 4), (640, 640), IOUV)
    with pytest.raises(ValueError):
        ops.val_match(d, c, none, none, none.reshape(0, 4), (640, 640), IOUV, cm=torch.zeros(3, 3, device=dev()))
    with pytest.raises(ValueError):
        ops.val_match(torch.zeros(1, 4096, 6, device=dev()), c[:1], none, none, none.reshape(0, 4), (640, 640), IOUV)


# ---- DetectionValidator(match="device") ------------------------------------------------------------------------------------------------
def _batches(n, seed, keyed=False):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch

    out = [synthetic_batch(2, 256, dev(), seed + i) for i in range(n)]
    for i, b in enumerate(out):
        b["cls"] = (torch.arange(b["cls"].numel(), device=dev()).float().reshape(-1, 1) + i) % 3
        if keyed:  # a letterboxing dataset's keys: another original shape per image, one pad given, one derived
            b["ori_shape"] = [(200 + 10 * i, 180), (120, 250)]
            b["ratio_pad"] = [None, ((1.02, 1.02), (1.0, 66.0))]
    return out


def _both_modes(model, batches, **kw):
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator

    out = []
    for mode in ("host", "device"):
        v = DetectionValidator(model, match=mode, **kw)
        out.append((v, v(batches)))
    return out


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("kind", ["tiny", "from_labels", "single_cls"])
def test_device_and_host_matching_give_identical_results(kind, keyed):
    from test_gpu_validator import _FromLabels, _raise_class_bias, _tiny_model

    batches = _batches(3, 51, keyed)
    if kind == "from_labels":
        model = _FromLabels(3, batches + batches)  # (one y per forward: two validations)
    else:
        model = _tiny_model(3)
        _raise_class_bias(model, torch.cat([b["img"] for b in batches]))
    (vh, rh), (vd, rd) = _both_modes(model, batches, single_cls=kind == "single_cls")
    assert vh.seen == vd.seen == 6 and len(vh.detections) == len(vd.detections) == 6
    assert sum(len(d) for d in vh.detections) > 0
    for a, b in zip(vh.detections, vd.detections):
        assert NX.same_bits(a, b), "detections"
    for k in ("tp", "conf", "pred_cls", "target_cls"):
        a, b = torch.cat(vh.stats[k], 0), torch.cat(vd.stats[k], 0)
        assert a.dtype == b.dtype and NX.same_bits(a, b), k
    assert np.array_equal(vh.confusion_matrix.matrix, vd.confusion_matrix.matrix) and vh.confusion_matrix.matrix.sum() > 0
    assert vd.confusion_matrix.matrix.shape == (4, 4) and vd.confusion_matrix.conf == 0.25
    assert np.array_equal(vh.nt_per_class, vd.nt_per_class) and np.array_equal(vh.nt_per_image, vd.nt_per_image)
    assert int(vd.nt_per_class.sum()) == 24 and (kind == "single_cls") == (int(vd.nt_per_class[0]) == 24)
    assert int(vd.nt_per_image.sum()) == (6 if kind == "single_cls" else 18)  # four labels per image: classes i, i+1, i+2, i+3 mod 3
    assert list(rh) == list(rd) == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"]
    for k in rh:
        assert abs(float(rh[k]) - float(rd[k])) <= 1e-9, (k, rh[k], rd[k])
    if kind == "from_labels" and not keyed:
        assert float(rd["metrics/mAP50(B)"]) > 0.5 and np.trace(vd.confusion_matrix.matrix) >= 18  # (labels that overlap each other suppress one another)
    print(f"[{kind}, keyed {keyed}] detections {[len(d) for d in vd.detections]} tp {int(torch.cat(vd.stats['tp']).sum())} matrix\n{vd.confusion_matrix.matrix}")


class _Crossings:
    """counts the calls that take a cuda tensor's data to the host"""

    def __init__(self, monkeypatch):
        self.n = 0
        for name in ("cpu", "tolist", "item", "numpy", "__bool__", "__int__", "__float__"):
            monkeypatch.setattr(torch.Tensor, name, self._wrap(getattr(torch.Tensor, name), lambda t, r: t.is_cuda))
        monkeypatch.setattr(torch.Tensor, "to", self._wrap(torch.Tensor.to, lambda t, r: t.is_cuda and torch.is_tensor(r) and not r.is_cuda))

    def _wrap(self, real, crosses):
        def call(t, *a, **k):
            r = real(t, *a, **k)
            self.n += bool(crosses(t, r))
            return r

        return call


def test_device_matching_crosses_to_the_host_once_per_validation(monkeypatch):
    """the number of device -> host crossings during v(batches) does not depend on the number of batches in device mode; in host mode it
    grows with it (which shows that the counter counts)"""
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from test_gpu_validator import _raise_class_bias, _tiny_model

    model = _tiny_model(3)
    batches = _batches(5, 61)
    _raise_class_bias(model, torch.cat([b["img"] for b in batches[:2]]))
    DetectionValidator(model, match="device", loss=True)(batches[:1])  # (first-use set-up, the criterion's included, stays out of the counts)
    counter = _Crossings(monkeypatch)
    seen = {}
    for mode in ("device", "host"):
        for n in (2, 5):
            v = DetectionValidator(model, match=mode, loss=True)
            before = counter.n
            v(batches[:n])
            seen[mode, n] = counter.n - before
            assert v.seen == 2 * n
    print(f"device -> host crossings: {seen}")
    assert seen["device", 2] == seen["device", 5] > 0
    assert seen["host", 5] >= seen["host", 2] + 3 * 2, "the counter does not see the host path's per-batch trips"


def test_validation_loss():
    """loss=True: val/box_loss, val/cls_loss, val/dfl_loss are the mean over the batches of model.loss(batch, preds)[1] on the same eval
    forward, bit for bit (if two direct evaluations differ among themselves: within twice their spread, printed below; 0 was observed)."""
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from test_gpu_validator import _tiny_model

    model = _tiny_model(3)
    batches = _batches(3, 71)

    def direct():
        total = None
        model.eval()
        with torch.no_grad():
            for b in batches:
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    preds = model(b["img"])
                    items = model.loss(b, preds)[1].detach()
                total = items.clone() if total is None else total + items
        return (total / len(batches)).cpu()

    a, b = direct(), direct()
    spread = float((a - b).abs().max())
    for mode in ("device", "host"):
        res = DetectionValidator(model, match=mode, loss=True)(batches)
        assert list(res) == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness", "val/box_loss", "val/cls_loss",
                             "val/dfl_loss"]
        got = torch.tensor([res["val/box_loss"], res["val/cls_loss"], res["val/dfl_loss"]], dtype=torch.float32)
        print(f"[{mode}] val losses {got.tolist()} direct {a.tolist()} spread of two direct evaluations {spread:.3e}")
        assert bool(torch.isfinite(got).all()) and float(got.min()) > 0
        assert float((got - a).abs().max()) <= 2 * spread, (got, a, spread)
    plain = DetectionValidator(model, match="device")(batches)
    assert list(plain) == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness"]
