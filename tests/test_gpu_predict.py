"""GPU: prediction on real images - ops.letterbox / ops.scale_boxes (csrc/resize.hip) against tests/letterbox_ref.py and the reference's
fixtures, then engine.predictor.DetectionPredictor and the native-space path of engine.validator.DetectionValidator.

The kernels are held to the restatement BIT FOR BIT (images) and as values (boxes: +0 and -0 compare equal); the restatement is held to the
fixtures of the real reference on the CPU by tests/test_letterbox_ref_cpu.py.  The predictor is compared teacher-forced on the product's own
decoded y: letterbox, model, detect_nms, then the restatement's scale_boxes."""
import json

import numpy as np
import pytest
import torch

import letterbox_ref as LR
from conftest import GOLDEN, golden_state, load_golden

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.asarray(a))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ letterbox
@pytest.mark.parametrize("name", list(LR.CASES))
def test_letterbox_equals_the_restatement_and_the_fixture_bit_for_bit(name):
    from improving_yolov8_cbam_swinblock_amd import ops

    d, c = load_golden(f"predict_{name}"), LR.CASES[name]
    sw, images = LR.case_switches(c), LR.case_images(name)
    got, rp = ops.letterbox(images, c["new_shape"], **sw)
    want, want_rp = LR.letterbox(images, c["new_shape"], **sw)
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous()
    assert same_bits(got.cpu(), want)
    assert rp == want_rp and [list(r[1]) for r in rp] == d["pad_left_top"].tolist()
    if "pre_u8" in d:
        assert same_bits(got.cpu(), t(d["pre_u8"]).float() / 255), "BasePredictor.preprocess's own output"
    # the 0..255 form in the image's own channel order is LetterBox's own output
    raw, _ = ops.letterbox(images, c["new_shape"], bgr=False, normalize=False, **sw)
    assert same_bits(raw.cpu(), t(d["out"]).permute(0, 3, 1, 2).contiguous().float())


def _ragged(n, seed):
    rs = np.random.RandomState(seed)
    sizes = [(37, 53), (90, 60), (120, 67), (200, 150), (48, 64), (64, 64), (64, 17), (5, 64), (1, 1), (3, 200), (65, 64), (64, 63)]
    sizes += [(int(rs.randint(2, 140)), int(rs.randint(2, 140))) for _ in range(n - len(sizes))]
    return [LR.seeded_image(900 + i, h, w) for i, (h, w) in enumerate(sizes[:n])]


def test_one_launch_holds_a_ragged_list():
    from improving_yolov8_cbam_swinblock_amd import ops

    images = _ragged(12, 1)  # 12 <= 32: one launch
    got, rp = ops.letterbox(images, 64)
    want, want_rp = LR.letterbox(images, 64)
    assert tuple(got.shape) == (12, 3, 64, 64) and rp == want_rp
    bad = [i for i in range(12) if not same_bits(got[i].cpu(), want[i])]
    assert not bad, [images[i].shape for i in bad]


def test_a_list_longer_than_one_launch():
    from improving_yolov8_cbam_swinblock_amd import ops

    images = _ragged(71, 2)  # 32 + 32 + 7: three launches
    got, _ = ops.letterbox(images, (64, 96))
    want, _ = LR.letterbox(images, (64, 96))
    bad = [i for i in range(len(images)) if not same_bits(got[i].cpu(), want[i])]
    assert not bad, bad


def test_host_device_and_mixed_inputs_agree():
    from improving_yolov8_cbam_swinblock_amd import ops

    images = _ragged(9, 3)
    host, _ = ops.letterbox(images, 64)
    tens, _ = ops.letterbox([torch.from_numpy(im) for im in images], 64)
    on_dev, _ = ops.letterbox([torch.from_numpy(im).to(dev()) for im in images], 64)
    mixed, _ = ops.letterbox([torch.from_numpy(im).to(dev()) if i % 2 else im for i, im in enumerate(images)], 64)
    view, _ = ops.letterbox([np.ascontiguousarray(np.pad(im, ((0, 0), (0, 3), (0, 0))))[:, : im.shape[1]] for im in images], 64)  # non-contiguous rows
    for other in (tens, on_dev, mixed, view):
        assert same_bits(host, other)


def test_pad_region_ramp_and_every_byte_value_are_exact():
    from improving_yolov8_cbam_swinblock_amd import ops

    # all 256 byte values through the identity path and the conversion: img.float() / 255 exactly; pad = 114 / 255 exactly
    img = np.zeros((16, 16, 3), np.uint8)
    img[..., 0] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img[..., 1] = img[..., 0][::-1]
    img[..., 2] = img[..., 0].T
    got, rp = ops.letterbox([img], (24, 32))
    assert rp == [((1.5, 1.5), (4, 0))]
    got1, rp1 = ops.letterbox([img], (24, 32), scaleup=False)
    assert rp1 == [((1.0, 1.0), (8, 4))]
    want = torch.full((3, 24, 32), 114.0) / 255
    want[:, 4:20, 8:24] = t(img).flip(-1).permute(2, 0, 1).float() / 255
    assert same_bits(got1[0].cpu(), want)
    for pv in (0, 114, 255):
        out, _ = ops.letterbox([img], (24, 32), scaleup=False, pad_value=pv, normalize=False)
        mask = torch.ones(24, 32, dtype=torch.bool)
        mask[4:20, 8:24] = False
        assert bool((out[0].cpu()[:, mask] == float(pv)).all())
    # a ramp: every output element of an up- and a down-scaling, against the restatement, and monotone along the ramp
    ramp = np.stack([np.tile(np.arange(100, dtype=np.uint8) * 2, (40, 1))] * 3, -1)
    ramp[..., 1] = ramp[..., 0].max() - ramp[..., 1]
    for target in ((64, 160), (16, 40), (50, 66)):  # (50, 66): a row length that is no multiple of four takes the scalar stores
        got, _ = ops.letterbox([ramp], target, scale_fill=True, normalize=False)
        want, _ = LR.letterbox([ramp], target, scale_fill=True, normalize=False)
        assert same_bits(got.cpu(), want)
        assert bool((got[0, 2].diff(dim=1) >= 0).all()) and bool((got[0, 1].diff(dim=1) <= 0).all())
        assert float(got.min()) >= 0 and float(got.max()) <= 198 and bool((got == got.round()).all())


def test_letterbox_refuses_what_it_cannot_do():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.data.augment import LetterBox

    with pytest.raises(ValueError, match="different sizes"):
        ops.letterbox([LR.seeded_image(1, 50, 83), LR.seeded_image(2, 83, 50)], 96, auto=True)
    with pytest.raises(ValueError, match="uint8"):
        ops.letterbox([np.zeros((4, 4, 3), np.float32)], 64)
    with pytest.raises(ValueError, match="uint8"):
        ops.letterbox([np.zeros((4, 4), np.uint8)], 64)
    with pytest.raises(NotImplementedError):
        LetterBox(64)(labels={"img": LR.seeded_image(1, 37, 53)})
    img = LR.seeded_image(501, 37, 53)
    out = LetterBox(64)(image=img)  # the reference's class: the letterboxed image, HWC, grey levels, the image's own channel order
    assert same_bits(out.cpu().contiguous(), t(load_golden("predict_s37x53")["out"][0]).float())


# ---------------------------------------------------------------------------------------------------------------- scale_boxes
@pytest.mark.parametrize("name", list(LR.CASES))
def test_scale_boxes_equals_the_fixtures(name):
    """the batch form on (det, count) with every image of the case, and utils.ops.scale_boxes / clip_boxes in place on one tensor"""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.utils import ops as uops

    d, c = load_golden(f"predict_{name}"), LR.CASES[name]
    img1 = tuple(d["out"].shape[1:3])
    ori = [(h0, w0) for _, h0, w0 in c["images"]]
    det = torch.stack([LR.seeded_boxes(700 + i, 24, img1) for i in range(len(ori))])
    count = torch.full((len(ori),), 24, dtype=torch.int32)
    rps = [((float(d[f"rp{i}_gain"]),) * 2, tuple(int(v) for v in d[f"rp{i}_pad"])) for i in range(len(ori))]
    forms = {"rows": {}, "rp": dict(ratio_pads=rps), "nopad": dict(padding=False), "xywh": dict(xywh=True)}
    for key, kw in forms.items():
        got = ops.scale_boxes(det.to(dev()), count.to(dev()), img1, ori, **kw).cpu()
        assert torch.equal(got, LR.scale_boxes(det, count, img1, ori, **kw)), key
        for i in range(len(ori)):
            assert torch.equal(got[i, :, :4], t(d[f"{key if key != 'rows' else 'none'}{i}"])), (key, i)
            assert torch.equal(got[i, :, 4:], det[i, :, 4:])
    for i, img0 in enumerate(ori):
        b4 = det[i, :, :4].contiguous()
        x = b4.to(dev())
        assert uops.scale_boxes(img1, x, img0) is x and torch.equal(x.cpu(), t(d[f"none{i}"]))
        assert torch.equal(uops.scale_boxes(img1, b4.to(dev()), img0, ratio_pad=rps[i]).cpu(), t(d[f"rp{i}"]))
        assert torch.equal(uops.scale_boxes(img1, b4.to(dev()), img0, padding=False).cpu(), t(d[f"nopad{i}"]))
        assert torch.equal(uops.scale_boxes(img1, b4.to(dev()), img0, xywh=True).cpu(), t(d[f"xywh{i}"]))
        x = b4.to(dev())
        assert uops.clip_boxes(x, img0) is x and torch.equal(x.cpu(), t(d[f"clip{i}"]))
        full = det[i].to(dev())
        uops.scale_boxes(img1, full[:, :4], img0)  # a view with row stride 6, as construct_result passes it
        assert torch.equal(full.cpu(), t(d[f"rows{i}"]))


def test_scale_boxes_counts_in_place_and_more_than_one_block():
    from improving_yolov8_cbam_swinblock_amd import ops

    B, M = 5, 300  # 300 rows: two blocks of 256 lanes per image
    ori = [(37, 53), (90, 60), (120, 67), (200, 150), (48, 64)]
    counts = [300, 0, 1, 257, 256]
    det = torch.zeros(B, M, 6)
    for b, n in enumerate(counts):
        det[b, :n] = LR.seeded_boxes(50 + b, max(n, 5), (64, 64))[:n]
    count = torch.tensor(counts, dtype=torch.int32)
    want = LR.scale_boxes(det, count, (64, 64), ori)
    d = det.to(dev())
    got = ops.scale_boxes(d, count.to(dev()), (64, 64), ori)
    assert got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), det), "out of place: the input is untouched"
    assert torch.equal(got.cpu(), want)
    for b, n in enumerate(counts):
        assert bool((got[b, n:] == 0).all()), "rows at or beyond count stay zero"
    # rows beyond count that are NOT zero on entry: written as zeros out of place, left alone in place
    dirty = det.clone()
    dirty[1, :, :] = 7.0
    got = ops.scale_boxes(dirty.to(dev()), count.to(dev()), (64, 64), ori)
    assert torch.equal(got.cpu(), want)
    d = det.to(dev())
    same = ops.scale_boxes(d, count.to(dev()), (64, 64), ori, inplace=True)
    assert same.data_ptr() == d.data_ptr() and torch.equal(d.cpu(), want)
    # one shape for all, one ratio_pad for all, xywh in place
    rp = ((0.5, 0.5), (3, 2))
    d = det.to(dev())
    ops.scale_boxes(d, count.to(dev()), (64, 64), (100, 90), rp, xywh=True, inplace=True)
    assert torch.equal(d.cpu(), LR.scale_boxes(det, count, (64, 64), [(100, 90)] * B, [rp] * B, xywh=True))
    with pytest.raises(RuntimeError, match="MI355X|cuda"):
        ops.scale_boxes(det, count, (64, 64), ori)


def test_scale_boxes_divides_as_the_header_says():
    """x / float32(gain) in IEEE float32: a gain whose reciprocal product and whose double-precision quotient both differ from it somewhere"""
    from improving_yolov8_cbam_swinblock_amd import ops

    gain = 64 / 90
    x = torch.arange(1, 4097, dtype=torch.float32) * 0.37
    det = torch.zeros(1, 1024, 6)
    det[0, :, :4] = x.reshape(1024, 4)
    count = torch.tensor([1024], dtype=torch.int32)
    rp = ((gain, gain), (0, 0))
    got = ops.scale_boxes(det.to(dev()), count.to(dev()), (64, 64), (10000, 10000), rp).cpu()[0, :, :4].reshape(-1)
    g32 = torch.tensor(gain, dtype=torch.float32)
    assert torch.equal(got, x / g32)
    y = x.clone()
    y /= gain
    assert torch.equal(got, y), "tensor /= python_float"
    assert not torch.equal(got, x * (1 / g32)) and not torch.equal(got, (x.double() / gain).float()), "the probe tells the three rules apart"


# ------------------------------------------------------------------------------------------------------- predictor, validator
def _tiny_model():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    model = DetectionModel(cfg, ch=3, nc=1)
    model.load_state_dict(golden_state(load_golden("e2e_tiny_seed7")), strict=True)
    return model.to(dev())


def _raise_class_bias(model, img, conf):
    """shift the class branch's bias until some tens of anchors per image score above conf (asserted by the callers on the result)"""
    with torch.no_grad():
        y = model.eval()(img)[0]
        top = y[:, 4:].amax(1).flatten().sort(descending=True)[0]
        target = float(top[min(len(top) - 1, 30 * img.shape[0])])
        want = 2 * conf
        shift = float(np.log(want / (1 - want)) - np.log(max(target, 1e-12) / max(1 - target, 1e-12)))
        for m in model.model[-1].cv3:
            m[-1].bias.add_(shift)


def _shrink_boxes(model):
    """the fixture's box branch predicts distances of several strides, i.e. boxes larger than a 64-pixel image, which the clip would turn into
    the image's own frame: lean the DFL distribution of every side towards its first bins so that most corners fall inside the image"""
    with torch.no_grad():
        for m in model.model[-1].cv2:
            m[-1].bias.view(4, -1).sub_(0.7 * torch.arange(m[-1].bias.numel() // 4, device=m[-1].bias.device, dtype=torch.float32))


def test_predictor_equals_the_composition_of_its_parts():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.predictor import DetectionPredictor
    from improving_yolov8_cbam_swinblock_amd.engine.results import Boxes, Results

    model = _tiny_model()
    images = [LR.seeded_image(31, 37, 53), LR.seeded_image(32, 90, 60), LR.seeded_image(33, 64, 64)]
    ori = [im.shape[:2] for im in images]
    img, _ = ops.letterbox(images, 64)
    conf = 0.25
    _shrink_boxes(model)
    _raise_class_bias(model, img, conf)
    model.train()
    p = DetectionPredictor(model, imgsz=64, batch=2)  # two chunks: 2 + 1 images
    assert (p.conf, p.iou, p.max_det, p.classes, p.agnostic_nms, p.dtype, p.augment, p.rect) == (0.25, 0.7, 300, None, False, torch.bfloat16, False, False)
    seen, post = [], p.postprocess
    p.postprocess = lambda preds, im, shapes: (seen.append((preds[0].detach().clone(), im.detach().clone())), post(preds, im, shapes))[1]
    res = p(images, paths=["a", "b", "c"])
    assert model.training, "the predictor must restore the mode it found"
    assert len(res) == 3 and len(seen) == 2 and all(isinstance(r, Results) and isinstance(r.boxes, Boxes) for r in res)
    assert [r.path for r in res] == ["a", "b", "c"] and [r.orig_shape for r in res] == [tuple(o) for o in ori] and res[0].names == model.names
    want_img, _ = LR.letterbox(images, 64)
    assert same_bits(torch.cat([s[1] for s in seen]).cpu(), want_img), "what the model saw is the letterboxed batch"
    k, raw_rows = 0, []
    for y, im in seen:
        det, count = ops.detect_nms(y, 0.25, 0.7, max_det=300)
        raw_rows += [det[b, : int(count[b])].cpu() for b in range(y.shape[0])]
        want = LR.scale_boxes(det.cpu(), count.cpu(), (64, 64), ori[k : k + y.shape[0]])
        for b in range(y.shape[0]):
            r = res[k + b]
            assert r.boxes.data.is_cuda and len(r.boxes) == int(count[b])
            assert torch.equal(r.boxes.data.cpu(), want[b, : int(count[b])])
            h0, w0 = r.orig_shape
            xyxy = r.boxes.xyxy
            assert bool((xyxy[:, [0, 2]] >= 0).all() and (xyxy[:, [0, 2]] <= w0).all() and (xyxy[:, [1, 3]] >= 0).all() and (xyxy[:, [1, 3]] <= h0).all())
            props = LR.boxes_properties(r.boxes.data.cpu(), r.orig_shape)
            for name, v in props.items():
                assert torch.equal(getattr(r.boxes, name).cpu(), v), name
        k += y.shape[0]
    n = [len(r.boxes) for r in res]
    inside = [int(((r.boxes.xyxyn > 0) & (r.boxes.xyxyn < 1)).sum()) for r in res]
    print(f"detections per image {n}; corner coordinates strictly inside the image {inside}")
    assert min(n) >= 1 and sum(n) >= 6, n
    assert min(inside) >= 4, "the comparison must not rest on boxes that the clip turned into the image's frame"
    moved = [not torch.equal(r.boxes.data.cpu(), det_row) for r, det_row in zip(res, raw_rows)]
    assert moved[0] and moved[1], "the letterboxed images' boxes were rescaled"
    # a single image, not in a list
    one = p(images[0])
    assert len(one) == 1 and one[0].orig_shape == (37, 53) and one[0].path is None


def test_predictor_passes_a_float_tensor_through():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.engine.predictor import DetectionPredictor

    model = _tiny_model().eval()
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(5)).to(dev())
    _raise_class_bias(model, x, 0.25)
    p = DetectionPredictor(model, imgsz=64, dtype=torch.float32)
    seen, post = [], p.postprocess
    p.postprocess = lambda preds, im, shapes: (seen.append((preds[0].detach().clone(), im)), post(preds, im, shapes))[1]
    res = p(x)
    assert not model.training and len(res) == 2 and [r.orig_shape for r in res] == [(64, 64)] * 2
    y, im = seen[0]
    assert same_bits(im, x), "unletterboxed and unnormalised"
    with torch.no_grad():
        assert torch.equal(model(x)[0], y)
    det, count = ops.detect_nms(y, 0.25, 0.7, max_det=300)
    want = LR.scale_boxes(det.cpu(), count.cpu(), (64, 64), [(64, 64)] * 2)  # gain 1, pad 0: the clip alone
    assert sum(int(c) for c in count) >= 2
    for b in range(2):
        assert torch.equal(res[b].boxes.data.cpu(), want[b, : int(count[b])])


class _Fixed(torch.nn.Module):
    """stands in for a model: nc classes and an eval forward whose result the test's postprocess replaces"""

    class _Head(torch.nn.Module):
        def __init__(self, nc):
            super().__init__()
            self.nc = nc

    def __init__(self, nc):
        super().__init__()
        self.model = torch.nn.ModuleList([self._Head(nc)])

    def forward(self, img):
        return torch.zeros(img.shape[0], 4 + self.model[-1].nc, 8, device=img.device), None


def test_validator_matches_in_native_space(monkeypatch):
    """a batch with ori_shape / ratio_pad: the predictions the matcher sees are the reference's _prepare_pred, the labels its _prepare_batch"""
    from improving_yolov8_cbam_swinblock_amd.engine import validator as V

    d = load_golden("predict_val_prepare")
    batch, preds = LR.val_batch()
    batch = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items()}
    batch["img"] = torch.zeros(2, 3, *LR.VAL_IMGSZ, device=dev())
    v = V.DetectionValidator(_Fixed(3), max_det=16)
    det = torch.zeros(2, 16, 6)
    for i, p in enumerate(preds):
        det[i, :12] = p
    v.postprocess = lambda _: (det.to(dev()), torch.tensor([12, 12], dtype=torch.int32, device=dev()))
    labels, real = [], V.box_iou
    monkeypatch.setattr(V, "box_iou", lambda a, b: (labels.append(a.clone()), real(a, b))[1])
    res = v(batch)
    assert v.seen == 2 and len(labels) == 2
    for si in range(2):
        assert torch.equal(v.detections[si], t(d[f"predn{si}"])), "native-space predictions"
        assert torch.equal(labels[si], t(d[f"bbox{si}"])), "native-space labels"
    assert all(np.isfinite(float(x)) for x in res.values())


def test_a_batch_without_the_keys_takes_the_unchanged_path():
    """with an identity ratio_pad the native-space path computes x - 0, x / 1 and the clip: the same detections clipped, and - for predictions
    that lie inside the image - the same numbers"""
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from test_gpu_validator import _FromLabels

    batches = [synthetic_batch(2, 256, dev(), 21 + i) for i in range(2)]
    keyed = [dict(b, ori_shape=[(256, 256)] * 2, ratio_pad=[((1.0, 1.0), (0, 0))] * 2) for b in batches]
    v0 = DetectionValidator(_FromLabels(1, batches))
    r0 = v0(batches)
    v1 = DetectionValidator(_FromLabels(1, batches))
    r1 = v1(keyed)
    assert {k: float(x) for k, x in r0.items()} == {k: float(x) for k, x in r1.items()} and float(r0["metrics/mAP50(B)"]) > 0.9
    assert all(torch.equal(a, b) for a, b in zip(v0.detections, v1.detections))
    # a real model, whose boxes may cross the border: the keyed path's detections are the plain path's, clipped
    model = _tiny_model()
    img = torch.cat([b["img"] for b in batches])
    with torch.no_grad():
        y = model.eval()(img)[0]
        top = y[:, 4:].amax(1).flatten().sort(descending=True)[0]
        shift = float(np.log(0.02 / 0.98) - np.log(max(float(top[400]), 1e-12) / max(1 - float(top[400]), 1e-12)))
        for m in model.model[-1].cv3:
            m[-1].bias.add_(shift)
    v0, v1 = DetectionValidator(model), DetectionValidator(model)
    v0(batches), v1(keyed)
    assert sum(len(x) for x in v0.detections) > 0
    for a, b in zip(v0.detections, v1.detections):
        c = a.clone()
        c[:, :4] = c[:, :4].clamp(0, 256)
        assert torch.equal(b, c)
