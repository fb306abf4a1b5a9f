"""GPU: csrc/resize.hip (ops.scale_image, ops.tta_merge) and what is built on it - utils.torch_utils.scale_img, DetectionModel.predict(augment=True),
DetectionValidator(augment=True), engine.trainer.preprocess_batch and TrainStep(image_shapes=N).

References: the fixtures the real reference produced (tests/golden/make_tta_golden.py) and tests/tta_ref.py, the pure-torch restatement that
tests/test_tta_ref_cpu.py holds to those fixtures.  Bounds:
  * exact (bit for bit): identity-size and uint8 -> float / 255 paths, the padded region, which source pixels are read (ramp images), class rows
    and anchor ranges of the merge, the loss of a step on a preprocessed uint8 batch;
  * interpolated pixels of [0, 1] images: 1e-5 absolute - five times the 2.0e-6 by which the plain float32 formula and F.interpolate differ over
    these shapes (rounding of the weights); an index or half-pixel error on random uint8 data is >= 1e-2;
  * merged boxes: 1e-6 relative (a division against a multiplication by the reciprocal is one rounding);
  * predict(augment=True) against the reference model: 1e-3 of the output's magnitude, the bound of the eval-mode decode comparison of the same
    model in tests/test_gpu_modules_golden.py::test_e2e_tiny_model_vs_reference;
  * graph against eager over several image shapes: the bounds of tests/test_gpu_fullsize.py::test_hip_graph_step_matches_eager_and_is_isolated.
Measured on an MI355X: every interpolated comparison with the restatement came out at 0.0 (the kernel rounds as the restatement does), against the
reference fixtures at <= 2.0e-6."""
import json
import random

import numpy as np
import pytest
import torch

import tta_ref as TR
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

INTERP_TOL = 1e-5
SCALE_CASES = ["a83", "a67_lr", "b83", "b83_same", "b150", "b100"]
PRE_CASES = ["down32", "up96", "same64", "rect96", "plain"]


def dev():
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.asarray(a))


def _ops():
    from improving_yolov8_cbam_swinblock_amd import ops

    return ops


# ---- scale_image --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCALE_CASES)
def test_scale_img_matches_the_reference_fixture_and_the_restatement(name):
    from improving_yolov8_cbam_swinblock_amd.utils.torch_utils import scale_img

    d = load_golden(f"tta_scale_{name}")
    u8, ref = t(d["img"]), t(d["out"])
    ratio, same, gs, flip = float(d["ratio"]), bool(d["same_shape"]), int(d["gs"]), int(d["flip"])
    xf = TR.to_unit(u8)
    if ratio == 1.0:
        g = xf.to(dev())
        assert scale_img(g, ratio, same, gs) is g, "ratio 1.0 returns the image itself"
        return
    (hs, ws), (hp, wp) = TR.scale_img_sizes(u8.shape[2], u8.shape[3], ratio, same, gs)
    want = TR.scale_image(u8, (hs, ws), (hp, wp), TR.PAD_VALUE, flip=flip or None)
    pad = torch.ones(hp, wp, dtype=torch.bool)
    pad[:hs, :ws] = False
    # the reference's call (a float image, flipped by the caller) through scale_img, and the one-launch form on the uint8 image
    src_f = (xf.flip(flip) if flip else xf).contiguous().to(dev())
    outs = {"scale_img(float32)": scale_img(src_f, ratio, same, gs), "scale_image(uint8, flip)": _ops().scale_image(u8.to(dev()), (hs, ws), (hp, wp), TR.PAD_VALUE, flip=flip or None)}
    if not flip:
        outs["scale_img(uint8)"] = scale_img(u8.to(dev()), ratio, same, gs)
    for what, got in outs.items():
        got = got.cpu()
        assert got.shape == ref.shape and got.dtype == torch.float32 and got.is_contiguous()
        assert torch.equal(got[:, :, pad], ref[:, :, pad]), f"{what}: padded region"
        e_ref, e_re = float((got - ref).abs().max()), float((got - want).abs().max())
        print(f"[{name}] {what}: {hs}x{ws} in {hp}x{wp}  max abs err vs reference {e_ref:.2e}, vs restatement {e_re:.2e} (bound {INTERP_TOL:.0e})")
        assert e_ref <= INTERP_TOL and e_re <= INTERP_TOL, what


def test_identity_size_and_uint8_conversion_are_exact():
    ops = _ops()
    # every byte value, widths that are and are not multiples of 4 (vector and scalar loads / stores), an odd offset into the storage
    base = torch.arange(256, dtype=torch.uint8).repeat(2 * 3 * 12 * 20 // 256 + 1)
    for shape, off in [((2, 3, 12, 20), 0), ((2, 3, 12, 20), 1), ((1, 3, 10, 18), 0), ((1, 2, 7, 13), 3)]:
        n = int(np.prod(shape))
        u8 = base[off : off + n].reshape(shape)
        g = base.to(dev())[off : off + n].reshape(shape)
        want = u8.float() / 255
        assert torch.equal(ops.scale_image(g, shape[2:]).cpu(), want), (shape, off)
        assert torch.equal(ops.scale_image(g, shape[2:], normalize=False).cpu(), u8.float())
        for flip in (2, 3, (2, 3)):
            assert torch.equal(ops.scale_image(g, shape[2:], flip=flip).cpu(), want.flip(flip)), (shape, off, flip)
        gf = want.to(dev())
        assert torch.equal(ops.scale_image(gf, shape[2:]).cpu(), want)
        assert torch.equal(ops.scale_image(gf, shape[2:], flip=3).cpu(), want.flip(3))
        # identity size inside a larger destination: the padding is written by the same launch
        out = ops.scale_image(g, shape[2:], (shape[2] + 5, shape[3] + 7), pad_value=0.447).cpu()
        assert torch.equal(out[:, :, : shape[2], : shape[3]], want)
        rest = torch.ones(out.shape[2:], dtype=torch.bool)
        rest[: shape[2], : shape[3]] = False
        assert bool((out[:, :, rest] == np.float32(0.447)).all())
    full = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16)
    assert torch.equal(ops.scale_image(full.to(dev()), (16, 16)).cpu(), full.float() / 255), "all 256 byte values round as img.float() / 255"


@pytest.mark.parametrize("shape,size,padded", [((1, 2, 40, 72), (33, 59), (64, 64)), ((2, 1, 24, 36), (36, 54), (36, 54)), ((1, 1, 96, 128), (64, 85), (96, 96)),
                                               ((1, 1, 64, 64), (32, 32), (32, 32)), ((1, 1, 5, 7), (11, 3), (12, 6))])
def test_ramp_images_pin_which_source_pixels_are_read(shape, size, padded):
    """a ramp along x (value = column) and along y (value = row): the output is l0 * i0 + l1 * i1 of the indices themselves, so any other
    neighbour, weight or clamp shows; the products and sums are float32 operations on both sides, hence bit equality."""
    ops = _ops()
    b, c, h, w = shape
    ramp_x = torch.arange(w, dtype=torch.float32).expand(b, c, h, w).contiguous()
    ramp_y = torch.arange(h, dtype=torch.float32)[:, None].expand(b, c, h, w).contiguous()
    code = (torch.arange(h, dtype=torch.float32)[:, None] * 256 + torch.arange(w, dtype=torch.float32)).expand(b, c, h, w).contiguous()
    for img in (ramp_x, ramp_y, code, code.to(torch.uint8)):
        for flip in (None, 3, 2):
            norm = False if img.dtype == torch.uint8 else None
            got = ops.scale_image(img.to(dev()), size, padded, pad_value=-1.0, flip=flip, normalize=norm).cpu()
            want = TR.scale_image(img, size, padded, pad_value=-1.0, flip=flip, normalize=norm)
            assert torch.equal(got, want), (shape, size, flip, img.dtype, float((got - want).abs().max()))
    # the indices and weights themselves: rows kept (vertical weights exactly 1 and 0), so a row of the output is l0 * i0 + l1 * i1
    i0, i1, l0, l1 = TR.bilinear_taps(size[1], w)
    got = ops.scale_image(ramp_x.to(dev()), (h, size[1])).cpu()
    assert torch.equal(got, (l0 * i0.float() + l1 * i1.float()).expand(b, c, h, size[1]))
    j0, j1, m0, m1 = TR.bilinear_taps(size[0], h)
    got = ops.scale_image(ramp_y.to(dev()), (size[0], w)).cpu()
    assert torch.equal(got, (m0 * j0.float() + m1 * j1.float())[:, None].expand(b, c, size[0], w))


@pytest.mark.parametrize("ratio", [0.83, 0.67])
def test_tta_sizes_of_a_640_image(ratio):
    """the sizes test-time augmentation produces at 640: 531 in 544 and 428 in 448 - ws % 4 = 3 and 0, several hundred workgroups"""
    ops = _ops()
    u8 = TR.seeded_u8(11, (1, 3, 640, 640))
    (hs, ws), (hp, wp) = TR.scale_img_sizes(640, 640, ratio, False, 32)
    assert (hs, hp) in ((531, 544), (428, 448))
    got = ops.scale_image(u8.to(dev()), (hs, ws), (hp, wp), TR.PAD_VALUE, flip=3).cpu()
    want = TR.scale_image(u8, (hs, ws), (hp, wp), TR.PAD_VALUE, flip=3)
    ref = torch.nn.functional.interpolate(TR.to_unit(u8).flip(3), size=(hs, ws), mode="bilinear", align_corners=False)
    err = float((got - want).abs().max())
    print(f"[640 x {ratio}] {hs} in {hp}: max abs err vs restatement {err:.2e} (bound {INTERP_TOL:.0e}); vs F.interpolate on the CPU {float((got[:, :, :hs, :ws] - ref).abs().max()):.2e}")
    assert torch.equal(got[:, :, hs:], want[:, :, hs:]) and torch.equal(got[:, :, :, ws:], want[:, :, :, ws:])
    assert err <= INTERP_TOL


def test_scale_image_refuses_what_it_cannot_do():
    ops = _ops()
    g = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=dev())
    with pytest.raises(RuntimeError):
        ops.scale_image(g.cpu(), (8, 8))
    with pytest.raises(ValueError):
        ops.scale_image(g, (8, 8), (4, 8))
    with pytest.raises(ValueError):
        ops.scale_image(g.float(), (8, 8), normalize=True)
    with pytest.raises(ValueError):
        ops.scale_image(g.half(), (8, 8))
    with pytest.raises(ValueError):
        ops.scale_image(g, (8, 8), flip=1)


# ---- tta_merge ------------------------------------------------------------------------------------------------------------------------
def _assert_merged(got, want):
    assert got.shape == want.shape
    assert torch.equal(got[:, 4:], want[:, 4:]), "class rows are copied bit for bit"
    torch.testing.assert_close(got[:, :4], want[:, :4], rtol=1e-6, atol=0)


def test_tta_merge_matches_the_reference_and_the_restatement():
    ops = _ops()
    d = load_golden("tta_descale")
    preds = [t(d[f"p{i}"]) for i in range(3)]
    scales, flips, img_size = [float(v) for v in d["scales"]], [int(v) or None for v in d["flips"]], tuple(int(v) for v in d["img_size"])
    gp = [p.to(dev()) for p in preds]
    ranges = ops.tta_clip_ranges([p.shape[-1] for p in preds], 3)
    assert ranges == TR.clip_ranges([p.shape[-1] for p in preds], 3) == [(0, 240), (0, 252), (144, 189)]
    for a in ([20, 20, 20], [21, 84, 336], [8400, 5929, 3969], [252], [252, 189]):
        assert ops.tta_clip_ranges(a, 3) == TR.clip_ranges(a, 3), a
    got = ops.tta_merge(gp, scales, flips, img_size, ranges).cpu()
    _assert_merged(got, t(d["merged"]))
    _assert_merged(got, TR.tta_merge(preds, scales, flips, img_size))
    for i, (p, s, f) in enumerate(zip(gp, scales, flips)):  # one source, everything kept: _descale_pred
        _assert_merged(ops.tta_merge([p], [s], [f], img_size).cpu(), t(d[f"d{i}"]))
    # other orders, an empty range, per-pass image sizes
    got = ops.tta_merge([gp[2], gp[0]], [0.5, 2.0], [2, 3], [(96, 128), (50, 70)], [(7, 7), (3, 250)]).cpu()
    _assert_merged(got, TR.descale_pred(preds[0], 3, 2.0, (50, 70))[..., 3:250])
    for p, q in zip(gp, preds):
        assert torch.equal(p.cpu(), q), "the sources are left as they were"


# ---- predict(augment=True) and the validator ------------------------------------------------------------------------------------------
def _tta_model():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    d = load_golden("tta_tiny")
    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    model = DetectionModel(cfg, ch=3, nc=int(d["nc"]))
    missing = model.load_state_dict(TR.seeded_model_state(model.state_dict(), int(d["seed"])), strict=False)
    assert not missing.unexpected_keys
    return model.to(dev()).eval(), d


def _close(got, ref, what):
    """tests/test_gpu_modules_golden.py close() with F32_TOL: 1e-3 of the reference's magnitude"""
    got, ref = got.detach().float().cpu(), ref.float()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"[{what}] max abs err {err:.3e} at scale {scale:.4g} (bound {1e-3 * scale:.3e})")
    assert err <= 1e-3 * scale, what


def test_predict_augment_matches_the_reference_model():
    model, d = _tta_model()
    x = TR.to_unit(t(d["img"])).to(dev())
    with torch.no_grad():
        plain = model.predict(x)[0]
        y, none = model.predict(x, augment=True)
        y2, _ = model(x, augment=True)
    assert none is None and y.dtype == torch.float32
    assert tuple(y.shape) == tuple(d["y"].shape) == (2, 4 + int(d["nc"]), 240 + 252 + 45)
    _close(plain, t(d["y_plain"]), "plain eval decode")
    _close(y, t(d["y"]), "augmented eval decode")
    assert torch.equal(y, y2) and torch.equal(y[..., :240], plain[..., :240]), "the first pass is the plain prediction"
    # the reference's helper names, on their own
    ys = [plain.clone(), plain.clone(), plain[..., :189].clone()]
    _assert_merged(model._descale_pred(ys[1], 3, 0.83, x.shape[-2:]).cpu(), TR.descale_pred(plain.cpu(), 3, 0.83, tuple(x.shape[-2:])))
    clipped = model._clip_augmented(list(ys))
    assert [c.shape[-1] for c in clipped] == [240, 252, 45] and torch.equal(clipped[2], ys[2][..., 144:])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        yb, _ = model.predict(x, augment=True)
    assert yb.shape == y.shape and torch.isfinite(yb).all()
    model.train()
    with pytest.raises(RuntimeError):
        model.predict(x, augment=True)


def test_validator_with_augment_equals_nms_of_the_merged_predictions():
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch
    from improving_yolov8_cbam_swinblock_amd.engine.validator import DetectionValidator
    from test_gpu_validator import _expected, _raise_class_bias, _tiny_model

    import nms_exact as NX

    model = _tiny_model(3)
    batch = synthetic_batch(2, 256, dev(), 21)
    batch["cls"] = torch.arange(batch["cls"].numel(), device=dev()).float().reshape(-1, 1) % 3
    _raise_class_bias(model, batch["img"])
    v = DetectionValidator(model, augment=True)
    assert DetectionValidator(model).augment is False
    ys, post = [], v.postprocess
    v.postprocess = lambda preds: (ys.append(preds[0].detach().clone()), post(preds))[1]
    res = v(batch)
    # 256 -> 1344 anchors; 0.83 -> 212 in 224: 1029; 0.67 -> 171 in 192: 756; clipped 1344 - 64 and 756 - 36 * 16
    assert len(ys) == 1 and tuple(ys[0].shape) == (2, 7, 1280 + 1029 + 180)
    dets, want = _expected(ys, [batch], 0.001, 0.7, 300, 3)
    assert sum(len(x) for x in dets) > 0
    for got, x in zip(v.detections, dets):
        assert NX.same_bits(got, x), "detections differ from nms_exact on the merged predictions"
    for k, val in want.items():
        assert abs(float(res[k]) - float(val)) <= 1e-9, (k, res[k], val)


# ---- preprocess_batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRE_CASES)
def test_preprocess_batch_matches_the_reference(name):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import preprocess_batch
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    d = load_golden(f"tta_pre_{name}")
    u8, ref, k = t(d["img"]), t(d["out"]), int(d["seed"])
    imgsz, stride = int(d["imgsz"]), int(d["stride"])
    labels = {"batch_idx": torch.zeros(2), "cls": torch.zeros(2, 1), "bboxes": torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.3, 0.3, 0.1, 0.1]]), "max_boxes": 2}
    conv = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1).model[0].conv
    for where in ("host", "device"):
        batch = dict(labels, img=u8 if where == "host" else u8.to(dev()))
        if k >= 0:
            random.seed(k)
        out = preprocess_batch(batch, imgsz, stride, multi_scale=k >= 0)
        assert out is not batch and batch["img"].dtype == torch.uint8, "a new dict; the caller's batch is untouched"
        assert all(out[n] is labels[n] for n in labels), "labels are normalised coordinates: they pass through"
        img = out["img"]
        assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and tuple(img.shape) == tuple(ref.shape)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert _ops().first_conv_ok(img, conv, None, None), "layer 0 keeps its direct kernels"
        if tuple(ref.shape[2:]) == tuple(u8.shape[2:]):
            assert torch.equal(img.cpu(), ref), "no resize: exactly img.float() / 255"
        else:
            err = float((img.cpu() - ref).abs().max())
            print(f"[preprocess {name}, {where}] {tuple(u8.shape[2:])} -> {tuple(ref.shape[2:])}: max abs err vs reference {err:.2e} (bound {INTERP_TOL:.0e})")
            assert err <= INTERP_TOL
    # a float32 batch is taken as normalised already; an own generator instead of the module `random`
    xf = TR.to_unit(u8).to(dev())
    assert preprocess_batch({"img": xf}, imgsz, stride)["img"] is xf
    if k >= 0:
        out = preprocess_batch({"img": xf}, imgsz, stride, multi_scale=True, rng=random.Random(k))["img"]
        assert tuple(out.shape) == tuple(ref.shape) and float((out.cpu() - ref).abs().max()) <= INTERP_TOL


def test_multi_scale_sizes_follow_the_reference_for_the_same_seed():
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import preprocess_batch

    table = json.loads((GOLDEN / "tta_multiscale_sizes.json").read_text())
    imgs = {}
    for h, w, imgsz, stride, k, oh, ow in table[::3]:
        img = imgs.setdefault((h, w), torch.zeros(1, 1, h, w, dtype=torch.uint8, device=dev()))
        random.seed(k)
        assert tuple(preprocess_batch({"img": img}, imgsz, stride, multi_scale=True)["img"].shape[2:]) == (oh, ow), (h, w, k)


def _cbam_step(**kw):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    torch.manual_seed(0)
    model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=1).to(dev())
    return model, TrainStep(model, world_size=1, lr=0.01, **kw)


def test_step_on_a_preprocessed_uint8_batch_is_the_step_on_float_over_255():
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import preprocess_batch, synthetic_batch

    u8 = TR.seeded_u8(31, (2, 3, 64, 64))
    items = []
    for as_u8 in (True, False):
        _, step = _cbam_step()
        batch = synthetic_batch(2, 64, dev(), 5)
        batch["img"] = u8 if as_u8 else (u8.float() / 255).to(dev())
        if as_u8:
            batch = preprocess_batch(batch, 64, 32)
        items.append(step(batch).float().cpu())
    assert torch.isfinite(items[0]).all() and torch.equal(items[0], items[1]), items


# ---- TrainStep(image_shapes=N) --------------------------------------------------------------------------------------------------------
SIZES = (64, 96, 64, 96, 64)  # the larger shape comes second: every workspace grows after the first capture
PROBE = ("model.0.conv.weight", "model.9.ca.shared_MLP.0.weight", "model.9.sa.conv.weight", "model.19.cv2.bn.weight", "model.23.cv3.0.2.bias")
_eager_run = {}


def _run_sizes(graph):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch

    model, step = _cbam_step(graph=graph, **({"image_shapes": 2} if graph else {}))
    out = []
    for i, sz in enumerate(SIZES):
        batch = synthetic_batch(2, sz, dev(), 40 + i)
        junk = None
        if graph and i >= 1:  # eager allocations between the replays, alive across the next one: a graph that still addressed a released
            junk = [torch.full((n,), 7.0, device=dev()) for n in (1 << 18, 1 << 20, 1 << 22, 1 << 24)]  # buffer would write into these
            torch.cuda.synchronize()
        out.append(step(batch).float().cpu().clone())
        if junk is not None:
            assert all(bool((j == 7.0).all()) for j in junk), f"step {i} wrote memory it does not own"
            del junk
    sd = model.state_dict()
    return model, step, torch.stack(out), {k: sd[k].detach().float().cpu().clone() for k in PROBE}


def _eager_reference():
    if not _eager_run:
        _, step, losses, params = _run_sizes(False)
        _eager_run.update(losses=losses, params=params, updates=int(step.ema.updates))
    return _eager_run


@pytest.mark.parametrize("graph", [True, "split"], ids=["graph", "split"])
def test_shape_cache_replays_each_image_shape_and_applies_every_batch_once(graph):
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import synthetic_batch

    ref = _eager_reference()
    assert ref["updates"] == len(SIZES)
    model, step, losses, params = _run_sizes(graph)
    print(f"[{graph}] loss items per step\n{losses}\neager\n{ref['losses']}")
    assert torch.isfinite(losses).all()
    torch.testing.assert_close(losses, ref["losses"], rtol=2e-2, atol=2e-2)
    for k in PROBE:
        err = float((params[k] - ref["params"][k]).norm() / ref["params"][k].norm().clamp(min=1e-9))
        print(f"[{graph}] {k}: relative error {err:.2e}")
        assert err < 5e-3, (k, err)
    assert int(step.ema.updates) == len(SIZES) and int(step.opt._state.view(torch.int64)[2]) == len(SIZES), "every batch applied exactly once"
    assert sorted(step._shapes) == [(2, 3, 64, 64), (2, 3, 96, 96)]
    with pytest.raises(ValueError):  # a third shape
        step(synthetic_batch(2, 128, dev(), 50))
    with pytest.raises(ValueError):  # labels stay static: at a captured shape ...
        step(synthetic_batch(2, 64, dev(), 51, boxes_per_image=3))
    assert int(step.ema.updates) == len(SIZES)
    # ... and the refused batches changed nothing: the next one still replays
    assert torch.isfinite(step(synthetic_batch(2, 96, dev(), 52))).all() and int(step.ema.updates) == len(SIZES) + 1


def test_shape_cache_limits():
    from improving_yolov8_cbam_swinblock_amd.engine.trainer import TrainStep, synthetic_batch

    model, step = _cbam_step(graph=True)  # the default, image_shapes=1: one static shape, as before
    assert step.image_shapes == 1
    step(synthetic_batch(2, 64, dev(), 1))
    with pytest.raises(ValueError):
        step(synthetic_batch(2, 96, dev(), 2))
    with pytest.raises(ValueError):
        TrainStep(model, world_size=1, graph="tail", image_shapes=2)
    with pytest.raises(ValueError):
        TrainStep(model, world_size=1, graph=True, image_shapes=0)
    _, step = _cbam_step(graph=True, image_shapes=2)
    step(synthetic_batch(2, 64, dev(), 1))
    with pytest.raises(ValueError):  # a new image shape may not bring new label shapes
        step(synthetic_batch(2, 96, dev(), 2, boxes_per_image=3))
    assert sorted(step._shapes) == [(2, 3, 64, 64)] and int(step.ema.updates) == 1
