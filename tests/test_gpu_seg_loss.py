"""v8SegmentationLoss on the GPU (csrc/seg.hip behind the detection loss of csrc/loss.hip) on the cases of tests/seg_common.py: the four loss
items and every input gradient against the reference's (tests/golden/seg_loss_*.npz) and against the float64 restatement (tests/seg_ref.py);
box, cls and dfl bit-equal to v8DetectionLoss on the same maps; two runs bit-equal; the no-foreground batch exactly zero and finite.

Tolerances.  Loss items: the loss bound of test_gpu_yolo11_e2e.py (2e-3), as every loss test here; the kernel's own distance from the float64
restatement is printed per case (1e-8 .. 2e-7 relative when this was written).  Gradients of the mask term are small numbers (max |g| 0.02 ..
0.08 on these cases), so they are held RELATIVE to the reference's largest element, with no floor (rel_close):
  float32   1.4e-6: the float32 reference's own gradients lie within 3.4e-7 of the float64 restatement's on every fixture (max-abs over max
            |g|, 1.7e-7 .. 3.4e-7 per tensor; tests/test_seg_cpu.py prints and asserts it), times 4 for another summation order.  Against the
            reference fixture and against float64.
  bfloat16  2^-8 + the float32 bound: the kernels read the bf16 maps as they are and sum in float32, so against the float64 restatement fed the
            SAME bf16-rounded operands and the kernel's own assignment the only error beyond float32's is the ONE rounding of each stored
            gradient element: half a unit in the last of bf16's 8 significant bits, at most 2^-8 of the element's own size, hence of the
            largest element's (seen: 2.0e-3 .. 3.3e-3).
The gradients of the box / class maps are the detection kernels' own, bit for bit (asserted), and keep twice F32_TOL against the reference."""
from types import SimpleNamespace

import pytest
import torch

import seg_ref
from conftest import load_golden
from seg_common import HYP, LOSS_CASES, NC, NM, NPR, CH, STRIDE, loss_case
from test_gpu_modules_golden import F32_TOL, P, close, dev, t

pytestmark = pytest.mark.gpu


def _criteria():
    """(v8SegmentationLoss, v8DetectionLoss) for a Segment(3, 32, 32, (32, 64, 128)) with strides 8, 16, 32"""
    from improving_yolov8_cbam_swinblock_amd.utils.loss import v8DetectionLoss, v8SegmentationLoss

    head = P().Segment(NC, NM, NPR, CH)
    head.stride = torch.tensor(STRIDE)
    holder = torch.nn.Module()
    holder.model = torch.nn.ModuleList([head])
    holder.args = SimpleNamespace(**HYP)
    holder = holder.to(dev())
    return v8SegmentationLoss(holder), v8DetectionLoss(holder)


def _inputs(name, dtype, mask_dtype=torch.uint8):
    feats, mc, proto, batch = loss_case(name, mask_dtype)
    leaves = [x.to(dev()).to(dtype).requires_grad_(True) for x in feats + [mc, proto]]
    batch = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in batch.items()}
    return leaves, batch


F32_GRAD_REL = 1.4e-6
BF16_GRAD_REL = 2.0 ** -8 + F32_GRAD_REL


def rel_close(a, b, rel, what):
    """max |a - b| <= rel * max |b|: no floor of 1, so small gradients are really compared"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all(), what
    err, scale = float((a - b).abs().max()), float(b.abs().max())
    print(f"  {what}: max abs err {err:.3e} / max |ref| {scale:.3e} = {err / max(scale, 1e-300):.2e} (bound {rel:.1e})")
    assert err <= rel * scale, f"{what}: max abs err {err:.3e} > {rel:.1e} * {scale:.3e}"


def _run(crit, leaves, batch):
    loss, items = crit((leaves[:3], leaves[3], leaves[4]), batch)
    grads = torch.autograd.grad(loss.sum(), leaves, allow_unused=True)
    return loss.detach(), items, [g if g is not None else torch.zeros_like(x) for g, x in zip(grads, leaves)]


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.float32], ids=["u8", "f32mask"])
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_loss_items_and_gradients_vs_reference(name, mask_dtype):
    seg, det = _criteria()
    d = load_golden(name)
    leaves, batch = _inputs(name, torch.float32, mask_dtype)
    loss, items, grads = _run(seg, leaves, batch)
    print(f"[{name}] items {items.cpu().tolist()} reference {d['items'].tolist()}")
    assert torch.allclose(items.cpu(), t(d["items"]), rtol=2e-3, atol=2e-3), (items, d["items"])
    assert torch.allclose(loss.cpu(), t(d["loss"]), rtol=2e-3, atol=2e-3)
    gtol = dict(atol=2 * F32_TOL["atol"], rtol=0)
    for n, g in zip(["f0", "f1", "f2"], grads):
        close(g, t(d["g." + n]), gtol, f"{name} grad {n}")
    rel_close(grads[3], t(d["g.mc"]), F32_GRAD_REL, f"{name} grad mc against the reference")
    rel_close(grads[4], t(d["g.proto"]), F32_GRAD_REL, f"{name} grad proto against the reference")
    # the float64 restatement on the reference's assignment
    img_hw = LOSS_CASES[name][0]
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in batch.items()}
    mc64, p64 = leaves[3].detach().cpu().double().requires_grad_(True), leaves[4].detach().cpu().double().requires_grad_(True)
    ref = seg_ref.mask_loss(mc64, p64, t(d["gidx"]).long(), seg_ref.dense_targets(cpu, 2, img_hw), cpu["masks"], img_hw)
    got = float(items[1]) / HYP["box"]
    print(f"[{name}] seg {got:.9f} float64 restatement {float(ref.detach()):.9f} relative distance {abs(got - float(ref.detach())) / max(float(ref.detach()), 1e-12):.2e}")
    assert abs(got - float(ref.detach())) <= 2e-3 * max(1.0, float(ref.detach()))
    gmc, gp = torch.autograd.grad(ref * HYP["box"] * 2, [mc64, p64])
    rel_close(grads[3], gmc, F32_GRAD_REL, f"{name} grad mc against float64")
    rel_close(grads[4], gp, F32_GRAD_REL, f"{name} grad proto against float64")
    # background anchors receive exactly zero
    bg = (t(d["gidx"]) < 0).to(dev())
    assert not grads[3].permute(0, 2, 1)[bg].any()
    # box, cls, dfl: the detection criterion's numbers on the same maps, bit for bit - items, loss and gradients
    dl, di = det(leaves[:3], batch)
    assert torch.equal(items[[0, 2, 3]], di) and torch.equal(loss[[0, 2, 3]], dl.detach())
    dg = torch.autograd.grad(dl.sum(), leaves[:3])
    for a, b in zip(grads[:3], dg):
        assert torch.equal(a, b)
    if name == "seg_loss_nofg":
        assert float(items[1]) == 0.0 and float(loss[1]) == 0.0
        assert not grads[3].any() and not grads[4].any() and all(torch.isfinite(g).all() for g in grads)


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_two_runs_are_bit_equal(name):
    seg, _ = _criteria()
    outs = []
    for _ in range(2):
        leaves, batch = _inputs(name, torch.float32)
        outs.append(_run(seg, leaves, batch))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    for a, b in zip(outs[0][2], outs[1][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_bf16_maps_against_the_restatement_on_the_same_operands(name):
    from improving_yolov8_cbam_swinblock_amd import ops

    seg, det = _criteria()
    leaves, batch = _inputs(name, torch.bfloat16)
    loss, items, grads = _run(seg, leaves, batch)
    assert all(torch.isfinite(g.float()).all() for g in grads) and torch.isfinite(items).all()
    dl, di = det(leaves[:3], batch)
    assert torch.equal(items[[0, 2, 3]], di)
    # the assignment the kernels made on these bf16 maps
    img_hw = LOSS_CASES[name][0]
    box = [f.detach()[:, :64].contiguous(memory_format=torch.channels_last) for f in leaves[:3]]
    cls = [f.detach()[:, 64:].contiguous(memory_format=torch.channels_last) for f in leaves[:3]]
    targets = ops.detect_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], 2, batch["max_boxes"], img_hw[1], img_hw[0], dev())
    scale = torch.tensor([7.5 * 2, 0.5 * 2, 1.5 * 2, 7.5, 0.5, 1.5], device=dev())
    _, _, gidx = ops.detect_loss_assign(box, cls, list(STRIDE), targets, scale)
    cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in batch.items()}
    mc64, p64 = leaves[3].detach().cpu().double().requires_grad_(True), leaves[4].detach().cpu().double().requires_grad_(True)
    ref = seg_ref.mask_loss(mc64, p64, gidx.cpu().long(), seg_ref.dense_targets(cpu, 2, img_hw), cpu["masks"], img_hw)
    got = float(items[1]) / HYP["box"]
    print(f"[{name} bf16] seg {got:.9f} float64 restatement on the bf16 operands {float(ref.detach()):.9f}")
    assert abs(got - float(ref.detach())) <= 2e-3 * max(1.0, float(ref.detach()))  # (the logit is not rounded: float32 bound)
    if int((gidx >= 0).sum()):
        gmc, gp = torch.autograd.grad(ref * HYP["box"] * 2, [mc64, p64])
        assert grads[3].dtype == torch.bfloat16 and grads[4].dtype == torch.bfloat16
        rel_close(grads[3], gmc, BF16_GRAD_REL, f"{name} bf16 grad mc")
        rel_close(grads[4], gp, BF16_GRAD_REL, f"{name} bf16 grad proto")
        assert not grads[3].permute(0, 2, 1)[gidx < 0].any()
    else:
        assert float(items[1]) == 0.0 and not grads[3].any() and not grads[4].any()


def test_split_predictions_give_the_same_numbers():
    """SegPreds (NHWC maps as the convolutions write them) against the reference layout (feats, mc [B, nm, A], p): same bits."""
    from improving_yolov8_cbam_swinblock_amd.nn.modules import SegPreds

    seg, _ = _criteria()
    leaves, batch = _inputs("seg_loss_base", torch.float32)
    loss, items, grads = _run(seg, leaves, batch)
    hws = [f.shape[2:] for f in leaves[:3]]
    cl = lambda x: x.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    box = [cl(f[:, :64]) for f in leaves[:3]]
    cls = [cl(f[:, 64:]) for f in leaves[:3]]
    mcs = [cl(m.reshape(2, NM, *hw)) for m, hw in zip(leaves[3].split([h * w for h, w in hws], 2), hws)]
    proto = cl(leaves[4])
    l2, i2 = seg(SegPreds(box, cls, mcs, proto), batch)
    assert torch.equal(l2.detach(), loss) and torch.equal(i2, items)
    gm = torch.autograd.grad(l2.sum(), mcs + [proto])
    assert torch.equal(torch.cat([g.reshape(2, NM, -1) for g in gm[:3]], 2), grads[3]) and torch.equal(gm[3], grads[4])


def test_overlap_mask_false_is_refused():
    from improving_yolov8_cbam_swinblock_amd.utils.loss import v8SegmentationLoss

    head = P().Segment(NC, NM, NPR, CH)
    head.stride = torch.tensor(STRIDE)
    holder = torch.nn.Module()
    holder.model = torch.nn.ModuleList([head])
    holder.args = SimpleNamespace(**{**HYP, "overlap_mask": False})
    with pytest.raises(NotImplementedError, match="loss.py:427-428"):
        v8SegmentationLoss(holder.to(dev()))
