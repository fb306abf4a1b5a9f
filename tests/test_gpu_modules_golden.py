"""GPU parity: the HIP operator modules (through the C ABI) against the reference's own outputs
(tests/golden/*.npz, produced by the real reference) and against the CPU oracle on seeded inputs.

float32 runs are the parity gate (tolerance 1e-3, BASELINE.json north_star); bfloat16 runs check the
fast path against the same references with a bf16-sized tolerance written next to each assert.
"""
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN, LARGE_SWIN, golden_state, large_swin_grad_errors, load_golden, load_large_swin

pytestmark = pytest.mark.gpu

F32_TOL = dict(rtol=1e-3, atol=1e-3)  # north_star: within 1e-3 of the fp32 CPU reference
BF16_TOL = dict(rtol=6e-2, atol=6e-2)  # bf16 has 8 significant bits; several chained ops


def t(a):
    return torch.from_numpy(np.asarray(a))


def dev():
    return torch.device("cuda:0")


def P():
    import improving_yolov8_cbam_swinblock_amd.nn.modules as M

    return M


def set_bn(m):
    for b in m.modules():
        if isinstance(b, torch.nn.BatchNorm2d):
            b.eps, b.momentum = 1e-3, 0.03


def run(m, x, dtype):
    if dtype == torch.bfloat16:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return m(x)
    return m(x)


def close(a, b, tol, what=""):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert torch.isfinite(a).all(), f"{what}: non-finite output"
    assert err <= tol["atol"] * scale + tol["rtol"] * 0, f"{what}: max abs err {err:.3e} (scale {scale:.3g}) > {tol['atol'] * scale:.3e}"


def close_l2(a, b, rel, what=""):
    """relative L2 error: for bf16 runs of ops with arg-max routing (max-pool, CBAM) a single near-tie decided
    differently moves one element by O(1), which max-abs would flag although the tensor is right."""
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    assert a.shape == b.shape and torch.isfinite(a).all(), what
    err = float((a - b).norm() / b.norm().clamp(min=1e-6))
    assert err <= rel, f"{what}: relative L2 error {err:.3e} > {rel:.1e}"


def grads_of(y, inputs, gy):
    return torch.autograd.grad(y, inputs, gy.to(y.dtype) if gy.dtype != y.dtype else gy, allow_unused=True)


CASES = {
    "conv_3x3_s1": lambda M: M.Conv(8, 16, 3, 1),
    "conv_3x3_s2": lambda M: M.Conv(8, 16, 3, 2),
    "conv_3x3_s2_c3": lambda M: M.Conv(3, 16, 3, 2),
    "conv_1x1": lambda M: M.Conv(24, 16, 1, 1),
    "bottleneck_add": lambda M: M.Bottleneck(16, 16, True, 1, k=((3, 3), (3, 3)), e=1.0),
    "c2f_n2_shortcut": lambda M: M.C2f(16, 32, 2, True),
    "c2f_n1_noshortcut": lambda M: M.C2f(24, 16, 1, False),
    "sppf_k5": lambda M: M.SPPF(16, 16, 5),
    "sppf_k7": lambda M: M.SPPF(16, 24, 7),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv_family_vs_reference(name, dtype):
    d = load_golden(name)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    m = CASES[name](P())
    set_bn(m)
    m.load_state_dict(golden_state(d), strict=True)
    m = m.to(dev()).train()
    x = t(d["x"]).to(dev()).requires_grad_(True)
    y = run(m, x, dtype)
    close(y, t(d["y_train"]), tol, f"{name} train fwd")
    params = [p for p in m.parameters() if p.requires_grad]
    names = ["x"] + [n for n, p in m.named_parameters() if p.requires_grad]
    gs = grads_of(y, [x] + params, t(d["gy"]).to(dev()))
    gtol = dict(atol=tol["atol"] * 2, rtol=0)
    for n, g in zip(names, gs):
        assert g is not None, f"{name}: no gradient for {n}"
        close(g, t(d["g." + n]), gtol, f"{name} grad {n}")
    sd = m.state_dict()
    for k, v in golden_state(d, "after.").items():
        close(sd[k].float(), v.float(), tol, f"{name} running stat {k}")
    m.eval()
    with torch.no_grad():
        close(run(m, x.detach(), dtype), t(d["y_eval"]), tol, f"{name} eval fwd")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_conv_fused_eval(dtype):
    from improving_yolov8_cbam_swinblock_amd.utils.torch_utils import fuse_conv_and_bn

    d = load_golden("conv_fused_eval")
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    m = P().Conv(8, 16, 3, 1)
    set_bn(m)
    m.load_state_dict(golden_state(d), strict=True)
    m = m.to(dev()).eval()
    with torch.no_grad():
        m.conv = fuse_conv_and_bn(m.conv, m.bn)
        delattr(m, "bn")
        close(m.conv.weight, t(d["fused_weight"]), F32_TOL, "fused weight")
        y = run(m, t(d["x"]).to(dev()), dtype)
    close(y, t(d["y"]), tol, "fused eval conv")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,ctor_c", [("cbam_lazy_c32", None), ("cbam_c64", 64), ("cbam_lazy_c512", None)])
def test_cbam_vs_reference(name, ctor_c, dtype):
    d = load_golden(name)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    M = P()
    m = M.CBAM(ctor_c) if ctor_c else M.CBAM()
    if m.ca.shared_MLP is None:
        m.ca.create_mlp(d["x"].shape[1])
    m.load_state_dict(golden_state(d), strict=True)
    m = m.to(dev())
    x = t(d["x"]).to(dev()).requires_grad_(True)
    y = run(m, x, dtype)
    close(y, t(d["y"]), tol, f"{name} fwd")
    names = ["x"] + [n for n, _ in m.named_parameters()]
    gs = grads_of(y, [x] + list(m.parameters()), t(d["gy"]).to(dev()))
    for n, g in zip(names, gs):
        assert g is not None, n
        if dtype == torch.float32:
            close(g, t(d["g." + n]), dict(atol=tol["atol"] * 2, rtol=0), f"{name} grad {n}")
        else:
            close_l2(g, t(d["g." + n]), 0.08, f"{name} grad {n}")


def test_cbam_lazy_creates_mlp_on_device():
    d = load_golden("cbam_lazy_c32")
    m = P().CBAM().to(dev())
    x = t(d["x"]).to(dev())
    y = m(x)
    assert m.ca.shared_MLP[0].weight.is_cuda and m.ca.shared_MLP[0].weight.shape == (2, 32, 1, 1)  # 32 // 16 = 2 (lazy rule)
    assert y.shape == x.shape


@pytest.mark.parametrize("hw", ["42x42", "84x84", "14x21"])
def test_window_index_bit_exact(hw):
    from improving_yolov8_cbam_swinblock_amd import ops

    d = load_golden(f"window_index_{hw}_ws7")
    B, H, W, ws = (int(v) for v in d["shape"])
    idx = ops.window_partition_index(B, H, W, ws, dev()).cpu().numpy()
    assert np.array_equal(idx.reshape(d["partition"].shape), d["partition"])
    # partition / reverse as data movement: exact round trip and exact agreement with the index map
    M = P()
    x = torch.arange(B * H * W * 8, dtype=torch.float32, device=dev()).view(B, H, W, 8)
    win = M.window_partition(x, ws)
    ref = x.view(B * H * W, 8)[torch.from_numpy(d["partition"].astype(np.int64)).to(dev()).view(-1)].view(win.shape)
    assert torch.equal(win, ref)
    assert torch.equal(M.window_reverse(win, ws, H, W).contiguous(), x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["swin_d32_7x7", "swin_d32_10x10", "swin_d64_14x21", "swin_d64_h4_20x20"])
def test_swin_block_vs_reference(name, dtype):
    d = load_golden(name)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    dim = d["x"].shape[1]
    m = P().SwinBlock(dim, int(d["heads"]))
    m.load_state_dict(golden_state(d), strict=True)
    m = m.to(dev())
    x = t(d["x"]).to(dev()).requires_grad_(True)
    y = run(m, x, dtype)
    close(y, t(d["y"]), tol, f"{name} fwd")
    names = ["x"] + [n for n, _ in m.named_parameters()]
    gs = grads_of(y, [x] + list(m.parameters()), t(d["gy"]).to(dev()))
    for n, g in zip(names, gs):
        assert g is not None, n
        close(g, t(d["g." + n]), dict(atol=tol["atol"] * 3, rtol=0), f"{name} grad {n}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", LARGE_SWIN)
def test_swin_block_head_dim_192_and_large_windows_vs_reference(name, dtype):
    """reference swin_block.py:23-58 at config 5's SwinBlock(384, 2) (head_dim 192) and with 14x14 windows (196 tokens >
    one 64-token tile): forward, input gradient and every parameter gradient.  float32: 1e-3 (north_star); bfloat16:
    6e-2 scaled max-abs forward, 5e-2 relative L2 on gradients."""
    m, x, gy, d, seeded = load_large_swin(name, lambda dim, heads, ws: P().SwinBlock(dim, heads, ws))
    m = m.to(dev())
    x = x.to(dev()).requires_grad_(True)
    y = run(m, x, dtype)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    close(y, t(d["y"]), tol, f"{name} fwd")
    gs = grads_of(y, [x] + list(m.parameters()), gy.to(dev()))
    if dtype == torch.float32:
        close(gs[0], t(d["g.x"]), dict(atol=3e-3, rtol=0), f"{name} grad x")
    else:
        close_l2(gs[0], t(d["g.x"]), 5e-2, f"{name} grad x")
    for n, emax, erel in large_swin_grad_errors(d, seeded, [k for k, _ in m.named_parameters()], gs[1:]):
        if dtype == torch.float32:
            assert emax <= 3e-3 or erel <= 1e-3, (n, emax, erel)
        else:
            assert erel <= 5e-2 or emax <= 2e-2, (n, emax, erel)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_detect_vs_reference(dtype):
    d = load_golden("detect_nc3")
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    det = P().Detect(3, [16, 32, 64])
    det.stride = torch.tensor([8.0, 16.0, 32.0])
    set_bn(det)
    det.load_state_dict(golden_state(d), strict=True)
    det = det.to(dev())
    det.stride = det.stride.to(dev())
    xs = [t(d[f"x{i}"]).to(dev()) for i in range(3)]
    det.train()
    for i, y in enumerate(run(det, [v.clone() for v in xs], dtype)):
        close(y, t(d[f"y_train{i}"]), tol, f"detect train level {i}")
    det.eval()
    with torch.no_grad():
        ye, _ = run(det, [v.clone() for v in xs], dtype)
    # decoded boxes are in pixels (up to ~300): compare relative to magnitude
    close(ye, t(d["y_eval"]), dict(atol=tol["atol"] * (1 if dtype == torch.float32 else 2), rtol=0), "detect eval decode")


def _tiny():
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    d = load_golden("e2e_tiny_seed7")
    model = DetectionModel(cfg, ch=3, nc=1)
    missing = model.load_state_dict(golden_state(d), strict=True)
    return model.to(dev()), d


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_e2e_tiny_model_vs_reference(dtype):
    model, d = _tiny()
    tol = F32_TOL if dtype == torch.float32 else dict(atol=0.15, rtol=0)  # 27 layers of bf16 + train-mode BN on 2 images
    img = t(d["img"]).to(dev())
    batch = {"img": img, "batch_idx": t(d["batch_idx"]).to(dev()), "cls": t(d["cls"]).to(dev()), "bboxes": t(d["bboxes"]).to(dev())}
    model.train()
    preds = run(model, img, dtype)
    for i, p in enumerate(preds):
        if dtype == torch.float32:
            close(p, t(d[f"pred{i}"]), tol, f"e2e pred level {i}")
        else:  # 27 bf16 layers with train-mode BN over 2 images (8 values per channel at P5): compare in norm
            # (level 2 is a 2x2 map: its BatchNorms normalise over 8 values, which amplifies bf16 rounding)
            close_l2(p, t(d[f"pred{i}"]), 0.12 if i < 2 else 0.35, f"e2e pred level {i}")
    loss, items = model.criterion(preds, batch) if getattr(model, "criterion", None) else model.init_criterion()(preds, batch)
    ltol = 2e-3 if dtype == torch.float32 else 0.1
    assert torch.allclose(loss.float().cpu(), t(d["loss"]), rtol=ltol, atol=ltol), (loss, d["loss"])
    loss.sum().backward()
    ref = json.loads((GOLDEN / "e2e_tiny_seed7_gradnorms.json").read_text())
    got = {n: float(p.grad.float().norm()) for n, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(ref), set(got) ^ set(ref)
    if dtype == torch.float32:
        bad = {n: (got[n], v) for n, v in ref.items() if abs(got[n] - v) > 2e-2 * max(abs(v), 1e-2) + 1e-4}
        assert not bad, bad
    model.eval()
    with torch.no_grad():
        ye, _ = run(model, img, dtype)
    if dtype == torch.float32:
        close(ye, t(d["y_eval"]), dict(atol=tol["atol"], rtol=0), "e2e eval decode")
    else:
        close_l2(ye, t(d["y_eval"]), 0.05, "e2e eval decode")


def test_loss_matches_reference_on_fixed_predictions():
    model, _ = _tiny()
    d = load_golden("loss_crowded")
    preds = [t(d[f"pred{i}"]).to(dev()).requires_grad_(True) for i in range(3)]
    batch = {"batch_idx": t(d["batch_idx"]).to(dev()), "cls": t(d["cls"]).to(dev()), "bboxes": t(d["bboxes"]).to(dev())}
    loss, items = model.init_criterion()(preds, batch)
    assert torch.allclose(loss.cpu(), t(d["loss"]), rtol=1e-4, atol=1e-4), (loss, d["loss"])
    loss.sum().backward()
    for i, p in enumerate(preds):
        assert torch.allclose(p.grad.cpu(), t(d[f"g.pred{i}"]), rtol=1e-3, atol=1e-5)


def test_stride_probe_side_effects_match_the_reference():
    """the reference's constructor measures strides with a train-mode forward of zeros(1, ch, 256, 256) (tasks.py:351-364), which
    moves every BatchNorm's running statistics (with nn.BatchNorm2d's default eps / momentum: initialize_weights runs after it) and
    sets num_batches_tracked = 1; fixture e2e_tiny_seed7 is the state_dict of such a freshly constructed reference model.  Here
    construction touches no buffer; DetectionModel.stride_probe() reproduces the side effects on the GPU: same buffers (the layers
    behind the first SwinBlock see non-zero activations - its Linear biases - so this is a numeric check, not 0.9 everywhere),
    same counts, and the strides the graph gave."""
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    sd = golden_state(load_golden("e2e_tiny_seed7"))
    model = DetectionModel(cfg, ch=3, nc=1)
    is_buf = lambda k: k.endswith(("running_mean", "running_var", "num_batches_tracked"))
    fresh = {k: v.clone() for k, v in model.state_dict().items() if is_buf(k)}
    assert all(float(v.float().abs().max()) == (1.0 if k.endswith("running_var") else 0.0) for k, v in fresh.items())  # untouched by construction
    model.load_state_dict(sd, strict=True)      # the reference's weights ...
    model.load_state_dict(fresh, strict=False)  # ... with a freshly built model's buffers
    model = model.to(dev())
    with pytest.raises(RuntimeError, match="no CPU path"):
        DetectionModel(cfg, ch=3, nc=1).stride_probe()
    strides = model.stride_probe()
    assert torch.equal(strides, model.stride.cpu().float())
    assert model.training and model.model[0].bn.eps == 1e-3 and model.model[0].bn.momentum == 0.03  # restored
    moved = 0
    for k, v in model.state_dict().items():
        if not is_buf(k):
            continue
        ref = sd[k]
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(ref) == 1, k
        else:
            assert float((v.cpu() - ref).abs().max()) <= 2e-5, (k, float((v.cpu() - ref).abs().max()))
            moved += int(float((ref - (1.0 if k.endswith("running_var") else 0.0)).abs().max()) > 1e-3 and abs(float(ref.reshape(-1)[0]) - 0.9) > 1e-4)
    assert moved > 10  # the check is not vacuous: many layers have data-dependent statistics


def _oracle_crit(nc):
    from oracle.loss import v8DetectionLoss as OracleLoss
    from oracle.tasks import DetectionModel as OracleModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    return OracleLoss(OracleModel(cfg, ch=3, nc=nc))


def _product_crit(nc):
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    cfg = json.loads((GOLDEN / "e2e_tiny_seed7_yaml.json").read_text())
    return DetectionModel(cfg, ch=3, nc=nc).to(dev()).init_criterion()


@pytest.mark.parametrize("nc", [1, 5, 80], ids=["nc1", "nc5", "nc80"])
@pytest.mark.parametrize("nb", [0, 1, 7, 40], ids=["empty", "one", "seven", "crowded"])
def test_hip_loss_vs_oracle_random_batches(nb, nc):
    """HIP loss (csrc/loss.hip) against the CPU oracle on random predictions: empty batch, images without labels,
    several gts claiming one anchor; losses and gradients with respect to the prediction maps (f32)."""
    crit, ocrit = _product_crit(nc), _oracle_crit(nc)
    g = torch.Generator().manual_seed(3 + nb)
    preds = [torch.randn(3, 64 + nc, s, s, generator=g) for s in (8, 4, 2)]
    bi = torch.randint(0, 3, (nb,), generator=g).float()
    boxes = torch.cat((torch.rand(nb, 2, generator=g) * 0.6 + 0.2, torch.rand(nb, 2, generator=g) * 0.4 + 0.05), 1)
    cls = torch.randint(0, nc, (nb, 1), generator=g).float()
    batch = {"batch_idx": bi, "cls": cls, "bboxes": boxes}
    pg = [p.clone().to(dev()).requires_grad_(True) for p in preds]
    po = [p.clone().requires_grad_(True) for p in preds]
    a, ia = crit(pg, {k: v.to(dev()) for k, v in batch.items()})
    b, ib = ocrit(po, batch)
    torch.testing.assert_close(a.cpu(), b, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(ia.cpu(), ib, rtol=2e-4, atol=2e-5)
    a.sum().backward()
    b.sum().backward()
    for x, y in zip(pg, po):
        torch.testing.assert_close(x.grad.cpu(), y.grad, rtol=2e-3, atol=2e-5)


def test_hip_loss_vs_oracle_topk_row_in_memory():
    """12,096 anchors (96 / 48 / 24 maps): more than the 10,240 metric values a top-k workgroup keeps in registers, so every selection
    round scans the gt's row in memory (the path of 1280 x 1280 images).  Every gt has at least 156 anchors of positive metric and the
    eleven largest metrics of a gt are at least 5.6e-4 apart relatively, so the selected set depends neither on tie order nor on
    rounding; comparison and tolerances as in test_hip_loss_vs_oracle_random_batches."""
    crit, ocrit = _product_crit(3), _oracle_crit(3)
    g = torch.Generator().manual_seed(22)
    preds = [torch.randn(2, 67, s, s, generator=g) for s in (96, 48, 24)]
    counts = [7, 3]  # labels per image
    n = sum(counts)
    bi = torch.cat([torch.full((c,), float(i)) for i, c in enumerate(counts)])
    boxes = torch.cat((torch.rand(n, 2, generator=g) * 0.6 + 0.2, torch.rand(n, 2, generator=g) * 0.3 + 0.05), 1)
    cls = torch.randint(0, 3, (n, 1), generator=g).float()
    batch = {"batch_idx": bi, "cls": cls, "bboxes": boxes}
    pg = [p.clone().to(dev()).requires_grad_(True) for p in preds]
    po = [p.clone().requires_grad_(True) for p in preds]
    a, ia = crit(pg, {k: v.to(dev()) for k, v in batch.items()})
    b, ib = ocrit(po, batch)
    torch.testing.assert_close(a.cpu(), b, rtol=2e-4, atol=2e-5)
    torch.testing.assert_close(ia.cpu(), ib, rtol=2e-4, atol=2e-5)
    a.sum().backward()
    b.sum().backward()
    for x, y in zip(pg, po):
        torch.testing.assert_close(x.grad.cpu(), y.grad, rtol=2e-3, atol=2e-5)


def test_hip_loss_bf16_maps_and_max_boxes_hint():
    """bf16 maps (the training dtype): same loss as on the f32 copy of the same bf16 values; a max_boxes hint larger
    than needed changes nothing (the extra slots are padding rows)."""
    crit, ocrit = _product_crit(1), _oracle_crit(1)
    g = torch.Generator().manual_seed(11)
    preds = [torch.randn(2, 65, s, s, generator=g).bfloat16() for s in (8, 4, 2)]
    bi = torch.tensor([0.0, 0.0, 1.0, 1.0, 1.0])
    boxes = torch.cat((torch.rand(5, 2, generator=g) * 0.6 + 0.2, torch.rand(5, 2, generator=g) * 0.4 + 0.05), 1)
    batch = {"batch_idx": bi, "cls": torch.zeros(5, 1), "bboxes": boxes}
    dbatch = {k: v.to(dev()) for k, v in batch.items()}
    pg = [p.clone().to(dev()).requires_grad_(True) for p in preds]
    po = [p.float().requires_grad_(True) for p in preds]
    a, _ = crit(pg, dict(dbatch, max_boxes=9))
    b, _ = ocrit(po, batch)
    torch.testing.assert_close(a.cpu(), b, rtol=2e-4, atol=2e-5)
    a.sum().backward()
    b.sum().backward()
    for x, y in zip(pg, po):  # gradients are rounded to bf16 on store
        close_l2(x.grad, y.grad, 5e-3, "bf16 loss gradient")
    a2, _ = crit([p.clone().to(dev()) for p in preds], dbatch)
    torch.testing.assert_close(a2, a.detach(), rtol=1e-6, atol=1e-7)


def test_weight_arena_pack_equals_per_call_pack():
    """the one-launch batched pack (ymi_pack_conv_weights_batch) writes exactly the operands the per-layer pack
    functions write: forward [O][tap][Ipad] and data-gradient [I][tap in class][Opad], stride 1 and 2, 1x1 and 3x3,
    with channel padding on both sides."""
    from improving_yolov8_cbam_swinblock_amd import ops

    torch.manual_seed(3)
    # (o, i, k, stride, ipad, opad); the data-gradient operand is transposed through LDS in 32 x 32 channel tiles: partial tiles on both axes
    cases = [(24, 13, 3, 2, 16, 24), (64, 64, 3, 1, 64, 64), (40, 32, 1, 1, 32, 40), (7, 8, 3, 2, 8, 8), (96, 40, 3, 1, 40, 96),
             (130, 70, 1, 1, 72, 136), (256, 128, 3, 2, 128, 256), (1, 64, 1, 1, 64, 8)]
    for dt in (torch.bfloat16, torch.float32):
        arena = ops.WeightArena()
        ops.RUN.arena = arena
        try:
            ws, ref = [], []
            for o, i, k, s, ipad, opad in cases:
                w = torch.randn(o, i, k, k, device=dev())
                ws.append(w)
                ref.append((ops.pack_conv_fwd(w, ipad, dt).clone(), ops.pack_conv_dgrad(w, opad, s, dt).clone()))  # recorded + per-call pack
            arena.build()
            arena.pack()
            for w, (o, i, k, s, ipad, opad), (rf, rd) in zip(ws, cases, ref):
                f = arena.lookup_fwd(w, ipad, dt)
                d = arena.lookup_dgrad(w, opad, s, dt)
                assert f is not None and d is not None
                assert torch.equal(f, rf), ("fwd", o, i, k, s)
                assert torch.equal(d, rd), ("dgrad", o, i, k, s)
        finally:
            ops.RUN.arena = None
