"""C3k / C3k2, Attention / PSABlock / C2PSA and the non-legacy Detect head on the GPU against the reference's own outputs (tests/golden/psa_*.npz,
written by tests/golden/make_psa_golden.py), as test_gpu_ghost_modules.py::test_ghost_family_vs_reference holds the ghost family: train forward,
gradients of x and of every parameter at twice the forward tolerance, running statistics, eval forward, eval forward after fuse().  The bounds
are test_gpu_modules_golden's F32_TOL / BF16_TOL - the project's contract with the reference.  Seeded cases (tests/psa_common.py) rebuild weights
and inputs from their seed and compare parameter gradients on the stored elements (all, or a strided sample and the norm)."""
import pytest
import torch

from conftest import golden_state, load_golden, same_elements, stored_elements
from psa_common import (CASES, DETECT_CASE, DETECT_CH, DETECT_NC, DETECT_SEED, DETECT_STRIDE, build, case_inputs, case_seed, detect_inputs, is_seeded,
                        seeded_module_state)
from test_gpu_modules_golden import BF16_TOL, F32_TOL, P, close, dev, grads_of, run, set_bn, t

pytestmark = pytest.mark.gpu


def _fuse(m):
    from improving_yolov8_cbam_swinblock_amd.utils.torch_utils import fuse_conv_and_bn

    for sub in m.modules():  # BaseModel.fuse
        if isinstance(sub, P().Conv) and hasattr(sub, "bn"):
            sub.conv = fuse_conv_and_bn(sub.conv, sub.bn)
            delattr(sub, "bn")
            sub.forward = sub.forward_fuse


def _close_param_grads(d, names, grads, gtol, what):
    """parameter gradients against whole arrays (g.<name>) or grad_record entries (gfull.<name> | gsample.<name> + gnorm.<name>)"""
    for n, g in zip(names, grads):
        assert g is not None, f"{what}: no gradient for {n}"
        if "g." + n in d:
            close(g, t(d["g." + n]), gtol, f"{what} grad {n}")
            continue
        close(same_elements(g), stored_elements("g", d, n), gtol, f"{what} grad {n} (stored elements)")
        if f"gnorm.{n}" in d:
            ref = float(d[f"gnorm.{n}"])
            got = float(g.detach().double().norm())
            assert abs(got - ref) <= gtol["atol"] * max(1.0, ref), f"{what} grad {n}: norm {got} against {ref}"


def _module(name):
    d = load_golden(name)
    m = build(P(), name)
    set_bn(m)
    if is_seeded(m):
        m.load_state_dict(seeded_module_state(m, case_seed(name)), strict=True)
        x, gy = case_inputs(name, d["y_train"].shape[1])
    else:
        m.load_state_dict(golden_state(d), strict=True)
        x, gy = t(d["x"]), t(d["gy"])
    return m.to(dev()), d, x, gy


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_psa_family_vs_reference(name, dtype):
    m, d, x, gy = _module(name)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    m.train()
    x = x.to(dev()).requires_grad_(True)
    y = run(m, x, dtype)
    close(y, t(d["y_train"]), tol, f"{name} train fwd")
    params = [p for p in m.parameters() if p.requires_grad]
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    gs = grads_of(y, [x] + params, gy.to(dev()))
    gtol = dict(atol=tol["atol"] * 2, rtol=0)
    assert gs[0] is not None
    close(gs[0], t(d["g.x"]), gtol, f"{name} grad x")
    _close_param_grads(d, names, gs[1:], gtol, name)
    sd = m.state_dict()
    for k, v in golden_state(d, "after.").items():
        close(sd[k].float(), v.float(), tol, f"{name} running stat {k}")
    m.eval()
    with torch.no_grad():
        close(run(m, x.detach(), dtype), t(d["y_eval"]), tol, f"{name} eval fwd")
        _fuse(m)
        close(run(m, x.detach(), dtype), t(d["y_fused"]), tol, f"{name} eval fwd after fuse")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_nonlegacy_detect_vs_reference(dtype):
    """Detect(3, (32, 64, 128)) with the depthwise class branch: train maps, gradients of the three inputs and of every parameter, running
    statistics, the decoded eval output before and after fuse()."""
    M = P()
    M.Detect.legacy = False
    try:
        m = M.Detect(DETECT_NC, DETECT_CH)
    finally:
        M.Detect.legacy = True
    assert m.legacy is False and not m.pair_ok
    set_bn(m)
    m.stride = torch.tensor(DETECT_STRIDE)
    m.load_state_dict(seeded_module_state(m, DETECT_SEED), strict=True)
    m = m.to(dev())
    m.stride = m.stride.to(dev())
    d = load_golden(DETECT_CASE)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    gtol = dict(atol=tol["atol"] * 2, rtol=0)
    xs, gys = detect_inputs(m.no)
    xs = [x.to(dev()).requires_grad_(True) for x in xs]
    m.train()
    maps = run(m, list(xs), dtype)
    for i, y in enumerate(maps):
        close(y, t(d[f"y_train{i}"]), tol, f"detect train map {i}")
    params = [p for p in m.parameters() if p.requires_grad]
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    gs = torch.autograd.grad(maps, xs + params, [g.to(dev()).to(y.dtype) for g, y in zip(gys, maps)], allow_unused=True)
    for i in range(len(xs)):
        close(gs[i], t(d[f"g.x{i}"]), gtol, f"detect grad x{i}")
    _close_param_grads(d, names, gs[len(xs):], gtol, "detect")
    sd = m.state_dict()
    for k, v in golden_state(d, "after.").items():
        close(sd[k].float(), v.float(), tol, f"detect running stat {k}")
    m.eval()
    with torch.no_grad():
        y, maps_eval = run(m, [x.detach() for x in xs], dtype)
        close(y, t(d["y_eval"]), tol, "detect decoded eval output")
        for i, mp in enumerate(maps_eval):
            close(mp, t(d[f"y_eval_map{i}"]), tol, f"detect eval map {i}")
        _fuse(m)
        close(run(m, [x.detach() for x in xs], dtype)[0], t(d["y_fused"]), tol, "detect decoded eval output after fuse")


class _no_joins:
    """every gradient sum left to autograd: mark_join does nothing, so no tensor carries a GradJoin (modules reach it through the ops package,
    chan_split2 through ops.conv)"""

    def __enter__(self):
        from improving_yolov8_cbam_swinblock_amd import ops

        self.ops, self.saved = ops, (ops.mark_join, ops.conv.mark_join)
        ops.mark_join = ops.conv.mark_join = lambda tensor, consumers, force=False: tensor

    def __exit__(self, *exc):
        self.ops.mark_join, self.ops.conv.mark_join = self.saved


def _same_gradients(got, ref, names, what):
    """relative L2 1e-4 per tensor (float32 sums in another order).  A BatchNorm bias takes the norm of its own scale's gradient as a second
    yardstick: some are zero in exact arithmetic - Attention.pe's always (its per-channel constant meets only proj's 1x1 convolution and
    train-mode BatchNorm, whose mean subtraction removes it), in C2PSA also proj's and ffn[1]'s of the last block (cv2 removes theirs) - and
    what both runs then hold is rounding noise of sums whose terms are as large as the scale's."""
    assert len(got) == len(ref)
    norms = {n: float(b.double().norm()) for n, b in zip(names, ref) if b is not None}
    for n, a, b in zip(names, got, ref):
        assert a is not None and b is not None, (what, n)
        a, b = a.double(), b.double()
        yard = max(float(b.norm()), norms.get(n[: -len("bias")] + "weight", 0.0) if n.endswith("bn.bias") else 0.0)
        assert float((a - b).norm()) <= 1e-4 * yard + 1e-12, (what, n, float((a - b).norm()), float(b.norm()))


def test_c3k2_with_c3k_members_keeps_the_joined_gradient():
    """a C3k member reads its input twice (cv1, cv2) and has no shortcut: C2f's consumer count for it is 2 (+ 1 for the concat from the second
    member on).  One too few loses a gradient, one too many leaves the sum waiting: every gradient equals the run in which autograd forms all
    the sums, and a join was really at work."""
    from improving_yolov8_cbam_swinblock_amd import ops

    torch.manual_seed(4)
    m = P().C3k2(32, 32, 2, True)
    set_bn(m)
    with torch.no_grad():
        for q in m.parameters():
            q.copy_(torch.randn_like(q) * 0.3 + (1.0 if q.dim() == 1 else 0.0))
    m = m.to(dev()).train()
    assert isinstance(m.m[0], P().C3k) and m._reads(m.m[0]) == 2
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x0 = torch.randn(2, 32, 9, 7, device=dev())
    gy = torch.randn(2, 32, 9, 7, device=dev())
    names = ["x"] + [n for n, _ in m.named_parameters()]
    seen = []
    real = ops.GradJoin.arrive

    def spy(self):
        seen.append(self.n)
        return real(self)

    ops.GradJoin.arrive = spy
    try:
        x = x0.clone().requires_grad_(True)
        got = grads_of(m(x), [x] + list(m.parameters()), gy)
    finally:
        ops.GradJoin.arrive = real
    assert 2 in seen and 3 in seen, seen  # first member: cv1 + cv2; second member: cv1 + cv2 + the concat
    m.load_state_dict(state, strict=True)
    with _no_joins():
        x = x0.clone().requires_grad_(True)
        ref = grads_of(m(x), [x] + list(m.parameters()), gy)
    _same_gradients(got, ref, names, "C3k2 with C3k members")


def test_psablock_whose_input_feeds_a_second_consumer_keeps_the_joined_gradient():
    """t feeds a PSABlock (its qkv convolution and its shortcut: two reads) and a second Conv; the caller's join counts three.  Every gradient
    equals the run in which autograd forms the sums."""
    from improving_yolov8_cbam_swinblock_amd import ops

    torch.manual_seed(6)
    M = P()
    pre, blk, side = M.Conv(64, 64, 1), M.PSABlock(64, num_heads=1), M.Conv(64, 32, 3)
    mods = torch.nn.ModuleList([pre, blk, side])
    set_bn(mods)
    with torch.no_grad():
        for q in mods.parameters():
            q.copy_(torch.randn_like(q) * 0.3 + (1.0 if q.dim() == 1 else 0.0))
    mods = mods.to(dev()).train()
    state = {k: v.clone() for k, v in mods.state_dict().items()}
    x0 = torch.randn(2, 64, 9, 8, device=dev())
    gy1, gy2 = torch.randn(2, 64, 9, 8, device=dev()), torch.randn(2, 32, 9, 8, device=dev())
    names = ["x"] + [n for n, _ in mods.named_parameters()]

    def step(join):
        mods.load_state_dict(state, strict=True)
        x = x0.clone().requires_grad_(True)
        tt = pre(x)
        if join:
            ops.mark_join(tt, 3)
            assert ops.join_of(tt) is not None
        return torch.autograd.grad([blk(tt), side(tt)], [x] + list(mods.parameters()), [gy1, gy2], allow_unused=True)

    got = step(True)
    with _no_joins():
        ref = step(False)
    _same_gradients(got, ref, names, "PSABlock beside a second consumer")


def test_psa_equals_c2psa_with_one_block():
    """PSA(c, c) is C2PSA(c, c, 1) with the block's attn / ffn as its own attributes (reference block.py:1394-1449 against :1452-1507): the same
    weights give the same bits, forward and backward."""
    torch.manual_seed(10)
    a, b = P().PSA(128, 128), P().C2PSA(128, 128, 1)
    set_bn(a)
    set_bn(b)
    with torch.no_grad():
        for q in b.parameters():
            q.copy_(torch.randn_like(q) * 0.3 + (1.0 if q.dim() == 1 else 0.0))
    a.load_state_dict({k.replace("m.0.", ""): v for k, v in b.state_dict().items()}, strict=True)
    a, b = a.to(dev()).train(), b.to(dev()).train()
    x0 = torch.randn(2, 128, 7, 9, device=dev())
    gy = torch.randn(2, 128, 7, 9, device=dev())
    outs = []
    for m in (a, b):
        x = x0.clone().requires_grad_(True)
        y = m(x)
        outs.append((y, dict(zip(["x"] + [n.replace("m.0.", "") for n, _ in m.named_parameters()], grads_of(y, [x] + list(m.parameters()), gy)))))
    assert torch.equal(outs[0][0], outs[1][0]) and set(outs[0][1]) == set(outs[1][1])
    for n, g in outs[0][1].items():
        assert torch.equal(g, outs[1][1][n]), n


def test_c2psa_marks_the_split_half_for_both_reads():
    """C2PSA: the second half of cv1's output is read by the first block's qkv convolution and by its shortcut; its gradient lands in the
    half's slice of cv1's gradient buffer.  Gradients equal the autograd-summed run."""
    torch.manual_seed(8)
    m = P().C2PSA(128, 128, 2)
    set_bn(m)
    with torch.no_grad():
        for q in m.parameters():
            q.copy_(torch.randn_like(q) * 0.3 + (1.0 if q.dim() == 1 else 0.0))
    m = m.to(dev()).train()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    x0 = torch.randn(2, 128, 9, 8, device=dev())
    gy = torch.randn(2, 128, 9, 8, device=dev())
    names = ["x"] + [n for n, _ in m.named_parameters()]
    x = x0.clone().requires_grad_(True)
    got = grads_of(m(x), [x] + list(m.parameters()), gy)
    m.load_state_dict(state, strict=True)
    with _no_joins():
        x = x0.clone().requires_grad_(True)
        ref = grads_of(m(x), [x] + list(m.parameters()), gy)
    _same_gradients(got, ref, names, "C2PSA")
