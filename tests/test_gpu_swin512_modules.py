"""GPU: SwinBlock(512, 2) - head_dim 256, the block of yolo11-cbam-swin - against the reference's outputs (tests/golden/swin_d512_*,
tests/golden/make_swin512_golden.py): four full 7 x 7 windows, padding tokens acting as keys, and 196-token windows with padding (the tiled
kernels).  The assertions and bounds are those of test_gpu_modules_golden.py::test_swin_block_head_dim_192_and_large_windows_vs_reference."""
import pytest
import torch

from conftest import large_swin_grad_errors, load_large_swin
from test_gpu_modules_golden import BF16_TOL, F32_TOL, P, close, close_l2, dev, grads_of, run, t
from test_swin512_cpu import SWIN512

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", SWIN512)
def test_swin_block_512_vs_reference(name, dtype):
    """forward, input gradient and every parameter gradient.  float32: 1e-3 (north_star); bfloat16: 6e-2 scaled max-abs forward, 5e-2 relative
    L2 on gradients."""
    m, x, gy, d, seeded = load_large_swin(name, lambda dim, heads, ws: P().SwinBlock(dim, heads, ws))
    assert m.dim == 512 and m.attn.num_heads == 2
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
