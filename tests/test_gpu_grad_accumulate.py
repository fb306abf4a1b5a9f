"""GPU: ymi_opt_grad_accumulate (csrc/optim.hip) through FusedSGD.accumulate / step / discard_pending, on its own: a toy module whose
parameter lengths sit on every edge of the kernel's chunking (ymi_opt_chunk_elems, YMI_OPT_MAX_GRADS tensors per launch).  The two fused
optimizers are compared with each other bit for bit, and the second with the float64 restatement tests/optim_exact.py after each step: a fault
in the tail handling, the scalar path or the second range would be the same on both fused sides."""
import pytest
import torch

import optim_exact as X
from optim_exact import Toy

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def seeded_grads(model, seed, scale):
    """{param: gradient}; the odd parameter's gradient is a view 4 bytes past a 16-byte boundary as well"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n, p in model.named_parameters():
        if n == "nograd":
            continue
        t = (torch.randn(p.numel() + 1, generator=g) * scale).to(dev())
        out[p] = t[1:] if n == "odd" else t[:-1].clone()
    return out


def test_accumulate_kernel_folds_steps_and_clears():
    from improving_yolov8_cbam_swinblock_amd import _lib
    from improving_yolov8_cbam_swinblock_amd.engine.optim import FusedSGD

    c = int(_lib.lib().ymi_opt_chunk_elems())
    a, b = Toy(c), Toy(c)
    assert a.odd.data_ptr() % 16 == 4 and all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    opt, ref = FusedSGD(a, lr=0.05), FusedSGD(b, lr=0.05)
    assert opt._arena is None and opt.pending == 0
    g1, g2 = seeded_grads(a, 11, 1.0), seeded_grads(a, 12, 0.37)
    assert g1[a.odd].data_ptr() % 16 == 4
    opt.accumulate(g1)                       # fold 1: an explicit map
    for p, g in g2.items():
        p.grad = g
    opt.accumulate()                         # fold 2: p.grad
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert opt.pending == 2 and len(opt.ranges) >= 2 and len(opt.params) > _lib.OPT_MAX_GRADS
    index = {p: i for i, p in enumerate(opt.params)}
    for p in g1:
        want = (torch.zeros_like(p) + g1[p]) + g2[p]
        assert torch.equal(opt._acc[index[p]], want), [n for n, q in a.named_parameters() if q is p]
    assert opt._acc[index[a.nograd]].abs().max() == 0
    assert opt._acc[index[a.w0]].data_ptr() % 16 == 0
    opt.step()                               # nothing new to fold: steps from the sums, clears
    torch.cuda.synchronize()
    assert opt.pending == 0 and float(opt._arena.abs().max()) == 0.0
    pb = dict(zip(a.parameters(), b.parameters()))
    sums = {pb[p]: g1[p] + g2[p] for p in g1}
    before = X.class_before(ref, sums)
    ref.step(sums)
    X.class_after(ref, before)               # the third party: the float64 restatement, every element of parameters and momentum
    torch.cuda.synchronize()
    assert opt.grad_norm() == ref.grad_norm() and opt.grad_norm() > 10.0  # the clip is active, on the total
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    # second round: one fold, then the updating step folds its own gradients in; then a discarded fold leaves no trace
    opt.accumulate(g2)
    opt.step(g1)
    sums = {pb[p]: g2[p] + g1[p] for p in g1}
    before = X.class_before(ref, sums)
    ref.step(sums)
    X.class_after(ref, before)
    opt.accumulate(g1)
    opt.discard_pending()
    torch.cuda.synchronize()
    assert opt.pending == 0 and float(opt._arena.abs().max()) == 0.0
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), n
    for m, r in zip(opt.momentum, ref.momentum):
        assert torch.equal(m, r)
    assert "arena" not in str(opt.state_dict().keys()) and set(opt.state_dict()) == {"state", "param_groups"}
