"""Generate the detection-loss fixtures under tests/golden/ by running the REAL reference on the CPU (the reference's tree must be present; the
import shim is make_golden.py's).  Writes data only:

    loss_exact_<case>.npz   the reference's v8DetectionLoss and its TaskAlignedAssigner on the guarded cases of tests/loss_exact.py
                            (base, rect, four_levels, crowded): target_gt_idx, fg_mask, target_bboxes (pixels), target_scores, loss
                            (= items * batch), items, and the gradients of (loss * GRAD_LOSS).sum() with respect to each level's map

    python tests/golden/make_loss_golden.py

Inputs are rebuilt from the cases' seeds on both sides; nothing of them is stored."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT))
sys.path.insert(0, str(OUT.parent))
from make_golden import import_reference_package, save  # noqa: E402

import loss_exact as X  # noqa: E402


def holder(inp):
    """what v8DetectionLoss reads of a model: a parameter (device), args (gains), model[-1] with stride / nc / reg_max"""
    m = torch.nn.Module()
    m.p = torch.nn.Parameter(torch.zeros(1))
    m.args = SimpleNamespace(box=X.HYP[0], cls=X.HYP[1], dfl=X.HYP[2])
    m.model = [SimpleNamespace(stride=torch.tensor(inp["strides"]), nc=inp["nc"], reg_max=X.REG)]
    return m


def main():
    torch.set_num_threads(4)
    import_reference_package()
    from ultralytics.utils.loss import v8DetectionLoss

    for name in X.GUARDED:
        inp = X.build(name)
        crit = v8DetectionLoss(holder(inp))
        kept = {}
        inner = crit.assigner.forward

        def spy(*a, _inner=inner, _kept=kept, **k):
            r = _inner(*a, **k)
            _kept["r"] = [t.detach().clone() for t in r]
            return r

        crit.assigner.forward = spy
        preds = [torch.cat((b, c), -1).permute(0, 3, 1, 2).contiguous().requires_grad_(True) for b, c in zip(inp["box"], inp["cls"])]
        batch = {"batch_idx": inp["batch_idx"], "cls": inp["labels"].view(-1, 1), "bboxes": inp["bboxes"]}
        loss, items = crit(preds, batch)
        grads = torch.autograd.grad((loss * torch.tensor(X.GRAD_LOSS)).sum(), preds)
        _, tb, ts, fg, gi = kept["r"]
        save(f"loss_exact_{name}", target_gt_idx=gi.numpy().astype(np.int16), fg_mask=fg.numpy(), target_bboxes=tb.numpy(), target_scores=ts.numpy(),
             loss=loss.detach().numpy(), items=items.numpy(), **{f"g.pred{i}": g.numpy() for i, g in enumerate(grads)})


if __name__ == "__main__":
    main()
