"""The oriented-box loss kernels of csrc/loss.hip, stage by stage, against the float64 restatement of tests/obb_ref.py, and the criterion against
the reference's fixtures (tests/golden/obb_loss_*.npz).

Through the C ABI with buffers this file owns: ymi_obb_targets, ymi_obb_loss_sizes / _fwd / _bwd.  State and workspace are sliced into named
views by the restated layouts (obb_ref.carve_state / carve_work, whose totals must equal ymi_obb_loss_sizes).

  discrete stages    inside mask, mpos, gidx, lab equal the restatement, except for the (gt, anchor) decisions whose float64 margin is below
                     obb_ref.THRESHOLD (obb_ref.uncertain); at most obb_ref.MAX_LEFT_OUT of a case's decisions may be left out
  continuous stages  obb_ref.scaled_err against float64 within KERNEL_FACTOR (4) times the recorded distance of the reference's float32
                     arithmetic (obb_ref.REF32_DISTANCE), floored at F32_TOL.  Every figure is printed before it is asserted.
  bfloat16 maps      the restatement is fed the same bf16-rounded maps and the kernel's own assignment; stored gradients add one rounding, 2^-8
  also               two runs bit-equal; a batch without labels gives exact zero box and angle gradients; OBBPreds, the train tuple and the
                     eval tuple give the criterion the same result bit for bit"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import obb_ref as R
from conftest import load_golden
from obb_common import CH, HYP, LOSS_CASES, NE, loss_case
from test_gpu_modules_golden import F32_TOL, P, dev

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
CASE_DTYPES = [(n, dt) for n in LOSS_CASES for dt in (F32, BF)]
IDS = [f"{n}-{'bf16' if dt == BF else 'f32'}" for n, dt in CASE_DTYPES]
assert R.F32_FLOOR == F32_TOL["atol"]


def L():
    from improving_yolov8_cbam_swinblock_amd import _lib

    return _lib


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def arr(ts):
    return (L().YmiTensor * len(ts))(*[L().as_ymi(t) for t in ts])


def bound(stage):
    return max(R.KERNEL_FACTOR * R.REF32_DISTANCE[stage], R.F32_FLOOR)


_runs = {}


def run(name, dtype, again=0):
    """one forward and backward of a case through the C ABI -> every buffer on the CPU"""
    key = (name, dtype, again)
    if key in _runs:
        return _runs[key]
    lib = L().lib()
    c = loss_case(name)
    B, nc, G, A, nl = c["B"], c["nc"], c["G"], c["A"], len(c["levels"])
    dcw = (nc + 7) // 8 * 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    feats = [t.to(dev()).to(dtype) for t in c["feats"]]
    box = [t[:, :64].contiguous(memory_format=torch.channels_last) for t in feats]
    cls = [t[:, 64:].contiguous(memory_format=torch.channels_last) for t in feats]
    angle = c["angle"].to(dev()).contiguous()
    strides = (ctypes.c_float * nl)(*c["strides"])
    bt = c["batch"]
    n = int(bt["batch_idx"].numel())
    bi, cl, bb = (t.to(dev()).float().reshape(-1).contiguous() if n else None for t in (bt["batch_idx"], bt["cls"], bt["bboxes"]))
    targets = torch.full((B, G, 6), float("nan"), device=dev())
    L().check(lib.ymi_obb_targets(p(bi), p(cl), p(bb), n, B, G, c["img_w"], c["img_h"], p(targets), stream), "obb_targets")
    sb, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    L().check(lib.ymi_obb_loss_sizes(B, A, G, ctypes.byref(sb), ctypes.byref(wb)), "obb_loss_sizes")
    (slay, stot), (wlay, wtot) = R.carve_state(B, A), R.carve_work(B, A, G)
    assert (stot, wtot) == (sb.value, wb.value), "the restated layouts no longer give the library's sizes"
    state = torch.full((stot + 256,), 0xFF, dtype=torch.uint8, device=dev())
    work = torch.full((wtot + 256,), 0xFF, dtype=torch.uint8, device=dev())
    scale6 = torch.tensor(R.out_scale(B), dtype=F32, device=dev())
    loss_out = torch.full((6,), float("nan"), device=dev())
    L().check(lib.ymi_obb_loss_fwd(nl, arr(box), arr(cls), p(angle), strides, p(targets), G, R.TOPK, R.ALPHA, R.BETA, p(scale6), p(loss_out), p(state), stot,
                                   p(work), wtot, stream), "obb_loss_fwd")
    gl = torch.tensor(R.GRAD_LOSS, dtype=F32, device=dev())
    dbox = [torch.full_like(t, float("nan")) for t in box]
    dcls = [torch.full((B, dcw, t.shape[2], t.shape[3]), float("nan"), dtype=dtype, device=dev()).contiguous(memory_format=torch.channels_last) for t in cls]
    dangle = torch.full((B, 1, A), float("nan"), device=dev())
    L().check(lib.ymi_obb_loss_bwd(nl, arr(box), arr(cls), p(angle), strides, p(state), stot, p(gl), p(scale6), arr(dbox), arr(dcls), p(dangle), stream),
              "obb_loss_bwd")
    torch.cuda.synchronize()
    assert (state[stot:] == 0xFF).all() and (work[wtot:] == 0xFF).all(), "a kernel wrote behind its buffer"
    sv, wv = R.views(state.cpu(), slay), R.views(work.cpu(), wlay)
    out = dict(case=c, feats=[t.float().cpu() for t in feats], targets=targets.cpu(), pb=wv["pb"].view(B, A, 5), ov=wv["ov"].view(B, G, A),
               al=wv["al"].view(B, G, A), mpos=wv["mpos"].view(B, G, A), inside=wv["inm"].view(B, G, A), gidx=wv["gidx"].view(B, A), pa=wv["pa"].view(B, G),
               po=wv["po"].view(B, G), tgt=sv["tgt"].view(B, A, 5), wgt=sv["wgt"].view(B, A), lab=sv["lab"].view(B, A), tss=sv["scal"][:1], loss6=loss_out.cpu(),
               dbox=[t.float().cpu() for t in dbox], dcls=[t.float().cpu() for t in dcls], dangle=dangle.cpu(), dcw=dcw)
    _runs[key] = out
    return out


_refs = {}


def reference(name, dtype):
    key = (name, dtype)
    if key not in _refs:
        o = run(name, dtype)
        kw = dict(grad_scale=R.out_scale(o["case"]["B"])[:3])
        if dtype == BF:
            kw.update(feats=o["feats"], mpos=o["mpos"].bool(), gidx=o["gidx"].long())
        _refs[key] = R.restate(o["case"], **kw)
    return _refs[key]


@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_stages_match_the_restatement(name, dtype):
    o, r = run(name, dtype), reference(name, dtype)
    c = o["case"]
    B, G, A, nc = c["B"], c["G"], c["A"], c["nc"]
    r64 = R.restate(c) if dtype == BF else r
    left, share = R.uncertain(c, r64)
    print(f"{name}: {int(left.sum())} of {left.numel()} (gt, anchor) decisions left out ({share:.4f})")
    assert share <= R.MAX_LEFT_OUT
    keep = ~left
    assert ((o["inside"] != 0) == r["inside"])[keep].all(), "inside mask"
    if dtype == F32:  # (bfloat16: the scores are rounded, the picks are the kernel's own and were handed to the restatement)
        assert ((o["mpos"] != 0) == r["mpos"])[keep].all(), "top-k picks"
        a_keep = keep.all(1)
        assert (o["gidx"].long() == r["gidx"])[a_keep].all(), "assignment"
    assert (o["lab"].long() == r["lab"])[keep.all(1)].all(), "labels"
    ref = dict(targets=r["targets"], pb=r["pb"], ov=r["ov"], al=r["al"], pa=r["pa"], po=r["po"], tgt=r["tgt"], wgt=r["wgt"], tss=r["tss"].reshape(1),
               loss6=r["loss6"])
    clean = bool(keep.all())
    fails = []
    for stage, want in ref.items():
        if not clean and stage not in ("targets", "pb"):
            continue  # (a decision left out may move everything behind it)
        err = R.scaled_err(o[stage], want)
        print(f"  {stage:8s} {err:.3e}  bound {bound(stage):.1e}  (float32 reference {R.REF32_DISTANCE[stage]:.1e})")
        if not err <= bound(stage):
            fails.append((stage, err))
    if clean:
        store = 2.0 ** -8 if dtype == BF else 0.0
        gb = torch.cat([g[:, :64].permute(0, 2, 3, 1).reshape(-1) for g in r["dfeats"]])
        gc = torch.cat([g[:, 64:].permute(0, 2, 3, 1).reshape(-1) for g in r["dfeats"]])
        ob = torch.cat([g.permute(0, 2, 3, 1).reshape(-1) for g in o["dbox"]])
        oc = torch.cat([g[:, :nc].permute(0, 2, 3, 1).reshape(-1) for g in o["dcls"]])
        for stage, got, want, b in (("dbox", ob, gb, bound("dfeats") + store), ("dcls", oc, gc, bound("dfeats") + store), ("dangle", o["dangle"], r["dangle"], bound("dangle"))):
            err = R.scaled_err(got, want)
            print(f"  {stage:8s} {err:.3e}  bound {b:.1e}")
            if not err <= b:
                fails.append((stage, err))
        assert all((g[:, nc:] == 0).all() for g in o["dcls"]), "class-gradient padding channels are exact zeros"
    assert not fails, fails


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_two_runs_are_bit_equal(dtype):
    a, b = run("obb_loss_crowded", dtype), run("obb_loss_crowded", dtype, again=1)
    for k in ("pb", "ov", "al", "mpos", "inside", "gidx", "pa", "po", "tgt", "wgt", "lab", "tss", "loss6", "dangle"):
        assert torch.equal(a[k], b[k]), k
    for k in ("dbox", "dcls"):
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_no_labels_gives_exact_zero_box_and_angle_gradients(dtype):
    o = run("obb_loss_nolabels", dtype)
    assert all((g == 0).all() for g in o["dbox"]) and (o["dangle"] == 0).all()
    assert float(o["loss6"][0]) == 0.0 and float(o["loss6"][2]) == 0.0 and float(o["loss6"][1]) > 0
    assert (o["gidx"] == -1).all() and (o["lab"] == -1).all()


def _criterion(c):
    from improving_yolov8_cbam_swinblock_amd.utils.loss import v8OBBLoss

    head = P().OBB(c["nc"], NE, CH[:1] * len(c["levels"]))
    head.stride = torch.tensor(c["strides"])
    holder = torch.nn.Module()
    holder.model = torch.nn.ModuleList([head])
    holder.args = SimpleNamespace(**HYP)
    return v8OBBLoss(holder.to(dev()))


def _leaves(c, dtype=F32):
    feats = [t.to(dev()).to(dtype).requires_grad_(True) for t in c["feats"]]
    angle = c["angle"].to(dev()).requires_grad_(True)
    batch = {k: (v.to(dev()) if torch.is_tensor(v) else v) for k, v in c["batch"].items()}
    return feats, angle, batch


@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_criterion_matches_the_reference_fixtures(name):
    """float32 maps in the reference layout (feats, angle): loss, items and the gradients with respect to the three maps and the angle"""
    c = loss_case(name)
    gold = load_golden(name)
    feats, angle, batch = _leaves(c)
    loss, items = _criterion(c)((feats, angle), batch)
    loss.sum().backward()
    fails = []
    for what, got, want, b in [("loss", loss, gold["loss"], bound("loss")), ("items", items, gold["items"], bound("loss")),
                               ("g.angle", angle.grad, gold["g.angle"], bound("dangle"))] + [
                                   (f"g.f{i}", f.grad, gold[f"g.f{i}"], bound("dfeats")) for i, f in enumerate(feats)]:
        err = R.scaled_err(got.detach().float().cpu(), torch.from_numpy(np.asarray(want)))
        print(f"{name} {what:8s} {err:.3e} bound {b:.1e}")
        if not err <= b:
            fails.append((what, err))
    assert not fails, fails


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_preds_forms_give_the_same_result_bit_for_bit(dtype):
    """OBBPreds (split maps), the train tuple (feats, angle) and the eval tuple (y, (feats, angle))"""
    c = loss_case("obb_loss_rect")
    crit = _criterion(c)
    res = []
    for form in ("split", "train", "eval"):
        feats, angle, batch = _leaves(c, dtype)
        if form == "split":
            nh = [f.contiguous(memory_format=torch.channels_last) for f in feats]
            preds = P().OBBPreds([f[:, :64] for f in nh], [f[:, 64:] for f in nh], angle)
        elif form == "train":
            preds = (feats, angle)
        else:
            preds = (torch.zeros(1, device=dev()), (feats, angle))
        loss, items = crit(preds, batch)
        loss.sum().backward()
        res.append([loss.detach(), items, angle.grad] + [f.grad for f in feats])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)
