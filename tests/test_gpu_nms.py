"""GPU: ops.detect_nms (csrc/nms.hip through the C ABI) against the reference's fixtures and against tests/nms_exact.py, bit for bit:
rows, order, counts and the zero padding.  tests/test_host_nms_check.py holds nms_exact itself to the reference on the CPU and asserts
the input conditions of the guarded cases (distinct scores, float64 margin >= 1e-5); they are asserted here again, never skipped.  No
element is left out of any comparison."""
import ctypes

import numpy as np
import pytest
import torch

import nms_exact as NX

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def run(y, c, **over):
    from improving_yolov8_cbam_swinblock_amd import ops

    kw = dict(NX.nms_kwargs(c), **over)
    det, count = ops.detect_nms(y.to(dev()), c["conf"], c["iou"], **kw)
    torch.cuda.synchronize()
    return det.cpu(), count.cpu()


def assert_same(got, want, what):
    (gd, gc), (wd, wc) = got, want
    assert gc.dtype == torch.int32 and gd.dtype == torch.float32
    assert torch.equal(gc, wc), (what, "counts", gc.tolist(), wc.tolist())
    if not NX.same_bits(gd, wd):
        bad = torch.nonzero((gd.view(torch.int32) != wd.view(torch.int32)).any(2))
        b, r = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} rows differ, first at image {b} row {r}: got {gd[b, r].tolist()} want {wd[b, r].tolist()}")


@pytest.mark.parametrize("name", list(NX.CASES))
def test_detect_nms_equals_reference_fixture_and_restatement(name):
    c = NX.CASES[name]
    y = NX.case_input(name)
    want, recorded = NX.load_expected(name)
    max_det = c.get("max_det", 300)
    if c["guarded"]:
        info = NX.margin(y, c["conf"], c["iou"], **NX.nms_kwargs(c))
        assert all(m[2] for m in info) and min(m[0] for m in info) >= NX.MARGIN_MIN
    got = run(y, c)
    print(f"[{name}] counts {got[1].tolist()[:8]} recorded float64 margin {recorded.min():.3e}")
    assert_same(got, NX.padded(want, max_det), f"{name} vs the reference fixture")
    assert_same(got, NX.nms_exact(y, c["conf"], c["iou"], **NX.nms_kwargs(c)), f"{name} vs nms_exact")
    assert bool((got[0][torch.arange(max_det)[None] >= got[1][:, None]] == 0).all()), "rows past the count must be zero"


@pytest.mark.parametrize("over", [dict(max_det=10), dict(max_det=1), dict(iou=0.45), dict(iou=0.6), dict(conf=0.25), dict(multi_label=False),
                                  dict(agnostic=True), dict(classes=[1]), dict(max_nms=5000)], ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_parameter_sweep_on_the_loaded_input(over):
    """the flagship input (nc 3, ~25 k candidates per image) under every parameter the op has, against nms_exact.  These variants are
    not guarded by a margin: like the unguarded case below they hold the kernel to the restatement's float32 operation order."""
    c = dict(NX.CASES["nc3_b3"])
    c.update({k: v for k, v in over.items() if k in ("conf", "iou")})
    kw = {k: v for k, v in over.items() if k not in ("conf", "iou")}
    y = NX.case_input("nc3_b3")
    full = dict(NX.nms_kwargs(c), **kw)
    assert_same(run(y, c, **kw), NX.nms_exact(y, c["conf"], c["iou"], **full), str(over))


def test_unguarded_random_case_equals_the_restatement_bit_for_bit():
    """off-grid coordinates, continuous jitter, margin not controlled: equal only if every IoU is rounded as the restatement rounds it
    (no contraction of area_i + area_j - inter, true division).  The float64 margin is printed so that a failure shows at once whether a
    near-threshold pair is involved."""
    y = torch.from_numpy(np.stack([NX.cluster_image(900 + i, 8400, 3, grid=0) for i in range(4)]))
    y80 = torch.from_numpy(NX.cluster_image(951, 8400, 80, density=0.05, grid=0)[None])
    for what, yy in (("nc3", y), ("nc80", y80)):
        info = NX.margin(yy, 0.001, 0.7, multi_label=True)
        print(f"[unguarded {what}] float64 margins {[f'{m[0]:.2e}' for m in info]}")
        c = dict(conf=0.001, iou=0.7, multi_label=True)
        assert_same(run(yy, c), NX.nms_exact(yy, 0.001, 0.7, multi_label=True), f"unguarded {what}")


@pytest.mark.parametrize("name", ["tie_scores", "tie_best_class"])
@pytest.mark.parametrize("max_nms", [1000, 1001, 37])
def test_equal_scores_straddling_the_max_nms_cut(name, max_nms):
    """the select kernel's hardest branch: the score of rank max_nms is shared by many candidates, some on either side of the cut, spread over
    threads and anchor chunks; those with the lowest (anchor, class) must be the ones taken."""
    c = NX.CASES[name]
    y = NX.case_input(name)
    s = NX.candidates(y[0], c["conf"], c["multi_label"])[1].sort(descending=True)[0]
    assert s.numel() > max_nms + 1
    cut = s[max_nms - 1]
    below, above = int((s[max_nms:] == cut).sum()), int((s[:max_nms] == cut).sum())
    print(f"[{name} max_nms {max_nms}] candidates {s.numel()}; with the cut score: {above} taken, {below} left out")
    assert above >= 2 and below >= 1, "the cut does not fall inside a run of equal scores"
    kw = dict(NX.nms_kwargs(c), max_nms=max_nms)
    assert_same(run(y, c, max_nms=max_nms), NX.nms_exact(y, c["conf"], c["iou"], **kw), f"{name} max_nms {max_nms}")
    # the restatement with the opposite tie order differs here: the comparison above can tell which equals were taken
    wrong = NX.nms_exact(y, c["conf"], c["iou"], fault="unstable_ties", **kw)
    right = NX.nms_exact(y, c["conf"], c["iou"], **kw)
    assert not (NX.same_bits(wrong[0], right[0]) and torch.equal(wrong[1], right[1]))


def test_empty_class_filter_keeps_nothing():
    from improving_yolov8_cbam_swinblock_amd.utils.ops import non_max_suppression

    c = NX.CASES["nc3_b3"]
    y = NX.case_input("nc3_b3")
    det, count = run(y, c, classes=[])
    assert not bool(count.any()) and not bool(det.any())
    assert_same((det, count), NX.nms_exact(y, c["conf"], c["iou"], **dict(NX.nms_kwargs(c), classes=[])), "empty filter")
    out = non_max_suppression(y.to(dev()), c["conf"], c["iou"], classes=[], multi_label=True)
    assert [tuple(o.shape) for o in out] == [(0, 6)] * 3


def test_two_runs_give_identical_bits():
    c = NX.CASES["nc80_over_max_nms"]
    y = NX.case_input("nc80_over_max_nms")
    a, b = run(y, c), run(y, c)
    assert NX.same_bits(a[0], b[0]) and torch.equal(a[1], b[1])
    c = NX.CASES["tie_scores"]
    y = NX.case_input("tie_scores")
    runs = [run(y, c) for _ in range(3)]
    assert all(NX.same_bits(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) for r in runs)


def test_captured_graph_replays_on_new_data():
    """eval forward + detect_nms captured once on one stream, replayed on a second input: equal to the eager result on that input."""
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.nn.tasks import DetectionModel

    torch.manual_seed(3)
    model = DetectionModel("yolov8n-cbam.yaml", ch=3, nc=3).to(dev()).eval()
    with torch.no_grad():
        for m in model.model[-1].cv3:
            m[-1].bias.add_(6.0)  # (the initial class bias leaves nothing above conf)
    g = torch.Generator().manual_seed(5)
    imgs = [torch.rand(2, 3, 256, 256, generator=g).to(dev()) for _ in range(2)]
    kw = dict(multi_label=True, max_det=50)

    def eager(x):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y = model(x)[0]
            return (y,) + ops.detect_nms(y, 0.25, 0.6, **kw)

    static = imgs[0].clone()
    for _ in range(2):
        eager(static)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gdet, gcount = eager(static)
    for x in (imgs[1], imgs[0]):
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        rep = (gdet.cpu().clone(), gcount.cpu().clone())
        ey, edet, ecount = eager(x)
        torch.cuda.synchronize()
        assert int(ecount.sum()) > 0
        assert NX.same_bits(gy, ey), "the eval forward itself differs between replay and eager"
        assert_same(rep, (edet.cpu(), ecount.cpu()), "graph replay vs eager")
        assert_same(rep, NX.nms_exact(ey.cpu(), 0.25, 0.6, **kw), "graph replay vs nms_exact")


@pytest.mark.parametrize("name", ["nc3_b3", "empty_and_all_survive", "nc3_filter", "nc80_best_agnostic_det1"])
def test_list_wrapper_equals_reference_shaped_fixture(name):
    from improving_yolov8_cbam_swinblock_amd.utils.ops import non_max_suppression

    c = NX.CASES[name]
    y = NX.case_input(name).to(dev())
    before = y.clone()
    want, _ = NX.load_expected(name)
    out = non_max_suppression((y, None), c["conf"], c["iou"], classes=c.get("classes"), agnostic=c.get("agnostic", False), multi_label=c["multi_label"],
                              max_det=c.get("max_det", 300), nc=c["nc"])
    assert torch.equal(y, before), "the wrapper must not modify its input"
    assert isinstance(out, list) and len(out) == len(want)
    for o, w in zip(out, want):
        assert o.is_cuda and o.shape == (len(w), 6) and NX.same_bits(o, w)


def test_bad_arguments_are_refused_before_any_launch():
    from improving_yolov8_cbam_swinblock_amd import _lib

    L = _lib.lib()
    y = NX.case_input("iou_equals_threshold").to(dev())
    det = torch.full((1, 300, 6), 7.0, device=dev())
    count = torch.full((1,), -5, dtype=torch.int32, device=dev())
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda conf, iou, nbytes: L.ymi_detect_nms(p(y), 1, 1, 64, conf, iou, 0, 0, None, 0, 300, 30000, 7680.0, p(det), p(count), p(ws), nbytes,
                                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(0.25, 0.5, 8) == -4  # YMI_EWORKSPACE
    assert call(1.25, 0.5, ws.numel()) == -1 and call(0.25, 1.5, ws.numel()) == -1  # YMI_EINVAL
    bad = (ctypes.c_int32 * 1)(5)
    assert L.ymi_detect_nms(p(y), 1, 1, 64, 0.25, 0.5, 0, 0, bad, 1, 300, 30000, 7680.0, p(det), p(count), p(ws), ws.numel(), None) == -1
    torch.cuda.synchronize()
    assert bool((det == 7.0).all()) and int(count[0]) == -5, "a refused call wrote its outputs"
    assert call(0.25, 0.5, ws.numel()) == 0
    torch.cuda.synchronize()
    assert int(count[0]) == 3  # (the pair at iou 0.5 exactly both stay, of the pair above it one)
