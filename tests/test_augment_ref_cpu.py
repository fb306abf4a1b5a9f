"""CPU: tests/augment_ref.py - the numpy restatement of the training augmentation that the GPU tests compare csrc/augment.hip with - against
fixtures the REAL reference produced (tests/golden/make_augment_golden.py: its own v8_transforms Compose, Mosaic, RandomPerspective, RandomHSV,
RandomFlip and Format).  Images are held bit for bit, matrices and draws exactly, labels as a set and to 1e-3 px.  OpenCV's part - the warp's
fixed-point interpolation and the 8-bit colour round trip - is pinned to the rule include/ymi.h writes out, not to OpenCV (not installed where
the fixtures were made; see the disclosure in augment_ref.py).  Each planted fault must be noticed by a fixture, and the host side of the
product - ops.mosaic_placement, ops.affine_matrix, ops.hsv_luts and data.augment's parameter classes - is held to the same fixtures here,
because it is host code."""
import json
import random
from types import SimpleNamespace

import numpy as np
import pytest

import augment_ref as AR
from conftest import GOLDEN, load_golden

DRAWS = json.loads((GOLDEN / "augment_draws.json").read_text())
NAMES = list(AR.CASES) + [f"seed{k}" for k in AR.SEEDS]
PX = 1e-3  # label coordinates: three float32 products summed at magnitudes <= 2048 are within 8 ulp, about 1e-3 px, of any other order of the sum


def case_setup(name):
    c = AR.CASES.get(name)
    hyp = AR.case_hyp(c) if c else dict(AR.HYP)
    index = c["index"] if c else int(name[4:]) % 4
    data = AR.dataset(c.get("labels", "normal") if c else "normal")
    params = AR.params_from_calls(DRAWS[name]["values"], hyp)
    return data, index, hyp, params


_GEO = {}


def case_geometry(name):
    if name not in _GEO:
        data, index, _, params = case_setup(name)
        _GEO[name] = AR.geometry(data, index, params)
    return _GEO[name]


def check_case(name, fault=None):
    """every comparison of one case with its fixture -> list of the names of those that fail"""
    d, g = load_golden(f"augment_{name}"), case_geometry(name)
    bad = []
    if not np.array_equal(g["M"], d["M"]) or g["M"].dtype != d["M"].dtype or float(g["label"]["scale"]) != float(d["scale"]):
        bad.append("matrix")
    if "canvas" in d:  # Mosaic._mosaic4's own canvas against the placements
        ch, cw = g["canvas_hw"]
        yy, xx = np.mgrid[0:ch, 0:cw]
        canvas = AR.canvas_taps(g["sources"], g["placements"], g["canvas_hw"], yy, xx, 0 if fault == "border0" else AR.BORDER, fault).astype(np.uint8)
        if not np.array_equal(canvas, d["canvas"]):
            bad.append("canvas")
    if not np.array_equal(AR.augment_image_u8(g, fault=fault), d["img"]):
        bad.append("image")
    rows, images = AR.batch_rows([g])
    keep, out, _ = AR.augment_labels(rows, images, fault=fault)
    _, cls, bb = AR.compact(keep, out)
    if bb.shape != d["bboxes"].shape or not np.array_equal(cls, d["cls"]):
        bad.append("kept labels")
    elif len(bb) and float(np.abs(bb - d["bboxes"]).max()) * AR.S > PX:
        bad.append("label coordinates")
    return bad


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    assert check_case(name) == []


@pytest.mark.parametrize("name", NAMES)
def test_every_label_decision_is_clear_of_its_threshold(name):
    """the GPU tests hold label coordinates to 1e-3 px and the kept set exactly: no row's box_candidates quantity or clip may lie within that
    margin of its threshold.  Every row of every case is checked; none is excluded."""
    g = case_geometry(name)
    rows, images = AR.batch_rows([g])
    _, _, margins = AR.augment_labels(rows, images)
    assert AR.decisions_clear(margins, PX) == []


def test_the_cases_cover_what_they_are_meant_to():
    geos = {n: case_geometry(n) for n in NAMES}
    assert [tuple(s.shape[:2]) for s in geos["seed1"]["sources"]] != [] and {tuple(im["img"].shape[:2]) for im in AR.dataset()} == set(AR.SOURCES)
    lo, hi = geos["centre_lo"]["placements"], geos["centre_hi"]["placements"]
    assert lo[0][:4] == (0, 0, 32, 32) and lo[0][4:] == (53 - 32, 37 - 32), "centre at the low extreme: the first image is cropped to its last 32 x 32"
    assert hi[3][:2] == (96, 96), "centre at the high extreme"
    affine = {n: case_setup(n)[3]["affine"] for n in ("scale05", "scale15", "rot10")}
    assert affine["scale05"]["scale"] == 0.5 and affine["scale15"]["scale"] == 1.5 and affine["rot10"]["angle"] == 10.0
    assert {(geos[n]["flip_ud"], geos[n]["flip_lr"]) for n in ("flip_none", "flip_lr", "flip_ud", "flip_both")} == {(a, b) for a in (False, True) for b in (False, True)}
    assert len(geos["no_labels"]["rows"]) == 0 and len(geos["all_filtered"]["rows"]) > 0 and len(load_golden("augment_all_filtered")["bboxes"]) == 0
    assert len(geos["single"]["sources"]) == 1 and geos["single"]["label"]["canvas"] == 0 and geos["no_hsv"]["hsv"] is None
    # a quadrant that shows nothing in the window and one that is cut by it
    g = geos["centre_lo"]
    window = AR.warp_affine([np.full(s.shape, 10 * (i + 1), np.uint8) for i, s in enumerate(g["sources"])], g["placements"], g["canvas_hw"], g["A"], AR.S)
    seen = {int(v) for v in np.unique(window)}
    assert 10 not in seen and {20, 30, 40} & seen, seen


# fault -> a case whose fixture notices it, and what fails
FAULTS = {
    "no_round16": ("scale15", "image"),
    "border0": ("scale05", "image"),           # at scale 0.5 the canvas is smaller than the window: border all round
    "canvas_fill0": ("centre_hi", "image"),    # the 37 x 53 image leaves its quadrant partly uncovered
    "hsv_no_sat": ("seed1", "image"),
    "flip_before_warp": ("flip_lr", "image"),
    "no_candidates": ("all_filtered", "kept labels"),
    "area_thr_seg": ("area_edge", "kept labels"),  # three boxes keep between 1 % and 10 % of their area
    "no_cat_clip": (None, "kept labels"),          # (any case with a box that the 2s x 2s canvas cuts)
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_every_planted_fault_is_noticed(fault):
    name, what = FAULTS[fault]
    noticed = {n: check_case(n, fault) for n in ([name] if name else NAMES)}
    assert any(what in bad for bad in noticed.values()), (fault, noticed)


def test_the_unzeroed_saturation_entry_is_inert():
    """"hsv_sat0" - RandomHSV without `lut_sat[0] = 0` (:1377) - CANNOT be noticed by any fixture: entry 0 is clip(0 * (r[1] + 1)) = 0 before the
    assignment for every finite gain, so the statement changes nothing in this version of the reference (it mattered for a table that adds).
    This test states that, over the whole gain range, rather than pretend a fixture catches it; the tables themselves are held to the
    reference's by every case with a colour stage, and "hsv_no_sat" plants a saturation fault that is noticed."""
    for r1 in np.linspace(-0.7, 0.7, 57):
        assert np.array_equal(AR.hsv_luts([0.01, r1, -0.2], fault="hsv_sat0"), AR.hsv_luts([0.01, r1, -0.2]))
    assert all(check_case(n, "hsv_sat0") == [] for n in NAMES)


def test_flip_before_warp_is_noticed_in_both_directions():
    assert "image" in check_case("flip_ud", "flip_before_warp") and "image" in check_case("flip_both", "flip_before_warp")
    assert check_case("flip_none", "flip_before_warp") == []


# ---------------------------------------------------------------------------------------------------------------- the product's host side
@pytest.mark.parametrize("name", NAMES)
def test_host_geometry_of_the_product(name):
    from improving_yolov8_cbam_swinblock_amd import ops

    d, g = load_golden(f"augment_{name}"), case_geometry(name)
    _, _, _, params = case_setup(name)
    mos = params["mosaic"]
    border = (-AR.S // 2, -AR.S // 2) if mos is not None else (0, 0)
    M, size, A = ops.affine_matrix(g["canvas_hw"], border, params["affine"])
    assert M.dtype == np.float32 and np.array_equal(M, d["M"]) and size == (AR.S, AR.S) and A == g["A"]
    if mos is not None:
        for i, (src, want) in enumerate(zip(g["sources"], g["placements"])):
            got = ops.mosaic_placement(i, mos["xc"], mos["yc"], src.shape[0], src.shape[1], AR.S)
            assert got[:6] == want and got[6:] == (want[0] - want[4], want[1] - want[5])
    if params["hsv"] is not None:
        assert np.array_equal(ops.hsv_luts(params["hsv"]), AR.hsv_luts(params["hsv"]))


@pytest.mark.parametrize("seed", AR.SEEDS)
def test_parameter_classes_reproduce_the_reference_draws(seed, monkeypatch):
    """same seeds, same parameters: the kinds and the values of every draw the reference's Compose made, in its order"""
    from improving_yolov8_cbam_swinblock_amd.data import augment as DA

    want = DRAWS[f"seed{seed}"]
    random.seed(seed)
    np.random.seed(seed)
    rec = AR.RecordingRandom()
    monkeypatch.setattr(DA, "random", rec)
    monkeypatch.setattr(DA, "np", SimpleNamespace(random=rec.np))
    params = DA.v8_transforms(SimpleNamespace(buffer=[0, 1, 2, 3]), AR.S, AR.HYP)()
    assert [k for k, _ in rec.calls] == want["kinds"] and [v for _, v in rec.calls] == want["values"]
    assert params == AR.params_from_calls(want["values"], AR.HYP)


def test_disabled_stages_still_draw_as_the_reference_does():
    """the reference's own recorded order: the mosaic test before p is looked at, MixUp's test at p = 0, a vertical flip's draw at p = 0"""
    kinds = DRAWS["seed1"]["kinds"]
    assert kinds == ["uniform", "choices"] + ["uniform"] * 2 + ["uniform"] * 8 + ["uniform", "np.uniform", "random", "random"]
    assert DRAWS["single"]["kinds"] == ["uniform"] + ["uniform"] * 8 + ["uniform", "np.uniform", "random", "random"], "mosaic = 0: the test is still drawn"
    assert DRAWS["no_hsv"]["kinds"] == ["uniform", "choices"] + ["uniform"] * 10 + ["uniform", "random", "random"], "all gains 0: no draw"


def test_scripted_cases_through_the_parameter_classes(monkeypatch):
    from improving_yolov8_cbam_swinblock_amd.data import augment as DA

    for name, c in AR.CASES.items():
        stream = AR.ScriptedRandom(c["unit"])
        monkeypatch.setattr(DA, "random", stream)
        monkeypatch.setattr(DA, "np", SimpleNamespace(random=stream.np))
        params = DA.v8_transforms(SimpleNamespace(buffer=[0, 1, 2, 3]), AR.S, AR.case_hyp(c))()
        assert not stream.unit and params == case_setup(name)[3], name


def test_what_is_not_built_says_so():
    from improving_yolov8_cbam_swinblock_amd import ops
    from improving_yolov8_cbam_swinblock_amd.data import augment as DA

    ds = SimpleNamespace(buffer=[0, 1, 2, 3])
    for hyp in (dict(perspective=0.001), dict(copy_paste=0.5)):
        with pytest.raises(NotImplementedError, match="data/augment.py"):
            DA.v8_transforms(ds, 64, hyp)
    with pytest.raises(NotImplementedError, match="data/augment.py"):
        DA.Mosaic(ds, 64, n=9)
    with pytest.raises(NotImplementedError, match="data/augment.py"):
        DA.RandomFlip(flip_idx=[1, 0])
    with pytest.raises(NotImplementedError, match="data/augment.py"):
        DA.v8_transforms(SimpleNamespace(buffer=[0], use_keypoints=True), 64, {})
    with pytest.raises(NotImplementedError, match="data/augment.py"):
        random.seed(0)
        DA.v8_transforms(ds, 64, dict(mixup=1.0))()
    with pytest.raises(NotImplementedError, match="data/augment.py"):
        ops.affine_matrix((128, 128), (-32, -32), dict(perspective=(1e-4, 0.0), angle=0.0, scale=1.0, shear=(0.0, 0.0), translate=(0.5, 0.5)))


@pytest.mark.parametrize("name", NAMES)
def test_the_inverse_matrix_inverts(name):
    """ops.invert_affine and the restatement's copy share their order of operations (warpAffine's, as recalled); independent of that order,
    A composed with M must be the identity: [A | b] applied after [M | t], in float64, to 1e-12 of the entries' magnitude (a 2 x 2 inverse in
    double is good to a few ulp of its entries: 4 ulp of 2 is 2e-15 for the linear part; the offset, products with |t| <= 128, to 128 x that)."""
    from improving_yolov8_cbam_swinblock_amd import ops

    g = case_geometry(name)
    M = np.asarray(g["M"], dtype=np.float64)[:2]
    A = np.asarray(ops.invert_affine(M), dtype=np.float64).reshape(2, 3)
    lin = A[:, :2] @ M[:, :2]
    off = A[:, :2] @ M[:, 2] + A[:, 2]
    assert np.abs(lin - np.eye(2)).max() <= 1e-14 and np.abs(off).max() <= 1e-12, (lin, off)
