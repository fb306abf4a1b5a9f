"""GPU: the first-layer kernels (csrc/first_conv.hip) and ymi_bn_finalize / ymi_bn_finalize_pair (csrc/elementwise.hip) element by element
through the C entry points, against the float64 references and derived bounds of tests/first_conv_exact.py (its docstring states every
bound; tests/test_host_first_conv_check.py shows that the checkers catch what the tensor-wide gates accept).

Which case covers what (shape = n x h x w of the image; a tile is 8 x 64 outputs = 16 x 128 inputs):
  3 x 8 x 8        smaller than a tile: every halo outside the image, three one-tile images
  1 x 16 x 128     exactly one tile (with c = 4: the fourth-channel path of the image copy)
  2 x 18 x 132     2 x 2 tiles per image: the last tile row holds one output row, the last tile column two pixels; left halo from the
                   neighbouring tile, top halo from the tile above, an image boundary between the two images; 8 tiles = two full
                   weight-gradient workgroups
  1 x 34 x 188     3 x 2 tiles, the last tile column 30 pixels wide (it ends inside a 16-pixel group); the second weight-gradient workgroup holds two tiles
  1 x 16 x 640     5 tiles in a row; the second weight-gradient workgroup holds one
  1100 x 2 x 4     1100 tiles of one output row: ymi_bn_finalize takes its staged path (> 1024 partial rows) through the real entry
                   point, the backward sums 1100 partial rows and runs 275 weight-gradient workgroups
  operands         "int" (Gate 1: raw an exact integer, partial rows bit for bit) on every shape; "dyadic" (raw exact AND rounded) on
                   three; "pos" (Gate 2: float32 accumulation of positive reals, two candidates) on multi-tile shapes
  cout, c          16 / 32 / 48 / 64 and 1 / 2 / 3 / 4 each with a multi-tile shape (asserted in test_host_first_conv_check.py)
  activation       none and SiLU on every case; backward also with gamma / beta null, by both routes (own slab sum, deferred record)
Sentinels and guard rows are those of tests/test_gpu_dwconv.py."""
import ctypes

import pytest
import torch

import first_conv_exact as X
from test_gpu_dwconv import EINVAL, EWORKSPACE, GUARD, SENTINEL, _L, _p, _stream, _tensor, _untouched, _y

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
WS_BYTE = 0x5A


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------------------ the forward
def run_forward(case, act, out_wide=False, ws_fill=SENTINEL, short=0, **change):
    """ymi_first_conv_bn_act_fwd on the case's operands -> (rc, outputs, buffers).  x4, out, the statistics and the workspace (GUARD floats
    longer than the entry point asks for) hold a sentinel before the call.  change: img / x4 / out / act / c / cout replaced (refusals)."""
    _, L = _L()
    n, c, h, w, co = case.n, case.c, case.h, case.w, case.cout
    ho, wo = h // 2, w // 2
    img, wt = change.get("img", case.img.to(DEV)), case.wt.to(DEV)
    gam, bet, rm, rv = case.gamma.to(DEV), case.beta.to(DEV), case.rm0.to(DEV), case.rv0.to(DEV)
    x4b, x4 = _tensor(n, 4, h, w, BF)
    ob, out = _tensor(n, co, ho, wo, BF, None, ld=2 * co if out_wide else None)
    x4b, x4 = change.get("x4", (x4b, x4))
    ob, out = change.get("out", (ob, out))
    stats = torch.full((2, co + GUARD), SENTINEL, device=DEV)
    need = X.fwd_workspace_floats(n, h, w, co)
    ws = torch.full((need + GUARD,), ws_fill, device=DEV)
    rc = L.ymi_first_conv_bn_act_fwd(_p(img), n, change.get("c", c), h, w, _p(wt), change.get("cout", co), _p(gam), _p(bet), _p(rm), _p(rv), X.MOMENTUM, X.EPS,
                                     change.get("act", act), _y(x4), _y(out), _p(stats[0]), _p(stats[1]), _p(ws), need * 4 - short, _stream())
    torch.cuda.synchronize()
    units = case.geo["units"]
    got = {"partials": ws[2 * co : 2 * co + units * 2 * co].view(units, 2, co), "save_mean": stats[0, :co], "save_invstd": stats[1, :co], "running_mean": rm, "running_var": rv,
           "out": out, "x4": x4}
    return rc, got, {"x4": x4b, "out": ob, "stats": stats, "ws": ws, "need": need}


def forward_untouched(case, buf):
    """guard rows, foreign channels, the statistics' guard words and the workspace beyond the size the entry point asked for"""
    n, h, w, co = case.n, case.h, case.w, case.cout
    assert _untouched(buf["out"], n * (h // 2) * (w // 2), 0, co), "out: guard rows or foreign channels written"
    assert bool((buf["x4"][n * h * w :] == SENTINEL).all()), "x4: guard rows written"
    assert bool((buf["stats"][:, co:] == SENTINEL).all()), "save_mean / save_invstd: written beyond cout"
    assert bool((buf["ws"][buf["need"] :] == SENTINEL).all()), "workspace written beyond the size asked for"


def x4_expected(case):
    want = torch.zeros(case.n, 4, case.h, case.w, dtype=BF)
    want[:, : case.c] = case.x.to(BF)
    return want


FWD = [(s, a) for s in X.CASES for a in (X.ACT_NONE, X.ACT_SILU)]
FWD_IDS = [f"{X.case_id(s)}-{'silu' if a else 'none'}" for s, a in FWD]


@pytest.mark.parametrize("spec,act", FWD, ids=FWD_IDS)
def test_forward_every_element(spec, act):
    """partial rows, saved and running statistics, every element of out and of the image copy; nothing else written"""
    case = X.case_of(spec)
    rc, got, buf = run_forward(case, act)
    assert rc == 0, _L()[1].ymi_last_error()
    assert _same_bits(got["x4"].cpu(), x4_expected(case)), "x4 is not the image rounded to bfloat16 with zero padding channels"
    ratios = X.check_forward(f"{case} act {act}", {k: v for k, v in got.items() if k != "x4"}, case, act)
    print(f"\n[first conv forward] {case} act {act}: error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    forward_untouched(case, buf)


LAYOUT = [("int", "2x2", 2, 48), ("dyadic", "3x2", 2, 32), ("pos", "5", 1, 16), ("int", "5", 3, 64)]


@pytest.mark.parametrize("spec", LAYOUT, ids=X.case_id)
def test_forward_into_a_channel_slice_and_twice(spec):
    """out as channels [0, cout) of a buffer with ld = 2 cout: the same bits, foreign channels and guard rows untouched.  A second run on a
    workspace full of NaN gives the same bits in every output: nothing depends on what a run finds there."""
    case = X.case_of(spec)
    rc, a, _ = run_forward(case, X.ACT_SILU)
    rc2, b, buf = run_forward(case, X.ACT_SILU, out_wide=True, ws_fill=float("nan"))
    assert rc == 0 and rc2 == 0, _L()[1].ymi_last_error()
    for k in a:
        assert _same_bits(a[k], b[k]), k
    n, h, w, co = case.n, case.h, case.w, case.cout
    assert _untouched(buf["out"], n * (h // 2) * (w // 2), 0, co)
    assert bool(torch.isnan(buf["ws"][buf["need"] :]).all())
    X.check_forward(f"{case} (slice)", {k: v for k, v in b.items() if k != "x4"}, case, X.ACT_SILU)


# ----------------------------------------------------------------------------------------------------------------------------- the backward
def _dout(case, mode):
    """dense; "slice": channels [cout, 2 cout) of a buffer with ld = 2 cout; "off8": a dense tensor whose base lies 4 elements (8 bytes)
    into its allocation -> (buffer, view)"""
    n, co, ho, wo = case.n, case.cout, case.h // 2, case.w // 2
    if mode == "off8":
        flat = torch.full((4 + (n * ho * wo + GUARD) * co,), SENTINEL, dtype=BF, device=DEV)
        v = flat[4 : 4 + n * ho * wo * co].view(n, ho, wo, co).permute(0, 3, 1, 2)
        v.copy_(case.dout.to(BF))
        assert v.data_ptr() % 16 == 8
        return flat, v
    return _tensor(n, co, ho, wo, BF, case.dout, ld=2 * co if mode == "slice" else None, off=co if mode == "slice" else 0)


def run_backward(case, act, affine, deferred, mode="dense", ws_fill=WS_BYTE, short=0, **change):
    lib, L = _L()
    n, c, h, w, co = case.n, case.c, case.h, case.w, case.cout
    stats = change["stats"] if "stats" in change else (lambda r: (r.mean, r.inv))(X.backward_reference(case, act, affine))
    _, x4 = change.get("x4", _tensor(n, 4, h, w, BF, x4_expected(case)))
    _, dout = change.get("dout", _dout(case, mode))
    wt, mean, inv = case.wt.to(DEV), stats[0].to(DEV), stats[1].to(DEV)
    gam, bet = (case.gamma.to(DEV), case.beta.to(DEV)) if affine else (None, None)
    dw = torch.full((co * c * 9 + GUARD,), SENTINEL, device=DEV)
    dgamma, dbeta = torch.full((co + GUARD,), SENTINEL, device=DEV), torch.full((co + GUARD,), SENTINEL, device=DEV)
    need = int(L.ymi_first_conv_bwd_workspace(n, h, w, co))
    ws = torch.full((need + 4 * GUARD,), ws_fill, dtype=torch.uint8, device=DEV)
    rec = lib.WgradPending()
    rc = L.ymi_first_conv_bn_act_bwd(_y(x4), _p(wt), change.get("c", c), co, _p(gam), _p(bet), _p(mean), _p(inv), change.get("act", act), _y(dout), _p(dgamma), _p(dbeta),
                                     _p(dw), _p(ws), need - short, ctypes.byref(rec) if deferred else None, _stream())
    if rc == 0 and deferred:
        table = torch.empty(ctypes.sizeof(lib.WgradPending), dtype=torch.uint8, device=DEV)
        assert L.ymi_wgrad_reduce_batch((lib.WgradPending * 1)(rec), 1, _p(table), _stream()) == 0, L.ymi_last_error()
    torch.cuda.synchronize()
    got = {"dbeta": dbeta[:co], "dgamma": dgamma[:co], "dW": dw[: co * c * 9].view(co, c, 3, 3)}
    return rc, got, {"dw": dw, "dgamma": dgamma, "dbeta": dbeta, "ws": ws, "need": need}


def backward_untouched(case, buf, ws_fill=WS_BYTE):
    co, c = case.cout, case.c
    assert bool((buf["dw"][co * c * 9 :] == SENTINEL).all()) and bool((buf["dgamma"][co:] == SENTINEL).all()) and bool((buf["dbeta"][co:] == SENTINEL).all())
    assert bool((buf["ws"][buf["need"] :] == ws_fill).all()), "workspace written beyond the size asked for"


BWD = [(s, a, f) for s in X.CASES if s[0] != "pos" for a, f in ((X.ACT_SILU, True), (X.ACT_NONE, True), (X.ACT_SILU, False), (X.ACT_NONE, False))]
BWD_IDS = [f"{X.case_id(s)}-{'silu' if a else 'none'}-{'affine' if f else 'null'}" for s, a, f in BWD]


@pytest.mark.parametrize("spec,act,affine", BWD, ids=BWD_IDS)
def test_backward_every_element_by_both_routes(spec, act, affine):
    """dbeta, dgamma and every element of dW against float64, by the entry point's own slab sum and by a deferred record; the routes give
    the same bits"""
    case = X.case_of(spec)
    rc, own, buf = run_backward(case, act, affine, False)
    assert rc == 0, _L()[1].ymi_last_error()
    ratios = X.check_backward(f"{case} act {act} affine {affine}", own, case, act, affine)
    print(f"\n[first conv backward] {case} act {act} affine {affine}: error / bound " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items() if k != "undecided")
          + f"  undecided d(raw) {100 * ratios['undecided']:.3f} %")
    backward_untouched(case, buf)
    rc, rec, buf = run_backward(case, act, affine, True)
    assert rc == 0, _L()[1].ymi_last_error()
    for k in own:
        assert _same_bits(own[k], rec[k]), f"{k}: the two routes differ"
    backward_untouched(case, buf)


@pytest.mark.parametrize("spec", [s for s in LAYOUT if s[0] != "pos"], ids=X.case_id)
def test_backward_dout_layouts_and_twice(spec):
    """dout as channels [cout, 2 cout) of a wider buffer and from a base that is only 8-byte aligned: the same bits as the dense tensor.
    A second run on a workspace of other bytes gives the same bits."""
    case = X.case_of(spec)
    rc, dense, _ = run_backward(case, X.ACT_SILU, True, False)
    assert rc == 0, _L()[1].ymi_last_error()
    for mode, fill in (("slice", WS_BYTE), ("off8", 0xFF), ("dense", 0xFF)):
        rc, got, buf = run_backward(case, X.ACT_SILU, True, False, mode=mode, ws_fill=fill)
        assert rc == 0, _L()[1].ymi_last_error()
        for k in dense:
            assert _same_bits(dense[k], got[k]), (mode, k)
        backward_untouched(case, buf, fill)


# ------------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_a_message_and_launch_nothing():
    _, L = _L()
    base = X.make_case("int", 1, 3, 8, 8, 16)

    def refused(rc, want, buf, what):
        assert rc == want, (what, rc)
        assert b"first_conv" in L.ymi_last_error(), (what, L.ymi_last_error())
        for k in ("x4", "out", "stats", "ws", "dw", "dgamma", "dbeta"):
            if k in buf:
                t = buf[k]
                assert bool((t == (WS_BYTE if t.dtype == torch.uint8 else SENTINEL)).all()), f"{what}: {k} was written"

    def fwd(what, case=base, want=EINVAL, **change):
        rc, _, buf = run_forward(case, change.pop("act", X.ACT_SILU), **change)
        refused(rc, want, buf, what)

    fwd("w % 4 != 0", X.make_case("int", 1, 3, 8, 6, 16))
    fwd("odd h", X.make_case("int", 1, 3, 7, 8, 16))
    fwd("cout = 24", X.make_case("int", 1, 3, 8, 8, 24))
    fwd("c = 5", X.make_case("int", 1, 5, 8, 8, 16))
    fwd("GELU", act=X.ACT_GELU)
    off = torch.zeros(1 * 3 * 8 * 8 + 4, device=DEV)
    fwd("image base off 16 bytes", img=off[1 : 1 + 192].view(1, 3, 8, 8))
    fwd("x4 ld != 4", x4=_tensor(1, 4, 8, 8, BF, None, ld=8))
    fwd("out ld % 8 != 0", out=_tensor(1, 16, 4, 4, BF, None, ld=20))
    fwd("workspace one byte short", want=EWORKSPACE, short=1)

    def bwd(what, case=base, want=EINVAL, **change):
        rc, _, buf = run_backward(case, change.pop("act", X.ACT_SILU), True, False, **change)
        refused(rc, want, buf, what)

    bwd("workspace one byte short", want=EWORKSPACE, short=1)
    plain = lambda co: (torch.zeros(co), torch.ones(co))  # noqa: E731  (save_mean, save_invstd: a refused shape has no reference)
    bwd("w % 4 != 0", X.make_case("int", 1, 3, 8, 6, 16), stats=plain(16))
    bwd("odd h", X.make_case("int", 1, 3, 7, 8, 16), stats=plain(16))
    bwd("cout = 24", X.make_case("int", 1, 3, 8, 8, 24), stats=plain(24))
    bwd("c = 5", c=5)
    bwd("GELU", act=X.ACT_GELU)
    bwd("x4 ld != 4", x4=_tensor(1, 4, 8, 8, BF, torch.zeros(1, 4, 8, 8), ld=8))
    bwd("dout ld % 4 != 0", dout=_tensor(1, 16, 4, 4, BF, torch.zeros(1, 16, 4, 4), ld=18))


# ------------------------------------------------------------------------------------------- ymi_bn_finalize on synthetic partial rows
def _params(C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5, torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5


def run_finalize(rows, count, C, null=(), split=0):
    """ymi_bn_finalize (split > 0: ymi_bn_finalize_pair, the channels >= split on a second parameter set in arrays of its own) on the given
    partial rows, which lie in a buffer of blocks + BN_STAGE_ROWS + GUARD rows of sentinels -> outputs, the float64 reference, the buffer.
    Every parameter array ends in GUARD sentinels: a kernel that ignored the split, or did not rebase the second set, would read them."""
    _, L = _L()
    blocks = rows.shape[0]
    buf = torch.full((blocks + X.BN_STAGE_ROWS + GUARD, 2, C), SENTINEL, device=DEV)
    buf[:blocks] = rows.to(DEV)
    host = dict(zip(("gamma", "beta", "rmean", "rvar"), _params(C, 100 * C + blocks % 97)))
    one, zero = torch.ones(C), torch.zeros(C)
    first = split if split else C
    guarded = lambda v: torch.cat([v, torch.full((GUARD,), SENTINEL)]).to(DEV)  # noqa: E731
    dev = {k: guarded(v[:first]) for k, v in host.items()}
    dev2 = {k: guarded(v[first:]) for k, v in host.items()}
    outs = {k: torch.full((C + GUARD,), SENTINEL, device=DEV) for k in ("scale", "shift", "smean", "sinv")}
    a = lambda k: None if k in null else _p((dev if k in dev else outs)[k])  # noqa: E731
    if split:
        rc = L.ymi_bn_finalize_pair(_p(buf), blocks, count, C, split, a("gamma"), a("beta"), a("rmean"), a("rvar"), _p(dev2["gamma"]), _p(dev2["beta"]), _p(dev2["rmean"]),
                                    _p(dev2["rvar"]), X.MOMENTUM, X.EPS, a("scale"), a("shift"), a("smean"), a("sinv"), _stream())
    else:
        rc = L.ymi_bn_finalize(_p(buf), blocks, count, C, a("gamma"), a("beta"), a("rmean"), a("rvar"), X.MOMENTUM, X.EPS, a("scale"), a("shift"), a("smean"), a("sinv"), _stream())
    torch.cuda.synchronize()
    assert rc == 0, L.ymi_last_error()
    ref = X.finalize_reference(rows, count, one if "gamma" in null else host["gamma"], zero if "beta" in null else host["beta"], host["rmean"], host["rvar"])
    whole = {k: torch.cat([dev[k][:first], dev2[k][: C - first]]) for k in dev}
    got = {"scale": outs["scale"][:C], "shift": outs["shift"][:C]}
    for name, key, store in (("save_mean", "smean", outs), ("save_invstd", "sinv", outs), ("running_mean", "rmean", whole), ("running_var", "rvar", whole)):
        if key in null:  # not written: the array still holds what it held
            assert bool((store[key][:C] == (SENTINEL if store is outs else host[key].to(DEV))).all()), key
        else:
            got[name] = store[key][:C]
    for k in dev:
        assert bool((dev[k][first:] == SENTINEL).all()) and bool((dev2[k][C - first :] == SENTINEL).all()), f"{k}: written beyond its channels"
        if k in ("gamma", "beta"):
            assert torch.equal(whole[k].cpu(), host[k]), f"{k} was changed"
    for k, t in outs.items():
        assert bool((t[C:] == SENTINEL).all()), f"{k}: written beyond C"
    return got, ref, buf


def rows_untouched(buf, rows):
    blocks = rows.shape[0]
    assert _same_bits(buf[:blocks].cpu(), rows), "the caller's partial rows were changed"
    assert bool((buf[blocks + X.BN_STAGE_ROWS :] == SENTINEL).all()), "written beyond row blocks + BN_STAGE_ROWS"
    if blocks <= 16 * X.BN_STAGE_ROWS:  # (no staging pass: nothing at all is written behind the rows)
        assert bool((buf[blocks:] == SENTINEL).all())


@pytest.mark.parametrize("C", X.FIN_CHANNELS)
@pytest.mark.parametrize("blocks", X.FIN_BLOCKS)
def test_finalize_every_branch_of_the_row_walk(blocks, C):
    """integer rows whose sums are exact in every float32 chain: scale, shift, saved and running statistics against the float64 rule"""
    rows, count = X.finalize_rows(blocks, C)
    got, ref, buf = run_finalize(rows, count, C)
    assert set(got) == {"scale", "shift", "save_mean", "save_invstd", "running_mean", "running_var"}
    X.check_finalize(f"finalize {blocks} rows x {C}", got, ref)
    rows_untouched(buf, rows)


@pytest.mark.parametrize("null", ["gamma", "beta", "rmean", "rvar", "smean", "sinv"])
def test_finalize_with_one_pointer_null(null):
    rows, count = X.finalize_rows(33, 48)
    got, ref, buf = run_finalize(rows, count, 48, null=(null,))
    X.check_finalize(f"finalize, {null} null", got, ref)
    rows_untouched(buf, rows)


@pytest.mark.parametrize("blocks", [97, 1088])
def test_finalize_pair_splits_the_parameters(blocks):
    """split = 32 of C = 80: the channels >= 32 read and update the second set, which lies in arrays of its own.  The two sets hold the
    values of one set over all 80 channels, so the result has the bits of the single-set call."""
    rows, count = X.finalize_rows(blocks, 80)
    got, ref, buf = run_finalize(rows, count, 80, split=32)
    X.check_finalize(f"finalize_pair {blocks} rows", got, ref)
    rows_untouched(buf, rows)
    one = run_finalize(rows, count, 80)[0]
    for k in got:
        assert _same_bits(got[k], one[k]), k


def test_finalize_variance_under_cancellation():
    """2048 rows of 512 real pixels, the per-channel mean 30 times the deviation: var = sumsq / count - mean^2 loses 900 to 1 of the relative
    accuracy of its inputs.  The rows are float32 sums of float32 values, as a statistics pass writes them: each within gamma(512) of
    its exact sum in relative terms (gamma(513) for the squares), so var is known to d_var = gamma(514) E[v^2] + 2 |m| d_m + d_m^2,
    d_m = gamma(513) E|v|, which acts on var + mean^2.  The one more rounding in each is the staging pass's (2048 > 1024 rows): it sums
    in double but stores its 64 rows as float32; the final pass and the rule are in double.  Printed: the variance against the data
    and against a float64 finalize of the rows as given (the staging pass's rounding alone, times the 900)."""
    C, R, PX = 16, 2048, 512
    g = torch.Generator().manual_seed(3)
    dev_c = 0.25 + 0.5 * torch.rand(C, generator=g)
    s = torch.zeros(3, C, dtype=torch.float64)
    rows = []
    for _ in range(8):
        v = (dev_c * 30.0 + dev_c * torch.randn(R // 8, PX, C, generator=g)).float()
        rows.append(torch.stack([v.sum(1), (v * v).sum(1)], 1))
        vd = v.double()
        s += torch.stack([vd.sum((0, 1)), (vd * vd).sum((0, 1)), vd.abs().sum((0, 1))])
    rows = torch.cat(rows).contiguous()
    count = R * PX
    got, ref, buf = run_finalize(rows, count, C)
    gam, bet, rm0, rv0 = _params(C, 100 * C + R % 97)  # (run_finalize's parameters)
    m, e2, ea = s[0] / count, s[1] / count, s[2] / count
    var = e2 - m * m
    true = {"save_mean": m, "save_invstd": 1.0 / torch.sqrt(var + X.EPS), "running_mean": (1 - X.MOMENTUM) * rm0.double() + X.MOMENTUM * m,
            "running_var": (1 - X.MOMENTUM) * rv0.double() + X.MOMENTUM * var * count / (count - 1.0)}
    true["scale"] = gam.double() * true["save_invstd"]
    true["shift"] = bet.double() - m * true["scale"]
    d_m = X.gamma(513) * ea
    d_var = X.gamma(514) * e2 + 2 * m.abs() * d_m + d_m * d_m
    assert bool((d_var < 0.5 * var).all())
    d_inv = 0.5 * d_var * (var - d_var + X.EPS) ** -1.5
    d_sc = gam.double().abs() * d_inv
    extra = {"save_mean": d_m, "save_invstd": d_inv, "running_mean": X.MOMENTUM * d_m, "running_var": X.MOMENTUM * d_var * count / (count - 1.0), "scale": d_sc,
             "shift": m.abs() * d_sc + d_m * (true["scale"].abs() + d_sc)}
    var_got = got["save_invstd"].double().cpu() ** -2 - X.EPS  # (the stored float32 inverse deviation: 1.2e-7 of var)
    print(f"\n[finalize cancellation] worst |var - var64| / var {float(((var_got - var).abs() / var).max()):.2e}; derived bound {float((d_var / var).max()):.2e}; "
          f"against the rows as given {float(((var_got - ref['var']).abs() / var).max()):.2e}")
    X.check_finalize("finalize under cancellation, against the data", got, true, extra)
    rows_untouched(buf, rows)
