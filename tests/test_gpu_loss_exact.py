"""The detection loss kernels of csrc/loss.hip, stage by stage, against the float64 restatement of tests/loss_exact.py.

Through the C ABI with buffers this file owns: ymi_detect_targets, ymi_detect_loss_fwd_assign (with gidx_out and out_scale, and without
either), ymi_detect_loss_bwd (with grad_scale and without), ymi_detect_decode / ymi_detect_decode_seg.  State and workspace are filled with
0xFF bytes before the call (the two int32 buffers in which -1 is a value: with 0x7F) and sliced into named views by the restated layouts
(loss_exact.carve_state / carve_work, whose totals must equal ymi_detect_loss_sizes).

  every word written   no poison in any stage view, every byte outside them still poison; class-gradient padding channels (dcw = nc rounded
                       up to 8) exactly 0; sentinel channels of channel-sliced maps (ld > c) and guard rows behind every buffer untouched
  discrete stages      mpos, gidx (workspace and gidx_out), lab and the zero pattern of wgt equal the restatement
  continuous stages    worst |err| / (|ref| + max |ref| of the stage) against float64, no floor.  Bound: 8 times the distance of the float32
                       oracle (oracle/loss.py on the CPU) from float64, measured per stage over the guarded cases by
                       tests/test_host_loss_check.py; 8 for another summation order plus the kernels' __expf / __logf / powf / atanf,
                       which the host oracle does not use.
                           stage     oracle     bound    |  stage    oracle     bound
                           targets   3.7e-8    3.0e-7    |  wgt      8.4e-7    6.7e-6
                           pb        9.1e-8    7.3e-7    |  tss      7.1e-7    5.7e-6
                           ov        3.2e-7    2.6e-6    |  loss     3.1e-8    2.5e-7   (the three items, out_scale null)
                           al        8.2e-7    6.6e-6    |  loss6    3.1e-8    2.5e-7   (the six scaled outputs)
                           pa        5.1e-7    4.1e-6    |  dbox     8.2e-7    6.6e-6
                           po        9.9e-8    7.9e-7    |  dcls     2.4e-7    1.9e-6
                           tgt       3.7e-8    3.0e-7    |
                       Worst kernel figures when this was written (float32 maps, every case): targets 3.6e-8, pb 9.4e-8, ov 6.8e-7, al 1.2e-6,
                       pa 1.2e-6, po 2.0e-7, tgt 3.6e-8, wgt 1.4e-6, tss 8.0e-7, loss and loss6 1.9e-7 (long_row), dbox 2.5e-6, dcls 4.9e-7.
  bfloat16 maps        the restatement is fed the same bf16-rounded maps and the kernel's own assignment; the forward stages are float32
                       either way and keep their bounds; stored gradients add their one rounding, 2^-8 |ref|
  gradients            grad_loss = (0.7, -1.3, 2.1), with grad_scale and with it null
  determinism          two runs bit-equal
  decode               ymi_detect_decode and ymi_detect_decode_seg (nm = 3, 32) on rect and four_levels: box rows at pb's bound; scores within
                       four float32 roundings of the element (exp, add, divide, store: 4 * 2^-24); coefficient rows copied exactly; the rows a
                       run without coefficients has (nm = 0) bit-equal to ymi_detect_decode"""
import ctypes

import pytest
import torch

import loss_exact as X

pytestmark = pytest.mark.gpu

F32, BF = torch.float32, torch.bfloat16
SENTINEL = -768.0  # (exact in bfloat16)
GUARD_ROWS = 3
CONT_FWD = ("targets", "pb", "ov", "al", "pa", "po", "tgt", "wgt", "tss")
CASE_DTYPES = [(n, dt) for n in X.CASES for dt in (F32, BF) if not (n == "long_row" and dt == BF)]
IDS = [f"{n}-{'bf16' if dt == BF else 'f32'}" for n, dt in CASE_DTYPES]


def bound(stage):
    return X.KERNEL_FACTOR * X.ORACLE_DISTANCE[stage]


def dev():
    return torch.device("cuda:0")


def L():
    from improving_yolov8_cbam_swinblock_amd import _lib

    return _lib


def tensor_arg(buf, c0, c):
    """channels [c0, c0 + c) of an NHWC buffer [B, H, W, ld] (guard rows may follow) as the library's tensor"""
    B, H, W, ld = buf.shape
    return L().YmiTensor(buf.data_ptr() + c0 * buf.element_size(), B, H, W, c, ld, L().ymi_dtype(buf.dtype), 0)


def arr(ts):
    return (L().YmiTensor * len(ts))(*ts)


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Maps:
    """per level one NHWC buffer [B, H, W, ld] of `dtype` plus GUARD_ROWS pixel rows behind it, everything SENTINEL; named channel ranges"""

    def __init__(self, inp, dtype, ranges, ld):
        self.inp, self.ranges, self.ld = inp, ranges, ld
        self.flat, self.bufs = [], []
        for H, W in inp["levels"]:
            f = torch.full(((inp["B"] * H * W + GUARD_ROWS) * ld,), SENTINEL, dtype=dtype, device=dev())
            self.flat.append(f)
            self.bufs.append(f[: inp["B"] * H * W * ld].view(inp["B"], H, W, ld))

    def fill(self, name, values):
        c0, c = self.ranges[name]
        for b, v in zip(self.bufs, values):
            b[..., c0: c0 + c] = v.to(device=dev(), dtype=b.dtype)

    def args(self, name, c=None):
        c0, cw = self.ranges[name]
        return arr([tensor_arg(b, c0, c or cw) for b in self.bufs])

    def get(self, name):
        c0, c = self.ranges[name]
        return [b[..., c0: c0 + c].cpu() for b in self.bufs]

    def untouched(self):
        """everything outside the named channel ranges, guard rows included, still SENTINEL"""
        for f, b in zip(self.flat, self.bufs):
            keep = torch.ones(self.ld, dtype=torch.bool)
            for c0, c in self.ranges.values():
                keep[c0: c0 + c] = False
            if not (b.cpu()[..., keep] == SENTINEL).all() or not (f[b.numel():].cpu() == SENTINEL).all():
                return False
        return True


def poisoned(nbytes, guard=256):
    return torch.full((nbytes + guard,), 0xFF, dtype=torch.uint8, device=dev())


_runs = {}


def run(name, dtype, sliced=False, plain=False, again=0):
    """one forward and backward of a case -> every buffer on the CPU.  plain: no gidx_out, no out_scale, no grad_scale.  sliced: box and class
    maps are channel ranges of one wider buffer per level, and so are the gradient maps."""
    key = (name, dtype, sliced, plain, again)
    if key in _runs:
        return _runs[key]
    lib = L().lib()
    inp = X.build(name)
    B, nc, G, A, nl = inp["B"], inp["nc"], inp["G"], inp["A"], len(inp["levels"])
    dcw = (nc + 7) // 8 * 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if sliced:
        ld = (4 * X.REG + nc + 5 + 7) // 8 * 8
        maps = Maps(inp, dtype, {"box": (0, 4 * X.REG), "cls": (4 * X.REG, nc)}, ld)
        gmaps = Maps(inp, dtype, {"dbox": (0, 4 * X.REG), "dcls": (4 * X.REG, dcw)}, 4 * X.REG + dcw + 8)
        box_m = cls_m = maps
        dbox_m = dcls_m = gmaps
    else:
        box_m, cls_m = Maps(inp, dtype, {"box": (0, 4 * X.REG)}, 4 * X.REG), Maps(inp, dtype, {"cls": (0, nc)}, nc)
        dbox_m, dcls_m = Maps(inp, dtype, {"dbox": (0, 4 * X.REG)}, 4 * X.REG), Maps(inp, dtype, {"dcls": (0, dcw)}, dcw)
    box_m.fill("box", inp["box"])
    cls_m.fill("cls", inp["cls"])
    strides = (ctypes.c_float * nl)(*inp["strides"])

    # dense targets
    n = int(inp["batch_idx"].numel())
    bi, cl, bb = (t.to(dev()).contiguous() if n else None for t in (inp["batch_idx"], inp["labels"], inp["bboxes"]))
    targets = poisoned(B * G * 5 * 4)
    L().check(lib.ymi_detect_targets(p(bi), p(cl), p(bb), n, B, G, inp["img_w"], inp["img_h"], p(targets), stream), "detect_targets")

    # forward
    sb, wb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    L().check(lib.ymi_detect_loss_sizes(B, A, G, ctypes.byref(sb), ctypes.byref(wb)), "detect_loss_sizes")
    (slay, stot), (wlay, wtot) = X.carve_state(B, A), X.carve_work(B, A, G)
    assert (stot, wtot) == (sb.value, wb.value), "the restated layouts no longer give the library's sizes"
    state, work = poisoned(stot), poisoned(wtot)
    X.views(state, slay)["lab"].fill_(0x7F7F7F7F)  # (-1 is a value of lab and gidx: their poison is another pattern)
    X.views(work, wlay)["gidx"].fill_(0x7F7F7F7F)
    gidx_out = None if plain else torch.full((B * A + 64,), 0x7F7F7F7F, dtype=torch.int32, device=dev())
    scale6 = None if plain else torch.tensor(X.out_scale(B), dtype=F32, device=dev())
    loss_out = poisoned(6 * 4)
    L().check(lib.ymi_detect_loss_fwd_assign(nl, box_m.args("box"), cls_m.args("cls"), strides, p(targets), G, X.TOPK, X.ALPHA, X.BETA, p(scale6),
                                             p(loss_out), p(state), stot, p(work), wtot, p(gidx_out), stream), "detect_loss_fwd_assign")
    # backward
    gl = torch.tensor(X.GRAD_LOSS, dtype=F32, device=dev())
    L().check(lib.ymi_detect_loss_bwd(nl, box_m.args("box"), cls_m.args("cls"), strides, p(state), stot, p(gl), None if plain else p(scale6),
                                      dbox_m.args("dbox"), dcls_m.args("dcls"), stream), "detect_loss_bwd")
    torch.cuda.synchronize()

    out = dict(inp=inp, dcw=dcw, slay=slay, wlay=wlay, state=state.cpu(), work=work.cpu(), targets_raw=targets.cpu(), loss_raw=loss_out.cpu(),
               gidx_out=None if plain else gidx_out.cpu(), dbox=dbox_m.get("dbox"), dcls=dcls_m.get("dcls"),
               maps_untouched=box_m.untouched() and cls_m.untouched(), grads_untouched=dbox_m.untouched() and dcls_m.untouched(),
               box=[t.float() for t in box_m.get("box")], cls=[t.float() for t in cls_m.get("cls")])
    sv, wv = X.views(out["state"], slay), X.views(out["work"], wlay)
    wr = X.written(B, A)
    out.update(targets=out["targets_raw"][: B * G * 20].view(F32).view(B, G, 5), pb=wv["pb"].view(B, A, 4), ov=wv["ov"].view(B, G, A), al=wv["al"].view(B, G, A),
               mpos=wv["mpos"].view(B, G, A), gidx_work=wv["gidx"].view(B, A), pa=wv["pa"].view(B, G), po=wv["po"].view(B, G), tss_part=wv["tss_part"][: wr["tss_part"]],
               part=wv["part"][: wr["part"]], tgt=sv["tgt"].view(B, A, 4), wgt=sv["wgt"].view(B, A), lab=sv["lab"].view(B, A), tss=sv["scal"][:1],
               loss_out=out["loss_raw"][:24].view(F32))
    out["gidx"] = out["gidx_work"] if plain else out["gidx_out"][: B * A].view(B, A)
    _runs[key] = out
    return out


_refs = {}


def reference(name, dtype, plain=False):
    """the restatement of a run: float32 maps as they are and its own assignment; bfloat16: the rounded maps and the kernel's assignment"""
    key = (name, dtype, plain)
    if key not in _refs:
        o = run(name, dtype)
        kw = dict(grad_scale=None if plain else X.out_scale(o["inp"]["B"])[:3])
        if dtype == BF:
            kw.update(box=o["box"], cls=o["cls"], mpos=o["mpos"].bool(), gidx=o["gidx"].long())
        _refs[key] = X.restate(o["inp"], **kw)
    return _refs[key]


def flat(ts):
    return torch.cat([t.reshape(-1) for t in ts]) if isinstance(ts, (list, tuple)) else ts


def check_stage(what, got, ref, bnd, stored_rel=0.0):
    """worst |err| / (bnd * (|ref| + max |ref|) + stored_rel * |ref|) <= 1; prints the figure in the scale of the bound"""
    got, ref = flat(got).double().reshape(-1), flat(ref).double().reshape(-1)
    e = X.scaled_err(got, ref)
    big = float(ref.abs().max()) if ref.numel() else 0.0
    allowed = bnd * (ref.abs() + big) + stored_rel * ref.abs()
    ok = bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= allowed).all())
    print(f"  {what}: |err| / (|ref| + max |ref|) = {e:.3e}  (bound {bnd:.1e}{f' + {stored_rel:.1e} |ref|' if stored_rel else ''})  {'ok' if ok else 'EXCEEDS'}")
    return ok


# ------------------------------------------------------------------------------------------------------------------------ every word written
@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_every_stage_word_is_written_and_nothing_else(name, dtype):
    for plain in (False, True):
        o = run(name, dtype, plain=plain)
        B, A, G = o["inp"]["B"], o["inp"]["A"], o["inp"]["G"]
        wr = X.written(B, A)
        for buf, lay in ((o["state"], o["slay"]), (o["work"], o["wlay"])):
            outside = torch.ones(buf.numel(), dtype=torch.bool)
            for stage, (off, dt, n) in lay.items():
                n = wr.get(stage, n)
                if stage == "gidx" and not plain:
                    n = 0  # (handed to gidx_out: the workspace's buffer stays as it was)
                nb = n * torch.empty((), dtype=dt).element_size()
                view = buf[off: off + nb]
                outside[off: off + nb] = False
                if stage in ("lab", "gidx"):
                    assert not (view.view(torch.int32) == 0x7F7F7F7F).any(), (stage, plain)
                elif stage == "mpos":
                    assert (view <= 1).all(), (stage, plain)
                else:
                    assert torch.isfinite(view.view(F32)).all(), (stage, plain)
            if lay is o["wlay"] and not plain:
                off, _, n = lay["gidx"]
                assert (buf[off: off + 4 * n] == 0x7F).all()
                outside[off: off + 4 * n] = False
            assert (buf[outside] == 0xFF).all(), plain  # (the 256 guard bytes behind the buffer included)
        assert torch.isfinite(o["targets"]).all() and (o["targets_raw"][B * G * 20:] == 0xFF).all()
        k = 3 if plain else 6
        assert torch.isfinite(o["loss_out"][:k]).all() and (o["loss_raw"][4 * k:] == 0xFF).all()
        if not plain:
            assert not (o["gidx_out"][: B * A] == 0x7F7F7F7F).any() and (o["gidx_out"][B * A:] == 0x7F7F7F7F).all()


@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_gradient_maps_padding_zero_sentinels_and_guard_rows_untouched(name, dtype):
    for kw in (dict(), dict(sliced=True)):
        o = run(name, dtype, **kw)
        nc = o["inp"]["nc"]
        assert o["maps_untouched"] and o["grads_untouched"], kw
        for g in o["dcls"]:
            assert g.shape[-1] == o["dcw"] and not g[..., nc:].any(), kw
        assert all(torch.isfinite(g.float()).all() for g in o["dbox"] + o["dcls"])
        bg = (o["lab"] < 0)
        x = torch.cat([g.float().reshape(o["inp"]["B"], -1, 4 * X.REG) for g in o["dbox"]], 1)
        assert not x[bg].any()  # background anchors: box gradients exactly zero


# --------------------------------------------------------------------------------------------------------------------------- discrete stages
@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_discrete_stages_equal_the_restatement(name, dtype):
    o, r = run(name, dtype), reference(name, dtype)
    if dtype == BF:  # (informative: the assignment itself is the kernel's here)
        free = X.restate(o["inp"], box=o["box"], cls=o["cls"])
        print(f"  bf16 maps: {int((free['mpos'] != o['mpos'].bool()).sum())} mpos and {int((free['gidx'] != o['gidx'].long()).sum())} gidx elements differ "
              "from the float64 assignment on the same maps")
    assert torch.equal(o["mpos"].bool(), r["mpos"]), (o["mpos"].bool() != r["mpos"]).nonzero().tolist()[:10]
    assert torch.equal(o["gidx"].long(), r["gidx"]), (o["gidx"].long() != r["gidx"]).nonzero().tolist()[:10]
    assert torch.equal(o["lab"].long(), r["lab"]), (o["lab"].long() != r["lab"]).nonzero().tolist()[:10]
    assert torch.equal(o["wgt"] == 0, r["wgt"] == 0)
    plain = run(name, dtype, plain=True)
    assert torch.equal(plain["gidx_work"], o["gidx"]) and torch.equal(plain["mpos"], o["mpos"]) and torch.equal(plain["lab"], o["lab"])


# ------------------------------------------------------------------------------------------------------------------------- continuous stages
@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_continuous_stages_against_float64(name, dtype):
    o, r, plain = run(name, dtype), reference(name, dtype), run(name, dtype, plain=True)
    print(f"[{name} {dtype}]")
    ok = [check_stage(s, o[s], r[s], bound(s)) for s in CONT_FWD]
    ok.append(check_stage("loss (three items)", plain["loss_out"][:3], r["loss"], bound("loss")))
    ok.append(check_stage("loss6 (six scaled)", o["loss_out"], r["loss6"], bound("loss6")))
    for s in CONT_FWD:  # the forward does not depend on where gidx goes or on out_scale
        assert torch.equal(plain[s], o[s]), s
    if name == "no_labels":
        assert float(o["tss"]) == 0.0 and float(o["loss_out"][0]) == 0.0 and float(o["loss_out"][2]) == 0.0
    assert all(ok)


@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_gradients_against_float64_with_and_without_grad_scale(name, dtype):
    stored = 2.0 ** -8 if dtype == BF else 0.0
    print(f"[{name} {dtype}]")
    ok = []
    for plain in (False, True):
        o, r = run(name, dtype, plain=plain), reference(name, dtype, plain=plain)
        nc = o["inp"]["nc"]
        tag = "grad_scale null" if plain else "grad_scale given"
        ok.append(check_stage(f"dbox ({tag})", [g.float() for g in o["dbox"]], r["dbox"], bound("dbox"), stored))
        ok.append(check_stage(f"dcls ({tag})", [g.float()[..., :nc] for g in o["dcls"]], r["dcls"], bound("dcls"), stored))
    assert all(ok)


# ------------------------------------------------------------------------------------------------------------- channel slices, determinism
BITWISE = CONT_FWD + ("mpos", "gidx", "lab", "loss_out", "tss_part", "part")


@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_channel_sliced_maps_give_the_same_bits(name, dtype):
    a, b = run(name, dtype), run(name, dtype, sliced=True)
    assert b["maps_untouched"] and b["grads_untouched"]
    for s in BITWISE:
        assert torch.equal(a[s], b[s]), s
    for s in ("dbox", "dcls"):
        assert all(torch.equal(x, y) for x, y in zip(a[s], b[s])), s


@pytest.mark.parametrize("name,dtype", CASE_DTYPES, ids=IDS)
def test_two_runs_are_bit_equal(name, dtype):
    a, b = run(name, dtype), run(name, dtype, again=1)
    for s in BITWISE:
        assert torch.equal(a[s], b[s]), s
    for s in ("dbox", "dcls"):
        assert all(torch.equal(x, y) for x, y in zip(a[s], b[s])), s


# ------------------------------------------------------------------------------------------------------------------------------------ decode
SCORE_BOUND = 4 * 2.0 ** -24


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["rect", "four_levels"])
def test_inference_decode_against_float64(name, dtype):
    lib = L().lib()
    inp = X.build(name)
    B, nc, A, nl = inp["B"], inp["nc"], inp["A"], len(inp["levels"])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    strides = (ctypes.c_float * nl)(*inp["strides"])
    ld = (4 * X.REG + nc + 5 + 7) // 8 * 8
    maps = Maps(inp, dtype, {"box": (0, 4 * X.REG), "cls": (4 * X.REG, nc)}, ld)
    maps.fill("box", inp["box"])
    maps.fill("cls", inp["cls"])
    box, cls = [t.float() for t in maps.get("box")], [t.float() for t in maps.get("cls")]

    def decoded(nm):
        y = poisoned(B * (4 + nc + nm) * A * 4)
        if nm:
            gen = torch.Generator().manual_seed(nm)
            mc = Maps(inp, dtype, {"mc": (0, nm)}, nm)
            mc.fill("mc", [torch.randn(B, H, W, nm, generator=gen) for H, W in inp["levels"]])
            L().check(lib.ymi_detect_decode_seg(nl, maps.args("box"), maps.args("cls"), mc.args("mc"), strides, p(y), stream), "detect_decode_seg")
        else:
            mc = None
            L().check(lib.ymi_detect_decode(nl, maps.args("box"), maps.args("cls"), strides, p(y), stream), "detect_decode")
        torch.cuda.synchronize()
        y = y.cpu()
        assert (y[B * (4 + nc + nm) * A * 4:] == 0xFF).all() and maps.untouched() and (mc is None or mc.untouched())
        return y[: B * (4 + nc + nm) * A * 4].view(F32).view(B, 4 + nc + nm, A), [t.float() for t in mc.get("mc")] if mc else None

    plain, _ = decoded(0)
    ref = X.decode(inp, box=box, cls=cls)
    print(f"[{name} {dtype}]")
    assert check_stage("box rows", plain[:, :4], ref[:, :4], bound("pb")) & check_stage("score rows", plain[:, 4:], ref[:, 4:], SCORE_BOUND)
    for nm in (3, 32):
        y, mc = decoded(nm)
        assert torch.equal(y[:, : 4 + nc], plain), nm  # the rows a run without coefficients has
        want = X.decode(inp, box=box, cls=cls, mc=mc)[:, 4 + nc:]
        assert torch.equal(y[:, 4 + nc:].double(), want), nm  # coefficients: copied as they are
