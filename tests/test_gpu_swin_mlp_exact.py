"""GPU: the fused SwinBlock MLP kernels of csrc/swin_mlp.hip checked element by element (tests/swin_mlp_exact.py), through the C ABI
(ymi_swin_ln_mlp_pack / _fwd / _bwd_data) at all three widths.

The case list is swin_mlp_exact.case_list: hidden of 1, 2, 3, 4 and 7 chunks (no second prologue issue; prologue only; the first in-loop issue;
the ring wraps onto stage 0; a second wrap with an odd count), the model's 4 C, and the width's cap at T = 33 (the full LDS opt-in); T = 1, 31
(one partial wave), 33 (a wave with one token), BM and 2 BM (no padding rows), BM + 1 (a workgroup that owns one token), 421 (a partial wave
inside a later workgroup); dense rows and ld = C + 8 for x / u / out / dout / du.  Every case runs Gate 1 (every stored value bit for bit on
constructed operands, the post the backward writes included) and Gate 2 (a per-element float64 bound per stage on N(0, 1)-scaled operands
and on a x3 variant of x).  Every output buffer is filled with a sentinel first: pad columns, guard rows, and everything behind the rows a
launch owns in the pre / post / d_pre buffers must keep it.  The evaluation forward gives a bit-equal out, each form run twice gives
bit-identical results, and the packed weight images equal the host mirror bit for bit.

One line per case: width, T, hidden, row stride, worst error / bound per stage."""
import ctypes
import functools

import pytest
import torch

import swin_mlp_exact as X

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GUARD = 8  # sentinel rows behind row T of every row-major output
GUARD_ELEMS = 4096  # sentinel elements behind the pre / post / d_pre buffers
SENTINEL = -1984.0  # (exact in bfloat16; no value here comes near it)
CASES = [(c, cs) for c in X.WIDTHS for cs in X.case_list(c)]
IDS = [f"C{c}-T{cs.t}-h{cs.hidden}-{'ld+8' if cs.strided else 'dense'}" for c, cs in CASES]


def _lib():
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    return L, L.lib()


def _dev():
    return torch.device("cuda:0")


def _rows(t, c, ld, fill):
    buf = torch.full((t + GUARD, ld), fill, dtype=BF, device=_dev())
    return buf, buf[:t, :c]


def _flat(n):
    return torch.full((n + GUARD_ELEMS,), SENTINEL, dtype=BF, device=_dev())


def _kept(buf, t, c):
    """the guard rows, and the pad columns of the rows in use, still hold the sentinel"""
    return bool((buf[t:] == SENTINEL).all()) and bool((buf[:t, c:] == SENTINEL).all())


def _forward(L, lib, k, train):
    c, t, hidden = k["c"], k["t"], k["hidden"]
    obuf, out = _rows(t, c, k["ld"], SENTINEL)
    r = dict(obuf=obuf, out=out)
    if train:
        r["ubuf"], r["u"] = _rows(t, c, k["ld"], SENTINEL)
        r["stats"] = torch.full((2, t + GUARD), float("nan"), dtype=torch.float32, device=_dev())
        r["pre"] = _flat(k["cap"])
    L.check(
        lib.ymi_swin_ln_mlp_fwd(ctypes.byref(L.as_ymi(k["x"])), L.ptr(k["gamma"]), L.ptr(k["beta"]), k["eps"], L.ptr(k["packed"]), L.ptr(k["b1"]), L.ptr(k["b2"]), hidden,
                                ctypes.byref(L.as_ymi(r["u"])) if train else None, L.ptr(r["stats"][0]) if train else None, L.ptr(r["stats"][1]) if train else None,
                                L.ptr(r["pre"]) if train else None, ctypes.byref(L.as_ymi(out)), L.stream_ptr()),
        "swin_ln_mlp_fwd",
    )
    torch.cuda.synchronize()
    return r


def _backward(L, lib, k, pre):
    c, t, hidden = k["c"], k["t"], k["hidden"]
    r = dict(postbuf=_flat(k["cap"]), dprebuf=_flat(k["cap"]))
    r["post"] = r["postbuf"][: k["cap"]].view(-1, hidden)[:t]
    r["dpre"] = r["dprebuf"][: k["cap"]].view(-1, hidden)[:t]
    r["dubuf"], r["du"] = _rows(t, c, k["ld"], SENTINEL)
    L.check(lib.ymi_swin_ln_mlp_bwd_data(ctypes.byref(L.as_ymi(k["dout"])), L.ptr(k["packed"]), L.ptr(pre), hidden, ctypes.byref(L.as_ymi(r["post"])),
                                         ctypes.byref(L.as_ymi(r["dpre"])), ctypes.byref(L.as_ymi(r["du"])), L.stream_ptr()), "swin_ln_mlp_bwd_data")
    torch.cuda.synchronize()
    return r


@functools.lru_cache(maxsize=None)
def _run(c, t, hidden, strided, kind):
    """one case's operands (kind: 'gate1', 'real' or 'real3') on the device, the training forward and the backward run twice each, the
    evaluation forward once: computed once, shared by the tests of the case, never modified"""
    L, lib = _lib()
    o = X.gate1_operands(c, t, hidden) if kind == "gate1" else X.real_operands(c, t, hidden, 3.0 if kind == "real3" else 1.0)
    o = X.to_device(o, _dev())
    ld = c + 8 if strided else c
    assert lib.ymi_swin_ln_mlp_supported(c, hidden, L.YMI_BF16) and X.supported(c, hidden)
    cap = lib.ymi_swin_ln_mlp_pre_elems(t, hidden)
    assert cap == X.pre_elems(t, hidden) and lib.ymi_swin_ln_mlp_pack_elems(c, hidden) == X.pack_elems(c, hidden)
    k = dict(c=c, t=t, hidden=hidden, ld=ld, cap=cap, eps=o["eps"], o=o)
    for n in ("gamma", "beta", "b1", "b2"):
        k[n] = o[n].contiguous()
    _, k["x"] = _rows(t, c, ld, 0.0)
    k["x"].copy_(o["x"])
    _, k["dout"] = _rows(t, c, ld, 0.0)
    k["dout"].copy_(o["dout"])
    packed = _flat(X.pack_elems(c, hidden))
    L.check(lib.ymi_swin_ln_mlp_pack(L.ptr(o["w1"]), L.ptr(o["w2"]), c, hidden, L.ptr(packed), L.stream_ptr()), "pack")
    torch.cuda.synchronize()
    k["packed"] = packed
    n = X.pack_elems(c, hidden)
    k["pack_ok"] = torch.equal(packed[:n], X.pack_images(o["w1"], o["w2"])) and bool((packed[n:] == SENTINEL).all())
    f, f2, fe = _forward(L, lib, k, True), _forward(L, lib, k, True), _forward(L, lib, k, False)
    b, b2 = _backward(L, lib, k, f["pre"]), _backward(L, lib, k, f["pre"])
    bm = X.cfg(c).bm
    owned = (t + bm - 1) // bm * bm * hidden  # the elements of pre / post / d_pre the launch's workgroups own
    k["fwd_twice"] = all(torch.equal(f[n], f2[n]) for n in ("out", "u", "pre")) and torch.equal(f["stats"][:, :t], f2["stats"][:, :t])
    k["eval_equal"] = torch.equal(f["out"], fe["out"])
    k["bwd_twice"] = all(torch.equal(b[n], b2[n]) for n in ("post", "dpre", "du"))
    k["kept"] = dict(
        out=_kept(f["obuf"], t, c), u=_kept(f["ubuf"], t, c), out_eval=_kept(fe["obuf"], t, c), du=_kept(b["dubuf"], t, c),
        stats=bool(torch.isnan(f["stats"][:, t:]).all()) and bool(torch.isfinite(f["stats"][:, :t]).all()),
        pre=bool((f["pre"][owned:] == SENTINEL).all()), post=bool((b["postbuf"][owned:] == SENTINEL).all()), dpre=bool((b["dprebuf"][owned:] == SENTINEL).all()),
    )
    k["got"] = dict(mean=f["stats"][0, :t], rstd=f["stats"][1, :t], u=f["u"], pre=X.decode_pre(f["pre"], c, t, hidden), out=f["out"], post=b["post"], dpre=b["dpre"],
                    du=b["du"])
    return k


def _tag(c, cs, kind):
    return f"[swin_mlp {kind} C {c} T {cs.t} hidden {cs.hidden} ld {c + 8 if cs.strided else c}]"


def test_library_agrees_with_the_mirrors():
    L, lib = _lib()
    for c in X.WIDTHS:
        k = X.cfg(c)
        assert k.hidden_max == {128: 8192, 256: 8192, 384: 4096}[c]
        for hidden in (0, 16, 32, 48, 96, 4 * c, k.hidden_max, k.hidden_max + 32):
            assert bool(lib.ymi_swin_ln_mlp_supported(c, hidden, L.YMI_BF16)) == X.supported(c, hidden), (c, hidden)
        for t in (1, 255, 256, 257, 421):
            assert lib.ymi_swin_ln_mlp_pre_elems(t, 96) == X.pre_elems(t, 96)
        X.assert_coverage(c)


@pytest.mark.parametrize("c,cs", [k for k in CASES if k[1].gate1], ids=[i for i, k in zip(IDS, CASES) if k[1].gate1])
def test_gate1_placement(c, cs):
    """u, pre (decoded from the private layout), post, out, d_pre, d_u bit for bit; the statistics within 1e-5"""
    k = _run(c, cs.t, cs.hidden, cs.strided, "gate1")
    exp = X.gate1_expected(k["o"])
    X.gate1_check(_tag(c, cs, "gate1"), k["o"], exp, k["got"])
    print(f"\n{_tag(c, cs, 'gate1')} u pre post out dpre du exact; margins " + X.fmt_ratios(exp["margins"]))


@pytest.mark.parametrize("kind", ["real", "real3"])
@pytest.mark.parametrize("c,cs", CASES, ids=IDS)
def test_gate2_precision(c, cs, kind):
    """every stage within its float64 bound, each fed the kernel's own stored input"""
    k = _run(c, cs.t, cs.hidden, cs.strided, kind)
    tag = _tag(c, cs, kind)
    r = X.gate2_forward(tag, k["o"], k["got"])
    r.update(X.gate2_backward(tag, k["o"], k["got"]["pre"], k["got"]))
    print(f"\n{tag} " + X.fmt_ratios(r))


@pytest.mark.parametrize("c,cs", CASES, ids=IDS)
def test_modes_and_sentinels(c, cs):
    """the packed images equal the host mirror; training and evaluation forward give a bit-equal out; each form run twice is bit-identical;
    nothing outside the owned rows and columns is written"""
    for kind in ("gate1", "real"):
        k = _run(c, cs.t, cs.hidden, cs.strided, kind)
        tag = _tag(c, cs, kind)
        assert k["pack_ok"], f"{tag}: the packed weight images differ from the host mirror"
        assert k["eval_equal"], f"{tag}: the evaluation forward gives another out"
        assert k["fwd_twice"], f"{tag}: two forward runs differ"
        assert k["bwd_twice"], f"{tag}: two backward runs differ"
        assert all(k["kept"].values()), f"{tag}: written outside the owned region: {[n for n, v in k['kept'].items() if not v]}"
