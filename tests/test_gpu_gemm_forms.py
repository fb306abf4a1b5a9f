"""GPU: every tile and epilogue form of the implicit-GEMM family checked element by element (tests/gemm_exact.py).

The dispatcher (csrc/igemm.hip choose_tile) picks one of its tile forms from the shape, and the K-step form (wide 64-deep, fast 32-deep
/ 16-deep float32, general), vector stores, the residual form (res1 joins the addend before the one rounding, res2nd after the
activation, from the LDS image) and the statistics epilogue follow from shapes, alignment and the entry point.  These tests force each
tile through the igemm_tile_bm / igemm_tile_bn options, prove the force took effect (the statistics mode reports ceil(M / BM) row
blocks) and compare with float64 host references: exact small-integer operands (Gate 1, bit for bit: placement) and real operands
(Gate 2, a per-element float64 bound: rounding and accumulation) on the direct stores, res1, the SiLU / res2nd path, the data gradient,
the weight-gradient slabs and the Swin MLP's GELU second output (y2) and activation-gradient multiplier (mul).  A force the dispatcher
cannot honour is reported as refused and the run is checked under the tile that really ran.  The weight gradient (csrc/wgrad.hip) is
covered the same way over its row tiles, split counts (forced through wgrad_blocks), slab types, patch widths and the deferred batched
sum.  Options are restored to their earlier values after every case.

One line per case: direction, dtype, tile that ran, K-step form, epilogue, worst Gate 1 / Gate 2 error.
YMI_GEMM_SOAK=N runs N random forward / data-gradient shapes per dtype (default 6) for a longer soak."""
import contextlib
import ctypes
import os
import random

import pytest
import torch

import gemm_exact as G
from improving_yolov8_cbam_swinblock_amd import ops
from improving_yolov8_cbam_swinblock_amd._lib import (ConvProblem, DgradProblem, WgradPending, as_ymi, check, get_option, lib as L, ptr,
                                                      set_option, stream_ptr)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DTYPES = [BF, F32]
TILES = [(256, 128), (128, 128), (128, 64), (128, 32), (64, 128), (64, 64), (0, 0)]
SOAK = int(os.environ.get("YMI_GEMM_SOAK", "6"))  # random shapes per dtype and direction; raise for a longer soak
SENTINEL = -99.0
ACT_SILU = 1


def dev():
    return torch.device("cuda:0")


def dname(dtype):
    return "bf16" if dtype == BF else "f32"


def tname(t):
    return "default" if t == (0, 0) else f"{t[0]}x{t[1]}"


@contextlib.contextmanager
def options(**kv):
    """set library options for the block; the earlier values come back afterwards, whatever happens inside."""
    old = {k: get_option(k) for k in kv}
    try:
        for k, v in kv.items():
            set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            set_option(k, v)


def forced(tile):
    return options(igemm_tile_bm=tile[0], igemm_tile_bn=tile[1])


def on_dev(t, dtype, ld=None, off=0, fill=SENTINEL):
    """host NCHW tensor -> device logical NCHW view in NHWC memory; channels [off, off + c) of a buffer of `ld` channels holding `fill`."""
    n, c, h, w = t.shape
    ld = ld or (c + off)
    buf = torch.full((n, h, w, ld), fill, dtype=dtype, device=dev())
    buf[..., off : off + c] = t.permute(0, 2, 3, 1).to(device=dev(), dtype=dtype)
    return buf.permute(0, 3, 1, 2)[:, off : off + c], buf


def out_dev(n, c, h, w, dtype, ld=None, off=0, fill=SENTINEL):
    return on_dev(torch.full((n, c, h, w), fill), dtype, ld, off, fill)


def untouched(what, buf, off, c):
    """channels of a wider buffer outside the output slice keep the caller's values."""
    rest = torch.cat([buf[..., :off], buf[..., off + c :]], -1).float()
    assert bool((rest == SENTINEL).all()), f"{what}: {int((rest != SENTINEL).sum())} elements outside the output slice were written"


def byref(t):
    return ctypes.byref(as_ymi(t)) if t is not None else None


def wdensity(k_terms, target):
    return min(1.0, target / k_terms)


# ================================================================================================ forward
def fwd_call(x, wp, cout, k, s, y, scale=None, bias=None, act=0, res=None, stats=False):
    m = y.shape[0] * y.shape[2] * y.shape[3]
    part, blocks = None, ctypes.c_int64(-1)
    if stats:
        nb = L().ymi_conv2d_stat_blocks(m, cout)
        part = torch.full((nb, 2, cout), float("nan"), device=dev())
    check(L().ymi_conv2d_fwd(byref(x), ptr(wp), cout, k, k, s, ptr(scale), ptr(bias), act, byref(res), byref(y), ptr(part),
                             ctypes.byref(blocks) if stats else None, stream_ptr()), "conv2d_fwd")
    torch.cuda.synchronize()
    return part, blocks.value


def check_partials(what, part, blocks, exp, bm, loc):
    """[blocks][2][cout] statistics rows: each block's row equals the exact sums over ITS rows of the stored output."""
    n, c, h, w = exp.shape
    rows = exp.permute(0, 2, 3, 1).reshape(-1, c)
    m = rows.shape[0]
    assert blocks == (m + bm - 1) // bm, f"{what}: {blocks} statistics blocks, the {bm}-row tile gives {(m + bm - 1) // bm}: the tile did not run"
    want = torch.zeros(blocks, 2, c, dtype=torch.float64)
    for b in range(blocks):
        r = rows[b * bm : (b + 1) * bm]
        want[b, 0], want[b, 1] = r.sum(0), (r * r).sum(0)
        assert float((r * r).abs().sum(0).max()) <= G.F32_EXACT, f"{what}: not an exact case (sum of squares of block {b})"
    G.check_exact(what + " statistics rows", part[:blocks].cpu(), want)


def check_partials_bound(what, part, blocks, y, bm):
    """Gate 2 on the statistics rows: float32 sums of at most BM stored values (and of their squares, one more rounding each)."""
    c = y.shape[1]
    rows = G._h(y).permute(0, 2, 3, 1).reshape(-1, c)
    want = torch.zeros(blocks, 2, c, dtype=torch.float64)
    for b in range(blocks):
        r = rows[b * bm : (b + 1) * bm]
        want[b, 0], want[b, 1] = r.sum(0), (r * r).sum(0)
    bound = torch.stack([G.gamma(bm) * want[:, 0].abs(), G.gamma(bm + 1) * want[:, 1]], 1)
    return G.check_bound(what + " statistics rows", part[:blocks].cpu(), want, bound)


def fwd_case(tile, dtype, n, cin, h, w, cout, k, s, epi, seed):
    """one forward run -> report line.  epi: stats | slices | affine | novec (Gate 1) | silu | gate2 (Gate 2)."""
    bf16 = dtype == BF
    g = torch.Generator().manual_seed(seed)
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    m, kt = n * ho * wo, cin * k * k
    fast = (cin // (8 if bf16 else 4)) % 4 == 0
    bm, bn, ok = G.choose_tile(m, cout, kt, bf16, fast, tile)
    ran = (bm, bn)
    tag = f"fwd {dname(dtype)} n{n} {cin}->{cout} {h}x{w} k{k} s{s} M={m} forced {tname(tile)} ran {ran[0]}x{ran[1]} K-form {G.kform(cin, dtype) if ran[0] != 256 else 'pp32'} epi {epi}"
    if tile != (0, 0) and not ok:
        tag += f" (REFUSED: {G.refusal_reason(tile, cout, bf16, fast)})"
    loc = G.gemm_locator(ran, m, G.fwd_row(ho, wo))
    if epi in ("silu", "gate2"):
        x = G.positive((n, cin, h, w), g, dtype=dtype)
        wt = G.positive((cout, cin, k, k), g, 0.0, 1.0 / kt, dtype=dtype)
        scale = G.positive((cout,), g, 0.5, 1.0)
        bias = G.positive((cout,), g, 0.0, 0.5)
        res = G.positive((n, cout, ho, wo), g, dtype=dtype)
    else:
        x = G.ints((n, cin, h, w), g)
        wt = G.ints((cout, cin, k, k), g, -1, 1, density=wdensity(kt, 24 if epi == "affine" else 80))
    wg = wt.to(dev())
    xoff, yoff, xld, yld = 0, 0, None, None
    if epi == "slices":
        xoff, yoff = (8, 8) if bf16 else (4, 4)
        xld, yld = cin + 2 * xoff, cout + 24
    if epi == "novec":
        yoff, yld = 1, cout + 8
    xd, _ = on_dev(x, dtype, xld, xoff)
    yd, ybuf = out_dev(n, cout, ho, wo, dtype, yld, yoff)
    wp = ops.pack_conv_fwd(wg, cin, dtype)
    ref, mag = G.conv_fwd64(x, wt, s), G.conv_fwd_mag(x, wt, s)
    with forced(tile):
        # statistics mode first: host_stat_blocks proves which row tile ran for this shape (the force rule depends on the shape only)
        if epi in ("stats", "slices"):
            part, blocks = fwd_call(xd, wp, cout, k, s, yd, stats=True)
            exp = G.exact_expected(ref, mag, dtype, what=tag)
            G.check_exact(tag, yd, exp, loc)
            check_partials(tag, part, blocks, exp, ran[0], loc)
            if yld:
                untouched(tag, ybuf, yoff, cout)
            return f"{tag}: Gate 1 exact (output + {blocks} statistics rows)"
        sd, sb = out_dev(n, cout, ho, wo, dtype)
        _, blocks = fwd_call(xd, wp, cout, k, s, sd, stats=True)
        assert blocks == (m + ran[0] - 1) // ran[0], f"{tag}: {blocks} statistics blocks: the {ran[0]}-row tile did not run"
        if epi == "affine" or epi == "novec":
            sc = torch.tensor([(0.5, 2.0, 1.0, 0.25)[i % 4] for i in range(cout)])
            bi = G.ints((cout,), g, -3, 3, nonzero=False)
            r = G.ints((n, cout, ho, wo), g)
            rd, _ = on_dev(r, dtype)
            fwd_call(xd, wp, cout, k, s, yd, scale=sc.to(dev()), bias=bi.to(dev()), res=rd)
            v = ref * sc.double().view(1, -1, 1, 1) + bi.double().view(1, -1, 1, 1)
            vmag = mag * sc.double().view(1, -1, 1, 1) + bi.double().abs().view(1, -1, 1, 1)
            G.exact_expected(v, vmag, dtype, what=tag + " (stored before the addend on the res2nd path)")
            exp = G.exact_expected(v + r.double(), vmag + r.double().abs(), dtype, what=tag)
            G.check_exact(tag, yd, exp, loc)
            if yld:
                untouched(tag, ybuf, yoff, cout)
            vec = yoff == 0 and cout % 4 == 0
            return f"{tag} ({'res1' if vec else 'res2nd'}): Gate 1 exact"
        if epi == "gate2":
            # real operands on the direct store paths: the raw output and its statistics rows, then scale, bias and the residual joined
            # before the one rounding (res1) - rounding by truncation or a bf16 accumulation fails here, not in Gate 1
            part, blocks = fwd_call(xd, wp, cout, k, s, yd, stats=True)
            w_raw = G.check_bound(tag + " raw", yd, ref, G.bound_plain(ref, mag, kt, dtype), loc)
            w_st = check_partials_bound(tag, part, blocks, yd, ran[0])
            yd2, _ = out_dev(n, cout, ho, wo, dtype)
            rd, _ = on_dev(res, dtype)
            fwd_call(xd, wp, cout, k, s, yd2, scale=scale.to(dev()), bias=bias.to(dev()), res=rd)
            z = ref * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)
            if cout % 4 == 0:  # res1: the residual joins the float32 value before the one rounding
                v, bound, form = z + res.double(), G.bound_plain(z + res.double(), z + res.double(), kt + 3, dtype), "res1"
            else:  # rows not 4-element aligned: res2nd, the residual added to the rounded LDS image
                (v, bound), form = G.bound_res2nd(z, z, kt + 2, res.double(), dtype), "res2nd"
            w_res = G.check_bound(tag + " " + form, yd2, v, bound, loc)
            return f"{tag} (raw + statistics, {form}): Gate 2 worst err/bound {max(w_raw, w_st, w_res):.3f}"
        # silu: act(scale * conv + bias) + residual, the residual added after the activation (res2nd) from the rounded LDS image
        rd, _ = on_dev(res, dtype)
        fwd_call(xd, wp, cout, k, s, yd, scale=scale.to(dev()), bias=bias.to(dev()), act=ACT_SILU, res=rd)
        z = ref * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)
        zerr = G.gamma(kt + 2) * z
        want, bound = G.bound_act(z, zerr, G.silu64(z), "silu", dtype, extra_ref=res.double(), final_dtype=dtype)
        worst = G.check_bound(tag, yd, want, bound, loc)
        return f"{tag} (res2nd): Gate 2 worst err/bound {worst:.3f}"


FWD_GEOM = [  # n, (cin bf16, cin f32), h, w, cout, k, s
    (1, (64, 16), 1, 1, 72, 3, 1),  # 1x1 map: eight of nine taps in the padding
    (2, (32, 32), 2, 3, 40, 3, 1),  # 2x3 maps, fast K steps
    (3, (24, 12), 7, 5, 136, 3, 2),  # odd stride-2 maps (4x3 out), general K steps
    (2, (128, 48), 9, 11, 200, 1, 2),  # k1 stride 2 on odd maps, wide K steps
    (1, (8, 4), 3, 100, 32, 3, 1),  # one-chunk general K, cout 32 (the 128x32 tile)
    (5, (96, 64), 6, 7, 128, 3, 1),  # tiles straddle images
    (1, (40, 12), 1, 1500, 48, 1, 1),  # span 192 rows: not a multiple of 128 / 256
    (1, (256, 64), 1, 191, 96, 1, 1),  # four K steps, M = 128 + 63
    (2, (40, 8), 5, 9, 24, 3, 2),  # cout 24, general K
]
FWD_EPIS = ["stats", "slices", "affine", "novec", "silu", "gate2"]


def _run_cases(lines_and_errors, fn, *args):
    try:
        line = fn(*args)
        print(line)
        lines_and_errors[0].append(line)
    except AssertionError as e:
        print("FAIL", e)
        lines_and_errors[1].append(str(e))


@pytest.mark.parametrize("tile", TILES, ids=tname)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_forward_tiles_geometry_and_epilogues(dtype, tile):
    acc = ([], [])
    for i, (n, cins, h, w, cout, k, s) in enumerate(FWD_GEOM):
        cin = cins[0] if dtype == BF else cins[1]
        for j, epi in enumerate(FWD_EPIS):
            _run_cases(acc, fwd_case, tile, dtype, n, cin, h, w, cout, k, s, epi, 100 * i + j)
    assert not acc[1], "\n\n".join(acc[1])


@pytest.mark.parametrize("tile", TILES, ids=tname)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_forward_ragged_last_tile_and_pipeline_depth(dtype, tile):
    """last M tiles of 1, BM/2-1, BM/2, BM/2+1 and BM-1 rows; K extents of 1, 2, 3, 4 and 9 K steps of the form that runs."""
    bf16 = dtype == BF
    acc = ([], [])
    cout = 24 if tile[1] == 32 else 136
    bm = tile[0] or 64
    for r in (1, bm // 2 - 1, bm // 2, bm // 2 + 1, bm - 1):
        _run_cases(acc, fwd_case, tile, dtype, 1, 32 if bf16 else 16, 1, 2 * bm + r, cout, 1, 1, "stats", r)
    step = 32 if tile[0] == 256 else (64 if bf16 else 16)
    for steps in (1, 2, 3, 4, 9):
        _run_cases(acc, fwd_case, tile, dtype, 1, step * steps, 1, 300, 72 if tile[1] != 32 else 24, 1, 1, "stats", 1000 + steps)
    _run_cases(acc, fwd_case, tile, dtype, 2, 32 if bf16 else 16, 3, 50, cout, 3, 1, "silu", 77)
    assert not acc[1], "\n\n".join(acc[1])


def test_forward_default_picks_the_ping_pong_tile():
    """>= 300 tiles of 256x128: the dispatcher picks the ping-pong form by itself (a 3x3 conv and a token GEMM)."""
    acc = ([], [])
    _run_cases(acc, fwd_case, (0, 0), BF, 3, 32, 160, 160, 128, 3, 1, "stats", 5)
    _run_cases(acc, fwd_case, (0, 0), BF, 1, 64, 1, 76800 + 77, 136, 1, 1, "stats", 6)
    assert not acc[1], "\n\n".join(acc[1])
    assert all("ran 256x128" in l for l in acc[0]), acc[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_forward_random_soak(dtype):
    rng = random.Random(1234)
    acc = ([], [])
    for i in range(SOAK):
        ch = 8 if dtype == BF else 4
        tile = rng.choice(TILES)
        k, s = rng.choice([1, 3]), rng.choice([1, 2])
        args = (tile, dtype, rng.randint(1, 4), ch * rng.randint(1, 40), rng.randint(1, 30), rng.randint(1, 30), rng.randint(1, 300), k, s,
                rng.choice(FWD_EPIS), 5000 + i)
        _run_cases(acc, fwd_case, *args)
    assert not acc[1], "\n\n".join(acc[1])


# ================================================================================================ fixed-point statistics
@pytest.mark.parametrize("tile", [(128, 64), (64, 64), (256, 128), (0, 0)], ids=tname)
def test_fixed_point_statistics_per_replica(tile):
    """ymi_conv2d_bn_silu_fwd_acc: stat_acc[4][2][cout] holds exactly sum(y) * 2^shift and sum(y^2) * 2^shift over the M blocks
    mb with mb & 3 == replica; save_mean / save_invstd within 1e-6 of float64."""
    dtype, n, cin, h, w, cout, k = BF, 2, 64, 13, 11, 128, 3
    g = torch.Generator().manual_seed(3)
    x = G.ints((n, cin, h, w), g)
    wt = G.ints((cout, cin, k, k), g, -1, 1, density=wdensity(cin * 9, 60))
    m = n * h * w
    bm, bn, ok = G.choose_tile(m, cout, cin * 9, True, True, tile)
    assert ok or tile == (0, 0)
    xd, _ = on_dev(x, dtype)
    wp = ops.pack_conv_fwd(wt.to(dev()), cin, dtype)
    raw, _ = out_dev(n, cout, h, w, dtype)
    out, _ = out_dev(n, cout, h, w, dtype)
    acc = torch.zeros(4, 2, cout, dtype=torch.int64, device=dev())
    gamma, beta = torch.ones(cout, device=dev()), torch.zeros(cout, device=dev())
    rm, rv = torch.zeros(cout, device=dev()), torch.ones(cout, device=dev())
    sm, si = torch.empty(cout, device=dev()), torch.empty(cout, device=dev())
    eps = 1e-3
    with forced(tile):
        check(L().ymi_conv2d_bn_silu_fwd_acc(byref(xd), ptr(wp), cout, k, k, 1, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), 0.03, eps, ACT_SILU,
                                             None, byref(raw), byref(out), ptr(sm), ptr(si), ptr(acc), stream_ptr()), "bn_silu_fwd_acc")
        torch.cuda.synchronize()
    ref, mag = G.conv_fwd64(x, wt, 1), G.conv_fwd_mag(x, wt, 1)
    exp = G.exact_expected(ref, mag, dtype, what="fixed-point stats")
    G.check_exact("fixed-point stats raw", raw, exp, G.gemm_locator((bm, bn), m, G.fwd_row(h, w)))
    lg = max(0, (m - 1).bit_length())
    shift = min(40, max(8, 37 - lg))
    rows = exp.permute(0, 2, 3, 1).reshape(-1, cout)
    want = torch.zeros(4, 2, cout, dtype=torch.int64)
    for b in range((m + bm - 1) // bm):
        r = rows[b * bm : (b + 1) * bm]
        want[b & 3, 0] += (r.sum(0) * 2.0 ** shift).long()
        want[b & 3, 1] += ((r * r).sum(0) * 2.0 ** shift).long()
    got = acc.cpu()
    bad = got != want
    assert not bool(bad.any()), f"fixed-point statistics ({bm}-row tile): {int(bad.sum())} of {bad.numel()} replica sums differ"
    mean = rows.mean(0)
    var = (rows * rows).mean(0) - mean * mean
    invstd = 1.0 / torch.sqrt(var + eps)
    em = float(((sm.cpu().double() - mean).abs() / mean.abs().clamp(min=1e-3)).max())
    ei = float(((si.cpu().double() - invstd).abs() / invstd).max())
    print(f"stat_acc bf16 tile {bm}x{bn} shift {shift}: replicas exact; save_mean rel {em:.1e} save_invstd rel {ei:.1e}")
    assert em <= 1e-6 and ei <= 1e-6, (em, ei)


# ================================================================================================ multi-problem forward
@pytest.mark.parametrize("tile", [(128, 64), (64, 64), (128, 128), (0, 0)], ids=tname)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_forward_multi_mixed_widths_shared_statistics_rows(dtype, tile):
    """ymi_conv2d_fwd_multi: two problems of one BatchNorm group share a statistics row array side by side (stat_stride / stat_offset), a
    third has its own rows; mixed output widths."""
    bf16 = dtype == BF
    g = torch.Generator().manual_seed(11)
    specs = [(2, 64 if bf16 else 32, 9, 7, 96, 3), (2, 64 if bf16 else 32, 9, 7, 40, 3), (1, 64 if bf16 else 32, 5, 30, 72, 1)]
    fast = True
    msum = sum(n * h * w for n, _, h, w, _, _ in specs)
    cmax, cmin = max(s[4] for s in specs), min(s[4] for s in specs)
    kmax = max(s[1] * s[5] ** 2 for s in specs)
    bm, bn, ok = G.choose_tile(msum, cmax, kmax, bf16, fast, tile)
    if bn > 64 and cmin <= 64 and cmax > 64 and bm != 256:
        bn = 64
    keep, probs, refs = [], [], []
    shared_m = specs[0][0] * specs[0][2] * specs[0][3]
    nb_shared = L().ymi_conv2d_stat_blocks(shared_m, 136)
    shared = torch.full((nb_shared, 2, 136), float("nan"), device=dev())
    own_m = specs[2][0] * specs[2][2] * specs[2][3]
    own = torch.full((L().ymi_conv2d_stat_blocks(own_m, 72), 2, 72), float("nan"), device=dev())
    for i, (n, cin, h, w, cout, k) in enumerate(specs):
        x = G.ints((n, cin, h, w), g)
        wt = G.ints((cout, cin, k, k), g, -1, 1, density=wdensity(cin * k * k, 60))
        xd, _ = on_dev(x, dtype)
        yd, _ = out_dev(n, cout, h, w, dtype)
        wp = ops.pack_conv_fwd(wt.to(dev()), cin, dtype)
        tx, ty = as_ymi(xd), as_ymi(yd)
        keep += [tx, ty, xd, yd, wp]
        p = ConvProblem()
        p.x, p.y = ctypes.pointer(tx), ctypes.pointer(ty)
        p.w_packed, p.cout, p.kh, p.kw, p.stride = wp.data_ptr(), cout, k, k, 1
        p.stat_partials = (shared if i < 2 else own).data_ptr()
        p.stat_stride, p.stat_offset = (136, 0 if i == 0 else 96) if i < 2 else (0, 0)
        probs.append(p)
        refs.append((G.conv_fwd64(x, wt, 1), G.conv_fwd_mag(x, wt, 1), yd, h, w))
    arr = (ConvProblem * len(probs))(*probs)
    with forced(tile):
        check(L().ymi_conv2d_fwd_multi(arr, len(probs), stream_ptr()), "conv2d_fwd_multi")
        torch.cuda.synchronize()
    exps = []
    for i, (ref, mag, yd, h, w) in enumerate(refs):
        exp = G.exact_expected(ref, mag, dtype, what=f"multi problem {i}")
        G.check_exact(f"multi problem {i} ({bm}x{bn})", yd, exp, G.gemm_locator((bm, bn), ref.shape[0] * h * w, G.fwd_row(h, w)))
        assert arr[i].stat_blocks == (ref.shape[0] * h * w + bm - 1) // bm, (i, arr[i].stat_blocks, bm)
        exps.append(exp)
    both = torch.cat([exps[0], exps[1]], 1)
    check_partials("multi shared rows", shared, arr[0].stat_blocks, both, bm, None)
    check_partials("multi own rows", own, arr[2].stat_blocks, exps[2], bm, None)
    print(f"fwd_multi {dname(dtype)} forced {tname(tile)} ran {bm}x{bn}: Gate 1 exact (3 problems, shared + own statistics rows)")


# ================================================================================================ Swin MLP (the y2 and mul epilogues)
def _probe_rows(m, cout, cin):
    """statistics-mode forward of a token GEMM [m, cin] x [cin, cout]: -> the row blocks the dispatcher's tile gives for (M, N, ktot)."""
    xd, _ = on_dev(torch.zeros(1, cin, 1, m), BF)
    yd, _ = out_dev(1, cout, 1, m, BF)
    return fwd_call(xd, ops.pack_conv_fwd(torch.zeros(cout, cin, 1, 1, device=dev()), cin, BF), cout, 1, 1, yd, stats=True)[1]


@pytest.mark.parametrize("tile", [(0, 0), (128, 128), (256, 128)], ids=tname)
def test_swin_mlp_second_output_and_multiplier_epilogues(tile):
    """config 5's unfused Swin MLP (C = 384, hidden 1536, bfloat16 tokens; ops/blocks.py _SwinMlp):
      ymi_swin_mlp_fwd     : pre = fc1(u) + b1 stored, post = GELU of the STORED pre (the y2 second output, read back from the rounded LDS
                             image), out = fc2(post) + b2 + residual (res1);
      ymi_swin_mlp_bwd_data: dpre = stored(dout W2) * gelu'(pre) (the mul epilogue), du = dpre W1 + add1.
    Every output against float64 on the exact operand values the kernel saw, Gate 2 per element.  The four GEMMs have the (M, N, ktot) of a
    token GEMM [392, 384] x [384, 1536] or [392, 1536] x [1536, 384]; statistics-mode probes of those two shapes prove the forced tile."""
    t, c, hid = 392, 384, 1536
    g = torch.Generator().manual_seed(31)
    u = G.positive((t, c), g, dtype=BF)
    w1 = G.positive((hid, c), g, 0.0, 2.0 / c, dtype=BF)
    b1 = torch.rand(hid, generator=g) * 2.0 - 1.5  # pre in about [-1.2, 0.8]: GELU and its derivative on both signs
    w2 = (torch.rand(c, hid, generator=g) * 2.0 - 1.0).mul(2.0 / hid).to(BF).float()
    b2 = G.positive((c,), g, 0.0, 0.5)
    res = G.positive((t, c), g, dtype=BF)
    dout = (torch.rand(t, c, generator=g) * 2.0 - 1.0).to(BF).float()
    add1 = G.positive((t, c), g, dtype=BF)
    ran = []
    with forced(tile):
        for m_, n_, k_ in ((t, hid, c), (t, c, hid)):
            bm, bn, ok = G.choose_tile(m_, n_, k_, True, True, tile)
            assert ok or tile == (0, 0)
            assert _probe_rows(m_, n_, k_) == (m_ + bm - 1) // bm, (m_, n_, k_, bm)
            ran.append(f"{bm}x{bn}")
        d = lambda a: a.to(device=dev(), dtype=BF).contiguous()
        ud, resd, doutd, a1d = d(u), d(res), d(dout), d(add1)
        b1d, b2d = b1.to(dev()), b2.to(dev())
        pre, post, dpre = (torch.full((t, hid), SENTINEL, dtype=BF, device=dev()) for _ in range(3))
        out, du = (torch.full((t, c), SENTINEL, dtype=BF, device=dev()) for _ in range(2))
        w1p, w2p = ops.pack_conv_fwd(w1.to(dev()), c, BF), ops.pack_conv_fwd(w2.to(dev()), hid, BF)
        check(L().ymi_swin_mlp_fwd(byref(ud), ptr(w1p), ptr(b1d), hid, ptr(w2p), ptr(b2d), byref(resd), byref(pre), byref(post), byref(out),
                                   stream_ptr()), "swin_mlp_fwd")
        w2d, w1d = ops.pack_conv_dgrad(w2.to(dev()), c, 1, BF), ops.pack_conv_dgrad(w1.to(dev()), hid, 1, BF)
        check(L().ymi_swin_mlp_bwd_data(byref(doutd), ptr(w2d), byref(pre), byref(dpre), ptr(w1d), byref(a1d), None, byref(du), stream_ptr()),
              "swin_mlp_bwd_data")
        torch.cuda.synchronize()
    h = lambda a: a.double()
    z = h(u) @ h(w1).T + h(b1)
    zmag = h(u) @ h(w1).abs().T + h(b1).abs()
    w_pre = G.check_bound("swin pre", pre, z, G.bound_plain(z, zmag, c + 1, BF))
    want, bound = G.bound_act(z, G.gamma(c + 1) * zmag, G.gelu64(z), "gelu", BF, final_dtype=BF)
    w_post = G.check_bound("swin post (y2 = GELU of the stored pre)", post, want, bound)
    ps = G._h(post)
    o = ps @ h(w2).T + h(b2) + h(res)
    omag = ps.abs() @ h(w2).abs().T + h(b2).abs() + h(res).abs()
    w_out = G.check_bound("swin out", out, o, G.bound_plain(o, omag, hid + 2, BF))
    gref, gmag = h(dout) @ h(w2), h(dout).abs() @ h(w2).abs()
    want, bound = G.bound_mul(gref, G.gamma(c) * gmag, G._h(pre), BF)
    w_dpre = G.check_bound("swin dpre (mul epilogue)", dpre, want, bound)
    ds = G._h(dpre)
    dur = ds @ h(w1) + h(add1)
    w_du = G.check_bound("swin du", du, dur, G.bound_plain(dur, ds.abs() @ h(w1).abs() + h(add1).abs(), hid + 1, BF))
    print(f"swin mlp bf16 C={c} forced {tname(tile)} ran {'/'.join(ran)}: Gate 2 worst err/bound pre {w_pre:.3f} post(y2) {w_post:.3f} "
          f"out {w_out:.3f} dpre(mul) {w_dpre:.3f} du {w_du:.3f}")


# ================================================================================================ data gradient
def dgrad_case(tile, dtype, n, cin, h, w, cout, k, s, epi, seed):
    """dx [n, cin, h, w] = dgrad(dy [n, cout, ho, wo], w [cout, cin, k, k]) (+ addends).  epi: plain | add12 | self (Gate 1) | gate2 (positive
    real operands, one addend where the form takes one: Gate 2)."""
    bf16 = dtype == BF
    g = torch.Generator().manual_seed(seed)
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    launches = G.dgrad_launches(n, h, w, cin, cout, k, s, dtype, tile)
    ran = sorted({(c["bm"], c["bn"]) for c in launches})
    tag = (f"dgrad {dname(dtype)} n{n} dy {cout}->dx {cin} {h}x{w} k{k} s{s} forced {tname(tile)} ran {','.join(f'{a}x{b}' for a, b in ran)} "
           f"K-form {G.kform(cout, dtype)} epi {epi}")
    if tile != (0, 0) and not all(c["honoured"] for c in launches):
        tag += f" (REFUSED: {G.refusal_reason(tile, cin, bf16, (cout // (8 if bf16 else 4)) % 4 == 0) or 'per-class rule'})"
    gate2 = epi == "gate2"
    if gate2:
        dy = G.positive((n, cout, ho, wo), g, dtype=dtype)
        wt = G.positive((cout, cin, k, k), g, 0.0, 1.0 / (cout * k * k), dtype=dtype)
    else:
        dy = G.ints((n, cout, ho, wo), g)
        wt = G.ints((cout, cin, k, k), g, -1, 1, density=wdensity(cout * k * k, 40))
    ref, mag = G.dgrad64(dy, wt, (n, cin, h, w), s), G.dgrad_mag(dy, wt, (n, cin, h, w), s)
    dyd, _ = on_dev(dy, dtype)
    wp = ops.pack_conv_dgrad(wt.to(dev()), cout, s, dtype)
    a1 = a2 = None
    pre = torch.full((n, cin, h, w), 5.0)  # what the caller wrote into dx (kept where no tap reaches: k1 stride 2)
    if epi == "self":
        pre = G.ints((n, cin, h, w), g)
    dxd, _ = on_dev(pre, dtype)
    want, wmag = ref.clone(), mag.clone()
    r1 = None
    if gate2 and not (k == 1 and s == 2):
        r1 = G.positive((n, cin, h, w), g, dtype=dtype)
        a1, _ = on_dev(r1, dtype)
    if epi == "add12":
        r1, r2 = G.ints((n, cin, h, w), g), G.ints((n, cin, h, w), g)
        a1, _ = on_dev(r1, dtype)
        a2, _ = on_dev(r2, dtype)
        want, wmag = want + r1.double() + r2.double(), wmag + r1.double().abs() + r2.double().abs()
    if epi == "self":
        a1 = dxd
        want, wmag = want + pre.double(), wmag + pre.double().abs()
    if k == 1 and s == 2:  # pixels off the stride grid keep the caller's value
        off = torch.ones(h, w, dtype=torch.bool)
        off[::2, ::2] = False
        want[:, :, off] = pre.double()[:, :, off]
    by_cls = {(c["ph"], c["pw"]): c for c in launches}

    def loc(nn, c, hh, ww):
        cl = by_cls.get((hh % s, ww % s))
        if cl is None:
            return "no GEMM row"
        mrow = (nn * cl["ho"] + hh // s) * cl["wo"] + ww // s
        mb = mrow // cl["bm"]
        return f"class {hh % s}{ww % s} m={mrow} tile {cl['bm']}x{cl['bn']} M-tile {mb} N-tile {c // cl['bn']} XCD {G.xcd_of_block(cl['M'], cl['bm'], mb)}"

    with forced(tile):
        check(L().ymi_conv2d_bwd_data_add(byref(dyd), ptr(wp), cin, k, k, s, byref(a1), byref(a2), byref(dxd), stream_ptr()), "conv2d_bwd_data_add")
        torch.cuda.synchronize()
    if gate2:
        # at most 9 taps x cout products per element; the addend joins before the one rounding (res1: dx rows 4-element aligned) or is
        # added to the rounded LDS image (res2nd)
        kt = cout * k * k
        if r1 is None:
            want, bound, form = want, G.bound_plain(want, wmag, kt, dtype), "no addend"
        elif cin % 4 == 0:
            want, bound, form = want + r1.double(), G.bound_plain(want + r1.double(), wmag + r1.double(), kt + 1, dtype), "res1"
        else:
            (want, bound), form = G.bound_res2nd(want, wmag, kt, r1.double(), dtype), "res2nd"
        worst = G.check_bound(tag, dxd, want, bound, loc)
        return f"{tag} ({form}): Gate 2 worst err/bound {worst:.3f}"
    exp = G.exact_expected(want, wmag, dtype, what=tag)
    G.check_exact(tag, dxd, exp, loc)
    return f"{tag}: Gate 1 exact"


DGRAD_GEOM = [  # n, cin (dx), h, w (dx), (cout bf16, cout f32) (dy), k, s
    (2, 72, 6, 5, (64, 16), 1, 1),
    (2, 40, 5, 7, (32, 32), 3, 1),
    (2, 136, 7, 5, (24, 12), 3, 2),  # odd maps: parity classes of unequal size
    (1, 64, 8, 6, (96, 48), 3, 2),  # even maps, the four classes in one launch (cin >= 64)
    (2, 32, 6, 9, (40, 8), 3, 2),  # cin < 64: one launch per class
    (2, 48, 9, 7, (128, 64), 1, 2),  # k1 stride 2: off-grid pixels keep the sentinel
    (1, 24, 1, 1, (64, 16), 3, 1),  # 1x1 map
    (3, 200, 4, 4, (32, 16), 3, 1),
]


@pytest.mark.parametrize("tile", TILES, ids=tname)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_data_gradient_tiles_geometry_and_addends(dtype, tile):
    acc = ([], [])
    for i, (n, cin, h, w, couts, k, s) in enumerate(DGRAD_GEOM):
        cout = couts[0] if dtype == BF else couts[1]
        for j, epi in enumerate(["plain", "add12", "self", "gate2"]):
            if k == 1 and s == 2 and epi in ("add12", "self"):
                continue  # (addends are refused there: EINVAL, the caller adds them)
            _run_cases(acc, dgrad_case, tile, dtype, n, cin, h, w, cout, k, s, epi, 300 + 10 * i + j)
    assert not acc[1], "\n\n".join(acc[1])


def test_data_gradient_default_ping_pong_with_dy_channels_off_the_32_grid():
    """stride-2 data gradient, bfloat16, 128 input channels on a 196 x 196 map (>= 300 tiles of 256x128), dy channels 72 (K steps of 9
    chunks: the general form) and 64.  The dispatcher used to pick the 256x128 ping-pong tile from the four-tap class's ktot % 32, so the
    72-channel launch failed with EINVAL; now it must run, and both must be exact.  A data gradient has no statistics mode, so which tile
    ran is not measured here: the tile names in the report lines come from the mirror (gemm_exact.choose_tile).  What is measured is the
    dispatcher's decision for the same arguments - M = 4 x 9604 rows, N = 128, ktot = 256 with whole-chunk taps for the 64-channel launch -
    through a statistics-mode forward of that shape (ktot = 288 with 9-chunk taps has no forward counterpart: k = 1 or 3 with 72 or 288
    input channels gives whole-chunk taps)."""
    acc = ([], [])
    _run_cases(acc, dgrad_case, (0, 0), BF, 2, 128, 196, 196, 72, 3, 2, "plain", 9)
    _run_cases(acc, dgrad_case, (0, 0), BF, 2, 128, 196, 196, 64, 3, 2, "plain", 10)
    assert not acc[1], "\n\n".join(acc[1])
    m = 4 * 98 * 98 * 2
    assert G.choose_tile(m, 128, 256, True, True)[:2] == (256, 128) and G.choose_tile(m, 128, 288, True, False)[:2] != (256, 128)
    xd, _ = on_dev(torch.zeros(1, 256, 1, m), BF)
    yd, _ = out_dev(1, 128, 1, m, BF)
    _, blocks = fwd_call(xd, ops.pack_conv_fwd(torch.zeros(128, 256, 1, 1, device=dev()), 256, BF), 128, 1, 1, yd, stats=True)
    assert blocks == (m + 255) // 256, f"the dispatcher chose {blocks} row blocks for M={m}, N=128, ktot=256: not the 256-row tile"


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_data_gradient_random_soak(dtype):
    rng = random.Random(4321)
    acc = ([], [])
    ch = 8 if dtype == BF else 4
    for i in range(SOAK):
        k, s = rng.choice([1, 3]), rng.choice([1, 2])
        args = (rng.choice(TILES), dtype, rng.randint(1, 4), rng.randint(1, 200), rng.randint(1, 30), rng.randint(1, 30), ch * rng.randint(1, 40),
                k, s, rng.choice(["plain", "gate2"]) if (k == 1 and s == 2) else rng.choice(["plain", "add12", "self", "gate2"]), 7000 + i)
        _run_cases(acc, dgrad_case, *args)
    assert not acc[1], "\n\n".join(acc[1])


@pytest.mark.parametrize("tile", [(128, 64), (64, 64), (64, 128), (0, 0)], ids=tname)
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_data_gradient_multi(dtype, tile):
    """ymi_conv2d_bwd_data_multi: stride-1 problems of mixed widths and kernel sizes in one launch, with addends (one of them dx itself)."""
    bf16 = dtype == BF
    g = torch.Generator().manual_seed(13)
    specs = [(2, 72, 6, 5, 64 if bf16 else 32, 3), (1, 136, 4, 9, 64 if bf16 else 32, 1), (3, 40, 3, 3, 64 if bf16 else 32, 3)]
    msum = sum(n * h * w for n, _, h, w, _, _ in specs)
    cmax, cmin = max(s[1] for s in specs), min(s[1] for s in specs)
    kmax = max(s[4] * s[5] ** 2 for s in specs)
    bm, bn, ok = G.choose_tile(msum, cmax, kmax, bf16, True, tile)
    if bn > 64 and cmin <= 64 and cmax > 64 and bm != 256:
        bn = 64
    keep, probs, checks = [], [], []
    for i, (n, cin, h, w, cout, k) in enumerate(specs):
        dy = G.ints((n, cout, h, w), g)
        wt = G.ints((cout, cin, k, k), g, -1, 1, density=wdensity(cout * k * k, 40))
        pre = G.ints((n, cin, h, w), g)
        dyd, _ = on_dev(dy, dtype)
        dxd, _ = on_dev(pre, dtype)
        wp = ops.pack_conv_dgrad(wt.to(dev()), cout, 1, dtype)
        ref, mag = G.dgrad64(dy, wt, (n, cin, h, w), 1), G.dgrad_mag(dy, wt, (n, cin, h, w), 1)
        tdy, tdx = as_ymi(dyd), as_ymi(dxd)
        p = DgradProblem()
        p.dy, p.dx, p.w_dgrad_packed, p.cin, p.k = ctypes.pointer(tdy), ctypes.pointer(tdx), wp.data_ptr(), cin, k
        if i != 1:
            p.add1 = ctypes.pointer(tdx)  # the addend is dx itself
            ref, mag = ref + pre.double(), mag + pre.double().abs()
        keep += [tdy, tdx, dyd, dxd, wp]
        probs.append(p)
        checks.append((ref, mag, dxd, h, w))
    arr = (DgradProblem * len(probs))(*probs)
    with forced(tile):
        check(L().ymi_conv2d_bwd_data_multi(arr, len(probs), stream_ptr()), "conv2d_bwd_data_multi")
        torch.cuda.synchronize()
    for i, (ref, mag, dxd, h, w) in enumerate(checks):
        exp = G.exact_expected(ref, mag, dtype, what=f"dgrad multi {i}")
        G.check_exact(f"dgrad multi problem {i} ({bm}x{bn})", dxd, exp, G.gemm_locator((bm, bn), ref.shape[0] * h * w, G.fwd_row(h, w)))
    print(f"dgrad_multi {dname(dtype)} forced {tname(tile)} ran {bm}x{bn}{'' if ok or tile == (0, 0) else ' (REFUSED)'}: Gate 1 exact")


# ================================================================================================ weight gradient
def sparse_dy(n, c, ho, wo, g, per_channel):
    """+-1 on structured pixels - every map border, the first and last pixel of each image - dealt round-robin to the channels, plus
    `per_channel` random pixels per channel: at most a few hundred nonzeros per channel, so bfloat16 slabs stay exact."""
    dy = torch.zeros(n, c, ho, wo)
    pix = []
    for b in range(n):
        for hh in range(ho):
            for ww in range(wo):
                if hh in (0, ho - 1) or ww in (0, wo - 1):
                    pix.append((b, hh, ww))
    for i, (b, hh, ww) in enumerate(pix):
        dy[b, i % c, hh, ww] = 1.0 if (i // c) % 2 == 0 else -1.0
    for ch in range(c):
        idx = torch.randint(0, n * ho * wo, (per_channel,), generator=g)
        flat = dy[:, ch].reshape(-1)
        flat[idx] = G.ints((per_channel,), g, -1, 1)
        dy[:, ch] = flat.view(n, ho, wo)
    return dy


WGRAD = [  # name, n, xc, cin_real, h, w, dyc, cout_real, k, s, wgrad_blocks (None: default), patch option
    ("1 split", 1, 16, 13, 8, 8, 24, 21, 3, 1, None, 1),
    ("<8 splits, bm 64", 2, 32, 32, 16, 32, 64, 64, 3, 1, None, 1),
    ("8-15 splits (xcd_map, f32 slabs)", 2, 16, 16, 32, 40, 32, 32, 3, 1, None, 1),
    ("forced 2 splits (3-D grid)", 2, 16, 16, 32, 40, 32, 32, 3, 1, 3, 1),
    (">=16 splits (bf16 slabs)", 2, 16, 16, 64, 64, 64, 60, 3, 1, None, 1),
    (">32 splits (16 lanes)", 4, 16, 16, 64, 64, 64, 64, 3, 1, None, 1),
    (">128 splits (32 lanes)", 2, 8, 8, 128, 160, 24, 24, 3, 1, None, 1),
    ("forced 24 splits", 2, 8, 8, 128, 160, 24, 24, 3, 1, 24, 1),
    ("row tile 128", 2, 16, 16, 32, 32, 128, 128, 3, 1, None, 1),
    ("stride 2", 2, 32, 32, 4, 64, 64, 64, 3, 2, None, 1),
    ("patch 16", 1, 16, 16, 16, 48, 32, 32, 3, 1, None, 1),
    ("patch 8", 1, 16, 16, 8, 40, 32, 32, 1, 1, None, 1),
    ("patch 4", 1, 16, 16, 16, 12, 32, 32, 3, 1, None, 1),
    ("patch 2", 1, 16, 16, 32, 6, 32, 32, 3, 1, None, 1),
    ("patch 1", 1, 16, 16, 32, 7, 32, 32, 3, 1, None, 1),
    ("raster (20x20 does not tile)", 2, 16, 16, 20, 20, 32, 32, 3, 1, None, 1),
    ("raster (patch off)", 2, 16, 16, 32, 32, 32, 32, 3, 1, None, 0),
    ("padded channels", 2, 24, 19, 12, 16, 40, 33, 1, 1, None, 1),
    ("row tile 128, bf16 slabs", 2, 16, 16, 64, 64, 128, 128, 3, 1, None, 1),
    ("row tile 128, bf16 slabs, ragged rows", 2, 16, 16, 64, 64, 264, 260, 3, 1, None, 1),
    ("row tile 128, f32 slabs, ragged rows", 2, 16, 16, 32, 32, 264, 260, 3, 1, None, 1),
    ("row tile 128, raster", 2, 16, 16, 64, 64, 128, 128, 3, 1, None, 0),
]


def wgrad_case(dtype, spec, deferred, seed, ws_fill=None):
    """ws_fill: a byte the workspace holds before the call (a caller that watches for the launch's first write: tests/test_gpu_bn_final.py)"""
    name, n, xc, cin_r, h, w, dyc, cout_r, k, s, blocks, patch = spec
    bf16 = dtype == BF
    if not bf16:
        xc, dyc = (xc + 3) // 4 * 4, (dyc + 3) // 4 * 4
    g = torch.Generator().manual_seed(seed)
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    mpix = n * ho * wo
    targets = (blocks or 1280, blocks or 768)
    bm, splits, slab16, lanes = G.wgrad_plan(mpix, dyc, k * k * xc, bf16, targets)
    x = G.ints((n, xc, h, w), g, -1, 1)
    dy = sparse_dy(n, dyc, ho, wo, g, 8) if slab16 else G.ints((n, dyc, ho, wo), g, -1, 1, density=0.7)
    pw = G.patch_width(ho, wo, mpix, bf16, bool(patch))
    tag = (f"wgrad {dname(dtype)} {name}: x {xc}({cin_r}) dy {dyc}({cout_r}) {h}x{w} k{k} s{s} M={mpix} row tile {bm} splits {splits} "
           f"{'bf16' if slab16 else 'f32'} slabs {'patch ' + str(pw) if pw else 'raster'}{' deferred, ' + str(lanes) + ' lanes' if deferred else ''}")
    ref = G.wgrad64(x[:, :cin_r], dy[:, :cout_r], (cout_r, cin_r, k, k), s)
    mag = G.wgrad_mag(x[:, :cin_r], dy[:, :cout_r], (cout_r, cin_r, k, k), s)
    exp = G.exact_expected(ref, mag, F32, slab_bf16=slab16, what=tag)
    dbias_want = dy.double().sum((0, 2, 3))
    xd, _ = on_dev(x, dtype)
    dyd, _ = on_dev(dy, dtype)
    opts = {"wgrad_patch": patch}
    if blocks:
        opts.update(wgrad_blocks=blocks, wgrad_blocks128=blocks)
    with options(**opts):
        need = L().ymi_conv2d_bwd_weight_workspace(mpix, dyc, xc, k, k)
        ws = torch.empty(int(need), dtype=torch.uint8, device=dev())
        if ws_fill is not None:
            ws.fill_(ws_fill)
        dw = torch.full((cout_r, cin_r, k, k), float("nan"), device=dev())
        db = torch.full((dyc,), float("nan"), device=dev())
        rec = WgradPending()
        if deferred:
            check(L().ymi_conv2d_bwd_weight_deferred(byref(xd), byref(dyd), cout_r, cin_r, k, k, s, ptr(dw), ptr(db), ptr(ws), ws.numel(),
                                                     ctypes.byref(rec), stream_ptr()), "bwd_weight_deferred")
        else:
            check(L().ymi_conv2d_bwd_weight(byref(xd), byref(dyd), cout_r, cin_r, k, k, s, ptr(dw), ptr(db), ptr(ws), ws.numel(), stream_ptr()),
                  "bwd_weight")
    return tag, rec, (exp, dbias_want, dw, db, ws, xd, dyd), (splits, lanes, slab16)


def wgrad_verify(tag, out):
    exp, dbias_want, dw, db, *_ = out
    G.check_exact(tag + " dW", dw, exp)
    G.check_exact(tag + " dbias", db, dbias_want)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_weight_gradient_tiles_splits_and_walks(dtype):
    acc = ([], [])
    for i, spec in enumerate(WGRAD):
        try:
            tag, _, out, _ = wgrad_case(dtype, spec, False, 900 + i)
            torch.cuda.synchronize()
            wgrad_verify(tag, out)
            print(tag + ": Gate 1 exact (dW, dbias)")
            acc[0].append(tag)
        except AssertionError as e:
            print("FAIL", e)
            acc[1].append(str(e))
    assert not acc[1], "\n\n".join(acc[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_weight_gradient_deferred_records_in_one_batched_sum(dtype):
    """every case as a deferred launch, all records summed by ONE ymi_wgrad_reduce_batch; each record's split count, lane count and
    slab type equal the plan's (the split force took effect)."""
    runs = []
    for i, spec in enumerate(WGRAD):
        tag, rec, out, plan = wgrad_case(dtype, spec, True, 900 + i)
        assert (rec.splits, rec.lanes, bool(rec.slab_bf16)) == plan, (tag, rec.splits, rec.lanes, rec.slab_bf16, plan)
        runs.append((tag, rec, out))
    recs = (WgradPending * len(runs))(*[r[1] for r in runs])
    table = torch.empty(len(runs) * ctypes.sizeof(WgradPending), dtype=torch.uint8, device=dev())
    check(L().ymi_wgrad_reduce_batch(recs, len(runs), ptr(table), stream_ptr()), "wgrad_reduce_batch")
    torch.cuda.synchronize()
    errs = []
    for tag, _, out in runs:
        try:
            wgrad_verify(tag, out)
            print(tag + ": Gate 1 exact (dW, dbias)")
        except AssertionError as e:
            print("FAIL", e)
            errs.append(str(e))
    assert not errs, "\n\n".join(errs)


@pytest.mark.parametrize("dtype,n,h,w,want_slab16", [(BF, 4, 64, 64, True), (BF, 1, 16, 32, False), (F32, 2, 32, 32, False)],
                         ids=["bf16-slabs", "bf16-f32-slabs", "f32"])
def test_weight_gradient_precision_gate2(dtype, n, h, w, want_slab16):
    """positive operands: |dW - ref| <= r * mag + (1 + r) gamma_(M + splits) * mag per element (mag = ref), r = 2^-8 where each split's
    partial sum is rounded once to a bfloat16 slab, 2^-24 for float32 slabs; dbias (float32 column sums of dY) within gamma_M of its sum.
    A second rounding, truncation or a bfloat16 accumulation fails."""
    g = torch.Generator().manual_seed(21)
    c, co, k = 16, 64, 3
    x = G.positive((n, c, h, w), g, dtype=dtype)
    dy = G.positive((n, co, h, w), g, dtype=dtype)
    bm, splits, slab16, lanes = G.wgrad_plan(n * h * w, co, k * k * c, dtype == BF)
    assert slab16 == want_slab16, (splits, slab16)
    xd, _ = on_dev(x, dtype)
    dyd, _ = on_dev(dy, dtype)
    need = L().ymi_conv2d_bwd_weight_workspace(n * h * w, co, c, k, k)
    ws = torch.empty(int(need), dtype=torch.uint8, device=dev())
    dw = torch.empty(co, c, k, k, device=dev())
    db = torch.empty(co, device=dev())
    check(L().ymi_conv2d_bwd_weight(byref(xd), byref(dyd), co, c, k, k, 1, ptr(dw), ptr(db), ptr(ws), ws.numel(), stream_ptr()), "bwd_weight")
    torch.cuda.synchronize()
    ref = G.wgrad64(x, dy, (co, c, k, k), 1)
    r = G.R_BF16 if slab16 else G.U32
    worst = G.check_bound("wgrad dW", dw, ref, r * ref + (1 + r) * G.gamma(n * h * w + splits) * ref)
    dbr = dy.double().sum((0, 2, 3))
    worst_b = G.check_bound("wgrad dbias", db, dbr, G.gamma(n * h * w + splits) * dbr)
    print(f"wgrad {dname(dtype)} {splits} splits, {'bf16' if slab16 else 'f32'} slabs: Gate 2 worst err/bound dW {worst:.3f} dbias {worst_b:.3f}")
