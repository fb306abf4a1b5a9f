"""GPU: the move_kernel family and the layout pair of csrc/elementwise.hip, bit for bit.

ymi_copy, ymi_upsample2x, ymi_upsample2x_bwd, ymi_upsample2x_bwd_acc, ymi_add_inplace through the C ABI (YmiTensors built by hand) against
torch float32 on the CPU written in the kernel's order - no multiplication anywhere, so contraction cannot change a bit:
  copy, upsample2x      round(src)
  upsample2x_bwd        round((a + b) + (c + e)), a b the upper pair and c e the lower pair of the 2 x 2 block
  add_inplace           round(src + dst)
  upsample2x_bwd_acc    round(((a + b) + (c + e)) + dst)
crossed with the four dtype pairs and with the vector path (c = 8 dense; ld > c on either side) and the scalar path by each of its
triggers (c = 6; ld = 10; a base 2 elements off) on either side; N = 2, 3 x 5 <-> 6 x 10.  Pad channels and guard words keep their bits,
the source keeps its.  One case of more than 2^20 groups for the grid-stride second trip.  ymi_nchw_to_nhwc (image path and general
path, zero pad channels below dst->c) and ymi_nhwc_to_nchw likewise; shape mismatches are refused with the destination untouched."""
import ctypes

import pytest
import torch

from improving_yolov8_cbam_swinblock_amd._lib import YMI_BF16, YMI_F32, YmiTensor, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SENTINEL, GUARD = -99.0, 64
YMI_EINVAL = -1
PAIRS = [(F32, F32), (BF, BF), (F32, BF), (BF, F32)]
# name -> (c, (source ld, elements the source starts into its buffer), (destination ld, lead), vector path?)
LAYOUTS = {
    "vec": (8, (8, 0), (8, 0), True),
    "vec_src_ld12": (8, (12, 0), (8, 0), True),
    "vec_dst_ld12": (8, (8, 0), (12, 0), True),
    "scalar_c6": (6, (6, 0), (6, 0), False),
    "scalar_c6_ld8": (6, (8, 0), (10, 0), False),
    "scalar_src_ld10": (8, (10, 0), (8, 0), False),
    "scalar_dst_ld10": (8, (8, 0), (10, 0), False),
    "scalar_src_base2": (8, (8, 2), (8, 0), False),
    "scalar_dst_base2": (8, (12, 0), (8, 2), False),
}
ENTRY = {"copy": "ymi_copy", "upsample2x": "ymi_upsample2x", "upsample2x_bwd": "ymi_upsample2x_bwd", "upsample2x_bwd_acc": "ymi_upsample2x_bwd_acc",
         "add_inplace": "ymi_add_inplace"}


def dev():
    return torch.device("cuda:0")


def dname(dtype):
    return "bf16" if dtype == BF else "f32"


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Map:
    """[N, H, W, c] with pixel stride ld, starting `lead` elements into a sentinel-filled buffer that ends in guard words."""

    def __init__(self, shape, dtype, ld=None, lead=0, values=None):
        N, H, W, c = shape
        self.shape, self.dtype, self.ld, self.lead = shape, dtype, ld or c, lead
        self.span = N * H * W * self.ld
        self.buf = torch.full((lead + self.span + GUARD,), SENTINEL, dtype=dtype, device=dev())
        assert self.buf.data_ptr() % 16 == 0
        self.view = self._slice(self.buf)
        self.view.copy_(values.to(dev()) if values is not None else torch.full(shape, float("nan")))
        self.before = self.buf.clone()

    def _slice(self, buf):
        N, H, W, c = self.shape
        return buf[self.lead : self.lead + self.span].view(N, H, W, self.ld)[..., :c]

    def ymi(self, **over):
        N, H, W, c = self.shape
        f = dict(n=N, h=H, w=W, c=c, ld=self.ld)
        f.update(over)
        return YmiTensor(self.view.data_ptr(), f["n"], f["h"], f["w"], f["c"], f["ld"], YMI_BF16 if self.dtype == BF else YMI_F32, 0)

    def vec4_ok(self):
        return self.shape[3] % 4 == 0 and self.ld % 4 == 0 and self.view.data_ptr() % (4 * self.view.element_size()) == 0

    def check(self, what, expected=None):
        """expected None: nothing at all changed; else the slice holds expected's bits and the rest (pads, lead, guards) did not change."""
        now = self.buf.clone()
        if expected is not None:
            got = self.view.cpu()
            bad = bits(got) != bits(expected)
            if bool(bad.any()):
                idx = [tuple(int(i) for i in r) for r in bad.nonzero()[:5]]
                lines = [f"  (n, h, w, c) = {i}: got {float(got[i])!r} expected {float(expected[i])!r}" for i in idx]
                raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first:\n" + "\n".join(lines))
            self._slice(now).copy_(self._slice(self.before))
        assert torch.equal(bits(now), bits(self.before)), f"{what}: words outside the tensor changed"


def rnd(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


def quad(s):
    """(a + b) + (c + e) over the 2 x 2 blocks of s [N, 2h, 2w, c] in float32: a b the upper pair, c e the lower."""
    return (s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + (s[:, 1::2, 0::2] + s[:, 1::2, 1::2])


def expected_of(entry, src, dst, ddt):
    s, d = src.float(), dst.float()
    if entry == "copy":
        v = s
    elif entry == "upsample2x":
        v = s.repeat_interleave(2, 1).repeat_interleave(2, 2)
    elif entry == "upsample2x_bwd":
        v = quad(s)
    elif entry == "add_inplace":
        v = s + d
    else:
        v = quad(s) + d
    return v.to(ddt)


def shapes_of(entry, N, h, w, c):
    """(source shape, destination shape), h x w the small side."""
    small, large = (N, h, w, c), (N, 2 * h, 2 * w, c)
    return {"copy": (small, small), "add_inplace": (small, small), "upsample2x": (small, large), "upsample2x_bwd": (large, small),
            "upsample2x_bwd_acc": (large, small)}[entry]


def run_move(entry, sdt, ddt, N, h, w, c, sl=(None, 0), dl=(None, 0), vec=None, seed=0):
    sshape, dshape = shapes_of(entry, N, h, w, c)
    sv, dv = rnd(sshape, sdt, 2 * seed + 1), rnd(dshape, ddt, 2 * seed + 2)
    src = Map(sshape, sdt, sl[0], sl[1], sv)
    dst = Map(dshape, ddt, dl[0], dl[1], dv if entry in ("add_inplace", "upsample2x_bwd_acc") else None)
    if vec is not None:
        assert (src.vec4_ok() and dst.vec4_ok()) == vec
    what = f"{entry} {dname(sdt)}->{dname(ddt)} {sshape}->{dshape} ld {src.ld},{dst.ld} lead {src.lead},{dst.lead}"
    rc = getattr(lib(), ENTRY[entry])(ctypes.byref(src.ymi()), ctypes.byref(dst.ymi()), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (what, lib().ymi_last_error())
    dst.check(what + " dst", expected_of(entry, sv, dv, ddt))
    src.check(what + " src")


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{dname(p[0])}-{dname(p[1])}")
@pytest.mark.parametrize("entry", list(ENTRY))
def test_map_moves_bit_exact_in_every_layout(entry, pair):
    for i, (name, (c, sl, dl, vec)) in enumerate(LAYOUTS.items()):
        run_move(entry, pair[0], pair[1], 2, 3, 5, c, sl, dl, vec, seed=i)


@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
@pytest.mark.parametrize("entry", ["copy", "upsample2x_bwd_acc"])
def test_map_moves_grid_stride_second_trip(entry, dtype):
    """1026 x 1024 pixels of one 4-channel group each: 2048 groups more than the 4096 x 256 threads of the capped grid."""
    assert 1026 * 1024 * (4 // 4) > 256 * 16 * 256
    run_move(entry, dtype, dtype, 1, 1026, 1024, 4, vec=True)


@pytest.mark.parametrize("C,c,dtype,ld", [(3, 4, F32, 4), (3, 8, BF, 8), (3, 8, BF, 16), (3, 8, BF, 12), (5, 8, F32, 8), (5, 8, F32, 12), (12, 16, BF, 16),
                                          (12, 16, BF, 20)], ids=lambda v: dname(v) if isinstance(v, torch.dtype) else str(v))
def test_nchw_to_nhwc_bit_exact_with_zero_pad_channels(C, c, dtype, ld):
    """(3, 8, bf16, ld 8 / 16): the image path (one 16-byte chunk a pixel); ld 12 takes the general path, as do the others.  Channels
    C .. c - 1 are written as zeros, channels c .. ld - 1 keep their bits."""
    N, H, W = 2, 5, 7
    sv = rnd((N, C, H, W), F32, 40 + C + ld)
    src = sv.to(dev()).contiguous()
    dst = Map((N, H, W, c), dtype, ld)
    rc = lib().ymi_nchw_to_nhwc(ptr(src), N, C, H, W, ctypes.byref(dst.ymi()), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().ymi_last_error()
    exp = torch.zeros((N, H, W, c))
    exp[..., :C] = sv.permute(0, 2, 3, 1)
    dst.check(f"nchw_to_nhwc C={C} c={c} {dname(dtype)} ld={ld}", exp.to(dtype))
    assert torch.equal(src.cpu(), sv)


@pytest.mark.parametrize("dtype", [F32, BF], ids=dname)
@pytest.mark.parametrize("c,ld", [(6, 6), (6, 10), (8, 8), (8, 12)])
def test_nhwc_to_nchw_bit_exact(c, ld, dtype):
    N, H, W = 2, 5, 7
    sv = rnd((N, H, W, c), dtype, 60 + c + ld)
    src = Map((N, H, W, c), dtype, ld, 0, sv)
    n = N * c * H * W
    dst = torch.full((n + GUARD,), float("nan"), device=dev())
    rc = lib().ymi_nhwc_to_nchw(ctypes.byref(src.ymi()), ptr(dst), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib().ymi_last_error()
    assert bool(torch.isnan(dst[n:]).all()), "written past the end"
    assert torch.equal(bits(dst[:n].cpu().view(N, c, H, W)), bits(sv.float().permute(0, 3, 1, 2)))
    src.check("nhwc_to_nchw src")


def test_map_moves_refuse_mismatched_shapes():
    small, large = (2, 3, 5, 8), (2, 6, 10, 8)
    s, l = Map(small, F32, values=rnd(small, F32, 1)), Map(large, F32, values=rnd(large, F32, 2))
    d_small, d_large = Map(small, F32), Map(large, F32)
    L = lib()

    def refused(rc, dst, what):
        torch.cuda.synchronize()
        assert rc == YMI_EINVAL, f"{what}: returned {rc}"
        dst.check(what)

    for over in (dict(n=1), dict(h=2), dict(w=4), dict(c=4)):
        refused(L.ymi_copy(ctypes.byref(s.ymi()), ctypes.byref(d_small.ymi(**over)), stream_ptr()), d_small, f"copy {over}")
        refused(L.ymi_add_inplace(ctypes.byref(s.ymi()), ctypes.byref(d_small.ymi(**over)), stream_ptr()), d_small, f"add_inplace {over}")
    refused(L.ymi_upsample2x(ctypes.byref(s.ymi()), ctypes.byref(d_small.ymi()), stream_ptr()), d_small, "upsample2x onto its own size")
    for over in (dict(n=1), dict(h=5), dict(w=9), dict(c=4)):
        refused(L.ymi_upsample2x(ctypes.byref(s.ymi()), ctypes.byref(d_large.ymi(**over)), stream_ptr()), d_large, f"upsample2x {over}")
        refused(L.ymi_upsample2x_bwd(ctypes.byref(l.ymi(**over)), ctypes.byref(d_small.ymi()), stream_ptr()), d_small, f"upsample2x_bwd {over}")
        refused(L.ymi_upsample2x_bwd_acc(ctypes.byref(l.ymi(**over)), ctypes.byref(d_small.ymi()), stream_ptr()), d_small, f"upsample2x_bwd_acc {over}")
    refused(L.ymi_upsample2x_bwd(ctypes.byref(s.ymi()), ctypes.byref(d_small.ymi()), stream_ptr()), d_small, "upsample2x_bwd from its own size")
    src = rnd((2, 5, 3, 5), F32, 3).to(dev())  # NCHW, 5 channels
    for args, what in (((2, 5, 3, 5), "dst->c 4 < C 5"), ((1, 3, 3, 5), "n"), ((2, 3, 4, 5), "h"), ((2, 3, 3, 4), "w")):
        d4 = Map((2, 3, 5, 4), F32)
        refused(L.ymi_nchw_to_nhwc(ptr(src), *args, ctypes.byref(d4.ymi()), stream_ptr()), d4, f"nchw_to_nhwc {what}")
    d6 = Map((2, 3, 5, 6), F32)
    refused(L.ymi_nchw_to_nhwc(ptr(src), 2, 5, 3, 5, ctypes.byref(d6.ymi()), stream_ptr()), d6, "nchw_to_nhwc into 6 channels (not 4-aligned)")
    assert L.ymi_nhwc_to_nchw(ctypes.byref(s.ymi()), None, stream_ptr()) == YMI_EINVAL
