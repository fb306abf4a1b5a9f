"""GPU: window attention at head_dim 196..256 (SwinBlock(512, 2): head_dim 256) checked element by element, through the harness of
tests/test_gpu_swin_exact.py: three windows, sentinel-filled outputs, every lse entry written, each form run twice bit-identical, a forward
without lse, Gate 1 (one-hot attention, bit for bit) where constructible and Gate 2 (attn_exact's per-element float64 bound, unchanged) on
N(0, 1) operands and on the x3 q / k variant.

Above head_dim 192 the dispatch is: bfloat16 windows of at most 64 tokens -> the tr kernels (16 head-dimension tiles); float32 -> the tiled
kernels at every window length (its one-tile backward image no longer fits the LDS); more than 64 tokens or attn_tiled = 1 -> tiled.  The tag
attn_case prints takes its form name from attn_exact.attn_form, which covers hd <= 192 and reads 'onetile-f32' for float32 windows of at most
64 tokens; the bound formula is the same for every form but tr, and the form that really runs is printed beside it."""
import ctypes

import pytest
import torch

from improving_yolov8_cbam_swinblock_amd._lib import as_ymi, lib, ptr, stream_ptr
from test_gpu_swin_exact import BF, F32, SENTINEL, attn_case, dev, dname
from test_swin512_cpu import form_above_192

pytestmark = pytest.mark.gpu

# (dtype, L, hd, heads, attn_tiled, layout, seed)
CASES = [
    # bfloat16, one tile: tr
    (BF, 49, 256, 2, 0, "dense", 2561),      # the model's launch
    (BF, 64, 256, 1, 0, "wide_ld", 2562),    # the full tile: the largest LDS image (153,600 B backward)
    (BF, 1, 196, 3, 0, "qkv_off4", 2563),    # 8-byte staging, hd != hdp
    (BF, 33, 200, 2, 0, "qkv_ld+4", 2564),
    (BF, 63, 252, 1, 0, "qkv_ld+8", 2565),
    (BF, 16, 224, 2, 0, "dense", 2566),
    # float32 at L <= 64: tiled now
    (F32, 49, 256, 2, 0, "dense", 2567),
    (F32, 64, 196, 1, 0, "wide_ld", 2568),
    (F32, 9, 252, 3, 0, "qkv_off4", 2569),
    # bfloat16 with attn_tiled = 1
    (BF, 49, 256, 2, 1, "dense", 2570),
    # bfloat16, natural tiled
    (BF, 65, 256, 2, 0, "dense", 2571),
    (BF, 196, 224, 1, 0, "qkv_ld+4", 2572),
    (BF, 100, 200, 3, 0, "qkv_off4", 2573),
    # float32, natural tiled
    (F32, 65, 256, 1, 0, "wide_ld", 2574),
    (F32, 196, 196, 2, 0, "dense", 2575),
    (F32, 256, 256, 1, 0, "dense", 2576),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{dname(c[0])}-L{c[1]}-hd{c[2]}-h{c[3]}-t{c[4]}-{c[5]}" for c in CASES])
def test_attention_form_above_head_dim_192(case):
    dtype, L, hd, heads, force, layout, seed = case
    print(attn_case(*case) + f" [runs: {form_above_192(L, hd, dtype, force)}, 16 head-dimension tiles]")


def test_head_dim_above_256_is_refused_without_a_launch():
    """head_dim 260 and 512, forward and backward: a non-zero return, an error text that names the limit, and outputs that keep their fill."""
    d = dev()
    for dtype in (BF, F32):
        for hd in (260, 512):
            T, L, heads = 16, 16, 1
            qkv = torch.zeros(T, 3 * hd, dtype=dtype, device=d)
            out = torch.full((T, hd), SENTINEL, dtype=dtype, device=d)
            dout = torch.zeros(T, hd, dtype=dtype, device=d)
            dqkv = torch.full((T, 3 * hd), SENTINEL, dtype=dtype, device=d)
            lse = torch.full((T * heads,), SENTINEL, device=d)
            by = lambda t: ctypes.byref(as_ymi(t))  # noqa: E731
            rc = lib().ymi_window_attention_fwd(by(qkv), L, heads, by(out), ptr(lse), stream_ptr())
            msg = lib().ymi_last_error().decode()
            assert rc != 0 and "head_dim" in msg and "256" in msg, (hd, rc, msg)
            rc = lib().ymi_window_attention_bwd(by(qkv), by(out), by(dout), ptr(lse), L, heads, by(dqkv), stream_ptr())
            msg = lib().ymi_last_error().decode()
            assert rc != 0 and "head_dim" in msg and "256" in msg, (hd, rc, msg)
            torch.cuda.synchronize()
            for name, t in (("out", out), ("dqkv", dqkv), ("lse", lse)):
                assert bool((t.float() == SENTINEL).all()), f"head_dim {hd} {dname(dtype)}: {name} was written"
