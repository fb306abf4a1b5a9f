"""CPU: the element-wise checks of tests/swin_mlp_exact.py on the fused SwinBlock MLP kernels (csrc/swin_mlp.hip) - the mirrors of the kernels'
bookkeeping, both gates against the float32 emulation of the kernels' rounding points on every case the GPU file runs, and planted faults
that the gates must flag with their location.

For the six faults that the tensor-wide gates of tests/test_gpu_swin_mlp_fused.py accept (out: relative L2 < 4e-3, its line 87, and max error
<= 2e-2 max |ref|, its line 85) at C = 256, T = 421, hidden = 1024 with that file's inputs, the acceptance is asserted too: it is the gap these
checks close."""
import re

import pytest
import torch

import swin_mlp_exact as X

OUT_L2, OUT_MAX = 4e-3, 2e-2  # tests/test_gpu_swin_mlp_fused.py:87 and :85 (tests/test_gpu_swin_mlp_widths.py:128 and :127)
C, T, HIDDEN = 256, 421, 1024


def _emu(o, ffault=None, bfault=None):
    f = X.emu_fwd(o, ffault)
    b = X.emu_bwd(o, f["pre"], bfault)
    got = dict(f)
    got.update(b)
    return got


def _gate1(o, got):
    X.gate1_check("planted", o, X.gate1_expected(o), got)


def _gate2(o, got):
    X.gate2_forward("planted", o, got)
    X.gate2_backward("planted", o, got["pre"], got)


def _raises(fn, *args):
    with pytest.raises(AssertionError) as e:
        fn(*args)
    assert not isinstance(e.value, X.NotExact), e.value
    return str(e.value)


def _locs(msg):
    """the (token, channel or unit) pairs a failure message lists"""
    return [(int(a), int(b)) for a, b in re.findall(r"\(token=(\d+), (?:channel|unit)=(\d+)\)", msg)]


def _count(msg):
    return int(re.search(r"(\d+) of \d+ elements wrong", msg).group(1))


@pytest.fixture(scope="module")
def g1():
    return X.gate1_operands(C, T, HIDDEN)


@pytest.fixture(scope="module")
def real():
    return X.real_operands(C, T, HIDDEN)


# ------------------------------------------------------------------------------------------------------------------------ 1. mirrors
def test_mirrors_of_the_configuration():
    assert [X.cfg(c).hidden_max for c in X.WIDTHS] == [8192, 8192, 4096]
    assert [(X.cfg(c).bm, X.cfg(c).nw) for c in X.WIDTHS] == [(256, 8), (256, 8), (128, 4)]
    assert X.cfg(256).lds_tile + 4 * 8192 == X.LDS_MAX  # the cap at C = 256 is exactly the CU's LDS
    assert sorted(X.unit_of_row(r) for r in range(32)) == list(range(32)) and sorted(X.unit_of_pos(p) for p in range(32)) == list(range(32))
    # the 16 results of lane half h (rows 8 q + 4 h + r) are the consecutive units 16 h + 4 q + r; k-step s takes units 16 h + 8 s + 0..7 from half h
    for h in range(2):
        assert [X.unit_of_row(8 * q + 4 * h + r) for q in range(4) for r in range(4)] == list(range(16 * h, 16 * h + 16))
        for s in range(2):
            assert [X.unit_of_pos(16 * s + 8 * h + j) for j in range(8)] == list(range(16 * h + 8 * s, 16 * h + 8 * s + 8))
    for c in X.WIDTHS:
        X.assert_coverage(c)


def test_mirrors_agree_with_the_library():
    from improving_yolov8_cbam_swinblock_amd import _lib as L

    if not L.LIB_PATH.exists():
        return  # not built: the mirrors above are all there is to check
    lib = L.lib()
    for c in X.WIDTHS + (64, 320, 512):
        for hidden in (0, 16, 32, 48, 96, 4 * c, 4096, 4128, 8192, 8224):
            assert bool(lib.ymi_swin_ln_mlp_supported(c, hidden, L.YMI_BF16)) == X.supported(c, hidden), (c, hidden)
            assert lib.ymi_swin_ln_mlp_pack_elems(c, hidden) == X.pack_elems(c, hidden)
        assert not lib.ymi_swin_ln_mlp_supported(c, 96, L.YMI_F32)
    for t in (1, 33, 128, 255, 256, 257, 421, 512, 56448):
        assert lib.ymi_swin_ln_mlp_pre_elems(t, 96) == X.pre_elems(t, 96)


@pytest.mark.parametrize("c", X.WIDTHS)
def test_pre_layout_decoder_and_weight_images(c):
    """decode_pre (a view and a permutation) inverts encode_pre (the kernel's address arithmetic); a 128-token tile of the narrow workgroup stays
    inside the 256-token padding; the weight images hold every weight once, where the kernel's fragment reads expect it"""
    k = X.cfg(c)
    for t, hidden in ((1, 32), (33, 96), (k.bm + 1, 64), (421, 224)):
        pre = torch.arange(t * hidden, dtype=torch.float32).view(t, hidden)
        priv = X.encode_pre(pre, c, fill=-1.0)
        assert priv.numel() == X.pre_elems(t, hidden)
        assert torch.equal(X.decode_pre(priv, c, t, hidden), pre)
    # token 32 w + l, unit 32 j + 16 h + 8 g + e of tile 0 sits at ((j NW + w) 2 + g) 512 + 8 (32 h + l) + e
    priv = X.encode_pre(torch.arange(64 * 96, dtype=torch.float32).view(64, 96), c)
    tok, unit = 32 * 1 + 5, 32 * 2 + 16 * 1 + 8 * 0 + 3
    assert priv[((2 * k.nw + 1) * 2 + 0) * 512 + 8 * (32 + 5) + 3] == tok * 96 + unit
    hidden = 64
    w1 = torch.arange(hidden * c, dtype=torch.float32).view(hidden, c) % 251
    w2 = (torch.arange(hidden * c, dtype=torch.float32).view(c, hidden) * 7) % 241
    img = X.pack_images(w1, w2).float().view(4, hidden // 32, -1)
    for i, src in enumerate((w1, w2, w2, w1)):
        assert sorted(img[i].reshape(-1).tolist()) == sorted(src.reshape(-1).tolist())
    # rows form, chunk 1, k-step 2, lane 37 (row 5 -> unit_of_row(5), lane half 1), element 6: w1[32 + unit][16 * 2 + 8 + 6]
    assert img[0, 1].view(c // 16, 64, 8)[2, 37, 6] == w1[32 + X.unit_of_row(5), 46]
    assert img[2, 1].view(c // 16, 64, 8)[2, 37, 6] == w2[46, 32 + X.unit_of_row(5)]
    # cols form, chunk 1, tile 3, step 1, lane 37 (channel 96 + 5), element 6: position 16 + 8 + 6
    assert img[1, 1].view(c // 32, 2, 64, 8)[3, 1, 37, 6] == w2[101, 32 + X.unit_of_pos(30)]
    assert img[3, 1].view(c // 32, 2, 64, 8)[3, 1, 37, 6] == w1[32 + X.unit_of_pos(30), 101]


def test_gate1_margins_over_the_value_set():
    """every multiple of 1/2 in [-2, 16]: gelu64 and gelu'64 lie at least MARGIN delta from a bfloat16 rounding boundary; below -3 they do not"""
    v = torch.arange(int(2 * X.PRE_LO), int(2 * X.PRE_HI) + 1).double() / 2
    mg, md = X._margins(v, X.gelu64, X.delta_gelu), X._margins(v, X.gelu_grad64, X.delta_grad)
    print(f"\n[swin_mlp margins] gelu {mg[0]:.1f} x delta at {mg[1]}, gelu' {md[0]:.1f} x delta at {md[1]}")
    assert mg[0] >= X.MARGIN and md[0] >= X.MARGIN
    low = torch.tensor([-4.0, -5.0], dtype=torch.float64)
    assert X._margins(low, X.gelu64, X.delta_gelu)[0] < X.MARGIN


# ------------------------------------------------------------------------------------------------- 2. the emulation passes both gates
@pytest.mark.parametrize("c", X.WIDTHS)
def test_emulation_passes_both_gates_on_every_case(c):
    worst = {}
    for cs in X.case_list(c):
        if cs.gate1:
            o = X.gate1_operands(c, cs.t, cs.hidden)
            got = _emu(o)
            _gate1(o, got)
            assert torch.equal(X.decode_pre(X.encode_pre(got["pre"], c), c, cs.t, cs.hidden), got["pre"])
        for xs in (1.0, 3.0):
            o = X.real_operands(c, cs.t, cs.hidden, xs)
            got = _emu(o)
            r = X.gate2_forward(f"emu C {c} {cs}", o, got)
            r.update(X.gate2_backward(f"emu C {c} {cs}", o, got["pre"], got))
            for n, v in r.items():
                worst[n] = max(worst.get(n, 0.0), v)
    print(f"\n[swin_mlp emulation C {c}] worst over {len(X.case_list(c))} cases: " + X.fmt_ratios(worst))


# ------------------------------------------------------------------------------------------------------------------- 3. planted faults
def test_fault_out_truncated(g1, real):
    msg = _raises(_gate2, real, _emu(real, ("out_trunc",)))
    assert "planted out [Gate 2" in msg and _count(msg) > 1000, msg
    assert "planted out [Gate 1" in _raises(_gate1, g1, _emu(g1, ("out_trunc",)))


def test_fault_rounded_twice(g1, real):
    msg = _raises(_gate2, real, _emu(real, ("double_round",)))
    assert "planted out [Gate 2" in msg and _count(msg) > 1000, msg
    assert "planted out [Gate 1" in _raises(_gate1, g1, _emu(g1, ("double_round",)))


def test_fault_accumulator_rounded_per_chunk(g1, real):
    msg = _raises(_gate2, real, _emu(real, ("acc_bf16_per_chunk",)))
    assert "planted out [Gate 2" in msg and _count(msg) > 1000, msg
    assert "planted out [Gate 1" in _raises(_gate1, g1, _emu(g1, ("acc_bf16_per_chunk",)))


def test_fault_b1_missing_for_one_unit(g1, real):
    unit = 32 * 17 + 21
    msg = _raises(_gate2, real, _emu(real, ("b1_missing", unit)))
    assert "planted pre [Gate 2" in msg and {j for _, j in _locs(msg)} == {unit} and "chunk 17 stage 2 half 1 g 0 e 5" in msg, msg
    unit = int(torch.nonzero(g1["b1"])[40])
    msg = _raises(_gate1, g1, _emu(g1, ("b1_missing", unit)))
    assert "planted pre [Gate 1" in msg and {j for _, j in _locs(msg)} == {unit} and _count(msg) == T, msg


def test_fault_b2_missing_on_four_channels_of_the_last_token(g1, real):
    ch0 = 4 * int(real["b2"].abs().view(-1, 4).amin(1).argmax())
    msg = _raises(_gate2, real, _emu(real, ("b2_missing", ch0)))
    assert "planted out [Gate 2" in msg and _count(msg) == 4 and set(_locs(msg)) == {(T - 1, ch0 + i) for i in range(4)}, msg
    ch0 = 4 * int(g1["b2"].abs().view(-1, 4).amin(1).argmax())
    msg = _raises(_gate1, g1, _emu(g1, ("b2_missing", ch0)))
    assert {t for t, _ in _locs(msg)} == {T - 1} and {ch for _, ch in _locs(msg)} <= set(range(ch0, ch0 + 4)), msg


def test_fault_tanh_gelu(g1, real):
    got = _emu(real, ("tanh_gelu",), ("tanh_gelu",))
    assert "planted out [Gate 2" in _raises(X.gate2_forward, "planted", real, got)
    assert "planted post [Gate 2" in _raises(X.gate2_backward, "planted", real, got["pre"], got)
    assert "planted post [Gate 1" in _raises(_gate1, g1, _emu(g1, ("tanh_gelu",), ("tanh_gelu",)))


def test_fault_hidden_units_swapped_in_fc2(g1, real):
    j1, j2 = 32 * 5 + 3, 32 * 5 + 20
    fed = set(torch.nonzero(g1["w2"][:, j1]).view(-1).tolist()) | set(torch.nonzero(g1["w2"][:, j2]).view(-1).tolist())
    msg = _raises(_gate1, g1, _emu(g1, ("swap_units", j1, j2)))
    assert "planted out [Gate 1" in msg and _locs(msg) and {ch for _, ch in _locs(msg)} <= fed, msg
    assert all("5" in re.findall(r"fed by chunks \[([^\]]*)\]", line)[0].split(", ") for line in msg.splitlines()[1:]), msg
    assert "planted out [Gate 2" in _raises(_gate2, real, _emu(real, ("swap_units", j1, j2)))


def test_fault_last_k_step_of_fc1_dropped_in_one_chunk(g1, real):
    jc = 9
    msg = _raises(_gate2, real, _emu(real, ("drop_last_kstep", jc)))
    assert "planted pre [Gate 2" in msg and {j // 32 for _, j in _locs(msg)} == {jc} and f"chunk {jc} stage {jc % 3}" in msg, msg
    last = C // 16 - 1
    jc = int((torch.nonzero((g1["w1"][:, 16 * last :] != 0).any(1)).view(-1) // 32)[0])
    msg = _raises(_gate1, g1, _emu(g1, ("drop_last_kstep", jc)))
    assert "planted pre [Gate 1" in msg and {j // 32 for _, j in _locs(msg)} == {jc}, msg
    assert all(str(last) in re.findall(r"fc1 k-steps \[([^\]]*)\]", line)[0].split(", ") for line in msg.splitlines()[1:]), msg


def test_fault_stale_ring_stage(g1, real):
    jc = 13
    msg = _raises(_gate1, g1, _emu(g1, ("stale_stage", jc)))
    assert "planted out [Gate 1" in msg and _locs(msg), msg
    for line in msg.splitlines()[1:]:
        chunks = set(re.findall(r"fed by chunks \[([^\]]*)\]", line)[0].split(", "))
        assert chunks & {str(jc), str(jc - 3)} and "stages" in line, line
    assert "planted out [Gate 2" in _raises(_gate2, real, _emu(real, ("stale_stage", jc)))


def test_fault_skip_of_the_last_token_from_the_clamped_row(g1, real):
    msg = _raises(_gate1, g1, _emu(g1, ("skip_clamped",)))
    assert "planted out [Gate 1" in msg and {t for t, _ in _locs(msg)} == {T - 1} and "wg 1 wave 5 lane32 4" in msg, msg
    msg = _raises(_gate2, real, _emu(real, ("skip_clamped",)))
    assert {t for t, _ in _locs(msg)} == {T - 1}, msg


def test_fault_accumulator_tile_misses_one_chunk_at_384():
    c, ct, jc = 384, 10, 4
    o = X.real_operands(c, 160, 224)
    msg = _raises(_gate2, o, _emu(o, ("tile_chunk_missing", ct, jc)))
    assert "planted out [Gate 2" in msg and {ch // 32 for _, ch in _locs(msg)} == {ct} and f"acc tile {ct}" in msg, msg
    o = X.gate1_operands(c, 160, 224)
    rows = torch.nonzero(o["w2"][32 * ct : 32 * ct + 32, 32 * jc : 32 * jc + 32].abs().sum(1)).view(-1)
    if len(rows):  # (the sparse Gate 1 weights feed this tile from this chunk)
        msg = _raises(_gate1, o, _emu(o, ("tile_chunk_missing", ct, jc)))
        assert {ch for _, ch in _locs(msg)} <= {32 * ct + int(r) for r in rows}, msg


def test_fault_d_post_not_rounded(g1, real):
    msg = _raises(_gate2, real, _emu(real, None, ("dpost_unrounded",)))
    assert "planted dpre [Gate 2" in msg and _count(msg) > 1000, msg
    _gate1(g1, _emu(g1, None, ("dpost_unrounded",)))  # (Gate 1's d_post is a power of two: only the per-element bound sees this one)


def test_fault_gelu_grad_sign_for_negative_x(g1, real):
    msg = _raises(_gate1, g1, _emu(g1, None, ("grad_sign",)))
    assert "planted dpre [Gate 1" in msg and re.findall(r"pre=(\S+):", msg) and all(float(v) < 0 for v in re.findall(r"pre=(\S+):", msg)), msg
    msg = _raises(_gate2, real, _emu(real, None, ("grad_sign",)))
    assert "planted dpre [Gate 2" in msg and all(float(v) < 0 for v in re.findall(r"pre=(\S+):", msg)), msg


# --------------------------------------------------------------------------------------------- 4. the gap: what the norm gates accept
def _fused_inputs(t, hidden, seed):
    """tests/test_gpu_swin_mlp_fused.py::_inputs on the host"""
    g = torch.Generator().manual_seed(seed)
    c = 256
    x = (torch.randn(t, c, generator=g) * 1.5 + 0.3).to(torch.bfloat16).float()
    gamma = torch.rand(c, generator=g) + 0.5
    beta = torch.randn(c, generator=g) * 0.3
    w1 = torch.randn(hidden, c, generator=g) / 16
    b1 = torch.randn(hidden, generator=g) * 0.2
    w2 = torch.randn(c, hidden, generator=g) / (hidden ** 0.5)
    b2 = torch.randn(c, generator=g) * 0.2
    return dict(c=c, t=t, hidden=hidden, x=x, gamma=gamma, beta=beta, eps=1e-5, w1=w1, b1=b1, w2=w2, b2=b2, dout=torch.zeros(t, c))


def _fused_reference_out(o):
    """tests/test_gpu_swin_mlp_fused.py::_reference: float64 with the product's storage roundings"""
    xd = o["x"].double()
    mu = xd.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + o["eps"])
    u = X.bf((xd - mu) * rs * o["gamma"].double() + o["beta"].double())
    pre = X.bf(u @ X.bf(o["w1"]).t() + o["b1"].double())
    post = X.bf(torch.nn.functional.gelu(pre))
    return post @ X.bf(o["w2"]).t() + o["b2"].double() + xd


def test_norm_gates_accept_the_six_table_faults():
    o = _fused_inputs(T, HIDDEN, T + HIDDEN)  # (the seed of test_fused_forward_against_float64)
    rout = _fused_reference_out(o)
    # the strongest group of four channels whose bias the max gate can still miss: max |b2| + one rounding of the largest output <= 2e-2 max |ref|
    grp = o["b2"].double().abs().view(-1, 4)
    room = (OUT_MAX - X.R) * rout.abs().max().item()
    ch0 = 4 * int(torch.where(grp.amax(1) <= room, grp.amin(1), torch.full_like(grp.amin(1), -1.0)).argmax())
    unit = int(o["b1"].abs().argsort()[HIDDEN // 2])  # a typical unit: the median |b1|
    faults = [None, ("out_trunc",), ("double_round",), ("acc_bf16_per_chunk",), ("b1_missing", unit), ("b2_missing", ch0), ("tanh_gelu",)]
    for fault in faults:
        got = _emu(o, fault, ("tanh_gelu",) if fault == ("tanh_gelu",) else None)
        e = (got["out"].double() - rout).abs().max().item() / rout.abs().max().item()
        rel = ((got["out"].double() - rout).norm() / rout.norm()).item()
        print(f"\n[swin_mlp norm gates] {fault}: max / max|ref| {e:.2e} (gate {OUT_MAX}) relative L2 {rel:.2e} (gate {OUT_L2})")
        assert e <= OUT_MAX and rel < OUT_L2, fault  # accepted by the tensor-wide gates ...
        if fault is not None:
            _raises(_gate2, o, got)  # ... and flagged element by element
        else:
            _gate2(o, got)
