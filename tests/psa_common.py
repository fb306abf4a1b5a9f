"""What tests/golden/make_psa_golden.py and the tests that replay its fixtures share: the module cases (C3k / C3k2, the PSA attention blocks, the
non-legacy Detect head) and the seed-built state of the yolo11n end-to-end fixture (tests/golden_weights.py: no weights are stored there)."""
import torch

from golden_weights import seeded_inputs, seeded_state

# name -> (constructor name, positional arguments, keyword arguments, input channels, (H, W) of the input map); inputs are [2, C, H, W].
# The maps of the attention cases are chosen by their token count L = H * W against the kernel's 64-token tile.
CASES = {
    "psa_attention_64_h1": ("Attention", (64,), {"num_heads": 1}, 64, (7, 9)),                         # L 63: one ragged tile; kd 32, hd 64
    "psa_attention_64_h2": ("Attention", (64,), {"num_heads": 2, "attn_ratio": 0.5}, 64, (8, 8)),      # L 64: a full tile; kd 16, hd 32
    "psa_psablock_128_h2": ("PSABlock", (128,), {"num_heads": 2}, 128, (9, 8)),                        # L 72: crosses the tile edge
    "psa_psablock_64_h1_noshortcut": ("PSABlock", (64,), {"num_heads": 1, "shortcut": False}, 64, (6, 5)),
    "psa_c2psa_128_n1": ("C2PSA", (128, 128, 1), {}, 128, (10, 10)),                                   # L 100: ragged second tile
    "psa_c2psa_256_n2": ("C2PSA", (256, 256, 2), {}, 256, (5, 4)),                                     # two heads, two blocks
    "psa_c3k_32_32_n2": ("C3k", (32, 32, 2), {}, 32, (12, 10)),
    "psa_c3k2_64_64_n2": ("C3k2", (64, 64, 2, False), {}, 64, (12, 10)),                               # Bottleneck members, default shortcut
    "psa_c3k2_64_64_n2_c3k": ("C3k2", (64, 64, 2, True), {}, 64, (12, 10)),                            # C3k members
    "psa_c3k2_32_64_n1_e025": ("C3k2", (32, 64, 1, False, 0.25), {}, 32, (12, 10)),
}
# cases whose weights and gradients would not fit a committed file: weights and inputs are rebuilt from CASE_SEED + position in CASES
# (golden_weights.seeded_state / seeded_inputs), parameter gradients are stored as golden_weights.grad_record entries
SEEDED_ABOVE = 60000  # parameters
CASE_SEED = 3100

DETECT_CASE = "psa_detect_nc3"  # Detect(3, (32, 64, 128)) with legacy = False on [2, C, h, w] maps; always seeded
DETECT_NC, DETECT_CH, DETECT_HW, DETECT_STRIDE, DETECT_SEED = 3, (32, 64, 128), ((8, 6), (4, 3), (2, 2)), (8.0, 16.0, 32.0), 3199

E2E_SEED, E2E_NC, E2E_BATCH, E2E_SIZE = 31, 3, 2, 128
SCALES = ("n", "s", "m")


def case_seed(name):
    return CASE_SEED + list(CASES).index(name)


def build(M, name):
    ctor, args, kwargs, _, _ = CASES[name]
    return getattr(M, ctor)(*args, **kwargs)


def is_seeded(module):
    return sum(p.numel() for p in module.parameters()) > SEEDED_ABOVE


def seeded_module_state(module, seed):
    """every floating tensor of the state dict from the seed (running variances made positive: |v| + 0.5); counters and Detect's frozen DFL
    weights stay as constructed."""
    sd = module.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if v.dtype.is_floating_point and ".dfl." not in k and not k.startswith("dfl.")}
    st = seeded_state(shapes, seed)
    for k in st:
        if k.endswith("running_var"):
            st[k] = st[k].abs() + 0.5
    return {**{k: v.clone() for k, v in sd.items()}, **st}


def case_inputs(name, out_channels=None):
    """(x, gy) of a seeded module case; gy has the output's shape (every case keeps the map size; out_channels defaults to the input's)."""
    _, _, _, cin, (h, w) = CASES[name]
    return seeded_inputs(case_seed(name), (2, cin, h, w), (2, out_channels or cin, h, w))


def detect_inputs(no):
    """([x per level], [gy per level]) of the Detect case; no = 64 + nc output channels."""
    xs, gys = [], []
    for i, (c, (h, w)) in enumerate(zip(DETECT_CH, DETECT_HW)):
        x, gy = seeded_inputs(DETECT_SEED + 10 * i, (2, c, h, w), (2, no, h, w))
        xs.append(x)
        gys.append(gy)
    return xs, gys


def e2e_state(model):
    return seeded_module_state(model, E2E_SEED)


def e2e_batch():
    img, _ = seeded_inputs(E2E_SEED, (E2E_BATCH, 3, E2E_SIZE, E2E_SIZE), (1,))
    img = (img * 0.25 + 0.5).clamp(0, 1)
    g = torch.Generator().manual_seed(E2E_SEED)
    nb = 3
    ctr = torch.rand(E2E_BATCH * nb, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(E2E_BATCH * nb, 2, generator=g) * 0.3 + 0.05
    return {"img": img, "batch_idx": torch.arange(E2E_BATCH).repeat_interleave(nb).float(),
            "cls": torch.randint(0, E2E_NC, (E2E_BATCH * nb, 1), generator=g).float(), "bboxes": torch.cat((ctr, wh), 1)}
