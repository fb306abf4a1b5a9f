"""What tests/golden/make_ghost_golden.py and the tests that replay its fixtures share: the module cases and the seed-built state of the
yolov8s-ghost end-to-end fixture (tests/golden_weights.py: no weights are stored)."""
import torch

from golden_weights import seeded_inputs, seeded_state

# name -> (constructor name, arguments, input channels); inputs are [2, C, 12, 10]
CASES = {
    "ghost_dwconv_16_k3_s1": ("DWConv", (16, 16, 3, 1), 16),
    "ghost_dwconv_16_k3_s2_noact": ("DWConv", (16, 16, 3, 2, 1, False), 16),
    "ghost_dwconv_8_k5_s1": ("DWConv", (8, 8, 5, 1), 8),
    "ghost_ghostconv_16_32_k1_s1": ("GhostConv", (16, 32, 1, 1), 16),
    "ghost_ghostconv_16_32_k3_s2": ("GhostConv", (16, 32, 3, 2), 16),
    "ghost_ghostconv_32_16_noact": ("GhostConv", (32, 16, 1, 1, 1, False), 32),
    "ghost_bottleneck_32_32": ("GhostBottleneck", (32, 32), 32),
    "ghost_bottleneck_16_32_k3_s2": ("GhostBottleneck", (16, 32, 3, 2), 16),
    "ghost_c3_32_32_n2": ("C3", (32, 32, 2, True), 32),
    "ghost_c3ghost_64_64_n2": ("C3Ghost", (64, 64, 2), 64),
}
INPUT_HW = (12, 10)

E2E_SEED, E2E_NC, E2E_BATCH, E2E_SIZE = 21, 3, 2, 128
SCALES = ("n", "s", "m")


def e2e_state(model):
    """the seeded state of a ghost model: every floating tensor from seeded_state, running variances made positive (|v| + 0.5); Detect's frozen
    DFL weights and the batch counters stay as constructed."""
    sd = model.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if v.dtype.is_floating_point and ".dfl." not in k}
    st = seeded_state(shapes, E2E_SEED)
    for k in st:
        if k.endswith("running_var"):
            st[k] = st[k].abs() + 0.5
    return {**{k: v.clone() for k, v in sd.items()}, **st}


def e2e_batch():
    img, _ = seeded_inputs(E2E_SEED, (E2E_BATCH, 3, E2E_SIZE, E2E_SIZE), (1,))
    img = (img * 0.25 + 0.5).clamp(0, 1)
    g = torch.Generator().manual_seed(E2E_SEED)
    nb = 3
    ctr = torch.rand(E2E_BATCH * nb, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(E2E_BATCH * nb, 2, generator=g) * 0.3 + 0.05
    return {"img": img, "batch_idx": torch.arange(E2E_BATCH).repeat_interleave(nb).float(),
            "cls": torch.randint(0, E2E_NC, (E2E_BATCH * nb, 1), generator=g).float(), "bboxes": torch.cat((ctr, wh), 1)}
