"""Block 1 of the split-bf16 classifier (resblock_x3_kernel<64, 128, G, R, 13>) and its fused head, at every block-1 input
height the kernel is compiled for: its output against the float64 oracle applied to the GPU's own block-1 input, the
logits against the float64 head applied to the GPU's own block-1 output, and batch invariance across the clip pairs of
a two-clip workgroup."""
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import synth
from oracle import resnet as ores

pytestmark = pytest.mark.gpu

# feature-image rows -> block-1 input rows at 101 frames (block-1 input 13 columns): 8, 9, 11, 12, 12, 13, 14
HEIGHTS = {64: 8, 68: 9, 90: 11, 92: 12, 96: 12, 103: 13, 110: 14}


@pytest.mark.parametrize("rows", sorted(HEIGHTS))
def test_block1_against_float64_oracle(rows):
    sd = synth.random_state_dict(seed=13)
    m = cda.create_model("residual", n_mels=rows, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    m.load_state_dict(sd)
    m = m.cuda().eval()
    assert m.effective_dtype(rows, 101) == "bf16x3"
    g = torch.Generator().manual_seed(100 + rows)
    n = 37   # odd: with two clips per workgroup the last workgroup holds one clip
    x = (torch.randn(n, 1, rows, 101, generator=g) * 2.0).cuda()
    logits = m(x).cpu()
    a2, a3 = m.read_activation(2).cpu(), m.read_activation(3).cpu()
    assert tuple(a2.shape[2:]) == (HEIGHTS[rows], 13)
    sd64 = {k: v.double() for k, v in sd.items()}
    want = ores.res_block(a2.double(), sd64, 1)
    err = (a3.double() - want).abs().max().item()
    print(f"{rows} rows (block 1 at {a2.shape[2]}x{a2.shape[3]}): max abs err {err:.2e} (ref max {want.abs().max():.2f})")
    assert a3.shape == want.shape and err < 5e-5 * max(1.0, want.abs().max().item())

    # the fused head: global mean -> Linear(128, 2) of the block's own output
    want_l = ores.head(a3.double(), sd64)
    lerr = (logits.double() - want_l).abs().max().item()
    assert logits.shape == (n, 2) and lerr < 1e-5 * max(1.0, want_l.abs().max().item()), lerr

    # batch invariance: a sub-batch starting mid-batch (the clip pairs of the workgroups shift by one), and a single
    # clip, give bit-identical block-1 outputs and logits
    for lo, hi in ((5, 12), (n - 1, n)):
        sub = m(x[lo:hi]).cpu()
        assert torch.equal(m.read_activation(3).cpu(), a3[lo:hi])
        assert torch.equal(sub, logits[lo:hi])
