"""Block 0 of the split-bf16 classifier (resblock_x3_kernel's 16x16x32 body) on its own, at every block-0 input height
the kernel is compiled for: its output against the float64 oracle applied to the GPU's own block-0 input."""
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import synth
from oracle import resnet as ores

pytestmark = pytest.mark.gpu

# feature-image rows -> block-0 input rows at 101 frames (block-0 input 25 columns): 16, 17, 22, 23, 24, 26, 27
HEIGHTS = {64: 16, 68: 17, 90: 22, 92: 23, 96: 24, 103: 26, 110: 27}


@pytest.mark.parametrize("rows", sorted(HEIGHTS))
def test_block0_against_float64_oracle(rows):
    sd = synth.random_state_dict(seed=11)
    m = cda.create_model("residual", n_mels=rows, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    m.load_state_dict(sd)
    m = m.cuda().eval()
    assert m.effective_dtype(rows, 101) == "bf16x3"
    g = torch.Generator().manual_seed(rows)
    n = 37
    x = (torch.randn(n, 1, rows, 101, generator=g) * 2.0).cuda()
    m(x)
    a1, a2 = m.read_activation(1).cpu(), m.read_activation(2).cpu()
    assert tuple(a1.shape[2:]) == (HEIGHTS[rows], 25)
    sd64 = {k: v.double() for k, v in sd.items()}
    want = ores.res_block(a1.double(), sd64, 0)
    err = (a2.double() - want).abs().max().item()
    print(f"{rows} rows (block 0 at {a1.shape[2]}x{a1.shape[3]}): max abs err {err:.2e} (ref max {want.abs().max():.2f})")
    assert a2.shape == want.shape and err < 5e-5 * max(1.0, want.abs().max().item())

    # batch invariance (block 0 runs one clip per workgroup): a sub-batch starting mid-batch, and a single clip, give
    # bit-identical block-0 outputs
    m(x[5:12])
    assert torch.equal(m.read_activation(2).cpu(), a2[5:12])
    m(x[n - 1:])
    assert torch.equal(m.read_activation(2).cpu(), a2[n - 1:])
