"""The border selects of the split-bf16 residual blocks, per pixel, at the block instantiations that
tests/test_gpu_resblock_borders.py does not reach: block 0 at 17, 23, 24, 26 and 27 rows, block 1 at 9, 12, 13 and 14 rows.

In the 16x16x32 body a tap outside the image is redirected to a zero cell by one v_cndmask_b32 whose 64-lane mask is a
compile-time constant per (tile, tap) (csrc/rbx_taps.h: rbx_tap_mask; conv2 everywhere, conv1 and the projection where the
x planes carry no border).  A wrong mask bit reads a neighbouring pixel, or a stale cell, instead of zero -- or zero
instead of a pixel -- and shows as a per-pixel excess on inputs whose border pixels are large or whose neighbour clip is
not zero.  Three clips, so that a two-clip workgroup runs half empty.

The construction is that of test_gpu_resblock_borders (transparent stem, and a transparent block 0 in front of block 1);
the bound is the derived per-pixel bound of resnet_layer_ref against the float64 block over the GPU's own block input."""
import pytest
import torch

import resnet_layer_ref as R
import test_gpu_resblock_borders as TB

pytestmark = pytest.mark.gpu

FRAMES, B = TB.FRAMES, TB.B
# block under test, image rows, its input, body, clips per workgroup
SHAPES = [(0, 68, (17, 25), "16x16x32", 1), (0, 92, (23, 25), "16x16x32", 1), (0, 96, (24, 25), "16x16x32", 1),
          (0, 104, (26, 25), "16x16x32", 1), (0, 110, (27, 25), "32x32", 1),
          (1, 68, (9, 13), "16x16x32", 2), (1, 92, (12, 13), "16x16x32", 2), (1, 104, (13, 13), "16x16x32", 1),
          (1, 110, (14, 13), "16x16x32", 1)]
PATTERNS = ("last_row_and_column", "first_row_and_column", "zero_clip_between_random")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("blk,rows,hw,body,clips", SHAPES, ids=[f"block{b}-{h}x{w}" for b, _, (h, w), _, _ in SHAPES])
def test_selects_per_pixel(blk, rows, hw, body, clips, pattern):
    assert B == 3
    st = R.plan("bf16x3", rows, FRAMES).blocks[blk]
    assert (st.kernel, st.body, st.in_hw, st.clips) == ("resblock_x3", body, hw, clips)
    sd, m = TB._weights(blk), TB._model(blk, rows)
    u = TB._pattern(pattern, hw, 7 * rows + blk)
    if pattern == "zero_clip_between_random":
        # non-zero data in every border pixel of the outer clips, a zero clip between them
        ring = torch.ones(hw, dtype=torch.bool)
        ring[1:-1, 1:-1] = False
        assert bool((u[0][:, ring] != 0).all()) and bool((u[2][:, ring] != 0).all()) and not bool(u[1].any())
    x = TB._image(blk, rows, u).cuda()
    m(x)
    a_in, a_out = m.read_activation(blk + 1).cpu(), m.read_activation(blk + 2).cpu()
    # the crafted input reached the block: non-zero exactly where the pattern is
    assert tuple(a_in.shape[2:]) == hw
    assert torch.equal((a_in != 0).any(dim=1), (u != 0).any(dim=1)) and bool((a_in >= 0).all())
    assert torch.equal((a_in != 0).all(dim=1), (u != 0).any(dim=1))
    w = R.check_stage(blk, st.kernel, a_out, R.block(a_in, sd, blk), R.stage_bound(blk, a_in, sd, st.scheme))
    print(f"block {blk} at {hw[0]}x{hw[1]} {pattern}: worst GPU / bound {w.ratio:.4f} at clip {w.clip} ch {w.channel} row {w.row} "
          f"col {w.col} (err {w.err:.3e}, bound {w.bound:.3e}, input max {float(a_in.max()):.1f})")
    assert w.ratio <= 1.0, w
    if pattern == "zero_clip_between_random":
        # nothing is read across the clip pitch: the all-zero clip alone (first in its workgroup) gives the same bits
        m(x[1:2])
        assert torch.equal(a_out[1:2], m.read_activation(blk + 2).cpu())
