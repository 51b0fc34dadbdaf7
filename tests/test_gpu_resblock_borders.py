"""The borders of the split-bf16 residual blocks (resblock_x3_kernel's 16x16x32 body), per pixel, on inputs a wrong border
shows up in: block 0 at 16x25 and 22x25 (bordered x planes, csrc/resnet_plan.h: rbx_border_x), block 1 at 8x13 and 11x13
(two clips per workgroup; three clips, so the last workgroup is half empty).

A block can only be reached through the net, so the net in front of it is made transparent: the stem copies pixels
(channel c takes pixel (2i + dy, 2j + dx) of the image, (dy, dx) by c % 4, times a scale of its own; no bias, identity
BatchNorm), so after the max-pool a1[c, r, q] = s_c * V[c % 4, r, q] for a non-negative pattern V written into the image at
(4r + dy, 4q + dx); for block 1, block 0 passes a1's even pixels through its projection (conv1 and conv2 zero).  The
block under test has random weights and BatchNorm statistics.  Its output is held to the derived per-pixel bound of
resnet_layer_ref against the float64 block over the GPU's own block input, whose zero pattern is asserted first."""
import functools

import pytest
import torch

import cough_detector_amd as cda
import resnet_layer_ref as R
from cough_detector_amd import synth

pytestmark = pytest.mark.gpu

FRAMES, B = 101, 3
# block under test, image rows, its input
SHAPES = [(0, 64, (16, 25)), (0, 90, (22, 25)), (1, 64, (8, 13)), (1, 90, (11, 13))]
PATTERNS = ("last_row_and_column", "first_row_and_column", "zero_clip_between_random")


def _identity_bn(sd, name):
    c = sd[name + ".weight"].shape[0]
    sd[name + ".weight"], sd[name + ".bias"] = torch.ones(c), torch.zeros(c)
    sd[name + ".running_mean"], sd[name + ".running_var"] = torch.zeros(c), torch.ones(c)


@functools.lru_cache(maxsize=None)
def _weights(blk):
    sd = synth.random_state_dict(seed=21 + blk)
    g = torch.Generator().manual_seed(5)
    w, s = torch.zeros(32, 1, 7, 7), torch.rand(32, generator=g) + 0.5
    for c in range(32):
        w[c, 0, 3 + (c & 1), 3 + ((c >> 1) & 1)] = s[c]
    sd["conv1.0.weight"], sd["conv1.0.bias"] = w, torch.zeros(32)
    _identity_bn(sd, "conv1.1")
    if blk == 1:                                         # block 0: a2[c', r, q] = p_c' * a1[c' % 32, 2r, 2q]
        p = "res_blocks.0"
        for conv in (".conv1", ".conv2", ".skip.0"):
            sd[p + conv + ".weight"], sd[p + conv + ".bias"] = torch.zeros_like(sd[p + conv + ".weight"]), torch.zeros(64)
        for c in range(64):
            sd[p + ".skip.0.weight"][c, c % 32, 0, 0] = 0.5 + float(torch.rand((), generator=g))
        for bn in (".bn1", ".bn2", ".skip.1"):
            _identity_bn(sd, p + bn)
    return sd


@functools.lru_cache(maxsize=None)
def _model(blk, rows):
    m = cda.create_model("residual", n_mels=rows, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    m.load_state_dict(_weights(blk))
    return m.cuda().eval()


def _pattern(name, hw, seed):
    """(B, 4, h, w) non-negative values of the four pixel sub-grids at the input of the block under test."""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    if name == "zero_clip_between_random":
        u = torch.rand(B, 4, h, w, generator=g) * 2 + 0.25
        u[1] = 0
        return u
    u = torch.zeros(B, 4, h, w)
    big = torch.rand(B, 4, h, w, generator=g) * 50 + 50     # far above what the block's bound allows to leak
    r, c = (h - 1, w - 1) if name == "last_row_and_column" else (0, 0)
    u[:, :, r, :], u[:, :, :, c] = big[:, :, r, :], big[:, :, :, c]
    return u


def _image(blk, rows, u):
    a1_hw = R.make_shapes(rows, FRAMES)[0]
    v = torch.zeros(B, 4, *a1_hw)
    if blk == 0:
        v[:] = u
    else:
        v[:, :, ::2, ::2] = u                            # block 0 hands the even pixels on
    x = torch.zeros(B, 1, rows, FRAMES)
    for k in range(4):
        dy, dx = k & 1, (k >> 1) & 1
        x[:, 0, dy:dy + 4 * a1_hw[0]:4, dx:dx + 4 * a1_hw[1]:4] = v[:, k]
    return x


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("blk,rows,hw", SHAPES, ids=[f"block{b}-{h}x{w}" for b, _, (h, w) in SHAPES])
def test_borders_per_pixel(blk, rows, hw, pattern):
    p = R.plan("bf16x3", rows, FRAMES)
    st = p.blocks[blk]
    assert (st.kernel, st.body, st.in_hw, st.clips) == ("resblock_x3", "16x16x32", hw, 1 + blk)
    sd, m = _weights(blk), _model(blk, rows)
    u = _pattern(pattern, hw, 7 * rows + blk)
    x = _image(blk, rows, u).cuda()
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
        # nothing is read across the clip pitch: the all-zero clip's output is the bias path of the block, to the bit what
        # the same clip gives alone (first in its workgroup instead of second) ...
        m(x[1:2])
        alone = m.read_activation(blk + 2).cpu()
        assert torch.equal(a_out[1:2], alone)
        # ... and that is the block over an all-zero input: conv1 adds exact zeros to b1, the projection to conv2 + b2
        zero = torch.zeros(1, a_in.shape[1], *hw)
        wz = R.check_stage(blk, st.kernel, alone, R.block(zero, sd, blk), R.stage_bound(blk, zero, sd, st.scheme))
        assert wz.ratio <= 1.0, wz
