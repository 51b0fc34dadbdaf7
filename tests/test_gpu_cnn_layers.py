"""The conv-stack inference kernels (csrc/cnn.hip) per pixel, at every depth, across their run-time dispatch.

Every case of ``cnn_layer_ref.CASES`` is first checked against the dispatch restatement ``plan()`` (so that a retune of
the tile configurations that moves a case off the path it was chosen for fails here), then every block's output, tapped
through prefix networks and ``conv_output``, is held to the DERIVED per-pixel bound of ``cnn_layer_ref.layer_bound``; see
that module for the bounds and profiles/cnn_layer_precision.txt for the measured worst ratios."""
import collections

import pytest
import torch
import torch.nn as nn

import cnn_layer_ref as R
from cough_detector_amd.model import _ConvStackNet

pytestmark = pytest.mark.gpu

HIDDEN = 48


class _StackNet(_ConvStackNet):
    """An arbitrary block list (dense or depthwise-separable, pool 1 or 2) with a head of its own size, on the library's
    ordinary entry points."""

    def __init__(self, blocks, compute_dtype, head_seed=7):
        super().__init__()
        self.stack = nn.ModuleList()
        for b in blocks:
            cin, cout = R.layer_dims([b])[0][:2]
            m = nn.Module()
            if b.dw_w is not None:
                m.dw = nn.Conv2d(cin, cin, 3, padding=1, groups=cin)
                m.conv = nn.Conv2d(cin, cout, 1)
                m.dw.weight.data.copy_(b.dw_w)
                m.dw.bias.data.copy_(b.dw_b)
            else:
                m.conv = nn.Conv2d(cin, cout, 3, padding=1)
            m.bn = nn.BatchNorm2d(cout)
            m.conv.weight.data.copy_(b.w)
            m.conv.bias.data.copy_(b.b)
            m.bn.weight.data.copy_(b.bn_w)
            m.bn.bias.data.copy_(b.bn_b)
            m.bn.running_mean.copy_(b.bn_mean)
            m.bn.running_var.copy_(b.bn_var)
            self.stack.append(m)
        self._pools = [int(b.pool) for b in blocks]
        self._n_pools, self._out_channels = sum(p == 2 for p in self._pools), int(blocks[-1].w.shape[0])
        g = torch.Generator().manual_seed(head_seed)
        self.fc1 = nn.Linear(self._out_channels, HIDDEN)
        self.fc2 = nn.Linear(HIDDEN, 2)
        with torch.no_grad():
            self.fc1.weight.copy_((torch.rand(self.fc1.weight.shape, generator=g) - 0.5) * 0.5)
            self.fc1.bias.copy_((torch.rand(HIDDEN, generator=g) - 0.5) * 0.2)
            self.fc2.weight.copy_((torch.rand(self.fc2.weight.shape, generator=g) - 0.5) * 2.0)
            self.fc2.bias.copy_((torch.rand(2, generator=g) - 0.5) * 0.2)
        self._init_native(compute_dtype)

    def _describe(self, sd):
        blocks = [(f"stack.{i}.conv", f"stack.{i}.bn", f"stack.{i}.dw" if hasattr(m, "dw") else None, self._pools[i])
                  for i, m in enumerate(self.stack)]
        return blocks, "fc1", "fc2", self.stack[0].bn.eps


def _blocks(case, cnn_golden):
    if case.net in R.BLOCKS:
        return R.BLOCKS[case.net](cnn_golden[case.net][0])
    return R.random_blocks(R.GENERIC[case.net], seed=sum(map(ord, case.net)))


EXPECT = R.EXPECT       # the hand-checked table, shared with tests/test_cnn_layer_ref_host.py
ODD_HW = {"std_91x101", "small_91x101", "std_89x99", "small_89x99", "std_33x35", "small_33x35", "std_17x17", "small_17x17"}

WORST = collections.defaultdict(lambda: (0.0, ""))      # path -> (worst GPU / bound, where); printed by the last test
PARAMS = [(c, dt) for c in R.CASES for dt in R.case_dtypes(c)]


def _record(path, ratio, where):
    if ratio > WORST[path][0]:
        WORST[path] = (ratio, where)


def _path(step, dtype):
    if step.kernel == "lds_x3":
        return f"lds_x3<{step.cin},{'pool' if step.pool == 2 else 'nopool'}>"
    if step.kernel in ("conv_f32", "conv_bf16"):
        return f"{step.kernel}<nt{step.nt},{'pool' if step.pool == 2 else 'nopool'}>"
    return step.kernel + (":odd" if step.odd_hw else "") + ("" if dtype != "bf16_approx" or step.kernel != "first" else ":bf16")


@pytest.mark.parametrize("case,dtype", PARAMS, ids=[f"{c.name}-{dt}" for c, dt in PARAMS])
def test_every_block_within_its_bound_and_the_head_consistent(cnn_golden, case, dtype):
    blocks = _blocks(case, cnn_golden)
    steps = R.plan(blocks, dtype, case.H, case.W)
    got_plan = [(s.kernel, s.band_rows, s.n_bands, s.fused_mean) for s in steps]
    if (case.name, dtype) in EXPECT:
        assert got_plan == EXPECT[(case.name, dtype)], got_plan
    if dtype == "bf16x3" and case.name in ODD_HW:
        assert steps[0].kernel == "first_x3" and steps[0].odd_hw
    assert all(s.kernel != "unsupported" for s in steps)

    # ---- every tap within its bound at every pixel
    x = R.case_image(case)
    nets = {}

    def tap(d):
        nets[d] = _StackNet(blocks[:d + 1], dtype).cuda().eval()
        return nets[d].conv_output(x.cuda()).cpu()

    worst = R.check_taps(x, blocks, steps, dtype, tap)
    for w in worst:
        where = (f"{case.name} {dtype} depth {w.depth} clip {w.clip} ch {w.channel} row {w.row} col {w.col} band row {w.band_row} "
                 f"err {w.err:.3e} bound {w.bound:.3e}")
        print(f"ratio {w.ratio:.4f} {w.kernel}: {where}")
        _record(_path(steps[w.depth], dtype), w.ratio, where)
    bad = [w for w in worst if not w.ratio <= 1.0]
    assert not bad, bad

    # ---- the head: forward's logits against a float64 head over the GPU's own conv_output
    full = nets[len(blocks) - 1]
    xg = x.cuda()
    logits = full(xg).cpu()
    act = full.conv_output(xg).cpu()
    ref, e_l = R.head_ref(act, full.fc1.weight.cpu(), full.fc1.bias.cpu(), full.fc2.weight.cpu(), full.fc2.bias.cpu())
    hr = float(((logits.double() - ref).abs() / e_l).max())
    head = "head:fused" if steps[-1].fused_mean else ("head:tail" if dtype != "bf16_approx" else "head:tail:bf16")
    print(f"ratio {hr:.4f} {head}: {case.name} {dtype}")
    _record(head, hr, f"{case.name} {dtype}")
    assert hr <= 1.0

    # ---- predict is consistent with those logits
    l2, probs, preds = full._run(xg, want_probs=True)
    assert torch.equal(l2.cpu(), logits)
    sm = torch.softmax(logits.double(), dim=1)
    gap = (logits[:, 1] - logits[:, 0]).abs().double()
    assert bool(((probs.cpu().double() - sm).abs() <= ((8 + gap) * R.U)[:, None]).all())
    assert torch.equal(preds.cpu().long(), (logits[:, 1] > logits[:, 0]).long())

    # ---- batch invariance to the bit, odd clips at odd float offsets when H * W is odd
    x5 = torch.cat([x, R.case_image(case, 5)])[:5].cuda()
    y5, a5 = full(x5).cpu(), full.conv_output(x5).cpu()
    for i in (1, 2, 4):
        assert torch.equal(full(x5[i:i + 1]).cpu(), y5[i:i + 1]), i
        assert torch.equal(full.conv_output(x5[i:i + 1]).cpu(), a5[i:i + 1]), i

    # ---- another size through the same handle, then back: identical bits
    other = (64, 47) if (case.H, case.W) != (64, 47) else (90, 101)
    assert R.plan(blocks, dtype, *other) is not None
    assert torch.isfinite(full(torch.rand(2, 1, *other, generator=torch.Generator().manual_seed(1)).cuda())).all()
    assert torch.equal(full(xg).cpu(), logits) and torch.equal(full.conv_output(xg).cpu(), act)


def test_bf16_approx_refuses_what_its_lds_image_cannot_hold(cnn_golden):
    """An image whose band does not fit the 48 KB LDS image (64 x 400), or whose pooled row is wider than all the tiles of
    a workgroup (40 x 560: a band of zero rows), is refused with a ValueError before anything is launched; the handle
    still works afterwards, and fp32 / bf16x3 take the same images."""
    blocks = R.standard_blocks(cnn_golden["standard"][0])
    m = _StackNet(blocks, "bf16_approx").cuda().eval()
    ok = torch.rand(2, 1, 90, 101, generator=torch.Generator().manual_seed(2)).cuda()
    before = m(ok).cpu()
    for h, w in ((64, 400), (40, 560)):
        steps = R.plan(blocks, "bf16_approx", h, w)
        assert steps[1].kernel == "unsupported"
        x = torch.rand(2, 1, h, w, generator=torch.Generator().manual_seed(3)).cuda()
        with pytest.raises(ValueError, match="too wide for the LDS-image convolution"):
            m(x)
        with pytest.raises(ValueError, match="too wide for the LDS-image convolution"):
            m.conv_output(x)
        assert torch.equal(m(ok).cpu(), before)
        for dtype in ("fp32", "bf16x3"):
            assert all(s.kernel != "unsupported" for s in R.plan(blocks, dtype, h, w))
            assert torch.isfinite(_StackNet(blocks, dtype).cuda().eval()(x)).all()


def test_bf16_approx_needs_16_channel_chunks():
    """cough_cnn_create: the single-bf16 kernels read 16 channels per k-step, so an 8- or 24-wide first block is refused there
    (fp32 and bf16x3 take it: the matrix runs both).  Only the first-block refusal can be reached: a later block's cin is
    the previous cout, a multiple of 32 (or the first block's, already a multiple of 16), so its "need cin % 16 == 0"
    message has no input that produces it."""
    for net in ("mixed", "first24"):
        blocks = R.random_blocks(R.GENERIC[net], seed=1)
        m = _StackNet(blocks, "bf16_approx").cuda().eval()
        with pytest.raises(ValueError, match="first block must be a dense 3x3 conv"):
            m(torch.zeros(1, 1, 72, 88).cuda())


def test_report_worst_ratios():
    """A reporter, not a check of its own: prints the worst GPU / bound ratio per kernel path that the tests above collected
    in this process (the source of profiles/cnn_layer_precision.txt).  Run alone, or in another process than they, it
    prints nothing; the bound itself is asserted per case above."""
    for path in sorted(WORST):
        print(f"PRECISION {path:28s} {WORST[path][0]:.4f}   {WORST[path][1]}")
    assert all(v[0] <= 1.0 for v in WORST.values())
