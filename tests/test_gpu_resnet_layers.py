"""The residual inference kernels (csrc/resnet.hip) per pixel, at every tap, across their run-time dispatch.

Every case of ``resnet_layer_ref.CASES`` is first checked against the dispatch restatement ``plan()`` and the hand-written
``EXPECT`` (so that a retune which moves a case off the path it was chosen for fails here), then the stem output is held to
the DERIVED per-pixel bound over the image, every block output to the bound over the GPU's own block input, and the logits
to the head bound over the GPU's own last activation; see that module for the bounds and
profiles/resnet_layer_precision.txt for the measured worst ratios."""
import collections
import warnings

import pytest
import torch

import cough_detector_amd as cda
import resnet_layer_ref as R

pytestmark = pytest.mark.gpu

WORST = collections.defaultdict(lambda: (0.0, ""))      # path -> (worst GPU / bound, where); printed by the last test


def _record(path, ratio, where):
    if ratio > WORST[path][0]:
        WORST[path] = (ratio, where)


def _model(case, sd):
    m = cda.create_model("residual", n_mels=case.H, num_classes=2, in_channels=1, channels=case.channels, compute_dtype=case.dtype)
    m.load_state_dict(sd)
    return m.cuda().eval()


def _run(m, x):
    """(logits, [a1, a2, ...]) of one forward, on the CPU."""
    logits = m(x).cpu()
    return logits, [m.read_activation(k).cpu() for k in range(1, len(m.channels) + 1)]


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_stage_within_its_bound_and_the_head_consistent(case):
    name = R.case_id(case)
    p = R.plan(case.dtype, case.H, case.W, case.channels)
    assert p is not None and R.plan_row(p) == R.EXPECT[name], R.plan_row(p)

    sd, x = R.case_weights(case), R.case_image(case)
    assert x.shape[0] == R.BATCH == 5
    xg = x.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # the announced fallback of a size without compiled kernels
        m = _model(case, sd)
        logits, acts = _run(m, xg)

        # ---- every tap within its bound at every pixel and channel
        worst = R.check_net(x, sd, p, lambda k: acts[k - 1])
        for w, stage in zip(worst, [p.stem] + list(p.blocks)):
            where = (f"{name} stage {w.stage} clip {w.clip} ch {w.channel} row {w.row} col {w.col} err {w.err:.3e} "
                     f"bound {w.bound:.3e}")
            print(f"ratio {w.ratio:.4f} {w.kernel}: {where}")
            _record(R.stage_path(stage), w.ratio, where)
        bad = [w for w in worst if not w.ratio <= 1.0]
        assert not bad, bad

        # ---- the head: the logits against a float64 head over the GPU's own last activation
        assert torch.isfinite(logits).all()
        ref, e_l = R.head_bound(acts[-1], sd)
        hr = (logits.double() - ref).abs() / e_l
        clip = int(hr.max(dim=1).values.argmax())
        head = "head:" + p.head + (":x3" if p.head == "fused" and case.dtype == "bf16x3" else ":bf16" if p.head == "fused" else "")
        print(f"ratio {float(hr.max()):.4f} {head}: {name} clip {clip}")
        _record(head, float(hr.max()), f"{name} clip {clip}")
        assert float(hr.max()) <= 1.0, (clip, hr)

        # ---- predict is consistent with those logits
        l2, probs, preds = m._run(xg, want_probs=True)
        assert torch.equal(l2.cpu(), logits)
        sm = torch.softmax(logits.double(), dim=1)
        gap = (logits[:, 1] - logits[:, 0]).abs().double()
        assert bool(((probs.cpu().double() - sm).abs() <= ((8 + gap) * R.U)[:, None]).all())
        assert torch.equal(preds.cpu().long(), (logits[:, 1] > logits[:, 0]).long())

        # ---- batch invariance to the bit: a clip's result does not depend on its place in a workgroup's clip group
        for lo, hi in ((1, 2), (2, 5), (4, 5)):
            sub_l, sub_a = _run(m, xg[lo:hi])
            assert torch.equal(sub_l, logits[lo:hi]), (lo, hi)
            for k, (a, b) in enumerate(zip(sub_a, acts)):
                assert torch.equal(a, b[lo:hi]), (lo, hi, k + 1)

        # ---- another size through the same handle, then the first again: identical bits
        other = (40, 33) if (case.H, case.W) != (40, 33) else (90, 101)
        assert R.plan(case.dtype, *other, case.channels) is not None
        assert torch.isfinite(m(torch.randn(2, 1, *other, generator=torch.Generator().manual_seed(1)).cuda())).all()
        again_l, again_a = _run(m, xg)
        assert torch.equal(again_l, logits) and all(torch.equal(a, b) for a, b in zip(again_a, acts))

        # ---- one NaN pixel in clip 3: that clip's logits are NaN, every other clip is bit-equal to the run without it
        if case.nan:
            xn = x.clone()
            xn[3, 0, case.H // 2, case.W // 3] = float("nan")
            ln, probs_n, _ = m._run(xn.cuda(), want_probs=True)
            ln = ln.cpu()
            assert torch.isnan(ln[3]).all() and torch.isnan(probs_n.cpu()[3]).all(), ln
            keep = [0, 1, 2, 4]
            assert torch.equal(ln[keep], logits[keep])


def test_report_worst_ratios():
    """A reporter, not a check of its own: prints the worst GPU / bound ratio per kernel path that the tests above collected
    in this process (the source of profiles/resnet_layer_precision.txt).  Run alone, or in another process than they, it
    prints nothing; the bound itself is asserted per case above."""
    for path in sorted(WORST):
        print(f"PRECISION {path:34s} {WORST[path][0]:.4f}   {WORST[path][1]}")
    assert all(v[0] <= 1.0 for v in WORST.values())
