"""CoughDetector ("standard") training on the MI355X (csrc/train_std.hip through cough_detector_amd.StandardTrainer)
against the float64 restatement (tests/train_std_ref.py) and the reference's own three steps
(tests/golden/train_std_step_golden.npz).

Tolerances are the other trainers' (train_std_ref.assert_step_matches): loss 1e-5 relative (or of the logits' bound),
logits 1e-5 of their scale, every gradient within 1e-4 of its tensor's largest, running statistics rtol 1e-5.  The 4
conv biases that feed a BatchNorm have a true gradient of 0 and are bounded, not compared.

Well-posedness, as in test_gpu_train_small.py: conv 0's weight and bias are put on a 2^-6 grid and the input on a 2^-10
grid, so every conv 0 output is exact in f32 and f64 and the first max-pool's windows tie exactly or differ by far more
than rounding; ReLU inputs within rounding of 0 are taken from the kernel's side by ``resolve_kinks``.  The golden head
(fc.3) gives logits in the hundreds on these images, where the CE terms saturate; it is scaled by 1/100 (the golden-step
test keeps the golden weights and the logits' bound for the loss).
"""
import copy

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd.training import StandardTrainer, train_epoch
from test_train_std_host import golden_grad_rtol, load_std_golden, std_sd
from train_std_ref import (BN_FED_BIASES, MASK_OFF, MASK_WIDTH, PARAM_NAMES, RefStep, assert_step_matches,
                           golden_sample, resolve_kinks, running_names, step_on_the_kernels_side)

pytestmark = pytest.mark.gpu
CW = [1.0, 2.5]
GRID = 2.0 ** -6
PB, PF = 0.1, 0.5


def _model(sd):
    m = cda.create_model("standard", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def qsd():
    sd = dict(std_sd())
    for k in ("conv_layers.0.conv.weight", "conv_layers.0.conv.bias"):
        sd[k] = torch.round(sd[k] / GRID) * GRID
    sd["fc.3.weight"] = sd["fc.3.weight"] / 100
    sd["fc.3.bias"] = sd["fc.3.bias"] / 100
    return sd


def _on_grid(x):
    """x rounded to a 2^-10 grid: conv 0 outputs are then multiples of 2^-16 below 2^8, exact in f32"""
    return torch.round(x.clamp(-8, 8) * 1024) / 1024


def _mask(b, g):
    m = torch.empty(b, MASK_WIDTH)
    m[:, :MASK_OFF[4]] = (torch.rand(b, MASK_OFF[4], generator=g) >= PB).float()
    m[:, MASK_OFF[4]:] = (torch.rand(b, MASK_WIDTH - MASK_OFF[4], generator=g) >= PF).float()
    return m


def _batch(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = _on_grid(torch.randn(b, 1, h, w, generator=g))
    y = torch.randint(0, 2, (b,), generator=g)
    return x, y, _mask(b, g)


def _check(sd, b, h, w, seed):
    x, y, mask = _batch(b, h, w, seed)
    tr = StandardTrainer(_model(sd), class_weights=CW)
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    torch.cuda.synchronize()
    ref = RefStep(sd, class_weights=CW)
    rloss, rlogits, rg = ref.grads(x, y, mask, PB, PF)
    g = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
    rg, _ = resolve_kinks(g, ref, rg)
    return assert_step_matches(tr.model, loss, logits, rloss, rlogits, rg, ref.state_dict(), sd)


@pytest.mark.parametrize("b,h,w", [(8, 90, 101), (8, 63, 101), (4, 16, 16), (1, 90, 101), (5, 37, 29), (3, 17, 33),
                                   (2, 16, 47)])
def test_step_matches_the_restatement(qsd, b, h, w):
    _check(qsd, b, h, w, seed=b * 7 + h + w)


def test_step_matches_the_restatement_at_256_clips(qsd):
    """B = 256 at 32 x 32, held to the same 1e-4 as the small shapes."""
    _check(qsd, 256, 32, 32, seed=256 * 7 + 32 + 32)


def test_256_clips_of_64x64_as_close_as_torchs_own_float32_step(qsd):
    """B = 256 at 64 x 64, with every gradient held to twice the worst error of torch's own float32 step (the same
    F.conv2d / batch_norm / autograd step on the CPU in float32) against the float64 restatement, and never looser than
    3e-3.  Loss, logits and running statistics keep their bounds.  Two effects make exact-f32 arithmetic miss 1e-4 at
    this size, in torch's step as in this one.  First, the 4.2 M pool windows after conv 1 hold values the input grid
    cannot make exact: a few of them have their top two values within f32 rounding and route their gradient to another
    pixel in float64.  Second, the weight gradients below a BatchNorm are sums over 262 K pixels that cancel to a small
    fraction of their terms' size, so the f32 rounding of those terms is amplified.  Measured on an MI355X: this kernel's
    worst tensor is conv 1's weight gradient at 2.9e-4 of its scale (torch's float32 step: 3.4e-5 there), torch's worst
    is conv 2's BN bias at 1.7e-4 (this kernel: the same), so the rule is 3.4e-4.  The test prints both steps' errors."""
    x, y, mask = _batch(256, 64, 64, seed=256 * 7 + 64 + 64)
    tr = StandardTrainer(_model(qsd), class_weights=CW)
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    torch.cuda.synchronize()
    ref = RefStep(qsd, class_weights=CW)
    rloss, rlogits, rg = ref.grads(x, y, mask, PB, PF)
    g = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
    rg, _ = resolve_kinks(g, ref, rg)
    _, _, g32 = RefStep(qsd, class_weights=CW, dtype=torch.float32).grads(x, y, mask, PB, PF)

    def errs(got):
        return {n: (got[n].double() - rg[n]).abs().max().item() / rg[n].abs().max().item()
                for n in PARAM_NAMES if n not in BN_FED_BIASES}

    mine, theirs = errs(g), errs(g32)
    print("gradient error / scale, this step and torch's float32 step:",
          {n: (f"{mine[n]:.2e}", f"{theirs[n]:.2e}") for n in mine})
    rule = max(1e-4, 2 * max(theirs.values()))
    assert rule <= 3e-3, rule
    assert_step_matches(tr.model, loss, logits, rloss, rlogits, rg, ref.state_dict(), qsd, grad_rtol=rule)


def test_three_reference_steps_from_the_golden():
    g, init = load_std_golden()
    lr = float(g["lr"])
    pb, pf = float(g["p_block"]), float(g["p_fc"])
    tr = StandardTrainer(_model(init), lr=lr, weight_decay=float(g["weight_decay"]), class_weights=g["class_weights"])
    for s in range(3):
        x, y, mask = (torch.from_numpy(g[k + str(s)]) for k in ("x", "y", "mask"))
        if s > 0:
            # from step 1 on, the two runs start from states that differ where AdamW moved noise-level gradients by ~lr
            # (test_gpu_train.py): these steps are checked against the restatement from this run's own state
            ref = RefStep({k: v.cpu() for k, v in tr.model.state_dict().items()}, lr=lr,
                          weight_decay=float(g["weight_decay"]), class_weights=g["class_weights"])
            ref.opt.load_state_dict(copy.deepcopy(tr.optimizer.state_dict()))
        # tr.step in its two halves, so that the unclipped gradients can be read in between
        loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
        if s > 0:
            # ReLU inputs within rounding of 0 from the kernel's side, as in every single-step check (resolve_kinks)
            grads = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
            rloss, rlogits, _, _, _ = step_on_the_kernels_side(ref, grads, x, y, mask, pb, pf)
        tr.optimizer.step()
        tr.model.invalidate()
        zscale = np.abs(g[f"logits{s}"]).max()
        if s == 0:
            # the golden head's logits reach the hundreds: the loss is a difference on that scale
            assert abs(loss.item() - float(g["loss0"])) <= max(1e-5 * abs(float(g["loss0"])), 1e-5 * zscale)
            np.testing.assert_allclose(logits.cpu().numpy(), g["logits0"], rtol=0, atol=1e-5 * zscale)
            for n, p in tr.model.named_parameters():
                if n not in BN_FED_BIASES:      # p.grad holds the clipped gradient, as the reference's does
                    want = g["grad1." + n]
                    err = np.abs(golden_sample(p.grad) - want).max()
                    assert err <= golden_grad_rtol(n) * np.abs(want).max(), n
        else:
            assert abs(loss.item() - rloss.item()) <= max(1e-5 * abs(rloss.item()), 1e-5 * zscale)
            assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * rlogits.abs().max().item()
    # step 2's AdamW update from this run's own moments: they differ from the restatement's by (1 - beta1) times the
    # clipped gradient's error (1 - beta2 times twice it for the second moment)
    ost = tr.optimizer.state_dict()["state"]
    rst = ref.opt.state_dict()["state"]
    for i, n in enumerate(PARAM_NAMES):
        if n in BN_FED_BIASES:
            continue
        gs = ref.P[n].grad.abs().max().item()          # clipped in place by clip_grad_norm_
        rt = golden_grad_rtol(n)
        dm = (ost[i]["exp_avg"].cpu().double() - rst[i]["exp_avg"]).abs().max().item()
        dv = (ost[i]["exp_avg_sq"].cpu().double() - rst[i]["exp_avg_sq"]).abs().max().item()
        assert dm <= 0.1 * rt * gs + 1e-12, (n, dm, gs)
        assert dv <= 0.001 * 2 * rt * gs * gs + 1e-15, (n, dv, gs)
    sd = tr.model.state_dict()
    for i, n in enumerate(PARAM_NAMES):
        d = np.abs(golden_sample(sd[n]) - g["final." + n])
        assert d.max() <= 6 * lr, n
        if n not in BN_FED_BIASES:
            assert np.median(d) <= 1e-5, n
            m_want, v_want = g["adam.exp_avg." + n], g["adam.exp_avg_sq." + n]
            # the moments mix the gradients of steps 1 and 2, taken from states that differ from the golden run's (see
            # above): measured on an MI355X, conv_layers.0.bn.weight's first moment at a median 5.0e-4 of its scale.
            # They are held to 1e-3 here, 2e-3 for the second moment (a square); step 2's own update is checked
            # against the restatement below
            assert np.median(np.abs(golden_sample(ost[i]["exp_avg"]) - m_want)) <= 1e-3 * np.abs(m_want).max(), n
            assert np.median(np.abs(golden_sample(ost[i]["exp_avg_sq"]) - v_want)) <= 2e-3 * np.abs(v_want).max(), n
    assert float(ost[0]["step"]) == float(g["adam.step"]) == 3.0
    for k in running_names():
        atol = 0.1 * 6 * lr if k.endswith("running_mean") else 1e-6
        np.testing.assert_allclose(sd[k].cpu().numpy(), g["final." + k], rtol=1e-4, atol=atol, err_msg=k)
        nbt = k.rsplit(".", 1)[0] + ".num_batches_tracked"
        assert int(sd[nbt]) == int(g["final." + nbt])


def test_a_repeat_is_bit_identical(qsd):
    x, y, _ = _batch(64, 90, 101, seed=3)
    outs = []
    for _ in range(2):
        tr = StandardTrainer(_model(qsd), class_weights=CW, seed=11)
        losses = [tr.step(x.cuda(), y.cuda())[0].item() for _ in range(2)]
        outs.append((losses, tr._params.cpu().clone(), tr._grads.cpu().clone(), tr._running.cpu().clone(),
                     tr._nbt.cpu().clone()))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("max_norm", [1e-3, 1e9])
def test_clipping_active_and_inactive(qsd, max_norm):
    x, y, mask = _batch(16, 90, 101, seed=5)
    tr = StandardTrainer(_model(qsd), class_weights=CW, max_norm=max_norm)
    tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    raw = tr._grads.clone()
    tr.optimizer.step()
    ref = RefStep(qsd, class_weights=CW, max_norm=max_norm)
    _, _, _, rnorm = ref.step(x, y, mask, PB, PF)
    norm = tr.optimizer.total_norm.item()
    assert abs(norm - rnorm) <= 1e-4 * rnorm
    assert (rnorm > max_norm) == (max_norm == 1e-3)
    coef = min(max_norm / (norm + 1e-6), 1.0)
    torch.testing.assert_close(tr._grads, raw * coef, rtol=1e-6, atol=0)


def test_device_dropout_planes_rates_and_reproducibility(qsd):
    b = 256
    x, y, _ = _batch(b, 32, 48, seed=9)
    masks = []
    for _ in range(2):
        tr = StandardTrainer(_model(qsd), seed=1234)
        m1 = torch.empty(b, MASK_WIDTH, device="cuda")
        m2 = torch.empty(b, MASK_WIDTH, device="cuda")
        tr.forward_backward(x.cuda(), y.cuda(), mask_out=m1)
        tr.forward_backward(x.cuda(), y.cuda(), mask_out=m2)
        masks.append((m1.cpu(), m2.cpu()))
    (a1, a2), (b1, b2) = masks
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    assert not torch.equal(a1, a2)
    for m in (a1, a2):
        assert set(m.unique().tolist()) <= {0.0, 1.0}
        # every site keeps about 1 - p of its units: the four blocks' planes (p = 0.1) and the hidden units (p = 0.5)
        for lo, hi, p in [(MASK_OFF[k], MASK_OFF[k + 1], PB) for k in range(4)] + [(MASK_OFF[4], MASK_WIDTH, PF)]:
            n, keep = b * (hi - lo), 1 - p
            assert abs(m[:, lo:hi].sum().item() - keep * n) <= 5 * (keep * (1 - keep) * n) ** 0.5, (lo, hi)
    tr = StandardTrainer(_model(qsd), seed=1235)
    m3 = torch.empty(b, MASK_WIDTH, device="cuda")
    tr.forward_backward(x.cuda(), y.cuda(), mask_out=m3)
    assert not torch.equal(m3.cpu(), a1)
    # a Dropout2d keep drops a whole (clip, channel) plane: the step with the device's draw is the step fed that draw
    xs, ys = x[:8].cuda(), y[:8].cuda()
    tr_d = StandardTrainer(_model(qsd), seed=77)
    drawn = torch.empty(8, MASK_WIDTH, device="cuda")
    loss_d, logits_d = tr_d.forward_backward(xs, ys, mask_out=drawn)
    assert (drawn[:, :MASK_OFF[4]] == 0).any()
    tr_f = StandardTrainer(_model(qsd), seed=0)
    loss_f, logits_f = tr_f.forward_backward(xs, ys, dropout_mask=drawn.clone())
    assert torch.equal(logits_d, logits_f) and torch.equal(tr_d._grads, tr_f._grads)
    ref = RefStep(qsd)
    rloss, rlogits, _ = ref.grads(x[:8], y[:8], drawn.cpu(), PB, PF)
    assert (logits_d.cpu().double() - rlogits).abs().max().item() <= 1e-5 * max(1.0, rlogits.abs().max().item())


def test_the_scheduler_drives_lr(qsd):
    x, y, mask = _batch(16, 90, 101, seed=13)
    tr = StandardTrainer(_model(qsd), class_weights=CW)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(tr.optimizer, T_0=10, T_mult=2, eta_min=1e-6)
    tr.step(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    sched.step()
    lr = tr.optimizer.param_groups[0]["lr"]
    assert abs(lr - (1e-6 + (1e-3 - 1e-6) * (1 + np.cos(np.pi / 10)) / 2)) < 1e-12
    state = copy.deepcopy(tr.optimizer.state_dict())
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in tr.model.parameters()]
    topt = torch.optim.AdamW(tparams)
    topt.load_state_dict(state)
    tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    for tp, p in zip(tparams, tr.model.parameters()):
        tp.grad = p.grad.detach().clone()
    torch.nn.utils.clip_grad_norm_(tparams, max_norm=1.0)
    topt.step()
    tr.optimizer.step()
    for tp, p in zip(tparams, tr.model.parameters()):
        torch.testing.assert_close(p.detach(), tp.detach(), rtol=1e-5, atol=1e-7)


def test_eval_after_training_uses_the_trained_state(qsd):
    x, y, _ = _batch(16, 90, 101, seed=17)
    model = _model(qsd)
    before = model(x.cuda()).cpu()
    tr = StandardTrainer(model, class_weights=CW)
    res = train_epoch(tr, [(x, y), (x, y)], 0)
    assert set(res) == {"loss", "accuracy"} and np.isfinite(res["loss"]) and 0 <= res["accuracy"] <= 100
    with pytest.raises(RuntimeError, match="inference-only"):
        model(x.cuda())
    model.eval()
    after = model(x.cuda()).cpu()
    fresh = _model({k: v.cpu() for k, v in model.state_dict().items()})
    assert torch.equal(after, fresh(x.cuda()).cpu())
    assert not torch.equal(after, before)
    assert int(model.state_dict()["conv_layers.0.bn.num_batches_tracked"]) == \
        int(qsd["conv_layers.0.bn.num_batches_tracked"]) + 2


def test_error_cases_and_non_finite_input(qsd):
    tr = StandardTrainer(_model(qsd))
    x, y, _ = _batch(4, 90, 101, seed=1)
    with pytest.raises(ValueError):
        tr.step(x[:, :, :15].contiguous().cuda(), y.cuda())
    with pytest.raises(ValueError):
        tr.step(x.cuda(), y.cuda(), dropout_mask=torch.ones(4, 128, device="cuda"))
    with pytest.raises(ValueError):
        tr.step(x.cuda(), y[:3].cuda())
    for bad in (float("nan"), float("inf")):
        xb = x.clone()
        xb[1, 0, 5, 7] = bad
        loss, _ = tr.forward_backward(xb.cuda(), y.cuda())
        assert torch.isnan(loss).item()


def test_end_to_end_augment_featurise_specaugment_train():
    import random
    from cough_detector_amd import synth
    random.seed(0)
    torch.manual_seed(0)
    seeds = list(range(96))
    wav = torch.from_numpy(np.stack([synth.make_clip(s) for s in seeds])).cuda()
    labels = torch.tensor([1 if s % 6 == 0 else 0 for s in seeds]).cuda()
    aug = cda.AudioAugmentor(p_augment=0.5)
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False,
                                use_spectral_contrast=False, device="cuda")
    spec = cda.SpecAugment()
    model = cda.create_model("standard", n_mels=90, num_classes=2, in_channels=1)
    tr = StandardTrainer(model, class_weights=[1.0, 5.0], seed=3)
    losses = []
    for step in range(40):
        feats = spec(pre.extract_features(aug.augment_batch(wav, seed=step)).unsqueeze(1))
        loss, _ = tr.step(feats, labels)
        losses.append(loss.item())
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    print(f"end-to-end: mean loss of steps 0-4 {first:.4f}, of steps 35-39 {last:.4f}")
    assert np.isfinite(losses).all() and last < 0.5 * first
