"""CoughDetectorResidual training on the MI355X (csrc/train.hip through cough_detector_amd.training) against the float64
restatement (tests/train_ref.py) and the reference's own three steps (tests/golden/train_step_golden.npz).

Tolerances: the kernels are exact f32 with sums of up to 2.4 M terms (the stem's wgrad at B = 256); 1e-4 of a tensor's
largest gradient leaves a decade over the f32 accumulation error of such sums.  The 7 conv biases that feed a BatchNorm
have a true gradient of 0: both sides are rounding noise, so they are bounded, not compared."""
import copy

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd.training import ResidualTrainer, train_epoch
from test_train_host import load_train_golden
from train_ref import BN_FED_BIASES, PARAM_NAMES, RefStep, assert_step_matches, golden_sample, running_names

pytestmark = pytest.mark.gpu
CW = [1.0, 2.5]


def _model(sd):
    m = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    m.load_state_dict(sd)
    return m


def _batch(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, 1, h, w, generator=g)
    y = torch.randint(0, 2, (b,), generator=g)
    mask = (torch.rand(b, 128, generator=g) >= 0.5).float()
    return x, y, mask


@pytest.mark.parametrize("b,h,w", [(8, 90, 101), (64, 103, 101), (256, 64, 101)])
def test_gradients_loss_and_running_stats_match_the_restatement(resnet_golden, b, h, w):
    sd, _ = resnet_golden
    x, y, mask = _batch(b, h, w, seed=b + h)
    tr = ResidualTrainer(_model(sd), class_weights=CW)
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    torch.cuda.synchronize()
    ref = RefStep(sd, class_weights=CW)
    rloss, rlogits, rg = ref.grads(x, y, mask, 0.5)
    assert_step_matches(tr.model, loss, logits, rloss, rlogits, rg, ref.state_dict(), sd)


def test_three_reference_steps_from_the_golden():
    g, init = load_train_golden()
    lr = float(g["lr"])
    tr = ResidualTrainer(_model(init), lr=lr, weight_decay=float(g["weight_decay"]), class_weights=g["class_weights"])
    for s in range(3):
        x, y, mask = (torch.from_numpy(g[k + str(s)]) for k in ("x", "y", "mask"))
        if s > 0:
            # from step 1 on the two runs no longer start from the same state: AdamW moves every parameter by ~lr whatever
            # the size of its gradient, so where a gradient is at f32 rounding level (the BN-fed biases, near-dead units)
            # each f32 run steps in its own direction and the step-2 loss differs from the golden by ~1e-4 relative.  The
            # arithmetic of these steps is checked instead against the float64 restatement started from this run's own
            # state (parameters, BN buffers, AdamW moments); the trajectory against the golden is bounded below.
            ref = RefStep({k: v.cpu() for k, v in tr.model.state_dict().items()}, lr=lr,
                          weight_decay=float(g["weight_decay"]), class_weights=g["class_weights"])
            ref.opt.load_state_dict(copy.deepcopy(tr.optimizer.state_dict()))
            rloss, rlogits, _, _ = ref.step(x, y, mask, float(g["p"]))
        loss, logits = tr.step(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
        if s == 0:
            # same starting state, float32 against float32 in another summation order
            assert abs(loss.item() - float(g["loss0"])) <= 1e-5 * abs(float(g["loss0"]))
            np.testing.assert_allclose(logits.cpu().numpy(), g["logits0"], rtol=0, atol=1e-4 * np.abs(g["logits0"]).max())
            for n, p in tr.model.named_parameters():
                if n not in BN_FED_BIASES:      # p.grad holds the clipped gradient, as the reference's does
                    want = g["grad1." + n]
                    assert np.abs(golden_sample(p.grad) - want).max() <= 1e-4 * np.abs(want).max(), n
        else:
            assert abs(loss.item() - rloss.item()) <= 1e-5 * abs(rloss.item())
            assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * rlogits.abs().max().item()
    sd = tr.model.state_dict()
    ost = tr.optimizer.state_dict()["state"]
    for i, n in enumerate(PARAM_NAMES):
        d = np.abs(golden_sample(sd[n]) - g["final." + n])
        # AdamW moves a parameter by at most ~lr per step (|m / sqrt(v)| <= 1 for a steady sign), so two runs that
        # disagree on the sign of a noise-level gradient end at most 6 lr apart after 3 steps; the bulk agrees to 1e-5
        assert d.max() <= 6 * lr, n
        if n not in BN_FED_BIASES:
            assert np.median(d) <= 1e-5, n
            m_want, v_want = g["adam.exp_avg." + n], g["adam.exp_avg_sq." + n]
            assert np.median(np.abs(golden_sample(ost[i]["exp_avg"]) - m_want)) <= 1e-4 * np.abs(m_want).max(), n
            assert np.median(np.abs(golden_sample(ost[i]["exp_avg_sq"]) - v_want)) <= 1e-4 * np.abs(v_want).max(), n
    assert float(ost[0]["step"]) == float(g["adam.step"]) == 3.0
    for k in running_names():
        atol = 0.1 * 6 * lr if k.endswith("running_mean") else 1e-6     # the mean sees the drifting conv bias
        np.testing.assert_allclose(sd[k].cpu().numpy(), g["final." + k], rtol=1e-4, atol=atol, err_msg=k)


def test_a_repeat_is_bit_identical(resnet_golden):
    sd, _ = resnet_golden
    x, y, _ = _batch(64, 90, 101, seed=3)
    outs = []
    for _ in range(2):
        tr = ResidualTrainer(_model(sd), class_weights=CW, seed=11)
        losses = [tr.step(x.cuda(), y.cuda())[0].item() for _ in range(2)]
        outs.append((losses, tr._params.cpu().clone(), tr._grads.cpu().clone(), tr._running.cpu().clone()))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("max_norm", [1.0, 1e9])
def test_clipping_active_and_inactive(resnet_golden, max_norm):
    sd, _ = resnet_golden
    x, y, mask = _batch(32, 90, 101, seed=5)
    tr = ResidualTrainer(_model(sd), class_weights=CW, max_norm=max_norm)
    tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    raw = tr._grads.clone()
    tr.optimizer.step()
    ref = RefStep(sd, class_weights=CW, max_norm=max_norm)
    _, _, _, rnorm = ref.step(x, y, mask, 0.5)
    norm = tr.optimizer.total_norm.item()
    assert abs(norm - rnorm) <= 1e-5 * rnorm
    assert (rnorm > max_norm) == (max_norm == 1.0)                       # the golden head's gradients are large
    coef = min(max_norm / (norm + 1e-6), 1.0)
    torch.testing.assert_close(tr._grads, raw * coef, rtol=1e-6, atol=0)


def test_device_dropout_statistics_and_reproducibility(resnet_golden):
    sd, _ = resnet_golden
    x, y, _ = _batch(256, 90, 101, seed=9)
    masks = []
    for _ in range(2):
        tr = ResidualTrainer(_model(sd), seed=1234)
        m1 = torch.empty(256, 128, device="cuda")
        m2 = torch.empty(256, 128, device="cuda")
        tr.forward_backward(x.cuda(), y.cuda(), mask_out=m1)
        tr.forward_backward(x.cuda(), y.cuda(), mask_out=m2)
        masks.append((m1.cpu(), m2.cpu()))
    (a1, a2), (b1, b2) = masks
    assert torch.equal(a1, b1) and torch.equal(a2, b2)                   # same seed, same draws
    assert not torch.equal(a1, a2)                                        # a new step draws a new mask
    n = a1.numel()
    for m in (a1, a2):
        assert set(m.unique().tolist()) <= {0.0, 1.0}
        assert abs(m.sum().item() - 0.5 * n) <= 5 * (0.25 * n) ** 0.5     # binomial(n, 1 - p), 5 sigma
    assert abs((a1 == a2).float().mean().item() - 0.5) <= 5 * (0.25 / n) ** 0.5   # the two draws are independent
    tr = ResidualTrainer(_model(sd), seed=1235)
    m3 = torch.empty(256, 128, device="cuda")
    tr.forward_backward(x.cuda(), y.cuda(), mask_out=m3)
    assert not torch.equal(m3.cpu(), a1)


def test_optimizer_state_moves_to_torch_adamw_and_the_scheduler_drives_lr(resnet_golden):
    sd, _ = resnet_golden
    x, y, mask = _batch(16, 90, 101, seed=13)
    tr = ResidualTrainer(_model(sd), class_weights=CW)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(tr.optimizer, T_0=10, T_mult=2, eta_min=1e-6)
    tr.step(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    sched.step()
    lr = tr.optimizer.param_groups[0]["lr"]
    assert abs(lr - (1e-6 + (1e-3 - 1e-6) * (1 + np.cos(np.pi / 10)) / 2)) < 1e-12
    state = copy.deepcopy(tr.optimizer.state_dict())
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in tr.model.parameters()]
    topt = torch.optim.AdamW(tparams)
    topt.load_state_dict(state)
    assert topt.param_groups[0]["lr"] == lr
    tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    for tp, p in zip(tparams, tr.model.parameters()):
        tp.grad = p.grad.detach().clone()
    torch.nn.utils.clip_grad_norm_(tparams, max_norm=1.0)
    topt.step()
    tr.optimizer.step()
    for tp, p in zip(tparams, tr.model.parameters()):
        # the same f32 update; the norm is summed in another order (an ulp of the clip coefficient)
        torch.testing.assert_close(p.detach(), tp.detach(), rtol=1e-5, atol=1e-7)
    assert float(tr.optimizer.state_dict()["state"][0]["step"]) == float(topt.state_dict()["state"][0]["step"]) == 2.0


def test_eval_after_training_uses_the_trained_state(resnet_golden):
    sd, _ = resnet_golden
    x, y, _ = _batch(16, 90, 101, seed=17)
    model = _model(sd)
    before = model(x.cuda()).cpu()
    tr = ResidualTrainer(model, class_weights=CW)
    res = train_epoch(tr, [(x, y), (x, y)], 0)
    assert set(res) == {"loss", "accuracy"} and np.isfinite(res["loss"]) and 0 <= res["accuracy"] <= 100
    with pytest.raises(RuntimeError, match="inference-only"):
        model(x.cuda())                                                   # train_epoch leaves train mode, as the reference
    model.eval()
    after = model(x.cuda()).cpu()
    fresh = _model({k: v.cpu() for k, v in model.state_dict().items()})
    assert torch.equal(after, fresh(x.cuda()).cpu())
    assert not torch.equal(after, before)
    assert int(model.state_dict()["conv1.1.num_batches_tracked"]) == int(sd["conv1.1.num_batches_tracked"]) + 2


def test_error_cases(resnet_golden):
    sd, _ = resnet_golden
    with pytest.raises(ValueError, match="channels"):
        ResidualTrainer(cda.create_model("residual", n_mels=90, channels=(16, 32, 64)))
    tr = ResidualTrainer(_model(sd))
    x, y, _ = _batch(4, 90, 101, seed=1)
    with pytest.raises(ValueError):
        tr.step(x[:, :, :2].contiguous().cuda(), y.cuda())                # too small for the network
    with pytest.raises(ValueError):
        tr.step(x.cuda(), y.cuda(), dropout_mask=torch.ones(4, 64, device="cuda"))
    with pytest.raises(ValueError):
        tr.step(x.cuda(), y[:3].cuda())
    with pytest.raises(ValueError):
        tr.step(x[:, 0].cuda(), y.cuda())
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
    labels = torch.tensor([1 if s % 6 == 0 else 0 for s in seeds]).cuda()   # kind 0: the cough-like burst
    aug = cda.AudioAugmentor(p_augment=0.5)
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False,
                                use_spectral_contrast=False, device="cuda")
    spec = cda.SpecAugment()
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1)
    tr = ResidualTrainer(model, class_weights=[1.0, 5.0], seed=3)
    losses = []
    for step in range(40):
        feats = spec(pre.extract_features(aug.augment_batch(wav, seed=step)).unsqueeze(1))
        loss, _ = tr.step(feats, labels)
        losses.append(loss.item())
    # measured on an MI355X: 0.434 over steps 0-4, 0.038 over steps 35-39; the test asks for half of that drop
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    print(f"end-to-end: mean loss of steps 0-4 {first:.4f}, of steps 35-39 {last:.4f}")
    assert np.isfinite(losses).all() and last < 0.5 * first
