"""The HIP training step (csrc/train.hip) against the float64 restatement (tests/train_ref.py) over the shapes and data
``cough_train_forward_backward`` accepts: odd and even sizes at every stage, the smallest trainable images, batches of 1
to 1024, exact max-pool ties, inputs far from zero mean, the head's dropout / class-weight branches, and a trajectory
whose batch shape changes between steps.  The comparison is test_gpu_train.py's (train_ref.assert_step_matches).

Well-posedness.  Where the top two values of a stem max-pool window lie closer than f32 rounding, the kernel and the
float64 reference may pick different winners and route that window's gradient to different pixels: measured on random
inputs, one such window moves a stem weight gradient by ~1e-2 of its scale, and a batch of 1024 has ~10 windows within
1e-7.  So every case here quantises the stem conv weight and bias to a 2^-6 grid and its input to a grid fine enough to
keep the image (``_on_grid``): every stem pre-activation is then an exact multiple of the product of the two grid steps,
so f32 and f64 compute it exactly in any order, and two values of a window either tie exactly or differ by a grid step,
far above f32 rounding.  The rest of the network keeps the 1e-4 rule of test_gpu_train.py unchanged.

ReLU kinks.  The same holds for a ReLU input within f32 rounding of 0: the two runs may take its derivative from
different sides, and everything upstream of it then moves by a full term.  Measured: a block-0 output at 1.0e-7 moved
block 0's and the stem's weight gradients by 1e-2 .. 5e-2 of their scale at B = 16, an input of block 0's first ReLU at
1.7e-7 moved the stem's by 6e-4 at B = 32; B = 1024 has a dozen block inputs within 1e-6 of 0.  Such inputs cannot be
avoided by construction past the first BatchNorm, so ``train_ref.resolve_kinks`` takes the derivative of the few
inputs within 1e-6 of 0 from the side that brings the restatement closer to the kernel before the 1e-4 rule is
applied; it never touches the forward pass, the loss or the logits, and a case that needs no flip is unaffected.

Loss.  The loss is lse - z_y, a difference of numbers on the logits' scale: where the logits are large against the
loss (a near-saturated CE term, e.g. loss 1.6e-3 with logits of +-3; or loss 0.86 with logits up to 10 on a 5 x 7
image), the f32 rounding of the logits that their own rule admits (1e-5 of max(1, |z|)) reaches the loss unscaled, so
the loss is held to the relative 1e-5 or, failing that, to the logits' absolute bound.

BatchNorm over 2 values.  At B = 2 on the smallest images, block 1 (3 x 3: also block 0) is 1 x 1 and its BatchNorms
see two values per channel: xhat = +-d / sqrt(d^2 + eps), and the backward's dy - mean(dy) - xhat mean(dy xhat) keeps
only the fraction eps / (d^2 + eps) = eps / (var + eps) of terms of the size of dy.  One f32 rounding of those terms is
2^-24 (var + eps) / eps of the result: 1.7e-2 and 7.4e-3 at the two B = 2 cases here (var up to 2.9 and 1.2), where the
kernel was measured at 4.4e-4 and 2.9e-4 and torch's own f32 step on the CPU at 3.2e-3 and 2.0e-4.  Where a BatchNorm
sees 2 values the gradient rule is therefore max(1e-4, 2^-24 (var + eps) / eps); it is 1e-4 everywhere else."""
import copy
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cough_detector_amd as cda
from cough_detector_amd.training import ResidualTrainer, train_epoch
from train_ref import (BN_FED_BIASES, PARAM_NAMES, RefStep, assert_step_matches, resolve_kinks,
                       step_on_the_kernels_side)

pytestmark = pytest.mark.gpu
CW = [1.0, 2.5]
STEM_GRID = 2.0 ** -6


def _sizes(n):
    """stem conv, stem max-pool, block 0, block 1 output sizes of an input side of n"""
    s = (n - 1) // 2 + 1
    p = s // 2
    b0 = (p - 1) // 2 + 1
    return s, p, b0, (b0 - 1) // 2 + 1


def _geo_id(b, h, w):
    """e.g. B8-H90[45*,22,11*,6]-W51[26,13*,7*,4]: stem, pool, block 0, block 1 sizes; * marks the odd ones"""
    side = lambda n: ",".join(f"{v}*" if v % 2 else str(v) for v in _sizes(n))
    return f"B{b}-H{h}[{side(h)}]-W{w}[{side(w)}]"


def _trainable(b, h, w):
    return _sizes(h)[1] >= 1 and _sizes(w)[1] >= 1 and b * _sizes(h)[3] * _sizes(w)[3] > 1


@pytest.fixture(scope="module")
def qsd(resnet_golden):
    """the golden state with the stem conv's weight and bias on the 2^-6 grid and the head scaled by 1/20: the golden
    head is calibrated for 90 x 101 images and gives logits of +-100 on other images, where the loss saturates (a CE
    term of log(1 + e^-12) keeps one significant digit in f32, in torch's f32 step as in this one) and the gradient
    vanishes to 1e-21; at 1/20 the logits stay within a few units"""
    sd = dict(resnet_golden[0])
    for k in ("conv1.0.weight", "conv1.0.bias"):
        sd[k] = torch.round(sd[k] / STEM_GRID) * STEM_GRID
    sd["fc.2.weight"] = sd["fc.2.weight"] / 20
    sd["fc.2.bias"] = sd["fc.2.bias"] / 20
    return sd


def _on_grid(x, step, sd):
    """x rounded to multiples of ``step``; asserts that every stem pre-activation is then exact in f32 (a multiple of
    step * 2^-6 below 2^24 of them)"""
    x = torch.round(x / step) * step
    bound = float(x.abs().max()) * float(sd["conv1.0.weight"].abs().sum(dim=(1, 2, 3)).max()) + float(
        sd["conv1.0.bias"].abs().max())
    assert bound < 2.0 ** 24 * step * STEM_GRID, bound
    return x


def _model(sd, p=0.5):
    m = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    m.load_state_dict(sd)
    m.fc[1].p = p
    return m


def _batch(b, h, w, seed, sd):
    g = torch.Generator().manual_seed(seed)
    x = _on_grid(torch.randn(b, 1, h, w, generator=g), 2.0 ** -8, sd)
    y = torch.randint(0, 2, (b,), generator=g)
    mask = (torch.rand(b, 128, generator=g) >= 0.5).float()
    return x, y, mask


def _check_step(sd, x, y, mask, p=0.5, class_weights=CW):
    """one forward/backward on both sides, compared; returns (trainer, ref, worst relative gradient error)"""
    tr = ResidualTrainer(_model(sd, p), class_weights=class_weights)
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    torch.cuda.synchronize()
    ref = RefStep(sd, class_weights=class_weights)
    rloss, rlogits, rg = ref.grads(x, y, mask, p)
    worst = _compare(tr, loss, logits, ref, rloss, rlogits, rg, sd)
    return tr, ref, worst


def _compare(tr, loss, logits, ref, rloss, rlogits, rg, sd):
    g = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
    # a BatchNorm over 2 values per channel (see the module docstring): its backward keeps only eps / (var + eps) of
    # its input gradient, one f32 rounding of which is 2^-24 (var + eps) / eps of what survives
    kappa = max([((v + 1e-5) / 1e-5).max().item() for n, v in ref.batch_var.values() if n == 2], default=0.0)
    rtol = max(1e-4, 2.0 ** -24 * kappa)
    rg, kept = resolve_kinks(g, ref, rg, rtol=rtol)
    worst = assert_step_matches(tr.model, loss, logits, rloss, rlogits, rg, ref.state_dict(), sd,
                                loss_on_logit_scale=True, grad_rtol=rtol)
    print(f"worst gradient error {worst:.2e} of scale; ReLU derivatives taken from the other side: {kept}")
    return worst


# ---------------------------------------------------------------------------------------------------------- geometry
GEOMETRY = [
    (8, 90, 51), (8, 90, 201),              # 0.5 s and 2 s windows
    (8, 67, 101), (8, 110, 101),            # H 67: 34, 17*, 9*, 5*;  H 110: 55*, 27*, 14, 7*
    (6, 64, 64),                            # 32, 16, 8, 4 on both sides: even at every stage
    (2, 3, 3), (3, 3, 3), (2, 5, 7), (3, 5, 7),   # the smallest trainable images: block 1 is 1 x 1, BN sees B values
]


@pytest.mark.parametrize("b,h,w", GEOMETRY, ids=[_geo_id(*g) for g in GEOMETRY])
def test_geometry(qsd, b, h, w):
    assert _trainable(b, h, w)
    _check_step(qsd, *_batch(b, h, w, seed=b * 1000 + h * 7 + w, sd=qsd))


def _fuzz_shapes(n=12, seed=2026):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        b, h, w = rng.randint(1, 40), rng.randint(3, 128), rng.randint(3, 256)
        if _trainable(b, h, w):
            out.append((b, h, w))
    return out


FUZZ = _fuzz_shapes()


@pytest.mark.parametrize("b,h,w", FUZZ, ids=[_geo_id(*g) for g in FUZZ])
def test_geometry_fuzz(qsd, b, h, w):
    _check_step(qsd, *_batch(b, h, w, seed=b + 3 * h + 5 * w, sd=qsd))


# ---------------------------------------------------------------------------------------------------------- batch
@pytest.mark.parametrize("b", [1, 2, 3, 33, 127, 129])
def test_batch_sizes(qsd, b):
    _check_step(qsd, *_batch(b, 90, 101, seed=b, sd=qsd))


def test_batch_of_1024(qsd):
    """The stem wgrad sums B * 32 * 51 = 1.67 M rows, inside the 2.4 M-term sums the 1e-4 rule was argued for."""
    import time
    x, y, mask = _batch(1024, 64, 101, seed=1024, sd=qsd)
    tr = ResidualTrainer(_model(qsd), class_weights=CW)
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = RefStep(qsd, class_weights=CW)
    rloss, rlogits, rg = ref.grads(x, y, mask, 0.5)
    print(f"float64 reference at B = 1024: {time.perf_counter() - t0:.1f} s")
    _compare(tr, loss, logits, ref, rloss, rlogits, rg, qsd)


# ---------------------------------------------------------------------------------------------------------- ties
def _pool_windows(ref, x):
    """the f64 stem ReLU(BN) outputs of every 2 x 2 max-pool window, (n, 4) in the pool's scan order"""
    P = ref.P
    with torch.no_grad():
        z = F.conv2d(x.double(), P["conv1.0.weight"], P["conv1.0.bias"], stride=2, padding=3)
        v = F.relu(F.batch_norm(z, None, None, P["conv1.1.weight"], P["conv1.1.bias"], training=True,
                                eps=ref.bn_eps))
    b, c, oh, ow = v.shape
    v = v[:, :, :oh // 2 * 2, :ow // 2 * 2].reshape(b, c, oh // 2, 2, ow // 2, 2)
    return v.permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)


def _blocky(b, h, w, seed, sd):
    """piecewise constant on 8 x 8 blocks, integer values (on the 2^-3 grid: few levels keep distinct pool values 1e-3
    apart), about 60 % of the blocks 0 (the floor)"""
    g = torch.Generator().manual_seed(seed)
    hb, wb = (h + 7) // 8, (w + 7) // 8
    v = torch.round(torch.randn(b, 1, hb, wb, generator=g))
    v = v * (torch.rand(b, 1, hb, wb, generator=g) >= 0.6)
    x = v.repeat_interleave(8, dim=2).repeat_interleave(8, dim=3)[:, :, :h, :w].contiguous()
    y = torch.randint(0, 2, (b,), generator=g)
    mask = (torch.rand(b, 128, generator=g) >= 0.5).float()
    return _on_grid(x, 2.0 ** -3, sd), y, mask


def test_max_pool_ties_exact_by_construction(qsd):
    """The stem pool keeps the first of equal values, as torch does; a kernel that kept another one would route the
    gradient of every tied window to a pixel under a different input patch."""
    x, y, mask = _blocky(16, 90, 101, seed=6, sd=qsd)
    win = _pool_windows(RefStep(qsd), x)
    top = win.max(dim=1).values
    d = (win.unsqueeze(2) - win.unsqueeze(1)).abs()                      # every pair of a window
    rel = d / top.clamp_min(1e-300).view(-1, 1, 1)
    pos = top > 0
    assert bool(((d == 0) | (rel > 1e-3))[pos].all()), "a window is neither an exact tie nor separated by 1e-3"
    top2 = win.sort(dim=1, descending=True).values[:, 1]
    tied = (top2 == top) & pos
    frac = tied.sum().item() / pos.sum().item()
    print(f"{frac:.1%} of the {pos.sum().item()} windows with a positive max are ties")
    assert frac >= 0.2
    _check_step(qsd, x, y, mask)


def test_max_pool_ties_from_padded_specaugmented_features(qsd):
    """synth clips zero-padded from half length, featurised, SpecAugment (p = 1): a constant floor and constant
    bands, as in real training."""
    from cough_detector_amd import synth
    random.seed(7)
    torch.manual_seed(7)
    wav = torch.from_numpy(np.stack([synth.make_clip(s) for s in range(24)]))
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False,
                                use_spectral_contrast=False, device="cuda")
    half = pre.pad_or_trim(wav[:, :wav.shape[1] // 2].cuda(), wav.shape[1])
    feats = cda.SpecAugment(p=1.0)(pre.extract_features(half).unsqueeze(1)).cpu()
    x = _on_grid(feats, 2.0 ** -10, qsd)
    y = torch.tensor([s % 2 for s in range(24)])
    mask = (torch.rand(24, 128, generator=torch.Generator().manual_seed(7)) >= 0.5).float()
    _check_step(qsd, x, y, mask)


# ---------------------------------------------------------------------------------------------------------- data scale
def test_raw_db_spectrogram_far_from_zero_mean(qsd):
    """The featuriser's own output is normalised ([0, 1] mel rows, z-scored MFCC); its STFT stage in dB (10 log10 of the
    power, 90 bins) sits around -60 with |x| up to ~100.  The BatchNorm statistics are centred sums for this."""
    from cough_detector_amd import synth
    wav = torch.from_numpy(np.stack([synth.make_clip(s, peak_normalize=False) for s in range(100, 112)])) * 0.05
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False,
                                use_spectral_contrast=False, device="cuda")
    power = pre.spectrogram_batch(wav.cuda()).cpu()
    db = 10.0 * torch.log10(power[:, 2:92].clamp_min(1e-10)).unsqueeze(1)
    print(f"raw dB image: mean {db.mean().item():.1f}, max |x| {db.abs().max().item():.1f}")
    x = _on_grid(db, 2.0 ** -6, qsd)
    y = torch.tensor([s % 2 for s in range(12)])
    mask = (torch.rand(12, 128, generator=torch.Generator().manual_seed(3)) >= 0.5).float()
    _check_step(qsd, x, y, mask)


def test_images_offset_by_1000(qsd):
    x, y, mask = _batch(16, 90, 101, seed=1000, sd=qsd)
    _check_step(qsd, _on_grid(x + 1000.0, 2.0 ** -3, qsd), y, mask)


# ---------------------------------------------------------------------------------------------------------- head
def test_dropout_p0(qsd):
    _check_step(qsd, *_batch(8, 90, 101, seed=40, sd=qsd), p=0.0)


def test_dropout_p1_leaves_only_the_fc_bias_gradient(qsd):
    tr, _, _ = _check_step(qsd, *_batch(8, 90, 101, seed=41, sd=qsd), p=1.0)
    for n, p in tr.model.named_parameters():
        if n != "fc.2.bias":
            assert torch.count_nonzero(p.grad).item() == 0, n
    assert torch.count_nonzero(tr.model.fc[2].bias.grad).item() == 2


def test_class_weight_zero_on_a_mixed_batch(qsd):
    x, y, mask = _batch(16, 90, 101, seed=42, sd=qsd)
    y[:8] = 0
    y[8:] = 1
    _check_step(qsd, x, y, mask, class_weights=[0.0, 1.0])


def test_all_targets_weight_zero_gives_nan(qsd):
    x, y, mask = _batch(8, 90, 101, seed=43, sd=qsd)
    y[:] = 0
    tr = ResidualTrainer(_model(qsd), class_weights=[0.0, 1.0])
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    rloss, rlogits, _ = RefStep(qsd, class_weights=[0.0, 1.0]).grads(x, y, mask, 0.5)
    assert torch.isnan(rloss).item() and torch.isnan(loss).item()       # 0 / 0, as torch
    assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * max(1.0, rlogits.abs().max().item())


@pytest.mark.parametrize("cls", [0, 1])
def test_single_class_batch(qsd, cls):
    x, y, mask = _batch(12, 90, 101, seed=44 + cls, sd=qsd)
    _check_step(qsd, x, torch.full_like(y, cls), mask)


# ---------------------------------------------------------------------------------------------------------- trajectory
def _loader(n, h, seed, sd):
    """what DataLoader(dataset of n, batch_size=32, shuffle=False) yields: batches of 32, 32, ..., n % 32"""
    x, y, _ = _batch(n, h, 101, seed=seed, sd=sd)
    return [(x[i:i + 32], y[i:i + 32]) for i in range(0, n, 32)]


def test_trajectory_with_changing_shapes_scheduler_device_dropout_and_zero_grad(qsd):
    """18 steps: 3 epochs of a 70-item loader at 90 x 101 (batches 32, 32, 6), then 3 at 103 x 101; the scheduler
    steps per epoch and the reference's optimizer.zero_grad() runs before every step.  Each step is checked against
    the restatement started from the trainer's own state (parameters, BN buffers, AdamW moments, lr): loss, logits,
    then the parameters and moments after the update; a restatement that runs free alongside bounds where the two
    trajectories end."""
    lr = 1e-3
    tr = ResidualTrainer(_model(qsd), lr=lr, class_weights=CW, seed=99)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(tr.optimizer, T_0=2, T_mult=1, eta_min=1e-5)
    free = RefStep(qsd, lr=lr, class_weights=CW)
    fsched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(free.opt, T_0=2, T_mult=1, eta_min=1e-5)
    flat = tr._grads
    lr_sum, steps = 0.0, 0
    for epoch in range(6):
        for x, y in _loader(70, 90 if epoch < 3 else 103, seed=epoch % 3, sd=qsd):
            tr.optimizer.zero_grad()
            if steps % 2:
                tr.model.zero_grad()                                     # torch's default set_to_none=True
            ref = RefStep({k: v.cpu() for k, v in tr.model.state_dict().items()}, lr=lr, class_weights=CW)
            ref.opt.load_state_dict(copy.deepcopy(tr.optimizer.state_dict()))
            assert ref.opt.param_groups[0]["lr"] == tr.optimizer.param_groups[0]["lr"]
            lr_t = tr.optimizer.param_groups[0]["lr"]
            lr_sum += lr_t
            m = torch.empty(x.shape[0], 128, device="cuda")
            loss, logits = tr.forward_backward(x.cuda(), y.cuda(), mask_out=m)
            for p in tr.model.parameters():
                assert p.grad is not None and p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
            # ReLU inputs within rounding of 0 from the kernel's side, as in every single-step check (resolve_kinks)
            grads = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
            tr.optimizer.step()
            rloss, rlogits, _, _, _ = step_on_the_kernels_side(ref, grads, x, y, m.cpu(), 0.5)
            assert abs(loss.item() - rloss.item()) <= 1e-5 * abs(rloss.item()), (steps, loss.item(), rloss.item())
            assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * max(1.0, rlogits.abs().max().item())
            # the update itself, from the same state: AdamW moves a parameter by at most ~lr, so where a gradient is at
            # f32 noise level the two may step apart by up to 2 lr; the bulk agrees to 1e-5, the moments' bulk to 1e-4
            # of their scale (test_three_reference_steps_from_the_golden's rules, per step)
            sd, ost, rsd = tr.model.state_dict(), tr.optimizer.state_dict()["state"], ref.state_dict()
            for i, n in enumerate(PARAM_NAMES):
                if n in BN_FED_BIASES:
                    continue
                d = (sd[n].cpu().double() - rsd[n]).abs()
                assert d.max().item() <= 2 * lr_t and d.median().item() <= 1e-5, (steps, n)
                rst = ref.opt.state[ref.P[n]]
                for k in ("exp_avg", "exp_avg_sq"):
                    got, want = ost[i][k].cpu().double(), rst[k]
                    assert (got - want).abs().median().item() <= 1e-4 * want.abs().max().item(), (steps, n, k)
            free.step(x, y, m.cpu(), 0.5)
            steps += 1
        sched.step()
        fsched.step()
    assert steps == 18
    sd = tr.model.state_dict()
    rsd = free.state_dict()
    worst = 0.0
    for n in PARAM_NAMES:
        if n in BN_FED_BIASES:                   # true gradient 0: AdamW steps of up to lr on rounding noise
            continue
        d = (sd[n].cpu().double() - rsd[n]).abs()
        # AdamW moves a parameter by at most ~lr per step: where a gradient is at noise level the two runs may step
        # apart, by at most 2 lr per step
        assert d.max().item() <= 2 * lr_sum, n
        worst = max(worst, d.median().item())
    print(f"free-running trajectories after 18 steps: largest median parameter difference {worst:.2e}")


def test_train_epoch_matches_the_same_loop_on_the_restatement(qsd):
    loader = _loader(70, 90, seed=11, sd=qsd)
    tr = ResidualTrainer(_model(qsd), class_weights=CW, seed=5)
    twin = ResidualTrainer(_model(qsd), class_weights=CW, seed=5)       # same seed: the same device dropout draws
    masks = []
    for x, y in loader:
        m = torch.empty(x.shape[0], 128, device="cuda")
        twin.forward_backward(x.cuda(), y.cuda(), mask_out=m)
        masks.append(m.cpu())
    res = train_epoch(tr, loader, 0)
    ref = RefStep(qsd, class_weights=CW)
    losses, correct, total = [], 0, 0
    for (x, y), m in zip(loader, masks):
        loss, logits, _, _ = ref.step(x, y, m, 0.5)
        losses.append(loss.item())
        correct += int((logits.argmax(1) == y).sum())
        total += y.numel()
    want = {"loss": float(np.mean(losses)), "accuracy": 100.0 * correct / total}
    print(f"train_epoch {res}, restatement {want}")
    assert set(res) == {"loss", "accuracy"}
    # steps 1 and 2 start from states that differ by f32 AdamW updates of noise-level gradients (see the trajectory
    # test): the mean loss of the three steps agrees to 1e-4, as test_gpu_train.py found for the golden's step 2
    assert abs(res["loss"] - want["loss"]) <= 1e-4 * abs(want["loss"])
    assert res["accuracy"] == want["accuracy"]
