"""The Small and Standard HIP training steps (csrc/train_small.hip, csrc/train_std.hip) against their float64
restatements on the data and branches that test_gpu_train_small.py / test_gpu_train_std.py leave out: exact max-pool
ties in every pool, ties from the real pipeline, images far from zero mean, the heads' dropout and class-weight
branches, a seeded shape fuzz and a trajectory whose batch shape changes.  test_gpu_train_shapes.py is the residual
net's file of the same kind and explains the rules; they are unchanged here: loss and logits 1e-5, every gradient within
1e-4 of its tensor's largest, running statistics rtol 1e-5, max(1e-4, 2^-24 (var + eps) / eps) where a BatchNorm sees
2 values.

Well-posedness.  Conv 0's weight and bias are on the 2^-6 grid and the input on a grid that keeps conv 0 exact
(``_on_grid`` asserts it), so the first pool's windows tie exactly or differ by far more than rounding.  The later pools
(two in Small, three in Standard) see rounded values: a window whose top two values lie within 1e-6 relative, like a
ReLU input within 1e-6 of 0, is a choice that float32 cannot make reliably, and ``resolve_kinks(ties=True)`` takes it
from the kernel's side (pool_ties_ref.py).  At most ``MAX_KEPT`` = 8 such choices per step: a step that needs more
fails.  Exact ties are never candidates: the first of equal values in scan order is what the tie tests check.

Standard's deeper pools.  The resolver's reach ends at 1e-6, but the Standard net's last pools see 576- and 1152-term
dot products whose float32 rounding is 1.4e-6 and 2e-6 of the value: measured, one batch in ten of 12 to 21 clips had a
window 1.3e-6 .. 3.7e-6 apart that the HIP step (and mostly torch's float32 step too) decided the other way, each
moving conv 0's weight gradient by 5e-4 .. 8e-3 of its scale and nothing else wrong to 2e-6.  The threshold stays; the
random Standard inputs are instead drawn (seed, seed + 1000, ...) until the float64 restatement alone shows no window of
the later pools 1e-6 .. 4e-6 apart (``pool_ties_ref.grey_windows``), and are kept below B F T = 80,000 so that such a
draw turns up.  The fixed inputs (blocks, pipeline features, raw dB, + 1000) and the trajectory take what they get.

Every check prints its worst gradient error (before it asserts) and the choices it took from the kernel's side.
"""
import copy
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
import train_small_ref
import train_std_ref
from cough_detector_amd.training import SmallTrainer, StandardTrainer
from pool_ties_ref import MAX_KEPT, equal_up_to_rounding, grey_windows, tie_census
from test_train_small_host import small_sd
from test_train_std_host import std_sd

pytestmark = pytest.mark.gpu
CW = [1.0, 2.5]
GRID = 2.0 ** -6


class _Net:
    """what differs between the two nets: restatement module, trainer, conv 0 / head names, dropout arguments"""

    def __init__(self, kind):
        self.kind = kind
        small = kind == "small"
        self.ref = train_small_ref if small else train_std_ref
        self.trainer_cls = SmallTrainer if small else StandardTrainer
        self.conv0 = "features.0" if small else "conv_layers.0.conv"
        self.head = "classifier.4" if small else "fc.3"
        self.ps = (0.3,) if small else (0.1, 0.5)           # the reference's defaults
        self.min_side = 8 if small else 16
        self.mask_width = 64 if small else train_std_ref.MASK_WIDTH
        self.pools = 3 if small else 4

    def __repr__(self):
        return self.kind

    def trainable(self, b, h, w):
        if self.kind == "small":
            return h >= 8 and w >= 8 and b * (h // 8) * (w // 8) > 1
        return h >= 16 and w >= 16

    def drawable(self, b, h, w):
        """Standard: few enough pool windows that a draw without a grey one turns up (pool_ties_ref.grey_windows)"""
        return self.trainable(b, h, w) and (self.kind == "small" or b * h * w <= 80000)

    def state(self):
        """the golden state with conv 0 on the 2^-6 grid and the head scaled by 1/100 (the ``qsd`` of
        test_gpu_train_small.py / test_gpu_train_std.py)"""
        sd = dict(small_sd() if self.kind == "small" else std_sd())
        for k in (self.conv0 + ".weight", self.conv0 + ".bias"):
            sd[k] = torch.round(sd[k] / GRID) * GRID
        sd[self.head + ".weight"] = sd[self.head + ".weight"] / 100
        sd[self.head + ".bias"] = sd[self.head + ".bias"] / 100
        return sd

    def model(self, sd, ps):
        m = cda.create_model(self.kind, n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
        m.load_state_dict(sd)
        if self.kind == "small":
            m.classifier[3].p = ps[0]
        else:
            for blk in m.conv_layers:
                blk.dropout.p = ps[0]
            m.fc[2].p = ps[1]
        return m

    def mask(self, b, g):
        if self.kind == "small":
            return (torch.rand(b, 64, generator=g) >= 0.3).float()
        off = train_std_ref.MASK_OFF[4]
        m = torch.empty(b, self.mask_width)
        m[:, :off] = (torch.rand(b, off, generator=g) >= 0.1).float()
        m[:, off:] = (torch.rand(b, self.mask_width - off, generator=g) >= 0.5).float()
        return m

    def compare(self, model, loss, logits, rloss, rlogits, rg, rsd, sd, rule):
        if self.kind == "small":
            return train_small_ref.assert_step_matches(model, loss, logits, rloss, rlogits, rg, rsd, sd,
                                                       loss_on_logit_scale=True, grad_rtol=rule)
        return train_std_ref.assert_step_matches(model, loss, logits, rloss, rlogits, rg, rsd, sd, grad_rtol=rule)


NETS = {"small": _Net("small"), "standard": _Net("standard")}
_STATES = {}


@pytest.fixture(params=["small", "standard"])
def net(request):
    return NETS[request.param]


def _sd(net):
    if net.kind not in _STATES:
        _STATES[net.kind] = net.state()
    return _STATES[net.kind]


def _on_grid(x, step, net):
    """x rounded to multiples of ``step``; asserts that every conv 0 output is then exact in f32 (a multiple of
    step * 2^-6 below 2^24 of them)"""
    sd = _sd(net)
    x = torch.round(x / step) * step
    bound = float(x.abs().max()) * float(sd[net.conv0 + ".weight"].abs().sum(dim=(1, 2, 3)).max()) + float(
        sd[net.conv0 + ".bias"].abs().max())
    assert bound < 2.0 ** 24 * step * GRID, bound
    return x


def _draw(net, b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = _on_grid(torch.randn(b, 1, h, w, generator=g), 2.0 ** -10, net)
    y = torch.randint(0, 2, (b,), generator=g)
    return x, y, net.mask(b, g)


def _grey(net, x, mask, ps):
    ref = net.ref.RefStep(_sd(net))
    with torch.no_grad():
        ref.forward(x.double(), mask, *ps)
    return grey_windows(ref)


def _first_without_grey(net, draw, seed, ps=None):
    """Standard: the first of draw(seed), draw(seed + 1000), ... whose float64 forward has no grey pool window
    (pool_ties_ref.grey_windows: a rule on the restatement alone; Small needs none and takes the first draw)"""
    for k in range(40):
        x, y, mask = draw(seed + 1000 * k)
        grey = _grey(net, x, mask, net.ps if ps is None else ps) if net.kind == "standard" else 0
        if grey == 0:
            return x, y, mask
        print(f"{net.kind} {tuple(x.shape)} seed {seed + 1000 * k}: {grey} grey pool windows, drawing again")
    raise AssertionError("40 draws with a grey pool window")


def _batch(net, b, h, w, seed, ps=None):
    return _first_without_grey(net, lambda s: _draw(net, b, h, w, s), seed, ps)


def _rule(ref):
    """1e-4, or 2^-24 (var + eps) / eps where a BatchNorm sees 2 values per channel (test_gpu_train_shapes.py)"""
    kappa = max([((v + 1e-5) / 1e-5).max().item() for n, v in ref.batch_var.values() if n == 2], default=0.0)
    return max(1e-4, 2.0 ** -24 * kappa)


def _check_step(net, x, y, mask, ps=None, class_weights=CW):
    """one forward/backward on both sides, compared; returns (trainer, ref, worst relative gradient error)"""
    sd = _sd(net)
    ps = net.ps if ps is None else ps
    tr = net.trainer_cls(net.model(sd, ps), class_weights=class_weights)
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    torch.cuda.synchronize()
    ref = net.ref.RefStep(sd, class_weights=class_weights)
    rloss, rlogits, rg = ref.grads(x, y, mask, *ps)
    g = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
    rule = _rule(ref)
    moved = equal_up_to_rounding(ref)
    if moved:
        rg = ref.regrad()
    plain = net.ref._worst(g, rg)
    rg, kept = net.ref.resolve_kinks(g, ref, rg, rtol=rule, ties=True)
    print(f"{net.kind} {tuple(x.shape)}: worst gradient error {net.ref._worst(g, rg):.2e} of scale (rule {rule:.1e}; "
          f"{plain:.2e} before {len(kept)} choices were taken from the kernel's side: {kept}); "
          f"{grey_windows(ref)} grey windows, {moved} windows of float64-equal values given to their first")
    assert len(kept) <= MAX_KEPT
    worst = net.compare(tr.model, loss, logits, rloss, rlogits, rg, ref.state_dict(), sd, rule)
    return tr, ref, worst


# ---------------------------------------------------------------------------------------------------------- ties
def _blocky(net, b, h, w, seed):
    """piecewise constant on 16 x 16 blocks, integer values, about 60 % of the blocks 0 (the floor): the blocks are
    wider than what the last pool sees of the image, so every pool has windows over constant input"""
    g = torch.Generator().manual_seed(seed)
    hb, wb = (h + 15) // 16, (w + 15) // 16
    v = torch.round(torch.randn(b, 1, hb, wb, generator=g))
    v = v * (torch.rand(b, 1, hb, wb, generator=g) >= 0.6)
    x = v.repeat_interleave(16, dim=2).repeat_interleave(16, dim=3)[:, :, :h, :w].contiguous()
    y = torch.randint(0, 2, (b,), generator=g)
    return _on_grid(x, 2.0 ** -3, net), y, net.mask(b, g)


BLOCKY = {"small": (16, 90, 101, 6), "standard": (8, 64, 80, 6)}


def test_exact_ties_in_every_pool(net):
    """Every pool keeps the first of equal values, as torch does: Small recomputes the window's winner in five kernels,
    Standard stores one byte per pooled value.  The image is such that, in the float64 restatement, every
    positive-maximum window of every pool is an exact tie or separated by 1e-6 relative (Standard's later pools: by
    4e-6, no grey window), and at least 5 % of each pool's are exact ties; the resolver then has no pool window to offer
    and first-of-equals is what is compared.  Exact means equal in float64 or within 1e-12 of the maximum: on CPUs with
    512-bit vectors torch's float64 convolution sums some pixels of a constant area in another order, and 0.05 to 0.3 %
    of the windows past the second pool then differ by 1e-16 .. 4e-13 (measured; none on 256-bit CPUs).  Those are
    the same value; ``equal_up_to_rounding`` gives them to their first pixel in the restatement, as the rule says."""
    b, h, w, seed = BLOCKY[net.kind]
    x, y, mask = _blocky(net, b, h, w, seed)
    ref = net.ref.RefStep(_sd(net), class_weights=CW)
    ref.grads(x, y, mask, *net.ps)
    assert len(ref.pool_in) == net.pools
    for name, v in ref.pool_in.items():
        c = tie_census(v)
        tied = c["exact"] + c["rounding"]
        print(f"{net.kind} {name}: {c['positive']} positive windows, {tied / c['positive']:.1%} exact ties "
              f"({c['rounding']} of them equal only up to float64 rounding), {c['near']} near ties, {c['grey']} grey")
        assert c["near"] == 0 and (c["grey"] == 0 or net.kind == "small" or name == "p0"), name
        assert tied >= 0.05 * c["positive"], name
    _check_step(net, x, y, mask)


def _padded_specaugmented(net):
    """synth clips zero-padded from half length, featurised, SpecAugment (p = 1): a constant floor and constant bands,
    as in real training (test_gpu_train_shapes.py's input)"""
    from cough_detector_amd import synth
    random.seed(7)
    torch.manual_seed(7)
    wav = torch.from_numpy(np.stack([synth.make_clip(s) for s in range(24)]))
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False,
                                use_spectral_contrast=False, device="cuda")
    half = pre.pad_or_trim(wav[:, :wav.shape[1] // 2].cuda(), wav.shape[1])
    feats = cda.SpecAugment(p=1.0)(pre.extract_features(half).unsqueeze(1)).cpu()
    x = _on_grid(feats, 2.0 ** -10, net)
    y = torch.tensor([s % 2 for s in range(24)])
    return x, y, net.mask(24, torch.Generator().manual_seed(7))


def test_ties_from_padded_specaugmented_features(net):
    _check_step(net, *_padded_specaugmented(net))


# ---------------------------------------------------------------------------------------------------------- data scale
def _raw_db(net):
    """the featuriser's STFT stage in dB (10 log10 of the power, 90 bins): around -60 with |x| up to ~100"""
    from cough_detector_amd import synth
    wav = torch.from_numpy(np.stack([synth.make_clip(s, peak_normalize=False) for s in range(100, 112)])) * 0.05
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False,
                                use_spectral_contrast=False, device="cuda")
    power = pre.spectrogram_batch(wav.cuda()).cpu()
    db = 10.0 * torch.log10(power[:, 2:92].clamp_min(1e-10)).unsqueeze(1)
    print(f"raw dB image: mean {db.mean().item():.1f}, max |x| {db.abs().max().item():.1f}")
    x = _on_grid(db, 2.0 ** -6, net)
    y = torch.tensor([s % 2 for s in range(12)])
    return x, y, net.mask(12, torch.Generator().manual_seed(3))


def test_raw_db_spectrogram_far_from_zero_mean(net):
    """the BatchNorm statistics (stats0 / stats / stats_part kernels: a float32 mean per range, then a Chan merge) on
    data whose mean is 2 to 3 times its spread"""
    _check_step(net, *_raw_db(net))


def _offset_by_1000(net):
    """no draw of this input is free of grey windows (hundreds in each: the zero padding of conv 0 puts the image
    borders hundreds away from the interior, whose values the BatchNorm then squeezes together), so the first draw is
    used as it is"""
    x, y, mask = _draw(net, 16, 90, 101, seed=1000)
    return _on_grid(x + 1000.0, 2.0 ** -3, net), y, mask


def test_images_offset_by_1000(net):
    _check_step(net, *_offset_by_1000(net))


# ---------------------------------------------------------------------------------------------------------- head
def _zero_grads(tr, names):
    for n, p in tr.model.named_parameters():
        if n in names:
            assert torch.count_nonzero(p.grad).item() == 0, n


def test_small_dropout_p0():
    _check_step(NETS["small"], *_batch(NETS["small"], 8, 90, 101, seed=40, ps=(0.0,)), ps=(0.0,))


def test_small_dropout_p1_leaves_only_the_last_bias_gradient():
    net = NETS["small"]
    tr, _, _ = _check_step(net, *_batch(net, 8, 90, 101, seed=41, ps=(1.0,)), ps=(1.0,))
    _zero_grads(tr, [n for n in train_small_ref.PARAM_NAMES if n != "classifier.4.bias"])
    assert torch.count_nonzero(tr.model.classifier[4].bias.grad).item() == 2


@pytest.mark.parametrize("p_fc", [0.0, 1.0])
def test_standard_dropout_p_fc(p_fc):
    net = NETS["standard"]
    tr, _, _ = _check_step(net, *_batch(net, 8, 90, 101, seed=40 + int(p_fc), ps=(0.1, p_fc)), ps=(0.1, p_fc))
    if p_fc == 1.0:
        _zero_grads(tr, [n for n in train_std_ref.PARAM_NAMES if n != "fc.3.bias"])
        assert torch.count_nonzero(tr.model.fc[3].bias.grad).item() == 2


def test_standard_dropout_p_block0():
    net = NETS["standard"]
    _check_step(net, *_batch(net, 8, 90, 101, seed=46, ps=(0.0, 0.5)), ps=(0.0, 0.5))


def test_standard_dropout_p_block1_stops_every_gradient_below_the_head():
    """Every block's output is dropped: the conv blocks and fc.0.weight see a gradient of exactly 0, the head trains on
    its biases alone, and the BatchNorm running statistics (of constant planes past block 0) still match."""
    net = NETS["standard"]
    tr, _, _ = _check_step(net, *_batch(net, 8, 90, 101, seed=47, ps=(1.0, 0.5)), ps=(1.0, 0.5))
    _zero_grads(tr, [n for n in train_std_ref.PARAM_NAMES if n.startswith("conv_layers.")] + ["fc.0.weight"])
    assert torch.count_nonzero(tr.model.fc[3].bias.grad).item() == 2


def test_class_weight_zero_on_a_mixed_batch(net):
    x, y, mask = _batch(net, 8, 90, 101, seed=42)
    y[:4] = 0
    y[4:] = 1
    _check_step(net, x, y, mask, class_weights=[0.0, 1.0])


def test_all_targets_weight_zero_gives_nan(net):
    x, y, mask = _batch(net, 8, 90, 101, seed=43)
    y[:] = 0
    tr = net.trainer_cls(net.model(_sd(net), net.ps), class_weights=[0.0, 1.0])
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    rloss, rlogits, _ = net.ref.RefStep(_sd(net), class_weights=[0.0, 1.0]).grads(x, y, mask, *net.ps)
    assert torch.isnan(rloss).item() and torch.isnan(loss).item()       # 0 / 0, as torch
    assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * max(1.0, rlogits.abs().max().item())


@pytest.mark.parametrize("cls", [0, 1])
def test_single_class_batch(net, cls):
    x, y, mask = _batch(net, 8, 90, 101, seed=44 + cls)
    _check_step(net, x, torch.full_like(y, cls), mask)


# ---------------------------------------------------------------------------------------------------------- fuzz
def _fuzz_shapes(net, n=12, seed=2026):
    rng = random.Random(f"{net.kind}-{seed}")
    out = []
    while len(out) < n:
        b, h, w = rng.randint(1, 24), rng.randint(net.min_side, 110), rng.randint(net.min_side, 130)
        if net.drawable(b, h, w):
            out.append((b, h, w))
    return out


FUZZ = [(k, *s) for k in NETS for s in _fuzz_shapes(NETS[k])]


@pytest.mark.parametrize("kind,b,h,w", FUZZ, ids=[f"{k}-B{b}-H{h}-W{w}" for k, b, h, w in FUZZ])
def test_geometry_fuzz(kind, b, h, w):
    _check_step(NETS[kind], *_batch(NETS[kind], b, h, w, seed=b + 3 * h + 5 * w))


# ---------------------------------------------------------------------------------------------------------- trajectory
def _loader(net, n, h, seed):
    """what DataLoader(dataset of n, batch_size=8, shuffle=False) yields: batches of 8, 8, ..., n % 8"""
    x, y, _ = _draw(net, n, h, 101, seed=seed)
    return [(x[i:i + 8], y[i:i + 8]) for i in range(0, n, 8)]


def test_trajectory_with_changing_shapes_scheduler_device_dropout_and_zero_grad(net):
    """12 steps: 2 epochs of a 20-item loader at 90 x 101 (batches 8, 8, 4), then 2 at 103 x 101, so the workspace is
    carved again at every step but the first of an epoch pair; the scheduler steps per epoch, optimizer.zero_grad()
    runs before every step and the module's zero_grad() (set_to_none) before every other one.  Each step is checked
    against the restatement started from the trainer's own state, as test_gpu_train_shapes.py's trajectory; a
    restatement that runs free alongside bounds where the two end."""
    sd0, lr, ps = _sd(net), 1e-3, net.ps
    tr = net.trainer_cls(net.model(sd0, ps), lr=lr, class_weights=CW, seed=99)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(tr.optimizer, T_0=2, T_mult=1, eta_min=1e-5)
    free = net.ref.RefStep(sd0, lr=lr, class_weights=CW)
    fsched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(free.opt, T_0=2, T_mult=1, eta_min=1e-5)
    names, fed = net.ref.PARAM_NAMES, net.ref.BN_FED_BIASES
    flat = tr._grads
    lr_sum, steps, changes = 0.0, 0, []
    for epoch in range(4):
        for x, y in _loader(net, 20, 90 if epoch < 2 else 103, seed=epoch % 2):
            tr.optimizer.zero_grad()
            if steps % 2:
                tr.model.zero_grad()                                     # torch's default set_to_none=True
            ref = net.ref.RefStep({k: v.cpu() for k, v in tr.model.state_dict().items()}, lr=lr, class_weights=CW)
            ref.opt.load_state_dict(copy.deepcopy(tr.optimizer.state_dict()))
            assert ref.opt.param_groups[0]["lr"] == tr.optimizer.param_groups[0]["lr"]
            lr_t = tr.optimizer.param_groups[0]["lr"]
            lr_sum += lr_t
            m = torch.empty(x.shape[0], net.mask_width, device="cuda")
            loss, logits = tr.forward_backward(x.cuda(), y.cuda(), mask_out=m)
            for p in tr.model.parameters():
                assert p.grad is not None and p.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
            grads = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
            tr.optimizer.step()
            rloss, rlogits, rg, _, kept = net.ref.step_on_the_kernels_side(ref, grads, x, y, m.cpu(), *ps, ties=True)
            print(f"{net.kind} step {steps} {tuple(x.shape)}: worst gradient error {net.ref._worst(grads, rg):.2e} of "
                  f"scale; taken from the kernel's side: {kept}")
            assert len(kept) <= MAX_KEPT
            changes.append(len(kept))
            assert abs(loss.item() - rloss.item()) <= 1e-5 * abs(rloss.item()), (steps, loss.item(), rloss.item())
            assert (logits.cpu().double() - rlogits).abs().max().item() <= 1e-5 * max(1.0, rlogits.abs().max().item())
            # the update itself, from the same state: AdamW moves a parameter by at most ~lr, so where a gradient is at
            # f32 noise level the two may step apart by up to 2 lr; the bulk agrees to 1e-5, the moments' bulk to 1e-4
            # of their scale
            sd, ost, rsd = tr.model.state_dict(), tr.optimizer.state_dict()["state"], ref.state_dict()
            for i, n in enumerate(names):
                if n in fed:
                    continue
                d = (sd[n].cpu().double() - rsd[n]).abs()
                assert d.max().item() <= 2 * lr_t and d.median().item() <= 1e-5, (steps, n)
                rst = ref.opt.state[ref.P[n]]
                for k in ("exp_avg", "exp_avg_sq"):
                    got, want = ost[i][k].cpu().double(), rst[k]
                    assert (got - want).abs().median().item() <= 1e-4 * want.abs().max().item(), (steps, n, k)
            free.step(x, y, m.cpu(), *ps)
            steps += 1
        sched.step()
        fsched.step()
    assert steps == 12
    sd, rsd = tr.model.state_dict(), free.state_dict()
    worst = 0.0
    for n in names:
        if n in fed:                             # true gradient 0: AdamW steps of up to lr on rounding noise
            continue
        d = (sd[n].cpu().double() - rsd[n]).abs()
        assert d.max().item() <= 2 * lr_sum, n
        worst = max(worst, d.median().item())
    print(f"{net.kind}: free-running trajectories after 12 steps: largest median parameter difference {worst:.2e}; "
          f"choices taken from the kernel's side per step: {changes}")
