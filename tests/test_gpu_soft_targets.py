"""Soft-target training on the MI355X: the three trainers' steps on (B, 2) class-probability targets
(``cough_train*_forward_backward_soft`` of libcough_amd_soft.so), ``cough_mix_batch``, and the loop and loader on mixed
batches.

No bound here is new.  The steps are held to ``assert_step_matches`` of the three restatements, given ``y.double()``
(``F.cross_entropy`` takes class probabilities unchanged): loss 1e-5 relative, logits 1e-5 of their scale, every gradient
within 1e-4 of its tensor's largest, running statistics rtol 1e-5, on the grids, with the ``resolve_kinks`` and the head
scaling of test_gpu_train_shapes.py, test_gpu_train_small.py and test_gpu_train_std.py, whose helpers are used as they
are (the widened gradient rule where a BatchNorm sees 2 values is theirs too).  Everything else is exact equality: a
one-hot soft step without class weights against the class-index step, a repeat, ``cough_mix_batch`` against
``MixUp.mix_batch``, ``train_epoch_async`` against ``train_epoch``, a mixing loader against the same loader without
``mixup`` followed by ``cough_mix_batch``.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
import soft_ref
import test_gpu_train_shapes as res_case
import test_gpu_train_small as small_case
import test_gpu_train_std as std_case
import train_ref
import train_small_ref
import train_std_ref
from cough_detector_amd import _lib
from cough_detector_amd import data as cdata
from cough_detector_amd.augmentation import mix_batch_rows, mix_coefficients
from cough_detector_amd.training import ResidualTrainer, SmallTrainer, StandardTrainer, train_epoch
from test_gpu_loop import CONFIG, SHIPPED, _Masked
from test_train_small_host import small_sd
from test_train_std_host import std_sd

pytestmark = pytest.mark.gpu
CW = [1.0, 2.5]
JUNK = 7.0e4


# ------------------------------------------------------------------------------------------------ the three trainers
@pytest.fixture(scope="module")
def states(resnet_golden):
    """the three models' states as the existing step tests prepare them: first conv on the 2^-6 grid, head scaled"""
    res = dict(resnet_golden[0])
    for k in ("conv1.0.weight", "conv1.0.bias"):
        res[k] = torch.round(res[k] / res_case.STEM_GRID) * res_case.STEM_GRID
    res["fc.2.weight"], res["fc.2.bias"] = res["fc.2.weight"] / 20, res["fc.2.bias"] / 20
    small = dict(small_sd())
    for k in ("features.0.weight", "features.0.bias"):
        small[k] = torch.round(small[k] / small_case.GRID) * small_case.GRID
    small["classifier.4.weight"], small["classifier.4.bias"] = small["classifier.4.weight"] / 100, small["classifier.4.bias"] / 100
    std = dict(std_sd())
    for k in ("conv_layers.0.conv.weight", "conv_layers.0.conv.bias"):
        std[k] = torch.round(std[k] / std_case.GRID) * std_case.GRID
    std["fc.3.weight"], std["fc.3.bias"] = std["fc.3.weight"] / 100, std["fc.3.bias"] / 100
    return {"residual": res, "small": small, "standard": std}


class _Kind:
    """What differs between the three trainers in a test: the trainer, its restatement, the batch recipe and the
    dropout probabilities its restatement takes."""

    def __init__(self, kind, sd):
        self.kind, self.sd = kind, sd
        self.cls = {"residual": ResidualTrainer, "small": SmallTrainer, "standard": StandardTrainer}[kind]
        self.ref_mod = {"residual": train_ref, "small": train_small_ref, "standard": train_std_ref}[kind]
        self.ps = {"residual": (0.5,), "small": (0.3,), "standard": (std_case.PB, std_case.PF)}[kind]

    def trainer(self, **kw):
        if self.kind == "residual":
            return ResidualTrainer(res_case._model(self.sd), **kw)
        return self.cls((small_case if self.kind == "small" else std_case)._model(self.sd), **kw)

    def ref(self, **kw):
        return self.ref_mod.RefStep(self.sd, **kw)

    def batch(self, b, h, w, seed):
        """(x, class indices, dropout mask) by the existing tests' recipe"""
        if self.kind == "residual":
            return res_case._batch(b, h, w, seed, self.sd)
        return (small_case if self.kind == "small" else std_case)._batch(b, h, w, seed)

    def shape_seed(self, b, h, w):
        """The seed the existing step test of this trainer draws its batch of this shape with.  The images are then the
        ones those tests have shown to be well-posed: on the smallest images, where every BatchNorm sees 2 values, another
        draw can leave a tensor with a true gradient of 0 by exact cancellation (measured at (2, 3, 3), seed 20: the stem
        BatchNorm's bias, 1.4e-13 in float64, where both clips pass every ReLU and the next BatchNorm removes the common
        shift), and a bound relative to that tensor's scale then says nothing about a float32 step."""
        return b * 1000 + h * 7 + w if self.kind == "residual" else b * 7 + h + w


def _state(tr):
    return [t.cpu().clone() for t in (tr._loss.reshape(1), tr._logits, tr._grads, tr._running, tr._nbt)]


SHAPES = {"small": [(2, 8, 8), (3, 8, 8), (5, 37, 29), (8, 90, 101)],
          "standard": [(4, 16, 16), (3, 17, 33), (8, 90, 101)],
          "residual": sorted(res_case.GEOMETRY, key=lambda g: g[0] * g[1] * g[2])[:2] + [(8, 90, 101)]}
STEP_CASES = [(k, b, h, w) for k in ("small", "standard", "residual") for b, h, w in SHAPES[k]]


def test_the_residual_shapes_are_the_two_smallest_of_the_geometry_list():
    assert SHAPES["residual"] == [(2, 3, 3), (3, 3, 3), (8, 90, 101)]


@pytest.mark.parametrize("cw", [None, CW], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind,b,h,w", STEP_CASES, ids=[f"{k}-{b}x{h}x{w}" for k, b, h, w in STEP_CASES])
def test_soft_step_matches_the_restatement(states, kind, b, h, w, cw):
    k = _Kind(kind, states[kind])
    x, _, mask = k.batch(b, h, w, seed=k.shape_seed(b, h, w))
    y = soft_ref.target_rows(b, seed=b + h)
    tr = k.trainer(class_weights=cw)
    loss, logits = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    torch.cuda.synchronize()
    ref = k.ref(class_weights=cw)
    rloss, rlogits, rg = ref.grads(x, y.double(), mask, *k.ps)
    # the float64 loss is the restated soft mean: the sum of the clips' terms over B
    want = soft_ref.soft_loss_and_dlogits(rlogits.numpy(), y.numpy(), cw)[0]
    assert abs(rloss.item() - want) <= 1e-12 * max(1.0, abs(want))
    g = {n: p.grad.detach().cpu().double() for n, p in tr.model.named_parameters()}
    # a BatchNorm over 2 values per channel keeps eps / (var + eps) of dy (test_gpu_train_shapes.py): the existing rule
    kappa = max([((v + 1e-5) / 1e-5).max().item() for n, v in ref.batch_var.values() if n == 2], default=0.0)
    rtol = max(1e-4, 2.0 ** -24 * kappa)
    rg, kept = k.ref_mod.resolve_kinks(g, ref, rg, rtol=rtol)
    kw = {} if kind == "standard" else {"loss_on_logit_scale": True}
    worst = k.ref_mod.assert_step_matches(tr.model, loss, logits, rloss, rlogits, rg, ref.state_dict(), k.sd, grad_rtol=rtol, **kw)
    print(f"{kind} {(b, h, w)} weights {cw}: loss {loss.item():.7f} float64 {rloss.item():.7f}; worst gradient error "
          f"{worst:.2e} of scale (rule {rtol:.1e}); ReLU derivatives from the other side: {len(kept)}")


@pytest.mark.parametrize("kind", ["small", "standard", "residual"])
def test_the_soft_mean_is_not_the_weighted_mean(states, kind):
    k = _Kind(kind, states[kind])
    x, t, mask = k.batch(8, 90, 101, seed=17)
    assert 0 < int(t.sum()) < 8
    y = torch.from_numpy(soft_ref.onehot(t.numpy()))
    tr = k.trainer(class_weights=CW)
    soft = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())[0].item()
    z = tr._logits.cpu().double().numpy()
    hard = k.trainer(class_weights=CW).forward_backward(x.cuda(), t.cuda(), dropout_mask=mask.cuda())[0].item()
    want = soft_ref.soft_loss_and_dlogits(z, y.numpy(), CW)[0]
    ratio = float(np.asarray(CW)[t.numpy()].sum()) / 8
    print(f"{kind}: soft {soft!r} restated {want!r} hard {hard!r} sum(w_y) / B {ratio!r}")
    assert abs(soft - want) <= 1e-5 * abs(want)
    assert abs(soft - hard * ratio) <= 1e-5 * abs(hard * ratio)
    assert abs(soft - hard) > 1e-2 * abs(hard) and ratio > 1.1


@pytest.mark.parametrize("kind", ["small", "standard", "residual"])
def test_one_hot_soft_targets_give_the_hard_step_bit_for_bit(states, kind):
    k = _Kind(kind, states[kind])
    x, t, mask = k.batch(5, 37, 29, seed=23)
    t[0], t[1] = 0, 1                                                      # both classes
    y = torch.from_numpy(soft_ref.onehot(t.numpy()))
    a, b = k.trainer(), k.trainer()
    a.forward_backward(x.cuda(), t.cuda(), dropout_mask=mask.cuda())
    b.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())
    for name, u, v in zip(("loss", "logits", "gradients", "running statistics", "num_batches_tracked"), _state(a), _state(b)):
        assert torch.equal(u, v), (kind, name, (u - v).abs().max().item())
    assert np.isfinite(_state(a)[0].item()) and _state(a)[2].abs().max().item() > 0


@pytest.mark.parametrize("kind", ["small", "standard", "residual"])
def test_a_repeated_soft_step_is_bit_identical_and_consumes_one_draw(states, kind):
    k = _Kind(kind, states[kind])
    x, t, _ = k.batch(5, 37, 29, seed=29)
    y = soft_ref.target_rows(5, seed=3)
    outs = []
    for _ in range(2):
        tr = k.trainer(class_weights=CW, seed=11)
        losses = []
        for i in range(2):
            losses.append(tr.step(x.cuda(), y.cuda())[0].item())
            assert tr._draws == i + 1
        tr.step(x.cuda(), t.cuda())                                        # a hard step consumes one as well
        assert tr._draws == 3
        outs.append([torch.tensor(losses)] + [v.cpu().clone() for v in (tr._params, tr._grads, tr._running)])
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    assert torch.isfinite(outs[0][0]).all()


@pytest.mark.parametrize("kind", ["small", "standard", "residual"])
def test_non_finite_input_gives_a_nan_loss_and_the_trainer_stays_usable(states, kind):
    k = _Kind(kind, states[kind])
    x, _, mask = k.batch(5, 37, 29, seed=31)
    y = soft_ref.target_rows(5, seed=5)
    tr = k.trainer(class_weights=CW)
    y_nan = y.clone()
    y_nan[3, 0] = float("nan")
    assert torch.isnan(tr.forward_backward(x.cuda(), y_nan.cuda(), dropout_mask=mask.cuda())[0]).item()
    fine = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())[0].item()
    x_nan = x.clone()
    x_nan[1, 0, 5, 7] = float("nan")
    assert torch.isnan(tr.forward_backward(x_nan.cuda(), y.cuda(), dropout_mask=mask.cuda())[0]).item()
    again = tr.forward_backward(x.cuda(), y.cuda(), dropout_mask=mask.cuda())[0].item()
    assert np.isfinite(fine) and again == fine                             # train mode reads no running statistic
    for bad in (torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 3), torch.zeros(5)):
        with pytest.raises(ValueError, match="targets"):
            tr.forward_backward(x.cuda(), bad.cuda())


# ------------------------------------------------------------------------------------------------ cough_mix_batch
def _perms(b):
    ident = list(range(b))
    cycle = [(i + 1) % b for i in range(b)]
    bad = list(cycle)
    bad[b // 2] = b if b % 2 else -1                                       # one entry outside 0..B-1
    return {"identity": ident, "cycle": cycle, "out of range": bad}


@pytest.mark.parametrize("n", [1, 7, 9090])
@pytest.mark.parametrize("b", [1, 2, 33])
def test_mix_batch_equals_mixup_mix_batch(b, n):
    g = torch.Generator().manual_seed(b * 10007 + n)
    labels = torch.randint(0, 2, (b,), generator=g)
    onehot = torch.from_numpy(soft_ref.onehot(labels.numpy()))
    mix = cda.MixUp(alpha=0.2)
    # x sits at every phase of 16 bytes inside a junk-filled buffer, and so does the output: nothing outside is touched
    for mis, (name, perm) in zip((0, 1, 2, 3), list(_perms(b).items()) + [("cycle", _perms(b)["cycle"])]):
        buf = torch.full((b * n + mis + 1,), JUNK)
        buf[mis:mis + b * n] = torch.randn(b * n, generator=g)
        dbuf = buf.cuda()
        x = dbuf[mis:mis + b * n].view(b, n)
        valid = [p if 0 <= p < b else r for r, p in enumerate(perm)]
        np.random.seed(b + n + mis)
        want_x, want_y = mix.mix_batch(x, onehot.cuda(), torch.tensor(valid))
        coef = torch.from_numpy(mix_coefficients(mix.last_lam)).cuda()
        dperm = torch.tensor(perm, dtype=torch.int32).cuda()
        obuf = torch.full((b * n + mis + 1,), JUNK, device="cuda")
        out, soft = obuf[mis:mis + b * n].view(b, n), torch.full((b, 2), JUNK, device="cuda")
        _lib.check_soft(_lib.load_soft().cough_mix_batch(x.data_ptr(), labels.cuda().data_ptr(), dperm.data_ptr(), coef.data_ptr(),
                                                         b, n, out.data_ptr(), soft.data_ptr(),
                                                         torch.cuda.current_stream().cuda_stream), "cough_mix_batch")
        for r, p in enumerate(perm):
            if not 0 <= p < b:                                             # no partner: the row comes back as it is
                want_x[r], want_y[r] = x[r], onehot[r].cuda()
        assert torch.equal(out, want_x) and torch.equal(soft, want_y), (name, mis)
        assert obuf[mis + b * n].item() == JUNK and (mis == 0 or obuf[mis - 1].item() == JUNK)
        assert torch.equal(dbuf.cpu(), buf)
        # the restatement, and the public wrapper on an aligned copy
        rx, ry = soft_ref.mix_batch(x.cpu().numpy(), labels.numpy(), perm, coef.cpu().numpy())
        assert np.array_equal(rx, out.cpu().numpy()) and np.array_equal(ry, soft.cpu().numpy())
        wx, wy = mix_batch_rows(x.contiguous(), labels.cuda(), dperm, coef)
        assert torch.equal(wx, out) and torch.equal(wy, soft)
    with pytest.raises(ValueError):
        mix_batch_rows(x.contiguous(), labels.cuda(), dperm[:-1] if b > 1 else dperm.long(), coef)


# ------------------------------------------------------------------------------------------------ loop and loader
def _soft_epoch(seed, sizes=(8, 8, 5)):
    g = torch.Generator().manual_seed(seed)
    data, masks = [], []
    for i, b in enumerate(sizes):
        y = soft_ref.target_rows(b, seed=seed + i)
        data.append((torch.randn(b, 1, 90, 101, generator=g), y))
        masks.append((torch.rand(b, 64, generator=g) >= 0.4).float())
    return data, masks


def test_train_epoch_async_equals_train_epoch_on_soft_batches(states):
    k = _Kind("small", states["small"])
    data, masks = _soft_epoch(seed=21)
    assert any((y[:, 0] == y[:, 1]).any() for _, y in data)               # ties are in
    a, b = k.trainer(class_weights=CW), k.trainer(class_weights=CW)
    logits = []

    class _Keep(_Masked):
        def step(self, inputs, targets):
            loss, z = super().step(inputs, targets)
            logits.append(z.cpu().clone())
            return loss, z

    want = [train_epoch(_Keep(a, masks), data, e) for e in range(2)]
    got = [cda.train_epoch_async(_Masked(b, masks), data, e) for e in range(2)]
    print(f"train_epoch {want} train_epoch_async {got}")
    assert got == want and np.isfinite(got[0]["loss"]) and got[0] != got[1]
    assert torch.equal(a._params, b._params) and torch.equal(a._running, b._running)
    # the accuracy counts the argmax of a soft row, a (0.5, 0.5) tie as class 0
    hits = sum(int(((z[:, 1] > z[:, 0]).long() == torch.from_numpy(soft_ref.soft_class(y.numpy()))).sum())
               for z, (_, y) in zip(logits[:3], data))
    assert want[0]["accuracy"] == 100.0 * hits / 21
    z, y = torch.tensor([[0.0, 1.0], [1.0, 0.0], [1.0, 0.0]]), torch.tensor([[0.5, 0.5], [0.5, 0.5], [0.2, 0.8]])
    meter = cda.EpochMeter("cuda")
    meter.update(z.cuda(), y.cuda(), batch_loss=torch.ones(1, device="cuda"))
    assert (meter.result()["correct"], meter.result()["total"]) == (1, 3)
    with pytest.raises(ValueError, match="batch_loss"):
        meter.update(z.cuda(), y.cuda())


LENGTHS = [700, 16000, 31, 16001, 8000]
LABELS = [0, 1, 0, 0, 1]


@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


@pytest.fixture(scope="module")
def bank():
    g = torch.Generator().manual_seed(23)
    return cda.DeviceClipBank([(torch.rand(n, generator=g) - 0.5) * 0.8 for n in LENGTHS], LABELS)


def _seed(s):
    random.seed(s); torch.manual_seed(s); np.random.seed(s)


def _loader(bank, pre, draws, mixup, seed=8):
    return cda.DeviceDataLoader(bank, pre, batch_size=4, audio_augmentor=cda.AudioAugmentor(p_augment=0.5),
                                spec_augmentor=cda.SpecAugment(p=0.5), use_weighted_sampler=False, drop_last=False,
                                draws=draws, generator=torch.Generator().manual_seed(seed), mixup=mixup)


@pytest.mark.parametrize("draws", ["host", "device"])
def test_a_mixing_loader_is_the_plain_loader_followed_by_mix_batch(bank, pre, draws):
    mixing = _loader(bank, pre, draws, cda.MixUp(alpha=0.2))
    _seed(3)
    got = [(f.clone(), y.clone()) for f, y in mixing]
    assert [f.shape[0] for f, _ in got] == [4, 1] == [y.shape[0] for _, y in got]
    # the same loader without mixup under the same seeds; in host mode the mixing draws come after each batch's own
    plain = _loader(bank, pre, draws, None)
    _seed(3)
    it = iter(plain)
    for k, (feats, soft) in enumerate(got):
        x, t = next(it)
        b = x.shape[0]
        if draws == "host":
            perm, lam = torch.randperm(b).numpy(), np.random.beta(0.2, 0.2, size=b)
        else:
            assert plain.last_epoch_seed == mixing.last_epoch_seed
            perm, lam = cdata.mix_draws(mixing.last_epoch_seed + k, b, 0.2)
        want_x, want_y = mix_batch_rows(x.contiguous(), t, torch.from_numpy(perm.astype(np.int32)).cuda(),
                                        torch.from_numpy(mix_coefficients(lam)).cuda())
        assert tuple(feats.shape) == (b, 1, 90, 101) and soft.dtype == torch.float32 and tuple(soft.shape) == (b, 2)
        assert torch.equal(feats, want_x) and torch.equal(soft, want_y), (draws, k)
        assert torch.isfinite(feats).all() and torch.allclose(soft.sum(1), torch.ones(b, device="cuda"), atol=1e-6)
    # a seeded epoch repeats itself
    again = _loader(bank, pre, draws, cda.MixUp(alpha=0.2))
    _seed(3)
    for (f, y), (f2, y2) in zip(got, again):
        assert torch.equal(f, f2) and torch.equal(y, y2)


@pytest.mark.parametrize("draws", ["host", "device"])
def test_fit_runs_on_a_mixing_loader(tmp_path, bank, pre, draws):
    torch.manual_seed(0)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    sd = model.state_dict()
    sd["classifier.4.bias"] = sd["classifier.4.bias"] + torch.tensor([0.0, 1.0])     # leans towards "cough": F1 > 0 from epoch 0
    model.load_state_dict(sd)
    tr = SmallTrainer(model, class_weights=cda.class_weights_from_counts(bank.class_counts), seed=5)
    train = _loader(bank, pre, draws, cda.MixUp(alpha=0.2))
    val = cda.DeviceDataLoader(bank, pre, batch_size=4, is_training=False)
    _seed(3)
    res = cda.fit(tr, train, val, str(tmp_path), epochs=2, patience=5, config=dict(CONFIG))
    print("fit on a mixing loader:", res["history"])
    assert res["epochs_run"] == 2 and [h["epoch"] for h in res["history"]] == [0, 1]
    for h in res["history"]:
        assert h["val"]["tp"] + h["val"]["fp"] + h["val"]["fn"] + h["val"]["tn"] == 5
        assert np.isfinite(h["train"]["loss"]) and np.isfinite(h["val"]["loss"]) and 0 <= h["train"]["accuracy"] <= 100
    assert (tmp_path / "best_model.pt").exists() and (tmp_path / "latest_model.pt").exists()
    ck = torch.load(str(tmp_path / "latest_model.pt"), map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["trainer_state"] == {"seed": 5, "draws": 4}       # 2 training batches per epoch
