"""Soft-target training without a GPU: the seventh library's symbols, version and argument checks, the restatement
(tests/soft_ref.py) against ``F.cross_entropy`` with probability targets and autograd, the trainers' and the meter's
refusals, and the mixing loader's draws in both modes with the launches patched out."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cough_detector_amd as cda
import soft_ref
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import data as cdata
from cough_detector_amd import training
from cough_detector_amd.augmentation import mix_coefficients

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_soft.h")
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
LENGTHS = [700, 16000, 1, 16001, 8000]
LABELS = [0, 1, 0, 0, 1]
FAKE = 1 << 20


# ------------------------------------------------------------------------------------------------ the library
def test_soft_library_exports_exactly_its_header():
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|size_t|const char\*) (cough_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert declared == set(_lib.SOFT_SYMBOLS), declared ^ set(_lib.SOFT_SYMBOLS)
    lib = _lib.load_soft()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_soft_abi_version() == 1 and "#define COUGH_SOFT_ABI_VERSION 1" in text
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.SOFT_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == declared, sorted(exported ^ declared)


def test_the_other_six_libraries_are_untouched():
    others = (("SYMBOLS", 53, "load", "cough_amd_abi_version", 5), ("LOOP_SYMBOLS", 3, "load_loop", "cough_loop_abi_version", 1),
              ("DATA_SYMBOLS", 5, "load_data", "cough_data_abi_version", 1),
              ("SEGMENTS_SYMBOLS", 6, "load_segments", "cough_segments_abi_version", 1),
              ("SCORE_SYMBOLS", 5, "load_score", "cough_score_abi_version", 1),
              ("DRAWS_SYMBOLS", 5, "load_draws", "cough_draws_abi_version", 1))
    for names, count, loader, version_fn, version in others:
        syms = getattr(_lib, names)
        assert len(syms) == count and not set(syms) & set(_lib.SOFT_SYMBOLS), names
        lib = getattr(_lib, loader)()
        assert getattr(lib, version_fn)() == version, names
        for s in _lib.SOFT_SYMBOLS:
            assert not hasattr(lib, s), (names, s)
    for header in ("cough_amd.h", "cough_amd_loop.h", "cough_amd_data.h", "cough_amd_segments.h", "cough_amd_score.h",
                   "cough_amd_draws.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        for s in _lib.SOFT_SYMBOLS:
            assert s not in text, (header, s)


@pytest.mark.parametrize("model", ["residual", "small", "standard"])
def test_soft_steps_refuse_bad_arguments_without_a_gpu(model):
    lib, hard = _lib.load_soft(), _lib.load()
    name = {"residual": "cough_train", "small": "cough_train_small", "standard": "cough_train_std"}[model]
    wsb = getattr(hard, name + "_workspace_bytes")(8, 90, 101)
    fn = getattr(lib, name + "_forward_backward_soft")
    ps = (0.1, 0.5) if model == "standard" else (0.5,)

    def fb(x=FAKE, n=8, h=90, w=101, soft=FAKE, p=None, params=FAKE, grads=FAKE, running=FAKE, nbt=FAKE, mom=0.1,
           eps=1e-5, loss=FAKE, logits=FAKE, ws=1 << 24, ws_bytes=wsb):
        pp = ps if p is None else ps[:-1] + (p,)
        return fn(x, n, h, w, soft, None, None, 0, 0, *pp, params, grads, running, nbt, mom, eps, loss, logits, None, ws,
                  ws_bytes, None)

    E = _lib.EINVAL
    for kw in ("x", "soft", "params", "grads", "running", "nbt", "loss", "logits", "ws"):
        assert fb(**{kw: None}) == E, kw
        assert b"NULL" in lib.cough_soft_last_error() and (name + "_forward_backward_soft").encode() in lib.cough_soft_last_error()
    assert fb(n=0) == E and fb(n=-1) == E and fb(h=0) == E and fb(w=-3) == E
    assert fb(h=2) == E and b"too small" in lib.cough_soft_last_error()
    assert fb(p=1.5) == E and fb(p=-0.1) == E and fb(p=float("nan")) == E
    assert b"dropout p" in lib.cough_soft_last_error()
    assert fb(mom=float("nan")) == E and fb(eps=-1.0) == E and fb(ws=(1 << 24) + 8) == E
    assert fb(ws_bytes=wsb - 1) == _lib.EWORKSPACE
    with pytest.raises(ValueError, match=name + "_forward_backward_soft"):
        _lib.check_soft(fb(n=0), name + "_forward_backward_soft")


def test_mix_batch_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_soft()

    def mix(x=FAKE, labels=FAKE, perm=FAKE, coef=FAKE, n=4, row=9090, out=2 * FAKE, soft=3 * FAKE):
        return lib.cough_mix_batch(x, labels, perm, coef, n, row, out, soft, None)

    E = _lib.EINVAL
    for kw in ("x", "labels", "perm", "coef", "out", "soft"):
        assert mix(**{kw: None}) == E, kw
        assert b"NULL" in lib.cough_soft_last_error()
    assert mix(n=0) == E and mix(n=-2) == E and mix(row=0) == E and mix(row=-1) == E
    assert b"bad sizes" in lib.cough_soft_last_error()
    assert mix(out=FAKE) == E and b"alias" in lib.cough_soft_last_error()
    assert mix(x=FAKE + 2) == E and mix(coef=FAKE + 4) == E and mix(labels=FAKE + 4) == E
    assert b"misaligned" in lib.cough_soft_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("cw", [None, [1.0, 2.5]])
def test_restatement_is_torchs_cross_entropy_with_probability_targets(cw):
    g = torch.Generator().manual_seed(5)
    z = (torch.randn(12, 2, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    y = soft_ref.target_rows(12, seed=1).double()
    assert {tuple(r) for r in y.tolist()} >= {(1.0, 0.0), (0.0, 1.0), (0.5, 0.5), (0.0, 0.0)}
    w = None if cw is None else torch.tensor(cw, dtype=torch.float64)
    loss = F.cross_entropy(z, y, weight=w)
    loss.backward()
    rloss, rdz, terms = soft_ref.soft_loss_and_dlogits(z.detach().numpy(), y.numpy(), cw)
    assert abs(rloss - loss.item()) <= 1e-14 * max(1.0, abs(loss.item()))
    np.testing.assert_allclose(rdz, z.grad.numpy(), rtol=0, atol=1e-15)
    assert terms[2] == 0.0 and (rdz[2] == 0.0).all()                      # the all-zero row contributes nothing
    # one-hot rows: the per-clip terms are the class-index terms, but the mean divides by B, not by the summed weights
    t = torch.tensor([0, 1, 1, 0, 1])
    zz, oh = z.detach()[:5], F.one_hot(t, 2).double()
    soft = F.cross_entropy(zz, oh, weight=w).item()
    hard = F.cross_entropy(zz, t, weight=w).item()
    assert abs(soft_ref.hard_loss(zz.numpy(), t.numpy(), cw) - hard) <= 1e-14
    ratio = 1.0 if cw is None else float(np.asarray(cw)[t.numpy()].sum()) / 5
    assert abs(soft - hard * ratio) <= 1e-14 and (cw is None or abs(soft - hard) > 1e-3)
    # a NaN in a row gives a NaN loss
    y_nan = y.clone()
    y_nan[3, 1] = float("nan")
    assert np.isnan(soft_ref.soft_loss_and_dlogits(z.detach().numpy(), y_nan.numpy(), cw)[0])
    assert torch.isnan(F.cross_entropy(z.detach(), y_nan, weight=w))


def test_soft_accuracy_rule_and_mix_restatement():
    y = np.array([[0.5, 0.5], [0.2, 0.8], [1.0, 0.0], [0.0, 0.0], [0.3, 0.3]], dtype=np.float32)
    assert soft_ref.soft_class(y).tolist() == torch.from_numpy(y).argmax(1).tolist() == [0, 1, 0, 0, 0]
    assert training.soft_class(torch.from_numpy(y)).tolist() == [0, 1, 0, 0, 0]
    z = np.array([[1.0, 1.0], [0.0, 2.0], [0.0, 1.0], [3.0, 1.0], [0.0, 0.5]])
    assert soft_ref.accuracy(z, y) == 60.0
    # the mix: torch's float32 `lam * x + (1 - lam) * x[perm]` operator by operator
    g = torch.Generator().manual_seed(2)
    x, labels = torch.randn(5, 7, generator=g), np.array([0, 1, 1, 0, 1])
    perm, lam = np.array([1, 2, 3, 4, 0]), np.random.RandomState(3).beta(0.2, 0.2, size=5)
    coef = mix_coefficients(lam)
    assert coef.dtype == np.float32 and np.array_equal(coef[:, 1], (1.0 - lam).astype(np.float32))
    out, soft = soft_ref.mix_batch(x.numpy(), labels, perm, coef)
    a, c = torch.from_numpy(coef[:, :1]), torch.from_numpy(coef[:, 1:])
    oh = torch.from_numpy(soft_ref.onehot(labels))
    assert torch.equal(torch.from_numpy(out), a * x + c * x[perm]) and torch.equal(torch.from_numpy(soft), a * oh + c * oh[perm])
    bad = perm.copy()
    bad[2] = 5
    out2, soft2 = soft_ref.mix_batch(x.numpy(), labels, bad, coef)
    assert np.array_equal(out2[2], x.numpy()[2]) and soft2[2].tolist() == [0.0, 1.0]
    assert np.array_equal(np.delete(out2, 2, 0), np.delete(out, 2, 0))


# ------------------------------------------------------------------------------------------------ trainers and meter
class _HostTrainer(training.SmallTrainer):
    """``_prepare``'s target checks run before anything touches the device; this stand-in has just enough state."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._shape = (4, 16, 16)


@pytest.mark.parametrize("targets", [torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, 3), torch.zeros(4),
                                     torch.zeros(4, 1), torch.zeros(3, 2), torch.zeros(2, 4), torch.zeros(8),
                                     torch.zeros(4, 2, dtype=torch.complex64), torch.zeros(3, dtype=torch.int64)])
def test_trainers_refuse_other_target_shapes_before_any_launch(targets):
    with pytest.raises(ValueError, match="targets"):
        _HostTrainer()._prepare(torch.zeros(4, 1, 16, 16), targets, None)


def test_trainers_accept_the_two_target_forms():
    tr = _HostTrainer()
    x = torch.zeros(4, 1, 16, 16)
    for t in (torch.tensor([0, 1, 1, 0]), [0, 1, 1, 0], torch.tensor([[0], [1], [1], [0]]), torch.tensor([0, 1, 1, 0], dtype=torch.int32)):
        got = tr._prepare(x, t, None)[1]
        assert got.dtype == torch.int64 and got.tolist() == [0, 1, 1, 0]
    for dtype in (torch.float64, torch.float32, torch.float16):
        y = torch.tensor([[1, 0], [0.25, 0.75], [0, 0], [0.5, 0.5]], dtype=dtype)
        got = tr._prepare(x, y.t().contiguous().t(), None)[1]
        assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, y.float())
    classes = (training.ResidualTrainer, training.SmallTrainer, training.StandardTrainer)
    assert tuple(c._soft_fn for c in classes) == _lib.SOFT_SYMBOLS[2:5] == tuple(c._fb_fn + "_soft" for c in classes)
    for cls in classes:
        assert "not over the summed class weights" in " ".join(cls.__doc__.lower().split())


def test_epoch_meter_refuses_soft_targets_without_a_batch_loss(monkeypatch):
    meter = object.__new__(cda.EpochMeter)
    meter.device = torch.device("cpu")
    z, y = torch.zeros(3, 2), torch.tensor([[1.0, 0.0], [0.5, 0.5], [0.2, 0.8]])
    with pytest.raises(ValueError, match="batch_loss"):
        meter.update(z, y)
    with pytest.raises(ValueError, match="batch_loss"):
        meter.update(z, y, class_weights=torch.ones(2))
    with pytest.raises(ValueError, match="soft targets"):
        meter.update(z, y[:2], batch_loss=torch.zeros(1))


# ------------------------------------------------------------------------------------------------ the mixing loader
def _bank():
    g = torch.Generator().manual_seed(5)
    return cda.DeviceClipBank([torch.randn(n, generator=g) for n in LENGTHS], LABELS, device="cpu")


def _pre():
    return cda.AudioPreprocessor(device="cpu", **SHIPPED)


class _Recorder:
    def __init__(self):
        self.batches = []

    def __call__(self, indices, plan):
        self.batches.append((list(indices), plan))
        return None, None


@pytest.mark.parametrize("augmented", [False, True])
def test_host_mode_draws_the_permutation_then_the_lams_after_the_items(augmented, monkeypatch):
    bank, pre = _bank(), _pre()
    aug = cda.AudioAugmentor(p_augment=1.0) if augmented else None
    spec = cda.SpecAugment(p=1.0) if augmented else None
    loader = cda.DeviceDataLoader(bank, pre, batch_size=4, audio_augmentor=aug, spec_augmentor=spec, use_weighted_sampler=False,
                                  drop_last=False, generator=torch.Generator().manual_seed(1), mixup=cda.MixUp(alpha=0.2))
    rec = _Recorder()
    monkeypatch.setattr(loader, "launch_batch", rec)
    random.seed(4); torch.manual_seed(4); np.random.seed(4)
    assert len(list(loader)) == 2 == len(loader)
    state = (random.getstate(), torch.get_rng_state(), np.random.get_state()[1].copy())
    random.seed(4); torch.manual_seed(4); np.random.seed(4)
    assert [len(idx) for idx, _ in rec.batches] == [4, 1]                  # a batch of 1 mixes with itself
    for indices, plan in rec.batches:
        if augmented:
            for row, idx in enumerate(indices):
                aug.draw_clip(LENGTHS[idx])
                assert not (random.random() > 1.0)
                assert plan.masks[row] == spec.draw_masks(90, 101)
            assert plan.seed == int(torch.randint(0, 2 ** 62, (1,)).item())
        else:
            assert plan.clips is None and plan.masks is None
        b = len(indices)
        assert torch.equal(plan.perm, torch.randperm(b))
        assert np.array_equal(plan.lam, np.random.beta(0.2, 0.2, size=b)) and plan.lam.dtype == np.float64
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])
    assert np.array_equal(np.random.get_state()[1], state[2])
    assert rec.batches[1][1].perm.tolist() == [0]
    # the order is MixUp.mix_batch's own: randperm, then the betas
    torch.manual_seed(9); np.random.seed(9)
    perm, lam = torch.randperm(4), np.random.beta(0.2, 0.2, size=4)
    mix = cda.MixUp(alpha=0.2)
    monkeypatch.setattr("cough_detector_amd.augmentation._mix", lambda x1, x2, lam_, index, who: index)
    torch.manual_seed(9); np.random.seed(9)
    got_perm, _ = mix.mix_batch(torch.zeros(4, 3), torch.zeros(4, 2))
    assert torch.equal(got_perm, perm) and np.array_equal(mix.last_lam, lam)


def test_a_loader_without_mixup_and_a_validation_loader_draw_nothing_more(monkeypatch):
    bank, pre = _bank(), _pre()
    for kw in (dict(), dict(is_training=False, mixup=cda.MixUp())):
        loader = cda.DeviceDataLoader(bank, pre, batch_size=4, use_weighted_sampler=False, **kw)
        rec = _Recorder()
        monkeypatch.setattr(loader, "launch_batch", rec)
        state = (torch.get_rng_state(), np.random.get_state()[1].copy())
        list(loader)
        assert all(pl.perm is None and pl.lam is None for _, pl in rec.batches) and rec.batches
        if kw:
            assert torch.equal(torch.get_rng_state(), state[0])
        assert np.array_equal(np.random.get_state()[1], state[1])
    with pytest.raises(ValueError, match="alpha"):
        cda.DeviceDataLoader(bank, pre, mixup=cda.MixUp(alpha=0.0))
    train, val = cda.create_data_loaders(bank, bank, pre, batch_size=4, mixup=cda.MixUp(0.4))
    assert train.mixup.alpha == 0.4 and train._mixes and val.mixup is None and not val._mixes


def test_device_mode_draws_are_philox_keyed_by_the_batch_seed(monkeypatch):
    for seed, b, alpha in ((0, 1, 0.2), (12345, 4, 0.2), (2 ** 64 - 1, 33, 0.4), (2 ** 64 + 7, 5, 1.0)):
        rng = np.random.Generator(np.random.Philox(key=seed % 2 ** 64))
        want_perm = rng.permutation(b)
        want_lam = rng.beta(alpha, alpha, size=b)
        perm, lam = cdata.mix_draws(seed, b, alpha)
        assert perm.dtype == np.int32 and np.array_equal(perm, want_perm) and sorted(perm.tolist()) == list(range(b))
        assert lam.dtype == np.float64 and np.array_equal(lam, want_lam) and ((lam >= 0) & (lam <= 1)).all()
    assert not np.array_equal(cdata.mix_draws(1, 8, 0.2)[1], cdata.mix_draws(2, 8, 0.2)[1])
    # the words that travel with the upload: padding to 8 bytes, (lam, 1 - lam) as float32, the permutation
    perm, lam = cdata.mix_draws(3, 3, 0.2)
    for before in (3, 4):
        packed = cdata.UploadWords()
        packed.add("lengths", np.arange(before, dtype=np.int32))
        packed.add("coef", mix_coefficients(lam), align8=True)
        packed.add("perm", perm)
        words, at = packed.array(), packed.at("coef")
        assert at % 2 == 0 and at - before == before % 2 and words.dtype == np.int32 and len(words) == at + 9
        assert words[:before].tolist() == list(range(before)) and not words[before:at].any()
        body = words[at:]
        assert np.array_equal(body[:6].view(np.float32).reshape(3, 2), mix_coefficients(lam)) and np.array_equal(body[6:], perm)
        sent = torch.from_numpy(words)                                 # the views the launches get after the upload
        assert np.array_equal(packed.view(sent, "coef").numpy(), mix_coefficients(lam))
        assert np.array_equal(packed.view(sent, "perm").numpy(), perm) and "coef" in packed and "warp" not in packed
    # batch k of an epoch is drawn under (epoch_seed + k) mod 2^64, with or without other draws
    bank, pre = _bank(), _pre()
    loader = cda.DeviceDataLoader(bank, pre, batch_size=4, use_weighted_sampler=False, drop_last=False, draws="device",
                                  generator=torch.Generator().manual_seed(1), mixup=cda.MixUp())
    seen = []
    monkeypatch.setattr(loader, "launch_batch_drawn", lambda indices, seed: seen.append((len(indices), seed)) or (None, None))
    list(loader)
    assert seen == [(4, loader.last_epoch_seed), (1, loader.last_epoch_seed + 1)]
    want = int(torch.randint(0, 2 ** 62, (1,), generator=_after_indices(5, 1)).item())
    assert loader.last_epoch_seed == want


def _after_indices(n, seed):
    """A generator in the state the loader's is in after an unweighted epoch's indices."""
    g = torch.Generator().manual_seed(seed)
    list(torch.utils.data.RandomSampler(range(n), generator=g))
    return g
