"""Waveform augmentation and MixUp on the HIP path (cough_augment_waveforms, cough_mix_rows) against the CPU restatement
of the reference (tests/waveform_aug_ref.py), with the same seeded host draws."""
import random

import numpy as np
import pytest
import torch

from cough_detector_amd import AudioPreprocessor, MixUp, _lib, augmentation, synth
from cough_detector_amd.augmentation import AudioAugmentor, SpecAugment
from oracle import augmentation as oaug, featurizer as ofeat
from parity import FEAT_TOL, SHIPPED, feature_errors
from waveform_aug_ref import AudioAugmentorRef, clip_log, mixup

pytestmark = pytest.mark.gpu

N = 4000
REL = 1e-6


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return ((got - want).abs().max() / want.abs().max().clamp(min=1e-30)).item()


def _bank(kind):
    g = torch.Generator().manual_seed(11)
    return {"none": [], "short+long": [torch.randn((1, 700), generator=g) * 0.3, torch.randn((1, 9000), generator=g)]}[kind]


def _augmentor(p, bank):
    aug = AudioAugmentor(p_augment=p)
    aug.noise_samples = list(bank)
    aug._pack_bank()
    return aug


def _clips(b, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((b, n), generator=g) - 0.5) * torch.linspace(0.2, 1.0, n)


@pytest.mark.parametrize("bank_kind", ["none", "short+long"])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_seeded_parity_with_the_reference(p, bank_kind):
    bank = _bank(bank_kind)
    aug, ref = _augmentor(p, bank), AudioAugmentorRef(p_augment=p, noise_samples=bank)
    x = _clips(6, N)
    seen = {k: set() for k in ("shift", "gain", "gauss", "bank")}
    for seed in range(12):
        # augment, one clip at a time
        random.seed(seed); torch.manual_seed(seed)
        want, logs = [], []
        for b in range(x.shape[0]):
            ref.log = []
            want.append(ref.augment(x[b:b + 1]))
            logs.append({t[0] for t in ref.log})
        random.seed(seed); torch.manual_seed(seed)
        got = [aug.augment(x[b:b + 1].cuda()) for b in range(x.shape[0])]
        for g, w in zip(got, want):
            assert g.shape == w.shape and rel_err(g, w) <= REL
        # augment_batch, the same draws in one launch
        random.seed(seed); torch.manual_seed(seed)
        batch = aug.augment_batch(x.cuda(), noise="host")
        assert rel_err(batch, torch.cat(want)) <= REL
        for names in logs:                                           # per clip: which coins fired
            for k in seen:
                seen[k].add(k in names)
    if p == 0.0:
        assert all(v == {False} for v in seen.values())
    elif p == 1.0:
        assert seen["shift"] == {True} and seen["gain"] == {True} and seen["gauss"] == {True}
        assert seen["bank"] == ({True} if bank else {False})
    else:                                                            # both branches of every coin
        for k in ("shift", "gain", "gauss") + (("bank",) if bank else ()):
            assert seen[k] == {True, False}, k


@pytest.mark.parametrize("bank_kind", ["none", "short+long"])
def test_single_methods_equal_the_reference(bank_kind):
    bank = _bank(bank_kind)
    aug, ref = _augmentor(0.5, bank), AudioAugmentorRef(p_augment=0.5, noise_samples=bank)
    x = _clips(1, N, seed=3)
    for name in ("time_shift", "speed_perturbation", "volume_perturbation", "add_gaussian_noise", "add_noise",
                 "pitch_shift"):
        fired = set()
        for seed in range(12):
            random.seed(seed); torch.manual_seed(seed)
            want = getattr(ref, name)(x)
            after = random.random()
            random.seed(seed); torch.manual_seed(seed)
            got = getattr(aug, name)(x.cuda())
            assert random.random() == after
            assert rel_err(got, want) <= REL, (name, seed)
            fired.add(not torch.equal(want, x))
        if name in ("speed_perturbation", "pitch_shift") or (name == "add_noise" and not bank):
            assert fired == {False}
        else:
            assert fired == {True, False}, name


def test_bank_entries_shorter_and_longer_than_the_clip_wrap_and_crop():
    bank = _bank("short+long")
    aug, ref = _augmentor(1.0, bank), AudioAugmentorRef(p_augment=1.0, noise_samples=bank)
    x = _clips(1, N, seed=4)
    entries = set()
    for seed in range(40):
        random.seed(seed); torch.manual_seed(seed)
        ref.log = []
        want = ref.add_noise(x)
        random.seed(seed)
        got = aug.add_noise(x.cuda())
        assert rel_err(got, want) <= REL
        entries.add(ref.log[0][1])
    assert entries == {0, 1}                                         # the 700-sample (wrapped) and 9000-sample entries


def test_ragged_lengths_equal_single_clip_augments():
    bank = _bank("short+long")
    aug, ref = _augmentor(0.7, bank), AudioAugmentorRef(p_augment=0.7, noise_samples=bank)
    lengths = [N, 1, 2500, 701, N - 3, 16, 3999, 1000]
    x = _clips(len(lengths), N, seed=5)
    for seed in range(4):
        random.seed(seed); torch.manual_seed(seed)
        batch = aug.augment_batch(x.cuda(), lengths=torch.tensor(lengths), noise="host").cpu()
        random.seed(seed); torch.manual_seed(seed)
        singles = [aug.augment(x[b:b + 1, :n].cuda()).cpu() for b, n in enumerate(lengths)]
        random.seed(seed); torch.manual_seed(seed)
        refs = [ref.augment(x[b:b + 1, :n]) for b, n in enumerate(lengths)]
        for b, n in enumerate(lengths):
            assert torch.equal(batch[b, :n], singles[b][0]), (seed, b)
            assert rel_err(batch[b, :n], refs[b][0]) <= REL
            assert torch.all(batch[b, n:] == 0)


def _run(x, clips, gaussian=None, seed=0, lengths=None, bank=()):
    aug = _augmentor(1.0, list(bank))
    return aug._run(x, clips, lengths, gaussian, seed)


def _clip(**kw):
    c = _lib.CoughAugClip(shift=0, gain=1.0, gaussian=0, bank_index=-1, gaussian_snr_db=0.0, bank_snr_db=0.0, bank_start=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_device_noise_is_reproducible_and_meets_the_drawn_snr():
    x = _clips(64, 16000, seed=6).cuda()
    rng = random.Random(1)
    clips = [_clip(shift=rng.randint(-3000, 3000), gain=rng.uniform(0.7, 1.3), gaussian=1,
                   gaussian_snr_db=rng.uniform(10, 30)) for _ in range(64)]
    a = _run(x, clips, seed=123)
    assert torch.equal(a, _run(x, clips, seed=123))                 # bit-identical
    b = _run(x, clips, seed=124)
    assert not torch.equal(a, b)
    assert (a - b).abs().max() > 0 and not torch.isnan(a).any()
    xc = x.cpu()
    for i, c in enumerate(clips):
        y = torch.zeros(16000)
        s = c.shift
        if s >= 0:
            y[s:] = xc[i, :16000 - s]
        else:
            y[:16000 + s] = xc[i, -s:]
        y = y * c.gain
        noise = a[i].cpu().double() - y.double()
        snr = 10 * torch.log10(y.double().pow(2).mean() / noise.pow(2).mean()).item()
        assert abs(snr - c.gaussian_snr_db) < 1e-4, (i, snr, c.gaussian_snr_db)


def test_device_noise_statistics_over_a_full_batch():
    """Clip = 1, gain 1, no shift, 0 dB: out - 1 = z / rms(z) per clip, the generator's output normalised by its clip's
    power.  Its mean, variance, fourth moment (3 for a normal law) and the correlations between clips and between
    neighbouring samples are checked against their sampling error (5 sigma)."""
    b, n = 4096, 16000
    x = torch.ones((b, n), device="cuda")
    z = (_run(x, [_clip(gaussian=1, gaussian_snr_db=0.0)] * b, seed=2026) - 1.0).double()
    m = z.numel()
    assert abs(z.mean().item()) < 5 / m ** 0.5
    assert abs(z.var().item() - 1) < 5 * (2 / m) ** 0.5
    assert abs(z.pow(4).mean().item() - 3) < 5 * (96 / m) ** 0.5
    for i, j in ((0, 1), (1, 2), (17, 4095), (100, 2148)):
        r = (z[i] * z[j]).mean().item()
        assert abs(r) < 5 / n ** 0.5, (i, j, r)
    lag1 = (z[:, 1:] * z[:, :-1]).mean().item()
    assert abs(lag1) < 5 / (b * (n - 1)) ** 0.5
    same_pos = (z[1:, :64] * z[:-1, :64]).mean().item()            # the same sample index in neighbouring clips
    assert abs(same_pos) < 5 / ((b - 1) * 64) ** 0.5


def test_zero_and_non_finite_clips():
    bank = [torch.randn((1, 500)), torch.zeros((1, 300))]
    n = 2000
    zero = torch.zeros((1, n), device="cuda")
    for c in (_clip(shift=300, gain=1.2, gaussian=1, gaussian_snr_db=15.0, bank_index=0, bank_start=100, bank_snr_db=8.0),
              _clip(gaussian=1, gaussian_snr_db=10.0)):
        assert torch.equal(_run(zero, [c], seed=3, bank=bank), zero)
    x = _clips(1, n, seed=7).cuda()
    x[0, 500] = float("nan")
    local = _run(x, [_clip(shift=37, gain=0.8)], bank=bank).cpu()
    assert torch.isnan(local[0, 537]) and torch.isnan(local).sum() == 1
    dropped = _run(x, [_clip(shift=-600)], bank=bank).cpu()        # shifted out of the clip
    assert not torch.isnan(dropped).any()
    for c in (_clip(gaussian=1, gaussian_snr_db=20.0), _clip(shift=5, bank_index=0, bank_start=3, bank_snr_db=10.0)):
        assert torch.isnan(_run(x, [c], seed=1, bank=bank)).all()
    silent = _run(x, [_clip(bank_index=1, bank_start=0, bank_snr_db=10.0)], bank=bank).cpu()   # Pn = 0: nothing added
    assert torch.isnan(silent).sum() == 1
    x[0, 500] = float("inf")
    assert not torch.isfinite(_run(x, [_clip(gaussian=1, gaussian_snr_db=20.0)], seed=1)).any()


@pytest.mark.parametrize("n", [1, 16000, 160000])
def test_clip_lengths(n):
    bank = _bank("short+long")
    aug, ref = _augmentor(1.0, bank), AudioAugmentorRef(p_augment=1.0, noise_samples=bank)
    x = _clips(3, n, seed=8)
    for seed in range(3):
        random.seed(seed); torch.manual_seed(seed)
        want = torch.cat([ref.augment(x[b:b + 1]) for b in range(3)])
        random.seed(seed); torch.manual_seed(seed)
        got = aug.augment_batch(x.cuda(), noise="host")
        assert got.shape == (3, n) and rel_err(got, want) <= REL
    random.seed(9)
    got = aug.augment_batch(x.cuda(), seed=5)                        # device noise (a 10 s clip takes the multi-pass path)
    random.seed(9)
    assert torch.equal(got, aug.augment_batch(x.cuda(), seed=5)) and torch.isfinite(got).all()


class _ScriptedDraws:
    """Stands in for the ``random`` module inside ``waveform_aug_ref`` and replays the draws one ``CoughAugClip`` records
    for a clip of ``n`` samples, so that ``AudioAugmentorRef(p_augment=1).augment`` evaluates exactly that record: the
    coins come in the order of ``augment`` (shift, gain, gauss, bank) and fire where the record has the step."""

    def __init__(self, c, n):
        self.c, self.n = c, n
        self.steps = iter(("shift", "gain", "gauss", "bank"))
        self.step = None

    def random(self):
        self.step = next(self.steps)
        c = self.c
        fired = {"shift": c.shift != 0, "gain": c.gain != 1.0, "gauss": bool(c.gaussian), "bank": c.bank_index >= 0}
        return 0.0 if fired[self.step] else 2.0                     # the coin is `random() > p_augment`: 2 never fires

    def uniform(self, lo, hi):
        c = self.c
        if self.step == "shift":                                    # int(n * u) == shift
            return (c.shift + (0.5 if c.shift > 0 else -0.5)) / self.n
        return {"gain": c.gain, "gauss": c.gaussian_snr_db, "bank": c.bank_snr_db}[self.step]

    def choice(self, seq):
        return self.c.bank_index

    def randint(self, lo, hi):
        assert lo <= self.c.bank_start <= hi
        return self.c.bank_start


def _ref_for_record(monkeypatch, x_row, c, z_row, bank):
    """``waveform_aug_ref``'s ``augment`` of one clip with the record's draws and the given gaussian noise."""
    import waveform_aug_ref
    with monkeypatch.context() as m:
        m.setattr(waveform_aug_ref, "random", _ScriptedDraws(c, x_row.shape[1]))
        m.setattr(torch, "randn_like", lambda w: z_row.clone())
        ref = AudioAugmentorRef(p_augment=1.0, noise_samples=bank)
        out = ref.augment(x_row)
    assert clip_log(c) == [tuple(t) for t in ref.log]                # the restatement took the record's steps, no other
    return out


def test_multi_pass_branch_with_ragged_rows_and_every_combination_of_noise_steps(monkeypatch):
    """n = 16257, the first length past AUG_LDS_MAX: ``augment_kernel<STAGED = false>`` recomputes the clip from the input
    and keeps the intermediate in the output row.  ``test_clip_lengths`` compares that branch with the restatement only
    with every step fired and every row full length; here the rows are ragged (16257, 1, 701, 16256) and every row takes
    gauss only, bank only (the 700-sample entry: wraps), both and neither in turn, with a given ``d_gaussian``."""
    n, lengths = 16257, [16257, 1, 701, 16256]
    bank = _bank("short+long")
    x, z = _clips(4, n, seed=12), torch.randn((4, n), generator=torch.Generator().manual_seed(13))
    for rot in range(4):
        clips = []
        for i, ln in enumerate(lengths):
            kind = (i + rot) % 4                                    # 0 gauss only, 1 bank only, 2 both, 3 neither
            c = _clip(shift=(ln // 9) * (1 if i % 2 else -1), gain=0.75 + 0.1 * kind)
            if kind in (0, 2):
                c.gaussian, c.gaussian_snr_db = 1, 11.0 + i
            if kind in (1, 2):
                rep = 700 if ln <= 700 else (ln // 700 + 1) * 700
                c.bank_index, c.bank_snr_db, c.bank_start = 0, 6.0 + i, min(650, rep - ln)
            clips.append(c)
        got = _run(x.cuda(), clips, gaussian=z.cuda(), lengths=lengths, bank=bank).cpu()
        for i, ln in enumerate(lengths):
            want = _ref_for_record(monkeypatch, x[i:i + 1, :ln], clips[i], z[i:i + 1, :ln], bank)
            assert rel_err(got[i, :ln], want[0]) <= REL, (rot, i)
            assert torch.all(got[i, ln:] == 0)
            if (i + rot) % 4 == 3:                                  # neither: shift and gain only, exact
                assert torch.equal(got[i, :ln], want[0])


def test_strided_rows_equal_contiguous_rows():
    big = _clips(5, 16400, seed=9).cuda()
    view = big[:, 150:150 + 16000]
    assert view.stride(0) == 16400 and not view.is_contiguous()
    clips = [_clip(shift=s, gain=0.9, gaussian=1, gaussian_snr_db=12.0) for s in (0, 5, -7, 1000, -3000)]
    assert torch.equal(_run(view, clips, seed=77), _run(view.contiguous(), clips, seed=77))


def test_mixup_pair_and_batch():
    mix = MixUp(alpha=0.4)
    g = torch.Generator().manual_seed(1)
    x1, x2 = torch.randn((1, 90, 101), generator=g), torch.randn((1, 90, 101), generator=g)
    y1, y2 = torch.tensor([1.0, 0.0]), torch.tensor([0.0, 1.0])
    np.random.seed(3)
    want_x, want_y = mixup(x1, y1, x2, y2, alpha=0.4)
    np.random.seed(3)
    got_x, got_y = mix(x1.cuda(), y1.cuda(), x2.cuda(), y2.cuda())
    assert rel_err(got_x, want_x) <= REL and rel_err(got_y, want_y) <= REL

    b = 64
    x = torch.randn((b, 1, 90, 101), generator=g)
    y = torch.nn.functional.one_hot(torch.randint(0, 2, (b,), generator=g), 2).float()
    perm = torch.randperm(b, generator=g)
    np.random.seed(4)
    xm, ym = mix.mix_batch(x.cuda(), y.cuda(), perm)
    lam = torch.from_numpy(mix.last_lam)
    np.random.seed(4)
    assert np.array_equal(np.random.beta(0.4, 0.4, size=b), mix.last_lam)
    lx = lam.view(b, 1, 1, 1)
    want = lx * x.double() + (1 - lx) * x[perm].double()
    assert rel_err(xm, want) <= REL and len(set(mix.last_lam.tolist())) == b
    assert rel_err(ym, lam.view(b, 1) * y.double() + (1 - lam.view(b, 1)) * y[perm].double()) <= REL
    assert torch.allclose(ym.sum(dim=1).cpu(), torch.ones(b), atol=1e-6)


def test_augment_featurise_spec_augment_chain_equals_the_reference_chain():
    bank = _bank("short+long")
    aug, ref = _augmentor(0.8, bank), AudioAugmentorRef(p_augment=0.8, noise_samples=bank)
    spec = SpecAugment(p=1.0)
    pre = AudioPreprocessor(**SHIPPED, device="cuda")
    x = torch.from_numpy(synth.make_clips(0, 8))
    for seed in range(3):
        random.seed(seed); torch.manual_seed(seed)
        wav = torch.cat([ref.augment(x[b:b + 1]) for b in range(x.shape[0])])
        want = oaug.spec_augment(ofeat.extract_features_batch(wav).unsqueeze(1), 10, 20, 2, 2, 1.0)
        random.seed(seed); torch.manual_seed(seed)
        got = spec(pre.extract_features(aug.augment_batch(x.cuda(), noise="host")).unsqueeze(1))
        mel, rel = feature_errors(got, want)
        assert mel < FEAT_TOL and rel < FEAT_TOL, (seed, mel, rel)
