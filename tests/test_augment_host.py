"""Waveform augmentation without a GPU: the C-ABI struct and argument checks, the host draw sequence of
``AudioAugmentor.augment_batch`` against the CPU restatement (tests/waveform_aug_ref.py), and the packing of the noise bank."""
import ctypes
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib, augmentation
from oracle import featurizer as ofeat
from waveform_aug_ref import AudioAugmentorRef, clip_log


def _clip(shift=0, gain=1.0, gaussian=0, bank_index=-1, bank_start=0):
    return _lib.CoughAugClip(shift=shift, gain=gain, gaussian=gaussian, bank_index=bank_index, gaussian_snr_db=20.0,
                             bank_snr_db=10.0, bank_start=bank_start)


def test_aug_clip_struct_matches_the_header():
    # int shift; float gain; int gaussian; int bank_index; double gaussian_snr_db; double bank_snr_db; long long bank_start
    assert ctypes.sizeof(_lib.CoughAugClip) == 40
    assert _lib.CoughAugClip.gaussian_snr_db.offset == 16 and _lib.CoughAugClip.bank_start.offset == 32
    assert "cough_augment_waveforms" in _lib.SYMBOLS and "cough_mix_rows" in _lib.SYMBOLS


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    fake = 1 << 20                                         # never dereferenced: every call below fails its checks first
    ws = 1 << 24
    wsb = lib.cough_augment_workspace_bytes(4)
    assert wsb >= 4 * 40 and wsb % 256 == 0 and lib.cough_augment_workspace_bytes(0) == 0

    def aug(clips, n=100, lengths=None, n_clips=None, stride=100, d_in=fake, d_out=fake + 4096, bank=None, ws_bytes=wsb,
            workspace=ws):
        arr = (_lib.CoughAugClip * len(clips))(*clips)
        lens = (ctypes.c_int * len(lengths))(*lengths) if lengths is not None else None
        offs, blen, nb, numel = None, None, 0, 0
        if bank is not None:
            offs = (ctypes.c_longlong * len(bank))(*[o for o, _ in bank])
            blen = (ctypes.c_int * len(bank))(*[l for _, l in bank])
            nb, numel = len(bank), sum(l for _, l in bank)
        return lib.cough_augment_waveforms(d_in, stride, d_out, len(clips) if n_clips is None else n_clips, n, lens, arr,
                                           fake if bank is not None else None, numel, offs, blen, nb, None, 7, workspace,
                                           ws_bytes, None)

    E = _lib.EINVAL
    assert aug([_clip()], d_in=None) == E and b"NULL" in lib.cough_amd_last_error()
    assert aug([_clip()], d_out=None) == E
    assert aug([_clip()], d_out=fake) == E                                   # aliasing
    assert aug([_clip()], n_clips=-1) == E
    assert aug([_clip()], n=0) == E
    assert aug([_clip()], stride=99) == E                                    # stride < n_samples
    assert aug([_clip(shift=100)]) == E and b"shift" in lib.cough_amd_last_error()
    assert aug([_clip(shift=-100)]) == E
    assert aug([_clip(shift=40)], lengths=[40]) == E                         # shift >= its own length
    assert aug([_clip()], lengths=[101]) == E and b"lengths" in lib.cough_amd_last_error()
    assert aug([_clip()], lengths=[0]) == E
    assert aug([_clip(gaussian=2)]) == E
    assert aug([_clip(bank_index=0)]) == E and b"bank_index" in lib.cough_amd_last_error()   # no bank
    assert aug([_clip(bank_index=1)], bank=[(0, 50)]) == E
    assert aug([_clip(bank_index=-2)], bank=[(0, 50)]) == E
    # entry of 50 samples, clip of 100: repeated to 150, so the crop start is 0..50
    assert aug([_clip(bank_index=0, bank_start=51)], bank=[(0, 50)]) == E and b"bank_start" in lib.cough_amd_last_error()
    assert aug([_clip(bank_index=0, bank_start=-1)], bank=[(0, 50)]) == E
    assert aug([_clip()], bank=[(0, 0)]) == E                                # empty entry
    assert aug([_clip()], ws_bytes=wsb - 1) == _lib.EWORKSPACE
    assert aug([_clip()], workspace=ws + 8) == _lib.EWORKSPACE                # misaligned
    assert aug([], n_clips=0) == _lib.OK                                     # nothing to do, nothing launched
    with pytest.raises(ValueError, match="shift"):
        _lib.check(aug([_clip(shift=100)]), "cough_augment_waveforms")

    assert lib.cough_mix_rows(None, fake, None, fake, 4, 10, fake, None) == E
    assert lib.cough_mix_rows(fake, fake, None, fake, 4, 10, None, None) == E
    assert lib.cough_mix_rows(fake, fake, None, fake, -1, 10, fake, None) == E
    assert lib.cough_mix_rows(fake, fake, None, fake, 4, -10, fake, None) == E
    assert lib.cough_mix_rows(None, None, None, None, 0, 10, None, None) == _lib.OK


def _bank(lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((1, n), generator=g) for n in lengths]


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("bank_lengths", [[], [700, 3000, 1200]])
def test_augment_batch_draws_what_the_reference_draws(p, bank_lengths):
    lengths = [1000, 1000, 640, 1000, 17, 1000, 999, 1]
    noise = _bank(bank_lengths)
    aug = augmentation.AudioAugmentor(p_augment=p)
    aug.noise_samples = list(noise)
    aug._pack_bank()
    fired = set()
    for seed in range(12):
        ref = AudioAugmentorRef(p_augment=p, noise_samples=noise)
        random.seed(seed); torch.manual_seed(seed)
        want = []
        for n in lengths:
            ref.log = []
            ref.augment(torch.rand((1, n)) - 0.5)
            want.append(ref.log)
        after_ref = random.random()
        random.seed(seed)
        got = [clip_log(c) for c in aug.draw_batch(lengths)]
        assert random.random() == after_ref                     # the same number of draws, in the same order
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert [t[0] for t in g] == [t[0] for t in w]
            for tg, tw in zip(g, w):
                if tg[0] == "gain":                              # the struct holds the gain as float32, as the kernel uses it
                    assert tg[1] == float(np.float32(tw[1]))
                else:
                    assert tg == tw
            fired.update(t[0] for t in g)
    if p == 0.0:
        assert not fired
    else:
        assert fired == ({"shift", "gain", "gauss", "bank"} if bank_lengths else {"shift", "gain", "gauss"})


def test_single_method_draws_without_a_bank_and_pitch_shift_is_the_identity():
    aug = augmentation.AudioAugmentor(p_augment=1.0)
    ref = AudioAugmentorRef(p_augment=1.0)
    x = torch.rand((1, 64))
    random.seed(5)
    assert aug.add_noise(x) is x                               # empty bank: the coin is drawn, nothing else
    assert aug.pitch_shift(x) is x
    assert aug.speed_perturbation(x) is x
    after = random.random()
    random.seed(5)
    ref.add_noise(x); ref.pitch_shift(x)
    assert random.random() == after
    assert augmentation.AudioAugmentor(p_augment=0.0).augment(x) is x


def test_noise_bank_is_packed_from_a_directory(tmp_path, monkeypatch):
    from scipy.io import wavfile
    rng = np.random.default_rng(2)
    a = rng.uniform(-0.5, 0.5, 3000).astype(np.float32)                      # mono, 16 kHz
    b = rng.uniform(-0.5, 0.5, (2205, 2)).astype(np.float32)                 # stereo, 22.05 kHz
    c = (rng.uniform(-0.5, 0.5, (800, 2)) * 32767).astype(np.int16)          # stereo int16, 16 kHz
    wavfile.write(str(tmp_path / "a.wav"), 16000, a)
    wavfile.write(str(tmp_path / "b.wav"), 22050, b)
    wavfile.write(str(tmp_path / "c.wav"), 16000, c)
    (tmp_path / "d.flac").write_bytes(b"fLaC not decodable here")         # skipped like an undecodable file
    (tmp_path / "notes.txt").write_text("not audio")                       # not globbed
    # the resampler is the GPU's cough_resample; on a CPU box the restatement of T.Resample stands in for it
    calls = []

    def cpu_resample(self, w, sr):
        calls.append(sr)
        return ofeat.resample(w, sr, self.sample_rate)
    monkeypatch.setattr(augmentation.AudioAugmentor, "_resample", cpu_resample)
    aug = cda.AudioAugmentor(sample_rate=16000, noise_dir=str(tmp_path), p_augment=0.5)
    order = list(tmp_path.glob("*.wav"))                                      # the reference's glob order
    want = {"a.wav": torch.from_numpy(a)[None],
            "b.wav": ofeat.resample(torch.from_numpy(np.ascontiguousarray(b.T)), 22050, 16000).mean(dim=0, keepdim=True),
            "c.wav": (torch.from_numpy(np.ascontiguousarray(c.T)).float() / 32768.0).mean(dim=0, keepdim=True)}
    assert calls == [22050]
    assert len(aug.noise_samples) == 3
    offset = 0
    for k, path in enumerate(order):
        w = want[path.name]
        assert torch.equal(aug.noise_samples[k], w)
        assert aug._bank_offsets[k] == offset and aug._bank_lengths[k] == w.shape[1]
        assert torch.equal(aug._bank_host[offset:offset + w.shape[1]], w[0])
        offset += w.shape[1]
    assert aug._bank_host.numel() == offset and aug._bank_lengths[order.index(tmp_path / "b.wav")] == 1600
    # max_samples keeps the first files of the glob order
    aug2 = augmentation.AudioAugmentor(sample_rate=16000, p_augment=0.5)
    aug2._load_noise_samples(str(tmp_path), max_samples=1)
    assert len(aug2.noise_samples) == 1 and torch.equal(aug2.noise_samples[0], want[order[0].name])
    assert augmentation.AudioAugmentor(noise_dir=str(tmp_path / "missing")).noise_samples == []


def test_pipeline_factory_and_exports():
    audio, spec = cda.create_augmentation_pipeline(sample_rate=16000, p_augment=0.3)
    assert isinstance(audio, cda.AudioAugmentor) and audio.p_augment == 0.3 and audio.sample_rate == 16000
    assert isinstance(spec, augmentation.SpecAugment) and spec.p == 0.3
    assert cda.create_augmentation_pipeline(use_spec_augment=False)[1] is None
    assert cda.MixUp().alpha == 0.2 and cda.MixUp(0.4).alpha == 0.4
    with pytest.raises(ValueError):
        cda.MixUp().mix_batch(torch.zeros(3, 4), torch.zeros(3, 2), perm=torch.tensor([0, 1, 3]))
    with pytest.raises(ValueError):
        augmentation.AudioAugmentor().augment_batch(torch.zeros(2, 8), noise="cpu")
    with pytest.raises(ValueError):
        augmentation.AudioAugmentor().augment_batch(torch.zeros(2, 8), lengths=[8, 9])
