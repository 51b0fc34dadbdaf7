"""The device-resident dataset and batch loader without a GPU: the third library's symbols and argument checks, the
bank's bookkeeping, and the loader's host side -- index order against torch's own samplers, ``__len__``, and the per-item
draw order against the restatements (tests/waveform_aug_ref.py, oracle/augmentation.py) with the launches patched out."""
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch.utils.data import RandomSampler, WeightedRandomSampler

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import data as cdata
from oracle import augmentation as oaug
from waveform_aug_ref import AudioAugmentorRef, clip_log

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_data.h")
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
LENGTHS = [1, 2, 15999, 16000, 16001, 16002, 40001, 700, 8000, 24000, 31, 12345]
LABELS = [0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def _bank(lengths=LENGTHS, labels=LABELS):
    g = torch.Generator().manual_seed(5)
    return cda.DeviceClipBank([torch.randn(n, generator=g) for n in lengths], labels, device="cpu")


# ------------------------------------------------------------------------------------------------ the library
def test_data_library_exports_exactly_its_header():
    declared = set(re.findall(r"\b(cough_[a-z_0-9]+)\s*\(", open(HEADER).read()))
    assert declared == set(_lib.DATA_SYMBOLS), declared ^ set(_lib.DATA_SYMBOLS)
    lib = _lib.load_data()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_data_abi_version() == 1
    assert "#define COUGH_DATA_ABI_VERSION 1" in open(HEADER).read()
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.DATA_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert exported == declared, sorted(exported ^ declared)


def test_the_other_libraries_are_untouched():
    assert not set(_lib.DATA_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.LOOP_SYMBOLS))
    assert len(_lib.SYMBOLS) == 53 and _lib.load().cough_amd_abi_version() == 5
    assert len(_lib.LOOP_SYMBOLS) == 3 and _lib.load_loop().cough_loop_abi_version() == 1
    for header in ("cough_amd.h", "cough_amd_loop.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        for s in _lib.DATA_SYMBOLS:
            assert s not in text, (header, s)


FAKE = 1 << 20


def _err():
    return _lib.load_data().cough_data_last_error()


def test_gather_rows_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_data()

    def call(src=FAKE, offs=FAKE, lens=FAKE, n=4, out=FAKE, stride=100, row_len=100):
        return lib.cough_gather_rows(src, offs, lens, n, out, stride, row_len, None)

    E = _lib.EINVAL
    for kw in ("src", "offs", "lens", "out"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_gather_rows" in _err(), kw
    assert call(n=-1) == E and b"n_rows" in _err()
    assert call(n=-2 ** 31) == E
    for v in (0, -1):
        assert call(row_len=v, stride=200) == E and b"row_len" in _err(), v
    assert call(stride=99) == E and b"out_stride" in _err()
    for kw in ("src", "out", "lens"):
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err(), kw
    assert call(offs=FAKE + 4) == E and b"8-byte" in _err()
    assert call(n=0) == _lib.OK                                            # nothing to do: no launch
    with pytest.raises(ValueError, match="cough_gather_rows: .*row_len"):
        _lib.check_data(call(row_len=0), "cough_gather_rows")
    assert b"row_len" not in _lib.load().cough_amd_last_error()            # the libraries keep their messages apart


def test_prepare_rows_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_data()

    def call(src=FAKE, offs=FAKE, lens=FAKE, n=4, out=FAKE, out_len=16000, flags=1):
        return lib.cough_prepare_rows(src, offs, lens, n, out, out_len, flags, None)

    E = _lib.EINVAL
    for kw in ("src", "offs", "lens", "out"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_prepare_rows" in _err(), kw
    assert call(n=-1) == E and b"n_rows" in _err()
    for v in (0, -5):
        assert call(out_len=v) == E and b"out_len" in _err(), v
    assert call(flags=2) == E and b"flags" in _err()
    for kw in ("src", "out", "lens"):
        assert call(**{kw: FAKE + 1}) == E and b"4-byte" in _err(), kw
    assert call(offs=FAKE + 4) == E and b"8-byte" in _err()
    assert call(n=0) == _lib.OK and call(n=0, flags=0) == _lib.OK


def test_mask_images_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_data()

    def call(src=FAKE, out=FAKE, n=3, h=90, w=101, n_masks=4, axis=FAKE, start=FAKE, end=FAKE):
        return lib.cough_mask_images(src, out, n, h, w, n_masks, axis, start, end, None)

    E = _lib.EINVAL
    for kw in ("src", "out", "axis", "start", "end"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_mask_images" in _err(), kw
    for v in (-1, 17, 1 << 20):
        assert call(n_masks=v) == E and b"n_masks" in _err(), v
    assert call(n=-1) == E and b"n_images" in _err()
    for kw in ("h", "w"):
        for v in (0, -3):
            assert call(**{kw: v}) == E and b"bad shape" in _err(), (kw, v)
    assert call(h=1 << 16, w=1 << 16) == _lib.EUNSUPPORTED
    for kw in ("src", "out", "axis", "start", "end"):
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err(), kw
    assert call(n=0) == _lib.OK
    assert call(n=0, n_masks=0, axis=None, start=None, end=None) == _lib.OK
    assert call(n=0, n_masks=16) == _lib.OK


def test_the_package_exports_the_loader():
    for name in ("DeviceClipBank", "DeviceDataLoader", "create_data_loaders"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cdata, name), name
    assert hasattr(cda.SpecAugment, "mask_batch")


# ------------------------------------------------------------------------------------------------ the bank
def test_bank_bookkeeping_and_weights():
    bank = _bank()
    assert len(bank) == 12 and bank.class_counts == {0: 9, 1: 3}
    assert bank.lengths.dtype == torch.int32 and bank.lengths.tolist() == LENGTHS
    assert bank.offsets.dtype == torch.int64 and bank.offsets.tolist() == [sum(LENGTHS[:k]) for k in range(12)]
    assert bank.labels.dtype == torch.int64 and bank.labels.tolist() == LABELS
    assert bank.data.numel() == sum(LENGTHS) and bank.data.dtype == torch.float32
    for dev, host in ((bank.offsets_dev, bank.offsets), (bank.lengths_dev, bank.lengths), (bank.labels_dev, bank.labels)):
        assert torch.equal(dev.cpu(), host) and dev.dtype == host.dtype
    w = bank.sample_weights
    assert w.dtype == torch.float32 and w.tolist() == torch.tensor([12 / (2 * {0: 9, 1: 3}[v]) for v in LABELS]).tolist()
    g = torch.Generator().manual_seed(5)
    clips = [torch.randn(n, generator=g) for n in LENGTHS]
    for k in (0, 3, 6, 11):
        assert torch.equal(bank.clip(k), clips[k].unsqueeze(0))
    sub = bank.subset([6, 0, 4])
    assert len(sub) == 3 and sub.lengths.tolist() == [40001, 1, 16001] and sub.labels.tolist() == [0, 0, 1]
    assert sub.offsets.tolist() == [0, 40001, 40002] and sub.class_counts == {0: 2, 1: 1}
    assert torch.equal(sub.clip(2), clips[4].unsqueeze(0)) and torch.equal(sub.clip(1), clips[0].unsqueeze(0))
    with pytest.raises(IndexError):
        bank.subset([12])
    # (1, n) clips and a label tensor are taken too; what is not a mono float clip is refused
    two = cda.DeviceClipBank([clips[1].unsqueeze(0), clips[2].double()], torch.tensor([1, 0]), device="cpu")
    assert two.lengths.tolist() == [2, 15999] and torch.equal(two.clip(1), clips[2].unsqueeze(0))
    for bad, exc in (([torch.zeros(0)], ValueError), ([torch.zeros(2, 5)], ValueError),
                     ([torch.zeros(4, dtype=torch.int16)], TypeError)):
        with pytest.raises(exc):
            cda.DeviceClipBank(bad, [0], device="cpu")
    with pytest.raises(ValueError):
        cda.DeviceClipBank([clips[0]], [2], device="cpu")
    with pytest.raises(ValueError):
        cda.DeviceClipBank([clips[0]], [0, 1], device="cpu")


def test_from_directory_follows_the_reference_order(tmp_path, monkeypatch):
    import numpy as np
    from scipy.io import wavfile
    g = torch.Generator().manual_seed(9)
    want = {}
    for cls, names in (("cough", ["b.wav", "a.WAV", "c.mp3"]), ("non_cough", ["z.wav", "notes.txt", "y.flac", "x.ogg"])):
        (tmp_path / cls).mkdir()
        for name in names:
            if name.lower().endswith(".wav"):
                x = (torch.randn(int(torch.randint(50, 400, (1,), generator=g)), generator=g) * 0.2).numpy().astype(np.float32)
                wavfile.write(str(tmp_path / cls / name), 16000, x)
                want[(cls, name)] = torch.from_numpy(x)
            else:
                (tmp_path / cls / name).write_bytes(b"not audio")
    pre = cda.AudioPreprocessor(**SHIPPED)
    with pytest.warns(UserWarning, match=r"skipped 3 audio file\(s\)") as rec:
        bank = cda.DeviceClipBank.from_directory(str(tmp_path), pre, device="cpu")
    assert len([w for w in rec if "skipped" in str(w.message)]) == 1
    order = [("non_cough", p.name) for p in (tmp_path / "non_cough").iterdir() if p.suffix.lower() == ".wav"]
    order += [("cough", p.name) for p in (tmp_path / "cough").iterdir() if p.suffix.lower() == ".wav"]
    assert len(bank) == 3 and bank.labels.tolist() == [0, 1, 1] and bank.class_counts == {0: 1, 1: 2}
    for k, key in enumerate(order):
        assert torch.equal(bank.clip(k)[0], want[key]), key
    with pytest.warns(UserWarning, match="not found"):
        (tmp_path / "only").mkdir()
        assert len(cda.DeviceClipBank.from_directory(str(tmp_path / "only"), pre, device="cpu")) == 0


# ------------------------------------------------------------------------------------------------ the loader's host side
def _pre():
    return cda.AudioPreprocessor(**SHIPPED)


@pytest.mark.parametrize("seed", [0, 7])
def test_index_order_is_that_of_torchs_samplers(seed):
    bank, pre = _bank(), _pre()
    gen = lambda: torch.Generator().manual_seed(seed)      # noqa: E731
    weighted = cda.DeviceDataLoader(bank, pre, batch_size=4, generator=gen())
    want = list(WeightedRandomSampler(bank.sample_weights, len(bank), True, generator=gen()))
    assert weighted.epoch_indices() == want and len(want) == 12
    shuffled = cda.DeviceDataLoader(bank, pre, batch_size=4, use_weighted_sampler=False, generator=gen())
    want = list(RandomSampler(range(12), generator=gen()))
    assert shuffled.epoch_indices() == want and sorted(want) == list(range(12))
    # a second epoch continues the generator, as a DataLoader's sampler does
    g2 = gen()
    list(RandomSampler(range(12), generator=g2))
    assert shuffled.epoch_indices() == list(RandomSampler(range(12), generator=g2))
    for kw in (dict(), dict(use_weighted_sampler=False)):
        val = cda.DeviceDataLoader(bank, pre, batch_size=4, is_training=False, generator=gen(), **kw)
        assert val.epoch_indices() == list(range(12))


def test_len_follows_the_drop_last_rule():
    bank, pre = _bank(), _pre()
    for bs, dropped, kept in ((4, 3, 3), (5, 2, 3), (12, 1, 1), (13, 0, 1), (32, 0, 1), (1, 12, 12)):
        assert len(cda.DeviceDataLoader(bank, pre, batch_size=bs)) == dropped, bs                       # training: drop_last
        assert len(cda.DeviceDataLoader(bank, pre, batch_size=bs, is_training=False)) == kept, bs
        assert len(cda.DeviceDataLoader(bank, pre, batch_size=bs, drop_last=False)) == kept, bs
        assert len(cda.DeviceDataLoader(bank, pre, batch_size=bs, is_training=False, drop_last=True)) == dropped, bs
    with pytest.raises(ValueError):
        cda.DeviceDataLoader(bank, pre, batch_size=0)
    with pytest.raises(ValueError):
        cda.DeviceDataLoader(bank, pre, noise="cpu")


class _Recorder:
    """Stands in for ``launch_batch``: keeps the indices and the plan of every batch, launches nothing."""

    def __init__(self):
        self.batches = []

    def __call__(self, indices, plan):
        self.batches.append((list(indices), plan))
        return None, None


def _noise_bank():
    g = torch.Generator().manual_seed(11)
    return [torch.randn((1, 700), generator=g) * 0.3, torch.randn((1, 9000), generator=g)]


@pytest.mark.parametrize("p", [1.0, 0.5])
@pytest.mark.parametrize("with_bank", [False, True])
def test_per_item_draw_order_is_the_references(p, with_bank, monkeypatch):
    bank, pre = _bank(), _pre()
    noise = _noise_bank() if with_bank else []
    aug = cda.AudioAugmentor(p_augment=p)
    aug.noise_samples = list(noise)
    aug._pack_bank()
    spec = cda.SpecAugment(p=p)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=4, audio_augmentor=aug, spec_augmentor=spec, noise="host",
                                  generator=torch.Generator().manual_seed(3))
    f, t = loader.feature_shape()
    assert (f, t) == (90, 101)
    rec = _Recorder()
    monkeypatch.setattr(loader, "launch_batch", rec)
    for seed in (0, 1, 2):
        rec.batches.clear()
        random.seed(seed); torch.manual_seed(seed)
        it = iter(loader)
        next(it)                                                           # one batch: nothing is drawn ahead
        state = (random.getstate(), torch.get_rng_state())
        (indices, plan), = rec.batches
        assert len(indices) == 4 and plan.seed == 0 and tuple(plan.gaussian.shape) == (4, max(LENGTHS[i] for i in indices))
        # the same draws, item by item, by the restatements
        random.seed(seed); torch.manual_seed(seed)
        ref = AudioAugmentorRef(p_augment=p, noise_samples=noise)
        for row, idx in enumerate(indices):
            n = LENGTHS[idx]
            ref.log.clear()
            gauss = []
            orig = torch.randn_like
            monkeypatch.setattr(torch, "randn_like", lambda x, **kw: gauss.append(orig(x, **kw)) or gauss[-1])
            ref.augment(torch.zeros(1, n))
            monkeypatch.setattr(torch, "randn_like", orig)
            # the struct holds the gain as float32, as the kernel uses it
            want = [(t[0], float(np.float32(t[1]))) if t[0] == "gain" else t for t in ref.log]
            assert clip_log(plan.clips[row]) == want, (seed, row)
            if plan.clips[row].gaussian:
                assert len(gauss) == 1 and torch.equal(plan.gaussian[row, :n], gauss[0][0])
            else:
                assert not gauss and not plan.gaussian[row].any()
            assert not plan.gaussian[row, n:].any()
            masks = []
            if not (random.random() > p):
                masks = [(0,) + oaug.draw_mask(10, f) for _ in range(2)] + [(1,) + oaug.draw_mask(20, t) for _ in range(2)]
            assert plan.masks[row] == masks, (seed, row)
        assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])
    if p == 0.5:
        fired = [bool(m) for _, pl in rec.batches for m in pl.masks]
        assert len(fired) == 4


def test_device_noise_draws_one_seed_per_batch_and_validation_draws_nothing(monkeypatch):
    bank, pre = _bank(), _pre()
    aug, spec = cda.AudioAugmentor(p_augment=1.0), cda.SpecAugment(p=1.0)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=4, audio_augmentor=aug, spec_augmentor=spec,
                                  use_weighted_sampler=False, generator=torch.Generator().manual_seed(1))
    rec = _Recorder()
    monkeypatch.setattr(loader, "launch_batch", rec)
    random.seed(4); torch.manual_seed(4)
    assert len(list(loader)) == 3
    random.seed(4); torch.manual_seed(4)
    seeds = []
    for indices, plan in rec.batches:
        assert plan.gaussian is None
        for row, idx in enumerate(indices):
            aug.draw_clip(LENGTHS[idx])
            assert not (random.random() > 1.0)
            assert plan.masks[row] == spec.draw_masks(90, 101)
        seeds.append(int(torch.randint(0, 2 ** 62, (1,)).item()))
        assert plan.seed == seeds[-1]
    assert len(set(seeds)) == 3
    assert sorted(i for idx, _ in rec.batches for i in idx) == list(range(12))
    # a validation loader ignores the augmentors and leaves both generators alone
    val = cda.DeviceDataLoader(bank, pre, batch_size=5, audio_augmentor=aug, spec_augmentor=spec, is_training=False)
    rec2 = _Recorder()
    monkeypatch.setattr(val, "launch_batch", rec2)
    state = (random.getstate(), torch.get_rng_state())
    assert len(list(val)) == 3
    assert [idx for idx, _ in rec2.batches] == [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11]]
    assert all(pl.clips is None and pl.masks is None and pl.gaussian is None for _, pl in rec2.batches)
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])


def test_cache_features_with_an_active_augmentor_raises():
    bank, pre = _bank(), _pre()
    aug, spec = cda.AudioAugmentor(p_augment=0.5), cda.SpecAugment()
    with pytest.raises(ValueError, match="cache_features"):
        cda.DeviceDataLoader(bank, pre, audio_augmentor=aug, cache_features=True)
    with pytest.raises(ValueError, match="cache_features"):
        cda.create_data_loaders(bank, bank, pre, audio_augmentor=aug, cache_features=True)
    # allowed where no waveform augmentation can run: SpecAugment only, or a validation loader
    assert cda.DeviceDataLoader(bank, pre, spec_augmentor=spec, cache_features=True).cache_features
    assert cda.DeviceDataLoader(bank, pre, audio_augmentor=aug, is_training=False, cache_features=True).cache_features


def test_create_data_loaders_mirrors_the_reference():
    bank, pre = _bank(), _pre()
    aug, spec = cda.AudioAugmentor(p_augment=0.5), cda.SpecAugment()
    gen = torch.Generator().manual_seed(2)
    train, val = cda.create_data_loaders(bank, bank.subset([0, 1, 2, 3, 4]), pre, batch_size=4, audio_augmentor=aug,
                                         spec_augmentor=spec, generator=gen, noise="host")
    assert train.is_training and train.drop_last and train.use_weighted_sampler and train.noise == "host"
    assert train.audio_augmentor is aug and train.spec_augmentor is spec and train.generator is gen and len(train) == 3
    assert not val.is_training and not val.drop_last and val.audio_augmentor is None and val.spec_augmentor is None
    assert len(val) == 2 and val.epoch_indices() == [0, 1, 2, 3, 4]
    train2, _ = cda.create_data_loaders(bank, bank, pre, use_weighted_sampler=False)
    assert not train2.use_weighted_sampler and train2.batch_size == 32 and len(train2) == 0


def test_a_bank_off_the_gpu_cannot_launch():
    loader = cda.DeviceDataLoader(_bank(), _pre(), batch_size=4, is_training=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(loader))
