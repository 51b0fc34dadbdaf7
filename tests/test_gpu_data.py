"""The device-resident dataset and batch loader on the MI355X (cough_detector_amd/data.py, csrc/data.hip).

Everything here is compared bit for bit (``torch.equal``).  ``cough_gather_rows`` and ``cough_mask_images`` move or zero
float32 values; ``cough_prepare_rows`` takes a maximum (exact in any order) and performs one IEEE division per sample,
which is what ``torch``'s ``waveform / waveform.abs().max()`` does on the CPU.  The loader strings per-clip computations
together -- the augment kernel reduces over a clip's own samples in an order fixed by the clip's length, the featuriser
works clip by clip -- so a batch equals its items run one at a time through the public per-clip path with the same
seeds.
"""
import random

import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd.augmentation import mask_images
from cough_detector_amd.training import SmallTrainer
from oracle import augmentation as oaug
from oracle import featurizer as ofeat

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
CONFIG = dict(model_type="small", sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400, f_min=100.0,
              f_max=4000.0, segment_duration=1.0, n_mfcc=13, use_mfcc=True, pre_emphasis_coef=0.97, n_contrast_bands=6,
              **SHIPPED)
LONG = [1, 2, 15999, 16000, 16001, 16002, 40001]
LENGTHS = LONG + [700, 8000, 24000, 31, 12345]
LABELS = [0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 0, 1]
JUNK = 7.0e4            # what lies between the rows of a packed buffer: a kernel that reads past a row shows it


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rows(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * 0.8 for n in lengths]


def _pack(rows, first=1):
    """Rows end to end with one junk element between them, the first at element ``first``: rows start on every phase of
    16 bytes.  -> (device buffer, device int64 offsets, device int32 lengths, host offsets)"""
    parts, offsets, pos = [torch.full((first,), JUNK)], [], first
    for r in rows:
        offsets.append(pos)
        parts += [r, torch.full((1,), JUNK)]
        pos += r.numel() + 1
    return (torch.cat(parts).cuda(), torch.tensor(offsets, dtype=torch.int64).cuda(),
            torch.tensor([r.numel() for r in rows], dtype=torch.int32).cuda(), offsets)


def _prepare(data, offs, lens, n, out_len, flags=1, misalign=0):
    buf = torch.full((n * out_len + misalign + 1,), JUNK, device="cuda")
    out = buf[misalign:misalign + n * out_len]
    _lib.check_data(_lib.load_data().cough_prepare_rows(data.data_ptr(), offs.data_ptr(), lens.data_ptr(), n,
                                                        out.data_ptr(), out_len, flags, _stream()), "cough_prepare_rows")
    assert buf[misalign + n * out_len].item() == JUNK and (misalign == 0 or buf[misalign - 1].item() == JUNK)
    return out.view(n, out_len).cpu()


def _special_rows(n, seed):
    """An all-zero row, a row holding a NaN, and a row whose peak is its first sample (outside any centre window)."""
    zero = torch.zeros(n)
    nan = _rows([n], seed)[0]
    nan[n // 2] = float("nan")
    edge = _rows([n], seed + 1)[0] * 0.5
    edge[0] = -3.0
    return [zero, nan, edge]


@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


# ------------------------------------------------------------------------------------------------ cough_prepare_rows
@pytest.mark.parametrize("out_len,lengths,special", [(8, list(range(1, 21)), 13), (16000, LONG, 40001)])
def test_prepare_rows_equals_normalize_then_pad_or_trim(out_len, lengths, special, pre):
    rows = _rows(lengths, seed=out_len) + _special_rows(special, seed=3) + _special_rows(max(out_len - 3, 1), seed=5)
    data, offs, lens, offsets = _pack(rows)
    assert {o % 4 for o in offsets} == {0, 1, 2, 3} or out_len == 16000
    n = len(rows)
    got = _prepare(data, offs, lens, n, out_len)
    for r, x in enumerate(rows):
        want = ofeat.pad_or_trim(ofeat.normalize(x.unsqueeze(0)), out_len)
        same = torch.equal(got[r:r + 1].nan_to_num(nan=123.0), want.nan_to_num(nan=123.0))
        assert same and torch.equal(got[r:r + 1].isnan(), want.isnan()), (r, x.numel())
        per_clip = pre._prepare(data[offsets[r]:offsets[r] + x.numel()].unsqueeze(0), out_len, True).cpu()
        assert torch.equal(got[r:r + 1].isnan(), per_clip.isnan())
        assert torch.equal(got[r:r + 1].nan_to_num(nan=123.0), per_clip.nan_to_num(nan=123.0)), (r, x.numel())
    k = len(lengths)
    assert not got[k].any()                                                # the all-zero row: unchanged, no 0 / 0
    assert got[k + 1].isnan().sum() == 1                                   # the NaN row: unscaled, the NaN where it was
    nan_row = rows[k + 1]
    assert torch.equal(got[k + 1].nan_to_num(nan=0.0), ofeat.pad_or_trim(nan_row.unsqueeze(0), out_len)[0].nan_to_num(nan=0.0))
    if special > out_len:                                                  # the peak (3.0) was trimmed away but still divides
        assert got[k + 2].abs().max() < 0.2 and torch.equal(got[k + 2], ofeat.pad_or_trim(rows[k + 2].unsqueeze(0) / 3.0, out_len)[0])
    # the flag off: pad_or_trim alone; an output that starts off 16 bytes: the same values
    off = _prepare(data, offs, lens, n, out_len, flags=0)
    for r, x in enumerate(rows):
        want = ofeat.pad_or_trim(x.unsqueeze(0), out_len)
        assert torch.equal(off[r:r + 1].nan_to_num(nan=123.0), want.nan_to_num(nan=123.0)), (r, x.numel())
    for misalign in (1, 2, 3):
        again = _prepare(data, offs, lens, n, out_len, misalign=misalign)
        assert torch.equal(again.nan_to_num(nan=123.0), got.nan_to_num(nan=123.0)), misalign
    if out_len == 16000:
        for r in (3, 6):                                                   # the public per-clip call
            clip = data[offsets[r]:offsets[r] + rows[r].numel()].unsqueeze(0)
            assert torch.equal(pre.prepare_clip(clip).cpu(), got[r:r + 1])


# ------------------------------------------------------------------------------------------------ cough_gather_rows
@pytest.mark.parametrize("extra,misalign", [(0, 0), (3, 1), (1, 2), (6, 3)])
def test_gather_rows_equals_slicing(extra, misalign):
    lengths = LONG + list(range(1, 10))
    rows = _rows(lengths, seed=17)
    data, offs, lens, _ = _pack(rows, first=1 + misalign)
    n, row_len = len(rows), max(lengths)
    stride = row_len + extra
    buf = torch.full((n * stride + misalign,), JUNK, device="cuda")
    out = buf[misalign:]
    _lib.check_data(_lib.load_data().cough_gather_rows(data.data_ptr(), offs.data_ptr(), lens.data_ptr(), n, out.data_ptr(),
                                                       stride, row_len, _stream()), "cough_gather_rows")
    got = out.view(n, stride).cpu()
    for r, x in enumerate(rows):
        assert torch.equal(got[r, :x.numel()], x), r
        assert not got[r, x.numel():row_len].any(), r                      # the zero tail
        assert (got[r, row_len:] == JUNK).all(), r                         # the pitch's padding is not touched
    assert (buf[:misalign] == JUNK).all()
    assert row_len == 40001 and got[6, row_len - 1] == rows[6][-1]         # row_len is the longest length


# ------------------------------------------------------------------------------------------------ cough_mask_images
def _mask_case(shape, sets, seed):
    b, h, w = shape
    x = torch.randn(b, h, w, generator=torch.Generator().manual_seed(seed))
    n = max(len(s) for s in sets)
    arr = torch.zeros(3, b, n, dtype=torch.int32)
    want = x.clone()
    for i, s in enumerate(sets):
        for k, (a, lo, hi) in enumerate(s):
            arr[:, i, k] = torch.tensor([a, lo, hi])
            idx = torch.arange(h if a == 0 else w)
            m = (idx >= lo) & (idx < hi)
            want[i] = want[i].masked_fill(m.unsqueeze(-1) if a == 0 else m, 0.0)
    return x, arr, want, n


SMALL_SETS = [[(0, 1, 3), (1, 2, 2), (1, 5, 7)],                           # an empty mask in the middle
              [],                                                          # the coin did not fire: every mask empty
              [(0, 0, 5), (1, 0, 1), (1, 0, 4)]]                           # full height; overlapping column masks
LARGE_SETS = [[(0, 10, 19), (0, 15, 22), (1, 0, 20), (1, 95, 101)],        # overlapping rows; both edges of the time axis
              [(1, 50, 50), (0, 89, 90), (1, 3, 4), (0, 0, 0)]]


@pytest.mark.parametrize("shape,sets", [((3, 5, 7), SMALL_SETS), ((2, 90, 101), LARGE_SETS)])
def test_mask_images_equals_masked_fill_per_image(shape, sets):
    x, arr, want, n = _mask_case(shape, sets, seed=shape[1])
    d = arr.cuda()
    src = x.cuda()
    out = torch.full_like(src, JUNK)
    mask_images(src, out, d[0].contiguous(), d[1].contiguous(), d[2].contiguous(), n)
    assert torch.equal(out.cpu(), want) and torch.equal(src.cpu(), x)      # out of place: the input is left alone
    mask_images(src, src, d[0].contiguous(), d[1].contiguous(), d[2].contiguous(), n)
    assert torch.equal(src.cpu(), want)                                    # in place
    # base pointers off 16 bytes (in and out in different phases, and in place)
    for a, b in ((1, 2), (3, 3)):
        bi, bo = torch.full((x.numel() + 4,), JUNK, device="cuda"), torch.full((x.numel() + 4,), JUNK, device="cuda")
        vi = bi[a:a + x.numel()].view(x.shape)
        vi.copy_(x)
        vo = vi if a == b else bo[b:b + x.numel()].view(x.shape)
        mask_images(vi, vo, d[0].contiguous(), d[1].contiguous(), d[2].contiguous(), n)
        assert torch.equal(vo.cpu(), want), (a, b)
        assert bo[b - 1].item() == JUNK and bo[b + x.numel()].item() == JUNK and bi[a + x.numel()].item() == JUNK
    # n_masks = 0: a copy
    out = torch.full_like(src, JUNK)
    mask_images(x.cuda(), out, None, None, None, 0)
    assert torch.equal(out.cpu(), x)


@pytest.mark.parametrize("p", [1.0, 0.5])
@pytest.mark.parametrize("shape", [(3, 1, 5, 7), (6, 1, 90, 101), (4, 90, 101)])
def test_mask_batch_equals_spec_augment_image_by_image(shape, p):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(2))
    spec = cda.SpecAugment(freq_mask_param=4 if shape[-2] == 5 else 10, time_mask_param=5 if shape[-1] == 7 else 20, p=p)
    for seed in (0, 1):
        random.seed(seed); torch.manual_seed(seed)
        got = spec.mask_batch(x)
        state = (random.random(), torch.rand(1).item())
        random.seed(seed); torch.manual_seed(seed)
        want = torch.stack([oaug.spec_augment(x[i], spec.freq_mask_param, spec.time_mask_param, 2, 2, p) for i in range(shape[0])])
        assert (random.random(), torch.rand(1).item()) == state
        assert got.device == x.device and torch.equal(got, want), seed
        random.seed(seed); torch.manual_seed(seed)
        on_gpu = spec.mask_batch(x.cuda())
        assert on_gpu.is_cuda and torch.equal(on_gpu.cpu(), want)
    if p == 1.0 and shape[-2] == 90:
        assert not torch.equal(got, x)


# ------------------------------------------------------------------------------------------------ the loader, end to end
def _noise_bank():
    g = torch.Generator().manual_seed(11)
    return [torch.randn((1, 700), generator=g) * 0.3, torch.randn((1, 9000), generator=g)]


def _augmentor(p):
    aug = cda.AudioAugmentor(p_augment=p)
    aug.noise_samples = _noise_bank()
    aug._pack_bank()
    return aug


@pytest.fixture(scope="module")
def bank():
    return cda.DeviceClipBank(_rows(LENGTHS, seed=23), LABELS)


def _seed(s):
    random.seed(s); torch.manual_seed(s)


def _diff(a, b):
    return (a.float().cpu() - b.float().cpu()).abs().nan_to_num(nan=float("inf")).max().item()


@pytest.mark.parametrize("p", [1.0, 0.5])
def test_training_batches_equal_the_per_clip_path(p, bank, pre):
    aug, spec = _augmentor(p), cda.SpecAugment(p=p)
    # shuffled, not weighted: every clip of the bank is visited, the trimmed ones at every phase of 16 bytes included
    loader = cda.DeviceDataLoader(bank, pre, batch_size=4, audio_augmentor=aug, spec_augmentor=spec, noise="host",
                                  use_weighted_sampler=False, generator=torch.Generator().manual_seed(31))
    order = cda.DeviceDataLoader(bank, pre, batch_size=4, use_weighted_sampler=False,
                                 generator=torch.Generator().manual_seed(31)).epoch_indices()
    assert sorted(order) == list(range(12))
    _seed(100)
    batches = list(loader)
    assert len(batches) == 3 == len(loader)
    # the same items, one at a time, through the public per-clip calls with the same seeds
    _seed(100)
    worst, unequal = 0.0, []
    for k, (feats, targets) in enumerate(batches):
        idx = order[4 * k:4 * k + 4]
        assert tuple(feats.shape) == (4, 1, 90, 101) and feats.dtype == torch.float32 and feats.is_cuda
        assert targets.dtype == torch.int64 and targets.is_cuda and targets.tolist() == [LABELS[i] for i in idx]
        for row, i in enumerate(idx):
            w = aug.augment(bank.clip(i))
            w = pre.pad_or_trim(pre.normalize(w))
            want = spec(pre.extract_features(w))
            d = _diff(feats[row], want)
            worst = max(worst, d)
            if not torch.equal(feats[row], want):
                unequal.append((k, row, i))
            print(f"p {p} batch {k} row {row} clip {i} (n = {LENGTHS[i]}): max |batch - per clip| = {d:.3e}")
    print(f"p {p}: largest difference {worst:.3e}; unequal items {unequal}")
    assert not unequal
    if p == 1.0:
        assert all((f == 0).any() for f, _ in batches)


def test_validation_loader_equals_process_per_clip(bank, pre):
    val = cda.DeviceDataLoader(bank, pre, batch_size=5, is_training=False, audio_augmentor=_augmentor(1.0),
                               spec_augmentor=cda.SpecAugment(p=1.0))
    batches = list(val)
    assert [f.shape[0] for f, _ in batches] == [5, 5, 2] and len(val) == 3     # the ragged last batch is kept
    feats, targets = torch.cat([f for f, _ in batches]), torch.cat([t for _, t in batches])
    assert targets.tolist() == LABELS
    for i in range(len(bank)):
        assert torch.equal(feats[i], pre.process(bank.clip(i), 16000)), i
    again = torch.cat([f for f, _ in val])
    assert torch.equal(again, feats)


def test_cached_features_and_device_noise_repeat(bank, pre):
    plain = torch.cat([f for f, _ in cda.DeviceDataLoader(bank, pre, batch_size=5, is_training=False)])
    cached = cda.DeviceDataLoader(bank, pre, batch_size=5, is_training=False, cache_features=True)
    first = torch.cat([f for f, _ in cached])
    cache_ptr = cached._cache.data_ptr()
    second = torch.cat([f for f, _ in cached])
    assert torch.equal(first, plain) and torch.equal(second, first) and cached._cache.data_ptr() == cache_ptr
    # a training loader with SpecAugment only: masks on top of the cached features, the cache itself stays unmasked
    spec = cda.SpecAugment(p=1.0)
    tr = cda.DeviceDataLoader(bank, pre, batch_size=4, spec_augmentor=spec, use_weighted_sampler=False, cache_features=True,
                              generator=torch.Generator().manual_seed(4))
    order = cda.DeviceDataLoader(bank, pre, batch_size=4, use_weighted_sampler=False,
                                 generator=torch.Generator().manual_seed(4)).epoch_indices()
    _seed(9)
    got = torch.cat([f for f, _ in tr])
    _seed(9)
    for row, i in enumerate(order):
        assert torch.equal(got[row], spec(plain[i])), (row, i)
    assert torch.equal(tr._cache, plain[:, 0])
    # noise="device": two loaders with the same seeds yield the same batches; another seed, other noise
    def run(seed):
        ld = cda.DeviceDataLoader(bank, pre, batch_size=4, audio_augmentor=_augmentor(1.0), spec_augmentor=cda.SpecAugment(p=0.5),
                                  generator=torch.Generator().manual_seed(6))
        _seed(seed)
        return [(f.clone(), t.clone()) for f, t in ld]
    a, b, c = run(1), run(1), run(2)
    assert len(a) == 3
    for (fa, ta), (fb, tb) in zip(a, b):
        assert torch.equal(fa, fb) and torch.equal(ta, tb) and torch.isfinite(fa).all()
    assert any(not torch.equal(fa, fc) for (fa, _), (fc, _) in zip(a, c))


def test_fit_runs_on_two_loaders(tmp_path, bank, pre):
    torch.manual_seed(0)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    sd = model.state_dict()
    sd["classifier.4.bias"] = sd["classifier.4.bias"] + torch.tensor([0.0, 1.0])     # leans towards "cough": F1 > 0 from epoch 0
    model.load_state_dict(sd)
    tr = SmallTrainer(model, class_weights=cda.class_weights_from_counts(bank.class_counts), seed=5)
    train, val = cda.create_data_loaders(bank, bank, pre, batch_size=4, audio_augmentor=_augmentor(0.5),
                                         spec_augmentor=cda.SpecAugment(p=0.5), generator=torch.Generator().manual_seed(8))
    _seed(3)
    res = cda.fit(tr, train, val, str(tmp_path), epochs=2, patience=5, config=dict(CONFIG))
    print("fit over two loaders:", res["history"])
    assert res["epochs_run"] == 2 and [h["epoch"] for h in res["history"]] == [0, 1]
    for h in res["history"]:
        assert h["val"]["tp"] + h["val"]["fp"] + h["val"]["fn"] + h["val"]["tn"] == 12
        assert h["train"]["loss"] == h["train"]["loss"] and h["val"]["loss"] == h["val"]["loss"]
    assert (tmp_path / "best_model.pt").exists() and (tmp_path / "latest_model.pt").exists()
    ck = torch.load(str(tmp_path / "latest_model.pt"), map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["trainer_state"] == {"seed": 5, "draws": 6}       # 3 training batches per epoch
