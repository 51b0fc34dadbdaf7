"""A batch's draws on the MI355X (cough_detector_amd/draws.py, csrc/draws.hip) against tests/draws_ref.py.

Everything here is compared bit for bit.  The draw kernel's float64 arithmetic is one IEEE operation per operator, which
is what numpy computes, so its records (ints, ``gain`` as float32 bits, the SNRs as float64 bits) and masks equal the
restatement's.  ``cough_augment_rows_drawn`` runs the kernel ``cough_augment_waveforms`` runs (csrc/augment_kernel.h) on
the same samples with the same records and seed; the one place the two could differ is ``pow(10, snr / 10)``, taken on
the device by one and by the host's libm by the other, and only where the float64 result lies within an ulp of a
float32 rounding boundary (about 2^-29 per draw).
"""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd.data import BatchPlan
from cough_detector_amd.training import SmallTrainer
import draws_ref as R

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
CONFIG = dict(model_type="small", sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400, f_min=100.0,
              f_max=4000.0, segment_duration=1.0, n_mfcc=13, use_mfcc=True, pre_emphasis_coef=0.97, n_contrast_bands=6,
              **SHIPPED)
LENGTHS = [1, 2, 5, 399, 16000, 16257]      # 1..5: negative shifts truncate to 0; 16257 > AUG_LDS_MAX: the unstaged kernel
BANK = [700, 9000, 20000]                   # 700 is shorter than most clips: the reference repeats it
JUNK = 7.0e4                                # between the rows of a packed buffer: a kernel that reads past a row shows it


@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


def _augmentor(p, n_bank=3):
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in BANK[:n_bank]]
    aug._pack_bank()
    return aug


def _rows(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * 0.8 for n in lengths]


def _pack(rows, first=1):
    """Rows end to end with one junk element between them, the first at element ``first``: rows start on every phase of
    16 bytes, most of them off it.  -> (device buffer, device int64 offsets, device int32 lengths, host offsets)"""
    parts, offsets, pos = [torch.full((first,), JUNK)], [], first
    for r in rows:
        offsets.append(pos)
        parts += [r, torch.full((1,), JUNK)]
        pos += r.numel() + 1
    return (torch.cat(parts).cuda(), torch.tensor(offsets, dtype=torch.int64).cuda(),
            torch.tensor([r.numel() for r in rows], dtype=torch.int32).cuda(), offsets)


def _records(clips_dev):
    return np.frombuffer(clips_dev.cpu().numpy().tobytes(), dtype=R.CLIP_DTYPE)


def _same_records(got, want):
    for name in ("shift", "gaussian", "bank_index", "bank_start"):
        assert (got[name] == want[name]).all(), (name, np.flatnonzero(got[name] != want[name])[:5])
    assert (got["gain"].view(np.uint32) == want["gain"].view(np.uint32)).all()
    for name in ("gaussian_snr_db", "bank_snr_db"):
        assert (got[name].view(np.uint64) == want[name].view(np.uint64)).all(), name


def _clip_structs(records):
    return [_lib.CoughAugClip(shift=int(r["shift"]), gain=float(r["gain"]), gaussian=int(r["gaussian"]),
                              bank_index=int(r["bank_index"]), gaussian_snr_db=float(r["gaussian_snr_db"]),
                              bank_snr_db=float(r["bank_snr_db"]), bank_start=int(r["bank_start"])) for r in records]


def _upload_records(records):
    return torch.from_numpy(np.frombuffer(records.tobytes(), dtype=np.uint8).copy()).view(len(records), 40).cuda()


# ------------------------------------------------------------------------------------------------ 1. the records
@pytest.mark.parametrize("b", [1, 64, 65])                                 # one thread; a full block; a block with one thread
def test_records_and_masks_equal_the_restatement(b):
    lengths = [LENGTHS[(5 * i + b) % len(LENGTHS)] for i in range(b)]
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    case, fired_any = 0, set()
    for p in (0.0, 0.5, 1.0):
        for n_bank in (0, 3):
            aug = _augmentor(p, n_bank)
            for n_f, n_t in ((0, 0), (2, 2), (8, 8)):
                for (h, w), (fp, tp) in (((5, 7), (5, 7)), ((90, 101), (10, 20))):
                    case += 1
                    seed = (case * 0x9E3779B97F4A7C15 + b) & (2**64 - 1)       # both key words in use
                    spec = cda.SpecAugment(freq_mask_param=fp, time_mask_param=tp, n_freq_masks=n_f, n_time_masks=n_t, p=p)
                    clips, masks = cda.draw_batch(seed, lens, aug, spec, (h, w))
                    want_clips, want_masks, fired = R.draw_ref(seed, lengths, p, BANK[:n_bank], p, n_f, fp, n_t, tp, h, w)
                    _same_records(_records(clips), want_clips)
                    if n_f + n_t == 0:
                        assert masks is None and want_masks is None
                        continue
                    got = masks.cpu().numpy()
                    assert got.shape == want_masks.shape == (3, b, n_f + n_t) and got.dtype == np.int32
                    assert (got == want_masks).all(), (p, n_bank, n_f, h, np.argwhere(got != want_masks)[:5])
                    assert not got[:, ~fired["spec"]].any()                # a coin that did not fire: (0, 0, 0) everywhere
                    fired_any |= {k for k, f in fired.items() if f.any() and not f.all()}
                    # SpecAugment alone: no records, the same masks
                    none, alone = cda.draw_batch(seed, lens, None, spec, (h, w))
                    assert none is None and (alone.cpu().numpy() == want_masks).all()
    assert case == 36
    if b > 1:
        assert fired_any == {"shift", "gain", "gaussian", "bank", "spec"}  # p = 0.5 mixed fired and blank rows of each kind
    clips, masks = cda.draw_batch(3, lens, _augmentor(0.5), None, (90, 101))
    assert masks is None and clips.shape == (b, 40)


# ------------------------------------------------------------------------------------------------ 2. the augmentation
@pytest.mark.parametrize("lengths,p", [([1, 2, 5, 399, 16000, 8001, 12345, 16000, 700], 1.0),      # <= AUG_LDS_MAX: staged
                                       ([1, 2, 5, 399, 16000, 16257, 9000, 16257], 1.0),            # the unstaged kernel
                                       ([16257, 399, 16000, 5, 701, 16001, 3, 9001, 16257, 2048], 0.5)])
def test_augment_rows_drawn_equals_augment_waveforms(lengths, p):
    rows = _rows(lengths, seed=len(lengths))
    data, offs, lens, offsets = _pack(rows)
    assert {o % 4 for o in offsets} == {0, 1, 2, 3} or len({o % 4 for o in offsets}) >= 3      # misaligned in-place rows
    aug = _augmentor(p)
    aug._bank_dev = torch.cat([torch.full((3,), JUNK), aug._bank_host]).cuda()[3:]            # the noise bank off 16 bytes too
    n, seed = max(lengths), 0xC0FFEE123456789
    clips_dev, _ = cda.draw_batch(seed, lens, aug, None, (90, 101))
    records = _records(clips_dev)
    got = cda.augment_rows_drawn(data, offs, lens, n, clips_dev, aug, seed)
    assert tuple(got.shape) == (len(rows), n) and got.dtype == torch.float32
    gathered = torch.zeros((len(rows), n))
    for r, x in enumerate(rows):
        gathered[r, :x.numel()] = x
    want = aug._run(gathered.cuda(), _clip_structs(records), lengths, None, seed)
    unequal = [r for r in range(len(rows)) if not torch.equal(got[r], want[r])]
    for r in unequal:
        d = (got[r] - want[r]).abs().max().item()
        print(f"row {r} (n = {lengths[r]}): max |drawn - waveforms| = {d:.3e}; record {records[r]}")
    assert not unequal
    assert torch.isfinite(got).all() and got.abs().max() < 100.0           # no junk was read
    for r, x in enumerate(rows):
        assert not got[r, x.numel():].any(), r                             # the zero tail
    if p == 1.0:
        assert all(rec["gaussian"] == 1 and rec["bank_index"] >= 0 for rec in records)
        assert not torch.equal(got[4, :16000].cpu(), rows[4])
    # the bank tables are uploaded once per augmentor
    tables = aug._bank_tables
    cda.augment_rows_drawn(data, offs, lens, n, clips_dev, aug, seed)
    assert aug._bank_tables is tables and tables[1].tolist() == [0, 700, 9700] and tables[2].tolist() == BANK


# ------------------------------------------------------------------------------------------------ 3. hostile records
def test_records_the_kernel_cannot_use_are_made_harmless():
    lengths = [399, 16000, 5000, 8000, 1000, 16000, 16000, 12000, 700, 16000]
    rows = _rows(lengths, seed=77)
    data, offs, lens, _ = _pack(rows)
    aug = _augmentor(1.0)
    seed = 99
    honest, _, _ = R.draw_ref(seed, lengths, 1.0, BANK, None, 0, 0, 0, 0, 90, 101)
    honest["shift"] = np.clip(honest["shift"], -100, 100)
    hostile, neutral = honest.copy(), honest.copy()
    rep = R.repeated_length(np.asarray(BANK)[honest["bank_index"]], np.asarray(lengths))
    hostile["bank_index"][0], neutral["bank_index"][0] = 3, -1             # bank_index out of range: the step is dropped
    hostile["bank_index"][1], neutral["bank_index"][1] = -5, -1
    hostile["bank_index"][2], neutral["bank_index"][2] = 2**31 - 1, -1
    hostile["bank_start"][3], neutral["bank_index"][3] = rep[3] - lengths[3] + 1, -1      # one past the last legal start
    hostile["bank_start"][4], neutral["bank_index"][4] = -1, -1
    hostile["bank_start"][8], neutral["bank_index"][8] = 2**62, -1
    hostile["gaussian"][5], neutral["gaussian"][5] = 7, 0                  # not 0 / 1: counts as 0
    hostile["gaussian"][9], neutral["gaussian"][9] = -1, 0
    hostile["shift"][6], hostile["shift"][7] = 2**30, -2**30               # every sample shifted out: a silent clip
    for rec in neutral:                                                    # what the host API takes for "not fired"
        if rec["bank_index"] < 0:
            rec["bank_start"], rec["bank_snr_db"] = 0, 0.0
    n = max(lengths)
    got = cda.augment_rows_drawn(data, offs, lens, n, _upload_records(hostile), aug, seed)
    torch.cuda.synchronize()                                               # the call returned normally
    gathered = torch.zeros((len(rows), n))
    for r, x in enumerate(rows):
        gathered[r, :x.numel()] = x
    neutral["shift"][6] = neutral["shift"][7] = 0                          # the host API refuses |shift| >= n: checked apart
    want = aug._run(gathered.cuda(), _clip_structs(neutral), lengths, None, seed)
    for r in range(len(rows)):
        if r in (6, 7):
            assert not got[r].any(), r                                     # silence in, silence out: 0 + 0 * noise
        else:
            assert torch.equal(got[r], want[r]), r
    assert torch.isfinite(got).all() and got.abs().max() < 100.0
    again = cda.augment_rows_drawn(data, offs, lens, n, _upload_records(neutral), aug, seed)
    for r in range(len(rows)):
        if r not in (6, 7):
            assert torch.equal(again[r], want[r]), r
    # lengths the kernel cannot use: clamped to the row (0 .. n_samples); nothing is read or written outside
    bad = torch.tensor([-3, 0, 5, 2**31 - 1] + lengths[4:], dtype=torch.int32).cuda()
    offs2 = offs.clone()
    offs2[3] = offs[1]                                                     # the over-long row reads 16000 legal samples
    out = cda.augment_rows_drawn(data, offs2, bad, 16000, _upload_records(neutral), aug, seed)
    torch.cuda.synchronize()
    assert not out[0].any() and not out[1].any() and not out[2, 5:].any() and torch.isfinite(out[:4]).all()


# ------------------------------------------------------------------------------------------------ 4. the loader
def _clip_bank():
    rng = np.random.default_rng(5)
    lengths = rng.integers(8000, 48001, size=40).tolist()
    labels = [int(i % 3 == 0) for i in range(40)]
    return cda.DeviceClipBank(_rows(lengths, seed=23), labels), lengths


@pytest.fixture(scope="module")
def clip_bank():
    return _clip_bank()


def _plan(seed, lengths, aug, spec, shape):
    """The BatchPlan that holds the restated draws of ``seed``."""
    n_f, n_t = (spec.n_freq_masks, spec.n_time_masks) if spec is not None else (0, 0)
    clips, masks, fired = R.draw_ref(seed, lengths, aug.p_augment if aug is not None else None,
                                     aug._bank_lengths if aug is not None else [], spec.p if spec is not None else None,
                                     n_f, spec.freq_mask_param if spec else 0, n_t, spec.time_mask_param if spec else 0, *shape)
    plan = BatchPlan(seed=seed)
    if clips is not None:
        plan.clips = _clip_structs(clips)
    if masks is not None:
        plan.masks = [[tuple(int(v) for v in masks[:, r, m]) for m in range(n_f + n_t)] if fired["spec"][r] else []
                      for r in range(len(lengths))]
    return plan


def test_launch_batch_drawn_equals_launch_batch_on_the_restated_plan(clip_bank, pre, monkeypatch):
    bank, lengths = clip_bank
    aug, spec = _augmentor(0.5), cda.SpecAugment(p=0.5)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=8, audio_augmentor=aug, spec_augmentor=spec, draws="device",
                                  generator=torch.Generator().manual_seed(1))
    masked = 0
    for k, seed in enumerate((7, 2**63 + 12345, 2**64 - 1)):
        indices = [(11 * k + 3 * i) % 40 for i in range(8)]
        feats, targets = loader.launch_batch_drawn(indices, seed)
        plan = _plan(seed, [lengths[i] for i in indices], aug, spec, loader.feature_shape())
        want, want_targets = loader.launch_batch(indices, plan)
        assert tuple(feats.shape) == (8, 1, 90, 101) and feats.dtype == torch.float32 and feats.is_cuda
        assert torch.equal(feats, want) and torch.equal(targets, want_targets), (k, seed)
        assert targets.tolist() == [int(i % 3 == 0) for i in indices]
        masked += sum(1 for m in plan.masks if m)
    assert 0 < masked < 24                                                 # fired and blank images both occurred
    # SpecAugment on cached features: the masks are drawn on the device, the cache stays unmasked
    cached = cda.DeviceDataLoader(bank, pre, batch_size=8, spec_augmentor=cda.SpecAugment(p=1.0), cache_features=True,
                                  draws="device", generator=torch.Generator().manual_seed(1))
    indices = list(range(5, 13))
    feats, _ = cached.launch_batch_drawn(indices, 21)
    want, _ = cached.launch_batch(indices, _plan(21, [lengths[i] for i in indices], None, cached.spec_augmentor, (90, 101)))
    plain = torch.cat([f for f, _ in cda.DeviceDataLoader(bank, pre, batch_size=8, is_training=False)])
    assert torch.equal(feats, want) and not torch.equal(feats, plain[5:13]) and torch.equal(cached._cache, plain[:, 0])
    # the Python loop over clips is not on the path
    monkeypatch.setattr(cda.DeviceDataLoader, "draw_batch", lambda *a: pytest.fail("draw_batch was called"))
    assert len(list(loader)) == 5 == len(loader)


def test_epochs_repeat_with_the_generator_seed(clip_bank, pre):
    bank, lengths = clip_bank

    def run(seed, epochs=2):
        ld = cda.DeviceDataLoader(bank, pre, batch_size=8, audio_augmentor=_augmentor(0.5), spec_augmentor=cda.SpecAugment(p=0.5),
                                  draws="device", generator=torch.Generator().manual_seed(seed))
        out, seeds = [], []
        for _ in range(epochs):
            out.append([(f.clone(), t.clone()) for f, t in ld])
            seeds.append(ld.last_epoch_seed)
        return out, seeds

    state = torch.random.get_rng_state()
    (a, sa), (b, sb), (c, sc) = run(6), run(6), run(9)
    assert torch.equal(torch.random.get_rng_state(), state)                # only the loader's own generator was used
    assert sa == sb and sa != sc and sa[0] != sa[1] and all(0 <= s < 2**62 for s in sa)
    for ea, eb in zip(a, b):
        assert len(ea) == 5
        for (fa, ta), (fb, tb) in zip(ea, eb):
            assert torch.equal(fa, fb) and torch.equal(ta, tb) and torch.isfinite(fa).all()
    assert any(not torch.equal(fa, fb) for (fa, _), (fb, _) in zip(a[0], a[1]))    # the second epoch is another epoch
    assert any(not torch.equal(fa, fc) for (fa, _), (fc, _) in zip(a[0], c[0]))    # another seed, other batches


def test_validation_is_unaffected_and_fit_runs(tmp_path, clip_bank, pre):
    bank, _ = clip_bank
    train, val = cda.create_data_loaders(bank, bank, pre, batch_size=8, audio_augmentor=_augmentor(0.5),
                                         spec_augmentor=cda.SpecAugment(p=0.5), generator=torch.Generator().manual_seed(8),
                                         draws="device")
    assert train.draws == "device" and val.draws == "host"
    plain = cda.DeviceDataLoader(bank, pre, batch_size=8, is_training=False)
    for (fa, ta), (fb, tb) in zip(val, plain):
        assert torch.equal(fa, fb) and torch.equal(ta, tb)
    assert val.last_epoch_seed is None
    # a validation loader told to draw on the device has nothing to draw: the same batches, no seed taken
    g = torch.Generator().manual_seed(2)
    before = g.get_state()
    val_dev = cda.DeviceDataLoader(bank, pre, batch_size=8, is_training=False, audio_augmentor=_augmentor(1.0), draws="device",
                                   generator=g)
    for (fa, _), (fb, _) in zip(val_dev, plain):
        assert torch.equal(fa, fb)
    assert torch.equal(g.get_state(), before) and val_dev.last_epoch_seed is None
    torch.manual_seed(0)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    sd = model.state_dict()
    sd["classifier.4.bias"] = sd["classifier.4.bias"] + torch.tensor([0.0, 1.0])     # leans towards "cough": F1 > 0 at once
    model.load_state_dict(sd)
    tr = SmallTrainer(model, class_weights=cda.class_weights_from_counts(bank.class_counts), seed=5)
    res = cda.fit(tr, train, val, str(tmp_path), epochs=1, patience=5, config=dict(CONFIG))
    print("fit with draws='device':", res["history"])
    assert res["epochs_run"] == 1 and train.last_epoch_seed is not None
    h = res["history"][0]
    assert h["val"]["tp"] + h["val"]["fp"] + h["val"]["fn"] + h["val"]["tn"] == 40
    assert h["train"]["loss"] == h["train"]["loss"] and h["val"]["loss"] == h["val"]["loss"]
    assert (tmp_path / "latest_model.pt").exists()
