"""Pitch shift on the MI355X (cough_detector_amd/pitch.py, csrc/pitch.hip) against tests/pitch_ref.py.

The stretch is compared per sample with the float64 restatement under the contract of include/cough_amd_pitch.h,
``|y - y_ref| <= 2^-24 |y_ref| + E[m]``, with the first-order bound ``E`` derived in tests/pitch_ref.py
(tests/test_pitch_host.py checks that the inputs are fit for it).  Copies, special rows, the draws, and everything
that composes kernels already compared elsewhere (the chain, the loader) are compared bit for bit.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import pitch as cpitch
from cough_detector_amd import warp as cwarp
from cough_detector_amd.data import BatchPlan
from cough_detector_amd.training import SmallTrainer
import draws_ref as R
import pitch_ref as P
import warp_ref as W

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
CONFIG = dict(model_type="small", sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400, f_min=100.0,
              f_max=4000.0, segment_duration=1.0, n_mfcc=13, use_mfcc=True, pre_emphasis_coef=0.97, n_contrast_bands=6,
              **SHIPPED)
BANK = [700, 9000, 20000]
SENTINEL = -3.0e7                           # around the output: a kernel that writes outside it shows it
MARGIN = 4096


def _stretch_guarded(data, offs, lens, plans, n_samples):
    """cough_stretch_rows into the middle of sentinel-filled buffers -> (out (B, n_samples), new lengths, intact)."""
    b = lens.numel()
    buf = torch.full((2 * MARGIN + b * n_samples,), SENTINEL, dtype=torch.float32, device="cuda")
    nl = torch.full((b + 128,), -77, dtype=torch.int32, device="cuda")
    plans_dev = torch.from_numpy(cpitch.plan_array(plans)).cuda()
    _lib.check_pitch(_lib.load_pitch().cough_stretch_rows(data.data_ptr(), offs.data_ptr(), lens.data_ptr(), b,
                                                          plans_dev.data_ptr(), buf[MARGIN:].data_ptr(), n_samples,
                                                          nl[64:].data_ptr(), torch.cuda.current_stream().cuda_stream),
                     "cough_stretch_rows")
    torch.cuda.synchronize()
    intact = bool((buf[:MARGIN] == SENTINEL).all() and (buf[MARGIN + b * n_samples:] == SENTINEL).all()
                  and (nl[:64] == -77).all() and (nl[64 + b:] == -77).all())
    return buf[MARGIN:MARGIN + b * n_samples].view(b, n_samples).cpu().numpy(), nl[64:64 + b].cpu().numpy(), intact


# ------------------------------------------------------------------------------------------------ 1. the stretch
@pytest.fixture(scope="module")
def batch():
    """The ragged batch of tests/pitch_ref.py at odd packed offsets with NaN between the rows, stretched once."""
    refs = P.case_refs()
    cases = [(name, x, shift, rate) for name, x, shift, rate, _ in refs]
    packed, offsets = P.pack(cases)
    assert len({int(o) % 4 for o in offsets}) >= 3                        # rows off every 8- and 16-byte boundary
    data, offs = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    lens = torch.tensor([x.size for _, x, _, _ in cases], dtype=torch.int32).cuda()
    n_samples = max(ref["n_s"] for *_, ref in refs)
    plans = [(shift, rate) for _, _, shift, rate in cases]
    out, new_lens, intact = _stretch_guarded(data, offs, lens, plans, n_samples)
    return dict(refs=refs, data=data, offs=offs, lens=lens, plans=plans, out=out, new_lens=new_lens, intact=intact,
                n_samples=n_samples)


def test_every_sample_is_inside_the_bound(batch):
    seen = 0
    for r, (name, x, shift, rate, ref) in enumerate(batch["refs"]):
        if not P.stretchable(rate, x.size) or not ref["peak"] > 0.0:
            continue
        y = batch["out"][r, :ref["n_s"]].astype(np.float64)
        tol = 2.0 ** -24 * np.abs(ref["y"]) + ref["E"]
        ratio = float((np.abs(y - ref["y"]) / tol).max())
        print(f"{name}: worst |y - y_ref| / (2^-24 |y_ref| + E) = {ratio:.3f}; worst error {np.abs(y - ref['y']).max():.2e}, "
              f"peak {np.abs(ref['y']).max():.3f}")
        assert ratio <= 1.0, (name, ratio)
        seen += 1
    assert seen >= 20


def test_layout_tails_margins_and_new_lengths(batch):
    assert batch["intact"]                                                 # nothing written outside d_out and d_new_lengths
    for r, (name, x, shift, rate, ref) in enumerate(batch["refs"]):
        assert batch["new_lens"][r] == ref["n_s"] == cpitch.stretched_length(x.size, rate), name
        assert not batch["out"][r, ref["n_s"]:].any(), name               # zeros up to n_samples
    # a narrower output cuts the rows: the same samples, the lengths min(n_s, n_samples)
    cut, cut_lens, intact = _stretch_guarded(batch["data"], batch["offs"], batch["lens"], batch["plans"], 1500)
    assert intact and (cut.view(np.uint32) == batch["out"][:, :1500].view(np.uint32)).all()
    assert (cut_lens == np.minimum(batch["new_lens"], 1500)).all()
    # the Python front: the same bits, the lengths on request
    plans_dev = torch.from_numpy(cpitch.plan_array(batch["plans"])).cuda()
    got, got_lens = cda.stretch_rows(batch["data"], batch["offs"], batch["lens"], plans_dev, 1500, return_lengths=True)
    assert (got.cpu().numpy().view(np.uint32) == cut.view(np.uint32)).all() and (got_lens.cpu().numpy() == cut_lens).all()
    assert cda.stretch_rows(batch["data"], batch["offs"], batch["lens"], plans_dev, 1500).shape == (len(batch["plans"]), 1500)
    # a length the device cannot use: negative counts as 0
    bad = batch["lens"].clone()
    bad[4] = -3
    out, new_lens, intact = _stretch_guarded(batch["data"], batch["offs"], bad, batch["plans"], 1500)
    assert intact and new_lens[4] == 0 and not out[4].any() and (out[5].view(np.uint32) == cut[5].view(np.uint32)).all()


def test_rows_the_kernel_does_not_stretch_are_copies_and_special_rows_are_special(batch):
    copies = 0
    for r, (name, x, shift, rate, ref) in enumerate(batch["refs"]):
        got = batch["out"][r, :ref["n_s"]]
        if not P.stretchable(rate, x.size):
            assert ref["n_s"] == x.size
            assert (got.view(np.uint32) == W.shifted(x, shift).view(np.uint32)).all(), name       # bit for bit, NaN and Inf too
            copies += 1
        elif not np.isfinite(W.shifted(x, shift)).all():
            assert np.isnan(got).all() and got.size == ref["n_s"] > 0, name
        elif ref["peak"] == 0.0:
            assert not got.any() and not np.signbit(got).any() and got.size == ref["n_s"] > 0, name
    names = [name for name, *_ in batch["refs"]]
    assert copies == 8 and {"1000 nan", "16000 inf", "1000 zeros", "1000 shifted out"} <= set(names)
    live = [r for r, (name, x, shift, rate, ref) in enumerate(batch["refs"]) if np.isfinite(ref["peak"]) and name != "1000 inf copied"]
    assert np.isfinite(batch["out"][live]).all() and np.abs(batch["out"][live]).max() < 10.0       # no NaN from between the rows


def test_a_row_alone_equals_the_row_in_the_batch_and_runs_repeat(batch):
    again, again_lens, _ = _stretch_guarded(batch["data"], batch["offs"], batch["lens"], batch["plans"], batch["n_samples"])
    assert (again.view(np.uint32) == batch["out"].view(np.uint32)).all() and (again_lens == batch["new_lens"]).all()
    names = [name for name, *_ in batch["refs"]]
    for name in ("257", "640", "1000 burst", "16000 tone", "16000 half", "48000 burst", "1000 nan", "1000 rate 1"):
        r = names.index(name)
        one, one_len, intact = _stretch_guarded(batch["data"], batch["offs"][r:r + 1].clone(), batch["lens"][r:r + 1].clone(),
                                                batch["plans"][r:r + 1], batch["n_samples"])
        assert intact and one_len[0] == batch["new_lens"][r]
        assert (one[0].view(np.uint32) == batch["out"][r].view(np.uint32)).all(), name


def _tone(n=16000, hz=440.0, sr=16000):
    return (0.5 * np.sin(2 * np.pi * hz * np.arange(n) / sr)).astype(np.float32)


def test_pitch_shift_rows_is_the_two_launches_and_keeps_the_length():
    sr, n = 16000, 16000
    g = torch.Generator().manual_seed(3)
    rows = [torch.from_numpy(_tone()), (torch.rand(n, generator=g) - 0.5), (torch.rand(n, generator=g) - 0.5) * 0.1,
            torch.from_numpy(P._burst(np.random.default_rng(4), n))]
    steps = [2, -2, 0, 1]
    x = torch.stack(rows).cuda()
    offs = (torch.arange(4, dtype=torch.int64) * n).cuda()
    lens = torch.full((4,), n, dtype=torch.int32).cuda()
    stretch = torch.from_numpy(cpitch.plan_array([(0, cpitch.pitch_rate(s)) for s in steps])).cuda()
    back = torch.from_numpy(cwarp.plan_array([(0,) + cpitch.pitch_rate_pair(s, sr) for s in steps])).cuda()
    width = max(cpitch.stretched_length(n, cpitch.pitch_rate(s)) for s in steps)
    got = cda.pitch_shift_rows(x.reshape(-1), offs, lens, stretch, back, n, width)
    stretched, n_s = cda.stretch_rows(x.reshape(-1), offs, lens, stretch, width, return_lengths=True)
    assert n_s.tolist() == [cpitch.stretched_length(n, cpitch.pitch_rate(s)) for s in steps]
    want = cda.warp_rows(stretched.reshape(-1), (torch.arange(4, dtype=torch.int64) * width).cuda(), n_s, back, n)
    assert tuple(got.shape) == (4, n) and torch.equal(got, want)
    assert torch.equal(got[2], x[2])                                       # 0 semitones: both launches copy
    assert torch.equal(cda.pitch_shift_rows(x.reshape(-1), offs, lens, stretch, back, n), got)     # the default stretch width
    # the tone, two semitones up, on the device: the restatement's result within the bounds, and its pitch
    y = got[0].cpu().numpy().astype(np.float64)
    peak_hz = np.abs(np.fft.rfft(y * np.hanning(n))).argmax() * sr / n
    print(f"tone on the device: peak at {peak_hz:.1f} Hz (440 * 2^(2/12) = {440 * 2 ** (2 / 12):.1f})")
    assert abs(peak_hz - 493.9) <= sr / n
    assert np.abs(y - P.pitch_shift_ref(_tone(), 2, sr)).max() <= 1e-5     # both halves are inside their own bounds; a gross check


# ------------------------------------------------------------------------------------------------ 2. the draws
@pytest.mark.parametrize("b", [1, 63, 64, 257])                            # one thread; a block less one; a block; several
def test_pitch_draws_equal_the_restatement(b):
    pool = [0, 1, 256, 257, 399, 16000, 16257, 48000, 2**31 - 1]
    lengths = [pool[(5 * i + b) % len(pool)] for i in range(b)]
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    case, mixed = 0, False
    for p in (0.0, 0.5, 1.0):
        for (lo, hi), sr in (((-2, 2), 16000), ((-12, 12), 16000), ((3, 3), 22050), ((-1, 0), 2**19)):
            case += 1
            seed = (case * 0x9E3779B97F4A7C15 + b) & (2**64 - 1)           # both key words in use
            stretch, back, n_s = cda.draw_pitch(seed, lens, p, (lo, hi), sr)
            rates, want_back, want_n_s, steps, fired = P.draw_pitch_ref(seed, lengths, p, lo, hi, sr)
            assert stretch.dtype == torch.uint8 and tuple(stretch.shape) == (b, 16) and tuple(back.shape) == (b, 3)
            want_stretch = cpitch.plan_array([(0, r) for r in rates])
            assert (stretch.cpu().numpy() == want_stretch).all(), (p, lo, hi, sr)
            assert (back.cpu().numpy() == want_back).all(), (p, lo, hi, sr)
            assert (n_s.cpu().numpy() == want_n_s).all(), (p, lo, hi, sr)
            mixed |= bool(fired.any() and not fired.all())
    assert mixed or b == 1
    table = torch.from_numpy(cpitch.step_table((-2, 2), 16000)).cuda()     # the caller's own table on the device
    a = cda.draw_pitch(77, lens, 0.5, (-2, 2), 16000, table)
    c = cda.draw_pitch(77, lens, 0.5, (-2, 2), 16000)
    assert all(torch.equal(u, v) for u, v in zip(a, c))


# ------------------------------------------------------------------------------------------------ 3. the chain
def _rows(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * 0.8 for n in lengths]


def _augmentor(p, speed=True, pitch=True, n_bank=3):
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed, pitch=pitch)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in BANK[:n_bank]]
    aug._pack_bank()
    return aug


CHAIN_LENGTHS = [1, 2, 257, 4097, 16000, 9000, 16257, 700]


@pytest.mark.parametrize("p,speed", [(1.0, True), (0.5, True), (0.7, False)])
def test_augment_batch_equals_augment_clip_by_clip(p, speed):
    rows = _rows(CHAIN_LENGTHS, seed=5)
    n = max(CHAIN_LENGTHS)
    x = torch.zeros((len(rows), n))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    aug = _augmentor(p, speed=speed)
    random.seed(31)
    torch.manual_seed(31)
    got, got_lens = aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="host", return_lengths=True)
    random.seed(31)
    torch.manual_seed(31)
    singles = [aug.augment(row[None].cuda()) for row in rows]
    random.seed(31)
    items = [aug.draw_item_pitched(v) for v in CHAIN_LENGTHS]
    assert sum(1 for it in items if it[3]) >= 2                            # rows with semitones ...
    assert any(not it[3] for it in items)                                  # ... and without
    assert got_lens.tolist() == [s.shape[1] for s in singles] == [it[2] for it in items]
    assert tuple(got.shape) == (len(rows), max(got_lens.tolist()) if speed else n) and got.is_cuda
    for r, s in enumerate(singles):
        assert torch.equal(got[r, :s.shape[1]], s[0]), r
        assert not got[r, s.shape[1]:].any(), r
    if not speed:
        assert got_lens.tolist() == CHAIN_LENGTHS                          # the pitch step keeps the lengths
    # pitch_shift alone: the two launches without a shift
    random.seed(8)
    y = aug.pitch_shift(rows[4][None].cuda(), (2, 2))
    random.seed(8)
    if not (random.random() > p):
        assert tuple(y.shape) == (1, 16000) and not torch.equal(y.cpu(), rows[4][None])
        want = P.pitch_shift_ref(rows[4].numpy(), 2, 16000)
        assert np.abs(y[0].cpu().numpy() - want).max() <= 1e-5
    else:
        assert y.shape == (1, 16000)


def test_pitch_off_is_todays_output():
    rows = _rows(CHAIN_LENGTHS, seed=5)
    n = max(CHAIN_LENGTHS)
    x = torch.zeros((len(rows), n))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    aug = _augmentor(0.7, speed=False, pitch=False)
    random.seed(12)
    got = aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="device", seed=99)
    random.seed(12)
    want = aug._run(x.cuda(), aug.draw_batch(CHAIN_LENGTHS), CHAIN_LENGTHS, None, 99)
    assert torch.equal(got, want) and tuple(got.shape) == (len(rows), n)


# ------------------------------------------------------------------------------------------------ 4. the loader
@pytest.fixture(scope="module")
def pre():
    return cda.AudioPreprocessor(device="cuda", **SHIPPED)


@pytest.fixture(scope="module")
def clip_bank():
    rng = np.random.default_rng(5)
    lengths = rng.integers(8000, 30001, size=24).tolist()
    labels = [int(i % 3 == 0) for i in range(24)]
    return cda.DeviceClipBank(_rows(lengths, seed=23), labels), lengths


@pytest.mark.parametrize("speed", [True, False])
def test_a_host_drawn_batch_equals_its_items_one_at_a_time(clip_bank, pre, speed):
    bank, lengths = clip_bank
    loader = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=_augmentor(0.6, speed=speed),
                                  spec_augmentor=cda.SpecAugment(p=0.5), noise="host", generator=torch.Generator().manual_seed(1))
    pitched = 0
    for k in range(3):
        indices = [(7 * k + 5 * i) % 24 for i in range(6)]
        random.seed(100 + k)
        torch.manual_seed(100 + k)
        plan = loader.draw_batch(indices)
        feats, targets = loader.launch_batch(indices, plan)
        assert tuple(feats.shape) == (6, 1, 90, 101) and torch.isfinite(feats).all()
        pitched += plan.pitches()
        for r, i in enumerate(indices):
            one = BatchPlan(clips=[plan.clips[r]], gaussian=plan.gaussian[r:r + 1].contiguous(), seed=plan.seed,
                            masks=[plan.masks[r]], pairs=[plan.pairs[r]] if speed else None,
                            new_lengths=[plan.new_lengths[r]] if speed else None, steps=[plan.steps[r]])
            f, t = loader.launch_batch([i], one)
            assert torch.equal(f[0], feats[r]) and torch.equal(t[0], targets[r]), (k, r)
    assert pitched >= 2
    # the pitch step changes the features where it fired, and only there
    random.seed(102)
    torch.manual_seed(102)
    indices = [(14 + 5 * i) % 24 for i in range(6)]
    plan = loader.draw_batch(indices)
    feats, _ = loader.launch_batch(indices, plan)
    fired = [bool(s) for s in plan.steps]
    plan.steps = [None] * 6
    plain, _ = loader.launch_batch(indices, plan)
    assert any(fired) and [not torch.equal(feats[r], plain[r]) for r in range(6)] == fired


def _restated_plan(seed, lengths, aug, spec, shape):
    """The BatchPlan that holds the restated draws of ``seed`` with the speed (if the augmentor has it) and pitch steps."""
    sr = aug.sample_rate
    if aug.speed:
        plans, new_lens, _ = W.draw_speed_ref(seed, lengths, aug.p_augment, aug.speed_range[0], aug.speed_range[1], sr)
    else:
        new_lens = np.asarray(lengths, dtype=np.int32)
    _, _, _, steps, fired = P.draw_pitch_ref(seed, new_lens, aug.p_augment, aug.pitch_range[0], aug.pitch_range[1], sr)
    n_f, n_t = (spec.n_freq_masks, spec.n_time_masks) if spec is not None else (0, 0)
    clips, masks, f = R.draw_ref(seed, new_lens, aug.p_augment, aug._bank_lengths, spec.p if spec is not None else None, n_f,
                                 spec.freq_mask_param if spec else 0, n_t, spec.time_mask_param if spec else 0, *shape)
    plan = BatchPlan(seed=seed, steps=[int(s) if fi else None for s, fi in zip(steps, fired)])
    if aug.speed:
        clips["shift"] = plans[:, 0]                                       # drawn for the original length
        plan.pairs, plan.new_lengths = [(int(o), int(m)) for _, o, m in plans], [int(v) for v in new_lens]
    plan.clips = [_lib.CoughAugClip(shift=int(r["shift"]), gain=float(r["gain"]), gaussian=int(r["gaussian"]),
                                    bank_index=int(r["bank_index"]), gaussian_snr_db=float(r["gaussian_snr_db"]),
                                    bank_snr_db=float(r["bank_snr_db"]), bank_start=int(r["bank_start"])) for r in clips]
    if masks is not None:
        plan.masks = [[tuple(int(v) for v in masks[:, r, m]) for m in range(n_f + n_t)] if f["spec"][r] else []
                      for r in range(len(lengths))]
    return plan, fired & (steps != 0)


@pytest.mark.parametrize("speed", [True, False])
def test_launch_batch_drawn_equals_launch_batch_on_the_restated_plan(clip_bank, pre, monkeypatch, speed):
    bank, lengths = clip_bank
    aug, spec = _augmentor(0.5, speed=speed), cda.SpecAugment(p=0.5)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=8, audio_augmentor=aug, spec_augmentor=spec, draws="device",
                                  generator=torch.Generator().manual_seed(1))
    pitched = 0
    for k, seed in enumerate((7, 2**63 + 12345, 2**64 - 1)):
        indices = [(11 * k + 3 * i) % 24 for i in range(8)]
        feats, targets = loader.launch_batch_drawn(indices, seed)
        plan, fired = _restated_plan(seed, [lengths[i] for i in indices], aug, spec, loader.feature_shape())
        want, want_targets = loader.launch_batch(indices, plan)
        assert tuple(feats.shape) == (8, 1, 90, 101) and feats.is_cuda
        assert torch.equal(feats, want) and torch.equal(targets, want_targets), (k, seed)
        pitched += int(fired.sum())
    assert 0 < pitched < 24                                                # rows with and without a pitch step
    monkeypatch.setattr(cda.DeviceDataLoader, "draw_batch", lambda *a: pytest.fail("draw_batch was called"))
    assert len(list(loader)) == 3 == len(loader)


@pytest.mark.parametrize("draws", ["host", "device"])
def test_fit_runs_with_pitch_speed_and_mixup(tmp_path, clip_bank, pre, draws):
    bank, _ = clip_bank
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    train, val = cda.create_data_loaders(bank, bank, pre, batch_size=8, audio_augmentor=_augmentor(0.8),
                                         spec_augmentor=cda.SpecAugment(p=0.5), mixup=cda.MixUp(0.2),
                                         generator=torch.Generator().manual_seed(8), draws=draws)
    assert train.audio_augmentor.pitch and train.audio_augmentor.speed and val.audio_augmentor is None
    plain = cda.DeviceDataLoader(bank, pre, batch_size=8, is_training=False)
    for (fa, ta), (fb, tb) in zip(val, plain):                             # validation is unaffected
        assert torch.equal(fa, fb) and torch.equal(ta, tb)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    tr = SmallTrainer(model, class_weights=cda.class_weights_from_counts(bank.class_counts), seed=5)
    res = cda.fit(tr, train, val, str(tmp_path), epochs=1, patience=5, config=dict(CONFIG))
    print(f"fit with pitch=True, speed=True, MixUp, draws={draws!r}:", res["history"])
    h = res["history"][0]
    assert res["epochs_run"] == 1 and h["train"]["loss"] == h["train"]["loss"] and h["val"]["loss"] == h["val"]["loss"]
    assert h["val"]["tp"] + h["val"]["fp"] + h["val"]["fn"] + h["val"]["tn"] == 24
