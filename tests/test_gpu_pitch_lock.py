"""The locked stretch on the MI355X (mode bit 0 of a plan's ``reserved`` word: identity phase locking) against
tests/pitch_lock_ref.py.

The stretch is compared per sample with the float64 restatement under the contract of include/cough_amd_pitch.h,
``|y - y_ref| <= 2^-24 |y_ref| + E_lock[m]`` (tests/test_pitch_lock_host.py checks that the inputs are fit for it: floor
and peak margins of at least 64).  Mixed batches, special rows, the draw, the chain and the loader are compared bit for
bit.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import pitch as cpitch
from cough_detector_amd import warp as cwarp
import pitch_lock_ref as L
import pitch_ref as P
import warp_ref as W
from test_gpu_pitch import SHIPPED, _restated_plan, _rows, _stretch_guarded

pytestmark = pytest.mark.gpu
LOCK = cpitch.PHASE_LOCK


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the stretch
@pytest.fixture(scope="module")
def batch():
    """``lock_cases()`` at odd packed offsets with NaN between the rows, stretched once all locked and once all plain."""
    refs = L.lock_refs()
    cases = [(name, x, shift, rate) for name, x, shift, rate, _, _ in refs]
    packed, offsets = P.pack(cases)
    assert len({int(o) % 4 for o in offsets}) >= 3
    data, offs = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    lens = torch.tensor([x.size for _, x, _, _ in cases], dtype=torch.int32).cuda()
    n_samples = max(lk["n_s"] for *_, lk, _ in refs)
    plans = [(shift, rate) for _, _, shift, rate in cases]
    locked = [(shift, rate, LOCK) for shift, rate in plans]
    out, new_lens, intact = _stretch_guarded(data, offs, lens, locked, n_samples)
    plain, plain_lens, plain_intact = _stretch_guarded(data, offs, lens, plans, n_samples)
    return dict(refs=refs, data=data, offs=offs, lens=lens, plans=plans, out=out, new_lens=new_lens, intact=intact,
                plain=plain, plain_lens=plain_lens, plain_intact=plain_intact, n_samples=n_samples)


def _live(name, x, rate, ref):
    return P.stretchable(rate, x.size) and ref["peak"] > 0.0


def test_every_locked_sample_is_inside_the_bound(batch):
    assert batch["intact"]                                                 # nothing written outside d_out and d_new_lengths
    seen = 0
    for r, (name, x, shift, rate, ref, _) in enumerate(batch["refs"]):
        assert batch["new_lens"][r] == ref["n_s"] == cpitch.stretched_length(x.size, rate), name
        assert not batch["out"][r, ref["n_s"]:].any(), name
        if not _live(name, x, rate, ref):
            continue
        y = batch["out"][r, :ref["n_s"]].astype(np.float64)
        tol = 2.0 ** -24 * np.abs(ref["y"]) + ref["E"]
        ratio = float((np.abs(y - ref["y"]) / tol).max())
        print(f"{name}: worst |y - y_ref| / (2^-24 |y_ref| + E_lock) = {ratio:.3f}; worst error {np.abs(y - ref['y']).max():.2e}, "
              f"peak {np.abs(ref['y']).max():.3f}, {ref['peaks_per_frame']:.1f} peaks per frame")
        assert ratio <= 1.0, (name, ratio)
        seen += 1
    assert seen >= 24


def test_a_locked_row_is_not_the_plain_row(batch):
    """Where the two restatements differ by a good part of the peak, so does the kernel's output from the plain
    restatement: a kernel that ignores the mode fails here."""
    seen = 0
    for r, (name, x, shift, rate, ref, plain) in enumerate(batch["refs"]):
        if not _live(name, x, rate, ref):
            continue
        peak = np.abs(plain["y"]).max()
        if np.abs(ref["y"] - plain["y"]).max() <= 0.2 * peak:              # the restatements (nearly) coincide
            continue
        y = batch["out"][r, :ref["n_s"]].astype(np.float64)
        assert np.abs(y - plain["y"]).max() > 0.1 * peak, name
        seen += 1
    assert seen >= 10


# ------------------------------------------------------------------------------------------------ 2. mixed batches
def test_modes_are_per_row_and_only_bit_0_counts(batch):
    assert batch["plain_intact"] and (batch["plain_lens"] == batch["new_lens"]).all()
    n = batch["n_samples"]
    for first in (0, 1):                                                   # modes alternate row by row, both ways round
        modes = [(r + first) % 2 for r in range(len(batch["plans"]))]
        plans = [(shift, rate, m) for (shift, rate), m in zip(batch["plans"], modes)]
        out, lens, intact = _stretch_guarded(batch["data"], batch["offs"], batch["lens"], plans, n)
        assert intact and (lens == batch["new_lens"]).all()
        for r, m in enumerate(modes):
            want = batch["out"] if m else batch["plain"]
            assert (_bits(out[r]) == _bits(want[r])).all(), (batch["refs"][r][0], m)
    # every other bit of the word is ignored
    odd = [(shift, rate, 0x7FFFFFFF if r % 2 else 0x7FFFFFFE) for r, (shift, rate) in enumerate(batch["plans"])]
    out, lens, intact = _stretch_guarded(batch["data"], batch["offs"], batch["lens"], odd, n)
    assert intact
    for r in range(len(odd)):
        want = batch["out"] if r % 2 else batch["plain"]
        assert (_bits(out[r]) == _bits(want[r])).all(), batch["refs"][r][0]
    sign = [(shift, rate, -2 if r % 2 else -1) for r, (shift, rate) in enumerate(batch["plans"])]      # 0xfffffffe, 0xffffffff
    out, _, intact = _stretch_guarded(batch["data"], batch["offs"], batch["lens"], sign, n)
    assert intact
    for r in range(len(sign)):
        want = batch["plain"] if r % 2 else batch["out"]
        assert (_bits(out[r]) == _bits(want[r])).all(), batch["refs"][r][0]
    # a row alone is the row in its batch
    names = [name for name, *_ in batch["refs"]]
    for name in ("257 slow", "640", "16000 tone", "16000 half", "48000 burst", "8000 stack", "6000 tie", "1000 nan", "1000 rate 1"):
        r = names.index(name)
        shift, rate = batch["plans"][r]
        one, one_len, intact = _stretch_guarded(batch["data"], batch["offs"][r:r + 1].clone(), batch["lens"][r:r + 1].clone(),
                                                [(shift, rate, LOCK)], n)
        assert intact and one_len[0] == batch["new_lens"][r]
        assert (_bits(one[0]) == _bits(batch["out"][r])).all(), name


def test_special_rows_in_mode_1_are_what_they_are_in_mode_0(batch):
    copies = poisoned = silent = 0
    for r, (name, x, shift, rate, ref, _) in enumerate(batch["refs"]):
        got = batch["out"][r, :ref["n_s"]]
        if not P.stretchable(rate, x.size):                                # rate 1, 3, NaN; n < 257
            assert ref["n_s"] == x.size and (_bits(got) == _bits(W.shifted(x, shift))).all(), name
            copies += 1
        elif not np.isfinite(W.shifted(x, shift)).all():
            assert np.isnan(got).all() and got.size == ref["n_s"] > 0, name
            poisoned += 1
        elif ref["peak"] == 0.0:                                           # zeros, shifted out
            assert not got.any() and not np.signbit(got).any() and got.size == ref["n_s"] > 0, name
            silent += 1
        else:
            continue
        assert (_bits(batch["out"][r]) == _bits(batch["plain"][r])).all(), name
    assert (copies, poisoned, silent) == (8, 2, 3)
    # while i0(t) == t the two modes are one formula; the kernel's two paths then agree to rounding
    for r, (name, x, shift, rate, ref, _) in enumerate(batch["refs"]):
        if _live(name, x, rate, ref) and ref["telescopes"]:
            assert np.abs(batch["out"][r] - batch["plain"][r]).max() <= 1e-6 * ref["peak"], name


# ------------------------------------------------------------------------------------------------ 3. the draw
def _table_dev(lo, hi, sr, modes):
    arr = np.zeros(hi - lo + 1, dtype=cpitch._STEP_DTYPE)
    for k, (rate, orig, mode) in enumerate(L.step_table(lo, hi, sr, modes)):
        arr[k] = (rate, orig, mode)
    return torch.from_numpy(arr.view(np.uint8).reshape(hi - lo + 1, 16)).cuda()


@pytest.mark.parametrize("b", [1, 64, 257])
def test_the_draw_hands_the_tables_mode_to_the_rows_with_semitones(b):
    pool = [0, 1, 256, 257, 399, 16000, 16257, 48000, 2**31 - 1]
    lengths = [pool[(5 * i + b) % len(pool)] for i in range(b)]
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    case, locked_rows, plain_fired = 0, 0, 0
    for p in (0.0, 0.5, 1.0):
        for (lo, hi), sr in (((-2, 2), 16000), ((-12, 12), 16000), ((3, 3), 22050), ((-1, 0), 2**19)):
            case += 1
            seed = (case * 0x9E3779B97F4A7C15 + b) & (2**64 - 1)
            # every entry locked (the Python front's table); words whose other bits are set; a table of zeros
            words = [0x7FFFFFFE + (k % 2) if k % 3 else k % 2 for k in range(hi - lo + 1)]
            for modes, table in ((1, None), (words, _table_dev(lo, hi, sr, words)), (0, _table_dev(lo, hi, sr, 0))):
                if table is None:
                    stretch, back, n_s = cda.draw_pitch(seed, lens, p, (lo, hi), sr, phase_lock=True)
                else:
                    stretch, back, n_s = cda.draw_pitch(seed, lens, p, (lo, hi), sr, table)
                rates, want_back, want_n_s, steps, fired, mode = L.draw_pitch_lock_ref(seed, lengths, p, lo, hi, sr, modes)
                want = cpitch.plan_array([(0, r, m) for r, m in zip(rates, mode)])
                assert (stretch.cpu().numpy() == want).all(), (p, lo, hi, sr)
                assert (back.cpu().numpy() == want_back).all() and (n_s.cpu().numpy() == want_n_s).all(), (p, lo, hi, sr)
                assert not mode[~(fired & (steps != 0))].any() and set(mode.tolist()) <= {0, 1}
                if modes == 1:
                    assert (mode == (fired & (steps != 0))).all()
                    locked_rows += int(mode.sum())
                    plain_fired += int((fired & (steps == 0)).sum())
                if modes == 0:                                             # a zero table draws what it always drew
                    plain = cda.draw_pitch(seed, lens, p, (lo, hi), sr)
                    assert not mode.any() and all(torch.equal(u, v) for u, v in zip(plain, (stretch, back, n_s)))
    assert locked_rows > 0 and (plain_fired > 0 or b == 1)


# ------------------------------------------------------------------------------------------------ 4. chain and loader
LENGTHS = [300, 16000, 4097, 9000, 700, 12001]
BANK = [700, 9000]


def _augmentor(p, speed, phase_lock):
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed, pitch=True, phase_lock=phase_lock)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in BANK]
    aug._pack_bank()
    return aug


def _padded(rows):
    x = torch.zeros((len(rows), max(r.numel() for r in rows)))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    return x


@pytest.mark.parametrize("speed", [False, True])
def test_augment_batch_equals_augment_clip_by_clip_and_the_flag_matters(speed):
    rows = _rows(LENGTHS, seed=5)
    x = _padded(rows).cuda()
    results = {}
    for lock in (True, False):
        aug = _augmentor(1.0, speed, lock)
        random.seed(31)
        torch.manual_seed(31)
        got, got_lens = aug.augment_batch(x, lengths=LENGTHS, noise="host", return_lengths=True)
        state = random.getstate()
        random.seed(31)
        torch.manual_seed(31)
        singles = [aug.augment(row[None].cuda()) for row in rows]
        assert random.getstate() == state
        assert got_lens.tolist() == [s.shape[1] for s in singles]
        for r, s in enumerate(singles):
            assert torch.equal(got[r, :s.shape[1]], s[0]), (lock, r)
        results[lock] = (got, got_lens.tolist(), state)
    assert results[True][1:] == results[False][1:]                        # the same draws, the same lengths
    random.seed(31)
    steps = [aug.draw_item_pitched(v)[3] for v in LENGTHS]
    assert sum(1 for s in steps if s) >= 2
    for r, s in enumerate(steps):                                          # rows with semitones differ; 300 at +-1 may telescope
        same = torch.equal(results[True][0][r], results[False][0][r])
        assert same if not s else (not same or LENGTHS[r] < 1000), (r, s)
    assert any(s and not torch.equal(results[True][0][r], results[False][0][r]) for r, s in enumerate(steps))


@pytest.fixture(scope="module")
def loader_parts():
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    return pre, cda.DeviceClipBank(_rows(LENGTHS, seed=23), [0, 1, 0, 1, 0, 1]), list(range(6))


def _calls(monkeypatch, fn):
    """The native calls ``fn`` makes, by name, in order, with its result."""
    seen = []
    for name in ("pitch", "warp", "draws", "data"):
        lib = getattr(_lib, f"load_{name}")()
        for symbol in getattr(_lib, f"{name.upper()}_SYMBOLS"):
            real = getattr(lib, symbol)
            monkeypatch.setattr(lib, symbol, (lambda real, symbol: lambda *a: (seen.append(symbol), real(*a))[1])(real, symbol))
    result = fn()
    monkeypatch.undo()
    return seen, result


@pytest.mark.parametrize("speed", [False, True])
def test_the_loader_carries_the_mode_in_both_draw_modes(loader_parts, monkeypatch, speed):
    pre, bank, indices = loader_parts
    spec = cda.SpecAugment(p=0.5)
    feats, calls = {}, {}
    for lock in (True, False):
        aug = _augmentor(1.0, speed, lock)
        dev = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=aug, spec_augmentor=spec, draws="device",
                                   generator=torch.Generator().manual_seed(1))
        host = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=aug, spec_augmentor=spec, draws="host",
                                    generator=torch.Generator().manual_seed(1))
        seed = 2**63 + 12345
        calls[lock, "device"], (got, targets) = _calls(monkeypatch, lambda: dev.launch_batch_drawn(indices, seed))
        plan, fired = _restated_plan(seed, LENGTHS, aug, spec, dev.feature_shape())
        assert fired.sum() >= 2
        # the host's plans of the restated draws are the bytes the device drew: exactly the rows with semitones locked
        plans = cda.chain.host_plans([c.shift for c in plan.clips], plan.pairs, plan.steps, LENGTHS, 16000,
                                     max(LENGTHS), lock)
        modes = plans.arrays["stretch"].view(cpitch._PLAN_DTYPE)["reserved"].reshape(-1)
        assert (modes == (fired & lock)).all()
        calls[lock, "host"], (want, want_targets) = _calls(monkeypatch, lambda: host.launch_batch(indices, plan))
        assert torch.equal(got, want) and torch.equal(targets, want_targets), lock
        feats[lock] = (got, fired)
    for draws in ("device", "host"):                                       # the launches of phase_lock=False
        assert calls[True, draws] == calls[False, draws] and "cough_stretch_rows" in calls[True, draws]
    fired = feats[True][1]
    differ = [not torch.equal(feats[True][0][r], feats[False][0][r]) for r in range(6)]
    assert not any(d and not f for d, f in zip(differ, fired)) and sum(differ) >= 2


# ------------------------------------------------------------------------------------------------ 5. the tone
def test_a_locked_tone_keeps_its_level_on_the_device():
    sr, n = 16000, 16000
    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)).astype(np.float32)
    src = torch.from_numpy(x).cuda()
    offs, lens = torch.zeros(1, dtype=torch.int64).cuda(), torch.tensor([n], dtype=torch.int32).cuda()
    back = torch.from_numpy(cwarp.plan_array([(0,) + cpitch.pitch_rate_pair(2, sr)])).cuda()
    level = {}
    for mode in (LOCK, 0):
        stretch = torch.from_numpy(cpitch.plan_array([(0, cpitch.pitch_rate(2), mode)])).cuda()
        y = cda.pitch_shift_rows(src, offs, lens, stretch, back, n).cpu().numpy()[0].astype(np.float64)
        level[mode] = np.sqrt((y[1000:-1000] ** 2).mean()) / np.sqrt((x[1000:-1000].astype(np.float64) ** 2).mean())
        if mode:
            peak_hz = np.abs(np.fft.rfft(y * np.hanning(n))).argmax() * sr / n
            assert abs(peak_hz - 493.9) <= sr / n
            assert np.abs(y - L.pitch_shift_lock_ref(x, 2, sr)).max() <= 1e-5
    print(f"440 Hz, +2 semitones on the device: rms ratio {level[LOCK]:.4f} locked, {level[0]:.4f} plain")
    assert 0.95 <= level[LOCK] <= 1.05 and level[0] <= 0.7
