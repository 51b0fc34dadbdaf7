"""Speed perturbation on the MI355X (cough_detector_amd/warp.py, csrc/warp.hip) against tests/warp_ref.py.

The resampler is compared per sample with the float64 restatement under the bound derived in tests/warp_ref.py,
``|y - y_ref| <= (2 * width + 4) * 2^-24 * A_m`` with ``A_m = sum |x_i| |h_i|``; where ``A_m == 0`` the output is
exactly 0.  Copies (``orig == new``), the draws, and everything that composes kernels already compared elsewhere (the
chain, the loader) are compared bit for bit.
"""
import random

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib, _tables
from cough_detector_amd import warp as cwarp
from cough_detector_amd.data import BatchPlan
from cough_detector_amd.training import SmallTrainer
import draws_ref as R
import warp_ref as W

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
CONFIG = dict(model_type="small", sample_rate=16000, n_mels=64, n_fft=512, hop_length=160, win_length=400, f_min=100.0,
              f_max=4000.0, segment_duration=1.0, n_mfcc=13, use_mfcc=True, pre_emphasis_coef=0.97, n_contrast_bands=6,
              **SHIPPED)
LENGTHS = [1, 2, 13, 255, 256, 257, 4097, 16000, 48000]     # below, at and above a wave, a block, a tile; many tiles
PAIRS = [(9, 10), (10, 9), (14400, 16000), (15999, 16000), (17599, 16000), (1, 1), (1, 4), (4, 1)]
BANK = [700, 9000, 20000]
JUNK = 7.0e4                                # between the rows of a packed buffer: a kernel that reads past a row shows it
SENTINEL = -3.0e7                           # around the output: a kernel that writes outside it shows it
MARGIN = 4096


def _shifts(n):
    return [0, 1, -1, n // 5, -(n // 5), n, -(n + 3), 2**31 - 1]


def _rows(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(n, generator=g) - 0.5) * 0.8 for n in lengths]


def _pack(rows, first=1):
    """Rows end to end with one junk element between them, the first at element ``first``: most rows start off a
    16-byte boundary.  -> (device buffer, device int64 offsets, device int32 lengths, host offsets)"""
    parts, offsets, pos = [torch.full((first,), JUNK)], [], first
    for r in rows:
        offsets.append(pos)
        parts += [r, torch.full((1,), JUNK)]
        pos += r.numel() + 1
    return (torch.cat(parts).cuda(), torch.tensor(offsets, dtype=torch.int64).cuda(),
            torch.tensor([r.numel() for r in rows], dtype=torch.int32).cuda(), offsets)


def _warp_guarded(data, offs, lens, plans, n_samples):
    """cough_warp_rows into the middle of sentinel-filled buffers -> (out (B, n_samples), new lengths, intact: bool)."""
    b = lens.numel()
    buf = torch.full((2 * MARGIN + b * n_samples,), SENTINEL, dtype=torch.float32, device="cuda")
    nl = torch.full((b + 128,), -77, dtype=torch.int32, device="cuda")
    plans_dev = torch.from_numpy(cwarp.plan_array(plans)).cuda()
    _lib.check_warp(_lib.load_warp().cough_warp_rows(data.data_ptr(), offs.data_ptr(), lens.data_ptr(), b, plans_dev.data_ptr(),
                                                     buf[MARGIN:].data_ptr(), n_samples, nl[64:].data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "cough_warp_rows")
    torch.cuda.synchronize()
    intact = bool((buf[:MARGIN] == SENTINEL).all() and (buf[MARGIN + b * n_samples:] == SENTINEL).all()
                  and (nl[:64] == -77).all() and (nl[64 + b:] == -77).all())
    return buf[MARGIN:MARGIN + b * n_samples].view(b, n_samples).cpu().numpy(), nl[64:64 + b].cpu().numpy(), intact


def _inside(y, y_ref, a, orig, new):
    """Worst |y - y_ref| / bound over the samples with A_m > 0; exact zeros where A_m == 0."""
    assert not y[a == 0].any()
    live = a > 0
    if not live.any():
        return 0.0
    return float((np.abs(y[live].astype(np.float64) - y_ref[live]) / (W.bound_factor(orig, new) * a[live])).max())


# ------------------------------------------------------------------------------------------------ 1. the resampler
@pytest.fixture(scope="module")
def batch():
    """Every length with every rate pair, the shift kinds cycling so that each length and each pair meets each kind."""
    cases = [(n, pair, _shifts(n)[(li + pi) % 8]) for li, n in enumerate(LENGTHS) for pi, pair in enumerate(PAIRS)]
    rows = _rows([c[0] for c in cases], seed=41)
    data, offs, lens, offsets = _pack(rows)
    assert len({o % 4 for o in offsets}) == 4                              # rows on every phase of 16 bytes
    n_samples = max(W.new_length(n, o, m) for n, (o, m), _ in cases)
    assert n_samples == 4 * 48000
    out, new_lens, intact = _warp_guarded(data, offs, lens, [(s, o, m) for _, (o, m), s in cases], n_samples)
    refs = [W.warp_ref(x.numpy(), s, o, m) for x, (_, (o, m), s) in zip(rows, cases)]
    return dict(cases=cases, rows=rows, data=data, offs=offs, lens=lens, out=out, new_lens=new_lens, intact=intact, refs=refs,
                n_samples=n_samples)


def test_every_sample_is_inside_the_bound(batch):
    worst = {}
    for r, ((n, (orig, new), shift), (y_ref, a, n_new)) in enumerate(zip(batch["cases"], batch["refs"])):
        ratio = _inside(batch["out"][r, :n_new], y_ref, a, orig, new)
        worst[(orig, new)] = max(worst.get((orig, new), 0.0), ratio)
        assert ratio <= 1.0, (n, orig, new, shift, ratio)
    for pair, ratio in worst.items():
        print(f"{pair}: worst |y - y_ref| / bound = {ratio:.3f}")
    assert np.isfinite(batch["out"]).all() and np.abs(batch["out"]).max() < 10.0       # no junk was read


def test_layout_tails_margins_and_new_lengths(batch):
    assert batch["intact"]                                                 # nothing written outside d_out and d_new_lengths
    for r, ((n, (orig, new), _), (_, _, n_new)) in enumerate(zip(batch["cases"], batch["refs"])):
        assert batch["new_lens"][r] == n_new == cwarp.warped_length(n, orig, new), (n, orig, new)
        assert not batch["out"][r, n_new:].any(), (n, orig, new)           # zeros up to n_samples
    # a narrower output cuts the rows: the same samples, the lengths min(n', n_samples); 1500 is not a multiple of the tile
    plans = [(s, o, m) for _, (o, m), s in batch["cases"]]
    cut, cut_lens, intact = _warp_guarded(batch["data"], batch["offs"], batch["lens"], plans, 1500)
    assert intact and (cut == batch["out"][:, :1500]).all()
    assert (cut_lens == np.minimum(batch["new_lens"], 1500)).all()
    # the Python front: the same bits, the lengths on request
    plans_dev = torch.from_numpy(cwarp.plan_array(plans)).cuda()
    got, got_lens = cda.warp_rows(batch["data"], batch["offs"], batch["lens"], plans_dev, 1500, return_lengths=True)
    assert (got.cpu().numpy() == cut).all() and (got_lens.cpu().numpy() == cut_lens).all()
    assert cda.warp_rows(batch["data"], batch["offs"], batch["lens"], plans_dev, 1500).shape == (len(plans), 1500)


def test_equal_rates_copy_bit_for_bit(batch):
    seen = 0
    for r, (n, (orig, new), shift) in enumerate(batch["cases"]):
        if orig == new:
            want = W.shifted(batch["rows"][r].numpy(), shift)
            assert (batch["out"][r, :n].view(np.uint32) == want.view(np.uint32)).all(), (n, shift)
            seen += 1
    assert seen == len(LENGTHS)
    rows = _rows([257, 4097], seed=2)
    data, offs, lens, _ = _pack(rows, first=3)
    for pair in ((16000, 16000), (2**20, 2**20)):
        out, new_lens, intact = _warp_guarded(data, offs, lens, [(-50,) + pair, (1000,) + pair], 4097)
        assert intact and new_lens.tolist() == [257, 4097]
        assert (out[0, :257] == W.shifted(rows[0].numpy(), -50)).all() and (out[1] == W.shifted(rows[1].numpy(), 1000)).all()


def test_unit_impulses_read_the_coefficients_out():
    equal = total = 0
    for n in (257, 4097):
        positions = [0, 1, n // 2, n - 1]
        rows = []
        for i in positions:
            x = torch.zeros(n)
            x[i] = 1.0
            rows.append(x)
        data, offs, lens, _ = _pack(rows, first=2)
        for orig, new in PAIRS:
            n_new = W.new_length(n, orig, new)
            out, _, intact = _warp_guarded(data, offs, lens, [(0, orig, new)] * 4, n_new)
            assert intact
            for r, i in enumerate(positions):
                m = np.arange(n_new, dtype=np.int64)
                if orig == new:
                    assert (out[r] == rows[r].numpy()).all()
                    continue
                h = W.coefficient(i * new - m * orig, orig, new)           # every output's coefficient for input i ...
                centre = m * orig // new
                w = W.filter_width(orig, new)
                h[(i < centre - w) | (i > centre + w + 1)] = 0.0           # ... inside the kernel's tap range
                assert np.abs(h).sum() > 0.05
                err = np.abs(out[r].astype(np.float64) - h.astype(np.float64))
                assert (err <= W.bound_factor(orig, new) * np.abs(h)).all(), (n, orig, new, i)
                nz = h != 0
                equal += int((out[r][nz].view(np.uint32) == h[nz].view(np.uint32)).sum())
                total += int(nz.sum())
    print(f"impulses: {equal} of {total} non-zero coefficients equal the restatement's float32 bit for bit")
    assert total >= 2 * 7 * 4 * 6          # an impulse meets about 12 outputs' filters, half of them at a row's end


def test_against_the_shipped_resampler_where_its_table_exists():
    lib = _lib.load()
    for n in (257, 4097, 16000):
        rows = _rows([n] * 3, seed=n)
        x = torch.stack(rows).cuda()
        offs = (torch.arange(3, dtype=torch.int64) * n).cuda()
        lens = torch.full((3,), n, dtype=torch.int32).cuda()
        for orig, new in ((9, 10), (10, 9), (14400, 16000), (1, 4), (4, 1)):
            kern, width, o, m = _tables.sinc_resample_kernel(orig, new)     # reduced by the gcd; the warp kernel's is not
            n_new = W.new_length(n, orig, new)
            want = torch.empty((3, n_new), dtype=torch.float32, device="cuda")
            table = kern.cuda()
            _lib.check(lib.cough_resample(x.data_ptr(), n, 3, n, table.data_ptr(), o, m, width, want.data_ptr(), n_new,
                                          n_new, torch.cuda.current_stream().cuda_stream), "cough_resample")
            plans = torch.tensor([[0, orig, new]] * 3, dtype=torch.int32).cuda()
            got = cda.warp_rows(x, offs, lens, plans, n_new).cpu().numpy()
            want = want.cpu().numpy()
            differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            worst = 0.0
            for r in range(3):
                _, a, _ = W.warp_ref(rows[r].numpy(), 0, orig, new)
                d = np.abs(got[r].astype(np.float64) - want[r].astype(np.float64))
                assert (d <= W.bound_factor(orig, new) * a).all(), (n, orig, new)
                worst = max(worst, float((d[a > 0] / (W.bound_factor(orig, new) * a[a > 0])).max()))
            print(f"n = {n}, ({orig}, {new}): {differ} of {got.size} samples differ from cough_resample; worst {worst:.3f} of the bound")


def test_plans_the_kernel_cannot_use_are_harmless():
    rows = _rows([16000, 16000, 5000, 257, 4097, 300, 300, 20000], seed=17)
    data, offs, lens, _ = _pack(rows)
    plans = [(3, 0, 16000), (0, 16000, -1), (-7, 5, 1), (2, 1, 5), (0, 2**20 + 1, 2**20), (0, -2**31, 2**31 - 1),
             (0, 9, 10), (0, 9, 10)]
    out, new_lens, intact = _warp_guarded(data, offs, lens, plans, 16000)
    assert intact and new_lens.tolist() == [16000, 16000, 5000, 257, 4097, 300, 334, 16000]
    for r in range(6):                                                     # each counts as orig == new: a shifted copy
        n = rows[r].numel()
        assert (out[r, :n] == W.shifted(rows[r].numpy(), plans[r][0])).all() and not out[r, n:].any(), r
    # lengths: negative and zero give an empty row; an over-long one is clamped and only read as far as the output needs
    bad = torch.tensor([-3, 0, 5, 257, 2**31 - 1, 300, 300, 2**31 - 1], dtype=torch.int32).cuda()
    offs2 = offs.clone()
    offs2[4] = offs[0]                                                     # 16000 legal samples, then junk, then row 1
    offs2[7] = offs[7]
    plans2 = [(0, 9, 10), (0, 1, 1), (0, 1, 1), (0, 1, 1), (0, 1, 1), (0, 1, 1), (0, 9, 10), (0, 10, 9)]
    out, new_lens, intact = _warp_guarded(data, offs2, bad, plans2, 16000)
    assert intact and new_lens.tolist() == [0, 0, 5, 257, 16000, 300, 334, 16000]
    assert not out[0].any() and not out[1].any() and not out[2, 5:].any()
    assert (out[4] == rows[0].numpy()).all()
    y_ref, a, _ = W.warp_ref(rows[7].numpy(), 0, 10, 9)                     # reads 17786 of the row's 20000 samples
    assert _inside(out[7, :15990], y_ref[:15990], a[:15990], 10, 9) <= 1.0
    assert np.isfinite(out).all() and np.abs(out).max() < 10.0


def test_tone_on_the_device():
    sr, n = 16000, 4096
    x = torch.from_numpy((0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)).astype(np.float32)).cuda()
    y, n_new = cda.warp_rows(x, torch.zeros(1, dtype=torch.int64).cuda(), torch.tensor([n], dtype=torch.int32).cuda(),
                             torch.tensor([[0, 9, 10]], dtype=torch.int32).cuda(), 4552, return_lengths=True)
    assert n_new.tolist() == [4552]
    y = y[0].cpu().numpy().astype(np.float64)
    peak_hz = np.abs(np.fft.rfft(y * np.hanning(4552))).argmax() * sr / 4552
    rms = np.sqrt((y[100:-100] ** 2).mean()) / np.sqrt((x[100:-100].cpu().numpy().astype(np.float64) ** 2).mean())
    print(f"tone on the device: peak at {peak_hz:.1f} Hz, rms ratio {rms:.5f}")
    assert abs(peak_hz - 900.0) <= sr / 4552 and abs(rms - 1.0) <= 1e-3


# ------------------------------------------------------------------------------------------------ 2. the draws
@pytest.mark.parametrize("b", [1, 64, 65])                                 # one thread; a full block; a block with one thread
def test_speed_draws_equal_the_restatement(b):
    pool = [0, 1, 2, 399, 16000, 16257, 48000, 2**31 - 1]
    lengths = [pool[(5 * i + b) % len(pool)] for i in range(b)]
    lens = torch.tensor(lengths, dtype=torch.int32).cuda()
    case, mixed = 0, set()
    for p in (0.0, 0.5, 1.0):
        for (lo, hi), sr in (((0.9, 1.1), 16000), ((0.25, 4.0), 16000), ((0.95, 0.95), 22050), ((1.0, 1.2), 2**19)):
            case += 1
            seed = (case * 0x9E3779B97F4A7C15 + b) & (2**64 - 1)           # both key words in use
            plans, new_lens = cda.draw_speed(seed, lens, p, (lo, hi), sr)
            want_plans, want_lens, fired = W.draw_speed_ref(seed, lengths, p, lo, hi, sr)
            assert plans.dtype == new_lens.dtype == torch.int32 and tuple(plans.shape) == (b, 3)
            assert (plans.cpu().numpy() == want_plans).all(), (p, lo, hi, sr, np.argwhere(plans.cpu().numpy() != want_plans)[:5])
            assert (new_lens.cpu().numpy() == want_lens).all(), (p, lo, hi, sr)
            mixed |= {k for k, f in fired.items() if f.any() and not f.all()}
            # the shift is the one the batch's record carries
            clips, _, _ = R.draw_ref(seed, np.minimum(lengths, 2**30), p, [], None, 0, 0, 0, 0, 90, 101)
            assert (clips["shift"] == want_plans[:, 0]).all()
    if b > 1:
        assert mixed == {"shift", "speed"}
    # clear_shifts zeroes the shift word of each record and nothing else
    aug = cda.AudioAugmentor(p_augment=1.0)
    clips, _ = cda.draw_batch(5, torch.full((b,), 16000, dtype=torch.int32).cuda(), aug, None, (90, 101))
    before = np.frombuffer(clips.cpu().numpy().tobytes(), dtype=R.CLIP_DTYPE).copy()
    cwarp.clear_shifts(clips)
    after = np.frombuffer(clips.cpu().numpy().tobytes(), dtype=R.CLIP_DTYPE).copy()
    assert before["shift"].any() and not after["shift"].any()
    before["shift"] = 0
    assert before.tobytes() == after.tobytes()


# ------------------------------------------------------------------------------------------------ 3. the chain
def _augmentor(p, speed=True, n_bank=3):
    g = torch.Generator().manual_seed(11)
    aug = cda.AudioAugmentor(p_augment=p, speed=speed)
    aug.noise_samples = [torch.randn((1, n), generator=g) * 0.3 for n in BANK[:n_bank]]
    aug._pack_bank()
    return aug


CHAIN_LENGTHS = [1, 2, 257, 4097, 16000, 9000, 16257, 700]


@pytest.mark.parametrize("p", [1.0, 0.5])
def test_augment_batch_equals_augment_clip_by_clip(p):
    rows = _rows(CHAIN_LENGTHS, seed=5)
    n = max(CHAIN_LENGTHS)
    x = torch.zeros((len(rows), n))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    aug = _augmentor(p)
    random.seed(31)
    torch.manual_seed(31)
    got, got_lens = aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="host", return_lengths=True)
    random.seed(31)
    torch.manual_seed(31)
    singles = [aug.augment(row[None].cuda()) for row in rows]
    assert got_lens.dtype == torch.int32 and got_lens.tolist() == [s.shape[1] for s in singles]
    assert tuple(got.shape) == (len(rows), max(got_lens.tolist())) and got.is_cuda
    for r, s in enumerate(singles):
        assert torch.equal(got[r, :s.shape[1]], s[0]), r
        assert not got[r, s.shape[1]:].any(), r
    if p == 1.0:
        assert got_lens.tolist() != CHAIN_LENGTHS                          # the speed step changed lengths
    # the composition spelled out: warp (shift + speed), then cough_augment_waveforms on zero-shift records
    random.seed(31)
    items = [aug.draw_item(v) for v in CHAIN_LENGTHS]
    assert [it[2] for it in items] == got_lens.tolist()
    plans = cwarp.plan_array([(c.shift,) + (pair or (1, 1)) for c, pair, _ in items])
    if p == 1.0:
        assert plans[:, 0].any()
    warped = cda.warp_rows(x.cuda(), (torch.arange(len(rows), dtype=torch.int64) * n).cuda(),
                           torch.tensor(CHAIN_LENGTHS, dtype=torch.int32).cuda(), torch.from_numpy(plans).cuda(), got.shape[1])
    clips = [_lib.CoughAugClip.from_buffer_copy(c) for c, _, _ in items]
    for c in clips:
        c.shift = 0
    seed = 0xABCDEF12345
    want = aug._run(warped, clips, got_lens.tolist(), None, seed)
    random.seed(31)
    assert torch.equal(aug.augment_batch(x.cuda(), lengths=CHAIN_LENGTHS, noise="device", seed=seed), want)
    # speed_perturbation alone: the resampler without a shift
    random.seed(8)
    y = aug.speed_perturbation(rows[3][None].cuda())
    random.seed(8)
    fired = not (random.random() > p)
    if fired:
        pair = cwarp.speed_rate_pair(random.uniform(0.9, 1.1), 16000)
        y_ref, a, n_new = W.warp_ref(rows[3].numpy(), 0, *pair)
        assert tuple(y.shape) == (1, n_new) and _inside(y[0].cpu().numpy(), y_ref, a, *pair) <= 1.0
    else:
        assert y.shape == (1, 4097)


def test_speed_off_is_todays_output():
    rows = _rows(CHAIN_LENGTHS, seed=5)
    n = max(CHAIN_LENGTHS)
    x = torch.zeros((len(rows), n))
    for r, row in enumerate(rows):
        x[r, :row.numel()] = row
    aug = _augmentor(0.7, speed=False)
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


def test_a_host_drawn_batch_equals_its_items_one_at_a_time(clip_bank, pre):
    bank, lengths = clip_bank
    loader = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=_augmentor(0.6), spec_augmentor=cda.SpecAugment(p=0.5),
                                  noise="host", generator=torch.Generator().manual_seed(1))
    warped = 0
    for k in range(3):
        indices = [(7 * k + 5 * i) % 24 for i in range(6)]
        random.seed(100 + k)
        torch.manual_seed(100 + k)
        plan = loader.draw_batch(indices)
        feats, targets = loader.launch_batch(indices, plan)
        assert tuple(feats.shape) == (6, 1, 90, 101) and torch.isfinite(feats).all()
        warped += plan.warps()
        for r, i in enumerate(indices):
            one = BatchPlan(clips=[plan.clips[r]], gaussian=plan.gaussian[r:r + 1].contiguous(), seed=plan.seed,
                            masks=[plan.masks[r]], pairs=[plan.pairs[r]], new_lengths=[plan.new_lengths[r]])
            f, t = loader.launch_batch([i], one)
            assert torch.equal(f[0], feats[r]) and torch.equal(t[0], targets[r]), (k, r)
    assert warped >= 2
    # against the same loader without the speed step: other features where a speed coin fired
    plain = cda.DeviceDataLoader(bank, pre, batch_size=6, audio_augmentor=_augmentor(0.6, speed=False), noise="host")
    random.seed(100)
    torch.manual_seed(100)
    assert not plain.draw_batch([0, 5, 10, 15, 20, 1]).warps()


def _restated_plan(seed, lengths, aug, spec, shape):
    """The BatchPlan that holds the restated draws of ``seed`` with the speed step."""
    plans, new_lens, fired = W.draw_speed_ref(seed, lengths, aug.p_augment, aug.speed_range[0], aug.speed_range[1], aug.sample_rate)
    n_f, n_t = (spec.n_freq_masks, spec.n_time_masks) if spec is not None else (0, 0)
    clips, masks, f = R.draw_ref(seed, new_lens, aug.p_augment, aug._bank_lengths, spec.p if spec is not None else None, n_f,
                                 spec.freq_mask_param if spec else 0, n_t, spec.time_mask_param if spec else 0, *shape)
    clips["shift"] = plans[:, 0]                                           # drawn for the original length
    plan = BatchPlan(seed=seed, pairs=[(int(o), int(m)) for _, o, m in plans], new_lengths=[int(v) for v in new_lens])
    plan.clips = [_lib.CoughAugClip(shift=int(r["shift"]), gain=float(r["gain"]), gaussian=int(r["gaussian"]),
                                    bank_index=int(r["bank_index"]), gaussian_snr_db=float(r["gaussian_snr_db"]),
                                    bank_snr_db=float(r["bank_snr_db"]), bank_start=int(r["bank_start"])) for r in clips]
    if masks is not None:
        plan.masks = [[tuple(int(v) for v in masks[:, r, m]) for m in range(n_f + n_t)] if f["spec"][r] else []
                      for r in range(len(lengths))]
    return plan, fired


def test_launch_batch_drawn_equals_launch_batch_on_the_restated_plan(clip_bank, pre, monkeypatch):
    bank, lengths = clip_bank
    aug, spec = _augmentor(0.5), cda.SpecAugment(p=0.5)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=8, audio_augmentor=aug, spec_augmentor=spec, draws="device",
                                  generator=torch.Generator().manual_seed(1))
    sped = 0
    for k, seed in enumerate((7, 2**63 + 12345, 2**64 - 1)):
        indices = [(11 * k + 3 * i) % 24 for i in range(8)]
        feats, targets = loader.launch_batch_drawn(indices, seed)
        plan, fired = _restated_plan(seed, [lengths[i] for i in indices], aug, spec, loader.feature_shape())
        want, want_targets = loader.launch_batch(indices, plan)
        assert tuple(feats.shape) == (8, 1, 90, 101) and feats.is_cuda
        assert torch.equal(feats, want) and torch.equal(targets, want_targets), (k, seed)
        sped += int(fired["speed"].sum())
    assert 0 < sped < 24                                                   # rows with and without a speed step
    monkeypatch.setattr(cda.DeviceDataLoader, "draw_batch", lambda *a: pytest.fail("draw_batch was called"))
    assert len(list(loader)) == 3 == len(loader)


def test_epochs_repeat_with_the_generator_seed(clip_bank, pre):
    bank, _ = clip_bank

    def run(seed, draws):
        ld = cda.DeviceDataLoader(bank, pre, batch_size=8, audio_augmentor=_augmentor(0.5), spec_augmentor=cda.SpecAugment(p=0.5),
                                  draws=draws, generator=torch.Generator().manual_seed(seed))
        random.seed(seed)
        torch.manual_seed(seed)
        return [[(f.clone(), t.clone()) for f, t in ld] for _ in range(2)]

    for draws in ("device", "host"):
        a, b, c = run(6, draws), run(6, draws), run(9, draws)
        for ea, eb in zip(a, b):
            assert len(ea) == 3
            for (fa, ta), (fb, tb) in zip(ea, eb):
                assert torch.equal(fa, fb) and torch.equal(ta, tb) and torch.isfinite(fa).all()
        assert any(not torch.equal(fa, fb) for (fa, _), (fb, _) in zip(a[0], a[1])), draws
        assert any(not torch.equal(fa, fc) for (fa, _), (fc, _) in zip(a[0], c[0])), draws


@pytest.mark.parametrize("draws", ["host", "device"])
def test_fit_runs_with_speed_and_mixup(tmp_path, clip_bank, pre, draws):
    bank, _ = clip_bank
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    train, val = cda.create_data_loaders(bank, bank, pre, batch_size=8, audio_augmentor=_augmentor(0.8),
                                         spec_augmentor=cda.SpecAugment(p=0.5), mixup=cda.MixUp(0.2),
                                         generator=torch.Generator().manual_seed(8), draws=draws)
    assert train.audio_augmentor.speed and val.audio_augmentor is None
    plain = cda.DeviceDataLoader(bank, pre, batch_size=8, is_training=False)
    for (fa, ta), (fb, tb) in zip(val, plain):                             # validation is unaffected
        assert torch.equal(fa, fb) and torch.equal(ta, tb)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1, compute_dtype="fp32")
    tr = SmallTrainer(model, class_weights=cda.class_weights_from_counts(bank.class_counts), seed=5)
    res = cda.fit(tr, train, val, str(tmp_path), epochs=1, patience=5, config=dict(CONFIG))
    print(f"fit with speed=True, MixUp, draws={draws!r}:", res["history"])
    h = res["history"][0]
    assert res["epochs_run"] == 1 and h["train"]["loss"] == h["train"]["loss"] and h["val"]["loss"] == h["val"]["loss"]
    assert h["val"]["tp"] + h["val"]["fp"] + h["val"]["fn"] + h["val"]["tn"] == 24
