"""Speed perturbation without a GPU: the restatement of the resampler's arithmetic (tests/warp_ref.py) against the shipped
polyphase table and a tone, the eighth library's symbols and argument checks, the build's staleness rule, the speed
draw's restatement and the ``n'`` arithmetic, and the Python surface's defaults."""
import ctypes as C
import math
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib, _tables
from cough_detector_amd import build as cbuild
from cough_detector_amd import warp as cwarp
import warp_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_warp.h")
TABLE_PAIRS = [(9, 10), (10, 9), (147, 160), (160, 147), (11, 10), (1, 2), (2, 1)]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("orig,new", TABLE_PAIRS)
def test_coefficients_equal_the_shipped_table_bit_for_bit(orig, new):
    kern, width, o, n = _tables.sinc_resample_kernel(orig, new)
    assert (o, n) == (orig, new) and width == W.filter_width(orig, new)
    phase, k = np.arange(new)[:, None], np.arange(2 * width + orig)[None, :]
    num = (k - width) * new - phase * orig                     # input blk * orig - width + k, output blk * new + phase
    want = kern.numpy().view(np.uint32)
    assert (W.coefficient(num, orig, new).view(np.uint32) == want).all()
    # the formula is homogeneous in (orig, new): an unreduced pair gives the same bits
    for scale in (3, 1600):
        assert W.filter_width(scale * orig, scale * new) == width
        assert (W.coefficient(scale * num, scale * orig, scale * new).view(np.uint32) == want).all(), scale
    # taps the kernel skips (|t| >= 6) are exactly zero in the table, and every non-zero one lies in the kernel's range
    t = np.abs(num * (min(orig, new) * 0.99 / (orig * new)))
    assert not kern.numpy()[t >= 6.0].any()
    centre = phase * orig // new
    assert ((k - width >= centre - width) & (k - width <= centre + width + 1))[kern.numpy() != 0].all()


def test_restatement_equals_the_table_convolution():
    # the whole row: torch's CPU convolution with the shipped table, torchaudio's own algorithm, sits well inside the bound
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(257, generator=g) - 0.5)
    for orig, new in ((9, 10), (10, 9), (147, 160)):
        kern, width, _, _ = _tables.sinc_resample_kernel(orig, new)
        padded = torch.nn.functional.pad(x[None, None], (width, width + orig))
        y = torch.nn.functional.conv1d(padded, kern[:, None], stride=orig).transpose(1, 2).reshape(-1)
        y_ref, a, n_new = W.warp_ref(x.numpy(), 0, orig, new)
        assert n_new == math.ceil(new * 257 / orig)
        ratio = np.abs(y[:n_new].numpy() - y_ref) / (W.bound_factor(orig, new) * a)
        print(f"({orig}, {new}): conv1d with the table sits at {ratio.max():.3f} of the bound")
        assert ratio.max() <= 1.0


def test_tone_keeps_its_level_and_moves_its_pitch():
    sr, n = 16000, 4096
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)).astype(np.float32)
    y, _, n_new = W.warp_ref(x, 0, 9, 10)
    assert n_new == 4552 == y.size
    spectrum = np.abs(np.fft.rfft(y * np.hanning(n_new)))
    peak_hz = spectrum.argmax() * sr / n_new
    rms = np.sqrt((y[100:-100] ** 2).mean()) / np.sqrt((x[100:-100].astype(np.float64) ** 2).mean())
    print(f"tone: peak at {peak_hz:.1f} Hz, rms ratio {rms:.5f}")
    assert abs(peak_hz - 900.0) <= sr / n_new and abs(rms - 1.0) <= 1e-3


def test_new_length_arithmetic():
    assert W.new_length(4096, 9, 10) == 4552 and W.new_length(16000, 15999, 16000) == 16002
    assert W.new_length(16000, 17599, 16000) == 14547 and W.new_length(1, 4, 1) == 1 and W.new_length(1, 1, 4) == 4
    assert W.new_length(2**30, 1, 4) == 2**32 and W.new_length(0, 9, 10) == 0
    for n, o, m in ((13, 9, 10), (48000, 14400, 16000), (255, 10, 9), (2**30, 2**20 - 1, 2**20)):
        assert cwarp.warped_length(n, o, m) == W.new_length(n, o, m) == -((-n * m) // o)      # exact, not float
    assert cwarp.warped_length(100, 0, 16000) == 100 and cwarp.warped_length(100, 16000, 3999) == 100   # unusable: a copy
    assert cwarp.warped_length(-5, 9, 10) == 0 and cwarp.warped_length(2**31, 1, 1) == 2**30
    assert cwarp.speed_rate_pair(0.9, 16000) == (14400, 16000) and cwarp.speed_rate_pair(1.0999999, 16000) == (17599, 16000)
    assert cwarp.speed_rate_pair(0.99999, 16000) == (15999, 16000)
    assert W.filter_width(4, 1) == 25 and W.filter_width(1, 4) == 7 and W.filter_width(17599, 16000) == 7
    assert cwarp.drawn_width(16000, (0.9, 1.1), 16000) == 17778 and cwarp.drawn_width(16000, (1.1, 1.2), 16000) == 16000
    x = np.arange(1.0, 6.0, dtype=np.float32)
    assert W.shifted(x, 2).tolist() == [0, 0, 1, 2, 3] and W.shifted(x, -1).tolist() == [2, 3, 4, 5, 0]
    assert not W.shifted(x, 5).any() and not W.shifted(x, -2**31).any() and W.shifted(x, 0).tolist() == x.tolist()


def test_distributions_of_the_speed_draw_restatement():
    N, p, sr = 200_000, 0.3, 16000
    plans, n_new, fired = W.draw_speed_ref(20261019, np.full(N, 16000), p, 0.9, 1.1, sr)
    bound = 5.0 * math.sqrt(p * (1.0 - p) / N)                             # 5 binomial standard deviations
    for name, f in fired.items():
        assert abs(float(f.mean()) - p) <= bound, (name, float(f.mean()))
    both = float((fired["shift"] & fired["speed"]).mean())                 # separate draws: independent coins
    assert abs(both - p * p) <= 5.0 * math.sqrt(p * p * (1 - p * p) / N), both
    # the shift is slot 0 of the batch's record: the same values tests/draws_ref.py draws
    import draws_ref as D
    clips, _, f = D.draw_ref(20261019, np.full(N, 16000), p, [], None, 0, 0, 0, 0, 90, 101)
    assert (clips["shift"] == plans[:, 0]).all() and (f["shift"] == fired["shift"]).all()
    orig, fs = plans[:, 1], fired["speed"]
    assert (plans[:, 2] == sr).all() and (orig[~fs] == sr).all()
    assert orig[fs].min() >= 14400 and orig[fs].max() <= 17599 and orig[fs].min() < 14410 and orig[fs].max() > 17590
    mean, sd = orig[fs].mean(), 3200 / math.sqrt(12)                       # uniform over a range of 3200
    assert abs(mean - 15999.5) <= 5.0 * sd / math.sqrt(fs.sum()), mean
    assert (n_new == (16000 * sr + orig.astype(np.int64) - 1) // orig).all() and (n_new[~fs] == 16000).all()
    assert n_new.min() == W.new_length(16000, orig.max(), sr) and n_new.max() <= cwarp.drawn_width(16000, (0.9, 1.1), sr)
    for p_end, want in ((0.0, False), (1.0, True)):
        _, _, f = W.draw_speed_ref(5, np.full(1000, 800), p_end, 0.9, 1.1, sr)
        assert f["speed"].all() == want and f["speed"].any() == want
    plans, n_new, f = W.draw_speed_ref(5, [0, -3, 1, 2**31 - 1], 1.0, 0.9, 1.1, sr)     # blank rows; an over-long one
    assert plans[:2].tolist() == [[0, sr, sr]] * 2 and n_new[:2].tolist() == [0, 0] and not f["speed"][:2].any()
    assert n_new[2] in (1, 2) and n_new[3] == 2**30


# ------------------------------------------------------------------------------------------------ the library
def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_warp_library_exports_exactly_its_header():
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|size_t|const char\*) (cough_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert declared == set(_lib.WARP_SYMBOLS), declared ^ set(_lib.WARP_SYMBOLS)
    assert len(_lib.WARP_SYMBOLS) == len(set(_lib.WARP_SYMBOLS)) == 5
    lib = _lib.load_warp()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_warp_abi_version() == 1 and "#define COUGH_WARP_ABI_VERSION 1" in text
    assert _exported(_lib.WARP_LIB_PATH) == declared
    assert C.sizeof(_lib.CoughWarpPlan) == 12 == 4 * cwarp.PLAN_WORDS
    assert [f[0] for f in _lib.CoughWarpPlan._fields_] == ["shift", "orig", "new_rate"]
    assert f"#define COUGH_WARP_MAX_RATE (1 << 20)" in text and _lib.WARP_MAX_RATE == W.MAX_RATE == 1 << 20
    assert "#define COUGH_WARP_MAX_RATIO 4" in text and _lib.WARP_MAX_RATIO == W.MAX_RATIO == 4


def test_the_other_seven_libraries_are_untouched():
    others = (("cough_amd.h", "SYMBOLS", 53, "LIB_PATH"), ("cough_amd_loop.h", "LOOP_SYMBOLS", 3, "LOOP_LIB_PATH"),
              ("cough_amd_data.h", "DATA_SYMBOLS", 5, "DATA_LIB_PATH"),
              ("cough_amd_segments.h", "SEGMENTS_SYMBOLS", 6, "SEGMENTS_LIB_PATH"),
              ("cough_amd_score.h", "SCORE_SYMBOLS", 5, "SCORE_LIB_PATH"), ("cough_amd_draws.h", "DRAWS_SYMBOLS", 5, "DRAWS_LIB_PATH"),
              ("cough_amd_soft.h", "SOFT_SYMBOLS", 6, "SOFT_LIB_PATH"))
    for header, names, count, path in others:
        syms = getattr(_lib, names)
        assert len(syms) == count and not set(syms) & set(_lib.WARP_SYMBOLS), header
        assert _exported(getattr(_lib, path)) == set(syms), header
        text = open(os.path.join(ROOT, "include", header)).read()
        for s in _lib.WARP_SYMBOLS:
            assert s not in text, (header, s)
    assert _lib.load().cough_amd_abi_version() == 5 and _lib.load_draws().cough_draws_abi_version() == 1


def test_the_augment_kernel_header_is_as_it_was():
    text = open(os.path.join(cbuild.CSRC, "augment_kernel.h")).read()
    assert "speed_perturbation is the identity" in text       # the resampler runs before it, with its shift; it is unchanged
    assert "augment_kernel" not in open(os.path.join(cbuild.CSRC, "warp.hip")).read()


FAKE = 1 << 20


def _err():
    return _lib.load_warp().cough_warp_last_error()


def test_warp_rows_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_warp()

    def call(src=FAKE, offs=FAKE, lens=FAKE, n=3, plans=FAKE, out=2 * FAKE, samples=16000, nlens=FAKE):
        return lib.cough_warp_rows(src, offs, lens, n, plans, out, samples, nlens, None)

    E = _lib.EINVAL
    for kw in ("src", "offs", "lens", "plans", "out"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_warp_rows" in _err(), kw
    for kw, v in (("n", -1), ("samples", 0), ("samples", -4)):
        assert call(**{kw: v}) == E and b"bad sizes" in _err(), (kw, v)
    assert call(samples=(1 << 30) + 1) == _lib.EUNSUPPORTED and b"2^30" in _err()
    assert call(n=(1 << 14) + 1, samples=1 << 20) == _lib.EUNSUPPORTED and b"2^24" in _err()     # rows x tiles: the grid
    assert call(out=FAKE) == E and b"alias" in _err()
    for kw in ("src", "lens", "plans", "out", "nlens"):
        assert call(**{kw: 8 * FAKE + 2}) == E and b"4-byte" in _err(), kw
    assert call(offs=FAKE + 4) == E and b"8-byte" in _err()
    assert call(n=0) == _lib.OK and call(n=0, src=None, out=None, plans=None) == _lib.OK
    with pytest.raises(ValueError, match="cough_warp_rows: .*bad sizes"):
        _lib.check_warp(call(samples=0), "cough_warp_rows")
    assert b"bad sizes" not in _lib.load_draws().cough_draws_last_error()     # the messages stay apart


def test_draw_speed_and_clear_shifts_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load_warp()

    def call(seed=1, n=4, lens=FAKE, p=0.5, lo=0.9, hi=1.1, sr=16000, plans=FAKE, nlens=FAKE):
        return lib.cough_draw_speed(seed, n, lens, p, lo, hi, sr, plans, nlens, None)

    E = _lib.EINVAL
    for kw in ("lens", "plans", "nlens"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_draw_speed" in _err(), kw
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err(), kw
    assert call(n=-1) == E and b"n_rows" in _err()
    for p in (-0.1, 1.5, math.nan):
        assert call(p=p) == E and b"p_augment" in _err(), p
    for lo, hi in ((0.2, 1.1), (1.2, 1.1), (0.9, 4.5), (math.nan, 1.1), (0.9, math.nan)):
        assert call(lo=lo, hi=hi) == E and b"speed range" in _err(), (lo, hi)
    for sr in (0, -16000, (1 << 20) + 1):
        assert call(sr=sr) == E and b"sample_rate" in _err(), sr
    assert call(hi=1.2, sr=1 << 20) == E and b"below 2^20" in _err()        # orig would pass the largest rate
    assert call(lo=0.25, sr=16001) == E and b"quarter" in _err()            # (int)(0.25 * 16001) = 4000 < 16001 / 4
    assert call(n=0, lo=0.25, sr=16000) == _lib.OK                        # a legal range (n = 0: nothing is launched)
    assert call(n=0) == _lib.OK and call(n=0, lens=None, plans=None, nlens=None) == _lib.OK
    assert lib.cough_clear_shifts(None, 3, None) == E and b"NULL" in _err()
    assert lib.cough_clear_shifts(FAKE + 4, 3, None) == E and b"8-byte" in _err()
    assert lib.cough_clear_shifts(FAKE, -1, None) == E and lib.cough_clear_shifts(None, 0, None) == _lib.OK


# ------------------------------------------------------------------------------------------------ the Python front
def test_the_package_exports_the_warp_functions():
    for name in ("warp_rows", "draw_speed", "speed_rate_pair"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cwarp, name), name
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.warp_rows(torch.zeros(8), torch.zeros(1, dtype=torch.int64), torch.tensor([8], dtype=torch.int32),
                      torch.tensor([[0, 9, 10]], dtype=torch.int32), 9)
    with pytest.raises(ValueError, match="int32"):
        cda.draw_speed(1, torch.tensor([800]), 0.5, (0.9, 1.1), 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.draw_speed(1, torch.tensor([800], dtype=torch.int32), 0.5, (0.9, 1.1), 16000)
    with pytest.raises(ValueError, match="speed_range"):
        cda.draw_speed(1, torch.tensor([800], dtype=torch.int32), 0.5, (0.1, 1.1), 16000)


def test_speed_is_opt_in_and_draws_nothing_by_default():
    aug = cda.AudioAugmentor(p_augment=1.0)
    assert aug.speed is False and aug.speed_range == (0.9, 1.1)
    x = torch.ones(1, 100)
    random.seed(4)
    state = random.getstate()
    assert aug.speed_perturbation(x) is x and random.getstate() == state   # the identity, and no draw
    # the record's draws are today's: shift, gain, gaussian (no bank), in that order
    random.seed(4)
    c, pair, n_new = aug.draw_item(16000)
    random.seed(4)
    shift = int(16000 * random.uniform(-0.2, 0.2)) if not (random.random() > 1.0) else 0
    gain = random.uniform(0.7, 1.3) if not (random.random() > 1.0) else None
    assert pair is None and n_new == 16000 and c.shift == shift and c.gain == np.float32(gain)
    random.seed(4)
    d = aug.draw_clip(16000)
    assert bytes(d) == bytes(c)
    for bad in ((0.1, 1.1), (1.2, 1.1), (0.9, 5.0)):
        with pytest.raises(ValueError, match="speed_range"):
            cda.AudioAugmentor(speed=True, speed_range=bad)
    cda.AudioAugmentor(speed=False, speed_range=(0.1, 9.0))                # not looked at while the step is off
    a, s = cda.create_augmentation_pipeline(p_augment=0.3, speed=True, speed_range=(0.95, 1.05))
    assert a.speed and a.speed_range == (0.95, 1.05) and s.p == 0.3
    assert cda.create_augmentation_pipeline()[0].speed is False


def test_draw_item_puts_the_speed_draws_between_shift_and_gain():
    aug = cda.AudioAugmentor(p_augment=1.0, speed=True)
    aug.noise_samples = [torch.zeros(1, 700), torch.zeros(1, 20000)]
    aug._pack_bank()
    random.seed(9)
    c, pair, n_new = aug.draw_item(16000)
    random.seed(9)
    random.random()
    shift = int(16000 * random.uniform(-0.2, 0.2))
    random.random()
    want_pair = cwarp.speed_rate_pair(random.uniform(0.9, 1.1), 16000)
    random.random()
    gain = random.uniform(0.7, 1.3)
    random.random()
    snr = random.uniform(10, 30)
    random.random()
    k = random.choice(range(2))
    want_n = cwarp.warped_length(16000, *want_pair)
    rep = 700 * (want_n // 700 + 1) if k == 0 else 20000
    start = random.randint(0, rep - want_n)                                # the crop is drawn for the warped length
    assert pair == want_pair and n_new == want_n != 16000 and c.shift == shift and c.gain == np.float32(gain)
    assert c.gaussian == 1 and c.gaussian_snr_db == snr and (c.bank_index, c.bank_start) == (k, start)
    aug.p_augment = 0.0
    assert aug.draw_item(800)[1:] == (None, 800) and aug.speed_perturbation(torch.ones(1, 8)).shape == (1, 8)


def test_the_loader_refuses_cached_features_with_a_speed_augmentor():
    bank = cda.DeviceClipBank([torch.zeros(800), torch.ones(20000)], [0, 1], device="cpu")
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
    with pytest.raises(ValueError, match="cache_features"):
        cda.DeviceDataLoader(bank, pre, audio_augmentor=cda.AudioAugmentor(speed=True), cache_features=True)
    loader = cda.DeviceDataLoader(bank, pre, batch_size=2, audio_augmentor=cda.AudioAugmentor(p_augment=1.0, speed=True),
                                  noise="host")
    random.seed(2)
    torch.manual_seed(2)
    plan = loader.draw_batch([0, 1])
    assert plan.warps() and len(plan.pairs) == 2 and plan.new_lengths == [cwarp.warped_length(n, *p)
                                                                          for n, p in zip((800, 20000), plan.pairs)]
    assert plan.gaussian.shape == (2, cwarp.drawn_width(20000, (0.9, 1.1), 16000))
    for r, n in enumerate(plan.new_lengths):                               # randn(n') per row, zeros behind
        assert plan.gaussian[r, :n].abs().sum() > 0 and not plan.gaussian[r, n:].any()
    plain = cda.DeviceDataLoader(bank, pre, batch_size=2, audio_augmentor=cda.AudioAugmentor(p_augment=1.0)).draw_batch([0, 1])
    assert plain.pairs is None and plain.new_lengths is None and not plain.warps()
    val = cda.DeviceDataLoader(bank, pre, batch_size=2, audio_augmentor=cda.AudioAugmentor(speed=True), is_training=False)
    assert val.draw_batch([0, 1]).clips is None
