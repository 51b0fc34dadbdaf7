"""Pitch shift without a GPU: the two restatements of the vocoder's arithmetic (tests/pitch_ref.py) against each other,
why the magnitude floor exists, the fitness of the GPU test's inputs, a tone, the ninth library's symbols and argument
checks, the build's staleness rule, the pitch draw's restatement, and the Python surface's defaults and draw order."""
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
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import pitch as cpitch
from cough_detector_amd import warp as cwarp
import pitch_ref as P
import warp_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_pitch.h")


def _stretched():
    """The GPU test's rows that the kernel stretches and that are neither silent nor poisoned."""
    return [(name, x, shift, rate, ref) for name, x, shift, rate, ref in P.case_refs()
            if P.stretchable(rate, x.size) and ref["peak"] > 0.0]


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_two_restatements_agree_on_every_input():
    rows = _stretched()
    assert len(rows) >= 20
    for name, x, shift, rate, ref in rows:
        angle = P.stretch_ref(x, shift, rate, form="angle")
        peak = np.abs(ref["y"]).max()
        worst = np.abs(angle["y"] - ref["y"]).max() / peak
        print(f"{name}: angle / cumsum against phasor product: {worst:.2e} of the peak")
        assert angle["n_s"] == ref["n_s"] == ref["y"].size and worst <= 1e-9, name


def test_a_perturbed_spectrum_stays_inside_the_bound_and_the_floor_is_why():
    for k, (name, x, shift, rate, ref) in enumerate(_stretched()):
        moved = P.stretch_ref(x, shift, rate, perturb=P.perturbation(x, shift, 4.0, seed=k))
        assert (np.abs(moved["y"] - ref["y"]) <= ref["E"]).all(), name
    # the same perturbation without the floor: a burst between exact zeros moves by a good part of its peak, so the
    # unfloored formula is not a function of the input that two implementations can agree on
    seen = 0
    for k, (name, x, shift, rate, ref) in enumerate(_stretched()):
        if "burst" not in name or x.size < 16000:
            continue
        plain = P.stretch_ref(x, shift, rate, floor=False)
        moved = P.stretch_ref(x, shift, rate, floor=False, perturb=P.perturbation(x, shift, 4.0, seed=k))
        ratio = np.abs(moved["y"] - plain["y"]).max() / np.abs(plain["y"]).max()
        print(f"{name}: without the floor the perturbation moves the output by {ratio:.2f} of its peak")
        assert ratio > 0.1, name
        seen += 1
    assert seen >= 3


def test_the_inputs_are_fit_for_a_comparison():
    for name, x, shift, rate, ref in _stretched():
        peak = np.abs(ref["y"]).max()
        below = float((ref["E"] <= 2.0 ** -24 * peak).mean())
        print(f"{name}: floor margin {ref['margin']:.1e}, max E {ref['E'].max() / peak:.1e} of the peak, "
              f"{100 * below:.1f} % of the row at or below 2^-24")
        assert ref["margin"] >= 64.0, name
        assert (ref["E"] <= 2.0 ** -20 * peak).all(), name
        assert below >= 0.9, name
        assert ref["env_min"] >= 0.25, name                                # the summed squared window over the kept range


def test_lengths_and_special_rows_of_the_restatement():
    assert P.stretched_length(16000, P.R1) == 15102 and P.stretched_length(16000, 1 / P.R1) == 16951
    assert P.stretched_length(257, 0.5) == 514 and P.stretched_length(256, 0.5) == 256 and P.stretched_length(1000, 3.0) == 1000
    assert P.stretched_length(1000, float("nan")) == 1000 and P.stretched_length(2**21, 0.5) == 2**21
    assert P.stretched_length(5, 2.0) == 5 and P.stretched_length(301, 2.0) == 150 and P.stretched_length(303, 2.0) == 152   # half to even
    for n, rate in ((16000, P.R1), (257, 0.5), (100, 0.5), (-3, 2.0), (2**22, 0.5), (1000, 1.0), (1000, 2.5)):
        assert cpitch.stretched_length(n, rate) == P.stretched_length(n, rate), (n, rate)
    refs = {name: (x, shift, rate, ref) for name, x, shift, rate, ref in P.case_refs()}
    for name in ("1000 rate 1", "1000 rate 3", "1000 rate nan", "256", "256 shifted", "one"):
        x, shift, rate, ref = refs[name]
        assert ref["n_s"] == x.size and (ref["y"] == W.shifted(x, shift)).all(), name
    for name in ("1000 zeros", "1000 shifted out", "1000 shifted out left"):
        assert refs[name][3]["n_s"] != 1000 and not refs[name][3]["y"].any(), name
    for name in ("1000 nan", "16000 inf"):
        assert np.isnan(refs[name][3]["y"]).all() and refs[name][3]["y"].size == P.stretched_length(refs[name][0].size, refs[name][2])
    x, shift, rate, ref = refs["1000 inf copied"]
    assert ref["n_s"] == 1000 and np.isinf(ref["y"][998])                  # rate 1: a copy, whatever it holds
    assert cpitch.pitch_rate(0) == 1.0 and cpitch.pitch_rate(12) == 0.5 and cpitch.pitch_rate(-12) == 2.0
    assert cpitch.pitch_rate_pair(1, 16000) == (16951, 16000) and cpitch.pitch_rate_pair(-2, 16000) == (14254, 16000)
    assert cpitch.pitch_rate_pair(12, 16000) == (32000, 16000) and cpitch.pitch_rate_pair(-12, 16000) == (8000, 16000)
    assert cpitch.drawn_width(16000, (-2, 2)) == P.stretched_length(16000, 2.0 ** (-2 / 12)) == 17959
    assert cpitch.drawn_width(16000, (-2, -1)) == 16000 and cpitch.drawn_width(100, (-2, 2)) == 100


def test_a_tone_moves_up_two_semitones():
    sr, n = 16000, 16000
    x = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)).astype(np.float32)
    y = P.pitch_shift_ref(x, 2, sr)
    assert y.size == n
    spectrum = np.abs(np.fft.rfft(y * np.hanning(n)))
    peak_hz = spectrum.argmax() * sr / n
    rms = np.sqrt((y[1000:-1000] ** 2).mean()) / np.sqrt((x[1000:-1000].astype(np.float64) ** 2).mean())
    print(f"tone: peak at {peak_hz:.1f} Hz (440 * 2^(2/12) = {440 * 2 ** (2 / 12):.1f}), rms ratio {rms:.4f}")
    # the level is not kept: the reflected start is not a stationary tone, the bins of the main lobe leave it with
    # other phase relations than a tone has, and a vocoder without phase locking never restores them (both restatements
    # give 0.597 here)
    assert abs(peak_hz - 493.9) <= sr / n and 0.4 <= rms <= 1.1


def test_distributions_of_the_pitch_draw_restatement():
    N, p, sr = 200_000, 0.3, 16000
    rates, plans, n_s, steps, fired = P.draw_pitch_ref(20261019, np.full(N, 16000), p, -2, 2, sr)
    assert abs(float(fired.mean()) - p) <= 5.0 * math.sqrt(p * (1.0 - p) / N)
    for s in range(-2, 3):                                                 # randint: every value with probability 1/5
        share = float((steps[fired] == s).mean())
        assert abs(share - 0.2) <= 5.0 * math.sqrt(0.2 * 0.8 / fired.sum()), (s, share)
    assert (steps[~fired] == 0).all() and steps.min() == -2 and steps.max() == 2
    idle = steps == 0
    assert (rates[idle] == 1.0).all() and (plans[idle] == [0, sr, sr]).all() and (n_s[idle] == 16000).all()
    for s in (-2, -1, 1, 2):
        sel = steps == s
        assert (rates[sel] == cpitch.pitch_rate(s)).all() and (plans[sel, 1] == cpitch.pitch_rate_pair(s, sr)[0]).all()
        assert (n_s[sel] == cpitch.stretched_length(16000, cpitch.pitch_rate(s))).all()
    # independent of the speed coin of the same rows
    _, _, f = W.draw_speed_ref(20261019, np.full(N, 16000), p, 0.9, 1.1, sr)
    both = float((fired & f["speed"]).mean())
    assert abs(both - p * p) <= 5.0 * math.sqrt(p * p * (1 - p * p) / N), both
    rates, plans, n_s, steps, fired = P.draw_pitch_ref(5, [0, -3, 100, 2**31 - 1], 1.0, 12, 12, sr)   # blank, short, over-long
    assert rates.tolist() == [1.0, 1.0, 0.5, 0.5] and n_s.tolist() == [0, 0, 100, 2**21] and fired.tolist() == [False, False, True, True]
    table = cpitch.step_table((-2, 2), sr).view(cpitch._STEP_DTYPE).reshape(-1)
    assert [(float(r), int(o)) for r, o, _ in table] == P.step_table(-2, 2, sr)


# ------------------------------------------------------------------------------------------------ the library
def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_pitch_library_exports_exactly_its_header():
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|size_t|const char\*) (cough_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert declared == set(_lib.PITCH_SYMBOLS), declared ^ set(_lib.PITCH_SYMBOLS)
    assert len(_lib.PITCH_SYMBOLS) == len(set(_lib.PITCH_SYMBOLS)) == 4
    lib = _lib.load_pitch()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.cough_pitch_abi_version() == 1 and "#define COUGH_PITCH_ABI_VERSION 1" in text
    assert _exported(_lib.PITCH_LIB_PATH) == declared
    assert C.sizeof(_lib.CoughStretchPlan) == 16 == cpitch.PLAN_BYTES == C.sizeof(_lib.CoughPitchStep)
    assert [f[0] for f in _lib.CoughStretchPlan._fields_] == ["shift", "reserved", "rate"]
    assert _lib.CoughStretchPlan.rate.offset == 8 and _lib.CoughPitchStep.orig.offset == 8
    assert cpitch.plan_array([(-5, 0.75)]).tobytes() == bytes(_lib.CoughStretchPlan(shift=-5, reserved=0, rate=0.75))
    assert "#define COUGH_PITCH_MAX_LENGTH (1 << 20)" in text and _lib.PITCH_MAX_LENGTH == P.MAX_LEN == 1 << 20
    assert "#define COUGH_PITCH_MAX_SAMPLES (1 << 21)" in text and _lib.PITCH_MAX_SAMPLES == 1 << 21
    assert "#define COUGH_PITCH_MAX_STEPS 12" in text and _lib.PITCH_MAX_STEPS == P.MAX_STEPS == 12
    assert "THIS HEADER IS THE CONTRACT" in text and "1/4" in text
    # the other libraries keep their symbols
    for names, path in ((_lib.WARP_SYMBOLS, _lib.WARP_LIB_PATH), (_lib.DRAWS_SYMBOLS, _lib.DRAWS_LIB_PATH),
                        (_lib.SOFT_SYMBOLS, _lib.SOFT_LIB_PATH), (_lib.SYMBOLS, _lib.LIB_PATH)):
        assert _exported(path) == set(names) and not set(names) & declared


def test_every_library_links_its_own_objects(monkeypatch, tmp_path):
    # the link step's slices of the object list: each library gets exactly the objects of its sources
    links = []

    def fake_run(cmd, check=True):
        if "-c" in cmd:
            return
        links.append((os.path.basename(cmd[cmd.index("-o") + 1]), [os.path.basename(a) for a in cmd if a.endswith(".o")]))

    monkeypatch.setattr(cbuild.subprocess, "run", fake_run)
    monkeypatch.setattr(cbuild, "OBJ", str(tmp_path))
    cbuild.build_library(force=True, verbose=False)
    got = dict(links)
    obj = lambda names: [n.replace(".hip", ".o") for n in names]           # noqa: E731
    assert got["libcough_amd.so"] == obj(cbuild.SOURCES) and got["libcough_amd_pitch.so"] == ["pitch.o"]
    assert got["libcough_amd_warp.so"] == ["warp.o"] and got["libcough_amd_draws.so"] == ["draws.o"]
    assert got["libcough_amd_soft.so"] == ["soft.o", "train_soft.o", "train_small_soft.o", "train_std_soft.o"]
    assert len(got) == 9 and sum(len(v) for v in got.values()) == 12 + 7 + 4


FAKE = 1 << 20


def _err():
    return _lib.load_pitch().cough_pitch_last_error()


def test_stretch_rows_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_pitch()

    def call(src=FAKE, offs=FAKE, lens=FAKE, n=3, plans=FAKE, out=2 * FAKE, samples=16000, nlens=FAKE):
        return lib.cough_stretch_rows(src, offs, lens, n, plans, out, samples, nlens, None)

    E = _lib.EINVAL
    for kw in ("src", "offs", "lens", "plans", "out"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_stretch_rows" in _err(), kw
    for kw, v in (("n", -1), ("samples", 0), ("samples", -4)):
        assert call(**{kw: v}) == E and b"bad sizes" in _err(), (kw, v)
    assert call(samples=(1 << 21) + 1) == _lib.EUNSUPPORTED and b"2^21" in _err()
    assert call(n=(1 << 24) + 1) == _lib.EUNSUPPORTED and b"2^24" in _err()
    assert call(out=FAKE) == E and b"alias" in _err()
    for kw in ("src", "lens", "out", "nlens"):
        assert call(**{kw: 8 * FAKE + 2}) == E and b"4-byte" in _err(), kw
    for kw in ("offs", "plans"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err(), kw
    assert call(n=0) == _lib.OK and call(n=0, src=None, out=None, plans=None) == _lib.OK
    with pytest.raises(ValueError, match="cough_stretch_rows: .*bad sizes"):
        _lib.check_pitch(call(samples=0), "cough_stretch_rows")
    assert b"bad sizes" not in _lib.load_warp().cough_warp_last_error()       # the messages stay apart


def test_draw_pitch_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load_pitch()

    def call(seed=1, n=4, lens=FAKE, p=0.5, lo=-2, hi=2, table=FAKE, sr=16000, stretch=FAKE, back=FAKE, nlens=FAKE):
        return lib.cough_draw_pitch(seed, n, lens, p, lo, hi, table, sr, stretch, back, nlens, None)

    E = _lib.EINVAL
    for kw in ("lens", "table", "stretch", "back", "nlens"):
        assert call(**{kw: None}) == E and b"NULL" in _err() and b"cough_draw_pitch" in _err(), kw
    for kw in ("lens", "back", "nlens"):
        assert call(**{kw: FAKE + 2}) == E and b"4-byte" in _err(), kw
    for kw in ("table", "stretch"):
        assert call(**{kw: FAKE + 4}) == E and b"8-byte" in _err(), kw
    assert call(n=-1) == E and b"n_rows" in _err()
    for p in (-0.1, 1.5, math.nan):
        assert call(p=p) == E and b"p_augment" in _err(), p
    for lo, hi in ((-13, 2), (-2, 13), (2, 1), (-2**31, 2**31 - 1)):
        assert call(lo=lo, hi=hi) == E and b"pitch range" in _err(), (lo, hi)
    for sr in (0, -16000, (1 << 20) + 1):
        assert call(sr=sr) == E and b"sample_rate" in _err(), sr
    assert call(n=0) == _lib.OK and call(n=0, lens=None, table=None, stretch=None, back=None, nlens=None) == _lib.OK
    assert call(n=0, lo=-12, hi=12) == _lib.OK and call(n=0, lo=3, hi=3) == _lib.OK


# ------------------------------------------------------------------------------------------------ the Python front
def test_the_package_exports_the_pitch_functions():
    for name in ("stretch_rows", "pitch_shift_rows", "draw_pitch", "pitch_rate", "pitch_rate_pair", "stretched_length"):
        assert name in cda.__all__ and getattr(cda, name) is getattr(cpitch, name), name
    src, offs, lens = torch.zeros(300), torch.zeros(1, dtype=torch.int64), torch.tensor([300], dtype=torch.int32)
    plans = torch.from_numpy(cpitch.plan_array([(0, 0.9)]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.stretch_rows(src, offs, lens, plans, 400)
    with pytest.raises(ValueError, match="uint8"):
        cda.stretch_rows(src, offs, lens, plans.view(torch.int32), 400)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.pitch_shift_rows(src, offs, lens, plans, torch.tensor([[0, 17000, 16000]], dtype=torch.int32), 300)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.draw_pitch(1, lens, 0.5, (-2, 2), 16000, torch.from_numpy(cpitch.step_table((-2, 2), 16000)))
    for bad in ((-13, 2), (2, -2), (0.5, 2)):
        with pytest.raises(ValueError, match="pitch_range"):
            cda.draw_pitch(1, lens, 0.5, bad, 16000)


def test_pitch_is_opt_in_and_moves_no_random_stream_by_default():
    aug = cda.AudioAugmentor(p_augment=1.0)
    assert aug.pitch is False and aug.pitch_range == (-2, 2)
    x = torch.ones(1, 100)
    random.seed(4)
    assert aug.pitch_shift(x) is x                                         # the identity ...
    after = random.getstate()
    random.seed(4)
    random.random()
    random.randint(-2, 2)
    assert random.getstate() == after                                      # ... behind the reference's two draws
    random.seed(4)
    assert aug.pitch_shift(x, (-5, 5)) is x
    # the record's draws are today's: shift, gain, gaussian (no bank), in that order, and nothing for the pitch
    random.seed(4)
    c, pair, n_new, steps = aug.draw_item_pitched(16000)
    after = random.getstate()
    random.seed(4)
    shift = int(16000 * random.uniform(-0.2, 0.2)) if not (random.random() > 1.0) else 0
    gain = random.uniform(0.7, 1.3) if not (random.random() > 1.0) else None
    snr = random.uniform(10, 30) if not (random.random() > 1.0) else None
    assert random.getstate() == after
    assert pair is None and steps is None and n_new == 16000 and c.shift == shift and c.gain == np.float32(gain)
    assert c.gaussian_snr_db == snr
    random.seed(4)
    d, pair3, n3 = aug.draw_item(16000)
    assert bytes(d) == bytes(c) and (pair3, n3) == (None, 16000)
    for bad in ((-13, 2), (2, 1), (0.5, 1)):
        with pytest.raises(ValueError, match="pitch_range"):
            cda.AudioAugmentor(pitch=True, pitch_range=bad)
    with pytest.raises(ValueError, match="sample_rate"):
        cda.AudioAugmentor(pitch=True, sample_rate=2**19 + 1)
    cda.AudioAugmentor(pitch=False, pitch_range=(-40, 40))                 # not looked at while the step is off
    a, s = cda.create_augmentation_pipeline(p_augment=0.3, pitch=True, pitch_range=(-1, 3))
    assert a.pitch and a.pitch_range == (-1, 3) and not a.speed and s.p == 0.3
    assert cda.create_augmentation_pipeline()[0].pitch is False


def test_draw_item_pitched_puts_the_pitch_draws_between_speed_and_gain():
    aug = cda.AudioAugmentor(p_augment=1.0, speed=True, pitch=True, pitch_range=(-3, 3))
    aug.noise_samples = [torch.zeros(1, 700), torch.zeros(1, 20000)]
    aug._pack_bank()
    random.seed(9)
    c, pair, n_new, steps = aug.draw_item_pitched(16000)
    after = random.getstate()
    random.seed(9)
    random.random()
    shift = int(16000 * random.uniform(-0.2, 0.2))
    random.random()
    want_pair = cwarp.speed_rate_pair(random.uniform(0.9, 1.1), 16000)
    random.random()
    want_steps = random.randint(-3, 3)
    random.random()
    gain = random.uniform(0.7, 1.3)
    random.random()
    snr = random.uniform(10, 30)
    random.random()
    k = random.choice(range(2))
    want_n = cwarp.warped_length(16000, *want_pair)
    rep = 700 * (want_n // 700 + 1) if k == 0 else 20000
    start = random.randint(0, rep - want_n)                                # the pitch step keeps n'
    random.uniform(5, 20)
    assert random.getstate() == after
    assert pair == want_pair and n_new == want_n and steps == want_steps and c.shift == shift and c.gain == np.float32(gain)
    assert c.gaussian == 1 and c.gaussian_snr_db == snr and (c.bank_index, c.bank_start) == (k, start)
    # without the speed step: shift, pitch coin, semitones, gain
    aug = cda.AudioAugmentor(p_augment=1.0, pitch=True)
    random.seed(10)
    c, pair, n_new, steps = aug.draw_item_pitched(800)
    random.seed(10)
    random.random()
    shift = int(800 * random.uniform(-0.2, 0.2))
    random.random()
    want_steps = random.randint(-2, 2)
    random.random()
    assert (c.shift, pair, n_new, steps, c.gain) == (shift, None, 800, want_steps, np.float32(random.uniform(0.7, 1.3)))
    aug.p_augment = 0.0
    assert aug.draw_item_pitched(800)[1:] == (None, 800, None) and aug.pitch_shift(torch.ones(1, 8)).shape == (1, 8)


def test_the_loader_carries_the_pitch_draws():
    bank = cda.DeviceClipBank([torch.zeros(800), torch.ones(20000)], [0, 1], device="cpu")
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
    with pytest.raises(ValueError, match="cache_features"):
        cda.DeviceDataLoader(bank, pre, audio_augmentor=cda.AudioAugmentor(pitch=True), cache_features=True)
    aug = cda.AudioAugmentor(p_augment=1.0, pitch=True, pitch_range=(1, 2))
    loader = cda.DeviceDataLoader(bank, pre, batch_size=2, audio_augmentor=aug, noise="host")
    random.seed(2)
    torch.manual_seed(2)
    plan = loader.draw_batch([0, 1])
    assert plan.pitches() and not plan.warps() and plan.pairs is None and all(s in (1, 2) for s in plan.steps)
    assert plan.gaussian.shape == (2, 20000)                               # the pitch step keeps the lengths
    random.seed(2)
    want = [aug.draw_item_pitched(n) for n in (800, 20000)]
    assert [w[3] for w in want] == plan.steps and [bytes(w[0]) for w in want] == [bytes(c) for c in plan.clips]
    plain = cda.DeviceDataLoader(bank, pre, batch_size=2, audio_augmentor=cda.AudioAugmentor(p_augment=1.0)).draw_batch([0, 1])
    assert plain.steps is None and not plain.pitches()
    val = cda.DeviceDataLoader(bank, pre, batch_size=2, audio_augmentor=cda.AudioAugmentor(pitch=True), is_training=False)
    assert val.draw_batch([0, 1]).clips is None
    packed = cda.data.UploadWords()
    packed.add("lengths", np.zeros(5, np.int32))
    packed.add("stretch", cpitch.plan_array([(3, 0.5), (-1, 2.0)]), align8=True)
    packed.add("back", cwarp.plan_array([(0, 9, 10), (0, 1, 1)]))
    words, at = packed.array(), packed.at("stretch")
    assert at == 6 and words.size == 5 + 1 + 8 + 6 and words.dtype == np.int32 and not words[:6].any()
    words = words[5:]
    assert words[1] == 3 and words[5] == -1 and words[9:].tolist() == [0, 9, 10, 0, 1, 1]
    sent = torch.from_numpy(packed.array())
    assert np.array_equal(packed.view(sent, "stretch").numpy(), cpitch.plan_array([(3, 0.5), (-1, 2.0)]))
    assert packed.view(sent, "back").tolist() == [[0, 9, 10], [0, 1, 1]]
