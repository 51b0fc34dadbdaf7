"""Identity phase locking without a GPU: the locked restatement (tests/pitch_lock_ref.py) against the plain one, its
first-order bound, the fitness of the GPU test's inputs (floor and peak margins), what locking buys on a tone, the
layouts that carry the mode, and the Python surface's defaults."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import chain as cchain
from cough_detector_amd import pitch as cpitch
import pitch_lock_ref as L
import pitch_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cough_amd_pitch.h")


def _stretched():
    """The GPU test's rows that the kernel stretches and that are neither silent nor poisoned."""
    return [(name, x, shift, rate, lk, pl) for name, x, shift, rate, lk, pl in L.lock_refs()
            if P.stretchable(rate, x.size) and lk["peak"] > 0.0]


# ------------------------------------------------------------------------------------------------ the restatement
def test_locked_equals_plain_while_the_frames_telescope_and_differs_elsewhere():
    rows = _stretched()
    assert len(rows) >= 24 and len(L.lock_refs()) == len(P.make_cases()) + 4
    same = differ = 0
    for name, x, shift, rate, lk, pl in rows:
        peak = np.abs(pl["y"]).max()
        worst = np.abs(lk["y"] - pl["y"]).max() / peak
        print(f"{name}: locked against plain: {worst:.2e} of the peak; i0(t) == t throughout: {lk['telescopes']}")
        assert lk["n_s"] == pl["n_s"] == lk["y"].size, name
        if lk["telescopes"]:
            assert worst <= 1e-12, name
            same += 1
        differ += worst > 0.1
    assert same >= 3 and differ >= 10
    # the special rows are the plain restatement's
    for name, x, shift, rate, lk, pl in L.lock_refs():
        if not (P.stretchable(rate, x.size) and lk["peak"] > 0.0):
            assert lk["n_s"] == pl["n_s"] and np.array_equal(lk["y"], pl["y"], equal_nan=True) and not lk["E"].any(), name


def test_a_perturbed_spectrum_stays_inside_the_locked_bound():
    for k, (name, x, shift, rate, lk, _) in enumerate(_stretched()):
        moved = L.stretch_lock_ref(x, shift, rate, perturb=P.perturbation(x, shift, 4.0, seed=k))
        assert (np.abs(moved["y"] - lk["y"]) <= lk["E"]).all(), name


def test_the_inputs_are_fit_for_a_locked_comparison():
    for name, x, shift, rate, lk, _ in _stretched():
        peak = np.abs(lk["y"]).max()
        below = float((lk["E"] <= 2.0 ** -24 * peak).mean())
        print(f"{name}: floor margin {lk['margin']:.1e}, peak margin {lk['peak_margin']:.1e}, {lk['peaks_per_frame']:.1f} peaks per "
              f"frame, max E_lock {lk['E'].max() / peak:.1e} of the peak, {100 * below:.1f} % of the row at or below 2^-24")
        assert lk["margin"] >= 64.0, name
        assert lk["peak_margin"] >= 64.0, name
        assert (lk["E"] <= 2.0 ** -20 * peak).all(), name
        assert below >= 0.9, name


def test_peaks_and_owners():
    M = np.zeros((4, P.BINS))
    M[0, [10, 16, 200]] = [5.0, 4.0, 3.0]
    M[0, [11, 12]] = [6.0, 1.0]                                            # 11 beats 10 within two bins; 12 is at the floor
    M[1, [0, 256]] = [2.0, 2.5]                                            # the ends have no mirror
    M[2, [40, 42]] = [3.0, 3.0]                                            # equal within reach: neither is a peak
    M[3, [7, 8]] = [0.5, 0.9]                                              # at or below the floor
    pk = L.peaks_of(M, 1.0)
    assert np.flatnonzero(pk[0]).tolist() == [11, 16, 200] and np.flatnonzero(pk[1]).tolist() == [0, 256]
    assert not pk[2].any() and not pk[3].any()
    own = L.owners(pk)
    assert own[0, :14].tolist() == [11] * 14 and own[0, 14:109].tolist() == [16] * 95     # 108 is tied: the lower peak
    assert own[0, 108] == 16 and own[0, 109] == 200 and own[0, 256] == 200
    assert own[1, 128] == 0 and own[1, 129] == 256
    assert (own[2] == np.arange(P.BINS)).all() and (own[3] == np.arange(P.BINS)).all()
    # the tie row has a frame whose two strongest peaks lie an even number of bins apart, and the rows cover one peak
    # (a tone), a few (the stack: partials under five bins apart) and many (noise)
    refs = {name: lk for name, x, shift, rate, lk, pl in L.lock_refs()}
    x = [x for name, x, *_ in L.lock_refs() if name == "6000 tie"][0]
    mags = np.abs(P.spectra(x.astype(np.float64)))
    top = np.sort(np.argsort(mags[10])[-2:])
    assert top.tolist() == [40, 46] and L.peaks_of(mags, 2.0 ** -16 * np.abs(x).max())[10, top].all()
    assert refs["16000 tone"]["peaks_per_frame"] <= 1.0 and 5.0 <= refs["8000 stack"]["peaks_per_frame"] <= 13.0
    assert refs["16000 noise"]["peaks_per_frame"] >= 40.0
    assert 147.3 / L.BIN_HZ < 2 * L.REACH + 1                              # neighbouring partials' +-2 windows overlap


def test_locking_keeps_a_tones_level():
    sr, n = 16000, 16000
    for hz in (440.0, 1000.0, 2500.0):
        x = (0.5 * np.sin(2 * np.pi * hz * np.arange(n) / sr)).astype(np.float32)
        rms = lambda y: np.sqrt((y[1000:-1000] ** 2).mean()) / np.sqrt((x[1000:-1000].astype(np.float64) ** 2).mean())   # noqa: E731
        y = L.pitch_shift_lock_ref(x, 2, sr)
        locked, plain = rms(y), rms(P.pitch_shift_ref(x, 2, sr))
        peak_hz = np.abs(np.fft.rfft(y * np.hanning(n))).argmax() * sr / n
        print(f"{hz:.0f} Hz, +2 semitones: rms ratio {locked:.4f} locked, {plain:.4f} plain; peak at {peak_hz:.1f} Hz")
        assert 0.95 <= locked <= 1.05 and plain <= 0.7
        assert abs(peak_hz - hz * 2 ** (2 / 12)) <= sr / n
    for name, x, shift, rate, lk, pl in L.lock_refs():
        if "burst" in name or name == "16000 half":
            top = np.abs(x).max()
            print(f"{name}: peak of the stretched burst over its input's: {np.abs(lk['y']).max() / top:.2f} locked, "
                  f"{np.abs(pl['y']).max() / top:.2f} plain")


# ------------------------------------------------------------------------------------------------ the layouts
def test_the_mode_rides_in_the_reserved_word():
    text = open(HEADER).read()
    assert "#define COUGH_STRETCH_PHASE_LOCK 1" in text and "not read" not in text
    assert "THE LOCKED STRETCH'S ARITHMETIC" in text and "THIS HEADER IS THE CONTRACT" in text and "1/4" in text
    assert "#define COUGH_PITCH_ABI_VERSION 1" in text and _lib.load_pitch().cough_pitch_abi_version() == 1
    declared = set(re.findall(r"^(?:int|size_t|const char\*) (cough_[a-z_0-9]+)\s*\(", text, flags=re.M))
    assert declared == set(_lib.PITCH_SYMBOLS) and len(declared) == 4
    assert cpitch.PHASE_LOCK == 1 == L.PHASE_LOCK
    two, three = cpitch.plan_array([(-5, 0.75), (3, 1.5)]), cpitch.plan_array([(-5, 0.75, 0), (3, 1.5, 1)])
    assert two[0].tobytes() == three[0].tobytes() == bytes(_lib.CoughStretchPlan(shift=-5, reserved=0, rate=0.75))
    assert three[1].tobytes() == bytes(_lib.CoughStretchPlan(shift=3, reserved=1, rate=1.5)) != two[1].tobytes()
    mixed = cpitch.plan_array([(0, 0.9), (0, 0.9, 0x7FFFFFFF), (1, 2.0, -1)])
    assert mixed.view(cpitch._PLAN_DTYPE)["reserved"].reshape(-1).tolist() == [0, 0x7FFFFFFF, -1]
    plain, locked = cpitch.step_table((-2, 2), 16000), cpitch.step_table((-2, 2), 16000, phase_lock=True)
    assert plain.shape == locked.shape == (5, 16) and not plain.view(cpitch._STEP_DTYPE)["reserved"].any()
    for k, s in enumerate(range(-2, 3)):
        want = _lib.CoughPitchStep(rate=cpitch.pitch_rate(s), orig=cpitch.pitch_rate_pair(s, 16000)[0], reserved=1)
        assert locked[k].tobytes() == bytes(want), s
        assert locked[k, :12].tobytes() == plain[k, :12].tobytes()
    assert [(r, o, m) for r, o, m in locked.view(cpitch._STEP_DTYPE).reshape(-1).tolist()] == L.step_table(-2, 2, 16000, 1)
    assert C.sizeof(_lib.CoughPitchStep) == 16 and _lib.CoughPitchStep.reserved.offset == 12


def test_the_draw_restatement_sets_the_mode_only_where_semitones_were_drawn():
    lengths = [16000] * 4000 + [0, -3]
    rates, plans, n_s, steps, fired, mode = L.draw_pitch_lock_ref(5, lengths, 0.5, -2, 2, 16000, 1)
    assert (mode == (fired & (steps != 0))).all() and 0 < mode.sum() < fired.sum() < 4000
    assert not L.draw_pitch_lock_ref(5, lengths, 0.5, -2, 2, 16000, 0)[5].any()
    words = [0x7FFFFFFE, 1, 1, 0, 3]                                       # per entry -2 .. 2: only bit 0 counts
    mode = L.draw_pitch_lock_ref(5, lengths, 1.0, -2, 2, 16000, words)[5]
    assert (mode == np.isin(steps_of(5, lengths), (-1, 2))).all()


def steps_of(seed, lengths):
    return P.draw_pitch_ref(seed, lengths, 1.0, -2, 2, 16000)[3]


# ------------------------------------------------------------------------------------------------ the Python front
def test_host_plans_mark_exactly_the_rows_with_semitones():
    shifts, steps, lengths = [5, -7, 0, 9, 1], [2, None, 0, -1, 1], [16000, 9000, 300, 16000, 700]
    for pairs in (None, [None, (15000, 16000), None, None, (17000, 16000)]):
        plain = cchain.host_plans(shifts, pairs, steps, lengths, 16000, 16000)
        locked = cchain.host_plans(shifts, pairs, steps, lengths, 16000, 16000, phase_lock=True)
        assert plain[1:] == locked[1:] and plain.arrays.keys() == locked.arrays.keys()
        for name in plain.arrays:
            if name != "stretch":
                assert np.array_equal(plain.arrays[name], locked.arrays[name]), name
        a, b = (p.arrays["stretch"].view(cpitch._PLAN_DTYPE).reshape(-1) for p in (plain, locked))
        assert not a["reserved"].any() and b["reserved"].tolist() == [1, 0, 0, 1, 1]
        assert np.array_equal(a["shift"], b["shift"]) and np.array_equal(a["rate"], b["rate"])
        assert np.array_equal(plain.arrays["stretch"],
                              cchain.host_plans(shifts, pairs, steps, lengths, 16000, 16000, False).arrays["stretch"])
    assert not cchain.host_plans(shifts, None, [None, 0, None, 0, 0], lengths, 16000, 16000, True).arrays


def test_phase_lock_is_opt_in_needs_pitch_and_draws_nothing():
    assert cda.AudioAugmentor().phase_lock is False and cda.AudioAugmentor(pitch=True).phase_lock is False
    assert cda.create_augmentation_pipeline()[0].phase_lock is False
    with pytest.raises(ValueError, match="phase_lock"):
        cda.AudioAugmentor(pitch=False, phase_lock=True)
    with pytest.raises(ValueError, match="phase_lock"):
        cda.create_augmentation_pipeline(phase_lock=True)
    a, _ = cda.create_augmentation_pipeline(p_augment=0.3, pitch=True, phase_lock=True)
    assert a.pitch and a.phase_lock is True
    drawn = {}
    for lock in (False, True):
        aug = cda.AudioAugmentor(p_augment=0.6, speed=True, pitch=True, phase_lock=lock)
        aug.noise_samples = [torch.zeros(1, 700), torch.zeros(1, 20000)]
        aug._pack_bank()
        random.seed(9)
        items = [aug.draw_item_pitched(n) for n in (16000, 800, 300, 12345)]
        drawn[lock] = ([(bytes(c), pair, n, steps) for c, pair, n, steps in items], random.getstate())
        x = torch.ones(1, 100)
        aug.p_augment = 0.0
        assert aug.pitch_shift(x) is x and aug.augment(x) is x
    assert drawn[False] == drawn[True]
    # the loader's host draws do not depend on the flag either
    bank = cda.DeviceClipBank([torch.zeros(800), torch.ones(20000)], [0, 1], device="cpu")
    pre = cda.AudioPreprocessor(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
    plans = []
    for lock in (False, True):
        aug = cda.AudioAugmentor(p_augment=1.0, pitch=True, pitch_range=(1, 2), phase_lock=lock)
        loader = cda.DeviceDataLoader(bank, pre, batch_size=2, audio_augmentor=aug, noise="host")
        random.seed(2)
        torch.manual_seed(2)
        plan = loader.draw_batch([0, 1])
        plans.append((plan.steps, [bytes(c) for c in plan.clips], plan.gaussian, random.getstate()))
    assert plans[0][:2] == plans[1][:2] and torch.equal(plans[0][2], plans[1][2]) and plans[0][3] == plans[1][3]
