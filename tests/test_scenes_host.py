"""The scenes, without a GPU: the numpy restatements (tests/scenes_ref.py) against each other and against hand-worked
cases, the plan's draws, the parameter checks of the Python front, and the library's entries in the open tables
(``_lib.OPEN`` / ``build.OPEN_UNITS``: this test asks whether "scenes" is in them, never what else is)."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import scenes as cscenes
import scenes_ref as R
import score_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "scenes"
SR, WINDOW, HOP = 16000, 16000, 4000


# ------------------------------------------------------------------------------------------------ fmaf and the mix
def _fma_exact(a, b, c):
    x = Fraction(float(np.float32(a))) * Fraction(float(np.float32(b))) + Fraction(float(np.float32(c)))
    lo = np.float32(float(x))                                    # float(x) rounds once to float64; search the float32 grid
    best = min((np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))),
               key=lambda r: (abs(Fraction(float(r)) - x), int(np.float32(r).view(np.uint32)) & 1))
    return np.float32(best)


def test_fmaf_rounds_once():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(2000).astype(np.float32), rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * 10.0 ** rng.integers(-6, 3, 2000)).astype(np.float32)
    got = R.fmaf(a, b, c)
    assert got.dtype == np.float32
    for k in range(2000):
        assert got[k] == _fma_exact(a[k], b[k], c[k]), k
    # just above and just below the midpoint between 1 and 1 + 2^-23: a separately rounded product would tie to even
    up, down = np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(2.0 ** -12 - 2.0 ** -36)
    assert R.fmaf(up, np.float32(2.0 ** -12), np.float32(1.0)) == np.float32(1 + 2.0 ** -23)
    assert R.fmaf(down, np.float32(2.0 ** -12), np.float32(1.0)) == np.float32(1.0)
    assert np.isnan(R.fmaf(np.float32(np.nan), 1.0, 1.0)) and R.fmaf(np.float32(np.inf), 1.0, 1.0) == np.inf


def _random_scene(rng, length, bg_len, n_events):
    bg = rng.standard_normal(bg_len).astype(np.float32)
    events, at = [], 0
    for _ in range(n_events):
        n = int(rng.integers(1, max(2, length // (2 * n_events))))
        at += int(rng.integers(0, 5))
        if at + n > length:
            break
        events.append((at, rng.standard_normal(n).astype(np.float32), np.float32(rng.uniform(0.1, 3.0))))
        at += n
    return bg, int(rng.integers(0, bg_len)), np.float32(rng.uniform(0.5, 2.0)), events


@pytest.mark.parametrize("seed,length,bg_len", [(0, 300, 1000), (1, 257, 7), (2, 64, 1), (3, 500, 499), (4, 1, 3)])
def test_the_two_forms_of_the_mix_agree(seed, length, bg_len):
    rng = np.random.default_rng(seed)
    bg, start, gain, events = _random_scene(rng, length, bg_len, 3)
    a, b = R.mix_loop(bg, start, gain, length, events), R.mix_slices(bg, start, gain, length, events)
    assert a.dtype == b.dtype == np.float32 and a.view(np.uint32).tolist() == b.view(np.uint32).tolist()


def test_the_mix_by_hand():
    bg = np.array([1.0, 2.0, 4.0], dtype=np.float32)
    events = [(0, np.array([1.0], np.float32), np.float32(0.5)), (3, np.array([1.0, -1.0], np.float32), np.float32(2.0))]
    want = [0.5 * 2 + 0.5, 0.5 * 4, 0.5 * 1, 0.5 * 2 + 2, 0.5 * 4 - 2]      # the background wraps: 2 4 1 2 4
    for form in (R.mix_loop, R.mix_slices):
        assert form(bg, 1, 0.5, 5, events).tolist() == want
    assert np.isnan(R.mix_slices(np.array([np.nan], np.float32), 0, 1.0, 3, [])).all()
    assert R.power_ref(bg, 2, 4) == (16 + 1 + 4 + 16) / 4 and R.power_ref(bg, 0, 0) == 0.0
    assert R.gain_ref(10.0, 0.5, 2.0, 5.0) == np.float32(1.0) and R.gain_ref(4.0, 1.0, 1.0, 1.0) == np.float32(2.0)
    for p_bg, p_ev in ((0.0, 1.0), (1.0, 0.0), (float("nan"), 1.0), (1.0, float("inf"))):
        assert R.gain_ref(10.0, 1.0, p_bg, p_ev) == np.float32(1.0)


# ------------------------------------------------------------------------------------------------ window ranges
def _scores(windows_per_clip, smoothing=3, hop=HOP, window=WINDOW):
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(windows_per_clip)]).astype(np.int64))
    n = int(offsets[-1])
    return cda.WindowScores(torch.zeros(n), torch.zeros(n, dtype=torch.float64), offsets, offsets, hop, window, SR, smoothing)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_the_two_forms_of_the_window_ranges_agree(seed, sparse):
    """Fresh parameters for every case.  ``sparse``: ``hop > window - m``, so that short events fall between two
    windows -- with a collar, the case in which an unreachable event must stay unreachable."""
    rng = np.random.default_rng(100 * seed + sparse)
    between = 0                                                  # unreachable events in front of a later window, collar > 0
    for _ in range(2000):
        window = int(rng.integers(200, 2000))
        m = int(rng.integers(1, min(window, 400) + 1))
        hop = int(rng.integers(window - m + 1, 3 * window)) if sparse else int(rng.integers(1, 900))
        collar = int(rng.integers(0, 4))
        n = int(rng.integers(1, 12000))
        n_windows = S.windows_per_clip(n, window, hop)
        onset = int(rng.integers(0, n))
        offset = int(rng.integers(onset + 1, min(n, onset + (150 if sparse and rng.random() < 0.5 else n)) + 1))
        lo, hi = R.ranges_closed(onset, offset, n_windows, hop, window, m, collar)
        brute = R.ranges_brute(onset, offset, n_windows, hop, window, m, collar)
        if brute is None:
            assert lo > hi, (n, onset, offset, hop, window, m, collar)
            between += collar > 0 and lo < n_windows
        else:
            assert (lo, hi) == brute, (n, onset, offset, hop, window, m, collar)
    assert between > 20 or not sparse, between


def test_window_ranges_by_hand():
    m = R.min_overlap_samples(0.1, SR)
    assert m == 1600 and R.least_windows(0.5 * SR, HOP) == 2 and R.least_windows(0, HOP) == 0 and R.least_windows(1, HOP) == 1
    # a 1.5 s cough at 1.25 s in a 10 s recording (37 windows): k*4000 <= 42400 and k*4000 + 16000 >= 21600
    assert R.ranges_closed(20000, 44000, 37, HOP, WINDOW, m, 0) == (2, 10) == R.ranges_brute(20000, 44000, 37, HOP, WINDOW, m, 0)
    assert R.ranges_closed(20000, 44000, 37, HOP, WINDOW, m, 2) == (2, 12)
    # shorter than min_overlap: the windows that hold all 50 samples
    assert R.ranges_closed(20000, 20050, 37, HOP, WINDOW, m, 0) == (2, 5) == R.ranges_brute(20000, 20050, 37, HOP, WINDOW, m, 0)
    # at the very start and at the very end of 160000 samples; the collar stops at the last window
    assert R.ranges_closed(0, 8000, 37, HOP, WINDOW, m, 0) == (0, 1) == R.ranges_brute(0, 8000, 37, HOP, WINDOW, m, 0)
    assert R.ranges_closed(152000, 160000, 37, HOP, WINDOW, m, 2) == (35, 36) == R.ranges_brute(152000, 160000, 37, HOP, WINDOW, m, 2)
    # a recording without a window, and an event behind the last window of a recording that ends between two hops
    lo, hi = R.ranges_closed(100, 900, 0, HOP, WINDOW, m, 2)
    assert lo > hi and R.ranges_brute(100, 900, 0, HOP, WINDOW, m, 2) is None
    lo, hi = R.ranges_closed(19000, 19900, 1, HOP, WINDOW, m, 0)
    assert lo > hi and R.ranges_brute(19000, 19900, 1, HOP, WINDOW, m, 0) is None
    # windows that do not overlap (hop = window): a cough across the seam of windows 0 and 1 overlaps either by less than
    # 1600 samples.  No window reaches it, and the collar of 2 must not hand it to windows 1 and 2
    assert R.ranges_closed(15000, 17400, 5, 16000, 16000, m, 2) == (1, 0) and R.ranges_brute(15000, 17400, 5, 16000, 16000, m, 2) is None
    assert R.ranges_closed(15000, 17700, 5, 16000, 16000, m, 2) == (1, 3) == R.ranges_brute(15000, 17700, 5, 16000, 16000, m, 2)
    # gaps between the windows (hop 380, window 220): 98 samples inside the gap behind window 12
    assert R.ranges_closed(4900, 4998, 22, 380, 220, 104, 1) == (13, 12) and R.ranges_brute(4900, 4998, 22, 380, 220, 104, 1) is None
    assert R.ranges_closed(4900, 5050, 22, 380, 220, 104, 1) == (13, 14) == R.ranges_brute(4900, 5050, 22, 380, 220, 104, 1)


def test_truth_window_ranges_is_the_closed_form():
    rng = np.random.default_rng(5)
    lengths = [160000, 15999, 16000, 100000, 47000]
    per = [S.windows_per_clip(n, WINDOW, HOP) for n in lengths]
    clip, onset, offset = [], [], []
    for c, n in enumerate(lengths):
        at = 0
        for _ in range(int(rng.integers(0, 5))):
            a = at + int(rng.integers(0, n // 6))
            b = a + int(rng.integers(1, n // 6))
            if b > n:
                break
            clip.append(c), onset.append(a), offset.append(b)
            at = b
    truth = cda.TruthTable.from_intervals(clip, onset, offset, n_clips=len(lengths))
    assert truth.counts.tolist() == np.bincount(clip, minlength=5).tolist() and truth.offsets[-1] == len(clip)
    for smoothing, collar_seconds, collar in ((3, None, 2), (1, None, 0), (3, 0.3, 2), (3, 0.25, 1), (3, 0.0, 0)):
        lo, hi = cscenes.truth_window_ranges(truth, _scores(per, smoothing), 0.1, collar_seconds)
        assert lo.dtype == hi.dtype == np.int32
        want = [R.ranges_closed(onset[j], offset[j], per[clip[j]], HOP, WINDOW, 1600, collar) for j in range(len(clip))]
        assert list(zip(lo.tolist(), hi.tolist())) == want
        for c in range(5):
            mine = np.flatnonzero(np.array(clip) == c)
            assert (np.diff(lo[mine]) >= 0).all() and (np.diff(hi[mine][lo[mine] <= hi[mine]]) >= 0).all()
    # windows side by side (hop = window) and the default collar of 2: the cough across a seam stays unreachable
    seam = cda.TruthTable.from_intervals([0, 0, 0], [3000, 15000, 40000], [9000, 17400, 47000], n_clips=1)
    lo, hi = cscenes.truth_window_ranges(seam, _scores([5], 3, hop=16000), 0.1)
    assert list(zip(lo.tolist(), hi.tolist())) == [(0, 2), (1, 0), (2, 4)]
    assert list(zip(lo.tolist(), hi.tolist())) == [R.ranges_closed(a, b, 5, 16000, 16000, 1600, 2)
                                                   for a, b in ((3000, 9000), (15000, 17400), (40000, 47000))]
    with pytest.raises(ValueError, match="more than a window"):
        cscenes.truth_window_ranges(truth, _scores(per), 1.5)
    with pytest.raises(ValueError, match="must not be negative"):
        cscenes.truth_window_ranges(truth, _scores(per), -0.1)
    with pytest.raises(ValueError, match="must not be negative"):
        cscenes.truth_window_ranges(truth, _scores(per), 0.1, -1.0)
    with pytest.raises(ValueError, match="the truth counts 5 recordings, the scores 4"):
        cscenes.truth_window_ranges(truth, _scores(per[:4]))


# ------------------------------------------------------------------------------------------------ the matcher
def test_the_matcher_by_hand():
    for form in (R.match_walk, R.match_greedy):
        # two coughs whose ranges overlap, one detection between them: the earlier cough takes it
        assert form([6], [2, 5], [7, 10]) == ([R.HIT], [6, -1])
        assert form([6, 7], [2, 5], [7, 10]) == ([R.HIT, R.HIT], [6, 7])
        # two detections in one range: a hit, then a repeat
        assert form([3, 6], [2], [7]) == ([R.HIT, R.REPEAT], [3])
        # a detection after k_hi and before the next k_lo
        assert form([3, 8, 13], [2, 12], [4, 15]) == ([R.HIT, R.FALSE_ALARM, R.HIT], [3, 13])
        # an empty range (k_lo > k_hi) is never hit; a detection before every range is a false alarm
        assert form([1, 5], [6], [4]) == ([R.FALSE_ALARM, R.FALSE_ALARM], [-1])
        assert form([0], [2], [7]) == ([R.FALSE_ALARM], [-1])
        # no truth at all, no detection at all
        assert form([0, 9], [], []) == ([R.FALSE_ALARM, R.FALSE_ALARM], [])
        assert form([], [2], [7]) == ([], [-1])
        # the second cough's range starts inside the first one's: hit, hit, then a repeat of the second
        assert form([4, 5, 9, 12], [2, 4], [6, 10]) == ([R.HIT, R.HIT, R.REPEAT, R.FALSE_ALARM], [4, 5])


def _monotone_ranges(rng, n_events, n_windows):
    lo = np.sort(rng.integers(0, max(n_windows, 1), n_events))
    hi = np.sort(lo + rng.integers(-2, 6, n_events))
    return lo.tolist(), np.maximum.accumulate(hi).tolist()


@pytest.mark.parametrize("seed", range(8))
def test_the_two_forms_of_the_matcher_agree(seed):
    rng = np.random.default_rng(seed)
    for _ in range(200):
        n_windows = int(rng.integers(0, 60))
        lo, hi = _monotone_ranges(rng, int(rng.integers(0, 6)), n_windows)
        fired = sorted(set(rng.integers(0, max(n_windows, 1), int(rng.integers(0, 12))).tolist())) if n_windows else []
        assert R.match_walk(fired, lo, hi) == R.match_greedy(fired, lo, hi), (fired, lo, hi)
        # unreachable events keep an uncollared k_hi below their k_lo, so k_hi as a whole need not ascend: k_lo does
        hi = [h if rng.random() < 0.6 else l - 1 - int(rng.integers(0, 3)) for l, h in zip(lo, hi)]
        assert R.match_walk(fired, lo, hi) == R.match_greedy(fired, lo, hi), (fired, lo, hi)


def test_the_classes_sum_to_the_sweep_counts():
    rng = np.random.default_rng(11)
    per = [0, 1, 40, 64, 65, 130]
    smoothed = [S.smooth_ref(rng.random(n).astype(np.float32), 3) for n in per]
    thresholds = np.linspace(0.0, 1.0, 23)
    offsets, lo, hi, onset = [0], [], [], []
    for n in per:
        a, b = _monotone_ranges(rng, int(rng.integers(0, 5)), n)
        lo += a
        hi += b
        onset += [HOP * v for v in a]
        offsets.append(len(lo))
    for gap in (1, 2, 200):
        for walk in (R.match_walk, R.match_greedy):
            got = R.match_ref(smoothed, thresholds, gap, offsets, lo, hi, onset, HOP, WINDOW, S.events_ref, walk)
            counts = np.array(S.sweep_ref(smoothed, thresholds, gap)["counts"])
            assert (got["hits"] + got["repeats"] + got["false_alarms"] == counts).all()
            assert (got["hits"] <= np.diff(offsets)[:, None]).all() and (got["latency"][got["hits"] == 0] == 0).all()


# ------------------------------------------------------------------------------------------------ the plan
def _banks():
    rng = np.random.default_rng(2)
    backgrounds = cda.DeviceClipBank([torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in (48000, 7, 20000)],
                                     [0, 0, 0], device="cpu")
    events = cda.DeviceClipBank([torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in (1600, 3000, 800, 1)],
                                [1, 1, 1, 1], device="cpu")
    return backgrounds, events


def _assert_valid(plan, backgrounds, events):
    bl, el = backgrounds.lengths.numpy(), events.lengths.numpy()
    assert ((plan.bg_start >= 0) & (plan.bg_start < bl[plan.background])).all()
    for s in range(len(plan)):
        mine = np.flatnonzero(plan.event_scene == s)
        on, end = plan.onset[mine], plan.onset[mine] + el[plan.event_clip[mine]]
        assert (on >= 0).all() and (end <= plan.length[s]).all() and (on[1:] >= end[:-1]).all()
    assert (np.diff(plan.event_scene) >= 0).all()


def test_draw_scene_plan_is_reproducible_and_valid():
    backgrounds, events = _banks()
    for seed in range(5):
        a = cda.draw_scene_plan(backgrounds, events, 12, 2.0, events_per_scene=(0, 6), min_gap_seconds=0.05, seed=seed)
        b = cda.draw_scene_plan(backgrounds, events, 12, 2.0, events_per_scene=(0, 6), min_gap_seconds=0.05, seed=seed)
        for f in ("background", "bg_start", "bg_gain", "length", "event_scene", "event_clip", "onset", "snr_db"):
            assert getattr(a, f).tolist() == getattr(b, f).tolist(), f
        _assert_valid(a, backgrounds, events)
        assert len(a) == 12 and (a.length == 32000).all() and ((a.snr_db >= 5) & (a.snr_db <= 20)).all()
        gap = 800
        for s in range(12):
            mine = np.flatnonzero(a.event_scene == s)
            end = a.onset[mine] + events.lengths.numpy()[a.event_clip[mine]]
            assert (a.onset[mine][1:] - end[:-1] >= gap).all()
    other = cda.draw_scene_plan(backgrounds, events, 12, 2.0, events_per_scene=(0, 6), min_gap_seconds=0.05, seed=99)
    assert other.onset.tolist() != a.onset.tolist()
    # the documented order of the draws, restated for the first scene
    rng = np.random.Generator(np.random.Philox(3))
    plan = cda.draw_scene_plan(backgrounds, events, 1, 2.0, events_per_scene=(2, 4), min_gap_seconds=0.05, seed=3)
    b = int(rng.integers(0, 3))
    start = int(rng.integers(0, int(backgrounds.lengths[b])))
    m = int(rng.integers(2, 5))
    clips = rng.integers(0, 4, size=m)
    snrs = rng.uniform(5, 20, size=m)
    el = events.lengths.numpy()[clips]
    cuts = np.sort(rng.integers(0, 32000 - int(el.sum()) - (m - 1) * 800 + 1, size=m))
    onsets = [int(cuts[j]) + int(el[:j].sum()) + j * 800 for j in range(m)]
    assert (plan.background.tolist(), plan.bg_start.tolist()) == ([b], [start])
    assert plan.event_clip.tolist() == clips.tolist() and plan.snr_db.tolist() == snrs.tolist() and plan.onset.tolist() == onsets


def test_draw_scene_plan_raises_when_the_events_cannot_fit_and_fills_a_scene_exactly():
    backgrounds, events = _banks()
    with pytest.raises(ValueError, match=r"scene 0: its 4 events .* need \d+ samples more than the scene's 1600"):
        cda.draw_scene_plan(backgrounds, events, 3, 0.1, events_per_scene=(4, 4), min_gap_seconds=0.5)
    only = events.subset([1])                                    # 3000 samples in a scene of 3000
    plan = cda.draw_scene_plan(backgrounds, only, 4, 3000 / SR, events_per_scene=(1, 1), min_gap_seconds=0.5, seed=1)
    assert plan.onset.tolist() == [0, 0, 0, 0] and (plan.length == 3000).all()
    with pytest.raises(ValueError, match="scene 0"):
        cda.draw_scene_plan(backgrounds, only, 1, 2999 / SR, events_per_scene=(1, 1))
    empty = cda.draw_scene_plan(backgrounds, events, 0, 1.0)
    assert len(empty) == 0 and empty.onset.size == 0


def test_every_parameter_check_raises_before_a_device_is_touched():
    backgrounds, events = _banks()                               # CPU banks: whatever reaches a kernel raises RuntimeError
    good = cda.draw_scene_plan(backgrounds, events, 3, 1.0, events_per_scene=(1, 2), seed=0)
    for kw, match in ((dict(n_scenes=-1), "n_scenes"), (dict(scene_seconds=0.0), "samples"), (dict(scene_seconds=float("nan")), "finite"),
                      (dict(events_per_scene=(3, 1)), "lo <= hi"), (dict(events_per_scene=(1.5, 2)), "integers"),
                      (dict(events_per_scene=5), "pair"), (dict(snr_range=(20, 5)), "lo <= hi"),
                      (dict(min_gap_seconds=-1), "negative"), (dict(bg_gain=float("inf")), "finite"), (dict(seed=-1), "seed"),
                      (dict(sample_rate=0), "sample_rate")):
        args = dict(n_scenes=2, scene_seconds=1.0)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            cda.draw_scene_plan(backgrounds, events, **args)
    with pytest.raises(ValueError, match="DeviceClipBank"):
        cda.draw_scene_plan([1, 2], events, 1, 1.0)
    with pytest.raises(ValueError, match="background bank is empty"):
        cda.draw_scene_plan(cda.DeviceClipBank([], [], device="cpu"), events, 1, 1.0)

    def changed(**kw):
        fields = {f: getattr(good, f).copy() for f in ("background", "bg_start", "bg_gain", "length", "event_scene",
                                                      "event_clip", "onset", "snr_db")}
        fields.update(kw)
        return cda.ScenePlan(**fields)
    m = good.onset.size
    for plan, match in ((changed(background=np.array([0, 3, 0])), "background indices"),
                        (changed(bg_start=np.array([0, -1, 0])), "scene 1: bg_start=-1"),
                        (changed(length=np.array([16000, 0, 16000])), "scene lengths"),
                        (changed(bg_gain=np.array([1, np.nan, 1], np.float32)), "bg_gain"),
                        (changed(event_clip=np.full(m, 4)), "event clips"),
                        (changed(event_scene=np.full(m, 3)), "event scenes"),
                        (changed(event_scene=good.event_scene[::-1].copy()), "ascending scene"),
                        (changed(onset=np.full(m, 16000)), "does not lie inside scene"),
                        (changed(onset=np.full(m, -1)), "does not lie inside scene"),
                        (changed(snr_db=np.full(m, np.inf)), "snr_db"),
                        (changed(onset=good.onset[:-1]), "onset holds")):
        with pytest.raises(ValueError, match=match):
            cda.compose_scenes(backgrounds, events, plan)
    two = cda.ScenePlan(np.array([0]), np.array([0]), np.array([1.0], np.float32), np.array([16000]), np.array([0, 0]),
                        np.array([0, 1]), np.array([100, 1000]), np.array([10.0, 10.0]))
    with pytest.raises(ValueError, match="event 1 overlaps the event before it in scene 0"):
        cda.compose_scenes(backgrounds, events, two)
    two.onset = np.array([5000, 100])
    with pytest.raises(ValueError, match="sorted by onset"):
        cda.compose_scenes(backgrounds, events, two)
    with pytest.raises(ValueError, match="ScenePlan"):
        cda.compose_scenes(backgrounds, events, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.compose_scenes(backgrounds, events, good)
    with pytest.raises(ValueError, match="inside its clip"):
        cscenes.span_power(backgrounds, [1], [7], [10])
    with pytest.raises(ValueError, match="clips must lie"):
        cscenes.span_power(backgrounds, [3], [0], [10])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cscenes.span_power(backgrounds, [1], [6], [10])

    for args, match in ((([0, 0], [10, 5], [20, 30]), "sorted by onset"), (([0, 0], [10, 15], [20, 30]), "overlaps"),
                        (([1, 0], [10, 15], [20, 30]), "ascending recording"), (([0], [10], [10]), "onset < offset"),
                        (([0], [-1], [10]), "onset < offset"), (([0, 0], [10], [20, 30]), "onset holds"),
                        (([2], [1], [2]), "recordings must lie")):
        with pytest.raises(ValueError, match=match):
            cda.TruthTable.from_intervals(*args, n_clips=2)
    truth = cda.TruthTable.from_intervals([0, 0, 1], [100, 30000, 5], [9000, 31000, 900], n_clips=2)
    scores = _scores([37, 0])
    bank = cda.DeviceClipBank([torch.zeros(160000), torch.zeros(1000)], [1, 1], device="cpu")
    for thresholds, match in (([], "thresholds"), ([float("nan")], "finite"), (np.zeros(1025), "thresholds")):
        with pytest.raises(ValueError, match=match):
            cda.match_events(scores, truth, thresholds)
    with pytest.raises(ValueError, match="debounce_seconds"):
        cda.match_events(scores, truth, [0.5], debounce_seconds=-1)
    with pytest.raises(ValueError, match="more than a window"):
        cda.match_events(scores, truth, [0.5], min_overlap_seconds=2.0)
    with pytest.raises(ValueError, match="threshold"):
        cscenes.list_matches(scores, truth, float("nan"))
    with pytest.raises(ValueError, match="event_counts holds 3 values, expected 2"):
        cscenes.list_matches(scores, truth, 0.5, event_counts=[1, 2, 3])
    with pytest.raises(ValueError, match="reaches past the end"):
        cda.missed_events(cda.DeviceClipBank([torch.zeros(160000), torch.zeros(800)], [1, 1], device="cpu"), truth, scores, 0.5)
    with pytest.raises(ValueError, match="holds 3 recordings"):
        cda.missed_events(cda.DeviceClipBank([torch.zeros(5)] * 3, [1] * 3, device="cpu"), truth, scores, 0.5)
    for call in (lambda: cda.match_events(scores, truth, [0.5]), lambda: cscenes.list_matches(scores, truth, 0.5),
                 lambda: cda.missed_events(bank, truth, scores, 0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_pick_threshold():
    report = {"thresholds": [0.9, 0.1, 0.5, 0.7], "false_alarms_per_minute": [0.0, 7.0, 1.0, 0.5], "recall": [0.2, 1.0, 0.85, 0.6]}
    assert cda.pick_threshold(report) == {"threshold": 0.5, "index": 2, "recall": 0.85, "false_alarms_per_minute": 1.0,
                                          "meets_recall": True}
    assert cda.pick_threshold(report, 0.6)["threshold"] == 0.7 and not cda.pick_threshold(report, 0.6)["meets_recall"]
    assert cda.pick_threshold(report, 0.6, 0.6)["meets_recall"]
    assert cda.pick_threshold(report, -1.0) == {"threshold": None, "index": None, "recall": None,
                                                "false_alarms_per_minute": None, "meets_recall": False}
    none = {"thresholds": [0.5], "false_alarms_per_minute": [None], "recall": [None]}
    assert cda.pick_threshold(none)["threshold"] is None
    assert cscenes.scene_tiles(np.array([1, 4096, 4097, 9000])).tolist() == [[0, 0], [1, 0], [2, 0], [2, 4096], [3, 0], [3, 4096],
                                                                            [3, 8192]]


# ------------------------------------------------------------------------------------------------ the library
def _header(name):
    return open(os.path.join(ROOT, "include", f"cough_amd_{name}.h")).read()


def _declared(name):
    return set(re.findall(r"^(?:int|size_t|const char\*|void) (cough_[a-z_0-9]+)\s*\(", _header(name), flags=re.M))


def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_library_is_in_the_open_tables():
    assert NAME in _lib.OPEN and NAME in cbuild.OPEN_UNITS and NAME in cbuild.OPEN_LIBS
    assert NAME not in _lib.LIBRARIES and NAME not in _lib.LATER and NAME not in cbuild.UNITS and NAME not in cbuild.LATER_UNITS
    assert cbuild.OPEN_UNITS[NAME] == (NAME + ".hip",) and NAME + ".hip" not in cbuild.SOURCES
    for f in (NAME + ".hip", f"exports_{NAME}.map", "score_walk.h"):
        assert os.path.exists(os.path.join(cbuild.CSRC, f)), f
    assert os.path.basename(cbuild.OPEN_LIBS[NAME]) == f"libcough_amd_{NAME}.so" == _lib.OPEN[NAME].soname
    assert os.path.exists(cbuild.OPEN_LIBS[NAME])


def test_header_record_and_file_name_the_same_entry_points():
    rec, text, declared = _lib.OPEN[NAME], _header(NAME), _declared(NAME)
    assert declared == set(rec.symbols) == set(rec.prototypes), declared ^ set(rec.symbols)
    assert declared == {"cough_scenes_abi_version", "cough_scenes_last_error", "cough_span_power", "cough_scene_gains",
                        "cough_mix_scenes", "cough_match_events", "cough_list_event_matches"}
    assert rec.symbols[0] == rec.abi_symbol == f"cough_{NAME}_abi_version" and rec.symbols[1] == rec.error_symbol
    assert _exported(rec.path) == declared, sorted(_exported(rec.path) ^ declared)
    assert _lib.SCENES_SYMBOLS is rec.symbols and _lib.SCENES_LIB_PATH == rec.path
    assert _lib.load_scenes == rec.load and _lib.check_scenes == rec.check
    lib = rec.load()
    assert getattr(lib, rec.abi_symbol)() == rec.abi == 1 and f"#define COUGH_{NAME.upper()}_ABI_VERSION 1\n" in text
    assert isinstance(getattr(lib, rec.error_symbol)(), bytes)
    # no entry point shares its name with one of another library: a program may link several of them
    for other in (*_lib.LIBRARIES.values(), *_lib.LATER.values(), *(r for r in _lib.OPEN.values() if r.name != NAME)):
        assert not declared & set(other.symbols), other.name
    assert re.search(rf"#define COUGH_SCENES_TILE {cscenes.TILE}\b", text)
    assert re.search(rf"#define COUGH_SCENES_MAX_THRESHOLDS {_lib.MAX_THRESHOLDS}\b", text)
    # every prototype has as many arguments as the header's declaration
    for symbol, (_, argtypes) in rec.prototypes.items():
        params = re.search(rf"\b{symbol}\s*\(([^)]*)\)", text).group(1)
        count = 0 if params.strip() == "void" else params.count(",") + 1
        assert count == (len(argtypes) if argtypes else 0), symbol


def test_the_score_library_still_exports_exactly_its_header():
    rec = _lib.LIBRARIES["score"]
    assert _exported(rec.path) == _declared("score") == set(rec.symbols) and len(rec.symbols) == 5
    assert rec.load().cough_score_abi_version() == 1
    src = open(os.path.join(cbuild.CSRC, "score.hip")).read()
    walk = open(os.path.join(cbuild.CSRC, "score_walk.h")).read()
    for fn in ("walk_fires", "walk_advance", "clip_windows"):
        assert re.search(rf"__device__ __forceinline__ \w[\w ]* {fn}\(", walk), fn     # defined once, in the shared header
        assert not re.search(rf"__device__ __forceinline__ \w[\w ]* {fn}\(", src), fn
    for unit in ("score.hip", "scenes.hip"):
        assert '#include "score_walk.h"' in open(os.path.join(cbuild.CSRC, unit)).read()


def test_the_c_abi_checks_its_arguments():
    lib = _lib.load_scenes()
    err = lambda: lib.cough_scenes_last_error().decode()
    assert lib.cough_span_power(None, 0, None, None, None, None, 0, None, None) == _lib.EINVAL and "NULL" in err()
    assert lib.cough_span_power(None, 0, 8, 8, 8, 8, -1, 8, None) == _lib.EINVAL and "n must not be negative" in err()
    assert lib.cough_span_power(None, 0, 8, 8, 8, 8, 0, 8, None) == _lib.OK                   # n == 0 launches nothing
    assert lib.cough_span_power(8, 4, 4, 8, 8, 8, 0, 8, None) == _lib.EINVAL and "8-byte aligned" in err()
    assert lib.cough_scene_gains(None, None, 0, None, 0, None, None, None, 0, None, None) == _lib.OK
    assert lib.cough_scene_gains(None, None, 0, None, 0, None, None, None, -1, None, None) == _lib.EINVAL
    assert lib.cough_scene_gains(8, 8, 1, 8, 1, 8, 8, 8, 1, None, None) == _lib.EINVAL and "NULL" in err()
    assert lib.cough_scene_gains(8, 8, 1, 8, 1, 8, 8, 4, 1, 8, None) == _lib.EINVAL and "8-byte aligned" in err()
    mix = [8, 1, 8, 8, 8, 8, 8, 8, 8, 1, 8, 1, 8, 8, 8, 8, 1, 8, 1, 8, 1, None]
    for at, value, match in ((9, 0, None), (18, 0, None), (9, -1, "negative"), (1, -1, "negative"), (2, None, "NULL"),
                             (12, None, "NULL event arrays"), (19, None, "d_out is NULL"), (0, 2, "4-byte aligned"),
                             (8, 4, "8-byte aligned")):
        args = list(mix)
        args[at] = value
        status = lib.cough_mix_scenes(*args)
        assert status == (_lib.OK if match is None else _lib.EINVAL), (at, value)
        assert match is None or match in err(), (at, err())
    match = [8, 8, 1, 1, 8, 1, 1, 8, 8, 8, 8, 1, 4000, 16000, 8, 8, 8, 8, None]
    for at, value, text in ((2, 0, None), (2, -1, "n_clips"), (3, 1 << 38, "n_windows"), (5, 0, "n_thresholds"),
                            (5, 1025, "n_thresholds"), (6, 0, "gap"), (12, 0, "hop"), (13, 0, "window"), (7, None, "NULL"),
                            (8, None, "NULL truth arrays"), (10, None, "d_onset"), (17, 4, "8-byte aligned"),
                            (14, 2, "4-byte aligned")):
        args = list(match)
        args[at] = value
        status = lib.cough_match_events(*args)
        assert status == (_lib.OK if text is None else _lib.EINVAL), (at, value)
        assert text is None or text in err(), (at, err())
    lst = [8, 8, 1, 1, 0.5, 1, 8, 8, 8, 1, 8, 8, 1, 8, None]
    for at, value, text in ((2, 0, None), (4, float("nan"), "NaN"), (5, 0, "gap"), (12, -1, "n_events"), (10, None, "d_truth_window"),
                            (11, None, "needs d_event_offsets"), (6, None, "NULL")):
        args = list(lst)
        args[at] = value
        status = lib.cough_list_event_matches(*args)
        assert status == (_lib.OK if text is None else _lib.EINVAL), (at, value)
        assert text is None or text in err(), (at, err())


def test_the_package_exports_the_names():
    names = ["ScenePlan", "TruthTable", "EventSweep", "draw_scene_plan", "compose_scenes", "truth_window_ranges",
             "match_events", "event_report", "pick_threshold", "missed_events"]
    for name in names:
        assert name in cda.__all__ and getattr(cda, name) is getattr(cscenes, name), name
    assert len(set(cda.__all__)) == len(cda.__all__)
    doc = cscenes.__doc__
    assert all(f"\n{k}. " in doc for k in range(1, 9)) and "python -m cough_detector_amd.scenes" in doc
