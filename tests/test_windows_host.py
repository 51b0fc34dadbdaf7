"""The composed windows, without a GPU: the numpy restatements (tests/windows_ref.py) against each other and with defects
planted in them, the plan's draws, the inner-window rule pushed through the worst the waveform chain can do, the labels of
sliding windows against brute force and against ``truth_window_ranges``, the parameter checks of the Python front, and
the library's entries in the open tables (this test asks whether "windows" is in them, never what else is)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import _lib
from cough_detector_amd import build as cbuild
from cough_detector_amd import scenes as cscenes
from cough_detector_amd import windows as cwin
import scenes_ref as R
import windows_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "windows"
SR = 16000


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64)


def _same(a, b):
    """Bit for bit, NaNs of any payload counting as equal."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(_bits(a[~np.isnan(a)]), _bits(b[~np.isnan(b)]))


def _snr_linear(rows):
    return 10.0 ** (W.plan_arrays(rows)[6] / 10.0)


# ------------------------------------------------------------------------------------------------ the restatements
def test_the_two_forms_of_the_power_agree():
    rng = np.random.default_rng(0)
    for n in (1, 2, 255, 256, 257, 1000, 4097):
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
        a, b = W.power_order(x), W.power_order_loop(x)
        assert np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), n
        exact = float(np.sum(x.astype(np.float64) ** 2) / n)
        assert abs(a - exact) <= 2 * n * 2.0 ** -53 * exact
    assert W.power_order(np.zeros(0, np.float32)) == 0.0 and W.power_order(np.array([2.0], np.float32)) == 4.0
    assert np.isnan(W.power_order(np.array([1.0, np.nan], np.float32))) and W.power_order(np.array([np.inf], np.float32)) == np.inf


@pytest.mark.parametrize("width", [1, 255, 257])
def test_the_two_forms_of_a_row_agree_bit_for_bit(width):
    bgs, evs = W.banks()
    rows = W.batch_rows(width)
    snr = _snr_linear(rows)
    assert 45 <= len(rows) <= 56
    for r, row in enumerate(rows):
        bg = None if row[0] < 0 else bgs[row[0]]
        events = W.row_events(row, evs, snr[r])
        a, b = W.compose_loop(bg, row[1], row[2], width, events), W.compose_slices(bg, row[1], row[2], width, events)
        assert a[0].dtype == b[0].dtype == np.float32 and _same(a[0], b[0]), r
        assert _same(np.float64(a[1]), np.float64(b[1])) and _same(np.array(a[2], np.float32), np.array(b[2], np.float32)), r


def test_a_row_by_hand():
    bg = np.array([1.0, 2.0, 4.0], dtype=np.float32)
    one = np.array([1.0, -1.0], np.float32)
    # width 5 from sample 1: 2 4 1 2 4, P_bg = 41 / 5; an event of power 1 at snr_linear 5 / 41 * 4: gain = 0.5 * 2
    events = [(one, -1, 4 * 5 / 41.0), (one, 4, 4 * 5 / 41.0)]
    for form in (W.compose_loop, W.compose_slices):
        out, p_bg, gains = form(bg, 1, 0.5, 5, events)
        assert p_bg == 41 / 5 and [float(g) for g in gains] == [1.0, 1.0]
        assert out.tolist() == [0.5 * 2 - 1, 0.5 * 4, 0.5 * 1, 0.5 * 2, 0.5 * 4 + 1]
        out, p_bg, gains = form(None, 0, float("inf"), 3, [(one, 1, 10.0)])                 # silence: +0.0, gain 1
        assert p_bg == 0.0 and gains == [np.float32(1.0)] and out.tolist() == [0.0, 1.0, -1.0] and not np.signbit(out[0])
        out, _, _ = form(bg, 0, 1.0, 4, [(one, -2, 1.0), (one, 4, 1.0), (one, 9, 1.0)])     # events that miss the row
        assert out.tolist() == [1.0, 2.0, 4.0, 1.0]


@pytest.mark.parametrize("defect", W.DEFECTS)
def test_a_planted_defect_is_caught_on_the_test_batch(defect):
    bgs, evs = W.banks()
    caught = 0
    for width in (257, 4097):
        rows = W.batch_rows(width)
        snr = _snr_linear(rows)
        for r, row in enumerate(rows):
            bg = None if row[0] < 0 else bgs[row[0]]
            events = W.row_events(row, evs, snr[r])
            good, bad = W.compose_slices(bg, row[1], row[2], width, events), W.compose_slices(bg, row[1], row[2], width, events, defect=defect)
            caught += not (_same(good[0], bad[0]) and _same(np.array(good[2], np.float32), np.array(bad[2], np.float32)))
    assert caught >= 2, (defect, caught)


# ------------------------------------------------------------------------------------------------ the plan's draws
def _banks(ev_lengths=(1600, 3000, 800, 1, 5000, 2400), ev_labels=(1, 1, 1, 1, 0, 0), bg_lengths=(48000, 7, 20000)):
    rng = np.random.default_rng(2)
    backgrounds = cda.DeviceClipBank([torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in bg_lengths],
                                     [0] * len(bg_lengths), device="cpu")
    events = cda.DeviceClipBank([torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in ev_lengths],
                                list(ev_labels), device="cpu")
    return backgrounds, events


FIELDS = ("background", "bg_start", "bg_gain", "n_events", "event_clip", "onset", "snr_db")


def test_draw_window_plan_repeats_itself_and_equals_the_restated_draws():
    backgrounds, events = _banks()
    bl, el, lab = backgrounds.lengths.numpy(), events.lengths.numpy(), events.labels.numpy()
    for seed, kw in ((0, {}), (1, dict(p_cough=0.8, p_distractor=0.6, coughs_per_window=(1, 4), bg_gain_range=(0.5, 2.0))),
                     (2**64 - 1, dict(margin=3201, rho_min=16000 / 17600, snr_range=(0, 3)))):
        a = cda.draw_window_plan(backgrounds, events, 64, 16000, SR, seed, **kw)
        b = cda.draw_window_plan(backgrounds, events, 64, 16000, SR, seed, **kw)
        want = W.draw_ref(bl, el, lab, 64, 16000, SR, seed, **kw)
        for f in FIELDS:
            assert getattr(a, f).tolist() == getattr(b, f).tolist() == want[f].tolist(), (seed, f)
        assert a.bg_gain.dtype == np.float32 and a.onset.shape == a.event_clip.shape == a.snr_db.shape == (64, 4)
    other = cda.draw_window_plan(backgrounds, events, 64, 16000, SR, 5)
    assert other.onset.tolist() != a.onset.tolist()
    assert len(cda.draw_window_plan(backgrounds, events, 0, 16000, SR, 0)) == 0


def test_draw_window_plan_stays_inside_its_ranges_over_ten_thousand_rows():
    backgrounds, events = _banks()
    bl, el, lab = backgrounds.lengths.numpy(), events.lengths.numpy(), events.labels.numpy()
    width, b = 16000, 10000
    plan = cda.draw_window_plan(backgrounds, events, b, width, SR, 3, coughs_per_window=(1, 3), bg_gain_range=(0.25, 1.0))
    used = plan.used()
    assert ((plan.background >= 0) & (plan.background < 3)).all() and ((plan.bg_start >= 0) & (plan.bg_start < bl[plan.background])).all()
    assert ((plan.bg_gain >= 0.25) & (plan.bg_gain <= 1.0)).all() and ((plan.n_events >= 0) & (plan.n_events <= 4)).all()
    assert ((plan.snr_db[used] >= 5) & (plan.snr_db[used] <= 20)).all() and (plan.event_clip[~used] == -1).all()
    labels = plan.labels(lab)
    is_cough = used & (lab[np.maximum(plan.event_clip, 0)] == 1)
    assert labels.tolist() == is_cough.any(1).astype(int).tolist() and 0.45 < labels.mean() < 0.55
    n_coughs, n_others = is_cough.sum(1), (used & ~is_cough).sum(1)
    assert set(n_coughs.tolist()) == {0, 1, 2, 3} and set(n_others.tolist()) == {0, 1, 2} and 0.27 < (n_others > 0).mean() < 0.33
    for r in range(0, b, 97):                                    # the coughs take the first slots
        assert is_cough[r, :n_coughs[r]].all() and not is_cough[r, n_coughs[r]:].any()
    # rule 7 without a margin: at least min(1600, n_c) samples inside the row, every phase that allows
    n_c = el[np.maximum(plan.event_clip, 0)]
    inside = np.minimum(plan.onset + n_c, width) - np.maximum(plan.onset, 0)
    assert (inside[used] >= np.minimum(1600, n_c)[used]).all()
    assert (plan.onset[used] < 0).any() and ((plan.onset + n_c)[used] > width).any()
    for c in (0, 1, 2):                                          # both ends of the range are drawn
        mine = plan.onset[used & (plan.event_clip == c)]
        need = min(1600, int(el[c]))
        assert mine.min() <= need - el[c] + 40 and mine.min() >= need - el[c] and width - need - 40 <= mine.max() <= width - need
    none = cda.draw_window_plan(backgrounds, events, 500, width, SR, 4, p_cough=0.0, p_distractor=0.0)
    assert (none.n_events == 0).all() and (none.labels(lab) == 0).all()
    every = cda.draw_window_plan(backgrounds, events, 500, width, SR, 4, p_cough=1.0, p_distractor=1.0, coughs_per_window=(4, 4))
    assert (every.n_events == 4).all() and (every.labels(lab) == 1).all()
    silent = cda.draw_window_plan(cda.DeviceClipBank([], [], device="cpu"), events, 8, width, SR, 0)
    assert (silent.background == -1).all() and (silent.bg_start == 0).all()


# ------------------------------------------------------------------------------------------------ the inner-window rule
def _left_inside(a, b, width, shift, pair):
    """How many of the samples ``[a, b)`` of a row of ``width`` are still inside it after the time shift (zero fill), the
    warp about sample 0 by ``pair = (orig, new)`` and ``pad_or_trim``'s symmetric crop or pad -- exact integer
    arithmetic: a sample at x goes to x * new / orig, and the samples of [a, b) become the integer positions of [a * new /
    orig, b * new / orig)."""
    a, b = max(a, 0) + shift, min(b, width) + shift
    a, b = max(a, 0), min(b, width)
    if a >= b:
        return 0
    n = width
    if pair is not None:
        orig, new = pair
        a, b, n = -((-a * new) // orig), -((-b * new) // orig), -((-width * new) // orig)
        b = min(b, n)
    move = -((n - width) // 2) if n > width else (width - n) // 2
    return max(0, min(b + move, width) - max(a + move, 0))


@pytest.mark.parametrize("speed", [False, True])
@pytest.mark.parametrize("width", [8000, 16000, 32000])
def test_a_drawn_cough_survives_the_worst_the_chain_can_do(width, speed):
    """Every positive of 2000 drawn rows through the shifts +-int(0.2 * width) and 0, the rate pairs at both ends of
    ``speed_range`` (and none), and the crop or pad: at least ``m_c - 2`` samples of it are left inside the row, where
    ``m_c = min(m, length)`` is taken of the clip as the chain left it (``floor(n_c * new / orig)`` samples: a clip of
    400 samples played 10 % faster has 363 to show, whatever the composer does).  The same walk over a plan drawn with
    the margin set to 0 finds a violation: that guards this test."""
    aug = cda.AudioAugmentor(sample_rate=SR, speed=speed, speed_range=(0.9, 1.1))
    backgrounds, events = _banks(ev_lengths=(1600, 3000, 400, 9000, 40000, 2400), ev_labels=(1, 1, 1, 1, 1, 0))
    el, lab = events.lengths.numpy(), events.labels.numpy()
    margin, (rho_min, rho_max) = cda.edge_margin(aug, width), cwin.speed_ratios(aug)
    spread = max(abs(rho_min - 1), abs(rho_max - 1))
    assert margin == int(np.ceil(rho_max * 0.2 * width + width * spread / 2)) + 1 and cda.edge_margin(None, width) == 0
    assert (rho_min, rho_max) == ((SR / 17600, SR / 14400) if speed else (1.0, 1.0))
    pairs = [None] + ([cda.speed_rate_pair(f, SR) for f in aug.speed_range] if speed else [])
    shifts = (int(0.2 * width), -int(0.2 * width), 0)
    m = 1600

    def violations(plan):
        bad, used = 0, plan.used()
        for r, e in zip(*np.nonzero(used & (lab[np.maximum(plan.event_clip, 0)] == 1))):
            n_c, on = int(el[plan.event_clip[r, e]]), int(plan.onset[r, e])
            for pair in pairs:
                length = n_c if pair is None else n_c * pair[1] // pair[0]
                for s in shifts:
                    bad += _left_inside(on, on + n_c, width, s, pair) < min(m, length) - 2
        return bad

    kw = dict(p_cough=1.0, coughs_per_window=(1, 3), rho_min=rho_min)
    assert violations(cda.draw_window_plan(backgrounds, events, 2000, width, SR, 11, margin=margin, **kw)) == 0
    assert violations(cda.draw_window_plan(backgrounds, events, 2000, width, SR, 11, margin=0, **kw)) > 0


def test_an_inner_window_that_cannot_hold_the_overlap_raises():
    backgrounds, events = _banks()
    aug = cda.AudioAugmentor(sample_rate=SR, speed=True, speed_range=(0.9, 1.1))
    with pytest.raises(ValueError, match="inner window"):
        cda.draw_window_plan(backgrounds, events, 4, 3000, SR, 0, margin=cda.edge_margin(aug, 3000), rho_min=cwin.speed_ratios(aug)[0])
    assert len(cda.draw_window_plan(backgrounds, events, 4, 3000, SR, 0)) == 4               # the same row without the chain
    with pytest.raises(ValueError, match="inner window"):
        cda.draw_window_plan(backgrounds, events, 4, 1000, SR, 0)
    assert len(cda.draw_window_plan(backgrounds, events, 4, 1600, SR, 0)) == 4


# ------------------------------------------------------------------------------------------------ labels of windows
def _scores(per, hop, window):
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(per)]).astype(np.int64))
    n = int(offsets[-1])
    return cda.WindowScores(torch.zeros(n), torch.zeros(n, dtype=torch.float64), offsets, offsets, hop, window, SR, 3)


@pytest.mark.parametrize("hop,window", [(4000, 16000), (1000, 16000), (16000, 16000), (20000, 16000), (380, 220)])
def test_window_labels_equal_brute_force_and_the_truth_ranges(hop, window):
    backgrounds, events = _banks(ev_lengths=(1600, 3000, 800, 1, 5000, 100))
    el = events.lengths.numpy()
    plan = cda.draw_scene_plan(backgrounds, events, 6, 7.3, events_per_scene=(0, 7), min_gap_seconds=0.01, seed=hop)
    lengths = plan.length.copy()
    lengths[1], lengths[2] = window - 1, window                 # a recording without a window, one with exactly one
    keep = (plan.event_scene != 1) & (plan.event_scene != 2)
    truth = cda.TruthTable.from_intervals(plan.event_scene[keep], plan.onset[keep], (plan.onset + el[plan.event_clip])[keep], n_clips=6)
    for overlap in (0.1, 0.0, 0.01):
        m = R.min_overlap_samples(overlap, SR)
        if m > window:
            with pytest.raises(ValueError, match="more than a window"):
                cda.window_labels(truth, lengths, window, hop, SR, overlap)
            continue
        table = cda.window_labels(truth, lengths, window, hop, SR, overlap)
        want = []
        for c in range(6):
            mine = truth.clip == c
            brute = W.window_labels_brute(truth.onset[mine].tolist(), truth.offset[mine].tolist(), int(lengths[c]), window, hop, m)
            want += [(c, k, lab, ov) for k, (lab, ov) in enumerate(brute)]
        assert list(zip(table.recording.tolist(), table.window.tolist(), table.label.tolist(), table.overlap.tolist())) == want
        assert table.hop_samples == hop and table.window_samples == window
        # the windows labelled 1 are the union of the closed ranges the event-level matcher counts, without a collar
        per = [sum(1 for c2, *_ in want if c2 == c) for c in range(6)]
        k_lo, k_hi = cscenes.truth_window_ranges(truth, _scores(per, hop, window), overlap, collar_seconds=0.0)
        union = {(int(c), k) for c, lo, hi in zip(truth.clip, k_lo, k_hi) for k in range(int(lo), int(hi) + 1)}
        assert union == {(c, k) for c, k, lab, _ in want if lab == 1}
        if overlap == 0.1 and hop <= window:
            assert {lab for *_, lab, _ in want} == {1, 0, -1}


def test_window_labels_by_hand():
    truth = cda.TruthTable.from_intervals([0, 0], [20000, 60000], [44000, 60050], n_clips=2)
    table = cda.window_labels(truth, [160000, 20000], 16000, 4000, SR)
    assert len(table) == 37 + 2 and table.recording.tolist() == [0] * 37 + [1] * 2 and table.window.tolist() == list(range(37)) + [0, 1]
    lab = table.label[:37].tolist()
    # the long cough: windows 2..10 count (scenes_ref's hand case), 1 and 11 touch it by less than 1600 samples
    assert lab[:12] == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0] and table.overlap[1] == 0 and table.overlap[2] == 4000
    # 50 samples at 60000: the windows that hold all of it are 12..15 (k*4000 <= 60000 and k*4000 + 16000 >= 60050)
    assert lab[12:17] == [1, 1, 1, 1, 0] and table.overlap[12:16].tolist() == [50] * 4 and table.label[37:].tolist() == [0, 0]
    with pytest.raises(ValueError, match="clip_lengths holds 1 values, expected 2"):
        cda.window_labels(truth, [160000], 16000, 4000, SR)
    with pytest.raises(ValueError, match="hop_samples"):
        cda.window_labels(truth, [160000, 20000], 16000, 0, SR)


# ------------------------------------------------------------------------------------------------ the Python front
def test_host_held_bad_plans_raise_before_a_device_is_touched():
    backgrounds, events = _banks()                               # CPU banks: whatever reaches a kernel raises RuntimeError
    good = cda.draw_window_plan(backgrounds, events, 6, 16000, SR, 0, p_cough=1.0, p_distractor=1.0)

    def changed(**kw):
        fields = {f: getattr(good, f).copy() for f in FIELDS}
        fields.update(kw)
        return cda.WindowPlan(**fields)
    far = good.onset.copy()
    far[0, 0] = 2**31
    for plan, match in ((changed(background=np.array([0, 3, 0, 0, 0, 0])), "background indices"),
                        (changed(background=np.full(6, -2)), "background indices"),
                        (changed(bg_start=np.full(6, -1)), "row 0: bg_start=-1"),
                        (changed(bg_start=np.full(6, 48000)), "bg_start=48000"),
                        (changed(bg_gain=np.full(6, np.nan, np.float32)), "bg_gain"),
                        (changed(n_events=np.full(6, 5)), "n_events"), (changed(n_events=np.full(6, -1)), "n_events"),
                        (changed(event_clip=np.full((6, 4), 6)), "event clips"),
                        (changed(event_clip=np.full((6, 4), -1)), "event clips"),
                        (changed(onset=far), "int32"), (changed(snr_db=np.full((6, 4), np.inf)), "snr_db"),
                        (changed(onset=good.onset[:5]), "onset holds 20 values, expected 24")):
        with pytest.raises(ValueError, match=match):
            cda.compose_windows(backgrounds, events, plan, 16000)
    for width in (0, 2**20 + 1, 16000.0):
        with pytest.raises(ValueError, match="width"):
            cda.compose_windows(backgrounds, events, good, width)
    with pytest.raises(ValueError, match="WindowPlan"):
        cda.compose_windows(backgrounds, events, None, 16000)
    with pytest.raises(ValueError, match="event_power"):
        cda.compose_windows(backgrounds, events, good, 16000, event_power=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        cda.compose_windows(backgrounds, events, good, 16000, event_power=torch.zeros(6, dtype=torch.float64), out=torch.zeros(5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cda.compose_windows(backgrounds, events, good, 16000)
    # what a plan may hold: silence, events across both edges, over each other and outside the row
    odd = cda.WindowPlan(np.array([-1, 1]), np.array([0, 6]), np.array([1.0, 0.0], np.float32), np.array([4, 2]),
                         np.array([[0, 0, 1, 3], [4, 4, 0, 0]]), np.array([[-1599, 15999, 100, -5], [2**31 - 1, -2**31 + 1, 0, 0]]),
                         np.zeros((2, 4))).checked(backgrounds.lengths.numpy(), events.lengths.numpy(), 16000)
    assert odd.labels(events.labels).tolist() == [1, 0] and odd.event_clip[1].tolist() == [4, 4, -1, -1]
    rec = odd.records()
    assert rec.dtype.itemsize == 80 and rec["snr_linear"][0].tolist() == [1.0] * 4 and rec["onset"][1, 1] == -2**31 + 1
    for kw, match in ((dict(p_cough=1.5), "p_cough"), (dict(p_distractor=-0.1), "p_distractor"), (dict(coughs_per_window=(0, 2)), "coughs_per_window"),
                      (dict(coughs_per_window=(1, 5)), "coughs_per_window"), (dict(snr_range=(20, 5)), "lo <= hi"), (dict(seed=-1), "seed"),
                      (dict(b=-1), "b="), (dict(margin=-1), "margin"), (dict(rho_min=1.5), "rho_min"), (dict(min_overlap_seconds=-1), "negative"),
                      (dict(bg_gain_range=(1.0, float("inf"))), "finite")):
        args = dict(b=4, width=16000, sample_rate=SR, seed=0)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            cda.draw_window_plan(backgrounds, events, **args)
    only_others = events.subset([4, 5])
    with pytest.raises(ValueError, match="no clip labelled 1"):
        cda.draw_window_plan(backgrounds, only_others, 4, 16000, SR, 0)
    with pytest.raises(ValueError, match="no clip labelled 0"):
        cda.draw_window_plan(backgrounds, events.subset([0, 1]), 4, 16000, SR, 0, p_distractor=0.5)
    assert (cda.draw_window_plan(backgrounds, events.subset([0, 1]), 50, 16000, SR, 0).n_events <= 2).all()


# ------------------------------------------------------------------------------------------------ the library
def _header():
    return open(os.path.join(ROOT, "include", f"cough_amd_{NAME}.h")).read()


def _declared():
    return set(re.findall(r"^(?:int|size_t|const char\*|void) (cough_[a-z_0-9]+)\s*\(", _header(), flags=re.M))


def _exported(path):
    nm = shutil.which("nm") or os.path.join(os.path.dirname(os.path.realpath(cbuild._hipcc())), "..", "lib", "llvm", "bin", "llvm-nm")
    out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_library_is_in_the_open_tables():
    assert NAME in _lib.OPEN and NAME in cbuild.OPEN_UNITS and NAME in cbuild.OPEN_LIBS
    assert NAME not in _lib.LIBRARIES and NAME not in _lib.LATER and NAME not in cbuild.UNITS and NAME not in cbuild.LATER_UNITS
    assert cbuild.OPEN_UNITS[NAME] == (NAME + ".hip",) and NAME + ".hip" not in cbuild.SOURCES
    for f in (NAME + ".hip", f"exports_{NAME}.map"):
        assert os.path.exists(os.path.join(cbuild.CSRC, f)), f
    assert os.path.basename(cbuild.OPEN_LIBS[NAME]) == f"libcough_amd_{NAME}.so" == _lib.OPEN[NAME].soname
    assert os.path.exists(cbuild.OPEN_LIBS[NAME])


def test_header_record_and_file_name_the_same_entry_points():
    rec, text, declared = _lib.OPEN[NAME], _header(), _declared()
    assert declared == set(rec.symbols) == set(rec.prototypes) == {"cough_windows_abi_version", "cough_windows_last_error",
                                                                  "cough_compose_windows"}
    assert rec.symbols[0] == rec.abi_symbol and rec.symbols[1] == rec.error_symbol
    assert _exported(rec.path) == declared, sorted(_exported(rec.path) ^ declared)
    assert _lib.WINDOWS_SYMBOLS is rec.symbols and _lib.load_windows == rec.load and _lib.check_windows == rec.check
    lib = rec.load()
    assert getattr(lib, rec.abi_symbol)() == rec.abi == 1 and "#define COUGH_WINDOWS_ABI_VERSION 1\n" in text
    assert isinstance(getattr(lib, rec.error_symbol)(), bytes)
    for other in (*_lib.LIBRARIES.values(), *_lib.LATER.values(), *(r for r in _lib.OPEN.values() if r.name != NAME)):
        assert not declared & set(other.symbols), other.name
    assert re.search(rf"#define COUGH_WINDOWS_MAX_EVENTS {cwin.MAX_EVENTS}\b", text) and W.MAX_EVENTS == cwin.MAX_EVENTS
    assert re.search(r"#define COUGH_WINDOWS_MAX_WIDTH \(1 << 20\)", text) and cwin.MAX_WIDTH == 1 << 20
    assert re.search(rf"#define COUGH_WINDOWS_THREADS {W.THREADS}\b", text)
    for symbol, (_, argtypes) in rec.prototypes.items():
        params = re.search(rf"\b{symbol}\s*\(([^)]*)\)", text).group(1)
        count = 0 if params.strip() == "void" else params.count(",") + 1
        assert count == (len(argtypes) if argtypes else 0), symbol
    # the plan's layout as the header words it: the field order of the host's record type, 80 bytes
    struct = re.search(r"typedef struct cough_window_plan \{(.*?)\} cough_window_plan;", text, flags=re.S).group(1)
    assert re.findall(r"\b(\w+)(?:\[\w+\])?;", struct) == ["background", "bg_start", "bg_gain", "n_events", "clip", "onset", "snr_linear"]
    assert [cwin.PLAN_DTYPE.fields[f][1] for f in cwin.PLAN_DTYPE.names] == [0, 4, 8, 12, 16, 32, 48] and cwin.PLAN_DTYPE.itemsize == 80


def test_the_c_abi_checks_its_arguments():
    lib = _lib.load_windows()
    err = lambda: lib.cough_windows_last_error().decode()
    #       bg n_bg off len n  ev n_ev off len p_ev n  plans rows width out p_bg gains stream
    good = [8, 1, 8, 8, 1, 8, 1, 8, 8, 8, 1, 8, 0, 16000, 8, None, None, None]
    assert lib.cough_compose_windows(*good) == _lib.OK                                       # n_rows == 0 launches nothing
    assert lib.cough_compose_windows(None, 0, None, None, 0, None, 0, None, None, None, 0, None, 0, 1, None, None, None, None) == _lib.OK
    for at, value, match in ((12, -1, "negative"), (4, -1, "negative"), (10, -1, "negative"), (1, -1, "negative"), (6, -1, "negative"),
                             (13, 0, "width"), (13, 2**20 + 1, "width")):
        args = list(good)
        args[at] = value
        assert lib.cough_compose_windows(*args) == _lib.EINVAL and match in err(), (at, err())
    one = list(good)
    one[12] = 1
    for at, value, match in ((11, None, "NULL argument"), (14, None, "NULL argument"), (2, None, "NULL background tables"),
                             (0, None, "d_bg is NULL"), (9, None, "NULL event tables"), (5, None, "d_ev is NULL"),
                             (0, 2, "4-byte aligned"), (14, 6, "4-byte aligned"), (16, 2, "4-byte aligned"),
                             (7, 4, "8-byte aligned"), (11, 4, "8-byte aligned"), (15, 4, "8-byte aligned"),
                             (14, 64008, "overlaps"), (5, 8 + 15999 * 4, "overlaps")):
        args = list(one)
        args[at] = value
        if match == "overlaps":
            args[0], args[1] = 64000, 16000                                                  # a bank of 64000 bytes at 64000
        assert lib.cough_compose_windows(*args) == _lib.EINVAL and match in err(), (at, err())


def test_the_package_exports_the_names():
    names = ["WindowPlan", "WindowLabels", "draw_window_plan", "edge_margin", "compose_windows", "ComposedWindowLoader",
             "window_labels", "scene_window_bank"]
    for name in names:
        assert name in cda.__all__ and getattr(cda, name) is getattr(cwin, name), name
    assert len(set(cda.__all__)) == len(cda.__all__)
    doc = cwin.__doc__
    assert all(f"\n{k}. " in doc for k in range(1, 9)) and "Philox(seed)" in doc
