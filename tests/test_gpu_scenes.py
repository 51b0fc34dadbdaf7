"""Scenes on the MI355X (cough_detector_amd/scenes.py, csrc/scenes.hip) against tests/scenes_ref.py.

Tolerances.  Powers: every term ``double(x)^2`` is exact and non-negative, so a sum of n of them in ANY order is within
``(n - 1) * 2^-53`` relative of the exact sum, numpy's pairwise sum too, and the division adds ``2^-53``: the two float64
results differ by at most ``2 * n * 2^-53 * P``.  Gains: the reference evaluates the same float64 expression on the
device's own powers; a float64 ``sqrt`` one ulp off moves the float32 result by at most one float32 ulp.  Mix: one rounded
product and one fmaf per sample on both sides, bit for bit on the device's own gains.  Measured SNR: the gain is a float32
(``2^-24`` relative, squared: ``2^-23``) and every scene sample is rounded to float32 once (``2^-24`` of a value about
``sqrt(1 + 1/snr)`` times the event's, averaged over the span), far inside ``1e-5``.  The matcher's outputs are integers:
no tolerance.
"""
import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import scenes as cscenes
import scenes_calls as K
import scenes_ref as R
import score_ref as S

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
HOP, WINDOW, SR = 4000, 16000, 16000


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.int64)


def _bank(clips, label=0):
    return cda.DeviceClipBank([torch.from_numpy(c) for c in clips], [label] * len(clips), device="cuda")


# ------------------------------------------------------------------------------------------------ powers
POWER_CLIPS = [1, 7, 16000, 40000, 257]
SPAN_LENGTHS = [0, 1, 255, 256, 257, 4097, 40000]


@pytest.fixture(scope="module")
def power_case():
    rng = np.random.default_rng(0)
    clips = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 0)).astype(np.float32) for n in POWER_CLIPS]
    spans = [(c, 0, n) for c in range(len(clips)) for n in SPAN_LENGTHS]                 # clips of 1, 7, 257 wrap many times
    spans += [(c, len(clips[c]) - 1, n) for c in range(len(clips)) for n in (1, 2, 300, 40000)]   # from the last sample on
    spans += [(2, 15990, 16000 * 2 + 21), (1, 3, 7 * 5), (3, 123, 39877)]
    clip, start, length = (np.array(v) for v in zip(*spans))
    bank = _bank(clips)
    return clips, bank, clip, start, length, cscenes.span_power(bank, clip, start, length).cpu().numpy()


def test_span_powers_are_within_the_summation_bound(power_case):
    clips, _, clip, start, length, got = power_case
    assert got.dtype == np.float64
    for r in range(len(clip)):
        want = R.power_ref(clips[clip[r]], int(start[r]), int(length[r]))
        assert abs(got[r] - want) <= 2 * int(length[r]) * 2.0 ** -53 * want, (r, clip[r], start[r], length[r], got[r], want)
        assert length[r] or got[r] == 0.0


def test_a_span_alone_gives_the_bits_it_gives_in_a_batch(power_case):
    _, bank, clip, start, length, got = power_case
    for r in (3, 6, 13, 20, len(clip) - 3, len(clip) - 1):
        alone = cscenes.span_power(bank, clip[r:r + 1], start[r:r + 1], length[r:r + 1]).cpu().numpy()
        assert _bits(alone).tolist() == _bits(got[r:r + 1]).tolist(), r
    again = cscenes.span_power(bank, clip[::-1].copy(), start[::-1].copy(), length[::-1].copy()).cpu().numpy()
    assert _bits(again[::-1]).tolist() == _bits(got).tolist()


def test_a_nan_or_inf_sample_gives_a_non_finite_power():
    x = np.ones(1000, dtype=np.float32)
    y = x.copy()
    y[700] = np.nan
    z = x.copy()
    z[3] = np.inf
    got = cscenes.span_power(_bank([x, y, z]), [0, 1, 1, 2, 2], [0, 0, 701, 0, 4], [1000, 1000, 299, 4, 999]).cpu().numpy()
    assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == 1.0 and got[3] == np.inf and got[4] == 1.0


# ------------------------------------------------------------------------------------------------ gains and the mix
SCENE_LENGTHS = [1, 255, 4097, 16000, 40000, 4097, 255, 9000]


@pytest.fixture(scope="module")
def mix_case():
    """Eight scenes by hand: backgrounds shorter than the scene (wraps inside a tile and across tiles) and longer;
    events at onset 0, ending exactly at L, of length 1, straddling the tile boundaries at 4096 and 8192; a scene
    without events; a NaN background (scene 6) and a silent one (scene 7); an all-zero event."""
    rng = np.random.default_rng(1)
    bgs = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (7, 1, 16000, 100003, 5001, 333)]
    bgs[5][100] = np.nan
    bgs.append(np.zeros(50, dtype=np.float32))
    evs = [rng.standard_normal(n).astype(np.float32) for n in (1, 30, 255, 1601, 4000, 12)]
    evs.append(np.zeros(20, dtype=np.float32))
    evs.append(np.full(1, 0.25, dtype=np.float32))
    #                scene: background, bg_start, bg_gain
    scenes = [(1, 0, 1.0), (0, 6, 0.5), (4, 5000, 1.0), (2, 15999, 2.0), (3, 77, 1.0), (0, 3, 1.0), (5, 0, 1.0), (6, 10, 1.0)]
    #         (scene, event clip, onset, snr_db)
    events = [(0, 0, 0, 10.0),
              (1, 1, 0, 5.0), (1, 0, 30, 20.0), (1, 5, 243, 7.5),
              (2, 2, 0, 12.0), (2, 1, 4066, 6.0), (2, 0, 4096, 15.0),
              (4, 3, 3000, 5.0), (4, 4, 8000, 10.0), (4, 2, 12000, 20.0), (4, 6, 20000, 10.0), (4, 3, 38399, 8.0),
              (5, 4, 97, 9.0),
              (6, 1, 10, 10.0),
              (7, 5, 100, 10.0), (7, 1, 8180, 10.0)]
    plan = cda.ScenePlan(np.array([s[0] for s in scenes]), np.array([s[1] for s in scenes]),
                         np.array([s[2] for s in scenes], np.float32), np.array(SCENE_LENGTHS),
                         *(np.array(v) for v in zip(*events)))
    bg_bank, ev_bank = _bank(bgs), _bank(evs, 1)
    bank, truth = cda.compose_scenes(bg_bank, ev_bank, plan)
    p_bg = cscenes.span_power(bg_bank, plan.background, plan.bg_start, plan.length).cpu().numpy()
    p_ev = cscenes.span_power(ev_bank, np.arange(len(evs)), np.zeros(len(evs), int), [len(e) for e in evs]).cpu().numpy()
    return dict(bgs=bgs, evs=evs, plan=plan, bank=bank, truth=truth, p_bg=p_bg, p_ev=p_ev,
                out=bank.data.cpu().numpy(), gain=truth.gain.cpu().numpy())


def test_gains_are_within_one_ulp_of_the_restatement_on_the_devices_powers(mix_case):
    c, plan = mix_case, mix_case["plan"]
    assert c["gain"].dtype == np.float32 and len(c["gain"]) == len(plan.onset)
    for e in range(len(plan.onset)):
        s, q = int(plan.event_scene[e]), int(plan.event_clip[e])
        want = R.gain_ref(10.0 ** (plan.snr_db[e] / 10.0), plan.bg_gain[s], c["p_bg"][s], c["p_ev"][q])
        assert abs(float(c["gain"][e]) - float(want)) <= float(np.spacing(want)), (e, c["gain"][e], want)
    by = {(int(s), int(q)): float(g) for s, q, g in zip(plan.event_scene, plan.event_clip, c["gain"])}
    assert by[(6, 1)] == 1.0 and np.isnan(c["p_bg"][6])                   # a NaN background
    assert by[(7, 5)] == 1.0 and by[(7, 1)] == 1.0 and c["p_bg"][7] == 0.0   # a silent background
    assert by[(4, 6)] == 1.0 and c["p_ev"][6] == 0.0                       # an all-zero event
    assert by[(0, 0)] != 1.0


def test_the_mix_equals_the_restatement_bit_for_bit(mix_case):
    c, plan, truth = mix_case, mix_case["plan"], mix_case["truth"]
    bank = c["bank"]
    assert bank.lengths.tolist() == SCENE_LENGTHS and bank.labels.tolist() == [1, 1, 1, 0, 1, 1, 1, 1]
    assert truth.counts.tolist() == [1, 3, 3, 0, 5, 1, 1, 2] and truth.clip.tolist() == plan.event_scene.tolist()
    assert truth.onset.tolist() == plan.onset.tolist() and truth.source.tolist() == plan.event_clip.tolist()
    assert (truth.offset - truth.onset).tolist() == [len(c["evs"][q]) for q in plan.event_clip]
    assert {int(o) % 4 for o in bank.offsets} == {0, 1, 2} and {int(o) % 4 for o in truth.onset} == {0, 1, 2, 3}
    for s in range(len(plan)):
        mine = np.flatnonzero(plan.event_scene == s)
        events = [(int(plan.onset[e]), c["evs"][plan.event_clip[e]], c["gain"][e]) for e in mine]
        want = R.mix_slices(c["bgs"][plan.background[s]], int(plan.bg_start[s]), plan.bg_gain[s], SCENE_LENGTHS[s], events)
        o = int(bank.offsets[s])
        got = c["out"][o:o + SCENE_LENGTHS[s]]
        if s == 6:                                                         # the NaN reaches this scene, and only it
            assert np.isnan(got).any() and np.array_equal(np.isnan(got), np.isnan(want))
            assert _bits(got[~np.isnan(got)]).tolist() == _bits(want[~np.isnan(want)]).tolist()
        else:
            assert not np.isnan(got).any() and np.array_equal(_bits(got), _bits(want)), s
    small = R.mix_loop(c["bgs"][0], 6, 0.5, 255, [(int(plan.onset[e]), c["evs"][plan.event_clip[e]], c["gain"][e]) for e in (1, 2, 3)])
    o = int(bank.offsets[1])
    assert np.array_equal(_bits(c["out"][o:o + 255]), _bits(small))


def test_the_measured_snr_is_the_planned_one(mix_case):
    c, plan, bank = mix_case, mix_case["plan"], mix_case["bank"]
    checked = 0
    for e in range(len(plan.onset)):
        s, q = int(plan.event_scene[e]), int(plan.event_clip[e])
        if s in (6, 7) or q == 6:                                          # the fallbacks have no SNR
            continue
        o, on, n = int(bank.offsets[s]), int(plan.onset[e]), len(c["evs"][q])
        bg = np.float32(plan.bg_gain[s]) * R.span_ref(c["bgs"][plan.background[s]], int(plan.bg_start[s]), SCENE_LENGTHS[s])
        added = c["out"][o + on:o + on + n].astype(np.float64) - bg[on:on + n].astype(np.float64)
        p_bg = np.mean(bg.astype(np.float64) ** 2)
        measured = np.mean(added ** 2) / p_bg
        want = 10.0 ** (plan.snr_db[e] / 10.0)
        assert abs(measured - want) <= 1e-5 * want, (e, measured, want)
        checked += 1
    assert checked == 12


@pytest.mark.parametrize("n_bg", [1100, 1000])
def test_every_phase_of_the_three_pointers(n_bg):
    """64 scenes in one launch: background, event and output each at every offset mod 4.  A scene is one tile and 37
    samples long, its background wraps three to four times, one event lies early and one straddles sample 4096.  A
    background of 1100 samples is split at its wrap points and read 16 bytes at a time; one of 1000 samples is under the
    kernel's threshold of 1024 and read through a cyclic index per thread."""
    rng = np.random.default_rng(3)
    L, n_e1, n_e2 = cscenes.TILE + 37, 9, 30
    combos = [(pb, pe, po) for pb in range(4) for pe in range(4) for po in range(4)]
    bg = rng.standard_normal(64 * (n_bg + 4) + 8).astype(np.float32)
    ev = rng.standard_normal(64 * 48 + 8).astype(np.float32)
    bg_off = np.array([(n_bg + 4) * k + pb for k, (pb, _, _) in enumerate(combos)])
    e1_off = np.array([48 * k + pe for k, (_, pe, _) in enumerate(combos)])
    e2_off = e1_off + n_e1 + 1                                            # the second event on the next phase
    out_off = np.array([(L + 7) // 4 * 4 * k + po for k, (_, _, po) in enumerate(combos)])
    n_out = int(out_off[-1]) + L + 4
    starts = rng.integers(0, n_bg, 64)
    gains = rng.uniform(0.5, 2.0, 128).astype(np.float32)
    bg_gain = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    onsets = np.tile([3, cscenes.TILE - 6], 64)
    out = torch.full((n_out,), -7.0, dtype=torch.float32, device="cuda")
    bg_dev, ev_dev = K.dev(bg, np.float32), K.dev(ev, np.float32)
    K.mix_scenes(bg_dev.data_ptr(), bg.size, bg_off, np.full(64, n_bg), starts, bg_gain, np.full(64, L), out_off,
                 np.arange(65) * 2, ev_dev.data_ptr(), ev.size, np.stack([e1_off, e2_off], 1).reshape(-1),
                 np.tile([n_e1, n_e2], 64), onsets, gains, cscenes.scene_tiles(np.full(64, L)), out.data_ptr(), n_out)
    got = out.cpu().numpy()
    covered = np.zeros(n_out, dtype=bool)
    for k in range(64):
        events = [(3, ev[e1_off[k]:e1_off[k] + n_e1], gains[2 * k]), (cscenes.TILE - 6, ev[e2_off[k]:e2_off[k] + n_e2], gains[2 * k + 1])]
        want = R.mix_slices(bg[bg_off[k]:bg_off[k] + n_bg], int(starts[k]), bg_gain[k], L, events)
        assert np.array_equal(_bits(got[out_off[k]:out_off[k] + L]), _bits(want)), combos[k]
        covered[out_off[k]:out_off[k] + L] = True
    assert (got[~covered] == -7.0).all()                                   # nothing between the scenes was written


# ------------------------------------------------------------------------------------------------ the matcher
PER_CLIP = [0, 1, 63, 64, 65, 200, 130]


@pytest.fixture(scope="module")
def match_case():
    rng = np.random.default_rng(4)
    probs = []
    for n in PER_CLIP:
        p = np.clip(0.5 + 0.5 * np.sin(np.arange(n) / 5.0 + rng.uniform(0, 6)) + rng.normal(0, 0.1, n), 0, 1).astype(np.float32)
        probs.append(p)
    probs[3][:] = np.linspace(0, 1, 64, dtype=np.float32)                 # a ramp
    probs[4][10:30] = 0.75                                                 # a plateau
    probs[5][50] = np.nan
    probs[5][120:140] = 1.0
    probs[6][::7] = np.nan
    scores = cda.WindowScores.from_probabilities(np.concatenate(probs), PER_CLIP, HOP, WINDOW, SR, 3)
    lengths = [WINDOW + (n - 1) * HOP + 123 if n else 9000 for n in PER_CLIP]
    clip, onset, offset = [], [], []
    for c, n in enumerate(lengths):
        if c == 0:                                                         # a cough in the recording without a window
            clip.append(0), onset.append(100), offset.append(5000)
            continue
        at = int(rng.integers(0, 3000))
        while True:
            a = at + int(rng.integers(0, 60000))
            b = a + int(rng.integers(50, 30000))
            if b > n:
                break
            clip.append(c), onset.append(a), offset.append(b)
            at = b + int(rng.integers(0, 3) == 0) * 20000
    truth = cda.TruthTable.from_intervals(clip, onset, offset, n_clips=len(PER_CLIP))
    smoothed = np.split(scores.smoothed.cpu().numpy(), np.cumsum(PER_CLIP)[:-1])
    return scores, truth, smoothed


@pytest.mark.parametrize("n_thr", [1, 64, 65, 1024])
@pytest.mark.parametrize("debounce", [0.0, 0.5, 1000.0])
def test_the_matcher_equals_the_restatement(match_case, n_thr, debounce):
    scores, truth, smoothed = match_case
    thresholds = np.array([0.5]) if n_thr == 1 else np.concatenate([np.linspace(0.01, 0.99, n_thr - 3), [0.0, 1.0, 1.5]])
    sweep = cda.match_events(scores, truth, thresholds, debounce_seconds=debounce)
    assert sweep.gap == S.gap_ref(debounce, SR, HOP) == {0.0: 1, 0.5: 2, 1000.0: 4000}[debounce]
    want = R.match_ref(smoothed, thresholds, sweep.gap, truth.offsets, sweep.k_lo, sweep.k_hi, truth.onset, HOP, WINDOW,
                       S.events_ref)
    for name, got in (("hits", sweep.hits), ("false_alarms", sweep.false_alarms), ("repeats", sweep.repeats),
                      ("latency", sweep.latency_samples)):
        assert got.shape == (len(PER_CLIP), n_thr) and got.dtype == (torch.int64 if name == "latency" else torch.int32)
        assert np.array_equal(got.cpu().numpy(), want[name]), name
    counts = cda.sweep_thresholds(scores, thresholds, debounce_seconds=debounce).counts
    assert torch.equal(sweep.hits + sweep.repeats + sweep.false_alarms, counts)
    assert int(sweep.hits[0].sum()) == 0                                   # no window, no hit
    if debounce == 0.0 and n_thr > 1:                                      # the case holds all three classes
        assert min(int(sweep.hits.sum()), int(sweep.repeats.sum()), int(sweep.false_alarms.sum())) > 0


def test_list_matches_agrees_with_the_sweep(match_case):
    scores, truth, smoothed = match_case
    for threshold, debounce in ((0.5, 0.0), (0.3, 0.5), (0.9, 0.25), (1.5, 0.5)):
        sweep = cda.match_events(scores, truth, [threshold], debounce_seconds=debounce)
        events = cda.detect_events(scores, threshold, debounce_seconds=debounce)
        window, classes = cscenes.list_matches(scores, truth, threshold, debounce_seconds=debounce, event_counts=events.counts)
        window, classes, clip = window.cpu().numpy(), classes.cpu().numpy(), events.clip.cpu().numpy()
        per = np.bincount(truth.clip[window >= 0], minlength=len(PER_CLIP))
        assert per.tolist() == sweep.hits[:, 0].tolist()
        for cls, t in ((R.HIT, sweep.hits), (R.REPEAT, sweep.repeats), (R.FALSE_ALARM, sweep.false_alarms)):
            assert np.bincount(clip[classes == cls], minlength=len(PER_CLIP)).tolist() == t[:, 0].tolist()
        fired = np.split(events.window.cpu().numpy(), np.cumsum(events.counts.numpy())[:-1])
        offs = truth.offsets
        for c in range(len(PER_CLIP)):
            want_cls, want_hit = R.match_walk(fired[c].tolist(), sweep.k_lo[offs[c]:offs[c + 1]].tolist(),
                                              sweep.k_hi[offs[c]:offs[c + 1]].tolist())
            assert window[offs[c]:offs[c + 1]].tolist() == want_hit and classes[clip == c].tolist() == want_cls
        only, none = cscenes.list_matches(scores, truth, threshold, debounce_seconds=debounce)
        assert none is None and only.cpu().numpy().tolist() == window.tolist()


def test_a_cough_between_two_windows_is_a_miss_whatever_the_collar():
    """Windows side by side (hop = window): the cough across the seam of windows 1 and 2 overlaps neither by 0.1 s.  Every
    window fires; none may hit it, with the default collar of 2 windows or a longer one, and the cough behind it is hit."""
    scores = cda.WindowScores.from_probabilities(np.ones(6, np.float32), [6], WINDOW, WINDOW, SR, 3)
    truth = cda.TruthTable.from_intervals([0, 0], [31000, 50000], [33400, 60000], n_clips=1)
    for collar in (None, 0.0, 3.0):
        sweep = cda.match_events(scores, truth, [0.5], debounce_seconds=0.0, collar_seconds=collar)
        assert (sweep.k_lo.tolist(), sweep.k_hi[0]) == ([2, 3], 1) and sweep.gap == 1
        assert (sweep.hits.item(), sweep.repeats.item(), sweep.false_alarms.item()) == (1, int(sweep.k_hi[1]) - 3, 5 - (int(sweep.k_hi[1]) - 3))
        assert sweep.latency_samples.item() == 3 * WINDOW + WINDOW - 50000
        window, _ = cscenes.list_matches(scores, truth, 0.5, debounce_seconds=0.0, collar_seconds=collar)
        assert window.tolist() == [-1, 3]


# ------------------------------------------------------------------------------------------------ end to end
def test_compose_score_match_and_report():
    rng = np.random.default_rng(6)
    torch.manual_seed(0)
    backgrounds = _bank([(rng.standard_normal(n) * 0.05).astype(np.float32) for n in (30000, 48001, 7000)])
    coughs = _bank([(rng.standard_normal(n) * np.hanning(n)).astype(np.float32) for n in (6000, 9001, 12000)], 1)
    plan = cda.draw_scene_plan(backgrounds, coughs, 6, 5.0, events_per_scene=(0, 3), min_gap_seconds=0.3, seed=5)
    scenes, truth = cda.compose_scenes(backgrounds, coughs, plan)
    assert len(scenes) == 6 and scenes.labels.tolist() == (truth.counts > 0).astype(int).tolist() and len(truth) == len(plan.onset)
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1)
    pipe = cda.CoughPipeline(cda.AudioPreprocessor(device="cuda", **SHIPPED), model.cuda().eval())
    scores = cda.score_bank(scenes, pipe, batch=16)
    lo, hi = float(scores.smoothed.min()), float(scores.smoothed.max())
    thresholds = np.concatenate([[0.0], np.linspace(lo, hi, 9), [1.5]])
    sweep = cda.match_events(scores, truth, thresholds)
    counts = cda.sweep_thresholds(scores, thresholds).counts
    assert torch.equal(sweep.hits + sweep.repeats + sweep.false_alarms, counts) and int(counts[:, 0].sum()) > 0
    report = cda.event_report(scenes, scores, sweep, truth)
    free = torch.from_numpy(truth.counts == 0).cuda()
    assert report["hits"] == sweep.hits.sum(0).tolist() and report["false_alarms"] == sweep.false_alarms.sum(0).tolist()
    assert report["repeats"] == sweep.repeats.sum(0).tolist() and report["latency_samples"] == sweep.latency_samples.sum(0).tolist()
    assert report["false_alarms_event_free"] == sweep.false_alarms[free].sum(0).tolist()
    assert report["truth_events"] == len(truth) and report["misses"] == [len(truth) - h for h in report["hits"]]
    assert report["minutes"] == 6 * 5.0 / 60 and report["minutes_event_free"] == int((truth.counts == 0).sum()) * 5.0 / 60
    assert report["recall"] == [h / len(truth) for h in report["hits"]] and report["hits"][-1] == 0
    assert report["false_alarms_per_minute"] == [v / report["minutes"] for v in report["false_alarms"]]
    assert report["mean_latency_seconds"][-1] is None
    assert cda.pick_threshold(report)["threshold"] is not None            # nothing fires at 1.5
    assert cda.detection_report(scenes, scores, cda.sweep_thresholds(scores, thresholds))["labels"]["cough"]["recordings"] == \
        int((truth.counts > 0).sum())

    # the missed coughs at a threshold in the middle: the planned source times its gain, plus the background
    t = float(thresholds[5])
    missed, which = cda.missed_events(scenes, truth, scores, t)
    window, _ = cscenes.list_matches(scores, truth, t)
    assert which.tolist() == np.flatnonzero(window.cpu().numpy() < 0).tolist() and len(missed) == len(which)
    assert len(truth) - len(which) == int(cda.match_events(scores, truth, [t]).hits.sum())
    everything, every = cda.missed_events(scenes, truth, scores, 1.5)    # at 1.5 nothing is hit: every cough comes back
    assert every.tolist() == list(range(len(truth))) and everything.labels.tolist() == [1] * len(truth)
    gains, data = truth.gain.cpu().numpy(), everything.data.cpu().numpy()
    for j in range(len(truth)):
        s, q = int(truth.clip[j]), int(truth.source[j])
        src = coughs.clip(q)[0].cpu().numpy()
        bg = backgrounds.clip(int(plan.background[s]))[0].cpu().numpy()
        bgs = np.float32(plan.bg_gain[s]) * R.span_ref(bg, int(plan.bg_start[s]) + int(truth.onset[j]), len(src))
        o = int(everything.offsets[j])
        assert np.array_equal(_bits(data[o:o + len(src)]), _bits(R.fmaf(gains[j], src, bgs))), j
    if len(which):
        o, j = int(missed.offsets[0]), int(which[0])
        n = int(truth.offset[j] - truth.onset[j])
        assert np.array_equal(missed.data[o:o + n].cpu().numpy(), data[int(everything.offsets[j]):int(everything.offsets[j]) + n])


def test_empty_plans_and_banks_launch_nothing_wrong():
    backgrounds, coughs = _bank([np.ones(10, np.float32)]), _bank([np.ones(4, np.float32)], 1)
    scenes, truth = cda.compose_scenes(backgrounds, coughs, cda.draw_scene_plan(backgrounds, coughs, 0, 1.0))
    assert len(scenes) == 0 and len(truth) == 0 and scenes.data.numel() == 0
    scenes, truth = cda.compose_scenes(backgrounds, coughs, cda.draw_scene_plan(backgrounds, coughs, 2, 0.002, events_per_scene=(0, 0)))
    assert scenes.labels.tolist() == [0, 0] and truth.gain.numel() == 0
    assert scenes.data.cpu().tolist() == [1.0] * (2 * int(scenes.lengths[0])) and int(scenes.lengths[0]) >= 31
    scores = cda.WindowScores.from_probabilities(torch.zeros(0), [0, 0], HOP, WINDOW, SR, 3)
    sweep = cda.match_events(scores, truth, [0.1, 0.5])
    assert sweep.hits.tolist() == sweep.false_alarms.tolist() == sweep.repeats.tolist() == sweep.latency_samples.tolist() == [[0, 0]] * 2
    window, classes = cscenes.list_matches(scores, truth, 0.5, event_counts=[0, 0])
    assert window.numel() == 0 and classes.numel() == 0
