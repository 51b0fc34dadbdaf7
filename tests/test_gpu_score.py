"""Offline scoring on the MI355X (cough_detector_amd/score.py, csrc/score.hip) against tests/score_ref.py.

Decisions.  The device smooths in numpy's summation order, so ``smoothed`` must equal ``float(np.mean(deque))`` bit for
bit (compared as int64 views, NaN positions included); every decision downstream compares those same float64 bits with
the same float64 thresholds, so counts, first windows, peaks, event tables and the report's integers admit no tolerance
and no case is excluded.  Event times are ``(k*hop + window) / sr``: an exact integer and one IEEE division on both
sides.  Only the report's per-minute rates are quotients formed twice (1e-12 relative).

End to end.  ``score_bank`` gathers windows at any element offset and runs the existing pipeline in batches that cross
recordings; the pipeline is batch-invariant (tests/test_gpu_pipeline.py), so the probabilities must equal
``pipeline.predict`` on the same windows sliced on the host, bit for bit.  The live engine sees the same windows one per
push; its Python ``sum(history) / len(history)`` may differ from numpy's mean in the last bit, so the threshold sits in
the middle of a gap of more than 1e-6 between two smoothed values and the confidences are compared to 1e-12.
"""
import math

import numpy as np
import pytest
import torch

import cough_detector_amd as cda
from cough_detector_amd import synth
import score_ref as R

pytestmark = pytest.mark.gpu
SHIPPED = dict(use_pcen=False, use_pre_emphasis=False, use_delta_delta=False, use_spectral_contrast=False)
HOP, WINDOW, SR = 4000, 16000, 16000
WINDOWS = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 128, 129, 1000, 5000]
ALL_HALF, NAN_AT_5, ALL_NAN = 64, 128, 9                                 # the recordings (by window count) with a special content
SMOOTHING = [1, 3, 7, 8, 9, 32]
THRESHOLD_COUNTS = [1, 64, 65, 130]
DEBOUNCES = [0.0, 0.25, 0.5, 0.6, 10.0]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _thresholds(count):
    if count == 1:
        return np.array([0.5])
    return np.concatenate([np.linspace(0.01, 0.99, count - 4), [0.0, 0.5, 1.0, 1.5]])


# ------------------------------------------------------------------------------------------------ synthetic probabilities
class Synthetic:
    """Seeded probabilities for the window counts of WINDOWS in one order, and every reference computed once."""

    def __init__(self, order):
        self.per_clip = WINDOWS if order == "in_order" else WINDOWS[::-1]
        rng = np.random.default_rng(11 if order == "in_order" else 12)
        self.probs = []
        for n in self.per_clip:
            # slow swells, so that neighbouring windows agree and the smoothed values spread over 0..1
            p = np.clip(0.5 + 0.5 * np.sin(np.arange(n) / 9.0 + rng.uniform(0, 6)) + rng.normal(0, 0.15, n), 0, 1).astype(np.float32)
            p[rng.random(n) < 0.05] = 0.0
            p[rng.random(n) < 0.05] = 0.5
            p[rng.random(n) < 0.05] = 1.0
            if n == ALL_HALF:
                p[:] = 0.5
            if n == NAN_AT_5:
                p[5] = np.nan
            if n == ALL_NAN:
                p[:] = np.nan
            self.probs.append(p)
        self.labels = [k % 2 for k in range(len(self.per_clip))]
        self.lengths = [3 * (n + 1) for n in self.per_clip]              # the report reads lengths and labels only
        self._scores, self._smoothed, self._sweeps = {}, {}, {}

    def scores(self, w):
        if w not in self._scores:
            self._scores[w] = cda.WindowScores.from_probabilities(np.concatenate(self.probs), self.per_clip, HOP, WINDOW, SR, w)
        return self._scores[w]

    def smoothed(self, w):
        if w not in self._smoothed:
            self._smoothed[w] = [R.smooth_ref(p, w) for p in self.probs]
        return self._smoothed[w]

    def sweep(self, w, count, gap):
        key = (w, count, gap)
        if key not in self._sweeps:
            self._sweeps[key] = R.sweep_ref(self.smoothed(w), _thresholds(count).tolist(), gap)
        return self._sweeps[key]


@pytest.fixture(scope="module", params=["in_order", "reversed"])
def synthetic(request):
    return Synthetic(request.param)


def test_the_synthetic_probabilities_hold_the_cases_they_should(synthetic):
    flat = np.concatenate(synthetic.probs)
    assert flat.dtype == np.float32 and flat.size == sum(WINDOWS) == 6479
    for v in (0.0, 0.5, 1.0):
        assert (flat == np.float32(v)).sum() > 100, v
    by_count = dict(zip(synthetic.per_clip, synthetic.probs))
    assert (by_count[ALL_HALF] == 0.5).all() and np.isnan(by_count[ALL_NAN]).all()
    assert np.flatnonzero(np.isnan(by_count[NAN_AT_5])).tolist() == [5]
    assert np.nanmin(flat) == 0.0 and np.nanmax(flat) == 1.0


@pytest.mark.parametrize("w", SMOOTHING)
def test_smoothed_equals_numpys_deque_mean_bit_for_bit(synthetic, w):
    scores = synthetic.scores(w)
    assert scores.prob.dtype == torch.float32 and scores.smoothed.dtype == torch.float64
    assert scores.prob.device.type == scores.smoothed.device.type == scores.window_offsets_dev.device.type == "cuda"
    assert scores.window_offsets.dtype == torch.int64 and scores.window_offsets.device.type == "cpu"
    assert scores.window_offsets.tolist() == np.concatenate([[0], np.cumsum(synthetic.per_clip)]).tolist()
    assert torch.equal(scores.window_offsets_dev.cpu(), scores.window_offsets) and len(scores) == len(WINDOWS)
    assert (scores.hop_samples, scores.window_samples, scores.sample_rate, scores.smoothing_window) == (HOP, WINDOW, SR, w)
    assert torch.equal(scores.prob.cpu().view(torch.int32), torch.from_numpy(np.concatenate(synthetic.probs)).view(torch.int32))
    got, want = scores.smoothed.cpu().numpy(), np.concatenate(synthetic.smoothed(w))
    assert np.isnan(want).sum() == ALL_NAN + min(w, NAN_AT_5 - 5)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


@pytest.mark.parametrize("debounce", DEBOUNCES)
@pytest.mark.parametrize("count", THRESHOLD_COUNTS)
def test_sweep_equals_the_restatement_exactly(synthetic, count, debounce):
    w = 3
    thresholds = _thresholds(count)
    assert thresholds.size == count
    sweep = cda.sweep_thresholds(synthetic.scores(w), thresholds, debounce_seconds=debounce)
    gap = R.gap_ref(debounce, SR, HOP)
    assert sweep.gap == gap == {0.0: 1, 0.25: 1, 0.5: 2, 0.6: 3, 10.0: 40}[debounce]
    ref = synthetic.sweep(w, count, gap)
    n = len(WINDOWS)
    assert sweep.counts.shape == sweep.first_window.shape == (n, count) and sweep.counts.dtype == sweep.first_window.dtype == torch.int32
    assert sweep.peak_conf.shape == sweep.peak_window.shape == (n,) and sweep.peak_conf.dtype == torch.float64
    assert sweep.peak_window.dtype == torch.int32 and sweep.thresholds.tolist() == thresholds.tolist()
    for t in (sweep.counts, sweep.first_window, sweep.peak_conf, sweep.peak_window):
        assert t.device.type == "cuda"
    assert sweep.counts.tolist() == ref["counts"]
    assert sweep.first_window.tolist() == ref["first_window"]
    assert sweep.peak_window.tolist() == ref["peak_window"]
    assert np.array_equal(_bits(sweep.peak_conf.cpu().numpy()), _bits(ref["peak_conf"]))
    by_count = dict(zip(synthetic.per_clip, range(n)))
    assert ref["peak_window"][by_count[0]] == -1 and ref["peak_window"][by_count[ALL_NAN]] == -1
    assert sum(map(sum, ref["counts"])) > 0
    if count > 1:
        half = count - 3                                                   # the threshold 0.5 itself: the all-0.5 recording fires
        assert thresholds[half] == 0.5 and ref["counts"][by_count[ALL_HALF]][half] == -(-ALL_HALF // gap)
        assert ref["counts"][by_count[ALL_HALF]][half + 1] == 0 and all(row[count - 1] == 0 for row in ref["counts"])
    again = cda.sweep_thresholds(synthetic.scores(w), thresholds, debounce_seconds=debounce)
    for a, b in ((again.counts, sweep.counts), (again.first_window, sweep.first_window), (again.peak_window, sweep.peak_window)):
        assert torch.equal(a, b)
    assert torch.equal(again.peak_conf.view(torch.int64), sweep.peak_conf.view(torch.int64))


@pytest.mark.parametrize("w,debounce", [(1, 0.5), (8, 0.0), (32, 0.6)])
def test_sweep_at_other_smoothing_windows(synthetic, w, debounce):
    sweep = cda.sweep_thresholds(synthetic.scores(w), _thresholds(65), debounce_seconds=debounce)
    ref = synthetic.sweep(w, 65, R.gap_ref(debounce, SR, HOP))
    assert sweep.counts.tolist() == ref["counts"] and sweep.first_window.tolist() == ref["first_window"]
    assert sweep.peak_window.tolist() == ref["peak_window"]
    assert np.array_equal(_bits(sweep.peak_conf.cpu().numpy()), _bits(ref["peak_conf"]))


@pytest.mark.parametrize("debounce", [0.0, 0.5, 10.0])
@pytest.mark.parametrize("t", [0.0, 0.5, 0.9, 1.5])
def test_events_equal_the_restatement(synthetic, t, debounce):
    scores, gap = synthetic.scores(3), R.gap_ref(debounce, SR, HOP)
    events = cda.detect_events(scores, threshold=t, debounce_seconds=debounce)
    ref = R.table_ref(synthetic.smoothed(3), t, gap, HOP, WINDOW, SR)
    assert events.clip.dtype == torch.int64 and events.window.dtype == torch.int32
    assert events.time.dtype == events.confidence.dtype == torch.float64
    assert events.counts.dtype == torch.int32 and events.counts.device.type == "cpu"
    for x in (events.clip, events.window, events.time, events.confidence):
        assert x.device.type == "cuda" and x.numel() == len(events)
    assert events.counts.tolist() == ref["counts"] and len(events) == len(ref["clip"])
    assert events.clip.tolist() == ref["clip"] and events.window.tolist() == ref["window"]
    assert np.array_equal(_bits(events.time.cpu().numpy()), _bits(ref["time"]))
    assert np.array_equal(_bits(events.confidence.cpu().numpy()), _bits(ref["confidence"]))
    column = cda.sweep_thresholds(scores, [0.25, t], debounce_seconds=debounce).counts[:, 1]
    assert torch.equal(column.cpu(), events.counts)
    if t == 1.5:
        assert len(events) == 0 and events.counts.tolist() == [0] * len(WINDOWS)
    else:
        assert len(events) > 20
    again = cda.detect_events(scores, threshold=t, debounce_seconds=debounce)
    assert torch.equal(again.window, events.window) and torch.equal(again.confidence.view(torch.int64), events.confidence.view(torch.int64))


def test_empty_and_window_less_banks_give_empty_results():
    pre = cda.AudioPreprocessor(device="cuda", **SHIPPED)
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3").cuda().eval()
    pipe = cda.CoughPipeline(pre, model)
    empty = cda.DeviceClipBank([], [], device="cuda")
    short = cda.DeviceClipBank([torch.ones(100), torch.ones(15999), torch.ones(1)], [0, 1, 0], device="cuda")
    for bank, make in ((empty, None), (short, None), (empty, []), (short, [0, 0, 0])):
        n = len(bank)
        scores = (cda.score_bank(bank, pipe, batch=4) if make is None else
                  cda.WindowScores.from_probabilities(torch.zeros(0), make, HOP, WINDOW, SR, 3))
        assert len(scores) == n and scores.prob.numel() == 0 and scores.smoothed.numel() == 0
        assert scores.prob.device.type == "cuda" and scores.window_offsets.tolist() == [0] * (n + 1)
        sweep = cda.sweep_thresholds(scores, _thresholds(65))
        assert sweep.counts.shape == (n, 65) and int(sweep.counts.abs().sum()) == 0
        assert sweep.first_window.shape == (n, 65) and bool((sweep.first_window == -1).all())
        assert bool(torch.isnan(sweep.peak_conf).all()) and sweep.peak_window.tolist() == [-1] * n
        events = cda.detect_events(scores, 0.0, debounce_seconds=0.0)
        assert len(events) == 0 and events.counts.tolist() == [0] * n and events.time.numel() == 0
        hard = cda.event_windows(bank, scores, events)
        assert len(hard) == 0 and hard.data.numel() == 0
        report = cda.detection_report(bank, scores, sweep)
        assert report["labels"]["non_cough"]["events"] == [0] * 65
        assert report["labels"]["cough"]["recordings"] == (1 if n else 0)
    torch.cuda.synchronize()                                               # no launch error is left behind


def test_detection_report_equals_the_restatement(synthetic):
    scores = synthetic.scores(3)
    bank = cda.DeviceClipBank([torch.zeros(n) for n in synthetic.lengths], synthetic.labels, device="cuda")
    thresholds = _thresholds(65)
    sweep = cda.sweep_thresholds(scores, thresholds, debounce_seconds=0.5)
    report = cda.detection_report(bank, scores, sweep)
    ref = R.report_ref(synthetic.lengths, synthetic.labels, synthetic.smoothed(3), thresholds.tolist(), 2, SR)
    assert report["thresholds"] == thresholds.tolist() and report["gap_windows"] == 2
    assert (report["hop_samples"], report["window_samples"], report["smoothing_window"]) == (HOP, WINDOW, 3)
    assert set(report["labels"]) == {"non_cough", "cough"}
    for name in ("non_cough", "cough"):
        got, want = report["labels"][name], ref[name]
        assert got["recordings"] == want["recordings"] == 7
        assert got["events"] == want["events"] and got["recordings_with_event"] == want["recordings_with_event"]
        assert sum(want["events"]) > 100 and all(isinstance(v, int) for v in got["events"] + got["recordings_with_event"])
        assert got["minutes"] == pytest.approx(want["minutes"], rel=1e-12) and want["minutes"] > 0
        assert got["events_per_minute"] == pytest.approx(want["events_per_minute"], rel=1e-12)
        assert got["share_with_event"] == pytest.approx(want["share_with_event"], rel=1e-12)
    import json
    json.loads(json.dumps(report))                                         # one JSON line, as the CLI prints it


# ------------------------------------------------------------------------------------------------ end to end
LENGTHS = [100, 16000, 16001, 19999, 20000, 24001, 52000]
ORDERS = {"stated": LENGTHS, "odd_first": [16001, 24001, 19999, 100, 16000, 20000, 52000],
          "longest_odd_first": [19999, 16001, 24001, 100, 16000, 20000, 52000]}


def _recordings(lengths, seed=60):
    stream = synth.make_stream(seed, 12.0)
    clips, pos = [], 0
    for n in lengths:
        clips.append(np.ascontiguousarray(stream[pos:pos + n]) * np.float32(0.3 + 0.1 * (len(clips) % 5)))
        pos += n
    assert pos <= stream.size
    return clips


def _host_windows(clips, window, hop):
    rows = [x[k * hop:k * hop + window] for x in clips for k in range(R.windows_per_clip(len(x), window, hop))]
    return torch.from_numpy(np.stack(rows))


@pytest.fixture(scope="module")
def residual_pipe(resnet_golden):
    sd, _ = resnet_golden                                                  # a head at a trained detector's scale
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    model.load_state_dict(sd)
    return cda.CoughPipeline(cda.AudioPreprocessor(device="cuda", **SHIPPED), model.cuda().eval())


def test_the_orders_put_recordings_on_every_16_byte_phase():
    """The stated order alone starts its recordings on phases 0 and 1 only (its odd lengths are 1, 3 and 1 mod 4); the
    two other orders of the same lengths add phases 2 and 3.  The hop is a multiple of 4 samples, so a recording's
    windows share its phase."""
    phases = {name: {int(o) % 4 for o in np.cumsum([0] + order[:-1])} for name, order in ORDERS.items()}
    assert phases == {"stated": {0, 1}, "odd_first": {0, 1, 2}, "longest_odd_first": {0, 1, 3}}
    assert HOP % 4 == 0 and sorted(ORDERS["odd_first"]) == sorted(ORDERS["longest_odd_first"]) == sorted(LENGTHS)


@pytest.mark.parametrize("order", list(ORDERS))
def test_score_bank_equals_the_pipeline_on_host_sliced_windows(residual_pipe, order):
    lengths = ORDERS[order]
    clips = _recordings(lengths)
    bank = cda.DeviceClipBank(clips, [k % 2 for k in range(len(clips))], device="cuda")
    scores = cda.score_bank(bank, residual_pipe, batch=4)
    per_clip = [R.windows_per_clip(n, WINDOW, HOP) for n in lengths]
    assert sorted(per_clip) == [0, 1, 1, 1, 2, 3, 10] and sum(per_clip) == 18 and 18 % 4 != 0
    if order == "stated":
        assert per_clip == [0, 1, 1, 1, 2, 3, 10]
    assert scores.window_offsets.tolist() == np.concatenate([[0], np.cumsum(per_clip)]).tolist()
    assert (scores.hop_samples, scores.window_samples, scores.sample_rate, scores.smoothing_window) == (HOP, WINDOW, SR, 3)
    want = residual_pipe.predict(_host_windows(clips, WINDOW, HOP).cuda(), normalize=True)[1][:, 1]
    assert scores.prob.dtype == torch.float32 and torch.equal(scores.prob, want)
    assert float(want.max() - want.min()) > 1e-3                           # the windows do not all score alike
    smoothed = np.concatenate([R.smooth_ref(p, 3) for p in np.split(want.cpu().numpy(), np.cumsum(per_clip)[:-1])])
    assert np.array_equal(_bits(scores.smoothed.cpu().numpy()), _bits(smoothed))
    for batch in (1, 18, 4096):                                            # the batch size changes nothing
        assert torch.equal(cda.score_bank(bank, residual_pipe, batch=batch).prob, want)
    raw = cda.score_bank(bank, residual_pipe, batch=5, normalize=False)
    assert torch.equal(raw.prob, residual_pipe.predict(_host_windows(clips, WINDOW, HOP).cuda(), normalize=False)[1][:, 1])


def test_score_bank_at_half_second_windows(resnet_golden):
    sd, _ = resnet_golden
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    model.load_state_dict(sd)
    pre = cda.AudioPreprocessor(device="cuda", segment_duration=0.5, **SHIPPED)
    pipe = cda.CoughPipeline(pre, model.cuda().eval())
    clips = _recordings(LENGTHS)
    bank = cda.DeviceClipBank(clips, [0] * len(clips), device="cuda")
    scores = cda.score_bank(bank, pipe, hop_duration=0.1, batch=4, smoothing_window=8)
    assert (scores.window_samples, scores.hop_samples) == (8000, 1600)
    per_clip = [R.windows_per_clip(n, 8000, 1600) for n in LENGTHS]
    assert per_clip == [0, 6, 6, 8, 8, 11, 28] and scores.window_offsets.tolist() == np.concatenate([[0], np.cumsum(per_clip)]).tolist()
    want = pipe.predict(_host_windows(clips, 8000, 1600).cuda(), normalize=True)[1][:, 1]
    assert torch.equal(scores.prob, want)
    smoothed = np.concatenate([R.smooth_ref(p, 8) for p in np.split(want.cpu().numpy(), np.cumsum(per_clip)[:-1])])
    assert np.array_equal(_bits(scores.smoothed.cpu().numpy()), _bits(smoothed))
    events = cda.detect_events(scores, threshold=float(np.median(smoothed)), debounce_seconds=0.3)
    ref = R.table_ref(np.split(smoothed, np.cumsum(per_clip)[:-1]), float(np.median(smoothed)), R.gap_ref(0.3, SR, 1600), 1600, 8000, SR)
    assert events.window.tolist() == ref["window"] and events.clip.tolist() == ref["clip"] and len(events) > 0
    assert np.array_equal(_bits(events.time.cpu().numpy()), _bits(ref["time"]))


def test_score_bank_with_the_small_net_through_the_unfused_path(cnn_golden):
    sd, _ = cnn_golden["small"]
    model = cda.create_model("small", n_mels=90, num_classes=2, in_channels=1)
    model.load_state_dict(sd)
    pipe = cda.CoughPipeline(cda.AudioPreprocessor(device="cuda", **SHIPPED), model.cuda().eval())
    assert not isinstance(model, cda.CoughDetectorResidual)                # featurise, then the conv stack: two steps
    clips = _recordings(LENGTHS)
    bank = cda.DeviceClipBank(clips, [0] * len(clips), device="cuda")
    scores = cda.score_bank(bank, pipe, batch=4)
    want = pipe.predict(_host_windows(clips, WINDOW, HOP).cuda(), normalize=True)[1][:, 1]
    assert scores.prob.numel() == 18 and torch.equal(scores.prob, want)


# ------------------------------------------------------------------------------------------------ the live engine
def test_offline_events_are_the_live_engines_detections(resnet_golden, residual_pipe):
    from cough_detector_amd.streaming import MultiStreamDetector
    clips = _recordings(LENGTHS)
    bank = cda.DeviceClipBank(clips, [0] * len(clips), device="cuda")
    scores = cda.score_bank(bank, residual_pipe, batch=4)
    lo = int(scores.window_offsets[-2])
    s = scores.smoothed[lo:].cpu().numpy()
    assert s.size == 10
    distinct = np.unique(s)                                                # sorted
    assert distinct.size >= 2
    below = max(0, min(distinct.size // 2 - 1, distinct.size - 2))         # the pair around the median
    threshold = float((distinct[below] + distinct[below + 1]) / 2)
    assert distinct[below + 1] - distinct[below] > 1e-6                    # a last-bit difference cannot flip a decision
    assert (s >= threshold).any() and (s < threshold).any()
    events = cda.detect_events(scores, threshold=threshold, debounce_seconds=0.5)
    mine = (events.clip == len(clips) - 1).cpu().numpy()
    windows = events.window.cpu().numpy()[mine].tolist()
    times = events.time.cpu().numpy()[mine].tolist()
    confs = events.confidence.cpu().numpy()[mine].tolist()
    assert windows == R.events_ref(s, threshold, 2) and 0 < len(windows) < 10

    sd, _ = resnet_golden
    model = cda.create_model("residual", n_mels=90, num_classes=2, in_channels=1, compute_dtype="bf16x3")
    model.load_state_dict(sd)
    det = None
    det = MultiStreamDetector(model, n_streams=1, confidence_threshold=threshold, smoothing_window=3, debounce_seconds=0.5,
                              use_graphs=False, clock=lambda: 1000.0 + float(det.written[0]) / SR)
    x, live = clips[-1], []
    live += det.push(x[None, :WINDOW])
    for pos in range(WINDOW, x.size, HOP):
        live += det.push(x[None, pos:pos + HOP])
        assert det.windows_seen == 1 + (pos - WINDOW) // HOP + 1           # exactly one window per push
    assert det.windows_seen == 10
    assert [d[0] for d in live] == [0] * len(live)
    live_windows = [int(round(((d[1] - 1000.0) * SR - WINDOW) / HOP)) for d in live]
    assert live_windows == windows
    assert [d[1] - 1000.0 for d in live] == times                          # multiples of 0.25 s: exact
    assert np.abs(np.array([d[2] for d in live]) - np.array(confs)).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ event_windows
def test_event_windows_hold_the_source_samples(residual_pipe):
    clips = _recordings(LENGTHS)
    labels = [0, 1, 0, 1, 0, 1, 0]
    bank = cda.DeviceClipBank(clips, labels, device="cuda")
    scores = cda.score_bank(bank, residual_pipe, batch=4)
    for threshold, debounce in ((0.0, 0.0), (float(scores.smoothed.median()), 0.5)):
        events = cda.detect_events(scores, threshold=threshold, debounce_seconds=debounce)
        hard = cda.event_windows(bank, scores, events)
        e = len(events)
        assert e == (18 if threshold == 0.0 else e) and e > 0
        assert isinstance(hard, cda.DeviceClipBank) and len(hard) == e and hard.device == bank.device
        assert hard.lengths.tolist() == [WINDOW] * e and hard.offsets.tolist() == [j * WINDOW for j in range(e)]
        src, at = events.clip.tolist(), events.window.tolist()
        for j in range(e):
            want = torch.from_numpy(clips[src[j]][at[j] * HOP:at[j] * HOP + WINDOW])
            assert torch.equal(hard.clip(j).cpu()[0].view(torch.int32), want.view(torch.int32)), j
        assert hard.labels.tolist() == [labels[c] for c in src] and torch.equal(hard.labels_dev.cpu(), hard.labels)
    assert set(hard.labels.tolist()) <= {0, 1}
    negatives = hard.subset([j for j, v in enumerate(hard.labels.tolist()) if v == 0])
    batches = list(cda.DeviceDataLoader(hard, residual_pipe.pre, batch_size=4, is_training=False))
    assert len(batches) == (len(hard) + 3) // 4 and batches[0][0].shape[1:] == (1, 90, 101)
    assert torch.equal(torch.cat([t for _, t in batches]).cpu(), hard.labels)
    assert len(negatives) == hard.labels.tolist().count(0)
