"""Whole recordings scored on the MI355X: how often the detector fires, on which recordings, at which threshold.

The reference's plan asks this once a model is trained (IMPROVEMENT_PLAN.md, Phase 3: detections per minute on silence
and on speech, the share of cough recordings caught, the ``--threshold`` to ship), and asks it of RECORDINGS, through the
engine's smoothing and debounce.  The engine (``CoughDetectorInference`` / ``MultiStreamDetector``) answers for one
window per stream per tick, with a Python decision per window and one threshold per pass.  Here a ``DeviceClipBank`` of
recordings is scored in one pass: windowing, featurise and classify are the existing kernels (``cough_gather_rows``, the
pipeline); the smoothing, the debounced decision at many thresholds at once and the event list are the three kernels of
``libcough_amd_score.so`` (``include/cough_amd_score.h``).

Specification, after the reference's ``RealtimePreprocessor.add_audio`` and ``process_audio_chunk``.  Recording ``c`` has
``n_c`` samples; ``window = pre.segment_samples``, ``sr = pre.sample_rate``, ``hop = int(sr * hop_duration) >= 1``,
``smoothing_window = W`` (1..32), ``debounce_seconds >= 0``, float64 thresholds.

1. Windows: ``K_c = 0`` if ``n_c < window`` else ``1 + (n_c - window) // hop``; window ``k`` is samples ``[k*hop, k*hop +
   window)``.  A recording shorter than a window has none, as in the reference.
2. Probability: ``p[k]`` is the float32 cough probability of the pipeline for that window,
   ``CoughPipeline.predict(rows, normalize)[1][:, 1]`` (``normalize=True``: per window, as ``add_audio``).
3. Smoothing: ``s[k] = float(np.mean(deque(p[max(0, k-W+1) .. k])))`` in float64; history never crosses recordings.  The
   device adds in numpy's order (left to right under 8 values; from 8 on eight accumulators over whole blocks of 8,
   ``((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))``, then the rest in order) and divides by the count: the same bits.
4. Debounce gap: ``G`` is the smallest integer ``g >= 1`` with ``g * hop >= debounce_seconds * sr`` (float64).
5. Decision: at threshold ``t`` window ``k`` fires iff ``s[k] >= t`` and no earlier window of the recording fired or ``k -
   j >= G`` for the last one ``j`` that did.  A NaN in the history makes ``s`` NaN, and a NaN never fires (the engine stays
   silent while a NaN sits in its history).  The engine also drops the later windows of the CHUNK a detection came in;
   that depends on how the audio was chunked, has no meaning offline and is not reproduced.
6. Event time: ``(k*hop + window) / sr`` seconds, the moment the window completes in a live feed.
7. Peak: ``peak_conf[c]`` is the largest non-NaN ``s[k]``, ``peak_window[c]`` its first index; NaN and -1 for a recording
   without a window or with NaN windows only.

The host reads nothing back while scoring or sweeping; ``detect_events`` reads the per-recording counts (they size its
table) and ``detection_report`` its sums.

CLI: ``python -m cough_detector_amd.score CHECKPOINT DATA_DIR [--thresholds 0.3,0.5,0.7 | --sweep 101] [--hop 0.25]
[--smoothing 3] [--debounce 0.5]``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._native import cuda_device
from .data import CLASSES, DeviceClipBank, _offsets, _owner, _ragged, _stream, _upload


@dataclass
class WindowScores:
    """The windows of a bank of recordings, recording after recording and in time order: ``prob`` (float32 ``[N]``) and
    ``smoothed`` (float64 ``[N]``) on the device; recording ``c`` owns ``window_offsets[c] : window_offsets[c + 1]`` (host
    int64 ``[n + 1]``, ``window_offsets_dev`` its device copy)."""
    prob: torch.Tensor
    smoothed: torch.Tensor
    window_offsets: torch.Tensor
    window_offsets_dev: torch.Tensor
    hop_samples: int
    window_samples: int
    sample_rate: int
    smoothing_window: int

    def __len__(self) -> int:
        return int(self.window_offsets.numel()) - 1

    @property
    def device(self) -> torch.device:
        return self.prob.device

    @property
    def windows_per_clip(self) -> np.ndarray:
        return np.diff(self.window_offsets.numpy())

    @classmethod
    def from_probabilities(cls, prob, windows_per_clip: Sequence[int], hop_samples: int, window_samples: int,
                           sample_rate: int, smoothing_window: int, device=None) -> "WindowScores":
        """Scores from per-window cough probabilities the caller already has (``prob``: ``sum(windows_per_clip)`` values,
        recording after recording): they are moved to the device and smoothed there."""
        w = _check_smoothing("WindowScores.from_probabilities", smoothing_window)
        for name, v, low in (("hop_samples", hop_samples, 1), ("window_samples", window_samples, 1),
                             ("sample_rate", sample_rate, 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
                raise ValueError(f"WindowScores.from_probabilities: {name}={v!r} must be a positive integer")
        per_clip = np.asarray(windows_per_clip, dtype=np.int64).reshape(-1)
        if (per_clip < 0).any():
            raise ValueError("WindowScores.from_probabilities: windows_per_clip must not be negative")
        p = torch.as_tensor(prob)
        if p.dim() != 1 or p.numel() != int(per_clip.sum()):
            raise ValueError(f"WindowScores.from_probabilities: {tuple(p.shape)} probabilities for {int(per_clip.sum())} windows")
        dev = torch.device(device) if device is not None else (p.device if p.is_cuda else cuda_device())
        _check_device("WindowScores.from_probabilities", dev)
        offsets = _offsets(per_clip)
        offs_dev, _ = _upload(dev, offsets, np.zeros(0, np.int32))
        p = p.to(device=dev, dtype=torch.float32).contiguous()
        return cls(p, _smooth(p, offs_dev, len(per_clip), w), torch.from_numpy(offsets), offs_dev, int(hop_samples),
                   int(window_samples), int(sample_rate), w)


@dataclass
class ThresholdSweep:
    """``counts`` and ``first_window`` (int32 ``(n, T)``: the windows of recording ``c`` that fire at ``thresholds[t]``, and
    the first of them or -1), ``peak_conf`` (float64 ``(n,)``) and ``peak_window`` (int32 ``(n,)``), all on the device;
    ``thresholds`` (host float64 ``(T,)``); ``gap``: the debounce in windows."""
    thresholds: torch.Tensor
    counts: torch.Tensor
    first_window: torch.Tensor
    peak_conf: torch.Tensor
    peak_window: torch.Tensor
    gap: int


@dataclass
class EventTable:
    """The windows that fired at one threshold, by recording and then time: ``clip`` (int64 index into the bank),
    ``window`` (int32, within the recording), ``time`` (float64 seconds from the recording's start to the end of the
    window) and ``confidence`` (float64, the smoothed probability), on the device; ``counts`` (host int32) holds the
    events of every recording."""
    clip: torch.Tensor
    window: torch.Tensor
    time: torch.Tensor
    confidence: torch.Tensor
    counts: torch.Tensor

    def __len__(self) -> int:
        return int(self.clip.numel())


# ------------------------------------------------------------------------------------------------ parameter checks
def _check_smoothing(what: str, w) -> int:
    if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or not 1 <= w <= _lib.MAX_SMOOTHING:
        raise ValueError(f"{what}: smoothing_window={w!r} must be an integer in 1..{_lib.MAX_SMOOTHING}")
    return int(w)


def _check_device(what: str, dev: torch.device) -> torch.device:
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: the data lives on {dev}; the kernels need it on the GPU (there is no CPU fallback)")
    return dev


def _number(what: str, name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"{what}: {name}={v!r} must be a finite number")
    return float(v)


def hop_samples(what: str, sample_rate: int, hop_duration) -> int:
    hop = int(sample_rate * _number(what, "hop_duration", hop_duration))
    if hop < 1:
        raise ValueError(f"{what}: hop_duration={hop_duration} gives a hop of {hop} samples; it must be at least one sample")
    if hop > 2**31 - 1:
        raise ValueError(f"{what}: hop_duration={hop_duration} is {hop} samples")
    return hop


def debounce_gap(debounce_seconds, sample_rate: int, hop: int, what: str = "debounce_gap") -> int:
    """The smallest integer ``g >= 1`` with ``g * hop >= debounce_seconds * sample_rate``: the windows between two
    detections of one recording."""
    d = _number(what, "debounce_seconds", debounce_seconds)
    if d < 0:
        raise ValueError(f"{what}: debounce_seconds={debounce_seconds} must not be negative")
    need = d * sample_rate
    g = max(1, math.ceil(need / hop))
    while g > 1 and (g - 1) * hop >= need:              # the quotient's rounding may have carried it one too far ...
        g -= 1
    while g * hop < need:                               # ... or left it one short
        g += 1
    if g > 2**31 - 1:
        raise ValueError(f"{what}: debounce_seconds={debounce_seconds} is {g} windows")
    return g


def _check_thresholds(what: str, thresholds) -> np.ndarray:
    try:
        t = np.array(thresholds, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: thresholds={thresholds!r} must be numbers") from None
    if t.size < 1 or t.size > _lib.MAX_THRESHOLDS:
        raise ValueError(f"{what}: {t.size} thresholds; 1..{_lib.MAX_THRESHOLDS} are accepted")
    if not np.isfinite(t).all():
        raise ValueError(f"{what}: thresholds must be finite")
    return t


def windows_per_clip(lengths, window: int, hop: int) -> np.ndarray:
    """Windows per recording (int64) for int recording ``lengths``."""
    n = np.asarray(lengths, dtype=np.int64)
    return np.where(n < window, 0, 1 + (n - window) // hop).astype(np.int64)


# ------------------------------------------------------------------------------------------------ scoring
def _smooth(prob: torch.Tensor, offs_dev: torch.Tensor, n_clips: int, w: int) -> torch.Tensor:
    smoothed = torch.empty(prob.numel(), dtype=torch.float64, device=prob.device)
    if prob.numel() == 0:                                                 # nothing to launch (and no pointer to hand over)
        return smoothed
    _lib.check_score(_lib.load_score().cough_smooth_windows(prob.data_ptr(), offs_dev.data_ptr(), n_clips, prob.numel(), w,
                                                            smoothed.data_ptr(), _stream(prob.device)),
                     "cough_smooth_windows")
    return smoothed


def score_bank(bank: DeviceClipBank, pipeline, hop_duration: float = 0.25, smoothing_window: int = 3, batch: int = 4096,
               normalize: bool = True) -> WindowScores:
    """Every window of every recording of ``bank`` through ``pipeline`` (a ``CoughPipeline`` of any of the three nets),
    ``batch`` windows per pass whatever recordings they belong to, then smoothed.  Stream-ordered: nothing here waits
    for the device."""
    what = "score_bank"
    w = _check_smoothing(what, smoothing_window)
    pre = pipeline.pre
    window, sr = int(pre.segment_samples), int(pre.sample_rate)
    hop = hop_samples(what, sr, hop_duration)
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"{what}: batch={batch!r} must be a positive integer")
    dev = _check_device(what, bank.device)
    offsets, clip, rank = _ragged(windows_per_clip(bank.lengths.numpy(), window, hop))
    n = int(offsets[-1])
    rows = bank.offsets.numpy()[clip] + rank * hop
    i64, row_lens = _upload(dev, np.concatenate([offsets, rows]), np.full(n, window, dtype=np.int32))
    offs_dev, rows_dev = i64[:len(bank) + 1], i64[len(bank) + 1:]
    prob = torch.empty(n, dtype=torch.float32, device=dev)
    if n:
        lib, buf = _lib.load_data(), torch.empty((min(int(batch), n), window), dtype=torch.float32, device=dev)
        for lo in range(0, n, int(batch)):
            b = min(int(batch), n - lo)
            _lib.check_data(lib.cough_gather_rows(bank.data.data_ptr(), rows_dev[lo:].data_ptr(), row_lens[lo:].data_ptr(), b,
                                                  buf.data_ptr(), window, window, _stream(dev)), "cough_gather_rows")
            prob[lo:lo + b] = pipeline.predict(buf[:b], normalize=normalize)[1][:, 1]
    return WindowScores(prob, _smooth(prob, offs_dev, len(bank), w), torch.from_numpy(offsets), offs_dev, hop, window, sr, w)


# ------------------------------------------------------------------------------------------------ decisions
def _sweep(scores: WindowScores, t: np.ndarray, gap: int, peaks: bool):
    dev, n, nt = scores.device, len(scores), int(t.size)
    i32 = dict(dtype=torch.int32, device=dev)
    if scores.smoothed.numel() == 0:                                      # no window anywhere: nothing to launch
        return (torch.zeros((n, nt), **i32), torch.full((n, nt), -1, **i32),
                torch.full((n,), math.nan, dtype=torch.float64, device=dev) if peaks else None,
                torch.full((n,), -1, **i32) if peaks else None)
    counts, first = torch.empty((n, nt), **i32), torch.empty((n, nt), **i32)
    peak_conf = torch.empty((n,), dtype=torch.float64, device=dev) if peaks else None
    peak_window = torch.empty((n,), **i32) if peaks else None
    thr = torch.from_numpy(t).to(dev, non_blocking=True)
    _lib.check_score(_lib.load_score().cough_sweep_thresholds(
        scores.smoothed.data_ptr(), scores.window_offsets_dev.data_ptr(), n, scores.smoothed.numel(), thr.data_ptr(), nt, gap,
        counts.data_ptr(), first.data_ptr(), peak_conf.data_ptr() if peaks else None,
        peak_window.data_ptr() if peaks else None, _stream(dev)), "cough_sweep_thresholds")
    return counts, first, peak_conf, peak_window


def sweep_thresholds(scores: WindowScores, thresholds, debounce_seconds: float = 0.5) -> ThresholdSweep:
    """How many windows of every recording fire at every one of ``thresholds`` (1..1024 finite values), and each
    recording's peak.  One launch; nothing is read back."""
    what = "sweep_thresholds"
    t = _check_thresholds(what, thresholds)
    gap = debounce_gap(debounce_seconds, scores.sample_rate, scores.hop_samples, what)
    _check_device(what, scores.device)
    counts, first, peak_conf, peak_window = _sweep(scores, t, gap, True)
    return ThresholdSweep(torch.from_numpy(t), counts, first, peak_conf, peak_window, gap)


def detect_events(scores: WindowScores, threshold: float = 0.5, debounce_seconds: float = 0.5) -> EventTable:
    """The windows that fire at ``threshold``.  One host read (the per-recording counts of a one-threshold sweep, which
    size the table); one launch then fills it."""
    what = "detect_events"
    t = _check_thresholds(what, [_number(what, "threshold", threshold)])
    gap = debounce_gap(debounce_seconds, scores.sample_rate, scores.hop_samples, what)
    dev, n = _check_device(what, scores.device), len(scores)
    counts = _sweep(scores, t, gap, False)[0].view(-1).cpu()             # the one host read
    per_clip = counts.numpy().astype(np.int64)
    offsets, clip = _offsets(per_clip), _owner(per_clip)
    n_events = int(offsets[-1])
    i64, _ = _upload(dev, np.concatenate([offsets, clip]), np.zeros(0, np.int32))
    window = torch.empty(n_events, dtype=torch.int32, device=dev)
    conf = torch.empty(n_events, dtype=torch.float64, device=dev)
    if n_events:
        _lib.check_score(_lib.load_score().cough_list_events(
            scores.smoothed.data_ptr(), scores.window_offsets_dev.data_ptr(), n, scores.smoothed.numel(), float(t[0]), gap,
            i64[:n + 1].data_ptr(), n_events, window.data_ptr(), conf.data_ptr(), _stream(dev)), "cough_list_events")
    time = (window.to(torch.float64) * scores.hop_samples + scores.window_samples) / scores.sample_rate
    return EventTable(i64[n + 1:], window, time, conf, counts)


def _check_bank(what: str, bank: DeviceClipBank, scores: WindowScores) -> None:
    if len(bank) != len(scores):
        raise ValueError(f"{what}: the bank holds {len(bank)} recordings, the scores {len(scores)}")


def event_windows(bank: DeviceClipBank, scores: WindowScores, events: EventTable) -> DeviceClipBank:
    """The windows of ``events`` as a bank of clips of ``scores.window_samples`` each, in table order, every clip with its
    recording's label: the windows that fired on ``non_cough`` recordings are the hard negatives to retrain on
    (``subset`` by label, then ``DeviceDataLoader``)."""
    what = "event_windows"
    _check_bank(what, bank, scores)
    if len(events.counts) != len(bank):
        raise ValueError(f"{what}: the events count {len(events.counts)} recordings, the bank holds {len(bank)}")
    _check_device(what, bank.device)
    starts = (events.window.to(torch.int64) * scores.hop_samples).to(torch.int32)
    return bank.cut(_owner(events.counts), starts, np.full(len(events), scores.window_samples, dtype=np.int64))


def detection_report(bank: DeviceClipBank, scores: WindowScores, sweep: ThresholdSweep) -> dict:
    """The plan's success table: per label the ``recordings``, their ``minutes`` (``sum(n_c) / sr / 60``) and, per
    threshold, the ``events``, ``events_per_minute``, ``recordings_with_event`` and their ``share`` (``None`` where a
    label has no recording).  The integer sums are formed on the device and read once."""
    what = "detection_report"
    _check_bank(what, bank, scores)
    if sweep.counts.shape[0] != len(bank):
        raise ValueError(f"{what}: the sweep counts {sweep.counts.shape[0]} recordings, the bank holds {len(bank)}")
    _check_device(what, scores.device)
    counts = sweep.counts.to(torch.int64)
    sums = []
    for label in range(len(CLASSES)):
        mine = (bank.labels_dev == label).unsqueeze(1)
        sums += [(counts * mine).sum(0), ((counts > 0) & mine).sum(0)]
    sums = torch.stack(sums).cpu().numpy()                                # the one host read
    lengths, labels = bank.lengths.numpy().astype(np.int64), bank.labels.numpy()
    report = {"thresholds": sweep.thresholds.tolist(), "gap_windows": int(sweep.gap), "hop_samples": scores.hop_samples,
              "window_samples": scores.window_samples, "smoothing_window": scores.smoothing_window, "labels": {}}
    for label, name in enumerate(CLASSES):
        recordings = int((labels == label).sum())
        minutes = float(int(lengths[labels == label].sum())) / scores.sample_rate / 60.0
        events, hit = sums[2 * label].tolist(), sums[2 * label + 1].tolist()
        report["labels"][name] = {
            "recordings": recordings, "minutes": minutes, "events": events,
            "events_per_minute": [v / minutes if minutes > 0 else None for v in events],
            "recordings_with_event": hit,
            "share_with_event": [v / recordings if recordings else None for v in hit]}
    return report


# ------------------------------------------------------------------------------------------------ CLI
def main(argv: Optional[Sequence[str]] = None) -> dict:
    import argparse
    import json
    from .inference import CoughDetectorInference
    parser = argparse.ArgumentParser(prog="python -m cough_detector_amd.score",
                                     description="Score the recordings of DATA_DIR/non_cough and DATA_DIR/cough (MI355X path)")
    parser.add_argument("checkpoint", help="trained model checkpoint")
    parser.add_argument("data_dir", help="directory with non_cough/ and cough/ WAVE files")
    group = parser.add_mutually_exclusive_group()
    group.add_argument("--thresholds", type=str, default="0.3,0.5,0.7", help="comma-separated confidence thresholds")
    group.add_argument("--sweep", type=int, default=None, help="this many thresholds evenly spaced over 0..1")
    parser.add_argument("--hop", type=float, default=0.25, help="seconds between windows")
    parser.add_argument("--smoothing", type=int, default=3, help="windows in the smoothing mean")
    parser.add_argument("--debounce", type=float, default=0.5, help="minimum seconds between detections")
    args = parser.parse_args(argv)
    if args.sweep is not None:
        if args.sweep < 2:
            parser.error("--sweep needs at least 2 thresholds")
        thresholds = np.linspace(0.0, 1.0, args.sweep)
    else:
        thresholds = [float(v) for v in args.thresholds.split(",")]
    engine = CoughDetectorInference(args.checkpoint, verbose=False)
    bank = DeviceClipBank.from_directory(args.data_dir, engine.preprocessor)
    scores = score_bank(bank, engine._pipeline, hop_duration=args.hop, smoothing_window=args.smoothing)
    sweep = sweep_thresholds(scores, thresholds, debounce_seconds=args.debounce)
    report = detection_report(bank, scores, sweep)
    print(json.dumps(report))
    # the non-cough recordings the detector is surest about: the ones to listen to first (mislabelled files)
    peak, at = sweep.peak_conf.cpu().numpy(), sweep.peak_window.cpu().numpy()
    negatives = [k for k in np.flatnonzero(bank.labels.numpy() == 0) if not math.isnan(peak[k])]
    suspects = sorted(negatives, key=lambda k: -peak[k])[:10]
    print("non_cough recordings with the largest smoothed cough confidence (index in directory order, confidence, seconds):")
    for k in suspects:
        seconds = (int(at[k]) * scores.hop_samples + scores.window_samples) / scores.sample_rate
        print(f"  {int(k):6d}  {peak[k]:.4f}  {seconds:8.2f}")
    return {"report": report, "suspects": [int(k) for k in suspects]}


if __name__ == "__main__":
    main()
