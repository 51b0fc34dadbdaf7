"""Soundscapes with known cough times, composed on the MI355X, and the detector scored against them event by event.

The reference's plan ends in event-level criteria (IMPROVEMENT_PLAN.md: "cough 10 times, count detections", "< 1
detection/minute on speech", "detection latency < 2 s") and has no recordings with annotated cough onsets to measure them
on.  Here clean cough segments (``extract_segments``) are placed at chosen times into minutes of background
(``slice_bank``'s negatives, speech, room noise, silence) at a chosen SNR, the truth is remembered, and the debounced
decision of ``score.py`` is matched to that truth at many thresholds at once.  The kernels live in
``libcough_amd_scenes.so`` (``include/cough_amd_scenes.h``); they decide whether a window fires with the very functions
of ``cough_sweep_thresholds`` (``csrc/score_walk.h``).

Specification.  ``sr`` samples per second; scene ``s`` has ``L_s`` samples.

1. Background: clip ``b_s`` of the background bank, ``n_b`` samples, read cyclically from ``bg_start[s]``: sample ``i`` of
   the scene reads ``B[(bg_start[s] + i) mod n_b]``, the way the reference's ``add_noise`` repeats a short noise sample.
2. Events: event ``e`` of scene ``s`` is clip ``c_e`` of the event bank, ``n_e`` samples, at ``onset[e]``; the events of
   a scene are sorted by onset, do not overlap and lie inside ``[0, L_s)``.
3. Powers (float64): ``P_bg[s]`` is the mean of ``double(x)^2`` over the ``L_s`` background samples the scene reads,
   ``P_ev[c]`` over the whole event clip -- whole-scene background power, ``add_noise``'s convention.
4. Gain: ``gain[e] = float32(sqrt(snr_linear * double(bg_gain[s])^2 * P_bg[s] / P_ev[c_e]))`` with ``snr_linear = 10 **
   (snr_db / 10)`` from the host; 1.0 when either power is 0 or not finite (a cough over digital silence stays audible).
5. Mix (float32): ``out[i] = fmaf(gain[e], E[i - onset[e]], bg_gain[s] * B[...])`` where event ``e`` covers ``i``, else
   ``bg_gain[s] * B[...]``.
6. Truth: event ``e`` occupies samples ``[onset, offset) = [onset[e], onset[e] + n_e)`` of its scene.
7. Window ranges (``truth_window_ranges``): with ``m = max(1, ceil(min_overlap_seconds * sr))`` and ``m_j = min(m,
   offset_j - onset_j)``, window ``k`` (samples ``[k*hop, k*hop + window)``) counts for event ``j`` iff it overlaps it by
   at least ``m_j`` samples: ``k*hop <= offset_j - m_j`` and ``k*hop + window >= onset_j + m_j``; ``k_lo`` / ``k_hi`` are
   the first and last such ``k`` among the recording's windows.  ``k_lo > k_hi``: no window reaches the event (it lies
   behind the last window, or between two windows when ``hop > window - m_j``); it is a miss at every threshold and
   its range stays as it is.  Only where ``k_lo <= k_hi`` is ``k_hi`` then extended by the collar (in windows, rounded
   up; by default the ``smoothing_window - 1`` windows by which the deque mean lags), up to the recording's last
   window.  ``k_lo`` is non-decreasing within a recording, and so is the ``k_hi`` of the events that can be reached.
8. Matching (``match_events``): the windows that fire are those of ``sweep_thresholds`` (same smoothing, same debounce).
   A firing window ``k`` takes ``p``, the first event after the last one hit with ``k_hi[p] >= k``; it is a *hit* of ``p``
   if ``k_lo[p] <= k``, else a *repeat* if an event was hit and ``k <= k_hi[last hit]``, else a *false alarm*.  Latency of
   a hit: ``k*hop + window - onset[p]`` samples, from the cough's onset to the moment the window completes.

Draws (``draw_scene_plan``): one ``numpy.random.Generator(Philox(seed))``; scene by scene, in this order: the background
clip (``integers(0, n_backgrounds)``), ``bg_start`` (``integers(0, n_b)``), the number of events ``m`` (``integers(lo, hi +
1)``), the ``m`` event clips (``integers(0, n_events, size=m)``), their SNRs (``uniform(snr_lo, snr_hi, size=m)``) and ``m``
cuts (``integers(0, slack + 1, size=m)``, sorted) of the slack ``L - sum(n_e) - (m - 1) * gap``: event ``j`` starts
``cuts[j]`` samples after the earliest place the events before it and their gaps allow.  Nothing is ever rejected.

``compose_scenes`` is four launches (two ``cough_span_power``, ``cough_scene_gains``, ``cough_mix_scenes``) and reads
nothing back; ``match_events`` is one launch; ``event_report`` and ``missed_events`` read once each.

CLI: ``python -m cough_detector_amd.scenes CHECKPOINT BACKGROUND_DIR COUGH_DIR [--scenes 64] [--seconds 60] [--events
5,10] [--snr 5,20] [--sweep 101] [--seed 0] [--write DIR]``; the last line printed is the report as JSON.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data import DeviceClipBank, _offsets, _ragged, _stream, _upload
from .score import (WindowScores, _check_bank, _check_device, _check_thresholds, _number, debounce_gap)

TILE = 4096                    # COUGH_SCENES_TILE
CLASS_HIT, CLASS_REPEAT, CLASS_FALSE_ALARM = 0, 1, 2
_I32_MAX = 2**31 - 1


# ------------------------------------------------------------------------------------------------ the plan
def _ints(what: str, name: str, v, n: Optional[int] = None) -> np.ndarray:
    a = np.asarray(v.tolist() if isinstance(v, torch.Tensor) else v)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{what}: {name} must hold integers, got {a.dtype}")
    a = a.astype(np.int64).reshape(-1)
    if n is not None and a.size != n:
        raise ValueError(f"{what}: {name} holds {a.size} values, expected {n}")
    return a


@dataclass
class ScenePlan:
    """What to compose, on the host.  Per scene: ``background`` (clip of the background bank), ``bg_start`` (its first
    sample read), ``bg_gain`` (float32) and ``length`` (samples).  Per event, scene after scene and by onset within a
    scene: ``event_scene``, ``event_clip`` (clip of the event bank), ``onset`` (samples from the scene's start) and
    ``snr_db`` (float64)."""
    background: np.ndarray
    bg_start: np.ndarray
    bg_gain: np.ndarray
    length: np.ndarray
    event_scene: np.ndarray
    event_clip: np.ndarray
    onset: np.ndarray
    snr_db: np.ndarray

    def __len__(self) -> int:
        return int(np.asarray(self.length).size)

    def checked(self, background_lengths, event_lengths, what: str = "ScenePlan") -> "ScenePlan":
        """The plan with its arrays normalised (int64 / float32 / float64), after checking it against the lengths of the
        two banks' clips: indices in range, scenes of 1..2^31 - 1 samples, ``bg_start`` inside its clip, gains and SNRs
        finite, events grouped by ascending scene, sorted by onset, not overlapping and inside their scene."""
        bl, el = _ints(what, "background_lengths", background_lengths), _ints(what, "event_lengths", event_lengths)
        length = _ints(what, "length", self.length)
        n = length.size
        bg, start = _ints(what, "background", self.background, n), _ints(what, "bg_start", self.bg_start, n)
        gain = np.asarray(self.bg_gain, dtype=np.float32).reshape(-1)
        if gain.size != n or not np.isfinite(gain).all():
            raise ValueError(f"{what}: bg_gain must hold {n} finite values")
        if n and (length.min() < 1 or length.max() > _I32_MAX):
            raise ValueError(f"{what}: scene lengths must lie in 1..2^31 - 1 samples")
        if n and (bg.min() < 0 or bg.max() >= bl.size):
            raise ValueError(f"{what}: background indices must lie in 0..{bl.size - 1}")
        if n and ((start < 0) | (start >= bl[bg])).any():
            s = int(np.flatnonzero((start < 0) | (start >= bl[bg]))[0])
            raise ValueError(f"{what}: scene {s}: bg_start={int(start[s])} lies outside its background of {int(bl[bg[s]])} samples")
        scene = _ints(what, "event_scene", self.event_scene)
        m = scene.size
        clip, onset = _ints(what, "event_clip", self.event_clip, m), _ints(what, "onset", self.onset, m)
        snr = np.asarray(self.snr_db, dtype=np.float64).reshape(-1)
        if snr.size != m or not np.isfinite(snr).all():
            raise ValueError(f"{what}: snr_db must hold {m} finite values")
        if m:
            if scene.min() < 0 or scene.max() >= n:
                raise ValueError(f"{what}: event scenes must lie in 0..{n - 1}")
            if clip.min() < 0 or clip.max() >= el.size:
                raise ValueError(f"{what}: event clips must lie in 0..{el.size - 1}")
            if (np.diff(scene) < 0).any():
                raise ValueError(f"{what}: events must be grouped by ascending scene")
            end = onset + el[clip]
            bad = (onset < 0) | (end > length[scene])
            if bad.any():
                e = int(np.flatnonzero(bad)[0])
                raise ValueError(f"{what}: event {e} (samples {int(onset[e])}..{int(end[e])}) does not lie inside scene "
                                 f"{int(scene[e])} of {int(length[scene[e]])} samples")
            same = scene[1:] == scene[:-1]
            if (same & (onset[1:] < onset[:-1])).any():
                raise ValueError(f"{what}: the events of a scene must be sorted by onset")
            if (same & (onset[1:] < end[:-1])).any():
                e = int(np.flatnonzero(same & (onset[1:] < end[:-1]))[0]) + 1
                raise ValueError(f"{what}: event {e} overlaps the event before it in scene {int(scene[e])}")
        return ScenePlan(bg, start, gain, length, scene, clip, onset, snr)


def _pair(what: str, name: str, v, integer: bool) -> Tuple[float, float]:
    try:
        lo, hi = v
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name}={v!r} must be a pair (lo, hi)") from None
    for x in (lo, hi):
        if integer and (isinstance(x, bool) or not isinstance(x, (int, np.integer))):
            raise ValueError(f"{what}: {name}={v!r} must hold integers")
        _number(what, name, x)
    if lo > hi or (integer and lo < 0):
        raise ValueError(f"{what}: {name}={v!r} must satisfy {'0 <= ' if integer else ''}lo <= hi")
    return lo, hi


def _bank_lengths(what: str, name: str, bank) -> np.ndarray:
    if not isinstance(bank, DeviceClipBank):
        raise ValueError(f"{what}: {name} must be a DeviceClipBank, got {type(bank).__name__}")
    return bank.lengths.numpy().astype(np.int64)


def draw_scene_plan(backgrounds: DeviceClipBank, events: DeviceClipBank, n_scenes: int, scene_seconds: float,
                    events_per_scene=(5, 10), snr_range=(5, 20), min_gap_seconds: float = 0.5, bg_gain: float = 1.0,
                    seed: int = 0, sample_rate: int = 16000) -> ScenePlan:
    """A plan of ``n_scenes`` scenes of ``int(scene_seconds * sample_rate)`` samples, drawn in the order the module
    docstring states.  Placement never rejects: a scene whose drawn events and the gaps between them do not fit raises
    ``ValueError`` naming it."""
    what = "draw_scene_plan"
    bl, el = _bank_lengths(what, "backgrounds", backgrounds), _bank_lengths(what, "events", events)
    for name, v in (("n_scenes", n_scenes), ("sample_rate", sample_rate), ("seed", seed)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < (1 if name == "sample_rate" else 0):
            raise ValueError(f"{what}: {name}={v!r} must be a {'positive' if name == 'sample_rate' else 'non-negative'} integer")
    L = int(_number(what, "scene_seconds", scene_seconds) * sample_rate)
    if not 1 <= L <= _I32_MAX:
        raise ValueError(f"{what}: scene_seconds={scene_seconds} is {L} samples; 1..2^31 - 1 are accepted")
    lo, hi = _pair(what, "events_per_scene", events_per_scene, True)
    snr_lo, snr_hi = _pair(what, "snr_range", snr_range, False)
    gap = _number(what, "min_gap_seconds", min_gap_seconds)
    if gap < 0:
        raise ValueError(f"{what}: min_gap_seconds={min_gap_seconds} must not be negative")
    gap = int(math.ceil(gap * sample_rate))
    gain = np.float32(_number(what, "bg_gain", bg_gain))
    if not np.isfinite(gain):
        raise ValueError(f"{what}: bg_gain={bg_gain} is not a finite float32")
    if n_scenes and bl.size == 0:
        raise ValueError(f"{what}: the background bank is empty")
    if n_scenes and hi > 0 and el.size == 0:
        raise ValueError(f"{what}: the event bank is empty")
    rng = np.random.Generator(np.random.Philox(int(seed)))
    background, start, scene, clip, onset, snr = [], [], [], [], [], []
    for s in range(int(n_scenes)):
        b = int(rng.integers(0, bl.size))
        background.append(b)
        start.append(int(rng.integers(0, bl[b])))
        m = int(rng.integers(lo, hi + 1))
        clips = rng.integers(0, max(el.size, 1), size=m)
        snrs = rng.uniform(snr_lo, snr_hi, size=m)
        slack = L - int(el[clips].sum()) - max(m - 1, 0) * gap
        if slack < 0:
            raise ValueError(f"{what}: scene {s}: its {m} events ({int(el[clips].sum())} samples) and the gaps of {gap} "
                             f"samples between them need {-slack} samples more than the scene's {L}")
        cuts = np.sort(rng.integers(0, slack + 1, size=m))
        at = 0                                           # the earliest place the events so far and their gaps allow
        for j in range(m):
            scene.append(s)
            clip.append(int(clips[j]))
            onset.append(at + int(cuts[j]))
            snr.append(float(snrs[j]))
            at += int(el[clips[j]]) + gap
    return ScenePlan(np.array(background, np.int64), np.array(start, np.int64), np.full(int(n_scenes), gain, np.float32),
                     np.full(int(n_scenes), L, np.int64), np.array(scene, np.int64), np.array(clip, np.int64),
                     np.array(onset, np.int64), np.array(snr, np.float64)).checked(bl, el, what)


# ------------------------------------------------------------------------------------------------ the truth
@dataclass
class TruthTable:
    """The known events of a bank of recordings, recording after recording and by onset: ``clip`` (the recording),
    ``onset`` and ``offset`` (samples: the event is ``[onset, offset)``), ``source`` (clip of the event bank, -1 when
    annotated by hand) and ``snr_db`` (NaN when annotated by hand), host arrays; ``gain`` (float32 on the device, the
    gain the mix applied; None when annotated by hand); ``counts`` (host int64): the events of every recording."""
    clip: np.ndarray
    onset: np.ndarray
    offset: np.ndarray
    source: np.ndarray
    snr_db: np.ndarray
    gain: Optional[torch.Tensor]
    counts: np.ndarray

    def __len__(self) -> int:
        return int(self.clip.size)

    @property
    def offsets(self) -> np.ndarray:
        """int64 ``[n + 1]``: recording ``c`` owns the events ``offsets[c] : offsets[c + 1]``."""
        return _offsets(self.counts)

    @classmethod
    def from_intervals(cls, clip, onset, offset, n_clips: Optional[int] = None) -> "TruthTable":
        """Hand-annotated events: ``[onset, offset)`` in samples of recording ``clip``, grouped by ascending recording,
        sorted by onset and not overlapping within one.  ``n_clips``: the recordings of the bank (default: the largest
        ``clip`` + 1)."""
        what = "TruthTable.from_intervals"
        clip = _ints(what, "clip", clip)
        onset, offset = _ints(what, "onset", onset, clip.size), _ints(what, "offset", offset, clip.size)
        n = int(clip.max()) + 1 if clip.size and n_clips is None else int(n_clips or 0)
        if clip.size:
            if clip.min() < 0 or clip.max() >= n:
                raise ValueError(f"{what}: recordings must lie in 0..{n - 1}")
            if (np.diff(clip) < 0).any():
                raise ValueError(f"{what}: events must be grouped by ascending recording")
            if (onset < 0).any() or (offset <= onset).any() or offset.max() > _I32_MAX:
                raise ValueError(f"{what}: every event needs 0 <= onset < offset <= 2^31 - 1")
            same = clip[1:] == clip[:-1]
            if (same & (onset[1:] < onset[:-1])).any():
                raise ValueError(f"{what}: the events of a recording must be sorted by onset")
            if (same & (onset[1:] < offset[:-1])).any():
                e = int(np.flatnonzero(same & (onset[1:] < offset[:-1]))[0]) + 1
                raise ValueError(f"{what}: event {e} overlaps the event before it in recording {int(clip[e])}")
        return cls(clip, onset, offset, np.full(clip.size, -1, np.int64), np.full(clip.size, math.nan),
                   None, np.bincount(clip, minlength=n).astype(np.int64))


# ------------------------------------------------------------------------------------------------ composing
def _spans(bank: DeviceClipBank, clips: np.ndarray, starts: np.ndarray, lengths: np.ndarray) -> torch.Tensor:
    """float64 powers of the spans ``(clip, start, length)`` of ``bank``: one launch."""
    dev, n = bank.device, int(clips.size)
    power = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        i64, i32 = _upload(dev, bank.offsets.numpy()[clips],
                           np.concatenate([bank.lengths.numpy()[clips], starts, lengths]).astype(np.int32))
        _lib.check_scenes(_lib.load_scenes().cough_span_power(
            bank.data.data_ptr(), bank.data.numel(), i64.data_ptr(), i32[:n].data_ptr(), i32[n:2 * n].data_ptr(),
            i32[2 * n:].data_ptr(), n, power.data_ptr(), _stream(dev)), "cough_span_power")
    return power


def span_power(bank: DeviceClipBank, clips, starts, lengths) -> torch.Tensor:
    """The float64 mean power of spans of ``bank`` on the device: span ``r`` reads ``lengths[r]`` samples of clip
    ``clips[r]`` cyclically from ``starts[r]`` on."""
    what = "span_power"
    _bank_lengths(what, "bank", bank)
    clips = _ints(what, "clips", clips)
    starts, lengths = _ints(what, "starts", starts, clips.size), _ints(what, "lengths", lengths, clips.size)
    if clips.size and (clips.min() < 0 or clips.max() >= len(bank)):
        raise ValueError(f"{what}: clips must lie in 0..{len(bank) - 1}")
    if clips.size and (starts.min() < 0 or (starts >= bank.lengths.numpy()[clips]).any()):
        raise ValueError(f"{what}: every start must lie inside its clip")
    if clips.size and (lengths.min() < 0 or lengths.max() > _I32_MAX):
        raise ValueError(f"{what}: span lengths must lie in 0..2^31 - 1")
    _check_device(what, bank.device)
    return _spans(bank, clips, starts, lengths)


def scene_tiles(lengths: np.ndarray) -> np.ndarray:
    """int32 ``[n_tiles, 2]``: ``(scene, first sample)`` of every tile of ``TILE`` samples, scene by scene."""
    _, scene, rank = _ragged((np.asarray(lengths, dtype=np.int64) + TILE - 1) // TILE)
    return np.stack([scene, rank * TILE], axis=1).astype(np.int32)


def compose_scenes(backgrounds: DeviceClipBank, events: DeviceClipBank, plan: ScenePlan) -> Tuple[DeviceClipBank, TruthTable]:
    """The scenes of ``plan`` as a bank (a scene's label is 1 when it holds an event, else 0) and their truth.  Four
    launches, stream-ordered; nothing is read back."""
    what = "compose_scenes"
    bl, el = _bank_lengths(what, "backgrounds", backgrounds), _bank_lengths(what, "events", events)
    if not isinstance(plan, ScenePlan):
        raise ValueError(f"{what}: plan must be a ScenePlan, got {type(plan).__name__}")
    plan = plan.checked(bl, el, what)
    if backgrounds.device != events.device:
        raise ValueError(f"{what}: the banks live on {backgrounds.device} and {events.device}; they must share one device")
    n, m = len(plan), int(plan.event_scene.size)
    tiles = scene_tiles(plan.length)
    if tiles.shape[0] > _I32_MAX:
        raise ValueError(f"{what}: {tiles.shape[0]} tiles do not fit one launch")
    dev = _check_device(what, backgrounds.device)
    counts = np.bincount(plan.event_scene, minlength=n).astype(np.int64)
    out = DeviceClipBank.from_packed(torch.empty(int(plan.length.sum()), dtype=torch.float32, device=dev), plan.length,
                                     counts > 0)
    used, which = np.unique(plan.event_clip, return_inverse=True)         # every event clip's power once
    p_bg = _spans(backgrounds, plan.background, plan.bg_start, plan.length)
    p_ev = _spans(events, used, np.zeros(used.size, np.int64), el[used])
    snr_linear = 10.0 ** (plan.snr_db / 10.0)
    i64, i32 = _upload(dev, np.concatenate([backgrounds.offsets.numpy()[plan.background], out.offsets.numpy(), _offsets(counts),
                                            events.offsets.numpy()[plan.event_clip], snr_linear.view(np.int64)]),
                       np.concatenate([bl[plan.background], plan.bg_start, plan.bg_gain.view(np.int32), plan.length,
                                       el[plan.event_clip], plan.onset, plan.event_scene, which,
                                       tiles.reshape(-1)]).astype(np.int32))
    bg_off, out_off, ev_off, src_off, snr_dev = (i64[:n], i64[n:2 * n], i64[2 * n:3 * n + 1], i64[3 * n + 1:3 * n + 1 + m],
                                                 i64[3 * n + 1 + m:].view(torch.float64))
    bg_len, bg_start, bg_gain, length = (i32[k * n:(k + 1) * n] for k in range(4))
    src_len, onset, ev_scene, ev_power = (i32[4 * n + k * m:4 * n + (k + 1) * m] for k in range(4))
    tiles_dev = i32[4 * n + 4 * m:]
    gain = torch.empty(m, dtype=torch.float32, device=dev)
    lib = _lib.load_scenes()
    if m:
        _lib.check_scenes(lib.cough_scene_gains(p_bg.data_ptr(), bg_gain.data_ptr(), n, p_ev.data_ptr(), int(used.size),
                                                ev_scene.data_ptr(), ev_power.data_ptr(), snr_dev.data_ptr(), m,
                                                gain.data_ptr(), _stream(dev)), "cough_scene_gains")
    if n:
        _lib.check_scenes(lib.cough_mix_scenes(
            backgrounds.data.data_ptr(), backgrounds.data.numel(), bg_off.data_ptr(), bg_len.data_ptr(), bg_start.data_ptr(),
            bg_gain.data_ptr(), length.data_ptr(), out_off.data_ptr(), ev_off.data_ptr(), n,
            events.data.data_ptr() if m else None, events.data.numel() if m else 0, src_off.data_ptr() if m else None,
            src_len.data_ptr() if m else None, onset.data_ptr() if m else None, gain.data_ptr() if m else None, m,
            tiles_dev.data_ptr(), int(tiles.shape[0]), out.data.data_ptr(), out.data.numel(), _stream(dev)),
            "cough_mix_scenes")
    truth = TruthTable(plan.event_scene.copy(), plan.onset.copy(), plan.onset + el[plan.event_clip], plan.event_clip.copy(),
                       plan.snr_db.copy(), gain, counts)
    return out, truth


# ------------------------------------------------------------------------------------------------ matching
def _least_windows(samples: float, hop: int) -> int:
    """The smallest integer ``g >= 0`` with ``g * hop >= samples``."""
    g = max(0, math.ceil(samples / hop))
    while g > 0 and (g - 1) * hop >= samples:
        g -= 1
    while g * hop < samples:
        g += 1
    return g


def truth_window_ranges(truth: TruthTable, scores: WindowScores, min_overlap_seconds: float = 0.1,
                        collar_seconds: Optional[float] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``(k_lo, k_hi)``, int32 per truth event: the closed range of its recording's windows that count as detecting it
    (rule 7 of the module docstring), in closed form on the host.  ``k_lo`` is non-decreasing within a recording, and so is ``k_hi`` over the events with
    ``k_lo <= k_hi``; an event no window reaches keeps ``k_lo > k_hi`` whatever the collar."""
    what = "truth_window_ranges"
    if not isinstance(truth, TruthTable) or not isinstance(scores, WindowScores):
        raise ValueError(f"{what}: expected a TruthTable and WindowScores")
    if truth.counts.size != len(scores):
        raise ValueError(f"{what}: the truth counts {truth.counts.size} recordings, the scores {len(scores)}")
    overlap = _number(what, "min_overlap_seconds", min_overlap_seconds)
    if overlap < 0:
        raise ValueError(f"{what}: min_overlap_seconds={min_overlap_seconds} must not be negative")
    hop, window, sr = scores.hop_samples, scores.window_samples, scores.sample_rate
    m = max(1, math.ceil(overlap * sr))
    if m > window:
        raise ValueError(f"{what}: min_overlap_seconds={min_overlap_seconds} is {m} samples, more than a window of {window}: "
                         "no window could count")
    if collar_seconds is None:
        collar = scores.smoothing_window - 1
    else:
        c = _number(what, "collar_seconds", collar_seconds)
        if c < 0:
            raise ValueError(f"{what}: collar_seconds={collar_seconds} must not be negative")
        collar = _least_windows(c * sr, hop)
    m_j = np.minimum(m, truth.offset - truth.onset)
    last = scores.windows_per_clip.astype(np.int64)[truth.clip] - 1      # the recording's last window, -1 without one
    k_lo = np.maximum(-((window - truth.onset - m_j) // hop), 0)          # ceil((onset + m_j - window) / hop)
    k_hi = np.minimum((truth.offset - m_j) // hop, last)
    k_hi = np.where(k_lo <= k_hi, np.minimum(k_hi + collar, last), k_hi)  # the collar never makes an unreachable event reachable
    return np.minimum(k_lo, _I32_MAX).astype(np.int32), k_hi.astype(np.int32)


@dataclass
class EventSweep:
    """``hits``, ``false_alarms``, ``repeats`` (int32 ``(n, T)``) and ``latency_samples`` (int64 ``(n, T)``: the sum over
    the hits of recording ``c`` at ``thresholds[t]``), on the device; ``thresholds`` (host float64 ``(T,)``); ``gap``: the
    debounce in windows; ``k_lo`` / ``k_hi``: the window ranges of the truth events (host int32)."""
    thresholds: torch.Tensor
    hits: torch.Tensor
    false_alarms: torch.Tensor
    repeats: torch.Tensor
    latency_samples: torch.Tensor
    gap: int
    k_lo: np.ndarray
    k_hi: np.ndarray


def _truth_upload(dev, truth: TruthTable, k_lo: np.ndarray, k_hi: np.ndarray):
    i64, i32 = _upload(dev, truth.offsets, np.concatenate([k_lo, k_hi, truth.onset]).astype(np.int32))
    m = len(truth)
    return i64, i32[:m], i32[m:2 * m], i32[2 * m:]


def match_events(scores: WindowScores, truth: TruthTable, thresholds, debounce_seconds: float = 0.5,
                 min_overlap_seconds: float = 0.1, collar_seconds: Optional[float] = None) -> EventSweep:
    """Every detection of every recording at every one of ``thresholds`` (1..1024 finite values) classified against
    ``truth`` (rule 8).  One launch; nothing is read back."""
    what = "match_events"
    t = _check_thresholds(what, thresholds)
    k_lo, k_hi = truth_window_ranges(truth, scores, min_overlap_seconds, collar_seconds)
    gap = debounce_gap(debounce_seconds, scores.sample_rate, scores.hop_samples, what)
    dev, n, nt, m = _check_device(what, scores.device), len(scores), int(t.size), len(truth)
    i32 = dict(dtype=torch.int32, device=dev)
    hits, fas, reps = torch.empty((n, nt), **i32), torch.empty((n, nt), **i32), torch.empty((n, nt), **i32)
    late = torch.empty((n, nt), dtype=torch.int64, device=dev)
    if n:
        offs, lo_dev, hi_dev, onset_dev = _truth_upload(dev, truth, k_lo, k_hi)
        thr = torch.from_numpy(t).to(dev, non_blocking=True)
        nw = scores.smoothed.numel()
        _lib.check_scenes(_lib.load_scenes().cough_match_events(
            scores.smoothed.data_ptr() if nw else None, scores.window_offsets_dev.data_ptr(), n, nw, thr.data_ptr(), nt, gap,
            offs.data_ptr(), lo_dev.data_ptr() if m else None, hi_dev.data_ptr() if m else None,
            onset_dev.data_ptr() if m else None, m, scores.hop_samples, scores.window_samples, hits.data_ptr(),
            fas.data_ptr(), reps.data_ptr(), late.data_ptr(), _stream(dev)), "cough_match_events")
    return EventSweep(torch.from_numpy(t), hits, fas, reps, late, gap, k_lo, k_hi)


def list_matches(scores: WindowScores, truth: TruthTable, threshold: float, debounce_seconds: float = 0.5,
                 min_overlap_seconds: float = 0.1, collar_seconds: Optional[float] = None,
                 event_counts=None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """At one threshold: ``truth_window`` (int32 per truth event on the device: the window that hit it, or -1) and, when
    ``event_counts`` (the per-recording counts of ``detect_events`` at this threshold and debounce) is given, the class of
    every fired window in the event table's order (int32 on the device: 0 hit, 1 repeat, 2 false alarm), else None."""
    what = "list_matches"
    t = _check_thresholds(what, [_number(what, "threshold", threshold)])
    k_lo, k_hi = truth_window_ranges(truth, scores, min_overlap_seconds, collar_seconds)
    gap = debounce_gap(debounce_seconds, scores.sample_rate, scores.hop_samples, what)
    n, m, per = len(scores), len(truth), None
    if event_counts is not None:
        per = _ints(what, "event_counts", event_counts, n)
        if per.size and per.min() < 0:
            raise ValueError(f"{what}: event_counts must not be negative")
    dev = _check_device(what, scores.device)
    window = torch.empty(m, dtype=torch.int32, device=dev)
    classes = torch.empty(int(per.sum()), dtype=torch.int32, device=dev) if per is not None else None
    if n:
        offs, lo_dev, hi_dev, _ = _truth_upload(dev, truth, k_lo, k_hi)
        ev_offs = None
        if per is not None and classes.numel():
            ev_offs, _ = _upload(dev, _offsets(per), np.zeros(0, np.int32))
        nw = scores.smoothed.numel()
        _lib.check_scenes(_lib.load_scenes().cough_list_event_matches(
            scores.smoothed.data_ptr() if nw else None, scores.window_offsets_dev.data_ptr(), n, nw, float(t[0]), gap,
            offs.data_ptr(), lo_dev.data_ptr() if m else None, hi_dev.data_ptr() if m else None, m,
            window.data_ptr() if m else None, ev_offs.data_ptr() if ev_offs is not None else None,
            classes.numel() if ev_offs is not None else 0, classes.data_ptr() if ev_offs is not None else None,
            _stream(dev)), "cough_list_event_matches")
    return window, classes


# ------------------------------------------------------------------------------------------------ reports
def event_report(bank: DeviceClipBank, scores: WindowScores, sweep: EventSweep, truth: TruthTable) -> dict:
    """The plan's event-level table, per threshold: ``recall`` (hits / truth events), ``false_alarms_per_minute`` over all
    minutes and ``false_alarms_per_minute_event_free`` over the recordings without an event, ``repeats``,
    ``mean_latency_seconds`` and the counts behind them (``hits``, ``misses``, ``false_alarms``,
    ``false_alarms_event_free``, ``latency_samples``); ``None`` where a ratio has no denominator.  The integer sums are
    formed on the device and read once."""
    what = "event_report"
    _check_bank(what, bank, scores)
    if sweep.hits.shape[0] != len(bank) or truth.counts.size != len(bank):
        raise ValueError(f"{what}: the sweep counts {sweep.hits.shape[0]} recordings, the truth {truth.counts.size}, the "
                         f"bank holds {len(bank)}")
    dev = _check_device(what, scores.device)
    free = torch.from_numpy(truth.counts == 0).to(dev).unsqueeze(1)
    fas = sweep.false_alarms.to(torch.int64)
    sums = torch.stack([sweep.hits.to(torch.int64).sum(0), fas.sum(0), sweep.repeats.to(torch.int64).sum(0),
                        sweep.latency_samples.sum(0), (fas * free).sum(0)]).cpu().numpy()     # the one host read
    lengths, sr, total = bank.lengths.numpy().astype(np.int64), scores.sample_rate, len(truth)
    minutes = float(int(lengths.sum())) / sr / 60.0
    minutes_free = float(int(lengths[truth.counts == 0].sum())) / sr / 60.0
    hits, fa, reps, late, fa_free = (row.tolist() for row in sums)
    return {"thresholds": sweep.thresholds.tolist(), "gap_windows": int(sweep.gap), "hop_samples": scores.hop_samples,
            "window_samples": scores.window_samples, "smoothing_window": scores.smoothing_window,
            "recordings": len(bank), "recordings_event_free": int((truth.counts == 0).sum()), "truth_events": total,
            "minutes": minutes, "minutes_event_free": minutes_free,
            "hits": hits, "misses": [total - h for h in hits], "false_alarms": fa, "false_alarms_event_free": fa_free,
            "repeats": reps, "latency_samples": late,
            "recall": [h / total if total else None for h in hits],
            "false_alarms_per_minute": [v / minutes if minutes > 0 else None for v in fa],
            "false_alarms_per_minute_event_free": [v / minutes_free if minutes_free > 0 else None for v in fa_free],
            "mean_latency_seconds": [v / h / sr if h else None for v, h in zip(late, hits)]}


def pick_threshold(report: dict, max_false_alarms_per_minute: float = 1.0, min_recall: float = 0.8) -> dict:
    """The lowest threshold of ``report`` whose ``false_alarms_per_minute`` is at most the bar, and whether the recall
    there reaches ``min_recall`` -- the plan's two numbers: ``{"threshold", "index", "recall", "false_alarms_per_minute",
    "meets_recall"}``; ``threshold`` and ``index`` are None when no threshold meets the false-alarm bar."""
    what = "pick_threshold"
    bar, need = _number(what, "max_false_alarms_per_minute", max_false_alarms_per_minute), _number(what, "min_recall", min_recall)
    best = None
    for k, (t, fa) in enumerate(zip(report["thresholds"], report["false_alarms_per_minute"])):
        if fa is not None and fa <= bar and (best is None or t < report["thresholds"][best]):
            best = k
    if best is None:
        return {"threshold": None, "index": None, "recall": None, "false_alarms_per_minute": None, "meets_recall": False}
    recall = report["recall"][best]
    return {"threshold": report["thresholds"][best], "index": best, "recall": recall,
            "false_alarms_per_minute": report["false_alarms_per_minute"][best],
            "meets_recall": recall is not None and recall >= need}


def missed_events(scenes: DeviceClipBank, truth: TruthTable, scores: WindowScores, threshold: float,
                  debounce_seconds: float = 0.5, min_overlap_seconds: float = 0.1,
                  collar_seconds: Optional[float] = None) -> Tuple[DeviceClipBank, np.ndarray]:
    """The truth events no detection hit at ``threshold``, cut from ``scenes`` as a bank of cough clips (label 1) -- the
    counterpart of ``event_windows``' hard negatives -- and their indices into ``truth``.  One host read (which events
    were hit); ``cough_list_event_matches``, then ``cough_copy_segments``."""
    what = "missed_events"
    _check_bank(what, scenes, scores)
    if truth.counts.size != len(scenes):
        raise ValueError(f"{what}: the truth counts {truth.counts.size} recordings, the bank holds {len(scenes)}")
    if (truth.offset > scenes.lengths.numpy().astype(np.int64)[truth.clip]).any():
        raise ValueError(f"{what}: a truth event reaches past the end of its recording")
    window, _ = list_matches(scores, truth, threshold, debounce_seconds, min_overlap_seconds, collar_seconds)
    _check_device(what, scenes.device)
    missed = np.flatnonzero(window.cpu().numpy() < 0)                     # the one host read
    return scenes.cut(truth.clip[missed], truth.onset[missed], (truth.offset - truth.onset)[missed], [1] * missed.size), missed


# ------------------------------------------------------------------------------------------------ CLI
def _bank_of(directory, preprocessor, label: int) -> DeviceClipBank:
    """The WAVE files of ``directory`` (sorted by name), resampled and mono, as a bank with one label."""
    from pathlib import Path
    waves = []
    for f in sorted(Path(directory).iterdir()):
        if f.suffix.lower() == ".wav":
            w, sr = preprocessor.load_audio(str(f))
            waves.append(preprocessor.to_mono(preprocessor.resample(w, sr)).cpu())
    if not waves:
        raise ValueError(f"{directory}: no WAVE files")
    return DeviceClipBank(waves, [label] * len(waves))


def main(argv: Optional[Sequence[str]] = None) -> dict:
    import argparse
    import csv
    import json
    import os
    from .inference import CoughDetectorInference
    from .score import score_bank
    from .slices import write_clips
    parser = argparse.ArgumentParser(prog="python -m cough_detector_amd.scenes",
                                     description="Compose cough soundscapes and score the detector by event (MI355X path)")
    parser.add_argument("checkpoint", help="trained model checkpoint")
    parser.add_argument("background_dir", help="directory of background WAVE files (speech, room noise, silence)")
    parser.add_argument("cough_dir", help="directory of clean cough segments (WAVE)")
    parser.add_argument("--scenes", type=int, default=64)
    parser.add_argument("--seconds", type=float, default=60.0, help="length of a scene")
    parser.add_argument("--events", type=str, default="5,10", help="lo,hi coughs per scene")
    parser.add_argument("--snr", type=str, default="5,20", help="lo,hi dB")
    parser.add_argument("--sweep", type=int, default=101, help="this many thresholds evenly spaced over 0..1")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--hop", type=float, default=0.25, help="seconds between windows")
    parser.add_argument("--smoothing", type=int, default=3, help="windows in the smoothing mean")
    parser.add_argument("--debounce", type=float, default=0.5, help="minimum seconds between detections")
    parser.add_argument("--write", type=str, default=None, help="save the scenes (WAVE) and truth.csv here")
    args = parser.parse_args(argv)
    if args.sweep < 2:
        parser.error("--sweep needs at least 2 thresholds")
    try:
        events = tuple(int(v) for v in args.events.split(","))
        snr = tuple(float(v) for v in args.snr.split(","))
    except ValueError:
        parser.error("--events takes lo,hi integers and --snr lo,hi numbers")
    engine = CoughDetectorInference(args.checkpoint, verbose=False)
    pre = engine.preprocessor
    backgrounds, coughs = _bank_of(args.background_dir, pre, 0), _bank_of(args.cough_dir, pre, 1)
    plan = draw_scene_plan(backgrounds, coughs, args.scenes, args.seconds, events_per_scene=events, snr_range=snr,
                           seed=args.seed, sample_rate=int(pre.sample_rate))
    scenes, truth = compose_scenes(backgrounds, coughs, plan)
    scores = score_bank(scenes, engine._pipeline, hop_duration=args.hop, smoothing_window=args.smoothing)
    sweep = match_events(scores, truth, np.linspace(0.0, 1.0, args.sweep), debounce_seconds=args.debounce)
    report = event_report(scenes, scores, sweep, truth)
    report["pick"] = pick_threshold(report)
    if args.write:
        write_clips(scenes, args.write, [f"scene_{k:05d}" for k in range(len(scenes))], sample_rate=int(pre.sample_rate))
        gains = truth.gain.cpu().numpy()
        with open(os.path.join(args.write, "truth.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["scene", "onset_samples", "offset_samples", "source_clip", "snr_db", "gain"])
            for j in range(len(truth)):
                w.writerow([int(truth.clip[j]), int(truth.onset[j]), int(truth.offset[j]), int(truth.source[j]),
                            repr(float(truth.snr_db[j])), repr(float(gains[j]))])
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
