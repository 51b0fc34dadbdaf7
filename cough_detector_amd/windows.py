"""Training windows composed on the MI355X: coughs at any phase of the window, over a background at a chosen SNR, with
labels that follow from what was placed -- and the validation bank that judges a model on the same kind of window.

The live engine, ``score_bank`` and the event-level evaluation of ``scenes.py`` all judge the detector on sliding windows
of ``segment_samples`` that cut a recording wherever the hop lands: a cough is seen in four to seven consecutive windows,
some holding only its first 100 ms, some only its tail, most with speech under it, and ``truth_window_ranges`` counts a
window for a cough as soon as it overlaps it by ``min_overlap_seconds``.  The clips the trainers otherwise see are centred
on their energy peak.  Here every batch is composed anew: per row a stretch of background, and up to four event clips
laid over it wherever the draw put them -- in front of sample 0, past the end, over each other.  One fused kernel
(``cough_compose_windows`` of ``libcough_amd_windows.so``, ``include/cough_amd_windows.h``) does a whole batch in one
launch: the background's power, the gains and the mix, in the arithmetic of ``compose_scenes``' three kernels.

Specification.  A row has ``width`` samples; ``sr`` samples per second.

1. Background: clip ``b`` of the background bank (``-1``: silence), ``n_b`` samples, read cyclically from ``bg_start``.
2. Events: slots ``0 .. n_events - 1`` (at most 4), slot ``e`` clip ``c_e`` of the event bank placed with its first
   sample at ``onset[e]``, which may be negative; events may overlap; what falls outside ``[0, width)`` is cut.
3. Powers (float64): ``P_bg`` over the ``width`` background samples the row reads (``span_power``'s bits), ``P_ev[c]``
   over the whole event clip -- not over the part of it that is visible.
4. Gain: ``gain[e] = float32(sqrt(snr_linear * double(bg_gain)^2 * P_bg / P_ev[c_e]))``, ``snr_linear = 10 ** (snr_db /
   10)`` from the host; 1.0 when either power is 0 or not finite.
5. Mix (float32): ``acc = bg_gain * B[(bg_start + i) mod n_b]``, then for ``e`` in slot order where the event covers
   ``i``: ``acc = fmaf(gain[e], E_e[i - onset[e]], acc)``.
6. Label (``WindowPlan.labels``): a row is 1 iff one of its events is a clip labelled 1.  Clips labelled 0 in the event
   bank (laughs, sneezes, throat clearing) are distractors: hard negatives in context.
7. Inner-window rule (``draw_window_plan``): with ``m = max(1, ceil(min_overlap_seconds * sr))``, ``m_c = min(m, n_c)``
   and ``need = min(n_c, ceil(m_c / rho_min))``, at least ``need`` samples of a drawn clip lie inside ``[margin, width -
   margin)``: the onset is uniform over the integers ``margin + need - n_c .. width - margin - need``.  ``margin`` and
   ``rho_min`` describe the waveform chain behind the composer (``edge_margin``, ``speed_ratios``): whatever that chain
   then does to the row, at least ``min(m, what the chain left of the clip's length)`` samples of the clip, give or take
   two for rounding, are still inside the window, so the label stays true by ``truth_window_ranges``' own rule.  (A
   clip shorter than ``m / rho_min`` lies wholly inside the inner window.)
8. Window labels (``window_labels``): window ``k`` of a recording is samples ``[k*hop, k*hop + window)``.  With ``m_j =
   min(m, offset_j - onset_j)``: label 1 iff some event overlaps it by at least its ``m_j`` samples (rule 7 of
   ``scenes.py``), label 0 iff no event overlaps it at all, label -1 (ambiguous) otherwise.

Draws (``draw_window_plan``): one ``numpy.random.Generator(Philox(seed))``, every draw vectorised over the batch of ``b``
rows and made whether or not the row uses it, in this order: the background clips (``integers(0, n_backgrounds,
size=b)``), ``bg_start`` (``integers(0, n_b)``, one per row), ``bg_gain`` (``uniform(lo, hi, size=b)``), the cough coin
(``random(b) < p_cough``), the number of coughs (``integers(lo, hi + 1, size=b)``), the distractor coin (``random(b) <
p_distractor``), the number of distractors (``integers(1, 3, size=b)``, cut to what the four slots leave), the cough
clips (``integers(0, n_coughs, size=(b, 4))`` into the clips labelled 1), the distractor clips (``integers(0,
n_distractors, size=(b, 4))`` into the clips labelled 0), the SNRs (``uniform(lo, hi, size=(b, 4))``) and the onsets
(``integers(lowest, highest + 1)``, ``(b, 4)``, rule 7's bounds; ``0 .. 0`` for a slot that is not used).  An empty
background bank skips the first two draws and every row is silence.  The coughs take the first slots, the distractors
the next.

``compose_windows`` is one pinned upload and one launch and reads nothing back.  ``ComposedWindowLoader`` composes every
batch into one reusable bank and hands it to an ordinary ``DeviceDataLoader``, so everything behind the composer -- shift,
speed, pitch, reverb, gain, noise, channel, ``cough_prepare_rows``, the featuriser, masks, MixUp -- is the existing code
with its existing draws.

Draws on the device (``draw_window_records``, ``ComposedWindowLoader(plan_draws="device")``): ``cough_draw_window_plans``
of ``libcough_amd_windraw.so`` writes the same records and the rows' labels from Philox4x32-10 blocks under the batch
seed, one thread per row; ``include/cough_amd_windraw.h`` states the contract.  The distributions are the ones above but
for the SNR, which is one of the 1024 level centres of ``snr_levels(snr_range)``; the stream is not numpy's.
``train_windows`` (``python -m cough_detector_amd.windows``) wires the loader, a held-out validation bank of composed
scenes, ``fit`` and the event-level report of the checkpoint into one call.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .augmentation import _SHIFT_LIMIT, AudioAugmentor, MixUp, SpecAugment
from .data import DeviceClipBank, DeviceDataLoader, _ragged, _stream, _upload
from .scenes import TruthTable, _bank_lengths, _ints, _pair, span_power
from .score import _check_device, _number, hop_samples, windows_per_clip

MAX_EVENTS = 4                 # COUGH_WINDOWS_MAX_EVENTS
MAX_WIDTH = 1 << 20            # COUGH_WINDOWS_MAX_WIDTH
_I32_MAX = 2**31 - 1
# cough_window_plan, byte for byte
PLAN_DTYPE = np.dtype([("background", "<i4"), ("bg_start", "<i4"), ("bg_gain", "<f4"), ("n_events", "<i4"),
                       ("clip", "<i4", (MAX_EVENTS,)), ("onset", "<i4", (MAX_EVENTS,)), ("snr_linear", "<f8", (MAX_EVENTS,))])
assert PLAN_DTYPE.itemsize == 80


# ------------------------------------------------------------------------------------------------ the plan
def _check_width(what: str, width) -> int:
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"{what}: width={width!r} must be an integer in 1..2^20")
    return int(width)


@dataclass
class WindowPlan:
    """What to compose, on the host, per row: ``background`` (clip of the background bank, -1 for silence), ``bg_start``
    (its first sample read), ``bg_gain`` (float32), ``n_events`` (0..4) and, ``(B, 4)`` each, ``event_clip`` (clip of the
    event bank), ``onset`` (samples from the row's first sample; may be negative) and ``snr_db`` (float64).  The slots
    from ``n_events`` on are not read."""
    background: np.ndarray
    bg_start: np.ndarray
    bg_gain: np.ndarray
    n_events: np.ndarray
    event_clip: np.ndarray
    onset: np.ndarray
    snr_db: np.ndarray

    def __len__(self) -> int:
        return int(np.asarray(self.background).size)

    def used(self) -> np.ndarray:
        """bool ``(B, 4)``: the slots below ``n_events``."""
        return np.arange(MAX_EVENTS)[None, :] < np.asarray(self.n_events).reshape(-1, 1)

    def checked(self, bg_lengths, ev_lengths, width: int, what: str = "WindowPlan") -> "WindowPlan":
        """The plan with its arrays normalised (int64 / float32 / float64) after checking it against the lengths of the
        two banks' clips and the rows' ``width``: backgrounds in range or -1, ``bg_start`` inside its clip (0 for
        silence), gains finite, ``n_events`` in 0..4 and, in the slots used, clips in range, onsets that fit an int32 and
        finite SNRs.  Where an event lies -- across an edge, over another, outside the row -- is not checked: all of
        that is allowed."""
        width = _check_width(what, width)
        bl, el = _ints(what, "bg_lengths", bg_lengths), _ints(what, "ev_lengths", ev_lengths)
        bg = _ints(what, "background", self.background)
        n = bg.size
        start, count = _ints(what, "bg_start", self.bg_start, n), _ints(what, "n_events", self.n_events, n)
        gain = np.asarray(self.bg_gain, dtype=np.float32).reshape(-1)
        if gain.size != n or not np.isfinite(gain).all():
            raise ValueError(f"{what}: bg_gain must hold {n} finite values")
        if n and (bg.min() < -1 or bg.max() >= bl.size):
            raise ValueError(f"{what}: background indices must lie in -1..{bl.size - 1}")
        limit = np.where(bg >= 0, bl[np.maximum(bg, 0)] if bl.size else 1, 1)
        if ((start < 0) | (start >= limit)).any():
            r = int(np.flatnonzero((start < 0) | (start >= limit))[0])
            raise ValueError(f"{what}: row {r}: bg_start={int(start[r])} lies outside its background of {int(limit[r])} "
                             "samples (0 for silence)")
        if n and (count.min() < 0 or count.max() > MAX_EVENTS):
            raise ValueError(f"{what}: n_events must lie in 0..{MAX_EVENTS}")
        clip = _ints(what, "event_clip", self.event_clip, n * MAX_EVENTS).reshape(n, MAX_EVENTS)
        onset = _ints(what, "onset", self.onset, n * MAX_EVENTS).reshape(n, MAX_EVENTS)
        snr = np.asarray(self.snr_db, dtype=np.float64).reshape(-1)
        if snr.size != n * MAX_EVENTS:
            raise ValueError(f"{what}: snr_db holds {snr.size} values, expected {n * MAX_EVENTS}")
        snr = snr.reshape(n, MAX_EVENTS)
        used = np.arange(MAX_EVENTS)[None, :] < count[:, None]
        if used.any():
            if clip[used].min() < 0 or clip[used].max() >= el.size:
                raise ValueError(f"{what}: event clips must lie in 0..{el.size - 1}")
            if np.abs(onset[used]).max() > _I32_MAX:
                raise ValueError(f"{what}: onsets must fit an int32")
            if not np.isfinite(snr[used]).all():
                raise ValueError(f"{what}: snr_db must be finite in the slots used")
        # what no slot uses travels as zeros
        return WindowPlan(bg, start, gain, count, np.where(used, clip, -1), np.where(used, onset, 0), np.where(used, snr, 0.0))

    def labels(self, event_labels) -> np.ndarray:
        """int64 ``(B,)``: 1 for a row one of whose events is a clip labelled 1 in ``event_labels`` (the event bank's
        ``labels``), else 0."""
        lab = _ints("WindowPlan.labels", "event_labels", event_labels)
        clip = np.asarray(self.event_clip, dtype=np.int64).reshape(len(self), MAX_EVENTS)
        used = self.used()
        if used.any() and (clip[used].min() < 0 or clip[used].max() >= lab.size):
            raise ValueError(f"WindowPlan.labels: event clips must lie in 0..{lab.size - 1}")
        cough = lab[np.where(used, clip, 0)] == 1 if lab.size else np.zeros_like(used)
        return (used & cough).any(axis=1).astype(np.int64)

    def records(self) -> np.ndarray:
        """The plan as ``cough_window_plan`` records (``PLAN_DTYPE``), one per row."""
        rec = np.zeros(len(self), dtype=PLAN_DTYPE)
        rec["background"], rec["bg_start"], rec["bg_gain"], rec["n_events"] = self.background, self.bg_start, self.bg_gain, self.n_events
        rec["clip"], rec["onset"] = self.event_clip, self.onset
        rec["snr_linear"] = 10.0 ** (np.asarray(self.snr_db, dtype=np.float64) / 10.0)
        return rec


def speed_ratios(augmentor: Optional[AudioAugmentor]) -> Tuple[float, float]:
    """``(rho_min, rho_max)``: the least and the greatest factor by which the augmentor's speed step can stretch a row,
    ``rho = sample_rate / int(f * sample_rate)`` at the two ends of ``speed_range``; ``(1.0, 1.0)`` without a speed step."""
    if augmentor is None or not augmentor.speed:
        return 1.0, 1.0
    sr = int(augmentor.sample_rate)
    rho = [sr / int(f * sr) for f in augmentor.speed_range]
    return min(rho), max(rho)


def edge_margin(augmentor: Optional[AudioAugmentor], width: int) -> int:
    """The largest displacement, in samples, that the waveform chain behind the composer can give a sample of a row of
    ``width``: 0 without an augmentor, else ``ceil(rho_max * 0.2 * width + width * max|rho - 1| / 2) + 1``.

    A sample at ``p`` goes, by the time shift ``s`` (zero fill, ``|s| <= int(0.2 * width)``), to ``p + s``; by the speed
    step, which warps about sample 0, to ``rho * (p + s)`` in a row of ``n' = ceil(rho * width)`` samples; and by
    ``pad_or_trim``'s symmetric crop or pad to ``rho * (p + s) - (n' - width) / 2``, half a sample either way.  Its
    displacement ``(rho - 1) * (p - width / 2) + rho * s`` is largest at a row's edge with the largest shift; the ``+
    1`` covers the two roundings.  Pitch shift keeps positions and a reverb's direct path is tap 0, so neither moves an
    onset.  The consequence: with an augmentor, ``draw_window_plan`` keeps the part of a clip that makes the label true
    in the central ``width - 2 * margin`` samples, and it is the augmentor's own shift that then spreads the events to
    the window's edges; without one the full range of phases is drawn directly."""
    width = _check_width("edge_margin", width)
    if augmentor is None:
        return 0
    rho_min, rho_max = speed_ratios(augmentor)
    return int(math.ceil(rho_max * _SHIFT_LIMIT * width + width * max(abs(rho_min - 1.0), abs(rho_max - 1.0)) / 2.0)) + 1


def min_overlap_samples(min_overlap_seconds, sample_rate: int, what: str = "min_overlap_samples") -> int:
    overlap = _number(what, "min_overlap_seconds", min_overlap_seconds)
    if overlap < 0:
        raise ValueError(f"{what}: min_overlap_seconds={min_overlap_seconds} must not be negative")
    return max(1, math.ceil(overlap * sample_rate))


def _probability(what: str, name: str, v) -> float:
    p = _number(what, name, v)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{what}: {name}={v!r} must lie in 0..1")
    return p


def draw_window_plan(backgrounds: DeviceClipBank, events: DeviceClipBank, b: int, width: int, sample_rate: int = 16000,
                     seed: int = 0, p_cough: float = 0.5, p_distractor: Optional[float] = None, coughs_per_window=(1, 2),
                     snr_range=(5, 20), bg_gain_range=(1.0, 1.0), min_overlap_seconds: float = 0.1, margin: int = 0,
                     rho_min: float = 1.0) -> WindowPlan:
    """A plan of ``b`` rows of ``width`` samples, drawn in the order the module docstring states.  A row is positive
    against ``p_cough`` and then holds ``coughs_per_window[0] .. [1]`` clips of ``events`` labelled 1; every row,
    independently, holds one or two clips labelled 0 against ``p_distractor`` (default: 0.3 when ``events`` holds such
    clips, else 0); four events per row at most.  Onsets follow the inner-window rule (rule 7) for ``margin`` and
    ``rho_min`` (``edge_margin`` / ``speed_ratios`` of the augmentor behind the composer; 0 and 1 without one): an inner
    window that cannot hold ``ceil(m / rho_min)`` samples raises ``ValueError``."""
    what = "draw_window_plan"
    (bl, el, width, b, coughs, distractors, p_cough, p_dis, c_lo, c_hi, snr_lo, snr_hi, g_lo, g_hi, rho_min,
     m) = _draw_arguments(what, backgrounds, events, b, width, sample_rate, seed, p_cough, p_distractor, coughs_per_window,
                          snr_range, bg_gain_range, min_overlap_seconds, margin, rho_min)

    rng = np.random.Generator(np.random.Philox(int(seed)))
    if bl.size:
        background = rng.integers(0, bl.size, size=b)
        start = rng.integers(0, bl[background])
    else:
        background, start = np.full(b, -1, np.int64), np.zeros(b, np.int64)
    gain = rng.uniform(g_lo, g_hi, size=b).astype(np.float32)
    positive = rng.random(b) < p_cough
    n_coughs = np.where(positive, rng.integers(c_lo, c_hi + 1, size=b), 0)
    distracted = rng.random(b) < p_dis
    n_dis = np.where(distracted, np.minimum(rng.integers(1, 3, size=b), MAX_EVENTS - n_coughs), 0)
    pick_c = rng.integers(0, max(coughs.size, 1), size=(b, MAX_EVENTS))
    pick_d = rng.integers(0, max(distractors.size, 1), size=(b, MAX_EVENTS))
    snr = rng.uniform(snr_lo, snr_hi, size=(b, MAX_EVENTS))
    slot = np.arange(MAX_EVENTS)[None, :]
    is_cough, used = slot < n_coughs[:, None], slot < (n_coughs + n_dis)[:, None]
    clip = np.where(is_cough, coughs[pick_c] if coughs.size else -1, distractors[pick_d] if distractors.size else -1)
    clip = np.where(used, clip, -1)
    n_c = np.where(used, el[np.maximum(clip, 0)] if el.size else 0, 0)
    need = np.minimum(n_c, np.ceil(np.minimum(m, n_c) / rho_min).astype(np.int64))
    lowest = np.where(used, int(margin) + need - n_c, 0)
    highest = np.where(used, width - int(margin) - need, 0)
    onset = rng.integers(lowest, highest + 1)
    return WindowPlan(background, start, gain, n_coughs + n_dis, clip, onset, np.where(used, snr, 0.0)).checked(bl, el, width, what)


def _draw_arguments(what, backgrounds, events, b, width, sample_rate, seed, p_cough, p_distractor, coughs_per_window,
                    snr_range, bg_gain_range, min_overlap_seconds, margin, rho_min):
    """The argument checks that ``draw_window_plan`` and ``draw_window_records`` share, in one order and with one set of
    messages; returns the checked values, the ``p_distractor=None`` rule resolved, the clips labelled 1 and 0 and ``m``."""
    bl, el = _bank_lengths(what, "backgrounds", backgrounds), _bank_lengths(what, "events", events)
    width = _check_width(what, width)
    for name, v, low in (("b", b, 0), ("sample_rate", sample_rate, 1), ("seed", seed, 0), ("margin", margin, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
            raise ValueError(f"{what}: {name}={v!r} must be an integer >= {low}")
    b = int(b)
    labels = events.labels.numpy()
    coughs, distractors = np.flatnonzero(labels == 1), np.flatnonzero(labels == 0)
    p_cough = _probability(what, "p_cough", p_cough)
    p_dis = (0.3 if distractors.size else 0.0) if p_distractor is None else _probability(what, "p_distractor", p_distractor)
    c_lo, c_hi = _pair(what, "coughs_per_window", coughs_per_window, True)
    if not 1 <= c_lo <= c_hi <= MAX_EVENTS:
        raise ValueError(f"{what}: coughs_per_window={coughs_per_window!r} must satisfy 1 <= lo <= hi <= {MAX_EVENTS}")
    snr_lo, snr_hi = _pair(what, "snr_range", snr_range, False)
    g_lo, g_hi = _pair(what, "bg_gain_range", bg_gain_range, False)
    if not (np.isfinite(np.float32(g_lo)) and np.isfinite(np.float32(g_hi))):
        raise ValueError(f"{what}: bg_gain_range={bg_gain_range!r} does not fit a float32")
    rho_min = _number(what, "rho_min", rho_min)
    if not 0.0 < rho_min <= 1.0:
        raise ValueError(f"{what}: rho_min={rho_min} must lie in (0, 1]")
    if p_cough > 0 and coughs.size == 0:
        raise ValueError(f"{what}: p_cough={p_cough} but the event bank holds no clip labelled 1")
    if p_dis > 0 and distractors.size == 0:
        raise ValueError(f"{what}: p_distractor={p_dis} but the event bank holds no clip labelled 0")
    m = min_overlap_samples(min_overlap_seconds, sample_rate, what)
    inner = width - 2 * int(margin)
    if inner < math.ceil(m / rho_min):
        raise ValueError(f"{what}: the inner window (width {width} less a margin of {margin} on each side: {inner} samples) "
                         f"cannot hold the {math.ceil(m / rho_min)} samples that min_overlap_seconds={min_overlap_seconds} "
                         f"asks for at rho_min={rho_min}")
    return bl, el, width, b, coughs, distractors, p_cough, p_dis, c_lo, c_hi, snr_lo, snr_hi, g_lo, g_hi, rho_min, m


# ------------------------------------------------------------------------------------------------ the plan, on the device
SNR_LEVELS = 1024              # COUGH_WINDRAW_SNR_LEVELS


def snr_levels(snr_range) -> np.ndarray:
    """float64 ``(1024,)``: ``10 ** ((lo + (hi - lo) * (j + 0.5) / 1024) / 10)``, the linear SNRs at the centres of 1024
    equal steps of ``snr_range`` (dB) -- the table ``cough_draw_window_plans`` picks a row's SNRs from."""
    lo, hi = _pair("snr_levels", "snr_range", snr_range, False)
    lo, hi = float(lo), float(hi)
    return 10.0 ** ((lo + (hi - lo) * (np.arange(SNR_LEVELS, dtype=np.float64) + 0.5) / 1024) / 10)


@dataclass
class WindowDrawTables:
    """What ``cough_draw_window_plans`` reads besides the banks' lengths, on the device, for a loader to keep: ``coughs``
    and ``distractors`` (int32: the event bank's clips labelled 1 and 0, ascending) and ``snr`` (float64 ``(1024,)``:
    ``snr_levels(snr_range)``); ``snr_range`` is the range the table was made for."""
    coughs: torch.Tensor
    distractors: torch.Tensor
    snr: torch.Tensor
    snr_range: Tuple[float, float]

    @classmethod
    def build(cls, events: DeviceClipBank, snr_range) -> "WindowDrawTables":
        """One pinned upload; nothing waits for it."""
        _bank_lengths("WindowDrawTables", "events", events)
        dev = _check_device("WindowDrawTables", events.device)
        labels = events.labels.numpy()
        coughs, distractors = np.flatnonzero(labels == 1).astype(np.int32), np.flatnonzero(labels == 0).astype(np.int32)
        i64, i32 = _upload(dev, snr_levels(snr_range).view(np.int64), np.concatenate([coughs, distractors]))
        return cls(i32[:coughs.size], i32[coughs.size:], i64.view(torch.float64), (float(snr_range[0]), float(snr_range[1])))


def _draw_launch(backgrounds: DeviceClipBank, events: DeviceClipBank, tables: WindowDrawTables, b: int, width: int, seed: int,
                 scalars: tuple) -> Tuple[torch.Tensor, torch.Tensor]:
    """The launch of ``draw_window_records`` on arguments that are checked already.  ``scalars``: ``(p_cough, c_lo, c_hi,
    p_distractor, g_lo, g_hi)`` and ``(m, margin, rho_min)``, the C call's scalars around its SNR table."""
    dev = backgrounds.device
    records = torch.empty((b, PLAN_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    labels = torch.empty(b, dtype=torch.int64, device=dev)
    n_bg, n_ev, n_c, n_d = len(backgrounds), len(events), tables.coughs.numel(), tables.distractors.numel()
    _lib.check_windraw(_lib.load_windraw().cough_draw_window_plans(
        int(seed) & (2**64 - 1), b, width, backgrounds.lengths_dev.data_ptr() if n_bg else None, n_bg,
        events.lengths_dev.data_ptr() if n_ev else None, n_ev, tables.coughs.data_ptr() if n_c else None, n_c,
        tables.distractors.data_ptr() if n_d else None, n_d, *scalars[0], tables.snr.data_ptr(), *scalars[1],
        records.data_ptr(), labels.data_ptr(), _stream(dev)), "cough_draw_window_plans")
    return records, labels


def draw_window_records(backgrounds: DeviceClipBank, events: DeviceClipBank, b: int, width: int, seed: int = 0, *,
                        sample_rate: int = 16000, p_cough: float = 0.5, p_distractor: Optional[float] = None,
                        coughs_per_window=(1, 2), snr_range=(5, 20), bg_gain_range=(1.0, 1.0),
                        min_overlap_seconds: float = 0.1, margin: int = 0, rho_min: float = 1.0,
                        tables: Optional[WindowDrawTables] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``draw_window_plan`` on the device: ``(records, labels)``, a uint8 ``(B, 80)`` tensor of ``cough_window_plan``
    records (``PLAN_DTYPE``; ``compose_window_records`` composes from them, ``read_window_records`` reads them) and the
    rows' labels, int64 ``(B,)``, both on the banks' device.  One launch (``cough_draw_window_plans`` of
    ``libcough_amd_windraw.so``), stream-ordered; nothing is uploaded per call when ``tables``
    (``WindowDrawTables.build(events, snr_range)``) is given, and nothing is read back.

    The arguments are ``draw_window_plan``'s, checked in its order with its messages.  The draws have its distributions
    with one exception, and not its random stream (``include/cough_amd_windraw.h`` states the contract; Philox4x32-10 by
    counter ``(slot, row, 0, 6)`` under ``seed``): an SNR is one of the 1024 level centres of ``snr_levels(snr_range)``
    -- 0.015 dB apart for the default range -- not uniform over the range."""
    what = "draw_window_records"
    (_, _, width, b, coughs, distractors, p_cough, p_dis, c_lo, c_hi, _, _, g_lo, g_hi, rho_min,
     m) = _draw_arguments(what, backgrounds, events, b, width, sample_rate, seed, p_cough, p_distractor, coughs_per_window,
                          snr_range, bg_gain_range, min_overlap_seconds, margin, rho_min)
    if backgrounds.device != events.device:
        raise ValueError(f"{what}: the banks live on {backgrounds.device} and {events.device}; they must share one device")
    _check_device(what, backgrounds.device)
    if tables is None:
        tables = WindowDrawTables.build(events, snr_range)
    elif (not isinstance(tables, WindowDrawTables) or tables.coughs.numel() != coughs.size
          or tables.distractors.numel() != distractors.size or tables.snr.device != events.device
          or tables.snr_range != (float(snr_range[0]), float(snr_range[1]))):
        raise ValueError(f"{what}: tables must be WindowDrawTables.build(events, snr_range) of these events and this range")
    return _draw_launch(backgrounds, events, tables, b, width, seed,
                        ((p_cough, int(c_lo), int(c_hi), p_dis, float(g_lo), float(g_hi)), (m, int(margin), rho_min)))


def read_window_records(records: torch.Tensor) -> np.ndarray:
    """The records of ``draw_window_records`` on the host, a numpy array of ``PLAN_DTYPE`` (one copy that waits for the
    device: for debugging and tests)."""
    _check_records("read_window_records", records, None)
    return records.cpu().numpy().view(PLAN_DTYPE).reshape(-1)


def _check_records(what: str, records, device) -> int:
    if (not isinstance(records, torch.Tensor) or records.dtype != torch.uint8 or records.dim() != 2
            or records.shape[1] != PLAN_DTYPE.itemsize or not records.is_contiguous() or records.data_ptr() % 8
            or (device is not None and records.device != device)):
        raise ValueError(f"{what}: records must be a contiguous, 8-byte aligned uint8 tensor of shape (B, {PLAN_DTYPE.itemsize})"
                         + (f" on {device}" if device is not None else ""))
    return int(records.shape[0])


# ------------------------------------------------------------------------------------------------ composing
def event_powers(events: DeviceClipBank) -> torch.Tensor:
    """float64 ``(len(events),)`` on the device: every event clip's mean power over the whole clip (one launch)."""
    el = _bank_lengths("event_powers", "events", events)
    return span_power(events, np.arange(el.size), np.zeros(el.size, np.int64), el)


def compose_windows(backgrounds: DeviceClipBank, events: DeviceClipBank, plan: WindowPlan, width: int,
                    event_power: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    return_diagnostics: bool = False):
    """The rows of ``plan`` as a float32 ``(B, width)`` tensor on the banks' device: one pinned upload and one launch,
    stream-ordered; nothing is read back.  ``event_power``: ``event_powers(events)``, worked out here when it is not
    given (one more launch: a loader keeps it).  ``out``: where to compose, a contiguous float32 tensor of ``B * width``
    elements on that device that overlaps neither bank.  ``return_diagnostics``: also the rows' background powers
    (float64 ``(B,)``) and the gains (float32 ``(B, 4)``, 0.0 in the slots not used), on the device."""
    what = "compose_windows"
    bl, el = _bank_lengths(what, "backgrounds", backgrounds), _bank_lengths(what, "events", events)
    if not isinstance(plan, WindowPlan):
        raise ValueError(f"{what}: plan must be a WindowPlan, got {type(plan).__name__}")
    plan = plan.checked(bl, el, width, what)
    if backgrounds.device != events.device:
        raise ValueError(f"{what}: the banks live on {backgrounds.device} and {events.device}; they must share one device")
    n, width = len(plan), int(width)
    if event_power is not None and (not isinstance(event_power, torch.Tensor) or event_power.dtype != torch.float64
                                    or event_power.numel() != el.size or event_power.device != events.device
                                    or not event_power.is_contiguous()):
        raise ValueError(f"{what}: event_power must be a contiguous float64 tensor of {el.size} values on {events.device}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.numel() != n * width
                            or out.device != backgrounds.device or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous float32 tensor of {n} x {width} elements on {backgrounds.device}")
    dev = _check_device(what, backgrounds.device)
    if event_power is None:
        event_power = event_powers(events)
    if out is None:
        out = torch.empty((n, width), dtype=torch.float32, device=dev)
    p_bg = torch.empty(n, dtype=torch.float64, device=dev) if return_diagnostics else None
    gains = torch.empty((n, MAX_EVENTS), dtype=torch.float32, device=dev) if return_diagnostics else None
    _launch(backgrounds, events, plan, width, event_power, out, p_bg, gains)
    out = out.view(n, width)
    return (out, p_bg, gains) if return_diagnostics else out


def compose_window_records(backgrounds: DeviceClipBank, events: DeviceClipBank, records: torch.Tensor, width: int,
                           event_power: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                           return_diagnostics: bool = False):
    """``compose_windows`` from records that are on the device already (``draw_window_records``' uint8 ``(B, 80)``): the
    same one launch without the upload; ``event_power``, ``out`` and ``return_diagnostics`` as there.  The host cannot
    check what the records hold; the kernel clamps it to the banks it was given (``include/cough_amd_windows.h``), so a
    garbage record composes a harmless row."""
    what = "compose_window_records"
    _, el = _bank_lengths(what, "backgrounds", backgrounds), _bank_lengths(what, "events", events)
    width = _check_width(what, width)
    if backgrounds.device != events.device:
        raise ValueError(f"{what}: the banks live on {backgrounds.device} and {events.device}; they must share one device")
    n = _check_records(what, records, backgrounds.device)
    if event_power is not None and (not isinstance(event_power, torch.Tensor) or event_power.dtype != torch.float64
                                    or event_power.numel() != el.size or event_power.device != events.device
                                    or not event_power.is_contiguous()):
        raise ValueError(f"{what}: event_power must be a contiguous float64 tensor of {el.size} values on {events.device}")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.numel() != n * width
                            or out.device != backgrounds.device or not out.is_contiguous()):
        raise ValueError(f"{what}: out must be a contiguous float32 tensor of {n} x {width} elements on {backgrounds.device}")
    dev = _check_device(what, backgrounds.device)
    if event_power is None:
        event_power = event_powers(events)
    if out is None:
        out = torch.empty((n, width), dtype=torch.float32, device=dev)
    p_bg = torch.empty(n, dtype=torch.float64, device=dev) if return_diagnostics else None
    gains = torch.empty((n, MAX_EVENTS), dtype=torch.float32, device=dev) if return_diagnostics else None
    _launch_records(backgrounds, events, records, n, width, event_power, out, p_bg, gains)
    out = out.view(n, width)
    return (out, p_bg, gains) if return_diagnostics else out


def _launch(backgrounds: DeviceClipBank, events: DeviceClipBank, plan: WindowPlan, width: int, event_power: torch.Tensor,
            out: torch.Tensor, p_bg: Optional[torch.Tensor] = None, gains: Optional[torch.Tensor] = None) -> None:
    """The upload and the launch of ``compose_windows`` on arguments that are checked already (``plan`` by
    ``WindowPlan.checked``)."""
    if len(plan) == 0:
        return
    records, _ = _upload(backgrounds.device, plan.records().view(np.int64).reshape(-1), np.zeros(0, np.int32))
    _launch_records(backgrounds, events, records, len(plan), width, event_power, out, p_bg, gains)


def _launch_records(backgrounds: DeviceClipBank, events: DeviceClipBank, records: torch.Tensor, n: int, width: int,
                    event_power: torch.Tensor, out: torch.Tensor, p_bg: Optional[torch.Tensor] = None,
                    gains: Optional[torch.Tensor] = None) -> None:
    """The launch of ``cough_compose_windows`` on ``n`` records that are on the device already."""
    n_bg, n_ev, dev = len(backgrounds), len(events), backgrounds.device
    if n == 0:
        return
    _lib.check_windows(_lib.load_windows().cough_compose_windows(
        backgrounds.data.data_ptr() if n_bg else None, backgrounds.data.numel(), backgrounds.offsets_dev.data_ptr() if n_bg else None,
        backgrounds.lengths_dev.data_ptr() if n_bg else None, n_bg, events.data.data_ptr() if n_ev else None, events.data.numel(),
        events.offsets_dev.data_ptr() if n_ev else None, events.lengths_dev.data_ptr() if n_ev else None,
        event_power.data_ptr() if n_ev else None, n_ev, records.data_ptr(), n, int(width), out.data_ptr(),
        p_bg.data_ptr() if p_bg is not None else None, gains.data_ptr() if gains is not None else None, _stream(dev)),
        "cough_compose_windows")


# ------------------------------------------------------------------------------------------------ the loader
class ComposedWindowLoader:
    """Batches of composed windows as ``(features (B, 1, F, T) float32, targets)`` on the banks' device, exactly what a
    ``DeviceDataLoader`` yields: ``fit``, ``train_epoch_async`` and the trainers take it as it is; with ``mixup`` the
    targets are soft ``(B, 2)``, else the rows' labels ``(B,)`` int64.  Iterating it anew is a new epoch of
    ``batches_per_epoch`` batches.

    Batch ``k`` of epoch ``e`` draws its plan with ``draw_window_plan`` under ``(seed + e * batches_per_epoch + k) mod
    2^64`` (``p_cough``, ``p_distractor``, ``coughs_per_window``, ``snr_range``, ``bg_gain_range``,
    ``min_overlap_seconds`` as there; ``margin`` and ``rho_min`` are ``edge_margin`` / ``speed_ratios`` of
    ``audio_augmentor``), composes it with one launch straight into the one bank of ``batch_size`` rows of
    ``preprocessor.segment_samples`` that the loader owns, sets that bank's labels and runs an inner ``DeviceDataLoader``
    over rows ``0 .. B - 1`` of it: ``launch_batch(range(B), draw_batch(range(B)))`` with ``draws="host"``,
    ``launch_batch_drawn(range(B), that seed)`` with ``draws="device"`` when there is anything to draw.  The bank's
    offsets and lengths never change.  The chain behind the composer draws as it always does (``draws="host"``: from
    Python's, numpy's and torch's global generators), so a run repeats itself when those are seeded too.

    ``plan_draws``: ``"host"`` (the default) is the above.  ``"device"`` draws the batch's plan on the device instead,
    under the same batch seed (``draw_window_records``: its distributions but for the 1024 SNR levels, not numpy's
    stream), composes from those records where they are and hands the inner loader the drawn labels as its targets
    (``launch_batch(..., targets=)``): per batch no plan is uploaded, no label is written from the host and no numpy
    runs.  It goes with both ``draws`` modes.  ``last_plan`` is then None; ``last_records`` (uint8 ``(B, 80)``) and
    ``last_labels`` (int64 ``(B,)``) are the device tensors of the latest batch."""

    def __init__(self, backgrounds: DeviceClipBank, events: DeviceClipBank, preprocessor, batch_size: int = 32,
                 batches_per_epoch: Optional[int] = None, seed: int = 0, p_cough: float = 0.5,
                 snr_range=(5, 20), min_overlap_seconds: float = 0.1, audio_augmentor: Optional[AudioAugmentor] = None,
                 spec_augmentor: Optional[SpecAugment] = None, mixup: Optional[MixUp] = None, draws: str = "host",
                 noise: str = "device", p_distractor: Optional[float] = None, coughs_per_window=(1, 2),
                 bg_gain_range=(1.0, 1.0), plan_draws: str = "host"):
        what = "ComposedWindowLoader"
        if plan_draws not in ("device", "host"):
            raise ValueError(f"{what}: plan_draws must be 'device' or 'host', got {plan_draws!r}")
        _bank_lengths(what, "backgrounds", backgrounds), _bank_lengths(what, "events", events)
        if backgrounds.device != events.device:
            raise ValueError(f"{what}: the banks live on {backgrounds.device} and {events.device}; they must share one device")
        for name, v in (("batch_size", batch_size), ("seed", seed)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < (1 if name == "batch_size" else 0):
                raise ValueError(f"{what}: {name}={v!r} must be a {'positive' if name == 'batch_size' else 'non-negative'} integer")
        if batches_per_epoch is None:
            batches_per_epoch = max(1, (len(backgrounds) + len(events)) // int(batch_size))
        if isinstance(batches_per_epoch, bool) or not isinstance(batches_per_epoch, (int, np.integer)) or batches_per_epoch < 1:
            raise ValueError(f"{what}: batches_per_epoch={batches_per_epoch!r} must be a positive integer")
        self.backgrounds, self.events, self.preprocessor = backgrounds, events, preprocessor
        self.batch_size, self.batches_per_epoch, self.seed = int(batch_size), int(batches_per_epoch), int(seed)
        self.width, self.sample_rate = int(preprocessor.segment_samples), int(preprocessor.sample_rate)
        self.margin, self.rho_min = edge_margin(audio_augmentor, self.width), speed_ratios(audio_augmentor)[0]
        self.plan_args = dict(p_cough=p_cough, p_distractor=p_distractor, coughs_per_window=coughs_per_window,
                              snr_range=snr_range, bg_gain_range=bg_gain_range, min_overlap_seconds=min_overlap_seconds,
                              margin=self.margin, rho_min=self.rho_min)
        self.draw_plan(0)                                 # refuse now what no batch could draw
        dev = backgrounds.device
        self.bank = DeviceClipBank.from_packed(torch.zeros(self.batch_size * self.width, dtype=torch.float32, device=dev),
                                               [self.width] * self.batch_size, [0] * self.batch_size)
        self.inner = DeviceDataLoader(self.bank, preprocessor, batch_size=self.batch_size, audio_augmentor=audio_augmentor,
                                      spec_augmentor=spec_augmentor, is_training=True, use_weighted_sampler=False,
                                      drop_last=True, noise=noise, draws=draws, mixup=mixup)
        self.draws, self.epoch = draws, 0
        self._event_power: Optional[torch.Tensor] = None
        self._rows = range(self.batch_size)
        self.last_plan: Optional[WindowPlan] = None
        self.plan_draws = plan_draws
        self.last_records: Optional[torch.Tensor] = None
        self.last_labels: Optional[torch.Tensor] = None
        self._tables: Optional[WindowDrawTables] = None
        self._scalars: Optional[tuple] = None
        if plan_draws == "device":                        # the C call's scalars, checked once
            (_, _, _, _, _, _, p, p_dis, c_lo, c_hi, _, _, g_lo, g_hi, rho,
             m) = _draw_arguments(what, backgrounds, events, self.batch_size, self.width, self.sample_rate, 0, **self.plan_args)
            self._scalars = ((p, int(c_lo), int(c_hi), p_dis, float(g_lo), float(g_hi)), (m, self.margin, rho))

    def __len__(self) -> int:
        return self.batches_per_epoch

    def batch_seed(self, epoch: int, k: int) -> int:
        return (self.seed + int(epoch) * self.batches_per_epoch + int(k)) & (2**64 - 1)

    def draw_plan(self, seed: int) -> WindowPlan:
        return draw_window_plan(self.backgrounds, self.events, self.batch_size, self.width, self.sample_rate, seed,
                                **self.plan_args)

    def launch_batch(self, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The batch drawn under ``seed``: the plan (kept as ``last_plan``), one composing launch, then the inner
        loader's launches; nothing here waits for the device."""
        _check_device("ComposedWindowLoader", self.backgrounds.device)
        if self._event_power is None:
            self._event_power = event_powers(self.events)
        inner, targets = self.inner, None
        if self.plan_draws == "device":
            if self._tables is None:
                self._tables = WindowDrawTables.build(self.events, self.plan_args["snr_range"])
            self.last_plan = None
            records, targets = _draw_launch(self.backgrounds, self.events, self._tables, self.batch_size, self.width, seed,
                                            self._scalars)
            self.last_records, self.last_labels = records, targets
            _launch_records(self.backgrounds, self.events, records, self.batch_size, self.width, self._event_power,
                            self.bank.data)
        else:
            plan = self.last_plan = self.draw_plan(seed)          # checked where it was drawn
            _launch(self.backgrounds, self.events, plan, self.width, self._event_power, self.bank.data)
            self.bank.labels[:] = torch.from_numpy(plan.labels(self.events.labels))
        if self.draws == "device" and (inner._augments or inner._masks or inner._mixes):
            return inner.launch_batch_drawn(self._rows, seed, targets=targets)
        return inner.launch_batch(self._rows, inner.draw_batch(self._rows), targets=targets)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        epoch, self.epoch = self.epoch, self.epoch + 1
        for k in range(self.batches_per_epoch):
            yield self.launch_batch(self.batch_seed(epoch, k))


# ------------------------------------------------------------------------------------------------ labels of real windows
@dataclass
class WindowLabels:
    """Sliding windows of a bank of recordings, recording after recording: ``recording``, ``window`` (its index ``k``
    within the recording: samples ``[k * hop, k * hop + window)``), ``label`` (1, 0, or -1 for ambiguous) and ``overlap``
    (samples of its largest overlap with one event), host int64 arrays; ``hop_samples`` and ``window_samples``."""
    recording: np.ndarray
    window: np.ndarray
    label: np.ndarray
    overlap: np.ndarray
    hop_samples: int
    window_samples: int

    def __len__(self) -> int:
        return int(self.recording.size)

    def select(self, keep: np.ndarray) -> "WindowLabels":
        return WindowLabels(self.recording[keep], self.window[keep], self.label[keep], self.overlap[keep], self.hop_samples,
                            self.window_samples)


def window_labels(truth: TruthTable, clip_lengths, window_samples: int, hop_samples: int, sample_rate: int,
                  min_overlap_seconds: float = 0.1) -> WindowLabels:
    """The label of every sliding window of every recording (rule 8 of the module docstring) from the recordings'
    lengths and their truth, in closed form on the host: per event the range of windows that overlap it at all, each
    (event, window) pair of those ranges once."""
    what = "window_labels"
    if not isinstance(truth, TruthTable):
        raise ValueError(f"{what}: truth must be a TruthTable, got {type(truth).__name__}")
    lengths = _ints(what, "clip_lengths", clip_lengths, truth.counts.size)
    for name, v in (("window_samples", window_samples), ("hop_samples", hop_samples), ("sample_rate", sample_rate)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{what}: {name}={v!r} must be a positive integer")
    window, hop = int(window_samples), int(hop_samples)
    m = min_overlap_samples(min_overlap_seconds, sample_rate, what)
    if m > window:
        raise ValueError(f"{what}: min_overlap_seconds={min_overlap_seconds} is {m} samples, more than a window of {window}: "
                         "no window could count")
    per = windows_per_clip(lengths, window, hop)
    first, recording, k = _ragged(per)                   # first[c]: the flat index of recording c's window 0
    label, overlap = np.zeros(recording.size, np.int64), np.zeros(recording.size, np.int64)
    onset, offset = truth.onset.astype(np.int64), truth.offset.astype(np.int64)
    last = per[truth.clip] - 1
    # the windows with k*hop < offset and k*hop + window > onset
    k_lo = np.maximum((onset - window) // hop + 1, 0)
    k_hi = np.minimum((offset - 1) // hop, last)
    _, event, rank = _ragged(np.maximum(k_hi - k_lo + 1, 0))
    kk = k_lo[event] + rank
    at = first[:-1][truth.clip[event]] + kk
    shared = np.minimum(kk * hop + window, offset[event]) - np.maximum(kk * hop, onset[event])
    np.maximum.at(overlap, at, shared)
    label[at] = -1
    hit = shared >= np.minimum(m, offset - onset)[event]
    label[at[hit]] = 1
    return WindowLabels(recording, k, label, overlap, hop, window)


def scene_window_bank(scenes: DeviceClipBank, truth: TruthTable, preprocessor, hop_duration: float = 0.25,
                      min_overlap_seconds: float = 0.1) -> Tuple[DeviceClipBank, WindowLabels]:
    """The sliding windows of ``scenes`` (composed by ``compose_scenes``, or recordings annotated by hand:
    ``TruthTable.from_intervals``) that are not ambiguous, as a bank of clips of ``preprocessor.segment_samples`` with the
    labels of ``window_labels``, and the table of those windows in the bank's order.  This is the bank of a validation
    loader: ``fit`` then selects its best model on the windows the detector will hear.  One upload and one launch
    (``DeviceClipBank.cut``)."""
    what = "scene_window_bank"
    _bank_lengths(what, "scenes", scenes)
    if not isinstance(truth, TruthTable) or truth.counts.size != len(scenes):
        raise ValueError(f"{what}: truth must be the TruthTable of the {len(scenes)} recordings of scenes")
    window, sr = int(preprocessor.segment_samples), int(preprocessor.sample_rate)
    hop = hop_samples(what, sr, hop_duration)
    table = window_labels(truth, scenes.lengths.numpy(), window, hop, sr, min_overlap_seconds)
    table = table.select(table.label >= 0)
    _check_device(what, scenes.device)
    return scenes.cut(table.recording, table.window * hop, np.full(len(table), window, np.int64), table.label), table


# ------------------------------------------------------------------------------------------------ the one-call trainer
def holdout_split(n: int, holdout: float = 0.2, random_state: int = 42, stream: int = 0) -> Tuple[list, list]:
    """``(kept, held_out)``: the clips ``0 .. n - 1`` of a list of one class split by a permutation drawn from
    ``numpy.random.Generator(Philox(key=random_state + stream))``: its first ``ceil(holdout * n)`` entries are held out,
    the rest kept, each side in ascending order.  (``stratified_split`` is for lists of two classes; each of the three
    lists ``train_windows`` splits has one, and takes ``stream`` 0, 1, 2: backgrounds, coughs, distractors.)"""
    what = "holdout_split"
    if isinstance(holdout, bool) or not isinstance(holdout, (float, np.floating)) or not 0.0 < holdout < 1.0:
        raise ValueError(f"{what}: holdout={holdout!r} must be a float in the (0, 1) range")
    for name, v in (("n", n), ("random_state", random_state), ("stream", stream)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"{what}: {name}={v!r} must be a non-negative integer")
    order = np.random.Generator(np.random.Philox(key=int(random_state) + int(stream))).permutation(int(n))
    cut = int(math.ceil(holdout * n))
    return sorted(order[cut:].tolist()), sorted(order[:cut].tolist())


def _window_banks(backgrounds, events, preprocessor) -> Tuple[DeviceClipBank, DeviceClipBank]:
    """``train_windows``' two inputs as banks: a directory of backgrounds is read as ``scenes._bank_of`` reads one, a
    directory of events is its ``cough/`` (label 1) followed by its ``non_cough/`` (label 0), when there is one."""
    from pathlib import Path
    from .scenes import _bank_of
    if not isinstance(backgrounds, DeviceClipBank):
        backgrounds = _bank_of(backgrounds, preprocessor, 0)
    if not isinstance(events, DeviceClipBank):
        root = Path(events)
        if not (root / "cough").is_dir():
            raise ValueError(f"train_windows: {root} holds no cough/ directory")
        banks = [_bank_of(root / "cough", preprocessor, 1)]
        if (root / "non_cough").is_dir():
            banks.append(_bank_of(root / "non_cough", preprocessor, 0))
        events = banks[0] if len(banks) == 1 else DeviceClipBank.concat(banks)
    return backgrounds, events


def window_split(backgrounds: DeviceClipBank, events: DeviceClipBank, holdout: float = 0.2, random_state: int = 42):
    """``(training backgrounds, training events, held-out backgrounds, held-out coughs)``: ``holdout_split`` of the
    backgrounds (stream 0), of the event clips labelled 1 (stream 1) and of those labelled 0 (stream 2), by clip.  The
    training events are the kept coughs and the kept distractors in the bank's order; the held-out distractors are not
    used.  A side left without a background or without a cough raises ``ValueError``."""
    what = "train_windows"
    _bank_lengths(what, "backgrounds", backgrounds), _bank_lengths(what, "events", events)
    labels = events.labels.numpy()
    coughs, others = np.flatnonzero(labels == 1), np.flatnonzero(labels == 0)
    bg_kept, bg_held = holdout_split(len(backgrounds), holdout, random_state, 0)
    c_kept, c_held = holdout_split(coughs.size, holdout, random_state, 1)
    o_kept, _ = holdout_split(others.size, holdout, random_state, 2)
    for side, bgs, cs in (("held-out", bg_held, c_held), ("training", bg_kept, c_kept)):
        if not bgs:
            raise ValueError(f"{what}: {len(backgrounds)} background(s) at holdout={holdout} leave the {side} side without a background")
        if not cs:
            raise ValueError(f"{what}: {coughs.size} cough(s) at holdout={holdout} leave the {side} side without a cough")
    kept = sorted(coughs[c_kept].tolist() + others[o_kept].tolist())
    return backgrounds.subset(bg_kept), events.subset(kept), backgrounds.subset(bg_held), events.subset(coughs[c_held].tolist())


def train_windows(backgrounds, events, output_dir: str, model_type: str = "small", epochs: int = 100, batch_size: int = 32,
                  learning_rate: float = 1e-3, weight_decay: float = 0.01, patience: int = 15, resume: Optional[str] = None, *,
                  batches_per_epoch: Optional[int] = None, holdout: float = 0.2, random_state: int = 42, val_scenes: int = 32,
                  scene_seconds: float = 30.0, events_per_scene=(3, 6), snr_range=(5, 20), p_cough: float = 0.5,
                  p_distractor: Optional[float] = None, p_augment: float = 0.3, speed: bool = False, draws: str = "device",
                  plan_draws: str = "device", min_overlap_seconds: float = 0.1, sweep: int = 101, seed: int = 0) -> str:
    """Train a detector on composed windows and judge it by event, in one call.

    ``backgrounds``: a directory of WAVE files (speech, room noise, silence) or a ``DeviceClipBank``.  ``events``: a
    directory with ``cough/`` and, optionally, ``non_cough/`` (distractors: laughs, sneezes, throat clearing), or a bank
    with labels 1 and 0.  The preprocessor is ``train.preprocessor_config()``'s.

    Split (``window_split``): backgrounds, coughs and distractors are each split by clip with ``holdout_split`` -- a Philox
    permutation under ``random_state``, since each list has one class -- ``ceil(holdout * n)`` of them held out.
    Training: a ``ComposedWindowLoader`` over the training sides (``batch_size``, ``batches_per_epoch``, ``seed``,
    ``p_cough``, ``p_distractor``, ``snr_range``, ``min_overlap_seconds``, ``draws``, ``plan_draws``) with
    ``AudioAugmentor(p_augment, speed=speed)`` behind the composer and ``SpecAugment(8, 15, 2, 2, p_augment)``.
    Validation: ``val_scenes`` scenes of ``scene_seconds`` with ``events_per_scene`` held-out coughs over held-out
    backgrounds (``draw_scene_plan`` under ``seed + 1``, ``compose_scenes``), cut into the windows the detector will hear
    (``scene_window_bank``) behind a plain ``DeviceDataLoader(is_training=False)``.  The trainer is ``model_type``'s, its
    class weights ``class_weights_from_counts`` of the expected window counts (``round(p_cough * batch_size *
    batches)`` positives per epoch, the rest negatives), so ``p_cough`` must lie strictly inside (0, 1).  ``seed`` also
    seeds ``random``, ``numpy`` and ``torch`` before the model is built, and the trainer's dropout: a run repeats itself
    bit for bit.

    ``fit`` writes ``config.json`` (the preprocessor keys ``CoughDetectorInference`` reads, the training arguments and a
    ``windows`` block of the arguments used here), ``latest_model.pt`` and ``best_model.pt``; ``history.json`` is written
    as ``train`` writes it.  When ``best_model.pt`` exists -- some epoch reached F1 > 0 -- the held-out scenes are scored
    with it (``score_bank``), matched by event over ``sweep`` thresholds evenly spaced over 0..1 (``match_events``) and
    ``event_report`` with its ``pick`` (``pick_threshold``: the recall at under one false alarm per minute) goes to
    ``events.json``.  Returns ``str(Path(output_dir) / "best_model.pt")``.  Nothing here launches a kernel of its own."""
    return _train_windows(**locals())["best_model"]


def _train_windows(backgrounds, events, output_dir, model_type, epochs, batch_size, learning_rate, weight_decay, patience,
                   resume, batches_per_epoch, holdout, random_state, val_scenes, scene_seconds, events_per_scene, snr_range,
                   p_cough, p_distractor, p_augment, speed, draws, plan_draws, min_overlap_seconds, sweep, seed) -> dict:
    """``train_windows``' work; returns ``fit``'s result with ``pick`` (None without a ``best_model.pt``) beside it."""
    import json
    import random
    from pathlib import Path
    from .inference import CoughDetectorInference
    from .loop import class_weights_from_counts, fit
    from .model import create_model
    from .preprocessing import AudioPreprocessor
    from .scenes import compose_scenes, draw_scene_plan, event_report, match_events, pick_threshold
    from .score import score_bank
    from .train import _TRAINERS, MODEL_TYPES, preprocessor_config
    what = "train_windows"
    if model_type not in _TRAINERS:
        raise ValueError(f"{what}: unknown model type {model_type!r}; choose from {list(MODEL_TYPES)}")
    p_cough = _probability(what, "p_cough", p_cough)
    if not 0.0 < p_cough < 1.0:
        raise ValueError(f"{what}: p_cough={p_cough} must lie strictly inside (0, 1): the class weights come from it")
    for name, v, low in (("seed", seed, 0), ("sweep", sweep, 2), ("val_scenes", val_scenes, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
            raise ValueError(f"{what}: {name}={v!r} must be an integer >= {low}")

    pre_config = preprocessor_config()
    preprocessor = AudioPreprocessor(device="cuda", **pre_config)
    backgrounds, events = _window_banks(backgrounds, events, preprocessor)
    train_bg, train_ev, held_bg, held_coughs = window_split(backgrounds, events, holdout, random_state)
    sr = int(preprocessor.sample_rate)

    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    loader = ComposedWindowLoader(train_bg, train_ev, preprocessor, batch_size=batch_size, batches_per_epoch=batches_per_epoch,
                                  seed=seed, p_cough=p_cough, snr_range=snr_range, min_overlap_seconds=min_overlap_seconds,
                                  audio_augmentor=AudioAugmentor(sample_rate=sr, p_augment=p_augment, speed=speed),
                                  spec_augmentor=SpecAugment(freq_mask_param=8, time_mask_param=15, n_freq_masks=2,
                                                             n_time_masks=2, p=p_augment),
                                  draws=draws, p_distractor=p_distractor, plan_draws=plan_draws)
    plan = draw_scene_plan(held_bg, held_coughs, val_scenes, scene_seconds, events_per_scene=events_per_scene,
                           snr_range=snr_range, seed=seed + 1, sample_rate=sr)
    scenes, truth = compose_scenes(held_bg, held_coughs, plan)
    val_bank, _ = scene_window_bank(scenes, truth, preprocessor, min_overlap_seconds=min_overlap_seconds)
    val_loader = DeviceDataLoader(val_bank, preprocessor, batch_size=batch_size, is_training=False)

    windows = loader.batch_size * loader.batches_per_epoch
    positives = int(round(p_cough * windows))
    config = dict(model_type=model_type, **pre_config, batch_size=batch_size, learning_rate=learning_rate,
                  weight_decay=weight_decay, epochs=epochs, patience=patience,
                  windows=dict(batches_per_epoch=loader.batches_per_epoch, holdout=holdout, random_state=random_state,
                               val_scenes=val_scenes, scene_seconds=scene_seconds, events_per_scene=list(events_per_scene),
                               snr_range=list(snr_range), p_cough=p_cough, p_distractor=p_distractor, p_augment=p_augment,
                               speed=bool(speed), draws=draws, plan_draws=plan_draws,
                               min_overlap_seconds=min_overlap_seconds, sweep=sweep, seed=seed))
    model = create_model(model_type, n_mels=preprocessor.get_num_features(), num_classes=2, in_channels=1)
    trainer = _TRAINERS[model_type](model, lr=learning_rate, weight_decay=weight_decay,
                                    class_weights=class_weights_from_counts({0: windows - positives, 1: positives}), seed=seed)
    result = fit(trainer, loader, val_loader, str(output_dir), epochs=epochs, patience=patience, config=config, resume=resume)
    with open(Path(output_dir) / "history.json", "w") as f:
        json.dump(result["history"], f, indent=2)
    result["pick"] = None
    if Path(result["best_model"]).exists():
        engine = CoughDetectorInference(result["best_model"], verbose=False)
        scores = score_bank(scenes, engine._pipeline)
        swept = match_events(scores, truth, np.linspace(0.0, 1.0, int(sweep)))
        report = event_report(scenes, scores, swept, truth)
        report["pick"] = result["pick"] = pick_threshold(report)
        with open(Path(output_dir) / "events.json", "w") as f:
            json.dump(report, f, indent=2)
    return result


def build_parser():
    import argparse
    from .train import MODEL_TYPES
    parser = argparse.ArgumentParser(prog="python -m cough_detector_amd.windows",
                                     description="Train on composed windows and score the checkpoint by event (MI355X path)")
    parser.add_argument("background_dir", help="directory of background WAVE files (speech, room noise, silence)")
    parser.add_argument("event_dir", help="directory with cough/ and, optionally, non_cough/ (distractors)")
    parser.add_argument("--output-dir", type=str, default="./checkpoints", help="Directory to save checkpoints")
    parser.add_argument("--model-type", type=str, default="small", choices=list(MODEL_TYPES), help="Model architecture")
    parser.add_argument("--epochs", type=int, default=100, help="Maximum training epochs")
    parser.add_argument("--batch-size", type=int, default=32, help="Batch size")
    parser.add_argument("--lr", type=float, default=0.001, help="Learning rate")
    parser.add_argument("--weight-decay", type=float, default=0.01, help="Weight decay")
    parser.add_argument("--patience", type=int, default=15, help="Early stopping patience")
    parser.add_argument("--resume", type=str, default=None, help="Resume from checkpoint")
    parser.add_argument("--batches-per-epoch", type=int, default=None, help="Composed batches in an epoch")
    parser.add_argument("--val-scenes", type=int, default=32, help="Held-out scenes composed for validation and scoring")
    parser.add_argument("--seconds", type=float, default=30.0, help="length of a held-out scene")
    parser.add_argument("--events", type=str, default="3,6", help="lo,hi coughs per held-out scene")
    parser.add_argument("--snr", type=str, default="5,20", help="lo,hi dB")
    parser.add_argument("--p-cough", type=float, default=0.5, help="Share of composed windows that hold a cough")
    parser.add_argument("--p-augment", type=float, default=0.3, help="Probability of each augmentation step")
    parser.add_argument("--speed", action="store_true", help="Speed perturbation behind the composer")
    parser.add_argument("--draws", type=str, default="device", choices=["host", "device"],
                        help="Where the chain behind the composer makes its draws")
    parser.add_argument("--plan-draws", type=str, default="device", choices=["host", "device"],
                        help="Where the window plans are drawn")
    parser.add_argument("--seed", type=int, default=0, help="Seed of plans, initialisation, draws and dropout")
    return parser


def main(argv: Optional[Sequence[str]] = None) -> dict:
    import json
    parser = build_parser()
    args = parser.parse_args(argv)
    try:
        events = tuple(int(v) for v in args.events.split(","))
        snr = tuple(float(v) for v in args.snr.split(","))
    except ValueError:
        parser.error("--events takes lo,hi integers and --snr lo,hi numbers")
    result = _train_windows(args.background_dir, args.event_dir, args.output_dir, args.model_type, args.epochs, args.batch_size,
                            args.lr, args.weight_decay, args.patience, args.resume, batches_per_epoch=args.batches_per_epoch,
                            holdout=0.2, random_state=42, val_scenes=args.val_scenes, scene_seconds=args.seconds,
                            events_per_scene=events, snr_range=snr, p_cough=args.p_cough, p_distractor=None,
                            p_augment=args.p_augment, speed=args.speed, draws=args.draws, plan_draws=args.plan_draws,
                            min_overlap_seconds=0.1, sweep=101, seed=args.seed)
    report = {"best_model": result["best_model"], "best_f1": result["best_f1"], "epochs_run": result["epochs_run"],
              "pick": result["pick"]}
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
