"""The waveform chain, in one place: ``time shift -> speed (cough_warp_rows) -> pitch (cough_stretch_rows +
cough_warp_rows) -> reverb (cough_reverb_rows)`` in front of the augmentation kernel; gain, gaussian noise and the noise
bank in it (``cough_augment_waveforms`` or ``cough_augment_rows_drawn``: room noise is not convolved with the talker's
response); the capture channel (``cough_channel_rows``) behind it, in place on its matrix: a microphone hears the room
and the noise.  ``AudioAugmentor`` and both modes of ``DeviceDataLoader`` run it through here.

* ``ItemDraw``: one item's host draws, all steps; ``columns`` turns a batch of them into ``BatchPlan``'s columns.
* ``host_plans``: the host's draws of a batch as the numpy plans of the launches, with the chain's rules: which launch
  carries the time shift, how wide the output is, what rows without a draw get.  ``launches``: those plans, once on
  the device, as what ``run`` and ``finish`` take.
* ``run``: the optional speed, pitch and reverb launches on packed device rows, whether their plans were uploaded or
  drawn on the device; ``unshifted``: the kernel's records behind them; ``finish``: the channel launch behind the kernel.
* ``run_drawn``: a ``draws="device"`` batch from its draws to the channel launch, with the hand-over of the time shift.

A new step is added in three places: here (``ItemDraw`` and ``columns``, ``host_plans`` and ``launches``, ``run`` or
``finish``, ``run_drawn``), in the augmentor's one draw method (``AudioAugmentor.draw_item_channel``) and as a column of
``BatchPlan``; the callers' control flow does not change.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import channel as _channel
from . import draws as _draws
from . import pitch as _pitch
from . import reverb as _reverb
from . import warp as _warp


class ItemDraw(NamedTuple):
    """One item's host draws: the kernel's record, the speed step's rate pair and the length behind it, the pitch step's
    semitones, the reverb step's response, the channel step's ``(filter, clip_ratio)``; None: off, or no coin fired."""
    record: _lib.CoughAugClip
    pair: Optional[Tuple[int, int]]
    length: int
    steps: Optional[int]
    rir: Optional[int]
    channel: Optional[Tuple[int, float]]


def columns(items: Sequence[ItemDraw], aug) -> Dict[str, Optional[list]]:
    """``BatchPlan``'s columns of a batch's items, by name; the column of a step that ``aug`` has switched off is None."""
    records, pairs, lengths, steps, rirs, channels = [list(c) for c in zip(*items)] or [[] for _ in ItemDraw._fields]
    return dict(clips=records, pairs=pairs if aug.speed else None, new_lengths=lengths if aug.speed else None,
                steps=steps if aug.pitch else None, rirs=rirs if aug.reverb is not None else None,
                channels=channels if aug.channel is not None else None)


class HostPlans(NamedTuple):
    """``arrays``: what the launches read on the device, by name, in the order of the launches -- ``warp`` ((B, 3) int32
    ``cough_warp_plan``s) and ``new_lengths`` (int32 (B,)) when a pair fired, ``stretch`` ((B, 16) uint8
    ``cough_stretch_plan``s) and ``back`` ((B, 3) int32 plans of the resampling behind them) when a row has semitones;
    ``reverb`` ((B, 4) int32 ``cough_reverb_plan``s) when a row has a response; ``channel`` ((B, 2) int32
    ``cough_channel_plan``s) when a row has a microphone; empty when nothing fired: no plan carries the time shift then,
    and the records keep it.  ``new_lengths``: the rows' lengths after the chain.  ``width`` / ``stretch_width``: the
    widths of the output and of the stretched rows."""
    arrays: Dict[str, np.ndarray]
    new_lengths: List[int]
    width: int
    stretch_width: int


def channel_plans(plans: Sequence[Optional[Tuple[int, float]]], n_bank: Optional[int] = None) -> np.ndarray:
    """The channel step's plans as int32 (B, 2) words (the ratio's bits in the second): a row without a plan is copied
    (``(-1, 1.0)``); with ``n_bank`` a filter the bank does not have raises ValueError."""
    return _channel.plan_array([p if p is not None else (-1, 1.0) for p in plans], n_bank).view(np.int32).reshape(-1, 2)


def host_plans(shifts: Sequence[int], pairs: Optional[Sequence[Optional[Tuple[int, int]]]],
               steps: Optional[Sequence[Optional[int]]], lengths: Sequence[int], sample_rate: int, n: int,
               phase_lock: bool = False, reverb: Optional[Sequence[Optional[int]]] = None,
               channel: Optional[Sequence[Optional[Tuple[int, float]]]] = None, n_channels: Optional[int] = None) -> HostPlans:
    """The plans of a batch drawn on the host.  Per row: its time shift, the speed step's ``(orig, new)`` (None when its
    coin did not fire), the pitch step's semitones (None likewise; 0 shifts nothing) and its length; ``pairs`` /
    ``steps`` are None as a whole when the step is switched off.  ``n`` is the width of the input rows.  ``reverb``: per
    row the reverb step's response (None when its coin did not fire), None as a whole when the step is switched off.
    ``channel``: likewise the channel step's ``(filter, clip_ratio)``, checked against a bank of ``n_channels`` entries.

    The first launch that reads the source rows carries the shift: the warp if any pair fired, else the stretch if any
    row has semitones, else the reverb if any row has a response, else the augmentation record.  A row without a pair is
    copied by the warp (``(1, 1)``), a row without semitones by the stretch and its resampling (rate 1, ``(1, 1)``), a row
    without a response by the reverb (``rir = -1``); the reverb keeps a row's length (``out_len = n'``).  The output is ``max n'`` wide with a
    speed step and ``n`` wide without.  With ``phase_lock`` the stretch plans of the rows with semitones other than 0
    carry the mode ``pitch.PHASE_LOCK`` and all other rows mode 0 -- the rule of ``cough_draw_pitch``, so the host's and
    the device's plans of the same draws are the same bytes.  The channel's plans come last and carry no shift."""
    lengths = [int(v) for v in lengths]
    warps = pairs is not None and any(p is not None for p in pairs)
    new_lengths = [l if p is None else _warp.warped_length(l, *p) for l, p in zip(lengths, pairs)] if warps else lengths
    width = max(new_lengths, default=0) if pairs is not None else n
    arrays, stretch_width = {}, 0
    if warps:
        arrays["warp"] = _warp.plan_array([(s,) + (p if p is not None else (1, 1)) for s, p in zip(shifts, pairs)])
        arrays["new_lengths"] = np.asarray(new_lengths, dtype=np.int32)
    if steps is not None and any(steps):
        rates = [_pitch.pitch_rate(s) if s else 1.0 for s in steps]
        modes = [_pitch.PHASE_LOCK if phase_lock and s else 0 for s in steps]
        arrays["stretch"] = _pitch.plan_array([(0 if warps else shift, r, m) for shift, r, m in zip(shifts, rates, modes)])
        arrays["back"] = _warp.plan_array([(0,) + (_pitch.pitch_rate_pair(s, sample_rate) if s else (1, 1)) for s in steps])
        stretch_width = max(_pitch.stretched_length(l, r) for l, r in zip(new_lengths, rates))
    if reverb is not None and any(r is not None for r in reverb):
        arrays["reverb"] = _reverb.plan_array([(shift if not arrays else 0, -1 if r is None else r, l)
                                               for shift, r, l in zip(shifts, reverb, new_lengths)])
    if channel is not None and any(c is not None for c in channel):
        arrays["channel"] = channel_plans(channel, n_channels)
    return HostPlans(arrays, new_lengths, width, stretch_width)


Launches = NamedTuple("Launches", [("speed", Optional[tuple]), ("pitch", Optional[tuple]), ("reverb", Optional[tuple]),
                                   ("channel", Optional[torch.Tensor]), ("front", int), ("chained", bool)])


def launches(plans: Optional[HostPlans], tensor: Callable[[str], torch.Tensor], aug, keep: bool = False) -> Launches:
    """The launches of ``plans`` (None: nothing fired): ``run``'s ``speed`` / ``pitch`` / ``reverb`` and ``finish``'s
    ``channel`` plans (None: no such launch), how many launches run in ``front`` of the kernel (0: the records keep their
    shifts) and whether ``run`` needs ``out_offsets`` (``chained``).  ``tensor(name)`` is ``plans.arrays[name]`` on the
    device, an upload of it or a view into one, asked only for what a launch reads; ``aug`` has the reverb bank.  A step's
    new lengths and output offsets are needed when a later step, or (``keep``) the caller, reads its (B, width) output."""
    a = plans.arrays if plans is not None else {}
    front = sum(name in a for name in ("warp", "stretch", "reverb"))
    chained = front > (0 if keep else 1)
    speed = (tensor("warp"), tensor("new_lengths") if chained else None, plans.width) if "warp" in a else None
    pitch = (tensor("stretch"), tensor("back"), plans.stretch_width, plans.width) if "stretch" in a else None
    reverb = (tensor("reverb"), aug.reverb, plans.width) if "reverb" in a else None
    return Launches(speed, pitch, reverb, tensor("channel") if "channel" in a else None, front, chained)


def unshifted(clips: Sequence[_lib.CoughAugClip]) -> List[_lib.CoughAugClip]:
    """Copies of the records with the shift zeroed: the chain's first launch has shifted the rows."""
    out = [_lib.CoughAugClip.from_buffer_copy(c) for c in clips]
    for c in out:
        c.shift = 0
    return out


def dense_offsets(b: int, width: int, dev: torch.device) -> torch.Tensor:
    """The int64 row offsets of a (b, width) matrix, on ``dev``."""
    return (torch.arange(b, dtype=torch.int64) * int(width)).to(dev)


def run(src: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor,
        speed: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
        pitch: Optional[Tuple[torch.Tensor, torch.Tensor, int, int]] = None,
        out_offsets: Optional[torch.Tensor] = None,
        reverb: Optional[Tuple[torch.Tensor, "_reverb.RirBank", int]] = None
        ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    """The speed, pitch and reverb steps on B rows of the flat float32 buffer ``src``: row b is the ``lengths[b]`` (int32) samples
    at ``offsets[b]`` (int64), all on the device.  ``speed``: ``(plans (B, 3) int32, new lengths int32 (B,), width)``;
    ``pitch``: ``(stretch plans (B, 16) uint8, resampling plans (B, 3) int32, stretch width, width)``; ``reverb``:
    ``(plans (B, 4) int32, the RirBank, width)``; the plans live on the device.  A step that runs leaves a dense (B, width) matrix whose row offsets are ``out_offsets``: a later
    step needs them to read an earlier step's output, and a caller that runs at most one step may leave them out.  Returns
    ``(rows, offsets, lengths)`` of the result -- the arguments themselves when neither step runs; the offsets of a
    matrix are None when ``out_offsets`` was left out (hence ``Optional`` in the return type)."""
    if speed is not None:                                        # shift and speed, read in place
        plans, new_lengths, width = speed
        src, offsets, lengths = _warp.warp_rows(src, offsets, lengths, plans, width), out_offsets, new_lengths
    if pitch is not None:                                        # the shift rides in the stretch's read if not in the warp's
        stretch, back, stretch_width, width = pitch
        src, offsets = _pitch.pitch_shift_rows(src.reshape(-1), offsets, lengths, stretch, back, width, stretch_width), out_offsets
    if reverb is not None:                                       # the shift rides here only when no launch ran before it
        plans, bank, width = reverb
        src, offsets = _reverb.reverb_rows(src.reshape(-1), offsets, lengths, plans, width, bank), out_offsets
    return src, offsets, lengths


def finish(matrix: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, plans: torch.Tensor,
           bank: "_channel.ChannelBank", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The channel step: one ``cough_channel_rows`` launch on the dense (B, width) ``matrix`` the kernel wrote (its row
    ``offsets``, the rows' ``lengths``, ``plans`` int32 (B, 2): on the device) into ``out``, which may be the matrix itself."""
    return _channel.channel_rows(matrix.view(-1), offsets, lengths, plans, matrix.shape[1], bank, out=out)


def drawn_width(row_len: int, aug) -> int:
    """How wide a batch's rows can get when its longest has ``row_len`` samples: ``warp.drawn_width`` with a speed step."""
    return _warp.drawn_width(row_len, aug.speed_range, aug.sample_rate) if aug is not None and aug.speed else row_len


def run_drawn(seed: int, src: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, out_offsets: torch.Tensor,
              width: int, aug, spec, feature_shape: Tuple[int, int]):
    """A ``draws="device"`` batch under ``seed``, from its draws to the channel step: ``(rows, masks)``.  Its B rows lie
    in the flat buffer ``src`` (``offsets`` int64, ``lengths`` int32, on the device); ``out_offsets``: the row offsets of
    a (B, width) matrix, ``width`` being ``drawn_width`` of the longest row; ``aug`` / ``spec``: the augmentors, or None.
    ``rows``: ``(src, offsets, lengths)`` of the result, the arguments themselves without ``aug``; ``masks``: ``draws.draw_batch``'s.

    The draws come first, each step's for the lengths the step before it leaves: speed, pitch, reverb, then
    ``cough_draw_batch``, whose records hold the shift.  The first launch that reads ``src`` carries it: the warp's plans are
    drawn with it; without a speed step its word is copied from the records into the stretch's plans, or else the
    reverb's; ``cough_clear_shifts`` then takes it from the records.  The channel's plans are drawn behind the kernel."""
    b, speed, pitch, reverb, lens = lengths.numel(), None, None, None, lengths
    if aug is not None and aug.speed:
        speed = _warp.draw_speed(seed, lens, aug.p_augment, aug.speed_range, aug.sample_rate) + (width,)
        lens = speed[1]
    if aug is not None and aug.pitch:
        pitch = _pitch.draw_pitch(seed, lens, aug.p_augment, aug.pitch_range, aug.sample_rate,
                                  aug.pitch_table(lens.device))[:2] + (_pitch.drawn_width(width, aug.pitch_range), width)
    if aug is not None and aug.reverb is not None:               # out_len is the row's current length: the step keeps it
        reverb = (_reverb.draw_reverb(seed, lens, aug.p_augment, aug.reverb), aug.reverb, width)
    clips, masks = _draws.draw_batch(seed, lens, aug, spec, feature_shape)
    rows = (src, offsets, lengths)
    if clips is not None:
        rows = run(*rows, speed=speed, out_offsets=out_offsets)
        steps = [s for s in (speed, pitch, reverb) if s is not None]
        if steps and speed is None:                              # the first 4-byte word of every plan and record is its shift
            steps[0][0].view(torch.int32).view(b, -1)[:, 0] = clips.view(torch.int32).view(b, _draws.CLIP_BYTES // 4)[:, 0]
        if steps:
            _warp.clear_shifts(clips)
        rows = run(*rows, pitch=pitch, reverb=reverb, out_offsets=out_offsets)      # in a call of its own: behind cough_clear_shifts
        rows = (_draws.augment_rows_drawn(*rows, width, clips, aug, seed), out_offsets, rows[2])
        if aug.channel is not None:
            mics = _channel.draw_channel(seed, b, aug.p_augment, aug.channel, aug.p_clip, aug.clip_range, lens.device)
            finish(rows[0], out_offsets, rows[2], mics, aug.channel, out=rows[0])
    return rows, masks
