"""The waveform chain in front of the augmentation kernel, in one place: ``time shift -> speed (cough_warp_rows) -> pitch
(cough_stretch_rows + cough_warp_rows) -> reverb (cough_reverb_rows)``; gain, gaussian noise and the noise bank follow in
``cough_augment_waveforms`` or ``cough_augment_rows_drawn`` (noise in a room is not convolved with the talker's response).  ``AudioAugmentor`` and both modes of ``DeviceDataLoader`` run it through here.

* ``host_plans``: the host's draws of a batch as the numpy plans of the launches, with the chain's rules: which launch
  carries the time shift, how wide the output is, what rows without a draw get.
* ``run``: the optional speed launch, the optional pitch launches and the optional reverb launch on packed device rows.
  It does not care whether its plans were uploaded (``host_plans``) or drawn on the device (``cough_draw_speed`` /
  ``cough_draw_pitch`` / ``cough_draw_reverb``).
* ``unshifted``: the records for the augmentation kernel once a launch of ``run`` has shifted the rows.

A new step of the chain adds its plan to ``HostPlans`` and ``host_plans``, its launch to ``run``, and its draw to the
three places that draw (``AudioAugmentor.draw_item_pitched``, ``DeviceDataLoader._draw_items`` for the ``BatchPlan``,
``launch_batch_drawn`` for the device's draws); the callers' own control flow does not change.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import pitch as _pitch
from . import reverb as _reverb
from . import warp as _warp


class HostPlans(NamedTuple):
    """``arrays``: what the launches read on the device, by name, in the order of the launches -- ``warp`` ((B, 3) int32
    ``cough_warp_plan``s) and ``new_lengths`` (int32 (B,)) when a pair fired, ``stretch`` ((B, 16) uint8
    ``cough_stretch_plan``s) and ``back`` ((B, 3) int32 plans of the resampling behind them) when a row has semitones;
    ``reverb`` ((B, 4) int32 ``cough_reverb_plan``s) when a row has a response;
    empty when nothing fired: no plan carries the time shift then, and the records keep it.  ``new_lengths``: the rows'
    lengths after the chain.  ``width`` / ``stretch_width``: the widths of the output and of the stretched rows."""
    arrays: Dict[str, np.ndarray]
    new_lengths: List[int]
    width: int
    stretch_width: int


def host_plans(shifts: Sequence[int], pairs: Optional[Sequence[Optional[Tuple[int, int]]]],
               steps: Optional[Sequence[Optional[int]]], lengths: Sequence[int], sample_rate: int, n: int,
               phase_lock: bool = False, reverb: Optional[Sequence[Optional[int]]] = None) -> HostPlans:
    """The plans of a batch drawn on the host.  Per row: its time shift, the speed step's ``(orig, new)`` (None when its
    coin did not fire), the pitch step's semitones (None likewise; 0 shifts nothing) and its length; ``pairs`` /
    ``steps`` are None as a whole when the step is switched off.  ``n`` is the width of the input rows.  ``reverb``: per
    row the reverb step's response (None when its coin did not fire), None as a whole when the step is switched off.

    The first launch that reads the source rows carries the shift: the warp if any pair fired, else the stretch if any
    row has semitones, else the reverb if any row has a response, else the augmentation record.  A row without a pair is
    copied by the warp (``(1, 1)``), a row without semitones by the stretch and its resampling (rate 1, ``(1, 1)``), a row
    without a response by the reverb (``rir = -1``); the reverb keeps a row's length (``out_len = n'``).  The output is ``max n'`` wide with a
    speed step and ``n`` wide without.  With ``phase_lock`` the stretch plans of the rows with semitones other than 0
    carry the mode ``pitch.PHASE_LOCK`` and all other rows mode 0 -- the rule of ``cough_draw_pitch``, so the host's and
    the device's plans of the same draws are the same bytes."""
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
    return HostPlans(arrays, new_lengths, width, stretch_width)


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
